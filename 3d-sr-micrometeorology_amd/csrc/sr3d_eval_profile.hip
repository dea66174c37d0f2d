// Height-resolved evaluation: every metric of the fused evaluation pass PER LEVEL, from one streaming pass (gfx950).
//
// The marching stencil of sr3d_eval_march.h reports the volume plane by plane, so the per-level sums are at hand where
// plane j is reported: here the terms are summed per PLANE instead of per block.
//
//   eval_profile_kernel   a block owns an (MY x MX x MZS) column.  For each reported plane every thread has kP = 20
//                         terms (its one voxel of that plane); a row's wave reduces them with an exchange reduction
//                         (sr3d_wave_reduce.h: 22 shuffles for all 20 sums, not 20 x 6) and 20 lanes store the row's sums to LDS
//                         [row][plane][acc].  After the march the MY rows are added in fixed order and [plane][acc]
//                         goes to the workspace at [sample][z tile][xy tile][plane][acc].
//   eval_profile_final    one block per (level, sample-or-batch): the partials of all (x, y) tiles of that level,
//                         summed in a fixed order in double; writes the raw sums and the ratios.
//
// No floating-point atomics; every order of summation is fixed by the indices alone: two calls are bit-equal, and a
// per-sample result is bit-equal to a one-sample call.
#include "sr3d_eval_march.h"
#include "sr3d_wave_reduce.h"

namespace {

static_assert(kP == 20, "the exchange reduction is laid out for 20 sums");

struct ProfParams : MarchInputs {
  float* part;    // [B][z tiles][xy tiles][MZS][kP]
  float* sums;    // ([B],) kP, Z
  float* values;  // ([B],) SR3D_PROFILE_COUNT, Z
};

constexpr int kFinalThreads = 256, kFinalSlots = kFinalThreads / 32;

// the march's sink: a row's wave reduces the 20 terms of a plane and 20 of its lanes store the sums
struct RowSums {
  float (*rowsum)[MZS][kP];
  int lane, row, slot;
  __device__ __forceinline__ void voxel(int, const float (&)[kP]) {}
  __device__ __forceinline__ void interior(const float (&)[kP]) {}
  __device__ __forceinline__ void plane(int j, float (&v)[kP]) {     // a lane without a voxel brings zeros
    wave_reduce20(v, lane);
    if (slot >= 0) rowsum[row - 1][j % MZS][slot] = v[0];
  }
};

__global__ __launch_bounds__(kMarchThreads) void eval_profile_kernel(const ProfParams q) {
#pragma clang fp contract(off)
  __shared__ float tile[2][MF][MROWS][64];
  __shared__ float rowsum[MY][MZS][kP];
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  RowSums sums{rowsum, lane, row, reduce20_slot(lane)};
  const int nz = eval_march(q, tile, sums);

  __syncthreads();
  // the rows in fixed order; planes past the grid's top were never reported and are never read
  const int nrep = nz * kP;
  if ((int)threadIdx.x < nrep) {
    const float* r = &rowsum[0][0][0];
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < MY; w++) s += r[w * MZS * kP + threadIdx.x];
    q.part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * (MZS * kP) + threadIdx.x] = s;
  }
}
static_assert(MZS * kP <= kMarchThreads, "one thread per (plane, sum) of a block");

// one block per (level, sample or batch)
__global__ __launch_bounds__(kFinalThreads) void eval_profile_final_kernel(const ProfParams q, int nxy, int per_sample) {
  __shared__ double red[kFinalSlots][32];
  __shared__ double S[kP];
  const int k = blockIdx.x, g = blockIdx.y;
  const int tiz = k / MZS, pl = k % MZS;
  const int ntz = (q.Z + MZS - 1) / MZS;
  const int nb = per_sample ? 1 : q.B, b0 = per_sample ? g : 0;
  const int n = nb * nxy;
  const int a = threadIdx.x & 31, s = threadIdx.x >> 5;
  double v = 0.0;
  if (a < kP)
    for (int i = s; i < n; i += kFinalSlots) {
      const int bi = b0 + i / nxy, txy = i % nxy;
      v += (double)q.part[((((long long)bi * ntz + tiz) * nxy + txy) * MZS + pl) * kP + a];
    }
  red[s][a] = v;
  __syncthreads();
  if (threadIdx.x < kP) {
    double t = 0.0;
    for (int w = 0; w < kFinalSlots; w++) t += red[w][threadIdx.x];
    S[threadIdx.x] = t;
    q.sums[((long long)g * kP + threadIdx.x) * q.Z + k] = (float)t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float eps = 1e-30f;   // the modules' default
  auto F = [&](int i) { return (float)S[i]; };
  float* o = q.values + (long long)g * SR3D_PROFILE_COUNT * q.Z + k;
  auto put = [&](int i, float val) { o[(long long)i * q.Z] = val; };
  const float n_lev = (float)((double)nb * q.Y * q.X), n_all = (float)(4.0 * (double)nb * q.Y * q.X);
  put(SR3D_PROFILE_L1, F(P_ABS) / n_all);
  put(SR3D_PROFILE_L2, F(P_SQ) / n_all);
  // masks are broadcast over the 4 channels before torch.sum: the denominator is 4 * sum(mask)
  put(SR3D_PROFILE_MASKED_L1, F(P_B_ABS) / (4.f * F(P_B) + eps));
  put(SR3D_PROFILE_MASKED_L2, F(P_B_SQ) / (4.f * F(P_B) + eps));
  put(SR3D_PROFILE_MASKED_L1_NEAR_WALL, F(P_NEAR_ABS) / (4.f * F(P_NEAR) + eps));
  put(SR3D_PROFILE_MASKED_L2_NEAR_WALL, F(P_NEAR_SQ) / (4.f * F(P_NEAR) + eps));
  const float n_grid = F(P_B_INT) - F(P_NEAR_INT);   // no eps: 0 / 0 = nan, as in the whole-volume metric
  put(SR3D_PROFILE_RESIDUAL_CONTINUITY, F(P_RES_P) / n_grid);
  put(SR3D_PROFILE_RESIDUAL_CONTINUITY_TARGET, F(P_RES_T) / n_grid);
  put(SR3D_PROFILE_ABS_DIFF_TEMPERATURE, F(P_T) / (F(P_B) + eps));
  put(SR3D_PROFILE_DIFF_VELOCITY_NORM, F(P_V) / (F(P_B) + eps));
  put(SR3D_PROFILE_ABS_DIFF_DIVERGENCE, F(P_DDIV) / n_grid);
  put(SR3D_PROFILE_DIFF_OMEGA_NORM, F(P_OMEGA) / n_grid);
  for (int c = 0; c < 4; c++) put(SR3D_PROFILE_CHANNELWISE_MSE_T + c, F(P_SQ_T + c) / n_lev);
}

}  // namespace

extern "C" {

size_t sr3d_eval_level_profiles_workspace_bytes(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)B * z_tiles(Z) * xy_tiles(Y, X) * MZS * kP * sizeof(float);
}

int sr3d_eval_level_profiles(const void* p, const void* t, const void* b, int B, int Z, int Y, int X,
                             const float stds[4], float delta_meter, int per_sample, void* sums_out, void* values_out,
                             void* workspace, void* stream) {
  SR3D_CHECK(sums_out && values_out && workspace, SR3D_E_ARG, "eval_level_profiles: null pointer");
  ProfParams q{};
  if (int rc = march_inputs(q, "eval_level_profiles", p, t, b, B, Z, Y, X, stds, delta_meter)) return rc;
  q.part = (float*)workspace, q.sums = (float*)sums_out, q.values = (float*)values_out;
  const int nxy = xy_tiles(Y, X), nbs = nxy * z_tiles(Z);
  SrProfScope prof(SR3D_PROF_EVAL, 36.0 * (double)B * Z * Y * X, (hipStream_t)stream);   // p, t (32 B) + b (4 B) per voxel
  hipLaunchKernelGGL(eval_profile_kernel, dim3(nbs, B), dim3(kMarchThreads), 0, (hipStream_t)stream, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(eval_profile_final_kernel, dim3(Z, per_sample ? B : 1), dim3(kFinalThreads), 0,
                     (hipStream_t)stream, q, nxy, per_sample ? 1 : 0);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
