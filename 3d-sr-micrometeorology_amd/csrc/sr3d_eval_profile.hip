// Height-resolved evaluation: every metric of the fused evaluation pass PER LEVEL, from one streaming pass (gfx950).
//
// sr3d_eval.hip serves one `lev` per launch and only for two metrics; a 32-level profile is 32 passes there.  The
// marching stencil of that file reports the volume plane by plane, so the per-level sums are at hand where plane j is
// reported.  This file is the same march (x by wave shuffles, y through the double-buffered LDS tile, z in a rolling
// register window, central differences as hi * w + lo * (-w) with contraction off) with the accumulators kept per
// PLANE instead of per block:
//
//   eval_profile_kernel   a block owns an (MY x MX x MZS) column.  For each reported plane every thread has kP = 20
//                         terms (its one voxel of that plane); a row's wave reduces them with an exchange reduction
//                         (below: 22 shuffles for all 20 sums, not 20 x 6) and 20 lanes store the row's sums to LDS
//                         [row][plane][acc].  After the march the MY rows are added in fixed order and [plane][acc]
//                         goes to the workspace at [sample][z tile][xy tile][plane][acc].
//   eval_profile_final    one block per (level, sample-or-batch): the partials of all (x, y) tiles of that level,
//                         summed in a fixed order in double; writes the raw sums and the ratios.
//
// No floating-point atomics; every order of summation is fixed by the indices alone: two calls are bit-equal, and a
// per-sample result is bit-equal to a one-sample call.
#include "sr3d_common.h"

namespace {

constexpr int kP = SR3D_PROFILE_SUM_COUNT;   // sums per level
static_assert(kP == 20, "the exchange reduction below is laid out for 20 sums");

enum {
  P_ABS = SR3D_PROFILE_SUM_ABS, P_SQ = SR3D_PROFILE_SUM_SQ, P_SQ_T = SR3D_PROFILE_SUM_SQ_T,
  P_B = SR3D_PROFILE_SUM_MASK, P_B_ABS = SR3D_PROFILE_SUM_MASK_ABS, P_B_SQ = SR3D_PROFILE_SUM_MASK_SQ,
  P_NEAR = SR3D_PROFILE_SUM_NEAR, P_NEAR_ABS = SR3D_PROFILE_SUM_NEAR_ABS, P_NEAR_SQ = SR3D_PROFILE_SUM_NEAR_SQ,
  P_T = SR3D_PROFILE_SUM_MASK_DT, P_V = SR3D_PROFILE_SUM_MASK_DV,
  P_B_INT = SR3D_PROFILE_SUM_MASK_INT, P_NEAR_INT = SR3D_PROFILE_SUM_NEAR_INT,
  P_RES_P = SR3D_PROFILE_SUM_RES_P, P_RES_T = SR3D_PROFILE_SUM_RES_T, P_DDIV = SR3D_PROFILE_SUM_DDIV,
  P_OMEGA = SR3D_PROFILE_SUM_OMEGA
};

struct ProfParams {
  const float* p;
  const float* t;
  const float* b;
  int B, Z, Y, X;
  float s[4];
  float w;        // 1 / (2 delta)
  float* part;    // [B][z tiles][xy tiles][MZS][kP]
  float* sums;    // ([B],) kP, Z
  float* values;  // ([B],) SR3D_PROFILE_COUNT, Z
};

// central difference exactly as the reference's depthwise convolution evaluates it (see sr3d_eval.hip)
__device__ __forceinline__ float cdiff(float hi, float lo, float w) {
#pragma clang fp contract(off)
  const float a = hi * w, b = lo * -w;
  return a + b;
}

// ---- exchange reduction: N sums over the 64 lanes of a wave ---------------------------------------------------------
// One step pairs lane l with lane l ^ O: the lane whose bit O is clear keeps the lower half of the values, the other
// one the upper half, and each sends the half it drops.  N values -> ceil(N / 2) per step (20 -> 10 -> 5 -> 3 -> 2 ->
// 1), then the two lanes that hold the same value add up: 10 + 5 + 3 + 2 + 1 + 1 = 22 shuffles for all 20 sums.
template <int N, int O>
__device__ __forceinline__ void exchange_step(float* v, int lane) {
  constexpr int H = (N + 1) / 2;
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const float lo = v[i], hi = (i + H < N) ? v[i + H] : 0.f;
    const float keep = up ? hi : lo, send = up ? lo : hi;
    v[i] = keep + __shfl_xor(send, O, 64);
  }
}

// after wave_reduce20, v[0] of an even lane with reduce20_slot(lane) >= 0 is the wave's sum of that slot
__device__ __forceinline__ void wave_reduce20(float* v, int lane) {
  exchange_step<20, 32>(v, lane);
  exchange_step<10, 16>(v, lane);
  exchange_step<5, 8>(v, lane);
  exchange_step<3, 4>(v, lane);
  exchange_step<2, 2>(v, lane);
  v[0] += __shfl_xor(v[0], 1, 64);
}

__device__ __forceinline__ int reduce20_slot(int lane) {
  const int s3 = ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);    // of 3 (slot 3 is padding)
  const int s5 = ((lane >> 3) & 1) * 3 + s3;                   // of 5 (slot 5 is padding)
  if ((lane & 1) || s3 >= 3 || s5 >= 5) return -1;
  return ((lane >> 5) & 1) * 10 + ((lane >> 4) & 1) * 5 + s5;
}

// ---- the pass: the 2.5-D marching stencil of eval_kernel (same tile: 8 rows x 62 columns x 16 planes) ---------------
constexpr int MY = 8, MX = 62, MROWS = MY + 2, MZS = 16;
constexpr int MF = 7;                            // fields that need y neighbours: 3 velocities x (p, t) + mask x-sum
constexpr int kMarchThreads = MROWS * 64;
constexpr int kFinalThreads = 256, kFinalSlots = kFinalThreads / 32;

__global__ __launch_bounds__(kMarchThreads) void eval_profile_kernel(const ProfParams q) {
#pragma clang fp contract(off)
  __shared__ float tile[2][MF][MROWS][64];
  __shared__ float rowsum[MY][MZS][kP];
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;          // row 0 / MROWS-1: halo rows
  int blk = blockIdx.x;
  const int ntx = (q.X + MX - 1) / MX, nty = (q.Y + MY - 1) / MY;
  const int tix = blk % ntx;
  blk /= ntx;
  const int tiy = blk % nty;
  const int tiz = blk / nty;
  const int bi = blockIdx.y;
  const int x = tix * MX - 1 + lane, y = tiy * MY - 1 + row;
  const int z_lo = tiz * MZS, z_hi = min(z_lo + MZS, q.Z);             // output planes [z_lo, z_hi)
  const bool in_xy = (unsigned)x < (unsigned)q.X && (unsigned)y < (unsigned)q.Y;
  const bool owner = in_xy && lane >= 1 && lane <= MX && row >= 1 && row <= MY;    // this thread reports outputs
  const bool inner_xy = owner && x >= 1 && x < q.X - 1 && y >= 1 && y < q.Y - 1;
  const bool row_reports = row >= 1 && row <= MY;                      // wave-uniform
  const int slot = reduce20_slot(lane);
  const long long zyx = (long long)q.Z * q.Y * q.X, sz = (long long)q.Y * q.X;
  const long long col = (long long)y * q.X + x;
  const float* pb = q.p + (long long)bi * 4 * zyx + col;
  const float* tb = q.t + (long long)bi * 4 * zyx + col;
  const float* mb = q.b + (long long)bi * zyx + col;

  // rolling window (index 0 = plane j-1, 1 = plane j, 2 = plane j+1 when plane j is reported)
  float vel[3][2][3];      // scaled velocity [plane][p / t][u, v, w]
  float pc1[4], tc1[4];    // all four channels of plane j (non-stencil sums)
  float b1 = 0.f, sxy[3] = {0.f, 0.f, 0.f};
  float gx1[2][3], gy1[2][3];   // x / y derivatives of plane j, formed when plane j arrived
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) vel[a][k][c] = 0.f;
#pragma unroll
  for (int c = 0; c < 4; c++) pc1[c] = tc1[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) gx1[k][c] = gy1[k][c] = 0.f;

  for (int zz = z_lo - 1; zz <= z_hi; zz++) {          // plane zz arrives; plane j = zz - 1 is reported
    const bool in_z = (unsigned)zz < (unsigned)q.Z;
    const bool live = in_xy && in_z;
    float pn[4], tn[4], bn = 1.f;                       // outside the grid: zero field, "fluid" mask (1 - b = 0)
#pragma unroll
    for (int c = 0; c < 4; c++) pn[c] = tn[c] = 0.f;
    if (live) {
      const long long o = (long long)zz * sz;
#pragma unroll
      for (int c = 0; c < 4; c++) pn[c] = pb[c * zyx + o], tn[c] = tb[c * zyx + o];
      bn = mb[o];
    }
    float vn[2][3];
#pragma unroll
    for (int c = 0; c < 3; c++) vn[0][c] = q.s[c + 1] * pn[c + 1], vn[1][c] = q.s[c + 1] * tn[c + 1];
    // x neighbours: shuffles (lanes 0 / 63 get garbage from the wrap-around; they are halo lanes and never report)
    float gxn[2][3];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        gxn[k][c] = cdiff(__shfl_down(vn[k][c], 1, 64), __shfl_up(vn[k][c], 1, 64), q.w);
    const float ib = 1.f - bn;
    const float sx = (__shfl_up(ib, 1, 64) + ib) + __shfl_down(ib, 1, 64);
    // y neighbours through LDS
    float (*T)[MROWS][64] = tile[zz & 1];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) T[k * 3 + c][row][lane] = vn[k][c];
    T[6][row][lane] = sx;
    __syncthreads();
    float gyn[2][3], sxy_n = 0.f;
    if (row_reports) {
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) gyn[k][c] = cdiff(T[k * 3 + c][row + 1][lane], T[k * 3 + c][row - 1][lane], q.w);
      sxy_n = (T[6][row - 1][lane] + sx) + T[6][row + 1][lane];
    } else {
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) gyn[k][c] = 0.f;
    }
    sxy[2] = sxy_n;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) vel[2][k][c] = vn[k][c];

    // ---- report plane j = zz - 1 (its z+1 neighbour has just arrived): this thread's terms, then the row's sums
    const int j = zz - 1;
    if (row_reports && j >= z_lo && j < z_hi) {          // wave-uniform: the whole wave takes part in the reduction
      float v[kP];
#pragma unroll
      for (int i = 0; i < kP; i++) v[i] = 0.f;
      if (owner) {
        const float bv = b1;
        const float box = (sxy[0] + sxy[1]) + sxy[2];
        const float near = ((box > 0.f ? 1.f : 0.f) * bv > 0.f) ? 1.f : 0.f;
        float sa = 0.f, sq = 0.f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const float d = pc1[c] - tc1[c];
          const float d2 = d * d;
          sa += fabsf(d), sq += d2;
          v[P_SQ_T + c] = d2;
        }
        v[P_ABS] = sa, v[P_SQ] = sq;
        v[P_B] = bv, v[P_B_ABS] = bv * sa, v[P_B_SQ] = bv * sq;
        v[P_NEAR] = near, v[P_NEAR_ABS] = near * sa, v[P_NEAR_SQ] = near * sq;
        // |T_p - T_t| * std_T and || std_v * v_p - std_v * v_t ||
        const float dT = fabsf(pc1[0] - tc1[0]) * q.s[0];
        float n2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float dv = vel[1][0][c] - vel[1][1][c];
          n2 += dv * dv;
        }
        const float dV = sqrtf(n2);
        v[P_T] = bv * dT, v[P_V] = bv * dV;
        if (inner_xy && j >= 1 && j < q.Z - 1) {
          v[P_B_INT] = bv, v[P_NEAR_INT] = near;
          const float M = bv * (1.f - near);
          float res[2], om[2][3];
#pragma unroll
          for (int k = 0; k < 2; k++) {
            float gz[3];
#pragma unroll
            for (int c = 0; c < 3; c++) gz[c] = cdiff(vel[2][k][c], vel[0][k][c], q.w);
            res[k] = (gx1[k][0] + gy1[k][1]) + gz[2];
            om[k][0] = gy1[k][2] - gz[1];       // dw/dy - dv/dz
            om[k][1] = gz[0] - gx1[k][2];       // du/dz - dw/dx
            om[k][2] = gx1[k][1] - gy1[k][0];   // dv/dx - du/dy
          }
          const float rp = res[0] * M, rt = res[1] * M;
          v[P_RES_P] = fabsf(rp), v[P_RES_T] = fabsf(rt), v[P_DDIV] = fabsf(rp - rt);
          float o2 = 0.f;
#pragma unroll
          for (int a = 0; a < 3; a++) {
            const float dd = om[0][a] * M - om[1][a] * M;
            o2 += dd * dd;
          }
          v[P_OMEGA] = sqrtf(o2);
        }
      }
      wave_reduce20(v, lane);
      if (slot >= 0) rowsum[row - 1][j - z_lo][slot] = v[0];
    }
    // ---- roll the window: plane zz becomes "plane j" of the next iteration
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        vel[0][k][c] = vel[1][k][c], vel[1][k][c] = vel[2][k][c];
        gx1[k][c] = gxn[k][c], gy1[k][c] = gyn[k][c];
      }
#pragma unroll
    for (int c = 0; c < 4; c++) pc1[c] = pn[c], tc1[c] = tn[c];
    b1 = bn;
    sxy[0] = sxy[1], sxy[1] = sxy[2];
  }

  __syncthreads();
  // the rows in fixed order; planes past the grid's top were never reported and are never read
  const int nrep = (z_hi - z_lo) * kP;
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

int xy_tiles(int Y, int X) { return ((X + MX - 1) / MX) * ((Y + MY - 1) / MY); }
int z_tiles(int Z) { return (Z + MZS - 1) / MZS; }

}  // namespace

extern "C" {

size_t sr3d_eval_level_profiles_workspace_bytes(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)B * z_tiles(Z) * xy_tiles(Y, X) * MZS * kP * sizeof(float);
}

int sr3d_eval_level_profiles(const void* p, const void* t, const void* b, int B, int Z, int Y, int X,
                             const float stds[4], float delta_meter, int per_sample, void* sums_out, void* values_out,
                             void* workspace, void* stream) {
  SR3D_CHECK(p && t && b && stds && sums_out && values_out && workspace, SR3D_E_ARG,
             "eval_level_profiles: null pointer");
  SR3D_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "eval_level_profiles: non-positive dimension");
  SR3D_CHECK((long long)Z * Y * X < (1ll << 31), SR3D_E_ARG, "eval_level_profiles: grid has >= 2^31 voxels");
  SR3D_CHECK(delta_meter > 0.f, SR3D_E_ARG, "eval_level_profiles: delta_meter must be positive");
  SR3D_CHECK(B <= 65535, SR3D_E_ARG, "eval_level_profiles: batch too large");
  ProfParams q{};
  q.p = (const float*)p, q.t = (const float*)t, q.b = (const float*)b;
  q.B = B, q.Z = Z, q.Y = Y, q.X = X;
  for (int i = 0; i < 4; i++) q.s[i] = stds[i];
  q.w = (float)(1.0 / (2.0 * (double)delta_meter));   // the kernel weight is a python float, then an fp32 tensor
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
