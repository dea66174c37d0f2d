// Wall-distance-resolved evaluation (gfx950): the Chebyshev distance to the nearest built cell as a byte volume, and
// every metric of the fused evaluation pass PER DISTANCE CLASS from one pass of the marching stencil.
//
// The reference's calc_mask_near_build_wall(b, n) applies a 27-tap box filter n times to 1 - b and tests > 0: a
// Chebyshev dilation by n cells, so near_n = (dist <= n) & (b > 0) for all n from ONE distance transform.  The
// transform separates exactly: min over (dz, dy, dx) of max(|dz|, |dy|, |dx|) is the distance along the row, then
// min over dy of max(|dy|, g1), then the same along z; values are capped at cap + 1, which commutes with min and max.
//
//   walldist_x_kernel     a wave owns a row and sweeps it in 64-cell chunks, left to right and back: one ballot gives a
//                         chunk's built cells, clz / ffs the nearest one within the chunk, a carried position the nearest
//                         one beyond it.  fp32 mask in, capped bytes out: the same work for any cap.
//   walldist_axis_kernel  one thread per voxel along y (then z) on bytes: best = min over k of max(k, g(+-k)), scanned
//                         outwards while k < best, so a voxel reads only as far as its own result (at most cap + 1).
//   walldist_profile_kernel   a third caller of eval_march: a row's wave bins its voxels by their distance byte (the
//                         column's bytes are fetched into LDS before the march: 8 KB), loops over the distinct bins it
//                         holds (ballot + first-lane readout; neighbours differ by at most 1),
//                         reduces the selected lanes' 20 terms with the exchange reduction and one fixed lane per slot
//                         adds into LDS [row][bin][sum]; popcount gives the bin's cells.
//   walldist_sums_kernel / walldist_values_kernel   rows, blocks and samples in fixed order in double; the ratios.
//                         (A row adds at most 62 x 16 voxels in fp32; from there on every sum is in double: on inputs
//                         whose terms are exact in fp32, as the tests' multiples of 1 / 4096, the totals are exact.)
//
// No floating-point atomics; every order of summation is fixed by the indices alone: two calls are bit-equal.
#include "sr3d_eval_march.h"
#include "sr3d_wave_reduce.h"

namespace {

static_assert(kP == 20, "the exchange reduction is laid out for 20 sums");
static_assert((int)SR3D_WALLDIST_SUM_POS == (int)P_NEAR && (int)SR3D_WALLDIST_SUM_POS_ABS == (int)P_NEAR_ABS &&
                  (int)SR3D_WALLDIST_SUM_POS_SQ == (int)P_NEAR_SQ && (int)SR3D_WALLDIST_SUM_OMEGA == (int)P_OMEGA &&
                  (int)SR3D_WALLDIST_SUM_CELLS == kP && (int)SR3D_WALLDIST_COUNT == (int)SR3D_PROFILE_COUNT,
              "the per-bin sums are the per-level sums with POS in the NEAR slots, then CELLS");

constexpr int kW = SR3D_WALLDIST_SUM_COUNT;          // sums per bin
constexpr int kMaxBins = SR3D_WALLDIST_MAX_D + 2;    // 32
constexpr int kDistThreads = 256, kDistWaves = kDistThreads / 64;

// ---- distance transform --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDistThreads) void walldist_x_kernel(const float* __restrict__ b, uint8_t* __restrict__ out,
                                                                 long long rows, int X, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (X + 63) / 64;
  for (long long r = (long long)blockIdx.x * kDistWaves + wave; r < rows; r += (long long)gridDim.x * kDistWaves) {
    const float* br = b + r * X;
    uint8_t* o = out + r * X;
    int last = -C;                                    // nothing built outside the grid: at least C away from every x >= 0
    for (int c = 0; c < nch; c++) {
      const int x = c * 64 + lane;
      const bool built = x < X && 1.0f - br[x] > 0.f;
      const unsigned long long m = __ballot(built);
      const unsigned long long below = m & (~0ull >> (63 - lane));
      const int pos = below ? c * 64 + 63 - __clzll((long long)below) : last;
      if (x < X) o[x] = (uint8_t)min(x - pos, C);
      if (m) last = c * 64 + 63 - __clzll((long long)m);
    }
    int next = X - 1 + C;
    for (int c = nch - 1; c >= 0; c--) {
      const int x = c * 64 + lane;
      const bool built = x < X && 1.0f - br[x] > 0.f;
      const unsigned long long m = __ballot(built);
      const unsigned long long above = m >> lane;
      const int pos = above ? x + __ffsll((long long)above) - 1 : next;
      if (x < X) o[x] = (uint8_t)min((int)o[x], min(pos - x, C));   // the lane's own byte of the first sweep
      if (m) next = c * 64 + __ffsll((long long)m) - 1;
    }
  }
}

// out = min over k of max(|k|, in(pos + k)) along the axis of `stride` elements and extent n; block (x: voxels of a
// sample, y: sample), so that a voxel's index within its sample and its position on the axis are 32-bit arithmetic
__global__ __launch_bounds__(kDistThreads) void walldist_axis_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                    unsigned zyx, unsigned stride, unsigned n) {
  const unsigned r = blockIdx.x * kDistThreads + threadIdx.x;
  if (r >= zyx) return;
  const long long i = (long long)blockIdx.y * zyx + r;
  const int pos = (int)((r / stride) % n);
  int best = in[i];
  // four steps a round, their loads independent of each other; a step at or beyond `best` cannot lower it
  for (int k0 = 1; k0 < best; k0 += 4) {
    int lo[4], hi[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = k0 + u;
      lo[u] = pos - k >= 0 ? (int)in[i - (long long)k * stride] : 255;
      hi[u] = pos + k < (int)n ? (int)in[i + (long long)k * stride] : 255;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) best = min(best, max(k0 + u, min(lo[u], hi[u])));
  }
  out[i] = (uint8_t)best;
}

// ---- per-bin evaluation --------------------------------------------------------------------------------------------
struct BinParams : MarchInputs {
  const uint8_t* dist;
  int D;
  double* part;   // [B][blocks][D + 2][kW]
  float* sums;    // kW, D + 2
  float* values;  // SR3D_WALLDIST_COUNT, D + 2
};

// the march's sink: the wave of a row adds the terms of a plane into the row's [bin][sum], bin by bin
struct BinSums {
  float (*binsum)[kMaxBins][kW];
  const uint8_t (*dcol)[MY][64];   // the column's distance bytes [plane][row][lane]
  int top;                 // D + 1: the bin of everything farther
  int lane, row, slot;
  bool owner;
  __device__ __forceinline__ void voxel(int, const float (&)[kP]) {}
  __device__ __forceinline__ void interior(const float (&)[kP]) {}
  __device__ __forceinline__ void plane(int j, float (&v)[kP]) {     // a lane without a voxel brings zeros
    const float pos = v[P_B] > 0.f ? 1.f : 0.f;
    v[P_NEAR] = pos, v[P_NEAR_ABS] = pos * v[P_ABS], v[P_NEAR_SQ] = pos * v[P_SQ];
    const int bin = owner ? min((int)dcol[j % MZS][row - 1][lane], top) : -1;
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {                                                   // wave-uniform
      const int cur = __shfl(bin, __ffsll((long long)todo) - 1, 64);
      const bool mine = bin == cur;
      const unsigned long long sel = __ballot(mine);
      todo &= ~sel;
      float w[kP];
#pragma unroll
      for (int i = 0; i < kP; i++) w[i] = mine ? v[i] : 0.f;
      wave_reduce20(w, lane);
      float* s = binsum[row - 1][cur];
      if (slot >= 0) s[slot] += w[0];
      if (lane == 1) s[kP] += (float)__popcll(sel);
    }
  }
};

__global__ __launch_bounds__(kMarchThreads) void walldist_profile_kernel(const BinParams q) {
#pragma clang fp contract(off)
  __shared__ float tile[2][MF][MROWS][64];
  __shared__ float binsum[MY][kMaxBins][kW];
  __shared__ uint8_t dcol[MZS][MY][64];
  for (int i = threadIdx.x; i < MY * kMaxBins * kW; i += kMarchThreads) (&binsum[0][0][0])[i] = 0.f;
  const MarchPlace at = march_place(q);
  // the thread's distance bytes of the whole column, all loads in flight at once (one byte a plane inside the march
  // would put a memory round trip into every plane); a thread reads back only what it wrote
  if (at.owner) {
    const long long sz = (long long)q.Y * q.X;
    const uint8_t* col = q.dist + ((long long)at.bi * q.Z + at.tiz * MZS) * sz + ((long long)at.y * q.X + at.x);
    const int nz = min(MZS, q.Z - at.tiz * MZS);
    uint8_t d[MZS];
#pragma unroll
    for (int k = 0; k < MZS; k++) d[k] = col[min(k, nz - 1) * sz];    // no branch: past the top, the top plane again
#pragma unroll
    for (int k = 0; k < MZS; k++) dcol[k][at.row - 1][at.lane] = d[k];
  }
  __syncthreads();
  BinSums sums{binsum, dcol, q.D + 1, at.lane, at.row, reduce20_slot(at.lane), at.owner};
  eval_march(q, tile, sums);

  __syncthreads();
  // the rows in fixed order, in double like everything after them: where a row's fp32 sums are exact the totals are
  const int nrep = (q.D + 2) * kW;
  double* dst = q.part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * nrep;
  for (int i = threadIdx.x; i < nrep; i += kMarchThreads) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < MY; w++) s += (double)(&binsum[w][0][0])[i];
    dst[i] = s;
  }
}

constexpr int kFinalThreads = 1024, kFinalSlots = kFinalThreads / 32;
static_assert(kW <= 32, "one thread of 32 per sum");

// one block per bin: the partials of every block of every sample, in a fixed order
__global__ __launch_bounds__(kFinalThreads) void walldist_sums_kernel(const BinParams q, int nparts) {
  __shared__ double red[kFinalSlots][32];
  const int k = blockIdx.x, nb = q.D + 2;
  const int a = threadIdx.x & 31, s = threadIdx.x >> 5;
  double v = 0.0;
  if (a < kW)
    for (int i = s; i < nparts; i += kFinalSlots) v += q.part[((long long)i * nb + k) * kW + a];
  red[s][a] = v;
  __syncthreads();
  if (threadIdx.x < kW) {
    double t = 0.0;
    for (int w = 0; w < kFinalSlots; w++) t += red[w][threadIdx.x];
    q.sums[threadIdx.x * nb + k] = (float)t;
  }
}

// one thread per bin: the ratios, from the fp32 sums the caller also gets
__global__ __launch_bounds__(64) void walldist_values_kernel(const BinParams q) {
  const int k = threadIdx.x, nb = q.D + 2;
  if (k >= nb) return;
  const float eps = 1e-30f;   // the modules' default
  auto F = [&](int i) { return q.sums[i * nb + k]; };
  auto put = [&](int i, float val) { q.values[i * nb + k] = val; };
  const float cells = F(kP);
  put(SR3D_WALLDIST_L1, F(P_ABS) / (4.f * cells));    // no eps: an empty bin is 0 / 0 = nan
  put(SR3D_WALLDIST_L2, F(P_SQ) / (4.f * cells));
  put(SR3D_WALLDIST_MASKED_L1, F(P_B_ABS) / (4.f * F(P_B) + eps));
  put(SR3D_WALLDIST_MASKED_L2, F(P_B_SQ) / (4.f * F(P_B) + eps));
  // cumulative over the bins 0 .. k: the reference's near-wall modules with num_filter_applications = k
  double cp = 0.0, ca = 0.0, cs = 0.0;
  for (int j = 0; j <= k; j++)
    cp += (double)q.sums[P_NEAR * nb + j], ca += (double)q.sums[P_NEAR_ABS * nb + j], cs += (double)q.sums[P_NEAR_SQ * nb + j];
  put(SR3D_WALLDIST_MASKED_L1_NEAR_WALL, (float)ca / (4.f * (float)cp + eps));
  put(SR3D_WALLDIST_MASKED_L2_NEAR_WALL, (float)cs / (4.f * (float)cp + eps));
  const float n_grid = F(P_B_INT) - F(P_NEAR_INT);   // no eps: 0 / 0 = nan, as in the per-level call
  put(SR3D_WALLDIST_RESIDUAL_CONTINUITY, F(P_RES_P) / n_grid);
  put(SR3D_WALLDIST_RESIDUAL_CONTINUITY_TARGET, F(P_RES_T) / n_grid);
  put(SR3D_WALLDIST_ABS_DIFF_TEMPERATURE, F(P_T) / (F(P_B) + eps));
  put(SR3D_WALLDIST_DIFF_VELOCITY_NORM, F(P_V) / (F(P_B) + eps));
  put(SR3D_WALLDIST_ABS_DIFF_DIVERGENCE, F(P_DDIV) / n_grid);
  put(SR3D_WALLDIST_DIFF_OMEGA_NORM, F(P_OMEGA) / n_grid);
  for (int c = 0; c < 4; c++) put(SR3D_WALLDIST_CHANNELWISE_MSE_T + c, F(P_SQ_T + c) / cells);
}
static_assert(kMaxBins <= 64, "one thread per bin");

int dist_blocks(long long work_items) {
  const long long nb = (work_items + kDistThreads - 1) / kDistThreads;
  return (int)(nb < 1 ? 1 : nb > 65536 ? 65536 : nb);
}

}  // namespace

extern "C" {

size_t sr3d_wall_distance_workspace_bytes(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)B * Z * Y * X;
}

int sr3d_wall_distance(const void* b, void* dist_out, int B, int Z, int Y, int X, int cap, void* workspace,
                       void* stream) {
  SR3D_CHECK(b && dist_out && workspace, SR3D_E_ARG, "wall_distance: null pointer");
  SR3D_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "wall_distance: non-positive dimension");
  SR3D_CHECK((long long)Z * Y * X < (1ll << 31), SR3D_E_ARG, "wall_distance: grid has >= 2^31 voxels");
  SR3D_CHECK(B <= 65535, SR3D_E_ARG, "wall_distance: batch too large");
  SR3D_CHECK(cap >= 1 && cap <= 254, SR3D_E_ARG, "wall_distance: cap must be in 1 .. 254 (got %d)", cap);
  const long long total = (long long)B * Z * Y * X, rows = (long long)B * Z * Y;
  uint8_t* out = (uint8_t*)dist_out;
  uint8_t* tmp = (uint8_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  SrProfScope prof(SR3D_PROF_DATA, 5.0 * (double)total, st);   // the mask in (4 B), the distance out (1 B) per voxel
  hipLaunchKernelGGL(walldist_x_kernel, dim3(dist_blocks(rows * 64)), dim3(kDistThreads), 0, st, (const float*)b, out,
                     rows, X, cap + 1);
  SR3D_HIP(hipGetLastError());
  const unsigned zyx = (unsigned)((long long)Z * Y * X);
  const dim3 per_voxel((zyx + kDistThreads - 1) / kDistThreads, B);
  hipLaunchKernelGGL(walldist_axis_kernel, per_voxel, dim3(kDistThreads), 0, st, out, tmp, zyx, (unsigned)X, (unsigned)Y);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(walldist_axis_kernel, per_voxel, dim3(kDistThreads), 0, st, tmp, out, zyx, (unsigned)(Y * X),
                     (unsigned)Z);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

size_t sr3d_eval_wall_distance_profiles_workspace_bytes(int B, int Z, int Y, int X, int D) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || D < 1 || D > SR3D_WALLDIST_MAX_D) return 0;
  return (size_t)B * march_blocks(Z, Y, X) * (D + 2) * kW * sizeof(double);
}

int sr3d_eval_wall_distance_profiles(const void* p, const void* t, const void* b, const void* dist, int B, int Z, int Y,
                                     int X, const float stds[4], float delta_meter, int D, void* sums_out,
                                     void* values_out, void* workspace, void* stream) {
  SR3D_CHECK(dist && sums_out && values_out && workspace, SR3D_E_ARG, "eval_wall_distance_profiles: null pointer");
  BinParams q{};
  if (int rc = march_inputs(q, "eval_wall_distance_profiles", p, t, b, B, Z, Y, X, stds, delta_meter)) return rc;
  SR3D_CHECK(D >= 1 && D <= SR3D_WALLDIST_MAX_D, SR3D_E_ARG,
             "eval_wall_distance_profiles: max distance must be in 1 .. %d (got %d)", SR3D_WALLDIST_MAX_D, D);
  SR3D_CHECK(((uintptr_t)workspace & 7) == 0, SR3D_E_ARG, "eval_wall_distance_profiles: workspace must be 8-byte aligned");
  q.dist = (const uint8_t*)dist, q.D = D;
  q.part = (double*)workspace, q.sums = (float*)sums_out, q.values = (float*)values_out;
  const int nbs = march_blocks(Z, Y, X);
  SR3D_CHECK((long long)nbs * B < (1ll << 31), SR3D_E_ARG, "eval_wall_distance_profiles: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  SrProfScope prof(SR3D_PROF_EVAL, 37.0 * (double)B * Z * Y * X, st);   // p, t (32 B) + b (4 B) + dist (1 B) per voxel
  hipLaunchKernelGGL(walldist_profile_kernel, dim3(nbs, B), dim3(kMarchThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(walldist_sums_kernel, dim3(D + 2), dim3(kFinalThreads), 0, st, q, nbs * B);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(walldist_values_kernel, dim3(1), dim3(64), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
