// Error-distribution evaluation (gfx950): histograms, exact min / max and cell counts of 13 per-voxel series over the
// fluid cells, split into near-wall and far cells, from ONE streaming pass over (p, t, b, dist): 36 B + 1 B per voxel.
// No stencil, so no marching (sr3d_eval_march.h): a voxel's contribution depends on that voxel alone.
//
//   eval_dist_kernel   block (x: group g of the sample, y: sample).  A sample's voxels are cut into G contiguous ranges
//                      (G depends on Z*Y*X alone, so a one-sample call cuts as the batch call does); a workgroup walks
//                      its range kDistThreads items at a time.  VEC: an item is 4 consecutive voxels, read with 16-byte
//                      loads -- taken when every channel plane is 16-byte aligned (Z*Y*X % 4 == 0 and aligned bases);
//                      otherwise an item is one voxel and every load is a dword (a wave still reads 256 contiguous
//                      bytes a plane), which takes any contiguous tensor.
//                      Counters: uint32 histograms in LDS, [series][class][slot] + the 3 cell counts = 6737 words, in
//                      kCopies = 2 copies picked by lane parity (54 KB), one no-return LDS add per series and voxel.
//                      Errors pile into a few bins -- with p == t every lane of every wave adds to the same counter --
//                      but the LDS takes that well: measured, p == t costs 13 % more than noisy fields, while taking
//                      out the first lane's bin with a ballot beforehand (one add of the popcount) cost 13 % on noisy
//                      fields and gained 2 % at p == t, so it is not done.
//                      A workgroup bins fewer than 2^31 voxels (one sample's at most): a uint32 counter cannot overflow.
//                      Min / max: 52 registers per thread (fminf / fmaxf drop a NaN operand, which is also how a value of
//                      the other class is kept out), reduced by shuffles, then across the waves in fixed order.
//                      The workgroup stores its record (6737 counters + 52 floats) to the workspace with plain stores.
//   eval_dist_final_kernel   sums the records of a sample (or of all samples) per counter into int64 and folds the
//                      min / max in record order.  Integer adds commute and the order of the min / max folds is fixed by
//                      the indices: the result is bit-reproducible without a global atomic, and since every word that
//                      is read was written by the first kernel nothing needs clearing between calls or graph replays.
//
// The binning rule (include/sr3d.h) is compiled without contraction: __fmul_rn / __fsub_rn are no barrier against it in
// HIP (sr3d_eltwise.hip), the pragma is.  No fast-math flag: sqrtf is the correctly rounded one.
#include <cmath>

#include "sr3d_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSeries = SR3D_DIST_SERIES, kClasses = SR3D_DIST_CLASSES, kSlots = SR3D_DIST_SLOTS;
constexpr int kHist = kSeries * kClasses * kSlots;   // 6734 counters
constexpr int kRec = kHist + 3;                      // + built, near, far cells
constexpr int kMM = kSeries * kClasses * 2;          // 52 min / max values
constexpr int kRecAll = kRec + kMM;                  // words of a workgroup's record in the workspace
constexpr int kCopies = 2;
constexpr int kDistThreads = 1024, kDistWaves = kDistThreads / 64;
constexpr int kMaxGroups = 256;                      // workgroups per sample: one per CU
constexpr int kGroupVoxels = 4 * kDistThreads;       // a sample smaller than G of these gets fewer groups
constexpr int kFinalThreads = 256, kFinalCols = 64, kFinalRows = kFinalThreads / kFinalCols;
static_assert(kCopies * kRec * 4 + kDistWaves * kMM * 4 <= 64 * 1024, "static LDS");
static_assert(kMM <= 64 && kMM <= kFinalThreads, "one thread per min / max value");

struct DistParams {
  const float* p;
  const float* t;
  const float* b;
  const uint8_t* dist;   // or null
  int B, zyx, G, near_width;
  float s[4];
  float lo[kSeries], inv[kSeries];
  unsigned* part;        // [B][G][kRecAll]
  long long* counts;     // ([B],) kHist
  float* minmax;         // ([B],) kMM
  long long* cells;      // ([B],) 3
};

int dist_groups(long long zyx) {
  const long long g = (zyx + kGroupVoxels - 1) / kGroupVoxels;
  return (int)(g < 1 ? 1 : g > kMaxGroups ? kMaxGroups : g);
}

// one count into counter idx of the lane's copy (no-return LDS add)
__device__ __forceinline__ void count(unsigned* h, int idx) { atomicAdd(&h[idx], 1u); }

// slot of value v: 0 underflow, 1 .. 256 the bins, 257 overflow, 258 NaN; clamped as a float, before the conversion
__device__ __forceinline__ int dist_slot(float v, float lo, float inv) {
  const float d = v - lo;
  const float k = floorf(d * inv);
  float c = fminf(fmaxf(k, -1.f), (float)SR3D_DIST_BINS);   // -inf and k < 0: -1; +inf and k >= 256: 256
  c = v != v ? (float)(SR3D_DIST_BINS + 1) : c;
  return (int)c + 1;
}

struct VoxelState {
  float mn[kSeries][kClasses], mx[kSeries][kClasses];
};

__device__ __forceinline__ void dist_voxel(const DistParams& q, unsigned* h, VoxelState& st, const float (&pv)[4],
                                           const float (&tv)[4], float bv, int dbyte) {
  const bool fluid = bv > 0.f;
  const bool near = dbyte <= q.near_width;           // dist == NULL: dbyte is 255 > near_width
  count(h, kHist + (fluid ? (near ? 1 : 2) : 0));
  if (!fluid) return;
  float val[kSeries];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    val[SR3D_DIST_ERR_T + c] = pv[c] - tv[c];
    val[SR3D_DIST_PRED_T + c] = pv[c], val[SR3D_DIST_TRUTH_T + c] = tv[c];
  }
  {
    const float a = q.s[1] * val[SR3D_DIST_ERR_U], b = q.s[2] * val[SR3D_DIST_ERR_V], c = q.s[3] * val[SR3D_DIST_ERR_W];
    const float aa = a * a, bb = b * b, cc = c * c;
    const float ab = aa + bb;
    val[SR3D_DIST_ERR_VEL_NORM] = sqrtf(ab + cc);
  }
  const float qnan = __builtin_nanf("");
  const int cbase = near ? 0 : kSlots;
#pragma unroll
  for (int s = 0; s < kSeries; s++) {
    const float v = val[s];
    count(h, s * (kClasses * kSlots) + cbase + dist_slot(v, q.lo[s], q.inv[s]));
    const float v0 = near ? v : qnan, v1 = near ? qnan : v;   // fminf / fmaxf return the other operand for a NaN
    st.mn[s][0] = fminf(st.mn[s][0], v0), st.mx[s][0] = fmaxf(st.mx[s][0], v0);
    st.mn[s][1] = fminf(st.mn[s][1], v1), st.mx[s][1] = fmaxf(st.mx[s][1], v1);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kDistThreads) void eval_dist_kernel(const DistParams q) {
  __shared__ unsigned hist[kCopies][kRec];
  __shared__ float red[kDistWaves][kMM];
  for (int i = threadIdx.x; i < kCopies * kRec; i += kDistThreads) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* h = hist[lane & (kCopies - 1)];
  const int bi = blockIdx.y, g = blockIdx.x;
  const long long zyx = q.zyx;
  const float* pb = q.p + (long long)bi * 4 * zyx;
  const float* tb = q.t + (long long)bi * 4 * zyx;
  const float* mb = q.b + (long long)bi * zyx;
  const uint8_t* db = q.dist ? q.dist + (long long)bi * zyx : nullptr;
  // the group's range of items (VEC: 4 voxels each)
  const int items = VEC ? q.zyx / 4 : q.zyx;
  const int per = (int)(((long long)items + q.G - 1) / q.G);
  const long long beg_ll = (long long)g * per;
  const int beg = (int)(beg_ll < items ? beg_ll : items);
  const int end = (int)(beg_ll + per < items ? beg_ll + per : items);

  VoxelState st;
#pragma unroll
  for (int s = 0; s < kSeries; s++)
#pragma unroll
    for (int k = 0; k < kClasses; k++) st.mn[s][k] = __builtin_inff(), st.mx[s][k] = -__builtin_inff();

  for (long long i = (long long)beg + threadIdx.x; i < end; i += kDistThreads) {
    if (VEC) {
      f32x4 P[4], T[4];
#pragma unroll
      for (int c = 0; c < 4; c++)
        P[c] = *reinterpret_cast<const f32x4*>(pb + c * zyx + 4 * i), T[c] = *reinterpret_cast<const f32x4*>(tb + c * zyx + 4 * i);
      const f32x4 Bv = *reinterpret_cast<const f32x4*>(mb + 4 * i);
      const unsigned dw = db ? *reinterpret_cast<const unsigned*>(db + 4 * i) : 0xffffffffu;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const float pv[4] = {P[0][u], P[1][u], P[2][u], P[3][u]}, tv[4] = {T[0][u], T[1][u], T[2][u], T[3][u]};
        dist_voxel(q, h, st, pv, tv, Bv[u], (int)((dw >> (8 * u)) & 0xffu));
      }
    } else {
      float pv[4], tv[4];
#pragma unroll
      for (int c = 0; c < 4; c++) pv[c] = pb[c * zyx + i], tv[c] = tb[c * zyx + i];
      dist_voxel(q, h, st, pv, tv, mb[i], db ? (int)db[i] : 255);
    }
  }

  // min / max: across the wave by shuffles, across the waves in fixed order
#pragma unroll
  for (int s = 0; s < kSeries; s++)
#pragma unroll
    for (int k = 0; k < kClasses; k++) {
      float mn = st.mn[s][k], mx = st.mx[s][k];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64)), mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      if (lane == 0) red[wave][(s * kClasses + k) * 2] = mn, red[wave][(s * kClasses + k) * 2 + 1] = mx;
    }
  __syncthreads();   // also: every LDS count of the workgroup has landed
  unsigned* rec = q.part + ((long long)bi * q.G + g) * kRecAll;
  for (int i = threadIdx.x; i < kRec; i += kDistThreads) {
    unsigned v = 0;
#pragma unroll
    for (int c = 0; c < kCopies; c++) v += hist[c][i];
    rec[i] = v;
  }
  if (threadIdx.x < kMM) {
    float m = red[0][threadIdx.x];
    for (int w = 1; w < kDistWaves; w++) m = (threadIdx.x & 1) ? fmaxf(m, red[w][threadIdx.x]) : fminf(m, red[w][threadIdx.x]);
    rec[kRec + threadIdx.x] = __float_as_uint(m);
  }
}

// block (x: 64 counters, the last block: the min / max values; y: sample, or 0 for the whole batch)
__global__ __launch_bounds__(kFinalThreads) void eval_dist_final_kernel(const DistParams q, int per_sample) {
  __shared__ unsigned long long red[kFinalRows][kFinalCols];
  const int gs = blockIdx.y;
  const int nparts = (per_sample ? 1 : q.B) * q.G;
  const unsigned* base = q.part + (long long)(per_sample ? gs : 0) * q.G * kRecAll;
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x < kMM) {
      const bool is_max = threadIdx.x & 1;
      float m = is_max ? -__builtin_inff() : __builtin_inff();
      for (int i = 0; i < nparts; i++) {
        const float v = __uint_as_float(base[(long long)i * kRecAll + kRec + threadIdx.x]);
        m = is_max ? fmaxf(m, v) : fminf(m, v);
      }
      q.minmax[(long long)gs * kMM + threadIdx.x] = m;
    }
    return;
  }
  const int col = threadIdx.x % kFinalCols, row = threadIdx.x / kFinalCols;
  const int c = blockIdx.x * kFinalCols + col;
  unsigned long long v = 0;
  if (c < kRec)
    for (int i = row; i < nparts; i += kFinalRows) v += base[(long long)i * kRecAll + c];
  red[row][col] = v;
  __syncthreads();
  if (row == 0 && c < kRec) {
    unsigned long long tot = 0;
#pragma unroll
    for (int r = 0; r < kFinalRows; r++) tot += red[r][col];
    if (c < kHist) q.counts[(long long)gs * kHist + c] = (long long)tot;
    else q.cells[(long long)gs * 3 + (c - kHist)] = (long long)tot;
  }
}

}  // namespace

extern "C" {

size_t sr3d_eval_distributions_workspace_bytes(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)B * dist_groups((long long)Z * Y * X) * kRecAll * sizeof(unsigned);
}

int sr3d_eval_distributions(const void* p, const void* t, const void* b, const void* dist, int B, int Z, int Y, int X,
                            const float stds[4], const float lo[SR3D_DIST_SERIES], const float hi[SR3D_DIST_SERIES],
                            int near_width, int per_sample, void* counts_out, void* minmax_out, void* cells_out,
                            void* workspace, void* stream) {
  const char* who = "eval_distributions";
  SR3D_CHECK(p && t && b && stds && lo && hi && counts_out && minmax_out && cells_out && workspace, SR3D_E_ARG,
             "%s: null pointer", who);
  SR3D_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "%s: non-positive dimension", who);
  SR3D_CHECK((long long)Z * Y * X < (1ll << 31), SR3D_E_ARG, "%s: grid has >= 2^31 voxels", who);
  SR3D_CHECK(B <= 65535, SR3D_E_ARG, "%s: batch too large", who);
  SR3D_CHECK(!dist || (near_width >= 0 && near_width <= 254), SR3D_E_ARG,
             "%s: near_width must be in 0 .. 254 (got %d)", who, near_width);
  SR3D_CHECK((((uintptr_t)p | (uintptr_t)t | (uintptr_t)b | (uintptr_t)workspace | (uintptr_t)minmax_out) & 3) == 0,
             SR3D_E_ARG, "%s: p, t, b, minmax_out and workspace must be 4-byte aligned", who);
  SR3D_CHECK((((uintptr_t)counts_out | (uintptr_t)cells_out) & 7) == 0, SR3D_E_ARG,
             "%s: counts_out and cells_out must be 8-byte aligned", who);
  DistParams q{};
  for (int s = 0; s < kSeries; s++) {
    SR3D_CHECK(std::isfinite(lo[s]) && std::isfinite(hi[s]) && hi[s] > lo[s], SR3D_E_ARG,
               "%s: series %d needs finite bounds with lo < hi (got %g, %g)", who, s, (double)lo[s], (double)hi[s]);
    q.lo[s] = lo[s];
    q.inv[s] = (float)((double)SR3D_DIST_BINS / ((double)hi[s] - (double)lo[s]));
    SR3D_CHECK(std::isfinite(q.inv[s]) && q.inv[s] > 0.f, SR3D_E_ARG, "%s: series %d: the range %g .. %g is too narrow", who, s,
               (double)lo[s], (double)hi[s]);
  }
  const long long zyx = (long long)Z * Y * X;
  q.p = (const float*)p, q.t = (const float*)t, q.b = (const float*)b, q.dist = (const uint8_t*)dist;
  q.B = B, q.zyx = (int)zyx, q.G = dist_groups(zyx), q.near_width = dist ? near_width : 0;
  for (int i = 0; i < 4; i++) q.s[i] = stds[i];
  q.part = (unsigned*)workspace, q.counts = (long long*)counts_out, q.minmax = (float*)minmax_out;
  q.cells = (long long*)cells_out;
  const bool vec = zyx % 4 == 0 && (((uintptr_t)p | (uintptr_t)t | (uintptr_t)b) & 15) == 0 && ((uintptr_t)dist & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
  SrProfScope prof(SR3D_PROF_EVAL, 37.0 * (double)B * (double)zyx, st);   // p, t (32 B) + b (4 B) + dist (1 B) per voxel
  if (vec) hipLaunchKernelGGL((eval_dist_kernel<true>), dim3(q.G, B), dim3(kDistThreads), 0, st, q);
  else hipLaunchKernelGGL((eval_dist_kernel<false>), dim3(q.G, B), dim3(kDistThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(eval_dist_final_kernel, dim3((kRec + kFinalCols - 1) / kFinalCols + 1, per_sample ? B : 1),
                     dim3(kFinalThreads), 0, st, q, per_sample ? 1 : 0);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
