// Near-surface (2 m) temperature: linear extrapolation of each (y, x) column to the building / ground top (gfx950).
//
// GPU form of the reference's make_2m_temperature notebook (infer_2m_height_temperature), which loops over every
// column on the host.  One lane per column, lanes along x: a lane reads the building-top height tz[y, x], finds the
// first level at or above it by comparing with the level heights (never by dividing by dz: tz == H[k] gives k) and
// reads two levels of one channel of an NCDHW fp32 tensor IN PLACE (no slice copy of the model output or of the raw
// HR volume).  Per column, with H the level heights and Z the level count:
//   tz > H[Z-1]                  NaN (building above the top level)
//   first = 0 if !(tz > H[0])    (extrapolation below the lowest level; a NaN tz lands here and gives NaN)
//   first == Z-1                 t1 itself
//   otherwise                    numpy >= 2's evaluation of t1 + (b - h1) * (t2 - t1) / (h2 - h1) with float32 t1, t2
//                                and float64 b, h1, h2: d = t2 - t1 in fp32, the rest in fp64, rounded once to fp32.
// An optional affine step (v * scale, rounded, + mean, rounded: torch's fp32 `data * scales + means`) dimensionalises
// a normalised model output first.
//
// The fused form takes the prediction and the truth (each with its own channel, level count and affine step), writes
// both maps (each optional) and adds sum (p - t)^2, sum |p - t| and the count over the columns where both maps are
// finite into a caller-owned fp64[3] on the device.  The sums are deterministic and per sample: each workgroup writes
// one fp64 partial triple, the last workgroup to arrive (an agent-scope ticket) reduces every sample's partials in a
// fixed order and adds the per-sample totals to the accumulator in sample order -- so two calls on two batches give
// bit for bit what one call on their concatenation gives.  One launch per call.
#include <math.h>

#include "sr3d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLevels = 128;
constexpr int kMaxGridY = 65535;
constexpr size_t kTicketBytes = 16;   // the ticket word, padded: partials start 16-byte aligned

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

struct SurfSrc {
  const float* p;       // element (0, channel, 0, 0, 0)
  long long bstride;    // C * Zs * Y * X
  int levels;
  int affine;
  float scale, mean;
};

struct SurfParams {
  SurfSrc src[2];       // prediction, truth (map-only: src[0])
  float* out[2];        // (B, Y, X) maps, each may be null in the fused form
  const double* tz;     // (Y, X)
  long long plane;      // Y * X
  int nblk;             // workgroups per sample
  int nh;
  double h[kMaxLevels];
  double* part;         // [B][nblk][3]
  unsigned* ticket;
  double* acc;          // [3]
};

__device__ __forceinline__ float level(const SurfSrc& s, int b, int k, long long plane, long long col) {
#pragma clang fp contract(off)
  float v = s.p[(long long)b * s.bstride + (long long)k * plane + col];
  if (s.affine) {
    v = v * s.scale;
    v = v + s.mean;
  }
  return v;
}

__device__ __forceinline__ float column_t2m(const SurfSrc& s, const double* H, double tz, int b, long long plane,
                                            long long col) {
#pragma clang fp contract(off)
  const int Z = s.levels;
  if (tz > H[Z - 1]) return __builtin_nanf("");
  int first = 0;
  if (tz > H[0]) {
    first = 1;
    while (!(H[first] >= tz)) first++;   // ends: H[Z-1] >= tz
  }
  const float t1 = level(s, b, first, plane, col);
  if (first == Z - 1) return t1;
  const float t2 = level(s, b, first + 1, plane, col);
  const float d = t2 - t1;
  const double h1 = H[first], h2 = H[first + 1];
  const double r = (double)t1 + ((tz - h1) * (double)d) / (h2 - h1);
  return (float)r;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool FUSED>
__global__ __launch_bounds__(kThreads) void surface_t2m_kernel(const SurfParams q) {
#pragma clang fp contract(off)
  __shared__ double H[kMaxLevels];
  __shared__ double red[3][kThreads];
  __shared__ int last;
  for (int k = threadIdx.x; k < q.nh; k += kThreads) H[k] = q.h[k];
  __syncthreads();

  const int b = blockIdx.y;
  const long long col = (long long)blockIdx.x * kThreads + threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  if (col < q.plane) {
    const double tz = q.tz[col];
    const float pv = column_t2m(q.src[0], H, tz, b, q.plane, col);
    if (q.out[0]) q.out[0][(long long)b * q.plane + col] = pv;
    if (FUSED) {
      const float tv = column_t2m(q.src[1], H, tz, b, q.plane, col);
      if (q.out[1]) q.out[1][(long long)b * q.plane + col] = tv;
      if (isfinite(pv) && isfinite(tv)) {
        const double d = (double)pv - (double)tv;
        a[0] = d * d, a[1] = fabs(d), a[2] = 1.0;
      }
    }
  }
  if (!FUSED) return;

  // ---- one partial triple per workgroup: wave sums, then the waves in a fixed order
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double v = wave_sum(a[k]);
    if (lane == 0) red[k][w] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* dst = q.part + ((long long)b * q.nblk + blockIdx.x) * 3;
    for (int k = 0; k < 3; k++) {
      double v = 0.0;
      for (int i = 0; i < kWaves; i++) v += red[k][i];
      // write-through (sc1) store: visible to the last workgroup on any XCD without a release fence
      __hip_atomic_store((gu64*)(dst + k), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the partials have left before the ticket is drawn
    const unsigned total = gridDim.x * gridDim.y;
    const unsigned t = __hip_atomic_fetch_add((gu32*)q.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == total - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;

  // ---- the last workgroup: per sample, its partials in a fixed order; then acc += that sample's sums, in order
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  const int B = gridDim.y;
  for (int s = 0; s < B; s++) {
    const double* ps = q.part + (long long)s * q.nblk * 3;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < q.nblk; i += kThreads)
#pragma unroll
      for (int k = 0; k < 3; k++)
        v[k] += __builtin_bit_cast(double, __hip_atomic_load((gu64*)(ps + (long long)i * 3 + k), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
    for (int k = 0; k < 3; k++) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o)
#pragma unroll
        for (int k = 0; k < 3; k++) red[k][threadIdx.x] += red[k][threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x < 3) q.acc[threadIdx.x] += red[threadIdx.x][0];
    __syncthreads();
  }
  if (threadIdx.x == 0) __hip_atomic_store((gu32*)q.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int blocks_per_sample(int Y, int X) { return (int)(((long long)Y * X + kThreads - 1) / kThreads); }

int check_src(const sr3d_surface_src_t* s, int nheights, const char* what, const char* name) {
  SR3D_CHECK(s && s->data, SR3D_E_ARG, "%s: null %s", what, name);
  SR3D_CHECK(s->C > 0 && s->Zs > 0, SR3D_E_ARG, "%s: %s: non-positive C or Zs", what, name);
  SR3D_CHECK(s->channel >= 0 && s->channel < s->C, SR3D_E_ARG, "%s: %s: channel %d outside [0, %d)", what, name,
             s->channel, s->C);
  SR3D_CHECK(s->levels >= 1 && s->levels <= s->Zs, SR3D_E_ARG, "%s: %s: levels %d outside [1, Zs = %d]", what, name,
             s->levels, s->Zs);
  SR3D_CHECK(s->levels <= nheights, SR3D_E_ARG, "%s: %s: %d levels but %d heights", what, name, s->levels, nheights);
  SR3D_CHECK(!s->affine || (isfinite(s->scale) && isfinite(s->mean)), SR3D_E_ARG,
             "%s: %s: affine scale / mean not finite", what, name);
  return SR3D_OK;
}

int check_common(int B, int Y, int X, const void* tz, const double* heights, int nheights, const char* what) {
  SR3D_CHECK(B > 0 && Y > 0 && X > 0, SR3D_E_ARG, "%s: non-positive dimension", what);
  SR3D_CHECK(B <= kMaxGridY, SR3D_E_ARG, "%s: batch %d > %d", what, B, kMaxGridY);
  SR3D_CHECK((long long)Y * X < (1ll << 31), SR3D_E_ARG, "%s: a (y, x) plane has >= 2^31 columns", what);
  SR3D_CHECK(tz, SR3D_E_ARG, "%s: null building height map", what);
  SR3D_CHECK(heights && nheights >= 1 && nheights <= kMaxLevels, SR3D_E_ARG, "%s: %d level heights (1 .. %d)", what,
             nheights, kMaxLevels);
  for (int k = 0; k < nheights; k++) {
    SR3D_CHECK(isfinite(heights[k]), SR3D_E_ARG, "%s: level height %d is not finite", what, k);
    SR3D_CHECK(k == 0 || heights[k] > heights[k - 1], SR3D_E_ARG, "%s: level heights must increase strictly", what);
  }
  return SR3D_OK;
}

SurfSrc make_src(const sr3d_surface_src_t* s, int Y, int X) {
  SurfSrc r{};
  const long long plane = (long long)Y * X;
  r.p = (const float*)s->data + (long long)s->channel * s->Zs * plane;
  r.bstride = (long long)s->C * s->Zs * plane;
  r.levels = s->levels;
  r.affine = s->affine ? 1 : 0;
  r.scale = s->scale, r.mean = s->mean;
  return r;
}

void fill_common(SurfParams& q, int Y, int X, const void* tz, const double* heights, int nheights) {
  q.tz = (const double*)tz;
  q.plane = (long long)Y * X;
  q.nblk = blocks_per_sample(Y, X);
  q.nh = nheights;
  for (int k = 0; k < nheights; k++) q.h[k] = heights[k];
}

}  // namespace

extern "C" {

size_t sr3d_surface_temperature_workspace_bytes(int B, int Y, int X) {
  if (B <= 0 || Y <= 0 || X <= 0) return 0;
  return kTicketBytes + (size_t)B * blocks_per_sample(Y, X) * 3 * sizeof(double);
}

int sr3d_surface_temperature(const sr3d_surface_src_t* src, int B, int Y, int X, const void* tz,
                             const double* heights, int nheights, void* out, void* stream) {
  const char* what = "surface_temperature";
  int rc = check_common(B, Y, X, tz, heights, nheights, what);
  if (rc) return rc;
  if ((rc = check_src(src, nheights, what, "src"))) return rc;
  SR3D_CHECK(out, SR3D_E_ARG, "%s: null output", what);
  SurfParams q{};
  fill_common(q, Y, X, tz, heights, nheights);
  q.src[0] = make_src(src, Y, X);
  q.out[0] = (float*)out;
  hipLaunchKernelGGL(surface_t2m_kernel<false>, dim3(q.nblk, B), dim3(kThreads), 0, (hipStream_t)stream, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

int sr3d_surface_temperature_errors(const sr3d_surface_src_t* pred, const sr3d_surface_src_t* truth, int B, int Y,
                                    int X, const void* tz, const double* heights, int nheights, void* pred_out,
                                    void* truth_out, void* acc, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* what = "surface_temperature_errors";
  int rc = check_common(B, Y, X, tz, heights, nheights, what);
  if (rc) return rc;
  if ((rc = check_src(pred, nheights, what, "prediction"))) return rc;
  if ((rc = check_src(truth, nheights, what, "truth"))) return rc;
  SR3D_CHECK(acc, SR3D_E_ARG, "%s: null accumulator", what);
  SR3D_CHECK(workspace, SR3D_E_ARG, "%s: null workspace", what);
  SR3D_CHECK(workspace_bytes >= sr3d_surface_temperature_workspace_bytes(B, Y, X), SR3D_E_WORKSPACE,
             "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
             sr3d_surface_temperature_workspace_bytes(B, Y, X));
  SurfParams q{};
  fill_common(q, Y, X, tz, heights, nheights);
  SR3D_CHECK((long long)q.nblk * B < (1ll << 32), SR3D_E_ARG, "%s: too many workgroups", what);
  q.src[0] = make_src(pred, Y, X);
  q.src[1] = make_src(truth, Y, X);
  q.out[0] = (float*)pred_out, q.out[1] = (float*)truth_out;
  q.ticket = (unsigned*)workspace;
  q.part = (double*)((char*)workspace + kTicketBytes);
  q.acc = (double*)acc;
  hipLaunchKernelGGL(surface_t2m_kernel<true>, dim3(q.nblk, B), dim3(kThreads), 0, (hipStream_t)stream, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
