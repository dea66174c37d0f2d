// The interpolation baseline (gfx950): the `fill_na` cell of the reference's plotting notebooks
// (pytorch/notebook/plot_horizontal_sections_at_various_locations.ipynb, "Define methods") without xarray and without
// a materialised trilinear volume.
//
//   1. trilinear upsample x s (s = 2, 4) of the LR field, F.interpolate(mode="trilinear", align_corners=False,
//      scale_factor=s): per axis src = max(0, (1/s)(dst + 0.5) - 0.5), i0 = floor(src), i1 = min(i0 + 1, n - 1),
//      l1 = src - i0, l0 = 1 - l1 (exact dyadic fractions), value = wz0*(wy0*(wx0*v000 + wx1*v001) + wy1*(..)) +
//      wz1*(..) in fp32, every w0*a + w1*b as fma(a, w0, fl(w1*b)) and nothing else contracted (lerp2 below).  The
//      bracket of one LR level does not depend on the HR level, so a lane keeps the two brackets it is between and
//      every LR cell is read once per HR column.
//   2. a cell is NaN where lr_is_in_build[z/s][y/s][x/s] != 0; a NaN of step 1 stays.
//   3. NaN cells are filled along z, then y, then x as xarray's interpolate_na(method="linear",
//      fill_value="extrapolate") does on index coordinates, i.e. scipy's interp1d(kind="linear"): a line with no NaN
//      or with fewer than two valid cells is left alone; otherwise a NaN cell i between valid cells lo < i < hi, or
//      past an end with (lo, hi) the two valid cells nearest that end, becomes
//      float((double(y_hi) - double(y_lo)) / (hi - lo) * (i - lo) + double(y_lo)).
//
// Three passes, stream-ordered, in place on the output, no host synchronisation:
//   interp_column_kernel   one lane per V (4 or 1) x-adjacent HR columns, lanes along x and then y, so a wavefront
//                          stores contiguous rows level by level (16 bytes per lane when V = 4).  The z fill is a
//                          scalar state per column: the last two valid levels and how many there were.  A valid
//                          level closes the gap below it (and, being the second one, the levels under the first);
//                          the levels above the last valid one are written after the walk.  Those writes go to cells
//                          the SAME lane stored as NaN before.  A column left with NaN marks xflag[bc][x].
//   interp_fill_y_kernel   one lane per (bc, z, x) line along y, lanes along x; lines of an unmarked x return at once;
//                          the others are loaded kChunk cells at a time.  A line left with NaN marks zflag[bc][z].
//   interp_fill_x_kernel   one lane per (bc, z, y) line along x; lines of an unmarked level return at once.  What is
//                          still NaN on a line is added to the count (integer atomic: the order cannot matter).
// The in-place hazard: in every pass a line is read and written by ONE lane only, which reads a cell before it writes
// any cell of that line at or above it and never reads what it wrote, so "valid" always means "valid before this
// pass"; the passes are separate launches.  Nothing depends on scheduling.
#include <math.h>

#include "sr3d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8;             // cells of a y line loaded before any of them is looked at

struct InterpParams {
  const float* lr;
  long long bstride, cstride;         // elements between samples / channels of lr
  const unsigned char* mask;          // (z, y, x)
  float* out;                         // (B, C, Zh, Yh, Xh) dense
  int* xflag;                         // (B * C, Xh)
  int* zflag;                         // (B * C, Zh)
  int* count;
  int B, C, z, y, x, shift, Zh, Yh, Xh;
  float inv;                          // 1 / s
};

__device__ __forceinline__ void src_index(int dst, float inv, int n, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
  float src = inv * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  w1 = src - (float)i0;
  w0 = 1.0f - w1;
}

// w0 * v0 + w1 * v1 the way ATen's CPU kernel for contiguous tensors rounds it (its `t0 * w0; += t1 * w1` compiled with
// contraction): the second product rounded to fp32, then one fused multiply-add.  Written out, so that no compiler
// setting moves it: with it the upsample is bit-equal to that kernel, not only within the rounding of a reordered sum.
__device__ __forceinline__ float lerp2(float w0, float v0, float w1, float v1) {
#pragma clang fp contract(off)
  const float hi = w1 * v1;
  return __builtin_fmaf(v0, w0, hi);
}

// the fill of one line as a running state: n valid cells so far, the last one (ka, va), the one before (kb, vb)
struct LineFill {
  int n, ka, kb;
  float va, vb;
};

__device__ __forceinline__ float line_value(int lo, float ylo, int hi, float yhi, int i) {
#pragma clang fp contract(off)
  const double slope = ((double)yhi - (double)ylo) / (double)(hi - lo);
  return (float)(slope * (double)(i - lo) + (double)ylo);
}

// cell k of the line holds the valid value v: fill the NaN cells it brackets
__device__ __forceinline__ void fill_valid(LineFill& f, float* line, long long stride, int k, float v) {
  if (f.n >= 1) {
    for (int i = f.ka + 1; i < k; i++) line[i * stride] = line_value(f.ka, f.va, k, v, i);
    if (f.n == 1)                                          // the second valid cell: extrapolate below the first
      for (int i = 0; i < f.ka; i++) line[i * stride] = line_value(f.ka, f.va, k, v, i);
  }
  f.kb = f.ka, f.vb = f.va, f.ka = k, f.va = v, f.n++;
}

// after the last cell: extrapolate above the last valid one; returns the number of cells left NaN
__device__ __forceinline__ int fill_finish(const LineFill& f, float* line, long long stride, int n) {
  if (f.n <= 1) return n - f.n;
  for (int i = f.ka + 1; i < n; i++) line[i * stride] = line_value(f.kb, f.vb, f.ka, f.va, i);
  return 0;
}

template <int V>
__global__ __launch_bounds__(kThreads) void interp_column_kernel(const InterpParams q) {
#pragma clang fp contract(off)
  const long long plane = (long long)q.Yh * q.Xh;
  const long long per = plane / V;                        // lanes of one (b, c): V divides Xh
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= per * q.B * q.C) return;
  const int bc = (int)(t / per);
  const long long p = (t - (long long)bc * per) * V;
  const int yh = (int)(p / q.Xh), x0 = (int)(p - (long long)yh * q.Xh);
  const int b = bc / q.C, c = bc - b * q.C;
  const float* src = q.lr + (long long)b * q.bstride + (long long)c * q.cstride;
  const long long lplane = (long long)q.y * q.x;

  int y0, y1;
  float wy0, wy1;
  src_index(yh, q.inv, q.y, y0, y1, wy0, wy1);
  int xa[V], xb[V], moff[V];
  float wx0[V], wx1[V];
#pragma unroll
  for (int j = 0; j < V; j++) {
    src_index(x0 + j, q.inv, q.x, xa[j], xb[j], wx0[j], wx1[j]);
    moff[j] = (yh >> q.shift) * q.x + ((x0 + j) >> q.shift);
  }
  // the (y, x) bracket of LR level k for the lane's columns
  auto bracket = [&](int k, float* r) {
    const float* r0 = src + (long long)k * lplane + (long long)y0 * q.x;
    const float* r1 = src + (long long)k * lplane + (long long)y1 * q.x;
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float a = lerp2(wx0[j], r0[xa[j]], wx1[j], r0[xb[j]]);
      const float d = lerp2(wx0[j], r1[xa[j]], wx1[j], r1[xb[j]]);
      r[j] = lerp2(wy0, a, wy1, d);
    }
  };

  float* out = q.out + (long long)bc * q.Zh * plane + (long long)yh * q.Xh + x0;
  const float qnan = __builtin_nanf("");
  LineFill f[V];
#pragma unroll
  for (int j = 0; j < V; j++) f[j] = LineFill{0, -1, -1, 0.0f, 0.0f};
  int k0 = -1, k1 = -1;
  float qa[V], qb[V];
  for (int zh = 0; zh < q.Zh; zh++) {
    int z0, z1;
    float wz0, wz1;
    src_index(zh, q.inv, q.z, z0, z1, wz0, wz1);
    if (z0 != k0) {                                       // (uniform: every lane walks the same levels)
      if (z0 == k1) {
#pragma unroll
        for (int j = 0; j < V; j++) qa[j] = qb[j];
      } else {
        bracket(z0, qa);
      }
      k0 = z0;
    }
    if (z1 != k1) {
      if (z1 == k0) {
#pragma unroll
        for (int j = 0; j < V; j++) qb[j] = qa[j];
      } else {
        bracket(z1, qb);
      }
      k1 = z1;
    }
    const unsigned char* m = q.mask + (long long)(zh >> q.shift) * lplane;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float t3 = lerp2(wz0, qa[j], wz1, qb[j]);
      v[j] = m[moff[j]] != 0 ? qnan : t3;
    }
    float* row = out + (long long)zh * plane;
    if constexpr (V == 4) {
      *reinterpret_cast<f32x4*>(row) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) row[j] = v[j];
    }
#pragma unroll
    for (int j = 0; j < V; j++)
      if (!isnan(v[j])) fill_valid(f[j], out + j, plane, zh, v[j]);
  }
#pragma unroll
  for (int j = 0; j < V; j++)
    if (fill_finish(f[j], out + j, plane, q.Zh) > 0)
      q.xflag[(long long)bc * q.Xh + x0 + j] = 1;         // every writer stores the same word
}

__global__ __launch_bounds__(kThreads) void interp_fill_y_kernel(const InterpParams q) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long long)q.B * q.C * q.Zh * q.Xh) return;
  const int xh = (int)(t % q.Xh);
  const long long r = t / q.Xh;                           // bc * Zh + zh
  const int bc = (int)(r / q.Zh);
  if (!q.xflag[(long long)bc * q.Xh + xh]) return;
  float* line = q.out + r * q.Yh * q.Xh + xh;
  LineFill f{0, -1, -1, 0.0f, 0.0f};
  // kChunk independent loads in flight, then the state machine over them: fill_valid at cell k writes below k only,
  // i.e. cells of this or an earlier chunk, all read already
  for (int k0 = 0; k0 < q.Yh; k0 += kChunk) {
    float v[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; j++) v[j] = k0 + j < q.Yh ? line[(long long)(k0 + j) * q.Xh] : 0.0f;
#pragma unroll
    for (int j = 0; j < kChunk; j++)
      if (k0 + j < q.Yh && !isnan(v[j])) fill_valid(f, line, q.Xh, k0 + j, v[j]);
  }
  if (fill_finish(f, line, q.Xh, q.Yh) > 0) q.zflag[r] = 1;
}

__global__ __launch_bounds__(kThreads) void interp_fill_x_kernel(const InterpParams q) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long long)q.B * q.C * q.Zh * q.Yh) return;
  const long long r = t / q.Yh;                           // bc * Zh + zh
  if (!q.zflag[r]) return;
  float* line = q.out + t * q.Xh;                         // t = (bc * Zh + zh) * Yh + yh
  LineFill f{0, -1, -1, 0.0f, 0.0f};
  for (int k = 0; k < q.Xh; k++) {
    const float v = line[k];
    if (!isnan(v)) fill_valid(f, line, 1, k, v);
  }
  const int left = fill_finish(f, line, 1, q.Xh);
  if (left > 0) atomicAdd(q.count, left);
}

bool dims_ok(int B, int C, int z, int y, int x, int scale) {
  return B > 0 && C > 0 && z > 0 && y > 0 && x > 0 && (scale == 2 || scale == 4);
}

}  // namespace

extern "C" {

size_t sr3d_interp_baseline_workspace_bytes(int B, int C, int z, int y, int x, int scale) {
  if (!dims_ok(B, C, z, y, x, scale)) return 0;
  return (size_t)B * C * ((size_t)x * scale + (size_t)z * scale) * sizeof(int);
}

int sr3d_interp_baseline(const void* lr, long long batch_stride, long long channel_stride, int dtype, int B, int C,
                         int z, int y, int x, const void* lr_is_in_build, int mz, int my, int mx, int scale, void* out,
                         void* n_unfilled, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "interp_baseline";
  SR3D_CHECK(dtype == SR3D_DTYPE_F32, SR3D_E_ARG, "%s: element type %d: only fp32 (SR3D_DTYPE_F32) is implemented",
             what, dtype);
  SR3D_CHECK(scale == 2 || scale == 4, SR3D_E_ARG, "%s: scale %d: only 2 and 4 are implemented", what, scale);
  SR3D_CHECK(lr && lr_is_in_build && out && n_unfilled, SR3D_E_ARG,
             "%s: null lr, lr_is_in_build, out or n_unfilled pointer", what);
  SR3D_CHECK(B > 0 && C > 0 && z > 0 && y > 0 && x > 0, SR3D_E_ARG, "%s: non-positive dimension", what);
  SR3D_CHECK(mz == z && my == y && mx == x, SR3D_E_ARG, "%s: mask (%d, %d, %d) is not the LR grid (%d, %d, %d)", what,
             mz, my, mx, z, y, x);
  const long long vol = (long long)z * y * x;
  SR3D_CHECK((channel_stride >= vol || C == 1) && (batch_stride >= vol || B == 1), SR3D_E_ARG,
             "%s: batch stride %lld or channel stride %lld < z * y * x", what, batch_stride, channel_stride);
  SR3D_CHECK(((uintptr_t)lr & 3) == 0 && ((uintptr_t)out & 3) == 0, SR3D_E_ARG, "%s: lr and out must be 4-byte aligned",
             what);
  const long long cells = (long long)B * C * vol * scale * scale * scale;
  SR3D_CHECK(cells < (1ll << 31), SR3D_E_ARG, "%s: %lld output cells: the count of unfilled cells is an int32", what,
             cells);
  SR3D_CHECK(workspace, SR3D_E_ARG, "%s: null workspace", what);
  SR3D_CHECK(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)n_unfilled & 3) == 0, SR3D_E_ARG,
             "%s: workspace and n_unfilled must be 4-byte aligned", what);
  const size_t need = sr3d_interp_baseline_workspace_bytes(B, C, z, y, x, scale);
  SR3D_CHECK(workspace_bytes >= need, SR3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
             need);

  InterpParams q{};
  q.lr = (const float*)lr, q.bstride = batch_stride, q.cstride = channel_stride;
  q.mask = (const unsigned char*)lr_is_in_build;
  q.out = (float*)out;
  q.B = B, q.C = C, q.z = z, q.y = y, q.x = x;
  q.shift = scale == 4 ? 2 : 1;
  q.Zh = z * scale, q.Yh = y * scale, q.Xh = x * scale;
  q.inv = 1.0f / (float)scale;
  q.xflag = (int*)workspace;
  q.zflag = q.xflag + (size_t)B * C * q.Xh;
  q.count = (int*)n_unfilled;

  hipStream_t st = (hipStream_t)stream;
  int rc = sr3d_zero_words(workspace, (int)(need / sizeof(int)), st);
  if (rc) return rc;
  rc = sr3d_zero_words(q.count, 1, st);
  if (rc) return rc;
  const long long bc = (long long)B * C;
  auto blocks = [](long long lanes) { return dim3((unsigned)((lanes + kThreads - 1) / kThreads)); };
  const bool vec = q.Xh % 4 == 0 && ((uintptr_t)out & 15) == 0;   // every row of every level then starts 16-byte aligned
  if (vec)
    hipLaunchKernelGGL(interp_column_kernel<4>, blocks(bc * q.Yh * (q.Xh / 4)), dim3(kThreads), 0, st, q);
  else
    hipLaunchKernelGGL(interp_column_kernel<1>, blocks(bc * q.Yh * q.Xh), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(interp_fill_y_kernel, blocks(bc * q.Zh * q.Xh), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(interp_fill_x_kernel, blocks(bc * q.Zh * q.Yh), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
