// Cubic-spline rotation of every (y, x) plane about the vertical axis, and the fused equivariance error (gfx950).
//
// GPU form of the reference's analysis module src/equivariance_error_calculator.py, which rotates the LR input, the
// building mask and the prediction with scipy.ndimage.rotate(a, angle, axes=(-2, -1), reshape=False) -- defaults
// order = 3, mode = 'constant', cval = 0, prefilter = True -- one 2-D plane at a time in float64 on the host.
//
//   prefilter  cubic B-spline direct filter along y, then along x (pole z = sqrt(3) - 2, gain 6), mirror boundary
//              (what spline_filter(..., mode='constant') does), in fp64.  The causal / anticausal recurrence pair is
//              replaced by its symmetric FIR h[k] = -6z / (1 - z^2) * z^|k|, |k| <= 27 (|z|^28 < 1e-16), over the
//              whole-sample-symmetric extension a[-i] = a[i], period 2(n - 1): a coalesced, LDS-tiled pass.
//   geometry   c, s = cosdg(angle), sindg(angle) (host side, exact at multiples of 90 degrees); M = [[c, s], [-s, c]],
//              offset = in_center - M @ out_center, center = (shape - 1) / 2.  Source (cy, cx) = M @ (oy, ox) + offset.
//   gather     a source coordinate strictly outside [0, n - 1] on either axis gives cval = 0 exactly; inside (edges
//              included) the value is the 4 x 4 B-spline sum over the mirror-extended coefficients.  Coordinates and
//              the 16 weights are computed once per output (y, x) and reused over every channel and z plane.
//
// The spline is linear and reproduces constants under the mirror boundary, so rotating the physical field x * s + m
// equals s * rotate(x) + m * inside: the kernels prefilter the NORMALISED field and dimensionalise in the epilogue,
// where the 2 x 2 velocity mix and the re-normalisation + clip happen too.  The fused error kernel never writes the
// rotated prediction: it gathers only the window and reduces |dT|, |dw| and ||(du, dv)|| deterministically in fp64
// (block partials in a fixed order, then one final block).
#include <math.h>

#include "sr3d_common.h"

namespace {

constexpr int kR = 27;                           // FIR half-length
constexpr int PF_TX = 64, PF_TY = 32;            // prefilter output tile
constexpr int kPfThreads = 256;
constexpr int G_T = 16;                          // gather output tile: 16 x 16 (y, x)
constexpr int G_ZCH = 4;                         // z planes per gather workgroup
constexpr int kGThreads = G_T * G_T;
constexpr int kMaxGridY = 65535;

struct PrefilterParams {
  const void* in;
  double* out;
  long long planes;
  int Y, X;
  double h[kR + 1];
};

// geometry of one rotation: source (cy, cx) = (m00 * oy + m01 * ox + off_y, m10 * oy + m11 * ox + off_x)
struct Geom {
  double m00, m01, m10, m11, off_y, off_x;
};

enum { MODE_FIELDS = 0, MODE_BUILDING = 1 };

struct GatherParams {
  const double* coef;   // [B][C][Z][Y][X] spline coefficients
  float* out;           // [B][C][Z][Y][X]
  int B, C, Z, Y, X;
  Geom g;
  double m[4], s[4];    // field mode: means, scales
  double cs, sn;        // field mode: velocity mix (channels 1, 2)
  int physical;         // field mode: SR3D_ROTATE_PHYSICAL (no re-normalisation / clip)
  float th;             // building mode: threshold (fp32, as numpy compares a float32 array with a python float)
};

struct ErrParams {
  const double* coef;   // [B][4][Z][Y][X] coefficients of preds
  const float* par;     // preds_after_rot
  int B, Z, Y, X;
  int sy, sx, wy, wx;   // window origin and extent
  Geom g;
  double m[4], s[4], cs, sn;
  double* part;         // [blocks][3]
  double* out;          // 3 means
};

__device__ __forceinline__ int mirror_idx(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = i < 0 ? -i : i;
  i %= p;
  return i > n - 1 ? p - i : i;
}

// ---- prefilter: one axis of the separable FIR, LDS-tiled (along y: 86 x 64 doubles = 44 KB; along x: 32 x 118 = 30 KB)
template <typename Tin, bool ALONG_X>
__global__ __launch_bounds__(kPfThreads) void rotate_prefilter_kernel(const PrefilterParams q) {
#pragma clang fp contract(off)
  constexpr int LY = ALONG_X ? PF_TY : PF_TY + 2 * kR;
  constexpr int LX = ALONG_X ? PF_TX + 2 * kR : PF_TX;
  __shared__ double s[LY][LX];
  const int Y = q.Y, X = q.X;
  const int ntx = (X + PF_TX - 1) / PF_TX;
  const int x0 = (int)(blockIdx.x % ntx) * PF_TX, y0 = (int)(blockIdx.x / ntx) * PF_TY;
  const int n = ALONG_X ? X : Y;
  const int tx = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const long long plane = (long long)Y * X;
  for (long long pl = blockIdx.y; pl < q.planes; pl += gridDim.y) {
    const Tin* src = (const Tin*)q.in + pl * plane;
    __syncthreads();   // the previous plane's LDS reads are done
    for (int e = threadIdx.x; e < LY * LX; e += kPfThreads) {
      const int ly = e / LX, lx = e - ly * LX;
      int gy, gx;
      if (ALONG_X) {
        gy = min(y0 + ly, Y - 1), gx = mirror_idx(x0 - kR + lx, X);
      } else {
        gy = mirror_idx(y0 - kR + ly, Y), gx = min(x0 + lx, X - 1);
      }
      s[ly][lx] = (double)src[(long long)gy * X + gx];
    }
    __syncthreads();
    double* dst = q.out + pl * plane;
#pragma unroll 2
    for (int k = 0; k < PF_TY / 4; k++) {
      const int r = tr + 4 * k, oy = y0 + r, ox = x0 + tx;
      if (oy >= Y || ox >= X) continue;
      double v;
      if (ALONG_X) {
        const double* a = &s[r][tx + kR];
        if (n == 1) {
          v = a[0];
        } else {
          v = q.h[0] * a[0];
#pragma unroll
          for (int j = 1; j <= kR; j++) v += q.h[j] * (a[-j] + a[j]);
        }
      } else {
        const int c = r + kR;
        if (n == 1) {
          v = s[c][tx];
        } else {
          v = q.h[0] * s[c][tx];
#pragma unroll
          for (int j = 1; j <= kR; j++) v += q.h[j] * (s[c - j][tx] + s[c + j][tx]);
        }
      }
      dst[(long long)oy * X + ox] = v;
    }
  }
}

// ---- taps of one output (oy, ox): mirror-mapped indices and B-spline weights; false if the source is outside
struct Taps {
  int iy[4], ix[4];
  double wy[4], wx[4];
};

__device__ __forceinline__ void spline_weights(double c, int n, int* idx, double* w) {
#pragma clang fp contract(off)
  const double f = floor(c);
  const double t = c - f, u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
  w[3] = t * t * t / 6.0;
  const int s0 = (int)f - 1;
#pragma unroll
  for (int k = 0; k < 4; k++) idx[k] = mirror_idx(s0 + k, n);
}

__device__ __forceinline__ bool make_taps(const Geom& g, int oy, int ox, int Y, int X, Taps& t) {
#pragma clang fp contract(off)
  // scipy's order: the matrix row times the output coordinates, then the offset (decides points on a plane edge)
  const double cy = (g.m00 * (double)oy + g.m01 * (double)ox) + g.off_y;
  const double cx = (g.m10 * (double)oy + g.m11 * (double)ox) + g.off_x;
  if (!(cy >= 0.0 && cy <= (double)(Y - 1) && cx >= 0.0 && cx <= (double)(X - 1))) return false;
  spline_weights(cy, Y, t.iy, t.wy);
  spline_weights(cx, X, t.ix, t.wx);
  return true;
}

__device__ __forceinline__ double interp(const double* P, int X, const Taps& t) {
#pragma clang fp contract(off)
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double* row = P + (long long)t.iy[i] * X;
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) r += t.wx[j] * row[t.ix[j]];
    v += t.wy[i] * r;
  }
  return v;
}

// the four channels of one rotated field voxel: dimensionalise (cval 0 is physical 0), mix channels 1 and 2 as a vector
__device__ __forceinline__ void field_epilogue(const double* r, bool inside, const double* m, const double* s, double cs,
                                               double sn, double* v) {
#pragma clang fp contract(off)
  double p[4];
#pragma unroll
  for (int c = 0; c < 4; c++) p[c] = inside ? s[c] * r[c] + m[c] : 0.0;
  v[0] = p[0];
  v[1] = cs * p[1] + sn * p[2];
  v[2] = -sn * p[1] + cs * p[2];
  v[3] = p[3];
}

__device__ __forceinline__ double renorm_clip(double v, double m, double s) {
  const double r = (v - m) / s;
  return fmin(fmax(r, 0.0), 1.0);
}

// ---- gather: one 16 x 16 (y, x) tile, G_ZCH planes, every channel
template <int MODE>
__global__ __launch_bounds__(kGThreads) void rotate_gather_kernel(const GatherParams q) {
#pragma clang fp contract(off)
  const int ntx = (q.X + G_T - 1) / G_T;
  const int oy = (int)(blockIdx.x / ntx) * G_T + (int)(threadIdx.x / G_T);
  const int ox = (int)(blockIdx.x % ntx) * G_T + (int)(threadIdx.x % G_T);
  if (oy >= q.Y || ox >= q.X) return;   // no barrier in this kernel
  const int z0 = blockIdx.y * G_ZCH, z1 = min(z0 + G_ZCH, q.Z);
  const long long plane = (long long)q.Y * q.X, zyx = (long long)q.Z * plane;
  Taps t;
  const bool inside = make_taps(q.g, oy, ox, q.Y, q.X, t);
  const long long pix = (long long)oy * q.X + ox;
  for (int b = blockIdx.z; b < q.B; b += gridDim.z) {
    for (int z = z0; z < z1; z++) {
      if (MODE == MODE_FIELDS) {
        const long long base = (long long)b * 4 * zyx + (long long)z * plane;
        double r[4], v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) r[c] = inside ? interp(q.coef + base + c * zyx, q.X, t) : 0.0;
        field_epilogue(r, inside, q.m, q.s, q.cs, q.sn, v);
#pragma unroll
        for (int c = 0; c < 4; c++)
          q.out[base + c * zyx + pix] = (float)(q.physical ? v[c] : renorm_clip(v[c], q.m[c], q.s[c]));
      } else {
        for (int c = 0; c < q.C; c++) {
          const long long base = ((long long)b * q.C + c) * zyx + (long long)z * plane;
          const float v = inside ? (float)interp(q.coef + base, q.X, t) : 0.f;   // scipy's float32 output
          q.out[base + pix] = v > q.th ? 1.f : 0.f;
        }
      }
    }
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- fused error: rotate preds (clip included) inside the window, compare with preds_after_rot, 3 block partials
__global__ __launch_bounds__(kGThreads) void equivar_err_kernel(const ErrParams q) {
#pragma clang fp contract(off)
  const int ntx = (q.wx + G_T - 1) / G_T;
  const int ly = (int)(blockIdx.x / ntx) * G_T + (int)(threadIdx.x / G_T);
  const int lx = (int)(blockIdx.x % ntx) * G_T + (int)(threadIdx.x % G_T);
  const bool live = ly < q.wy && lx < q.wx;
  const int oy = q.sy + ly, ox = q.sx + lx;
  const int z0 = blockIdx.y * G_ZCH, z1 = min(z0 + G_ZCH, q.Z);
  const int b = blockIdx.z;
  const long long plane = (long long)q.Y * q.X, zyx = (long long)q.Z * plane;
  double acc[3] = {0.0, 0.0, 0.0};
  if (live) {
    Taps t;
    const bool inside = make_taps(q.g, oy, ox, q.Y, q.X, t);
    const long long pix = (long long)oy * q.X + ox;
    for (int z = z0; z < z1; z++) {
      const long long base = (long long)b * 4 * zyx + (long long)z * plane;
      double r[4], v[4], d[4];
#pragma unroll
      for (int c = 0; c < 4; c++) r[c] = inside ? interp(q.coef + base + c * zyx, q.X, t) : 0.0;
      field_epilogue(r, inside, q.m, q.s, q.cs, q.sn, v);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        // the reference: (scales * rotated + means) - (scales * preds_after_rot + means), in float64
        const double rot = q.s[c] * renorm_clip(v[c], q.m[c], q.s[c]) + q.m[c];
        const double aft = q.s[c] * (double)q.par[base + c * zyx + pix] + q.m[c];
        d[c] = rot - aft;
      }
      acc[0] += fabs(d[0]);
      acc[1] += fabs(d[3]);
      acc[2] += sqrt(d[1] * d[1] + d[2] * d[2]);
    }
  }
  __shared__ double sm[kGThreads / 64][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double v = wave_sum_d(acc[k]);
    if (lane == 0) sm[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int i = 0; i < kGThreads / 64; i++) v += sm[i][threadIdx.x];
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    q.part[blk * 3 + threadIdx.x] = v;
  }
}

constexpr int kFinThreads = 256;

__global__ __launch_bounds__(kFinThreads) void equivar_err_final_kernel(const ErrParams q, long long nblk, double count) {
  __shared__ double red[kFinThreads];
  for (int k = 0; k < 3; k++) {
    double v = 0.0;
    for (long long b = threadIdx.x; b < nblk; b += kFinThreads) v += q.part[b * 3 + k];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kFinThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) q.out[k] = red[0] / count;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- host side
long long err_blocks(int B, int Z, int wy, int wx) {
  return (long long)((wy + G_T - 1) / G_T) * ((wx + G_T - 1) / G_T) * ((Z + G_ZCH - 1) / G_ZCH) * B;
}

// cosdg / sindg (scipy.special): the angle reduced modulo 360, exact values at multiples of 90 degrees
void cos_sin_deg(double angle, double* c, double* s) {
  double a = fmod(angle, 360.0);
  if (a < 0.0) a += 360.0;
  if (a == 0.0) {
    *c = 1.0, *s = 0.0;
  } else if (a == 90.0) {
    *c = 0.0, *s = 1.0;
  } else if (a == 180.0) {
    *c = -1.0, *s = 0.0;
  } else if (a == 270.0) {
    *c = 0.0, *s = -1.0;
  } else {
    const double r = a * (M_PI / 180.0);
    *c = cos(r), *s = sin(r);
  }
}

Geom make_geom(double c, double s, int Y, int X) {
  // scipy.ndimage.rotate: rot_matrix = [[c, s], [-s, c]], offset = in_center - rot_matrix @ out_center
  const double hy = (Y - 1) / 2.0, hx = (X - 1) / 2.0;
  Geom g;
  g.m00 = c, g.m01 = s, g.m10 = -s, g.m11 = c;
  g.off_y = hy - (c * hy + s * hx);
  g.off_x = hx - (-s * hy + c * hx);
  return g;
}

size_t coef_bytes(long long n) { return (size_t)n * sizeof(double); }

// both FIR passes: x (fp32) -> tmp (fp64, along y) -> coef (fp64, along x)
int prefilter(const float* x, long long planes, int Y, int X, double* coef, double* tmp, hipStream_t st) {
  PrefilterParams q{};
  q.planes = planes, q.Y = Y, q.X = X;
  const double z = sqrt(3.0) - 2.0;
  double h = -6.0 * z / (1.0 - z * z);
  for (int k = 0; k <= kR; k++) q.h[k] = h, h *= z;
  const int tiles = ((X + PF_TX - 1) / PF_TX) * ((Y + PF_TY - 1) / PF_TY);
  const dim3 grid(tiles, (unsigned)(planes < kMaxGridY ? planes : kMaxGridY));
  q.in = x, q.out = tmp;
  hipLaunchKernelGGL((rotate_prefilter_kernel<float, false>), grid, dim3(kPfThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  q.in = tmp, q.out = coef;
  hipLaunchKernelGGL((rotate_prefilter_kernel<double, true>), grid, dim3(kPfThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

// Python-slice bounds [s, e) on an axis of n: negatives count from the end; a window must be non-empty and inside
bool window(int s, int e, int n, int* s0, int* len) {
  if (s < 0) s += n;
  if (e < 0) e += n;
  if (s < 0 || e > n || s >= e) return false;
  *s0 = s, *len = e - s;
  return true;
}

int check_common(const void* a, const void* out, int B, int C, int Z, int Y, int X, int flags, const void* ws,
                 size_t ws_bytes, const char* what) {
  SR3D_CHECK(a && out, SR3D_E_ARG, "%s: null tensor pointer", what);
  SR3D_CHECK(ws, SR3D_E_ARG, "%s: null workspace", what);
  SR3D_CHECK(B > 0 && C > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "%s: non-positive dimension", what);
  SR3D_CHECK((long long)Y * X < (1ll << 31), SR3D_E_ARG, "%s: a (y, x) plane has >= 2^31 voxels", what);
  SR3D_CHECK(B <= kMaxGridY && (Z + G_ZCH - 1) / G_ZCH <= kMaxGridY, SR3D_E_ARG, "%s: batch or depth too large", what);
  SR3D_CHECK((flags & ~(SR3D_ROTATE_COEF_READY | SR3D_ROTATE_PHYSICAL)) == 0, SR3D_E_ARG, "%s: unknown flags 0x%x",
             what, flags);
  SR3D_CHECK(ws_bytes >= sr3d_rotate_workspace_bytes(B, C, Z, Y, X), SR3D_E_WORKSPACE,
             "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, sr3d_rotate_workspace_bytes(B, C, Z, Y, X));
  return SR3D_OK;
}

int check_scales(const double* means, const double* scales, const char* what) {
  SR3D_CHECK(means && scales, SR3D_E_ARG, "%s: null means / scales", what);
  for (int c = 0; c < 4; c++)
    SR3D_CHECK(scales[c] != 0.0 && isfinite(scales[c]) && isfinite(means[c]), SR3D_E_ARG,
               "%s: channel %d: scale must be finite and non-zero, mean finite", what, c);
  return SR3D_OK;
}

}  // namespace

extern "C" {

size_t sr3d_rotate_workspace_bytes(int B, int C, int Z, int Y, int X) {
  if (B <= 0 || C <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  const long long n = (long long)B * C * Z * Y * X;
  return 2 * coef_bytes(n) + (size_t)err_blocks(B, Z, Y, X) * 3 * sizeof(double);
}

int sr3d_rotate_fields(const void* x, void* y, int B, int C, int Z, int Y, int X, const double means[4],
                       const double scales[4], double angle_deg, int flags, void* workspace, size_t workspace_bytes,
                       void* stream) {
  int rc = check_common(x, y, B, C, Z, Y, X, flags, workspace, workspace_bytes, "rotate_fields");
  if (rc) return rc;
  SR3D_CHECK(C == 4, SR3D_E_ARG, "rotate_fields: the field has 4 channels (T, u, v, w), got %d", C);
  SR3D_CHECK(isfinite(angle_deg), SR3D_E_ARG, "rotate_fields: angle is not finite");
  if ((rc = check_scales(means, scales, "rotate_fields"))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * C * Z * Y * X;
  double* coef = (double*)workspace;
  if (!(flags & SR3D_ROTATE_COEF_READY))
    if ((rc = prefilter((const float*)x, (long long)B * C * Z, Y, X, coef, coef + n, st))) return rc;
  GatherParams q{};
  q.coef = coef, q.out = (float*)y;
  q.B = B, q.C = C, q.Z = Z, q.Y = Y, q.X = X;
  double c, s;
  cos_sin_deg(angle_deg, &c, &s);
  q.g = make_geom(c, s, Y, X);
  for (int i = 0; i < 4; i++) q.m[i] = means[i], q.s[i] = scales[i];
  // the reference's channel matrix uses np.cos / np.sin(np.deg2rad(angle)); cosdg / sindg differ from those by ~1e-16
  // (and are exact at multiples of 90 degrees), far below the fp32 output's resolution
  q.cs = c, q.sn = s;
  q.physical = (flags & SR3D_ROTATE_PHYSICAL) ? 1 : 0;
  const dim3 grid(((X + G_T - 1) / G_T) * ((Y + G_T - 1) / G_T), (Z + G_ZCH - 1) / G_ZCH, B);
  hipLaunchKernelGGL(rotate_gather_kernel<MODE_FIELDS>, grid, dim3(kGThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

int sr3d_rotate_building(const void* b, void* y, int B, int C, int Z, int Y, int X, double angle_deg, double th,
                         int flags, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_common(b, y, B, C, Z, Y, X, flags, workspace, workspace_bytes, "rotate_building");
  if (rc) return rc;
  SR3D_CHECK(!(flags & SR3D_ROTATE_PHYSICAL), SR3D_E_ARG, "rotate_building: SR3D_ROTATE_PHYSICAL is a field flag");
  SR3D_CHECK(isfinite(angle_deg) && isfinite(th), SR3D_E_ARG, "rotate_building: angle / threshold not finite");
  const hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * C * Z * Y * X;
  double* coef = (double*)workspace;
  if (!(flags & SR3D_ROTATE_COEF_READY))
    if ((rc = prefilter((const float*)b, (long long)B * C * Z, Y, X, coef, coef + n, st))) return rc;
  GatherParams q{};
  q.coef = coef, q.out = (float*)y;
  q.B = B, q.C = C, q.Z = Z, q.Y = Y, q.X = X;
  double c, s;
  cos_sin_deg(angle_deg, &c, &s);
  q.g = make_geom(c, s, Y, X);
  q.th = (float)th;
  const dim3 grid(((X + G_T - 1) / G_T) * ((Y + G_T - 1) / G_T), (Z + G_ZCH - 1) / G_ZCH, B);
  hipLaunchKernelGGL(rotate_gather_kernel<MODE_BUILDING>, grid, dim3(kGThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

int sr3d_equivariance_errors(const void* preds, const void* preds_after_rot, int B, int Z, int Y, int X,
                             const double means[4], const double scales[4], double angle_deg, int sy, int ey, int sx,
                             int ex, int flags, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_common(preds, out, B, 4, Z, Y, X, flags, workspace, workspace_bytes, "equivariance_errors");
  if (rc) return rc;
  SR3D_CHECK(preds_after_rot, SR3D_E_ARG, "equivariance_errors: null preds_after_rot");
  SR3D_CHECK(!(flags & SR3D_ROTATE_PHYSICAL), SR3D_E_ARG, "equivariance_errors: SR3D_ROTATE_PHYSICAL is a field flag");
  SR3D_CHECK(isfinite(angle_deg), SR3D_E_ARG, "equivariance_errors: angle is not finite");
  if ((rc = check_scales(means, scales, "equivariance_errors"))) return rc;
  ErrParams q{};
  SR3D_CHECK(window(sy, ey, Y, &q.sy, &q.wy) && window(sx, ex, X, &q.sx, &q.wx), SR3D_E_ARG,
             "equivariance_errors: window [%d:%d, %d:%d] is empty or outside the (%d, %d) plane", sy, ey, sx, ex, Y, X);
  const hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * 4 * Z * Y * X;
  double* coef = (double*)workspace;
  if (!(flags & SR3D_ROTATE_COEF_READY))
    if ((rc = prefilter((const float*)preds, (long long)B * 4 * Z, Y, X, coef, coef + n, st))) return rc;
  q.coef = coef, q.par = (const float*)preds_after_rot;
  q.B = B, q.Z = Z, q.Y = Y, q.X = X;
  double c, s;
  cos_sin_deg(angle_deg, &c, &s);
  q.g = make_geom(c, s, Y, X);
  for (int i = 0; i < 4; i++) q.m[i] = means[i], q.s[i] = scales[i];
  q.cs = c, q.sn = s;
  q.part = coef + 2 * n, q.out = (double*)out;
  const long long nblk = err_blocks(B, Z, q.wy, q.wx);
  const dim3 grid(((q.wx + G_T - 1) / G_T) * ((q.wy + G_T - 1) / G_T), (Z + G_ZCH - 1) / G_ZCH, B);
  hipLaunchKernelGGL(equivar_err_kernel, grid, dim3(kGThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  const double count = (double)B * Z * q.wy * q.wx;
  hipLaunchKernelGGL(equivar_err_final_kernel, dim3(1), dim3(kFinThreads), 0, st, q, nblk, count);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
