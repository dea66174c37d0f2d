// LR training data from an HR field, building-aware (gfx950): the per-time-step part of the reference's
// make_dl_data_using_outside_lr_builds script (training_data_maker.make_coarse_grained_dataarray_with_outside_lr_
// buildings, scale 4) without a filled copy of the volume.
//
// Per channel of the raw (C, Z, Y, X) fp32 volume, a cell is VALID when the HR mask (Z, Y, X) is clear there, the
// value is not NaN and (align_nan, channels > 0) channel 0 is not NaN there.  The reference fills invalid cells with
// xarray's interpolate_na(method="nearest", fill_value="extrapolate") along lev, then lat, then lon.  On one line that
// is scipy's interp1d(kind="nearest"): with lo / hi the nearest valid positions below / above, the cell takes lo when
// its coordinate is <= lo / 2 + hi / 2 (fp64), hi otherwise; past either end it takes the edge value; a line without
// any valid cell stays NaN.  After the lev fill a cell is NaN only if its whole column is, so the lat and lon fills
// only pick a SOURCE COLUMN per (c, y, x):
//   live column (any valid cell)           itself
//   dead, but x has a live column          the nearest live y at that x (lat coordinates)
//   dead, and every column at x is dead    the nearest x with a live column (lon coordinates), then at that x the
//                                          column y if live, else the nearest live y
//   no live column in the channel          NaN
// The source column is filled along lev (lev coordinates); cells z < tops[0] of the block's LR column (the resized
// LR buildings at HR levels) then become NaN, and every 4x4x4 block is summed in fp64 in numpy's pairwise order for 64
// contiguous elements (eight strided accumulators, then a fixed tree) and scaled by 1/64, which is exact.  A NaN
// cell makes the block NaN: this is the reference's sum(window * w), where NaN * 0 = NaN, so the pooling weights never
// matter.  LR levels kz < tops[1] (the LR buildings at LR levels) are NaN.  The masked HR volume is written as well;
// both outputs cover only the window that lies hr_margin cells inside the lateral edges.
//
// Two passes, stream-ordered, no host synchronisation:
//   lrdata_dead_kernel   one lane per (c, y, x) of the full domain: dead[c][y][x], and xlive[c][x] = 1 for every x
//                        that has a live column.  It scans from the top level down and stops at the first valid
//                        cell, so it reads about one plane per channel.
//   lrdata_main_kernel   one lane per (c, y, x) of the window; a wavefront is 4 rows x 16 columns of one channel, so
//                        it holds four whole blocks.  Lanes walk up their (source) column with two scalar states
//                        (last valid level, next valid level): every cell is read once, twice at most inside a gap.
//                        The block sums are cross-lane (rows 2, 3 hand their values to rows 0, 1; then xor 1, 2, 16).
#include <math.h>

#include "sr3d_common.h"

namespace {

constexpr int kS = 4;                 // the reference asserts SR_SCALE == 4
constexpr int kThreads = 256;         // four wavefronts: 4 rows x 64 columns of one channel
constexpr int kTileX = 64;
constexpr int kMaxLevels = 128;
constexpr int kMaxGridY = 65535;

struct LrParams {
  const float* raw;
  long long cstride;                  // elements between channels
  const unsigned char* mask;          // (Z, Y, X)
  const int* tops;                    // (2, Y/4, X/4)
  const double* lat;                  // (Y) or null: index coordinates
  const double* lon;                  // (X) or null
  float* hr;                          // (C, Z, Yc, Xc)
  float* lr;                          // (C, Z/4, Yc/4, Xc/4)
  unsigned char* dead;                // (C, Y, X)
  int* xlive;                         // (C, X)
  int C, Z, Y, X, m, Yc, Xc, tiles_x, align;
  int has_lev;
  double lev[kMaxLevels];
};

__device__ __forceinline__ bool valid_cell(const LrParams& q, int c, long long cell, float v) {
  if (q.mask[cell] != 0 || isnan(v)) return false;
  if (q.align && c > 0 && isnan(q.raw[cell])) return false;   // channel 0 (tm) is NaN there
  return true;
}

__global__ __launch_bounds__(kThreads) void lrdata_dead_kernel(const LrParams q) {
  const long long plane = (long long)q.Y * q.X;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= plane * q.C) return;
  const int c = (int)(i / plane);
  const long long col = i - (long long)c * plane;
  const float* src = q.raw + (long long)c * q.cstride;
  bool live = false;
  for (int z = q.Z - 1; z >= 0 && !live; z--) {
    const long long cell = (long long)z * plane + col;
    live = valid_cell(q, c, cell, src[cell]);
  }
  q.dead[i] = live ? 0 : 1;
  if (live) q.xlive[(long long)c * q.X + (int)(col % q.X)] = 1;   // every writer stores the same word
}

__device__ __forceinline__ double coord(const double* v, int k) { return v ? v[k] : (double)k; }

// scipy interp1d(kind="nearest") between the valid neighbours lo < k < hi (either may be missing: -1 / n):
// k takes lo when coord(k) <= coord(lo) / 2 + coord(hi) / 2, ties to the lower coordinate
__device__ __forceinline__ bool take_lo(double ck, double clo, double chi) {
#pragma clang fp contract(off)
  const double mid = clo * 0.5 + chi * 0.5;
  return ck <= mid;
}

// the nearest live y at column x of channel c (-1 if none)
__device__ int nearest_live_y(const LrParams& q, const unsigned char* dead, int y, int x) {
  if (!dead[(long long)y * q.X + x]) return y;
  int lo = y - 1, hi = y + 1;
  while (lo >= 0 && dead[(long long)lo * q.X + x]) lo--;
  while (hi < q.Y && dead[(long long)hi * q.X + x]) hi++;
  if (lo < 0) return hi < q.Y ? hi : -1;
  if (hi >= q.Y) return lo;
  return take_lo(coord(q.lat, y), coord(q.lat, lo), coord(q.lat, hi)) ? lo : hi;
}

// the nearest x with a live column in channel c (-1 if none)
__device__ int nearest_live_x(const LrParams& q, const int* xlive, int x) {
  int lo = x - 1, hi = x + 1;
  while (lo >= 0 && !xlive[lo]) lo--;
  while (hi < q.X && !xlive[hi]) hi++;
  if (lo < 0) return hi < q.X ? hi : -1;
  if (hi >= q.X) return lo;
  return take_lo(coord(q.lon, x), coord(q.lon, lo), coord(q.lon, hi)) ? lo : hi;
}

__global__ __launch_bounds__(kThreads) void lrdata_main_kernel(const LrParams q) {
#pragma clang fp contract(off)
  __shared__ double lev[kMaxLevels];
  for (int k = threadIdx.x; k < q.Z; k += kThreads) lev[k] = q.has_lev ? q.lev[k] : (double)k;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane >> 4;                              // dy inside the block row
  const int c = blockIdx.x % q.C, tx = blockIdx.x / q.C;
  const int ky = blockIdx.y;                              // LR row inside the window
  const int yc = ky * kS + row;
  const int xc = tx * kTileX + wave * 16 + (lane & 15);
  const bool inside = xc < q.Xc;                          // whole blocks: Xc is a multiple of 4
  const int y = yc + q.m, x = xc + q.m;
  const long long plane = (long long)q.Y * q.X;
  const float* src = q.raw + (long long)c * q.cstride;

  // ---- source column
  int sy = -1, sx = -1;
  bool own = false;
  int kh = 0, kl = 0;
  if (inside) {
    const unsigned char* dead = q.dead + (long long)c * plane;
    const int* xlive = q.xlive + (long long)c * q.X;
    if (!dead[(long long)y * q.X + x]) {
      sy = y, sx = x, own = true;
    } else if (xlive[x]) {
      sy = nearest_live_y(q, dead, y, x), sx = x;
    } else {
      sx = nearest_live_x(q, xlive, x);
      if (sx >= 0) sy = nearest_live_y(q, dead, y, sx);
      if (sy < 0) sx = -1;
    }
    const long long t = (long long)(y / kS) * (q.X / kS) + x / kS;
    kh = q.tops[t];
    kl = q.tops[(long long)(q.Y / kS) * (q.X / kS) + t];
  }
  const long long scol = sy >= 0 ? (long long)sy * q.X + sx : 0;
  const long long plane_c = (long long)q.Yc * q.Xc;
  float* hr = q.hr + (long long)c * q.Z * plane_c + (long long)yc * q.Xc + xc;
  const float qnan = __builtin_nanf("");

  // ---- walk up the column: p / vp the last valid level, n / vn the next one (n == Z: none above)
  int p = -1, n = -1;
  float vp = qnan, vn = qnan;
  const int LZ = q.Z / kS;
  const int Xl = q.Xc / kS;
  for (int kz = 0; kz < LZ; kz++) {
    float v[kS];
    bool ok[kS];
#pragma unroll
    for (int d = 0; d < kS; d++) {                        // the block's four loads first: they are independent
      v[d] = qnan, ok[d] = false;
      if (sy >= 0) {
        const long long cell = (long long)(kz * kS + d) * plane + scol;
        v[d] = src[cell];
        ok[d] = valid_cell(q, c, cell, v[d]);
      }
    }
    float f[kS];
#pragma unroll
    for (int d = 0; d < kS; d++) {
      const int z = kz * kS + d;
      if (inside) hr[(long long)z * plane_c] = (own && ok[d]) ? v[d] : qnan;
      float fz = qnan;
      if (ok[d]) {
        p = z, vp = v[d], fz = v[d];
      } else if (sy >= 0) {
        if (n <= z) {                                     // find the next valid level above z
          n = z + 1;
          for (; n < q.Z; n++) {
            const long long cell = (long long)n * plane + scol;
            const float w = src[cell];
            if (valid_cell(q, c, cell, w)) {
              vn = w;
              break;
            }
          }
        }
        if (p < 0) fz = vn;                               // extrapolate below the first valid level
        else if (n >= q.Z) fz = vp;                       // ... and above the last one
        else fz = take_lo(lev[z], lev[p], lev[n]) ? vp : vn;
      }
      if (z < kh) fz = qnan;                              // resized LR buildings, after the fill
      f[d] = fz;
    }
    // ---- the block sum: numpy's pairwise order over e = dz*16 + dy*4 + dx, i.e. accumulator j = (dy & 1)*4 + dx
    // adds i = dz*2 + (dy >> 1) for i = 0..7, then ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)).  Every term of the
    // reference is x * (1/64); scaling by a power of two commutes with each rounding, so it is applied once at the end.
    float g[kS];
#pragma unroll
    for (int d = 0; d < kS; d++) g[d] = __shfl_xor(f[d], 32, 64);   // rows 2, 3 -> rows 0, 1
    double r = (double)f[0];
    r = r + (double)g[0];
#pragma unroll
    for (int d = 1; d < kS; d++) {
      r = r + (double)f[d];
      r = r + (double)g[d];
    }
    r = r + __shfl_xor(r, 1, 64);
    r = r + __shfl_xor(r, 2, 64);
    r = r + __shfl_xor(r, 16, 64);
    if (inside && row == 0 && (xc & (kS - 1)) == 0) {
      const float o = kz < kl ? qnan : (float)(r * 0.015625);
      q.lr[(((long long)c * LZ + kz) * (q.Yc / kS) + ky) * Xl + xc / kS] = o;
    }
  }
}

}  // namespace

extern "C" {

size_t sr3d_lrdata_workspace_bytes(int C, int Y, int X) {
  if (C <= 0 || Y <= 0 || X <= 0) return 0;
  const size_t dead = ((size_t)C * Y * X + 15) & ~(size_t)15;
  return dead + (size_t)C * X * sizeof(int);
}

int sr3d_lrdata(const sr3d_lrdata_params_t* p, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "lrdata";
  SR3D_CHECK(p, SR3D_E_ARG, "%s: null parameters", what);
  SR3D_CHECK(p->scale == kS, SR3D_E_ARG, "%s: scale %d: only %d is implemented (the reference asserts it)", what,
             p->scale, kS);
  SR3D_CHECK(p->raw && p->hr_mask && p->lr_tops && p->hr_out && p->lr_out, SR3D_E_ARG,
             "%s: null raw, hr_mask, lr_tops or output pointer", what);
  SR3D_CHECK(p->C > 0 && p->Z > 0 && p->Y > 0 && p->X > 0, SR3D_E_ARG, "%s: non-positive dimension", what);
  SR3D_CHECK(p->Z % kS == 0 && p->Y % kS == 0 && p->X % kS == 0, SR3D_E_ARG,
             "%s: (Z, Y, X) = (%d, %d, %d) must be multiples of %d", what, p->Z, p->Y, p->X, kS);
  SR3D_CHECK(p->Z <= kMaxLevels, SR3D_E_ARG, "%s: %d levels > %d", what, p->Z, kMaxLevels);
  SR3D_CHECK(p->hr_margin >= 0 && p->hr_margin % kS == 0, SR3D_E_ARG, "%s: hr_margin %d must be a multiple of %d",
             what, p->hr_margin, kS);
  SR3D_CHECK(2 * p->hr_margin < p->Y && 2 * p->hr_margin < p->X, SR3D_E_ARG,
             "%s: hr_margin %d leaves no window of (%d, %d)", what, p->hr_margin, p->Y, p->X);
  SR3D_CHECK(p->channel_stride >= (long long)p->Z * p->Y * p->X || p->C == 1, SR3D_E_ARG,
             "%s: channel stride %lld < Z * Y * X", what, p->channel_stride);
  SR3D_CHECK((long long)p->C * p->Y * p->X < (1ll << 31), SR3D_E_ARG, "%s: more than 2^31 columns", what);
  if (p->lev) {
    for (int k = 0; k < p->Z; k++) {
      SR3D_CHECK(isfinite(p->lev[k]), SR3D_E_ARG, "%s: level coordinate %d is not finite", what, k);
      SR3D_CHECK(k == 0 || p->lev[k] > p->lev[k - 1], SR3D_E_ARG, "%s: level coordinates must increase strictly",
                 what);
    }
  }
  SR3D_CHECK(workspace, SR3D_E_ARG, "%s: null workspace", what);
  const size_t need = sr3d_lrdata_workspace_bytes(p->C, p->Y, p->X);
  SR3D_CHECK(workspace_bytes >= need, SR3D_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
             workspace_bytes, need);

  LrParams q{};
  q.raw = (const float*)p->raw;
  q.cstride = p->channel_stride;
  q.mask = (const unsigned char*)p->hr_mask;
  q.tops = (const int*)p->lr_tops;
  q.lat = p->lat, q.lon = p->lon;
  q.hr = (float*)p->hr_out, q.lr = (float*)p->lr_out;
  q.C = p->C, q.Z = p->Z, q.Y = p->Y, q.X = p->X, q.m = p->hr_margin;
  q.Yc = p->Y - 2 * p->hr_margin, q.Xc = p->X - 2 * p->hr_margin;
  q.tiles_x = (q.Xc + kTileX - 1) / kTileX;
  q.align = p->align_nan ? 1 : 0;
  q.has_lev = p->lev ? 1 : 0;
  if (p->lev)
    for (int k = 0; k < p->Z; k++) q.lev[k] = p->lev[k];
  const size_t dead_bytes = ((size_t)q.C * q.Y * q.X + 15) & ~(size_t)15;
  q.dead = (unsigned char*)workspace;
  q.xlive = (int*)((char*)workspace + dead_bytes);
  SR3D_CHECK((long long)q.tiles_x * q.C <= 0x7fffffffll && q.Yc / kS <= kMaxGridY, SR3D_E_ARG, "%s: grid too large",
             what);

  hipStream_t st = (hipStream_t)stream;
  int rc = sr3d_zero_words(q.xlive, q.C * q.X, st);
  if (rc) return rc;
  const long long cols = (long long)q.C * q.Y * q.X;
  hipLaunchKernelGGL(lrdata_dead_kernel, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(lrdata_main_kernel, dim3(q.tiles_x * q.C, q.Yc / kS), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
