// GrADS decode (gfx950): one time step of the LES's four output files (tm, vl, vp, vr) from the raw bytes of the
// step's level window to the dense (4, Z, Y, X) fp32 volume the LR-data maker reads -- the reference's
// io_grads.read_xarray (`xr.where(da == ds.undef, nan, da)`) and align_nan_grids, without xgrads / xarray / dask.
//
// Per value: byte swap if the file's order is not the host's, compare as fp32 with (float)undef -> NaN (a NaN in the
// file stays what it is), and with align_nan the three velocity components are NaN wherever tm is.  yrev / zrev read
// row Y-1-y / level Z-1-z.  The values travel as 32-bit words; only the comparison sees them as floats, so every
// value that is kept keeps its bits.
//
// A pure streaming kernel: the lanes run along x, one lane owns a quad of x-neighbours of ALL FOUR variables (tm is
// read once, the four loads of a lane are independent and issued first).  blockIdx.y is the output level.
//   grads_decode_kernel<true>    16-byte loads and stores: X % 4 == 0 and every slab base and pitch 16-byte aligned
//   grads_decode_kernel<false>   4-byte loads and stores: ragged X, or `options sequential`, whose record markers
//                                shift every slab by 4 bytes
// Plain vector stores, one launch, no workspace, no host synchronisation.
#include <math.h>

#include "sr3d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGridY = 65535;
constexpr unsigned kNaN = 0x7fc00000u;   // numpy's float32 nan

struct GrParams {
  const unsigned char* src[4];
  long long off[4], pitch[4];
  float undef[4];
  unsigned* out;                      // (4, Z, Y, X) words
  unsigned char* tm_is_nan;           // (Z, Y, X) or null
  int X, Y, Z, swap, yrev, zrev, align;
};

__device__ __forceinline__ unsigned decode_word(unsigned u, float undef, int swap) {
  if (swap) u = __builtin_bswap32(u);
  return __builtin_bit_cast(float, u) == undef ? kNaN : u;   // a NaN never compares equal: it stays
}

__device__ __forceinline__ bool word_is_nan(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }

template <bool kVec>
__global__ __launch_bounds__(kThreads) void grads_decode_kernel(const GrParams q) {
  constexpr int kW = kVec ? 4 : 1;                        // values per lane and variable
  const int Xq = q.X / kW;
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= (long long)q.Y * Xq) return;
  const int z = blockIdx.y;
  const int y = (int)(p / Xq), x = (int)(p - (long long)y * Xq) * kW;
  const int sz = q.zrev ? q.Z - 1 - z : z, sy = q.yrev ? q.Y - 1 - y : y;
  const long long in_slab = ((long long)sy * q.X + x) * 4;
  const long long plane = (long long)q.Y * q.X;
  const long long cell = (long long)z * plane + (long long)y * q.X + x;

  unsigned w[4][kW];
#pragma unroll
  for (int v = 0; v < 4; v++) {                           // the four loads first: they are independent
    const unsigned char* s = q.src[v] + q.off[v] + (long long)sz * q.pitch[v] + in_slab;
    if constexpr (kVec) {
      const uint4 u = *reinterpret_cast<const uint4*>(s);
      w[v][0] = u.x, w[v][1] = u.y, w[v][2] = u.z, w[v][3] = u.w;
    } else {
      w[v][0] = *reinterpret_cast<const unsigned*>(s);
    }
  }
  unsigned char nan0[kW];
#pragma unroll
  for (int k = 0; k < kW; k++) {
    w[0][k] = decode_word(w[0][k], q.undef[0], q.swap);
    const bool tn = word_is_nan(w[0][k]);
    nan0[k] = tn ? 1 : 0;
#pragma unroll
    for (int v = 1; v < 4; v++) {
      const unsigned d = decode_word(w[v][k], q.undef[v], q.swap);
      w[v][k] = (q.align && tn) ? kNaN : d;
    }
  }
#pragma unroll
  for (int v = 0; v < 4; v++) {
    unsigned* o = q.out + (long long)v * q.Z * plane + cell;
    if constexpr (kVec) {
      *reinterpret_cast<uint4*>(o) = uint4{w[v][0], w[v][1], w[v][2], w[v][3]};
    } else {
      *o = w[v][0];
    }
  }
  if (q.tm_is_nan) {
    if constexpr (kVec) {
      *reinterpret_cast<uchar4*>(q.tm_is_nan + cell) = uchar4{nan0[0], nan0[1], nan0[2], nan0[3]};
    } else {
      q.tm_is_nan[cell] = nan0[0];
    }
  }
}

}  // namespace

extern "C" {

int sr3d_grads_decode(const void* const src[4], const sr3d_grads_params_t* p, void* stream) {
  const char* what = "grads_decode";
  SR3D_CHECK(src && p, SR3D_E_ARG, "%s: null source table or parameters", what);
  SR3D_CHECK(p->out, SR3D_E_ARG, "%s: null output pointer", what);
  SR3D_CHECK(p->X > 0 && p->Y > 0 && p->Z > 0, SR3D_E_ARG, "%s: non-positive size (Z, Y, X) = (%d, %d, %d)", what,
             p->Z, p->Y, p->X);
  SR3D_CHECK(p->Z <= kMaxGridY, SR3D_E_ARG, "%s: %d levels > %d", what, p->Z, kMaxGridY);
  const long long slab = (long long)p->Y * p->X * 4;
  SR3D_CHECK((long long)p->Z * slab / 4 < (1ll << 40), SR3D_E_ARG, "%s: volume too large", what);

  GrParams q{};
  bool vec = p->X % 4 == 0 && ((uintptr_t)p->out & 15) == 0 && ((uintptr_t)p->tm_is_nan & 3) == 0;
  for (int v = 0; v < 4; v++) {
    SR3D_CHECK(src[v], SR3D_E_ARG, "%s: null source pointer of variable %d", what, v);
    SR3D_CHECK(p->level_pitch[v] >= slab, SR3D_E_ARG, "%s: variable %d: level pitch %lld < one slab of %lld bytes",
               what, v, p->level_pitch[v], slab);
    SR3D_CHECK(p->level_offset[v] >= 0 && p->level_offset[v] % 4 == 0 && p->level_pitch[v] % 4 == 0 &&
                   ((uintptr_t)src[v] & 3) == 0,
               SR3D_E_ARG, "%s: variable %d: misaligned source, offset %lld or pitch %lld (multiples of 4 needed)",
               what, v, p->level_offset[v], p->level_pitch[v]);
    const long long need = p->level_offset[v] + (long long)(p->Z - 1) * p->level_pitch[v] + slab;
    SR3D_CHECK(p->src_bytes[v] >= need, SR3D_E_ARG, "%s: variable %d: source of %lld bytes, %lld needed", what, v,
               p->src_bytes[v], need);
    q.src[v] = (const unsigned char*)src[v];
    q.off[v] = p->level_offset[v], q.pitch[v] = p->level_pitch[v];
    q.undef[v] = (float)p->undef[v];
    vec = vec && (((uintptr_t)src[v] + (uintptr_t)p->level_offset[v]) & 15) == 0 && p->level_pitch[v] % 16 == 0;
  }
  SR3D_CHECK(((uintptr_t)p->out & 3) == 0, SR3D_E_ARG, "%s: misaligned output pointer", what);
  q.out = (unsigned*)p->out;
  q.tm_is_nan = (unsigned char*)p->tm_is_nan;
  q.X = p->X, q.Y = p->Y, q.Z = p->Z;
  q.swap = p->byteswap ? 1 : 0, q.yrev = p->yrev ? 1 : 0, q.zrev = p->zrev ? 1 : 0, q.align = p->align_nan ? 1 : 0;

  hipStream_t st = (hipStream_t)stream;
  const long long lanes = (long long)p->Y * (p->X / (vec ? 4 : 1));
  const long long blocks = (lanes + kThreads - 1) / kThreads;
  SR3D_CHECK(blocks <= 0x7fffffffll, SR3D_E_ARG, "%s: grid too large", what);
  const dim3 grid((unsigned)blocks, (unsigned)p->Z);
  if (vec)
    hipLaunchKernelGGL(grads_decode_kernel<true>, grid, dim3(kThreads), 0, st, q);
  else
    hipLaunchKernelGGL(grads_decode_kernel<false>, grid, dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
