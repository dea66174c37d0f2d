// Shared pieces of the split-f16 kernels (sr3d_hconv.hip, sr3d_hconv_s2.hip, sr3d_hwgrad.hip, _s2, _fc): fp32 operands as two fp16
// halves on v_mfma_f32_32x32x16_f16.  gfx950 only.
#pragma once
#include "sr3d_common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// store one result as the activation element type (BF: bfloat16, round to nearest even)
template <bool BF>
__device__ __forceinline__ void st_act(float* base, long long idx, float v) {
  if constexpr (BF)
    reinterpret_cast<__bf16*>(base)[idx] = (__bf16)v;
  else
    base[idx] = v;
}
typedef __attribute__((address_space(3))) void* lds_p;

// Exponent s with amax * 2^s in [2^13, 2^14): the largest element then splits into hi = fp16(a), lo = fp16(a - hi) with
// |a - hi - lo| <= 2^-22 |a| and cannot overflow.  kSplitScaleNone for amax = 0 ("no opinion": running minima keep
// their value), 0 for inf / NaN.
constexpr int kSplitScaleNone = 120;
__host__ __device__ inline int split_scale_exp(float amax) {
  if (amax != amax || amax > 3.0e38f) return 0;
  if (!(amax > 0.f)) return kSplitScaleNone;
  int e;
  frexpf(amax, &e);   // amax = m * 2^e, m in [0.5, 1)
  const int s = 14 - e;
  return s > kSplitScaleNone ? kSplitScaleNone : s;
}
// ... as the exponent of a per-tensor or per-layer scale: 0, i.e. no scaling, for an all-zero tensor
__host__ __device__ inline int split_scale_exp_or0(float amax) {
  const int s = split_scale_exp(amax);
  return s == kSplitScaleNone ? 0 : s;
}

// 16 bytes per lane, global -> LDS, buffer form.  (The buffer form on purpose: global_load_lds is a FLAT instruction
// touching two address spaces, and while one is pending hipcc turns every LDS wait of the wave into lgkmcnt(0).  Device
// pass only: the host pass of hipcc rejects the 16-byte size of this builtin -- it checks it against the host's
// feature set -- and then drops the calling kernel's stub without a message.)
__device__ __forceinline__ void split_lds_dma16(__amdgpu_buffer_rsrc_t rs, lds_p dst, int voffset) {
#if __HIP_DEVICE_COMPILE__
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, voffset, 0, 0, 0);
#endif
}

// keeps a wave-uniform value in a scalar register and opaque to the optimiser
template <typename T>
__device__ __forceinline__ void split_pin_scalar(T& x) {
  asm volatile("" : "+s"(x));
}

__device__ __forceinline__ float split_act(float v, int act) {
  if (act == SR3D_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == SR3D_ACT_LRELU) return v > 0.f ? v : 0.01f * v;
  return v;
}

// The split of TWO elements: hi = fp16(v * mult), lo = fp16(v * mult - hi), packed (a in the low halves): two v_fma_mix
// per element, written straight into the halves of the packed dwords.  (hipcc turns the plain C form -- multiply, convert,
// convert back, subtract, convert -- into 3 instructions per element, a third of them packed fp32 (v_pk_mul_f32 /
// v_pk_fma_f32): each of those costs ~20 cycles of vector issue beside MFMAs, and an MFMA 16x16x32 leaves the SIMD's
// vector issue free for only 8 of its 16 cycles -- MI355X_MICROARCH.md, cycle constants.)  Same values as the C form: the
// product by a power of two is exact, so each half is rounded once.
__device__ __forceinline__ void split_pair(const float a, const float b, const float mult, unsigned& hi, unsigned& lo) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(a), "v"(mult));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(b), "v"(mult));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(a), "v"(mult), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(b), "v"(mult), "v"(hi));
}
// ... of 8 elements v[0], v[st], ..., v[7 st] into one 16-byte piece per part
__device__ __forceinline__ void split_piece(const float* v, const int st, const float mult, h8& hi, h8& lo) {
  unsigned h[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; k++) split_pair(v[2 * k * st], v[(2 * k + 1) * st], mult, h[k], l[k]);
  hi = __builtin_bit_cast(h8, u32x4{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(h8, u32x4{l[0], l[1], l[2], l[3]});
}

// Largest value of a non-negative float over the 64 lanes of the wave, returned wave-uniform.  Four DPP steps inside the
// rows of 16 lanes (quad swaps, half-row mirror, row mirror) and four lane reads: vector-ALU only.  (__shfl_xor is a
// ds_bpermute per step: six dependent trips through the LDS pipe, ~700 cycles in front of a barrier.)
__device__ __forceinline__ float split_wave_max(float m) {
// (old = the value itself: every lane has a valid source in these four patterns, and a constant would cost a v_mov per step)
#define SR3D_DPP_MAX(ctrl) m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), ctrl, 0xf, 0xf, false)))
  SR3D_DPP_MAX(0xB1);    // quad_perm [1, 0, 3, 2]
  SR3D_DPP_MAX(0x4E);    // quad_perm [2, 3, 0, 1]
  SR3D_DPP_MAX(0x141);   // row_half_mirror
  SR3D_DPP_MAX(0x140);   // row_mirror
#undef SR3D_DPP_MAX
  const int mi = __builtin_bit_cast(int, m);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// ---- workgroup geometry shared by the forward / input-gradient kernels (sr3d_hconv.hip, sr3d_hconv_s2.hip)
// virtual workgroup id -> (row block, voxel tile): the row blocks of one tile run next to each other on one XCD
struct SplitTile {
  int nblk, tix, tiy, tiz;
};
__device__ __forceinline__ SplitTile split_tile_of(const int v, const int nblk, const int ntx, const int nty) {
  SplitTile t;
  t.nblk = v % nblk;
  int blk = v / nblk;
  t.tix = blk % ntx;
  blk /= ntx;
  t.tiy = blk % nty;
  t.tiz = blk / nty;
  return t;
}
// GEMM rows -> n2 64-row blocks, and n1 (0 or 1) last block of <= 32 rows
inline void split_row_split(int rows, int* n2, int* n1) {
  const int nfull = rows / 64, rem = rows - nfull * 64;
  *n2 = nfull + (rem > 32 ? 1 : 0);
  *n1 = (rem > 0 && rem <= 32) ? 1 : 0;
}

// Per-slice base pointers of sample b of a channel concatenation, pinned in scalar registers: left to itself hipcc turns the
// slice selects into dependent kernel-argument loads (two or three ~200-cycle scalar-load round trips per channel, in every
// wave, at the start of every chunk).  ESZ = bytes per element, chan_bytes = bytes of one channel volume.
// (separate members, not arrays: an array would be indexed in scratch memory)
template <int ESZ>
struct SplitSliceBases {
  unsigned long long sb0, sb1, sb2, sb3, dsb1, dsb2, dsb3;
  int cb0, cb1, cb2, cb3, dcb1, dcb2, dcb3;
  int chan_bytes;
  __device__ __forceinline__ SplitSliceBases(const ChanCat& in, const int b, const int chan_bytes_) : chan_bytes(chan_bytes_) {
#define SR3D_SLICE_BASE(i) (reinterpret_cast<unsigned long long>(in.ptr[i]) + (unsigned long long)((long long)b * in.bstride[i]) * ESZ)
    sb0 = SR3D_SLICE_BASE(0), sb1 = SR3D_SLICE_BASE(1), sb2 = SR3D_SLICE_BASE(2), sb3 = SR3D_SLICE_BASE(3);
#undef SR3D_SLICE_BASE
    cb0 = in.cbeg[0], cb1 = in.cbeg[1], cb2 = in.cbeg[2], cb3 = in.cbeg[3];
    split_pin_scalar(sb0), split_pin_scalar(sb1), split_pin_scalar(sb2), split_pin_scalar(sb3);
    split_pin_scalar(cb0), split_pin_scalar(cb1), split_pin_scalar(cb2), split_pin_scalar(cb3);
    dsb1 = sb1 - sb0, dsb2 = sb2 - sb1, dsb3 = sb3 - sb2;
    dcb1 = cb1 - cb0, dcb2 = cb2 - cb1, dcb3 = cb3 - cb2;
    split_pin_scalar(dsb1), split_pin_scalar(dsb2), split_pin_scalar(dsb3), split_pin_scalar(dcb1), split_pin_scalar(dcb2), split_pin_scalar(dcb3);
  }
  __device__ __forceinline__ int slice_of(const int gc) const { return (gc >= cb1) + (gc >= cb2) + (gc >= cb3); }
  // address of concat channel gc (wave-uniform)
  // (mask arithmetic instead of selects: hipcc turns a select chain over four values into a lookup table in scratch)
  __device__ __forceinline__ unsigned long long chan_base(const int gc) const {
    const long long m1 = -(long long)(gc >= cb1), m2 = -(long long)(gc >= cb2), m3 = -(long long)(gc >= cb3);
    const unsigned long long base = sb0 + (dsb1 & (unsigned long long)m1) + (dsb2 & (unsigned long long)m2) + (dsb3 & (unsigned long long)m3);
    const int c0 = cb0 + (dcb1 & (int)m1) + (dcb2 & (int)m2) + (dcb3 & (int)m3);
    return base + (unsigned long long)(unsigned)(gc - c0) * (unsigned long long)(unsigned)chan_bytes;
  }
};

// Running per-slice maxima of |x| over a workgroup's halo tiles, exported at the end for the split-f16 weight gradient of the
// same layer (it needs max |x| per slice; the forward kernels see every element anyway).
struct SplitSliceMax {
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
  __device__ __forceinline__ void credit(const int sl, const float mv) {
    m0 = sl == 0 ? fmaxf(m0, mv) : m0;
    m1 = sl == 1 ? fmaxf(m1, mv) : m1;
    m2 = sl == 2 ? fmaxf(m2, mv) : m2;
    m3 = sl == 3 ? fmaxf(m3, mv) : m3;
  }
  // one lane per wave: into slot[slice * 64] (bits of a non-negative float order like unsigned integers)
  __device__ __forceinline__ void export_to(unsigned* slot) const {
    if (m0 > 0.f) atomicMax(slot, __float_as_uint(m0));
    if (m1 > 0.f) atomicMax(slot + 64, __float_as_uint(m1));
    if (m2 > 0.f) atomicMax(slot + 128, __float_as_uint(m2));
    if (m3 > 0.f) atomicMax(slot + 192, __float_as_uint(m3));
  }
};

// Tile scale: the four waves of a workgroup exchange the largest magnitude of their rows of a chunk through
// xmax[chunk parity][wave] in LDS (the caller's barrier lies between the two calls).  BF: no scaling, bf16 has fp32's
// exponent range.
// this wave's maximum m (one value per lane) -> its slot; returns the maximum, wave-uniform
template <bool BF>
__device__ __forceinline__ float split_publish_max(float* xmax, const int parity, const int wave, const int lane, float m) {
  if constexpr (BF) return 0.f;
  m = split_wave_max(m);
  if (lane == 0) xmax[parity * 4 + wave] = m;
  return m;
}
// running scale exponent: the largest chunk magnitude seen so far decides (kSplitScaleNone until a non-zero chunk came)
template <bool BF>
__device__ __forceinline__ int split_next_scale(const float* xmax, const int parity, const int s_run) {
  if constexpr (BF) return 0;
  const float m = fmaxf(fmaxf(xmax[parity * 4 + 0], xmax[parity * 4 + 1]), fmaxf(xmax[parity * 4 + 2], xmax[parity * 4 + 3]));
  const int s_c = __builtin_amdgcn_readfirstlane(split_scale_exp(m));
  return s_c < s_run ? s_c : s_run;
}

// max |x| of a tensor into *slot with atomicMax (bits of a non-negative float order like unsigned integers; the caller
// zeroes the slot).  Defined in sr3d_hconv.hip.
int sr3d_absmax_launch(const float* x, long long n, unsigned* slot, hipStream_t st);

// ---- shared by the weight-gradient files (sr3d_hwgrad.hip, sr3d_hwgrad_s2.hip, sr3d_hwgrad_fc.hip); defined in sr3d_hwgrad.hip
// Split count of the (b, z, y) rows: 2 .. 6 rounds over the 256 CUs (one workgroup per CU; cols = workgroups per split), the
// count that leaves the last round fullest, with at least min_rows_per_split rows each (the warm-up steps per plane segment)
long long sr3d_hwgrad_splits(long long rows, long long cols, int min_rows_per_split);
// dW[n][c][tap] = 2^-(sx(c)+sd(n)) * sum_s slab[s][tap][n][c], the S slabs summed in a fixed order (amax = nullptr: unscaled);
// swapped: dW[c][n][26 - tap] (sr3d_hwgrad_fc).  x / dy: the kernel's channel / row operands, for the slice of every c / n.
int sr3d_hwgrad_reduce_launch(const float* slab, float* dw, int S, int N, int C, int ldc, int Npad, int Cpad, const float* amax,
                              const ChanCat& x, const ChanCat& dy, bool swapped, hipStream_t st);
