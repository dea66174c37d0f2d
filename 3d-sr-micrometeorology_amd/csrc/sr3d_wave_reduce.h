// Exchange reduction: N sums over the 64 lanes of a wave (gfx950), shared by the evaluation kernels that reduce the
// marching stencil's 20 terms per wave (sr3d_eval_profile.hip per plane, sr3d_walldist.hip per distance class).
#pragma once
#include "sr3d_common.h"

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
