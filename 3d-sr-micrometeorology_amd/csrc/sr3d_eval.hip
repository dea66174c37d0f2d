// All evaluation metrics of the reference's final test pass in ONE streaming kernel (gfx950).
//
// The reference evaluates ten nn.Modules one after the other on every test sample (script/train_model.py:366-390,
// src/loss_maker.py:522-741): each re-reads prediction, target and mask, and the divergence / vorticity ones run
// 27-tap depthwise convolutions for 2-tap central differences.  Here one pass over (p, t, b) -- 36 B per voxel --
// accumulates every sum those modules need; a one-block kernel turns them into the metric values.  The pass is the
// marching stencil of sr3d_eval_march.h, which defines every term; this file adds them up over the whole volume.
//
// Reductions are two-stage with a fixed order (per-thread -> wave (DPP) -> block -> ordered final sum in double):
// bit-reproducible run to run.
#include "sr3d_eval_march.h"

namespace {

constexpr int kThreads = 256;
constexpr int kAcc = 20;

enum {
  A_ABS = 0,     // sum |d|, 4 channels
  A_B_ABS,       // sum b * |d|
  A_B,           // sum b
  A_NEAR_ABS,    // sum near * |d|
  A_NEAR,        // sum near
  A_RES_P,       // sum_int M |div(p)|
  A_RES_T,       // sum_int M |div(t)|
  A_B_INT,       // sum_int b
  A_NEAR_INT,    // sum_int near
  A_T,           // sum b |d_T| * std_T
  A_V,           // sum b ||std_v * d_v||
  A_T_LEV,       // the same two restricted to z == lev
  A_V_LEV,
  A_B_LEV,       // sum_{z == lev} b
  A_DDIV,        // sum_int |M div(p) - M div(t)|
  A_OMEGA,       // sum_int M ||omega(p) - omega(t)||
  A_SQ,          // sum d^2
  A_B_SQ,        // sum b d^2
  A_NEAR_SQ,     // sum near d^2
  A_UNUSED
};

struct EvalParams : MarchInputs {
  int lev;
  float* part;    // [blocks][kAcc]
  float* out;     // SR3D_EVAL_COUNT values
  long long vox;  // B * Z * Y * X
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the march's sink: every lane adds its voxel's terms into its own accumulators
struct BlockSums {
  float acc[kAcc];
  int lev;
  __device__ __forceinline__ void voxel(int j, const float (&v)[kP]) {
    acc[A_ABS] += v[P_ABS], acc[A_SQ] += v[P_SQ];
    acc[A_B] += v[P_B], acc[A_B_ABS] += v[P_B_ABS], acc[A_B_SQ] += v[P_B_SQ];
    acc[A_NEAR] += v[P_NEAR], acc[A_NEAR_ABS] += v[P_NEAR_ABS], acc[A_NEAR_SQ] += v[P_NEAR_SQ];
    acc[A_T] += v[P_T], acc[A_V] += v[P_V];
    if (j == lev) acc[A_T_LEV] += v[P_T], acc[A_V_LEV] += v[P_V], acc[A_B_LEV] += v[P_B];
  }
  __device__ __forceinline__ void interior(const float (&v)[kP]) {
    acc[A_B_INT] += v[P_B_INT], acc[A_NEAR_INT] += v[P_NEAR_INT];
    acc[A_RES_P] += v[P_RES_P], acc[A_RES_T] += v[P_RES_T], acc[A_DDIV] += v[P_DDIV];
    acc[A_OMEGA] += v[P_OMEGA];
  }
  __device__ __forceinline__ void plane(int, const float (&)[kP]) {}
};

__global__ __launch_bounds__(kMarchThreads) void eval_kernel(const EvalParams q) {
#pragma clang fp contract(off)
  __shared__ float tile[2][MF][MROWS][64];
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;

  BlockSums sums;
#pragma unroll
  for (int i = 0; i < kAcc; i++) sums.acc[i] = 0.f;
  sums.lev = q.lev;
  eval_march(q, tile, sums);
  const float (&acc)[kAcc] = sums.acc;

  __shared__ float sm[kMarchThreads / 64][kAcc];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kAcc; i++) {
    const float v = wave_sum(acc[i]);
    if (lane == 0) sm[row][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kAcc) {
    float v = 0.f;
    for (int w = 0; w < kMarchThreads / 64; w++) v += sm[w][threadIdx.x];
    q.part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * kAcc + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(kThreads) void eval_final_kernel(const EvalParams q, int nblk) {
  // every accumulator: 256 strided partial sums (independent loads, all in flight), then a fixed-order tree in LDS
  __shared__ double S[kAcc];
  __shared__ double red[kThreads];
  for (int k = 0; k < kAcc; k++) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kThreads) v += (double)q.part[(long long)b * kAcc + k];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) S[k] = red[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float eps = 1e-30f;   // the modules' default (loss_maker.py:523, 540, 557, 578, 638, 674)
  auto F = [&](int i) { return (float)S[i]; };
  float* o = q.out;
  const float n_all = (float)(4.0 * (double)q.vox);
  o[SR3D_EVAL_L1] = F(A_ABS) / n_all;
  o[SR3D_EVAL_L2] = F(A_SQ) / n_all;
  // masks are broadcast over the 4 channels before torch.sum: the denominator is 4 * sum(mask)
  o[SR3D_EVAL_MASKED_L1] = F(A_B_ABS) / (4.f * F(A_B) + eps);
  o[SR3D_EVAL_MASKED_L2] = F(A_B_SQ) / (4.f * F(A_B) + eps);
  o[SR3D_EVAL_MASKED_L1_NEAR_WALL] = F(A_NEAR_ABS) / (4.f * F(A_NEAR) + eps);
  o[SR3D_EVAL_MASKED_L2_NEAR_WALL] = F(A_NEAR_SQ) / (4.f * F(A_NEAR) + eps);
  const float n_grid = F(A_B_INT) - F(A_NEAR_INT);   // loss_maker.py:110 (no eps: 0 / 0 = nan there too)
  o[SR3D_EVAL_RESIDUAL_CONTINUITY] = F(A_RES_P) / n_grid;
  o[SR3D_EVAL_RESIDUAL_CONTINUITY_TARGET] = F(A_RES_T) / n_grid;
  o[SR3D_EVAL_ABS_DIFF_TEMPERATURE] = F(A_T) / (F(A_B) + eps);
  o[SR3D_EVAL_DIFF_VELOCITY_NORM] = F(A_V) / (F(A_B) + eps);
  o[SR3D_EVAL_ABS_DIFF_TEMPERATURE_LEV] = F(A_T_LEV) / (F(A_B_LEV) + eps);
  o[SR3D_EVAL_DIFF_VELOCITY_NORM_LEV] = F(A_V_LEV) / (F(A_B_LEV) + eps);
  o[SR3D_EVAL_ABS_DIFF_DIVERGENCE] = F(A_DDIV) / n_grid;
  o[SR3D_EVAL_DIFF_OMEGA_NORM] = F(A_OMEGA) / n_grid;
  // raw sums (the weighted losses of loss_maker.py:216-255 combine them with a run-time weight)
  o[SR3D_EVAL_SUM_ABS] = F(A_ABS), o[SR3D_EVAL_SUM_MASK_ABS] = F(A_B_ABS);
  o[SR3D_EVAL_SUM_SQ] = F(A_SQ), o[SR3D_EVAL_SUM_MASK_SQ] = F(A_B_SQ);
  o[SR3D_EVAL_SUM_MASK] = F(A_B);
}

}  // namespace

extern "C" {

size_t sr3d_eval_metrics_workspace_bytes(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)B * march_blocks(Z, Y, X) * kAcc * sizeof(float);
}

int sr3d_eval_metrics(const void* p, const void* t, const void* b, int B, int Z, int Y, int X, const float stds[4],
                      float delta_meter, int lev, void* out, void* workspace, void* stream) {
  SR3D_CHECK(out && workspace, SR3D_E_ARG, "eval_metrics: null pointer");
  EvalParams q{};
  if (int rc = march_inputs(q, "eval_metrics", p, t, b, B, Z, Y, X, stds, delta_meter)) return rc;
  SR3D_CHECK(lev >= 0 && lev < Z, SR3D_E_ARG, "eval_metrics: level %d is outside the grid (Z = %d)", lev, Z);
  q.lev = lev;
  q.part = (float*)workspace, q.out = (float*)out;
  q.vox = (long long)B * Z * Y * X;
  const int nbs = march_blocks(Z, Y, X), nb = nbs * B;
  SrProfScope prof(SR3D_PROF_EVAL, 36.0 * (double)q.vox, (hipStream_t)stream);   // p, t (32 B) + b (4 B) per voxel
  hipLaunchKernelGGL(eval_kernel, dim3(nbs, B), dim3(kMarchThreads), 0, (hipStream_t)stream, q);
  SR3D_HIP(hipGetLastError());
  hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, q, nb);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
