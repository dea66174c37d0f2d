// Scale-resolved evaluation (gfx950): two-point moments of the predicted, the true and the error field over the valid
// fluid pairs (x, x + r e_d), per sample, level, direction d and lag r = 1 .. R (include/sr3d.h states the pair rules).
// Everything is summed in fp64: fourth moments of fp32 data lose everything in fp32.
//
//   scale_run_{x,y,z}_kernel   unobstructed rule only: three uint8 volumes in the workspace, run_d(x) = the number of
//                      consecutive fluid cells from x in +d, capped at 255 (> SR3D_SCALE_MAX_LAG).  A pair is then valid
//                      iff run_d(x) > r: both ends and everything between them are fluid, and x + r e_d is inside.
//                      x: a wave per row, 64 cells at a time from the row's end, the run inside a chunk from the ballot of
//                      the fluid flags; y and z: a thread per column walking down from its end (lanes along x: coalesced).
//   scale_kernel       block (x: (level, direction, lag, channel), y: sample): one workgroup owns one channel of one
//                      output row.  It sweeps the level's plane of first cells once: the second cell is a shifted read
//                      of the same row (d = x, left to L1) or a coalesced read of another row / plane (d = y, z).  24
//                      fp64 accumulators per thread (3 series x 8 moments), added only under the pair's validity -- a
//                      value of a cell outside every valid pair is never loaded into a sum (a NaN there changes
//                      nothing).  Reduced over the wave by shuffles and over the 4 waves in index order, stored
//                      directly: no partial records, no atomics, nothing to clear; two calls are bit-equal and a
//                      sample's rows do not depend on the batch around it.  A lag that does not fit has an empty sweep
//                      and stores exact zeros.
#include "sr3d_common.h"

namespace {

constexpr int kSeries = SR3D_SCALE_SERIES, kMoments = SR3D_SCALE_MOMENTS, kDirs = SR3D_SCALE_DIRS;
constexpr int kAcc = 3 * kMoments;                   // pred, truth, error of one channel
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRunCap = 255;
static_assert(kRunCap > SR3D_SCALE_MAX_LAG, "a capped run must still exceed every lag");
static_assert(kSeries == 12 && kMoments == 8 && kDirs == 3, "layout of sums_out");

struct ScaleParams {
  const float* p;
  const float* t;
  const float* b;
  const uint8_t* run;    // [3][B][Z*Y*X], or null: the pair is valid when both ends are fluid
  uint8_t* run_out;
  int B, Z, Y, X, R;
  double* sums;          // (B, Z, 3, R, 12, 8)
  long long* pairs;      // (B, Z, 3, R)
};

__device__ __forceinline__ uint8_t run_step(int& run, float bv) {
  run = bv > 0.f ? (run < kRunCap ? run + 1 : kRunCap) : 0;
  return (uint8_t)run;
}

// a wave per row (sample, z, y)
__global__ __launch_bounds__(kThreads) void scale_run_x_kernel(const ScaleParams q) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)q.B * q.Z * q.Y;
  const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;                         // wave-uniform
  const float* mb = q.b + row * q.X;
  uint8_t* out = q.run_out + row * q.X;            // direction 0
  int carry = 0;                                   // the run of the first cell of the chunk to the right
  for (int x0 = (q.X - 1) / 64 * 64; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    const bool fluid = x < q.X && mb[x] > 0.f;
    const unsigned long long after = ~(__ballot(fluid) >> lane);   // bit k: the cell k to the right is not fluid
    const int n = after ? __ffsll(after) - 1 : 64;                 // zeros shifted in end the count at 64 - lane
    int run = n + (n == 64 - lane ? carry : 0);
    run = run < kRunCap ? run : kRunCap;
    if (x < q.X) out[x] = (uint8_t)run;
    carry = __shfl(run, 0, 64);
  }
}

// a thread per column (sample, z, x), walking y down from Y - 1
__global__ __launch_bounds__(kThreads) void scale_run_y_kernel(const ScaleParams q) {
  const long long cols = (long long)q.B * q.Z * q.X;
  const long long col = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (col >= cols) return;
  const long long plane = (long long)q.Y * q.X;
  const long long base = col / q.X * plane + col % q.X;
  const float* mb = q.b + base;
  uint8_t* out = q.run_out + (long long)q.B * q.Z * plane + base;   // direction 1
  int run = 0;
  for (int y = q.Y - 1; y >= 0; y--) out[(long long)y * q.X] = run_step(run, mb[(long long)y * q.X]);
}

// a thread per column (sample, y, x), walking z down from Z - 1
__global__ __launch_bounds__(kThreads) void scale_run_z_kernel(const ScaleParams q) {
  const long long plane = (long long)q.Y * q.X;
  const long long cols = (long long)q.B * plane;
  const long long col = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (col >= cols) return;
  const long long base = col / plane * q.Z * plane + col % plane;
  const float* mb = q.b + base;
  uint8_t* out = q.run_out + 2 * (long long)q.B * q.Z * plane + base;   // direction 2
  int run = 0;
  for (int z = q.Z - 1; z >= 0; z--) out[z * plane] = run_step(run, mb[z * plane]);
}

// the 8 moments of one series for the pair (f0, f1)
__device__ __forceinline__ void add_pair(double* a, double f0, double f1) {
  const double d = f1 - f0, d2 = d * d;
  a[0] += d;
  a[1] += d2;
  a[2] += d2 * d;
  a[3] += d2 * d2;
  a[4] += f0;
  a[5] += f1;
  a[6] += f0 * f0;
  a[7] += f1 * f1;
}

__global__ __launch_bounds__(kThreads) void scale_kernel(const ScaleParams q) {
  __shared__ double red[kWaves][kAcc];
  __shared__ int red_n[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int bid = blockIdx.x;
  const int c = bid & 3;
  bid >>= 2;
  const int r = bid % q.R + 1;
  bid /= q.R;
  const int d = bid % kDirs, z = bid / kDirs;
  const int bi = blockIdx.y;
  const int X = q.X, plane = q.Y * q.X;
  const long long zyx = (long long)q.Z * plane;
  // first cells i of the plane that can have a partner inside the volume: i < lim (d = x: and x + r < X)
  const long long off = d == 0 ? r : d == 1 ? (long long)r * X : (long long)r * plane;
  const int lim = d == 0 ? (r < X ? plane : 0) : d == 1 ? (r < q.Y ? (q.Y - r) * X : 0) : (z + r < q.Z ? plane : 0);
  const long long cell0 = (long long)bi * zyx + (long long)z * plane;
  const float* pc = q.p + ((long long)bi * 4 + c) * zyx + (long long)z * plane;
  const float* tc = q.t + ((long long)bi * 4 + c) * zyx + (long long)z * plane;
  const float* mb = q.b + cell0;
  const uint8_t* run = q.run ? q.run + (long long)d * q.B * zyx + cell0 : nullptr;

  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; k++) acc[k] = 0.0;
  int n = 0;
  for (unsigned i = threadIdx.x; i < (unsigned)lim; i += kThreads) {   // lim < 2^31: i cannot wrap
    bool valid;
    if (run) {
      valid = (int)run[i] > r;                     // implies that the partner is inside the volume
    } else {
      valid = mb[i] > 0.f && (d != 0 || i % (unsigned)X + r < (unsigned)X);
      if (valid) valid = mb[i + off] > 0.f;        // read only where it is inside
    }
    if (valid) {                                   // selected, not multiplied by 0
      const double p0 = (double)pc[i], p1 = (double)pc[i + off], t0 = (double)tc[i], t1 = (double)tc[i + off];
      add_pair(acc, p0, p1);
      add_pair(acc + kMoments, t0, t1);
      add_pair(acc + 2 * kMoments, p0 - t0, p1 - t1);
      n++;
    }
  }

  // across the wave by shuffles, across the waves in index order
#pragma unroll
  for (int k = 0; k < kAcc; k++) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][k] = v;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) red_n[wave] = n;
  __syncthreads();
  const long long row = (((long long)bi * q.Z + z) * kDirs + d) * q.R + (r - 1);
  if (threadIdx.x < kAcc) {
    double v = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; w++) v += red[w][threadIdx.x];
    const int kind = threadIdx.x / kMoments, m = threadIdx.x % kMoments;   // 0 pred, 1 truth, 2 error
    q.sums[(row * kSeries + kind * 4 + c) * kMoments + m] = v;
  }
  if (c == 0 && threadIdx.x == 0) {
    long long tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) tot += red_n[w];
    q.pairs[row] = tot;
  }
}

}  // namespace

extern "C" {

size_t sr3d_eval_scale_statistics_workspace_bytes(int B, int Z, int Y, int X, int R) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || R < 1 || R > SR3D_SCALE_MAX_LAG) return 0;
  const size_t vol = (size_t)B * Z * Y * X;        // one byte per voxel and direction (any R, either pair rule)
  return (kDirs * vol + 7) / 8 * 8;
}

int sr3d_eval_scale_statistics(const void* p, const void* t, const void* b, int B, int Z, int Y, int X, int R,
                               int unobstructed, void* sums_out, void* pairs_out, void* workspace, void* stream) {
  const char* who = "eval_scale_statistics";
  SR3D_CHECK(p && t && b && sums_out && pairs_out && workspace, SR3D_E_ARG, "%s: null pointer", who);
  SR3D_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "%s: non-positive dimension", who);
  SR3D_CHECK(R >= 1 && R <= SR3D_SCALE_MAX_LAG, SR3D_E_ARG, "%s: R must be in 1 .. %d (got %d)", who,
             SR3D_SCALE_MAX_LAG, R);
  SR3D_CHECK((long long)Z * Y * X < (1ll << 31), SR3D_E_ARG, "%s: grid has >= 2^31 voxels", who);
  SR3D_CHECK(B <= 65535, SR3D_E_ARG, "%s: batch too large", who);
  SR3D_CHECK((long long)Z * kDirs * R * 4 < (1ll << 31), SR3D_E_ARG, "%s: too many levels for R = %d", who, R);
  SR3D_CHECK((((uintptr_t)p | (uintptr_t)t | (uintptr_t)b) & 3) == 0, SR3D_E_ARG, "%s: p, t and b must be 4-byte aligned",
             who);
  SR3D_CHECK((((uintptr_t)sums_out | (uintptr_t)pairs_out) & 7) == 0, SR3D_E_ARG,
             "%s: sums_out and pairs_out must be 8-byte aligned", who);
  ScaleParams q{};
  q.p = (const float*)p, q.t = (const float*)t, q.b = (const float*)b;
  q.run = unobstructed ? (const uint8_t*)workspace : nullptr, q.run_out = (uint8_t*)workspace;
  q.B = B, q.Z = Z, q.Y = Y, q.X = X, q.R = R;
  q.sums = (double*)sums_out, q.pairs = (long long*)pairs_out;
  const long long plane = (long long)Y * X, vol = (long long)B * Z * plane;
  const long long gx = (B * (long long)Z * Y + kWaves - 1) / kWaves, gy = (B * (long long)Z * X + kThreads - 1) / kThreads,
                  gz = (B * plane + kThreads - 1) / kThreads;
  SR3D_CHECK(gx < (1ll << 31) && gy < (1ll << 31) && gz < (1ll << 31), SR3D_E_ARG, "%s: batch too large for this grid", who);
  hipStream_t st = (hipStream_t)stream;
  // p, t at both ends of a pair (32 B) + b or the run (4 B) per voxel, direction and lag
  SrProfScope prof(SR3D_PROF_EVAL, 36.0 * (double)vol * kDirs * R, st);
  if (unobstructed) {
    hipLaunchKernelGGL(scale_run_x_kernel, dim3((unsigned)gx), dim3(kThreads), 0, st, q);
    SR3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_run_y_kernel, dim3((unsigned)gy), dim3(kThreads), 0, st, q);
    SR3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(scale_run_z_kernel, dim3((unsigned)gz), dim3(kThreads), 0, st, q);
    SR3D_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(scale_kernel, dim3(Z * kDirs * R * 4, B), dim3(kThreads), 0, st, q);
  SR3D_HIP(hipGetLastError());
  return SR3D_OK;
}

}  // extern "C"
