// The 2.5-D marching stencil of the evaluation passes (gfx950): one walk over (p, t, b) that hands every voxel's error
// terms, plane by plane, to a sink.  sr3d_eval.hip adds them up over the whole volume, sr3d_eval_profile.hip per level,
// sr3d_walldist.hip per class of distance from the walls; the stencil, the rounding rules and the formula of every term
// exist here and nowhere else.
//
//   d = p - t (4 channels: T, u, v, w);  near = calc_mask_near_build_wall(b) (loss_maker.py:57-83)
//   interior = voxels 1 .. n-2 in z, y, x;  M = b * (1 - near) there (loss_maker.py:84-113, 133-160)
//   vel(q) = stds[1:] * q[1:];  div(q) = d_x vel_u + d_y vel_v + d_z vel_w,  central differences with step delta
//   omega(q) = (d_y w - d_z v, d_z u - d_x w, d_x v - d_y u)                (loss_maker.py:163-191)
//
// A workgroup owns a column of the grid: MY = 8 rows x MX = 62 columns, MZS planes, and walks it plane by plane.
//   x: one row = one wave; lanes 0 and 63 are halo columns, so the x neighbours of lanes 1..62 are two wave SHUFFLES
//      away and every global load is one contiguous 256-byte row segment;
//   y: waves 0 and 9 are halo rows; a plane's values go through an LDS tile [field][10 rows][64] (double-buffered by
//      plane parity: one barrier per plane) and the y neighbours are read back from the rows above and below;
//   z: each thread keeps the previous / current / next plane of its column in REGISTERS (rolling window), so a value is
//      loaded from HBM once per tile (plus the halo shell: 10/8 x 64/62 x (ZS+2)/ZS = 1.45x at ZS = 16).
// The near-wall flag (27-tap box of the mask in the reference) is the same separable walk: sum over x by shuffles,
// over y through LDS, over z in the rolling window.
#pragma once
#include "sr3d_common.h"

constexpr int MY = 8, MX = 62, MROWS = MY + 2, MZS = 16;
constexpr int MF = 7;                            // fields that need y neighbours: 3 velocities x (p, t) + mask x-sum
constexpr int kMarchThreads = MROWS * 64;

constexpr int xy_tiles(int Y, int X) { return ((X + MX - 1) / MX) * ((Y + MY - 1) / MY); }
constexpr int z_tiles(int Z) { return (Z + MZS - 1) / MZS; }
constexpr int march_blocks(int Z, int Y, int X) { return xy_tiles(Y, X) * z_tiles(Z); }   // grid.x; grid.y = B

// a voxel's terms: the raw sums of include/sr3d.h, in that order
constexpr int kP = SR3D_PROFILE_SUM_COUNT;
enum {
  P_ABS = SR3D_PROFILE_SUM_ABS, P_SQ = SR3D_PROFILE_SUM_SQ, P_SQ_T = SR3D_PROFILE_SUM_SQ_T,
  P_B = SR3D_PROFILE_SUM_MASK, P_B_ABS = SR3D_PROFILE_SUM_MASK_ABS, P_B_SQ = SR3D_PROFILE_SUM_MASK_SQ,
  P_NEAR = SR3D_PROFILE_SUM_NEAR, P_NEAR_ABS = SR3D_PROFILE_SUM_NEAR_ABS, P_NEAR_SQ = SR3D_PROFILE_SUM_NEAR_SQ,
  P_T = SR3D_PROFILE_SUM_MASK_DT, P_V = SR3D_PROFILE_SUM_MASK_DV,
  P_B_INT = SR3D_PROFILE_SUM_MASK_INT, P_NEAR_INT = SR3D_PROFILE_SUM_NEAR_INT,
  P_RES_P = SR3D_PROFILE_SUM_RES_P, P_RES_T = SR3D_PROFILE_SUM_RES_T, P_DDIV = SR3D_PROFILE_SUM_DDIV,
  P_OMEGA = SR3D_PROFILE_SUM_OMEGA
};

// what the march reads; the parameter structs of both kernels derive from it
struct MarchInputs {
  const float* p;
  const float* t;
  const float* b;
  int B, Z, Y, X;
  float s[4];
  float w;        // 1 / (2 delta)
};

// the argument checks both entry points share (`who` prefixes the error text), then the inputs
static inline int march_inputs(MarchInputs& q, const char* who, const void* p, const void* t, const void* b, int B, int Z,
                               int Y, int X, const float stds[4], float delta_meter) {
  SR3D_CHECK(p && t && b && stds, SR3D_E_ARG, "%s: null pointer", who);
  SR3D_CHECK(B > 0 && Z > 0 && Y > 0 && X > 0, SR3D_E_ARG, "%s: non-positive dimension", who);
  SR3D_CHECK((long long)Z * Y * X < (1ll << 31), SR3D_E_ARG, "%s: grid has >= 2^31 voxels", who);
  SR3D_CHECK(delta_meter > 0.f, SR3D_E_ARG, "%s: delta_meter must be positive", who);
  SR3D_CHECK(B <= 65535, SR3D_E_ARG, "%s: batch too large", who);
  q.p = (const float*)p, q.t = (const float*)t, q.b = (const float*)b;
  q.B = B, q.Z = Z, q.Y = Y, q.X = X;
  for (int i = 0; i < 4; i++) q.s[i] = stds[i];
  q.w = (float)(1.0 / (2.0 * (double)delta_meter));   // math_helper.py:17: the kernel weight is a python float, then an fp32 tensor
  return SR3D_OK;
}

// central difference exactly as the reference's depthwise convolution evaluates it: hi * w + lo * (-w)
// (contraction off: hipcc would otherwise fuse one product into an fma; the convolution rounds both products)
__device__ __forceinline__ float cdiff(float hi, float lo, float w) {
#pragma clang fp contract(off)
  const float a = hi * w, b = lo * -w;
  return a + b;
}

// A thread's place in the launch (block (x: march_blocks, y: sample), kMarchThreads threads): the integer decoding the
// march starts from, also for a sink that reads a further volume at its voxel.
struct MarchPlace {
  int lane, row;        // row 0 / MROWS-1: halo rows
  int x, y, tiz, bi;    // the thread's column, its z tile and its sample
  bool in_xy;
  bool row_reports;     // wave-uniform
  bool owner;           // this thread's voxels have terms
};
__device__ __forceinline__ MarchPlace march_place(const MarchInputs& q) {
  MarchPlace at;
  at.lane = threadIdx.x & 63, at.row = threadIdx.x >> 6;
  int blk = blockIdx.x;
  const int ntx = (q.X + MX - 1) / MX, nty = (q.Y + MY - 1) / MY;
  const int tix = blk % ntx;
  blk /= ntx;
  const int tiy = blk % nty;
  at.tiz = blk / nty;
  at.bi = blockIdx.y;
  at.x = tix * MX - 1 + at.lane, at.y = tiy * MY - 1 + at.row;
  at.in_xy = (unsigned)at.x < (unsigned)q.X && (unsigned)at.y < (unsigned)q.Y;
  at.row_reports = at.row >= 1 && at.row <= MY;
  at.owner = at.in_xy && at.lane >= 1 && at.lane <= MX && at.row_reports;
  return at;
}

// The march of one workgroup (kMarchThreads threads, block (x: march_blocks, y: sample)) over its column; `tile` is the
// calling kernel's LDS.  The column holds the planes tiz * MZS .. of z tile tiz (so j % MZS is a plane's index within
// its column); the march returns how many.  For every plane j of the column, in rising order, v[kP] holds the terms of
// the lane's voxel (x, y, j) -- all zero for a halo lane or a lane outside the grid, the terms from P_B_INT on zero off
// the interior -- and the sink is told in three places, so that a sink which adds per lane does so under the branch
// that computed the terms and a sink which reduces across the wave sees all lanes:
//   sink.voxel(j, v)     by a lane that has a voxel, once v[.. P_V] are set;
//   sink.interior(v)     by a lane whose voxel is interior, once v[P_B_INT ..] are set;
//   sink.plane(j, v)     by ALL lanes of every wave of the rows 1 .. MY (wave-uniform), with the complete v.
// A sink uses either the first two or the last one and leaves the others empty.  (With the wave-uniform call alone the
// adding kernel measured 3 % slower than with its adds under the branches: 20 zero-filled registers merged per plane.)
template <typename Sink>
__device__ __forceinline__ int eval_march(const MarchInputs& q, float (*tile)[MF][MROWS][64], Sink& sink) {
#pragma clang fp contract(off)
  const MarchPlace at = march_place(q);
  const int lane = at.lane, row = at.row, tiz = at.tiz, bi = at.bi, x = at.x, y = at.y;
  const int z_lo = tiz * MZS, z_hi = min(z_lo + MZS, q.Z);             // output planes [z_lo, z_hi)
  const bool in_xy = at.in_xy, row_reports = at.row_reports, owner = at.owner;
  const bool inner_xy = owner && x >= 1 && x < q.X - 1 && y >= 1 && y < q.Y - 1;
  const long long zyx = (long long)q.Z * q.Y * q.X, sz = (long long)q.Y * q.X;
  const long long col = (long long)y * q.X + x;
  const float* pb = q.p + (long long)bi * 4 * zyx + col;
  const float* tb = q.t + (long long)bi * 4 * zyx + col;
  const float* mb = q.b + (long long)bi * zyx + col;

  // rolling window (index 0 = plane j-1, 1 = plane j, 2 = plane j+1 when plane j is reported)
  float vel[3][2][3];      // scaled velocity [plane][p / t][u, v, w]
  float pc1[4], tc1[4];    // all four channels of plane j (non-stencil sums)
  float b1 = 0.f, sxy[3] = {0.f, 0.f, 0.f};
  float gx1[2][3], gy1[2][3];   // x / y derivatives of plane j, formed when plane j arrived
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) vel[a][k][c] = 0.f;
#pragma unroll
  for (int c = 0; c < 4; c++) pc1[c] = tc1[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) gx1[k][c] = gy1[k][c] = 0.f;

  for (int zz = z_lo - 1; zz <= z_hi; zz++) {          // plane zz arrives; plane j = zz - 1 is reported
    const bool in_z = (unsigned)zz < (unsigned)q.Z;
    const bool live = in_xy && in_z;
    float pn[4], tn[4], bn = 1.f;                       // outside the grid: zero field, "fluid" mask (1 - b = 0)
#pragma unroll
    for (int c = 0; c < 4; c++) pn[c] = tn[c] = 0.f;
    if (live) {
      const long long o = (long long)zz * sz;
#pragma unroll
      for (int c = 0; c < 4; c++) pn[c] = pb[c * zyx + o], tn[c] = tb[c * zyx + o];
      bn = mb[o];
    }
    float vn[2][3];
#pragma unroll
    for (int c = 0; c < 3; c++) vn[0][c] = q.s[c + 1] * pn[c + 1], vn[1][c] = q.s[c + 1] * tn[c + 1];
    // x neighbours: shuffles (lanes 0 / 63 get garbage from the wrap-around; they are halo lanes and never report)
    float gxn[2][3];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        gxn[k][c] = cdiff(__shfl_down(vn[k][c], 1, 64), __shfl_up(vn[k][c], 1, 64), q.w);
    const float ib = 1.f - bn;
    const float sx = (__shfl_up(ib, 1, 64) + ib) + __shfl_down(ib, 1, 64);
    // y neighbours through LDS
    float (*T)[MROWS][64] = tile[zz & 1];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) T[k * 3 + c][row][lane] = vn[k][c];
    T[6][row][lane] = sx;
    __syncthreads();
    float gyn[2][3], sxy_n = 0.f;
    if (row_reports) {
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) gyn[k][c] = cdiff(T[k * 3 + c][row + 1][lane], T[k * 3 + c][row - 1][lane], q.w);
      sxy_n = (T[6][row - 1][lane] + sx) + T[6][row + 1][lane];
    } else {
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) gyn[k][c] = 0.f;
    }
    sxy[2] = sxy_n;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) vel[2][k][c] = vn[k][c];

    // ---- report plane j = zz - 1 (its z+1 neighbour has just arrived): this thread's terms, handed to the sink
    const int j = zz - 1;
    if (row_reports && j >= z_lo && j < z_hi) {          // wave-uniform
      float v[kP];
#pragma unroll
      for (int i = 0; i < kP; i++) v[i] = 0.f;
      if (owner) {
        const float bv = b1;
        const float box = (sxy[0] + sxy[1]) + sxy[2];
        const float near = ((box > 0.f ? 1.f : 0.f) * bv > 0.f) ? 1.f : 0.f;
        float sa = 0.f, sq = 0.f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const float d = pc1[c] - tc1[c];
          const float d2 = d * d;
          sa += fabsf(d), sq += d2;
          v[P_SQ_T + c] = d2;
        }
        v[P_ABS] = sa, v[P_SQ] = sq;
        v[P_B] = bv, v[P_B_ABS] = bv * sa, v[P_B_SQ] = bv * sq;
        v[P_NEAR] = near, v[P_NEAR_ABS] = near * sa, v[P_NEAR_SQ] = near * sq;
        // |T_p - T_t| * std_T and || std_v * v_p - std_v * v_t ||  (loss_maker.py:636-703)
        const float dT = fabsf(pc1[0] - tc1[0]) * q.s[0];
        float n2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float dv = vel[1][0][c] - vel[1][1][c];
          n2 += dv * dv;
        }
        const float dV = sqrtf(n2);
        v[P_T] = bv * dT, v[P_V] = bv * dV;
        sink.voxel(j, v);
        if (inner_xy && j >= 1 && j < q.Z - 1) {
          v[P_B_INT] = bv, v[P_NEAR_INT] = near;
          const float M = bv * (1.f - near);
          float res[2], om[2][3];
#pragma unroll
          for (int k = 0; k < 2; k++) {
            float gz[3];
#pragma unroll
            for (int c = 0; c < 3; c++) gz[c] = cdiff(vel[2][k][c], vel[0][k][c], q.w);
            res[k] = (gx1[k][0] + gy1[k][1]) + gz[2];
            om[k][0] = gy1[k][2] - gz[1];       // dw/dy - dv/dz
            om[k][1] = gz[0] - gx1[k][2];       // du/dz - dw/dx
            om[k][2] = gx1[k][1] - gy1[k][0];   // dv/dx - du/dy
          }
          const float rp = res[0] * M, rt = res[1] * M;
          v[P_RES_P] = fabsf(rp), v[P_RES_T] = fabsf(rt), v[P_DDIV] = fabsf(rp - rt);
          float o2 = 0.f;
#pragma unroll
          for (int a = 0; a < 3; a++) {
            const float dd = om[0][a] * M - om[1][a] * M;
            o2 += dd * dd;
          }
          v[P_OMEGA] = sqrtf(o2);
          sink.interior(v);
        }
      }
      sink.plane(j, v);
    }
    // ---- roll the window: plane zz becomes "plane j" of the next iteration
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        vel[0][k][c] = vel[1][k][c], vel[1][k][c] = vel[2][k][c];
        gx1[k][c] = gxn[k][c], gy1[k][c] = gyn[k][c];
      }
#pragma unroll
    for (int c = 0; c < 4; c++) pc1[c] = pn[c], tc1[c] = tn[c];
    b1 = bn;
    sxy[0] = sxy[1], sxy[1] = sxy[2];
  }
  return z_hi - z_lo;
}
