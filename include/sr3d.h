/* libsr3d -- C ABI of the MI355X-native voxel super-resolution training hot path.
 *
 * The reference (YukiYasuda2718/3d-sr-micrometeorology) has no FFI of its own:
 * every operation on its hot path is a call into PyTorch/ATen (SURVEY.md section
 * 2b, 8b).  Each entry point below replaces one such call site; the reference
 * line it stands in for is cited next to it.  A Python/ctypes binding is in
 * 3d-sr-micrometeorology_amd/_lib.py; INTEGRATION.md shows how the reference's
 * modules would call it.
 *
 * Conventions
 *  - all tensors are dense, layout NCDHW = (B, C, z, y, x), x contiguous.  Element type: fp32 everywhere (the
 *    reference's precision, dataset.py:29), or -- `dtype = SR3D_DTYPE_BF16` in the convolution descriptor and in the
 *    activation-backward / bias-gradient calls -- ACTIVATIONS AND THEIR GRADIENTS in bfloat16 (BASELINE configs[4]:
 *    bf16 storage + bf16 MFMA with fp32 accumulation).  Weights, biases, weight / bias gradients, the loss and the
 *    optimizer state are fp32 in both modes (fp32 master weights);
 *  - every pointer is a DEVICE pointer unless stated; the library never
 *    allocates, frees or caches device memory -- workspaces are passed in and
 *    sized by the *_bytes() queries;
 *  - every call is asynchronous on the hipStream_t handed in (passed as void*)
 *    and re-entrant (autograd calls backward from another thread);
 *  - return value 0 = ok, negative = SR3D_E_*; sr3d_last_error() gives the
 *    message of the calling thread's last failure.  Nothing throws.
 */
#ifndef SR3D_H_
#define SR3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libsr3d.so is linked with -fvisibility=hidden: what this header declares is ALL the library exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define SR3D_VERSION 100 /* 0.1.0 */

enum {
  SR3D_OK = 0,
  SR3D_E_ARG = -1,     /* bad argument / unsupported shape */
  SR3D_E_HIP = -2,     /* a HIP runtime call failed */
  SR3D_E_WORKSPACE = -3 /* workspace too small */
};

/* element type of activations and activation gradients (see Conventions) */
enum { SR3D_DTYPE_F32 = 0, SR3D_DTYPE_BF16 = 1 };

/* activations fused into conv epilogues (custom_conv.py:111-126, unet.py:35,84,105) */
enum { SR3D_ACT_NONE = 0, SR3D_ACT_RELU = 1, SR3D_ACT_LRELU = 2 /* slope 0.01 */,
       SR3D_ACT_OUT_F32 = 0x100 /* flag OR-ed to `act` of sr3d_conv3d_fwd: see there */,
       SR3D_ACT_FROM_Y = 0x200 /* flag OR-ed to `act` of sr3d_gated_act_bwd: see there */,
       SR3D_ACT_UNSHUFFLE = 0x400 /* flag OR-ed to `act` of sr3d_conv3d_bwd_data_act / _fuses_act: see there */ };

/* One operand of a virtual channel concatenation (replaces torch.cat at
 * unet.py:255-293): `channels` channels of a (B, channels, Z, Y, X) tensor.
 * As a gradient destination ptr may be NULL (that slice needs no gradient). */
typedef struct {
  void* ptr;
  int32_t channels;
} sr3d_slice_t;

/* 3x3x3 convolution, padding 1 (every nn.Conv3d of the model: unet.py:30,44,76,
 * 89,103,196,243).  (Z,Y,X) is the INPUT grid; the output grid is
 * floor((Z-1)/stride)+1 per dim.  For gated layers Cout is the width of ONE
 * branch. */
typedef struct {
  int32_t B, Cin, Cout;
  int32_t Z, Y, X;
  int32_t stride; /* 1 or 2 */
  int32_t dtype;  /* SR3D_DTYPE_*: element type of x / y / saved activations / dy / dx */
} sr3d_conv_desc_t;

/* kinds of packed (MFMA-tile-ordered) weight images; the two BWD kinds are built inside
 * sr3d_conv3d_bwd_data (in its workspace) and are not accepted by sr3d_pack_weights */
enum {
  SR3D_PACK_FWD = 0,        /* plain conv forward                              */
  SR3D_PACK_FWD_GATED = 1,  /* feature + gate branches interleaved by 32 rows  */
  SR3D_PACK_BWD = 2,        /* transposed image, rows = input channels that need a gradient */
  SR3D_PACK_BWD_GATED = 3,  /* same with K = [d_feat ; d_gate]                 */
  SR3D_PACK_FWD_UNSHUFFLE = 4 /* plain conv forward of a layer that is called with unshuffle != 0 (UpBlock.up): the
                                 image may hold its rows in voxel-unshuffle order so that the two x-neighbours of an
                                 output voxel are stored together; an image packed as SR3D_PACK_FWD works too */
};

int sr3d_version(void);
const char* sr3d_last_error(void);

/* ---- weights ------------------------------------------------------------ */
/* bytes of the packed image of one layer */
size_t sr3d_packed_weight_bytes(const sr3d_conv_desc_t* d, int kind);
/* w_feat / w_gate: (Cout, Cin, 3,3,3) as in the state_dict; w_gate only for *_GATED */
int sr3d_pack_weights(const sr3d_conv_desc_t* d, int kind, const void* w_feat, const void* w_gate,
                      void* w_packed, void* stream);

/* ---- forward ------------------------------------------------------------ */
/* y = act(conv3d(cat(x_srcs); W) + bias)           nn.Conv3d + LeakyReLU: unet.py:196-198, 72-97, 240-246
 * unshuffle != 0: y is written as unshuffle_voxels(., 2) of that (voxel_shuffle.py:26-42, unet.py:99-108),
 *                 i.e. y has Cout/8 channels on the 2x grid.
 * act | SR3D_ACT_OUT_F32 (bf16 storage, stride 1, no unshuffle): y is an fp32 tensor -- the network's prediction (`last`,
 *                 unet.py:240-246, 295) leaves the engine unrounded, the accumulator's value. */
int sr3d_conv3d_fwd(const sr3d_conv_desc_t* d, const sr3d_slice_t* x_srcs, int n_src, const void* w_packed,
                    const void* bias, void* y, int act, int unshuffle, void* x_absmax, void* stream);

/* Operand maxima for the split-f16 weight gradient, without a separate sweep of the tensors.
 * The split kernels scale their operands by powers of two taken from max |x| and max |dY| per slice.  Kernels that see
 * every element anyway can export those maxima: `x_absmax` of the two forward calls (optional; 4 x 64 uint32, ZEROED by the
 * caller; slice i's maximum is the largest of [64 i, 64 i + 64) read as float bits) is filled when
 * sr3d_conv3d_fwd_exports_absmax() says so for this layer (1: the forward runs on the split-f16 kernel; 0: it does not,
 * the buffer stays untouched and must not be handed on); `absmax_out` of the three activation-backward calls (64 uint32
 * per output tensor, zeroed by the caller, fp32 only).  sr3d_conv3d_bwd_weight takes them as `x_absmax` ([n_src][64]) and
 * `dy_absmax` ([n_dy][64]); NULL = compute by a sweep. */
int sr3d_conv3d_fwd_exports_absmax(const sr3d_conv_desc_t* d, int gated);

/* y = sigmoid(conv(x;Wg)+bg) * act(conv(x;Wf)[+bf])   custom_conv.py:119-123, 303-304
 * save_f = act(feat), save_s = sigmoid(gate) are kept for the backward pass. */
int sr3d_gated_conv3d_fwd(const sr3d_conv_desc_t* d, const sr3d_slice_t* x_srcs, int n_src, const void* w_packed,
                          const void* bias_f, const void* bias_g, void* y, void* save_f, void* save_s, int act,
                          void* x_absmax, void* stream);

/* ---- backward (autograd of the above: optim_helper.py:165 loss.backward()) -- */
/* dx_dsts[i] = slice i of d(cat(x)) = conv_transpose(cat(dy_srcs); W)  (aten convolution_backward, input grad)
 * dy_srcs hold the gradient w.r.t. the PRE-activation conv outputs (1 slice, or 2 = [d_feat, d_gate]);
 * w_feat / w_gate are the (Cout, Cin, 3,3,3) state_dict tensors (w_gate only when n_dy == 2).
 * Destination slices with a NULL ptr (building mask, network input) are not computed at all: their rows
 * are left out of the GEMM.  The workspace receives the transposed weight image. */
size_t sr3d_conv3d_bwd_data_workspace_bytes(const sr3d_conv_desc_t* d, int n_dy);
int sr3d_conv3d_bwd_data(const sr3d_conv_desc_t* d, const sr3d_slice_t* dy_srcs, int n_dy, const void* w_feat,
                         const void* w_gate, const sr3d_slice_t* dx_dsts, int n_dst, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The same with the activation backward of ONE destination slice fused into the epilogue: slice `act_slice` of
 * cat(x) is the output y of a LeakyReLU layer (act = SR3D_ACT_LRELU; `act_y` = that tensor, same shape as the slice), and what
 * is stored there is dL/dy * lrelu'(y) = dL/dpre of THAT layer -- its lrelu_bwd pass (autograd's leaky_relu_backward,
 * pytorch/model/unet.py:72-97,192-199) never runs; in fp32 the stored values are bit-identical to sr3d_conv3d_bwd_data followed
 * by sr3d_lrelu_bwd.  act_absmax (optional, [64] zeroed words, fp32 storage): max |stored| for that layer's weight gradient.
 * Only launches for which sr3d_conv3d_bwd_data_fuses_act answers 1 have this epilogue (the split-f16 / bf16 stride-1 kernel).
 * act | SR3D_ACT_UNSHUFFLE: the slice is the voxel-UNSHUFFLED output of a conv + LeakyReLU layer (UpBlock.up, unet.py:99-108):
 * act_y has the slice's own (fine-grid) layout, and dx_dsts[act_slice].ptr -- a buffer with the slice's element count --
 * receives dL/dpre of THAT layer in ITS layout, (B, 8 C, Z/2, Y/2, X/2) for a slice of C channels (what
 * sr3d_unshuffle_lrelu_bwd would have produced).  Needs X % 4 == 0. */
int sr3d_conv3d_bwd_data_fuses_act(const sr3d_conv_desc_t* d, int n_dy, const sr3d_slice_t* dx_dsts, int n_dst, int act_slice, int act);
int sr3d_conv3d_bwd_data_act(const sr3d_conv_desc_t* d, const sr3d_slice_t* dy_srcs, int n_dy, const void* w_feat,
                             const void* w_gate, const sr3d_slice_t* dx_dsts, int n_dst, int act_slice, const void* act_y,
                             int act, void* act_absmax, void* workspace, size_t workspace_bytes, void* stream);

/* dw[(n, c, kz,ky,kx)] over n in cat(dy_srcs) channels (so for gated layers dw = [dWf ; dWg]).
 * deterministic: fixed split of the voxel reduction + ordered second stage. */
size_t sr3d_conv3d_bwd_weight_workspace_bytes(const sr3d_conv_desc_t* d, int n_total);
int sr3d_conv3d_bwd_weight(const sr3d_conv_desc_t* d, const sr3d_slice_t* x_srcs, int n_src,
                           const sr3d_slice_t* dy_srcs, int n_dy, void* dw, void* workspace, size_t workspace_bytes,
                           const void* x_absmax, const void* dy_absmax, void* stream);

/* db[c] = sum_{b,voxels} dy[b,c,:]   (bias gradient, fp32); workspace >= sr3d_bias_grad_workspace_bytes.
 * `dtype` (here and in the three activation-backward calls below): element type of dy / y / saved tensors / outputs */
size_t sr3d_bias_grad_workspace_bytes(int B, int C, long long voxels);
int sr3d_bias_grad(const void* dy, int B, int C, long long voxels, void* db, void* workspace, int dtype, void* stream);

/* d_feat = dy * s * act'(f),  d_gate = dy * f * s * (1 - s)      (autograd of custom_conv.py:119-123); f = act(feat), s = sigmoid(gate)
 * act | SR3D_ACT_FROM_Y: `save_f` is the layer's OUTPUT y = s * f instead (s > 0: y has the sign of f, and f * s = y), so the
 * forward pass need not store act(feat) at all (sr3d_gated_conv3d_fwd with save_f = NULL, save_s given) */
int sr3d_gated_act_bwd(const void* dy, const void* save_f, const void* save_s, void* d_feat, void* d_gate,
                       long long n, int act, int dtype, void* absmax_out /* [2][64]: d_feat, d_gate */, void* stream);
/* the same with dy + dy2 as the incoming gradient (dy2 may be NULL): a gated output that feeds TWO consumers -- the next block and the
 * U-Net's skip connection (unet.py:262-283: f0..f3) -- receives two gradient tensors, which autograd would add in a pass of its own
 * (AccumulateGrad / the engine's sum of a node's incoming gradients) before this one; the sum is formed in fp32 */
int sr3d_gated_act_bwd_sum(const void* dy, const void* dy2, const void* save_f, const void* save_s, void* d_feat, void* d_gate,
                           long long n, int act, int dtype, void* absmax_out /* [2][64] */, void* stream);
/* dpre = dy * (y > 0 ? 1 : 0.01)        (autograd of nn.LeakyReLU, y = post-activation) */
int sr3d_lrelu_bwd(const void* dy, const void* y, void* dpre, long long n, int dtype, void* absmax_out, void* stream);
/* dpre(B, 8C, Z, Y, X) = shuffle_voxels(dy * lrelu'(y)) for y, dy of shape (B, C, 2Z, 2Y, 2X)
 * (autograd of unet.py:99-108 up to the conv) */
int sr3d_unshuffle_lrelu_bwd(const void* dy, const void* y, void* dpre, int B, int C, int Z, int Y, int X, int dtype,
                             void* absmax_out, void* stream);

/* ---- small data-movement ops ------------------------------------------------ */
/* x0 = cat[nearest_upsample(x, scale), b]     unet.py:143,254-255 ; x: (B,C,Z/s,Y/s,X/s), b: (B,1,Z,Y,X) */
int sr3d_upsample_cat(const void* x, const void* b, void* x0, int B, int C, int Z, int Y, int X, int scale,
                      void* stream);
/* out = AvgPool3d(2,2)(in) for a (B,1,Z,Y,X) mask          unet.py:156,261 */
int sr3d_avgpool2(const void* in, void* out, int B, int Z, int Y, int X, void* stream);
/* near = calc_mask_near_build_wall(b)                       loss_maker.py:57-83 */
int sr3d_near_wall(const void* b, void* near, int B, int Z, int Y, int X, void* stream);

/* Sample preprocessing of the reference's Dataset on the device (dataset.py:139-161, 174, 191-195):
 * out = nan_to_num(clamp?((scaling * x - means[c]) / stds[c], 0, 1), nan = nan_value) for x: (B, C, Z, Y, X) in
 * physical units (C <= 8; means / stds are HOST arrays); z levels below discard_z are then set to nan_value
 * (max_discarded_lr_z_index).  Bit-identical to the CPU expressions of the reference. */
int sr3d_preprocess(const void* x, void* out, int B, int C, int Z, int Y, int X, const float* means, const float* stds,
                    float scaling, int clip, float nan_value, int discard_z, void* stream);

/* ---- PartialConv3d (model/custom_conv.py:129-234; not reachable from UNetSR, kept as an op) ---------------- */
/* update_mask = clamp(s, 0, 1), mask_ratio = slide_winsize / (s + 1e-8) * update_mask with s = sum of the mask over the
 * zero-padded 3x3x3 window and its Cm channels; mask: (Bm, Cm, Z, Y, X) -> both outputs (Bm, 1, OZ, OY, OX). */
int sr3d_pconv_mask_update(const void* mask, int Bm, int Cm, int Z, int Y, int X, int stride, float slide_winsize,
                           void* update_mask, void* mask_ratio, void* stream);
/* out = x * mask, the mask broadcast over batch (Bm = 1) and / or channels (Cm = 1) */
int sr3d_mul_mask(const void* x, const void* mask, void* out, int B, int C, long long voxels, int Bm, int Cm,
                  void* stream);
/* forward (backward = 0): out = bias ? ((in - bias[c]) * ratio + bias[c]) * update : in * ratio
 * backward (= 1): out = in * ratio * (bias ? update : 1); bias_terms (optional) = in * update * (1 - ratio), whose
 * per-channel sum (sr3d_bias_grad) is the bias gradient */
int sr3d_pconv_scale(const void* in, const void* bias, const void* update_mask, const void* mask_ratio, void* out,
                     void* bias_terms, int B, int C, long long voxels, int Bm, int backward, void* stream);

/* ---- losses (forward value + dL/dp in one pass) --------------------------- */
/* out[0] = mean|p-t| ; dLdp = sign(p-t)/n * grad_scale           MyL1Loss, loss_maker.py:194-202 */
size_t sr3d_loss_workspace_bytes(int B, int Z, int Y, int X);
int sr3d_l1_fwd_bwd(const void* p, const void* t, long long n, void* loss_out, void* dLdp, void* workspace,
                    void* stream);
/* MixedDivergenceGradientL2Loss, loss_maker.py:358-450.  p,t: (B,4,Z,Y,X); b: (B,1,Z,Y,X).
 * terms_out (device, 4 floats) = {mse, grd_mse, div_mse, total};  dLdp may be NULL. */
int sr3d_mixed_div_grad_l2_fwd_bwd(const void* p, const void* t, const void* b, int B, int Z, int Y, int X,
                                   const float scales[3], float delta_meter, float w_g, float w_d,
                                   void* terms_out, void* dLdp, void* workspace, void* stream);

/* Gradient of WeightedL1Loss / WeightedL2Loss (loss_maker.py:216-255):
 *   dLdp = e'(p - t) * (b * coef[0] + (1 - b) * coef[1]),   e = |.| (power 1) or (.)^2 (power 2),
 * coef: 2 floats in DEVICE memory (the region weights divided by their voxel counts, times the upstream gradient). */
int sr3d_weighted_lp_bwd(const void* p, const void* t, const void* b, int B, int C, long long voxels, int power,
                         const void* coef, void* dLdp, void* stream);

/* dLdp = d(wts[0]*mse + wts[1]*grd_mse + wts[2]*div_mse)/dp with the three weights read from DEVICE memory
 * (autograd / GradNorm, gradnorm.py:95-100, differentiate individual terms); reuses the workspace a previous
 * sr3d_mixed_div_grad_l2_fwd_bwd call with the same arguments filled. */
int sr3d_mixed_div_grad_l2_bwd(const void* p, const void* t, int B, int Z, int Y, int X, const float scales[3],
                               float delta_meter, float w_g, float w_d, const void* term_weights, void* dLdp,
                               void* workspace, void* stream);

/* ---- evaluation metrics (forward-only test pass) -------------------------------- */
/* Every metric of the reference's final evaluation (script/train_model.py:366-379; modules at loss_maker.py:194-213,
 * 522-741) from ONE pass over prediction, target and building mask.  p, t: (B,4,Z,Y,X); b: (B,1,Z,Y,X);
 * stds = config['data']['stds'] (temperature scale, then the three velocity scales); `lev` is the z index of the
 * *_LEV entries (the reference uses lev = 0).  out: SR3D_EVAL_COUNT floats in DEVICE memory. */
enum {
  SR3D_EVAL_L1 = 0,                      /* MyL1Loss                      loss_maker.py:194-202 */
  SR3D_EVAL_L2 = 1,                      /* MyL2Loss                      :205-213 */
  SR3D_EVAL_MASKED_L1 = 2,               /* MaskedL1Loss                  :522-536 */
  SR3D_EVAL_MASKED_L2 = 3,               /* MaskedL2Loss                  :539-553 */
  SR3D_EVAL_MASKED_L1_NEAR_WALL = 4,     /* MaskedL1LossNearWall          :556-574 */
  SR3D_EVAL_MASKED_L2_NEAR_WALL = 5,     /* MaskedL2LossNearWall          :577-595 */
  SR3D_EVAL_RESIDUAL_CONTINUITY = 6,     /* ResidualContinuity.forward    :598-615 */
  SR3D_EVAL_RESIDUAL_CONTINUITY_TARGET = 7, /* ... .calc_both_pred_and_target, target part   :617-633 */
  SR3D_EVAL_ABS_DIFF_TEMPERATURE = 8,    /* AbsDiffTemperature            :674-703 */
  SR3D_EVAL_DIFF_VELOCITY_NORM = 9,      /* DiffVelocityVectorNorm        :636-671 */
  SR3D_EVAL_ABS_DIFF_TEMPERATURE_LEV = 10, /* the same two at z == lev */
  SR3D_EVAL_DIFF_VELOCITY_NORM_LEV = 11,
  SR3D_EVAL_ABS_DIFF_DIVERGENCE = 12,    /* AbsDiffDivergence             :706-727 */
  SR3D_EVAL_DIFF_OMEGA_NORM = 13,        /* DiffOmegaVectorNorm           :730-745 */
  SR3D_EVAL_SUM_ABS = 14,                /* raw sums over the 4 channels: sum |p - t|, sum b |p - t|,            */
  SR3D_EVAL_SUM_MASK_ABS = 15,           /* sum (p - t)^2, sum b (p - t)^2 and sum b (one channel) -- what the      */
  SR3D_EVAL_SUM_SQ = 16,                 /* weighted losses (loss_maker.py:216-255) are made of                     */
  SR3D_EVAL_SUM_MASK_SQ = 17,
  SR3D_EVAL_SUM_MASK = 18,
  SR3D_EVAL_COUNT = 19
};
size_t sr3d_eval_metrics_workspace_bytes(int B, int Z, int Y, int X);
int sr3d_eval_metrics(const void* p, const void* t, const void* b, int B, int Z, int Y, int X, const float stds[4],
                      float delta_meter, int lev, void* out, void* workspace, void* stream);

/* ---- height-resolved evaluation: every metric per level from ONE pass ------------ */
/* The formulas of the evaluation modules above restricted to z == k in numerator and denominator alike, for every
 * level k at once (csrc/sr3d_eval_profile.hip): ABS_DIFF_TEMPERATURE / DIFF_VELOCITY_NORM at level k are exactly the
 * reference's AbsDiffTemperature(lev=k) / DiffVelocityVectorNorm(lev=k).  Same inputs as sr3d_eval_metrics.
 * per_sample == 0: sums_out is (SR3D_PROFILE_SUM_COUNT, Z) and values_out (SR3D_PROFILE_COUNT, Z), over the whole
 * batch (what the reference's modules see); per_sample != 0: (B, ., Z), one profile per sample, bit-equal to B
 * one-sample calls.  Both in DEVICE memory, fp32 (sums rounded from double totals).  The interior profiles
 * (RESIDUAL_CONTINUITY .. , ABS_DIFF_DIVERGENCE, DIFF_OMEGA_NORM) divide by sum_int b - sum_int near without eps:
 * NaN where a level has no such voxel, always at levels 0 and Z-1.  No atomics: two calls are bit-equal. */
enum {
  SR3D_PROFILE_SUM_ABS = 0,        /* sum |d| over the 4 channels (d = p - t) */
  SR3D_PROFILE_SUM_SQ = 1,         /* sum d^2 over the 4 channels */
  SR3D_PROFILE_SUM_SQ_T = 2,       /* sum d^2 of channel T; U, V, W follow at 3, 4, 5 */
  SR3D_PROFILE_SUM_SQ_U = 3,
  SR3D_PROFILE_SUM_SQ_V = 4,
  SR3D_PROFILE_SUM_SQ_W = 5,
  SR3D_PROFILE_SUM_MASK = 6,       /* sum b */
  SR3D_PROFILE_SUM_MASK_ABS = 7,   /* sum b |d| */
  SR3D_PROFILE_SUM_MASK_SQ = 8,    /* sum b d^2 */
  SR3D_PROFILE_SUM_NEAR = 9,       /* sum near (near-wall flag of the mask) */
  SR3D_PROFILE_SUM_NEAR_ABS = 10,
  SR3D_PROFILE_SUM_NEAR_SQ = 11,
  SR3D_PROFILE_SUM_MASK_DT = 12,   /* sum b |d_T| std_T */
  SR3D_PROFILE_SUM_MASK_DV = 13,   /* sum b || std_v d_v || */
  SR3D_PROFILE_SUM_MASK_INT = 14,  /* on the interior (1 <= z, y, x <= n - 2), M = b (1 - near): sum b */
  SR3D_PROFILE_SUM_NEAR_INT = 15,  /* sum near */
  SR3D_PROFILE_SUM_RES_P = 16,     /* sum |M div p| */
  SR3D_PROFILE_SUM_RES_T = 17,     /* sum |M div t| */
  SR3D_PROFILE_SUM_DDIV = 18,      /* sum |M div p - M div t| */
  SR3D_PROFILE_SUM_OMEGA = 19,     /* sum || M omega(p) - M omega(t) || */
  SR3D_PROFILE_SUM_COUNT = 20
};
enum {
  SR3D_PROFILE_L1 = 0,             /* over 4 B Y X */
  SR3D_PROFILE_L2 = 1,
  SR3D_PROFILE_MASKED_L1 = 2,      /* / (4 sum b + 1e-30) */
  SR3D_PROFILE_MASKED_L2 = 3,
  SR3D_PROFILE_MASKED_L1_NEAR_WALL = 4,   /* / (4 sum near + 1e-30) */
  SR3D_PROFILE_MASKED_L2_NEAR_WALL = 5,
  SR3D_PROFILE_RESIDUAL_CONTINUITY = 6,   /* / (sum_int b - sum_int near) */
  SR3D_PROFILE_RESIDUAL_CONTINUITY_TARGET = 7,
  SR3D_PROFILE_ABS_DIFF_TEMPERATURE = 8,  /* / (sum b + 1e-30) */
  SR3D_PROFILE_DIFF_VELOCITY_NORM = 9,
  SR3D_PROFILE_ABS_DIFF_DIVERGENCE = 10,
  SR3D_PROFILE_DIFF_OMEGA_NORM = 11,
  SR3D_PROFILE_CHANNELWISE_MSE_T = 12,    /* over B Y X; U, V, W follow at 13, 14, 15 */
  SR3D_PROFILE_CHANNELWISE_MSE_U = 13,
  SR3D_PROFILE_CHANNELWISE_MSE_V = 14,
  SR3D_PROFILE_CHANNELWISE_MSE_W = 15,
  SR3D_PROFILE_COUNT = 16
};
size_t sr3d_eval_level_profiles_workspace_bytes(int B, int Z, int Y, int X);
int sr3d_eval_level_profiles(const void* p, const void* t, const void* b, int B, int Z, int Y, int X,
                             const float stds[4], float delta_meter, int per_sample, void* sums_out, void* values_out,
                             void* workspace, void* stream);

/* ---- wall-distance-resolved evaluation (csrc/sr3d_walldist.hip) ------------------ */
/* Chebyshev distance to the nearest built cell.  b: (B,1,Z,Y,X) fp32; dist_out: (B,1,Z,Y,X) UINT8; 1 <= cap <= 254.
 * A cell with 1.0f - b > 0 gets 0, every other cell min(distance to the nearest such cell of the same sample, cap + 1);
 * nothing is built outside the grid, and a sample with nothing built is cap + 1 everywhere.  The reference's
 * calc_mask_near_build_wall(b, num_filter_applications = n) (loss_maker.py:57-83: n box filters, then > 0) is
 * (dist <= n) & (b > 0) for every n <= cap.  Three launches (one per axis) for any cap; workspace: one byte per voxel. */
size_t sr3d_wall_distance_workspace_bytes(int B, int Z, int Y, int X);
int sr3d_wall_distance(const void* b, void* dist_out, int B, int Z, int Y, int X, int cap, void* workspace,
                       void* stream);

/* Every metric of the evaluation PER DISTANCE CLASS from one pass of the marching stencil.  Same inputs as
 * sr3d_eval_level_profiles plus dist (uint8, made by sr3d_wall_distance with cap >= D), 1 <= D <= 30, whole batch only.
 * Bins: 0 is dist == 0, k = 1 .. D is dist == k, D + 1 is dist > D.  sums_out is (SR3D_WALLDIST_SUM_COUNT, D + 2) and
 * values_out (SR3D_WALLDIST_COUNT, D + 2), fp32 in DEVICE memory, rounded from double totals.  The values are the
 * formulas of SR3D_PROFILE_* restricted to the bin in numerator and denominator alike, except:
 *   L1, L2 divide by 4 CELLS and CHANNELWISE_MSE_* by CELLS (an empty bin gives NaN);
 *   MASKED_L1/L2_NEAR_WALL at bin k are CUMULATIVE: sum_{j<=k} POS_ABS / (4 sum_{j<=k} POS + 1e-30), which is the
 *   reference's MaskedL1LossNearWall(num_filter_applications = k) for k = 1 .. D;
 *   the interior rows keep M = b (1 - near_1) and are NaN where a bin has no such voxel (bins 0 and 1 of a binary mask).
 * No atomics: two calls are bit-equal. */
enum {
  SR3D_WALLDIST_SUM_ABS = 0,        /* 0 .. 8 and 12 .. 19: as SR3D_PROFILE_SUM_*, over the voxels of the bin */
  SR3D_WALLDIST_SUM_SQ = 1,
  SR3D_WALLDIST_SUM_SQ_T = 2,
  SR3D_WALLDIST_SUM_SQ_U = 3,
  SR3D_WALLDIST_SUM_SQ_V = 4,
  SR3D_WALLDIST_SUM_SQ_W = 5,
  SR3D_WALLDIST_SUM_MASK = 6,
  SR3D_WALLDIST_SUM_MASK_ABS = 7,
  SR3D_WALLDIST_SUM_MASK_SQ = 8,
  SR3D_WALLDIST_SUM_POS = 9,        /* sum [b > 0]: the cells the reference's near-wall flag can select */
  SR3D_WALLDIST_SUM_POS_ABS = 10,   /* sum [b > 0] |d| */
  SR3D_WALLDIST_SUM_POS_SQ = 11,    /* sum [b > 0] d^2 */
  SR3D_WALLDIST_SUM_MASK_DT = 12,
  SR3D_WALLDIST_SUM_MASK_DV = 13,
  SR3D_WALLDIST_SUM_MASK_INT = 14,
  SR3D_WALLDIST_SUM_NEAR_INT = 15,
  SR3D_WALLDIST_SUM_RES_P = 16,
  SR3D_WALLDIST_SUM_RES_T = 17,
  SR3D_WALLDIST_SUM_DDIV = 18,
  SR3D_WALLDIST_SUM_OMEGA = 19,
  SR3D_WALLDIST_SUM_CELLS = 20,     /* voxels of the bin */
  SR3D_WALLDIST_SUM_COUNT = 21
};
enum {
  SR3D_WALLDIST_L1 = 0,             /* over 4 CELLS */
  SR3D_WALLDIST_L2 = 1,
  SR3D_WALLDIST_MASKED_L1 = 2,
  SR3D_WALLDIST_MASKED_L2 = 3,
  SR3D_WALLDIST_MASKED_L1_NEAR_WALL = 4,   /* cumulative over the bins 0 .. k */
  SR3D_WALLDIST_MASKED_L2_NEAR_WALL = 5,
  SR3D_WALLDIST_RESIDUAL_CONTINUITY = 6,
  SR3D_WALLDIST_RESIDUAL_CONTINUITY_TARGET = 7,
  SR3D_WALLDIST_ABS_DIFF_TEMPERATURE = 8,
  SR3D_WALLDIST_DIFF_VELOCITY_NORM = 9,
  SR3D_WALLDIST_ABS_DIFF_DIVERGENCE = 10,
  SR3D_WALLDIST_DIFF_OMEGA_NORM = 11,
  SR3D_WALLDIST_CHANNELWISE_MSE_T = 12,    /* over CELLS; U, V, W follow at 13, 14, 15 */
  SR3D_WALLDIST_CHANNELWISE_MSE_U = 13,
  SR3D_WALLDIST_CHANNELWISE_MSE_V = 14,
  SR3D_WALLDIST_CHANNELWISE_MSE_W = 15,
  SR3D_WALLDIST_COUNT = 16
};
#define SR3D_WALLDIST_MAX_D 30
size_t sr3d_eval_wall_distance_profiles_workspace_bytes(int B, int Z, int Y, int X, int D);
int sr3d_eval_wall_distance_profiles(const void* p, const void* t, const void* b, const void* dist, int B, int Z, int Y,
                                     int X, const float stds[4], float delta_meter, int D, void* sums_out,
                                     void* values_out, void* workspace, void* stream);

/* ---- error-distribution evaluation (csrc/sr3d_eval_dist.hip) ---------------------- */
/* Histograms of 13 per-voxel series over the fluid cells (b > 0), split by wall distance, from ONE streaming pass
 * over p, t (B,4,Z,Y,X; fp32, normalised), b (B,1,Z,Y,X) and dist (uint8, made by sr3d_wall_distance with
 * cap >= near_width; or NULL).  Counts are integers: they add exactly over batches and ranks, and every quantile and
 * PDF distance follows from them.
 * Series: ERR_c = p_c - t_c (signed, normalised); ERR_VEL_NORM = sqrtf((a*a + b*b) + c*c) with a = stds[1] * ERR_U,
 *   b = stds[2] * ERR_V, c = stds[3] * ERR_W, every product and sum rounded to fp32 (the integrand of
 *   DiffVelocityVectorNorm); PRED_c = p_c, TRUTH_c = t_c.
 * Classes: 0 = fluid cells with dist <= near_width (the reference's calc_mask_near_build_wall(b, near_width)), 1 = the
 *   other fluid cells; dist == NULL: every fluid cell is class 1 and near_width is ignored (else 0 <= near_width <= 254).
 * Slots: 0 underflow, 1 .. 256 the bins, 257 overflow, 258 NaN.  The binning rule of series s is, by definition,
 *     inv = (float)(256.0 / ((double)hi[s] - (double)lo[s]))      on the host
 *     k   = floorf((v - lo[s]) * inv)                             fp32: difference and product each rounded, no fma
 *   k < 0 or v == -inf: underflow; k >= 256 or v == +inf: overflow; NaN: the NaN slot; else slot 1 + k.  Bins are
 *   left-closed: bin k holds what the rule sends to k, about [lo + k w, lo + (k + 1) w) with w = (hi - lo) / 256.
 *   hi <= lo, a non-finite bound or a non-finite inv is SR3D_E_ARG.
 * Outputs (DEVICE): counts_out int64 (SR3D_DIST_SERIES, SR3D_DIST_CLASSES, SR3D_DIST_SLOTS); minmax_out fp32
 *   (SR3D_DIST_SERIES, SR3D_DIST_CLASSES, 2): exact min and max of the non-NaN values (+inf / -inf for an empty class);
 *   cells_out int64 (3): built (not b > 0), near, far cells.  per_sample != 0: each gets a leading B, bit-equal to B
 *   one-sample calls.  Every word of the outputs, and every word of the workspace that is read, is written by the
 *   call's own kernels: nothing has to be cleared beforehand and a captured call replays faithfully.  Integer sums and
 *   min / max in a fixed order, no global atomics: two calls are bit-equal.  p, t, b may be any 4-byte-aligned
 *   contiguous tensors (16-byte loads are used where every channel plane is 16-byte aligned).  Z*Y*X < 2^31, B <= 65535. */
enum {
  SR3D_DIST_ERR_T = 0,
  SR3D_DIST_ERR_U = 1,
  SR3D_DIST_ERR_V = 2,
  SR3D_DIST_ERR_W = 3,
  SR3D_DIST_ERR_VEL_NORM = 4,
  SR3D_DIST_PRED_T = 5,
  SR3D_DIST_PRED_U = 6,
  SR3D_DIST_PRED_V = 7,
  SR3D_DIST_PRED_W = 8,
  SR3D_DIST_TRUTH_T = 9,
  SR3D_DIST_TRUTH_U = 10,
  SR3D_DIST_TRUTH_V = 11,
  SR3D_DIST_TRUTH_W = 12
};
#define SR3D_DIST_SERIES 13
#define SR3D_DIST_CLASSES 2
#define SR3D_DIST_BINS 256
#define SR3D_DIST_SLOTS 259
size_t sr3d_eval_distributions_workspace_bytes(int B, int Z, int Y, int X);
int sr3d_eval_distributions(const void* p, const void* t, const void* b, const void* dist /* uint8 or NULL */,
                            int B, int Z, int Y, int X, const float stds[4],
                            const float lo[SR3D_DIST_SERIES], const float hi[SR3D_DIST_SERIES],
                            int near_width, int per_sample,
                            void* counts_out, void* minmax_out, void* cells_out,
                            void* workspace, void* stream);

/* ---- scale-resolved evaluation (csrc/sr3d_eval_scale.hip) -------------------------- */
/* Two-point moments over the valid fluid pairs (x, x + r e_d): the raw sums behind structure functions, increment
 * skewness and flatness and the two-point correlation of the prediction, the truth and the error, per sample, level,
 * direction d (0 = x, 1 = y, 2 = z) and lag r = 1 .. R.  The building-aware stand-in for a spectrum.
 * Inputs: p, t (B,4,Z,Y,X; fp32, normalised), b (B,1,Z,Y,X).  A cell is fluid iff b > 0 (as sr3d_eval_distributions).
 * Pairs: (x, x + r e_d) is valid iff both cells are inside the volume and fluid; with unobstructed != 0 every cell
 *   between them along d must be fluid too (pairs through a building are dropped).  The pair belongs to the level z of
 *   its first cell x (d = z: the lower one).  A lag >= the axis length has no pairs: that is no error.
 * Series: f = (double)p_c (SR3D_SCALE_PRED_T + c), (double)t_c (SR3D_SCALE_TRUTH_T + c) or e_c = (double)p_c -
 *   (double)t_c (SR3D_SCALE_ERR_T + c), c = 0 .. 3 (T, u, v, w).
 * Moments, each summed over the valid pairs, with delta = f(x + r e_d) - f(x) in fp64:
 *   D1 .. D4 = sum delta, delta^2, delta^3, delta^4;  F0 = sum f(x), F1 = sum f(x + r e_d);  FF0 = sum f(x)^2,
 *   FF1 = sum f(x + r e_d)^2.  Products and sums are fp64, in the implementation's order; an entry with no pairs is
 *   exactly 0.  What is not stored follows on the host: sum f f' = (FF0 + FF1 - D2) / 2 and
 *   sum delta_p delta_t = (D2_pred + D2_truth - D2_err) / 2.
 * The value of a cell that is part of no valid pair never reaches a sum (it is selected out, not multiplied by 0): a
 *   NaN in a built cell changes nothing.  A NaN in a fluid cell propagates to the sums the cell belongs to.
 * Outputs (DEVICE): sums_out fp64 (B, Z, SR3D_SCALE_DIRS, R, SR3D_SCALE_SERIES, SR3D_SCALE_MOMENTS); pairs_out int64
 *   (B, Z, SR3D_SCALE_DIRS, R): the number of valid pairs.  Sample i of a B-sample call is bit-equal to the one-sample
 *   call on it.  Every word of both outputs, and every word of the workspace that is read, is written by the call's own
 *   kernels: nothing has to be cleared beforehand and a captured call replays faithfully.  Fixed reduction order, no
 *   global atomics: two calls are bit-equal.  p, t, b 4-byte aligned, the outputs 8-byte aligned.
 * SR3D_E_ARG, before anything is launched: R < 1 or R > SR3D_SCALE_MAX_LAG, a null pointer (the workspace included,
 *   under either pair rule), a non-positive dimension, Z*Y*X >= 2^31, B > 65535. */
enum {
  SR3D_SCALE_PRED_T = 0,     /* PRED_U, V, W follow at 1, 2, 3 */
  SR3D_SCALE_TRUTH_T = 4,    /* TRUTH_U, V, W at 5, 6, 7 */
  SR3D_SCALE_ERR_T = 8       /* ERR_U, V, W at 9, 10, 11 */
};
enum {
  SR3D_SCALE_MOMENT_D1 = 0,
  SR3D_SCALE_MOMENT_D2 = 1,
  SR3D_SCALE_MOMENT_D3 = 2,
  SR3D_SCALE_MOMENT_D4 = 3,
  SR3D_SCALE_MOMENT_F0 = 4,
  SR3D_SCALE_MOMENT_F1 = 5,
  SR3D_SCALE_MOMENT_FF0 = 6,
  SR3D_SCALE_MOMENT_FF1 = 7
};
#define SR3D_SCALE_MAX_LAG 64
#define SR3D_SCALE_SERIES 12
#define SR3D_SCALE_MOMENTS 8
#define SR3D_SCALE_DIRS 3
size_t sr3d_eval_scale_statistics_workspace_bytes(int B, int Z, int Y, int X, int R);
int sr3d_eval_scale_statistics(const void* p, const void* t, const void* b, int B, int Z, int Y, int X,
                               int R, int unobstructed,
                               void* sums_out  /* fp64 (B, Z, 3, R, 12, 8) */,
                               void* pairs_out /* int64 (B, Z, 3, R) */,
                               void* workspace, void* stream);

/* Rotation about the vertical axis (reference src/equivariance_error_calculator.py): every (y, x) plane of an NCDHW
 * fp32 tensor rotated as scipy.ndimage.rotate(a, angle_deg, axes=(-2, -1), reshape=False) does it -- cubic B-spline
 * (prefilter with the mirror boundary, fp64 coefficients), mode 'constant', cval = 0.  angle_deg is reduced modulo
 * 360 on the host, with exact cos / sin at multiples of 90 degrees (scipy.special.cosdg / sindg).
 * The workspace (sr3d_rotate_workspace_bytes of the rotated tensor's shape; C = 4 for sr3d_equivariance_errors)
 * starts with the tensor's fp64 spline coefficients.  flags:
 *   SR3D_ROTATE_COEF_READY  the workspace already holds the coefficients of THIS input (an earlier call on the same
 *                           tensor and workspace, any angle): the prefilter is skipped -- an angle sweep pays it once;
 *   SR3D_ROTATE_PHYSICAL    sr3d_rotate_fields only: return the physical field (rescaled = False), no clip. */
enum { SR3D_ROTATE_COEF_READY = 1, SR3D_ROTATE_PHYSICAL = 2 };
size_t sr3d_rotate_workspace_bytes(int B, int C, int Z, int Y, int X);
/* rotate_temperature_velocity (equivariance_error_calculator.py:6-46): x (B, 4, Z, Y, X) normalised fields (T, u, v,
 * w); HOST means[4], scales[4].  y = clip((Q @ rotate(x * scales + means) - means) / scales, 0, 1), Q mixing channels
 * 1 and 2 by (cos, sin; -sin, cos) -- the velocity rotated as a vector.  C must be 4. */
int sr3d_rotate_fields(const void* x, void* y, int B, int C, int Z, int Y, int X, const double means[4],
                       const double scales[4], double angle_deg, int flags, void* workspace, size_t workspace_bytes,
                       void* stream);
/* rotate_building_height (:49-60): y = (float32(rotate(b)) > float32(th)) ? 1 : 0, any C */
int sr3d_rotate_building(const void* b, void* y, int B, int C, int Z, int Y, int X, double angle_deg, double th,
                         int flags, void* workspace, size_t workspace_bytes, void* stream);
/* calc_preds_for_equivariance_errors + calc_equivariance_errors (:63-158) after the two forwards: preds and
 * preds_after_rot (B, 4, Z, Y, X); R = scales * rotate_fields(preds) + means, A = scales * preds_after_rot + means;
 * out (3 doubles, DEVICE) = means over [:, sy:ey, sx:ex] of |R_T - A_T|, |R_w - A_w| and ||(R_u, R_v) - (A_u, A_v)||
 * (keys tm, vr, vl_vp), reduced deterministically in fp64.  The window bounds follow Python slices (negative = from
 * the end); an empty window or one outside the plane is SR3D_E_ARG. */
int sr3d_equivariance_errors(const void* preds, const void* preds_after_rot, int B, int Z, int Y, int X,
                             const double means[4], const double scales[4], double angle_deg, int sy, int ey, int sx,
                             int ex, int flags, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* Near-surface (2 m) temperature (reference notebook make_2m_temperature: infer_2m_height_temperature, with the
 * prediction dimensionalised as make_inference does).  A source is one channel of an NCDHW fp32 tensor, read in
 * place: src[b, channel, k, y, x] for k < levels.  tz: (Y, X) fp64 building / ground top heights (DEVICE; the
 * transpose of read_building_height's (i = x, j = y) array); heights: HOST, nheights (<= 128) strictly increasing
 * fp64 level heights H[k] (reference: k * 5 + 17.5).  Per column, Z = levels: NaN if tz > H[Z-1]; first = 0 if
 * !(tz > H[0]), else the first k with H[k] >= tz; t1 if first == Z-1; else, with t1, t2 the levels first, first + 1,
 * float(double(t1) + ((tz - H[first]) * double(t2 - t1)) / (H[first+1] - H[first])) -- numpy >= 2's rounding of
 * the notebook's expression (t2 - t1 in fp32, the rest in fp64).  affine != 0: every value read is first mapped to
 * (v * scale) + mean, each step rounded to fp32 (torch's `data * scales + means`).  No alignment requirement. */
typedef struct {
  const void* data;     /* (B, C, Zs, Y, X) fp32, dense */
  int32_t C, Zs;
  int32_t channel;      /* 0 <= channel < C */
  int32_t levels;       /* 1 <= levels <= Zs, and <= nheights */
  int32_t affine;
  float scale, mean;
} sr3d_surface_src_t;
/* the map alone: out (B, Y, X) fp32 */
int sr3d_surface_temperature(const sr3d_surface_src_t* src, int B, int Y, int X, const void* tz,
                             const double* heights, int nheights, void* out, void* stream);
/* workspace of sr3d_surface_temperature_errors: a ticket word, then one fp64 partial triple per workgroup.  The
 * ticket must be ZERO before the first call (allocate the workspace zeroed); every call leaves it zero. */
size_t sr3d_surface_temperature_workspace_bytes(int B, int Y, int X);
/* prediction and truth in ONE launch (each with its own C, Zs, channel, levels, affine; one B, Y, X, tz, heights):
 * both maps (pred_out, truth_out: (B, Y, X) fp32, each may be NULL), and acc (3 doubles, DEVICE) += (sum (p - t)^2,
 * sum |p - t|, count) over the columns where both maps are finite, differences in fp64.  Deterministic: per sample a
 * fixed-order sum, the samples added to acc in order -- two calls on two batches equal one call on both. */
int sr3d_surface_temperature_errors(const sr3d_surface_src_t* pred, const sr3d_surface_src_t* truth, int B, int Y,
                                    int X, const void* tz, const double* heights, int nheights, void* pred_out,
                                    void* truth_out, void* acc, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* LR training data from one HR time step, building-aware (reference datascience/: training_data_maker.make_coarse_
 * grained_dataarray_with_outside_lr_buildings and the script make_dl_data_using_outside_lr_builds, SR_SCALE 4).
 * Per channel, a cell is valid when hr_mask is 0 there, the value is not NaN and (align_nan, channel > 0) channel 0
 * is not NaN there.  Invalid cells are filled as xarray's interpolate_na(method="nearest", fill_value="extrapolate")
 * along lev, then lat, then lon does (scipy interp1d: ties to the lower coordinate, edge values past the ends); cells
 * z < lr_tops[0][y/4][x/4] then become NaN; each 4x4x4 block is the fp64 mean of its 64 cells, summed in numpy's
 * pairwise order, rounded once to fp32, NaN if any cell is NaN; LR levels kz < lr_tops[1][Y/4][X/4] are NaN.
 *   hr_out = raw with invalid cells NaN, the window [m, Y-m) x [m, X-m):     (C, Z, Y-2m, X-2m) fp32, dense
 *   lr_out = the blocks of that window:                                      (C, Z/4, (Y-2m)/4, (X-2m)/4) fp32, dense
 * Coordinates must increase strictly; NULL gives index coordinates.  Z <= 128; Z, Y, X, hr_margin multiples of 4.
 * Three launches on `stream` (workspace init, column map, main pass), no host synchronisation. */
typedef struct {
  const void* raw;            /* (C, Z, Y, X) fp32: channel c at raw + c * channel_stride floats, each (Z, Y, X) dense */
  long long channel_stride;   /* >= Z * Y * X */
  int32_t C, Z, Y, X;
  int32_t scale;              /* must be 4 */
  int32_t hr_margin;          /* m: lateral cells cut from each edge of both outputs */
  int32_t align_nan;          /* channels > 0 are invalid where channel 0 is NaN (reference align_nan_grids) */
  const void* hr_mask;        /* (Z, Y, X) uint8, non-zero = masked */
  const void* lr_tops;        /* (2, Y/4, X/4) int32: masked HR levels, masked LR levels per LR column */
  const double* lat;          /* DEVICE (Y) fp64 or NULL */
  const double* lon;          /* DEVICE (X) fp64 or NULL */
  const double* lev;          /* HOST (Z) fp64 or NULL */
  void* hr_out;
  void* lr_out;
} sr3d_lrdata_params_t;
size_t sr3d_lrdata_workspace_bytes(int C, int Y, int X);
int sr3d_lrdata(const sr3d_lrdata_params_t* params, void* workspace, size_t workspace_bytes, void* stream);

/* One time step of the LES's GrADS output, decoded on the device (reference datascience/: io_grads.read_xarray +
 * align_nan_grids, without xgrads / xarray): four variables (tm, vl, vp, vr), each given as the raw bytes of the
 * step's level window exactly as they lie in the data file.  Variable v, output level z, row y, column x reads the
 * 4-byte word at
 *   src[v] + level_offset[v] + (zrev ? Z-1-z : z) * level_pitch[v] + ((yrev ? Y-1-y : y) * X + x) * 4
 * (level_pitch carries the two 4-byte record markers of `options sequential`), swaps its bytes if `byteswap`,
 * compares it as fp32 with (float)undef[v] (numpy's `da == ds.undef` on a float32 array): equal -> NaN, a NaN in the
 * file stays NaN; with align_nan, variables 1..3 are NaN wherever variable 0 is.  out: (4, Z, Y, X) fp32 dense, bit
 * identical to that numpy expression; tm_is_nan (optional): (Z, Y, X) uint8, 1 where out[0] is NaN.
 * 16-byte loads and stores when X % 4 == 0 and every slab base and pitch keeps 16-byte alignment, 4-byte ones
 * otherwise.  One launch on `stream`, no host synchronisation, no workspace. */
typedef struct {
  int32_t X, Y, Z;
  int32_t byteswap;           /* the file's byte order is not the host's (little endian) */
  int32_t yrev, zrev;         /* the file stores rows / levels in descending order */
  int32_t align_nan;
  long long level_offset[4];  /* bytes from src[v] to the first value of file level 0; a multiple of 4 */
  long long level_pitch[4];   /* bytes between level slabs, >= Y * X * 4; a multiple of 4 */
  long long src_bytes[4];     /* size of src[v]: level_offset + (Z-1) * level_pitch + Y * X * 4 must fit */
  double undef[4];
  void* out;
  void* tm_is_nan;            /* or NULL */
} sr3d_grads_params_t;
int sr3d_grads_decode(const void* const src[4], const sr3d_grads_params_t* params, void* stream);

/* The interpolation baseline of the reference's plotting notebooks (`fill_na`, pytorch/notebook/plot_horizontal_
 * sections_at_various_locations.ipynb and plot_horizontal_vertical_section_at_fixed_location.ipynb, cell "Define
 * methods"): lr (B, C, z, y, x) fp32, sample b / channel c at lr + b * batch_stride + c * channel_stride floats, each
 * (z, y, x) volume dense, NaN allowed; lr_is_in_build (mz, my, mx) uint8, which must be the LR grid, shared by every
 * sample and channel; scale s = 2 or 4.
 *   1. F.interpolate(mode="trilinear", align_corners=False, scale_factor=s): per axis src = max(0, (dst + 0.5) / s -
 *      0.5), i0 = floor(src), i1 = min(i0 + 1, n - 1), l1 = src - i0, l0 = 1 - l1; the value is wz0 * (wy0 * (wx0 *
 *      v000 + wx1 * v001) + wy1 * (..)) + wz1 * (..) in fp32, each w0 * a + w1 * b evaluated as fma(a, w0, fl(w1 * b))
 *      and nothing else contracted: the rounding of ATen's CPU kernel for contiguous tensors;
 *   2. a cell is NaN where lr_is_in_build[z / s][y / s][x / s] != 0 (a NaN of step 1 stays);
 *   3. along z, then y, then x, each pass on the result of the one before: a line with k NaN cells out of n is left
 *      alone if k == 0 or k >= n - 1; otherwise each NaN cell i becomes float((double(y_hi) - double(y_lo)) / (hi - lo)
 *      * (i - lo) + double(y_lo)), (lo, hi) the valid cells around i, or the two nearest valid cells past an end
 *      (scipy interp1d(kind="linear", fill_value="extrapolate") on index coordinates).  Valid cells are never rewritten.
 * out: (B, C, s*z, s*y, s*x) fp32 dense (16-byte stores when s*x % 4 == 0 and out is 16-byte aligned, 4-byte stores
 * otherwise); n_unfilled: one int32 (DEVICE) = the number of cells still NaN at the end.  dtype must be
 * SR3D_DTYPE_F32; lr, out, n_unfilled and workspace must be 4-byte aligned.  Five launches on `stream` (two that zero
 * the flags and the count, the column pass, the y and x fills), no host synchronisation; results do not depend on
 * scheduling. */
size_t sr3d_interp_baseline_workspace_bytes(int B, int C, int z, int y, int x, int scale);
int sr3d_interp_baseline(const void* lr, long long batch_stride, long long channel_stride, int dtype, int B, int C,
                         int z, int y, int x, const void* lr_is_in_build, int mz, int my, int mx, int scale, void* out,
                         void* n_unfilled, void* workspace, size_t workspace_bytes, void* stream);

/* SSIM3D (reference src/ssim.py:52-115: masked structural similarity with a w x w x w Gaussian or uniform window,
 * zero padding).  img1, img2: (B, C, Z, Y, X); mask: (B, Cm, Z, Y, X) with Cm = 1 or C; `window`: the n 1-D taps
 * (HOST array, n odd, <= 15) whose triple outer product is the reference's 3-D window; mean_out: 1 float (device) =
 * mean of the SSIM map; ssim_map (optional): the map itself (size_average = False). */
size_t sr3d_ssim3d_workspace_bytes(int B, int C, int Z, int Y, int X);
int sr3d_ssim3d(const void* img1, const void* img2, const void* mask, int B, int C, int Cm, int Z, int Y, int X,
                const float* window, int n, float max_val, float eps, void* mean_out, void* ssim_map, void* workspace,
                void* stream);

/* ---- optimizer -------------------------------------------------------------- */
/* torch.optim.Adam defaults (train_model.py:183) on one flat fp32 buffer; step is 1-based.  The
 * hyper-parameters are doubles, as in torch (1 - beta2 must be formed in double to match it). */
int sr3d_adam_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, long long n, double lr,
                   double beta1, double beta2, double eps, int step, double grad_scale, void* stream);

/* The same update with the step number kept in DEVICE memory: `step_counter` (int32, device) is incremented by the call
 * itself and the bias corrections are derived from it on the device (`scalars`: 2 floats of device scratch), so a
 * training step captured into a hipGraph advances correctly on every replay (the host-side `step` of sr3d_adam_step
 * would be frozen into the graph). */
int sr3d_adam_step_device_counter(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, long long n, double lr,
                                  double beta1, double beta2, double eps, void* step_counter, void* scalars,
                                  double grad_scale, void* stream);

/* ---- measurement hook (bench.py's roofline leg; no reference counterpart) --------
 * When enabled, every launch of the kernels below is bracketed by two HIP events (taken from a pool that
 * sr3d_profile_enable(1) creates, so nothing is allocated inside a timed region) on the stream it is launched on.
 * sr3d_profile_read() returns, for one kernel family, the summed event time, the summed ALGORITHMIC work and the
 * number of launches since the last enable.  Work = FLOPs (2 * 27 * Cin * Cout * output voxels, padding not counted)
 * for the convolution families, BYTES (compulsory reads + writes of the operation) for the HBM-bound families. */
enum {
  SR3D_PROF_IGEMM_S1 = 0,     /* stride-1 conv forward and stride-1 input gradient           [FLOP] */
  SR3D_PROF_IGEMM_S2 = 1,     /* stride-2 conv forward                                       [FLOP] */
  SR3D_PROF_IGEMM_BWD_S2 = 2, /* stride-2 input gradient (8 parity classes)                  [FLOP] */
  SR3D_PROF_WGRAD = 3,        /* weight gradient (main kernel, without the slab reduce)      [FLOP] */
  SR3D_PROF_LOSS = 4,         /* L1 / mixed loss: value + dL/dp (all passes)                 [byte] */
  SR3D_PROF_ACT_BWD = 5,      /* gated / LeakyReLU / unshuffle activation backward           [byte] */
  SR3D_PROF_BIAS_GRAD = 6,    /* bias gradient (both stages)                                 [byte] */
  SR3D_PROF_ADAM = 7,         /* fused Adam                                                  [byte] */
  SR3D_PROF_DATA = 8,         /* upsample+concat, mask pyramid, near-wall mask               [byte] */
  SR3D_PROF_PACK = 9,         /* weight packing / transforms and split-K reductions          [byte] */
  SR3D_PROF_EVAL = 10,        /* fused evaluation metrics                                    [byte] */
  SR3D_PROF_HCONV = 11,       /* stride-1 conv on the split-f16 kernel (SR3D_SPLIT_F16=1): launches of at least 448
                                 workgroups, which fill the chip's 512 slots                                  [FLOP] */
  SR3D_PROF_HCONV_SMALL = 12, /* ... its launches below that (U-Net levels 3-4: small grids, one partial round) [FLOP] */
  SR3D_PROF_FAMILIES = 13,
  SR3D_PROF_DROPPED = 99      /* launches: records lost because the event pool was exhausted */
};
/* on = 1: every family; on = 2: only the stride-1 convolution families (SR3D_PROF_HCONV, SR3D_PROF_HCONV_SMALL, SR3D_PROF_IGEMM_S1): bench.py
 * brackets only the dominant kernel inside its timed region (48 instead of ~1100 event records per training step) and
 * collects the other families in a separate, untimed pass; on = 0: off. */
int sr3d_profile_enable(int on);
int sr3d_profile_read(int kernel_id, double* ms, double* work, long long* launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SR3D_H_ */
