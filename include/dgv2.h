/*
 * dgv2.h -- C ABI of libdgv2.so, the MI355X (gfx950) native kernels behind the
 * dusty_v2 G+D training hot path.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory;
 *   - the CALLER allocates every output (so buffers can come from the host
 *     framework's caching allocator and launches stay hipGraph-capturable);
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*);
 *     nothing here allocates, synchronises or keeps mutable global state, so
 *     entry points are re-entrant from the autograd thread;
 *   - return value: 0 on success, a hipError_t value if the launch failed,
 *     DGV2_EINVAL (-1) for invalid arguments;
 *   - dtype: DGV2_F32 = 0, DGV2_BF16 = 1 (bf16 storage, fp32 accumulate);
 *   - activations are channels-last: [B, H, W, C] ("pixels x channels").
 *
 * Each declaration cites the reference interface it replaces (paths relative to
 * the reference tree kazuto1011/dusty-gan-v2).
 */
#ifndef DGV2_H
#define DGV2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGV2_F32 0
#define DGV2_BF16 1
#define DGV2_FP8 2 /* OCP e4m3fn bytes; only where an entry says so (the *_fp8 / *_q8 entries) */
#define DGV2_F16 3 /* IEEE half; only where an entry says so (the dgv2_seg_loss_* entries: AMP's fp16 logits; dgv2_fire_fwd; dgv2_cam_fwd; the dgv2_bn_* entries) */
#define DGV2_EINVAL (-1)
#define DGV2_ENOTSUP (-3) /* valid request that this build's kernels do not cover: use the documented fallback */

/* Status words.  A few entries check a promise of the caller on the values they stage (dgv2_conv3x3_x3_fwd /
 * dgv2_conv3x3_x3_wgrad: `x_exact`; dgv2_fir_same_mfma_prep: the table contract).  A breach cannot be a return code
 * (the launch is asynchronous), and the library keeps no flag of its own: such entries take `int* status`, a device
 * int32 the CALLER owns (zero-initialised once), and OR one of the bits below into it.  The caller reads the word
 * whenever it synchronises anyway (gans.trainer.Trainer: scalar sync, validation, checkpoint; native.status_check). */
#define DGV2_STATUS_X_INEXACT 1 /* a value outside an x_exact promise was staged: that launch computed on its bf16 rounding */
#define DGV2_STATUS_FIR_TABLE 2 /* dgv2_fir_same_mfma_prep met a table entry outside its contract: the bands are unusable */

/* Library/ABI version; bumped when a signature changes. */
int dgv2_abi_version(void);

/* Workspaces.  Where the library sizes a kernel's workspace, the kernel entry <entry> has ONE host-only sibling
 * <entry>_scratch(int64_t* elems, ...) (named without the entry's variant suffix: _ld, _pl, _skip, _forward).  It takes
 * the geometry / dtype arguments of <entry> the size depends on, in that entry's order, launches nothing, and writes the
 * fp32 ELEMENTS of the whole workspace (an entry that counts another unit says so).  It returns DGV2_ENOTSUP where
 * <entry> refuses that geometry -- "use the documented fallback" -- and DGV2_EINVAL for bad arguments; a sibling sees
 * only its own arguments, so <entry> may still refuse what depends on the others.  <entry> takes the buffer as
 * `scratch, scratch_elems` and returns DGV2_EINVAL when it is too small.  Both call one plan function, so each size is
 * written once.  Below, "scratch: <entry>_scratch elements" means this.
 * (Capacities the CALLER chooses -- splits of dgv2_gemm_x3, the sumsq_cap partial buffers, the rows of
 * dgv2_bias_act_bwd_rs -- are not workspaces in this sense.) */

/* ---------------------------------------------------------------------------
 * fused bias + activation
 * replaces: fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 *   gans/models/ops/fused_act/fused_bias_act.cpp:18-32,
 *   gans/models/ops/fused_act/fused_bias_act_kernel.cu:19-105
 * act: 1 = linear, 3 = leaky-ReLU.  grad: 0 = forward, 1 = first derivative
 * (uses `ref` = forward OUTPUT), 2 = second derivative (zero).
 * bias index = (i / step_b) % size_b; bias/ref may be NULL (= "empty tensor").
 * ------------------------------------------------------------------------- */
int dgv2_fused_bias_act(void* y, const void* x, const void* bias, const void* ref,
                        int64_t size_x, int64_t step_b, int64_t size_b,
                        int act, int grad, float alpha, float scale, int dtype, void* stream);

/* Per-channel sum over everything else: gb[c] = sum_i x[i] with c = (i/step_b)%size_b.
 * replaces: grad_input.sum(dim) in FusedLeakyReLUFunctionBackward.forward
 *   (gans/models/ops/fused_act/fused_act.py:33-45).  gb is fp32 [size_b], overwritten. */
int dgv2_bias_grad(float* gb, const void* x, int64_t size_x, int64_t step_b, int64_t size_b,
                   int dtype, void* stream);

/* Fused backward of bias + leaky-ReLU for channels-last activations: one pass produces
 * gx = (ref > 0 ? gy : alpha*gy) * scale and gb[c] = sum_rows gx[:,c] (fp32 [C]).
 * replaces: FusedLeakyReLUFunctionBackward.forward (act kernel + grad_input.sum), fused_act.py:22-45.
 * Returns DGV2_EINVAL for shapes it does not cover (C % vec != 0 or (C/vec) not dividing 256);
 * callers then use dgv2_fused_bias_act(grad=1) + dgv2_bias_grad. */
/* scratch (optional fp32 [>= 2048*C]): many-block mode with a partial-sum reduce instead of atomics. */
/* row_scale (fp32 [C], NULL = none): an optional per-channel factor on the STORED gradient only (gb sums the unscaled
 * one): backward of y = act(acc * row_scale[c] + b[c]) with respect to acc. */
int dgv2_bias_act_bwd_rs(void* gx, float* gb, const void* gy, const void* ref, int64_t rows, int C,
                         float alpha, float scale, const float* row_scale, float* scratch,
                         int64_t scratch_elems, int dtype, void* stream);
/* y[i] = (ydtype)(x[i] * row_scale[i % C]): the same for activation-free layers (the output heads). */
int dgv2_scale_cast(void* y, const void* x, const float* row_scale, int64_t n, int C, int xdtype, int ydtype,
                    void* stream);

/* ---------------------------------------------------------------------------
 * upfirdn2d
 * replaces: upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel[kh,kw],
 *   up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
 *   gans/models/ops/upfirdn2d/upfirdn2d.cpp:17-31, upfirdn2d_kernel.cu:44-425
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y (same for w);
 * out is [major, out_h, out_w, minor], caller-allocated.  kernel is fp32.
 * ------------------------------------------------------------------------- */
int dgv2_upfirdn2d(void* out, const void* in, const float* kernel,
                   int major, int in_h, int in_w, int minor, int kh, int kw,
                   int up_x, int up_y, int down_x, int down_y,
                   int pad_x0, int pad_x1, int pad_y0, int pad_y1, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * ring-aware separable FIR resampler (channels-last)
 * replaces: Resample.forward, gans/models/ops/common.py:105-135 (zero-insert +
 *   F.pad + depthwise F.conv2d) and its autograd transpose.
 * Per axis: out[n] = sum_i taps[i] * z[n*down + i - p0], z = zero-stuffed (x up)
 * extension of the input; W extends circularly if ring else by replication, H by
 * replication.  taps_h / taps_w: fp32 [kh] / [kw] (k <= 8; k = 1 with tap 1.0 = identity axis).
 * adjoint = 0: forward, x [B,H,W,C] -> y [B,Ho,Wo,C];
 * adjoint = 1: transpose, x is [B,Ho,Wo,C] (a gradient) -> y [B,H,W,C].
 * H, W are always the forward INPUT size, Ho, Wo the forward OUTPUT size.
 * y may be a channel slice of a wider tensor: ldy = channel stride (elements) of y
 * per pixel, ldx likewise for x (pass C for dense).
 * ------------------------------------------------------------------------- */
int dgv2_resample(void* y, const void* x, const float* taps_h, const float* taps_w,
                  int B, int H, int W, int C, int Ho, int Wo, int ldx, int ldy,
                  int kh, int up_h, int down_h, int p0_h,
                  int kw, int up_w, int down_w, int p0_w,
                  int ring, int adjoint, int dtype, void* stream);

/* Table-driven form of the same operator (the hot-path entry): per axis the sparse rows of the
 * resampling matrix, built once on the host per (spec, size, direction): idx/coef [n_out, E]
 * row-major, cnt [n_out] valid entries per row.  y[b,ho,wo,:] = sum_a sum_c coef_h[ho,a] *
 * coef_w[wo,c] * x[b, idx_h[ho,a], idx_w[wo,c], :].  Same reference lines as dgv2_resample.
 * It can also leave the sum of squares of what it wrote (the next modulated conv's input statistic, ModConv2d.forward
 * style.py:98-103: x.square().mean() for the EMA) as per-block partials, saving a separate pass over the activation:
 * sumsq fp32 [sumsq_cap] device buffer (NULL with sumsq_cap = 0 and sumsq_used = NULL: the plain resampler, nothing
 * else is written); *sumsq_used (host) = number of partials written, 0 when this launch configuration cannot provide
 * them (the caller then runs dgv2_sum_squares).  Partials feed dgv2_ema_scalar(sumsq, nsum = *sumsq_used). */
int dgv2_resample_tab_sq(void* y, const void* x, const int* idx_h, const float* coef_h, const int* cnt_h,
                         int Eh, const int* idx_w, const float* coef_w, const int* cnt_w, int Ew,
                         int B, int C, int ldx, int ldy, int in_h, int in_w, int out_h, int out_w,
                         int dtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);

/* y = resid + dgv2_resample_tab_sq(x) for packed few-channel images (C in {1, 2, 4}, ld = C; y, x, resid of `dtype`):
 * `o + self.resample(skip)` of SynthesisBlock.forward (dusty_v2.py:179-180) in one launch, bit-equal to the two-launch
 * form.  DGV2_ENOTSUP for other channel counts / misaligned pointers.
 * rscale / rbias (fp32 [C], both or neither; NULL = resid enters as it is): resid enters as rscale[c] * resid + rbias[c],
 * `c * heads(x) + bias` of Head.forward (dusty_v2.py:30-57) formed in the same store when the heads' contraction left
 * conv2's epilogue (dgv2_modconv_pe_fwd_head). */
int dgv2_resample_tab_add_affine(void* y, const void* x, const void* resid, const float* rscale, const float* rbias,
                                 const int* idx_h, const float* coef_h, const int* cnt_h, int Eh, const int* idx_w,
                                 const float* coef_w, const int* cnt_w, int Ew, int B, int C, int in_h, int in_w, int out_h,
                                 int out_w, int dtype, void* stream);

/* Resampling (normally the ADJOINT tables of a blur/down) followed by the backward of a fused bias + leaky-ReLU in the
 * same pass:  y = R(x) * (ref > 0 ? 1 : alpha) * scale,  gb[c] = sum of the stored y over everything but the channel.
 * ref = forward OUTPUT of the activation, [B, out_h, out_w, C] contiguous like y; gb fp32 [C].
 * scratch: dgv2_resample_tab_actbwd_scratch elements.  DGV2_ENOTSUP when the streaming kernel does not cover the
 * geometry (then: dgv2_resample_tab_sq + dgv2_bias_act_bwd_rs).
 * replaces: Resample adjoint (common.py:105-135) + FusedLeakyReLUFunctionBackward (fused_act.py:22-45) of the
 * discriminator's conv1 -> activation -> blur/down chain (dusty_v2.py:325-345) run backwards. */
int dgv2_resample_tab_actbwd_scratch(int64_t* elems, int B, int C, int out_h, int out_w, int Eh, int dtype);
int dgv2_resample_tab_actbwd(void* y, float* gb, float* scratch, int64_t scratch_elems, const void* x, const void* ref,
                             const int* idx_h, const float* coef_h, const int* cnt_h, int Eh, const int* idx_w,
                             const float* coef_w, const int* cnt_w, int Ew, int B, int C, int in_h, int in_w, int out_h,
                             int out_w, float alpha, float scale, int dtype, void* stream);

/* Same-size separable FIR (the blur in front of the discriminator's stride-2 convs, and its adjoint) on the MFMA cores,
 * bf16, x / y [B,H,W,C] contiguous:  y = R x.  Each pass is one 16x16x32 MFMA per 16 outputs x 16 channels with the
 * filter band as a constant operand (fir_mfma.hip).
 * dgv2_fir_same_mfma_prep builds the band operands ONCE from sparse-row tables exactly as dgv2_resample_tab_sq takes them
 *   (bands: device buffer, 16-byte aligned, of dgv2_fir_same_mfma_prep_scratch BYTES -- not fp32 elements).
 *   Contract on the tables (a violation raises DGV2_STATUS_FIR_TABLE in *status and the bands are unusable):
 *   |idx_h[ho][a] - ho| <= 4,  (idx_w[wo][e] - wo + 8) mod W < 24,  every coefficient -- and every sum of the
 *   coefficients of one row that name the same input -- exactly representable in bf16.  DGV2_ENOTSUP unless
 *   H % 8 == 0 and W % 32 == 0.
 * dgv2_fir_same_mfma / _actbwd: DGV2_ENOTSUP unless C % 32 == 0, H % 8 == 0, W % 32 == 0 (then: dgv2_resample_tab_sq /
 *   dgv2_resample_tab_actbwd, whose contracts they share).  scratch: dgv2_fir_same_mfma_actbwd_scratch elements.
 * replaces: Blur / Resample(up = down = 1) (gans/models/ops/common.py:105-135) at gans/models/dusty_v2.py:325-345, its
 *   adjoint, and FusedLeakyReLUFunctionBackward (gans/models/ops/fused_act/fused_act.py:22-45) behind it. */
int dgv2_fir_same_mfma_prep_scratch(int64_t* bytes, int H, int W);
int dgv2_fir_same_mfma_prep(void* bands, int64_t bands_bytes, const int* idx_h, const float* coef_h, const int* cnt_h,
                            int Eh, const int* idx_w, const float* coef_w, const int* cnt_w, int Ew, int H, int W,
                            int* status, void* stream);
int dgv2_fir_same_mfma(void* y, const void* x, const void* bands, int B, int C, int H, int W, void* stream);
int dgv2_fir_same_mfma_actbwd_scratch(int64_t* elems, int B, int C, int H, int W);
int dgv2_fir_same_mfma_actbwd(void* y, float* gb, float* scratch, int64_t scratch_elems, const void* x, const void* ref,
                              const void* bands, int B, int C, int H, int W, float alpha, float scale, void* stream);

/* ---------------------------------------------------------------------------
 * Fourier features (positional encoding of the laser angles)
 * replaces: FourierFeature.forward, gans/models/ops/fourier.py:77-82
 * angle fp32 [Ba, 2, H, W] (NCHW as in the module API; Ba = 1 broadcasts),
 * shift fp32 [B] or NULL (added to the azimuth channel, dusty_v2.py:267-274),
 * freqs fp32 [F, 2], phase fp32 [F];
 * out [B, H, W, ld] channels-last, writes channels [c0, c0 + 2F): sin then cos.
 * ------------------------------------------------------------------------- */
int dgv2_fourier_feature(void* out, const float* angle, const float* shift,
                         const float* freqs, const float* phase,
                         int B, int Ba, int H, int W, int F, int ld, int c0, int dtype, void* stream);

/* Angle pyramid step: sin/cos -> FIR down-2 (ring / replicate) -> atan2.
 * replaces: SynthesisBlock.downsample_angle, gans/models/dusty_v2.py:135-140.
 * in fp32 [Ba,2,H,W] (Ba = 1 broadcasts), shift fp32 [B] or NULL (added to the azimuth
 * channel first) -> out fp32 [B,2,H/2,W/2] (NCHW, both channels are angles).  taps fp32 [4]. */
int dgv2_downsample_angle(float* out, const float* in, const float* shift, const float* taps,
                          int B, int Ba, int H, int W, int ring, void* stream);

/* ---------------------------------------------------------------------------
 * batched channel GEMM = the contraction of the modulated 1x1 convolution
 * replaces: F.conv2d(x[1,B*I,H,W], w[B*O,I,1,1], groups=B) in ModConv2d.forward,
 *   gans/models/ops/style.py:105-118, and its autograd dgrad / wgrad.
 *   nn:  y[b,p,o]  = sum_i x[b,p,i] * w[b,o,i]        (forward; dgrad with w^T)
 *   tn:  gw[b,o,i] = sum_p gy[b,p,o] * x[b,p,i]       (wgrad, fp32 output)
 * x [B,P,ldx] (first I channels used), w [B,O,I], y [B,P,ldy] (first O written).
 * wstride = element stride between samples of w (0 = one weight shared by the batch).
 * ydtype = dtype of y (DGV2_F32 allowed with bf16 inputs: the heads stay fp32, dusty_v2.py:174-178).
 * Fused epilogue (nn only): y = act(y + bias[o]) with bias fp32 [O] or NULL, act 0 = none /
 * 3 = leaky-ReLU(alpha) * scale -- the FusedLeakyReLU that follows each trunk conv
 * (fused_bias_act_kernel.cu:19-65), saving one pass over the activation.
 * The nn entry (dgv2_bmm_nn_sq, declared with its concatenating sibling below) has three more optional operands:
 * row_scale, resid and the sum-of-squares partials; NULL / 0 in those positions is the contraction as written here.
 * ------------------------------------------------------------------------- */
int dgv2_bmm_tn(float* gw, const void* gy, const void* x, int B, int P, int I, int O,
                int ldgy, int ldx, int dtype, void* stream);

/* Level-input conv of the generator with the positional encoding kept BATCH-SHARED:
 *   y[b,p,o] = act( sum_{k<Ka} xa[b,p,k] w[b,o,k] + sum_{k<Ks} xs[p,k] w[b,o,Ka+k] + bias[o] )
 * xa [B,P,Ka] = FIR-upsampled previous activation (NULL when Ka = 0), xs [P,Ks] = PE of the
 * unshifted angle grid, ONE copy for the batch (the per-sample azimuth shift of dusty_v2.py:267-274
 * is a per-frequency rotation folded into w by the host); w [B,O,Ka+Ks].  Ka, Ks multiples of the
 * 16-byte vector.  replaces: torch.cat([h, pe]) + ModConv2d contraction + FusedLeakyReLU,
 *   gans/models/dusty_v2.py:153-162, gans/models/ops/style.py:105-118.
 * tn: gw[b,o,:] = sum_p gy[b,p,o] * [xa[b,p,:] | xs[p,:]]  (fp32 [B,O,Ka+Ks]).
 * The entries are dgv2_bmm_nn_cat_sq and dgv2_bmm_tn_cat, declared below. */
/* The same level-input conv with the block's up-sampling COMMUTED past the contraction (a 1x1 conv acts per pixel, the
 * FIR per channel): W_a . up2(h) == up2(W_a . h), so the xa columns run at a quarter of the pixels (T = W_a . h at the
 * previous level's resolution, dgv2_modconv_up_t below) and this entry evaluates
 *   y[b,p,:O] = act( row_scale * ( up2(W_a h)[b,p,:] + sum_{k<Ks} xs[p,k] w[b,:,koff+k] ) + bias )      (bf16)
 * with row_scale and gain = scale (1 + alpha) / 2 (act 3; 1 for act 0: the leaky ReLU is then the single fma
 * f' + |f'| (1 - alpha) / (1 + alpha)) already inside T and the weight image, the bias (fp32, times gain) as the C input
 * of each chain's first MFMA, and up2 as two more K-steps (of 32) of the same v_mfma_f32_16x16x32_bf16 chain (A = the wave's window of T, B = the constant interpolation
 * matrix of its 32 pixels, built in registers from the tables).
 * O in {32, 64, 128} (generator levels 4 / 3 / 2): the launch runs O / 32 slabs of 32 channels of the same kernel.
 * t [B,Hin,O/16,Win/8,16,8]: row_scale * gain * T in 8-pixel units (row, 16-channel tile, unit u, channel: pixels 8u..8u+7) and
 * wimg [B,O/32,Ks/32,2,4,16,8]: row_scale * gain * the PE columns of the prepared per-sample weights as the MFMA operand image
 * -- both written by dgv2_modconv_up_t (the caller passes it that gain), so that
 * every LDS-DMA piece of the sample walk is one contiguous 1 KB; up2 given as two-tap tables idx/coef [Hout][2],
 * [Wout][2] (low-resolution index, weight: the sparse rows of Resample(up=2), gans/models/ops/common.py:105-135, with
 * its ring / replicate extension); xs: the PE [Hout*Wout,Ks] as the MFMA fragment image [Hout*Wout/16][Ks/32][4][16][8]
 * (element [p][k] at [p/16][k/32][(k%32)/8][p%16][k%8]; a constant of the run, laid out once).  O = 32, Ks = 512
 * (generator level 4), Wout % 32 == 0,
 * Win % 8 == 0, Win >= 32; DGV2_ENOTSUP otherwise.  Contract on the (device-resident) tables, checked by the caller
 * once per table set: both W taps of output column X lie in the window [(X & ~31) / 2 - 8, +32) mod Win.
 * in_scale (device fp32 scalar or NULL): a factor c on the whole contraction, y = act(c (up2(T) + W_s PE) + bias) -- the
 * layer's input-magnitude factor when T and the image came from dgv2_modconv_up_t_lag (which cannot know it yet: the
 * statistic it emits is what updates the running mean c derives from); applied once per block to the B operands.
 * sumsq: per-block partial sums of squares of the stored y.
 * replaces: Resample(up=2) + torch.cat([h, pe]) + ModConv2d contraction + FusedLeakyReLU,
 *   gans/models/dusty_v2.py:153-162, gans/models/ops/style.py:105-118. */
int dgv2_modconv_up_fwd(void* y, const void* t, const void* xs, const void* wimg, int B, int Hout, int Wout, int Hin,
                        int Win, int Ks, int O, const int* idx_h, const float* coef_h, const int* idx_w,
                        const float* coef_w, const float* bias, const float* in_scale, int act, float alpha, float scale,
                        int dtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
/* The low-resolution xa part of the commuted level-input conv and the operand images of dgv2_modconv_up_fwd:
 *   tcm [B,Hlow,O/16,Wlow/8,16,8]: T[b][o][p] = f[o] sum_{c<Ka} w[b][o][c] h[b][p][c] in 8-pixel units (per row: the units
 *   of channels 0..15, then those of channels 16..31, ...), f[o] = row_scale[o] * gain
 *   (row_scale fp32 [O] or NULL = 1: the input-magnitude factor of ModConv2d, style.py:98-103);
 *   wimg [B,O/32,Ks/32,2,4,16,8] (or NULL): f[o] w[b][32 z + 16 mt + o16][koff + 32 s + 8 kq + j] at [b][z][s][mt][kq][o16][j]
 *   (the A fragments of v_mfma_f32_16x16x32_bf16: one contiguous 1 KB per (K-step, M tile)).
 * h [B,Hlow*Wlow,Ka], w [B,O,I] (bf16); O in {32, 64, 128}, Ka in {64, 128, 256} (the fused dgv2_modconv_up_t_lag: Ka <= 128),
 * Wlow % 32 == 0, Ks % 32 == 0.
 * replaces: the xa columns of the ModConv2d contraction, gans/models/ops/style.py:105-118. */
int dgv2_modconv_up_t(void* tcm, void* wimg, const void* h, const void* w, const float* row_scale, float gain, int B,
                      int Hlow, int Wlow, int Ka, int Ks, int O, int I, int koff, int dtype, void* stream);
/* dgv2_modconv_up_t (row_scale = NULL) and dgv2_up2_lag_sumsq (when ghd != NULL; Gram vectors and sumsq contract as
 * there) in ONE pass over h: a wave walks a 32-column segment down the rows, its T fragments double as the operands of
 * the quadratic form's neighbourhood products.  The factor c then goes to dgv2_modconv_up_fwd as in_scale.
 * replaces: the xa columns of the ModConv2d contraction and its ema_var statistic, gans/models/ops/style.py:98-118. */
int dgv2_modconv_up_t_lag(void* tcm, void* wimg, const void* h, const void* w, float gain, const float* ghd,
                          const float* gho, const float* gwd, const float* gwo, int B, int Hlow, int Wlow, int Ka, int Ks,
                          int O, int I, int koff, int dtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
/* Per-block partial sums of sum_{b,p,c} up2(h)[b,p,c]^2 taken from h at its own (low) resolution: with U = Uh (x) Uw
 * the up-2 operator, sum (U h)^2 = h^T (Gh (x) Gw) h with tridiagonal Gram matrices Gh = Uh^T Uh, Gw = Uw^T Uw (ring axis:
 * circulant).  ghd / gho [Hin]: diagonal and (i, i+1) entries of Gh (gho[Hin-1] = 0); gwd / gwo [Win]: diagonal and
 * (j, j+1 mod Win) entries of Gw.  h [B,Hin,Win,C] bf16, C % 8 == 0, 256 % (C/8) == 0.  sumsq / cap / used as in
 * dgv2_resample_tab_sq (DGV2_ENOTSUP when cap is too small).
 * replaces: the statistic mean(x^2) of ModConv2d's ema_var update on the up-sampled input, gans/models/ops/style.py:98-103
 *   (x = Resample(up=2)(h), gans/models/dusty_v2.py:153-155), without a pass at the up-sampled size. */
int dgv2_up2_lag_sumsq(const void* h, const float* ghd, const float* gho, const float* gwd, const float* gwo, int B,
                       int Hin, int Win, int C, int dtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
/* The nn contraction and the level-input conv above (x / w / ldx / ldy / wstride / ydtype, xa / xs, bias / act / alpha /
 * scale as described there).  Both can also leave per-block partial sums of squares of the stored outputs (sumsq /
 * sumsq_cap / sumsq_used: contract as in dgv2_resample_tab_sq; NULL, 0, NULL = none), and take an optional
 * per-output-channel factor ahead of the bias: y = act(acc * row_scale[o] + bias[o]) (row_scale fp32 [O], NULL = 1) --
 * the input-magnitude factor of ModConv2d (style.py:98-103) when the weights were prepared by dgv2_mod_prep_all_fwd.
 * resid (dgv2_bmm_nn_sq only): NULL = nothing is added. */
int dgv2_bmm_nn_sq(void* y, const void* x, const void* w, int B, int P, int I, int O, int ldx, int ldy,
                   int64_t wstride, const float* row_scale, const float* bias, int act, float alpha, float scale,
                   const void* resid /* optional [B,P,ldy] in ydtype, added to the result */, int dtype, int ydtype,
                   float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
int dgv2_bmm_nn_cat_sq(void* y, const void* xa, const void* xs, const void* w, int B, int P, int Ka, int Ks,
                       int O, const float* row_scale, const float* bias, int act, float alpha, float scale, int dtype, int ydtype,
                       float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
int dgv2_bmm_tn_cat(float* gw, const void* gy, const void* xa, const void* xs, int B, int P, int Ka, int Ks,
                    int O, int dtype, void* stream);
/* The same per-sample weight gradient for O <= 4 output channels (the generator's output heads, dusty_v2.py:32-57):
 * a streaming weighted column sum instead of a 2-of-16-rows GEMM, one block per sample (the same bits every run:
 * split long pixel ranges over B and sum the parts).  DGV2_ENOTSUP outside its shapes. */
int dgv2_bmm_tn_small(float* gw, const void* gy, const void* x, int B, int P, int I, int O, int dtype,
                      void* stream);
/* ... and their data gradient y[b,p,k] = sum_{o<O} x[b,p,o] w[b,k,o] (+ resid), a contraction of O <= 4 terms. */
int dgv2_bmm_nn_small(void* y, const void* x, const void* w, const void* resid, int B, int P, int O, int K,
                      int dtype, void* stream);
/* ... followed (ref != NULL) by the activation backward of the upstream bias + leaky-ReLU layer whose OUTPUT `ref`
 * [B,P,K] is this operator's forward input (the heads read the trunk's last activation):
 *   y = (x.w^T + resid) * (ref > 0 ? 1 : alpha) * ascale * row_scale[k];  gb[k] = column sums of the value before
 *   row_scale (fp32 [K]) -- FusedLeakyReLUFunctionBackward (fused_act.py:22-45) without its own pass.
 * scratch (with ref): dgv2_bmm_nn_small_act_scratch elements. */
int dgv2_bmm_nn_small_act_scratch(int64_t* elems, int B, int P, int O, int K, int dtype);
int dgv2_bmm_nn_small_act(void* y, const void* x, const void* w, const void* resid, int B, int P, int O, int K,
                          const void* ref, const float* row_scale, float alpha, float ascale, float* gb,
                          float* scratch, int64_t scratch_elems, int dtype, void* stream);
/* The whole backward of a level's output heads in ONE streaming pass + one reduce launch (round 5): the heads' input
 * x = ref [B,P,K] is read once (operand of the head weight gradient AND reference of the upstream layer's activation
 * backward), the skip gradient gyf fp32 [B,P,O] once:
 *   g = T(gyf * cvec[o]);  y = ((g . w[b]^T) + resid) * (ref > 0 ? 1 : alpha) * ascale * row_scale[k]  (as _small_act);
 *   gb_up[k] = column sums of the unscaled rounded y;  gw[b,o,k] = sum_p g[p,o] ref[p,k];  gbh[o] = sum gyf[.,o].
 * replaces: the autograd of the two ModConv2d heads of a SynthesisBlock (gans/models/dusty_v2.py:30-57,171-178 on
 *   gans/models/ops/style.py:105-118) and of the FusedLeakyReLU in front of them (fused_act.py:22-45) -- five launches per
 *   level here before (column sum, scale + cast, dgv2_bmm_nn_small_act, dgv2_bmm_tn_small, reducers / zero fills).
 * scratch: dgv2_head_bwd_scratch elements.  DGV2_ENOTSUP as _small_act. */
int dgv2_head_bwd_scratch(int64_t* elems, int B, int P, int O, int K, int dtype);
int dgv2_head_bwd(void* y, float* gw, float* gbh, float* gb_up, float* scratch, int64_t scratch_elems, const float* gyf,
                  const float* cvec, const void* w, const void* resid, const void* ref, const float* row_scale, float alpha,
                  float ascale, int B, int P, int O, int K, int dtype, void* stream);

/* The same contraction as dgv2_bmm_nn_cat_sq, organised for the two top pyramid levels where it dominates
 * the generator ((Ka, Ks, O) = (64, 512, 32) and, as two 32-channel slabs, (128, 512, 64); bf16): a block owns a tile of pixels and walks the
 * samples, the shared PE fragments stay in registers, xa streams straight into registers and only the
 * per-sample weights go through LDS (LDS-DMA, double-buffered) -- HBM sees xa and y once, the PE once per block.
 * Returns DGV2_EINVAL for any other shape / dtype (use dgv2_bmm_nn_cat_sq).
 * row_scale (fp32 [O], NULL = 1) as there; sumsq / sumsq_cap / sumsq_used: the per-block sum-of-squares partials of the
 * stored outputs (contract as in dgv2_resample_tab_sq; NULL, 0, NULL = none). */
int dgv2_modconv_pe_fwd_sq(void* y, const void* xa, const void* xs, const void* w, int B, int P, int Ka, int Ks,
                           int O, const float* row_scale, const float* bias, int act, float alpha, float scale, int dtype, float* sumsq,
                           int sumsq_cap, int* sumsq_used, void* stream);
/* ... and with the contraction of the level's two 1-channel output heads taken in this layer's epilogue instead of by a
 * pass of their own over y: head_out[b,p,j] = sum_o y[b,p,o] head_w[b,j,o], j < 2 (on the stored bf16 values, fp32 sums;
 * the heads' input-magnitude factor and bias are applied by the caller: they depend on the statistic of y this very launch
 * produces).  head_w [B,2,O] bf16 (the heads' prepared weights), head_out fp32 [B,P,2]; both or neither.
 * replaces: the ModConv2d contractions of Head.forward (gans/models/dusty_v2.py:30-57,171-178) behind conv2 of a
 * SynthesisBlock (:161-170).  PE-free one-slab shapes (Ka, O) = (32, 32), (64, 64) (conv2 of levels 4 / 3); DGV2_ENOTSUP for
 * any other shape when head_w is given. */
int dgv2_modconv_pe_fwd_head(void* y, const void* xa, const void* xs, const void* w, int B, int P, int Ka, int Ks,
                             int O, const float* row_scale, const float* bias, int act, float alpha, float scale, int dtype,
                             float* sumsq, int sumsq_cap, int* sumsq_used, const void* head_w, float* head_out, void* stream);

/* Data gradient of a PE-free K -> K modulated 1x1 layer (conv2 of a generator level) FUSED with the activation backward
 * of the layer that produced its input (conv1 of the level): one pass over the gradient instead of three.
 * replaces: the autograd chain ModConv2d (data gradient, gans/models/ops/style.py:105-118) -> FusedLeakyReLU backward
 *   (fused_act.py:46-59, fused_bias_act_kernel.cu:19-60) between the two convs of a SynthesisBlock (dusty_v2.py:160-170)
 *   g[b,p,k]    = sum_o gy[b,p,o] wt[b,k,o]                    (rounded to bf16)
 *   t           = (yref[b,p,k] > 0 ? g : g * alpha) * scale
 *   gpre[b,p,k] = bf16(t * up_scale[k]),   gb[k] = sum_{b,p} bf16(t)
 * -- bit for bit what dgv2_modconv_pe_fwd_sq (Ks = 0) followed by dgv2_bias_act_bwd_rs produce.
 * gy [B,P,K], wt [B,K,K], yref [B,P,K] (the upstream layer's forward output), gpre [B,P,K]: bf16; up_scale, gb fp32 [K];
 * scratch: dgv2_modconv_pe_dgrad_actbwd_scratch elements.
 * K in {32, 64} (generator levels 4 / 3), dtype DGV2_BF16; DGV2_ENOTSUP otherwise. */
int dgv2_modconv_pe_dgrad_actbwd_scratch(int64_t* elems, int B, int P, int K, int dtype);
int dgv2_modconv_pe_dgrad_actbwd(void* gpre, float* gb, float* scratch, int64_t scratch_elems, const void* gy,
                                 const void* wt, const void* yref, const float* up_scale, float alpha, float scale, int B,
                                 int P, int K, int dtype, void* stream);

/* Per-sample weights of the modulated conv, written directly as the GEMM operand, and the exact
 * backward of that preparation (max-normalisations, modulation, demodulation, input-magnitude
 * scaling, optional rotation of the positional-encoding columns by shift_b * fw).
 * replaces: ModConv2d.forward weight path, gans/models/ops/style.py:72-103 (and its autograd).
 * W fp32 [O,I]; s fp32 [B,I] (style after the affine); ema_var fp32 [1]; wb [B,Otot,I] (this layer's
 * rows at [row_off, row_off+O)), dtype wb_dtype; stats fp32 [2+2B] and dsave fp32 [B,O] are produced
 * by fwd and consumed by bwd; shift fp32 [B] / fw fp32 [F] or NULL (F must be 256, PE columns
 * [cin, cin+2F)); I <= 1024.  bwd: G fp32 [B,Otot,I] -> gW fp32 [O,I], gs fp32 [B,I]; corr fp32 [1]. */
/* Adam (torch.optim.Adam semantics, no weight decay / amsgrad; the optimizers of gans/trainer.py:142-171) over a
 * list of L <= 72 fp32 parameter tensors in one launch -- the tensors of torch's own optimizer state, addresses
 * by value (HOST arrays of device pointers).  dgv2_adam_prep advances the device step counter and leaves the
 * bias corrections of that step in sc (fp32 [4]) for dgv2_adam_step. */
/* dst[l] <- lerp(dst[l], src[l], weight), L <= 72 fp32 tensors, one launch: ema_inplace (trainer.py:30-41). */
int dgv2_lerp_list(float* const* dst, const float* const* src, const int* n, int L, float weight, void* stream);
int dgv2_adam_prep(float* sc, float* step, float b1, float b2, void* stream);
int dgv2_adam_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int* n,
                   int L, const float* sc, float lr, float b1, float b2, float eps, void* stream);

/* The optimizer tail of the segmentation models' training step over a list of fp32 tensors (HOST arrays of L <= 72
 * device pointers, by value in the launch, as dgv2_adam_step): torch.optim.SGD with momentum and weight decay
 * (dampening 0, no Nesterov; train_semseg.py:201-212, lr as the schedule of 360-362 leaves it in the param group) with
 * GradScaler.unscale_, clip_grad_norm_, GradScaler.step's overflow skip and GradScaler.update (train_semseg.py:278-283)
 * folded in.  Three entries, no atomics, no host synchronisation, every launch hipGraph-capturable; the gradients are
 * only read.  The workspace is the CALLER's: DGV2_SUMSQ_PARTS floats per tensor (no _scratch sibling).
 *
 * dgv2_sumsq_list: block (x, l) of a (DGV2_SUMSQ_PARTS, L) grid writes partials[l*DGV2_SUMSQ_PARTS + x] = the sum of
 *   g[l][i]^2 over its share -- the 4-element groups x*256 + t, + 64*256, ... and one tail element -- accumulated in fp32
 *   in a fixed order (thread chain of fused multiply-adds, wave reduce, block reduce): the bits depend on n[l] alone
 *   (16-byte loads where g[l] is 16-byte aligned, element loads of the same groups otherwise).
 * dgv2_clip_prep: one block adds the `count` partials in double in a fixed order (thread t the partials t, t + 256, ...
 *   in index order, then a fixed tree) and writes sc (fp32 [4]).  scale_state: fp32 [2] = (loss scale, growth tracker),
 *   or NULL for "no loss scale".  With s = scale (1 when NULL) and norm = sqrt(sum) / s, computed in double:
 *     sc[0] = norm                                          the unscaled total gradient norm
 *     sc[1] = min(1, max_norm / (norm + 1e-6)) / s          the factor on every raw gradient (max_norm <= 0: 1 / s)
 *     sc[2] = 1 when scale_state is given and sum is not finite, else 0
 *     sc[3] = s                                             the loss scale this step ran under
 *   and, when scale_state is given, GradScaler.update: on overflow scale *= backoff, tracker = 0; otherwise tracker += 1
 *   and, when it equals growth_interval, scale *= growth, tracker = 0.  Without a loss scale a non-finite norm goes on
 *   into the parameters as it does in the reference (a NaN norm gives a NaN factor).
 * dgv2_sgd_step: where sc[2] != 0 every block returns before touching p or m; else per element
 *     d = sc[1]*g + weight_decay*p;   m = momentum*m + d;   p -= lr*m
 *   evaluated in double from the fp32 operands, m and p each rounded to fp32 once (p from the unrounded m)
 *   (a momentum buffer of zeros reproduces torch's first step buf = d exactly: no first-step flag).  Five fp32 streams
 *   per element (p, g, m read; p, m written).  momentum == 0: p -= lr*d, m is neither read nor written (m, or any
 *   m[l], may be NULL).  DGV2_EINVAL, nothing launched (dgv2_sumsq_list and dgv2_sgd_step alike): a NULL pointer, L
 *   outside [1, 72], an n[l] that is negative or above DGV2_SGD_N_MAX (the kernels index with int). */
#define DGV2_SUMSQ_PARTS 64
#define DGV2_SGD_N_MAX (2147483647 - (1 << 17))
int dgv2_sumsq_list(const float* const* g, const int* n, int L, float* partials, void* stream);
int dgv2_clip_prep(const float* partials, int count, float max_norm, float* scale_state, float growth, float backoff,
                   int growth_interval, float* sc, void* stream);
int dgv2_sgd_step(float* const* p, const float* const* g, float* const* m, const int* n, int L, const float* sc, float lr,
                  float momentum, float weight_decay, void* stream);

/* Pack / unpack a list of L <= 48 small fp32 matrices (HOST array of device pointers, by value in the launch)
 * into / out of one zero-padded [L, Rmax, Cmax] tensor: the 19 style affines of the generator (EqualLR Linear
 * of every ModConv2d, style.py:30,75) then run as one batched library GEMM forward and two backward. */
int dgv2_pack2d(float* packed, const float* const* src, const int* rows, const int* cols, int L, int Rmax,
                int Cmax, void* stream);
int dgv2_unpack2d(float* const* dst, const float* packed, const int* rows, const int* cols, int L, int Rmax,
                  int Cmax, void* stream);

/* Input-magnitude EMA of ModConv2d (style.py:98-103) as one scalar launch:
 * if update: ema <- lerp(ema, (sum(sumsq[0..nsum)) + add) * inv_count, weight); snapshot[0] <- ema[0].
 * sumsq (NULL allowed): the per-block partial sums dgv2_sum_squares leaves (nsum = 512).
 * cvec (NULL allowed): cvec[0..ncvec) <- 1/(sqrt(ema)+1e-8), the factor the layer applies to its output rows
 * (row_scale of the GEMM entries below); snapshot may then be NULL. */
int dgv2_ema_scalar(float* ema, float* snapshot, const float* sumsq, int nsum, float add, float inv_count,
                    float weight, int update, float* cvec, int ncvec, void* stream);
/* The same update for n <= 8 layers that share their input -- the output heads of one generator level
 * (dusty_v2.py:32-57, one ModConv2d per output with its own ema_var): emas / rows are HOST arrays (device pointers /
 * row counts, by value in the launch); layer i fills rows[i] entries of cvec behind those of the layers before it. */
int dgv2_ema_scalar_group(float* const* emas, const int* rows, int n, const float* sumsq, int nsum, float add,
                          float inv_count, float weight, int update, float* cvec, void* stream);
int dgv2_mod_prep_fwd(void* wb, float* dsave, float* stats, const float* W, const float* s,
                      const float* ema_var, const float* shift, const float* fw, int B, int O, int I,
                      int Otot, int row_off, int demod, int cin, int F, int wb_dtype, void* stream);
int dgv2_mod_prep_bwd(float* gW, float* gs, float* corr, const float* G, const float* W, const float* s,
                      const float* stats, const float* dsave, const float* ema_var, const float* shift,
                      const float* fw, int B, int O, int I, int Otot, int row_off, int demod, int cin,
                      int F, int corr_elems, void* stream);

/* All L <= 32 modulated layers of one generator pass prepared in one launch each way (the per-layer entries
 * above cost four launches per layer and pass).  Host arrays of length L: W[l] fp32 [O,I], s[l] fp32 [B,I],
 * fw[l] fp32 [256] (layers with flags & 2), wb[l] -> [B, Otot[l], I[l]] GEMM operand (bf16 if flags & 4 else
 * fp32; layers sharing a GEMM pass the same buffer and different row_off), dsave[l] fp32 [B,O]; stats fp32
 * [L, 2+2B]; rot fp32 [L, B, 512] scratch (the rotating layers' sin/cos table, filled by fwd, read by bwd).
 * flags: 1 demodulate, 2 rotate the PE columns [cin, cin+512) by shift[b] (shift NULL: none),
 * 4 bf16 operand.  These weights do NOT contain 1/(sqrt(ema_var)+1e-8): that factor is the GEMM's row_scale
 * (dgv2_*_sq), its gradient side dgv2_bias_act_bwd_rs / dgv2_scale_cast; so G below is dL/d(these weights).
 * bwd: out[l] = [gW (O*I) | gs (B*I) | corr scratch (ncorr[l] >= 1)] fp32, all inside flat[flat_elems] which
 * is cleared here once.  replaces: ModConv2d.forward weight path, gans/models/ops/style.py:72-103. */
int dgv2_mod_prep_all_fwd(void* const* wb, float* const* dsave, float* stats, float* rot, const float* const* W,
                          const float* const* s, const float* const* fw, const int* O, const int* I,
                          const int* Otot, const int* row_off, const int* cin, const int* flags,
                          const float* shift, int B, int L, void* stream);
int dgv2_mod_prep_all_bwd(float* flat, int64_t flat_elems, float* const* out, const int* ncorr,
                          const float* const* G, const float* const* W, const float* const* s,
                          const float* stats, const float* rot, float* const* dsave,
                          const float* const* fw, const int* O, const int* I, const int* Otot,
                          const int* row_off, const int* cin, const int* flags, const float* shift, int B,
                          int L, float* scratch, int64_t scratch_elems, void* stream);
/* scratch (fp32, 16-byte aligned, >= dgv2_mod_prep_all_bwd_scratch elements): the backward then keeps its sums over a
 * unit's samples in registers and leaves per-unit partials there, which its two fix-up kernels fold -- no atomics,
 * nothing cleared, bit-identical from run to run (needs I % 4 == 0 and cin % 4 == 0 on rotating layers; NULL or any
 * other shape: the atomic form on `flat`, which this entry clears).  The forward takes the matching float4 form under
 * the same shape conditions by itself. */
int dgv2_mod_prep_all_bwd_scratch(int64_t* elems, const int* O, const int* I, int B, int L);

/* Batched transposes in one launch: dst[l][b, c, r] = src[l][b, r, c] (r < rows[l], c < cols[l], source leading
 * dimension ld[l]); HOST arrays of L <= 32 device pointers, elem_size 2 or 4 bytes.  Produces the operands of all
 * modulated layers' data gradients (contraction over the output channels of the per-sample weights [B, O, I])
 * up front instead of one strided copy per layer in backward (ModConv2d autograd, style.py:105-118). */
int dgv2_transpose_list(void* const* dst, const void* const* src, const int* rows, const int* cols,
                        const int* ld, int L, int B, int elem_size, void* stream);

/* Sum of squares of the first C channels of x [N, ld] into acc[0] (fp32, ACCUMULATES).
 * replaces: x.pow(2).mean() in ModConv2d.forward (style.py:100-101). */
int dgv2_sum_squares(float* acc, const void* x, int64_t N, int C, int ld, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * minibatch standard deviation + concat (discriminator epilogue)
 * replaces: MinibatchStdDev.forward + torch.cat, gans/models/ops/common.py:226-250 (mbdis_feat = 1), used at
 *   gans/models/dusty_v2.py:376-385.  x [B, P, C] channels-last (P = H*W), out [B, P, Cp] same dtype with
 *   out[..., :C] = x, out[..., C] = the group statistic of the sample, out[..., C+1:] = 0 (channel padding for the
 *   conv engine, Cp > C, both multiples of the 16-byte vector).  B = splits * group * m: `splits` independent
 *   sub-batches (real | fake in one pass), group members strided by m as in the reference.  scratch: fp32
 *   [>= 64 * B / group].  bwd: gx [B, P, C] from the gradient of `out` and x.
 * The epilogue's cast is folded in: x / gx in xdtype, out (ydtype) / gout (gdtype) the same (the plain form: pass xdtype
 * twice) or fp32 for a bf16 x -- x.float() of the reference's fp32 epilogue (gans/models/dusty_v2.py:394-395) and its
 * adjoint without their own passes over the activation.
 * ------------------------------------------------------------------------- */
int dgv2_mbstd_cat_fwd_x(void* out, float* scratch, const void* x, int B, int P, int C, int Cp, int splits, int group,
                         int xdtype, int ydtype, void* stream);
int dgv2_mbstd_cat_bwd_x(void* gx, const void* gout, const void* x, int B, int P, int C, int Cp, int splits, int group,
                         int xdtype, int gdtype, void* stream);
/* C[i, j] = scale * sum_{t < T} A(i, t) B(j, t) in fp32-equivalent arithmetic on the bf16 matrix cores: every operand
 * value is split into three bf16 planes (x = h + m + l, residual <= 2^-26 |x|) while its tile is staged into LDS and a
 * product is taken as six bf16 products with fp32 accumulation (the dropped terms are below 2^-25 of the product).
 * a_trans == 0: A [I, lda], t contiguous; != 0: A [T, lda], i contiguous (same for B).  C [I, ldo].  I % 64 == 0,
 * J % 128 == 0, T % 32 == 0, lda / ldb % 4 == 0 (DGV2_ENOTSUP otherwise).  splits > 1: split-K through
 * scratch [splits * I * J] (ldo == J) and a summing launch.
 * replaces: F.linear and its autograd GEMMs for EqualLR(nn.Linear(65536, 512)) of the discriminator's fp32 epilogue,
 *   gans/models/dusty_v2.py:381-383,394-395 (forward: both direct, split-K; dgrad: W transposed; wgrad: both
 *   transposed). */
int dgv2_gemm_x3(float* c, float* scratch, int64_t scratch_elems, const float* a, const float* b, int I, int J,
                 int64_t T, int a_trans, int b_trans, int64_t lda, int64_t ldb, int64_t ldo, int splits, float scale,
                 void* stream);
/* Weight gradient of the batch-shared positional-encoding columns of the modulated 1x1 convs:
 *   gw[b, o, col0 + k] = sum_p g[b, p, o] * pe[p, k], k < Ks      (gw fp32 [B, O, ldo]; g [B, P, O], pe [P, Ks] bf16)
 * 128 / O samples share a block's M tile, so one staged PE tile feeds several samples' accumulators (as a batched
 * library GEMM the encoding is re-read per sample); the pixel axis is split over blocks through `scratch`
 * (>= dgv2_pe_wgrad_scratch elements).  O divides 128, O % 8 == 0, B * O % 128 == 0, Ks % 128 == 0, P % 32 == 0.
 * replaces: the PE columns of ModConv2d's weight gradient (autograd of gans/models/ops/style.py:105-118 on the
 *   concatenated input of gans/models/dusty_v2.py:153-162). */
int dgv2_pe_wgrad_scratch(int64_t* elems, int B, int P, int O, int Ks);
int dgv2_pe_wgrad(float* gw, float* scratch, int64_t scratch_elems, const void* g, const void* pe, int B, int P, int O,
                  int Ks, int64_t ldo, int col0, void* stream);

/* ---------------------------------------------------------------------------
 * dense convolution with ring padding (discriminator)
 * replaces: ops.Conv2d = Pad(circular W / replicate H) + nn.Conv2d, via cuDNN/ATen
 *   gans/models/ops/common.py:10-24,187-210, used at gans/models/dusty_v2.py:325-385
 * x [B,H,W,C]; w [O,kh,kw,C] (channels-last filter); y [B,Ho,Wo,O];
 * pad on every side, Ho = (H + 2*pad - kh)/stride + 1.
 *   fwd  : y  = conv(pad(x), w), optionally followed by the fused bias + leaky-ReLU epilogue
 *          (bias fp32 [O] or NULL, act 0 / 3, alpha, scale) as in dgv2_bmm_nn_sq
 *   dgrad: gx = pad^T(conv^T(gy, w))         (gx [B,H,W,C]; wt = w transposed to [C,kh,kw,O];
 *          gxp_scratch [B,H+2pad,W+2pad,C] holds the padded-domain gradient, NULL if pad == 0)
 *   wgrad: gw[o,ky,kx,c] = sum gy * pad(x)   (fp32 [O,kh,kw,C], overwritten)
 * ------------------------------------------------------------------------- */
int dgv2_conv_fwd(void* y, const void* x, const void* w, int B, int H, int W, int C, int O,
                  int kh, int kw, int stride, int pad, int ring,
                  const float* bias, int act, float alpha, float scale, int dtype, void* stream);
int dgv2_conv_dgrad(void* gx, void* gxp_scratch, const void* gy, const void* wt,
                    int B, int H, int W, int C, int O,
                    int kh, int kw, int stride, int pad, int ring, int dtype, void* stream);
int dgv2_conv_wgrad(float* gw, const void* gy, const void* x, int B, int H, int W, int C, int O,
                    int kh, int kw, int stride, int pad, int ring, int dtype, void* stream);

/* Direct (LDS halo-tile) weight gradient for the small-channel / large-image layers (same reference
 * lines as dgv2_conv_wgrad): gw fp32 [O, k*k, C] = sum over pixels of gy [B,Ho,Wo,O] x padded x
 * [B,H,W,C].  k in {1,3}, pad = (k-1)/2, stride in {1,2}, C % 32 == 0, O % vec == 0; bf16 or (fp32,
 * stride 1).  Returns DGV2_EINVAL for anything else (use dgv2_conv_wgrad). */
int dgv2_conv_wgrad_direct(float* gw, const void* gy, const void* x, int B, int H, int W, int C, int O,
                           int k, int stride, int pad, int ring, int dtype, void* stream);

/* Per-sample 1x1 weight gradient of the modulated conv (ModConv2d autograd, style.py:105-118) on the streaming
 * engine above: gw fp32 [B,O,C] = sum over the H*W pixels of sample b of gy [B,H,W,O] x [B,H,W,C]; splits stay
 * inside an image.  C, O multiples of the 16-byte vector and O*C a multiple of 4.
 * x_shared != 0 (0 = x holds one image per sample): x is ONE image [H, W, C] contracted against every sample's gy -- the
 * weight gradient of the batch-shared positional-encoding columns, gw[b,o,c] = sum_p gy[b,p,o] * pe[p,c] (DESIGN.md
 * section 5.3).
 * ldo, a row pitch: gw is [B, O, ldo] (ldo >= C, ldo % 4 == 0; 0 = contiguous [B, O, C]), the columns [0, C) of the layer's
 * whole [B, O, Ka + Ks] weight gradient written in place next to the PE columns of dgv2_pe_wgrad -- no concatenation. */
int dgv2_bmm_tn_stream_scratch(int64_t* elems, int B, int H, int W, int C, int O, int dtype);
int dgv2_bmm_tn_stream_ld(float* gw, int64_t ldo, float* scratch, int64_t scratch_elems, const void* gy, const void* x,
                          int x_shared, int B, int H, int W, int C, int O, int dtype, void* stream);

/* Compute-dtype copies of all conv weights of the discriminator in ONE launch (L <= 32): from each fp32
 * master [O,C,kh,kw] (EqualLR runtime scale folded in: common.py:158-184) the forward layout
 * wf [O, kh*kw, Cpad] and the data-gradient layout wt [Cpad, kh*kw, O].  HOST arrays of device pointers.
 * w8 / w8t: two more, optional outputs per layer (array or entry NULL: none).  w8t[l]: the staging image of the stride-1
 * data gradient dgv2_conv3x3_dgrad8 -- [Cpad / 64][O / 32][2304 units], row = t' * 64 + c % 64 with the gradient's tap
 * order t' = 8 - (ky * 3 + kx), plane = (o % 32) / 8 (needs Cpad % 64 == 0, O % 32 == 0).  w8[l]: the STAGING IMAGE of
 * the eight-wave forward conv dgv2_conv3x3_fwd8 -- [O / 64][Cpad / 32][2304 units of 16 bytes], unit (row = tap * 64 + o % 64,
 * plane = (c % 32) / 8) at (row >> 3) * 32 + plane * 8 + (row & 7), the order the kernel's staging slots read it: a
 * slab's K-chunk is one contiguous 36 KB run instead of 576 pieces of 64 bytes.  Same values as wf.  Needs kh*kw == 9,
 * O % 64 == 0, Cpad % 32 == 0, DGV2_BF16.  dtype DGV2_F32: the images are the three-plane images of
 * dgv2_conv3x3_x3_fwd / _dgrad instead -- every value split as h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), one image
 * per plane in the layout above: w8 [3][O / 64][ceil(Cpad / 32)][2304] (O % 64 == 0, Cpad % 8 == 0; zeros past C),
 * w8t [3][floor(Cpad / 64)][O / 32][2304] (O % 32 == 0, Cpad >= 64).
 * replaces: the same EqualLR weights (common.py:158-210). */
int dgv2_conv_weight_bank_ex(void* const* wf, void* const* wt, void* const* w8, void* const* w8t,
                             const float* const* src, const int* O, const int* C, const int* Cpad, const int* kk,
                             const float* scale, int L, int dtype, void* stream);
/* Forward 3x3 ring conv, stride 1 or 2, pad 1, on that image (conv8.hip: eight waves per block = two groups of four that
 * share the halo tile (stride 2: two 64-channel slabs per 8 x 32 pixel tile) or the weight slab (stride 1: two pixel
 * tiles per slab)):  y [B, Hin/stride, Win/stride, O] (bf16) = act( conv(x [B,Hin,Win,Cin], w) + resid + bias ) * scale,
 * act 0 | 3 (leaky ReLU with `alpha`), bias [O] fp32 or NULL, resid like y or NULL.
 * replaces: ops.Conv2d forward (gans/models/ops/common.py:187-210) at ResidualBlock.conv1 / .conv2
 * (gans/models/dusty_v2.py:325-345).  DGV2_ENOTSUP where the engine does not cover the geometry (O % 64 (stride 1) /
 * O % 128 (stride 2), Cin % 32, Cin >= 64, at least 4 output rows and 32 / 64 output columns): callers then run
 * dgv2_conv_direct_fwd on wf. */
int dgv2_conv3x3_fwd8(void* y, const void* x, const void* w8, int B, int Hin, int Win, int Cin, int O, int stride,
                      const float* bias, const void* resid, int act, float alpha, float scale, int dtype, void* stream);
/* The stride-1 data gradient of the same conv on the transposed image w8t: gx [B,H,W,C] (bf16) from gy [B,H,W,O], the
 * replicate-row terms of rows 0 and H - 1 included, + resid (the gradient of a sibling branch of the same input, like gx,
 * or NULL).  replaces: the cuDNN data gradient autograd calls for ops.Conv2d (common.py:187-210) at ResidualBlock.conv1
 * (dusty_v2.py:329).  DGV2_ENOTSUP where the engine does not cover the geometry (C % 64, O % 32, O >= 64, H >= 8,
 * W >= 32 / 64): callers then run dgv2_conv_direct_dgrad on wt. */
int dgv2_conv3x3_dgrad8(void* gx, const void* gy, const void* w8t, int B, int H, int W, int C, int O, const void* resid,
                        int dtype, void* stream);
/* The STRIDE-2 data gradient of the 3x3 ring conv (pad 1) on the eight-wave engine (conv8_s2d.hip), from the transposed row
 * weights wt [C, 9, O] (dgv2_conv_weight_bank_ex's wt): gx [B, 2 Hg, 2 Wg, C] (bf16) from gy [B, Hg, Wg, O], the replicate row of
 * output row 0 included -- two launches, one per output row parity (three or six taps, two column classes each) on eight-row
 * tiles where those fill the chip, one four-class launch on four-row tiles otherwise.
 * replaces: the cuDNN data gradient autograd calls for ops.Conv2d (common.py:187-210) at ResidualBlock.conv2
 * (dusty_v2.py:337-345).  DGV2_ENOTSUP where the engine does not cover the geometry (C % 128, O % 32, O >= 64, Hg % 4,
 * Wg % 32, DGV2_BF16): callers then run dgv2_conv_direct_dgrad on wt. */
int dgv2_conv3x3_s2_dgrad8(void* gx, const void* gy, const void* wt, int B, int Hg, int Wg, int C, int O, int dtype,
                           void* stream);

/* fp32 3x3 ring conv (stride 1, pad 1) on the bf16 matrix cores (conv_x3.hip): the fp32 operands as three bf16 planes
 * each (x = h + m + l), six bf16 products per multiply, fp32 accumulation -- fp32-equivalent (dropped terms < 2^-25 of a
 * product), at 3/8 of the cost of v_mfma_f32_16x16x4_f32.  w3 = the three plane images dgv2_conv_weight_bank_ex writes
 * for dtype DGV2_F32 (w8: [3][O / 64][ceil(Cx / 32)][2304 units of 8 bf16]); the activations are split while staged.
 *   y [B,H,W,O] (fp32) = act( conv(x [B,H,W,Cx] fp32, w) + bias ) * scale + resid,  act 0 | 3, bias [O] or NULL,
 *   resid like y or NULL.
 * replaces: ops.Conv2d(ch(4) + 1, ch(4), 3, 1, 1, ring) + FusedLeakyReLU of Discriminator.epilogue
 * (gans/models/dusty_v2.py:376-379) in the fp32 island of Discriminator.forward (:394-395).  DGV2_ENOTSUP where the
 * kernel does not cover the geometry (W % 32, Cx % 8, Cx >= 64, O % 64): callers then run dgv2_conv_direct_fwd in fp32. */
int dgv2_conv3x3_x3_fwd(void* y, const void* x, const void* w3, int B, int H, int W, int Cx, int x_exact, int O,
                        const float* bias, const void* resid, int act, float alpha, float scale, int* status,
                        void* stream);
/* x_exact (forward and weight gradient): the caller's promise that channels [0, x_exact) of x hold bf16-representable
 * values -- the activations of a bf16 trunk widened to fp32, which is what the discriminator's epilogue receives
 * (dusty_v2.py:394: h.to(torch.float32)).  Their planes m and l are zero, so three of the six products of a multiply are
 * products with zero: they are not issued (same sum, half the MFMAs).  0 = no promise.  The kernels check the promise on
 * the values they stage: a value that breaks it raises DGV2_STATUS_X_INEXACT in *status (the caller's device word, see
 * "Status words" above; required when x_exact > 0) -- that launch then computed with the bf16-rounded input. */
/* Its data gradient: gx [B,H,W,ldx] (fp32) from gy [B,H,W,O] fp32 -- channels [0, C) the gradient (+ resid), [C, ldx)
 * resid or zero.  w3t = the transposed plane images (w8t of dgv2_conv_weight_bank_ex, dtype DGV2_F32:
 * [3][ldx / 64][O / 32][2304 units]) serve the channels of whole 64-channel slabs; wt [ldx, 9, O] fp32 (the bank's
 * data-gradient layout) the channels behind them in exact fp32, one pass per channel (the minibatch-stddev channel of
 * 512 + 1; at most 16).  replaces: the cuDNN data gradient autograd calls for that conv.  DGV2_ENOTSUP: H < 2, W % 32,
 * O % 32, O < 64, C < 64, C % 64 > 16, ldx / 64 != C / 64. */
int dgv2_conv3x3_x3_dgrad(void* gx, const void* gy, const void* w3t, const void* wt, int B, int H, int W, int C, int ldx,
                          int O, const void* resid, void* stream);
/* Its weight gradient (conv_wgrad_stream.hip: conv_wgrad_x3_kernel, both operands split while staged):
 * gw fp32 [O, 9, C] (param_layout != 0: [O, C, 3, 3]) = scale * sum_{b,h,w} gy[b,h,w,o] xpad[b,h+ky-1,w+kx-1,c] from
 * gy [B,H,W,O], x [B,H,W,C] fp32.  Input channels [0, 64 floor(C/64)) on the matrix cores, [.., clive) in exact fp32
 * (at most 16), [clive, C) = 0 (x's padding channels).  scratch: fp32 [>= dgv2_conv3x3_x3_wgrad_scratch(...)].
 * replaces: the cuDNN weight gradient autograd calls for that conv.  DGV2_ENOTSUP: O % 128, C < 64, C % 8, W % 32,
 * more than 16 such channels. */
int dgv2_conv3x3_x3_wgrad(float* gw, float* scratch, int64_t scratch_elems, const void* gy, const void* x, int B, int H,
                          int W, int C, int clive, int x_exact, int O, float scale, int param_layout, int* status,
                          void* stream);
int dgv2_conv3x3_x3_wgrad_scratch(int64_t* elems, int B, int H, int W, int C, int clive, int O);
/* Both image sets from weight VALUES w [O, 9, Cp] fp32 (the operand layout of dgv2_conv_direct_fwd), for passes that do not
 * run on the weight bank (R1's double backward): w3 [3][O / 64][ceil(Cp / 32)][2304 units of 8 bf16], w3t
 * [3][Cp / 64][O / 32][2304 units]; either may be NULL.  O % 64 == 0, Cp % 8 == 0, Cp >= 64. */
int dgv2_conv_x3_images(void* w3, void* w3t, const void* w, int O, int Cp, void* stream);

/* Streaming weight gradient -- the hot-path engine for every discriminator conv (same reference lines as
 * dgv2_conv_wgrad).  A block keeps one (o, c) tile of gw for all k*k taps in registers and streams its
 * slice of the batch's pixel tiles; the per-slice partial sums go to `scratch` (plain stores) and are
 * reduced into gw fp32 [O, k*k, C] (overwritten).  k in {1,3}, pad = (k-1)/2, stride in {1,2}, C and O
 * multiples of the 16-byte vector.  dgv2_conv_wgrad_stream_scratch reports the fp32 element count the
 * scratch buffer must hold for a geometry.
 * The entry writes scale * gw (1.f: the plain gradient), and with param_layout != 0 in the parameter's own layout
 * [O, C, k, k] (nn.Conv2d weight, common.py:187-210) instead of [O, k*k, C] (0): the EqualLR factor and the layout
 * change of the weight gradient cost no separate pass. */
int dgv2_conv_wgrad_stream_scratch(int64_t* elems, int B, int H, int W, int C, int O, int k, int stride,
                                   int pad, int dtype);
int dgv2_conv_wgrad_stream_pl(float* gw, float* scratch, int64_t scratch_elems, const void* gy, const void* x,
                              int B, int H, int W, int C, int O, int k, int stride, int pad, int ring,
                              float scale, int param_layout, int dtype, void* stream);

/* Direct (LDS halo-tile) convolution on the matrix cores (conv_direct.hip) -- the hot-path engine for the discriminator
 * convs and their data gradients.  The caller states the conv; the library chooses the kernel (strip, eight-wave,
 * image pairs, pipelined, synchronous) and builds its parameters.  Common to the three entries: channels-last tensors,
 * k in {1, 3} with pad (k - 1) / 2, stride in {1, 2}, ring (circular) padding along W and replicate padding along H
 * (common.py:10-24) -- nothing padded is materialised --, 16-byte aligned operands, contraction length (Cin forward, O in
 * the data gradient) a multiple of one 64-byte K-chunk (32 bf16 / 16 fp32 / 64 e4m3 values).  DGV2_EINVAL otherwise.
 *
 * Forward:  y [B,Ho,Wo,O] = act( conv(x [B,H,W,Cin], w [O,k*k,Cin]) + resid + bias ) * scale,  Ho = (H + 2 pad - k) / stride + 1,
 *   act 0 | 3 (leaky ReLU with `alpha`), bias [O] fp32 or NULL, resid like y or NULL (the residual sum of ResidualBlock,
 *   dusty_v2.py:343-345, costs no extra pass).  dtype DGV2_F32 | DGV2_BF16.
 * replaces: ops.Conv2d forward (gans/models/ops/common.py:187-210) at gans/models/dusty_v2.py:325-385. */
int dgv2_conv_direct_fwd(void* y, const void* x, const void* w, int B, int H, int W, int Cin, int O, int k, int stride,
                         const float* bias, const void* resid, int act, float alpha, float scale, int dtype, void* stream);
/* The whole data gradient of that conv:  gx [B,H,W,C] from gy [B,Ho,Wo,O] and the transposed weights wt [C,k*k,O], the
 * replicate-row terms of the H border included.  One launch where the pipelined kernel covers the geometry (stride 1:
 * the border rows re-weighted in place, a channel count just past a multiple of 64 as two channel ranges; stride 2: the
 * four output parity classes and the top border together), else the same sums as a sequence of launches (stride 1: main
 * + two one-row accumulate launches; stride 2: four classes + two top-border launches).  stride 2 needs k == 3 and even
 * H, W (DGV2_EINVAL).
 * resid (like gx, or NULL: the gradient of a sibling branch of the same input) is added in the epilogue of the fused
 * stride-1 3x3 form ONLY.  Where it cannot be folded -- k == 1, stride 2, or a geometry that form does not cover -- the
 * entry returns DGV2_ENOTSUP before anything is launched and gx is untouched: call again with resid = NULL and add it.
 * With resid = NULL the entry never answers DGV2_ENOTSUP.  DGV2_NO_FUSED_DGRAD (environment, A/B benchmarking) forces the
 * launch sequences.
 * replaces: the cuDNN data gradient autograd calls for ops.Conv2d (common.py:187-210) at dusty_v2.py:325-385. */
int dgv2_conv_direct_dgrad(void* gx, const void* gy, const void* wt, int B, int H, int W, int C, int O, int k, int stride,
                           const void* resid, int dtype, void* stream);

/* The 1x1 stride-1 conv as a streaming GEMM over the B * P pixels (conv1x1.hip: the slab's weights stay in LDS, the
 * activations go from 16-byte global loads straight into the matrix cores, K ascending in one fp32 accumulator, the
 * residual added to the rounded product: bit for bit what dgv2_conv_direct_fwd / _dgrad compute for the same operands):
 *   dgv2_conv1x1_fwd:    y [B,P,O]  = x [B,P,C]  . wf [O,C]^T (+ resid [B,P,O])
 *   dgv2_conv1x1_dgrad:  gx [B,P,C] = gy [B,P,O] . wt [C,O]^T (+ resid [B,P,C])
 * wf / wt: the weight bank's forward / transposed layouts (dgv2_conv_weight_bank_ex; any runtime scale already folded in);
 * no bias, no activation.  DGV2_BF16, C % 32 == 0, O % 32 == 0, contraction length (C forward, O data gradient) <= 512,
 * 16-byte aligned pointers; DGV2_ENOTSUP otherwise: callers then run dgv2_conv_direct_fwd / _dgrad on the same operands.
 * replaces: ops.Conv2d forward / data gradient (gans/models/ops/common.py:187-210) of ResidualBlock.skip behind its
 *   decimating blur (gans/models/dusty_v2.py:337-345). */
int dgv2_conv1x1_fwd(void* y, const void* x, const void* wf, int B, int P, int C, int O, const void* resid, int dtype,
                     void* stream);
int dgv2_conv1x1_dgrad(void* gx, const void* gy, const void* wt, int B, int P, int C, int O, const void* resid,
                       int dtype, void* stream);

/* The bf16 per-sample-weight contractions of the generator's two lowest levels with a deeper operand delivery
 * (gemm_stream.hip: stages of four K-steps per barrier, the next stage's loads in flight across the MFMAs, the pixel
 * operand of the NN form straight from global memory into the matrix cores, the fp32 tile of the TN form in 16-byte
 * stores).  Arguments and RESULTS are those of the generic entries, bit for bit -- every output, every sum-of-squares
 * partial and the slot it is written to (same block tile, same fragment ownership, the K-steps of 32 ascending into one
 * accumulator per fragment, the same epilogue):
 *   dgv2_gemm_stream_nn      = dgv2_bmm_nn_sq       dgv2_gemm_stream_nn_cat = dgv2_bmm_nn_cat_sq
 *   dgv2_gemm_stream_tn      = dgv2_bmm_tn          dgv2_gemm_stream_tn_cat = dgv2_bmm_tn_cat
 * Invalid arguments: DGV2_EINVAL as the generic entry.  DGV2_ENOTSUP (nothing launched; callers run the generic entry)
 * outside:  NN: DGV2_BF16 in and out, O > 64 (the generic 128-channel tile), contraction length a multiple of 32 (cat:
 * Ka % 32 == 0 and Ks % 32 == 0), ldx % 8 == 0, wstride % 8 == 0, ldy % 4 == 0, 16-byte aligned y / x / w / resid, one
 * sample's operand below 2^31 elements;  TN: DGV2_BF16, O > 32 and O % 8 == 0 (the generic 64 x 128 tile), no split-K
 * (B * ceil(O / 64) * ceil(J / 128) >= 512 or P < 1024), I % 8 == 0, ldgy % 8 == 0, ldx % 8 == 0, 16-byte aligned
 * gw / gy / x.
 * replaces: nothing new -- another engine for the grouped F.conv2d of ModConv2d.forward and its gradients
 *   (gans/models/ops/style.py:105-118) at the 4 x 32 and 8 x 64 levels of the generator (gans/models/dusty_v2.py:153-170). */
int dgv2_gemm_stream_nn(void* y, const void* x, const void* w, int B, int P, int I, int O, int ldx, int ldy,
                        int64_t wstride, const float* row_scale, const float* bias, int act, float alpha, float scale,
                        const void* resid, int dtype, int ydtype, float* sumsq, int sumsq_cap, int* sumsq_used,
                        void* stream);
int dgv2_gemm_stream_nn_cat(void* y, const void* xa, const void* xs, const void* w, int B, int P, int Ka, int Ks, int O,
                            const float* row_scale, const float* bias, int act, float alpha, float scale, int dtype,
                            int ydtype, float* sumsq, int sumsq_cap, int* sumsq_used, void* stream);
int dgv2_gemm_stream_tn(float* gw, const void* gy, const void* x, int B, int P, int I, int O, int ldgy, int ldx, int dtype,
                        void* stream);
int dgv2_gemm_stream_tn_cat(float* gw, const void* gy, const void* xa, const void* xs, int B, int P, int Ka, int Ks, int O,
                            int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * discriminator stem in one pass: BlurVH -> 1x1 conv (2 -> O) -> bias + leaky ReLU, and its backward.
 * replaces: Discriminator layers[0:3] (dusty_v2.py:364-367) = ops.BlurVH (common.py:141-155) +
 *   ops.Conv2d 1x1 (common.py:187-210) + FusedLeakyReLU (fused_act.py:20-129) and their autograd.
 * x fp32 [B,H,W] (one channel); w fp32 [O,2] (column 0 multiplies blur_v(x), column 1 blur_h(x)); O in
 * {8,16,32,64}; y, gy [B,H,W,O] fp32 or bf16.  Backward outputs gw fp32 [O,2], gb fp32 [O], gx fp32 [B,H,W]
 * (or NULL); scratch: fp32, element count from dgv2_stem_bwd_scratch.  First-order only: the R1 double
 * backward uses the composable ops. */
int dgv2_stem_fwd(void* y, const float* x, const float* w, const float* bias, int B, int H, int W, int O,
                  int ring, float alpha, float scale, int ydtype, void* stream);
int dgv2_stem_bwd_scratch(int64_t* elems, int B, int H, int W, int O);
/* The backward, optionally with the gradient of the first ResidualBlock's skip branch folded in: gsk [B,Hs,Ws,O]
 * (dtype) = dL/d(blur_down(y)),
 * the decimating blur in front of ResidualBlock.skip (gans/models/dusty_v2.py:337-345), gathered through the blur's ADJOINT
 * tables (idx_h / coef_h / cnt_h: H rows of Eh entries naming rows of gsk; idx_w / coef_w / cnt_w: W rows of Ew entries,
 * exactly the tables dgv2_resample_tab_sq takes for the adjoint pass): dL/dy = gy + blur_down^T(gsk) is never materialised
 * (it was scattered to a [B,H,W,O] tensor by one pass, added to conv1's data gradient by another and read back here).
 * gsk NULL: the stem's backward alone (dL/dy = gy); the six tables may then be NULL and Eh = Ew = Hs = Ws = 0. */
int dgv2_stem_bwd_skip(float* gx, float* gw, float* gb, float* scratch, int64_t scratch_elems, const void* gy, const void* y,
                       const float* x, const float* w, const void* gsk, const int* idx_h, const float* coef_h,
                       const int* cnt_h, int Eh, const int* idx_w, const float* coef_w, const int* cnt_w, int Ew, int Hs,
                       int Ws, int B, int H, int W, int O, int ring, float alpha, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * generator output stage: cancel the azimuth shift (circular bilinear shift),
 * scale, tanh, Gumbel-sigmoid ray-drop mask, blend.
 * replaces: dusty_v2.py:290-306 (affine_grid + grid_sample + *0.25 + tanh),
 *   dusty_v1.py:20-25 (RayDropModel), ops/gumbel.py:23-29.
 * skip fp32 [B,H,W,2] (ch0 image, ch1 raydrop_logit); shift fp32 [B] radians or NULL;
 * u fp32 [B,H,W] uniforms in (0,1); outputs fp32 [B,H,W] each.
 * backward: g_image, g_image_orig, g_logit, g_mask (any may be NULL) -> g_skip [B,H,W,2];
 * scratch fp32 [B,H,W,2] is required when shift != NULL.
 * ------------------------------------------------------------------------- */
int dgv2_gen_tail_fwd(float* image, float* image_orig, float* logit, float* mask,
                      const float* skip, const float* shift, const float* u,
                      int B, int H, int W, float out_scale, float raydrop_const, float temperature,
                      void* stream);
int dgv2_gen_tail_bwd(float* g_skip, float* scratch, const float* g_image, const float* g_image_orig,
                      const float* g_logit, const float* g_mask,
                      const float* image_orig, const float* logit, const float* mask, const float* u,
                      const float* shift, int B, int H, int W, float out_scale, float raydrop_const,
                      float temperature, void* stream);

/* ---------------------------------------------------------------------------
 * ADA resampler, separable operator form:
 *   y[b] = a[b] * (Ay[b] @ x[b] @ Cx[b]^T) + c[b]
 * replaces: AdaptiveAugment.forward geometric + colour stages,
 *   gans/augment/adaptive_augment.py:471-545 (pad, 2x upfirdn2d, grid_sample,
 *   2x upfirdn2d, colour affine).
 * x, y fp32 [B,H,W]; Ay fp32 [B,H,H]; kx fp32 [B,K] circular taps:
 *   (x Cx^T)[j] = sum_t kx[t] * x[(sgn*j + off + t) mod W], sgn[b] in {+1,-1}, off[b] int.
 * transpose = 1 applies the adjoint (backward / used for double backward).
 * ------------------------------------------------------------------------- */
int dgv2_ada_apply(float* y, const float* x, const float* Ay, const float* kx, const int* off,
                   const int* sgn, const float* a, const float* c, int B, int H, int W, int K,
                   int transpose, void* stream);

/* ADA random parameters and operator construction (three launches instead of ~160 tiny tensor ops).
 * replaces: AdaptiveAugment.sample_affine / sample_color and the geometry set-up of forward,
 *   gans/augment/adaptive_augment.py:386-469, 488-535.
 * sample: u fp32 [B,16] uniforms, n fp32 [B,8] normals, p fp32 [1] (device); policy_host = HOST array of
 *   11 floats (lr_flip, ud_flip, int_trans, iso_scale, frac_trans, brightness, contrast, luma_flip, hue,
 *   saturation multipliers, h_trans_factor) -> gaff [B,4] = (sx, tx, sy, ty), a [B], c [B].
 * build: gaff + chain constants M1y [2(3H-2),H], M1x [2(3W-2),W], taps [12] -> Ay [B,H,H], kx [B,K],
 *   off [B], sgn [B] as consumed by dgv2_ada_apply. */
int dgv2_ada_sample(float* gaff, float* a, float* c, const float* u, const float* n, const float* p,
                    const float* policy_host, int B, int H, int W, void* stream);
int dgv2_ada_build(float* Ay, float* kx, int* off, int* sgn, const float* gaff, const float* M1y,
                   const float* M1x, const float* taps, int B, int H, int W, int K, void* stream);

/* ADA image-space stages: band filter, additive noise, cutout.
 * replaces: the last third of AdaptiveAugment.forward, gans/augment/adaptive_augment.py:547-621.
 * All three are linear in the image, so they ride in the separable operator form:
 *   y[b] = mask[b] * (a[b] * (Ay'[b] @ x[b] @ Cx'[b]^T) + c'[b] + sigma[b] * eps[b]).
 * sample_img: u2 fp32 [B,8] uniforms in [0,1), n2 fp32 [B,8] standard normals, p fp32 [1] (device); policy_host =
 *   HOST array of 3 floats (imgfilter, noise, cutout multipliers).  Slot layout:
 *     u2: 0-3 band selects, 4 noise select, 5 cutout select, 6 cutout centre x, 7 cutout centre y;
 *     n2: 0-3 band log2-gains, 4 sigma (5-7 unused).
 *   -> g [B,4] band gains (per band, in order: gain 2^n2 or 1, then the whole vector divided by the root of its
 *   expected power against (10,1,1,1)/13, accumulated by product), sigma [B] = |n2[4]| * 0.1 or 0,
 *   cut [B,4] = (centre x, centre y, size x, size y) in units of the image, size 0.5 or 0.
 * fold: the per-sample band filter h = g @ fbank (fbank fp32 [NB,T], T odd; H > (T-1)/2) composed into the operators of
 *   dgv2_ada_build: Ay2 = Fy Ay (Fy: correlation with h over the reflect-padded rows), kx2 [B,K+T-1] = kx * h (h
 *   flipped for a sample with sgn = -1), off2 = off - (T-1)/2 (mod W), c2 = c * (sum h)^2.
 * apply_img: dgv2_ada_apply with the image-space terms, one read and one write of the image.  cut (fp32 [B,4]),
 *   sigma (fp32 [B]) + eps (fp32 [B,H,W] standard normals; both or neither) and c may each be NULL.  A pixel (i, j) is
 *   kept when |(j+0.5)/W - cx| >= sx/2 or |(i+0.5)/H - cy| >= sy/2 (plain distance: the box does not wrap round the
 *   ring).  transpose = 0: y = mask * (a * (Ay x Cx^T) + c + sigma * eps); transpose = 1 (adjoint): the mask is
 *   applied to the input, c / sigma / eps are ignored.  Any K; H <= 64, H % 4 == 0, K <= 80 take the LDS kernel. */
int dgv2_ada_sample_img(float* g, float* sigma, float* cut, const float* u2, const float* n2, const float* p,
                        const float* policy_host, int B, void* stream);
int dgv2_ada_fold(float* Ay2, float* kx2, int* off2, float* c2, const float* Ay, const float* kx, const int* off,
                  const int* sgn, const float* c, const float* g, const float* fbank, int B, int H, int W, int K,
                  int NB, int T, void* stream);
int dgv2_ada_apply_img(float* y, const float* x, const float* Ay, const float* kx, const int* off, const int* sgn,
                       const float* a, const float* c, const float* cut, const float* sigma, const float* eps, int B,
                       int H, int W, int K, int transpose, void* stream);

/* ---------------------------------------------------------------------------
 * range-image projection
 * replaces: CoordBridge.convert / depth_to_point_map, gans/coords.py:88-185
 * mode: 0 depth -> inv_depth_norm (the fetch_reals path, trainer.py:211-217, incl.
 *         *2-1 and mask blend when mask != NULL), out [B,1,H,W];
 *       1 inv_depth_norm -> depth, out [B,1,H,W];
 *       2 inv_depth_norm -> point_map [B,3,H,W];  3 depth -> point_map.
 * angle fp32 [1,2,H,W].
 * ------------------------------------------------------------------------- */
int dgv2_coords_convert(float* out, const float* in, const float* mask, const float* angle,
                        int B, int H, int W, float min_depth, float max_depth, float raydrop_const,
                        int mode, void* stream);

/* ---------------------------------------------------------------------------
 * surface normals of a coordinated point map (logging / visualisation path)
 * replaces: estimate_surface_normal, gans/geometry.py:38-127
 * points / out fp32 [B,3,H,W]; neighbours at distance d (replicate rows, circular columns);
 * mode 0 "closest" (pair (k,k+2) with the smallest summed distance, first minimum), 1 "mean".
 * ------------------------------------------------------------------------- */
int dgv2_surface_normal(float* out, const float* points, int B, int H, int W, int d, int mode, void* stream);

/* ---------------------------------------------------------------------------
 * non-saturating GAN objective + the logged discriminator statistics in one launch
 * replaces: GANLoss("nsgan") gans/models/loss.py:37-41,66-69 (softplus + mean), the y.mean() scalars of
 *   gans/trainer.py:400-406 and AdaptiveAugment.cumulate's sign sum (adaptive_augment.py:368-370)
 * y fp32 [n_real + n_fake] logits, reals first (either count may be 0: loss_G = mean softplus(-y_fake) is the
 * "real" formula applied to the fakes); stats fp32 [4] = loss, mean y_real, mean y_fake, sum sign(y_real);
 * gy fp32 [n_real + n_fake] = gy_scale * d loss / d y  (gy_scale: the objective's weight cfg.training.loss.gan, so that
 * gy is the cotangent the step body hands to y.backward() directly -- no scalar-loss graph, gans/trainer.py:293-297).
 * sign_cum / n_cum (both or neither, fp32 [1]): AdaptiveAugment's running statistic, updated in the same launch
 * (+= sum sign(y_real), += n_real: AdaptiveAugment.cumulate, adaptive_augment.py:368-370).
 * ------------------------------------------------------------------------- */
int dgv2_nsgan_loss(float* stats, float* gy, const float* y, int n_real, int n_fake, float gy_scale, float* sign_cum,
                    float* n_cum, void* stream);

/* ---------------------------------------------------------------------------
 * tail of the discriminator's epilogue: FusedLeakyReLU(K) + EqualLR(Linear(K, 1)) on [B, K] in one launch each way
 * replaces: ops.FusedLeakyReLU(ch(4)) + ops.EqualLR(nn.Linear(ch(4), 1)), gans/models/dusty_v2.py:383-384
 *   (fused_leaky_relu, fused_act.py:20-59,113-129: lrelu(x + b) * scale, backward masked by the sign of the OUTPUT,
 *   fused_bias_act_kernel.cu:19-60; EqualLR, common.py:158-184: gain * (bias + scale * x W^T))
 * fwd: a[b,k] = lrelu_alpha(h[b,k] + b1[k]) * act_scale (written: saved for the backward), y[b] = gain2 * (b2[0] +
 *      scale2 * sum_k w2[k] a[b,k]).  h, a fp32 [B,K]; b1 fp32 [K] or NULL; w2 fp32 [K]; b2 fp32 [1] or NULL; y fp32 [B].
 * bwd: gh[b,k] = gy[b] * gain2 * scale2 * w2[k] * (a[b,k] > 0 ? act_scale : alpha * act_scale); optional (NULL = not
 *      wanted) gb1[k] = sum_b gh[b,k], gw2[k] = gain2 * scale2 * sum_b gy[b] a[b,k], gb2[0] = gain2 * sum_b gy[b].
 *      Sums run over the batch in index order: bit-identical from run to run.
 * ------------------------------------------------------------------------- */
int dgv2_d_tail_fwd(float* y, float* a, const float* h, const float* b1, const float* w2, const float* b2, int B, int K,
                    float alpha, float act_scale, float scale2, float gain2, void* stream);
int dgv2_d_tail_bwd(float* gh, float* gb1, float* gw2, float* gb2, const float* gy, const float* a, const float* w2,
                    int B, int K, float alpha, float act_scale, float scale2, float gain2, void* stream);

/* dst fp32 [K] <- lerp(dst, mean over the B rows of src (fp32 [B, ld], ld >= K), w) in one launch.
 * replaces: Generator.moving_average_w, gans/models/base.py:89-97 (w[:, 0].mean(0) and the lerp into w_avg). */
int dgv2_colmean_lerp(float* dst, const float* src, int B, int K, int64_t ld, float w, void* stream);

/* ---------------------------------------------------------------------------
 * every random number of one step body from ONE launch
 * replaces: the torch.randn / torch.rand calls of an iteration -- Trainer.sample_z (gans/trainer.py:206-208), the azimuth
 *   shift (gans/models/dusty_v2.py:267-274), the uniforms of GumbelSigmoid (gans/models/ops/gumbel.py:23-29), the draws of
 *   AdaptiveAugment.sample_affine / sample_color (gans/augment/adaptive_augment.py:386-470), the warm-up keep mask
 *   (gans/trainer.py:241-245).
 * Philox4x32-10 (the generator torch.cuda uses); the stream state is DEVICE memory the caller owns: state uint64[4] =
 * {seed, offset, 0, 0}.  The launch advances `offset` itself (its last block to finish), so a launch captured into a
 * hipGraph draws fresh numbers on every replay.  nseg <= 16 segments: out[s] fp32 [count[s]],
 *   kind 0: uniform in [a, b);  kind 1: normal, mean a, standard deviation b;  kind 2: u in [0, 1) clamped to [a, b];
 *   kind 3: Bernoulli(a) as 0.0 / 1.0 (the valid-return mask of a synthetic scan).
 * out / count / kind / a / b are HOST arrays (read during the call).  Launches on one state must be stream-ordered.
 * ------------------------------------------------------------------------- */
int dgv2_rng_fill(float* const* out, const int64_t* count, const int* kind, const float* a, const float* b, int nseg,
                  uint64_t* state, void* stream);

/* ---------------------------------------------------------------------------
 * KITTI scan -> range image (the front end of the real-data path)
 * replaces: KITTIRaw.load_pts_as_img (scan-unfolding spherical projection, numba scatter after an argsort by depth)
 *   and the nearest resize + mask of __getitem__, gans/datasets/kitti.py:264-279,317-370
 * pts fp32 [n,4] (x, y, z, reflectance); row int32 [n] = ring index per point from the scan order (the host derives
 * it from the quadrant sequence, :328-346; -1 means ring H-1 as in the reference) or NULL for rows from the pitch angle
 * (:347-351); key = uint64 scratch [H*W]; out fp32 [6,H,Wout] = x, y, z, reflectance, depth, mask of the NEAREST point
 * of pixel (h, w * W/Wout), multiplied by the mask (min_depth <= depth <= max_depth) when apply_mask (the item of
 * __getitem__; 0 = the raw projection of load_pts_as_img).  W % Wout == 0.
 * ------------------------------------------------------------------------- */
/* ring index per point from the scan order (scan unfolding, gans/datasets/kitti.py:328-346): pts fp32 [n,4] in file order ->
 * row int32 [n] as dgv2_kitti_project takes it (0 before the first ring boundary and for rings older than H + 1 from the
 * end, -1 for the (H+1)-th from the end like the reference); counts: int32 scratch of ceil(n / 4096) entries (delimiters per
 * block of 4096 points); two launches: count, then scan + write */
int dgv2_kitti_rows(int* row, int* counts, const float* pts, int n, int H, void* stream);
int dgv2_kitti_project(float* out, unsigned long long* key, const float* pts, const int* row, int n, int H, int W,
                       int Wout, float min_depth, float max_depth, int apply_mask, void* stream);

/* ---------------------------------------------------------------------------
 * point-cloud natives of the evaluation path
 *
 * furthest point sampling + gather
 * replaces: fps.furthest_point_sampling / gather_points / gather_points_grad
 *   gans/sampling/fps/furthest_point_sampling.cpp:26-112, furthest_point_sampling.cu:37-263
 * xyz fp32 [B, n, 3]; idxs int32 [B, m]: idxs[:, 0] = 0, then m - 1 rounds of "the point with the largest distance to
 * the selected set"; points with |p|^2 <= 1e-3 never take part; equal distances resolve in the order of the
 * reference's 2^floor(log2 n) (<= 512)-thread block reduction, so the indices are the reference's.  temp: fp32
 * scratch of dgv2_fps_scratch(B, n) floats (0 for n <= 32768, where the running distances live on chip; may be NULL then).
 * gather: points fp32 [B, C, n], idx int32 [B, m] -> out [B, C, m]; grad: grad_out [B, C, m] -> grad_points [B, C, n]
 * (zero-filled here, atomic adds for repeated indices).
 * ------------------------------------------------------------------------- */
int dgv2_fps_scratch(int64_t* floats, int B, int n);
int dgv2_fps(int* idxs, float* temp, const float* xyz, int B, int n, int m, void* stream);
int dgv2_gather_points(float* out, const float* points, const int* idx, int B, int C, int n, int m, void* stream);
int dgv2_gather_points_grad(float* grad_points, const float* grad_out, const int* idx, int B, int C, int n, int m,
                            void* stream);

/* chamfer distance: nearest neighbour in both directions
 * replaces: cd.forward_cuda / cd.backward_cuda (and the CPU twins cd.forward / cd.backward)
 *   gans/metrics/distance/cd/chamfer_distance.cpp:18-144, chamfer_distance.cu:6-190
 * xyz1 fp32 [B, n, 3], xyz2 fp32 [B, m, 3]; dist1 [B, n] = min_k |xyz1_j - xyz2_k|^2 with idx1 the FIRST minimiser
 * (strict <), dist2 / idx2 [B, m] the other direction; the squared distance is ((dx*dx + dy*dy) + dz*dz) in fp32
 * without contraction, i.e. bit-identical to the reference's CPU nnsearch.  bwd: gxyz1 / gxyz2 (zero-filled here)
 * receive 2 g (a - b) at the point and -2 g (a - b) at its neighbour for both directions (float atomics).
 * ------------------------------------------------------------------------- */
int dgv2_chamfer_fwd(float* dist1, int* idx1, float* dist2, int* idx2, const float* xyz1, const float* xyz2, int B,
                     int n, int m, void* stream);
/* one direction of the above: nearest neighbour of every xyz point [B, n, 3] in ref [B, m, 3], or in ONE set ref [m, 3]
 * shared by all clouds (ref_shared = 1: the occupancy-grid voting of the JSD metric, gans/metrics/jsd.py:46-62) */
int dgv2_nn_search(float* dist, int* idx, const float* xyz, const float* ref, int B, int n, int m, int ref_shared,
                   void* stream);
int dgv2_chamfer_bwd(float* gxyz1, float* gxyz2, const float* xyz1, const float* xyz2, const float* gdist1,
                     const float* gdist2, const int* idx1, const int* idx2, int B, int n, int m, void* stream);

/* earth mover's distance by approximate matching
 * replaces: emd.approxmatch_forward / matchcost_forward / matchcost_backward
 *   gans/metrics/distance/emd/earth_mover_distance.cpp:26-95, earth_mover_distance.cu:3-364
 * xyz1 fp32 [B, n, 3], xyz2 fp32 [B, m, 3]; match fp32 [B, m, n] (written, not accumulated); temp fp32
 * [B, 2 (n + m)] scratch; cost fp32 [B] = sum match[l, k] |xyz1_k - xyz2_l|; grad1 [B, n, 3], grad2 [B, m, 3] =
 * d cost / d xyz for a FIXED match (the reference does not differentiate the matching).
 * ------------------------------------------------------------------------- */
int dgv2_emd_approxmatch(float* match, float* temp, const float* xyz1, const float* xyz2, int B, int n, int m,
                         void* stream);
int dgv2_emd_matchcost(float* cost, const float* match, const float* xyz1, const float* xyz2, int B, int n, int m,
                       void* stream);
int dgv2_emd_matchcost_grad(float* grad1, float* grad2, const float* match, const float* xyz1, const float* xyz2, int B,
                            int n, int m, void* stream);

/* all-pairs approximate-matching EMD cost without the match matrix (the distance matrices of COV / MMD / 1-NNA)
 * replaces: the (row, chunk) loop of _pairwise_distance over earth_mover_distance for the "emd" metric
 *   gans/metrics/cov_mmd_1nna.py:16-40, gans/metrics/distance/emd/earth_mover_distance.cu:3-226
 * xyz1 fp32 [B1, n, 3], xyz2 fp32 [B2, m, 3]; cost fp32 [B1, B2] (written), cost[i, j] = what dgv2_emd_matchcost returns
 * for dgv2_emd_approxmatch(xyz1[i], xyz2[j]); NOT divided by the point count.
 * arithmetic, per pair: remainL = multiL, remainR = multiR (the integer quotients max(m / n, 1), max(n / m, 1)); for
 * level = -4^j, j = 7 .. -1, with e_kl = __expf(level |x1_k - x2_l|^2):
 *   ratioL_k = remainL_k / (1e-9 + sum_l e_kl remainR_l)
 *   s_l = remainR_l sum_k e_kl ratioL_k;  ratioR_l = min(remainR_l / (s_l + 1e-9), 1) remainR_l;  remainR_l = max(0, remainR_l - s_l)
 *   w_kl = e_kl ratioR_l ratioL_k;  cost += w_kl |x1_k - x2_l|;  remainL_k = max(0, remainL_k - sum_l w_kl)
 * (the state arithmetic is that of dgv2_emd_approxmatch, term for term; |.| is the hardware square root, 1 ulp)
 * One workgroup of 1024 lanes per pair, grid (B2, B1); the four state arrays (2 (n + m) floats) and a 16 KB tile of the
 * other cloud live in LDS; no workspace, no memset, no atomics.  A lane's cost chain is in fixed order: levels outer,
 * then its own points k = lane, lane + 1024, ..., then l ascending (9 ceil(n / 1024) m adds); one fixed-tree block sum
 * (6 butterfly steps, then the 16 wave partials in order) ends it: the same bits for a pair wherever it sits in the grid.
 * n, m >= 1 and n + m <= DGV2_EMD_PAIR_MAX_POINTS (state + tile = 48 KB of LDS); B1 <= 65535.  DGV2_ENOTSUP above the
 * cap (callers fall back to the batched entries above), DGV2_EINVAL for null pointers or a bad shape; nothing is
 * launched in either case.  No gradient.
 * ------------------------------------------------------------------------- */
#define DGV2_EMD_PAIR_MAX_POINTS 4096
int dgv2_emd_pairwise_cost(float* cost, const float* xyz1, const float* xyz2, int B1, int B2, int n, int m,
                           void* stream);

/* ---- fp8 (OCP e4m3) operands for the decimating branch convs of the discriminator (BASELINE configs[4]) --------------
 * The two tensors of a ResidualBlock (gans/models/dusty_v2.py:325-345) that exist only as MFMA operands -- the blurred
 * activation in front of the 3x3 stride-2 conv2 and the blur-decimated block input in front of the 1x1 skip conv -- are
 * written as e4m3 (unit scale) by the FIR kernels that produce them, the two convs' weights as e4m3 with a per-tensor
 * power-of-two scale; v_mfma_f32_16x16x32_fp8_fp8 contracts them with fp32 accumulation.  The residual stream and the
 * activation outputs read by a backward pass stay bf16; the weight-gradient stream reads the saved e4m3 tensor through
 * dgv2_fp8_dequant.  The reference's reduced-precision switch: gans/models/dusty_v2.py:388-394 (fp16 autocast). */
/* y8 [B,H,W,C] (e4m3 bytes) = R x for a same-size separable resampling: dgv2_fir_same_mfma with the result rounded to
 * e4m3 (saturating at +-448) at the store.  replaces: Resample(up = down = 1) / Blur, gans/models/ops/common.py:105-135. */
int dgv2_fir_same_mfma_q8(void* y8, const void* x, const void* bands, int B, int C, int H, int W, void* stream);
/* dgv2_resample_tab_sq (x bf16, tables as there) with the result stored as e4m3 bytes y8 [B,out_h,out_w,C]; C % 8 == 0,
 * Ew <= 4, Eh <= 64, else DGV2_ENOTSUP.  replaces: Resample, gans/models/ops/common.py:105-135. */
int dgv2_resample_tab_q8(void* y8, const void* x, const int* idx_h, const float* coef_h, const int* cnt_h, int Eh,
                         const int* idx_w, const float* coef_w, const int* cnt_w, int Ew, int B, int C, int in_h,
                         int in_w, int out_h, int out_w, void* stream);
/* n <= 16 conv weights in one launch pair: w8[l] [O,kk,C] = e4m3(src[l] [O,C,kk] fp32 * 2^k_l), 2^k_l the largest power of
 * two with max|src[l]| * 2^k_l <= 448; descale[l] (device, fp32) = eq[l] / 2^k_l -- the factor the conv epilogue puts on
 * its accumulator (eq = the EqualLR factor).  amax: n words of device scratch.  w8 / src / O / C / kk / eq: HOST arrays.
 * C % 8 == 0.  replaces: the `weight * scale` operand of ops.Conv2d, gans/models/ops/common.py:158-210. */
int dgv2_fp8_quant_weights(void* const* w8, const void* const* src, const int* O, const int* C, const int* kk,
                           const float* eq, int n, float* descale, void* amax, void* stream);
/* y (bf16) = x (e4m3) * scale for n elements, n % 16 == 0: the saved e4m3 activations as the bf16 operand of the
 * weight-gradient stream (dgv2_conv_wgrad_stream_pl). */
int dgv2_fp8_dequant(void* y, const void* x, int64_t n, float scale, void* stream);
/* dgv2_conv_direct_fwd on e4m3 operands x8 [B,H,W,Cin], w8 [O,k*k,Cin] (same shapes, padding and epilogue; y / resid bf16):
 *   y (bf16) = act( acc * acc_scale[0] + resid + bias ) * scale,  acc_scale a DEVICE scalar (dgv2_fp8_quant_weights).
 * Cin % 64 == 0, O >= 64; DGV2_ENOTSUP otherwise (callers then run the bf16 conv).  replaces: ops.Conv2d forward
 * (gans/models/ops/common.py:187-210) of ResidualBlock.conv2 / .skip (gans/models/dusty_v2.py:331-345). */
int dgv2_conv_direct_fwd_fp8(void* y, const void* x8, const void* w8, const float* acc_scale, int B, int H, int W, int Cin,
                             int O, int k, int stride, const float* bias, const void* resid, int act, float alpha,
                             float scale, void* stream);

/* Grouped small Linear layers in fp32 on the matrix cores (glin.hip): L <= 24 layers that share the batch B and the
 * input width K in ONE launch, the layers' parameter addresses as HOST arrays (they travel by value in the kernel
 * arguments).  y_l [B,N_l] = act( alpha * PN(x_l) W_l^T + beta * bias_l ): x_l rows of K floats at row stride lda[l]
 * (a style vector inside ws [B,S,K]: lda = S*K), W_l [N_l,K], bias_l [N_l] or NULL; act 0 | 1 = leaky ReLU(slope);
 * prenorm: rows normalised by rsqrt(mean_k x^2 + 1e-8) first, the factors stored in rnorm [B] when given.
 * Exact fp32 (v_mfma_f32_16x16x4_f32 = fmaf chains).  K % 64 == 0.
 * replaces: PixelNorm + EqualLR(nn.Linear) + LeakyReLU of MappingNetwork (gans/models/dusty_v2.py:13-29,
 * ops/common.py:158-184,213-223) and the style affine ModConv2d.mod of every modulated conv (ops/style.py:30,75). */
int dgv2_glin_fwd(float* const* y, const float* const* x, const float* const* w, const float* const* bias, const int* N,
                  const int* lda, int L, int B, int K, float alpha, float beta, int act, float slope, int prenorm,
                  float* rnorm, void* stream);
/* Its input gradient: dx [B,K] at row stride ldx (=|+= when accumulate) alpha * sum_l (g_l . act'(y_l)) W_l over the L
 * layers that read this input; g_l, y_l [B,N_l] contiguous (yact entries NULL: no activation), N_l % 32 == 0.  The
 * contraction over all layers' features runs in chunks of 256 (one block each) whose partials a second kernel folds in
 * fixed order: scratch fp32 [>= B * K * sum_l ceil(N_l / 256)]. */
int dgv2_glin_dinput(float* dx, int ldx, float* scratch, int64_t scratch_elems, const float* const* g,
                     const float* const* yact, const float* const* w, const int* N, int L, int B, int K, float alpha,
                     float slope, int accumulate, void* stream);
/* ... and the parameter gradients of all L layers in one launch: dW_l [N_l,K] = alpha * (g_l . act'(y_l))^T (x_l * rnorm),
 * dbias_l [N_l] = beta * column sums (dbias or entries NULL: skipped); x_l rows at stride ldx[l], rnorm [B] or NULL. */
int dgv2_glin_dweight(float* const* dw, float* const* dbias, const float* const* g, const float* const* yact,
                      const float* const* x, const int* N, const int* ldx, int L, int B, int K, float alpha, float beta,
                      float slope, const float* rnorm, void* stream);

/* ---------------------------------------------------------------------------
 * GAN inversion (inversion.hip).  All fp32, NCHW, ring convention of ops.Pad(1, "replicate", ring=True): circular
 * along W, replicate along H; a level [Hi,Wi] pools to [(Hi+1)/2, (Wi+1)/2].  Every entry is ONE launch (one block per
 * sample walks the levels; per-sample sums are fixed-order block reductions: run-to-run bit-identical, no atomics).
 * L <= 16 levels; every pooled level has Wi >= 2.
 *
 * Target pyramid, once per target.  replaces: the ref / mask side of MultiScaleMaskedLoss.forward, update_mask and
 *   blurpool, gans/inversion.py:45-76 (which recomputes it on every call).
 * ref [B,C,H,W], mask [B,1,H,W] -> refp: levels 0 .. L-1 of ref ([B,C,Hi,Wi] each, level after level); maskp, normp:
 * [B,Hi,Wi] per level in the same order (normp's level i is the norm that scales level i = 9 / window count of level
 * i-1's mask, 9 where the count is 0; its level 0 is not written); invm [L,B] = 1 / (sum(mask_i) + 1e-8).
 * ------------------------------------------------------------------------- */
int dgv2_msml_prepare(float* refp, float* maskp, float* normp, float* invm, const float* ref, const float* mask, int B,
                      int C, int H, int W, int L, void* stream);
/* The loss: loss [B] = sum_i masked_loss(ref_i, gen_i, mask_i), gen_{i+1} = blurpool(gen_i mask_i) norm_{i+1}.
 * replaces: masked_loss and the gen side of MultiScaleMaskedLoss.forward, gans/inversion.py:23-29,64-76 (without the
 *   blurpool after the last level, whose result the reference discards).
 * metric 0 = F.l1_loss, 1 = F.mse_loss; relative: (loss mask) / (ref + 1e-11), then mask again, as the reference.
 * genp: levels 1 .. L-1 of the generated pyramid (refp's layout less level 0; NULL when L == 1), kept for backward. */
int dgv2_msml_fwd(float* loss, float* genp, const float* gen, const float* refp, const float* maskp, const float* normp,
                  const float* invm, int B, int C, int H, int W, int L, int metric, int relative, void* stream);
/* ggen [B,C,H,W] = gloss[b] * d loss[b] / d gen (sign(0) = 0 for l1).  gscratch: genp's size, the gradients of levels
 * 1 .. L-1 on their way down.  replaces: autograd through gans/inversion.py:23-29,48-76. */
int dgv2_msml_bwd(float* ggen, float* gscratch, const float* gloss, const float* gen, const float* genp,
                  const float* refp, const float* maskp, const float* normp, const float* invm, int B, int C, int H, int W,
                  int L, int metric, int relative, void* stream);
/* Input gradient of dgv2_coords_convert (same modes, same in / mask / angle): gx [B,1,H,W] from gout ([B,1,H,W], modes
 * 2 / 3: [B,3,H,W]).  The validity masks are constants, d(1/(x+tol)) = -1/(x+tol)^2, mode 0 with a mask carries the
 * factor 2 mask of its blend.  replaces: autograd through CoordBridge.convert, gans/coords.py:88-185
 *   (demo_inversion.py:169 differentiates inv_depth_norm -> depth_norm). */
int dgv2_coords_convert_bwd(float* gx, const float* gout, const float* in, const float* mask, const float* angle, int B,
                            int H, int W, float min_depth, float max_depth, int mode, void* stream);
/* Angle gradient of dgv2_fourier_feature: g [B,H,W,ld] (dtype) holds the gradient of the encoding in channels
 * [c0, c0+2F) -> g_angle fp32 [B,2,H,W], g_a = sum_f freqs[f,a] (g_sin[f] cos c_f - g_cos[f] sin c_f) with c_f
 * recomputed from angle [Ba,2,H,W] (+ shift [B] on the azimuth).  replaces: autograd through the 1x1 conv + sin / cos
 *   of gans/models/ops/fourier.py:77-82 (demo_inversion.py:164 optimises angle + phase). */
int dgv2_fourier_feature_bwd(float* g_angle, const void* g, const float* angle, const float* shift, const float* freqs,
                             const float* phase, int B, int Ba, int H, int W, int F, int ld, int c0, int dtype,
                             void* stream);

/* ---------------------------------------------------------------------------
 * frame post-processing of a latent walk (gans/interpolation.py)
 * replaces: demo_interpolation.py:79-86 (tanh_to_sigmoid, CoordBridge.convert to a point map, kornia median_blur
 *   (3, 3), convert to a normal map, tanh_to_sigmoid, / max_depth, two rearranges) -- ONE launch.
 * image fp32 [B,1,H,W] in [-1,1] (the generator's "image"), angle fp32 [1,2,H,W] ->
 *   points fp32 [B,H*W,3] = median3x3(point_map((image + 1) / 2)) / max_depth, the conversion being that of
 *   dgv2_coords_convert mode 2; colors fp32 [B,H*W,3] = (1 - n) / 2 with n the dgv2_surface_normal (d = 2, "closest")
 *   of points, NaN -> 0.
 * border: what the median's window sees outside the image: 0 zeros (kornia), 1 replicate rows / circular columns.
 *   The normal's neighbour at a clamped row / wrapped column is the median AT that pixel under this rule.
 * DGV2_EINVAL where dgv2_surface_normal rejects (W <= 2, empty shapes, null pointers) and for another border.
 * ------------------------------------------------------------------------- */
int dgv2_frame_points(float* points, float* colors, const float* image, const float* angle, int B, int H, int W,
                      float min_depth, float max_depth, int border, void* stream);
/* Colour lookup.  replaces: colorize, gans/utils.py:167-191 (mul, clamp, long, embedding, permute).
 * x fp32 [B,H,W], lut fp32 [n_colors,3] -> out fp32 [B,3,H,W] = lut[(long) clamp(x * n_colors, 0, n_colors - 1)]. */
int dgv2_colorize(float* out, const float* x, const float* lut, int B, int H, int W, int n_colors, void* stream);

/* ---------------------------------------------------------------------------
 * CRF-RNN refinement layer of the range-image segmentation models (crf.hip; semseg/models/crf_as_rnn.py here)
 * replaces: CRFRNN.forward and autograd through it, semseg/models/crf_as_rnn.py:110-132 (F.unfold + einops + a Python
 *   loop over samples over a materialised [B,C,K-1,H*W] bilateral kernel).
 * All fp32, NCHW.  unary U [B,C,H,W], xyz [B,3,H,W], mask m [B,H,W] (multiplied in; may be non-binary),
 * kernel_gamma / kernel_alpha [C,C,kh,kw] (only the diagonal [c,c] is read: g_c, a_c), theta_beta [C],
 * weight_smoothness ws / weight_appearance wa [C], compat M [C,C] (label_compatibility.weight[:, :, 0, 0]).
 * n runs over the kh*kw window offsets; a position outside the image contributes 0.  Q = U, then num_iters times
 *   P      = softmax(Q, dim=1)
 *   S_c(p) = sum_n g_c(n) P_c(p+n)                L_c(p) = sum_n a_c(n) P_c(p+n)      (centre taps read from the buffers)
 *   A_c(p) = m(p) sum_{n != 0} beta_c(p,n) m(p+n) P_c(p+n),   beta_c(p,n) = exp(-|xyz(p+n) - xyz(p)|^2 / (2 theta_beta[c]^2))
 *   T_c    = ws[c] S_c + wa[c] A_c L_c
 *   Q_c    = U_c - sum_c' M[c,c'] T_c'
 * One launch per iteration; beta is recomputed from xyz staged in LDS.  out [B,C,H,W]; qsave [num_iters-1][B,C,H,W]
 * receives the inputs Q of iterations 1 .. num_iters-1 (iteration 0's is U), which is what the backward reads (NULL
 * when num_iters == 1).
 * Backward of one iteration, given the cotangent dQ' of its output (beta is symmetric, so one gather stencil serves):
 *   dU += dQ'      dM[c,c'] = -sum_{b,p} dQ'_c T_c'      dT_c' = -sum_c M[c,c'] dQ'_c
 *   dws[c] = sum_{b,p} dT_c S_c      dwa[c] = sum_{b,p} dT_c A_c L_c      dS = ws dT    dL = wa dT A    dA = wa dT L
 *   dP_c(q) = sum_n [g_c(-n) dS_c(q+n) + a_c(-n) dL_c(q+n)] + m(q) sum_{n != 0} beta_c(q,n) m(q+n) dA_c(q+n)
 *   dQ_c    = P_c (dP_c - sum_c' P_c' dP_c')
 * Two launches per iteration plus one finishing launch: g_unary [B,C,H,W], g_weight_smoothness / g_weight_appearance
 * [C], g_compat [C,C], all overwritten; the parameter gradients are per-block partial sums in `scratch` (fp32,
 * >= dgv2_crf_rnn_backward_scratch elements) folded in a fixed order: no float atomics, bit-identical from run to run.
 * xyz and mask get no gradient (the reference detaches the bilateral kernel; the mask is data).
 * 1 <= C <= 8; kh, kw odd, kh <= 5, kw <= 9; any H, W >= 1; num_iters >= 1.  DGV2_EINVAL outside that range, for null
 * pointers, empty shapes and a short scratch.
 * ------------------------------------------------------------------------- */
int dgv2_crf_rnn_forward(float* out, float* qsave, const float* unary, const float* xyz, const float* mask,
                         const float* kernel_gamma, const float* kernel_alpha, const float* theta_beta,
                         const float* weight_smoothness, const float* weight_appearance, const float* compat, int B,
                         int C, int H, int W, int kh, int kw, int num_iters, void* stream);
int dgv2_crf_rnn_backward_scratch(int64_t* elems, int B, int C, int H, int W, int num_iters);
int dgv2_crf_rnn_backward(float* g_unary, float* g_weight_smoothness, float* g_weight_appearance, float* g_compat,
                          float* scratch, int64_t scratch_elems, const float* g_out, const float* qsave,
                          const float* unary, const float* xyz, const float* mask, const float* kernel_gamma,
                          const float* kernel_alpha, const float* theta_beta, const float* weight_smoothness,
                          const float* weight_appearance, const float* compat, int B, int C, int H, int W, int kh,
                          int kw, int num_iters, void* stream);

/* ---------------------------------------------------------------------------
 * kNN label filter of the range-image segmentation models (knn.hip; semseg/models/knn.py here)
 * replaces: kNN2d.forward, semseg/models/knn.py:38-76 (the RangeNet++ filter: F.unfold + a K-channel depthwise conv
 *   over a [B,1,K,H*W] tensor + topk + two gathers + scatter_add_ into [B,1,C+1,H*W] + argmax).
 * depth fp32 [B,1,H,W], label int64 [B,H,W], dist_kernel fp32 [kh,kw] (the module's buffer) -> out int64 [B,H,W].
 * All arithmetic in fp32.  K = kh*kw window slots with offsets o_k in row-major order, ph = kh/2, pw = kw/2:
 *   nb_k(q)   = depth(q + o_k), 0 outside the image (unfold's padding), then +inf where that is < 0; the anchor
 *               depth(q) is used raw
 *   jump_k(q) = |nb_k(q) - depth(q)| for q inside the image, 0 for q outside (the conv's padding)
 *   dist_k(p) = sum_j w(o_j) jump_k(p + o_j)
 *   w         = 1 - G / sum G,  G(dy,dx) = exp(-(dy^2 + dx^2) / (2 sigma^2)): built by the caller in float32 exactly
 *               as the reference's get_gaussian_kernel does and passed as dist_kernel
 * The k slots of smallest dist_k(p) are selected; ties go to the lower slot index (the reference's
 * topk(sorted=False) leaves ties unspecified: this is the definition here).  A selected slot votes for
 * label(p + o_k), 0 outside the image; with cutoff > 0 a slot with dist_k(p) > cutoff votes for the discarded bin
 * instead, and so does a label outside [0, num_classes) (the reference raises there).  out(p) is the class of
 * [0, num_classes) with the most votes; ties and "no votes" go to the lowest class, as argmax does.
 * One launch; a block stages depth with a halo of (2 ph, 2 pw) and the labels with a halo of (ph, pw) in LDS and
 * computes the rest from there; num_classes is unbounded (the vote counts equal labels pairwise).
 * Supported: kh, kw odd and <= 5 with kh*kw > 1 (a 1 x 1 window has w = 0, hence 0 * inf), 1 <= k <= kh*kw,
 * num_classes >= 1, any B, H, W >= 1, cutoff not NaN.  DGV2_EINVAL outside that range and for null pointers.
 * ------------------------------------------------------------------------- */
int dgv2_knn2d(int64_t* out, const float* depth, const int64_t* label, const float* dist_kernel, int B, int H, int W,
               int kh, int kw, int k, int num_classes, float cutoff, void* stream);
/* Confusion counts of a segmentation evaluation (segcount.hip).  replaces: the per-class masked sums of evaluate,
 * test_semseg.py:23-42, after preds * mask and label * mask of its lines 136-137.
 * label, pred int64 [n], mask fp32 [n] or NULL; conf int64 [C+1,C+1] is ACCUMULATED INTO (the caller zeroes it once
 * per evaluation): conf[row(label), col(pred)] += 1 per pixel, where a value of [0,C) is its own row / column and any
 * other value the last one.  Where mask == 0 both label and prediction count as 0; any other mask value (the
 * datasets' masks are binary) counts as 1.  tp_c = conf[c,c], fp_c = sum_r conf[r,c] - tp_c, fn_c = sum_r conf[c,r] -
 * tp_c over all C+1 rows / columns.  Integer atomics only: bit-identical from run to run.
 * 1 <= num_classes <= 32, 1 <= n < 2^40; DGV2_EINVAL otherwise and for null conf / label / pred. */
int dgv2_seg_confusion(int64_t* conf, const int64_t* label, const int64_t* pred, const float* mask, int64_t n,
                       int num_classes, void* stream);

/* ---------------------------------------------------------------------------
 * training objective of the range-image segmentation models (segloss.hip; semseg/models/loss.py here)
 * replaces: FocalLoss.forward, semseg/models/loss.py:13-21 (cross_entropy + softmax + gather + pow + mul), under
 *   masked_loss, train_semseg.py:194-197 (* mask, sum, mask.sum(), div), the argmax of its lines 270-273 and the
 *   pred * mask, label * mask and masked sums of `evaluate` of its lines 290-296 -- and autograd through all of it.
 * logit [B,C,H,W] NCHW contiguous of `dtype` (DGV2_F32, DGV2_BF16 or DGV2_F16), label int64 [B,H,W], mask fp32
 * [B,H,W] or NULL (= 1 everywhere), alpha fp32 [C] or NULL (= 1 for every class).  All arithmetic in fp32, whatever
 * the dtype.  Per pixel q with logits z_0..z_{C-1}, label y, mask m, class weights a_c:
 *   p_c     = softmax(z)_c                    (max-subtracted)
 *   lp      = log p_y                         (= z_y - max - log sum exp(z - max))
 *   w       = (1 - p_y)^gamma                 (gamma == 0: w = 1 exactly, also where p_y == 1; 1 - p_y is taken as
 *                                              sum_{c != y} exp(z_c - max) / sum_c exp(z_c - max): no cancellation)
 *   L(q)    = -a_y w lp
 *   loss    = sum_q m(q) L(q) / sum_q m(q)    (sum m == 0: 0 / 0 = NaN, as the reference)
 *   dL/dz_j = a_y (delta_jy - p_j) (gamma p_y (1 - p_y)^(gamma-1) lp - (1 - p_y)^gamma)
 *             (gamma == 0: a_y (p_j - delta_jy), plain weighted cross-entropy)
 *   g_z(q)_j = gout m(q) / sum m * dL/dz_j    (per_pixel: gout(q) dL/dz_j, no mask, no sum)
 * gamma == 0 or gamma >= 1: for 0 < gamma < 1 the reference's own gradient is NaN wherever p_y rounds to 1.
 * A label outside [0, C) has L = 0 and a zero gradient, and its mask weight still counts in sum m (the reference raises
 * or device-asserts there; this is the definition here).  The mask is a float WEIGHT for the loss and a FLAG for pred /
 * conf: mask == 0 there means "count as class 0", any other value 1 -- the rule of dgv2_seg_confusion.
 * pred(q) = lowest index among the largest logits (compared in the logits' own dtype; unspecified where a logit is
 * NaN, and the loss is NaN there), times (m != 0).  conf int64 [C+1,C+1] is ACCUMULATED INTO: conf[row(label (m != 0)), col(pred)] += 1 with
 * the rows / columns of dgv2_seg_confusion; integer atomics only, per block in LDS first.
 *
 * dgv2_seg_loss_forward.  Outputs, each NULL when not wanted (at least one is): loss_map fp32 [B,H,W] = L(q), unmasked
 * (the reference's reduction="none"); pred int64 [B,H,W]; conf; sums fp32 [3] = {loss, sum m L, sum m}.  ONE launch does
 * the per-pixel work; with `sums` a SECOND launch of one block folds the blocks' partial sums, which the first left in
 * `scratch` (fp32, >= dgv2_seg_loss_scratch elements; required with sums), in a fixed order and divides: no float
 * atomics, bit-identical from run to run, and the same bits for bf16 / fp16 logits as for their fp32 cast.
 * The logits are read from HBM once: C <= 8 holds a pixel's C values in registers; 8 < C <= 32 walks the class planes
 * twice (three times in the backward), the re-reads served by the cache.  Each thread reads 4 consecutive pixels of a
 * plane with one 16-byte (fp32) / 8-byte (half) load where every pointer is 16-byte aligned and H*W % 4 == 0, and
 * element by element otherwise, with the same results.
 * dgv2_seg_loss_backward.  ONE launch, no scratch, no atomics: g_logit [B,C,H,W] in the logits' dtype (fp32 rounded to
 * nearest even), the softmax recomputed.  per_pixel == 0: gout is ONE device float (the loss's upstream gradient) and
 * sums the forward's (sum m is read from sums[2] on the device: nothing is read on the host, the step stays
 * capturable).  per_pixel == 1: gout fp32 [B,H,W] (the cotangent of loss_map); mask and sums are not read.
 * DGV2_EINVAL, nothing launched: a null required pointer (logit, label; forward: every output null, or sums without
 * enough scratch; backward: g_logit, gout, sums when per_pixel == 0), B, H or W < 1, C outside 1..32, another dtype,
 * gamma outside {0} U [1, inf) (NaN included), B*H*W >= 2^40, per_pixel not 0 / 1.
 * ------------------------------------------------------------------------- */
int dgv2_seg_loss_scratch(int64_t* elems, int B, int H, int W);
int dgv2_seg_loss_forward(float* loss_map, int64_t* pred, int64_t* conf, float* sums, float* scratch,
                          int64_t scratch_elems, const void* logit, const int64_t* label, const float* mask,
                          const float* alpha, int B, int C, int H, int W, float gamma, int dtype, void* stream);
int dgv2_seg_loss_backward(void* g_logit, const void* logit, const int64_t* label, const float* mask,
                           const float* alpha, const float* gout, const float* sums, int B, int C, int H, int W,
                           float gamma, int dtype, int per_pixel, void* stream);

/* ---------------------------------------------------------------------------
 * Fire module of the SqueezeSeg trunks, evaluation mode (fire.hip; semseg/models/squeezeseg_v1.py / _v2.py here)
 * replaces: Fire.forward, semseg/models/squeezeseg_v2.py:39-56 and squeezeseg_v1.py:8-24, over the ConvReLU /
 *   ConvReLUNorm / DeconvReLU sequences of semseg/models/common.py:56-111 (conv, ReLU, eval batch norm, transposed conv,
 *   cat), and the decoder's residual adds of squeezeseg_v2.py:169-172 -- 10 to 13 launches -- with ONE launch.
 * x [B,Cin,H,W], skip (or NULL) and y [B,E1+E3,H,Wout] are contiguous NCHW of one `dtype` (DGV2_F32, DGV2_BF16 or
 * DGV2_F16); Wout = 2 W with `up`, else W.  Every parameter is float32 in the layout of its torch module:
 * w_s [Cs,Cin,1,1], w_d [Cs(in),Cs(out),1,4] (ConvTranspose2d), w_1 [E1,Cs,1,1], w_3 [E3,Cs,3,3], biases per channel.
 *   s  = N_s(relu(W_s x + b_s))
 *   u  = relu(sum_{ci,k} s[ci][h][w] w_d[ci][co][0][k] + b_d[co])  over the taps (w, k) with w' = 2 w - 1 + k and
 *        0 <= w < W (others dropped)                      only with `up`; else u = s
 *   e1 = N_1(relu(W_1 u + b_1))
 *   e3 = N_3(relu(W_3 * u + b_3))         3x3, zero padding 1 APPLIED TO u: a position outside the image contributes 0,
 *                                         not N_s(relu(b_s)) and not the squeeze of a clamped or wrapped pixel
 *   y  = cat(e1, e3) [+ skip]
 * N(v) = (v - mean) * (gamma * (1 / sqrtf(var + eps))) + beta per channel, in float32, folded in the kernel from the
 * four vectors (correctly rounded divide and square root); the four pointers of a set all NULL: no batch norm (V1's
 * ConvReLU).  Accumulation is float32 throughout.  DGV2_F32 runs the exact f32-input MFMA (one k-ordered fmaf chain per
 * output); the 16-bit dtypes convert the weights to that dtype in registers, hold s and u in it (one rounding each)
 * and run the 16x16x32 MFMA.  No tensor with Cs channels reaches memory; no atomics, no scratch buffer; the output
 * bits do not depend on the grid.
 * Range: Cin, Cs, E1, E3 multiples of 16, 16 <= Cin <= 512, 16 <= Cs <= 64, 16 <= E1, E3 <= 256; B, H, W >= 1.
 * DGV2_EINVAL, nothing launched and y untouched: outside that range, another dtype, a null required pointer (y, x,
 * the four conv weights and biases; w_d / b_d exactly when up == 1), a conv weight that is not 16-byte aligned (they
 * are read with 16-byte loads), a batch-norm set that is partly null, a negative or NaN eps, up not 0 / 1, more than
 * 2^31 - 1 blocks.
 * ------------------------------------------------------------------------- */
int dgv2_fire_fwd(void* y, const void* x, const void* skip, const float* w_s, const float* b_s, const float* g_s,
                  const float* beta_s, const float* mean_s, const float* var_s, const float* w_d, const float* b_d,
                  const float* w_1, const float* b_1, const float* g_1, const float* beta_1, const float* mean_1,
                  const float* var_1, const float* w_3, const float* b_3, const float* g_3, const float* beta_3,
                  const float* mean_3, const float* var_3, float eps_s, float eps_1, float eps_3, int B, int Cin,
                  int Cs, int E1, int E3, int H, int W, int up, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Context aggregation module (CAM) of SqueezeSegV2, evaluation mode (cam.hip; semseg/models/squeezeseg_v2.py here)
 * replaces: the reference's context-aggregation class, semseg/models/squeezeseg_v2.py:20-36 -- MaxPool2d(7, 1, 3),
 *   Conv2d(C, Cr, 1), ReLU, Conv2d(Cr, C, 1), Sigmoid and the multiply: six launches -- with ONE launch.
 * x and y [B,C,H,W] are contiguous NCHW of one `dtype` (DGV2_F32, DGV2_BF16 or DGV2_F16) and do not overlap (a
 * block reads the halo of pixels that another block writes).  Every parameter is float32
 * in the layout of its torch module: w1 [Cr,C,1,1], b1 [Cr], w2 [C,Cr,1,1], b2 [C].  Per sample and pixel (h, w):
 *   m[c] = max of x[c][h'][w'] over |h' - h| <= 3, |w' - w| <= 3 INSIDE the image: the padding is -inf, not 0, so a
 *          window never sees a value that is not in x (max is exact in every dtype)
 *   a[j] = relu(t_C + b1[j]),  t_0 = 0, t_{c+1} = fmaf(w1[j][c], m[c], t_c)        c = 0 .. C-1 in increasing order
 *   s[c] = u_Cr + b2[c],       u_0 = 0, u_{j+1} = fmaf(w2[c][j], a[j], u_j)        j = 0 .. Cr-1 in increasing order
 *   g[c] = 1 / (1 + expf(-s[c]))                                                   (correctly rounded divide)
 *   y[c] = x[c] * g[c]                                                             rounded once to `dtype`
 * all in float32: the parameters are used as they are, m is converted exactly, a and g are never rounded to the
 * activations' dtype.  m reaches LDS and registers only (a separable row-then-column maximum over a haloed 8 x 32
 * tile, eight channels at a time; the parameters are staged once per block in LDS); no atomics, no workspace; each
 * output is one fixed-order chain of its own pixel, so its bits depend neither on the grid nor on the batch.  A NaN
 * in x is dropped by the maximum where torch's pool propagates it.
 * Range: C a multiple of 16, 16 <= C <= 128; 1 <= Cr <= 8; B, H, W >= 1; C*H*W <= 2^31 - 1 (offsets inside a sample are
 * 32-bit).  DGV2_EINVAL, nothing launched and y untouched: outside that range, another dtype, a null pointer, more than
 * 2^31 - 1 blocks.
 * ------------------------------------------------------------------------- */
int dgv2_cam_fwd(void* y, const void* x, const float* w1, const float* b1, const float* w2, const float* b2, int B,
                 int C, int Cr, int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Bird's-eye view of a point cloud, and the bilinear splat under it (bev.hip; gans/render.py here)
 * replaces: render.py:21-127 -- render_point_clouds (kornia's pinhole projection, the mask, the depth weight) and
 *   bilinear_rasterizer: about 70 tensor-op launches over [B,N,C] temporaries with four float scatter_add_ calls, whose
 *   sums depend on the arrival order -- with three launches (clear, splat, resolve) whose output bits do not.
 * dgv2_bev_render: points [B,N,3], colors [B,N,C] (1 <= C <= 4, values in [-1, 1]), R [3,3] or NULL, t [3] or NULL,
 * out [B,C,size,size], all float32 and contiguous.  Per point, in float32:
 *   p = (x, y, -z);  p = p . R (row vector times matrix) if R;  p += t if t
 *   s = 1 / (p_z + 1e-8) if |p_z| > 1e-8 else 1;   u_k = (p_k * s * focal + 0.5) * size, k = x, y   (principal point
 *       0.5; a point behind the camera projects too, mirrored)
 *   keep = 0 < u_x < size - 1 and 0 < u_y < size - 1 (strict);  row = size - u_x, col = size - u_y
 *   d = |p|;  e = expf(-3 d) if d > 1e-8 else 0
 *   for the four corners (floor(row) + i, floor(col) + j), i, j in {0, 1}, with the bilinear weight b: a corner outside
 *   [0, size - 1]^2 or with b < 1e-3 is dropped;  num[c] += (e * b) * colors[c] if keep;  den += e * b  (a point that is
 *   not kept still dilutes its pixels)
 *   out = num / (den + 1e-8)                                               (in double, rounded once to float)
 * dgv2_bilinear_splat: the same splat with e = 1, keep = 1, the raster coordinates given (coords [B,N,2] = (row, col))
 * and no division: out [B,C,H,W] = sum of b * values[c] (values [B,N,C] in [-1, 1]).
 * Accumulation is in 64-bit integers: each addend is saturated to [-1, 1], scaled by 2^40 (exact for a float), rounded
 * to an integer and added with an integer atomic.  Integer addition is associative: the output is bit-identical from
 * run to run and under any permutation of the points.  Only bits below 2^-40 of an addend are lost; N < 2^22 keeps
 * N * 2^40 < 2^63.
 * acc: int64, caller-allocated, [B,size,size,C+1] for dgv2_bev_render and [B,H,W,C] for dgv2_bilinear_splat; its
 * contents on entry do not matter (the entry clears it) and are the scaled sums afterwards.  Its size is this formula,
 * not a library plan: there is no _scratch sibling.
 * A coordinate becomes an index only behind a range comparison on the float, so a NaN or huge coordinate drops its point
 * and never forms an address; non-finite inputs are otherwise unspecified.
 * DGV2_EINVAL, nothing launched: a null out / acc / points / colors, B, N or a size < 1, C outside [1, 4], N >= 2^22,
 * more than 2^31 - 1 blocks.
 * ------------------------------------------------------------------------- */
int dgv2_bev_render(float* out, int64_t* acc, const float* points, const float* colors, const float* R, const float* t,
                    int B, int N, int C, int size, float focal, void* stream);
int dgv2_bilinear_splat(float* out, int64_t* acc, const float* coords, const float* values, int B, int N, int C, int H,
                        int W, void* stream);

/* ---------------------------------------------------------------------------
 * Latent fitting: what a stage-1 inversion step does after backward(), in one launch (latent.hip; gans/sim2real.py here)
 * replaces: inversion.py:10-20,81-90 and demo_inversion.py:147-152 -- geocross_loss and autograd through it, the
 *   LambdaLR schedule (a Python float per step, which keeps the step out of a hipGraph), torch.optim.Adam /
 *   SphericalOptimizer on the latent and the phase, and the host-side append of the loss: about 50 launches on a few KB.
 * z, g_z, m_z, v_z [B,N,D] (N = 1 for the latent types "w" and "z"); phase, g_phase, m_p, v_p [B,2], all four NULL = the
 * phase is not optimised; step int32 [B]; loss_terms [B] (the data terms autograd produced); loss_log [num_steps,B];
 * geo [B] (output).  All float32 (step: int32) and contiguous.  One block per sample, no atomics, no workspace, no
 * dependence between samples: a sample's bits depend neither on B nor on its place in the batch, and are the same from
 * run to run (block sums: strided partial, xor shuffle, wave partials in order).
 * Per sample b, with k = step[b]; k outside [0, num_steps) leaves everything of that sample untouched (an over-replayed
 * graph is harmless):
 *   1. geo[b] = mean over all N^2 ordered pairs (i, j), the diagonal included, of atan2(A, B)^3  (= (2 atan2)^3 / 8),
 *      A = sqrt(|x_i - x_j|^2 + 1e-9), B = sqrt(|x_i + x_j|^2 + 1e-9), both sums taken over the differences / sums
 *      themselves (equal styles give exactly 0 + 1e-9; a Gram form would not).  g_z += geo_coef * d geo / d z (analytic).
 *      geo_coef = 0 skips the term (geo[b] = 0, g_z not written); the reference's "w+" value is 5e-3.
 *   2. loss_log[k,b] = loss_terms[b] + geo_coef * geo[b]
 *   3. lr = lr0 * gamma(k): t = k / num_steps, gamma = min(1, (1 - t) / rampdown_ratio),
 *      gamma = (0.5 - 0.5 cos(pi gamma)) * min(1, t / rampup_ratio), in double.  gamma(0) = 0: the first step moves the
 *      moments and leaves the parameters bit-unchanged.
 *   4. torch.optim.Adam's update of z and phase (no weight decay, no amsgrad), bias corrections with k + 1; the scalar
 *      factors (1 - beta, lr / (1 - beta1^(k+1)), sqrt(1 - beta2^(k+1))) in double from the float arguments, rounded once;
 *      element-wise in float32:  m += (1 - beta1) (g - m);  v = v beta2 + (1 - beta2) g g;
 *      p -= step_size * (m / (sqrt(v) / bias2_sqrt + eps))
 *   5. hypersphere != 0: every row z[b,n,:] is divided by sqrt(mean(row^2) + 1e-9) after the update (phase is not).
 *   6. step[b] = k + 1
 * DGV2_EINVAL, nothing launched: a null z / g_z / m_z / v_z / step / loss_terms / loss_log / geo; B, N, D or num_steps
 * < 1; N * D > 16384 (the sample's z is held in LDS); geo_coef != 0 with N < 2; the four phase pointers neither all
 * NULL nor all set.  The launch function allocates and synchronises nothing: it may be captured into a hipGraph.
 * ------------------------------------------------------------------------- */
int dgv2_latent_step(float* z, float* g_z, float* m_z, float* v_z, float* phase, const float* g_phase, float* m_p,
                     float* v_p, int* step, const float* loss_terms, float* loss_log, float* geo, int B, int N, int D,
                     int num_steps, float lr0, float rampup_ratio, float rampdown_ratio, float beta1, float beta2,
                     float eps, float geo_coef, int hypersphere, void* stream);

/* ---------------------------------------------------------------------------
 * Synchronised batch norm of the segmentation models, training mode (syncbn.hip; semseg/models/syncbn.py here)
 * replaces: torch.nn.SyncBatchNorm as train_semseg.py:172-174 puts it over every BatchNorm2d of semseg/models/common.py
 *   (batch_norm_stats, an all_gather of means / inverse deviations / counts, batch_norm_gather_stats_with_counts,
 *   batch_norm_elemt; batch_norm_backward_reduce, an all_reduce, batch_norm_backward_elemt), whose fp32 merge of the
 *   ranks' statistics depends on how the batch is split over the ranks.
 * x, y, dy, dx [B,C,H,W] are contiguous NCHW of one `dtype` (DGV2_F32, DGV2_BF16 or DGV2_F16).  weight, bias, the
 * running buffers and the saved statistics are float32 [C]; num_batches_tracked is ONE int64.  part is float64
 * [B,C,2] where an entry writes it and [Btot,C,2] where an entry reads it: the blocks of all ranks, rank-major, then
 * the sample index (the caller gathers them; one rank: the array as written).  All sums and all arithmetic below are
 * float64; a result is rounded once to float32 and, for a 16-bit dtype, once more to that dtype.
 *   dgv2_bn_partials      part[b][c] = (sum x, sum x^2) over the plane x[b][c]
 *   dgv2_bn_apply         (S, Q) = part[0][c] + part[1][c] + ... + part[Btot-1][c], in index order;  n = Btot H W
 *                         mean = S / n;  var = max(Q / n - mean^2, 0);  invstd = 1 / sqrt(var + eps)
 *                         y = (x - mean) (invstd weight[c]) + bias[c]            (weight / bias NULL: 1 / 0)
 *                         save_mean[c] = mean, save_invstd[c] = invstd
 *                         running_mean[c] = (1 - f) running_mean[c] + f mean
 *                         running_var[c]  = (1 - f) running_var[c]  + f var n / (n - 1)
 *                         f = momentum, and num_batches_tracked += 1 (NULL: not counted);  momentum < 0 is torch's
 *                         momentum=None, the cumulative average: f = 1 / num_batches_tracked, which the CALLER has
 *                         already incremented for this batch (every channel's block reads the word, so none writes it).
 *                         running_mean and running_var both NULL: no running statistics.
 *   dgv2_bn_bwd_partials  part[b][c] = (sum dy, sum dy xhat),  xhat = (x - mean[c]) invstd[c] from the SAVED float32 values
 *   dgv2_bn_bwd_apply     (S, Q) as above over the gathered backward partials;  m1 = S / n, m2 = Q / n
 *                         dx = (invstd[c] weight[c]) ((dy - m1) - xhat m2)
 *                         dbias[c] = part[b_off][c][0] + ... + part[b_off+B-1][c][0], dweight[c] the same over [1]: the
 *                         LOCAL samples only, torch.nn.SyncBatchNorm's semantics (the gradient reduction averages them
 *                         over the ranks afterwards); either may be NULL.
 * One block per plane.  A plane's sums are added in an order that its size H W and the dtype fix -- not B, not the
 * grid, not the plane's address (16-byte loads where a plane is 16-byte aligned, the same groups element by element
 * where it is not; syncbn.hip spells the order out) -- and the fold runs in index order on every rank, so the
 * statistics, y and dx are the same bits however Btot samples are split over ranks, and from run to run.  No atomics,
 * no workspace (the partials are outputs: there is no _scratch sibling).  In dgv2_bn_apply the block of sample 0 of a
 * channel writes that channel's statistics and running buffers, and block 0 counts the batch.
 * DGV2_EINVAL, nothing launched: a null required pointer (everything but weight, bias, the running buffers,
 * num_batches_tracked, dweight, dbias), one running buffer without the other, momentum < 0 with running buffers and
 * no num_batches_tracked, B, C, H or W < 1, B C, Btot C or H W above 2^31 - 1, Btot < B, b_off outside
 * [0, Btot - B], another dtype, a negative or NaN eps, a NaN momentum, and Btot H W == 1 (torch: "Expected more than 1
 * value per channel when training").
 * ------------------------------------------------------------------------- */
int dgv2_bn_partials(double* part, const void* x, int B, int C, int H, int W, int dtype, void* stream);
int dgv2_bn_apply(void* y, float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, const void* x, const double* part, const float* weight,
                  const float* bias, int B, int Btot, int C, int H, int W, float eps, float momentum, int dtype,
                  void* stream);
int dgv2_bn_bwd_partials(double* part, const void* dy, const void* x, const float* mean, const float* invstd, int B,
                         int C, int H, int W, int dtype, void* stream);
int dgv2_bn_bwd_apply(void* dx, float* dweight, float* dbias, const void* dy, const void* x, const double* part,
                      const float* mean, const float* invstd, const float* weight, int B, int Btot, int b_off, int C,
                      int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * PointNet trunk of the FPD / KPD feature extractor (pointnet.hip; gans/metrics/pointnet.py here)
 * replaces: gans/metrics/pointnet.py:22-26 (the spatial transformer's conv1-3 / bn1-3, ReLUs and torch.max over the
 *   points) and :46-55 (the bmm with the transform, the feature trunk's conv1-3 / bn1-3 and its max): per trunk three
 *   GEMMs, their activations and a reduction over a [B,N,1024] tensor -- with a launch that keeps no per-point value
 *   in memory.
 * pts [B,N,3] (points as rows), trans [B,3,3] or NULL, feat [B,1024]; w1 [64,3], b1 [64], w2 [128,64], b2 [128],
 * w3 [1024,128], b3 [1024] are the three affine maps with the evaluation-mode batch norms already folded in.  All
 * float32 and contiguous; w2 and w3 16-byte aligned (they are read with 16-byte loads).  The widths 3 / 64 / 128 / 1024
 * are the contract.  Per cloud b and point p, in float32:
 *   q[j]   = fmaf(z, T[2][j], fmaf(y, T[1][j], x * T[0][j])),  (x, y, z) = pts[b][p], T = trans[b]      (the bmm);
 *            trans == NULL: q = (x, y, z)
 *   h1[c]  = relu(fmaf(w1[c][2], q[2], fmaf(w1[c][1], q[1], w1[c][0] * q[0])) + b1[c])
 *   h2[c]  = relu(S_64(w2[c], h1) + b2[c])
 *   h3[c]  = S_128(w3[c], h2) + b3[c],  through a ReLU when relu_last == 1 (the transformer's trunk: 1, the feature
 *            trunk: 0)
 *   feat[b][c] = max over p of h3[c]
 * S_K(w, h) is ONE fmaf chain from 0 over all K products (the exact v_mfma_f32_32x32x2_f32; no bf16 split), in the
 * fixed order k = 0, 4, 1, 5, 2, 6, 3, 7, then the same pattern from 8, 16, ...  The order does not depend on where a
 * point sits, and a maximum does not depend on the order of its operands, so a cloud's features are the same bits
 * alone or in a batch, under any permutation or repetition of its points, under any split of N over blocks and from
 * run to run.  A block owns DGV2_POINTNET_TILE points of one cloud and keeps them in registers and LDS through all
 * three layers; in a ragged tile the lanes beyond N repeat the cloud's last point, so nothing that is not an image of
 * a point of the cloud enters the maximum.  N > DGV2_POINTNET_TILE: the blocks of a cloud combine their maxima in
 * feat with integer atomic max / min on the floats' bits after a launch that fills feat with -inf (two launches;
 * otherwise one).  No workspace: there is no _scratch sibling.  Nothing allocates or synchronises; the launches may
 * be captured into a hipGraph.
 * Non-finite coordinates or parameters are outside the contract (a NaN is dropped by the maximum where torch
 * propagates it); nothing is read back to check.
 * Range: B, N >= 1, 64-bit offsets; B * ceil(N / DGV2_POINTNET_TILE) <= DGV2_POINTNET_MAX_TILES, above which the entry
 * returns DGV2_ENOTSUP (fallback: the library-GEMM composition of gans/metrics/pointnet.py).  DGV2_EINVAL: a null
 * pointer other than trans, B or N < 1, relu_last not 0 / 1, a misaligned w2 / w3.  On every refusal nothing is
 * launched and feat is untouched.
 * ------------------------------------------------------------------------- */
#define DGV2_POINTNET_TILE 128
#define DGV2_POINTNET_FEATURES 1024
#define DGV2_POINTNET_MAX_TILES (1 << 28)
int dgv2_pointnet_trunk(float* feat, const float* pts, const float* trans, const float* w1, const float* b1,
                        const float* w2, const float* b2, const float* w3, const float* b3, int B, int N,
                        int relu_last, void* stream);

/* ---------------------------------------------------------------------------
 * Beam upsampling: holding out beams of a scan, the interpolation baselines and the depth scores of the held-out
 * pixels (upsample.hip; gans/upsampling.py here)
 * replaces: gans/metrics/depth.py:4-45 -- compute_depth_error and compute_depth_accuracy (about 25 tensor-op launches
 *   and a dozen [B,1,H,W] temporaries per call, summed in float32 in the order the library picks) -- with one launch
 *   of fixed-order float64 sums; the reference has no code that holds beams out or interpolates them (the paper's
 *   upsampling table is described, not shipped), so dgv2_beam_split replaces nothing there.
 *
 * dgv2_beam_split, one launch: depth, valid [B,1,H,W] float32, contiguous; valid == NULL is 1 everywhere, any other
 * non-zero value of valid counts as valid.  Row h is observed when h % factor == offset.
 *   obs  = 1 where the pixel is observed and valid, else 0                              (the fitting mask)
 *   held = 1 where the pixel is valid and its row is not observed, else 0               (the scoring mask)
 *   recon, recon_mask: the baseline reconstruction from the observed rows only.  mode 0: nothing is reconstructed and
 *   both pointers may be NULL; mode 1: nearest; mode 2: linear.  For row h, lo is the nearest observed row with index
 *   <= h and hi the nearest with index >= h (before the first / after the last observed row only one exists; on an
 *   observed row lo = hi = h).  A neighbour is valid where it exists and valid says so at (row, w); d_lo, d_hi are the
 *   depths there.
 *     linear   both valid: t = (float)(h - lo) / (float)factor;  recon = d_lo + t * (d_hi - d_lo)  -- a float32
 *              division, subtraction, multiplication and addition, each rounded; lo = hi: recon = d_lo
 *              one valid: that one's depth;  none: recon = 0, recon_mask = 0
 *     nearest  the neighbour with the smaller row distance, a tie to lo; if it is not valid the other one if that is;
 *              else recon = 0, recon_mask = 0
 *   recon_mask = 1 wherever a value was taken.  Observed rows are therefore copied, and an observed invalid pixel is
 *   reconstructed from nothing and stays invalid; the pixel's own validity on a row that is not observed plays no part
 *   in recon.  Depths are read only where valid says so or as operands that are then discarded: non-finite depths at
 *   valid pixels are outside the contract.
 * Range: 1 <= factor <= H, 0 <= offset < factor, B, H, W >= 1 (H need not be a multiple of factor).  DGV2_EINVAL,
 * nothing launched: outside that range, a mode other than 0 .. 2, a null obs / held / depth, a null recon / recon_mask
 * in mode 1 or 2, more than 2^31 - 1 blocks.
 *
 * dgv2_depth_score, one launch, no workspace: ref, gen, mask [B,n] float32, contiguous; mask == NULL is 1 everywhere;
 * mask is a weight, as in the reference.  Per pixel, in float32, every operation rounded on its own:
 *   r = ref + 1e-8f;  g = gen + 1e-8f;  d = r - g
 *   e0 = |d| / r;  e1 = (d * d) / r;  e2 = d * d;  e3 = (logf(r) - logf(g))^2
 *   delta = max(ref / gen, gen / ref) on the raw values;  a_i = (delta < 1.25^i), i = 1, 2, 3 (1.25, 1.5625, 1.953125:
 *   exact in float32; a NaN delta compares false)
 *   sums[b] = { S m e0, S m e1, S m e2, S m e3, S m a1, S m a2, S m a3, S m }: each product m * term is float32, the
 *   sums S over the n pixels of image b are float64.
 * A pixel with m == 0 is skipped: the reference multiplies and gives NaN there when the term is not finite.
 * One block per image.  The order of an image's sums is fixed by n alone (upsample.hip spells it out): no floating-point
 * atomics, 16-byte loads where the image's three addresses are 16-byte aligned and the same groups element by element
 * where they are not, so an image's eight sums are the same bits from run to run, alone or in a batch, at any place in
 * the batch and at any address.  The ratios and square roots of the seven summaries are the caller's.
 * DGV2_EINVAL, nothing launched: a null sums / ref / gen, B < 1, n < 1 or n >= 2^31.
 * Neither entry has a workspace (no _scratch sibling), allocates or synchronises: both may be captured into a hipGraph.
 * ------------------------------------------------------------------------- */
int dgv2_beam_split(float* recon, float* recon_mask, float* obs, float* held, const float* depth, const float* valid,
                    int B, int H, int W, int factor, int offset, int mode, void* stream);
int dgv2_depth_score(double* sums, const float* ref, const float* gen, const float* mask, int B, int64_t n,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGV2_H */
