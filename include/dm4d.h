/*
 * dm4d.h -- C ABI of libdm4d.so: the MI355X (gfx950) operator library underneath the
 * Diffuman4D sliding iterative denoiser.
 *
 * The reference (zju3dv/Diffuman4D) has no native layer and no FFI: every device op on its hot
 * path is an implicit torch / diffusers call.  Each entry point below
 * therefore cites the *call site* in the reference whose arithmetic it replaces.  A reference
 * maintainer binds these with ctypes; diffuman4d_amd/host/lib.py is that
 * binding.
 *
 * Conventions
 *   - all tensors are device pointers owned by the caller; bf16 unless noted; activations are
 *     token-major / NHWC: [B, H*W, C] with C contiguous
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); every call is asynchronous
 *   - return value: 0 = ok, <0 = error; dm4d_last_error() returns a thread-local message
 *   - no entry point allocates, synchronises or touches host memory
 */
#ifndef DM4D_H
#define DM4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM4D_OK 0
#define DM4D_ERR_ARG -1
#define DM4D_ERR_LAUNCH -2

/* gemm / conv epilogue flags */
#define DM4D_EPI_GEGLU 1u /* W holds [2*N, K]: out = (x W_h^T + b_h) * gelu(x W_g^T + b_g)   */
#define DM4D_EPI_SILU 2u  /* out = silu(acc + bias ...) (time embedding MLP)                 */
#define DM4D_EPI_F32OUT 4u /* C is float* [M, ldc] (ldc in floats): the result is stored unrounded */
/* parity-precision launches (two-term bf16 operands, fp32 tensors between kernels; see "Parity precision" below) */
#define DM4D_EPI_F32SIDE 8u   /* rowbias and residual are float* (their strides in floats) */
#define DM4D_EPI_SPLITOUT 16u /* C is bf16 [M, ldc >= 2 N]: hi = bf16(result) at column n, lo = bf16(result - hi) at column N + n */
/* fp16-precision launches (see "fp16 precision" below): set by the *_f16 entries themselves, never passed by a caller */
#define DM4D_EPI_H16 32u      /* A, W, bias and every 16-bit side input / output are IEEE fp16; the matrix unit runs v_mfma_f32_32x32x16_f16 */

int dm4d_version(void);
const char* dm4d_last_error(void);

/* Linear layers: out[M,N] = epi( [A | A2][M,K] @ W[N,K]^T )
 *   replaces nn.Linear calls of diffusers Attention.to_q/k/v/to_out, Transformer2DModel.proj_in/out,
 *   FeedForward/GEGLU, TimestepEmbedding, ResnetBlock2D.time_emb_proj and the 1x1 conv_shortcut
 *   (reference call sites: attention.py:73-78,90,142; transformer_multiview.py:160,209;
 *   unet_multiview_condition.py:520; unet_multiview_blocks.py:342,518,697).
 *   A2 != NULL: columns [K1, K) come from A2 (channel concat of the up-block skip, :667) .
 *   epilogue: acc (+bias[n]) (GEGLU|SILU) (+rowbias[m / rows_per_rowbias, n]) (+residual[m,n]) * out_scale
 *   K, K1 multiples of 32; lda/ldw multiples of 8.                                              */
int dm4d_gemm_bf16(void* stream, const void* A, int64_t lda, const void* A2, int64_t lda2, int K1, const void* W,
                   int64_t ldw, void* C, int64_t ldc, int M, int N, int K, const void* bias, const void* rowbias,
                   int64_t ld_rowbias, int rows_per_rowbias, const void* residual, int64_t ld_res, unsigned flags,
                   float out_scale);

/* 3x3 convolution, NHWC, implicit GEMM on MFMA.
 *   replaces nn.Conv2d(k=3) in ResnetBlock2D.conv1/conv2, Downsample2D.conv (stride 2),
 *   Upsample2D (nearest x2 fused into the gather: upsample=1), conv_in, conv_out
 *   (unet_multiview_condition.py:549,593; unet_multiview_blocks.py:342,381,460,518,620,697).
 *   X [B,H,W,Cin] (Cin % 32 == 0), Wt [Cout][3][3][Cin], Y [B,Ho,Wo,Cout];
 *   Ho = upsample ? 2H : (H + 2*pad_hi... see dm4d_conv_out_size). pad = leading pad (1 for the UNet,
 *   0 for the VAE encoder's asymmetric (0,1,0,1) pad); trailing pad is implied by Ho/Wo.
 *   epilogue as in dm4d_gemm_bf16 (rowbias row = batch index: the temb projection, resnet.py)   */
int dm4d_conv3x3_nhwc_bf16(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt, void* Y, int Ho,
                           int Wo, int Cout, int stride, int pad, int upsample, const void* bias, const void* rowbias,
                           int64_t ld_rowbias, const void* residual, int64_t ld_res, float out_scale);

/* Same convolution with a caller-owned fp32 workspace.  Stride-1 convolutions on small images with a deep K (H*W <= 64,
 *   Cin >= 512: the 9x5 level of the UNet, unet_multiview_blocks.py:71,274,585 at the deepest resolution) are split
 *   over the three kernel rows -- three workgroups per output tile, partial sums in ws, a second launch adds them in a
 *   fixed order and applies the epilogue -- because B*45 output rows cannot fill 256 CUs against an 11520-deep K.
 *   dm4d_conv3x3_ws_bytes() returns the bytes needed for a shape (0 = never split); ws == NULL or too small runs the
 *   un-split kernel.  The split depends on the per-image geometry only, not on B.                                   */
size_t dm4d_conv3x3_ws_bytes(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int stride, int pad, int upsample);
int dm4d_conv3x3_nhwc_bf16_ws(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt, void* Y, int Ho,
                              int Wo, int Cout, int stride, int pad, int upsample, const void* bias, const void* rowbias,
                              int64_t ld_rowbias, const void* residual, int64_t ld_res, float out_scale, void* ws,
                              size_t ws_bytes);

/* The same convolution with epilogue flags (DM4D_EPI_F32OUT: Y is float* [B,Ho,Wo,Cout]; DM4D_EPI_F32SIDE: rowbias / residual are
 *   float*): the parity-precision form.  X then usually carries two-term operands, [hi(Cin/2) | lo(Cin/2)] per pixel, against weights
 *   duplicated along Cin; the kernel neither knows nor cares.  Never split over the kernel rows (no workspace).             */
int dm4d_conv3x3_nhwc_bf16_flags(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt, void* Y, int Ho,
                                 int Wo, int Cout, int stride, int pad, int upsample, const void* bias, const void* rowbias,
                                 int64_t ld_rowbias, const void* residual, int64_t ld_res, float out_scale, unsigned flags);

/* Upsample2D -- third-party: diffusers==0.33.1 (requirements.txt:5), instantiated by the reference at
 * src/diffusers/models/unets/unet_multiview_blocks.py:620 and by the VAE decoder; its published forward is
 * F.interpolate(x, scale_factor=2.0, mode="nearest") then conv3x3(padding=1) -- as four 2x2 convolutions of the
 * LOW-resolution input, one per output phase (restated and checked against that form in oracle/up2x.py):
 * 4/9 of the multiply-adds.  `Wp` [4][Cout][4*Cin] is made once per layer from the 3x3 weights W [Cout][9*Cin]
 * (ky, kx, ci order) by dm4d_conv_up2x_prepare_bf16 (sums of 1, 2 or 4 taps in fp32, rounded to bf16 once).
 * X [B, H, W, Cin] -> Y [B, 2H, 2W, Cout], Cin % 64 == 0, Cout % 8 == 0; bias optional.                               */
int dm4d_conv_up2x_prepare_bf16(void* stream, const void* W, void* Wp, int Cout, int Cin);
int dm4d_conv_up2x_nhwc_bf16(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wp, void* Y, int Cout,
                             const void* bias);

/* Direct (fp32 FMA) convolution for thin layers, NHWC: the PoseEncoder's conv stack
 *   (pose_encoder.py:14-31: 3x3 stride 1 / 4x4 stride 2, padding 1, 3..64 input channels, SiLU after each).
 *   X [B,H,W,Cin], Wt [Cout][ksize*ksize][Cin], Y [B,Ho,Wo,Cout]; Cin, Cout multiples of 4 (zero-pad the 3-channel
 *   image and the first layer's filters); ksize <= 4; Ho = (H + 2*pad - ksize)/stride + 1.                        */
int dm4d_conv2d_direct_nhwc_bf16(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt,
                                 const void* bias, void* Y, int Ho, int Wo, int Cout, int ksize, int stride, int pad,
                                 int apply_silu);
/* The same chain on fp32 tensors (image, filters, bias, result all fp32; nothing rounded to bf16): the PoseEncoder of the parity
 * precision (see "Parity precision" below).                                                                              */
int dm4d_conv2d_direct_nhwc_f32(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt,
                                const void* bias, void* Y, int Ho, int Wo, int Cout, int ksize, int stride, int pad,
                                int apply_silu);

/* GroupNorm (+SiLU) over [X1 | X2] (channel concat, X2 may be NULL), NHWC.
 *   replaces nn.GroupNorm + SiLU in ResnetBlock2D.norm1/norm2, TransformerMultiviewModel.norm
 *   (transformer_multiview.py:43-45), conv_norm_out (unet_multiview_condition.py:590-592).
 *   ws: fp32 scratch of dm4d_groupnorm_ws_bytes(B, HW) bytes.  Statistics in fp32.              */
size_t dm4d_groupnorm_ws_bytes(int B, int HW, int groups);
int dm4d_groupnorm_nhwc_bf16(void* stream, const void* X1, int C1, const void* X2, int C2, int B, int HW, int groups,
                             float eps, const void* gamma, const void* beta, void* Y, int apply_silu, void* ws);

/* LayerNorm over the last dim.  replaces BasicTransformerBlock.norm1/norm3 (attention.py:49,129) */
int dm4d_layernorm_bf16(void* stream, const void* X, int64_t ldx, const void* gamma, const void* beta, void* Y,
                        int64_t ldy, int M, int C, float eps);

/* Self-attention, head_dim 64, no mask: O = softmax(Q K^T * scale) V per (batch, head).
 *   replaces AttnProcessor2_0 / F.scaled_dot_product_attention reached from attention.py:73-78;
 *   the "(b t) hw c -> b (t hw) c" frame folding (attention.py:69-71,81-83) is expressed by
 *   batch = B / num_frames, L = num_frames * HW on the SAME memory (token-major rows).
 *   Q/K/V/O rows are tokens; element (b, t, h, d) lives at ptr[(b*L + t)*ld + h*64 + d].
 *   Pointers 16-byte aligned, row strides multiples of 8 elements.                                    */
int dm4d_attention_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                        int64_t ldv, int64_t ldo, int batch, int heads, int L, float scale);

/* Same kernel with separate query / key lengths: queries are the Lq local tokens of this rank, keys/values the Lk
 *   tokens gathered from every rank (in-window frame sharding).  Element (b, t) of K/V lives at
 *   ptr[(b*Lk + t)*ld + h*64 + d]; of Q/O at ptr[(b*Lq + t)*ld + h*64 + d].                                        */
int dm4d_attention_kv_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                           int64_t ldv, int64_t ldo, int batch, int heads, int Lq, int Lk, float scale);

/* Same attention for a Q that already carries the softmax scale: Q' = Q * scale * log2(e)  (DM4D_LOG2E), i.e.
 *   O = softmax2(Q' K^T) V with softmax2 in base 2.  The model folds the factor into the to_q rows of the fused
 *   QKV weight when the checkpoint is loaded (attention.py:73-78 computes to_q(x) then SDPA's q*scale), so the
 *   scale costs no instruction at all: the kernel starts its QK^T accumulator from -rowmax and P = exp2(S).
 *   Layout, strides and Lq/Lk as in dm4d_attention_kv_bf16.                                                    */
#define DM4D_LOG2E 1.4426950408889634
int dm4d_attention_qscaled_kv_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq,
                                   int64_t ldk, int64_t ldv, int64_t ldo, int batch, int heads, int Lq, int Lk);

/* Generic-head-dim attention pieces for the VAE mid block (AutoencoderKL mid_block.attentions.0: single head, d = 512,
 *   reached from pipeline_diffuman4d.py:52,65): P = softmax(S * scale) per row, P in bf16.  The f32in form takes the
 *   logits as dm4d_gemm_bf16(..., DM4D_EPI_F32OUT) leaves them (SDPA keeps its logits in fp32); lds, ldp multiples
 *   of 4 and >= N there, any N: columns behind N of a padded row are neither read nor written.                      */
int dm4d_softmax_rows_bf16(void* stream, const void* S, int64_t lds, void* P, int64_t ldp, int M, int N, float scale);
int dm4d_softmax_rows_f32in_bf16(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N, float scale);

/* sinusoidal timestep embedding, diffusers get_timestep_embedding (unet_multiview_condition.py:494):
 *   out[b, :] = [cos(t*f) | sin(t*f)] (flip_sin_to_cos) in bf16, t given as fp32                  */
int dm4d_timestep_embedding_bf16(void* stream, const float* t, void* out, int B, int dim, int flip_sin_to_cos,
                                 float freq_shift);

int dm4d_silu_bf16(void* stream, const void* X, void* Y, int64_t n);

/* Model-input assembly for one window (pipeline_diffuman4d.py:375-395, 348-357):
 *   out [cfg*F, HW, cpad] NHWC: channels [latent 4 | plucker 6 | skeleton-latent 4 (opt) | mask 1 | 0...]
 *   cond rows (is_cond[f] != 0) take the clean image latents (and +1.0 in the negative half);
 *   negative half: plucker 0, skeleton -1.  Also performs the reference's aliasing side effect
 *   (SURVEY 8a P-4 iv): latents[cond rows] <- image latents, in place.
 *   frame_idx (int32 [F], may be NULL): window frame f reads row frame_idx[f] of the task-level
 *   tensors latents/pv_lat/plucker/skel/mask -- the x[window] gathers of :522-531 without copies.     */
int dm4d_pack_model_input_bf16(void* stream, void* latents, const void* pv_lat, const void* plucker, const void* skel,
                               const void* mask, const int32_t* is_cond, const int32_t* frame_idx, void* out, int F,
                               int HW, int cpad, int use_cfg);

/* CFG combine + per-latent DDIM step (pipeline_diffuman4d.py:408-422), one launch for the window:
 *   eps = u + s (c - u);  x <- sqrt(a_prev) x0 + sqrt(1 - a_prev) eps_hat   for non-cond rows.
 *   noise_pred [cfg*F, HW, ldn]; coef [F,4] fp32 = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)}
 *   frame_idx as above: the update is scattered straight into the task-level latents (:543).         */
int dm4d_cfg_ddim_step_bf16(void* stream, void* latents, const void* noise_pred, int64_t ldn, const float* coef,
                            const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg,
                            float guidance_scale, int v_prediction);

/* CFG combine + per-latent LINEAR MULTISTEP step: the update of any scheduler whose step is linear in the sample, the model
 * output and one stored prediction -- DPM-Solver++ of order 1 / 2, where the reference keeps one stateful scheduler object per
 * latent (pipeline_diffuman4d.py:265-271, 420, 500-501):   m = u + s (c - u);  x <- a x + b m + c p;  p <- d x + e m
 * for non-cond rows.  coef [F,8] fp32 = {a, b, c, d, e, -, -, -} per frame (host/scheduler.py::step_rows); x0_prev = the task's
 * stored x0 predictions, same shape and indexing as latents (rows whose c is 0 are not read).                                */
int dm4d_cfg_linear_step_bf16(void* stream, void* latents, void* x0_prev, const void* noise_pred, int64_t ldn,
                              const float* coef, const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg,
                              float guidance_scale);

/* CFG combine + per-latent GENERAL linear multistep step with up to three stored tensors per latent: UniPC (with its corrector) and DEIS,
 * where the reference keeps one stateful scheduler object per latent (pipeline_diffuman4d.py:265-271, 420, 500-501).  coef [F,16] fp32 rows
 * (k0..k10, host/scheduler.py::step_rows):   m = u + s (c - u);   conv = k0 x + k1 m;   xc = k2 x + k3 s3 + k4 s1 + k5 s2 + k6 conv;
 * x <- k7 xc + k8 conv + k9 s1 + k10 s2 + k11 s3;   s3 <- xc, s2 <- s1, s1 <- conv   for non-cond rows.  s1 / s2 / s3: same shape and
 * indexing as latents, ZERO at the start of a sliding_iterative_denoise call (s2, s3 may be NULL).  k12 selects what the stored tensors
 * become: 0 as written, 1 kept unchanged, 2 shifted as a history (s3 <- s2, s2 <- s1, s1 <- conv): PNDM's linear multistep form (PLMS),
 * whose repeated second step re-does the first from the stored sample (host/scheduler.py::PNDMScheduler).                                 */
int dm4d_cfg_multistep_step_bf16(void* stream, void* latents, void* s1, void* s2, void* s3, const void* noise_pred, int64_t ldn,
                                 const float* coef, const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg,
                                 float guidance_scale);

/* VAE posterior sample, DiagonalGaussianDistribution.sample() * scaling_factor
 *   (pipeline_diffuman4d.py:52,55): out[m,c] = (mean + exp(0.5*clamp(logvar,-30,20)) * noise[m,c]) * scale
 *   moments rows hold [mean(C) | logvar(C) | ...] with row stride ldm; noise/out are [M, C].          */
int dm4d_vae_sample_bf16(void* stream, const void* moments, int64_t ldm, const void* noise, void* out, int64_t M, int C,
                         float scale);

/* Y[m, 0:cpad] = [X[m, 0:C] * scale | 0]   (latents / scaling_factor before post_quant_conv, :66)     */
int dm4d_scale_pad_bf16(void* stream, const void* X, int64_t ldx, void* Y, int cpad, int64_t M, int C, float scale);

/* F.interpolate(size=(h,w), mode = bilinear (1) | nearest (0)), fp32 NCHW -> bf16 NHWC
 *   (encode_image_resizing, pipeline_diffuman4d.py:90-100: Pluecker maps and condition masks)        */
int dm4d_resize_nchw_f32_to_nhwc_bf16(void* stream, const float* X, void* Y, int B, int C, int H, int W, int h, int w,
                                      int bilinear);

/* Pluecker ray maps at latent resolution, from the cameras: calc_plucker_embeds(H, W, K, pose) (data/utils/ray_utils.py:101-112,
 *   called at spatem_dataset.py:169-176) followed by F.interpolate(size=(h, w), mode="bilinear") and the cast to bf16
 *   (encode_image_resizing, pipeline_diffuman4d.py:90-100, 218-222) in one launch: no [N, 6, H, W] fp32 map on the host, no
 *   H2D copy of it.  cams [N, 24] fp32 = per frame {K^-1 (9, row major) | R (9) | T (3) | o = -R^T T (3)} with [R | T] =
 *   inverse(camera-to-world pose)[:3]; Y [N, h*w, 6] bf16 = [ray direction | o x direction].                        */
int dm4d_plucker_latent_bf16(void* stream, const float* cams, void* Y, int N, int H, int W, int h, int w);

/* F.interpolate(size=(h, w), mode="bilinear", antialias=True) on `planes` fp32 H x W planes (NCHW with planes = N * C): the down-scale of
 *   the result writer's snapshot mosaic (samplers/utils/sampling_utils.py:70-93 -> torchvision's antialiased resize); PIL's separable
 *   triangle filter of support max(H / h, 1), normalised per axis.                                                            */
int dm4d_resize_aa_nchw_f32(void* stream, const float* X, float* Y, int64_t planes, int H, int W, int h, int w);

/* Crop + bicubic resize of captured frames (diffuman4d_amd/host/capture.py::SpaTemDataset; spatem_dataset.py:58-69 + 157-166):
 *   Pillow's Image.crop((left, top, left + cw, top + ch)).resize((W, H), BICUBIC) byte for byte on each frame's image (RGB), mask (L)
 *   and skeleton (RGB), then TF.to_tensor -> x * 2 - 1 and, for the image, apply_fmask(white, vae_normalized=True), each fp32
 *   operation rounded on its own.  Two launches for all frames: the horizontal pass into `scratch` (8 bytes per pixel, uint8 as in
 *   Pillow), the vertical pass + epilogue into pixel_values / skeletons [n_frames, 3, H, W] fp32.
 *   staging: device copy of the frames' packed uint8 planes (HWC, rows tight).  desc: n_frames x DM4D_CAPTURE_FIELDS int64 =
 *   {image, mask, skeleton byte offsets in staging | source h, w | crop top, left, height, width (may extend past the image) |
 *   horizontal table offset, ksize | vertical table offset, ksize | scratch byte offset (16-aligned) | first crop row the vertical
 *   windows read, number of such rows}.  tab: int32 tables; one table for n outputs = n x {window start, window length} followed by
 *   n x ksize coefficients with 22 fractional bits.  desc_host / tab_host are host copies of the same bytes as desc_dev / tab_dev:
 *   every offset, window and region is validated on them before anything is launched.  W % 4 == 0.                           */
#define DM4D_CAPTURE_FIELDS 16
int dm4d_capture_crop_resize_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                 const int64_t* desc_dev, int n_frames, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len,
                                 void* scratch, int64_t scratch_bytes, float* pixel_values, float* skeletons, int H, int W);

/* The same resize with the result kept as uint8 "cells" on the device, and cells turned into samples (capture.hip; the device cell cache
 *   of SpaTemDataset(device_cache=True), diffuman4d_amd/host/capture_cache.py).
 * A cell is one resized frame: H * W packed pixels, row-major, 8 bytes each = {i0 i1 i2 m s0 s1 s2 0} (image RGB, mask, skeleton RGB,
 *   a zero pad): the bytes of one scratch row of the horizontal pass, and the clip8 values the vertical pass holds before its epilogue.
 *   H * W * 8 bytes on a 16-byte address.  cell: n x DM4D_CAPTURE_CELL_FIELDS int64 = {slab address (a device allocation, 16-byte
 *   aligned) | slab bytes | byte offset of the cell in the slab (16-byte aligned) | output row}; cells of one call may lie in any
 *   number of slabs.  cell_host is the host copy of the bytes at cell_dev and is validated before anything is launched: a slab
 *   address that is zero or unaligned, an offset that is negative or unaligned, a cell that leaves its slab.
 * dm4d_capture_crop_resize_packed_u8: the arguments, checks and horizontal pass of dm4d_capture_crop_resize_f32; the vertical pass
 *   stores frame f's packed pixels into cell f (32 bytes per lane for 4 columns) instead of the fp32 planes.  The output row field is
 *   ignored; two frames that name the same (slab, offset) are refused.  Two launches.
 * dm4d_capture_unpack_cells_f32: one launch; a lane loads 32 bytes (4 columns of one row of one cell), applies the epilogue of
 *   dm4d_capture_crop_resize_f32 (the same device function) and stores 6 x 16 bytes into row `output row` of pixel_values / skeletons
 *   [n_out_rows, 3, H, W] fp32.  Output rows outside [0, n_out_rows) and two rows with one output row are refused; rows of the outputs
 *   that no descriptor names are not touched.  unpack(packed(x)) is dm4d_capture_crop_resize_f32(x) bit for bit.
 * No atomics, no block waits on another; a cell's bytes and a row's floats do not depend on what else is in the call.  W % 4 == 0. */
#define DM4D_CAPTURE_CELL_FIELDS 4
int dm4d_capture_crop_resize_packed_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                       const int64_t* desc_dev, int n_frames, const int32_t* tab_host, const int32_t* tab_dev,
                                       int64_t tab_len, void* scratch, int64_t scratch_bytes, const int64_t* cell_host,
                                       const int64_t* cell_dev, int H, int W);
int dm4d_capture_unpack_cells_f32(void* stream, const int64_t* cell_host, const int64_t* cell_dev, int n_rows, float* pixel_values,
                                  float* skeletons, int n_out_rows, int H, int W);

/* Box and byte sum of uint8 planes that lie in a device blob, and masks that are filled rectangles (capture.hip): what
 *   SpaTemDataset(device_decode=True) needs of planes that were decoded on the device and never visit the host.
 * dm4d_capture_plane_stats_u8: desc = n x DM4D_CAPTURE_PLANE_FIELDS int64 = {byte offset in blob (16-byte aligned) | h | w | channels: 1
 *   or 3 | 0 ...}; planes are HWC with tight rows, of any sizes from 1 to 32768 a side.  out [n, 5] int64 = {first column, first row,
 *   last column, last row, sum}: columns and rows of the pixels with at least one non-zero channel, {w, h, -1, -1} for a plane without
 *   one (as dm4d_skeleton_box_mask_u8), and the sum of all the plane's bytes.  Two launches on `stream`: per-block partials over
 *   16-byte loads (a scalar tail where a plane does not end on one), then one wave per plane that folds them.  Integers only, no
 *   atomics, no block waits on another: a plane's row is the same alone or in any batch, and bitwise repeatable.
 *   ws: dm4d_capture_plane_stats_ws_bytes(n, the largest plane's bytes) bytes (0 for arguments out of range), 8-byte aligned.
 * dm4d_capture_fill_rects_u8: desc = n x DM4D_CAPTURE_RECT_FIELDS int64 = {mask byte offset in blob (any alignment) | h | w | c0 | r0 |
 *   c1 | r1 | 0}; the whole [h, w] plane is written: 255 on rows r0 .. r1 - 1 and columns c0 .. c1 - 1, 0 elsewhere (c0 == c1 or
 *   r0 == r1: all 0).  One launch.  With the rectangle of capture.py's skeleton_mask_rect the plane is skeleton_to_mask's byte for byte.
 * desc_host is the host copy of the bytes at desc_dev: n, every size, offset and rectangle (0 <= c0 <= c1 <= w, 0 <= r0 <= r1 <= h, the
 *   plane inside the blob) is validated on it before anything is launched.                                                        */
#define DM4D_CAPTURE_PLANE_FIELDS 8
#define DM4D_CAPTURE_RECT_FIELDS 8
size_t dm4d_capture_plane_stats_ws_bytes(int n, int64_t max_plane_bytes);
int dm4d_capture_plane_stats_u8(void* stream, const void* blob, int64_t blob_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                                int64_t* out, void* ws, int64_t ws_bytes);
int dm4d_capture_fill_rects_u8(void* stream, void* blob, int64_t blob_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n);

/* Result evaluation of n_pairs (predicted, ground-truth) images (diffuman4d_amd/host/metrics.py::ImageEvaluator; the reference's
 *   ImageEvaluator.__call__, data/utils/metric_utils.py:98-137, called from evaluate_results :157-182 and sampling_runner.py:64-77):
 *   apply_fmask (x * m + (1 - m) * bg, fp32, each operation rounded on its own), torchvision's nearest resize to the canvas
 *   (src = min((int)floorf(dst * (float)in / out), in - 1)), mask_to_bbox(padding=8) of the union of the resized masks, the crop, then
 *   PSNR = 10 log10(1 / mean((p - t)^2)) and torchmetrics' SSIM (11 x 11 Gaussian window, sigma 1.5, c1 = 1e-4, c2 = 9e-4, mean of the map
 *   over the interior (h - 10) x (w - 10) of each channel) -- window sums and means in fp64, fixed summation order, no floating-point
 *   atomics: a pair's result is bitwise the same on every run and in every batch.
 *   blob: device bytes holding every plane.  desc: n_pairs x DM4D_EVAL_FIELDS int64 = {pred, gt byte offsets | pred mask, gt mask byte
 *   offsets (-1: absent) | source h, w | resized h, w | flags | crop left, top, right, bottom in the resized image (right / bottom
 *   exclusive; read when DM4D_EVAL_CROP_MASKS is not set) | 3 spare}.  Images: uint8 HWC (to_tensor's / 255 is applied) or, with
 *   DM4D_EVAL_IMAGE_F32, fp32 CHW; masks: one uint8 or (DM4D_EVAL_MASK_F32) fp32 plane.  Background: flags >> DM4D_EVAL_BG_SHIFT =
 *   0 black, 1 white, 2 grey.  desc_host is the host copy of desc_dev: every offset, size and box is validated on it before anything
 *   is launched.  workspace: dm4d_eval_ws_bytes(n_pairs, max resized h, max resized w) bytes.
 *   out [n_pairs, DM4D_EVAL_OUT] fp64 = {psnr, ssim, pred min, pred max, gt min, gt max (of the cropped composites: the reference's
 *   "should be normalized" check), sum of squared errors, sum of the SSIM map}; boxes [n_pairs, 4] int32 = the crop used (an empty
 *   mask gives 0, 0, 0, 0 and NaN results); debug (optional) [n_pairs, 2, 3, dbg_h, dbg_w] fp32 receives the cropped composites of
 *   pred and gt at [.., :h, :w].                                                                                              */
#define DM4D_EVAL_FIELDS 16
#define DM4D_EVAL_OUT 8
#define DM4D_EVAL_IMAGE_F32 1
#define DM4D_EVAL_MASK_F32 2
#define DM4D_EVAL_CROP_MASKS 4
#define DM4D_EVAL_BG_SHIFT 3
size_t dm4d_eval_ws_bytes(int n_pairs, int max_h, int max_w);
int dm4d_eval_psnr_ssim_f64(void* stream, const void* blob, int64_t blob_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                            int n_pairs, void* workspace, int64_t workspace_bytes, double* out, int32_t* boxes, float* debug, int dbg_h,
                            int dbg_w);

/* LPIPS-VGG of one (ground-truth, predicted) pair of cropped composites (diffuman4d_amd/host/lpips.py::LpipsVGG; the reference's
 *   ImageEvaluator.lpips = torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="vgg", normalize=True),
 *   data/utils/metric_utils.py:14-19, called at :134-137).  The thirteen VGG-16 convolutions run on dm4d_conv3x3_nhwc_bf16_flags
 *   (DM4D_EPI_F32OUT | DM4D_EPI_F32SIDE, the fp32 bias as its row bias) with three-term bf16 products: activations as pattern-1
 *   operands [hi | lo | hi] (see dm4d_split_f32) against fp32 weights packed per tap as [w_hi | w_hi | w_lo]; the entries below are
 *   the steps around them.  A pair is a batch of two images: 0 = ground truth, 1 = prediction.
 *
 * dm4d_lpips_input_split: the net's first lines (x = 2 img - 1; (x - shift) / scale, _LPIPS.forward with normalize=True and its
 *   ScalingLayer).  gt / pred: fp32 planes [3, h, w] in [0, 1], element (c, y, x) at [c * chan_stride + y * row_stride + x] (the
 *   evaluator's cropped composites are such views) -> Y bf16 [2, h, w, DM4D_LPIPS_IN_COLS] = [hi(3) | lo(3) | hi(3) | zeros]: the
 *   operand of features.0, whose packed weights carry [w_hi(3) | w_hi(3) | w_lo(3) | zeros] per tap.
 * dm4d_lpips_relu_pool_split: nn.ReLU (+ nn.MaxPool2d(2, 2), floor sizes, when pool != 0: torchvision's vgg16().features between the
 *   convolutions) of a convolution's fp32 output X [B, H, W, C] -> Y bf16 [B, Ho, Wo, 3 C] = [hi(C) | lo(C) | hi(C)]; C % 8 == 0.
 * dm4d_lpips_tap_distance_f64: one tap of _LPIPS.forward's loop: F fp32 [2, H, W, C] (BEFORE ReLU: it is applied on read) ->
 *   n = f / sqrt(1e-8 + sum_c f^2) per pixel (_normalize_tensor), d = mean_{y,x} sum_c lin[c] (n_0 - n_1)^2 (NetLinLayer, spatial_average);
 *   out[tap] = d (out: fp64 [DM4D_LPIPS_TAPS]; the value is the sum of the five, which the host takes in tap order).  fp64 sums in a
 *   fixed order, no floating-point atomics: the same bits on every run, and for the two images swapped.
 *   C: 64, 128, 256 or 512.  workspace: dm4d_lpips_ws_bytes(H, W) bytes (one fp64 partial per DM4D_LPIPS_DIST_PIXELS pixels).       */
#define DM4D_LPIPS_TAPS 5
#define DM4D_LPIPS_IN_COLS 64
#define DM4D_LPIPS_DIST_PIXELS 256
int dm4d_lpips_input_split(void* stream, const float* gt, const float* pred, int64_t chan_stride, int64_t row_stride, int h, int w,
                           void* Y);
int dm4d_lpips_relu_pool_split(void* stream, const float* X, void* Y, int B, int H, int W, int C, int pool);
size_t dm4d_lpips_ws_bytes(int H, int W);
int dm4d_lpips_tap_distance_f64(void* stream, const float* F, const float* lin, int H, int W, int C, int tap, void* workspace,
                                int64_t workspace_bytes, double* out);

/* Visual-hull carving (diffuman4d_amd/host/vhull.py::carve_visual_hull; the reference's scripts/preprocess/carve_visual_hull.py:76-151,
 *   the loop over batches of voxels with its ~20 torch operators).  Grid: xs [nx], ys [ny], zs [nz] fp32 on the device; voxel idx in
 *   [0, nx ny nz), z fastest: iz = idx % nz, iy = (idx / nz) % ny, ix = idx / (ny nz); X = (xs[ix], ys[iy], zs[iz]) widened to fp64.
 *   Per view b with P[b] (3 x 4 fp64, row-major; P: [B, 12] on the device): x_r = ((P[r][0] X0 + P[r][1] X1) + P[r][2] X2) + P[r][3], every
 *   operation rounded on its own; z = x_2, u = rint(x_0 / max(z, 1e-8)), v = rint(x_1 / max(z, 1e-8)) (ties to even);
 *   inside_b = z > 0 && 0 <= u < W && 0 <= v < H (tested in fp64, before any conversion) && mask[b][v][u].  A voxel is kept iff all B
 *   views are inside (min_views == 0) or at least min_views are (min_views > B keeps nothing).
 *
 * dm4d_vhull_pack_masks: masks uint8 [B, H, W] (nonzero = foreground; a torch.bool tensor as it lies in memory) -> bits uint32
 *   [B, H, (W + 31) / 32]: bit (x & 31) of word x >> 5 of row (b, y); the unused bits of a row's last word are 0.
 * dm4d_vhull_carve_chunk: the voxels [first, first + n_voxels) of the grid, n_voxels <= DM4D_VHULL_MAX_CHUNK, in three launches (flags +
 *   per-block counts, a one-block scan, gather).  *total (device int64) is the running number of kept points of the frame: the kept
 *   centres of this chunk go to out[*total ...] (fp32 [capacity, 3]) in ascending idx and *total grows by their number; the caller
 *   zeroes it before the first chunk and walks the chunks in ascending order on one stream.  Points at positions >= capacity are
 *   counted and not written: *total is always the true count, and out holds min(*total, capacity) points.  Positions come from
 *   ballots, popcounts and the scan, never from an atomic; no block waits for another.
 *   workspace: dm4d_vhull_ws_bytes(n_voxels) bytes (0 for an n_voxels out of range), 8-byte aligned, reusable by the next chunk.  */
#define DM4D_VHULL_BLOCK 256
#define DM4D_VHULL_MAX_CHUNK (1ll << 26)
int dm4d_vhull_pack_masks(void* stream, const void* masks, void* bits, int B, int H, int W);
/* the same bits from gray values (decoded mode-L mask files, host/pngdec.py): a pixel is foreground where its value >= threshold (1 .. 255) */
int dm4d_vhull_pack_masks_u8(void* stream, const void* masks, void* bits, int B, int H, int W, int threshold);
size_t dm4d_vhull_ws_bytes(int64_t n_voxels);
int dm4d_vhull_carve_chunk(void* stream, const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                           const double* P, const void* bits, int B, int H, int W, int min_views, int64_t first, int64_t n_voxels,
                           void* workspace, int64_t workspace_bytes, int64_t* total, float* out, int64_t capacity);

/* Skeleton triangulation (diffuman4d_amd/host/triang.py::triangulate_points / project_points; the reference's
 *   scripts/preprocess/utils/triang_utils.py, called from scripts/preprocess/triangulate_skeleton.py:149 and :158).  All tensors fp64 on
 *   the device (n_views int32), row-major; K [.., 3, 3] intrinsics, T [.., 4, 4] world -> camera, P = K @ T[:3].
 *
 * dm4d_triangulate_points_f64 (triangulate_points -> triangulate_one_point per keypoint, triang_utils.py:53-126 and :129-175) for a
 *   batch of F frames in one launch: K [n, 3, 3], T [n, 4, 4], kp2d [F, n, k, 2], score [F, n, k], thr [F, k] = the score threshold of
 *   each (frame, keypoint) (the host's max(score_thr, percentile); the device only compares) -> kp3d [F, k, 3], reproj [F, k], n_views
 *   [F, k].  View j is selected iff score >= thr; n_views counts them; with fewer than min_views, kp3d = reproj = -1e6 (INVALID).
 *   Otherwise: the linear (DLT) start on rows scaled by sqrt(score), from the eigenvector of the smallest eigenvalue of the 4 x 4 normal
 *   matrix (selected views with score <= 0, u < 0 or v < 0 give no rows to the start only), x[:3] / (x[3] + 1e-9); then the minimiser
 *   of scipy's Huber cost 0.5 sum rho(r^2), r = (P X / (depth + 1e-9) - obs) sqrt(score) per scalar component, f_scale = 1, by a
 *   damped Gauss-Newton iteration on the 3 x 3 system run to fp64 convergence (at most 64 evaluations; the last iterate is written
 *   in any case); reproj = sum(err_px score) / (sum score + 1e-9) over the selected views.  One wave per (frame, keypoint), lanes over
 *   views (any n up to DM4D_TRIANG_MAX_VIEWS), sums over views in a fixed order: bitwise repeatable, and a frame's result does not
 *   depend on the batch around it.  No atomics; no block waits on another.
 * dm4d_project_points_f64 (project_points -> project_one_point, triang_utils.py:7-23): kp3d [F, k, 3], K [m, 3, 3], T [m, 4, 4] ->
 *   kp2d [F, m, k, 2] = xy / (depth + 1e-9), depth [F, m, k] = the third homogeneous coordinate; a point with any coordinate equal to
 *   -1e6 gives -1e6 in kp2d and depth for every camera.                                                                            */
#define DM4D_TRIANG_MAX_VIEWS 65536
int dm4d_triangulate_points_f64(void* stream, const double* K, const double* T, const double* kp2d, const double* score,
                                const double* thr, int F, int n, int k, int min_views, double* kp3d, double* reproj,
                                int32_t* n_views);
int dm4d_project_points_f64(void* stream, const double* kp3d, const double* K, const double* T, int F, int m, int k, double* kp2d,
                            double* depth);

/* Skeleton maps (diffuman4d_amd/host/skeleton.py::draw_skeleton_maps; the reference's scripts/preprocess/draw_skeleton.py:158-178: the
 *   loop of cv2.line / cv2.circle calls on a canvas of 2048 pixels, then Image.fromarray(canvas).resize((w, h))) for n_frames frames of
 *   one shape in one launch.  prims: int32 records of DM4D_SKEL_FIELDS = {kind, x1, y1, x2, y2, size, r | g << 8 | b << 16, 0}, a frame's
 *   records in paint order; kind DM4D_SKEL_LINE: the segment p1 p2 with thickness `size` >= 1; DM4D_SKEL_CIRCLE: the disc of radius
 *   `size` >= 0 about p1 (p2 = p1).  offsets [n_frames + 1]: frame f owns records offsets[f] .. offsets[f + 1] - 1, at most
 *   DM4D_SKEL_MAX_PRIMS of them.  Coordinates lie in [DM4D_SKEL_COORD_MIN, DM4D_SKEL_COORD_MAX], sizes in [0, DM4D_SKEL_MAX_SIZE].
 *   Rasteriser (an exact integer rule, NOT OpenCV's edge walker, from which it differs on a primitive's rim only): a pixel is its integer
 *   coordinate (x, y), 0 <= x < W, 0 <= y < H.  A circle covers (x - x1)^2 + (y - y1)^2 <= size^2.  A line, with d = p2 - p1, L2 = d . d,
 *   v = (x, y) - p1, covers the union of {0 <= v . d <= L2 and 4 (v x d)^2 <= size^2 L2} (only when L2 > 0), 4 |(x, y) - p1|^2 <= size^2
 *   and 4 |(x, y) - p2|^2 <= size^2.  A pixel takes the colour of the last record of its frame that covers it, black if none does.
 *   Reduction: Pillow's Image.resize((w, h), BICUBIC) of the H x W RGB canvas, byte for byte: htab (W -> w) and vtab (H -> h) are tables
 *   of n outputs = n x {window start, window length} followed by n x ksize int32 coefficients with 22 fractional bits (hk, vk = ksize);
 *   the horizontal pass is rounded and clipped to uint8 before the vertical one.  The canvas is never stored: a workgroup paints the
 *   part of it that one tile of the output reads, in LDS; the entry picks the largest tile (32, 16 or 8 outputs square) whose part fits
 *   and refuses shapes where none does (canvas / output ratios above about 8).  out [n_frames, h, w, 3] uint8.
 *   *_host are host copies of the bytes at *_dev: counts, records and windows are validated on them before anything is launched.
 *   A frame's map is a function of its own records: bitwise repeatable, and independent of the batch.  No atomics.                  */
#define DM4D_SKEL_FIELDS 8
#define DM4D_SKEL_LINE 0
#define DM4D_SKEL_CIRCLE 1
#define DM4D_SKEL_MAX_PRIMS 512
#define DM4D_SKEL_COORD_MIN (-8192)
#define DM4D_SKEL_COORD_MAX 8191
#define DM4D_SKEL_MAX_SIZE 16384
int dm4d_skeleton_draw_u8(void* stream, const int32_t* prims_host, const int32_t* prims_dev, const int32_t* offsets_host,
                          const int32_t* offsets_dev, int n_frames, const int32_t* htab_host, const int32_t* htab_dev, int hk,
                          const int32_t* vtab_host, const int32_t* vtab_dev, int vk, int H, int W, int h, int w, uint8_t* out);

/* Skeleton maps straight from poses_3d (diffuman4d_amd/host/skeleton.py::draw_skeleton_maps_kp3d; DESIGN.md "Skeleton maps from
 *   poses_3d"): the plan that host/skeleton.py::plan_draw_calls makes of the poses_2d file which triangulate_skeleton would have written
 *   for a map's frame and camera, made on the device, and the draw of such a plan.
 *
 * dm4d_skeleton_plan_kp3d: n_maps maps (at most 65535) in one launch, one wave per map.  kp3d [F, k, 3], K [m, 3, 3], T [m, 4, 4] fp64 as
 *   dm4d_project_points_f64 takes them (k <= DM4D_SKEL_MAX_KPTS); jobs [n_maps, 2] int32 = {frame, camera}; scores [n_maps, k] fp32 or
 *   null (all ones): the score override.  Per map, computed on the host as plan_draw_calls does: scale [n_maps, 2] fp64 = {scale_ratio,
 *   centring offset}, sizes [n_maps, 2] int32 = {radius, thickness} after int(round(.)) (thickness >= 1, both <= DM4D_SKEL_MAX_SIZE / 2).
 *   Per palette: links [L, DM4D_SKEL_LINK_FIELDS] int32 = {keypoint 1, keypoint 2, id, radius multiplier, thickness multiplier (1 or 2:
 *   the MAJOR_LINKS rule), 0, 0, 0} in plan_draw_calls' order, X links appended; colors [k + L, 4] fp32 = {r, g, b, has-colour flag} of the
 *   keypoints, then of the links; low_thr, high_thr and thr_span = (float)(high_thr - low_thr) with the difference formed in fp64.
 *   A keypoint: project (the device function of dm4d_project_points_f64), u, v, depth rounded to fp32, score 0 where min(u, v) < 0 in
 *   fp32, x = (double)u * scale_ratio + offset (two fp64 roundings, likewise y), rint (half to even), inside iff both lie in
 *   [DM4D_SKEL_COORD_MIN, DM4D_SKEL_COORD_MAX].  A link: line_score = min of its endpoints' scores (fp32, a NaN wins); kept unless
 *   line_score < low_thr; a kept link with an endpoint that is not finite on the canvas sets DM4D_SKEL_ST_NONFINITE; a kept link with
 *   an endpoint not inside is dropped with its circles and counted; a link still kept that joins a keypoint without a colour sets
 *   DM4D_SKEL_ST_NOCOLOR, and the first such link's list index is stored above DM4D_SKEL_ST_LINK_SHIFT.  Colours: c * ((clip(score,
 *   low_thr, high_thr) - low_thr) / thr_span) in fp32, rint, uint8.  Paint order = Python's stable sorted(): descending on the fp64 mean of the
 *   two fp32 depths when any keypoint's depth is non-zero; else ascending on line_score when any keypoint's score differs from 1; else
 *   list order -- as a rank counted over all kept links (keys smaller, plus equal keys earlier in the list), no sort.
 *   -> records [n_maps, 3 L, DM4D_SKEL_FIELDS] int32 (16-byte aligned; a kept link gives {line, circle at keypoint 1, circle at
 *   keypoint 2}; the slots past a map's count are zero), counts [n_maps] int32, status [n_maps, 2] int32 = {flag bits, dropped links}.
 *   3 L <= DM4D_SKEL_MAX_PRIMS.  *_host are host copies of the bytes at *_dev, validated before the launch (jobs inside F and m, sizes,
 *   link indices inside k, ids inside L, multipliers, colours inside [0, 255], every link coloured).  No atomics, no workgroup waits on
 *   another; a map's output is a function of its own inputs: bitwise repeatable and independent of the batch.
 * dm4d_skeleton_draw_planned_u8: dm4d_skeleton_draw_u8 (one kernel body) on such a plan: map f owns records f * stride .. f * stride +
 *   counts[f] - 1 with stride = 3 L; the kernel clamps the count it reads to [0, stride].  Shapes, alignment, stride and the tables'
 *   windows are validated on the host; the records are in range by construction.  Same output layout.                                  */
#define DM4D_SKEL_MAX_KPTS 2048
#define DM4D_SKEL_LINK_FIELDS 8
#define DM4D_SKEL_ST_NONFINITE 1
#define DM4D_SKEL_ST_NOCOLOR 2
#define DM4D_SKEL_ST_LINK_SHIFT 8
int dm4d_skeleton_plan_kp3d(void* stream, const double* kp3d, const double* K, const double* T, int F, int m, int k,
                            const int32_t* jobs_host, const int32_t* jobs_dev, int n_maps, const float* scores,
                            const double* scale_host, const double* scale_dev, const int32_t* sizes_host, const int32_t* sizes_dev,
                            const int32_t* links_host, const int32_t* links_dev, int L, const float* colors_host,
                            const float* colors_dev, float low_thr, float high_thr, float thr_span, int32_t* records,
                            int32_t* counts, int32_t* status);
int dm4d_skeleton_draw_planned_u8(void* stream, const int32_t* records, const int32_t* counts, int n_frames, int stride,
                                  const int32_t* htab_host, const int32_t* htab_dev, int hk, const int32_t* vtab_host,
                                  const int32_t* vtab_dev, int vk, int H, int W, int h, int w, uint8_t* out);

/* Bounding box and box mask of drawn skeleton maps (diffuman4d_amd/host/capture.py::SpaTemDataset, skeleton_source="kp2d"; the reference's
 *   src/data/utils/crop_utils.py skeleton_to_mask, called from spatem_dataset.py:124-127 for has_gt_target=False targets).
 *   maps [n_frames, h, w, 3] uint8, tight (what dm4d_skeleton_draw_u8 writes).  A pixel counts when any of its channels is non-zero.
 *   boxes [n_frames, 4] int32 = {first column, first row, last column, last row} of the counting pixels, {w, h, -1, -1} for a map without
 *   one.  Mask slot f = masks + f * mask_stride holds [h, w] uint8 (mask_stride >= h * w; slots need no alignment): 255 on rows
 *   max(first row - 1 - pad_top, 0) .. min(last row + 1 + pad_bottom, h) - 1 and columns max(first column - 1 - pad_x, 0) ..
 *   min(last column + 1 + pad_x, w) - 1, 0 elsewhere; all 0 for a map without a counting pixel.  With pad_bottom = pad_y = int(0.03 h),
 *   pad_top = 3 pad_y and pad_x = int(0.03 w) this plane is skeleton_to_mask's result byte for byte (its float32 channel mean is non-zero
 *   exactly where a channel is, and every pixel it leaves outside the box is zero).
 *   Three launches on `stream`: per-block extrema over 16-byte loads (scalar head and tail where a frame does not start or end on a
 *   16-byte address), one wave per frame that folds them (fixed lanes, then a shuffle tree), and the fill, which reads boxes on the device (no host
 *   round trip in between).  Integers only, no atomics, no block waits on another: a frame's result is the same alone or in a batch.
 *   ws: dm4d_skeleton_box_mask_ws_bytes(n_frames, h, w) bytes (0 for a shape out of range), 4-byte aligned.                          */
size_t dm4d_skeleton_box_mask_ws_bytes(int n_frames, int h, int w);
int dm4d_skeleton_box_mask_u8(void* stream, const uint8_t* maps, int n_frames, int h, int w, int pad_top, int pad_bottom, int pad_x,
                              int32_t* boxes, uint8_t* masks, int64_t mask_stride, void* ws, int64_t ws_bytes);

/* Result images on the device (jpeg.hip): the two host steps of the reference's result writer, sampling_utils.py:95-114
 *   (`restore_cropped_image(to_pil_image(img), crop).save(path, quality=90)`) and image_utils.py:62-93 (restore_cropped_image).
 *
 * dm4d_restore_crop_u8 (image_utils.py:62-93): per image, Pillow's Image.resize((cw, ch), BICUBIC) of the H x W RGB source (horizontal
 *   pass rounded to uint8 into `scratch`, then the vertical pass: the arithmetic of dm4d_capture_crop_resize_f32) pasted at (cl, ct) of a
 *   white canvas_h x canvas_w canvas, clipped to the canvas.  Two launches for all images.  desc: n x DM4D_RESTORE_FIELDS int64 = {source
 *   byte offset in pixels | H, W | ct, cl, ch, cw | canvas_h, canvas_w | horizontal table offset, ksize | vertical table offset, ksize |
 *   scratch byte offset (H x cw x 3 bytes) | canvas byte offset in canvases | 0}; tab as for dm4d_capture_crop_resize_f32 (W -> cw and
 *   H -> ch).  desc_host / tab_host are host copies of desc_dev / tab_dev; every size, offset, window and region is validated on them
 *   before anything is launched, and canvas regions may not overlap (they must be listed in ascending order).
 *
 * dm4d_jpeg_encode_rgb_u8 (sampling_utils.py:95-114, PIL's Image.save(path, quality=q) of an RGB image): the entropy-coded segment of
 *   the baseline 4:2:0 JPEG libjpeg writes with the Annex-K Huffman tables, for n images of different sizes in one call, byte for byte.
 *   Integer arithmetic only.  Eight launches for the whole batch and no workgroup waits for another: coefficients (colour conversion,
 *   h2v2 downsample, jfdctint "islow", quantisation, zig-zag; one wave per 16 x 16 MCU), Huffman bit length of every MCU, a scan per
 *   image, emission of the unstuffed bit stream (the MCU in which a byte starts writes it; the few trailing bits come from the next
 *   MCU's "head bits" of the sizing pass), 0xFF counts per DM4D_JPEG_CHUNK bytes, their scan, the images' offsets, and the stuffed write.
 *   An image's bytes do not depend on the rest of the batch.
 *   desc: n x DM4D_JPEG_FIELDS int64 = {space: 0 = pixels, 1 = canvases | byte offset of the uint8 HWC image there (rows tight) |
 *   h, w in 1..65535 | index of the image's first MCU = the MCUs of the images before it | index of its first stuffing chunk = the sum of
 *   ceil(mcus * DM4D_JPEG_MCU_UNSTUFFED / DM4D_JPEG_CHUNK) before it | 0, 0}.  qtab: uint16 [2][64], the luma and chroma quantisation
 *   tables in natural order, values 1..255.  desc_host / qtab_host are host copies, validated before anything is launched.
 *   Bound per MCU: a block codes at most 20 bits of DC (9 + 11) and 63 x 26 bits of AC (16 + 10), so an MCU of six blocks is at most
 *   9948 bits = 1244 bytes unstuffed (DM4D_JPEG_MCU_UNSTUFFED reserves 1248) and, were every byte 0xFF, DM4D_JPEG_MCU_BOUND = 2488 bytes
 *   stuffed; the padded last byte is inside that count.  An MCU is never shorter than 32 bits (4 x (2 + 4) + 2 x (2 + 2)).
 *   dm4d_jpeg_scan_bound(h, w) = mcus * DM4D_JPEG_MCU_BOUND (0 for a size outside 1..65535 or one whose bit count could pass 2^32).
 *   blob: the n scans back to back; blob_bytes >= the sum of the images' bounds.  out: device int64 [2 n] = n byte offsets into blob,
 *   then n lengths; the host reads them and copies blob[: offset[n - 1] + length[n - 1]].
 *   workspace: dm4d_jpeg_ws_bytes(total MCUs, n) bytes, 16-byte aligned (0 for counts out of range).                                    */
#define DM4D_RESTORE_FIELDS 16
#define DM4D_JPEG_FIELDS 8
#define DM4D_JPEG_MCU_UNSTUFFED 1248
#define DM4D_JPEG_MCU_BOUND 2488
#define DM4D_JPEG_CHUNK 4096
int dm4d_restore_crop_u8(void* stream, const void* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                         const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, void* scratch, int64_t scratch_bytes,
                         void* canvases, int64_t canvases_bytes);
size_t dm4d_jpeg_scan_bound(int h, int w);
size_t dm4d_jpeg_ws_bytes(int64_t total_mcus, int n);
int dm4d_jpeg_encode_rgb_u8(void* stream, const void* pixels, int64_t pixels_bytes, const void* canvases, int64_t canvases_bytes,
                            const int64_t* desc_host, const int64_t* desc_dev, int n, const uint16_t* qtab_host, const uint16_t* qtab_dev,
                            void* workspace, int64_t workspace_bytes, void* blob, int64_t blob_bytes, int64_t* out);

/* 2-D keypoint prediction around a caller-named pose network (pose.hip, diffuman4d_amd/host/pose.py::predict_keypoints; the reference's
 *   predict_keypoints stage, scripts/preprocess/sapiens/lite/demo/vis_pose.py:45-63 and :92-109 with pose_utils.py:13-179 and :182-279).
 *   The network itself is the caller's; these are the steps on either side of it.
 *
 * dm4d_pose_input_u8_f32 (vis_pose.py preprocess_pose with sapiens_utils' Image.composite(image, black, fmask) before it): the network's
 *   input for `rows` (image, box) pairs in one launch -> out [rows, 3, H, W] fp32, planes R, G, B.
 *   staging: device bytes holding uint8 RGB images (HWC, rows tight) and uint8 L masks.  desc: rows x DM4D_POSE_FIELDS int64 = {image byte
 *   offset | mask byte offset or -1 | image h, w (1..DM4D_POSE_MAX_SIDE) | offset of the row's warp table in tab, in int32 elements | 0, 0, 0};
 *   rows may differ in size and may share an image.  A row's warp table = {adelta[W] | bdelta[W] | X0[H] | Y0[H]} int32 with 10 fractional
 *   bits, made by the host from the inverse A of get_udp_warp_matrix(center, scale, 0, (W, H)) in fp64: adelta[x] = rint(1024 A00 x),
 *   bdelta[x] = rint(1024 A10 x), X0[y] = rint(1024 (A01 y + A02)) + 16, Y0[y] = rint(1024 (A11 y + A12)) + 16, each within +-DM4D_POSE_TAB_LIMIT.
 *   Output pixel (x, y): X = (X0[y] + adelta[x]) >> 5, Y = (Y0[y] + bdelta[x]) >> 5 (1/32 pixel); source pixel (X >> 5, Y >> 5), fractions
 *   fx = X & 31, fy = Y & 31; weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (they sum to 32768) on the taps
 *   (0,0), (1,0), (0,1), (1,1); v = (sum w t + 2^14) >> 15.  A tap is the composited pixel MULDIV255(p, m) = (((p m + 128) >> 8) + p m + 128) >> 8
 *   of the image byte p and the mask byte m (p itself without a mask), 0 outside the image.  Integers only up to here: a rule modelled on
 *   OpenCV's bilinear warpAffine, not a copy of its code paths.  out = (float(v) - mean[c]) / std[c], each operation rounded to fp32 on its
 *   own (bit-equal to torch-CPU `(v.float() - mean) / std`); norm_host = {mean R, G, B | std R, G, B} fp32 on the host.
 *   desc_host / tab_host are host copies of the bytes at desc_dev / tab_dev: offsets, sizes and table entries are validated on them before
 *   the launch.  A row's result is a function of its own descriptor, table and planes: independent of the batch, bitwise repeatable.
 * dm4d_pose_mask_box_u8: boxes [n, 4] int32 = {x1, y1, x2, y2} = {first column, first row, last column + 1, last row + 1} of the pixels >= 128
 *   of each row's mask (descriptor fields 1-3; field 0 is not read), {0, 0, w, h} for a mask without one.  One workgroup per mask, one pass
 *   of 16-byte loads, shuffles and LDS; no atomics.
 * dm4d_pose_udp_decode_f32 (pose_utils.py udp_decode up to its division by the heatmap size: get_heatmap_maximum, gaussian_blur with an
 *   11 x 11 kernel, refine_keypoints_dark_udp): heatmaps [n, K, Hh, Wh] fp32 contiguous -> scores [n, K] = each map's maximum, bit for bit;
 *   locs [n, K, 2] fp32 = the refined (x, y) in heatmap pixels.  One workgroup per map.  The location starts at the first maximum in
 *   row-major order (np.argmax).  The map is blurred with the separable 11-tap Gaussian of sigma 2 (taps exp(-x^2 / 8) / sum in fp64, rounded
 *   to fp32; zeros outside the map, which is what the reference's pad-by-5 + reflecting blur + crop computes), rows first, in bands of at
 *   most 32 rows with a 5-row halo either side held in LDS, each tap sum an fmaf chain in ascending tap order; scaled by maximum /
 *   blurred maximum, clipped to [1e-3, 50], log; dx, dy, dxx, dyy, dxy from the 3 x 3 neighbourhood (replicated at the map's edge) in fp32
 *   as the reference writes them; the 2 x 2 Hessian + FLT_EPSILON I is inverted in fp64 (adjugate / determinant) and location - H^-1 d is
 *   rounded to fp32 once.  A map whose maximum is <= 0 keeps location (-1, -1) and is not refined (the reference reads wrapped-around
 *   memory there).  Non-finite heatmaps are unspecified.  No atomics; a map's result does not depend on the batch.                   */
#define DM4D_POSE_FIELDS 8
#define DM4D_POSE_MAX_SIDE 16384
#define DM4D_POSE_MAX_HEATMAP_H 4096
#define DM4D_POSE_MAX_HEATMAP_W 1024
#define DM4D_POSE_TAB_LIMIT (1 << 29) /* |warp table entry|: the sum of two stays inside int32 */
int dm4d_pose_input_u8_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                           int rows, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const float* norm_host, float* out,
                           int H, int W);
int dm4d_pose_mask_box_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                          int32_t* boxes);
int dm4d_pose_udp_decode_f32(void* stream, const float* heatmaps, int n, int K, int Hh, int Wh, float* scores, float* locs);

/* Person boxes around a caller-named detector (detect.hip, diffuman4d_amd/host/detect.py; the reference's detector step of
 *   predict_keypoints: scripts/preprocess/sapiens/lite/demo/vis_pose.py:425-440, detector_utils.py process_one_image_bbox, pose_utils.py
 *   nms).  The network itself is the caller's; these are the steps on either side of it.  tests/detect_model.py is the definition in
 *   numpy and DESIGN.md "Person boxes" its text.  No global atomics, no float atomics, no workgroup waits on another; an image's result
 *   is a function of its own descriptor, table, planes and rows: independent of the batch, bitwise repeatable.
 *
 * dm4d_detect_input_u8_f32: the detector's input for n staged images of different sizes in one launch -> out [n, 3, H, W] fp32.
 *   staging / desc (n x DM4D_POSE_FIELDS) / desc_host / tab_host as for dm4d_pose_input_u8_f32, with every plane offset 16-byte aligned
 *   and field 4 the offset of the image's resize table in tab, in int32 elements.  The table = {nw, nh | xofs[nw] | yofs[nh] | alpha[nw]
 *   | beta[nh]}: the size nw x nh (1..W x 1..H) of the keep-ratio resized image in the canvas' top-left corner; the first source column /
 *   row of every output column / row (0..w - 1, 0..h - 1); and per column / row the two int16 weights c0 | c1 << 16 (each 0..2048) of the
 *   taps s and min(s + 1, last).  A tap is the composited pixel MULDIV255(p, m) (p itself without a mask).  Horizontal pass in int32:
 *   S = t[s] c0 + t[s + 1] c1 per row; vertical: v = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.  Integers only up to
 *   here: a rule modelled on OpenCV's 8-bit INTER_LINEAR resize, not a copy of its code paths.  Outside nw x nh, v = pad_value (0..255).
 *   out plane c = (float(v of channel c, or of channel 2 - c with bgr != 0) - mean[c]) / std[c], each operation rounded to fp32 on its
 *   own; norm_host = {mean[3] | std[3]} fp32 on the host.  A workgroup owns a 64 x 4 tile of the canvas.
 * dm4d_detect_select_f32: dense detector output -> kept boxes, one workgroup per image.  boxes [n, A, 4] fp32 (x1, y1, x2, y2 in
 *   network-input pixels), scores [n, A, C] fp32, inv_scale [n, 2] fp32 = {inv_w, inv_h}, all on the device, contiguous; 1 <= A <=
 *   DM4D_DETECT_MAX_ANCHORS, 1 <= C <= DM4D_DETECT_MAX_CLASSES, 0 <= cat < C, 1 <= max_per_img <= DM4D_DETECT_MAX_KEEP, thresholds finite.
 *   (1) candidates: scores[a, cat] > score_thr (NaN never passes); (2) image box = (x1 inv_w, y1 inv_h, x2 inv_w, y2 inv_h), one fp32
 *   multiply each; a candidate whose image box is not finite or has x2 <= x1 or y2 <= y1 is dropped; (3) the rest ordered by score
 *   descending (-0 counts as +0), then anchor index ascending; the first max_per_img stay; (4) greedy NMS in that order in fp32, every
 *   operation rounded on its own: area = (x2 - x1 + 1)(y2 - y1 + 1), w = max(0, min(x2) - max(x1) + 1), h likewise, ovr = w h / (area_i
 *   + area_j - w h) by IEEE division; a later box survives iff ovr <= nms_thr (a NaN ovr does not).  Out: counts [n, 3] int32 = {kept,
 *   dropped in (2), candidates of (1)}; out_boxes [n, max_per_img, 5] fp32 = x1, y1, x2, y2, score in kept order, zeros behind `kept`;
 *   out_idx [n, max_per_img] int32 anchor indices, -1 behind `kept`.  The selection is exact whatever the number of candidates: a radix
 *   select (8 bits a pass, LDS histograms with integer LDS atomics) over the unique 64-bit keys {ordered score bits << 32 | ~index}, run
 *   only when more than max_per_img candidates remain, then a bitonic sort of at most DM4D_DETECT_MAX_KEEP keys.                     */
#define DM4D_DETECT_MAX_ANCHORS (1 << 20)
#define DM4D_DETECT_MAX_CLASSES 4096
#define DM4D_DETECT_MAX_KEEP 256
#define DM4D_DETECT_MAX_CANVAS 4096
#define DM4D_DETECT_COEF_ONE 2048 /* the sum of a tap pair's weights */
int dm4d_detect_input_u8_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev,
                             int n, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const float* norm_host, float* out,
                             int H, int W, int pad_value, int bgr);
int dm4d_detect_select_f32(void* stream, const float* boxes, const float* scores, const float* inv_scale, int n, int A, int C, int cat,
                           float score_thr, float nms_thr, int max_per_img, int32_t* counts, float* out_boxes, int32_t* out_idx);

/* Foreground-mask prediction around a caller-named matting network (matting.hip, diffuman4d_amd/host/matting.py::remove_background; the
 *   reference's remove_background stage, scripts/preprocess/remove_background.py:15-22 and :36-93).  The network itself is the caller's;
 *   these are the steps on either side of it.  Integer arithmetic apart from the table lookups; no atomics, no workgroup waits on
 *   another; an image's result is a function of its own descriptor, tables and plane: independent of the batch, bitwise repeatable.
 *
 * Both entries take n x DM4D_MATTING_FIELDS int64 descriptors = {byte offset of the image's plane | h, w of the image as stored
 *   (1..DM4D_MATTING_MAX_SIDE) | offset of the horizontal coefficient table in tab (int32 elements), or -1 | its ksize | offset of the
 *   vertical table, or -1 | its ksize | byte offset of the image's scratch region (16-byte aligned)}.  rot = quarter turns clockwise
 *   (0..3) of Image.rotate(-90 rot, expand=True), applied as an index map: the rotated image is rh x rw = h x w (rot even) or w x h (odd).
 *   tab as for dm4d_capture_crop_resize_f32: per table, `out` windows {start, length} then out x ksize weights with 22 fractional bits,
 *   applied by Pillow's rule (horizontal pass rounded to uint8, then the vertical pass; clip8((2^21 + sum u k) >> 22)).  An axis whose
 *   size does not change has no table (-1) and is not filtered, as in Pillow; any other axis must have one.  desc_host / tab_host are
 *   host copies of the bytes at desc_dev / tab_dev: sizes, offsets, windows and regions are validated on them before anything is launched.
 *
 * dm4d_matting_input_u8 (transforms.Resize + ToTensor + Normalize + .half()): staging holds uint8 RGB images (HWC, rows tight).  Each is
 *   rotated, resized rw -> S_w (scratch: rh x S_w packed words r | g << 8 | b << 16) and rh -> S_h, and every byte b of channel c becomes
 *   lut[c * 256 + b] -> out [n, 3, S_h, S_w] of fp16 (out_f32 = 0) or fp32 (1); lut_dev: 3 x 256 values of that type on the device, made
 *   by the host with the reference's own arithmetic.  At most two launches.
 * dm4d_matting_mask_f16_u8 (.sigmoid() + to_pil_image + resize(image.size) + the rotation back): logits [n, S_h, S_w] fp16; a value with
 *   bit pattern p is the byte qtab_dev[p] (65536 bytes on the device: the kernels contain no exp).  The byte plane is resized S_w -> rw
 *   (the lookup is part of this pass; scratch: S_h x rw bytes) and S_h -> rh, turned back by the same index map and written as h x w bytes
 *   (rows tight) at the image's offset in blob, which must be 16-byte aligned.  At most two launches.                                  */
#define DM4D_MATTING_FIELDS 8
#define DM4D_MATTING_MAX_SIDE 16384
int dm4d_matting_input_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                          const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* lut_dev, void* scratch,
                          int64_t scratch_bytes, void* out, int S_h, int S_w, int rot, int out_f32);
int dm4d_matting_mask_f16_u8(void* stream, const void* logits, const int64_t* desc_host, const int64_t* desc_dev, int n,
                             const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* qtab_dev, void* scratch,
                             int64_t scratch_bytes, void* blob, int64_t blob_bytes, int S_h, int S_w, int rot);

/* PNG files on the device (png.hip; diffuman4d_amd/host/png.py, the `device_png` route of host/matting.py::remove_background): n 8-bit
 *   images of different sizes -> n complete files back to back in blob, every byte made on the device (signature, IHDR, one IDAT chunk
 *   per stripe, IEND, the chunk CRC-32s, the zlib header and the Adler-32).  tests/png_model.py is the definition in numpy and DESIGN.md
 *   "Device PNG" its text: Paeth filter (type 4) on every row; the filtered stream (R = 1 + w * channels bytes a row) in stripes of
 *   max(1, DM4D_PNG_STRIPE_BYTES / R) whole rows; in a stripe a maximal run of n equal bytes = a literal, (n - 1) / 258 matches of length
 *   258 at distance 1, and the rest r as one match (r >= 3) or r literals; one dynamic-Huffman block per stripe from a canonical code
 *   built on the device (lengths at most 15, and 7 for the code-length alphabet), then an empty stored block to the byte boundary.
 *   Integer only; five launches whatever n is; no workgroup waits on another; LDS integer atomics only; a file depends on its image
 *   alone and is the same in every call.
 * desc: n x DM4D_PNG_FIELDS int64 = {kind: DM4D_PNG_L or DM4D_PNG_RGBA | h, w in 1..DM4D_MATTING_MAX_SIDE | L: byte offset of the plane
 *   in `planes`; RGBA: of the packed 3-byte RGB image in `rgb` | its row stride in bytes (>= w, >= 3 w) | RGBA: byte offset of the alpha
 *   plane in `planes`, and its row stride; L: 0, 0 | byte offset of the image's filtered stream = the sum of h * R before it | index of
 *   its first stripe = the stripes before it | 0 ...}.  desc_host is the host copy of desc_dev, validated before anything is launched.
 * dm4d_png_bound(h, w, channels 1 or 4) = 64 + 576 stripes + 2 h R (0 out of range): a token costs at most 15 bits per byte it covers,
 *   a block header at most 17 + 57 + 288 x 14 bits.  blob_bytes >= the sum of the images' bounds, or the call is an error.
 * out: device int64 [2 n] = n byte offsets into blob, then n lengths; the host copies blob[: offset[n - 1] + length[n - 1]].
 * workspace: dm4d_png_ws_bytes(sum of h * R, total stripes, n) bytes, 16-byte aligned (0 for counts out of range).                    */
#define DM4D_PNG_FIELDS 16
#define DM4D_PNG_L 0
#define DM4D_PNG_RGBA 1
#define DM4D_PNG_STRIPE_BYTES 32768
#define DM4D_PNG_STRIPE_REC 1712
size_t dm4d_png_bound(int h, int w, int channels);
size_t dm4d_png_ws_bytes(int64_t filtered_bytes, int64_t stripes, int n);
int dm4d_png_encode_u8(void* stream, const void* planes, int64_t planes_bytes, const void* rgb, int64_t rgb_bytes, const int64_t* desc_host,
                       const int64_t* desc_dev, int n, void* workspace, int64_t workspace_bytes, void* blob, int64_t blob_bytes,
                       int64_t* out);

/* Lossless WebP files on the device (webp.hip; diffuman4d_amd/host/webp.py, the `device_webp` route of host/skeleton.py::draw_skeleton):
 *   n packed 8-bit RGB images of different sizes -> n complete files (RIFF framing + one VP8L chunk) back to back in blob.
 *   tests/webp_model.py is the definition in numpy and DESIGN.md "Device WebP (lossless)" its text: no transform, no colour cache, one
 *   group of five prefix codes per image; the pixels p = y w + x in stripes of DM4D_WEBP_STRIPE_PIXELS; a pixel's kind is U (equals
 *   pixel p - w), else L (equals pixel p - 1), else literal; within a stripe a maximal run of one kind is cut into backward references
 *   of at most 4096 pixels with distance plane code 1 (U) or 2 (L); canonical codes (lengths at most 15, and 7 for the code-length
 *   code) from the image's histograms, sent as simple codes where at most two symbols below 256 are used.  Stripes are not byte
 *   aligned: a stripe stores the bytes it fills alone and records its first and last partial bytes, which one lane per shared byte
 *   ORs together in the last launch.  Integer only; five launches whatever n is; no workgroup waits on another; LDS integer atomics
 *   only; a file depends on its image alone and is the same in every call.
 * desc: n x DM4D_WEBP_FIELDS int64 = {h, w in 1..DM4D_WEBP_MAX_SIDE | byte offset of the image in `rgb` | its row stride in bytes
 *   (>= 3 w) | index of its first pixel = the sum of h * w before it | index of its first stripe = the stripes before it | 0, 0}.
 *   desc_host is the host copy of desc_dev, validated before anything is launched.
 * dm4d_webp_bound(h, w) = 800 + 6 h w (0 out of range): a pixel costs at most 45 bits, the header and code tables less than 780 bytes.
 *   blob_bytes >= the sum of the images' bounds, or the call is an error.
 * out: device int64 [2 n] = n byte offsets into blob, then n lengths; the host copies blob[: offset[n - 1] + length[n - 1]].
 * workspace: dm4d_webp_ws_bytes(sum of h * w, total stripes, n) bytes, 16-byte aligned (0 for counts out of range).                  */
#define DM4D_WEBP_FIELDS 8
#define DM4D_WEBP_MAX_SIDE 16383
#define DM4D_WEBP_STRIPE_PIXELS 8192
#define DM4D_WEBP_STRIPE_REC 3200
#define DM4D_WEBP_IMAGE_REC 4096
size_t dm4d_webp_bound(int h, int w);
size_t dm4d_webp_ws_bytes(int64_t pixels, int64_t stripes, int n);
int dm4d_webp_encode_u8(void* stream, const void* rgb, int64_t rgb_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                        void* workspace, int64_t workspace_bytes, void* blob, int64_t blob_bytes, int64_t* out);

/* Baseline JPEG files decoded on the device (jpegdec.hip; diffuman4d_amd/host/jpegdec.py): n files of the supported set (SOF0, 8 bits,
 *   one interleaved Huffman scan without restart markers, grayscale or YCbCr at 4:4:4 / 4:2:2 / 4:2:0 -- host/jpegdec.py::probe) ->
 *   their pixels, byte for byte libjpeg's default decompression (Huffman decoding, jidctint "islow", "fancy" up-sampling, the 16-bit
 *   YCbCr -> RGB tables).  tests/jpegdec_model.py is the definition in numpy and DESIGN.md "Device JPEG decode" its text.  Integer only;
 *   a fill and two launches whatever n is; no workgroup waits on another; no atomics; an image depends on its file alone and is the
 *   same in every call.
 * scans: the files' entropy-coded segments with the FF 00 stuffing removed, each starting on a multiple of 4 bytes.
 * desc: n x DM4D_JPEGDEC_FIELDS int64 = {byte offset of the scan in `scans` | its bytes (1 .. DM4D_JPEGDEC_MAX_SCAN_BYTES - 1) | h, w in
 *   1..65535 | components 1 or 3 | luma sampling factors h, v: 1 1, 2 1 or 2 2 (1 1 for one component) | byte offset of the image in
 *   `out` | bytes per pixel there: 3 (grayscale replicated), or 1 for one component; rows tight | index of its first coefficient block =
 *   the blocks before it, an image having MCUs x (1 or h v + 2) | 0 ...}.  desc_host is the host copy of desc_dev, validated before
 *   anything is launched.
 * tab: n x DM4D_JPEGDEC_TABLE_BYTES uint8 = per component (three; a grayscale file repeats its one) {DC BITS [16], DC HUFFVAL [16], AC
 *   BITS [16], AC HUFFVAL [256]}, then per component the 64 quantisers (8-bit) in natural order.  The lookup tables are built on the
 *   device.  tab_host is validated like libjpeg validates a DHT.
 * The scan is decoded speculatively in subsequences of DM4D_JPEGDEC_SUB_BITS bits, DM4D_JPEGDEC_TILE_LANES of them per tile.
 * status: device int32 [n]; nonzero (DM4D_JPEGDEC_ST_* bits) = the image's pixels are unspecified: a window no Huffman code starts, a
 *   zig-zag index past 63, a scan that ends early or has data left over, a dequantised coefficient outside [-8192, 8191].
 * workspace: dm4d_jpeg_decode_ws_bytes(total blocks, n) bytes (int16 [64] per block), 16-byte aligned (0 for counts out of range).  */
#define DM4D_JPEGDEC_FIELDS 16
#define DM4D_JPEGDEC_TABLE_BYTES 1104
#define DM4D_JPEGDEC_SUB_BITS 1024
#define DM4D_JPEGDEC_TILE_LANES 256
#define DM4D_JPEGDEC_MAX_SCAN_BYTES (1 << 28)
#define DM4D_JPEGDEC_ST_BAD_CODE 1
#define DM4D_JPEGDEC_ST_ZIGZAG 2
#define DM4D_JPEGDEC_ST_END 4
#define DM4D_JPEGDEC_ST_RANGE 8
size_t dm4d_jpeg_decode_ws_bytes(int64_t total_blocks, int n);
int dm4d_jpeg_decode_u8(void* stream, const void* scans, int64_t scans_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                        const uint8_t* tab_host, const uint8_t* tab_dev, void* workspace, int64_t workspace_bytes, void* out,
                        int64_t out_bytes, int32_t* status);

/* 8-bit PNG files decoded on the device (pngdec.hip; diffuman4d_amd/host/pngdec.py): n files of the supported set (bit depth 8, colour
 *   type 0, 2 or 6, not interlaced -- host/pngdec.py::probe) -> their pixels, byte for byte ``np.asarray(Image.open(file))``.
 *   tests/pngdec_model.py is the definition in numpy and DESIGN.md "Device PNG decode" its text.  Integer only; two launches whatever n
 *   is; no workgroup waits on another; no atomics; an image depends on its file alone and is the same in every call.
 *   inflate   one workgroup (one wave) per image: zlib header, stored / fixed / dynamic blocks (RFC 1950 / 1951, table validity as
 *             zlib's inflate_table), lookup tables built in LDS, literal runs and match copies by all lanes; the last
 *             DM4D_PNGDEC_RING_BYTES / 2 bytes of output live in an LDS ring whose halves are flushed to the workspace with 16-byte
 *             stores and summed into the Adler-32.  Output: the filtered scanlines, h * (1 + w * channels) bytes.
 *   unfilter  one wave per image, a skewed wavefront over bands of 64 rows (lane j = row 64 b + j, one pixel behind lane j - 1); the
 *             five predictors are selected by the row's filter byte; a band's last row stays in LDS (DM4D_PNGDEC_MAX_ROW_BYTES).
 * streams: the files' concatenated IDAT payloads, each starting on a multiple of 4 bytes (and padded to one).
 * desc: n x DM4D_PNGDEC_FIELDS int64 = {byte offset of the stream in `streams` | its bytes (2 .. DM4D_PNGDEC_MAX_STREAM_BYTES - 1) | h, w
 *   >= 1 with w * channels <= DM4D_PNGDEC_MAX_ROW_BYTES and h * (1 + w * channels) < 2^31 | the file's channels: 1, 3 or 4 | byte offset
 *   of the image in `out` | bytes per pixel there: the file's channels; rows tight | byte offset of its filtered stream in the workspace
 *   = the sum of h * (1 + w * channels), each rounded up to 16, before it}.  desc_host is the host copy of desc_dev, validated before
 *   anything is launched.
 * status: device int32 [n]; nonzero (DM4D_PNGDEC_ST_* bits) = the image's pixels are unspecified: HEADER the zlib header; BLOCK a block
 *   header, a stored length, a code-length rule or an invalid set of code lengths; CODE an undefined or reserved code; DISTANCE a
 *   distance before the start of the output; END the stream exhausted before the final block ends, or an output length other than
 *   h * (1 + w * channels); ADLER the Adler-32; FILTER a filter byte other than 0 .. 4.  The unfilter launch skips an image whose
 *   inflate status is nonzero.
 * workspace: dm4d_png_decode_ws_bytes(sum of the rounded filtered sizes, n) bytes, 16-byte aligned (0 for counts out of range).        */
#define DM4D_PNGDEC_FIELDS 8
#define DM4D_PNGDEC_RING_BYTES 65536
#define DM4D_PNGDEC_MAX_ROW_BYTES 32768
#define DM4D_PNGDEC_MAX_STREAM_BYTES (1 << 28)
#define DM4D_PNGDEC_ST_HEADER 1
#define DM4D_PNGDEC_ST_BLOCK 2
#define DM4D_PNGDEC_ST_CODE 4
#define DM4D_PNGDEC_ST_DISTANCE 8
#define DM4D_PNGDEC_ST_END 16
#define DM4D_PNGDEC_ST_ADLER 32
#define DM4D_PNGDEC_ST_FILTER 64
size_t dm4d_png_decode_ws_bytes(int64_t total_filtered_bytes, int n);
int dm4d_png_decode_u8(void* stream, const void* streams, int64_t streams_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                       void* workspace, int64_t workspace_bytes, void* out, int64_t out_bytes, int32_t* status);

/* Raw-capture rectification (rectify.hip; diffuman4d_amd/host/rectify.py::extract_images; the reference's
 *   scripts/download/extract_dnar_images.py:89-120 calib_undist_image): colour correction, undistortion to a pinhole camera, area resize
 *   and crop of n uint8 RGB images of different sizes, cameras and tables in ONE launch.  tests/rectify_model.py is the definition in
 *   numpy and DESIGN.md "Raw-capture rectification" its text; the result is the model's byte for byte.  A workgroup owns a 32 x 8 tile of
 *   an image's cropped output and keeps the patch of the undistorted image that the tile's area windows name in LDS only.  No atomics, no
 *   workgroup waits on another; an image's result depends on its own descriptor, tables and source: independent of the batch, bitwise
 *   repeatable.
 * staging: uint8 RGB sources, HWC with tight rows.  desc: n x DM4D_RECTIFY_FIELDS int64 = {byte offset of the source in staging (16-byte
 *   aligned) | h, w of the source | uh, uw of the undistorted image | rh, rw of the resized image (all 1..DM4D_RECTIFY_MAX_SIDE, each
 *   axis' scale uw / rw, uh / rh in 1..DM4D_RECTIFY_MAX_SCALE) | top, left, height, width of the crop of the resized image | offset of
 *   the horizontal table in tab (int32 elements), its taps per window (ksize) | the same for the vertical table | offset of the camera
 *   constants in tab | byte offset of the result in out (16-byte aligned; height x width x 3 bytes, rows tight) | 0 ...}.
 * tab: int32 / fp32 words.  A table of an axis n_in -> n_out: n_out windows {first source cell, taps (1..ksize)}, starts and ends
 *   ascending, inside 0..n_in; then n_out x ksize fp32 weights.  Camera constants: 16 fp32 = {fx, fy, cx, cy of the distorted camera |
 *   k1, k2, p1, p2, k3 | cx, cy of the undistorted camera | fp32(1 / fx), fp32(1 / fy) of it, divided in fp64 | 0, 0, 0}.
 * lut_dev: n x 3 x 256 fp32 on the device: what the colour correction makes of every byte of every channel of image k.
 * desc_host / tab_host are the host copies of desc_dev / tab_dev: every size, offset, window and crop is validated on them before
 *   anything is launched (DM4D_ERR_ARG).                                                                                              */
#define DM4D_RECTIFY_FIELDS 20
#define DM4D_RECTIFY_MAX_SIDE 16384
#define DM4D_RECTIFY_MAX_SCALE 8
int dm4d_rectify_u8(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host, const int64_t* desc_dev, int n,
                    const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len, const void* lut_dev, void* out, int64_t out_bytes);

/* VaeImageProcessor.postprocess(do_denormalize): (x/2 + 0.5).clamp(0,1), NHWC(ldx) -> NCHW (:282-284)  */
int dm4d_postprocess_images_bf16(void* stream, const void* X, void* Y, int B, int C, int HW, int ldx);

/* Fused feed-forward of a transformer block (attention.py:129-149 `ff(norm3(x)) + x`; diffusers FeedForward with GEGLU:
 * Linear(C -> 2 hidden) -> hidden * gelu(gate) -> Linear(hidden -> C)) in ONE launch:
 *     Out[M, C] = residual + W2 (h * gelu(g)) + b2,   [h | g] = W1 Y' + b1,   Y' = LayerNorm(Y) when ln_gamma / ln_beta are given
 *     (norm3 folded in: Y is then the block's residual stream itself), Y' = Y when both are NULL.
 * The [M, hidden] intermediate stays on the chip.  Same products in the same order, same rounding points (the hidden tensor is
 * rounded to bf16 between the two products) as dm4d_gemm_bf16(GEGLU) followed by dm4d_gemm_bf16(residual): bit-identical.
 * dm4d_ff_geglu_supported(C, hidden) says whether the kernel is built for the shape (C = 320: level 0 of an SD-class UNet);
 * dm4d_ff_geglu_prepare_bf16 makes the per-step packed weight copies once per layer from the checkpoint's tensors:
 *   W1 [2 hidden, C] (rows 0..hidden-1 = hidden half, then the gate half), b1 [2 hidden] or NULL, W2 [C, hidden]
 *   -> W1p [2 hidden * C], b1p [2 hidden], W2p [C * hidden] (caller-owned, bf16).                                         */
int dm4d_ff_geglu_supported(int C, int hidden);
int dm4d_ff_geglu_prepare_bf16(void* stream, const void* W1, const void* b1, const void* W2, void* W1p, void* b1p, void* W2p,
                               int C, int hidden);
int dm4d_ff_geglu_fused_bf16(void* stream, const void* Y, int64_t ldy, const void* ln_gamma, const void* ln_beta, float ln_eps,
                             const void* W1p, const void* b1p, const void* W2p, const void* b2, const void* residual,
                             int64_t ld_res, void* Out, int64_t ldo, int M, int C, int hidden);
/* The same launch with the attention output projection in front of it -- the whole tail of a transformer block
 * (attention.py:88-90: attn1.to_out + residual; :129-149: ff(norm3(h)) + h):
 *     h = A0 Wo^T + bo + X          (A0 [M, C] = the attention output, Wo [C, C] row-major, bo [C] or NULL, X [M, C] = the block's input)
 *     Out = h + W2 (u * gelu(g)) + b2,   [u | g] = W1 LayerNorm(h) + b1
 * h is rounded to bf16 once, exactly as dm4d_gemm_bf16(A0, Wo, bias, residual) leaves it.  Since round 6 it never leaves the registers:
 * LayerNorm is taken from the accumulators it was formed in, and its bf16 values start the accumulators of the second product
 * (Out = (h + b2) + W2 (...)), so nothing of h is stored or re-read.  Same products and rounding points as that GEMM followed by
 * dm4d_ff_geglu_fused_bf16 with LayerNorm; fp32 additions in another order (isolated one-ulp differences of a bf16 rounding; rounds
 * 3-5 kept h in Out between the two halves of the launch and were bit-identical).  Out may not alias A0 or X.                      */
int dm4d_attn_out_ff_geglu_fused_bf16(void* stream, const void* A0, int64_t lda0, const void* Wo, const void* bo, const void* X,
                                      int64_t ldx, const void* ln_gamma, const void* ln_beta, float ln_eps, const void* W1p,
                                      const void* b1p, const void* W2p, const void* b2, void* Out, int64_t ldo, int M, int C,
                                      int hidden);

/* proj_in + norm1 + QKV projection of a level-0 transformer (C = 320) in one launch (transformer_multiview.py:160 proj_in;
 * attention.py:73-78 norm1 and attn1's to_q / to_k / to_v; the block tail above covers attention.py:88-90, :129-149, and
 * transformer_multiview.py:209 proj_out stays a dm4d_gemm_bf16 call):
 *     H = N Wpi^T + bpi             (N [M, C] = the transformer's GroupNorm output, Wpi [C, C] row-major, bpi [C] or NULL)
 *     QKV = LayerNorm(H) Wqkv^T     (Wqkv [3 C, C] row-major, bias-free; QKV [M, 3 C] with row stride ldq)
 * H is rounded to bf16 once in the registers and stored: bit-identical to dm4d_gemm_bf16(N, Wpi, bias).  norm1 is taken from those
 * values in the accumulators and never stored, unless n1_out is given (the operator trace: LayerNorm(H) as rounded to bf16, [M, C]).
 * Same products, k order and rounding points as dm4d_gemm_bf16, dm4d_layernorm_bf16, dm4d_gemm_bf16; the fp32 row sums of the
 * LayerNorm are added in another order (at most isolated one-ulp differences of a bf16 rounding in QKV).  The outputs may not alias
 * the input or each other.  dm4d_l0_linear_fused_supported(C) says whether the kernel is built for the channel count (C = 320).   */
int dm4d_l0_linear_fused_supported(int C);
int dm4d_proj_in_ln_qkv_fused_bf16(void* stream, const void* N, int64_t ldn, const void* Wpi, const void* bpi, const void* ln_gamma,
                                   const void* ln_beta, float ln_eps, const void* Wqkv, void* H, int64_t ldh, void* QKV, int64_t ldq,
                                   void* n1_out, int64_t ldn1, int M, int C);

/* ---- Parity precision -------------------------------------------------------------------------------------------------------
 * north_star (BASELINE.json) asks for decoded RGB within 1e-3 rel-L2 of the reference's fp32 CPU path
 * (pipeline_diffuman4d.py:439-559 run with fp32 modules).  bf16 MFMA operands alone cost 7e-3 on the judged UNet call, so the
 * pipeline has a second arithmetic, selected per model object (host: precision="parity"): tensors BETWEEN kernels are fp32 and every
 * activation that feeds the matrix unit is a TWO-TERM bf16 OPERAND  [hi(C) | lo(C)],  hi = bf16(x), lo = bf16(x - hi)  (16 mantissa
 * bits), multiplied against the checkpoint's bf16 weights duplicated along K:  x W^T = [hi | lo] [W | W]^T  -- the same GEMM /
 * convolution kernels with DM4D_EPI_F32OUT / F32SIDE / SPLITOUT.  The entries below produce and consume those operands.        */

/* fp32 -> operand.  Y[m, :] = planes of act(X[m, :]) * scale over Cp >= C1 + C2 columns (columns behind C1 + C2 are zero):
 *   pattern 0: [hi | lo] (ldy >= 2 Cp)   1: [hi | lo | hi]   2: [hi | hi | lo] (ldy >= 3 Cp; the three-term product of two
 *   activations, A in pattern 1 against B in pattern 2 = hi hi + lo hi + hi lo: VAE mid-block attention).
 *   X1 element (m, c) at X1[m * row_stride1 + c * col_stride1] (a transposed read when col_stride1 != 1); X2 (optional second
 *   source = channel concat of the up-block skip, unet_multiview_blocks.py:667) at X2[m * row_stride2 + c].  act_silu: SiLU first. */
int dm4d_split_f32(void* stream, const float* X1, int64_t row_stride1, int64_t col_stride1, int C1, const float* X2,
                   int64_t row_stride2, int C2, void* Y, int64_t ldy, int64_t M, int Cp, int act_silu, float scale, int pattern);

/* GroupNorm (+SiLU) as dm4d_groupnorm_nhwc_bf16, fp32 NHWC in (X2 optional), operand out: Y [B*HW, 2 (C1 + C2)].
 *   Statistics are summed in fp64; ws: dm4d_groupnorm_f32_ws_bytes(B, HW, groups) bytes.                                          */
size_t dm4d_groupnorm_f32_ws_bytes(int B, int HW, int groups);
int dm4d_groupnorm_nhwc_f32_split(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups,
                                  float eps, const void* gamma, const void* beta, void* Y, int apply_silu, void* ws);

/* LayerNorm as dm4d_layernorm_bf16, fp32 in, operand out: Y [M, ldy >= 2 C].                                                      */
int dm4d_layernorm_f32_split(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y, int64_t ldy,
                             int M, int C, float eps);

/* P = softmax(S * scale) per row of fp32 logits -> three planes [p_hi | p_lo | p_hi], each Np >= N columns wide (columns N .. Np-1
 *   zero: a key axis padded to the GEMM's K granularity), ldp >= 3 Np.                                                           */
int dm4d_softmax_rows_f32_split(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N, int Np, float scale);

/* dm4d_attention_kv_bf16 on two-term Q / K / V: the hi plane at the pointer, the lo plane `*_lo` ELEMENTS behind it (the planes
 *   dm4d_gemm_bf16(DM4D_EPI_SPLITOUT) leaves for a fused QKV projection).  S = Kh Qh + Kh Ql + Kl Qh, fp32 running-max softmax,
 *   O = Vh Ph + Vl Ph + Vh Pl; O is written as an operand (hi plane at O, lo plane o_lo elements behind it).  head_dim 64.          */
int dm4d_attention_split_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                              int64_t ldv, int64_t ldo, int64_t q_lo, int64_t k_lo, int64_t v_lo, int64_t o_lo, int batch,
                              int heads, int Lq, int Lk, float scale);

/* fp32-tensor forms of the small kernels around the UNet / VAE calls (same arithmetic, no rounding on the way out):
 *   dm4d_pack_model_input_f32_split writes the operand of conv_in, rows [hi(cpad) | lo(cpad)].                                    */
int dm4d_timestep_embedding_f32(void* stream, const float* t, float* out, int B, int dim, int flip_sin_to_cos, float freq_shift);
int dm4d_pack_model_input_f32_split(void* stream, float* latents, const float* pv_lat, const float* plucker, const float* skel,
                                    const float* mask, const int32_t* is_cond, const int32_t* frame_idx, void* out, int F, int HW,
                                    int cpad, int use_cfg);
int dm4d_cfg_ddim_step_f32(void* stream, float* latents, const float* noise_pred, int64_t ldn, const float* coef,
                           const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg, float guidance_scale,
                           int v_prediction);
int dm4d_cfg_linear_step_f32(void* stream, float* latents, float* x0_prev, const float* noise_pred, int64_t ldn, const float* coef,
                             const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg, float guidance_scale);
int dm4d_cfg_multistep_step_f32(void* stream, float* latents, float* s1, float* s2, float* s3, const float* noise_pred, int64_t ldn,
                                const float* coef, const int32_t* is_cond, const int32_t* frame_idx, int F, int HW, int use_cfg,
                                float guidance_scale);
int dm4d_vae_sample_f32(void* stream, const float* moments, int64_t ldm, const float* noise, float* out, int64_t M, int C, float scale);
int dm4d_resize_nchw_f32_to_nhwc_f32(void* stream, const float* X, float* Y, int B, int C, int H, int W, int h, int w, int bilinear);
int dm4d_plucker_latent_f32(void* stream, const float* cams, float* Y, int N, int H, int W, int h, int w);
int dm4d_postprocess_images_f32(void* stream, const float* X, float* Y, int B, int C, int HW, int ldx);
int dm4d_nhwc_to_nchw_f32(void* stream, const float* X, float* Y, int B, int C, int HW, int ldx);

/* ---- fp16 precision ---------------------------------------------------------------------------------------------------------
 * The arithmetic that meets north_star's 1e-3 on decoded RGB at ONE MFMA per product (host: precision="fp16"; round 5).  Measured on
 * the judged UNet call (tools/error_budget.py): rounding every MFMA operand to bf16 costs 7.0e-3, rounding it to IEEE fp16 (three more
 * mantissa bits) 8.5e-4.  So tensors BETWEEN kernels are fp32 as in the parity precision, and every activation that feeds the matrix
 * unit is rounded ONCE to fp16 by the kernel that produces it (GroupNorm / LayerNorm / GEGLU / the QKV projection / attention), against
 * the checkpoint's weights held in fp16 (a bf16 or fp16 checkpoint's weights are exact in fp16 -- except bf16 values below 2^-14, which
 * keep an absolute error below 2^-25).  It is also the faithful form of the reference's torch_dtype "fp16"
 * (sampling_utils.py:27-29), with fp32 instead of fp16 storage between operators.  Same tile geometries and K order as the fast
 * precision; same MFMA rate (v_mfma_f32_32x32x16_f16).                                                                            */

/* dm4d_gemm_bf16 with fp16 A / A2 / W / bias.  flags: DM4D_EPI_GEGLU, DM4D_EPI_SILU, DM4D_EPI_F32OUT (C is float*), DM4D_EPI_F32SIDE
 *   (rowbias / residual are float*, else fp16).  Without F32OUT C is fp16 [M, ldc]: the operand of the next contraction.
 *   scale_cols / col_scale: output columns [0, scale_cols) (a multiple of 8) are multiplied by col_scale in fp32 before the one
 *   rounding -- the to_q third of a fused QKV projection takes scale * log2(e) this way (attention.py:73-78), so that the attention
 *   kernel needs no per-score multiply and Q is still rounded once.                                                               */
int dm4d_gemm_f16(void* stream, const void* A, int64_t lda, const void* A2, int64_t lda2, int K1, const void* W, int64_t ldw,
                  void* C, int64_t ldc, int M, int N, int K, const void* bias, const void* rowbias, int64_t ld_rowbias,
                  int rows_per_rowbias, const void* residual, int64_t ld_res, unsigned flags, float out_scale, int scale_cols,
                  float col_scale);

/* dm4d_conv3x3_nhwc_bf16_ws with fp16 X / Wt / bias; flags: DM4D_EPI_F32OUT, DM4D_EPI_F32SIDE.  ws as for the bf16 entry
 *   (dm4d_conv3x3_ws_bytes; NULL runs the un-split kernels).                                                                      */
int dm4d_conv3x3_nhwc_f16(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wt, void* Y, int Ho, int Wo,
                          int Cout, int stride, int pad, int upsample, const void* bias, const void* rowbias, int64_t ld_rowbias,
                          const void* residual, int64_t ld_res, float out_scale, unsigned flags, void* ws, size_t ws_bytes);

/* dm4d_conv_up2x_prepare_bf16 / dm4d_conv_up2x_nhwc_bf16 (Upsample2D as four 2x2 phase convolutions) with fp16 weights and input: the
 *   phase kernels are sums of up to four taps taken in fp32 and rounded ONCE to fp16 (relative 2^-12 per weight; the model-level effect is
 *   inside the precision's budget, tests/modelcheck.py fp16_unet_sd21_*).  flags: DM4D_EPI_F32OUT (Y is float*), else Y is fp16.          */
int dm4d_conv_up2x_prepare_f16(void* stream, const void* W, void* Wp, int Cout, int Cin);
int dm4d_conv_up2x_nhwc_f16(void* stream, const void* X, int B, int H, int W, int Cin, const void* Wp, void* Y, int Cout,
                            const void* bias, unsigned flags);

/* fp32 -> fp16 operand: Y[m, :Cp] = fp16(act(X[m, :]) * scale), columns behind C1 + C2 zero (dm4d_split_f32's addressing: second
 *   source = the up-block channel concat, col_stride1 != 1 = a transposed read).                                                  */
int dm4d_to_f16_f32(void* stream, const float* X1, int64_t row_stride1, int64_t col_stride1, int C1, const float* X2,
                    int64_t row_stride2, int C2, void* Y, int64_t ldy, int64_t M, int Cp, int act_silu, float scale);

/* GroupNorm (+SiLU) / LayerNorm / row softmax with fp32 input and ONE fp16 plane out (gamma, beta fp16): Y [B*HW, C1 + C2] /
 *   Y [M, ldy >= C] / P [M, ldp >= Np] (columns N .. Np-1 zero).  GroupNorm statistics: fp32 shifted sums (the fast precision's) on the
 *   vectorised path (channel counts that are multiples of 8; ws = float[B][chunks][groups][2]), fp64 only in the `_general` fall-back kernels;
 *   dm4d_groupnorm_f32_ws_bytes is an upper bound for both.  fp16 outputs saturate at +-65504 (they never become inf).              */
int dm4d_groupnorm_nhwc_f32_f16(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups, float eps,
                                const void* gamma, const void* beta, void* Y, int apply_silu, void* ws);
/* ... and the same GroupNorm with a SECOND output Yraw [B*HW, C1 + C2] = fp16 of the un-normalised input (the channel concat of X1 | X2):
 *   the operand of a resnet's 1x1 shortcut convolution, which reads the tensor its first GroupNorm reads (unet_multiview_blocks.py:667 +
 *   ResnetBlock2D.conv_shortcut), without a pass of its own over the fp32 tensor.  C1, C2 multiples of 8, 16-byte aligned tensors.  */
int dm4d_groupnorm_nhwc_f32_f16_raw(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups, float eps,
                                    const void* gamma, const void* beta, void* Y, void* Yraw, int apply_silu, void* ws);
/* ... and with an fp16 INPUT (one or two sources): the activation a convolution already left in fp16 -- conv1 of a resnet, whose only
 *   reader is norm2 (resnet.py ResnetBlock2D.forward: conv1 -> + temb -> norm2) -- read at two bytes per element.  ws as above.    */
int dm4d_groupnorm_nhwc_f16_f16(void* stream, const void* X1, int C1, const void* X2, int C2, int B, int HW, int groups, float eps,
                                const void* gamma, const void* beta, void* Y, int apply_silu, void* ws);
int dm4d_layernorm_f32_f16(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y, int64_t ldy, int M,
                           int C, float eps);
int dm4d_softmax_rows_f32_f16(void* stream, const float* S, int64_t lds, void* P, int64_t ldp, int M, int N, int Np, float scale);
/* The two entries above take any channel count / alignment: shapes that are not 16-byte vectors of eight channels are forwarded to these
 *   general kernels (fp64 GroupNorm statistics, one or four channels per thread; one wave per LayerNorm row), same arguments.           */
int dm4d_groupnorm_f32_f16_general(void* stream, const float* X1, int C1, const float* X2, int C2, int B, int HW, int groups, float eps,
                                   const void* gamma, const void* beta, void* Y, int apply_silu, void* ws);
int dm4d_layernorm_f32_f16_general(void* stream, const float* X, int64_t ldx, const void* gamma, const void* beta, void* Y, int64_t ldy,
                                   int M, int C, float eps);

/* dm4d_attention_qscaled_kv_bf16 on fp16 Q (carrying scale * log2 e) / K / V -> fp16 O: the same optimistic-softmax loop with
 *   v_mfma_f32_32x32x16_f16; probabilities are kept below 65504 by an offset of 2^-8 on the first tile's maximum and a row-sum check
 *   at 2^16 (attention.hip, "H16").  replaces F.scaled_dot_product_attention via attention.py:73-78.                                */
int dm4d_attention_qscaled_kv_f16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                                  int64_t ldv, int64_t ldo, int batch, int heads, int Lq, int Lk);

/* Head dimensions 40, 80 and 160 (the SD-1.x UNet layout: attention_head_dim = 8 heads over 320 / 640 / 1280 channels; reference
 *   unet_multiview_condition.py:184 and :222-228, attention.py:73-78).  Same contracts as the head_dim 64 entries they stand beside;
 *   head_dim 64 is refused here (it has its own entries: dm4d_attention_qscaled_kv_bf16 / _f16, dm4d_attention_split_bf16).
 *   Q / K / V / O are [batch * L, >= heads * head_dim] row-strided views (strides multiples of 8 elements, e.g. column slices of the
 *   fused [M, 3 C] QKV output); the kernels read and write exactly the head's head_dim columns.  Exact running-max softmax per row, so
 *   results do not depend on how query rows are grouped into workgroups (attention_hd.hip).
 *   dm4d_attention_hd_qscaled_kv_bf16: as dm4d_attention_qscaled_kv_bf16 (Q carries scale * log2 e, softmax in base 2).
 *   dm4d_attention_hd_qscaled_kv_f16:  as dm4d_attention_qscaled_kv_f16 (fp16 operands, fp16 O).
 *   dm4d_attention_hd_split_bf16:      as dm4d_attention_split_bf16 (two-term operands, parity precision), head_dim last.          */
int dm4d_attention_hd_qscaled_kv_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                                      int64_t ldv, int64_t ldo, int batch, int heads, int head_dim, int Lq, int Lk);
int dm4d_attention_hd_qscaled_kv_f16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                                     int64_t ldv, int64_t ldo, int batch, int heads, int head_dim, int Lq, int Lk);
int dm4d_attention_hd_split_bf16(void* stream, const void* Q, const void* K, const void* V, void* O, int64_t ldq, int64_t ldk,
                                 int64_t ldv, int64_t ldo, int64_t q_lo, int64_t k_lo, int64_t v_lo, int64_t o_lo, int batch,
                                 int heads, int Lq, int Lk, float scale, int head_dim);

/* The tail of a transformer block in one launch, precision "fp16" (dm4d_attn_out_ff_geglu_fused_bf16 above; attention.py:88-90 and
 *   :129-149): A0 [M, C] fp16 attention output, Wo / bo / LayerNorm vectors / b2 fp16, W1p / b1p / W2p = dm4d_ff_geglu_prepare_bf16 of
 *   the fp16 matrices (a permutation of 16-bit words), X [M, C] the fp32 residual stream (ldx in floats, a multiple of 4):
 *       h = A0 Wo^T + bo + X  (fp32, never rounded and never stored: it stays in the accumulators it was formed in),
 *       Out = h + W2 (u * gelu(g)) + b2,  [u | g] = W1 fp16(LayerNorm(h)) + b1,
 *   Out fp32 (out_f32 = 1) or rounded once to fp16 (out_f32 = 0: the operand of the transformer's proj_out).  Same products and
 *   rounding points as dm4d_gemm_f16 (fp32 out + residual), dm4d_layernorm_f32_f16, dm4d_gemm_f16 (GEGLU), dm4d_gemm_f16 (+ fp32
 *   residual); only the ORDER of fp32 additions differs (h enters the output sum first, the LayerNorm row sums are added up in another
 *   order), so the two forms agree to fp32 rounding, not bit for bit (tests/opcheck.py h16_ff_proj_fused_*).  C = 320 only
 *   (dm4d_ff_geglu_supported).  Out may not alias A0 or X.                                                                           */
int dm4d_attn_out_ff_geglu_fused_f16(void* stream, const void* A0, int64_t lda0, const void* Wo, const void* bo, const float* X,
                                     int64_t ldx, const void* ln_gamma, const void* ln_beta, float ln_eps, const void* W1p,
                                     const void* b1p, const void* W2p, const void* b2, void* Out, int64_t ldo, int out_f32, int M, int C,
                                     int hidden);

/* dm4d_pack_model_input_f32_split with ONE fp16 plane out: rows of cpad fp16 channels (the operand of conv_in).                    */
int dm4d_pack_model_input_f32_f16(void* stream, float* latents, const float* pv_lat, const float* plucker, const float* skel,
                                  const float* mask, const int32_t* is_cond, const int32_t* frame_idx, void* out, int F, int HW,
                                  int cpad, int use_cfg);

/* Model-input assembly for a SUBSET of a window's frames (the per-sweep prefix cache of host/pipeline.py): as dm4d_pack_model_input_*,
 *   but frame f is written to row out_row[f] of a compact result [cfg*Fo, HW, ...] = [negative half (Fo) | positive half (Fo)], and a
 *   frame whose out_row is negative is not written at all.  out_row: int32 [F] on the device, its non-negative entries a permutation
 *   of 0 .. Fo-1 (1 <= Fo <= F).  The aliasing side effect latents[cond rows] <- image latents covers EVERY conditioning frame of
 *   the window, written or not.                                                                                                      */
int dm4d_pack_model_input_rows_bf16(void* stream, void* latents, const void* pv_lat, const void* plucker, const void* skel,
                                    const void* mask, const int32_t* is_cond, const int32_t* frame_idx, const int32_t* out_row,
                                    void* out, int F, int Fo, int HW, int cpad, int use_cfg);
int dm4d_pack_model_input_rows_f32_split(void* stream, float* latents, const float* pv_lat, const float* plucker, const float* skel,
                                         const float* mask, const int32_t* is_cond, const int32_t* frame_idx,
                                         const int32_t* out_row, void* out, int F, int Fo, int HW, int cpad, int use_cfg);
int dm4d_pack_model_input_rows_f32_f16(void* stream, float* latents, const float* pv_lat, const float* plucker, const float* skel,
                                       const float* mask, const int32_t* is_cond, const int32_t* frame_idx, const int32_t* out_row,
                                       void* out, int F, int Fo, int HW, int cpad, int use_cfg);

/* Row mover: one launch copies whole rows for a small table of jobs, dst[dst_row_idx[r]] = src[src_row_idx[r]] for r < n_rows of
 *   every job, in 16-byte pieces with 64-bit addressing (tensors may exceed 4 GiB).  `jobs` is a HOST array of n_jobs <=
 *   DM4D_ROWS_MOVE_MAX_JOBS entries (it travels in the kernel arguments); src, dst and the int32 index tables are device pointers, src
 *   and dst 16-byte aligned, row_bytes a positive multiple of 16; a job with n_rows = 0 is skipped and its pointers are not looked at.
 *   Rows are dense: row i of a tensor starts at byte i * row_bytes.  The caller vouches for the indices (they are not read on the host)
 *   and for dst rows that are written once per launch; a src row may be read by several.                                              */
#define DM4D_ROWS_MOVE_MAX_JOBS 16
typedef struct {
  const void* src;
  void* dst;
  const int32_t* src_row_idx;
  const int32_t* dst_row_idx;
  int64_t n_rows;
  int64_t row_bytes;
} Dm4dRowsMoveJob;
int dm4d_rows_move(void* stream, const Dm4dRowsMoveJob* jobs, int n_jobs);

/* The GroupNorm statistics of a sample are summed over chunks of its pixels, and the number of chunks follows the batch of the launch
 *   (more samples, fewer chunks each), so a sample's fp32 sums round differently in a batch of another size.  A caller that runs SOME
 *   rows of a batch on their own and needs the bits they have inside the whole batch (the prefix cache's compact head runs) names that
 *   batch here: until it is reset with 0, every GroupNorm launch of THIS THREAD with fewer than B samples plans its chunks as for B.
 *   The workspace sizes of dm4d_groupnorm_ws_bytes / _f32_ws_bytes for the launch's own batch still suffice (fewer chunks).           */
int dm4d_groupnorm_plan_batch(int B);

/* Tuning hook (not part of the operator surface): force one GEMM/conv kernel configuration id for all
 * subsequent launches of this process; 0 restores the built-in heuristic.  Used by tools/gemm_tune.py. */
int dm4d_tune_set_gemm_config(int id);
/* Tuning hook: 0 forces the two-launch GroupNorm (statistics, apply) for every shape; 1 (default) lets maps that fit
 * in registers take the single-launch kernel.  Used by tests/opcheck.py and tests/opbench.py for the A/B.            */
int dm4d_tune_set_groupnorm_resident(int on);

/* layout converters at the pipeline boundary (NCHW <-> NHWC, any C) */
int dm4d_nchw_to_nhwc_bf16(void* stream, const void* X, void* Y, int B, int C, int HW, int cpad);
int dm4d_nhwc_to_nchw_bf16(void* stream, const void* X, void* Y, int B, int C, int HW, int ldx);

#ifdef __cplusplus
}
#endif
#endif /* DM4D_H */
