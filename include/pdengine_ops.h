/* pdengine_ops.h -- per-operator parity hooks of libpdengine.so (test surface, not the product path).
 *
 * Each hook runs exactly one kernel family of the hot path on host fp32 arrays in the reference's
 * layouts, in the engine's precision mode, so tests/ can compare it with the oracle:
 *   pd_op_conv2d     nn.Conv2d 3x3/1x1 (stride 1/2, fused nearest-x2 upsample)   openaimodel.py:90-159,200-240
 *   pd_op_conv2d_upfold  Upsample's conv3x3(nearest_x2(x)) through the weight fold and the four-phase kernel   openaimodel.py:115-117
 *   pd_op_linear     nn.Linear / GEGLU / SiLU->Linear (emb_layers)                 attention.py:49-76, openaimodel.py:217-223
 *   pd_op_linear_ex / pd_op_conv2d_ex  the same launches with every epilogue and addressing form the networks pass (pd_gemm_ex_args)
 *   pd_op_linear_fp8 the e4m3 form of nn.Linear used by the SD3 path's sd3_fp8 option
 *   pd_op_groupnorm  GroupNorm32 (+SiLU)                                           util.py:217-219, attention.py:88-89
 *   pd_op_layernorm  nn.LayerNorm                                                  attention.py:263-265
 *   pd_op_groupnorm_slabs / pd_op_groupnorm_coef  the derived forms of GroupNorm32 (split-K slab input; {scale, shift} coefficients)
 *   pd_op_ln_linear  nn.LayerNorm -> nn.Linear as a kernel pair and as the folded GEMM   attention.py:271-275
 *   pd_op_attention  softmax(q k^T dh^-0.5) v, heads from the engine config        attention.py:171-193
 *   pd_op_attention_ex  the same kernels with heads, causal mask, scale, relative-position bias, strided q | k rows and padding fills
 *   pd_op_vae_attention  the first stage's single-head attention (flash / materialised)   ldm/modules/diffusionmodules/model.py:171-202
 *   pd_op_spatial_transformer  one SpatialTransformer block of the loaded networks  attention.py:271-275,321-340
 *   pd_op_time_embed timestep_embedding + the time_embed MLP of a loaded network    util.py:154-174, openaimodel.py:526-531
 *   pd_op_vae_downsample  the KL-VAE encoder's Downsample (asymmetric pad)          ldm/modules/diffusionmodules/model.py:68-88
 *   pd_op_canny_hysteresis  the flood of cv2.Canny's hysteresis on a given state map  annotator/canny/__init__.py
 *   pd_op_sd3_update  the update kernel of the SD3 img2img / inpainting / seeded loops (start state, CFG + Euler, blend)
 *   pd_op_ip_attention_add  IP-Adapter's image term, att + s softmax(q K_ip^T) V_ip (ip_attention.hip)
 *   pd_op_spatial_transformer_ip  one SpatialTransformer block of the UNet with that term
 *   pd_op_pag_identity  perturbed-attention guidance's identity attention: the transposition of V^T into token rows (pag.hip)
 *   pd_op_cfg_combine   the guidance of the update kernel alone: CFG and the perturbed-attention term (sampler_update.hip)
 *   pd_op_spatial_transformer_pag  one SpatialTransformer block with its last samples perturbed
 */
#ifndef PDENGINE_OPS_H
#define PDENGINE_OPS_H
#include "pdengine.h"
#ifdef __cplusplus
extern "C" {
#endif
int pd_op_conv2d(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, int B, int Cin, int H,
                 int W, int Cout, int k, int stride, int upsample, int act_silu, float scale, int stream_out, float* y);
/* conv3x3(nearest_x2(x)) + bias [+ residual] with ad-hoc weights through the decoder Upsample's own call path: the weights are folded
 * into the four phase matrices (option "ups_fold") and the call goes through the engine's dispatch, which must put it on the four-phase
 * kernel (PD_GEMM_UPFOLD; option "ups_fold_tiles" is the grid threshold).  A call the dispatch would send elsewhere -- a source height
 * or width that is no multiple of 16, a residual, an fp32-storage mode, the option off, too small a grid -- is an error, not a
 * fall-back.  x [B, Cin, H, W], w [Cout, Cin, 3, 3], y [B, Cout, 2H, 2W]. */
int pd_op_conv2d_upfold(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, int B, int Cin, int H,
                        int W, int Cout, float* y);
int pd_op_linear(pd_engine* e, const float* x, const float* w, const float* bias, int M, int K, int N, int geglu, int a_silu,
                 float* y);
/* pd_engine::gemm on a linear layer in every form its callers launch; pd_op_linear is this call with everything else at 0 / NULL.
 * Host fp32 arrays in and out; the call goes through check_gemm / fill_gemm / plan_gemm / gemm() like a network's, so the options
 * ("gemm_tile", "gemm_splitk", "ring", "ring_tile", ...) decide the kernel and the stats "gemm_family" / "gemm_tile" / "gemm_splitk" say
 * which one ran.  A combination the kernels refuse or would ignore is an error, not a fall-back.
 *   x [M][K], w [N][K] (act 2 / 7: [2N][K] packed [x | gate], bias [2N]), bias [N] or NULL; K a multiple of 8
 *   act       Activation of pd_common.h: 0 none, 1 SiLU, 2 GEGLU, 3 quick-GELU, 4 tanh-GELU, 5 ReLU, 6 erf-GELU, 7 gated tanh-GELU
 *   a_silu    SiLU on x while it is loaded (x then stays fp32 on the device)
 *   scale     0: 1
 *   dtype codes (res_dt, out_dt): 0 fp32, 1 the compute type T, 2 the residual-stream type S
 *   residual  [M][N] or NULL, held in res_dt with row stride N; added after scale and gate, read at the call's own row m
 *   rows_per_sample  tokens per sample (0: M, one sample); M = B x tokens
 *   rowvec, gate     [B][N] or NULL: added before the activation / multiplied in after scale
 *   vt_begin  0: none; else a multiple of 4: the columns >= vt_begin go transposed to vt [B][N - vt_begin][tokens] instead of y.  The
 *             device V^T rows are round_up(vt_tok_off + tokens, 8) + vt_extra long and token t lands at vt_tok_off + t.
 *   c_sample_rows / c_row_off   0 / 0: row m of C; else row m = (b, t) lands at b * c_sample_rows + c_row_off + t of a joint buffer
 *   a_sample_rows / a_row_off   the same for the rows of A: the hook scatters x into a joint buffer whose other rows hold NaN
 *   ldc_extra  the output row stride is N + ldc_extra (a multiple of 4)
 *   ln_gamma, ln_beta  [K] or NULL: LayerNorm(x) folded into the layer as pd_op_ln_linear's mode 1 does (x then lives in S; K <= 2048)
 * Before the launch every output buffer is filled with NaN: C with the other stream's rows, its pad columns and the columns >= vt_begin,
 * V^T with the pad tokens and the other stream's.  y [M][N] (its columns >= vt_begin come back as the NaN fill of C) and vt receive the call's
 * own elements; `touched` the number of elements outside them whose bytes the launch changed. */
typedef struct pd_gemm_ex_args {
    const float *x, *w, *bias, *residual, *rowvec, *gate, *ln_gamma, *ln_beta;
    int32_t M, K, N, act, a_silu, res_dt, out_dt, rows_per_sample;
    int32_t vt_begin, vt_extra, vt_tok_off, c_sample_rows, c_row_off, a_sample_rows, a_row_off, ldc_extra;
    float scale;
    float *y, *vt;
    int64_t touched;
} pd_gemm_ex_args;
int pd_op_linear_ex(pd_engine* e, pd_gemm_ex_args* a);
/* pd_op_conv2d plus the per-sample row of a ResBlock's time embedding (rowvec [B][Cout] or NULL, added before the activation) and
 * act 5 (ReLU; act 0 / 1 as act_silu 0 / 1) -- through the dispatch, so igemm, its split-K finalize pass and the patch generations all
 * take it; the dispatch keeps an activation away from the family that has none (the 4-wave patch conv). */
int pd_op_conv2d_ex(pd_engine* e, const float* x, const float* w, const float* bias, const float* residual, const float* rowvec, int B, int Cin,
                    int H, int W, int Cout, int k, int stride, int upsample, int act, float scale, int stream_out, float* y);
/* the SD3 path's PREC_FP8 linear layer (option sd3_fp8): e4m3 operands quantised on the device with one scale per row of x
 * and of w, block-scaled MFMA, scales applied in the epilogue; act 0 or 4 (tanh-GELU).  2-byte engine modes only. */
int pd_op_linear_fp8(pd_engine* e, const float* x, const float* w, const float* bias, int M, int K, int N, int act, float* y);
int pd_op_groupnorm(pd_engine* e, const float* x, const float* gamma, const float* beta, int B, int C, int H, int W, float eps,
                    int silu, float* y);
int pd_op_layernorm(pd_engine* e, const float* x, const float* gamma, const float* beta, int rows, int C, float* y);
/* GroupNorm32 (+SiLU) of a tensor that exists only as the fp32 partial sums of a split-K GEMM (option "slab_gn"): slabs
 * [nslab][B * H * W][C] (pixel rows, channels last), bias [C] or NULL, row [B][C] (the per-sample time-embedding row) or NULL.  The
 * kernel rebuilds x = round_S(slab_0 + slab_1 + ... + bias + row), summed in fp32 in that order (splitk_finalize_kernel's), S the
 * residual-stream type, and normalises it: bit-identical to pd_op_groupnorm of that x.  Runs launch_gn_fused_slabs (the register kernel
 * or the LDS-slab kernel, stat "gn_kernel"); an error where no single-kernel GroupNorm applies to the shape.  y [B, C, H, W]. */
int pd_op_groupnorm_slabs(pd_engine* e, const float* slabs, int nslab, const float* bias, const float* row, const float* gamma,
                          const float* beta, int B, int C, int H, int W, float eps, int silu, float* y);
/* The coefficient form of GroupNorm32 (gn_stats_kernel + gn_coef_kernel) that the GroupNorm-fused patch conv and the fused
 * SpatialTransformer front apply while staging: x [B, C, H, W] -> coef [B][C][2] = {a, b} with GroupNorm(x)[b, c] = x * a + b. */
int pd_op_groupnorm_coef(pd_engine* e, const float* x, const float* gamma, const float* beta, int B, int C, int H, int W, float eps,
                         float* coef);
/* y [M][N] = Linear(LayerNorm(h)) (eps 1e-5; gamma, beta [K]; w [N][K]; bias [N] or NULL) the three ways a transformer block computes
 * it, through the engine's own gemm(); h [M][K] lives in the residual-stream type, y is written in the compute type.
 *   mode 0: layernorm_kernel, then the GEMM on the normalised rows;
 *   mode 1: the fold -- the GEMM reads h itself against round(w * gamma) and its epilogue applies rstd * (acc - mean * colsum) + bias',
 *           with {sum, sum of squares} of every row from row_stats_kernel;
 *   mode 2: the fold with the statistics left by the producing GEMM's epilogue: h = x [M][K] . w1 [K][K]^T + b1 (+ residual [M][K]) is
 *           computed here (h is ignored; b1, residual may be NULL) and h_out [M][K], when non-NULL, receives h as it was stored -- what
 *           the consumer read.
 * x, w1, b1, residual are ignored in modes 0 / 1.  K a multiple of 8, at most 2048.
 * stats_parts (may be NULL) receives how many {sum, sum of squares} partials per row fed the fold: 0 in mode 0, 1 from row_stats_kernel
 * (mode 1, and mode 2 where the producer ran split-K and left no statistics of its own), the producing tile's wave columns otherwise.
 * row_stats [M][2] (may be NULL; modes 1 / 2) receives those partials summed per row in fp32, in their order, as ln_row_stats does. */
int pd_op_ln_linear(pd_engine* e, int mode, const float* h, const float* x, const float* w1, const float* b1, const float* residual,
                    const float* gamma, const float* beta, const float* w, const float* bias, int M, int K, int N, float* h_out, float* y,
                    int* stats_parts, float* row_stats);
int pd_op_attention(pd_engine* e, const float* q, const float* k, const float* v, int B, int Nq, int Nk, int C, float* o);
/* pd_engine::attention in every form its callers launch; pd_op_attention is this call with everything after C at 0 / NULL.
 * q [B, Nq, C], k, v [B, Nk, C], o [B, Nq, C] host fp32.
 *   heads     0: pd_config.num_heads; dh = C / heads must be one of the built head dims (8, 16, 32, 40, 64, 80, 160)
 *   causal    keys after the query are masked (Nq == Nk)
 *   scale     0: dh^-0.5
 *   relbias   NULL, or the Toeplitz bias rows [heads][2 Nk - 1] in natural-log units: logit(query, key) += relbias[h][key - query + Nk - 1]
 *             (T5); converted to the kernel's exp2 units by the T5 path's own kernel.  dh 64, Nq == Nk, not causal.
 *   layout    0: q and k contiguous (row stride C).  1: one device buffer [B][Nk][2C] holding q | k, as a fused projection leaves them;
 *             the queries are its first Nq <= Nk rows, the row stride of q and k is 2C, their sample stride Nk * 2C, and the output buffer
 *             is [B][Nk][C] with sample stride Nk * C (the MMDiT joint block, and its context_pre_only form where Nq < Nk).
 *   vt_extra  keys of V^T row padding beyond round_up(Nk, 8); a multiple of 8
 *   pad_fill  written (NaN allowed) into every V^T pad column and, in layout 1, into the q half of the rows >= Nq and into the whole
 *             output buffer before the launch
 *   touched   may be NULL; layout 1: the number of elements in the output rows >= Nq whose bytes the launch changed (0 in layout 0)
 * Sets stat "attn_kernel".  A combination the engine does not launch is an error, not a fall-back. */
int pd_op_attention_ex(pd_engine* e, const float* q, const float* k, const float* v, int B, int Nq, int Nk, int C, int heads, int causal,
                       float scale, const float* relbias, int layout, int vt_extra, float pad_fill, float* o, int64_t* touched);
/* softmax(q k^T C^-0.5) v with one head over all C channels -- the first stage's AttnBlock (model.py:171-202) between its projections;
 * q, k, v, o [B, N, C].  Option "vae_flash" 1: the single-head flash kernel (vae_attention.hip; 2-byte modes, C = 128 or 512, any
 * N >= 1 -- another mode or C is an error); 0 / -1: the materialised path (score GEMM, row softmax, value GEMM per sample; every mode,
 * N a multiple of 8). */
int pd_op_vae_attention(pd_engine* e, const float* q, const float* k, const float* v, int B, int N, int C, float* o);
/* SpatialTransformer.forward of the block whose weights were loaded under `prefix` (reference state-dict prefix ending in '.'),
 * x [B, C, H, W], context [B, context_len, context_dim], y [B, C, H, W]; the same code path as a sampling step (2-byte modes at
 * 320 channels: self-attention + the fused tail kernel). */
int pd_op_spatial_transformer(pd_engine* e, const char* prefix, const float* x, const float* context, int B, int H, int W, float* y);
/* ... with a context of any length: context [B, L, context_dim], 1 <= L <= PD_MAX_CONTEXT_LEN.  At 320 channels the fused tail takes
 * L <= 288 (one to three 96-key windows, st_tail.hip); longer contexts take the per-layer path.  pd_op_spatial_transformer is this call
 * with L = pd_config.context_len. */
int pd_op_spatial_transformer_ctx(pd_engine* e, const char* prefix, const float* x, const float* context, int B, int H, int W, int L, float* y);
/* IP-Adapter's image term alone (ip_attn_add_kernel): out = round_T(att + s * softmax(q2 k_ip^T scale) v_ip) per head, every operand
 * rounded to the compute type T first, logits / softmax / the product with v_ip / the multiply by s / the add in fp32.  q2, att, out
 * [B, N, C]; k_ip, v_ip [Bk, T, C] with Bk = B, or 1: one set of keys for every sample; heads 0: pd_config.num_heads; C / heads one of
 * 8, 16, 32, 40, 80, 160; 1 <= T <= 64; C a multiple of 8; scale 0: dh^-0.5. */
int pd_op_ip_attention_add(pd_engine* e, const float* q2, const float* att, const float* k_ip, const float* v_ip, int B, int N, int C, int heads, int T,
                           int Bk, float scale, float s, float* out);
/* launch_pag_identity: out [count, N, C] = vt[src : src + count] transposed, vt [Bs, C, N].  vt is rounded to the engine's storage type
 * and laid out as the QKV GEMM writes V^T (rows of round_up(N, 8), pad columns holding a non-zero fill the kernel must not copy); the
 * kernel is a bit copy, so values that type holds exactly come back exactly. */
int pd_op_pag_identity(pd_engine* e, const float* vt, int Bs, int C, int N, int src, int count, float* out);
/* cfg_update_kernel with do_update = 0, in the form an evaluation with pd_set_pag on launches it (every operation of the guidance rounded
 * on its own; pag_scale 0 is a step at the adaptive scale's clamp -- an engine with the state off keeps the earlier CFG line, whose
 * multiply-add the compiler contracts): out [B, HW, C] = the guided eps of eps [Bt, HW, C], Bt = (use_cfg ? 2 : 1) * B samples
 * [uncond ;] cond and, when pag_scale != 0, B more, the perturbed branch.  eps is converted to eps_dtype (PD_DT_*) on the host first. */
int pd_op_cfg_combine(pd_engine* e, const float* eps, int B, int HW, int C, int eps_dtype, int use_cfg, float cfg_scale, float pag_scale,
                      float* out);
/* pd_op_spatial_transformer_ctx with the last n_perturbed of the B samples perturbed from their own V (PagTerm without a fork): their
 * self-attention is the identity, their cross-attention reads their own context in a launch of its own. */
int pd_op_spatial_transformer_pag(pd_engine* e, const char* prefix, const float* x, const float* context, int B, int H, int W, int L,
                                  int n_perturbed, float* y);
/* pd_op_spatial_transformer_ctx of a UNet block with IP-Adapter's image term (pd_ip_adapter_configure, adapter weights loaded): tokens
 * [B, T, context_dim] go through the block's to_k_ip / to_v_ip and the term enters at the block's current scale (pd_ip_adapter_set_scale),
 * through the code path of a sampling step.  At scale 0 the call is pd_op_spatial_transformer_ctx, fused tail included. */
int pd_op_spatial_transformer_ip(pd_engine* e, const char* prefix, const float* x, const float* context, const float* tokens, int B, int H, int W,
                                 int L, int T, float* y);
/* timestep_embedding(t, model_channels) (util.py:154-174: [cos | sin], max_period 10000, frequencies i / half) -> temb [n][model_channels],
 * and time_embed(temb) = Linear -> SiLU -> Linear of the loaded network (net 0: UNet, 1: ControlNet; openaimodel.py:526-531) -> emb
 * [n][4 * model_channels]; exactly what the sampler computes once per call for all its steps (pd_engine::compute_emb). */
int pd_op_time_embed(pd_engine* e, int net, const int64_t* t, int n, float* temb, float* emb);
/* Host only (no engine, no GPU): the sinusoidal timestep_embedding [n, dim] the engine feeds its time_embed MLP, from integer
 * timesteps and from the fractional model times of a linear multistep loop ((float)t * freqs; the same bits for integers). */
int pd_op_timestep_embedding_i(const int64_t* t, int n, int dim, float* out);
int pd_op_timestep_embedding_f(const double* t, int n, int dim, float* out);
/* Downsample.forward with_conv (model.py:80-88): F.pad(x, (0,1,0,1)) then Conv2d 3x3, stride 2, padding 0; x [B, C, H, W] ->
 * y [B, C, H/2, W/2] (floor), w [C, C, 3, 3], bias [C] or NULL; the implicit-GEMM gather with GemmParams::pad_shift = 1 */
int pd_op_vae_downsample(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, float* y);
/* The FreeU skip concat of a decoder block (freeu_concat_kernel), in the storage type of the residual stream:
 * y = cat([(h + h_add) with channels < C_h / 2 scaled by b, fourier_filter(skip + skip_add, threshold 1, scale s)], dim=1).
 * h, h_add [B, C_h, H, W]; skip [skip_B, C_skip, H, W]; skip_add [skip_add_B, C_skip, H, W]; skip_B, skip_add_B are B or B / 2
 * (read for both halves of the batch); h_add / skip_add may be NULL; y [B, C_h + C_skip, H, W].  C_h, C_skip multiples of 4. */
int pd_op_freeu_concat(pd_engine* e, const float* h, const float* h_add, const float* skip, const float* skip_add, int B, int C_h,
                       int C_skip, int H, int W, int skip_B, int skip_add_B, float s, float b, float* y);
/* The per-stage tail of the HED edge detector (hed_stage_tail_kernel), in the engine's compute type: x [B, C, H, W] ->
 * score [B, H, W] = conv1x1(x, w [C], bias[0]) with fp32 accumulation and, when pooled is non-NULL (H, W even),
 * pooled [B, C, H/2, W/2] = max_pool2d(x, 2, 2).  C a multiple of 8. */
int pd_op_hed_stage_tail(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, float* score,
                         float* pooled);
/* The end of the HED edge detector (hed_fuse_kernel), fp32 in every mode: scores = the five score maps back to back, map i
 * [B, H >> i, W >> i] (H, W multiples of 16); cw [5], cb [1]; what PD_HED_EDGE: out [B, 1, H, W] = sigmoid(cb + sum_i cw[i] up_i),
 * PD_HED_SIDES: out [B, 5, H, W] = up_i, the bilinear upsamples (align_corners = False) to H x W. */
int pd_op_hed_fuse(pd_engine* e, const float* scores, const float* cw, const float* cb, int B, int H, int W, int what, float* out);
/* The hysteresis of the Canny edge detector (canny_hysteresis_kernel and its sweep loop, as pd_canny runs them) on a caller's state
 * map: states [B, H, W] uint8 of PD_CANNY_NONE (0), PD_CANNY_WEAK (1), PD_CANNY_STRONG (2) -- any other value counts as NONE and is
 * passed through -> out [B, H, W], the same map with every weak pixel that is 8-connected, through weak pixels, to a strong one set
 * to PD_CANNY_STRONG.  states and out live in `mem`.  Stat "canny_sweeps" holds the launches it took. */
int pd_op_canny_hysteresis(pd_engine* e, const uint8_t* states, int B, int H, int W, int mem, uint8_t* out);
/* The M-LSD line detector's own kernels (mlsd.hip), one at a time.
 * pd_op_dwconv3x3: depthwise conv3x3 + bias + ReLU6 in the compute type; x [B, C, H, W], w [C, 1, 3, 3], bias [C] -> y [B, C, Ho, Wo].
 *   stride 1: padding 1, Ho = H; stride 2: F.pad(x, (0, 1, 0, 1)) + padding 0, Ho = H / 2 (H, W even).  in_relu6 != 0: the kernel reads
 *   min(max(x, 0), 6) (the ReLU6 of the producing layer, applied while loading).  C a multiple of 8.
 * pd_op_upcat_bilinear: F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) of x [B, C, h, w] into channels
 *   c_off .. c_off + C - 1 of y [B, Cy, 2h, 2w], which is read (in the compute type), written in place and returned: its other channels
 *   must come back as they went in.  C, Cy, c_off multiples of 8.
 * pd_op_conv2d_dilated: nn.Conv2d(Cin, Cout, 3, padding=d, dilation=d) (+ ReLU) through the engine's dispatch, which sends a dilated
 *   conv to the implicit-GEMM gather (GemmParams::dil_m1).
 * pd_op_mlsd_decode: tp [B, 9, h, w] fp32 -> segs int32 [B, 200, 4], count int32 [B]: pred_lines' decode (3x3 NMS of channel 0, the
 *   200 best, score > thr_v and length > thr_d, end points 2 (x + disp) truncated), fp32 in every mode.
 * pd_op_draw_lines: segs int32 [B, n, 4], count [B] -> out uint8 [B, H, W]: cv2.line(thickness 1, LINE_8) of each, 255 on 0. */
int pd_op_dwconv3x3(pd_engine* e, const float* x, const float* w, const float* bias, int B, int C, int H, int W, int stride, int in_relu6,
                    float* y);
int pd_op_upcat_bilinear(pd_engine* e, const float* x, int B, int C, int h, int w, int Cy, int c_off, float* y);
int pd_op_conv2d_dilated(pd_engine* e, const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout, int dilation,
                         int relu, float* y);
int pd_op_mlsd_decode(pd_engine* e, const float* tp, int B, int h, int w, float thr_v, float thr_d, int32_t* segs, int32_t* count);
int pd_op_draw_lines(pd_engine* e, const int32_t* segs, const int32_t* count, int B, int n, int H, int W, uint8_t* out);
/* The assembling kernel of a tiled VAE call (vae_tile_blend_kernel) alone, on a caller's tiles: plan = the rows x cols entries of
 * pd_vae_tile_plan (th, tw, ev, eh, oh, ow are read); tiles = the tiles back to back in plan order, each fp32 [B][th][tw][Cpad] (NHWC, Cpad
 * a multiple of 4).  nchw != 0: out [B][C][H][W] (the decode side, channels >= C dropped); else out [B][H][W][Cpad] (the encode side's
 * moments); H x W is the sum of the kept rectangles.  fp32 in every mode, host arrays. */
int pd_op_vae_tile_blend(pd_engine* e, const float* tiles, const pd_vae_tile* plan, int rows, int cols, int B, int C, int Cpad, int nchw,
                         float* out);
/* One launch of the SD3 loop's update kernel (sd3_update_kernel; arithmetic under pd_sd3_loop_args in pdengine.h) on a caller's
 * tensors, fp32 in `mem`.  v NULL: the start state, x_out = pure ? eps : sigma eps + (1 - sigma) z0 (x is not read).  v set
 * ([2B, C, H, W] = [negative ; positive] with use_cfg, else [B, C, H, W]): x_out = the CFG + Euler update of x [B, C, H, W] by
 * dsigma and, with a mask [B, 1, H, W] (needs z0), its blend with k = (1 - sigma) z0 + sigma eps.  eps [B, C, H, W], or NULL with
 * seeded != 0: drawn from the engine's generator at (PD_RNG_XT, 0).  x_in_out (may be NULL) [2B, C, H, W]: the doubled input
 * of the next step as the kernel stores it (both halves). */
int pd_op_sd3_update(pd_engine* e, const float* v, const float* x, const float* z0, const float* mask, const float* eps, int B, int C,
                     int H, int W, int use_cfg, float guidance, float dsigma, float sigma, int pure, int seeded, int mem, float* x_out,
                     float* x_in_out);
#ifdef __cplusplus
}
#endif
#endif
