/* pdengine.h -- C ABI of the MI355X-native Prompt-Diffusion DDIM sampling engine.
 *
 * This is the drop-in boundary for the reference's hot path: the work the
 * reference does, per denoising step, inside
 *     DDIMSampler.sample / ddim_sampling / p_sample_ddim      cldm/ddim_hacked.py:55-234
 *     ControlLDM.apply_model                                   cldm/cldm.py:369-382
 *     ControlNet.forward / ControlledUnetModel.forward          cldm/cldm.py:302-325, :23-45
 * and, under diffusers naming, inside PromptDiffusionPipeline.__call__'s loop
 *     pipeline_prompt_diffusion.py:1210-1290 + promptdiffusioncontrolnet.py:188-391.
 *
 * Plain C: opaque handle, pointers and sizes only; no torch types.  All tensors that cross
 * the boundary are float32 in the reference's own layouts (NCHW images/latents,
 * [B, L, D] text context).  Every entry point returns 0 on success, non-zero on error and
 * never throws; pd_last_error() returns the thread-local message of the last failure.
 * One engine <-> one GPU <-> one HIP stream; calls on one engine must be serialised by the
 * caller (the reference pipeline is not thread-safe either, pipeline_prompt_diffusion.py:1065).
 */
#ifndef PDENGINE_H
#define PDENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_ABI_VERSION 2

/* arithmetic mode of the engine */
#define PD_PREC_BF16 0 /* bf16 MFMA operands, fp32 accumulate / norm statistics / softmax */
#define PD_PREC_F32 1  /* fp32 MFMA (v_mfma_f32_16x16x4_f32): bit-faithful fp32 arithmetic */
#define PD_PREC_F16 2  /* fp16 MFMA operands (the reference's own GPU dtype, README.md:44-45 torch_dtype=torch.float16;
                          same MFMA rate as bf16, 3 more mantissa bits), fp32 accumulate / norm statistics / softmax */
#define PD_PREC_F16X2 3 /* fp32 storage; every MFMA operand split into fp16 hi + lo in registers, three fp16 MFMAs per
                           8 K-elements (hi*hi + hi*lo + lo*hi): ~22-bit operands, fp32-class results at ~5x the fp32 MFMA rate */

/* where caller-owned I/O buffers live */
#define PD_MEM_HOST 0
#define PD_MEM_DEVICE 1

/* dtype tags for pd_load_weights */
#define PD_DT_F32 0
#define PD_DT_F16 1
#define PD_DT_BF16 2

#define PD_MAX_LEVELS 8
#define PD_NUM_CONTROL 13 /* 12 input blocks + middle, cldm/cldm.py:313-323 */

typedef struct pd_engine pd_engine;

/* Hyper-parameters = models/cldm_v15.yaml:30-62 (ControlNet and UNet share them). */
typedef struct pd_config {
    int32_t in_channels;      /* 4 */
    int32_t out_channels;     /* 4 */
    int32_t hint_channels;    /* 6: example pair, cldm/cldm.py:147 */
    int32_t query_channels;   /* 3: query image, cldm/cldm.py:166 */
    int32_t model_channels;   /* 320 */
    int32_t num_levels;       /* 4 */
    int32_t channel_mult[PD_MAX_LEVELS]; /* 1,2,4,4 */
    int32_t num_res_blocks;   /* 2 */
    int32_t num_attn_res;     /* 3 */
    int32_t attention_resolutions[PD_MAX_LEVELS]; /* 4,2,1 */
    int32_t num_heads;        /* 8 */
    int32_t context_dim;      /* 768 */
    int32_t context_len;      /* 77 */
    int32_t hint_widths[7];   /* 16,16,32,32,96,96,256: cldm/cldm.py:147-163 */
    int32_t timesteps;        /* 1000 */
    double linear_start;      /* 0.00085 (double: the schedule is derived in float64, util.py:22-25) */
    double linear_end;        /* 0.0120 */
    int32_t precision;        /* PD_PREC_* */
    int32_t stream_f32;       /* PD_PREC_BF16 / PD_PREC_F16: keep the residual stream (block outputs) in fp32 */
    /* first-stage KL-VAE decoder (models/cldm_v15.yaml:64-85).  vae_ch = 0: not built */
    int32_t vae_ch;           /* 128 */
    int32_t vae_num_levels;   /* 4 */
    int32_t vae_ch_mult[PD_MAX_LEVELS]; /* 1,2,4,4 */
    int32_t vae_num_res_blocks; /* 2 */
    int32_t vae_out_ch;       /* 3 */
    double scale_factor;      /* 0.18215, cldm_v15.yaml:17 */
    /* cond-stage CLIP text transformer (ldm/modules/encoders/modules.py:88-131).  Width = context_dim,
     * length = context_len.  text_layers = 0: not built */
    int32_t text_vocab;       /* 49408 */
    int32_t text_layers;      /* 12 */
    int32_t text_heads;       /* 12 */
    int32_t text_ff;          /* 3072 */
    /* first-stage KL-VAE encoder (Encoder + quant_conv, ldm/models/autoencoder.py:31-33, 83-87; same vae_* hyper-parameters,
     * double_z, no attention in the levels).  0: not built (the default); needs vae_ch > 0 */
    int32_t vae_encoder;
    int32_t reserved[1];
} pd_config;

/* Arguments of one sampling call (replaces DDIMSampler.sample's arguments,
 * cldm/ddim_hacked.py:55-79, and the loop state of PromptDiffusionPipeline.__call__). */
typedef struct pd_sample_args {
    int32_t batch;            /* B images; the engine runs the CFG-doubled batch 2B when use_cfg */
    int32_t h, w;             /* latent height/width = image/8 */
    int32_t steps;            /* S */
    float eta;                /* ddim eta */
    float cfg_scale;          /* unconditional_guidance_scale / guidance_scale */
    int32_t use_cfg;          /* (L): unconditional_conditioning is not None, ddim_hacked.py:188;
                                 (D): guidance_scale > 1, pipeline_prompt_diffusion.py:878 */
    int32_t guess_mode;       /* (D) :1220-1224,:1248-1253: ControlNet sees the cond half only */
    int32_t only_mid_control; /* cldm/cldm.py:38 */
    float temperature;        /* ddim_hacked.py:230 */
    int32_t mem;              /* PD_MEM_* of every pointer below */
    const float* x_T;         /* [B, in_ch, h, w] initial latents (required unless PD_XT_FROM_SEED) */
    const float* ctx_cond;    /* [B, L, D] */
    const float* ctx_uncond;  /* [B, L, D] (use_cfg) */
    const float* pair;        /* [B, hint_ch, 8h, 8w] example pair */
    const float* query;       /* [B, query_ch, 8h, 8w] query image */
    const float* pair_uncond; /* optional: unconditional example pair (NULL = same as pair) */
    const float* query_uncond;/* optional */
    const float* control_scales;      /* [13] or NULL (= all 1.0), cldm/cldm.py:335,379 */
    const float* control_scales_step; /* optional [steps][13]: per-step scales in sampling order
                                         (controlnet_keep gating, pipeline :1196-1202,:1229-1235) */
    const float* noise;       /* eta > 0: [steps][B, in_ch, h, w] standard normal draws (required then: ddim_hacked.py:230),
                                 or NULL with PD_NOISE_FROM_SEED */
    const int64_t* timesteps; /* optional, HOST memory whatever `mem` says: [steps] custom DDIM timesteps in sampling order
                                 (strictly descending) replacing the uniform grid of make_ddim_timesteps -- the (D) pipeline's
                                 `timesteps=` argument (pipeline_prompt_diffusion.py:101-142) and diffusers' leading-spaced
                                 grid for step counts that do not divide 1000 */
    /* img2img / inpainting (diffusers' semantics for a 4-channel UNet).  With sa(t) = sqrtf(abar[t]), sb(t) = sqrtf(1 - abar[t])
     * from the engine's fp32 table and t_0 .. t_{S-1} the grid in sampling order:
     *   init_latents: x_T is the noise draw eps; the loop starts from sa(t_0) z0 + sb(t_0) eps (from eps itself with
     *     PD_INIT_PURE_NOISE); per_step_out[0] holds the start latents.
     *   mask: after the update of step i the latents become (1 - m) k_i + m x (fp32, in this order, no FMA) before anything
     *     reads them, with k_i = sa(t_{i+1}) z0 + sb(t_{i+1}) eps for i < S - 1 and k_{S-1} = z0; m broadcasts over channels.
     *     Applies in pd_ddim_sample, pd_unipc_sample and pd_sample_step (also after pd_sample_set_latents), never in
     *     pd_sample_eps_at (host-driven schedulers blend on the host). */
    const float* init_latents; /* optional [B, in_ch, h, w] in `mem`: z0 = scale_factor * the init image's latents */
    const float* mask;         /* optional [B, 1, h, w] in `mem`, needs init_latents; weight of the SAMPLED latents (1 = repaint, 0 = keep) */
    int32_t init_flags;        /* PD_INIT_PURE_NOISE: start from x_T itself (diffusers' strength == 1 inpainting);
                                  PD_NOISE_FROM_SEED / PD_XT_FROM_SEED: see "Seeded noise" below */
    int32_t context_len;       /* L of ctx_cond / ctx_uncond, 1 .. PD_MAX_CONTEXT_LEN; 0: pd_config.context_len.  (The text transformer
                                  keeps pd_config.context_len positions: longer contexts are several of its windows side by side.) */
} pd_sample_args;
#define PD_MAX_CONTEXT_LEN 1024   /* sanity bound of pd_sample_args.context_len */
#define PD_INIT_PURE_NOISE 1
#define PD_NOISE_FROM_SEED 2 /* the per-step draws (eta > 0 DDIM, multistep rows with [14] != 0) come from the engine's generator;
                                `noise` must be NULL */
#define PD_XT_FROM_SEED    4 /* x_T must be NULL: the session's start kernel draws it (stream PD_RNG_XT, draw 0); per_step_out[0]
                                reports it; with init_latents it is the img2img noise eps, exactly as a caller's x_T is */

const char* pd_last_error(void);
int pd_abi_version(void);

/* lifecycle (replaces create_model + load_state_dict + .to(device), cldm/model.py:12-28) */
int pd_engine_create(const pd_config* cfg, int device_id, pd_engine** out);
void pd_engine_destroy(pd_engine* e);

/* parameter registry: names/shapes are the reference checkpoint's (model.diffusion_model.*,
 * control_model.*; tool_add_control.py:36-45) */
int pd_param_count(pd_engine* e);
int pd_param_info(pd_engine* e, int index, const char** name, int32_t* ndim, int64_t shape[4]);
/* copy one tensor from HOST memory; the engine repacks it (NHWC taps, bf16, fused QKV). */
int pd_load_weights(pd_engine* e, const char* name, const void* data, const int64_t* shape,
                    int32_t ndim, int32_t dtype);
/* device-side seeded N(0, 1/fan_in)-style initialisation of every tensor (benchmarks only) */
int pd_init_random_weights(pd_engine* e, uint64_t seed);
/* number of UNet + ControlNet tensors not loaded yet (0 = ready to sample); the VAE decoder is counted separately */
int pd_weights_missing(pd_engine* e);
int pd_vae_weights_missing(pd_engine* e);
/* Read one tensor back in the checkpoint layout of pd_load_weights, as fp32 (HOST memory, prod(shape) floats): the exact
 * inverse of pd_load_weights for values representable in the storage type.  Matrices read back whatever is merged into them. */
int pd_read_weights(pd_engine* e, const char* name, float* out);

/* LoRA adapters, merged into the matrix weights on the device (any matrix parameter: UNet, ControlNet, text transformer, VAE,
 * SD3).  W = W0 + sum over the adapters of scale_a * up_a . down_a, rebuilt from the saved base rows W0 at every merge, in the
 * storage type; the sampling path is unchanged.  None of these may run during a sampling session.
 * pd_lora_add: register one factor pair of adapter `adapter` (id >= 0, caller-chosen) on tensor `name`; HOST fp32:
 *   up [up_rows, rank] (= [N, r, 1, 1]) with up_rows the tensor's rows, down [rank, K] or [rank, cin, kh, kw] (K = cin * kh * kw).
 *   A new adapter starts inactive (scale 0); pd_lora_add changes no weight unless the adapter is already active.
 * pd_lora_set_scales: scale of adapter id i = scales[i] (i < n), 0 for every id >= n; 0 = inactive.  Merges whatever changed.
 * pd_lora_remove: forget one adapter (-1: all); parameters no adapter touches any more get W0 back bit-exactly.
 * pd_load_weights / pd_init_random_weights on an adapted tensor replace its W0 and merge again. */
int pd_lora_add(pd_engine* e, int32_t adapter, const char* name, const float* up, int32_t up_rows, int32_t rank, const float* down,
                const int64_t* down_shape, int32_t down_ndim);
int pd_lora_set_scales(pd_engine* e, const float* scales, int32_t n);
int pd_lora_remove(pd_engine* e, int32_t adapter);
/* Adapters that are not a plain factor pair (DESIGN.md §7 "LoRA adapters" has the formulas).  An adapter contributes
 *   E = s * D                                      without a magnitude,
 *   E = (m / n) (.) (W0 + s * D) - W0, row-wise,   with one (DoRA); n[o] = || (W0 + s * D)[o, :] ||_2 in fp32, factor 0 where n = 0,
 * with s its pd_lora_set_scales scale and D by kind (N rows, K = cin * kh * kw columns in checkpoint order [.., cin, kh, kw]):
 *   PD_LORA_PAIR  D = scale * up . down                      up [N, rank], down [rank, K]
 *   PD_LORA_HADA  D = scale * (up . down) (.) (up2 . down2)  up2 [N, rank2], down2 [rank2, K]
 *   PD_LORA_KRON  D[i * c + p, j * d + q, y, x] = scale * w1[i, j] * w2[p, q, y, x]
 *                 up = w1 [kron_a, kron_b], down = w2 [c, d, kh, kw] with kron_a * c = N and kron_b * d = cin.
 * W = round_T(W0 + (plain pd_lora_add columns) + E_1 + E_2 + ...), the E in load order, summed in fp32 and rounded once.
 * A PD_LORA_PAIR without a magnitude is what pd_lora_add registers (scale is multiplied into up first, in fp32).  HOST fp32. */
enum { PD_LORA_PAIR = 0, PD_LORA_HADA = 1, PD_LORA_KRON = 2 };
typedef struct pd_lora_factors {
    int32_t kind;             /* PD_LORA_* */
    int32_t rank, rank2;      /* PAIR / HADA: inner dimension of up . down (and of up2 . down2) */
    int32_t kron_a, kron_b;   /* KRON: shape of w1 */
    float scale;              /* alpha / r (1 where the format has none) */
    const float *up, *down, *up2, *down2;
    const float* magnitude;   /* [N], or NULL */
} pd_lora_factors;
int pd_lora_add_ex(pd_engine* e, int32_t adapter, const char* name, const pd_lora_factors* f);

/* FreeU (diffusers UNet2DConditionModel.enable_freeu / disable_freeu): engine state that every later UNet evaluation applies
 * (pd_eps, pd_ddim_sample, pd_unipc_sample, the per-step export, captured graphs).  In the decoder blocks of the lowest
 * resolution (stage 1: s1, b1) and the next one (stage 2: s2, b2), before each skip concat: the first half of the backbone
 * channels is multiplied by b, and the skip tensor (control residual added) passes through fourier_filter(threshold 1,
 * scale s).  Any value 0 (all zeros: the disable call) turns it off -- diffusers' `s1 and s2 and b1 and b2` -- and the
 * decoder then runs exactly what it runs without FreeU.  Non-finite values are rejected.  A call that changes the state drops
 * the captured graphs; the next UNet evaluation uses the new values.
 * pd_get_freeu: out[4] = {s1, s2, b1, b2} as set (zeros when disabled); returns 0. */
int pd_set_freeu(pd_engine* e, float s1, float s2, float b1, float b2);
int pd_get_freeu(pd_engine* e, float out[4]);

/* Perturbed-attention guidance, PAG (Ahn et al., arXiv:2403.17377; diffusers' PAGMixin and PAGCFGIdentitySelfAttnProcessor2_0):
 * engine state like pd_set_freeu, so pd_sample_args and pd_abi_version() are what they were.  While it is on, every evaluation that is
 * followed by a guided eps (pd_ddim_sample, pd_unipc_sample, pd_lms_sample, pd_sample_step, pd_sample_eps_at, captured graphs, img2img
 * and inpainting; not pd_eps, which forms none) carries `batch` more samples: perturbed sample j is conditional sample j -- latent,
 * timestep, text context, example pair, query, the conditional ControlNet residuals (also in guess mode) and IP-Adapter tokens, FreeU,
 * LoRA -- except that in the UNet transformer blocks of layer_mask the self-attention is the identity: attn1 = to_out(to_v(norm1(h))),
 * bias included, no softmax.  The ControlNet is never perturbed.  The guided eps is, in fp32 with every operation rounded on its own,
 *   (e_u + s (e_c - e_u)) + p_i (e_c - e_p)      with use_cfg,          e_c + p_i (e_c - e_p)      without,
 * p_i = scale when adaptive_scale == 0, else max(scale - adaptive_scale (1000 - t_i), 0) with t_i the timestep of evaluation i (the
 * literal is 1000), computed on the host in double and passed to the update kernel as fp32.
 *   layer_mask  bit j = UNet transformer block j in the order of pd_ip_adapter_configure's blocks: the encoder's, then the decoder's,
 *               then the middle block (SD1.5: 0-5, 6-14, 15).  Bits beyond the network's blocks are refused.
 * scale == 0 or layer_mask == 0 means off: every call then launches exactly what it launches on an engine that never heard of PAG.
 * Negative or non-finite values are refused, and so is switching it on while a sampling session is active (the session's workspace
 * was sized at its begin; switching off is always possible).  A call that changes the state drops the captured graphs.
 * The perturbed samples exist from the first masked block on (they carry the conditional samples' numbers before it): the batch grows
 * from Bf to Bf + batch there, ordered [uncond ; cond ; perturbed].  Option "pag_fork" 0 (pd_set_option; not in pd_option_info's list)
 * instead runs them as a full third of the UNet's batch from conv_in on -- the plain evaluation the fork is tested against.  A masked
 * block runs layer by layer, never the fused 320-channel kernels.  Stats: "pag_launches" counts the identity launches and the second
 * launch of everything the branch splits (its cross-attention, its image term, its skip concat, an unmasked block behind the fork),
 * "pag_fork_block" is the block where the last evaluation forked (-1: none, or pag_fork 0).  "pag_launches" does not count what a masked
 * 320-channel block adds by leaving the fused front / tail kernels for its per-layer path.  Option "pag_fork" is refused inside a session.
 * The guided eps of an evaluation with the state off is computed exactly as before the state existed (the CFG multiply-add as one FMA).
 * pd_get_pag: out[2] = {scale, adaptive_scale}, *layer_mask (may be NULL) as set; returns 0. */
int pd_set_pag(pd_engine* e, float scale, float adaptive_scale, uint32_t layer_mask);
int pd_get_pag(pd_engine* e, float out[2], uint32_t* layer_mask);
/* The identity-attention kernel alone (pag.hip) on B samples of N tokens and C channels in the engine's storage type, `iters` launches
 * between two events, and a device-to-device copy of the bytes it moves (B N C elements read and written); milliseconds per launch. */
int pd_bench_pag_identity(pd_engine* e, int32_t B, int32_t N, int32_t C, int32_t iters, float* ms_kernel, float* ms_copy);

/* Seeded noise.  The engine draws standard normals itself with the counter-based generator Philox4x32-10 (multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds): one block maps (counter[4], key[2]) to four
 * uint32 r0..r3, and Box-Muller in fp32 turns them into four normals:
 *   u(r) = (float)r * 2^-32 + 2^-33                                   in (0, 1]
 *   (z0, z1) = sqrtf(-2 logf(u(r0))) * (cospif, sinpif)(2 u(r1)),     (z2, z3) the same from r2, r3
 * Addressing -- the contract; a value depends on nothing else (not on the batch split, the grid or the kernel that draws it):
 *   key     = (seed low 32 bits, seed high 32 bits)
 *   counter = (q, sample, draw, stream),  the element takes z[lane]
 *   q = e / 4 (low 32 bits), lane = e % 4, e = the element's index within its sample in the caller's NCHW layout (c * HW + p)
 *   sample  = sample_base + b: a 64-bit add of which the low 32 bits are used, so samples 2^32 apart share their draws
 *   draw    = the step (DDIM) or row (linear multistep) index; 0 for x_T and the VAE posterior
 *   stream  = PD_RNG_XT, PD_RNG_STEP, PD_RNG_VAE, or PD_RNG_USER + k (k >= 0) for a caller's own draws through pd_randn
 * pd_philox4x32_10: one block on the host (no engine, no GPU).
 * pd_set_rng / pd_get_rng: engine state like FreeU, default (0, 0).  The two values live in a small device buffer the kernels
 *   read, updated by a copy ordered on the engine's stream: a captured graph (option "graph") replays with the new seed, it is
 *   neither dropped nor captured again.
 * pd_randn: out[B][per_sample] (fp32, `mem`) = the values the loop draws at (stream, draw, sample_base + b, e); any
 *   per_sample >= 1. */
#define PD_RNG_XT   0
#define PD_RNG_STEP 1
#define PD_RNG_VAE  2
#define PD_RNG_USER 16
void pd_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
int pd_set_rng(pd_engine* e, uint64_t seed, uint64_t sample_base);
int pd_get_rng(pd_engine* e, uint64_t* seed, uint64_t* sample_base);
int pd_randn(pd_engine* e, int32_t stream, int32_t draw, int32_t B, int64_t per_sample, int32_t mem, float* out);

/* first-stage decode, LatentDiffusion.decode_first_stage (ldm/models/diffusion/ddpm.py:820-828) ->
 * AutoencoderKL.decode (ldm/models/autoencoder.py:89-92) -> Decoder.forward (ldm/modules/diffusionmodules/model.py:619-653):
 * latents [B, in_ch, h, w] -> images [B, vae_out_ch, 8h, 8w] in roughly [-1, 1] (fp32, NCHW).  Call after the sampling
 * session has ended; parameters are the checkpoint's first_stage_model.decoder.* / first_stage_model.post_quant_conv.* */
int pd_vae_decode(pd_engine* e, const float* latents, int32_t B, int32_t h, int32_t w, int32_t mem, float* images_out);

/* first-stage encode, LatentDiffusion.encode_first_stage + get_first_stage_encoding (ddpm.py:831-832, :655-662) ->
 * AutoencoderKL.encode (autoencoder.py:83-87) -> Encoder.forward (model.py:508-544) -> DiagonalGaussianDistribution
 * (ldm/modules/distributions/distributions.py:24-62; logvar clamped to [-30, 20], std = exp(0.5 logvar)).
 * images [B, vae_out_ch, H, W] in [-1, 1], NCHW fp32; H and W multiples of 8 with (H/8)*(W/8) a multiple of 64.  `images`,
 * `noise` and `out` live in `mem`.  Needs an engine created with vae_encoder = 1, its first_stage_model.encoder.* /
 * first_stage_model.quant_conv.* weights, and no active sampling session.  Random draws come from the caller, or, with
 * `noise` NULL, from the engine's generator at (PD_RNG_VAE, draw 0): */
#define PD_VAE_MEAN    0  /* scale_factor * posterior.mode()                        -> [B, z, H/8, W/8]   */
#define PD_VAE_SAMPLE  1  /* scale_factor * posterior.sample() (`noise` or seeded)  -> [B, z, H/8, W/8]   */
#define PD_VAE_MOMENTS 2  /* quant_conv output (mean ; logvar), unscaled            -> [B, 2z, H/8, W/8]  */
int pd_vae_encode(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what,
                  const float* noise /* [B, z, H/8, W/8] or NULL, SAMPLE only */, float* out);
/* number of encoder tensors not loaded yet (0 when the encoder is not built) */
int pd_vae_encoder_weights_missing(pd_engine* e);

/* Tiled and sliced VAE calls (diffusers AutoencoderKL.enable_tiling / enable_slicing; the reference's pipeline_prompt_diffusion.py:242-272).
 * Opt-in engine state like pd_set_freeu: with both switches off every call runs exactly what it ran before.  `which` selects the VAE:
 * PD_VAE_SD15 (pd_vae_decode / pd_vae_encode) or PD_VAE_SD3 (pd_sd3_vae_decode / pd_sd3_vae_encode).
 *
 * Tiling, with T = tile_latent, f = overlap_factor, u = 2^(num_levels - 1) = 8 (all of it diffusers' tiled_decode / tiled_encode):
 *   decode of z [B, C, h, w], only when h > T or w > T:  ov = int(T (1 - f)), be = int(T u f), limit = T u - be.  For i in range(0, h, ov),
 *   j in range(0, w, ov): tile = decoder(post_quant_conv(z[:, :, i:i+T, j:j+T])) (truncated at the border).  Then in row-major order and in
 *   place: tile = blend_v(tile above, tile, be) if i > 0; tile = blend_h(tile to the left, tile, be) if j > 0; the output is the
 *   concatenation of tile[:, :, :limit, :limit].  blend_v(a, b, e): e = min(a.H, b.H, e); b[y] = a[a.H - e + y] * (1 - y / e) + b[y] * (y / e)
 *   for y < e, the two weights computed in double and rounded to fp32, both products and the sum rounded to fp32 on their own; blend_h
 *   the same along W.
 *   encode of x [B, 3, H, W], only when H > T u or W > T u:  ov = int(T u (1 - f)), be = int(T f), limit = T - be; a tile is
 *   quant_conv(encoder(window)), the moments; blend and crop run on the moments and the posterior is taken once from the assembled ones.
 * The last row / column of the grid may be a remainder of a single latent pixel; e then shrinks through the min.  Accepted: 0 < f <= 1/3
 * and T f an integer (so that limit = ov u, which diffusers assumes silently); then each output value depends on at most four raw tiles and
 * the engine assembles the output in one kernel, byte-identical in fp32 to the sequential procedure applied to the same tiles.
 * Tiles of equal shape run through the layers as one batch, tile_batch tiles at a time.  A tile whose h_t * w_t is no multiple of 8 takes the
 * flash attention kernel (2-byte modes); the fp32-storage modes reject such a call and name the tile.
 *
 * Slicing: with B > 1 every sample is decoded / encoded on its own, in order (and tiled, with both switches on); noise and seeded draws
 * address the samples as in the unsliced call.
 *
 * pd_vae_set_tiling: with on != 0, tile_latent / overlap_factor / tile_batch replace the stored parameters, 0 = the default (T 64 for
 * SD1.5 and 128 for SD3 -- 512 / 1024 pixels, diffusers' tile_sample_min_size = sample_size; f 0.25; tile_batch 4).  With on = 0 tiling
 * is switched off and an argument of 0 KEEPS the stored parameter (pd_vae_set_tiling(e, which, 0, 0, 0, 0) is the plain disable call);
 * a non-zero argument still replaces it.  A refused call changes nothing.
 * pd_vae_get_tiling: the state with defaults resolved; any pointer may be NULL. */
#define PD_VAE_SD15 0
#define PD_VAE_SD3  1
int pd_vae_set_tiling(pd_engine* e, int32_t which, int32_t on, int32_t tile_latent, double overlap_factor, int32_t tile_batch);
int pd_vae_set_slicing(pd_engine* e, int32_t which, int32_t on);
int pd_vae_get_tiling(pd_engine* e, int32_t which, int32_t* tiling, int32_t* slicing, int32_t* tile_latent, double* overlap_factor,
                      int32_t* tile_batch);
/* The tile grid of one tiled call; host only (no engine, no GPU).  decode (encode = 0): h, w are the latent size; encode (encode = 1): the
 * image size, multiples of u.  *rows = *cols = 0 when the call is not tiled (h <= T and w <= T, resp. T u).  With tiles non-NULL (cap >=
 * rows * cols entries, row-major): the input window (y0, x0, h, w) in input pixels, the kept output rectangle (oy, ox, oh, ow) and the
 * tile's own output size (th, tw) in output pixels, the blend extents ev / eh against the tile above / to the left (0 in the first row /
 * column) and cls, the index of the tile's shape class (tiles of equal h and w; numbered in order of first appearance, *classes of them). */
typedef struct pd_vae_tile {
    int32_t y0, x0, h, w;
    int32_t oy, ox, oh, ow;
    int32_t th, tw, ev, eh;
    int32_t cls, reserved[3];
} pd_vae_tile;
int pd_vae_tile_plan(int32_t h, int32_t w, int32_t tile_latent, double overlap_factor, int32_t u, int32_t encode, int32_t* rows, int32_t* cols,
                     int32_t* classes, pd_vae_tile* tiles, int32_t cap);

/* HED edge detector: the annotator that turns a photograph into the condition map of `query` / `pair` (apply_hed of the reference's
 * demo; HEDdetector.__call__ and Network.forward, annotator/hed/__init__.py:71-114): a VGG-16 trunk of 13 conv3x3 + ReLU in five
 * stages, one conv1x1 score head per stage, the five score maps upsampled bilinearly (align_corners = False) to the input size,
 * a 5 -> 1 combine and a sigmoid.
 * pd_hed_configure registers its 38 tensors on an existing engine (any pd_config; a registry group of its own, like
 * pd_sd3_configure) under "hed." + Network's names: hed.netVggOne.0.weight .. hed.netCombine.0.bias.  Calling it again does nothing.
 * pd_hed_detect: images [B, 3, H, W] fp32 NCHW, RGB in [0, 1] (the (D) pipeline's image convention); the BGR flip and the
 * x * 255 - (104.00698793, 116.66876762, 122.67891434) of the reference happen inside, in fp32.  H and W multiples of 16 (four
 * 2x2 max-pools; the reference's resize_image gives multiples of 64).  `images` and `out` live in `mem`.  Needs all hed.* weights
 * and no active sampling session. */
#define PD_HED_EDGE  0   /* sigmoid(netCombine(cat(5 upsampled side maps)))  -> [B, 1, H, W] in [0, 1] */
#define PD_HED_SIDES 1   /* the five bilinearly upsampled score maps, pre-combine -> [B, 5, H, W]        */
int pd_hed_configure(pd_engine* e);
int pd_hed_weights_missing(pd_engine* e);    /* 0 when not configured */
int pd_hed_detect(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, float* out);

/* M-LSD line detector: the annotator behind the reference's "mlsd" task, the straight-line condition map (MLSDdetector.__call__,
 * annotator/mlsd/__init__.py:27-39; pred_lines, annotator/mlsd/utils.py:47-86; MobileV2_MLSD_Large, models/mbv2_mlsd_large.py):
 * MobileNetV2 features 0..13 (depthwise conv3x3 + pointwise conv1x1), a top-down decoder (blocks 15..23: conv1x1 pairs into a
 * concat, bilinear x2 upsamples with align_corners = True, conv3x3 pairs, one conv3x3 of dilation 5), then on the [B, 9, H/2, W/2]
 * map: 3x3 non-maximum suppression of the centre channel, the 200 best peaks, score and length thresholds, end points, cv2.line.
 * pd_mlsd_configure registers the network on an existing engine (any pd_config; a registry group of its own) under "mlsd." + the
 * checkpoint's keys.  Every BatchNorm is FOLDED into the conv in front of it, and the registry holds the folded form only: per conv its
 * weight under the conv's own key ("mlsd.backbone.features.0.0.weight", [32, 4, 3, 3]) and one bias under the key of the BatchNorm's
 * bias ("mlsd.backbone.features.0.1.bias"); block23.conv3, which has no BatchNorm, keeps its own weight and bias.  With s = gamma /
 * sqrt(running_var + 1e-5): weight' = weight * s[:, None, None, None], bias' = (conv_bias - running_mean) * s + beta (conv_bias 0
 * where the conv has none).  A host folds before pd_load_weights (the Python Engine.load_mlsd_state_dict does, in fp64, rounding once);
 * pd_read_weights returns folded tensors.  Calling pd_mlsd_configure again does nothing.
 * pd_mlsd_detect: images [B, H, W, 3] uint8 RGB; the constant-one fourth channel and x / 127.5 - 1 happen inside, in fp32.  H and W
 * multiples of 32 (five stride-2 layers; the reference's resize_image gives multiples of 64).  The reference handles one image per call
 * with input_shape = the image's own shape; a batch is B independent images.  thr_v >= 0.  `images` and `out` live in `mem`.  Needs all
 * mlsd.* weights and no active sampling session.  The rasteriser restates cv2.line (thickness 1, LINE_8: clipLine, then LineIterator);
 * its byte parity with OpenCV itself is unverified where OpenCV is absent. */
#define PD_MLSD_TPMAP    0   /* the network output, channels 7..15 of block23   -> float [B, 9, H/2, W/2]                            */
#define PD_MLSD_SEGMENTS 1   /* the kept segments, best score first             -> int32 [B, 200, 4] (x0, y0, x1, y1), then int32 [B] counts */
#define PD_MLSD_LINES    2   /* the segments drawn white on black               -> uint8 [B, H, W] of 0 / 255                        */
int pd_mlsd_configure(pd_engine* e);
int pd_mlsd_weights_missing(pd_engine* e);   /* 0 when not configured */
int pd_mlsd_detect(pd_engine* e, const uint8_t* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, float thr_v, float thr_d,
                   void* out);
/* ... with, for PD_MLSD_LINES, the float form pd_canny also gives: channels c_off .. c_off + 2 of dst_f [B, Cf, H, W] fp32 (in mem_f)
 * receive (v / 255) * mul + add, the other channels keep their values; out may then be NULL.  dst_f NULL: pd_mlsd_detect. */
typedef struct pd_mlsd_args {
    const uint8_t* images;
    int32_t B, H, W, mem, what;
    float thr_v, thr_d;
    void* out;
    float* dst_f;
    int32_t mem_f, Cf, c_off;
    float mul, add;
} pd_mlsd_args;
int pd_mlsd_detect_ex(pd_engine* e, const pd_mlsd_args* a);

/* Image ends: the uint8 pictures at both ends of a call, on the device.  Every step is integer or single-rounding fp32 arithmetic,
 * so the results are bit-identical to the host code they replace (Pillow's 8-bit Image.resize, NumPy's / 255, clip, round).
 *
 * pd_resample_coefficients: the tables of Pillow's 8-bit resampler (Resample.c: precompute_coeffs + normalize_coeffs_8bpc) along
 * one axis; host only (no engine, no GPU).  All of it in double until the last line:
 *   scale = in / out, fs = max(scale, 1), support = S fs (S = 3 Lanczos, 0.5 box), *ksize = 2 ceil(support) + 1; per output xx:
 *   center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in),
 *   w[x] = f((x + xmin - center + 0.5) * (1 / fs)) for x < xmax - xmin (Pillow multiplies by the reciprocal), divided by their sum
 *   when that is non-zero; kk = (int)(w 2^22 + 0.5) for w >= 0, (int)(w 2^22 - 0.5) for w < 0 (truncation towards zero).
 *   Lanczos f(t) = sinc(t) sinc(t / 3) for -3 <= t < 3 (sinc(t) = sin(pi t) / (pi t), 1 at 0), else 0; box f(t) = 1 for -0.5 < t <= 0.5.
 * With bounds and kk NULL only *ksize is written; otherwise bounds[out_size][2] = (xmin, xmax - xmin) and kk[out_size][*ksize], zero
 * padded.  Reductions beyond in_size > PD_RESAMPLE_MAX_SCALE * out_size are refused (callers keep their host path), as are unknown filters.
 * A pass computes clip8((2^21 + sum pixel * kk) >> 22) in int32 (arithmetic shift) and stores uint8; the horizontal pass runs first
 * and its rounded bytes feed the vertical one; a pass whose sizes are equal is skipped. */
#define PD_RESAMPLE_LANCZOS 1   /* PIL.Image.LANCZOS */
#define PD_RESAMPLE_BOX     4   /* PIL.Image.BOX */
#define PD_RESAMPLE_MAX_SCALE 8
int pd_resample_coefficients(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* kk);

/* pd_image_load: uint8 pictures [Bs, Hs, Ws, 3] (NHWC) -> channels c_off .. c_off + 2 of an fp32 NCHW tensor [B, C, H, W]; the other
 * channels are not touched (the two halves of an example pair land in one [B, 6, H, W] tensor).  Resampled to H x W with the tables
 * above when the sizes differ, then y = v * mul + add with v = (float)u8 / 255.0f correctly rounded, the product and the sum each
 * rounded once (the semantics of __fmul_rn / __fadd_rn; the kernels compile these lines with FP contraction off, because hipcc fuses
 * even those two intrinsics into an FMA): (1, 0) gives [0, 1], (2, -1) gives [-1, 1], as NumPy's float32
 * (a / 255) * mul + add does for any mul / add.  Bs == B, or Bs divides B: PD_IMAGE_REPEAT reads source b / (B / Bs) (np.repeat),
 * PD_IMAGE_TILE source b % Bs (whole-batch repeats).  src and dst each live in their own memory space.  Tables, the intermediate
 * picture of the horizontal pass and the staging of host buffers are engine-owned and grow on demand: a repeated call at the same
 * shapes allocates nothing (stat "image_allocs" counts the allocations).  Runs on the engine's stream, synchronised on return. */
#define PD_IMAGE_REPEAT 0
#define PD_IMAGE_TILE   1
typedef struct pd_image_load_args {
    const uint8_t* src;       /* [Bs, Hs, Ws, 3] */
    int32_t Bs, Hs, Ws;
    int32_t mem_src;          /* PD_MEM_* of src */
    float* dst;               /* [B, C, H, W] */
    int32_t B, C, H, W;
    int32_t c_off;            /* 0 <= c_off, c_off + 3 <= C */
    int32_t mem_dst;          /* PD_MEM_* of dst */
    int32_t filter;           /* PD_RESAMPLE_*; only read when the sizes differ */
    int32_t batch_mode;       /* PD_IMAGE_*; only read when Bs != B */
    float mul, add;
    int32_t reserved[4];      /* zero */
} pd_image_load_args;
int pd_image_load(pd_engine* e, const pd_image_load_args* args);

/* pd_image_store: fp32 NCHW [B, C, H, W], C in {1, 3} -> uint8 NHWC [B, H, W, C]: u = min(max(x * mul + add, 0), 1) * 255 in fp32
 * (each operation rounded once), then PD_ROUND_NEAREST_EVEN (np.round: the pipeline's (im * 255).round()) or PD_ROUND_TRUNC
 * (astype(uint8): the annotators' edge maps).  Inputs are finite.  Runs on the engine's stream, synchronised on return. */
#define PD_ROUND_NEAREST_EVEN 0
#define PD_ROUND_TRUNC        1
int pd_image_store(pd_engine* e, const float* src, int32_t B, int32_t C, int32_t H, int32_t W, int32_t mem_src, float mul, float add,
                   int32_t rounding, uint8_t* dst, int32_t mem_dst);

/* PIL.Image.BICUBIC for the 8-bit resampler: Pillow's bicubic kernel with a = -0.5, support 2 --
 *   f(t) = ((a + 2) |t| - (a + 3)) t^2 + 1 for |t| < 1, (((|t| - 5) |t| + 8) |t| - 4) a for |t| < 2, else 0
 * through the same precompute_coeffs / normalize_coeffs_8bpc arithmetic as above.  pd_resample_coefficients and pd_image_load keep
 * their two filters (and keep refusing 3); pd_resample_coefficients_ex takes LANCZOS, BOX and BICUBIC, same arguments, same tables for
 * the first two. */
#define PD_RESAMPLE_BICUBIC 3   /* PIL.Image.BICUBIC */
int pd_resample_coefficients_ex(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* kk);

/* ---------------------------------------------------------------------------------------------------------------
 * CLIP image tower (transformers' CLIPVisionModelWithProjection): what the reference pipeline's image_encoder / encode_image
 * (pipeline_prompt_diffusion.py:490-513) and safety_checker / run_safety_checker (:514-528) rest on.  Opt-in: an engine that never
 * calls pd_clip_vision_configure is unchanged.
 *
 * pd_clip_preprocess: CLIPImageProcessor() with its defaults on uint8 pictures [B, H, W, 3] --
 *   1. resize the shortest edge to image_size: (H, W) -> (S, (int)(S * W / H)) for H <= W, ((int)(S * H / W), S) otherwise
 *      (get_resize_output_image_size; 96 x 160 -> 224 x 373), PIL BICUBIC on uint8, horizontal pass first, its rounded bytes feed the
 *      vertical pass; 2. centre crop to S x S (top = (Hr - S) / 2, left = (Wr - S) / 2); 3. (v / 255 - mean) / std in fp32, every
 *      operation rounded once.
 * Only the columns and rows that survive the crop are resampled.  pd_clip_preprocess_geometry gives (Hr, Wr, top, left); host only.
 * out_mode:
 *   PD_CLIP_OUT_PIXEL_VALUES  fp32 [B, 3, S, S]
 *   PD_CLIP_OUT_PATCHES       the patch GEMM's operand: [B * (S / patch)^2, Kw] in the engine's operand type (fp32 in the fp32-storage
 *                             modes, else f16 / bf16), Kw = round_up(3 patch^2, 8) = pd_clip_patch_width(patch), element k = c patch^2 +
 *                             py patch + px of patch row b (S / patch)^2 + ty (S / patch) + tx (the flattened Conv2d weight's order), columns
 *                             past 3 patch^2 zero.  S must be a multiple of patch.
 *   PD_CLIP_OUT_BYTES         uint8 [B, S, S, 3]: the resized and cropped picture before normalisation
 * Reductions beyond PD_RESAMPLE_MAX_SCALE are refused (callers keep their host processor). */
#define PD_CLIP_OUT_PIXEL_VALUES 0
#define PD_CLIP_OUT_PATCHES      1
#define PD_CLIP_OUT_BYTES        2
typedef struct pd_clip_preprocess_args {
    const uint8_t* src;       /* [B, H, W, 3] */
    int32_t B, H, W;
    int32_t mem_src;          /* PD_MEM_* of src */
    int32_t image_size;       /* S */
    int32_t patch;            /* read for PD_CLIP_OUT_PATCHES only */
    int32_t out_mode;         /* PD_CLIP_OUT_* */
    int32_t mem_dst;          /* PD_MEM_* of dst */
    void* dst;
    float mean[3], std[3];    /* image_mean / image_std (OpenAI's: 0.48145466, 0.4578275, 0.40821073 / 0.26862954, 0.26130258, 0.27577711) */
    int32_t reserved[4];      /* zero */
} pd_clip_preprocess_args;
int pd_clip_preprocess(pd_engine* e, const pd_clip_preprocess_args* args);
int pd_clip_preprocess_geometry(int32_t H, int32_t W, int32_t image_size, int32_t* Hr, int32_t* Wr, int32_t* top, int32_t* left);
int pd_clip_patch_width(int32_t patch);

/* The tower.  pd_clip_vision_configure registers one CLIPVisionModelWithProjection on an existing engine (any pd_config) in a registry
 * group of its own; up to two towers per engine, told apart by `prefix` ("safety_checker.vision_model." and "image_encoder." in a
 * diffusers checkpoint).  Configuring a prefix again does nothing.  Tensors carry transformers' names under the prefix (its
 * "pre_layrnorm" spelling included):
 *   <prefix>vision_model.embeddings.class_embedding [C], ...patch_embedding.weight [C, 3, p, p] (no bias), ...position_embedding.weight
 *   [P + 1, C], <prefix>vision_model.pre_layrnorm.{weight,bias}, <prefix>vision_model.encoder.layers.N.* (as the text stack),
 *   <prefix>vision_model.post_layernorm.{weight,bias}, and visual_projection.weight [D, C] next to the outermost "vision_model.":
 *   "image_encoder.visual_projection.weight", "safety_checker.visual_projection.weight" (a trailing "vision_model." of the prefix is
 *   dropped for it).
 * hidden = heads * dh with dh one of the attention kernels' head dims (64: ViT-L/14, 80: ViT-H/14); hidden <= 2048, hidden and ff
 * multiples of 8; image_size a multiple of patch.  stream_f32 != 0 keeps the residual stream in fp32 in every precision mode (the choice
 * of the SD3 text encoders; for image_encoder); 0 keeps it in the engine's stream type (the SD1.5 text encoder's; for the safety tower). */
typedef struct pd_clip_vision_config {
    int32_t hidden, layers, heads, ff, patch, image_size, proj_dim;
    int32_t act;              /* PD_CLIP_ACT_* */
    float eps;                /* layer_norm_eps, 1e-5 */
    int32_t stream_f32;
    float mean[3], std[3];    /* of the uint8 input path */
    char prefix[64];
    int32_t reserved[4];      /* zero */
} pd_clip_vision_config;
int pd_clip_vision_configure(pd_engine* e, const pd_clip_vision_config* cfg);
int pd_clip_vision_weights_missing(pd_engine* e, const char* prefix);   /* 0 when that prefix is not configured */
/* One forward pass.  input: uint8 pictures [B, H, W, 3] (PD_CLIP_IN_U8: through pd_clip_preprocess's patch-matrix path, no fp32 picture
 * is written) or fp32 pixel_values [B, 3, S, S] (PD_CLIP_IN_PIXEL_VALUES; H = W = image_size).  Outputs, each NULL or a buffer in `mem`:
 *   image_embeds  [B, D]        visual_projection(pooler_output)
 *   pooler_output [B, C]        post_layernorm(last_hidden_state[:, 0])
 *   hidden        [B, P + 1, C] hidden_states[hidden_layer]: 0 = the output of pre_layrnorm, k = after k blocks, negative values count
 *                               from the end (-1 = after the last block, -2 = encode_image's); never through post_layernorm. */
#define PD_CLIP_IN_U8           0
#define PD_CLIP_IN_PIXEL_VALUES 1
typedef struct pd_clip_vision_args {
    const char* prefix;
    const void* input;
    int32_t input_kind;       /* PD_CLIP_IN_* */
    int32_t B, H, W;
    int32_t mem;              /* PD_MEM_* of input and of every output */
    int32_t hidden_layer;     /* read when hidden != NULL */
    float* image_embeds;
    float* pooler_output;
    float* hidden;
    int64_t reserved[2];      /* zero */
} pd_clip_vision_args;
int pd_clip_vision_forward(pd_engine* e, const pd_clip_vision_args* args);

/* Safety checker: diffusers' StableDiffusionSafetyChecker.forward on the image_embeds of the tower under "safety_checker.vision_model."
 * (which must be configured first).  pd_safety_configure registers, in a group of its own, safety_checker.concept_embeds [17, D],
 * safety_checker.special_care_embeds [3, D], safety_checker.concept_embeds_weights [17], safety_checker.special_care_embeds_weights [3].
 * pd_safety_check, everything in fp32, one block per image: cosines of the L2-normalised embedding against the L2-normalised rows;
 * adj = 0; for the special-care rows j = 0, 1, 2 in order: s = cos - thr_j + adj, and adj becomes 0.01 once an s counts as positive
 * (carried into the later rows, as diffusers' loop does); then for the 17 concept rows s = cos - thr_j + adj; flag = any concept score
 * positive.  diffusers rounds with Python's round(s, 3) before `> 0`: a score is positive iff it exceeds 0.0005 (no fp32 value equals
 * that boundary).  embeds [B, D] and flags int32 [B] live in `mem`; scores (NULL, or [B, 20] = 3 special then 17 concept, unrounded) too.
 * pd_safety_blank writes `value` over every element of the flagged images of a DEVICE batch [B][per_image] fp32 (flags in mem_flags):
 * 0 is what the checker itself writes; a caller whose pd_image_store denormalises with (mul, add) passes -add / mul so that the
 * stored picture is black, which is what the reference's postprocess(do_denormalize = [not nsfw]) makes of the zeroed image. */
#define PD_SAFETY_CONCEPTS 17
#define PD_SAFETY_SPECIAL  3
int pd_safety_configure(pd_engine* e);
int pd_safety_weights_missing(pd_engine* e);   /* 0 when not configured */
int pd_safety_check(pd_engine* e, const float* embeds, int32_t B, int32_t mem, int32_t* flags, float* scores);
int pd_safety_blank(pd_engine* e, float* images, int32_t B, int64_t per_image, const int32_t* flags, int32_t mem_flags, float value);

/* ---------------------------------------------------------------------------------------------------------------
 * IP-Adapter image prompts (the reference pipeline's ip_adapter_image / ip_adapter_image_embeds; diffusers' IPAdapterAttnProcessor with
 * the linear ImageProjection: ip-adapter_sd15, ip-adapter_sd15_light).  Opt-in engine state like pd_set_freeu: an engine that never
 * configures an adapter, has no image set, or has every scale at 0 makes exactly the launches it makes without this section.
 *
 * pd_ip_adapter_configure registers, in a registry group of its own and under the flattened checkpoint names,
 *   image_proj.proj.{weight [T D, E], bias [T D]}, image_proj.norm.{weight, bias} [D]           (D = pd_config.context_dim)
 *   ip_adapter.{2 j + 1}.to_k_ip.weight, ip_adapter.{2 j + 1}.to_v_ip.weight   [C_j, D] each, no bias
 * for the UNet's cross-attention blocks j in diffusers' processor order: those of the input blocks, then those of the output blocks,
 * then the middle block (16 blocks, ids 1 .. 31, for the SD1.5 topology).  The ControlNet carries no adapter.  They load through
 * pd_load_weights.  1 <= num_tokens <= 64; embed_dim and context_dim multiples of 8; every block's head dim one of 8, 16, 32, 40, 80, 160.
 * One adapter per engine; configuring again does nothing.
 *
 * pd_ip_adapter_set_image: cond [Bi, E] fp32 image embeddings in `mem`, uncond [Bi, E] or NULL (zeros, as the reference's encode_image
 * returns for the unconditional half -- their projection is LayerNorm(bias), not zero, and runs through the same code).  Right then, once:
 *   tok = LayerNorm_D(reshape(proj.weight e + proj.bias, [T, D]), eps 1e-5);  K_ip,j = tok to_k_ip_j^T,  V_ip,j = tok to_v_ip_j^T
 * for both halves and every block, into engine-owned buffers in the compute type.  pd_ip_adapter_clear_image drops the state (the buffers stay
 * allocated).  Setting an image is refused while a sampling session is open; clearing is not, so that a caller can always leave.  A sampling call of batch B needs Bi == B or Bi == 1 (one image for every sample).
 *
 * pd_ip_adapter_set_scale: n = 1 (every block) or one scale per block; all 1 after configure.  The adapter is active when an image is
 * set and at least one scale is non-zero.  Then every UNet evaluation of the engine (pd_ddim_sample, pd_unipc_sample, pd_lms_sample,
 * pd_sample_step, pd_eps, pd_sample_eps_at, captured graphs) computes in every block with s_j != 0
 *   attn2(x) = to_out(softmax(q k^T / sqrt(dh)) v + s_j softmax(q K_ip,j^T / sqrt(dh)) V_ip,j)
 * with the block's own q and heads and a softmax of its own over the T image keys: one launch per block and guidance half after the text
 * cross-attention, in fp32 with one rounding to the compute type (ip_attention.hip).  With use_cfg the unconditional half of the batch
 * reads the unconditional buffers; without it only the conditional ones are used.  A UNet block with a term runs its per-layer path
 * (the fused 320-channel tail cannot take the term); the ControlNet is untouched.  Every setter drops the captured graphs.  Stat
 * "ip_launches" counts the term's launches. */
typedef struct pd_ip_adapter_config {
    int32_t num_tokens;       /* T */
    int32_t embed_dim;        /* E */
    int32_t reserved[6];      /* zero */
} pd_ip_adapter_config;
int pd_ip_adapter_configure(pd_engine* e, const pd_ip_adapter_config* cfg);
int pd_ip_adapter_weights_missing(pd_engine* e);   /* 0 when not configured */
int pd_ip_adapter_set_scale(pd_engine* e, const float* scales, int32_t n);
int pd_ip_adapter_get_scale(pd_engine* e, float* scales, int32_t n);   /* n = the number of blocks */
int pd_ip_adapter_set_image(pd_engine* e, const float* cond, const float* uncond, int32_t Bi, int32_t mem);
int pd_ip_adapter_clear_image(pd_engine* e);
/* The term's kernel alone on random data in the compute type (one key set for every sample, heads = pd_config.num_heads): ms per launch
 * over `iters` back-to-back launches, and ms per device-to-device copy of the 3 B N C elements the kernel moves, timed the same way. */
int pd_bench_ip_attention(pd_engine* e, int32_t B, int32_t N, int32_t C, int32_t T, int32_t iters, float* ms_kernel, float* ms_copy);

/* Canny edge detector: the annotator of the reference's `canny` task (annotator/canny/__init__.py: cv2.Canny(img, low, high), called
 * with 100 and 200).  It has no weights and every step is integer arithmetic, so the result is pinned byte for byte -- to a
 * restatement of OpenCV's portable C++ path (canny.cpp, aperture 3, L2gradient = false), which tests/canny_ref.py states in NumPy:
 *   lo = floor(low), hi = floor(high), swapped if lo > hi.  Per channel, 3x3 Sobel in int32 over replicated borders:
 *   dx = (p[-1,+1] + 2 p[0,+1] + p[+1,+1]) - (p[-1,-1] + 2 p[0,-1] + p[+1,-1]) ([row, col] offsets), dy its transpose, n = |dx| + |dy|.
 *   With C = 3 a pixel takes dx, dy and m = n from the channel with the largest n (the lowest index on a tie).  m is 0 outside the
 *   picture.  A pixel is a candidate iff m > lo and, with x = |dx|, y = |dy| << 15, t22 = 13573 x, t67 = t22 + (x << 16):
 *     y < t22:        m > m[0,-1] and m >= m[0,+1]
 *     else y > t67:   m > m[-1,0] and m >= m[+1,0]
 *     else:           s = (dx ^ dy) < 0 ? -1 : +1;  m > m[-1,-s] and m > m[+1,+s]
 *   A candidate with m > hi is strong, the others are weak.  The output is 255 at every candidate that is 8-connected, through
 *   candidates, to a strong one, and 0 elsewhere.
 * The connection is found on the GPU: a kernel that promotes weak pixels next to strong ones inside 64 x 64 tiles is relaunched
 * until a launch changes nothing (at most one launch per pixel, else an error).  Promotion is monotone, so the result is the same
 * bytes in every run; only the number of launches (stat "canny_sweeps", of the last call) may differ.
 * src: uint8 [B, H, W, C] (NHWC), C 1 or 3, H, W >= 1.  At least one destination: dst_u8 [B, H, W] uint8 (0 / 255) and / or dst_f, an
 * fp32 NCHW tensor [B, Cf, H, W] whose channels c_off .. c_off + 2 all receive (v / 255) * mul + add with pd_image_load's rounding
 * (the reference's HWC3 of a grey map, in the layout of `query` and of one half of the pair); its other channels are not touched.
 * Every pointer lives in its own memory space.  The state map, the sweep flags and the staging of host buffers are engine-owned
 * and grow on demand (counted in stat "image_allocs"): a repeated call at the same shape allocates nothing.  Runs on the engine's
 * stream, synchronised on return. */
#define PD_CANNY_NONE   0   /* states of the intermediate map (pd_op_canny_hysteresis): not a candidate */
#define PD_CANNY_WEAK   1   /* a candidate with m <= hi */
#define PD_CANNY_STRONG 2   /* a candidate with m > hi, or a weak one that the hysteresis reached */
typedef struct pd_canny_args {
    const uint8_t* src;       /* [B, H, W, C] */
    int32_t B, H, W, C;
    int32_t mem_src;          /* PD_MEM_* of src */
    float low, high;          /* finite */
    uint8_t* dst_u8;          /* [B, H, W] or NULL */
    int32_t mem_u8;           /* PD_MEM_* of dst_u8 */
    int32_t Cf, c_off;        /* 0 <= c_off, c_off + 3 <= Cf; only read with dst_f */
    float* dst_f;             /* [B, Cf, H, W] or NULL */
    float mul, add;
    int32_t mem_f;            /* PD_MEM_* of dst_f */
    int32_t reserved[4];      /* zero */
} pd_canny_args;
int pd_canny(pd_engine* e, const pd_canny_args* args);

/* operator boundary: eps = apply_model(x, t, cond), cldm/cldm.py:369-382.
 *   x [Bf,in_ch,h,w], t [Bf] (int64), ctx [Bf,L,D], pair [Bf,hint_ch,8h,8w], query [Bf,q_ch,8h,8w],
 *   scales [13] or NULL.  eps_out [Bf,out_ch,h,w].  residuals_out (optional): the 13 scaled
 *   control tensors, NCHW, concatenated in list order (sizes from pd_control_shape). */
int pd_eps(pd_engine* e, const float* x, const int64_t* t, const float* ctx, const float* pair,
           const float* query, const float* scales, int32_t Bf, int32_t h, int32_t w, int32_t mem,
           float* eps_out, float* residuals_out);
/* ... with ctx [Bf, context_len, context_dim]: context_len as in pd_sample_args (0: pd_config.context_len) */
int pd_eps_ctx(pd_engine* e, const float* x, const int64_t* t, const float* ctx, int32_t context_len, const float* pair,
               const float* query, const float* scales, int32_t Bf, int32_t h, int32_t w, int32_t mem,
               float* eps_out, float* residuals_out);
int pd_control_shape(pd_engine* e, int index, int32_t h, int32_t w, int32_t* C, int32_t* H, int32_t* W);

/* the fused loop: begin + S steps + read-back; blocking (stream-synchronised on return).
 *   latents_out [B,in_ch,h,w]; per_step_out optional [S+1][B,in_ch,h,w] = x_inter incl. x_T
 *   (intermediates with log_every_t=1, ddim_hacked.py:143,174-176). */
int pd_ddim_sample(pd_engine* e, const pd_sample_args* args, int32_t mem_out, float* latents_out,
                   float* per_step_out);

/* stepwise form, for callbacks that inspect or replace latents between steps
 * (callback/img_callback ddim_hacked.py:171-172; callback_on_step_end pipeline :1275-1283) */
int pd_sample_begin(pd_engine* e, const pd_sample_args* args);
int pd_sample_step(pd_engine* e, int32_t i); /* i = 0..steps-1, asynchronous on the engine stream */
#define PD_GET_LATENTS 0
#define PD_GET_PRED_X0 1
#define PD_GET_EPS 2 /* guided noise prediction of the last step */
int pd_sample_get(pd_engine* e, int32_t what, int32_t mem, float* out);
int pd_sample_set_latents(pd_engine* e, int32_t mem, const float* latents);
/* unconditional_guidance_scale of the following steps: DDIMSampler.ddim_sampling's ucg_schedule (cldm/ddim_hacked.py:159-161)
 * replaces the scale before every p_sample_ddim */
int pd_sample_set_guidance(pd_engine* e, float scale);
/* guided eps at an arbitrary timestep for the current latents, no update: lets a host-side
 * scheduler (pipeline :1273 scheduler.step) drive the engine */
int pd_sample_eps_at(pd_engine* e, int64_t t, const float* scales13);
int pd_sample_end(pd_engine* e);

/* UniPC multistep solver inside the engine's loop (Zhao et al. 2023, "UniPC", data-prediction form: UniP-p predictor +
 * UniC corrector; the same update as the host plug-in UniPCMultistepScheduler of the Python package).  Given the grid,
 * every coefficient of every step is fixed, so one step is one elementwise kernel over the guided eps, the latents, the
 * last corrected sample and up to three earlier x0 predictions; that state is kept in fp64 on the device, and only the
 * sample each step returns is rounded to fp32 -- exactly where the host scheduler rounds.
 * The grid is pd_sample_args.timesteps (required, HOST memory, strictly descending, sampling order) with `steps` entries;
 * eta must be 0 and noise NULL (UniPC draws no noise). */
typedef struct pd_unipc_args {
    int32_t order;              /* solver_order, 1..3 */
    int32_t bh2;                /* 1: B(h) = expm1(h) ("bh2"), 0: B(h) = h ("bh1") */
    int32_t lower_order_final;  /* the last steps lower the order to the number of steps left */
    int32_t n_disable_corrector;
    const int32_t* disable_corrector; /* HOST, n_disable_corrector entries: no corrector at step i + 1 for every listed i
                                         (UniPCMultistepScheduler.disable_corrector) */
    int32_t reserved[4];
} pd_unipc_args;
/* One coefficient row per step i, fp64.  m_i = (x_i - sigma_i * eps_i) / alpha_i is the x0 prediction at step i.
 *   [0] alpha_i   [1] sigma_i
 *   [2] 1.0 when the corrector runs at step i, else 0.0
 *   [3..7]  corrector: x_c = [3] last_sample + [4] m_i + [5] m_{i-1} + [6] m_{i-2} + [7] m_{i-3}   (x_c = x_i when off)
 *   [8..11] predictor: x_{i+1} = [8] x_c + [9] m_i + [10] m_{i-1} + [11] m_{i-2}
 *   [12] predictor order   [13] corrector order (0: off)   [14], [15] zero
 * last_sample is the x_c of the previous step. */
#define PD_UNIPC_NCOEF 16
/* Host only (no engine, no GPU): rows [steps][PD_UNIPC_NCOEF] for the grid `timesteps` (sampling order, strictly
 * descending, inside [0, cfg->timesteps)), alphas_cumprod derived from cfg in fp64 as pd_make_schedule derives it (before
 * its float32 rounding). */
int pd_unipc_coefficients(const pd_config* cfg, const pd_unipc_args* u, const int64_t* timesteps, int32_t steps,
                          double* coef);
/* The fused UniPC loop: begin + steps + read-back, blocking; latents_out / per_step_out as in pd_ddim_sample.  Option
 * "graph" captures it like the DDIM loop. */
int pd_unipc_sample(pd_engine* e, const pd_sample_args* args, const pd_unipc_args* u, int32_t mem_out, float* latents_out,
                    float* per_step_out);
/* Stepwise form: pd_sample_step / _get / _set_latents / _set_guidance / _end then work as for DDIM.  PD_GET_PRED_X0 is
 * m_i of the last step, PD_GET_EPS its guided eps. */
int pd_sample_begin_unipc(pd_engine* e, const pd_sample_args* args, const pd_unipc_args* u);

/* Linear multistep solvers inside the engine's loop.  Once the grid is fixed, PLMS (PLMSSampler, ldm/models/diffusion/plms.py)
 * and DPM-Solver++ multistep (DPM_Solver.sample(method="multistep"), ldm/models/diffusion/dpm_solver/dpm_solver.py) are linear
 * in a base sample and a short history of model outputs, so one evaluation ends in one elementwise kernel driven by a
 * coefficient row computed on the host in fp64.  The device state -- a ring of three earlier model outputs and one kept
 * sample -- is fp64; only the sample and pred_x0 a row returns are rounded to fp32.  eta must be 0 and noise NULL; a stochastic
 * solver adds seeded noise through slot [14] of its rows (PD_NOISE_FROM_SEED).
 * One row = one UNet evaluation.  A row may or may not complete a sampling step: PLMS's first step takes two evaluations
 * (plms.py:227-231), so PLMS over S steps has S + 1 rows at the times t_0, t_1, t_1, t_2, ..; per_step_out still has S + 1
 * entries (x_T and the sample after every completed step), the inpainting blend and control_scales_step follow completed
 * steps, and pd_sample_step(i) indexes rows. */
#define PD_LMS_PLMS  0 /* PLMSSampler: Adams-Bashforth on eps, orders 1..4 by warm-up, pseudo improved Euler first step */
#define PD_LMS_DPMPP 1 /* DPM-Solver++ multistep (data prediction), order 1..3 */
#define PD_LMS_ROWS  2 /* the caller's own rows / row_times / n_rows */
#define PD_LMS_EULER_A 3 /* Euler ancestral (k-diffusion sample_euler_ancestral, eta = 1) in the engine's VP variables; needs
                            PD_NOISE_FROM_SEED.  With alpha = sqrt(abar), sigma = sqrt(1 - abar), s = sigma / alpha, for the step from
                            t_i to t_{i+1} (s = 0 after the last): s_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2),
                            s_down = sqrt(s_to^2 - s_up^2); one row per step with m_i = eps: [3] = alpha_to / alpha_from,
                            [4] = alpha_to (s_down - s_from), [14] = alpha_to s_up, [8] = 1 / alpha_from,
                            [9] = -sigma_from / alpha_from, flags PD_LMS_F_STEP; the last row has [14] = 0 */
#define PD_LMS_DPM_SOLVER 0 /* solver_type "dpm_solver" (diffusers "midpoint") */
#define PD_LMS_TAYLOR     1 /* solver_type "taylor" (diffusers "heun") */
typedef struct pd_lms_args {
    int32_t kind;               /* PD_LMS_* */
    int32_t order;              /* DPMPP: 1..3 */
    int32_t solver_type;        /* DPMPP: PD_LMS_DPM_SOLVER / PD_LMS_TAYLOR (the second-order update; order 3 has one form) */
    int32_t lower_order_final;  /* DPMPP: order of evaluation i is min(order, i + 1, steps - i) instead of min(order, i + 1) */
    /* DPMPP, optional, HOST [steps + 1], strictly descending, inside [0, cfg->timesteps - 1]: the model times of the `steps`
     * evaluations and, last, the point the loop lands on -- the reference's continuous grid, (t - 1/N) * 1000 of
     * model_wrapper.  log(alpha) is interpolated linearly between the integer points as NoiseScheduleVP('discrete') does, and
     * the UNet is fed the fractional time.  When NULL the grid is pd_sample_args.timesteps (int64, `steps` entries, strictly
     * descending) and the loop lands on sigma = 0 (alpha = 1), the diffusers-style grid, with a first-order last step.
     * init_latents / mask need the integer grid. */
    const double* model_times;
    const double* rows;         /* PD_LMS_ROWS: HOST [n_rows][PD_LMS_NCOEF] */
    const double* row_times;    /* PD_LMS_ROWS: HOST [n_rows] model time of every evaluation */
    int32_t n_rows;             /* PD_LMS_ROWS: rows; the rows flagged "completes a step" must number pd_sample_args.steps */
    int32_t reserved[3];
} pd_lms_args;
/* One coefficient row per evaluation i, fp64.  m_i is the model output of this evaluation: the x0 prediction
 * (x - sigma_i eps) / alpha_i with PD_LMS_F_DATA_PRED, else the guided eps.  base is the current sample x, or the kept
 * sample with PD_LMS_F_BASE_KEEP.
 *   [0] alpha_i   [1] sigma_i   [2] flags (sum of PD_LMS_F_*)
 *   [3..7]  x_next  = [3] base + [4] m_i + [5] m_{i-1} + [6] m_{i-2} + [7] m_{i-3}
 *   [8..12] pred_x0 = [8] base + [9] m_i + [10] m_{i-1} + [11] m_{i-2} + [12] m_{i-3}
 *   [13] how many of m_{i-1}, m_{i-2}, m_{i-3} the row reads (at most the rows pushed so far)
 *   [14] noise coefficient: x_next += [14] z, z the seeded normal at (PD_RNG_STEP, draw = row index), added in fp64 after the
 *        sum above (a row with [14] == 0 computes exactly what it did without the slot); pred_x0 takes no noise; a non-zero
 *        [14] needs PD_NOISE_FROM_SEED   [15] zero
 * m_{i-k} counts pushed outputs only: an evaluation without PD_LMS_F_PUSH never enters the history. */
#define PD_LMS_NCOEF 16
#define PD_LMS_F_DATA_PRED  1 /* m_i is the x0 prediction */
#define PD_LMS_F_BASE_KEEP  2 /* base is the kept sample */
#define PD_LMS_F_STORE_KEEP 4 /* keep the current sample before updating */
#define PD_LMS_F_PUSH       8 /* push m_i into the history */
#define PD_LMS_F_STEP      16 /* the row completes a sampling step (per_step_out entry, inpainting blend) */
/* Host only (no engine, no GPU): rows [n][PD_LMS_NCOEF] and row_times [n] with *n_rows = n <= steps + 1 (size both for
 * steps + 1) for the grid `timesteps` (or u->model_times, then `timesteps` may be NULL); alphas_cumprod derived from cfg in
 * fp64 as for pd_unipc_coefficients.  PLMS: a_prev of a step is alphas_cumprod at the next grid point and alphas_cumprod[0]
 * after the last (make_ddim_sampling_parameters).  PD_LMS_ROWS checks the caller's rows and copies them; with more than steps + 1 of them it fails and writes nothing (the engine
 * itself, pd_lms_sample / pd_sample_begin_lms, takes up to 4 * cfg->timesteps rows). */
int pd_lms_coefficients(const pd_config* cfg, const pd_lms_args* u, const int64_t* timesteps, int32_t steps, double* rows,
                        double* row_times, int32_t* n_rows);
/* The fused loop: begin + every row + read-back, blocking; latents_out / per_step_out as in pd_ddim_sample.  Option "graph"
 * captures it like the DDIM loop. */
int pd_lms_sample(pd_engine* e, const pd_sample_args* args, const pd_lms_args* u, int32_t mem_out, float* latents_out,
                  float* per_step_out);
/* Stepwise form: pd_sample_step(i) runs row i (i = 0 .. pd_sample_rows(e) - 1); _get / _set_latents / _set_guidance / _end work
 * as for DDIM.  PD_GET_PRED_X0 is the row's pred_x0, PD_GET_EPS its guided eps. */
int pd_sample_begin_lms(pd_engine* e, const pd_sample_args* args, const pd_lms_args* u);
/* rows of the active session (steps for DDIM / UniPC) */
int32_t pd_sample_rows(pd_engine* e);

/* schedule exactly as DDIMSampler.make_schedule derives it (cldm/ddim_hacked.py:23-52):
 * fills timesteps[S] (ascending), alphas[S], alphas_prev[S], sigmas[S], sqrt_one_minus_alphas[S] */
int pd_make_schedule(pd_engine* e, int32_t steps, float eta, int64_t* timesteps, float* alphas,
                     float* alphas_prev, float* sigmas, float* sqrt_one_minus_alphas);

/* instrumentation */
int pd_synchronize(pd_engine* e);
void* pd_stream(pd_engine* e);              /* hipStream_t the engine launches on */
/* PD_MEM_DEVICE inputs: make the engine's (non-blocking) streams wait for the work already enqueued on `producer`, the
 * hipStream_t that wrote those buffers (NULL = the default stream) -- the engine-side half of what `.to(device)` ordering
 * gives the reference (everything on torch's current stream).  Call before handing device buffers over; outputs need no
 * counterpart because every call that fills a caller buffer synchronises the engine stream before it returns. */
int pd_wait_stream(pd_engine* e, void* producer);
/* Multi-GPU: images are independent through every denoising step, so a batch shards over the GPUs of a node with
 * no per-step exchange -- one process and one engine per GPU, exactly how the reference shards its evaluation set
 * (eval/distributed.py:25-27 init_process_group, eval/evaluate_gen.py:55-57 batch_ids[rank::world_size]).  The one collective
 * is an all-gather of the final latents over an RCCL communicator the engine owns (librccl is opened on first use):
 *   rank 0: pd_comm_new_id(id) and hands the 128 bytes to every rank by any host channel (file, pipe, MPI, torch.distributed);
 *   every rank: pd_comm_init(e, id, world, rank) (collective: returns once all ranks have joined), sample its shard, then
 *   pd_comm_all_gather(e, my_latents, all_latents, count, mem): all_latents[world][count] in rank order, equal `count` on
 *   every rank (pad ragged shards).  Without a communicator the gather is a copy (world 1). */
#define PD_COMM_ID_BYTES 128
int pd_comm_new_id(uint8_t id[PD_COMM_ID_BYTES]);
int pd_comm_init(pd_engine* e, const uint8_t id[PD_COMM_ID_BYTES], int32_t world, int32_t rank);
int pd_comm_world(pd_engine* e, int32_t* world, int32_t* rank);
int pd_comm_all_gather(pd_engine* e, const float* send, float* recv, int64_t count, int32_t mem);
int pd_comm_destroy(pd_engine* e); /* also done by pd_engine_destroy */
/* Tuning / instrumentation knobs (defaults are the measured best; tests and tools/ flip them for A/B runs).  Every knob belongs to the
 * engine it is set on: nothing is process-wide.  The list below has every key of the engine's option table (csrc/options.h, walked by
 * pd_option_info) in the table's order, each with its default.  Tile-count options -- "splitk_tiles", "dense_tiles", "conv_patch2_tiles",
 * "patch_split_tiles", "patch_split_fill" -- are given per 256 CUs: the engine stores and reports the value as given and scales it by
 * ncu / 256 (stat "ncu") where the dispatch plan reads it.
 *   "verbose" (0; 1: workspace sizes; 2: one stderr line per contraction launch saying which kernel family / tile / split-K count it takes),
 *   "profile" (a command rather than a stored knob: HIP events around every contraction launch from now on, see pd_profile_read; 0),
 *   "two_streams" (ControlNet on a second stream beside the UNet encoder, default 1),
 *   "cfg_share" (classifier-free guidance feeds both halves of the doubled batch the same latent and timestep, ddim_hacked.py:189-192, and
 *   -- unless pair_uncond / query_uncond say otherwise -- the same example pair and query: the layers in front of the first
 *   cross-attention (conv_in, the first ResBlock, the first SpatialTransformer up to attn2.to_q, in the UNet and in the ControlNet)
 *   run once on the B samples the halves have in common instead of twice; exact, default 1; stat "cfg_shared" tells whether the
 *   last evaluation did: bit 0 UNet, bit 1 ControlNet; bit 2: guess mode under guidance ran the ControlNet on the conditional half only,
 *   as pipeline_prompt_diffusion.py:1220-1224 does, instead of on the doubled batch with the unconditional residuals zeroed afterwards),
 *   "graph" (pd_ddim_sample captures its step loop in a hipGraph and replays it on later calls with equal arguments, 0),
 *   "conv_patch" (LDS-patch conv3x3 kernel, 1), "conv_patch2" / "conv_patch2_tiles" (its wave-specialised second generation in the 2-byte modes, for
 *   launches of at least that many blocks and every split launch, 1 / 768), "patch4" (the
 *   fourth generation -- 4 waves per block, one per SIMD, 32x32x16 MFMAs, LDS-DMA operands -- for every unsplit 2-byte patch conv, 1;
 *   bit-identical to the others), "patch_split" / "patch_split_tiles" (that kernel with the channel chunks
 *   split over 2-4 slices when it has fewer tiles than CUs but at least this many, 1 / 64), "patch_split_fill" (the slices are chosen to
 *   reach about this many blocks, 256), "patch_split_min" (at least this many 128-byte channel chunks per slice, 4; values below 1 are
 *   refused), "gn_fuse" (GroupNorm applied while the patch is staged, 0),
 *   "ln_fuse" (norm1 / norm2 of a transformer block folded into the to_q/k/v and attn2.to_q GEMMs, row statistics carried
 *   from the producing GEMM's epilogue: -1 = on in the 2-byte modes and off in the fp32-storage modes, 0 / 1 forced),
 *   "gn_single" (single-kernel LDS-slab GroupNorm where a sample's group bundle fits, 1), "gn_reg" (its register-resident
 *   form -- one block per (sample, group), the group's slab in registers, one barrier -- for 2-byte tensors of 64 / 256 / 1024 pixels, 1),
 *   "big_tile" / "wide_tile" (256x160 / 256x320 GEMM tiles, 1), "dense_k" / "dense_tiles" (8-wave unsplit tile for
 *   linear layers with at most that many K steps, 40 / 128), "short_k" (8-wave 128x160 tile at 16 waves per CU for
 *   linear layers with at most that many K steps, 20), "splitk_tiles" (split K below this many tiles, 256), "splitk_max" (into at most
 *   this many slices, 16), "splitk_big" (a split-K conv3x3 of at least 1024 rows on 256x160 tiles where tiles x slices still give every CU a
 *   block, 0), "splitk_fused" (in-kernel split-K finalize, 0), "tile192" (256x192 GEMM tile for widths that divide by 192 but not by
 *   160: the MMDiT's 1536 / 4608 / 6144, 1), "gemv" (weight-streaming kernel for a Linear over <= 4 fp32 rows with >= 4096
 *   outputs: the MMDiT modulation matrix, 1),
 *   "sd3_fp8" (SD3 path, 2-byte modes: 0 off; 1 the projections fed by an AdaLN output -- q/k/v of both streams, ff / ff_context
 *   net.0 -- take e4m3 operands with one scale per token and per output channel on the block-scaled K = 128 MFMA; 2 also the
 *   feed-forward-out projections, their input stored as e4m3 under a row bound; default 0),
 *   "attn_legacy" (single-buffered attention kernel, 0),
 *   "st_fuse" (320-channel SpatialTransformer blocks: st_front / st_tail fused kernels in the 2-byte modes, 1),
 *   "ring" / "ring_tile" / "ring_geglu" (gemm_ring.hip: linear layers over 2-byte operands with at most that many 64-element K steps
 *   take the persistent LDS-DMA ring GEMM, 80 / its tile -1 auto, 0 = 128x160, 1 = 256x160 / GEGLU projections too, 1; results are
 *   bit-identical to the igemm tiles'), "ring_small" (small-M linear layers -- at most a quarter chip of 128x160 tiles, the 8x8 level's M = 1024 --
 *   on 64x80 ring tiles without split-K slabs and a finalize pass: 0 off, d = where the 128x160 grid fills at most 1/d of the chip, 4), "ring_pp" (its ping-pong form -- two wave groups half a K step apart -- for K >= 2560 and for one
 *   256-row tile per CU, 1; bit-identical), "slab_gn" (a ResBlock conv1 that runs split-K hands its fp32 slabs to the single-kernel
 *   GroupNorm that reads them instead of running a finalize pass, 1; bit-identical), "ups_fold" / "ups_fold_tiles" (2-byte modes: a UNet decoder Upsample conv --
 *   conv3x3 of a nearest-x2 upsampled tensor, bias only, source height and width multiples of 16 -- runs as four 2x2-tap phase
 *   convolutions over the source with folded weights, conv_upfold.hip, 4/9 of the products, when its phase grid has at least that many
 *   blocks: 1 / -1 = three quarters of the CUs, the block count at which a patch conv runs unsplit.  Not bit-identical to the nine-tap
 *   path: every folded weight is rounded once more; stat "ups_fold_launches" counts the launches that took it),
 *   "vae_flash" (2-byte modes: the first stage's mid-block attention on the single-head flash kernel, vae_attention.hip, instead of
 *   the materialised [N, N] scores: -1 = per VAE -- never for the SD1.5 first stage; for SD3's VAE where the score buffers would pass 2 GiB
 *   (past about 1100^2 pixels; below that the materialised launches measure faster) or h * w is no multiple of 8; 0 / 1 force both.  The
 *   fp32-storage modes always materialise; stat "vae_flash_launches" counts the launches that took the kernel),
 *   "gemm_tile" / "gemm_splitk" (test surface, -1 / -1 = the plan's own: the tile -- 0 = 128x160, 1 = 256x160, 2 = 128x160 on 8 waves,
 *   3 = 256x320, 4 = 256x192 -- and the K slices -- 1 never, n >= 2 that many, at most one per K step -- of every launch the dispatch
 *   sends to the implicit-GEMM family.  A launch the kernels do not have in that form is then an error: a split GEGLU or V^T launch; the
 *   256x192 tile on a conv; and every tile the launcher would replace by another -- 2 / 3 / 4 in the fp32-storage modes, which have 0 and
 *   1; 256x320 with a gate, a row remap, tanh- or erf-GELU, or on a conv (256x160 runs there); 2 / 3 / 4 on a split launch.  The plan's
 *   own tile requests are mapped in the same way without an error; stat "gemm_tile" reports the tile that ran.  The defaults leave every plan as it is). */
int pd_set_option(pd_engine* e, const char* key, int64_t value);
/* The value an option holds now, as pd_set_option stored it (0 / 1 for the on / off knobs; "profile": whether the brackets are on), so a
 * caller can save and restore a knob without knowing its default. */
int pd_get_option(pd_engine* e, const char* key, int64_t* value);
/* Row `index` of the option table: its key (a static string) and its default.  Needs no engine; non-zero past the last row. */
int pd_option_info(int32_t index, const char** key, int64_t* default_value);
/* "ncu" (compute units of the engine's device, to which the chip-fill rules of the dispatch are scaled; the option defaults assume 256),
 * "graph_captures" / "graph_replays" (step loops captured / replayed from a captured graph since the engine was created),
 * "workspace_bytes", "side_workspace_bytes" (the workspace of everything outside a sampling step -- first stage, HED, text encoders, SD3's VAE:
 * it grows to the largest call so far and holds that call's intermediates, I/O staging and 64 MiB of slack), "vae_flash_launches", "weight_bytes", "launches" (engine launches, split-K finalize passes not counted), "ring_launches" / "gn_from_slabs" / "ups_fold_launches"
 * (of which: gemm_ring.hip / GroupNorm fed by split-K slabs / the four-phase upsample conv), "steps", "event_overhead_ns", "cfg_shared" (see option "cfg_share"),
 * "gn_kernel" (which kernel the engine's last GroupNorm launch took: PD_GN_TWO_PASS = gn_stats + gn_apply, PD_GN_LDS_SLAB = the
 * single LDS-slab kernel, PD_GN_REGISTER = the register-resident kernel of the 2-byte modes; 0 before the first launch.  The choice
 * depends on the storage type, H * W, C / 32, a 100 KB LDS budget and the options "gn_single" / "gn_reg"; pd_op_groupnorm and
 * pd_op_groupnorm_slabs set it, so a test can assert that a shape ran on the kernel it was chosen for),
 * "gemm_family" (which kernel family the engine's last convolution / linear launch took, PD_GEMM_* in the order of the names the
 * option "verbose" 2 dispatch trace prints: the weight-streaming GEMV, the LDS-patch conv3x3 generations 1 / 2 / 4, the ring GEMM, the
 * implicit GEMM, the four-phase upsample conv; -1 before the first launch.  pd_op_conv2d and pd_op_linear set it through the same dispatch as the network, so a
 * test can assert that an option setting put a shape on the kernel it names),
 * "gemm_tile" / "gemm_splitk" (the tile of the instantiation that launch ran, as option "gemm_tile" numbers them -- not the plan's request
 * where the launcher maps it to another; 0 outside the implicit-GEMM family -- and its K or channel-chunk slices),
 * "gemm_ring_tile" (a ring GEMM launch: its tile, 0 = 128x160, 1 = 256x160, 2 / 3 their ping-pong forms, 4 = 64x80; -1 otherwise),
 * "attn_kernel" (which kernel family the engine's last multi-head attention launch took: PD_ATTN_GENERIC = attn_kernel, every mode,
 * head dim, causal mask and relative-position bias; PD_ATTN_PIPELINED = the double-buffered attn2_kernel of the 2-byte modes, which
 * takes every launch without mask and bias unless option "attn_legacy" is 1; 0 before the first launch) */
#define PD_ATTN_GENERIC 1
#define PD_ATTN_PIPELINED 2
#define PD_GN_TWO_PASS 1
#define PD_GN_LDS_SLAB 2
#define PD_GN_REGISTER 3
#define PD_GEMM_GEMV 0
#define PD_GEMM_PATCH1 1
#define PD_GEMM_PATCH2 2
#define PD_GEMM_PATCH4 3
#define PD_GEMM_RING 4
#define PD_GEMM_IGEMM 5
#define PD_GEMM_UPFOLD 6
int64_t pd_get_stat(pd_engine* e, const char* key);
/* Per-launch timing: while option "profile" is 1 the engine brackets every contraction launch with HIP
 * events on its stream.  klass 0 = igemm_kernel on a conv3x3, 1 = igemm_kernel / rgemm_kernel on a conv1x1/linear,
 * 2 = attention, 3 = the conv3x3 patch kernels (all generations), 4 = st_front / st_tail, 5 / 6 / 7 = pd_canny's suppression, sweep and
 * emit kernels, -1 = all.  One bracket = one launch (split-K finalize excluded).
 * Returns summed device time, launch count and algorithmic FLOPs (2*M*N*K, logical channel counts).  The elapsed time of
 * a bracket around an empty one-block kernel, calibrated when "profile" is switched on (stat "event_overhead_ns"), is
 * taken off every bracket. */
int pd_profile_read(pd_engine* e, int32_t klass, double* total_ms, int64_t* n_launches, double* flops);
int pd_profile_dump(pd_engine* e, const char* csv_path); /* one row per profiled launch */
/* Micro-benchmark hook used by bench.py's roofline leg: times `iters` launches of the dominant
 * conv3x3 implicit-GEMM kernel (Cin->Cout at HxW, batch Bf) with HIP events on the engine
 * stream; returns average ms per launch in *ms. */
int pd_bench_conv3x3(pd_engine* e, int32_t Bf, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     int32_t iters, float* ms);

/* Cond stage (replaces FrozenCLIPEmbedder.forward after tokenisation, ldm/modules/encoders/modules.py:118-128, and
 * text_encoder(ids)[0] in PromptDiffusionPipeline.encode_prompt, pipeline_prompt_diffusion.py:308-487): token ids
 * [B, context_len] int32 -> last_hidden_state [B, context_len, context_dim] fp32.  mem: PD_MEM_HOST / PD_MEM_DEVICE for both
 * buffers.  Needs the cond_stage_model.transformer.text_model.* weights (pd_text_weights_missing() == 0). */
int pd_text_encode(pd_engine* e, const int32_t* ids, int32_t B, int32_t mem, float* out);
/* clip_skip k > 0 (pipeline_prompt_diffusion.py:398-413): the hidden state after block text_layers - k, passed through
 * final_layer_norm (= hidden_states[-(k+1)] of transformers' CLIPTextModel); k = 0 is pd_text_encode */
int pd_text_encode_ex(pd_engine* e, const int32_t* ids, int32_t B, int32_t mem, int32_t clip_skip, float* out);
int pd_text_weights_missing(pd_engine* e);

/* Same for one Linear / conv1x1 layer ([M,K] x [N,K]^T, optional residual add) in isolation. */
int pd_bench_linear(pd_engine* e, int32_t M, int32_t K, int32_t N, int32_t residual, int32_t iters, float* ms);
/* The first stage's mid-block attention product alone, softmax(q k^T C^-0.5) v with one head over C channels for B samples of N tokens
 * (N a multiple of 8) on random data: flash 1 = the single-head flash kernel, 0 = the three launches per sample through the [N, N] score
 * buffers; ms per call over `iters` back-to-back calls, score_bytes (may be NULL) = the bytes of those buffers. */
int pd_bench_vae_attention(pd_engine* e, int32_t B, int32_t N, int32_t C, int32_t flash, int32_t iters, float* ms, int64_t* score_bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * SD3 / MMDiT variant of the path.  Replaces, per denoising step,
 *     SD3PromptDiffusionModel.forward                       promptdiffusioncontrolnet_sd3.py:362-483
 *     self.transformer(..., block_controlnet_hidden_states)  promptdiffusioncontrolnetpipeline_sd3.py:1226-1234
 *     CFG + scheduler.step (FlowMatchEuler)                  promptdiffusioncontrolnetpipeline_sd3.py:1237-1243
 * The block arithmetic lives in diffusers (absent offline): PARITY UNPINNED, checked against oracle/sd3_oracle.py only.
 * Parameter names are diffusers' state-dict names under the prefixes "transformer." (SD3Transformer2DModel) and
 * "controlnet." (SD3PromptDiffusionModel).  The example-pair / query conditions arrive as VAE latents: pd_sd3_down_proj is the
 * Conv2d(6, 3) half of encode_support_pair (promptdiffusioncontrolnet_sd3.py:189-198); vae.encode stays with the caller.
 * Not built: use_pos_embed = False (the ControlNet fed pre-embedded tokens, which the reference's own pipeline never does),
 * joint_attention_kwargs / LoRA scale. */
typedef struct pd_sd3_config {
    int32_t in_channels;        /* 16 */
    int32_t out_channels;       /* 16 */
    int32_t patch_size;         /* 2 */
    int32_t heads;              /* 24 (SD3-medium); hidden = heads * head_dim */
    int32_t head_dim;           /* 64 */
    int32_t layers;             /* transformer blocks (24); the last one is context_pre_only */
    int32_t cn_layers;          /* ControlNet blocks (reference default 18, promptdiffusioncontrolnet_sd3.py:59); 0: no ControlNet */
    int32_t joint_dim;          /* joint_attention_dim 4096 */
    int32_t pooled_dim;         /* pooled_projection_dim 2048 */
    int32_t pos_embed_max_size; /* 192: side of the transformer's sin/cos table "transformer.pos_embed.pos_embed" */
    int32_t cn_pos_embed_max_size; /* the ControlNet's own table (promptdiffusioncontrolnet_sd3.py:102 default 96); 0: same */
    int32_t cn_zero_pooled;     /* force_zeros_for_pooled_projection (promptdiffusioncontrolnet_sd3.py:108, pipeline :1164-1168):
                                   the ControlNet sees zero pooled projections; 0: cn_pooled, or pooled when that is NULL */
    int32_t qk_norm;            /* 0: none; 1: "rms_norm" -- RMSNorm(head_dim, eps 1e-6) on the queries and keys of every head
                                   (attn.norm_q / norm_k / norm_added_q / norm_added_k), promptdiffusioncontrolnet_sd3.py:105,140 */
    uint32_t dual_mask;         /* bit i: transformer block i carries attn2, a second attention over the image tokens alone
                                   (dual_attention_layers, :104,141; norm1.linear then has 9 chunks) */
    uint32_t cn_dual_mask;      /* the same for the ControlNet's blocks */
    int32_t cn_single;          /* 1: the ControlNet consists of SD3SingleTransformerBlocks (joint_attention_dim = None, :147-160): no
                                   context_embedder, no context stream; its blocks see the image tokens alone */
} pd_sd3_config;

typedef struct pd_sd3_args {
    int32_t batch;            /* B: rows of every tensor below (<= 32 per call) */
    int32_t height, width;    /* latent size (multiples of patch_size) */
    int32_t context_len;      /* S tokens of `context` */
    int32_t mem;              /* PD_MEM_HOST / PD_MEM_DEVICE of all tensor pointers (timestep is always host) */
    float conditioning_scale; /* controlnet_conditioning_scale */
    const float* latents;     /* [B, C, H, W] */
    const float* timestep;    /* [B] (sigma * 1000), host */
    const float* context;     /* [B, S, joint_dim]  encoder_hidden_states */
    const float* pooled;      /* [B, pooled_dim]    pooled_projections */
    const float* cond;        /* [B, C, H, W] controlnet_cond latents, or NULL: transformer alone */
    const float* pair;        /* [B, C, H, W] controlnet_example_pair_cond latents */
    const float* cn_pooled;   /* [B, pooled_dim] controlnet_pooled_projections, or NULL (see cn_zero_pooled) */
    int64_t reserved[3];
} pd_sd3_args;

/* Registers the SD3 networks' parameters on an existing engine (any pd_config; the UNet path keeps working) and allocates
 * their weights.  Once per engine. */
int pd_sd3_configure(pd_engine* e, const pd_sd3_config* cfg);
int pd_sd3_weights_missing(pd_engine* e);
/* One evaluation: velocity [B, out_channels, H, W] (fp32, args->mem) = transformer(latents | ControlNet residuals). */
int pd_sd3_forward(pd_engine* e, const pd_sd3_args* args, float* v_out);
/* ControlNet alone (the model-level call): residual i as [B, (H/p)(W/p), hidden] fp32, i in [0, cn_layers)
 * (controlnet_block_samples); pooled projections = cn_pooled, or pooled when that is NULL -- cn_zero_pooled is the
 * pipeline's choice and does not apply here. */
int pd_sd3_control(pd_engine* e, const pd_sd3_args* args, int32_t index, float* out);
/* The whole loop: sigmas[steps + 1] (host, descending, last = 0 for a full schedule); guidance > 1 runs the doubled batch
 * [negative ; positive]: context / pooled / cn_pooled then hold 2B rows, latents / cond / pair B rows.
 * step_scales: per-step conditioning scale [steps] (host) = controlnet_conditioning_scale * controlnet_keep[i]
 * (pipeline :1155-1162, :1202-1208), or NULL: args->conditioning_scale at every step; a step with scale 0 skips the
 * ControlNet (its residuals would be all zero).  latents_out: [B, C, H, W]. */
int pd_sd3_sample(pd_engine* e, const pd_sd3_args* args, const float* sigmas, int32_t steps, float guidance,
                  const float* step_scales, float* latents_out);
/* Img2img, inpainting and seeded noise inside that loop (diffusers' SD3 img2img pipeline and the 16-channel path of its SD3
 * inpainting pipeline -- absent offline, so PARITY UNPINNED like the rest of the SD3 path).  sigma_0 .. sigma_steps are the
 * `sigmas` of the call: truncating the grid by `strength` is the caller's (the loop just gets the tail), and so is
 * controlnet_keep over the remaining steps (step_scales).  eps [B, C, H, W] is `noise` when set, else args->latents, else -- with
 * PD_XT_FROM_SEED, where both must be NULL -- the engine's draw at (PD_RNG_XT, draw 0, sample_base + b, element), "Seeded noise"
 * above, evaluated inside the kernel that consumes it: no eps tensor exists then.
 *   init_latents  z0 [B, C, H, W] = (vae.encode(image) - shift_factor) * scaling_factor.  The loop starts from
 *                 x = sigma_0 eps + (1 - sigma_0) z0 (FlowMatchEulerDiscreteScheduler.scale_noise), or from eps itself with
 *                 PD_INIT_PURE_NOISE.  NULL: the loop starts from eps (with PD_XT_FROM_SEED: start latents the engine draws).
 *   mask          m [B, 1, H, W], needs init_latents; 1 = repaint, 0 = keep, values in between allowed, broadcast over the
 *                 channels.  After the Euler update of step i to x' the state becomes (1 - m) k_i + m x' with
 *                 k_i = (1 - sigma_{i+1}) z0 + sigma_{i+1} eps -- the same eps at every step; k is z0 itself at sigma = 0.
 * All of it is fp32, every operation rounded on its own in the written order (no FMA), so a NumPy float32 restatement has the
 * same bits; the CFG + Euler update in front of it is the plain loop's own code.  One launch (sd3_update_kernel) per step and one
 * for the start state write the state and both halves of the next step's doubled input: no device-to-device copies.
 * A `loop` that is NULL or sets nothing is pd_sd3_sample, kernel for kernel. */
typedef struct pd_sd3_loop_args {
    const float* init_latents; /* [B, C, H, W] in args->mem, or NULL */
    const float* mask;         /* [B, 1, H, W] in args->mem, or NULL */
    const float* noise;        /* [B, C, H, W] in args->mem, or NULL: eps is args->latents (or the seeded draw) */
    int32_t flags;             /* PD_INIT_PURE_NOISE (needs init_latents) | PD_XT_FROM_SEED (noise and args->latents NULL) */
    int32_t reserved0;
    int64_t reserved[4];
} pd_sd3_loop_args;
int pd_sd3_sample_ex(pd_engine* e, const pd_sd3_args* args, const pd_sd3_loop_args* loop, const float* sigmas, int32_t steps,
                     float guidance, const float* step_scales, float* latents_out);
/* SD3PromptDiffusionModel.down_proj (promptdiffusioncontrolnet_sd3.py:114, :189-194): Conv2d(6, 3, kernel 3, padding 1) over
 * pair = cat([cond, gt], 1) [B, 6, H, W] -> out [B, 3, H, W] (fp32, `mem` as in pd_sd3_args). */
int pd_sd3_down_proj(pd_engine* e, const float* pair, int32_t B, int32_t H, int32_t W, int32_t mem, float* out);

/* ---------------------------------------------------------------------------------------------------------------
 * SD3 text encoders: what the reference's encode_prompt runs (promptdiffusioncontrolnetpipeline_sd3.py:238-545) -- CLIP-L and CLIP-G
 * (transformers' CLIPTextModelWithProjection) and the T5 encoder (T5EncoderModel).  Tokenisation stays with the caller: the boundary
 * takes token ids.  Parameter names are the checkpoint's: "text_encoder.text_model.*" + "text_encoder.text_projection.weight", the same
 * under "text_encoder_2.", and "text_encoder_3.shared.weight", "text_encoder_3.encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight",
 * "...block.0.layer.0.SelfAttention.relative_attention_bias.weight", "...layer.0.layer_norm.weight",
 * "...layer.1.DenseReluDense.{wi_0,wi_1,wo}.weight", "...layer.1.layer_norm.weight", "text_encoder_3.encoder.final_layer_norm.weight"
 * (the tied "text_encoder_3.encoder.embed_tokens.weight" is not a parameter: loaders skip it).  The residual streams of all three
 * encoders are fp32 in every precision mode; T5's gated product is formed in fp32 and saturates to +-65504 on an fp16 store.
 * Whether fp16 is usable with real T5-XXL weights is unmeasured: prefer bf16 for the T5 slot. */
#define PD_CLIP_ACT_QUICK_GELU 0   /* CLIP-L */
#define PD_CLIP_ACT_GELU 1         /* CLIP-G: exact (erf) GELU */
typedef struct pd_sd3_clip_config {
    int32_t vocab, hidden, ff, heads, layers;   /* layers == 0: this encoder is absent; hidden / heads must be 64 */
    int32_t max_positions;                       /* 77 */
    int32_t proj_dim;                            /* rows of text_projection.weight [proj_dim, hidden] (no bias) */
    int32_t eos_token_id;                        /* 2 (both SD3 configs): pooled row = argmax(ids); else the first ids == eos_token_id */
    int32_t act;                                 /* PD_CLIP_ACT_* */
} pd_sd3_clip_config;
typedef struct pd_sd3_t5_config {
    int32_t vocab, d_model, d_kv, heads, d_ff, layers;   /* layers == 0: absent; d_kv must be 64; heads * d_kv need not equal d_model */
    int32_t num_buckets, max_distance;                    /* relative_attention_num_buckets 32, relative_attention_max_distance 128 */
    float eps;                                            /* layer_norm_epsilon 1e-6 */
} pd_sd3_t5_config;
typedef struct pd_sd3_text_config {
    pd_sd3_clip_config clip_l, clip_g;
    pd_sd3_t5_config t5;
    int32_t joint_dim;       /* row width of prompt_embeds: >= clip_l.hidden + clip_g.hidden, and == t5.d_model when T5 is present */
    int32_t reserved[3];
} pd_sd3_text_config;
typedef struct pd_sd3_text_args {
    int32_t batch;               /* B */
    int32_t t5_len;              /* Lt in [1, 512] (ignored without a T5 encoder) */
    int32_t clip_skip;           /* >= 0; the hidden state is hidden_states[-(clip_skip + 2)], without the final LayerNorm */
    int32_t mem;                 /* PD_MEM_HOST / PD_MEM_DEVICE of the ids and of both outputs */
    const int32_t* ids_clip_l;   /* [B, 77] */
    const int32_t* ids_clip_g;   /* [B, 77] */
    const int32_t* ids_t5;       /* [B, Lt] */
    int64_t reserved[3];
} pd_sd3_text_args;
/* Registers the encoders' parameters (registry group of their own) on an existing engine and allocates their weights.  Once per engine;
 * an engine that never calls it is unchanged. */
int pd_sd3_text_configure(pd_engine* e, const pd_sd3_text_config* cfg);
int pd_sd3_text_weights_missing(pd_engine* e);
/* encode_prompt after tokenisation.  prompt_embeds [B, 77 + Lt, joint_dim] fp32: rows 0..76 hold the CLIP-L hidden state in columns
 * [0, hidden_l), CLIP-G's in [hidden_l, hidden_l + hidden_g) and zeros up to joint_dim; rows 77.. hold T5's last_hidden_state.  Without
 * a T5 encoder the output is [B, 77, joint_dim] (the reference appends its zero block of 77 more rows itself).  pooled
 * [B, proj_l + proj_g] fp32 = cat(text_embeds_l, text_embeds_g).  Both CLIP encoders must be configured. */
int pd_sd3_encode_prompt(pd_engine* e, const pd_sd3_text_args* args, float* prompt_embeds, float* pooled);
/* One encoder alone.  which 0 / 1 (CLIP-L / CLIP-G): ids [B, 77] -> hidden [B, 77, hidden] (as above) and pooled [B, proj_dim], either
 * may be NULL; which 2 (T5): ids [B, len] -> hidden [B, len, d_model], pooled must be NULL.  len is read for T5 only. */
int pd_sd3_text_encoder(pd_engine* e, int32_t which, const int32_t* ids, int32_t B, int32_t len, int32_t clip_skip, int32_t mem,
                        float* hidden, float* pooled);
/* T5Attention._relative_position_bucket (bidirectional) on the host: out[i] = bucket of relative position (key - query) = i - (L - 1)
 * for i in [0, 2 L - 1).  Needs no engine and no GPU. */
int pd_t5_relative_buckets(int32_t L, int32_t num_buckets, int32_t max_distance, int32_t* out);

/* ---- SD3's VAE (diffusers AutoencoderKL: 16 latent channels, no quant convs, scaling and shift) ----
 * The three places the reference's SD3 pipeline calls its VAE (promptdiffusioncontrolnetpipeline_sd3.py): vae.encode(control_image)
 * .latent_dist.sample(), then (z - shift) * scaling (:1132-1133); the same on the down-projected example pair (:1112-1115); and
 * vae.decode(latents / scaling + shift) (:1271-1273).  Same layers as the SD1.5 first stage (pd_vae_decode / pd_vae_encode), with a
 * description of its own; parameters are registered under diffusers' names, prefix "vae." (encoder.down_blocks.{i}.resnets.{j}.*,
 * {encoder,decoder}.mid_block.{resnets.{0,1},attentions.0.{group_norm,to_q,to_k,to_v,to_out.0}}, decoder.up_blocks.{i}.*,
 * conv_norm_out, ...; to_q / to_k / to_v / to_out.0 are Linear [C, C]).  In the 2-byte modes the mid-block attention runs the single-head flash
 * kernel (vae_attention.hip) where its score buffers would pass 2 GiB or h * w is no multiple of 8, and whenever option "vae_flash" is 1. */
typedef struct pd_sd3_vae_config {
    int32_t ch, num_levels, ch_mult[PD_MAX_LEVELS], num_res_blocks, z_channels, out_ch;   /* 128, 4, {1,2,4,4}, 2, 16, 3 */
    int32_t encoder;                        /* 0: decoder only */
    int32_t quant_conv, post_quant_conv;    /* 0 for SD3 (use_quant_conv / use_post_quant_conv false) */
    double scaling_factor, shift_factor;    /* 1.5305, 0.0609 */
} pd_sd3_vae_config;
/* Registers the VAE's parameters (registry group of their own) on an existing engine and allocates their weights.  Once per engine; an
 * engine that never calls it is unchanged. */
int pd_sd3_vae_configure(pd_engine* e, const pd_sd3_vae_config* cfg);
int pd_sd3_vae_weights_missing(pd_engine* e);
/* sizeof(pd_sd3_vae_config) and the byte offsets of scaling_factor / shift_factor as this library was compiled: what a binding checks
 * its own struct against.  Needs no engine and no GPU. */
int pd_sd3_vae_config_layout(int32_t* size, int32_t* off_scaling, int32_t* off_shift);
/* latents [B, z, h, w] -> images [B, out_ch, 8h, 8w] (2^(num_levels - 1) per side), fp32 in `mem` space: decode(latents / scaling +
 * shift); raw != 0: decode(latents).  Any h, w >= 1 in the 2-byte modes; the fp32-storage modes (and option "vae_flash" 0) need h * w a multiple of 8. */
int pd_sd3_vae_decode(pd_engine* e, const float* latents, int32_t B, int32_t h, int32_t w, int32_t mem, int32_t raw, float* images);
/* images [B, out_ch, H, W] (H, W multiples of 8) -> PD_VAE_MEAN / PD_VAE_SAMPLE: (z - shift) * scaling, [B, z, H/8, W/8] (raw != 0: z
 * itself); PD_VAE_MOMENTS: the unscaled [B, 2z, H/8, W/8] moments.  noise as in pd_vae_encode (NULL with PD_VAE_SAMPLE: the seeded draw). */
int pd_sd3_vae_encode(pd_engine* e, const float* images, int32_t B, int32_t H, int32_t W, int32_t mem, int32_t what, const float* noise,
                      int32_t raw, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PDENGINE_H */
