// pdengine: engine object behind the C ABI of include/pdengine.h (host-side orchestration).
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pdengine.h"
#include "options.h"
#include "pd_common.h"

void pd_set_error(const char* fmt, ...);
// timestep_embedding (util.py:154-174) of n timesteps on the host: [cos | sin] halves, fp32 like the reference
void pd_host_timestep_embedding(const int64_t* t, int n, int dim, std::vector<float>& out);
// its sibling for fractional model times (the reference's timesteps[:, None].float() * freqs): the same bits for integer values
void pd_host_timestep_embedding_f(const double* t, int n, int dim, std::vector<float>& out);
// rows [n_rows][PD_LMS_NCOEF] and the model time of every row for a linear multistep loop over n steps (multistep.cpp)
int pd_lms_table(const pd_config& cfg, const pd_lms_args& u, const int64_t* ts, int n, std::vector<double>& rows, std::vector<double>& times);
// coefficient rows [n][PD_UNIPC_NCOEF] of the fused UniPC loop (multistep.cpp; pd_unipc_coefficients)
// bounds [out_size][2] and kk [out_size][*ksize] of one axis (image_host.cpp; LANCZOS, BOX or BICUBIC); non-zero with the error set on a refusal
int pd_resample_axis(int in_size, int out_size, int filter, int* ksize, std::vector<int32_t>& bounds, std::vector<int32_t>& kk);
int pd_unipc_table(const pd_config& cfg, const pd_unipc_args& u, const int64_t* ts, int n, std::vector<double>& coef);

#define HIP_OK(expr)                                                                            \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            pd_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)
#define PD_TRY(expr)            \
    do {                        \
        int _r = (expr);        \
        if (_r) return _r;      \
    } while (0)
// One launch protocol for every enqueue function of engine `eng`: nothing in a dry pass, nothing after a workspace overflow, `n`
// launches counted in stat "launches", an event bracket of profiling class `k` around them (k < 0: none); a non-zero `call` sets the
// printf-style message that follows and returns 1.
#define PD_LAUNCH_K(eng, n, k, call, ...)       \
    do {                                        \
        pd_engine* _pe = (eng);                 \
        if (!_pe->arena.dry) {                  \
            PD_TRY(_pe->check_arena());         \
            Bracket _br(_pe, (k));              \
            _pe->launches += (n);               \
            if (call) {                         \
                pd_set_error(__VA_ARGS__);      \
                return 1;                       \
            }                                   \
        }                                       \
    } while (0)
#define PD_LAUNCH(eng, call, ...) PD_LAUNCH_K(eng, 1, -1, call, __VA_ARGS__)

// A GEMM weight matrix [Nalloc][Kpad] in the compute type, K-contiguous, plus its fp32 bias.
struct WMat {
    void* w = nullptr;
    float* bias = nullptr;
    int N = 0;       // weight rows the kernel sees (virtual columns; GEGLU: interleaved blocks)
    int Nout = 0;    // logical output columns
    int K = 0;       // logical reduction length taps*cin_pad
    int Kpad = 0;
    int taps = 1;
    int cin = 0, cin_pad = 0;
    int fan_in = 1;
    bool geglu = false;
    // LayerNorm folded into this layer (pd_engine::fold_layernorms): W * diag(gamma), its column sums, bias + beta . W^T
    void* w_ln = nullptr;
    float* colsum = nullptr;
    float* bias_ln = nullptr;
    // conv3x3 behind a nearest-x2 upsample (pd_engine::fold_upconv): the four phase matrices [4][N][4 * cin_pad], conv_upfold.hip
    void* w_up = nullptr;
    // e4m3 copy with one scale per output row (pd_engine::sd3_quantize): the PREC_FP8 form of this layer
    void* w8 = nullptr;
    float* wscale = nullptr;
    int Kpad8 = 0;
    float wnorm_max = 0.f, bias_max = 0.f;   // max_n |W_n|_2 and max |bias|: bound of this layer's outputs from its input row's norm
};

// LayerNorm statistics handed from the GEMM that writes a residual-stream tensor to the GEMM that consumes its LayerNorm
struct LnStats {
    float* stats = nullptr;   // [rows][parts][2] {sum, sum of squares}
    int parts = 0;
    int C = 0;
    int cap_parts = 0;        // partials per row the buffer holds (producers check it before writing)
};

struct ConvW {
    WMat m;
    int cin = 0, cout = 0, k = 1, stride = 1;
    int pad_shift = 0;   // GemmParams::pad_shift: 1 = the encoder Downsample's F.pad(x, (0, 1, 0, 1)) + padding 0
    int dilation = 1;    // conv3x3 only: taps `dilation` pixels apart, padding = dilation (GemmParams::dil_m1)
};

struct ResW {
    int cin = 0, cout = 0;
    float *gn1_g = nullptr, *gn1_b = nullptr, *gn2_g = nullptr, *gn2_b = nullptr;
    ConvW conv1, conv2, skip;
    WMat emb;
    bool has_skip = false;
    float eps = 1e-5f;  // GroupNorm eps (1e-6 in the VAE's ResnetBlock)
    int emb_slot = -1;  // index into the per-net table of projected time embeddings
};

struct STW {
    int C = 0;
    float *gn_g = nullptr, *gn_b = nullptr;
    float* ln_g[3] = {nullptr, nullptr, nullptr};
    float* ln_b[3] = {nullptr, nullptr, nullptr};
    ConvW proj_in, proj_out;
    WMat qkv, out1, q2, kv2, out2, ff1, ff2;
    int kv_slot = -1;  // index into the per-net table of hoisted context K / V^T
    int ip_slot = -1;  // UNet only, set by pd_ip_adapter_configure: the block's index j among the UNet's cross-attention blocks (IpAdapterW)
    // fused tail (st_tail.hip): the block's matrices after self-attention in MFMA-fragment order + its fp32 vectors
    void* tail_w = nullptr;
    float* tail_vec = nullptr;
    void* front_w = nullptr;    // proj_in + to_q/k/v (norm1 folded) in the same order, for the fused front kernel
    float* front_vec = nullptr;
};

struct EncBlock {
    int kind = 0;  // 0 conv_in, 1 res(+attn), 2 down
    ConvW conv;
    ResW res;
    bool attn = false;
    STW st;
    int cout = 0, ds = 1;
};

struct DecBlock {
    ResW res;
    bool attn = false, up = false;
    STW st;
    ConvW upconv;
    int skip_c = 0, cout = 0;
};

struct NetW {
    WMat te0, te2;
    std::vector<EncBlock> enc;
    ResW mid0, mid2;
    STW mid1;
    // UNet only
    std::vector<DecBlock> dec;
    float *out_g = nullptr, *out_b = nullptr;
    ConvW outconv;
    // ControlNet only
    std::vector<ConvW> zero;
    ConvW mid_out;
    std::vector<ConvW> hint_pair, hint_query;
    int n_emb = 0, n_kv = 0;
    std::vector<ResW*> res_list;  // in emb_slot order
    std::vector<STW*> st_list;    // in kv_slot order
};

// AttnBlock (model.py:144-202) of the first stage's mid level: norm, fused q|k|v rows, proj_out (decoder and encoder)
struct VaeAttnW {
    int C = 0;
    float *g = nullptr, *b = nullptr;
    WMat qkv;
    ConvW proj_out;
};
// First-stage decoder: ldm/modules/diffusionmodules/model.py:546-653 + post_quant_conv (autoencoder.py:34)
struct VaeLevel {
    std::vector<ResW> blocks;
    bool up = false;
    ConvW upconv;
    int ch = 0;
};
// What a first stage is made of (the SD1.5 instance is filled from pd_config, SD3's from pd_sd3_vae_config)
struct VaeDesc {
    int z = 0, zpad = 0;                       // latent channels; round_up(z, 8): the channel width of the latent activations
    int ch = 0, num_levels = 0, ch_mult[PD_MAX_LEVELS] = {0}, num_res_blocks = 0, out_ch = 0;
    bool quant = true;                         // post_quant_conv (decoder) / quant_conv (encoder) present
    double scaling = 1.0, shift = 0.0;         // decode(z / scaling + shift); encode: (z - shift) * scaling
    bool flash_auto = false;                   // option "vae_flash" at -1: false = never, true = where the score buffers pass 2 GiB (vae_flash_on)
    bool diffusers = false;                    // parameter names: diffusers AutoencoderKL instead of ldm
    int group = 0, enc_group = 0;              // WeightGroup of the decoder / the encoder
};
struct VaeW {
    bool built = false;
    VaeDesc d;
    ConvW post_quant, conv_in, conv_out;
    ResW mid1, mid2;
    VaeAttnW attn;
    float *out_g = nullptr, *out_b = nullptr;
    std::vector<VaeLevel> levels;  // execution order (highest resolution level last)
    int top = 0;
};
// First-stage encoder (option vae_encoder): Encoder (model.py:452-544, double_z, no attention in the levels) + quant_conv
// (autoencoder.py:33); levels in module order = execution order, every level but the last ends in a Downsample
struct VaeEncLevel {
    std::vector<ResW> blocks;
    bool down = false;
    ConvW downconv;   // stride 2, pad_shift 1
};
struct VaeEncW {
    bool built = false;
    VaeDesc d;
    ConvW conv_in, conv_out, quant;
    std::vector<VaeEncLevel> levels;
    ResW mid1, mid2;
    VaeAttnW attn;
    float *out_g = nullptr, *out_b = nullptr;
    int top = 0;
};

// The tile grid of a tiled VAE call (vae_tile.cpp: vae_make_tile_plan, what pd_vae_tile_plan returns) and what one run of it holds
struct VaeTilePlan {
    bool tiled = false;
    int nrow = 0, ncol = 0, limit = 0, be = 0, nclass = 0;   // limit, be in output pixels
    std::vector<pd_vae_tile> tiles;                          // row-major
    std::vector<std::vector<int>> members;                   // per shape class: tile indices, row-major
};
struct VaeTileRun {
    std::vector<float*> res;        // per class: the tile results, fp32 [members][B][th][tw][cpad]
    long long* tile_off = nullptr;  // device tables (VaeBlendParams) ...
    int *rows = nullptr, *cols = nullptr, *origins = nullptr;   // ... origins: (y0, x0) per tile, class by class
    float* wtab = nullptr;
    std::vector<int> origin_at;     // per class: its first entry in origins
};
// non-zero with the error set when (T, f) is not accepted; p.tiled false when the size needs no tiling
int vae_make_tile_plan(int h, int w, int T, double f, int u, bool encode, VaeTilePlan& p);

// HED edge detector (pd_hed_configure, hed.cpp): annotator/hed/__init__.py Network -- the 13 conv3x3 + ReLU of the VGG-16 trunk in five
// stages (2, 2, 3, 3, 3), one conv1x1 C -> 1 score head per stage and the 5 -> 1 combine; heads and combine are fp32 vectors
struct HedW {
    bool built = false;
    ConvW conv[13];
    float* score_w[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* score_b[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float *comb_w = nullptr, *comb_b = nullptr;
};

// M-LSD line detector (pd_mlsd_configure, mlsd.cpp): annotator/mlsd/models/mbv2_mlsd_large.py MobileV2_MLSD_Large -- MobileNetV2
// features 0..13 and the decoder blocks 15..23, every BatchNorm folded into its conv by the loader
struct MlsdDw { float* w = nullptr; float* b = nullptr; int C = 0, stride = 1; };   // depthwise conv3x3 [C][9] + folded bias, fp32
struct MlsdIR {                 // InvertedResidual: (expand 1x1 + ReLU6)? -> depthwise + ReLU6 -> project 1x1 (+ x)
    bool expand = false, res = false;
    ConvW pw1, pw2;
    MlsdDw dw;
};
struct MlsdW {
    bool built = false;
    ConvW conv0;                // features.0: conv3x3 stride 2 (pad_shift 1), 4 -> 32
    MlsdIR ir[13];              // features.1 .. features.13
    ConvW a1[4], a2[4];         // BlockTypeA 15, 17, 19, 21: conv1 (deep input), conv2 (skip input)
    ConvW b1[4], b2[4];         // BlockTypeB 16, 18, 20, 22
    ConvW c1, c2, c3;           // BlockTypeC 23
};

// CLIP text transformer (text.cpp): the SD1.5 cond stage and SD3's CLIP-L / CLIP-G are this one stack
struct TextLayerW {
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    WMat qkv, out, fc1, fc2;
};
struct ClipW {
    bool built = false;
    int vocab = 0, hidden = 0, ff = 0, heads = 0, positions = 0;
    int proj_dim = 0;                      // rows of text_projection.weight; 0: no projection head (SD1.5)
    int eos_token_id = 0;                  // pooled row (pd_sd3_clip_config)
    Activation act = ACT_QUICK_GELU;       // of the MLP
    bool causal = true;                    // the text encoders' mask; false in the image tower (clip_vision.cpp)
    float eps = 1e-5f;                     // layer_norm_eps of the blocks
    WMat tok, pos, proj;
    std::vector<TextLayerW> layers;        // sized by the caller of build_clip, never resized again (Params point into it)
    float *fln_g = nullptr, *fln_b = nullptr;
};
// CLIP image tower (clip_vision.cpp; pd_clip_vision_configure): the text stack's blocks without the mask, behind a patch embedding.
// t carries the blocks, post_layernorm (fln_*) and visual_projection (proj); t.positions = P + 1
struct ClipVisionW {
    bool built = false;
    bool broken = false;                   // a weight allocation failed while it was registered: the slot is taken, every use is refused
    std::string prefix;
    pd_clip_vision_config c{};
    ClipW t;
    WMat patch;                            // patch_embedding.weight [C][3 p p] as a linear layer over the patch matrix (no bias)
    float *cls = nullptr, *pos = nullptr;  // class_embedding [C], position_embedding.weight [P + 1][C], fp32
    float *pre_g = nullptr, *pre_b = nullptr;
    int patches = 0;                       // P = (image_size / patch)^2
    int group = 0;                         // WeightGroup
};
// StableDiffusionSafetyChecker's buffers (pd_safety_configure), fp32
struct SafetyW {
    bool built = false, broken = false;    // broken: as ClipVisionW's
    int D = 0;
    float *cpt = nullptr, *spc = nullptr, *cpt_thr = nullptr, *spc_thr = nullptr;   // concept / special-care rows and thresholds
};

// IP-Adapter for the UNet (ip_adapter.cpp; pd_ip_adapter_configure): the linear ImageProjection, and to_k_ip / to_v_ip of every UNet
// cross-attention block j in diffusers' processor order (input blocks, output blocks, middle block; checkpoint id 2 j + 1).
// The image state (pd_ip_adapter_set_image): K_ip / V_ip of every block for both guidance halves in one engine-owned allocation,
// half 0 = unconditional, 1 = conditional, each [Bi][T][C_j] in the compute type.
struct IpAdapterW {
    bool built = false, broken = false;    // broken: as ClipVisionW's
    int T = 0, E = 0;                      // image tokens; width of the image embedding
    WMat proj;                             // image_proj.proj [T * D][E] + bias
    float *norm_g = nullptr, *norm_b = nullptr;
    std::vector<WMat> to_k, to_v;          // [C_j][D] each, no bias
    std::vector<STW*> blocks;              // block j
    std::vector<float> scale;              // s_j (all 1 after configure)
    int Bi = 0;                            // images of the state; 0: none set
    void* kv = nullptr;                    // the allocation (grown on demand, never shrunk)
    size_t kv_cap = 0;
    std::vector<size_t> k_off, v_off;      // byte offset of half 0 of block j; half 1 follows at + Bi * T * C_j elements
    uint64_t gen = 0;                      // bumped by every set / clear: part of the graph replay key
    bool active() const {
        if (!built || broken || Bi < 1) return false;
        for (float s : scale)
            if (s != 0.f) return true;
        return false;
    }
};
// What pd_engine::transformer adds to a block's text cross-attention: nseg equal runs of the block's output batch, run r against K[r] /
// V[r] ([Bk][T][C], kv_bs elements apart, 0 = one set for every sample of the run)
struct IpTerm {
    const void* K[2] = {nullptr, nullptr};
    const void* V[2] = {nullptr, nullptr};
    int nseg = 1, T = 0;
    long long kv_bs = 0;
    float s = 0.f;
};

// Perturbed-attention guidance (pd_set_pag) in one transformer block: the last n samples of the block's output are the perturbed
// branch, whose self-attention is the identity (attn1 = to_out(V), pag.hip).  fork: x does not hold them yet -- they begin here as
// copies of x's samples [src, src + n), and take those samples' V; otherwise they are x's own last n samples.  Their cross-attention
// (and image term) reads the context of samples [src, src + n).
struct PagTerm {
    int n = 0;
    bool fork = false;
    int src = 0;
};

// SD3's T5 encoder stack (sd3_text.cpp): no biases anywhere, RMSNorm weights only, wi = [wi_1 | wi_0] packed like a GEGLU matrix
struct T5LayerW {
    float *ln1 = nullptr, *ln2 = nullptr;
    WMat qkv, o, wi, wo;
};
struct Sd3T5W {
    bool built = false;
    pd_sd3_t5_config c{};
    WMat tok, relbias;    // shared.weight; block 0's relative_attention_bias.weight [num_buckets][heads]
    std::vector<T5LayerW> layers;
    float* fln = nullptr;
};

// SD3 / MMDiT: one JointTransformerBlock
struct Sd3BlockW {
    WMat qkv, qkv_c;     // to_q|to_k|to_v and add_q_proj|add_k_proj|add_v_proj, rows [0,D) q, [D,2D) k, [2D,3D) v
    WMat out, out_c;     // attn.to_out.0, attn.to_add_out (absent when pre_only)
    WMat ff1, ff2, ffc1, ffc2;
    int mod_off = 0, mod_c_off = 0;   // first row of norm1.linear / norm1_context.linear in the net's modulation matrix
    bool pre_only = false;            // context_pre_only (last transformer block): context gives keys / values only
    bool single = false;              // SD3SingleTransformerBlock: no context stream at all (ControlNet with joint_attention_dim = None)
    // qk_norm = "rms_norm": RMSNorm weights [head_dim] of the image / context queries and keys
    float *nq = nullptr, *nk = nullptr, *naq = nullptr, *nak = nullptr;
    // dual_attention_layers: attn2, self-attention over the image tokens (norm1.linear has 9 chunks: shift2 / scale2 / gate2 last)
    bool dual = false;
    WMat qkv2, out2;
    float *nq2 = nullptr, *nk2 = nullptr;
};
struct Sd3NetW {
    bool built = false, single = false;
    int layers = 0, pos_max = 0;
    WMat pe, pe_in, t1, t2, p1, p2, ctx_emb, mod, proj_out;
    ConvW down_proj;                  // ControlNet only: Conv2d(6, 3, 3, padding 1) of encode_support_pair
    float* pos = nullptr;             // pos_embed.pos_embed [pos_max * pos_max][D] fp32
    std::vector<Sd3BlockW> blocks;
    std::vector<WMat> zero;           // controlnet_blocks
    int mod_rows = 0, norm_out_off = 0;
};

// Param::group: the weights a family of entry points needs loaded (its *_weights_missing count, its "not loaded" refusal)
enum WeightGroup {
    GROUP_SAMPLER = 0,       // UNet + ControlNet (needed to sample)
    GROUP_VAE = 1,           // VAE decoder
    GROUP_TEXT = 2,          // SD1.5 text transformer
    GROUP_SD3 = 3,           // SD3 networks
    GROUP_VAE_ENCODER = 4,
    GROUP_HED = 5,
    GROUP_SD3_TEXT = 6,      // SD3 text encoders
    GROUP_SD3_VAE = 7,       // SD3's VAE decoder
    GROUP_SD3_VAE_ENCODER = 8,
    GROUP_MLSD = 9,
    GROUP_CLIP_VISION_0 = 10,   // the two image towers, one group each
    GROUP_CLIP_VISION_1 = 11,
    GROUP_SAFETY = 12,
    GROUP_IP_ADAPTER = 13,
};

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    int kind = 0;  // 0 fp32 vector, 1 matrix rows (linear / conv)
    // vector destination
    float* vdst = nullptr;
    bool geglu_vec = false;
    int geglu_half = 0;  // 4C for GEGLU permutation
    // matrix destination
    WMat* mat = nullptr;
    int row_off = 0;
    bool conv = false;  // OIHW source
    char init = 'w';    // recipe class for pd_init_random_weights: w, b, g(amma), e(beta)
    bool loaded = false;
    WeightGroup group = GROUP_SAMPLER;
};

struct Act {
    void* p = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    int dt = DT_F32;
    long long rows() const { return (long long)B * H * W; }
    size_t bytes() const { return (size_t)rows() * C * dt_size(dt); }
};

struct Arena {
    char* base = nullptr;
    size_t cap = 0, top = 0, peak = 0;
    bool dry = false;
    bool overflow = false;   // an allocation ran past cap: every enqueue refuses to launch until the arena is reset
    void* alloc(size_t bytes) {
        size_t a = (top + 255) & ~(size_t)255;
        top = a + bytes;
        if (top > peak) peak = top;
        if (dry) return reinterpret_cast<void*>((size_t)0x1000 + a);
        if (top > cap) { overflow = true; return base; }   // never hand out memory beyond the workspace
        return base + a;
    }
    size_t mark() const { return top; }
    void release(size_t m) { top = m; }
};

// A split-K conv whose only consumer is a single-kernel GroupNorm (resblock conv1 -> norm2 at the 16x16 / 8x8 levels) leaves its
// slabs un-summed: `allow` is set by the caller of gemm(), `active` by gemm() when it did skip the finalize pass; the slabs
// stay on the workspace stack until the caller's own mark is released.
struct SlabDefer { bool allow = false, active = false; const float* slabs = nullptr; int nslab = 0; const float* bias = nullptr; const float* rowvec = nullptr; int rowvec_stride = 0; };

// Everything a gemm() / conv() call says besides the weight, the input and the output; the defaults are a plain linear layer.
struct GemmCall {
    int stride = 1, ups = 0;                                  // conv geometry (conv() takes the stride from its ConvW); ups: nearest x2 in the gather
    Activation act = ACT_NONE;                                // (a GEGLU weight matrix implies ACT_GEGLU)
    float scale = 1.f;
    const Act* R = nullptr;                                   // residual
    const float* rowvec = nullptr; int rowvec_stride = 0;     // per-sample row vector (time embedding)
    bool a_silu = false;                                      // SiLU on the input while it is loaded
    void* VT = nullptr; int vt_begin = 0, vt_ld = 0;          // V^T side output of the columns from vt_begin on
    int ldc = 0;                                              // output row stride (0: out.C)
    const float* gn_coef = nullptr; bool gn_silu = false;     // GroupNorm applied while staging (patch conv)
    const LnStats* ln_in = nullptr; LnStats* ln_out = nullptr;   // LayerNorm of the input folded in / row statistics of the output wanted
    const float *a_scale = nullptr, *c_scale = nullptr;       // fp8 row scales of the input / the output
    const float* gate = nullptr;                              // MMDiT: gated residual, joint-buffer row remaps (GemmParams)
    int gate_stride = 0, c_sample_rows = 0, c_row_off = 0, vt_tok_off = 0, a_sample_rows = 0, a_row_off = 0;
    int pad_shift = 0;                                        // ConvW::pad_shift, set by conv()
    SlabDefer* defer = nullptr;
    int dilation = 1;                                         // ConvW::dilation, set by conv()
};

// Which kernel a gemm() call takes (pd_engine::plan_gemm): the verbose-2 dispatch trace prints exactly this.
enum GemmFamily { GEMM_GEMV, GEMM_PATCH1, GEMM_PATCH2, GEMM_PATCH4, GEMM_RING, GEMM_IGEMM, GEMM_UPFOLD };
struct GemmPlan {
    GemmFamily family = GEMM_IGEMM;
    int splitk = 1, big_tile = 0, ring_tile = 0;   // K (igemm) or channel-chunk (patch) slices; GemmParams::big_tile (igemm); launch_ring_gemm's tile (ring)
    bool fused_tile_cnt = false;  // split-K finalize in the last-arriving slice (option "splitk_fused")
    bool defer_finalize = false;  // the caller's SlabDefer is honoured: no finalize pass
    int stats_parts = 0;          // LayerNorm-statistics partials per row from this launch's own epilogue (0: none)
    bool patch() const { return family == GEMM_PATCH1 || family == GEMM_PATCH2 || family == GEMM_PATCH4; }
};
// The chip-fill rules of plan_gemm, the one place where the CU count enters the dispatch.  The tile-count options are numbers for a
// 256-CU part and are scaled here (v * ncu / 256); the fractions of the chip that grids are compared against get their names.
struct ChipFill {
    int splitk_tiles, dense_tiles, conv_patch2_tiles, patch_split_tiles, patch_split_fill;   // the options of these names, scaled
    int whole;            // a block for every CU: big_tile, wide_tile, splitk_big's 256-row tiles, ring_small's 1 / d of the chip, the ping-pong ring's one tile per CU
    int three_quarters;   // a patch conv runs unsplit (192 of 256 CUs); the 256 x 192 tile (tile192)
    int seven_eighths;    // the ring GEMM's 256-row tile
    int half;             // ring_small: the 64 x 80 grid fills at least this much
    int two_per_cu;       // split-K: slices to reach about two blocks per CU
    ChipFill(const EngineOptions& o, int ncu)
        : splitk_tiles(scaled(o.splitk_tiles, ncu)), dense_tiles(scaled(o.dense_tiles, ncu)), conv_patch2_tiles(scaled(o.conv_patch2_tiles, ncu)),
          patch_split_tiles(scaled(o.patch_split_tiles, ncu)), patch_split_fill(scaled(o.patch_split_fill, ncu)), whole(ncu),
          three_quarters(ncu * 3 / 4), seven_eighths(ncu * 7 / 8), half(ncu / 2), two_per_cu(2 * ncu) {}
    static int scaled(int v, int ncu) { return (int)((long long)v * ncu / 256); }
};

// K [B][L][C], V^T [B][C][round_up(L, 8)]; P: the same in st_tail.hip's fragment order (fused blocks); L: context keys per sample (0: cfg.context_len)
struct KVSlot { void* K = nullptr; void* VT = nullptr; void* P = nullptr; int L = 0; };

enum { SOLVER_DDIM = 0, SOLVER_UNIPC = 1, SOLVER_LMS = 2 };

struct Session {
    bool active = false;
    pd_sample_args a{};
    int Bf = 0;
    int S = 0;
    int L = 0;                       // context tokens per sample of this session (pd_sample_args.context_len, or cfg.context_len)
    std::vector<int64_t> timesteps;  // ascending (ddim_timesteps)
    std::vector<int64_t> custom_ts;  // copy of pd_sample_args.timesteps (descending), empty = uniform grid
    std::vector<float> alphas, alphas_prev, sigmas, sqrt_1m;
    std::vector<float> scales_step;  // [S][13]
    // device state
    float* x_state = nullptr;   // [B, HW, 8] fp32
    float* x_in = nullptr;      // [Bf, HW, 8] fp32
    float* pred_x0 = nullptr;   // [B, HW, C]
    float* eps_g = nullptr;     // [B, HW, C]
    float* noise = nullptr;     // [S][B, C, HW] or null
    bool noise_seeded = false;  // PD_NOISE_FROM_SEED: the update kernels draw the per-step noise themselves (no arena for it)
    void* ctx = nullptr;        // [Bf, L, Dpad] compute type
    Act hint;                   // guided_hint [Bf, h, w, C0]
    std::vector<KVSlot> kv_u, kv_c;
    std::vector<float*> emb_u, emb_c;  // per ResBlock [rows, Cout]
    int emb_rows = 0;
    float* per_step = nullptr;  // optional [S+1][B,C,h,w]
    Act control[PD_NUM_CONTROL];
    size_t session_top = 0;
    // shared CFG front (pd_engine::forward_eps): both halves of the batch see the same guided_hint; this evaluation runs the UNet's /
    // the ControlNet's layers in front of the first cross-attention once for both halves
    bool hint_shared = false, share_u = false, share_c = false;
    int pag_B = 0;               // perturbed-attention guidance: samples of the perturbed branch in this evaluation (forward_eps); 0: none
    bool cn_cond_only = false;   // guess mode under guidance: this evaluation runs the ControlNet on the conditional half only (run_controlnet)
    // solver of step(): DDIM, or the fused UniPC loop (pd_sample_begin_unipc / pd_unipc_sample)
    int solver = 0;                  // SOLVER_DDIM / SOLVER_UNIPC / SOLVER_LMS
    std::vector<double> unipc_coef;  // [S][PD_UNIPC_NCOEF] (multistep.cpp)
    int unipc_ring = 0;              // x0 predictions kept: the solver order
    double* u_last = nullptr;        // [B, HW, C] fp64: corrected sample of the previous step
    double* u_ring[3] = {nullptr, nullptr, nullptr};   // [B, HW, C] fp64 each: m_j in slot j % unipc_ring
    // linear multistep loop (pd_sample_begin_lms / pd_lms_sample): one row per evaluation, S completed steps
    std::vector<double> lms_coef;    // [n_rows][PD_LMS_NCOEF] (multistep.cpp)
    std::vector<double> lms_times;   // [n_rows] model time of every evaluation
    std::vector<int> lms_step;       // [n_rows] steps completed before the row
    std::vector<int> lms_pushed;     // [n_rows] model outputs pushed before the row
    int lms_ring = 0;                // history slots: the deepest n_hist of the rows (at least 1)
    bool lms_keep = false;           // some row keeps a sample
    double* l_keep = nullptr;        // [B, HW, C] fp64
    double* l_ring[3] = {nullptr, nullptr, nullptr};   // [B, HW, C] fp64 each: pushed output j in slot j % lms_ring
    int rows() const { return solver == SOLVER_LMS ? (int)lms_times.size() : S; }   // evaluations of the loop
    // img2img / inpainting (pd_sample_args.init_latents / mask): z0 and eps [B, C, HW] and the mask [B, HW], fp32, allocated after
    // everything else; blend[i] = the coefficients of the blend after step i (fp32 from the engine's fp32 table, on the host)
    float* init_z0 = nullptr;
    float* init_eps = nullptr;
    float* mask = nullptr;
    std::vector<BlendCoef> blend;
};

struct pd_engine {
    pd_config cfg{};
    int device = 0;
    int ncu = 256;      // compute units of the device (hipDeviceProp_t::multiProcessorCount; stat "ncu"): the tile / split-K rules scale with it (ChipFill)
    hipStream_t stream = nullptr;
    void* comm = nullptr;   // ncclComm_t of pd_comm_init (comm.cpp); the final all-gather of a sharded batch
    int comm_world = 1, comm_rank = 0;
    bool f32 = false;   // fp32 storage of activations and weights (PD_PREC_F32 and PD_PREC_F16X2)
    int P = DT_BF16;    // MFMA precision code handed to the contraction launchers: T, or PREC_F16X2
    int T = DT_BF16;  // compute (MFMA operand) type: DT_BF16, DT_F16 or DT_F32
    int S = DT_BF16;  // residual-stream type: T, or DT_F32 with stream_f32
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    NetW unet, cnet;
    VaeW vae;
    VaeEncW vae_enc;
    ClipW text;
    // captured step loops (option "graph"): key = everything a step's kernel arguments depend on
    struct GraphEntry { uint64_t key; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    void clear_graphs();
    int run_steps_graph();
    WeightGroup reg_group = GROUP_SAMPLER;   // group of the parameters being registered
    int missing(WeightGroup g) const;        // parameters of g not loaded yet
    int require_loaded(WeightGroup g, const char* what);   // non-zero, with "<what> weights not loaded: '<name>' (and possibly more)" set
    std::vector<void*> owned;  // device allocations (weights)
    bool alloc_failed = false; // a hipMalloc in dmalloc() failed (reported by build() / the bench hooks)
    int check_arena();         // non-zero (with the error set) when a workspace allocation overflowed
    size_t weight_bytes = 0;
    Arena arena;
    // second context for the ControlNet pass (own stream / workspace / GroupNorm scratch), see forward_eps
    Arena arena2;
    hipStream_t stream2 = nullptr;
    double* gn_partial2 = nullptr;
    int* tile_cnt2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool cn_pending = false;
    EngineOptions opt;   // every pd_set_option knob (options.h): per engine, stored as given
    // FreeU (pd_set_freeu): {s1, s2, b1, b2}, all zero when off; per engine, read by run_unet at every decoder block
    float freeu[4] = {0.f, 0.f, 0.f, 0.f};
    bool freeu_on() const { return freeu[0] != 0.f && freeu[1] != 0.f && freeu[2] != 0.f && freeu[3] != 0.f; }
    // Perturbed-attention guidance (pd_set_pag): {scale, adaptive scale} and the mask of perturbed UNet transformer blocks (bit j = block
    // j of IpAdapterW's order: encoder, decoder, middle); per engine, read by forward_eps / run_unet and by the update launch
    float pag[2] = {0.f, 0.f};
    uint32_t pag_mask = 0;
    bool pag_on() const { return pag[0] != 0.f && pag_mask != 0; }
    float pag_scale_at(double t) const;   // p_i of an evaluation at model time t (the adaptive rule, in double), 0 when off
    long long pag_launches = 0;           // stat "pag_launches": the identity launches and the second launch of everything split for the branch
    int pag_fork_block = -1;              // stat "pag_fork_block": the block where the last evaluation forked; -1: none, or option pag_fork 0
    // seeded noise (pd_set_rng; addressing in include/pdengine.h): {seed_lo, seed_hi, base_lo, base_hi} on the device, read by the
    // update / start / posterior / fill kernels, rewritten by a copy ordered on `stream` (captured graphs see the new values)
    uint32_t* rng_dev = nullptr;
    uint32_t rng_host[4] = {0u, 0u, 0u, 0u};
    uint64_t rng_seed = 0, rng_base = 0;
    long long graph_captures = 0, graph_replays = 0;   // stats: step loops captured / replayed
    void swap_context();
    int join_controlnet();
    Session ses;
    long long launches = 0;
    long long gn_from_slabs = 0;   // GroupNorm launches that summed a split-K GEMM's slabs (stat "gn_from_slabs")
    long long ring_launches = 0;   // launches that took gemm_ring.hip (stat "ring_launches")
    int gn_kernel = 0;             // GN_KIND_* of the last groupnorm() launch (stat "gn_kernel"), set where the launch is decided
    long long ups_fold_launches = 0;   // launches that took conv_upfold.hip (stat "ups_fold_launches")
    int attn_kernel = 0;           // ATTN_KIND_* of the last attention() launch (stat "attn_kernel"), set by the launcher; 0: none yet
    int gemm_tile = -1, gemm_splitk = -1;   // the tile of the instantiation that launch took (gemm_launched_tile; 0 outside the igemm family) and its slices (stats "gemm_tile", "gemm_splitk")
    int gemm_ring_tile = -1;                // launch_ring_gemm's tile of that launch, 2 / 3 the ping-pong forms; -1: not a ring launch (stat "gemm_ring_tile")
    int gemm_family = -1;          // GemmFamily of the last gemm() launch (stat "gemm_family"), set where gemm() launches; -1: none yet
    // optional per-launch timing (bench.py roofline leg): HIP events around every contraction launch
    struct ProfRec { hipEvent_t a, b; int klass; double flops; int M, N, K, taps; };
    bool profiling = false;
    float prof_overhead_ms = 0.f;   // elapsed time of an EMPTY event bracket on this stream (calibrated when profiling is switched on)
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t next_event();
    void prof_begin(ProfRec& r, int klass, double flops);
    void prof_end(ProfRec& r);
    double* gn_partial = nullptr;  // scratch for GroupNorm partial sums
    int* tile_cnt = nullptr;       // split-K arrival counters (kTileCnt ints, zero between GEMMs), one set per stream
    static constexpr int kTileCnt = 4096;
    size_t gn_partial_cap = 0;

    // construction
    int build();
    void* dmalloc(size_t bytes);
    void make_mat(WMat& m, int n_rows, int k_logical, int taps, int cin, bool bias, bool geglu = false);
    void reg_mat(const std::string& name, std::vector<int64_t> shape, WMat* m, int row_off, bool conv);
    void reg_vec(const std::string& name, int n, float** dst, char init);
    void reg_bias(const std::string& name, WMat* m, int off, int n, bool geglu = false);
    void build_conv(const std::string& prefix, ConvW& c, int cin, int cout, int k, int stride);
    void build_res(const std::string& prefix, ResW& r, int cin, int cout, NetW& net);
    void build_st(const std::string& prefix, STW& s, int ch, NetW& net);
    void build_encoder(const std::string& prefix, NetW& net);
    void build_middle(const std::string& prefix, NetW& net);
    void build_vres(const std::string& prefix, ResW& r, int cin, int cout, bool diffusers = false);
    void build_vattn(const std::string& prefix, VaeAttnW& a, int C, bool diffusers = false);
    void build_vae();           // the SD1.5 first stage from pd_config: fills vae.d, then build_vae_decoder
    void build_vae_encoder();
    void build_vae_decoder(VaeW& v, const std::string& prefix);      // v.d filled by the caller; prefix "first_stage_model." / "vae."
    void build_vae_encoder(VaeEncW& v, const std::string& prefix);
    // SD3's VAE (sd3_vae.cpp, pd_sd3_vae_configure): the same layers under a description of its own
    VaeW sd3_vae;
    VaeEncW sd3_vae_enc;
    long long vae_flash_launches = 0;
    bool vae_flash_on(const VaeDesc& d, int C, long long N) const;   // N: tokens per sample
    // scale / shift: what the layout kernel applies to the latents (decode) or the posterior kernel to z (encode)
    int vae_forward(VaeW& v, const float* latents_dev, int B, int h, int w, float* out_dev, float scale, float shift);
    int vae_encoder_forward(VaeEncW& v, const float* images_dev, int B, int H, int W, int what, const float* noise_dev, float* out_dev, float scale,
                            float shift);
    int vae_attention(const VaeAttnW& a, const VaeDesc& d, const Act& x, Act& out);
    // softmax(q k^T C^-0.5) v of B samples: q | k rows [B][N][ld] (k = q + C elements), vt [B][C][npad], att [B][N][C], all in T.  flash: one
    // launch of vae_attention.hip, any N; else three launches per sample through sc [N][N] fp32 and pr [N][npad] T (N a multiple of 8,
    // npad = round_up(N, 64), the pad columns of vt and pr zero)
    int vae_attn_product(const void* qk, int ld, const void* vt, int npad, void* att, int B, int N, int C, bool flash, float* sc, void* pr);
    // the layers between the two layout kernels: z / x in the compute type (NHWC), img / mom fp32 NHWC allocated by the caller
    int vae_decode_layers(VaeW& v, const Act& z, Act& img);
    int vae_encode_layers(VaeEncW& v, const Act& x, Act& mom);
    // decode / encode behind the C ABI, shared by pd_vae_* and pd_sd3_vae_*; which: PD_VAE_SD15 / PD_VAE_SD3 (the tiling state)
    int vae_decode_call(VaeW& v, int which, const float* latents, int B, int h, int w, int mem, float scale, float shift, float* images_out);
    int vae_encode_call(VaeEncW& v, int which, const float* images, int B, int H, int W, int mem, int what, const float* noise, float scale,
                        float shift, float* out);
    // Tiled / sliced calls (vae_tile.cpp; pd_vae_set_tiling, pd_vae_set_slicing).  All zero = off: the calls above then run as ever.
    struct VaeTiling { bool tiling = false, slicing = false; int tile = 0; double overlap = 0.0; int batch = 0; };
    VaeTiling vae_tiling[2];
    bool vae_tile_odd_flash = false;   // set while tiles run: a tile with N % 8 != 0 takes the flash kernel on a VAE without flash_auto
    std::vector<char> vae_tile_blob;   // host image of the device tables of the running tiled call (alive until the call's final sync)
    long long vae_tiles_run = 0;       // stat "vae_tiles": tiles decoded / encoded so far
    VaeTilePlan vae_plan_for(int which, int h, int w, int u, bool encode) const;   // .tiled false when the state or the size says no
    int vae_check_tiles(const VaeTilePlan& p, const VaeDesc& d, int C, const char* who) const;
    int vae_tile_setup(const VaeTilePlan& p, int B, int cpad, VaeTileRun& run);
    int vae_tile_blend(const VaeTilePlan& p, const VaeTileRun& run, int B, int C, int cpad, bool nchw, float* out);
    int vae_decode_managed(VaeW& v, int which, const float* src, int B, int h, int w, float* dout, float scale, float shift);
    int vae_encode_managed(VaeEncW& v, int which, const float* src, int B, int H, int W, int what, const float* noise, float* dout, float scale,
                           float shift);
    // Everything that runs outside a sampling step (first stage, annotators, text / image encoders): body(SideCall&) is written once and
    // run twice in the ControlNet context's workspace (arena2, idle outside a sampling step).  The first run is dry and measures the
    // workspace -- the staging the body takes from its SideCall included -- which is grown to that plus 64 MiB of slack if needed (both
    // streams synchronised, captured graphs dropped); the second enqueues for real on the main stream.  Then the staged destinations are
    // copied out and the stream is synchronised, once.  `what` names the caller in the allocation-failure message.
    template <class Body> int side_call(const char* what, Body&& body);
    int side_grow(const char* what, size_t need);
    // The frame of the seven pd_*_configure: session refusal, check() (the caller's own argument checks, in their old place), device,
    // build() with the parameters it registers in group g, and the allocation-failure report; `who` is the entry point's name.
    template <class Check, class Build> int configure(const char* who, WeightGroup g, Check&& check, Build&& build);
    template <class Build> int configure(const char* who, WeightGroup g, Build&& build) { return configure(who, g, [] { return 0; }, build); }

    // CLIP text stack (text.cpp).  build_clip registers one CLIPTextModel under `prefix` (its "text_model."); the caller has filled the
    // dimensions and sized w.layers.  clip_blocks runs blocks [first, last) on the residual stream x, whose type the block's sums follow.
    void build_clip(const std::string& prefix, ClipW& w);
    void build_clip_layers(const std::string& prefix, ClipW& w);   // "encoder.layers.N.*" alone (the image tower has other embeddings)
    void build_text();
    int clip_embed(const ClipW& w, const int* ids_dev, Act& x);
    // att (allocated here) = attention over q | k and V^T of ln, projected by `qkv` [3 * inner rows]; relbias / scale as in attention()
    int self_attention(const WMat& qkv, const Act& ln, int inner, int heads, bool causal, const float* relbias, float scale, Act& att);
    int clip_block(const TextLayerW& l, Act& x, int heads, Activation act, bool causal, float eps = 1e-5f);
    int clip_blocks(const ClipW& w, int first, int last, Act& x);
    int text_forward(const int* ids_dev, int B, float* out_dev, int clip_skip);

    // HED edge detector (hed.cpp): registered by pd_hed_configure, runs in the same workspace as the first stage
    HedW hed;
    void build_hed();
    int hed_forward(const float* images_dev, int B, int H, int W, int what, float* out_dev);

    // M-LSD line detector (mlsd.cpp): registered by pd_mlsd_configure, runs in the same workspace as the first stage
    MlsdW mlsd;
    void build_mlsd();
    void build_conv_bn(const std::string& conv, const std::string& bn, ConvW& c, int cin, int cout, int k, int stride);
    void build_dw_bn(const std::string& conv, const std::string& bn, MlsdDw& d, int C, int stride);
    int mlsd_dwconv(const MlsdDw& d, const Act& x, Act& y);
    // images_dev [B][H][W][3] u8 -> tp_dev [B][9][H/2][W/2] fp32
    int mlsd_forward(const uint8_t* images_dev, int B, int H, int W, float* tp_dev);
    // tp [B][9][h][w] -> segs [B][200][4], count [B] (both device, allocated by the caller)
    int mlsd_decode(const float* tp_dev, int B, int h, int w, float thr_v, float thr_d, int* segs_dev, int* count_dev);

    // Image ends (image_host.cpp, image_io.hip): buffers of pd_image_load / pd_image_store that grow on demand and never shrink
    struct ImageBuf { void* p = nullptr; size_t cap = 0; };
    ImageBuf img_u8;     // the source pictures of a host caller (load) / the bytes on their way to a host caller (store)
    ImageBuf img_tmp;    // the picture between the horizontal and the vertical pass
    ImageBuf img_f32;    // the float tensor of a host caller
    ImageBuf img_tab;    // both axes' tables: bounds + kk of the horizontal pass, then of the vertical one
    std::vector<int32_t> img_tab_host;
    int32_t img_tab_key[5] = {0, 0, 0, 0, 0};   // (Ws, W, Hs, H, filter) the device tables hold now; all zero: none
    long long image_allocs = 0;                 // stat "image_allocs"
    int image_grow(ImageBuf& b, size_t bytes);
    void image_release();

    // Canny edge detector (canny.cpp, canny.hip): scratch that grows like the image ends' and is counted in image_allocs with it
    ImageBuf canny_states;                      // the state map [B][H][W]
    ImageBuf canny_flags;                       // kCannyBatch ints: sweep i of a batch raises flag i
    int* canny_flags_host = nullptr;            // their pinned copy, read after every batch
    static constexpr int kCannyBatch = 4;       // sweeps enqueued between two looks at the flags
    long long canny_sweeps = 0;                 // stat "canny_sweeps": hysteresis launches of the last call
    // sweeps the device map [B][H][W] to its fixed point: at most B * H * W + 1 launches, else an error
    int canny_hysteresis(uint8_t* states_dev, int B, int H, int W);

    // CLIP image tower and safety checker (clip_vision.cpp, clip_vision.hip)
    ClipVisionW clip_vision[2];
    SafetyW safety;
    ImageBuf clip_tmp;     // the picture between the two passes of the preprocessing (crop columns only)
    ImageBuf clip_tab;     // its tables, crop rows / columns only: bounds_h | kk_h | bounds_v | kk_v
    ImageBuf clip_out;     // staging of a host destination
    std::vector<int32_t> clip_tab_host;
    int32_t clip_tab_key[3] = {0, 0, 0};   // (H, W, image_size) the device tables hold now
    ClipVisionW* find_clip_vision(const char* prefix);
    // src_dev [B][H][W][3] u8 -> dst_dev in `mode` (PD_CLIP_OUT_*; patches in T); everything on `stream`, nothing synchronised
    int clip_preprocess_dev(const uint8_t* src_dev, int B, int H, int W, int S, int patch, const float* mean, const float* stdv, int mode, void* dst_dev);
    // patches [B * P][Kw] in T -> hidden_states[k] [B][P + 1][C], pooler_output [B][C], image_embeds [B][D] (fp32, device; null: not wanted)
    int clip_vision_forward(ClipVisionW& v, const void* patches_dev, int B, int k, float* hid_dev, float* pooled_dev, float* embeds_dev);

    // SD3 / MMDiT path (sd3.cpp)
    pd_sd3_config sd3{};
    Sd3NetW sd3_tr, sd3_cn;
    std::vector<hipEvent_t> sd3_ev;   // ControlNet residual i written (recorded on the second stream)
    struct Sd3Io {   // device pointers of one evaluation
        const float *latents, *context, *pooled, *cond, *pair;
        const float* cn_pooled;   // ControlNet's pooled projections; null: zeros
        const float* t_host;
        int B, H, W, S;
        float scale;
    };
    void build_sd3_net(const std::string& prefix, Sd3NetW& net, bool controlnet);
    int sd3_embed(Sd3NetW& net, const Sd3Io& io, bool controlnet, Act& hs, Act& c, Act& modbuf);
    int sd3_block(const Sd3BlockW& b, Act& x, Act& c, const Act& modbuf, const Act& qk, const Act& vt, const Act* pre_add = nullptr);
    int sd3_forward(const Sd3Io& io, float* v_out_dev, int control_index, float* control_out_dev);
    // SD3 text encoders (pd_sd3_text_configure): CLIP-L, CLIP-G (text.cpp's stack) and T5 (sd3_text.cpp).  Residual streams are fp32 in every mode.
    ClipW sd3_clip[2];
    Sd3T5W sd3_t5;
    int sd3_text_joint = 0;
    std::vector<int32_t> t5_bucket_host;   // bucket of every distance -(L - 1) .. L - 1 of the last T5 call (kept alive for the upload)
    void build_sd3_t5(const std::string& prefix);
    // hidden (hidden_states[-(clip_skip + 2)], no final LayerNorm) -> columns [c_off, c_off + width) of hid [B][hid_rows][hid_ld] (columns past the
    // encoder's own are zeroed); pooled (text_embeds) -> pooled [B][pooled_ld]; either destination may be null
    int sd3_clip_forward(ClipW& w, const int* ids_dev, int B, int clip_skip, float* hid, int hid_rows, int hid_ld, int c_off, int width,
                         float* pooled, int pooled_ld);
    // last_hidden_state -> rows [row_off, row_off + Lt) of out [B][out_rows][d_model]
    int sd3_t5_forward(const int* ids_dev, int B, int Lt, float* out, int out_rows, int row_off);
    int t5_block(const T5LayerW& l, Act& x, const float* relbias);
    int rmsnorm(const Act& x, void* y, int y_dt, const float* w, float eps, int y_sample_rows = 0, int y_row_off = 0, int y_ld = 0);
    bool sd3_fp8_dirty = true;   // option "sd3_fp8" or a weight changed: sd3_quantize() has work to do
    int sd3_quantize();        // (re)builds the e4m3 weights of the layers option "sd3_fp8" names after a weight change

    // LoRA adapters merged in place into matrix parameters (lora.cpp, lora.hip).  A target is one Param that at least one
    // adapter touches: its base rows W0 in T (all m.N rows of a GEGLU matrix), and every adapter's up^T / down stacked in load
    // order as the merge kernel's UT [R][rows] / D [R][Kpad] operands.
    struct LoraEntry { int adapter = 0, r = 0; };
    // One adapter that is not a stack of rank-1 columns.  PAIR (under a magnitude) / HADA: ut1 [r1][rows], d1 [r1][Kpad] (and
    // ut2 / d2 [r2]...) laid out like ut / d; KRON: ut1 = w1 [ka][kb], d1 = w2 [rows / ka][taps][cin / kb].  mag [rows] or null.
    // All of it lives in the one device allocation `buf`; the format's alpha / r is already multiplied into ut1.
    struct LoraForm {
        int adapter = 0, kind = 0, r1 = 0, r2 = 0, ka = 0, kb = 0;
        float* buf = nullptr;
        size_t bytes = 0;
        float *ut1 = nullptr, *d1 = nullptr, *ut2 = nullptr, *d2 = nullptr, *mag = nullptr;
    };
    struct LoraTarget {
        void* w0 = nullptr;
        size_t w0_bytes = 0;
        float* ut = nullptr;
        float* d = nullptr;
        int R = 0;
        std::vector<LoraEntry> entries;   // column blocks of ut / d, in load order
        std::vector<float> merged;        // multiplier of each entry that W holds now; empty: W holds W0
        std::vector<LoraForm> forms;      // pd_lora_add_ex adapters (Hadamard, Kronecker, magnitude), in load order
        std::vector<float> fmerged;       // multiplier of each form that W holds now; cleared together with `merged`
    };
    float* lora_tmp = nullptr;                 // fp32 scratch of a merge with forms: one adapter's delta, and the running sum
    float* lora_sum = nullptr;
    size_t lora_tmp_cap = 0;                   // floats in each
    int lora_add_ex(int adapter, const char* name, const pd_lora_factors& f);
    int lora_target_base(int pi);              // the first adapter on a parameter saves its rows as W0
    std::map<int, LoraTarget> lora;            // by parameter index (ordered: merges launch in registry order)
    std::map<int, float> lora_scale;           // adapter id -> multiplier (0: inactive)
    float* lora_scale_dev = nullptr;
    size_t lora_scale_cap = 0;
    int lora_add(int adapter, const char* name, const float* up, int up_rows, int rank, const float* down, const int64_t* down_shape,
                 int down_ndim);
    int lora_set_scales(const float* scales, int n);
    int lora_remove(int adapter);
    int lora_merge(int only_param, bool force);   // only_param -1: every target
    int lora_rebase(int only_param);              // base weights were written: W -> W0, then merge again
    void lora_release();
    size_t lora_bytes(bool base_only) const;
    int read_param(const Param& p, float* out);

    // weights
    int load(const char* name, const void* data, const int64_t* shape, int ndim, int dtype);
    int init_random(uint64_t seed);
    int upload_vec(float* dst_dev, const float* src, int n, bool geglu, int half);
    int upload_rows(WMat& m, int row_off, const float* src, int rows, bool conv);

    // primitive ops (enqueue on stream; honour arena.dry)
    Act new_act(int B, int H, int W, int C, int dt);
    // gemm() = check + fill (call -> GemmParams), plan (which kernel: shapes, options and ncu only), run (workspace, launch, profiling)
    int gemm(const WMat& m, const Act& in, Act& out, const GemmCall& c = {});
    int check_gemm(const WMat& m, const Act& in, const Act& out, const GemmCall& c) const;
    static GemmParams fill_gemm(const WMat& m, const Act& in, const Act& out, const GemmCall& c);
    GemmPlan plan_gemm(const GemmParams& p, const WMat& m, const GemmCall& c, bool allow_splitk = true) const;
    ChipFill chip_fill() const { return ChipFill(opt, ncu); }
    int patch_tiles(const GemmParams& p) const; bool patch_unsplit(int ptiles) const;
    int fold_upconv(WMat& m);   // (re)builds m.w_up from m.w; fold_upconvs(): for every UNet decoder Upsample conv the dispatch can take
    int fold_upconvs();
    bool upfold_wanted(const WMat& m) const;
    int fold_layernorms();     // (re)builds the folded weights of every transformer block after a weight change
    bool ln_dirty = true;
    bool st_tail_on(const STW& s, int rows_per_sample, int L) const;   // L: context keys of the call
    int gn_stats(const Act& x, int& nchunk);
    // conv3x3 / conv1x1 of `c`: call.stride and call.pad_shift come from the ConvW.  conv_gn: conv(act(GroupNorm(x))); call carries the
    // residual / row vector / defer pointer of the conv
    int conv(const ConvW& c, const Act& in, Act& out, GemmCall call = {});
    int conv_gn(const ConvW& c, const Act& x, Act& out, const float* g, const float* b, float eps, bool silu, GemmCall call = {},
                const SlabDefer* in_slabs = nullptr);
    int groupnorm(const Act& x, Act& y, const float* g, const float* b, float eps, bool silu, const SlabDefer* from_slabs = nullptr);
    int layernorm(const Act& x, Act& y, const float* g, const float* b, float eps = 1e-5f);
    int resblock(const ResW& r, const Act& x, Act& out, const float* embrow, int emb_stride);
    // out_given: `out` is the caller's tensor (a batch view of a larger one) instead of a new allocation
    int transformer(const STW& s, const Act& x, Act& out, const KVSlot& kv, int out_B = 0, const IpTerm* ip = nullptr, const PagTerm* pag = nullptr,
                    bool out_given = false);
    // src and a copy of its samples [first, first + count) behind them
    int extend_act(const Act& src, int first, int count, Act& dst);
    KVSlot kv_from(const KVSlot& k, int C, int first) const;   // the hoisted context K / V^T from sample `first` on
    // IP-Adapter (ip_adapter.cpp)
    IpAdapterW ip;
    long long ip_launches = 0;   // stat "ip_launches": image-term launches so far
    // the term of block s in a network evaluation at batch Bf (use_cfg: [unconditional ; conditional] halves); false: none (inactive, not a
    // UNet block, s_j == 0)
    bool ip_term(const STW& s, int Bf, bool use_cfg, IpTerm& t) const;
    int ip_check_batch(int B) const;   // non-zero with the error set when the image state does not fit a sampling batch B
    int ip_image_term(const void* q2, void* att, const IpTerm& t, int B, int N, int C, int q_shared);
    int repeat_act(const Act& src, int reps, Act& dst);
    static Act batch_view(const Act& a, int first, int count);
    int attention(const void* Q, int ldq, const void* K, int ldk, const void* VT, int vt_ld, void* O, int ldo, int B, int Nq,
                  int Nk, int C, int heads = 0, bool causal = false, long long q_bs = 0, long long k_bs = 0, long long o_bs = 0,
                  const float* relbias = nullptr, float scale = 0.f);   // relbias: T5's Toeplitz bias rows (launch_attention_bias); scale 0: dh^-0.5

    // networks
    int run_controlnet(const Act& x_in, int emb_row, int emb_stride, const float* scales);
    int run_unet(const Act& x_in, int emb_row, int emb_stride, bool only_mid, Act& eps);
    int forward_eps(int emb_row, int emb_stride, const float* scales, Act& eps);

    // sessions
    int ensure_arena(int rows, bool per_step);
    int session_setup(const pd_sample_args& a, const int64_t* t_rows, int n_rows, bool want_per_step, const double* t_rows_f = nullptr);
    int compute_emb(NetW& net, std::vector<float*>& tabs, const int64_t* t, int n, int row0, const double* tf = nullptr);   // tf: fractional times instead of t
    int begin(const pd_sample_args* a, bool want_per_step, const pd_unipc_args* u = nullptr, const pd_lms_args* l = nullptr);
    int step(int i);   // eps, then the solver's update launch (step_ddim / step_unipc / step_lms), then the optional per-step copy
    UpdateState update_state(const Act& eps, double t) const;   // t: the model time of the evaluation (the adaptive PAG scale)
    int step_ddim(int i, const UpdateState& u, const BlendArgs* bl);
    int step_unipc(int i, const UpdateState& u, const BlendArgs* bl);
    int step_lms(int i, const UpdateState& u, const BlendArgs* bl);
    int make_schedule(int steps, float eta, std::vector<int64_t>& ts, std::vector<float>& a, std::vector<float>& ap,
                      std::vector<float>& sg, std::vector<float>& s1m, const int64_t* custom_desc = nullptr);
};

// One profiled launch (option "profile"): an event bracket of class `klass` around what is enqueued while it lives.  Nothing with
// profiling off, in a dry pass, or for klass < 0 (PD_LAUNCH).
struct Bracket {
    pd_engine* e;
    pd_engine::ProfRec rec{};
    const bool on;
    Bracket(pd_engine* e_, int klass) : e(e_), on(klass >= 0 && e_->profiling && !e_->arena.dry) {
        if (on) e->prof_begin(rec, klass, 0.0);
    }
    ~Bracket() {
        if (on) e->prof_end(rec);
    }
};

// Parameters registered while it lives belong to group g; GROUP_SAMPLER again on every path out.
struct RegGroup {
    pd_engine& e;
    RegGroup(pd_engine& e_, int g) : e(e_) { e.reg_group = (WeightGroup)g; }
    ~RegGroup() { e.reg_group = GROUP_SAMPLER; }
};

// The staging of one pd_engine::side_call, handed to its body.  Every allocation comes from the workspace in both passes, so the dry
// pass measures it; copies are enqueued on the main stream in the real pass only.  n counts elements of T.
struct SideCall {
    pd_engine& e;
    template <class T> T* scratch(size_t n) { return reinterpret_cast<T*>(e.arena.alloc(n * sizeof(T))); }
    // *dev = the caller's p [n] as device memory: p itself from the device, a workspace copy (uploaded here) from the host
    template <class T> int src(const T** dev, const T* p, size_t n, int mem) {
        *dev = p;
        if (mem == PD_MEM_DEVICE) return 0;
        T* d = scratch<T>(n);
        *dev = d;
        return upload(d, p, n * sizeof(T));
    }
    int upload(void* dev, const void* host, size_t bytes);   // host memory -> a workspace allocation made elsewhere
    // A workspace buffer that is copied to the caller's p (either memory space) after the body: `rows` rows of n elements, the caller's
    // rows `pitch` elements apart (0: dense)
    template <class T> T* dst(T* p, size_t n, int mem, size_t rows = 1, size_t pitch = 0) {
        return reinterpret_cast<T*>(stage(p, n * sizeof(T), rows, pitch * sizeof(T), mem));
    }
    void* stage(void* p, size_t width, size_t rows, size_t pitch, int mem);
    int finish();   // the copies out, then the call's one stream synchronisation
    struct Back { void* dst; const void* src; size_t width, rows, pitch; int mem; };
    std::vector<Back> backs;
};

template <class Body>
int pd_engine::side_call(const char* what, Body&& body) {
    SideCall f{*this};
    std::swap(arena, arena2);
    const Arena saved = arena;
    arena.base = nullptr; arena.cap = 0; arena.top = 0; arena.peak = 0; arena.dry = true;
    int r = body(f);
    const size_t need = arena.peak + (64u << 20);
    arena = saved;
    arena.dry = false;
    if (!r) r = side_grow(what, need);
    if (!r) {
        arena.top = 0; arena.peak = 0;
        r = body(f);
        if (!r) r = f.finish();
        else hipStreamSynchronize(stream);   // an upload from the caller's memory may still be in flight
        arena.top = 0;
    }
    std::swap(arena, arena2);
    return r;
}

template <class Check, class Build>
int pd_engine::configure(const char* who, WeightGroup g, Check&& check, Build&& build) {
    if (ses.active) { pd_set_error("%s: end the sampling session first", who); return 1; }
    PD_TRY(check());
    HIP_OK(hipSetDevice(device));
    alloc_failed = false;
    {
        RegGroup rg(*this, g);
        build();
    }
    if (alloc_failed) { pd_set_error("%s: weight allocation failed", who); return 1; }
    return 0;
}
