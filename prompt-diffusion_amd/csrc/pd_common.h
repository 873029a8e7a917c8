// Shared declarations of the pdengine HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

// Storage / MFMA operand types.  DT_BF16 and DT_F16 share one byte-level data path (2-byte elements); the engine's
// compute type T is one of the three and selects the MFMA instruction and the converts.
enum PdDType : int { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2, DT_FP8 = 4 };   // DT_FP8: OCP e4m3fn bytes + one fp32 scale per row
static inline size_t dt_size(int dt) { return dt == DT_F32 ? 4 : dt == DT_FP8 ? 1 : 2; }
// MFMA precision codes handed to the contraction launchers: the operand PdDType, or PREC_F16X2 -- fp32 storage like
// DT_F32, but every operand is split into fp16 hi + lo halves in registers and the product runs as two fp16 MFMAs
// (all four hi/lo cross terms): ~22-bit operands at a quarter of the fp16 MFMA rate, 4x the fp32 MFMA rate.
constexpr int PREC_F16X2 = 3;
// PREC_FP8 (== DT_FP8): both operands e4m3 with per-row scales (A: per token, W: per output channel), one
// v_mfma_scale_f32_16x16x128_f8f6f4 (block scales 1.0) per accumulator and 128-byte K step -- twice the f16 MFMA rate at
// half the LDS bytes per FLOP; the scales multiply the accumulator in the epilogue.  Linear layers of the SD3 path only.
constexpr int PREC_FP8 = 4;
constexpr bool prec_f32_storage(int P) { return P == DT_F32 || P == PREC_F16X2; }

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#if defined(__HIPCC__)
__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
    __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return __builtin_bit_cast(uint16_t, b);
}
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
    // one v_cvt_pk_bf16_f32 (RNE, NaN stays NaN) instead of two converts + shift + or
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
__device__ __forceinline__ float h2f(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }   // v_cvt_f16_f32, RNE
__device__ __forceinline__ uint32_t pack2h(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
}
// 16-bit flavour helpers: DT is DT_BF16 or DT_F16 (compile-time in the kernels that are templated on it)
template <int DT> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    if constexpr (DT == DT_F16) return pack2h(lo, hi); else return pack2bf(lo, hi);
}
template <int DT> __device__ __forceinline__ void unpack2(uint32_t w, float& lo, float& hi) {
    if constexpr (DT == DT_F16) {
        const f16x2_t h = __builtin_bit_cast(f16x2_t, w);
        lo = (float)h[0]; hi = (float)h[1];
    } else {
        lo = __uint_as_float(w << 16); hi = __uint_as_float(w & 0xffff0000u);
    }
}
template <int DT> __device__ __forceinline__ uint16_t cvt16(float f) {
    if constexpr (DT == DT_F16) return f2h(f); else return f2bf(f);
}
template <int DT> __device__ __forceinline__ float cvt32(uint16_t v) {
    if constexpr (DT == DT_F16) return h2f(v); else return bf2f(v);
}
// runtime-tagged forms (dt is wave-uniform: a kernel argument)
__device__ __forceinline__ uint16_t cvt16_rt(float f, int dt) { return dt == DT_F16 ? f2h(f) : f2bf(f); }
__device__ __forceinline__ float cvt32_rt(uint16_t v, int dt) { return dt == DT_F16 ? h2f(v) : bf2f(v); }
// 8 packed 16-bit values (one uint4) <-> 8 floats
template <int DT> __device__ __forceinline__ void unpack8(const uint4& r, float* f) {
    unpack2<DT>(r.x, f[0], f[1]); unpack2<DT>(r.y, f[2], f[3]); unpack2<DT>(r.z, f[4], f[5]); unpack2<DT>(r.w, f[6], f[7]);
}
template <int DT> __device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 u;
    u.x = pack2<DT>(f[0], f[1]); u.y = pack2<DT>(f[2], f[3]); u.z = pack2<DT>(f[4], f[5]); u.w = pack2<DT>(f[6], f[7]);
    return u;
}
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;  // single instruction: hipcc otherwise canonicalises MFMA outputs with extra v_max before fmaxf
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
// exact-erf GELU with erf from Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7): ~12 instructions instead of
// libm erff's ~45; used where the result is rounded to bf16 anyway
__device__ __forceinline__ float gelu_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = poly * t * __expf(-z * z);   // 1 - erf(z)
    const float erfz = 1.0f - e;
    return 0.5f * x * (1.0f + copysignf(erfz, x));
}

// XCD-aware block order: blocks b and b + 8 share an XCD / L2, so hardware block `bid` of `nblk` takes the work item that gives each
// XCD one contiguous run of items -- neighbours that share operand rows or 128-byte lines then hit the same L2.  (gemm_ring.hip's
// persistent blocks walk a run per XCD instead: a different scheme.)
__device__ __forceinline__ int xcd_tile_order(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
// Byte offset of 16-byte chunk `chunk` of row `row` in an LDS tile of 128-byte rows whose chunks are permuted by XORing the chunk
// index with (row >> 1) & 7: fragment reads of 16 consecutive rows starting at a multiple of 16 are conflict-free.  swz8_chunk: the
// slot a chunk sits in (and, the XOR being an involution, the chunk a slot holds).
__device__ __forceinline__ int swz8_chunk(int row, int chunk) { return (chunk ^ (row >> 1)) & 7; }
__device__ __forceinline__ int swz8(int row, int chunk) { return (row * 128) + (swz8_chunk(row, chunk) << 4); }

// x * m + a with the product and the sum each rounded once: the value map of the image ends (image_io.hip) and of the Canny edge map
// (canny.hip).  (hipcc contracts a * b + c into an FMA by default, through __fmul_rn / __fadd_rn as well: they are plain operators in
// HIP's headers.  The pragma is what keeps the two roundings apart.)
__device__ __forceinline__ float mul_add_rn(float x, float m, float a) {
#pragma clang fp contract(off)
    const float p = x * m;
    return p + a;
}

// 4 consecutive elements of a [.., C] row, as floats, from an f32 or bf16 buffer
__device__ __forceinline__ f32x4 load4(const void* base, size_t idx, int dt) {
    f32x4 r;
    if (dt == DT_F32) {
        r = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx);
    } else {
        uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + idx);
        float a, b, c, d;
        if (dt == DT_F16) {
            unpack2<DT_F16>(u.x, a, b);
            unpack2<DT_F16>(u.y, c, d);
        } else {
            unpack2<DT_BF16>(u.x, a, b);
            unpack2<DT_BF16>(u.y, c, d);
        }
        r = f32x4{a, b, c, d};
    }
    return r;
}
__device__ __forceinline__ void store4(void* base, size_t idx, int dt, f32x4 v) {
    if (dt == DT_F32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + idx) = v;
    } else {
        uint2 u;
        if (dt == DT_F16) {
            u.x = pack2h(v[0], v[1]);
            u.y = pack2h(v[2], v[3]);
        } else {
            u.x = pack2bf(v[0], v[1]);
            u.y = pack2bf(v[2], v[3]);
        }
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(base) + idx) = u;
    }
}
#endif

// One-time (per device) opt-in to more than 64 KB of dynamic LDS for a kernel.  `done` is a static bit mask owned by the
// launcher (one bit per device id: engines on different devices share the process).
static inline int ensure_dyn_smem(const void* fn, int bytes, unsigned long long* done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    const unsigned long long bit = 1ull << (dev & 63);
    if (*done & bit) return 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return 1;
    *done |= bit;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution / linear:  C[M,N] = epilogue( A_gather[M,K] x W[N,K]^T )
// ---------------------------------------------------------------------------------------------
// GemmParams::act (the kernels compare against the values).  ACT_RELU is compiled into instantiations of its own (pd_mma.h epilogue4_value<MM, RELU>:
// plain conv3x3 on igemm / patch1 / patch2, conv1x1 on igemm (M-LSD), and the split-K finalize pass), so no other launch carries a branch for
// it; the ring GEMM and the 4-wave patch conv refuse it
// ACT_ERF_GELU (CLIP-G's fc1) lives in the MM instantiations like ACT_TANH_GELU; ACT_GATED_TANH_GELU (T5's wi_0 / wi_1 pair, packed like a GEGLU
// matrix: x half = wi_1, gate half = wi_0) is gelu_new(gate) * x formed in fp32, saturated to the fp16 range on an fp16 store, in GG instantiations
// of its own (gemm.hip GT).  Neither runs on the ring GEMM.
enum Activation { ACT_NONE = 0, ACT_SILU = 1, ACT_GEGLU = 2, ACT_QUICK_GELU = 3, ACT_TANH_GELU = 4, ACT_RELU = 5, ACT_ERF_GELU = 6, ACT_GATED_TANH_GELU = 7 };
struct GemmParams {
    const void* A;        // activations, NHWC (conv) or [M, lda] rows (linear)
    const void* W;        // weights [Nw][Kpad] in the compute type, K-contiguous (taps x Cin)
    const float* bias;    // [Nw] fp32 or null
    void* C;              // output [M, ldc]
    const void* R;        // residual [M, ldr] or null (added after scale)
    const float* rowvec;  // per-sample broadcast row (time-embedding projection) or null
    void* VT;             // optional transposed output for columns >= vt_begin: [B][N-vt_begin][vt_ld]
    int M, N, K;          // K: logical reduction length (taps*Cin); N: weight rows (virtual cols)
    int Kpad;             // weight row stride in elements (multiple of the K tile)
    int lda, ldc, ldr;    // element strides (lda = pixel stride for conv)
    int a_dt, c_dt, r_dt; // PdDType of A / C / R
    int taps;             // 1 (linear / conv1x1) or 9 (conv3x3, pad 1)
    int Cin;              // channels per tap
    int Hin, Win, Hout, Wout, stride, ups;  // conv geometry; ups=1: nearest x2 upsample fused in the gather
    int rows_per_sample;  // Hout*Wout (conv) or tokens per sample (linear)
    int rowvec_stride;    // elements between samples in rowvec (0: one row for all)
    int act;              // Activation: 0 none, 1 SiLU, 2 GEGLU (weights pre-interleaved in 80+80 blocks), 3 quick-GELU, 4 tanh-GELU, 5 ReLU
    int a_silu;           // apply SiLU to A on load (emb_layers)
    float out_scale;      // applied to (acc + bias [+ rowvec]) before the residual
    int vt_begin, vt_ld;  // see VT
    int Nout;             // GEGLU: logical output columns (N/2 rounded), else == N
    int splitk;           // >1: grid.y slices K; each slice stores an fp32 slab, a finalize pass sums them + epilogue
    void* slab;           // [splitk][M][N] fp32 workspace
    int* tile_cnt;        // split-K: one zeroed counter per 128x160 tile -> finalize fused into the last-arriving slice; null: separate pass
    int defer_finalize;   // split-K without tile counters: 1 = no finalize pass here -- the consumer (norm.hip gn_fused_kernel, slab mode) sums the slabs
    int big_tile;         // tile: 0 128 x 160 (4 waves), 1 256 x 160, 2 128 x 160 on 8 waves (short K), 3 256 x 320, 4 256 x 192
    const float* gn_coef; // conv_patch only: [B][Cin][2] GroupNorm coefficients applied (+SiLU) while staging A; null = none
    int gn_silu;
    int ldw;              // weight row stride in elements (0: Kpad) -- lets a device activation act as the W operand
    // LayerNorm folded into this GEMM (consumer side): A is the RAW residual-stream tensor, W holds W * diag(gamma), and the
    // epilogue turns acc = x . W'^T into LN(x) . W^T = rstd[m] * (acc - mean[m] * colsum[n]) (+ bias, which carries beta . W^T).
    // ln_stats: [M][ln_parts][2] fp32 {sum, sum of squares} partials of each row of A over disjoint column ranges.
    const float* ln_stats;
    const float* ln_colsum;   // [N] sum_k W'[n][k] of the stored (rounded) weights
    int ln_parts;
    int ln_C;                 // row length of A (number of normalised channels)
    float ln_eps;
    // producer side: this GEMM writes a residual-stream tensor that a LayerNorm reads next -- every (row, column range of
    // one wave) leaves its {sum, sum of squares} in stats_out[M][stats_parts][2] (igemm_kernel epilogue only)
    float* stats_out;
    int stats_parts;
    // MMDiT (sd3.cpp): per-sample gate row multiplied into (acc + bias) * out_scale before the residual (AdaLN-Zero), and a
    // row remap of the stores so that two token streams land in one joint [sample][c_sample_rows] buffer:
    // row = sample * c_sample_rows + c_row_off + tok (c_sample_rows = 0: row = gm); V^T tokens shift by vt_tok_off.
    const float* gate;
    int gate_stride;
    int c_sample_rows, c_row_off, vt_tok_off;
    // ... and of the A rows (linear, MM instantiations): row = sample * a_sample_rows + a_row_off + tok -- one token stream
    // read out of a joint buffer (a_sample_rows = 0: row = m)
    int a_sample_rows, a_row_off;
    // PREC_FP8: acc * a_scale[m] * w_scale[n] before everything else in the epilogue
    const float* a_scale;
    const float* w_scale;
    // c_dt == DT_FP8 (MM instantiations): the output rows are written as e4m3 of value / c_scale[row]; the caller guarantees
    // |value| <= 448 c_scale[row] (sd3.cpp: a Cauchy-Schwarz bound from the input row's norm)
    const float* c_scale;
    // conv3x3 in the implicit-GEMM gather only: shifts the window's top-left corner by this many pixels down / right.  0 is
    // the symmetric pad 1 of every other conv; 1 gives F.pad(x, (0, 1, 0, 1)) + padding 0, the KL-VAE encoder's Downsample
    // (model.py:80-88) -- the bounds check already reads row Hin / column Win as the bottom / right zero.
    int pad_shift;
    // conv3x3 in the implicit-GEMM gather only: dilation - 1 (0 everywhere but M-LSD's block23.conv1, dilation 5): the taps sit
    // dilation pixels apart and the padding is dilation on every side, so the output keeps the input's size
    int dil_m1;
};

// element-wise / norm / attention launchers (definitions in the .hip files)
struct AttnParams {
    const void* Q; const void* K; const void* VT; void* O;
    int ldq, ldk, ldo;   // element strides between tokens
    int vt_ld;           // VT row stride (keys, padded)
    long long q_bs, k_bs, vt_bs, o_bs;  // element strides between samples
    int Nq, Nk, heads, dh;
    float scale;
    int B;
    int legacy;  // 1: use the single-buffered reference kernel (debug)
    int causal;  // keys after the query are masked (CLIP text transformer)
};

int launch_gemm(const GemmParams& p, int prec, hipStream_t s, hipEvent_t mid = nullptr, int* parts = nullptr);   // prec: the compute type (DT_*)
// LayerNorm-statistics partials per row (GemmParams::stats_parts) that launch_gemm / launch_ring_gemm write for this launch:
// column tiles x waves across N of the tile their dispatch takes (parts != null runs that dispatch without launching); 0: none
int gemm_stats_parts(const GemmParams& p, int prec);
int gemm_launched_tile(const GemmParams& p, int prec);   // the tile (GemmParams::big_tile numbering) of the instantiation launch_gemm takes for p
int ring_gemm_stats_parts(const GemmParams& p, int prec, int tile);
// gemm_ring.hip: persistent LDS-DMA ring GEMM for plain linear layers over 2-byte operands (tile 0: 128 x 160, 1: 256 x 160); ncu: the
// device's compute units (pd_engine::ncu), which size the persistent grid
bool ring_gemm_eligible(const GemmParams& p, int prec);
int launch_ring_gemm(const GemmParams& p, int prec, int tile, int ncu, hipStream_t s, int* parts = nullptr);
// fp8 (e4m3) rows with one scale per row: dst[r][k] = e4m3(src[r][k] / scale[r]), scale[r] = max_k |src[r][k]| / 448 (weights of
// the SD3 linear layers that run in PREC_FP8); src in dtype src_dt with row stride src_ld, dst row stride dst_ld >= K (pad zeroed)
int launch_quant_rows(const void* src, int src_dt, int src_ld, void* dst, int dst_ld, float* scale, int rows, int K, hipStream_t s);
// y[b][n] = bias[n] + sum_k W[n][k] * f(a[b][k]) for B <= 4 fp32 rows (f = SiLU when a_silu): the weight-streaming form of
// a Linear over a handful of rows (MMDiT modulation vectors); w_dt: DT_F32 / DT_F16 / DT_BF16, K % 8 == 0, K <= 2048
int launch_gemv(const float* a, int lda, const void* W, int w_dt, int Kpad, const float* bias, float* y, int ldy, int B, int N, int K,
                int a_silu, hipStream_t s);
int gemm_tiles(int M, int N);
int launch_splitk_finalize(const GemmParams& p, hipStream_t s);   // sums p.splitk fp32 slabs in slice order + epilogue
int conv_patch_tiles(const GemmParams& p, int prec);  // 0: shape not eligible for the LDS-patch conv kernel
int launch_conv_patch(const GemmParams& p, int prec, hipStream_t s);
int launch_conv_patch2(const GemmParams& p, int prec, hipStream_t s);   // conv_patch2.hip: compute / loader wave specialisation (2-byte types)
bool conv_patch4_eligible(const GemmParams& p, int prec);              // conv_patch4.hip: 4 waves per block, one per SIMD, 32x32x16 MFMAs, LDS-DMA operands (2-byte types)
int launch_conv_patch4(const GemmParams& p, int prec, hipStream_t s);
// conv_upfold.hip: conv3x3(nearest_x2(x)) as four 2x2-tap phase convs over the source (2-byte types, bias-only epilogue); p is the nine-tap call's
bool conv_upfold_eligible(const GemmParams& p, int prec);
int conv_upfold_tiles(const GemmParams& p);   // blocks of the phase launch
int launch_conv_upfold(const GemmParams& p, const void* w_up, int prec, hipStream_t s);
int launch_upfold_weights(const void* w, void* w_up, int dt, int N, int cin_pad, int Kpad, hipStream_t s);   // [N][9][cin_pad] -> [4][N][4][cin_pad]
// which kernel family an attention launch took (stat "attn_kernel": PD_ATTN_* in include/pdengine.h): attn_kernel, at every mode, head
// dim, mask and bias, or the double-buffered attn2_kernel of the 2-byte modes (not causal, no bias, AttnParams::legacy 0)
enum { ATTN_KIND_GENERIC = 1, ATTN_KIND_PIPELINED = 2 };
int launch_attention(const AttnParams& p, int prec, hipStream_t s, int* kind = nullptr);   // kind: which family took it (ATTN_KIND_*; 0: no launch)
// vae_attention.hip: softmax(Q K^T * scale) V with one head over all C channels (the first stage's AttnBlock), C = 128 / 512, 2-byte modes.
// Q, K [B][N][..] token-major (ldq / ldk elements between tokens), VT [B][C][vt_ld] with vt_ld >= round_up(N, 8), O [B][N][ldo]; *_bs:
// elements between samples.  Any N >= 1.  One launch for the batch.  Returns 2 for a (mode, C) that has no instantiation.
struct VaeAttnParams {
    const void* Q; const void* K; const void* VT; void* O;
    int ldq, ldk, ldo, vt_ld;
    long long q_bs, k_bs, vt_bs, o_bs;
    int B, N, C;
    float scale;
};
bool vae_attention_eligible(int prec, int C);
int launch_vae_attention(const VaeAttnParams& p, int prec, hipStream_t s);
// T5 self-attention: softmax(Q K^T * scale + bias) V, bias[h][q][k] = relbias[h][k - q + Nk - 1] (fp32, in exp2 units: times log2 e); dh 64, Nq == Nk
int launch_attention_bias(const AttnParams& p, const float* relbias, int prec, hipStream_t s, int* kind = nullptr);
// st_tail.hip: everything after the self-attention product of a 320-channel SpatialTransformer block in one kernel (attn1.to_out +
// residual, norm2, attn2 against the hoisted context K / V, norm3, GEGLU feed-forward, proj_out + the block residual)
bool st_tail_eligible(int prec, int C, int heads, int rows_per_sample, int Nk);
size_t st_tail_weight_bytes();
size_t st_tail_vec_floats();
size_t st_tail_kv_bytes(int B, int Nk);   // B samples' context K / V in fragment order, ceil(Nk / 96) windows each
int st_tail_windows(int Nk);
double st_tail_flops(long long M, int Nk);
// ... and its front: GroupNorm apply + proj_in + norm1 + to_q / to_k / to_v (h, q | k and V^T out)
size_t st_front_weight_bytes();
size_t st_front_vec_floats();
double st_front_flops(long long M);
int launch_st_front_pack(const void* wpi, const void* wqkv_ln, int ld, const float* bpi, const float* bqkv_ln, void* wdst, float* vdst, hipStream_t s);
int launch_st_front(const void* x, const float* coef, void* h, void* qk, void* vt, const void* wpk, const float* vec, long long M, int rows_per_sample,
                    int vt_ld, int prec, hipStream_t s);
int launch_st_tail_pack(const void* wo1, const void* wq_ln, const void* wo2, const void* w1_ln, const void* w2, const void* wp, int ld_c, int ld_w2,
                        void* dst, hipStream_t s);
int launch_st_tail_vec(const float* bo1, const float* bq_ln, const float* bo2, const float* b1_ln, const float* b2, const float* bp, float* dst,
                       hipStream_t s);
int launch_st_tail_kv_pack(const void* K, const void* VT, void* dst, int B, int Nk, int lpad, hipStream_t s);
int launch_st_tail(const void* att, const void* h, const void* x_in, void* out, const void* wpk, const float* vec, const void* kvp, long long M,
                   int rows_per_sample, int Nk, int s_dt, float scale, int prec, hipStream_t s, long long in_rows = 0);
int launch_gn_stats(const void* x, int x_dt, double* partial, int B, int HW, int C, int groups, int nchunk, hipStream_t s);
int launch_gn_apply(const void* x, int x_dt, void* y, int y_dt, const double* partial, const float* gamma,
                    const float* beta, int B, int HW, int C, int groups, int nchunk, float eps, int silu, hipStream_t s);
// which kernel a GroupNorm launch took (stat "gn_kernel": PD_GN_* in include/pdengine.h)
enum { GN_KIND_TWO_PASS = 1, GN_KIND_LDS_SLAB = 2, GN_KIND_REGISTER = 3 };
// norm.hip: > 0 when the single-kernel GroupNorm applies.  reg (here and in the two launchers): the caller's option "gn_reg", the
// register-resident kernel where the shape has one
int gn_fused_bundle(int x_dt, int HW, int C, int groups, bool reg);
int launch_gn_fused(const void* x, int x_dt, void* y, int y_dt, const float* gamma, const float* beta, int B, int HW, int C, int groups,
                    float eps, int do_silu, bool reg, hipStream_t s, int* kind = nullptr);   // kind: which kernel took it (GN_KIND_*)
// the same kernel fed by a split-K GEMM's fp32 slabs instead of a stored tensor: x[row][c] = round_T(sum_s slab[s][row][c] + bias[c] +
// rowvec[sample][c]) -- splitk_finalize_kernel's arithmetic and rounding, so the result is bit-identical to finalize + launch_gn_fused
int launch_gn_fused_slabs(const float* slabs, int nslab, const float* bias, const float* rowvec, int rowvec_stride, int x_dt, void* y, int y_dt,
                          const float* gamma, const float* beta, int B, int HW, int C, int groups, float eps, int do_silu, bool reg, hipStream_t s, int* kind = nullptr);
int launch_gn_coef(const double* partial, const float* gamma, const float* beta, float* coef, int B, int HW, int C, int groups,
                   int nchunk, float eps, hipStream_t s);
// {sum, sum of squares} of every row: the single-part form of the LayerNorm statistics above (producers whose epilogue
// cannot emit them: split-K finalize, patch conv)
int launch_row_stats(const void* x, int x_dt, float* stats, int rows, int C, hipStream_t s);
// W' = W * diag(gamma) in the compute type, colsum[n] = sum_k W'[n][k], bias_out[n] = bias_in[n] + sum_k beta[k] * W[n][k]
int launch_ln_fold(const void* W, void* Wout, int dt, int N, int K, int Kpad, const float* gamma, const float* beta, const float* bias_in,
                   float* colsum, float* bias_out, hipStream_t s);
int launch_layernorm(const void* x, int x_dt, void* y, int y_dt, const float* gamma, const float* beta,
                     int rows, int C, float eps, hipStream_t s);
// out[b][p][c] = scale * in[b][c][p] + shift for c < C, 0 for the pad channels
int launch_nchw_to_nhwc(const float* in, void* out, int out_dt, int B, int C, int H, int W, int Cpad, hipStream_t s,
                        float scale = 1.0f, float shift = 0.0f);
int launch_softmax_rows(const float* in, void* out, int out_dt, int rows, int n, hipStream_t s);
// out[b,l,:] = tok[ids[b,l]] + pos[l]  (CLIP text embeddings); tables are [rows][ld] in dtype dt
int launch_embed_tokens(const int* ids, const void* tok, int tok_ld, const void* pos, int pos_ld, int dt, void* out, int out_dt,
                        int B, int L, int C, int vocab, hipStream_t s);
int launch_nhwc_to_nchw(const void* in, int in_dt, float* out, int B, int C, int H, int W, int Cpad, float scale, hipStream_t s);
// vae_tile.hip: the two ends of a tiled VAE call (pd_vae_set_tiling)
// out[t * B + b][y][x][c] = scale * in[b][c][origins[2t] + y][origins[2t + 1] + x] + shift for c < C, 0 for the pad channels; in is
// [B][C][H][W] fp32, every window [th][tw] must lie inside it (the caller checks)
int launch_vae_tile_gather(const float* in, void* out, int out_dt, const int* origins, int ntile, int B, int C, int H, int W, int th, int tw,
                           int Cpad, float scale, float shift, hipStream_t s);
// Tile (ti, tj) of the nrow x ncol grid is fp32 [B][rows[4 ti]][cols[4 tj]][Cpad] at tiles + tile_off[ti * ncol + tj] (a multiple of 4
// floats) and owns the output rectangle from (ti * limit, tj * limit).  rows[4 ti + 1] is its blend extent against the tile above (0 in
// row 0) and rows[4 ti + 2] the offset in wtab of that extent's 2 e weights (1 - y / e, then y / e); cols the same along x.
struct VaeBlendParams {
    const float* tiles; const long long* tile_off; const int* rows; const int* cols; const float* wtab;
    float* out;          // nchw: [B][C][H][W]; else [B][H][W][Cpad]
    int B, C, Cpad, H, W, nrow, ncol, limit, nchw;
};
int launch_vae_tile_blend(const VaeBlendParams& p, hipStream_t s);
// sd3_text_kernels.hip: the small kernels of the SD3 text encoders (T5: sd3_text.cpp; the CLIP pooling and the joint write: text.cpp)
// out[row][:] = tok[clamp(ids[row])][:] (table rows [vocab][tok_ld] in dt) -> fp32 [rows][C]: T5's token embedding (no positions)
int launch_embed_rows(const int* ids, const void* tok, int tok_ld, int dt, float* out, long long rows, int C, int vocab, hipStream_t s);
// T5LayerNorm: y = w * x * rsqrt(mean(x^2) + eps), statistics in fp32, x fp32 [rows][C]; row r of y lands at
// y + ((r / rows_per_sample) * y_sample_rows + y_row_off + r % rows_per_sample) * y_ld (y_sample_rows 0: row r), in y_dt
int launch_rmsnorm_rows(const float* x, void* y, int y_dt, const float* w, long long rows, int C, float eps, int rows_per_sample, int y_sample_rows,
                        int y_row_off, int y_ld, hipStream_t s);
// relbias[h][i] = log2(e) * table[bucket[i]][h] for i < 2 L - 1 (bucket: host-made, pd_t5_relative_buckets); table [num_buckets][ld] in dt
int launch_t5_relbias(const int* bucket, const void* table, int ld, int dt, float* relbias, int heads, int n, hipStream_t s);
// dst[(b * dst_sample_rows + r) * dst_ld + c_off + c] = c < C ? src[(b * rows_per_sample + r) * C + c] : 0 for c < width: one encoder's hidden
// state (and, with width > C, the zero pad behind it) into the joint [B, 77 + Lt, joint_dim] layout
int launch_joint_write(const float* src, float* dst, int B, int rows_per_sample, int C, int width, int dst_sample_rows, int dst_ld, int c_off,
                       hipStream_t s);
// out[b][:] = x[b * L + pos(b)][:], pos = argmax(ids[b]) (first maximum) when eos_id == 2, else the first ids == eos_id (0 when absent):
// transformers' CLIPTextTransformer pooling
int launch_eos_gather(const int* ids, const float* x, float* out, int B, int L, int C, int eos_id, hipStream_t s);
int launch_cast_rows(const float* in, void* out, int out_dt, long long rows, int C, int Cpad, hipStream_t s);
int launch_concat_add(const void* a, const void* a_add, const void* b, const void* b_add, void* out, int dt,
                      long long rows, int Ca, int Cb, hipStream_t s, long long b_rows = 0, long long b_add_rows = 0);
int launch_add_inplace(void* a, const void* b, int dt, long long n, hipStream_t s);
// FreeU's skip concat (freeu.hip): launch_concat_add's output with the first Ch / 2 backbone channels scaled by b and the skip
// half passed through fourier_filter(threshold 1, scale s) per (sample, channel) plane; rows = B * H * W
int launch_freeu_concat(const void* h, const void* h_add, const void* skip, const void* skip_add, void* out, int dt, int B, int H,
                        int W, int Ch, int Cs, float s, float b, hipStream_t st, long long skip_rows = 0, long long skip_add_rows = 0);
// IP-Adapter's image term (ip_attention.hip): att [B][N][C] += s * softmax(q2 K_ip^T scale) V_ip per head, in place, one rounding to
// dt at the store.  q2, att [B][N][C], K_ip / V_ip [.][T][C] in dt, kv_sample_stride elements between two samples' keys (0: one set
// for every sample); 1 <= T <= 64, C % 8 == 0, C / heads one of 8, 16, 32, 40, 80, 160.  0 launched, 1 launch failure, 2 shape refused
int launch_ip_attention_add(const void* q2, void* att, const void* K_ip, const void* V_ip, long long kv_sample_stride, int B, int N, int C, int heads,
                            int T, float scale, float s, int dt, hipStream_t stream);
// Perturbed-attention guidance (pag.hip): att [count][N][C] = the transposition of samples [src, src + count) of VT [.][C][npad], a bit
// copy of a storage type of elem_bytes (2 or 4)
int launch_pag_identity(const void* VT, void* att, int elem_bytes, int src, int count, int N, int C, int npad, hipStream_t s);
// The end of a denoising step (sampler_update.hip): guidance + solver update (+ inpainting blend) + the next step's x_in.
// What every update launch of a session shares: the UNet's eps [Bf, HW, eps_C] (uncond half first) in eps_dt, x_state
// [B, HW, Cpad] fp32 updated in place, pred_x0 / eps_guided [B, HW, C] fp32, x_in [dup * B, HW, Cpad] fp32.
struct UpdateState {
    const void* eps; int eps_dt, eps_C;
    float* x_state; float* pred_x0; float* eps_guided; float* x_in;
    int B, HW, C, Cpad, use_cfg;
    // perturbed-attention guidance (pd_set_pag): eps holds a third run of B samples from sample pag_off on (2 B under CFG, else B), the
    // conditional branch with perturbed self-attention, and the guided eps gains pag_scale * (eps_cond - eps_perturbed).  pag: the
    // evaluation carries that run (0: none, and the kernel executes what it executed before the state existed); pag_scale may then
    // still be 0 on a step (the adaptive clamp): the run is not read, the guidance is formed without FMA contraction all the same
    int pag = 0;
    float pag_scale = 0.f;
    int pag_off = 0;
};
// img2img / inpainting (semantics in include/pdengine.h, pd_sample_args.init_latents / mask).  z0, ieps: [B, C, HW] fp32 NCHW;
// mask: [B, HW].  The blend (1 - m) k + m x, k = last ? z0 : sa z0 + sb eps, is evaluated in fp32 without contraction and
// applied to the updated sample before x_state / x_in are written.
struct BlendCoef { float sa, sb; int last; };
struct BlendArgs { const float* z0; const float* ieps; const float* mask; BlendCoef coef; };
struct DdimCoef { float sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, sigma, cfg_scale; };
// do_update 0: only eps_guided is written; bl null: no blend.  rng_state (the engine's device RNG state, pd_set_rng) non-null:
// the draw comes from the generator at (PD_RNG_STEP, draw) and noise must be null
int launch_cfg_ddim(const UpdateState& u, const DdimCoef& k, const float* noise, float temperature, int do_update, const BlendArgs* bl,
                    hipStream_t s, const uint32_t* rng_state = nullptr, uint32_t draw = 0);
// Fused UniPC step (include/pdengine.h, PD_UNIPC_NCOEF): one coefficient row, passed by value so a captured graph bakes it in.
//   c_m[0..3]: corrector weights of m_i, m_{i-1}, m_{i-2}, m_{i-3}; p_m[0..2]: predictor weights of m_i, m_{i-1}, m_{i-2};
//   n_hist: how many of the history slots m_{i-1}, m_{i-2}, m_{i-3} the step reads (the others may be null)
struct UnipcCoef { double alpha, sigma, c_last, c_m[4], p_x, p_m[3]; int corr, n_hist; float cfg_scale; };
// last [B, HW, C] fp64: corrected sample of the previous step (rewritten); m_out [B, HW, C] fp64: m_i (may alias hist[n_hist-1],
// which is read first)
int launch_cfg_unipc(const UpdateState& u, const UnipcCoef& k, double* last, double* m_out, const double* const hist[3],
                     const BlendArgs* bl, hipStream_t s);
// One row of a linear multistep solver (include/pdengine.h, PD_LMS_NCOEF), by value like UnipcCoef.
//   x_next = c_x base + sum_k c_m[k] m_{i-k},  pred_x0 = q_x base + sum_k q_m[k] m_{i-k},  base = base_keep ? keep : x;
//   data_pred: m_i = (x - sigma eps) / alpha, else m_i = eps; store_keep: keep = x before the update; push: m_i -> m_out;
//   n_hist: how many of m_{i-1}, m_{i-2}, m_{i-3} the row reads
//   c_z: x_next += c_z z with z the seeded normal at (PD_RNG_STEP, draw); needs rng_state when non-zero
struct LmsCoef { double alpha, sigma, c_x, c_m[4], q_x, q_m[4]; int data_pred, base_keep, store_keep, push, n_hist; float cfg_scale; double c_z; };
// keep [B, HW, C] fp64: the kept sample (null when no flag uses it); m_out / hist as in launch_cfg_unipc
int launch_cfg_lms(const UpdateState& u, const LmsCoef& k, double* keep, double* m_out, const double* const hist[3], const BlendArgs* bl,
                   hipStream_t s, const uint32_t* rng_state = nullptr, uint32_t draw = 0);
// start latents: x = pure ? eps : sa z0 + sb eps -> x_state [B, HW, Cpad] (channels >= C zero), x_in (dup copies), and
// optionally out_nchw [B, C, HW].  rng_state non-null: eps is drawn at (PD_RNG_XT, draw 0) instead of read, and stored to
// eps_out [B, C, HW] when that is non-null
int launch_init_latents(const float* z0, const float* eps, float sa, float sb, int pure, float* x_state, float* x_in, float* out_nchw,
                        int B, int dup, int C, int Cpad, int HW, hipStream_t s, const uint32_t* rng_state = nullptr,
                        float* eps_out = nullptr);
// out [B][per_sample] fp32 = the seeded normals at (stream, draw, sample b, element e) (pd_philox.h; pd_randn)
int launch_randn(const uint32_t* rng_state, uint32_t stream, uint32_t draw, int B, long long per_sample, float* out, hipStream_t s);
int launch_fill_random(void* p, int dt, long long n, float scale, float shift, uint64_t seed, hipStream_t s);
// LoRA merge (lora.hip) of one matrix parameter: W rows = round_dt(W0 + (scale . UT)^T D); UT [R][rows], D [R][Kpad] fp32,
// scale [R]; source row n -> WMat row row_off + n, or the 80 + 80 GEGLU interleave when geglu_half > 0 (row_off 0); W0 holds the
// destination rows from row_off on.  Kpad must be a multiple of 32.
int launch_lora_merge(int dt, void* W, const void* W0, int rows, int row_off, int geglu_half, int Kpad, const float* UT,
                      const float* D, const float* scale, int R, hipStream_t s);
// Adapter forms beyond a stack of rank-1 columns (lora.hip).  The delta launches write fp32 out [rows][Kpad] in source-row order:
//   form: out = (sum_j mul_j UT1[j] (x) D1[j]) (.) (sum_j UT2[j] (x) D2[j]) (the second product only when UT2 is given); mul_j = scale[j],
//         or s when scale is null;
//   kron: out[i * c + p, tap * cin_pad + j * d + q] = (s * w1[i, j]) * w2[p, tap, q], w1 [a][b], w2 [rows / a][taps][cin / b]; pad columns 0.
// apply: sum = (first ? W0 : sum) + E, E = delta, or (mag[n] / |W0 + delta|_2)(W0 + delta) - W0 per row when mag is given; with `last`
// the sum is rounded to dt and written to W through launch_lora_merge's row mapping instead.  `sum` is fp32 [rows][Kpad].
int launch_lora_form_delta(float* out, int rows, int Kpad, const float* UT1, const float* D1, const float* scale, float s, int R1,
                           const float* UT2, const float* D2, int R2, hipStream_t st);
int launch_lora_kron_delta(float* out, int rows, int Kpad, int cin, int cin_pad, int taps, const float* w1, const float* w2, float s, int a,
                           int b, hipStream_t st);
int launch_lora_form_apply(int dt, void* W, const void* W0, float* sum, const float* delta, const float* mag, int rows, int row_off,
                           int geglu_half, int Kpad, int first, int last, hipStream_t st);
// DiagonalGaussianDistribution of the first-stage encoder (distributions.py:24-62) from quant_conv's NHWC output `mom` (dtype mom_dt,
// Cpad >= 2 z channels: mean 0..z-1, logvar z..2z-1) into caller-layout fp32 NCHW: what = PD_VAE_MEAN: scale * mean,
// PD_VAE_SAMPLE: scale * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise[B, z, HW]), PD_VAE_MOMENTS: the raw [B, 2z, HW] moments
// noise null with PD_VAE_SAMPLE: the seeded normals at (PD_RNG_VAE, draw 0) from rng_state.  shift: MEAN and SAMPLE become
// scale * (x - shift), SD3's (z - shift_factor) * scaling_factor
int launch_vae_posterior(const void* mom, int mom_dt, int Cpad, const float* noise, float* out, int B, int z, int HW, int what, float scale,
                         hipStream_t s, const uint32_t* rng_state = nullptr, float shift = 0.0f);
// hed.hip: the element-wise kernels of the HED edge detector (hed.cpp)
// images [B][3][H][W] fp32 RGB in [0, 1] -> out [B][H][W][Cpad] in out_dt: channel c < 3 = image channel 2 - c (BGR) * 255 - the VGG mean of
// channel c, in fp32, rounded once; channels >= 3 zero.  Cpad a multiple of 4
int launch_hed_upload(const float* in, void* out, int out_dt, int B, int H, int W, int Cpad, hipStream_t s);
// x [B][H][W][C] in dt (C a multiple of 16 bytes) -> score [B][H][W] fp32 = x . sw + sb[0] (fp32 accumulation) and, when pooled is non-null
// (H, W even), pooled [B][H/2][W/2][C] in dt = max_pool2d(x, 2, 2); x is read once
int launch_hed_stage_tail(const void* x, int dt, const float* sw, const float* sb, float* score, void* pooled, int B, int H, int W, int C,
                          hipStream_t s);
// scores[i] [B][H >> i][W >> i] fp32 (H, W multiples of 16), cw [5], cb [1] -> what 0: out [B][1][H][W] = sigmoid(cb + sum_i cw[i] up_i),
// what 1: out [B][5][H][W] = up_i; up_i the bilinear upsample (align_corners = False) of map i by 2^i
int launch_hed_fuse(const float* const scores[5], const float* cw, const float* cb, float* out, int B, int H, int W, int what, hipStream_t s);
// mlsd.hip: the kernels of the M-LSD line detector that are no contraction (mlsd.cpp; include/pdengine.h "M-LSD line detector")
// images [B][H][W][3] u8 -> out [B][H][W][8] in out_dt: channels 0..2 = u8 / 127.5 - 1 (fp32, each operation rounded once), channel 3 =
// 1 / 127.5 - 1 (the reference's constant-one plane through the same map), channels 4..7 zero
int launch_mlsd_upload(const uint8_t* in, void* out, int out_dt, int B, int H, int W, hipStream_t s);
// depthwise conv3x3 + bias + ReLU6 on NHWC rows in dt: x [B][H][W][C] -> y [B][Ho][Wo][C]; w [C][9] fp32 (the checkpoint's [C, 1, 3, 3]),
// bias [C] fp32; stride 1: padding 1, Ho = H; stride 2: a zero row / column at the bottom / right only, Ho = H / 2 (H, W even).
// in_relu6: min(max(x, 0), 6) while loading (the producer's ReLU6; it stored max(x, 0)).  C a multiple of 16 bytes of dt
int launch_mlsd_dwconv(const void* x, void* y, int dt, const float* w, const float* bias, int B, int H, int W, int C, int stride, int in_relu6,
                       hipStream_t s);
// F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) of x [B][h][w][C] (row stride ldx) into channels of a wider
// buffer: y [B][2h][2w][ldy] + the caller's channel offset; fp32 arithmetic, one rounding to dt.  C, ldx, ldy multiples of 16 bytes
int launch_mlsd_upcat(const void* x, int ldx, void* y, int ldy, int dt, int B, int h, int w, int C, hipStream_t s);
// x [B][h][w][16] fp32 NHWC -> tp [B][9][h][w] fp32: channels 7..15 (MobileV2_MLSD_Large.forward's x[:, 7:])
int launch_mlsd_tpmap(const float* x, float* tp, int B, int h, int w, hipStream_t s);
constexpr int MLSD_TOPK = 200;
// tp [B][9][h][w] fp32 -> segs [B][MLSD_TOPK][4] int32 (x0, y0, x1, y1 in input pixels), count [B]; cand [B][h * w] and ncand [B] are
// scratch (ncand zeroed by the launcher).  Two launches: peaks of the 3x3 non-maximum suppression, then per image the 200 best and
// their thresholds and endpoints
int launch_mlsd_decode(const float* tp, unsigned long long* cand, int* ncand, int* segs, int* count, int B, int h, int w, float thr_v,
                       float thr_d, hipStream_t s);
// segs / count as above -> map [B][H][W] u8 (zeroed by the launcher): CANNY_STRONG on every pixel of cv2.line(p0, p1, thickness 1,
// LINE_8) -- clipped to the image, then the 8-connected Bresenham walk
int launch_mlsd_draw(const int* segs, const int* count, int max_segs, uint8_t* map, int B, int H, int W, hipStream_t s);
// image_io.hip: the image ends (image_host.cpp; include/pdengine.h "Image ends")
// Pillow's horizontal 8-bit pass: src [rows][Ws][3] u8 -> out [rows][W][3] u8 with bounds [W][2] = (xmin, count <= ksize), kk [W][ksize]
int launch_image_hpass(const uint8_t* src, uint8_t* out, const int* bounds, const int* kk, int ksize, long long rows, int Ws, int W,
                       hipStream_t s);
// src [Bs][Hs][W][3] u8 -> channels c_off .. c_off + 2 of dst [B][C][H][W] fp32 = (u8 / 255) * mul + add; the vertical pass first when
// bounds is non-null (bounds [H][2], kk [H][ksize]), else Hs == H; B a multiple of Bs: sample b reads b / (B / Bs), or b % Bs with `tile`
int launch_image_vpass(const uint8_t* src, float* dst, const int* bounds, const int* kk, int ksize, int Bs, int Hs, int H, int W, int B,
                       int C, int c_off, int tile, float mul, float add, hipStream_t s);
// src [B][C][H][W] fp32, C in {1, 3} -> dst [B][H][W][C] u8 = round(min(max(x * mul + add, 0), 1) * 255), half to even or truncated
int launch_image_store(const float* src, uint8_t* dst, int B, int C, int H, int W, float mul, float add, int trunc, hipStream_t s);
// clip_vision.hip: the CLIP image tower's preprocessing and embedding kernels and the safety checker (clip_vision.cpp; include/pdengine.h
// "CLIP image tower").  Output modes: PD_CLIP_OUT_*; rows of the checker: PD_SAFETY_SPECIAL, then PD_SAFETY_CONCEPTS
constexpr int CLIPV_OUT_PIXEL_VALUES = 0, CLIPV_OUT_PATCHES = 1, CLIPV_OUT_BYTES = 2;
constexpr int SAFETY_SPECIAL = 3, SAFETY_CONCEPTS = 17;
// Pillow's horizontal pass over crop columns only: src [B][H][W][3] u8, rows r0 .. r0 + Hn - 1 of every image -> tmp [B][Hn][S][3] u8;
// bounds [S][2] / kk [S][ksize]: the crop columns' rows of the axis tables
int launch_clipv_hpass(const uint8_t* src, uint8_t* tmp, const int* bounds, const int* kk, int ksize, int B, int H, int W, int r0, int Hn,
                       int S, hipStream_t s);
// in [B][Hin][Win][3] u8 -> the S x S crop in `mode`: fp32 [B][3][S][S] of (v / 255 - mean) / std, the patch operand rows
// [B (S / patch)^2][round_up(3 patch^2, 8)] in dt (element c patch^2 + py patch + px, pad columns zero), or the bytes [B][S][S][3].  Crop
// column x is in's column x_off + x.  bounds non-null: the vertical pass first (bounds [S][2] / kk [S][ksize] of the crop rows, in source
// rows; in's row 0 is source row row_off); else crop row y is in's row row_off + y
int launch_clipv_vpass(const uint8_t* in, void* dst, int mode, int dt, const int* bounds, const int* kk, int ksize, int B, int S, int Hin,
                       int Win, int x_off, int row_off, int patch, const float* mean, const float* sd, hipStream_t s);
int launch_clipv_patchify(const float* pv, void* out, int out_dt, int B, int S, int patch, hipStream_t s);   // fp32 [B][3][S][S] -> operand rows
// x [B][P + 1][C] fp32: row 0 = cls + pos[0], row 1 + t = patches[b P + t] + pos[1 + t]; C % 4 == 0
int launch_clipv_embed(const float* patches, const float* cls, const float* pos, float* x, int B, int P, int C, hipStream_t s);
// out [B][rows_out][C] fp32 = the first rows_out rows of every sample of x [B][L][C] (dt)
int launch_clipv_rows(const void* x, int dt, float* out, int B, int L, int C, int rows_out, hipStream_t s);
// StableDiffusionSafetyChecker.forward on embeds [B][D]: flags [B], scores [B][20] or null; everything fp32
int launch_safety_check(const float* embeds, const float* special, const float* cpt, const float* special_thr, const float* cpt_thr, int B,
                        int D, int* flags, float* scores, hipStream_t s);
int launch_safety_blank(float* images, const int* flags, int B, long long per, float value, hipStream_t s);   // images [B][per] = value where flags[b]
// canny.hip: the Canny edge detector (canny.cpp; include/pdengine.h "Canny edge detector").  States: PD_CANNY_NONE / WEAK / STRONG
constexpr int CANNY_NONE = 0, CANNY_WEAK = 1, CANNY_STRONG = 2;
// src [B][H][W][C] u8, C in {1, 3} -> states [B][H][W] u8: Sobel, channel select and non-maximum suppression; lo <= hi, both strict
int launch_canny_nms(const uint8_t* src, uint8_t* states, int B, int H, int W, int C, int lo, int hi, hipStream_t s);
// one sweep over states [B][H][W]: inside every tile, weak pixels 8-connected to a strong one become strong; *flag = 1 if any tile changed
int launch_canny_hysteresis(uint8_t* states, int B, int H, int W, int* flag, hipStream_t s);
// states -> dst_u8 [B][H][W] (255 where strong, else 0; may be null) and / or channels c_off .. c_off + 2 of dst_f [B][Cf][H][W] fp32 =
// (v / 255) * mul + add (may be null)
int launch_canny_emit(const uint8_t* states, uint8_t* dst_u8, float* dst_f, int B, int H, int W, int Cf, int c_off, float mul, float add,
                      hipStream_t s);
// sd3_kernels.hip: element-wise pieces of the MMDiT path
// y_dt == DT_FP8: y holds e4m3 bytes and y_scale[row] the row's scale (max |value| / 448); add: x <- x + add first (written back)
int launch_adaln(const void* x, int x_dt, void* y, int y_dt, const float* mod, int mod_stride, int shift_off, int scale_off, int rows,
                 int rows_per_sample, int C, float eps, hipStream_t s, float* y_scale = nullptr, const void* add = nullptr,
                 float* bound_out = nullptr, float bound_mul = 0.f, float bound_add = 0.f);   // bound_out[row] = |y_row|_2 * mul + add
// max over rows of the row L2 norm of W (dtype dt, row stride ld) and max |bias| -> out[0], out[1] (fp32, device, zeroed by the caller)
int launch_rows_norm_max(const void* W, int dt, int ld, const float* bias, int rows, int K, float* out, hipStream_t s);
// per-head RMSNorm (qk_norm = "rms_norm") of the q and k halves of a [rows][2 * heads * dh] buffer, in place: row r of sample b uses (wq, wk) when
// its token index < n_first, else (wq2, wk2) (the context stream's norm_added_q / norm_added_k); dh <= 64, dh % 8 == 0
int launch_qk_rmsnorm(void* qk, int dt, long long rows, int rows_per_sample, int n_first, int heads, int dh, const float* wq, const float* wk,
                      const float* wq2, const float* wk2, float eps, hipStream_t s);
int launch_patchify(const float* nchw, void* out, int out_dt, int B, int C, int H, int W, int patch, int Cpad, int Kpad, hipStream_t s);
// Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0) of B <= 64 host-side timesteps: out[b] = [cos(t f_i) | sin(t f_i)],
// f_i = exp(-ln(10000) i / 128); the values are passed by value (no host buffer has to outlive the launch)
int launch_timestep_embedding(const float* t_host, int B, float* out, hipStream_t s);
int launch_pos_crop(const float* table, float* out, int B, int h, int w, int max_size, int D, hipStream_t s);
int launch_unpatchify(const void* in, int in_dt, int ld, float* nchw, int B, int C, int h, int w, int patch, hipStream_t s);
int launch_cfg_euler(const float* v, float* x, int B, long long n, float guidance, float dsigma, int use_cfg, hipStream_t s);
// One launch of sd3_update_kernel (the img2img / inpainting / seeded forms of the SD3 loop; include/pdengine.h, pd_sd3_loop_args).
// Everything is fp32 NCHW, `per` = C * HW elements per sample.
//   v null  -- the start state: x = pure ? eps : sigma eps + (1 - sigma) z0
//   v set   -- one step: x' = cfg_euler_kernel's update of x; with a mask x = (1 - m) k + m x', k = (1 - sigma) z0 + sigma eps
// eps is read from `eps`, or drawn at (PD_RNG_XT, draw 0, sample_base + b, element) when rng_state is set (then eps must be null).
// The result goes to x and, when x_in is set (the CFG loop), to both halves of x_in [2B, per].
struct Sd3Update {
    const float* v = nullptr;      // [B or 2B, per]: [negative ; positive] under use_cfg
    float* x = nullptr;            // [B, per]
    float* x_in = nullptr;         // [2B, per] or null
    const float* z0 = nullptr;     // [B, per]; needed unless pure (start) / without a mask (step)
    const float* mask = nullptr;   // [B, HW]; step launches only
    const float* eps = nullptr;    // [B, per]
    const uint32_t* rng_state = nullptr;
    int B = 0, HW = 0;
    long long per = 0;
    float guidance = 0.f, dsigma = 0.f, sigma = 0.f;   // sigma: sigma_0 for the start, sigma_{i+1} for the blend of step i
    int use_cfg = 0, pure = 0;
};
int launch_sd3_update(const Sd3Update& u, hipStream_t s);
// x_in[d * B + b] = x_state[b] for d < dup, both [., HW, Cpad] fp32
int launch_fill_x_in(const float* x_state, float* x_in, int B, int dup, int Cpad, int HW, hipStream_t s);
