// pdengine: the element-wise kernels of the CLIP image tower and the safety checker (host side in clip_vision.cpp; contract in
// include/pdengine.h, "CLIP image tower").  All HBM-bound or tiny:
//   clipv_hpass_kernel   u8 [B][H][W][3] -> u8 [B][Hn][S][3]: Pillow's horizontal 8-bit pass over the S crop columns of the Hn source
//                        rows the vertical pass reads (image_io.hip's arithmetic, other indexing)
//   clipv_vpass_kernel   -> the vertical pass over the S crop rows, then (v / 255 - mean) / std, written as fp32 NCHW pixel_values, as the
//                        patch GEMM's operand rows, or as the bytes themselves; a thread owns two neighbouring pixels of a row
//   clipv_patchify_kernel  fp32 pixel_values [B][3][S][S] -> the same operand rows
//   clipv_embed_kernel   patch GEMM output + class row + position embedding -> [B][P + 1][C] fp32
//   clipv_rows_kernel    the first rows of every sample of a [B][L][C] tensor -> fp32 (hidden-state read-out, class-row gather)
//   safety_check_kernel  StableDiffusionSafetyChecker.forward on image_embeds, one block per image
//   safety_blank_kernel  a constant over the flagged images of a batch
#include "pd_common.h"

namespace {

constexpr int TPB = 256;
constexpr int PX = 4;             // pixels per thread, horizontal pass
constexpr int kPrecBits = 22;     // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecBits;   // arithmetic shift, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (v / 255 - mean) / std, each operation rounded once: CLIPImageProcessor's rescale + normalize in float32
__device__ __forceinline__ float clip_normalize(int u, float mean, float sd) {
#pragma clang fp contract(off)
    const float v = __fdiv_rn((float)u, 255.0f);
    const float d = v - mean;
    return __fdiv_rn(d, sd);
}

// tmp[b][r][x][c] = clip8(2^21 + sum_j src[b][r0 + r][xmin(x) + j][c] * kk[x][j]) for r < Hn, x < S; bounds / kk are the crop columns'
// rows of the axis tables, xmin + count <= W by construction.  vec: S % 4 == 0 (tmp is 4-byte aligned)
__global__ __launch_bounds__(TPB) void clipv_hpass_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int B,
                                                           int H, int W, int r0, int Hn, int S, int vec) {
    const int gw = (S + PX - 1) / PX;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * Hn * gw) return;
    const int x0 = (int)(i % gw) * PX;
    const int r = (int)((i / gw) % Hn);
    const int b = (int)(i / ((long long)gw * Hn));
    const int n = min(PX, S - x0);
    const uint8_t* row = src + ((long long)b * H + r0 + r) * W * 3;
    int v[3 * PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        int s0 = 1 << (kPrecBits - 1), s1 = s0, s2 = s0;
        if (p < n) {
            const int x = x0 + p;
            const int xmin = bounds[2 * x], cnt = bounds[2 * x + 1];
            const int* k = kk + (long long)x * ksize;
            const uint8_t* q = row + (long long)xmin * 3;
            for (int j = 0; j < cnt; ++j) {
                const int w = k[j];
                s0 += (int)q[3 * j] * w;
                s1 += (int)q[3 * j + 1] * w;
                s2 += (int)q[3 * j + 2] * w;
            }
        }
        v[3 * p] = clip8(s0); v[3 * p + 1] = clip8(s1); v[3 * p + 2] = clip8(s2);
    }
    uint8_t* o = tmp + (((long long)b * Hn + r) * S + x0) * 3;
    if (vec && n == PX) {
        uint32_t* q = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int e = 0; e < 3; ++e)
            q[e] = (uint32_t)v[4 * e] | ((uint32_t)v[4 * e + 1] << 8) | ((uint32_t)v[4 * e + 2] << 16) | ((uint32_t)v[4 * e + 3] << 24);
    } else {
#pragma unroll
        for (int e = 0; e < 3 * PX; ++e)
            if (e < 3 * n) o[e] = (uint8_t)v[e];
    }
}

struct VpassGeom {
    int B, S;
    int Hin, Win;      // rows per image and pixels per row of `in`
    int x_off;         // first crop column inside a row of `in`
    int row_off;       // RESIZE: source row of in's row 0 (bounds hold source rows); else: in's row of output row 0
    int patch, G, Kw;  // PATCHES: patch size, patches per side, operand row width
    int pair;          // S even (and patch even for PATCHES) and the destination aligned for two-element stores
};

// One thread: pixels x, x + 1 of crop row y of image b.  MODE: CLIPV_OUT_*; DT: the operand type of PATCHES.
template <bool RESIZE, int MODE, int DT>
__global__ __launch_bounds__(TPB) void clipv_vpass_kernel(const uint8_t* __restrict__ in, void* __restrict__ dst,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           VpassGeom g, float m0, float m1, float m2, float d0, float d1, float d2) {
    const int S = g.S, gw = (S + 1) / 2;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)g.B * S * gw) return;
    const int x = (int)(i % gw) * 2;
    const int y = (int)((i / gw) % S);
    const int b = (int)(i / ((long long)gw * S));
    const int n = min(2, S - x);
    int u[6];
    if (RESIZE) {
        const int ymin = bounds[2 * y], cnt = bounds[2 * y + 1];
        const int* k = kk + (long long)y * ksize;
        int s[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) s[e] = 1 << (kPrecBits - 1);
        const uint8_t* q = in + (((long long)b * g.Hin + (ymin - g.row_off)) * g.Win + g.x_off + x) * 3;
        for (int j = 0; j < cnt; ++j, q += (long long)g.Win * 3) {
            const int w = k[j];
#pragma unroll
            for (int e = 0; e < 6; ++e)
                if (e < 3 * n) s[e] += (int)q[e] * w;
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) u[e] = clip8(s[e]);
    } else {
        const uint8_t* q = in + (((long long)b * g.Hin + g.row_off + y) * g.Win + g.x_off + x) * 3;
#pragma unroll
        for (int e = 0; e < 6; ++e) u[e] = e < 3 * n ? (int)q[e] : 0;
    }
    if constexpr (MODE == CLIPV_OUT_BYTES) {
        uint8_t* o = reinterpret_cast<uint8_t*>(dst) + (((long long)b * S + y) * S + x) * 3;
#pragma unroll
        for (int e = 0; e < 6; ++e)
            if (e < 3 * n) o[e] = (uint8_t)u[e];
        return;
    }
    const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
    float f[3][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) f[c][p] = clip_normalize(u[3 * p + c], mean[c], sd[c]);
    const bool two = g.pair && n == 2;
    if constexpr (MODE == CLIPV_OUT_PIXEL_VALUES) {
        float* o = reinterpret_cast<float*>(dst) + ((long long)b * 3 * S + y) * S + x;
#pragma unroll
        for (int c = 0; c < 3; ++c, o += (long long)S * S) {
            if (two) *reinterpret_cast<float2*>(o) = make_float2(f[c][0], f[c][1]);
            else {
                o[0] = f[c][0];
                if (n == 2) o[1] = f[c][1];
            }
        }
    } else {
        // operand row b G^2 + ty G + tx, element c p^2 + py p + px; with p even a pair never straddles two patches
        const int p = g.patch, pp = p * p;
        const int ty = y / p, py = y - ty * p;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q == 1 && (two || n < 2)) break;
            const int xx = x + q, tx = xx / p, px = xx - tx * p;
            const long long base = (((long long)b * g.G + ty) * g.G + tx) * g.Kw + py * p + px;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long at = base + (long long)c * pp;
                if constexpr (DT == DT_F32) {
                    float* o = reinterpret_cast<float*>(dst) + at;
                    if (two) *reinterpret_cast<float2*>(o) = make_float2(f[c][0], f[c][1]);
                    else o[0] = f[c][q];
                } else {
                    uint16_t* o = reinterpret_cast<uint16_t*>(dst) + at;
                    if (two) *reinterpret_cast<uint32_t*>(o) = pack2<DT>(f[c][0], f[c][1]);
                    else o[0] = cvt16<DT>(f[c][q]);
                }
            }
            if (py == 0 && px == 0) {   // the first pixel of a patch also clears the row's pad columns
                const long long row = (((long long)b * g.G + ty) * g.G + tx) * g.Kw;
                for (int k = 3 * pp; k < g.Kw; ++k) {
                    if constexpr (DT == DT_F32) reinterpret_cast<float*>(dst)[row + k] = 0.f;
                    else reinterpret_cast<uint16_t*>(dst)[row + k] = 0;
                }
            }
        }
    }
}

template <int DT>
__global__ __launch_bounds__(TPB) void clipv_patchify_kernel(const float* __restrict__ pv, void* __restrict__ out, int B, int S, int p,
                                                              int Kw) {
    const int G = S / p, pp = p * p;
    const long long total = (long long)B * G * G * Kw;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int k = (int)(i % Kw);
        const long long r = i / Kw;
        float val = 0.f;
        if (k < 3 * pp) {
            const int c = k / pp, py = (k - c * pp) / p, px = k - c * pp - py * p;
            const int tx = (int)(r % G), ty = (int)((r / G) % G), b = (int)(r / ((long long)G * G));
            val = pv[(((long long)b * 3 + c) * S + ty * p + py) * S + tx * p + px];
        }
        if constexpr (DT == DT_F32) reinterpret_cast<float*>(out)[i] = val;
        else reinterpret_cast<uint16_t*>(out)[i] = cvt16<DT>(val);
    }
}

// x[b][0] = cls + pos[0]; x[b][1 + t] = patches[b P + t] + pos[1 + t]; four channels per thread (C % 4 == 0)
__global__ __launch_bounds__(TPB) void clipv_embed_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, float* __restrict__ x, int B, int P, int C) {
    const int c4 = C / 4;
    const long long total = (long long)B * (P + 1) * c4;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % c4) * 4;
    const int r = (int)((i / c4) % (P + 1));
    const int b = (int)(i / ((long long)c4 * (P + 1)));
    const f32x4 a = r == 0 ? *reinterpret_cast<const f32x4*>(cls + c)
                           : *reinterpret_cast<const f32x4*>(patches + ((long long)b * P + r - 1) * C + c);
    const f32x4 e = *reinterpret_cast<const f32x4*>(pos + (long long)r * C + c);
    *reinterpret_cast<f32x4*>(x + ((long long)b * (P + 1) + r) * C + c) = a + e;
}

// out[b][r] = x[b][r] for r < rows_out (fp32), x [B][L][C] in dt
__global__ __launch_bounds__(TPB) void clipv_rows_kernel(const void* __restrict__ x, int dt, float* __restrict__ out, int B, int L, int C,
                                                          int rows_out) {
    const int c4 = C / 4;
    const long long total = (long long)B * rows_out * c4;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % c4) * 4;
    const int r = (int)((i / c4) % rows_out);
    const int b = (int)(i / ((long long)c4 * rows_out));
    const f32x4 v = load4(x, ((size_t)b * L + r) * C + c, dt);
    *reinterpret_cast<f32x4*>(out + ((long long)b * rows_out + r) * C + c) = v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int kRows = SAFETY_SPECIAL + SAFETY_CONCEPTS;

// One block per image.  Wave w takes rows w, w + 4, ... of [special | concept]: cos = e . r / (|e| |r|); thread 0 then walks the scores in
// diffusers' order.  A score is positive iff it exceeds 0.0005 (the comparison is made in double: exact for every fp32 score).
__global__ __launch_bounds__(TPB) void safety_check_kernel(const float* __restrict__ embeds, const float* __restrict__ special,
                                                            const float* __restrict__ cpt, const float* __restrict__ special_thr,
                                                            const float* __restrict__ cpt_thr, int D, int* __restrict__ flags,
                                                            float* __restrict__ scores) {
    __shared__ float cosv[kRows];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* e = embeds + (long long)b * D;
    float ee = 0.f;
    for (int k = lane; k < D; k += 64) ee += e[k] * e[k];
    ee = wave_sum(ee);
    for (int j = wave; j < kRows; j += TPB / 64) {
        const float* r = j < SAFETY_SPECIAL ? special + (long long)j * D : cpt + (long long)(j - SAFETY_SPECIAL) * D;
        float er = 0.f, rr = 0.f;
        for (int k = lane; k < D; k += 64) {
            const float v = r[k];
            er += e[k] * v;
            rr += v * v;
        }
        er = wave_sum(er);
        rr = wave_sum(rr);
        if (lane == 0) cosv[j] = er / (sqrtf(ee) * sqrtf(rr));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float adj = 0.f;
        int flag = 0;
        for (int j = 0; j < kRows; ++j) {
            const float thr = j < SAFETY_SPECIAL ? special_thr[j] : cpt_thr[j - SAFETY_SPECIAL];
            const float s = cosv[j] - thr + adj;
            if (scores) scores[(long long)b * kRows + j] = s;
            if ((double)s > 0.0005) {
                if (j < SAFETY_SPECIAL) adj = 0.01f;
                else flag = 1;
            }
        }
        flags[b] = flag;
    }
}

__global__ __launch_bounds__(TPB) void safety_blank_kernel(float* __restrict__ images, const int* __restrict__ flags, int B,
                                                            long long per, float value) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * per) return;
    if (flags[i / per]) images[i] = value;
}

inline bool grid_for(long long threads, dim3& grid) {
    const long long blocks = (threads + TPB - 1) / TPB;
    if (threads < 1 || blocks > 0x7fffffffll) return false;
    grid = dim3((unsigned)blocks);
    return true;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <bool RESIZE, int MODE>
void launch_vpass_dt(int dt, dim3 grid, hipStream_t s, const uint8_t* in, void* dst, const int* bounds, const int* kk, int ksize,
                     const VpassGeom& g, const float* mean, const float* sd) {
#define PD_CLIPV(DT) hipLaunchKernelGGL((clipv_vpass_kernel<RESIZE, MODE, DT>), grid, dim3(TPB), 0, s, in, dst, bounds, kk, ksize, g, mean[0], \
                                        mean[1], mean[2], sd[0], sd[1], sd[2])
    if constexpr (MODE == CLIPV_OUT_PATCHES) {   // only the operand rows have a type: the other modes exist once
        if (dt == DT_F32) PD_CLIPV(DT_F32);
        else if (dt == DT_F16) PD_CLIPV(DT_F16);
        else PD_CLIPV(DT_BF16);
    } else {
        PD_CLIPV(DT_F32);
    }
#undef PD_CLIPV
}

}  // namespace

int launch_clipv_hpass(const uint8_t* src, uint8_t* tmp, const int* bounds, const int* kk, int ksize, int B, int H, int W, int r0, int Hn,
                       int S, hipStream_t s) {
    dim3 grid;
    if (B < 1 || H < 1 || W < 1 || ksize < 1 || r0 < 0 || Hn < 1 || r0 + Hn > H || S < 1) return 1;
    if (!grid_for((long long)B * Hn * ((S + PX - 1) / PX), grid)) return 1;
    hipLaunchKernelGGL(clipv_hpass_kernel, grid, dim3(TPB), 0, s, src, tmp, bounds, kk, ksize, B, H, W, r0, Hn, S,
                       (int)(S % PX == 0 && aligned(tmp, 4)));
    return hipGetLastError() != hipSuccess;
}

int launch_clipv_vpass(const uint8_t* in, void* dst, int mode, int dt, const int* bounds, const int* kk, int ksize, int B, int S, int Hin,
                       int Win, int x_off, int row_off, int patch, const float* mean, const float* sd, hipStream_t s) {
    dim3 grid;
    if (B < 1 || S < 1 || Hin < 1 || Win < 1 || x_off < 0 || x_off + S > Win) return 1;
    const bool resize = bounds != nullptr;
    if (!resize && (row_off < 0 || row_off + S > Hin)) return 1;
    VpassGeom g{};
    g.B = B; g.S = S; g.Hin = Hin; g.Win = Win; g.x_off = x_off; g.row_off = row_off;
    g.pair = S % 2 == 0 && aligned(dst, 8);
    if (mode == CLIPV_OUT_PATCHES) {
        if (patch < 1 || S % patch) return 1;
        g.patch = patch; g.G = S / patch; g.Kw = (3 * patch * patch + 7) / 8 * 8;
        g.pair = g.pair && patch % 2 == 0;
        if ((long long)B * g.G * g.G * g.Kw >= (1ll << 40)) return 1;
    } else if (mode != CLIPV_OUT_PIXEL_VALUES && mode != CLIPV_OUT_BYTES) {
        return 1;
    }
    if (!grid_for((long long)B * S * ((S + 1) / 2), grid)) return 1;
#define PD_CLIPV_MODE(R)                                                                                                      \
    do {                                                                                                                      \
        if (mode == CLIPV_OUT_PATCHES) launch_vpass_dt<R, CLIPV_OUT_PATCHES>(dt, grid, s, in, dst, bounds, kk, ksize, g, mean, sd);           \
        else if (mode == CLIPV_OUT_BYTES) launch_vpass_dt<R, CLIPV_OUT_BYTES>(dt, grid, s, in, dst, bounds, kk, ksize, g, mean, sd);          \
        else launch_vpass_dt<R, CLIPV_OUT_PIXEL_VALUES>(dt, grid, s, in, dst, bounds, kk, ksize, g, mean, sd);                                  \
    } while (0)
    if (resize) PD_CLIPV_MODE(true);
    else PD_CLIPV_MODE(false);
#undef PD_CLIPV_MODE
    return hipGetLastError() != hipSuccess;
}

int launch_clipv_patchify(const float* pv, void* out, int out_dt, int B, int S, int patch, hipStream_t s) {
    if (B < 1 || patch < 1 || S < patch || S % patch) return 1;
    const int Kw = (3 * patch * patch + 7) / 8 * 8;
    const long long total = (long long)B * (S / patch) * (S / patch) * Kw;
    const int blocks = (int)((total + TPB - 1) / TPB < 4096 ? (total + TPB - 1) / TPB : 4096);
    if (out_dt == DT_F32) hipLaunchKernelGGL((clipv_patchify_kernel<DT_F32>), dim3(blocks), dim3(TPB), 0, s, pv, out, B, S, patch, Kw);
    else if (out_dt == DT_F16) hipLaunchKernelGGL((clipv_patchify_kernel<DT_F16>), dim3(blocks), dim3(TPB), 0, s, pv, out, B, S, patch, Kw);
    else hipLaunchKernelGGL((clipv_patchify_kernel<DT_BF16>), dim3(blocks), dim3(TPB), 0, s, pv, out, B, S, patch, Kw);
    return hipGetLastError() != hipSuccess;
}

int launch_clipv_embed(const float* patches, const float* cls, const float* pos, float* x, int B, int P, int C, hipStream_t s) {
    dim3 grid;
    if (B < 1 || P < 1 || C < 4 || C % 4 || !grid_for((long long)B * (P + 1) * (C / 4), grid)) return 1;
    hipLaunchKernelGGL(clipv_embed_kernel, grid, dim3(TPB), 0, s, patches, cls, pos, x, B, P, C);
    return hipGetLastError() != hipSuccess;
}

int launch_clipv_rows(const void* x, int dt, float* out, int B, int L, int C, int rows_out, hipStream_t s) {
    dim3 grid;
    if (B < 1 || L < 1 || rows_out < 1 || rows_out > L || C < 4 || C % 4 || !grid_for((long long)B * rows_out * (C / 4), grid)) return 1;
    hipLaunchKernelGGL(clipv_rows_kernel, grid, dim3(TPB), 0, s, x, dt, out, B, L, C, rows_out);
    return hipGetLastError() != hipSuccess;
}

int launch_safety_check(const float* embeds, const float* special, const float* cpt, const float* special_thr, const float* cpt_thr, int B,
                        int D, int* flags, float* scores, hipStream_t s) {
    if (B < 1 || D < 1) return 1;
    hipLaunchKernelGGL(safety_check_kernel, dim3(B), dim3(TPB), 0, s, embeds, special, cpt, special_thr, cpt_thr, D, flags, scores);
    return hipGetLastError() != hipSuccess;
}

int launch_safety_blank(float* images, const int* flags, int B, long long per, float value, hipStream_t s) {
    dim3 grid;
    if (B < 1 || per < 1 || !grid_for((long long)B * per, grid)) return 1;
    hipLaunchKernelGGL(safety_blank_kernel, grid, dim3(TPB), 0, s, images, flags, B, per, value);
    return hipGetLastError() != hipSuccess;
}
