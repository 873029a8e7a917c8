// pdengine: the element-wise kernels of the HED edge detector (annotator/hed/__init__.py; host side in hed.cpp).  All three are
// HBM-bound and read every input once:
//   hed_upload_kernel      NCHW fp32 RGB in [0, 1] -> NHWC in the compute type, BGR order, x * 255 - mean (Network.forward :72-73)
//   hed_stage_tail_kernel  a stage's last feature map -> its score map (netScore*: conv1x1 C -> 1) and the 2x2 max-pooled map
//   hed_fuse_kernel        five score maps -> bilinear upsamples (align_corners = False) -> netCombine -> sigmoid
#include "pd_common.h"

namespace {

constexpr int TPB = 256;

// out[b][p][c] for c < Cpad: channel c of the network input is B, G, R = image channel 2 - c; fp32 arithmetic, one rounding
__global__ __launch_bounds__(TPB) void hed_upload_kernel(const float* __restrict__ in, void* __restrict__ out, int out_dt, int B, int HW,
                                                          int Cpad) {
    const long long total = (long long)B * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW;
        const int p = (int)(i - b * HW);
        const float* src = in + b * 3 * HW + p;
        const float mean[3] = {104.00698793f, 116.66876762f, 122.67891434f};
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = src[(long long)(2 - c) * HW] * 255.0f - mean[c];
        if (out_dt == DT_F32) {
            float* o = reinterpret_cast<float*>(out) + i * Cpad;
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], 0.f};
            for (int c = 4; c < Cpad; c += 4) *reinterpret_cast<f32x4*>(o + c) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            uint16_t* o = reinterpret_cast<uint16_t*>(out) + i * Cpad;
            uint2 u;
            u.x = out_dt == DT_F16 ? pack2h(v[0], v[1]) : pack2bf(v[0], v[1]);
            u.y = out_dt == DT_F16 ? pack2h(v[2], 0.f) : pack2bf(v[2], 0.f);
            *reinterpret_cast<uint2*>(o) = u;
            for (int c = 4; c < Cpad; c += 4) *reinterpret_cast<uint2*>(o + c) = uint2{0u, 0u};
        }
    }
}

// 16 bytes of a feature row as floats: VEC = 4 (fp32) or 8 (2-byte types)
template <int DT> struct HedVec;
template <> struct HedVec<DT_F32> {
    static constexpr int VEC = 4;
    typedef f32x4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3]; }
    static __device__ __forceinline__ raw pack(const float* f) { return f32x4{f[0], f[1], f[2], f[3]}; }
};
template <> struct HedVec<DT_F16> {
    static constexpr int VEC = 8;
    typedef uint4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { unpack8<DT_F16>(r, f); }
    static __device__ __forceinline__ raw pack(const float* f) { return pack8<DT_F16>(f); }
};
template <> struct HedVec<DT_BF16> {
    static constexpr int VEC = 8;
    typedef uint4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float* f) { unpack8<DT_BF16>(r, f); }
    static __device__ __forceinline__ raw pack(const float* f) { return pack8<DT_BF16>(f); }
};

// One group of G lanes (a power of two <= 64, aligned inside a wave) per 2x2 pixel quad; lane l of the group owns the 16-byte channel
// chunks l, l + G, ..  For every chunk it loads the quad's four rows once, adds their products with the score weights to four fp32
// sums and stores the element-wise maximum as the pooled row; a butterfly over the group then finishes the four dot products.
//   x [B][H][W][C] (post-ReLU), sw [C] fp32, sb [1]; score [B][H][W] fp32; pooled [B][H/2][W/2][C] in x's type, or null (stage 5).
// Quads cover ceil(H / 2) x ceil(W / 2): pixels past the bottom / right edge are neither read nor written (odd sizes only without pooling).
template <int DT>
__global__ __launch_bounds__(TPB) void hed_stage_tail_kernel(const void* __restrict__ x, const float* __restrict__ sw, const float* __restrict__ sb,
                                                              float* __restrict__ score, void* __restrict__ pooled, int B, int H, int W, int C,
                                                              int G) {
    typedef HedVec<DT> V;
    typedef typename V::raw raw;
    constexpr int VEC = V::VEC;
    const int qh = (H + 1) >> 1, qw = (W + 1) >> 1;
    const long long nquad = (long long)B * qh * qw;
    const long long quad = ((long long)blockIdx.x * TPB + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    // (a whole group leaves together: the butterfly below stays inside groups that run)
    if (quad >= nquad) return;
    const int qx = (int)(quad % qw);
    const int qy = (int)((quad / qw) % qh);
    const long long b = quad / ((long long)qw * qh);
    const int y0 = 2 * qy, x0 = 2 * qx;
    const bool vy = y0 + 1 < H, vx = x0 + 1 < W;
    const raw* r00 = reinterpret_cast<const raw*>(x) + ((b * H + y0) * W + x0) * (C / VEC);
    const raw* r01 = r00 + (vx ? C / VEC : 0);               // out-of-range pixels alias (0, 0): valid reads, results dropped
    const raw* r10 = r00 + (vy ? (long long)W * (C / VEC) : 0);
    const raw* r11 = r10 + (vx ? C / VEC : 0);
    raw* po = pooled ? reinterpret_cast<raw*>(pooled) + ((b * (H >> 1) + qy) * (W >> 1) + qx) * (C / VEC) : nullptr;
    float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
    for (int ch = gl; ch < C / VEC; ch += G) {
        const raw a = r00[ch], bq = r01[ch], c = r10[ch], d = r11[ch];
        float fa[VEC], fb[VEC], fc[VEC], fd[VEC], w[VEC], m[VEC];
        V::unpack(a, fa); V::unpack(bq, fb); V::unpack(c, fc); V::unpack(d, fd);
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(sw + ch * VEC + k);
            w[k] = wv[0]; w[k + 1] = wv[1]; w[k + 2] = wv[2]; w[k + 3] = wv[3];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            s00 = fmaf(fa[k], w[k], s00);
            s01 = fmaf(fb[k], w[k], s01);
            s10 = fmaf(fc[k], w[k], s10);
            s11 = fmaf(fd[k], w[k], s11);
            m[k] = fmaxf(fmaxf(fa[k], fb[k]), fmaxf(fc[k], fd[k]));
        }
        if (po) po[ch] = V::pack(m);   // the maximum of four values of the storage type is one of them: no rounding
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        s00 += __shfl_xor(s00, o);
        s01 += __shfl_xor(s01, o);
        s10 += __shfl_xor(s10, o);
        s11 += __shfl_xor(s11, o);
    }
    if (gl == 0) {
        const float bias = sb[0];
        float* so = score + (b * H + y0) * W + x0;
        so[0] = s00 + bias;
        if (vx) so[1] = s01 + bias;
        if (vy) so[W] = s10 + bias;
        if (vy && vx) so[W + 1] = s11 + bias;
    }
}

struct HedMaps { const float* s[5]; };

// PyTorch's upsample_bilinear2d with align_corners = False along one axis: source index and weights of output index d for an input of
// n = N >> lvl entries (scale = n / N = 2^-lvl, exact)
__device__ __forceinline__ void hed_axis(int d, int lvl, int n, int& i0, int& i1, float& l0, float& l1) {
    const float scale = 1.0f / (float)(1 << lvl);
    const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
    i0 = (int)src;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// out[b][y][x] = sigmoid(cb + sum_i cw[i] up_i[b][y][x])  (what 0: [B][1][H][W]), or the five up_i themselves (what 1: [B][5][H][W]);
// up_i = bilinear upsample of score map i [B][H >> i][W >> i] by 2^i.  fp32, products and sums kept apart (no contraction) in the
// order ATen's separable kernel evaluates them: along x first, then along y
__global__ __launch_bounds__(TPB) void hed_fuse_kernel(HedMaps maps, const float* __restrict__ cw, const float* __restrict__ cb,
                                                        float* __restrict__ out, int B, int H, int W, int what) {
#pragma clang fp contract(off)
    const long long total = (long long)B * H * W;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const long long b = i / ((long long)W * H);
    float up[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        const int h = H >> l, w = W >> l;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        hed_axis(y, l, h, y0, y1, ly0, ly1);
        hed_axis(x, l, w, x0, x1, lx0, lx1);
        const float* s = maps.s[l] + b * h * w;
        const float t0 = lx0 * s[(long long)y0 * w + x0] + lx1 * s[(long long)y0 * w + x1];
        const float t1 = lx0 * s[(long long)y1 * w + x0] + lx1 * s[(long long)y1 * w + x1];
        up[l] = ly0 * t0 + ly1 * t1;
    }
    if (what == 1) {
#pragma unroll
        for (int l = 0; l < 5; ++l) out[((b * 5 + l) * H + y) * W + x] = up[l];
        return;
    }
    float acc = cw[0] * up[0];
#pragma unroll
    for (int l = 1; l < 5; ++l) acc = acc + cw[l] * up[l];
    acc = acc + cb[0];
    out[i] = 1.0f / (1.0f + expf(-acc));
}

}  // namespace

int launch_hed_upload(const float* in, void* out, int out_dt, int B, int H, int W, int Cpad, hipStream_t s) {
    if (Cpad < 4 || Cpad % 4) return 1;
    long long g = ((long long)B * H * W + TPB - 1) / TPB;
    if (g > (1 << 20)) g = 1 << 20;   // grid-stride beyond that
    hipLaunchKernelGGL(hed_upload_kernel, dim3((unsigned)g), dim3(TPB), 0, s, in, out, out_dt, B, H * W, Cpad);
    return hipGetLastError() != hipSuccess;
}

int launch_hed_stage_tail(const void* x, int dt, const float* sw, const float* sb, float* score, void* pooled, int B, int H, int W, int C,
                          hipStream_t s) {
    const int vec = dt == DT_F32 ? 4 : 8;
    if (B < 1 || H < 1 || W < 1 || C < vec || C % vec) return 1;
    if (pooled && ((H | W) & 1)) return 1;   // the pooled map needs whole quads
    int G = 1;
    while (G < 64 && G * 2 * vec <= C) G *= 2;   // lanes per quad: the largest power of two <= min(64, C / vec)
    const long long nquad = (long long)B * ((H + 1) / 2) * ((W + 1) / 2);
    const long long blocks = (nquad * G + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    const dim3 grid((unsigned)blocks), blk(TPB);
    if (dt == DT_F32) hipLaunchKernelGGL(hed_stage_tail_kernel<DT_F32>, grid, blk, 0, s, x, sw, sb, score, pooled, B, H, W, C, G);
    else if (dt == DT_F16) hipLaunchKernelGGL(hed_stage_tail_kernel<DT_F16>, grid, blk, 0, s, x, sw, sb, score, pooled, B, H, W, C, G);
    else if (dt == DT_BF16) hipLaunchKernelGGL(hed_stage_tail_kernel<DT_BF16>, grid, blk, 0, s, x, sw, sb, score, pooled, B, H, W, C, G);
    else return 1;
    return hipGetLastError() != hipSuccess;
}

int launch_hed_fuse(const float* const scores[5], const float* cw, const float* cb, float* out, int B, int H, int W, int what, hipStream_t s) {
    if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16 || (what != 0 && what != 1)) return 1;
    HedMaps m;
    for (int i = 0; i < 5; ++i) m.s[i] = scores[i];
    const long long blocks = ((long long)B * H * W + TPB - 1) / TPB;
    if (blocks > 0x7fffffffll) return 1;
    hipLaunchKernelGGL(hed_fuse_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, m, cw, cb, out, B, H, W, what);
    return hipGetLastError() != hipSuccess;
}
