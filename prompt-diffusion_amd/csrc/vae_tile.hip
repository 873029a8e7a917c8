// Tiled VAE decode / encode (pd_vae_set_tiling): the two layout kernels at the ends of a tiled call (gfx950).
//   vae_tile_gather_kernel   windows of the fp32 NCHW source -> a batch of equal-shape NHWC tiles in the compute type: the windowed
//                            form of nchw_to_nhwc_kernel (elementwise.hip), same scale / shift arithmetic and zeroed pad channels
//   vae_tile_blend_kernel    the decoded tiles (fp32 NHWC, as conv_gn / quant_conv leave them) -> the assembled output, written once:
//                            diffusers' blend_v / blend_h / crop / cat in closed form
// Both are bandwidth bound: the gather moves the small side of the VAE, the blend reads each kept tile pixel once (the overlap bands up
// to four times) and takes the place of the exit nhwc_to_nchw launch -- the full-size image makes no extra trip through HBM.
#include "../../include/pdengine.h"
#include "pd_common.h"

namespace {

constexpr int TPB = 256;
inline int nblocks(long long n, int per = TPB, int cap = 65535 * 16) {
    long long b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// entry = tile * B + b; out[entry][y][x][c] = scale * in[b][c][oy + y][ox + x] (+ shift), 0 for c >= C.  c is the fastest thread
// index like in nchw_to_nhwc_kernel: the writes are contiguous, the reads of one channel contiguous along x.
__global__ void vae_tile_gather_kernel(const float* __restrict__ in, void* __restrict__ out, int out_dt, const int* __restrict__ origins,
                                       int ntile, int B, int C, int H, int W, int th, int tw, int Cpad, float scale, float shift) {
    const long long total = (long long)ntile * B * th * tw * Cpad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        long long r = i / Cpad;
        const int x = (int)(r % tw);
        r /= tw;
        const int y = (int)(r % th);
        const int entry = (int)(r / th);
        const int b = entry % B, t = entry / B;
        const int sy = origins[2 * t] + y, sx = origins[2 * t + 1] + x;
        float v = c < C ? scale * in[(((long long)b * C + c) * H + sy) * W + sx] : 0.f;
        if (shift != 0.f && c < C) v += shift;   // (shift 0 keeps the product's own bits, -0 included)
        if (out_dt == DT_F32) reinterpret_cast<float*>(out)[i] = v;
        else reinterpret_cast<uint16_t*>(out)[i] = cvt16_rt(v, out_dt);
    }
}

// a * wa + b * wb with every product and the sum rounded on its own (no FMA contraction): torch's a * (1 - y / e) + b * (y / e)
// (HIP's __fmul_rn / __fadd_rn are plain * and + to the compiler, and under the default -ffp-contract=fast the backend fuses them
// whatever a pragma says: passing each rounded product through an empty asm statement is what keeps the three roundings apart)
__device__ __forceinline__ float rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ f32x4 mix4(f32x4 a, float wa, f32x4 b, float wb) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = __fadd_rn(rounded(__fmul_rn(a[k], wa)), rounded(__fmul_rn(b[k], wb)));
    return r;
}

// One thread per output pixel and group of four channels.  The pixel lies in the kept rectangle of exactly one tile (ti, tj) =
// (Y / limit, X / limit); inside the top band (y < e_v) and the left band (x < e_h) it also reads the tile above, the tile to the
// left and the one above-left, all raw.  Nothing is written back to the tiles.  Reads are float4 along the tiles' x axis; writes
// are float4 (NHWC moments) or one float per channel plane, contiguous along X (NCHW images).
__global__ void vae_tile_blend_kernel(VaeBlendParams p) {
    const int G = p.Cpad / 4;
    const long long total = (long long)p.B * p.H * p.W * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        long long r = i / G;
        const int X = (int)(r % p.W);
        r /= p.W;
        const int Y = (int)(r % p.H);
        const int b = (int)(r / p.H);
        const int ti = Y / p.limit, tj = X / p.limit;
        const int y = Y - ti * p.limit, x = X - tj * p.limit;
        const int th = p.rows[4 * ti], ev = p.rows[4 * ti + 1];
        const int tw = p.cols[4 * tj], eh = p.cols[4 * tj + 1];
        const float* wv = p.wtab + p.rows[4 * ti + 2];   // wv[y] = 1 - y / e_v, wv[e_v + y] = y / e_v
        const float* wh = p.wtab + p.cols[4 * tj + 2];
        auto ld = [&](int ri, int ci, int hh, int ww, int yy, int xx) {
            const float* t = p.tiles + p.tile_off[ri * p.ncol + ci] + (((long long)b * hh + yy) * ww + xx) * p.Cpad + 4 * g;
            return *reinterpret_cast<const f32x4*>(t);
        };
        f32x4 v = ld(ti, tj, th, tw, y, x);
        const bool inv = y < ev, inh = x < eh;
        const int ah = inv ? p.rows[4 * (ti - 1)] : 0, lw = inh ? p.cols[4 * (tj - 1)] : 0;
        const int ay = ah - ev + y, lx = lw - eh + x;
        if (inv) {
            f32x4 a = ld(ti - 1, tj, ah, tw, ay, x);
            if (inh) a = mix4(ld(ti - 1, tj - 1, ah, lw, ay, lx), wh[x], a, wh[eh + x]);
            v = mix4(a, wv[y], v, wv[ev + y]);
        }
        if (inh) {
            f32x4 l = ld(ti, tj - 1, th, lw, y, lx);
            if (inv) l = mix4(ld(ti - 1, tj - 1, ah, lw, ay, lx), wv[y], l, wv[ev + y]);
            v = mix4(l, wh[x], v, wh[eh + x]);
        }
        if (p.nchw) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < p.C) p.out[(((long long)b * p.C + 4 * g + k) * p.H + Y) * p.W + X] = v[k];
        } else {
            *reinterpret_cast<f32x4*>(p.out + (((long long)b * p.H + Y) * p.W + X) * p.Cpad + 4 * g) = v;
        }
    }
}

}  // namespace

#define CHECK_LAUNCH() return hipGetLastError() == hipSuccess ? 0 : 1

int launch_vae_tile_gather(const float* in, void* out, int out_dt, const int* origins, int ntile, int B, int C, int H, int W, int th, int tw,
                           int Cpad, float scale, float shift, hipStream_t s) {
    if (ntile < 1 || B < 1 || th < 1 || tw < 1 || th > H || tw > W || C > Cpad) return 1;
    const long long n = (long long)ntile * B * th * tw * Cpad;
    hipLaunchKernelGGL(vae_tile_gather_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, in, out, out_dt, origins, ntile, B, C, H, W, th, tw, Cpad,
                       scale, shift);
    CHECK_LAUNCH();
}

int launch_vae_tile_blend(const VaeBlendParams& p, hipStream_t s) {
    if (p.Cpad % 4 || p.C > p.Cpad || p.limit < 1 || p.nrow != (p.H + p.limit - 1) / p.limit || p.ncol != (p.W + p.limit - 1) / p.limit) return 1;
    const long long n = (long long)p.B * p.H * p.W * (p.Cpad / 4);
    hipLaunchKernelGGL(vae_tile_blend_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, p);
    CHECK_LAUNCH();
}
