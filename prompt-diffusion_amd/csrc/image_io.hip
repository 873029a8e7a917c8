// pdengine: the image ends of a call (host side in image_host.cpp; contract in include/pdengine.h, "Image ends").  Integer or
// single-rounding fp32 arithmetic throughout, so every kernel is bit-identical to the Pillow / NumPy code it replaces.  All are
// HBM-bound; a thread owns four neighbouring pixels of a row:
//   image_hpass_kernel  u8 NHWC [N][Hs][Ws][3] -> u8 NHWC [N][Hs][W][3]: Pillow's horizontal 8-bit resampling pass
//   image_vpass_kernel  u8 NHWC [N][Hs][W][3]  -> fp32 planar channels c_off .. c_off + 2 of [B][C][H][W]: the vertical pass (or none:
//                       the pack-only instantiation), u8 / 255, * mul + add, and the batch duplication, from one read of the source
//   image_store_kernel  fp32 NCHW [B][C][H][W] -> u8 NHWC [B][H][W][C]: clip(x * mul + add, 0, 1) * 255, rounded
#include "pd_common.h"

namespace {

constexpr int TPB = 256;
constexpr int PX = 4;             // pixels per thread
constexpr int kPrecBits = 22;     // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecBits;   // arithmetic shift, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// 3 * n bytes (n <= PX pixels) starting at p; `vec`: p is 4-byte aligned and n == PX -> three dword loads
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ p, bool vec, int n, int v[3 * PX]) {
    if (vec) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t u = q[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * i + j] = (int)((u >> (8 * j)) & 0xffu);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i) v[i] = i < 3 * n ? (int)p[i] : 0;
    }
}

__device__ __forceinline__ void store_px(uint8_t* __restrict__ p, bool vec, int n, const int v[3 * PX]) {
    if (vec) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            q[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) | ((uint32_t)v[4 * i + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i)
            if (i < 3 * n) p[i] = (uint8_t)v[i];
    }
}

// out[r][x][c] = clip8(2^21 + sum_j src[r][xmin(x) + j][c] * kk[x][j]), r over the N * Hs source rows.  bounds [W][2] = (xmin, count),
// kk [W][ksize]; xmin + count <= Ws by construction (pd_resample_coefficients).  `vec`: W % 4 == 0 and `out` 4-byte aligned.
__global__ __launch_bounds__(TPB) void image_hpass_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           long long rows, int Ws, int W, int vec) {
    const int gw = (W + PX - 1) / PX;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= rows * gw) return;
    const int x0 = (int)(i % gw) * PX;
    const long long r = i / gw;
    const int n = min(PX, W - x0);
    const uint8_t* row = src + r * (long long)Ws * 3;
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
    store_px(out + (r * W + x0) * 3, vec && n == PX, n, v);
}

// One thread: pixels x0 .. x0 + 3 of row y of source image bs.  RESIZE: the vertical pass over tmp [Bs][Hs][W][3] with bounds [H][2],
// kk [H][ksize]; otherwise Hs == H and the row is read as it is.  The float values go to every destination sample that reads this
// source: rep = B / Bs of them, b = bs * rep + d (tile == 0, np.repeat) or b = bs + d * Bs (tile == 1, whole-batch repeats).
// vec_in: W % 4 == 0 and the source 4-byte aligned; vec_out: W % 4 == 0 and dst 16-byte aligned.
template <bool RESIZE>
__global__ __launch_bounds__(TPB) void image_vpass_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int Bs,
                                                           int Hs, int H, int W, int C, int c_off, int rep, int tile, float mul, float add,
                                                           int vec_in, int vec_out) {
    const int gw = (W + PX - 1) / PX;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)Bs * H * gw) return;
    const int x0 = (int)(i % gw) * PX;
    const int y = (int)((i / gw) % H);
    const int bs = (int)(i / ((long long)gw * H));
    const int n = min(PX, W - x0);
    const bool vin = vec_in && n == PX;
    int u[3 * PX];
    if (RESIZE) {
        const int ymin = bounds[2 * y], cnt = bounds[2 * y + 1];
        const int* k = kk + (long long)y * ksize;
        int s[3 * PX];
#pragma unroll
        for (int e = 0; e < 3 * PX; ++e) s[e] = 1 << (kPrecBits - 1);
        const uint8_t* q = src + (((long long)bs * Hs + ymin) * W + x0) * 3;
        for (int j = 0; j < cnt; ++j, q += (long long)W * 3) {
            const int w = k[j];
            int v[3 * PX];
            load_px(q, vin, n, v);
#pragma unroll
            for (int e = 0; e < 3 * PX; ++e) s[e] += v[e] * w;
        }
#pragma unroll
        for (int e = 0; e < 3 * PX; ++e) u[e] = clip8(s[e]);
    } else {
        load_px(src + (((long long)bs * H + y) * W + x0) * 3, vin, n, u);
    }
    float f[3][PX];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c][p] = mul_add_rn(__fdiv_rn((float)u[3 * p + c], 255.0f), mul, add);
    const long long HW = (long long)H * W;
    for (int d = 0; d < rep; ++d) {
        const long long b = tile ? (long long)bs + (long long)d * Bs : (long long)bs * rep + d;
        float* o = dst + (b * C + c_off) * HW + (long long)y * W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c, o += HW) {
            if (vec_out && n == PX) {
                *reinterpret_cast<f32x4*>(o) = f32x4{f[c][0], f[c][1], f[c][2], f[c][3]};
            } else {
#pragma unroll
                for (int p = 0; p < PX; ++p)
                    if (p < n) o[p] = f[c][p];
            }
        }
    }
}

// One thread: PX neighbouring pixels (in the flattened H * W of one sample) of all C <= 3 channels.  `vec`: HW % 4 == 0, src 16-byte
// and dst 4-byte aligned (C = 3 stores three dwords, C = 1 one).
template <int C>
__global__ __launch_bounds__(TPB) void image_store_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int B, long long HW,
                                                           float mul, float add, int trunc, int vec) {
    const long long gp = (HW + PX - 1) / PX;
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)B * gp) return;
    const long long p0 = (i % gp) * PX;
    const long long b = i / gp;
    const int n = (int)(HW - p0 < PX ? HW - p0 : PX);
    const bool v4 = vec && n == PX;
    int u[3 * PX];
#pragma unroll
    for (int e = 0; e < 3 * PX; ++e) u[e] = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* s = src + (b * C + c) * HW + p0;
        float x[PX];
        if (v4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(s);
            x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p) x[p] = p < n ? s[p] : 0.f;
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            float t = mul_add_rn(x[p], mul, add);
            t = fminf(fmaxf(t, 0.f), 1.f) * 255.0f;
            u[C * p + c] = (int)(trunc ? t : rintf(t));   // t in [0, 255]; rintf rounds half to even
        }
    }
    uint8_t* o = dst + (b * HW + p0) * C;
    if (v4 && C == 3) {
        store_px(o, true, PX, u);
    } else if (v4 && C == 1) {
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16) | ((uint32_t)u[3] << 24);
    } else {
#pragma unroll
        for (int e = 0; e < C * PX; ++e)
            if (e < C * n) o[e] = (uint8_t)u[e];
    }
}

inline bool grid_for(long long threads, dim3& grid) {
    const long long blocks = (threads + TPB - 1) / TPB;
    if (threads < 1 || blocks > 0x7fffffffll) return false;
    grid = dim3((unsigned)blocks);
    return true;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int launch_image_hpass(const uint8_t* src, uint8_t* out, const int* bounds, const int* kk, int ksize, long long rows, int Ws, int W,
                       hipStream_t s) {
    dim3 grid;
    if (rows < 1 || Ws < 1 || W < 1 || ksize < 1 || !grid_for(rows * ((W + PX - 1) / PX), grid)) return 1;
    const int vec = W % PX == 0 && aligned(out, 4);
    hipLaunchKernelGGL(image_hpass_kernel, grid, dim3(TPB), 0, s, src, out, bounds, kk, ksize, rows, Ws, W, vec);
    return hipGetLastError() != hipSuccess;
}

int launch_image_vpass(const uint8_t* src, float* dst, const int* bounds, const int* kk, int ksize, int Bs, int Hs, int H, int W, int B,
                       int C, int c_off, int tile, float mul, float add, hipStream_t s) {
    dim3 grid;
    if (Bs < 1 || B < Bs || B % Bs || Hs < 1 || H < 1 || W < 1 || c_off < 0 || c_off + 3 > C) return 1;
    const bool resize = bounds != nullptr;
    if (!resize && Hs != H) return 1;
    if (!grid_for((long long)Bs * H * ((W + PX - 1) / PX), grid)) return 1;
    const int vec_in = W % PX == 0 && aligned(src, 4), vec_out = W % PX == 0 && aligned(dst, 16);
    if (resize)
        hipLaunchKernelGGL(image_vpass_kernel<true>, grid, dim3(TPB), 0, s, src, dst, bounds, kk, ksize, Bs, Hs, H, W, C, c_off, B / Bs, tile,
                           mul, add, vec_in, vec_out);
    else
        hipLaunchKernelGGL(image_vpass_kernel<false>, grid, dim3(TPB), 0, s, src, dst, bounds, kk, ksize, Bs, Hs, H, W, C, c_off, B / Bs, tile,
                           mul, add, vec_in, vec_out);
    return hipGetLastError() != hipSuccess;
}

int launch_image_store(const float* src, uint8_t* dst, int B, int C, int H, int W, float mul, float add, int trunc, hipStream_t s) {
    dim3 grid;
    if (B < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) return 1;
    const long long HW = (long long)H * W;
    if (!grid_for((long long)B * ((HW + PX - 1) / PX), grid)) return 1;
    const int vec = HW % PX == 0 && aligned(src, 16) && aligned(dst, 4);
    if (C == 3) hipLaunchKernelGGL(image_store_kernel<3>, grid, dim3(TPB), 0, s, src, dst, B, HW, mul, add, trunc, vec);
    else hipLaunchKernelGGL(image_store_kernel<1>, grid, dim3(TPB), 0, s, src, dst, B, HW, mul, add, trunc, vec);
    return hipGetLastError() != hipSuccess;
}
