// img2img / inpainting inside the sampling loop (pd_sample_args.init_latents / mask, include/pdengine.h), gfx950.
// Elementwise over the B x C x HW latents, like the update kernels they extend:
//   init_latents_kernel  the start: x = sa z0 + sb eps (or eps itself), replacing nchw_to_nhwc + dup_rows of a plain session
//   cfg_ddim_blend_kernel / cfg_unipc_blend_kernel  cfg_ddim_kernel / cfg_unipc_kernel (elementwise.hip) with the known region put
//     back after the update: x <- (1 - m) k + m x, k = sa z0 + sb eps at the next step's timestep, or z0 after the last step.
// The update arithmetic is copied from elementwise.hip, not shared, so that the plain loop's kernels stay exactly as they are.
// Only x_state and x_in receive the blended value; pred_x0, the guided eps and the UniPC fp64 state (last, the x0 ring) are
// the update's own.  z0 / eps / the noise draws are NCHW fp32 (the caller's layout), the mask [B, HW].  Every blend operation
// is a separately rounded fp32 operation (no FMA contraction), so a NumPy fp32 blend of the same sample gives the same bits.
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

// (1 - m) k + m x, k = last ? z0 : sa z0 + sb eps, at NCHW index j and mask index bp
__device__ __forceinline__ float blend(float x, const float* __restrict__ z0, const float* __restrict__ ieps,
                                       const float* __restrict__ mask, long long j, long long bp, BlendCoef bc) {
    const float z = z0[j];
    const float k = bc.last ? z : __fadd_rn(__fmul_rn(bc.sa, z), __fmul_rn(bc.sb, ieps[j]));
    const float m = mask[bp];
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m), k), __fmul_rn(m, x));
}

__device__ __forceinline__ void store_x(float* __restrict__ x_state, float* __restrict__ x_in, long long xi, long long half,
                                        int use_cfg, float v) {
    x_state[xi] = v;
    x_in[xi] = v;
    if (use_cfg) x_in[half + xi] = v;
}

//   x_state [B, HW, Cpad], x_in [dup * B, HW, Cpad], out_nchw [B, C, HW] (optional)
__global__ void init_latents_kernel(const float* __restrict__ z0, const float* __restrict__ eps, float sa, float sb, int pure,
                                    float* __restrict__ x_state, float* __restrict__ x_in, float* __restrict__ out_nchw, int B,
                                    int dup, int C, int Cpad, int HW) {
    const long long n = (long long)B * HW * Cpad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const long long bp = i / Cpad;
        const int p = (int)(bp % HW);
        const int b = (int)(bp / HW);
        float v = 0.f;
        if (c < C) {
            const long long j = ((long long)b * C + c) * HW + p;
            v = pure ? eps[j] : __fadd_rn(__fmul_rn(sa, z0[j]), __fmul_rn(sb, eps[j]));
            if (out_nchw) out_nchw[j] = v;
        }
        x_state[i] = v;
        for (int d = 0; d < dup; ++d) x_in[(long long)d * n + i] = v;
    }
}

__global__ void cfg_ddim_blend_kernel(const void* __restrict__ eps, int eps_dt, int eps_C, float* __restrict__ x_state,
                                      float* __restrict__ pred_x0, float* __restrict__ eps_guided, float* __restrict__ x_in,
                                      const float* __restrict__ noise, int B, int HW, int C, int Cpad, int use_cfg, DdimCoef k,
                                      float temperature, const float* __restrict__ z0, const float* __restrict__ ieps,
                                      const float* __restrict__ mask, BlendCoef bc) {
    const long long total = (long long)B * HW * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long bp = i / C;
        const int p = (int)(bp % HW);
        const int b = (int)(bp / HW);
        auto ld = [&](long long j) {
            return eps_dt == DT_F32 ? reinterpret_cast<const float*>(eps)[j] : cvt32_rt(reinterpret_cast<const uint16_t*>(eps)[j], eps_dt);
        };
        float e;
        if (use_cfg) {
            const float eu = ld(((long long)b * HW + p) * eps_C + c);
            const float ec = ld(((long long)(B + b) * HW + p) * eps_C + c);
            e = __fadd_rn(eu, __fmul_rn(k.cfg_scale, __fsub_rn(ec, eu)));
        } else {
            e = ld(((long long)b * HW + p) * eps_C + c);
        }
        eps_guided[i] = e;
        const long long xi = ((long long)b * HW + p) * Cpad + c;
        const long long j = ((long long)b * C + c) * HW + p;
        const float x = x_state[xi];
        const float pred = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.sqrt_one_minus_at, e)), k.sqrt_at);
        const float dir = __fmul_rn(k.dir_coef, e);
        float xp = __fadd_rn(__fmul_rn(k.sqrt_a_prev, pred), dir);
        if (noise) {
            const float nz = __fmul_rn(__fmul_rn(k.sigma, noise[j]), temperature);
            xp = __fadd_rn(xp, nz);
        }
        pred_x0[i] = pred;
        store_x(x_state, x_in, xi, (long long)B * HW * Cpad, use_cfg, blend(xp, z0, ieps, mask, j, bp, bc));
    }
}

__global__ void cfg_unipc_blend_kernel(const void* __restrict__ eps, int eps_dt, int eps_C, float* __restrict__ x_state,
                                       float* __restrict__ pred_x0, float* __restrict__ eps_guided, float* __restrict__ x_in, int B,
                                       int HW, int C, int Cpad, int use_cfg, UnipcCoef k, double* __restrict__ last, double* m_out,
                                       const double* h1, const double* h2, const double* h3, const float* __restrict__ z0,
                                       const float* __restrict__ ieps, const float* __restrict__ mask, BlendCoef bc) {
    const long long total = (long long)B * HW * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long bp = i / C;
        const int p = (int)(bp % HW);
        const int b = (int)(bp / HW);
        auto ld = [&](long long j) {
            return eps_dt == DT_F32 ? reinterpret_cast<const float*>(eps)[j] : cvt32_rt(reinterpret_cast<const uint16_t*>(eps)[j], eps_dt);
        };
        float e;
        if (use_cfg) {
            const float eu = ld(((long long)b * HW + p) * eps_C + c);
            const float ec = ld(((long long)(B + b) * HW + p) * eps_C + c);
            e = __fadd_rn(eu, __fmul_rn(k.cfg_scale, __fsub_rn(ec, eu)));
        } else {
            e = ld(((long long)b * HW + p) * eps_C + c);
        }
        eps_guided[i] = e;
        const long long xi = ((long long)b * HW + p) * Cpad + c;
        const double x = (double)x_state[xi];
        const double m = __ddiv_rn(__dsub_rn(x, __dmul_rn(k.sigma, (double)e)), k.alpha);
        const double m1 = k.n_hist > 0 ? h1[i] : 0.0;
        const double m2 = k.n_hist > 1 ? h2[i] : 0.0;
        const double m3 = k.n_hist > 2 ? h3[i] : 0.0;
        double xc = x;
        if (k.corr) xc = k.c_last * last[i] + k.c_m[0] * m + k.c_m[1] * m1 + k.c_m[2] * m2 + k.c_m[3] * m3;
        const double xn = k.p_x * xc + k.p_m[0] * m + k.p_m[1] * m1 + k.p_m[2] * m2;
        last[i] = xc;   // the corrected sample from before the blend (the scheduler's last_sample)
        m_out[i] = m;
        pred_x0[i] = (float)m;
        const long long j = ((long long)b * C + c) * HW + p;
        store_x(x_state, x_in, xi, (long long)B * HW * Cpad, use_cfg, blend((float)xn, z0, ieps, mask, j, bp, bc));
    }
}

}  // namespace

#define CHECK_LAUNCH() return hipGetLastError() == hipSuccess ? 0 : 1

int launch_init_latents(const float* z0, const float* eps, float sa, float sb, int pure, float* x_state, float* x_in, float* out_nchw,
                        int B, int dup, int C, int Cpad, int HW, hipStream_t s) {
    if (!eps || (!pure && !z0) || C > Cpad || dup < 1) return 1;
    const long long n = (long long)B * HW * Cpad;
    hipLaunchKernelGGL(init_latents_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, z0, eps, sa, sb, pure, x_state, x_in, out_nchw, B, dup,
                       C, Cpad, HW);
    CHECK_LAUNCH();
}

int launch_cfg_ddim_blend(const void* eps, int eps_dt, int eps_C, float* x_state, float* pred_x0, float* eps_guided, void* x_in,
                          const float* noise, int B, int HW, int C, int Cpad, int use_cfg, DdimCoef k, float temperature,
                          const float* z0, const float* ieps, const float* mask, BlendCoef bc, hipStream_t s) {
    if (!z0 || !ieps || !mask) return 1;
    const long long n = (long long)B * HW * C;
    hipLaunchKernelGGL(cfg_ddim_blend_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, eps, eps_dt, eps_C, x_state, pred_x0, eps_guided,
                       reinterpret_cast<float*>(x_in), noise, B, HW, C, Cpad, use_cfg, k, temperature, z0, ieps, mask, bc);
    CHECK_LAUNCH();
}

int launch_cfg_unipc_blend(const void* eps, int eps_dt, int eps_C, float* x_state, float* pred_x0, float* eps_guided, void* x_in,
                           int B, int HW, int C, int Cpad, int use_cfg, const UnipcCoef& k, double* last, double* m_out,
                           const double* const hist[3], const float* z0, const float* ieps, const float* mask, BlendCoef bc,
                           hipStream_t s) {
    if (k.n_hist < 0 || k.n_hist > 3 || !last || !m_out || !z0 || !ieps || !mask) return 1;
    for (int j = 0; j < k.n_hist; ++j)
        if (!hist[j]) return 1;
    const long long n = (long long)B * HW * C;
    hipLaunchKernelGGL(cfg_unipc_blend_kernel, dim3(nblocks(n)), dim3(TPB), 0, s, eps, eps_dt, eps_C, x_state, pred_x0, eps_guided,
                       reinterpret_cast<float*>(x_in), B, HW, C, Cpad, use_cfg, k, last, m_out, hist[0], hist[1], hist[2], z0, ieps,
                       mask, bc);
    CHECK_LAUNCH();
}
