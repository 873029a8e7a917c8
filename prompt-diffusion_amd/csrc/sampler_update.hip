// The end of a denoising step, elementwise over the B x HW x C latents (gfx950): classifier-free guidance, the solver's update
// (DDIM, fused UniPC or a linear multistep row), the optional inpainting blend, and the store of the new sample for the next step -- plus the start of
// an img2img / inpainting session (pd_sample_args.init_latents / mask, include/pdengine.h).  Each piece of arithmetic exists
// once: the index decomposition, the guidance and the stores in the one kernel template, the three solvers and the blend as
// __device__ functions it calls; the kernels are its instantiations over the solver, a compile-time "blend or not" and, for DDIM
// and the linear multistep rows, a compile-time "draws seeded noise or not" (pd_philox.h): the instantiations that draw none
// carry nothing of the generator.  The small fill kernel behind pd_randn evaluates the same address -> value map.
//   eps      [Bf, HW, eps_C] fp32 / 16-bit: UNet output, uncond half first (ddim_hacked.py:189-192); with perturbed-attention
//            guidance (UpdateState::pag_scale != 0) B more samples, the perturbed branch, from sample pag_off on
//   x_state  [B, HW, Cpad] fp32 (channels >= C are zero)    -> updated in place
//   x_in     [dup*B, HW, Cpad] fp32: the CFG-duplicated latents the next step's conv_in reads
//   pred_x0, eps_guided  [B, HW, C] fp32, index i
// z0 / eps / the noise draws of img2img and inpainting are NCHW fp32 (the caller's layout), the mask [B, HW].  With a blend,
// only x_state and x_in receive the blended value; pred_x0, the guided eps and the UniPC fp64 state (last, the x0 ring) are the
// update's own (so are the linear multistep solver's history ring and kept sample).
#include "../../include/pdengine.h"
#include "pd_common.h"
#include "pd_philox.h"

namespace {

constexpr int TPB = 256;
inline int nblocks(long long n, int per = TPB, int cap = 65535 * 16) {
    long long b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// The solvers: what differs between the kernels.  update() takes the sample x and the guided eps e of element i (NCHW index j =
// element el of sample b), stores pred_x0[i] and its own state, and returns the new sample.

// DDIMSampler.p_sample_ddim (cldm/ddim_hacked.py:218,229-233) in the reference's own fp32 operation order (no FMA contraction).
// do_update 0: the kernel stops after the guided eps (pd_sample_eps_at).  SEEDED: the draw of the step comes from the
// generator at (PD_RNG_STEP, draw) instead of the caller's noise[j]; the arithmetic around it is the same.
template <bool SEEDED> struct DdimSolver {
    DdimCoef k; const float* __restrict__ noise; float temperature; int do_update; PdRng rng; uint32_t draw;
    __device__ __forceinline__ bool active() const { return do_update != 0; }
    __device__ __forceinline__ float update(float x, float e, long long i, long long j, int b, long long el,
                                            float* __restrict__ pred_x0) const {
        if constexpr (SEEDED) {
            // The same draw from either source has to give the same bits, so this instantiation does not leave the choice of
            // FMAs to the compiler: contraction is off here and the operations are spelled as the caller-noise instantiation
            // below is compiled -- x - s e and the final xp + (sigma z) t fused, every other operation rounded on its own.
#pragma clang fp contract(off)
            const float z = pd_rng_normal(rng, PD_RNG_STEP, draw, (uint32_t)b, el);
            const float pred = __fdiv_rn(__builtin_fmaf(-k.sqrt_one_minus_at, e, x), k.sqrt_at);
            const float xp = k.sqrt_a_prev * pred + k.dir_coef * e;
            pred_x0[i] = pred;
            return __builtin_fmaf(k.sigma * z, temperature, xp);
        }
        const float pred = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.sqrt_one_minus_at, e)), k.sqrt_at);
        const float dir = __fmul_rn(k.dir_coef, e);
        float xp = __fadd_rn(__fmul_rn(k.sqrt_a_prev, pred), dir);
        if (noise) {
            const float nz = __fmul_rn(__fmul_rn(k.sigma, noise[j]), temperature);
            xp = __fadd_rn(xp, nz);
        }
        pred_x0[i] = pred;
        return xp;
    }
};

// One fused UniPC step (data prediction, UniP predictor + UniC corrector; coefficient layout in include/pdengine.h).  The solver
// state is fp64 like the host scheduler's (model_outputs / last_sample), and only the returned sample is rounded to fp32, where
// the scheduler rounds it.  The corrector and predictor sums are plain fp64 expressions that the compiler contracts into FMAs:
// their operand order and parentheses decide the last bit of the state, so they stay exactly as written.
//   last, m_out, h1..h3  [B, HW, C] fp64, index i; m_out may alias one of h1..h3 (each element is read before it is written);
//   last receives the corrected sample from before any blend (the scheduler's last_sample)
struct UnipcSolver {
    UnipcCoef k; double* __restrict__ last; double* m_out; const double* h1; const double* h2; const double* h3;
    __device__ __forceinline__ bool active() const { return true; }
    __device__ __forceinline__ float update(float xf, float e, long long i, long long, int, long long, float* __restrict__ pred_x0) const {
        const double x = (double)xf;
        // m_i = (x - sigma e) / alpha, in the scheduler's operation order
        const double m = __ddiv_rn(__dsub_rn(x, __dmul_rn(k.sigma, (double)e)), k.alpha);
        const double m1 = k.n_hist > 0 ? h1[i] : 0.0;
        const double m2 = k.n_hist > 1 ? h2[i] : 0.0;
        const double m3 = k.n_hist > 2 ? h3[i] : 0.0;
        double xc = x;
        if (k.corr) xc = k.c_last * last[i] + k.c_m[0] * m + k.c_m[1] * m1 + k.c_m[2] * m2 + k.c_m[3] * m3;
        const double xn = k.p_x * xc + k.p_m[0] * m + k.p_m[1] * m1 + k.p_m[2] * m2;
        last[i] = xc;
        m_out[i] = m;
        pred_x0[i] = (float)m;
        return (float)xn;
    }
};

// One row of a linear multistep solver (PLMS, DPM-Solver++ multistep, or rows the caller brought; layout PD_LMS_NCOEF in
// include/pdengine.h).  With the grid fixed, the new sample and the reported pred_x0 are linear in a base sample -- the current
// one or the kept one -- and the model outputs m_i .. m_{i-3}; m_i is the x0 prediction (data prediction) or the guided eps
// itself.  State is fp64 like UnipcSolver's and only the two results are rounded to fp32; the sums are plain fp64 expressions
// that the compiler contracts into FMAs, so their operand order and parentheses stay exactly as written.
//   keep, m_out, h1..h3  [B, HW, C] fp64, index i; m_out may alias one of h1..h3 (each element is read before it is written);
//   keep is read / written only by rows whose flags say so and may be null otherwise
// NOISE (rows with [14] != 0): x_next += c_z z, z the seeded normal at (PD_RNG_STEP, draw = row index), two separately rounded
// fp64 operations after the sum; pred_x0 takes none.
template <bool NOISE> struct LmsSolver {
    LmsCoef k; double* keep; double* m_out; const double* h1; const double* h2; const double* h3; PdRng rng; uint32_t draw;
    __device__ __forceinline__ bool active() const { return true; }
    __device__ __forceinline__ float update(float xf, float e, long long i, long long, int b, long long el,
                                            float* __restrict__ pred_x0) const {
        const double x = (double)xf;
        // m_i: (x - sigma e) / alpha in the operation order of UnipcSolver, or eps
        const double m = k.data_pred ? __ddiv_rn(__dsub_rn(x, __dmul_rn(k.sigma, (double)e)), k.alpha) : (double)e;
        const double m1 = k.n_hist > 0 ? h1[i] : 0.0;
        const double m2 = k.n_hist > 1 ? h2[i] : 0.0;
        const double m3 = k.n_hist > 2 ? h3[i] : 0.0;
        if (k.store_keep) keep[i] = x;
        const double base = k.base_keep ? keep[i] : x;
        double xn = k.c_x * base + k.c_m[0] * m + k.c_m[1] * m1 + k.c_m[2] * m2 + k.c_m[3] * m3;
        if constexpr (NOISE) xn = __dadd_rn(xn, __dmul_rn(k.c_z, (double)pd_rng_normal(rng, PD_RNG_STEP, draw, (uint32_t)b, el)));
        const double p0 = k.q_x * base + k.q_m[0] * m + k.q_m[1] * m1 + k.q_m[2] * m2 + k.q_m[3] * m3;
        if (k.push) m_out[i] = m;
        pred_x0[i] = (float)p0;
        return (float)xn;
    }
};

// inpainting: (1 - m) k + m x, k = last ? z0 : sa z0 + sb eps (at the next step's timestep), at NCHW index j and mask index bp.
// Every operation is a separately rounded fp32 operation (no FMA contraction), so a NumPy fp32 blend of the same sample gives
// the same bits.
__device__ __forceinline__ float blend(float x, const BlendArgs& bl, long long j, long long bp) {
    const float z = bl.z0[j];
    const float k = bl.coef.last ? z : __fadd_rn(__fmul_rn(bl.coef.sa, z), __fmul_rn(bl.coef.sb, bl.ieps[j]));
    const float m = bl.mask[bp];
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m), k), __fmul_rn(m, x));
}

// The one update kernel: guided eps (eps_uncond + scale (eps_cond - eps_uncond), ddim_hacked.py:193; + pag_scale (eps_cond -
// eps_perturbed) where the evaluation carried a perturbed branch) -> eps_guided, the solver's
// update, the blend where BLEND (compile-time: the plain instantiations carry nothing of it), and the new sample -> x_state, x_in
// and x_in's CFG half.
template <class Solver, bool BLEND>
__global__ void cfg_update_kernel(UpdateState u, Solver s, BlendArgs bl) {
    const auto& k = s.k;
    const long long total = (long long)u.B * u.HW * u.C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % u.C);
        const long long bp = i / u.C;
        const int p = (int)(bp % u.HW);
        const int b = (int)(bp / u.HW);
        auto ld = [&](long long q) {
            return u.eps_dt == DT_F32 ? reinterpret_cast<const float*>(u.eps)[q] : cvt32_rt(reinterpret_cast<const uint16_t*>(u.eps)[q], u.eps_dt);
        };
        float e, eu = 0.f, ec;
        if (u.use_cfg) {
            eu = ld(((long long)b * u.HW + p) * u.eps_C + c);
            ec = ld(((long long)(u.B + b) * u.HW + p) * u.eps_C + c);
            e = __fadd_rn(eu, __fmul_rn(k.cfg_scale, __fsub_rn(ec, eu)));
        } else {
            e = ec = ld(((long long)b * u.HW + p) * u.eps_C + c);
        }
        if (u.pag) {
            // An evaluation with perturbed-attention guidance: (e_u + s (e_c - e_u)) + p (e_c - e_p), every operation rounded on its own.
            // The lines above are compiled with the scale's multiply-add contracted into one FMA (hipcc takes __fmul_rn / __fadd_rn for
            // plain operators); that is the arithmetic of every evaluation without the state and stays as it is.  Here contraction is
            // off and the CFG sum is formed again, so a NumPy fp32 restatement gives the same bits -- also on the steps whose p is 0
            // (the clamp of the adaptive scale), where the third run of eps is not read.
#pragma clang fp contract(off)
            e = u.use_cfg ? eu + k.cfg_scale * (ec - eu) : ec;
            if (u.pag_scale != 0.f) {
                const float ep = ld(((long long)(u.pag_off + b) * u.HW + p) * u.eps_C + c);
                e = e + u.pag_scale * (ec - ep);
            }
        }
        u.eps_guided[i] = e;
        if (!s.active()) continue;
        const long long xi = ((long long)b * u.HW + p) * u.Cpad + c;   // NHWC index in x_state / x_in
        const long long j = ((long long)b * u.C + c) * u.HW + p;       // NCHW index in noise / z0 / the img2img eps
        float xp = s.update(u.x_state[xi], e, i, j, b, (long long)c * u.HW + p, u.pred_x0);
        if constexpr (BLEND) xp = blend(xp, bl, j, bp);
        u.x_state[xi] = xp;
        u.x_in[xi] = xp;
        if (u.use_cfg) u.x_in[(long long)u.B * u.HW * u.Cpad + xi] = xp;
    }
}

template <class Solver> int launch_update(const UpdateState& u, const Solver& sv, const BlendArgs* bl, hipStream_t s) {
    if (bl && !(bl->z0 && bl->ieps && bl->mask)) return 1;
    const dim3 grid(nblocks((long long)u.B * u.HW * u.C));
    if (bl) hipLaunchKernelGGL((cfg_update_kernel<Solver, true>), grid, dim3(TPB), 0, s, u, sv, *bl);
    else hipLaunchKernelGGL((cfg_update_kernel<Solver, false>), grid, dim3(TPB), 0, s, u, sv, BlendArgs{});
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// the start of an img2img / inpainting session: x = pure ? eps : sa z0 + sb eps, replacing nchw_to_nhwc + dup_rows of a plain one
//   x_state [B, HW, Cpad], x_in [dup * B, HW, Cpad], out_nchw [B, C, HW] (optional)
// SEEDED (PD_XT_FROM_SEED): eps is drawn at (PD_RNG_XT, draw 0) and, where the blend will read it again, stored to eps_out
// [B, C, HW]; with pure and no z0 this is also the start of a plain session whose x_T the engine draws.
template <bool SEEDED>
__global__ void init_latents_kernel(const float* __restrict__ z0, const float* __restrict__ eps, float sa, float sb, int pure,
                                    float* __restrict__ x_state, float* __restrict__ x_in, float* __restrict__ out_nchw, int B,
                                    int dup, int C, int Cpad, int HW, PdRng rng, float* __restrict__ eps_out) {
    const long long n = (long long)B * HW * Cpad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const long long bp = i / Cpad;
        const int p = (int)(bp % HW);
        const int b = (int)(bp / HW);
        float v = 0.f;
        if (c < C) {
            const long long j = ((long long)b * C + c) * HW + p;
            float ev;
            if constexpr (SEEDED) {
                ev = pd_rng_normal(rng, PD_RNG_XT, 0u, (uint32_t)b, (long long)c * HW + p);
                if (eps_out) eps_out[j] = ev;
            } else {
                ev = eps[j];
            }
            v = pure ? ev : __fadd_rn(__fmul_rn(sa, z0[j]), __fmul_rn(sb, ev));
            if (out_nchw) out_nchw[j] = v;
        }
        x_state[i] = v;
        for (int d = 0; d < dup; ++d) x_in[(long long)d * n + i] = v;
    }
}

// out [B][per_sample]: one thread per Philox block = four consecutive elements of a sample (the tail block writes fewer)
__global__ void randn_kernel(PdRng rng, uint32_t stream, uint32_t draw, int B, long long per_sample, float* __restrict__ out) {
    const long long nq = (per_sample + 3) / 4, total = (long long)B * nq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long q = i % nq;
        const int b = (int)(i / nq);
        uint32_t r[4];
        pd_philox4x32_10_block((uint32_t)q, rng.state[2] + (uint32_t)b, draw, stream, rng.state[0], rng.state[1], r);
        float* o = out + (long long)b * per_sample + 4 * q;
        const int n = (int)(per_sample - 4 * q < 4 ? per_sample - 4 * q : 4);
        for (int l = 0; l < n; ++l) o[l] = pd_philox_normal_lane(r, l);
    }
}

}  // namespace

int launch_randn(const uint32_t* rng_state, uint32_t stream, uint32_t draw, int B, long long per_sample, float* out, hipStream_t s) {
    if (!rng_state || !out || B < 1 || per_sample < 1) return 1;
    hipLaunchKernelGGL(randn_kernel, dim3(nblocks((long long)B * ((per_sample + 3) / 4))), dim3(TPB), 0, s, PdRng{rng_state}, stream, draw,
                       B, per_sample, out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_init_latents(const float* z0, const float* eps, float sa, float sb, int pure, float* x_state, float* x_in, float* out_nchw,
                        int B, int dup, int C, int Cpad, int HW, hipStream_t s, const uint32_t* rng_state, float* eps_out) {
    if ((!eps && !rng_state) || (!pure && !z0) || C > Cpad || dup < 1) return 1;
    const long long n = (long long)B * HW * Cpad;
    if (rng_state)
        hipLaunchKernelGGL(init_latents_kernel<true>, dim3(nblocks(n)), dim3(TPB), 0, s, z0, eps, sa, sb, pure, x_state, x_in, out_nchw,
                           B, dup, C, Cpad, HW, PdRng{rng_state}, eps_out);
    else
        hipLaunchKernelGGL(init_latents_kernel<false>, dim3(nblocks(n)), dim3(TPB), 0, s, z0, eps, sa, sb, pure, x_state, x_in, out_nchw,
                           B, dup, C, Cpad, HW, PdRng{nullptr}, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_cfg_ddim(const UpdateState& u, const DdimCoef& k, const float* noise, float temperature, int do_update, const BlendArgs* bl,
                    hipStream_t s, const uint32_t* rng_state, uint32_t draw) {
    if (rng_state) {
        if (noise) return 1;
        return launch_update(u, DdimSolver<true>{k, nullptr, temperature, do_update, PdRng{rng_state}, draw}, bl, s);
    }
    return launch_update(u, DdimSolver<false>{k, noise, temperature, do_update, PdRng{nullptr}, 0u}, bl, s);
}

int launch_cfg_unipc(const UpdateState& u, const UnipcCoef& k, double* last, double* m_out, const double* const hist[3],
                     const BlendArgs* bl, hipStream_t s) {
    if (k.n_hist < 0 || k.n_hist > 3 || !last || !m_out) return 1;
    for (int j = 0; j < k.n_hist; ++j)
        if (!hist[j]) return 1;
    return launch_update(u, UnipcSolver{k, last, m_out, hist[0], hist[1], hist[2]}, bl, s);
}

int launch_cfg_lms(const UpdateState& u, const LmsCoef& k, double* keep, double* m_out, const double* const hist[3], const BlendArgs* bl,
                   hipStream_t s, const uint32_t* rng_state, uint32_t draw) {
    if (k.n_hist < 0 || k.n_hist > 3 || (k.push && !m_out) || ((k.store_keep || k.base_keep) && !keep)) return 1;
    for (int j = 0; j < k.n_hist; ++j)
        if (!hist[j]) return 1;
    if (k.c_z != 0.0) {
        if (!rng_state) return 1;
        return launch_update(u, LmsSolver<true>{k, keep, m_out, hist[0], hist[1], hist[2], PdRng{rng_state}, draw}, bl, s);
    }
    return launch_update(u, LmsSolver<false>{k, keep, m_out, hist[0], hist[1], hist[2], PdRng{nullptr}, 0u}, bl, s);
}
