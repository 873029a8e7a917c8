// pdengine: coefficient rows of the fused UniPC loop (host, fp64).
// Restates UniPCMultistepScheduler._coeffs / _uni_p / _uni_c / step (prompt-diffusion_amd/schedulers.py): UniPC, Zhao et al.
// 2023, data-prediction form, B(h) = expm1(h) ("bh2") or h ("bh1").  With the grid fixed, the predictor and the corrector of
// every step are linear combinations of the latents, the last corrected sample and the x0 predictions m_j with weights known
// in advance; this file expands the scheduler's D1 / rho form into those weights (layout: PD_UNIPC_NCOEF in pdengine.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "engine.h"

namespace {

// np.linalg.solve for the 2x2 / 3x3 systems of the order-3 predictor and the order-2/3 corrector (partial pivoting)
bool solve_small(int n, double A[3][3], double* b, double* x) {
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
        if (A[p][c] == 0.0) return false;
        if (p != c) {
            for (int k = 0; k < n; ++k) std::swap(A[p][k], A[c][k]);
            std::swap(b[p], b[c]);
        }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < n; ++k) A[r][k] -= f * A[c][k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < n; ++k) s -= A[r][k] * x[k];
        x[r] = s / A[r][r];
    }
    return true;
}

struct Coeffs {   // schedulers.py _coeffs
    double h_phi_1, B_h, alpha1, sig_ratio;
    double rks[3];
    double R[3][3], b[3];
};

struct Grid {
    std::vector<double> alpha, sigma, lambda;   // n + 1 points, the last one sigma = 0 (lambda = +inf)
    bool bh2 = true;

    Coeffs coeffs(int i0, int order, const int* hidx) const {
        Coeffs c{};
        const double lam0 = lambda[i0], lam1 = lambda[i0 + 1];
        const double h = lam1 - lam0;
        for (int k = 0; k < order - 1; ++k) c.rks[k] = (lambda[hidx[k]] - lam0) / h;
        c.rks[order - 1] = 1.0;
        const double hh = -h;
        const bool fin = std::isfinite(hh);
        c.h_phi_1 = fin ? std::expm1(hh) : -1.0;
        double h_phi_k = fin ? c.h_phi_1 / hh - 1.0 : -1.0;
        c.B_h = bh2 ? c.h_phi_1 : hh;
        double fact = 1.0;
        for (int i = 1; i <= order; ++i) {
            for (int k = 0; k < order; ++k) c.R[i - 1][k] = std::pow(c.rks[k], (double)(i - 1));
            c.b[i - 1] = h_phi_k * fact / c.B_h;
            fact *= i + 1;
            h_phi_k = fin ? h_phi_k / hh - 1.0 / fact : -1.0 / fact;
        }
        c.alpha1 = alpha[i0 + 1];
        c.sig_ratio = sigma[i0 + 1] / sigma[i0];
        return c;
    }
};

}  // namespace

// alphas_cumprod of make_schedule in fp64 (make_schedule keeps the float32 rounding of register_schedule for DDIM)
static void alphas_cumprod_f64(const pd_config& cfg, std::vector<double>& ac) {
    const int T_ = cfg.timesteps;
    const double s0 = std::sqrt(cfg.linear_start), s1 = std::sqrt(cfg.linear_end);
    const double st = T_ > 1 ? (s1 - s0) / (double)(T_ - 1) : 0.0;
    ac.resize(T_);
    double cp = 1.0;
    for (int i = 0; i < T_; ++i) {
        const double b = i == T_ - 1 ? s1 : s0 + st * (double)i;
        cp *= 1.0 - b * b;
        ac[i] = cp;
    }
}

int pd_unipc_table(const pd_config& cfg, const pd_unipc_args& u, const int64_t* ts, int n, std::vector<double>& coef) {
    if (u.order < 1 || u.order > 3) { pd_set_error("unipc: order must be 1, 2 or 3 (got %d)", u.order); return 1; }
    if (!ts) { pd_set_error("unipc: the timestep grid (pd_sample_args.timesteps) is required"); return 1; }
    if (n < 1 || n > cfg.timesteps) { pd_set_error("unipc: steps must be in [1, %d]", cfg.timesteps); return 1; }
    if (u.n_disable_corrector < 0 || (u.n_disable_corrector > 0 && !u.disable_corrector)) {
        pd_set_error("unipc: bad disable_corrector list");
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        if (ts[i] < 0 || ts[i] >= cfg.timesteps) { pd_set_error("unipc: timestep %lld outside [0, %d)", (long long)ts[i], cfg.timesteps); return 1; }
        if (i > 0 && ts[i] >= ts[i - 1]) {
            pd_set_error("unipc: the timestep grid must be strictly descending (a repeated point gives h = 0)");
            return 1;
        }
    }
    std::vector<double> ac;
    alphas_cumprod_f64(cfg, ac);
    Grid g;
    g.bh2 = u.bh2 != 0;
    g.alpha.resize(n + 1); g.sigma.resize(n + 1); g.lambda.resize(n + 1);
    for (int i = 0; i < n; ++i) {
        g.alpha[i] = std::sqrt(ac[ts[i]]);
        g.sigma[i] = std::sqrt(1.0 - ac[ts[i]]);
    }
    g.alpha[n] = 1.0;
    g.sigma[n] = 0.0;
    for (int i = 0; i <= n; ++i) g.lambda[i] = std::log(g.alpha[i]) - std::log(g.sigma[i]);   // +inf at the last point
    auto disabled = [&](int j) {
        for (int k = 0; k < u.n_disable_corrector; ++k)
            if (u.disable_corrector[k] == j) return true;
        return false;
    };
    coef.assign((size_t)n * PD_UNIPC_NCOEF, 0.0);
    int lower_order_nums = 0, this_order = 1;
    for (int i = 0; i < n; ++i) {
        double* r = &coef[(size_t)i * PD_UNIPC_NCOEF];
        r[0] = g.alpha[i];
        r[1] = g.sigma[i];
        // ---- corrector (_uni_c) for the step i-1 -> i the previous predictor took, of that predictor's order
        if (i > 0 && !disabled(i - 1)) {
            const int q = this_order;
            int hidx[2] = {i - 2, i - 3};
            const Coeffs c = g.coeffs(i - 1, q, hidx);
            double rhos[3] = {0.5, 0.0, 0.0};
            if (q > 1) {
                double A[3][3], b[3];
                std::memcpy(A, c.R, sizeof(A));
                std::memcpy(b, c.b, sizeof(b));
                if (!solve_small(q, A, b, rhos)) { pd_set_error("unipc: singular corrector system at step %d", i); return 1; }
            }
            // x_c = sig_ratio last - a1 phi1 m_{i-1} - a1 B_h (sum_k rho_k (m_{i-1-k} - m_{i-1}) / r_k + rho_q (m_i - m_{i-1}))
            const double ab = c.alpha1 * c.B_h;
            const double rl = rhos[q - 1];
            r[2] = 1.0;
            r[3] = c.sig_ratio;
            r[4] = -ab * rl;
            double w_prev = -c.alpha1 * c.h_phi_1 + ab * rl;
            for (int k = 0; k < q - 1; ++k) {
                const double w = ab * rhos[k] / c.rks[k];
                r[6 + k] = -w;
                w_prev += w;
            }
            r[5] = w_prev;
            r[13] = q;
        }
        // ---- order of this step's predictor (step(): warm-up, lower_order_final, first order onto sigma = 0)
        const int order = u.lower_order_final ? std::min(u.order, n - i) : u.order;
        this_order = std::min(order, lower_order_nums + 1);
        if (!std::isfinite(g.lambda[i + 1])) this_order = 1;
        // ---- predictor (_uni_p): x_{i+1} = sig_ratio x_c - a1 phi1 m_i - a1 B_h sum_k rho_k (m_{i-k} - m_i) / r_k
        {
            const int p = this_order;
            int hidx[2] = {i - 1, i - 2};
            const Coeffs c = g.coeffs(i, p, hidx);
            double rhos[2] = {0.5, 0.0};
            if (p == 3) {
                double A[3][3], b[3];
                std::memcpy(A, c.R, sizeof(A));
                std::memcpy(b, c.b, sizeof(b));
                if (!solve_small(2, A, b, rhos)) { pd_set_error("unipc: singular predictor system at step %d", i); return 1; }
            }
            r[8] = c.sig_ratio;
            double w0 = -c.alpha1 * c.h_phi_1;
            if (p > 1) {
                const double ab = c.alpha1 * c.B_h;
                for (int k = 0; k < p - 1; ++k) {
                    const double w = ab * rhos[k] / c.rks[k];
                    r[10 + k] = -w;
                    w0 += w;
                }
            }
            r[9] = w0;
            r[12] = p;
        }
        if (lower_order_nums < u.order) ++lower_order_nums;
    }
    return 0;
}

extern "C" int pd_unipc_coefficients(const pd_config* cfg, const pd_unipc_args* u, const int64_t* timesteps, int32_t steps,
                                     double* coef) {
    if (!cfg || !u || !coef) { pd_set_error("null argument"); return 1; }
    std::vector<double> tab;
    PD_TRY(pd_unipc_table(*cfg, *u, timesteps, steps, tab));
    std::memcpy(coef, tab.data(), tab.size() * sizeof(double));
    return 0;
}
