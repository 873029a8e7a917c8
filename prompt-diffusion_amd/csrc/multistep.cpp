// pdengine: coefficient rows of the fused UniPC loop and of the linear multistep solvers (host, fp64).
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

// ------------------------------------------------------------------------------------ linear multistep rows
// PLMS restates PLMSSampler.p_sample_plms / plms_sampling (ldm/models/diffusion/plms.py:146-244), DPM-Solver++ restates
// DPM_Solver.sample(method="multistep") with multistep_dpm_solver_{second,third}_update and dpm_solver_first_update
// (ldm/models/diffusion/dpm_solver/dpm_solver.py:469-501, 723-825, 1044-1074), each expanded into the weights of the sample
// and the model outputs (layout: PD_LMS_NCOEF in pdengine.h).
namespace {

// get_x_prev_and_pred_x0 (plms.py:205-224) with eta = 0: x_prev = sqrt(a_prev) (x - sqrt(1 - a_t) e) / sqrt(a_t) + sqrt(1 - a_prev) e
struct DdimForm { double x, e, px, pe; };
DdimForm ddim_form(double a_t, double a_prev) {
    DdimForm f;
    f.px = 1.0 / std::sqrt(a_t);
    f.pe = -std::sqrt(1.0 - a_t) / std::sqrt(a_t);
    f.x = std::sqrt(a_prev) * f.px;
    f.e = std::sqrt(a_prev) * f.pe + std::sqrt(1.0 - a_prev);
    return f;
}

int check_desc_grid(const pd_config& cfg, const int64_t* ts, int n, const char* who) {
    if (!ts) { pd_set_error("%s: the timestep grid (pd_sample_args.timesteps) is required", who); return 1; }
    for (int i = 0; i < n; ++i) {
        if (ts[i] < 0 || ts[i] >= cfg.timesteps) { pd_set_error("%s: timestep %lld outside [0, %d)", who, (long long)ts[i], cfg.timesteps); return 1; }
        if (i > 0 && ts[i] >= ts[i - 1]) { pd_set_error("%s: the timestep grid must be strictly descending", who); return 1; }
    }
    return 0;
}

int plms_rows(const pd_config& cfg, const int64_t* ts, int n, std::vector<double>& rows, std::vector<double>& times) {
    PD_TRY(check_desc_grid(cfg, ts, n, "plms"));
    std::vector<double> ac;
    alphas_cumprod_f64(cfg, ac);
    static const double AB[4][4] = {{1.0, 0.0, 0.0, 0.0},
                                    {3.0 / 2.0, -1.0 / 2.0, 0.0, 0.0},
                                    {23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0, 0.0},
                                    {55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0}};
    rows.assign((size_t)(n + 1) * PD_LMS_NCOEF, 0.0);
    times.assign(n + 1, 0.0);
    auto a_prev = [&](int i) { return i + 1 < n ? ac[ts[i + 1]] : ac[0]; };
    auto head = [&](double* r, int64_t t, int flags) {
        r[0] = std::sqrt(ac[t]);
        r[1] = std::sqrt(1.0 - ac[t]);
        r[2] = flags;
    };
    // row 0: the trial update from t_0 with e_0 alone; the sample it started from is kept, e_0 enters old_eps
    const DdimForm f0 = ddim_form(ac[ts[0]], a_prev(0));
    {
        double* r = &rows[0];
        head(r, ts[0], PD_LMS_F_STORE_KEEP | PD_LMS_F_PUSH);
        r[3] = f0.x; r[4] = f0.e;
        r[8] = f0.px; r[9] = f0.pe;
        times[0] = (double)ts[0];
    }
    // row 1: e_next at t_1 on the trial sample; the step is redone from the kept sample with (e_0 + e_next) / 2
    {
        double* r = &rows[PD_LMS_NCOEF];
        const int64_t t1 = ts[std::min(1, n - 1)];
        head(r, t1, PD_LMS_F_BASE_KEEP | PD_LMS_F_STEP);
        r[3] = f0.x; r[4] = 0.5 * f0.e; r[5] = 0.5 * f0.e;
        r[8] = f0.px; r[9] = 0.5 * f0.pe; r[10] = 0.5 * f0.pe;
        r[13] = 1;
        times[1] = (double)t1;
    }
    // rows 2..: Adams-Bashforth of order min(len(old_eps), 3) + 1 over e_t and old_eps
    for (int i = 1; i < n; ++i) {
        double* r = &rows[(size_t)(i + 1) * PD_LMS_NCOEF];
        const DdimForm f = ddim_form(ac[ts[i]], a_prev(i));
        const int nh = std::min(i, 3);
        head(r, ts[i], PD_LMS_F_PUSH | PD_LMS_F_STEP);
        r[3] = f.x; r[8] = f.px;
        for (int k = 0; k <= nh; ++k) { r[4 + k] = f.e * AB[nh][k]; r[9 + k] = f.pe * AB[nh][k]; }
        r[13] = nh;
        times[i + 1] = (double)ts[i];
    }
    return 0;
}

int dpmpp_rows(const pd_config& cfg, const pd_lms_args& u, const int64_t* ts, int n, std::vector<double>& rows, std::vector<double>& times) {
    if (u.order < 1 || u.order > 3) { pd_set_error("dpm-solver++: order must be 1, 2 or 3 (got %d)", u.order); return 1; }
    if (u.solver_type != PD_LMS_DPM_SOLVER && u.solver_type != PD_LMS_TAYLOR) { pd_set_error("dpm-solver++: unknown solver_type %d", u.solver_type); return 1; }
    std::vector<double> ac;
    alphas_cumprod_f64(cfg, ac);
    std::vector<double> al(n + 1), sg(n + 1), lam(n + 1);
    times.assign(n, 0.0);
    if (u.model_times) {
        // NoiseScheduleVP('discrete').marginal_log_mean_coeff: log alpha linear between the trained points
        for (int i = 0; i <= n; ++i) {
            const double t = u.model_times[i];
            if (!(t >= 0.0 && t <= (double)(cfg.timesteps - 1))) { pd_set_error("dpm-solver++: model time %g outside [0, %d]", t, cfg.timesteps - 1); return 1; }
            if (i > 0 && !(t < u.model_times[i - 1])) { pd_set_error("dpm-solver++: the model times must be strictly descending"); return 1; }
            const int lo = std::min((int)std::floor(t), cfg.timesteps - 2 < 0 ? 0 : cfg.timesteps - 2);
            const double w = t - (double)lo;
            const double l0 = 0.5 * std::log(ac[lo]);
            const double la = cfg.timesteps > 1 ? l0 + w * (0.5 * std::log(ac[lo + 1]) - l0) : l0;
            al[i] = std::exp(la);
            sg[i] = std::sqrt(1.0 - std::exp(2.0 * la));
            if (i < n) times[i] = t;
        }
    } else {
        PD_TRY(check_desc_grid(cfg, ts, n, "dpm-solver++"));
        for (int i = 0; i < n; ++i) {
            al[i] = std::sqrt(ac[ts[i]]);
            sg[i] = std::sqrt(1.0 - ac[ts[i]]);
            times[i] = (double)ts[i];
        }
        al[n] = 1.0;
        sg[n] = 0.0;
    }
    for (int i = 0; i <= n; ++i) lam[i] = std::log(al[i]) - std::log(sg[i]);   // +inf on sigma = 0
    rows.assign((size_t)n * PD_LMS_NCOEF, 0.0);
    for (int i = 0; i < n; ++i) {
        double* r = &rows[(size_t)i * PD_LMS_NCOEF];
        r[0] = al[i];
        r[1] = sg[i];
        r[2] = PD_LMS_F_DATA_PRED | PD_LMS_F_PUSH | PD_LMS_F_STEP;
        r[9] = 1.0;   // pred_x0 = m_i
        int order = std::min(u.order, i + 1);
        if (u.lower_order_final) order = std::min(order, n - i);
        const double h = lam[i + 1] - lam[i];
        if (!std::isfinite(h)) order = 1;   // onto sigma = 0: x0 itself
        const double a1 = al[i + 1];
        const double phi = std::isfinite(h) ? std::expm1(-h) : -1.0;   // exp(-h) - 1
        r[3] = sg[i + 1] / sg[i];
        double w0 = -a1 * phi, w1 = 0.0, w2 = 0.0;
        if (order == 2) {
            // D1_0 = (m_i - m_{i-1}) / r0
            const double r0 = (lam[i] - lam[i - 1]) / h;
            const double d = u.solver_type == PD_LMS_DPM_SOLVER ? -0.5 * (a1 * phi) : a1 * (phi / h + 1.0);
            w0 += d / r0;
            w1 -= d / r0;
        } else if (order == 3) {
            const double r0 = (lam[i] - lam[i - 1]) / h, r1 = (lam[i - 1] - lam[i - 2]) / h;
            // D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1), D2 = (D1_0 - D1_1) / (r0 + r1); x += cD1 D1 + cD2 D2
            const double cD1 = a1 * (phi / h + 1.0);
            const double cD2 = -a1 * ((phi + h) / (h * h) - 0.5);
            const double g0 = cD1 * (1.0 + r0 / (r0 + r1)) + cD2 / (r0 + r1);   // weight of D1_0
            const double g1 = -cD1 * r0 / (r0 + r1) - cD2 / (r0 + r1);          // weight of D1_1
            w0 += g0 / r0;
            w1 += -g0 / r0 + g1 / r1;
            w2 += -g1 / r1;
        }
        r[4] = w0; r[5] = w1; r[6] = w2;
        r[13] = order - 1;
    }
    return 0;
}

// Euler ancestral: k-diffusion's sample_euler_ancestral (eta = 1) restated in the engine's VP variables.  With x~ = x / alpha the
// sample of the variance-exploding form and s = sigma / alpha its noise level, d = (x~ - denoised) / s is the guided eps, and
//   x~' = x~ + d (s_down - s_from) + z s_up,  s_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2),  s_down = sqrt(s_to^2 - s_up^2);
// multiplied by alpha_to this is one row with m_i = eps and the noise coefficient in slot [14].  The loop lands on s = 0, where
// s_up = s_down = 0 and the row returns the x0 prediction.
int euler_a_rows(const pd_config& cfg, const int64_t* ts, int n, std::vector<double>& rows, std::vector<double>& times) {
    PD_TRY(check_desc_grid(cfg, ts, n, "euler_a"));
    std::vector<double> ac;
    alphas_cumprod_f64(cfg, ac);
    rows.assign((size_t)n * PD_LMS_NCOEF, 0.0);
    times.assign(n, 0.0);
    for (int i = 0; i < n; ++i) {
        double* r = &rows[(size_t)i * PD_LMS_NCOEF];
        const double a_from = std::sqrt(ac[ts[i]]), sg_from = std::sqrt(1.0 - ac[ts[i]]), s_from = sg_from / a_from;
        const bool last = i + 1 == n;
        const double a_to = last ? 1.0 : std::sqrt(ac[ts[i + 1]]);
        const double s_to = last ? 0.0 : std::sqrt(1.0 - ac[ts[i + 1]]) / a_to;
        const double s_up = std::sqrt(s_to * s_to * (s_from * s_from - s_to * s_to) / (s_from * s_from));
        const double s_down = std::sqrt(s_to * s_to - s_up * s_up);
        r[0] = a_from;
        r[1] = sg_from;
        r[2] = PD_LMS_F_STEP;
        r[3] = a_to / a_from;
        r[4] = a_to * (s_down - s_from);
        r[8] = 1.0 / a_from;
        r[9] = -sg_from / a_from;
        r[14] = last ? 0.0 : a_to * s_up;
        times[i] = (double)ts[i];
    }
    return 0;
}

}  // namespace

// checks rows a caller brought (or the generators made): flags, history depth against the pushes so far, the step count
static int lms_check_rows(const std::vector<double>& rows, int n_rows, int steps) {
    int pushed = 0, done = 0;
    const int all = PD_LMS_F_DATA_PRED | PD_LMS_F_BASE_KEEP | PD_LMS_F_STORE_KEEP | PD_LMS_F_PUSH | PD_LMS_F_STEP;
    bool kept = false;
    for (int i = 0; i < n_rows; ++i) {
        const double* r = &rows[(size_t)i * PD_LMS_NCOEF];
        const int fl = (int)r[2], nh = (int)r[13];
        if ((double)fl != r[2] || (fl & ~all)) { pd_set_error("lms: row %d has unknown flags %g", i, r[2]); return 1; }
        if ((double)nh != r[13] || nh < 0 || nh > 3 || nh > pushed) { pd_set_error("lms: row %d reads %g earlier outputs, %d pushed", i, r[13], pushed); return 1; }
        if ((fl & PD_LMS_F_DATA_PRED) && !(r[0] > 0.0)) { pd_set_error("lms: row %d predicts data with alpha %g", i, r[0]); return 1; }
        if (fl & PD_LMS_F_STORE_KEEP) kept = true;
        if ((fl & PD_LMS_F_BASE_KEEP) && !kept) { pd_set_error("lms: row %d reads the kept sample before any row stored it", i); return 1; }
        for (int k = 0; k < PD_LMS_NCOEF; ++k)
            if (!std::isfinite(r[k])) { pd_set_error("lms: row %d holds a non-finite coefficient", i); return 1; }
        if (r[15] != 0.0) { pd_set_error("lms: row %d: slot [15] must be zero (got %g)", i, r[15]); return 1; }
        if (fl & PD_LMS_F_PUSH) ++pushed;
        if (fl & PD_LMS_F_STEP) ++done;
    }
    if (done != steps) { pd_set_error("lms: %d rows complete a step, steps = %d", done, steps); return 1; }
    if (n_rows < 1 || !((int)rows[(size_t)(n_rows - 1) * PD_LMS_NCOEF + 2] & PD_LMS_F_STEP)) { pd_set_error("lms: the last row must complete a step"); return 1; }
    return 0;
}

int pd_lms_table(const pd_config& cfg, const pd_lms_args& u, const int64_t* ts, int n, std::vector<double>& rows, std::vector<double>& times) {
    if (n < 1 || n > cfg.timesteps) { pd_set_error("lms: steps must be in [1, %d]", cfg.timesteps); return 1; }
    if (u.kind == PD_LMS_PLMS) {
        if (u.model_times) { pd_set_error("plms: runs on the integer grid (model_times is for dpm-solver++)"); return 1; }
        PD_TRY(plms_rows(cfg, ts, n, rows, times));
    } else if (u.kind == PD_LMS_DPMPP) {
        PD_TRY(dpmpp_rows(cfg, u, ts, n, rows, times));
    } else if (u.kind == PD_LMS_EULER_A) {
        if (u.model_times) { pd_set_error("euler_a: runs on the integer grid (model_times is for dpm-solver++)"); return 1; }
        PD_TRY(euler_a_rows(cfg, ts, n, rows, times));
    } else if (u.kind == PD_LMS_ROWS) {
        if (!u.rows || !u.row_times || u.n_rows < 1 || u.n_rows > 4 * cfg.timesteps) { pd_set_error("lms: rows, row_times and n_rows are required"); return 1; }
        rows.assign(u.rows, u.rows + (size_t)u.n_rows * PD_LMS_NCOEF);
        times.assign(u.row_times, u.row_times + u.n_rows);
        for (double t : times)
            if (!(t >= 0.0 && t <= (double)(cfg.timesteps - 1))) { pd_set_error("lms: row time %g outside [0, %d]", t, cfg.timesteps - 1); return 1; }
    } else {
        pd_set_error("lms: unknown kind %d", u.kind);
        return 1;
    }
    return lms_check_rows(rows, (int)times.size(), n);
}

extern "C" int pd_lms_coefficients(const pd_config* cfg, const pd_lms_args* u, const int64_t* timesteps, int32_t steps, double* rows,
                                   double* row_times, int32_t* n_rows) {
    if (!cfg || !u || !rows || !row_times || !n_rows) { pd_set_error("null argument"); return 1; }
    std::vector<double> tab, times;
    PD_TRY(pd_lms_table(*cfg, *u, timesteps, steps, tab, times));
    // the documented capacity of rows / row_times; the caller's own rows are already there and need no copy
    if ((int)times.size() > steps + 1) { pd_set_error("lms: %d rows do not fit the steps + 1 = %d the output buffers hold", (int)times.size(), steps + 1); return 1; }
    std::memcpy(rows, tab.data(), tab.size() * sizeof(double));
    std::memcpy(row_times, times.data(), times.size() * sizeof(double));
    *n_rows = (int32_t)times.size();
    return 0;
}
