"""NumPy fp64 helpers for the linear multistep solver tests (PLMS, DPM-Solver++ multistep): the update chains written out
from the papers' formulas, and the application of pd_lms_coefficients rows.  Shared by tests/test_lms_cpu.py,
tests/test_lms_gpu.py and the fixture generator tests/golden/make_golden_samplers.py."""
import math

import numpy as np

NCOEF = 16
F_DATA_PRED, F_BASE_KEEP, F_STORE_KEEP, F_PUSH, F_STEP = 1, 2, 4, 8, 16
AB = ((1.0,), (1.5, -0.5), (23 / 12, -16 / 12, 5 / 12), (55 / 24, -59 / 24, 37 / 24, -9 / 24))


def alphas_cumprod64(linear_start=0.00085, linear_end=0.012, T=1000):
    return np.cumprod(1.0 - np.linspace(linear_start ** 0.5, linear_end ** 0.5, T, dtype=np.float64) ** 2)


def apply_rows(rows, x0, model_outputs):
    """Run the rows on the recorded guided eps of every evaluation.  Returns (x after every row, pred_x0 of every row,
    completes-a-step flag of every row), all fp64."""
    x = np.asarray(x0, np.float64)
    hist, keep = [], None
    xs, preds, done = [], [], []
    for r, e in zip(np.asarray(rows, np.float64).reshape(-1, NCOEF), model_outputs):
        fl, nh = int(r[2]), int(r[13])
        e = np.asarray(e, np.float64)
        m = (x - r[1] * e) / r[0] if fl & F_DATA_PRED else e
        assert nh <= len(hist)
        old = [hist[-1 - k] if k < nh else 0.0 for k in range(3)]
        if fl & F_STORE_KEEP:
            keep = x
        base = keep if fl & F_BASE_KEEP else x
        xn = r[3] * base + r[4] * m + r[5] * old[0] + r[6] * old[1] + r[7] * old[2]
        p0 = r[8] * base + r[9] * m + r[10] * old[0] + r[11] * old[1] + r[12] * old[2]
        if fl & F_PUSH:
            hist = (hist + [m])[-3:]
        x = xn
        xs.append(xn); preds.append(p0); done.append(bool(fl & F_STEP))
    return xs, preds, done


def plms_chain(ac, grid, x0, eps):
    """PLMS over `grid` (sampling order) from the len(grid) + 1 recorded guided eps (the second one is e_next of the first
    step).  Returns (x after every step [S], pred_x0 of every step [S]); a_prev = ac at the next grid point, ac[0] at the end."""
    ac = np.asarray(ac, np.float64)
    x = np.asarray(x0, np.float64)
    eps = [np.asarray(e, np.float64) for e in eps]
    S = len(grid)

    def move(x, e, j):
        a_t = ac[grid[j]]
        a_prev = ac[grid[j + 1]] if j + 1 < S else ac[0]
        pred = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
        return math.sqrt(a_prev) * pred + math.sqrt(1.0 - a_prev) * e, pred
    xs, preds, old = [], [], []
    x, p = move(x, (eps[0] + eps[1]) / 2, 0)
    old.append(eps[0])
    xs.append(x); preds.append(p)
    for j in range(1, S):
        e = eps[j + 1]
        w = AB[min(len(old), 3)]
        ep = sum(wk * ek for wk, ek in zip(w, [e] + old[::-1]))
        x, p = move(x, ep, j)
        old = (old + [e])[-3:]
        xs.append(x); preds.append(p)
    return xs, preds


def vp_points(ac, model_times):
    """alpha, sigma, lambda at (possibly fractional) model times: log alpha linear between the trained points."""
    ac = np.asarray(ac, np.float64)
    la = np.interp(np.asarray(model_times, np.float64), np.arange(len(ac)), 0.5 * np.log(ac))
    al, sg = np.exp(la), np.sqrt(1.0 - np.exp(2.0 * la))
    return al, sg, np.log(al) - np.log(sg)


def dpmpp_chain(al, sg, x0, eps, order, solver_type, lower_order_final):
    """DPM-Solver++ multistep over len(eps) evaluations; al / sg have one more entry, the landing point (sigma may be 0).
    Returns (x after every step, the x0 prediction of every step)."""
    with np.errstate(divide="ignore"):
        lam = np.log(al) - np.log(sg)
    x = np.asarray(x0, np.float64)
    n = len(eps)
    ms, xs = [], []
    for i in range(n):
        m0 = (x - sg[i] * np.asarray(eps[i], np.float64)) / al[i]
        ms.append(m0)
        o = min(order, i + 1)
        if lower_order_final:
            o = min(o, n - i)
        h = lam[i + 1] - lam[i]
        if not np.isfinite(h):
            o = 1
        phi = math.expm1(-h) if np.isfinite(h) else -1.0
        a1 = al[i + 1]
        xn = (sg[i + 1] / sg[i]) * x - a1 * phi * m0
        if o >= 2:
            r0 = (lam[i] - lam[i - 1]) / h
            D10 = (m0 - ms[-2]) / r0
        if o == 2:
            xn = xn - 0.5 * a1 * phi * D10 if solver_type in ("dpm_solver", "dpmsolver", "midpoint") else xn + a1 * (phi / h + 1.0) * D10
        elif o == 3:
            r1 = (lam[i - 1] - lam[i - 2]) / h
            D11 = (ms[-2] - ms[-3]) / r1
            D1 = D10 + r0 / (r0 + r1) * (D10 - D11)
            D2 = (D10 - D11) / (r0 + r1)
            xn = xn + a1 * (phi / h + 1.0) * D1 - a1 * ((phi + h) / h ** 2 - 0.5) * D2
        x = xn
        xs.append(x)
    return xs, ms


def maxdiff(a, b):
    return float(max(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max() for x, y in zip(a, b)))
