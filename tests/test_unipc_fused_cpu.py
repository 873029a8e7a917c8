"""Coefficient rows of the fused UniPC loop (pd_unipc_coefficients, csrc/multistep.cpp), checked on the CPU: evaluated in
NumPy exactly as the device kernel combines them, on a fake model, they must reproduce the host plug-in
UniPCMultistepScheduler (the reference these rows restate) step by step, for every variant the scheduler offers."""
import itertools
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


def fake_eps(x, t):
    """a non-linear "model" so that every history term matters"""
    return np.tanh(x) * (0.3 + t / 1000.0) + 0.1 * np.sin(3 * x + t / 250.0)


def run_rows(coef, ts, x_T):
    """The device kernel's update (UnipcSolver::update, sampler_update.hip) in fp64 NumPy."""
    x = np.asarray(x_T, np.float64)
    ring, last, out = {}, None, []
    for i, t in enumerate(ts):
        r = coef[i]
        m = (x - r[1] * fake_eps(x, int(t))) / r[0]
        hist = [ring.get(i - 1 - k) for k in range(3)]
        use = lambda w, v: 0.0 if w == 0.0 else w * v
        xc = x
        if r[2]:
            xc = r[3] * last + r[4] * m + use(r[5], hist[0]) + use(r[6], hist[1]) + use(r[7], hist[2])
        x = r[8] * xc + r[9] * m + use(r[10], hist[0]) + use(r[11], hist[1])
        last = xc
        ring[i] = m
        out.append(x)
    return out


def run_scheduler(sc, x_T):
    x, out = np.asarray(x_T, np.float64), []
    for t in sc.timesteps:
        x = sc.step(fake_eps(x, int(t)), t, x, return_dict=False)[0]
        out.append(x)
    return out


def test_rows_match_host_scheduler_every_step(lib):
    x_T = np.random.default_rng(0).standard_normal((2, 4, 4, 4))
    worst, n_cases = 0.0, 0
    for order, st, lof, dc, spacing, steps in itertools.product((1, 2, 3), ("bh1", "bh2"), (True, False), ((), (1,), (0, 2)),
                                                                 ("linspace", "leading", "trailing"), (1, 2, 3, 5, 20, 50)):
        sc = UniPCMultistepScheduler(solver_order=order, solver_type=st, lower_order_final=lof, disable_corrector=list(dc),
                                     timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
        sc.set_timesteps(steps)
        ref = run_scheduler(sc, x_T)
        coef = E.unipc_coefficients(W.TINY, sc.timesteps, order=order, solver_type=st, lower_order_final=lof,
                                    disable_corrector=dc)
        assert coef.shape == (steps, E.PD_UNIPC_NCOEF)
        got = run_rows(coef, sc.timesteps, x_T)
        for i, (g, r) in enumerate(zip(got, ref)):
            err = float(np.abs(g - r).max() / np.abs(r).max())
            assert err <= 1e-10, (order, st, lof, dc, spacing, steps, i, err)
            worst = max(worst, err)
        n_cases += 1
    print(f"max relative error over {n_cases} variants: {worst:.3e}")


def test_row_layout(lib):
    sc = UniPCMultistepScheduler(solver_order=3)
    sc.set_timesteps(6)
    ac = E.alphas_cumprod(W.TINY)
    np.testing.assert_allclose(ac, sc.alphas_cumprod, rtol=1e-12, atol=0)
    coef = E.unipc_coefficients(W.TINY, sc.timesteps, order=3, disable_corrector=[2])
    np.testing.assert_allclose(coef[:, 0], np.sqrt(ac[sc.timesteps]), rtol=1e-15)
    np.testing.assert_allclose(coef[:, 1], np.sqrt(1.0 - ac[sc.timesteps]), rtol=1e-15)
    # warm-up 1, 2, 3, then lower_order_final 3, 2, and the step onto sigma = 0 is first order: x_S = m_{S-1}
    assert list(coef[:, 12]) == [1, 2, 3, 3, 2, 1]
    # corrector: none at step 0 and after step 2; otherwise of the previous predictor's order
    assert list(coef[:, 2]) == [0, 1, 1, 0, 1, 1]
    assert list(coef[:, 13]) == [0, 1, 2, 0, 3, 2]
    last = coef[-1]
    assert last[8] == 0.0 and last[9] == 1.0 and not last[10:12].any()
    assert not coef[:, 14:].any()


def test_rejected_inputs(lib):
    ts = [999, 600, 200]
    for bad in (dict(order=0), dict(order=4)):
        with pytest.raises(E.PdError, match="order"):
            E.unipc_coefficients(W.TINY, ts, **bad)
    with pytest.raises(E.PdError, match="strictly descending"):
        E.unipc_coefficients(W.TINY, [999, 600, 600, 200])
    with pytest.raises(E.PdError, match="strictly descending"):
        E.unipc_coefficients(W.TINY, [200, 600, 999])
    with pytest.raises(E.PdError, match="outside"):
        E.unipc_coefficients(W.TINY, [1000, 600])
    with pytest.raises(E.PdError, match="required"):
        E.unipc_coefficients(W.TINY, [])
    with pytest.raises(ValueError, match="solver_type"):
        E.unipc_coefficients(W.TINY, ts, solver_type="midpoint")
