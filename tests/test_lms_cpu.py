"""Linear multistep solvers (PLMS, DPM-Solver++ multistep) without a GPU: the coefficient rows of pd_lms_coefficients and the
host schedulers against tests/golden/samplers_lms.npz, which the reference's own PLMSSampler / DPM_Solver produced
(tests/golden/make_golden_samplers.py).

Tolerances are not constants chosen here: each trajectory's bound is 4 x the fixture's own `<tag>_f64diff`, the distance
between the reference's fp32 run and the same chain in fp64 from the recorded eps.  The reference's fp32 chain and any fp64
chain differ by that accumulated rounding; a handful of ulps of headroom keeps the test from pinning fp32 noise."""
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import schedulers as SCH
from prompt_diffusion_amd import weights as W
from tests import lms_ref as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CFG = W.TINY


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "samplers_lms.npz"))


PLMS_TAGS = ["an_plms_s3", "an_plms_s5", "an_plms_s10", "tiny_plms_s5"]
DPM_TAGS = [f"an_dpmpp_o{o}_{st}_lof{l}" for o in (1, 2, 3) for st in ("dpm_solver", "taylor") for l in (1, 0)] + \
           ["tiny_dpmpp_int_s9", "tiny_dpmpp_frac_s5"]


def _dpm_kw(fx, tag):
    mt = fx[tag + "_model_times"]
    S = len(mt) - 1
    return dict(kind="dpmsolver++", order=int(fx[tag + "_order"]), solver_type="taylor" if int(fx[tag + "_taylor"]) else "dpm_solver",
                lower_order_final=bool(fx[tag + "_lof"]) and S < 15, model_times=mt)


@pytest.mark.parametrize("tag", PLMS_TAGS)
def test_plms_rows_reproduce_reference(fx, tag):
    grid, xs, preds, eps = fx[tag + "_grid"], fx[tag + "_x"], fx[tag + "_pred_x0"], fx[tag + "_eps"]
    rows, times = E.lms_coefficients(CFG, grid, kind="plms")
    S = len(grid)
    assert rows.shape == (S + 1, E.PD_LMS_NCOEF)
    # the evaluation points: t0, t1, t1, t2, ... exactly where the reference evaluated its model
    assert times.tolist() == fx[tag + "_eval_t"].tolist()
    got_x, got_p, done = L.apply_rows(rows, xs[0], eps)
    assert done == [False] + [True] * S
    gx = [x for x, d in zip(got_x, done) if d]
    gp = [p for p, d in zip(got_p, done) if d]
    tol = 4.0 * float(fx[tag + "_f64diff"])
    dx, dp = L.maxdiff(gx, xs[1:]), L.maxdiff(gp, preds)
    print(f"{tag}: |x - ref| {dx:.3e}, |pred_x0 - ref| {dp:.3e}, bound {tol:.3e}")
    assert dx <= tol and dp <= tol


@pytest.mark.parametrize("tag", DPM_TAGS)
def test_dpmpp_rows_reproduce_reference(fx, tag):
    xs, preds, eps = fx[tag + "_x"], fx[tag + "_pred_x0"], fx[tag + "_eps"]
    kw = _dpm_kw(fx, tag)
    rows, times = E.lms_coefficients(CFG, **kw)
    assert len(rows) == len(eps) and np.array_equal(times, kw["model_times"][:-1])
    got_x, got_p, done = L.apply_rows(rows, xs[0], eps)
    assert all(done)
    tol = 4.0 * float(fx[tag + "_f64diff"])
    dx, dp = L.maxdiff(got_x, xs[1:]), L.maxdiff(got_p, preds)
    print(f"{tag}: |x - ref| {dx:.3e}, |pred_x0 - ref| {dp:.3e}, bound {tol:.3e}")
    assert dx <= tol and dp <= tol


@pytest.mark.parametrize("tag", PLMS_TAGS)
def test_pndm_scheduler_reproduces_reference(fx, tag):
    grid, xs, preds, eps = fx[tag + "_grid"], fx[tag + "_x"], fx[tag + "_pred_x0"], fx[tag + "_eps"]
    s = SCH.PNDMScheduler()
    s.set_timesteps(timesteps=grid)
    # the duplicated second timestep = the reference's evaluation points
    assert [int(t) for t in s.timesteps] == fx[tag + "_eval_t"].tolist()
    x = xs[0].astype(np.float64)
    got_x, got_p = [], []
    for i, t in enumerate(s.timesteps):
        ends = s.completes_step()
        x = s.step(eps[i].astype(np.float64), t, x, return_dict=False)[0]
        if ends:
            got_x.append(x); got_p.append(s.pred_original_sample)
    tol = 4.0 * float(fx[tag + "_f64diff"])
    dx, dp = L.maxdiff(got_x, xs[1:]), L.maxdiff(got_p, preds)
    print(f"{tag}: scheduler |x - ref| {dx:.3e}, |pred_x0 - ref| {dp:.3e}, bound {tol:.3e}")
    assert len(got_x) == len(grid) and dx <= tol and dp <= tol


@pytest.mark.parametrize("tag", DPM_TAGS)
def test_dpm_scheduler_reproduces_reference(fx, tag):
    xs, preds, eps = fx[tag + "_x"], fx[tag + "_pred_x0"], fx[tag + "_eps"]
    kw = _dpm_kw(fx, tag)
    s = SCH.DPMSolverMultistepScheduler(solver_order=kw["order"], solver_type="heun" if kw["solver_type"] == "taylor" else "midpoint",
                                        lower_order_final=bool(fx[tag + "_lof"]))
    s.set_model_times(kw["model_times"])
    x = xs[0].astype(np.float64)
    got_x, got_p = [], []
    for i, t in enumerate(s.timesteps):
        x = s.step(eps[i].astype(np.float64), t, x, return_dict=False)[0]
        got_x.append(x); got_p.append(s.pred_original_sample)
    tol = 4.0 * float(fx[tag + "_f64diff"])
    dx, dp = L.maxdiff(got_x, xs[1:]), L.maxdiff(got_p, preds)
    print(f"{tag}: scheduler |x - ref| {dx:.3e}, |pred_x0 - ref| {dp:.3e}, bound {tol:.3e}")
    assert dx <= tol and dp <= tol


def test_scheduler_grids_and_rows_agree():
    """On its own (diffusers-style, sigma = 0 landing) grid each host scheduler and the rows of its fused form are the same
    linear map: random eps, fp64, a few ulps apart."""
    g = np.random.default_rng(3)
    for sched in [SCH.PNDMScheduler()] + [SCH.DPMSolverMultistepScheduler(solver_order=o, solver_type=st)
                                         for o in (1, 2, 3) for st in ("midpoint", "heun")]:
        sched.set_timesteps(7)
        kw = sched.fused_lms()
        rows, times = E.lms_coefficients(CFG, kw.pop("timesteps"), **kw)
        assert [float(t) for t in sched.timesteps] == times.tolist()
        eps = g.standard_normal((len(times), 1, 4, 4, 4))
        x = x0 = g.standard_normal((1, 4, 4, 4))
        for i, t in enumerate(sched.timesteps):
            x = sched.step(eps[i], t, x, return_dict=False)[0]
        got = L.apply_rows(rows, x0, eps)[0][-1]
        assert np.abs(got - x).max() < 1e-12 * max(1.0, np.abs(x).max())


def test_dpmpp2m_is_unipc_bh2_predictor():
    """DPM-Solver++(2M, 'dpm_solver') = UniPC's order-2 bh2 predictor with the corrector off -- the identity
    tests/golden/dpm_solver_2m.npz states, now through the new rows."""
    ts = [981, 801, 621, 441, 261, 81]
    u = E.unipc_coefficients(CFG, ts, order=2, solver_type="bh2", lower_order_final=True, disable_corrector=list(range(len(ts))))
    rows, _ = E.lms_coefficients(CFG, ts, kind="dpmsolver++", order=2, solver_type="dpm_solver", lower_order_final=True)
    assert np.all(u[:, 2] == 0.0)
    np.testing.assert_allclose(rows[:, 0:2], u[:, 0:2], rtol=0, atol=0)
    np.testing.assert_allclose(rows[:, 3:7], u[:, 8:12], rtol=1e-13, atol=1e-15)
    assert rows[:, 13].tolist() == (u[:, 12] - 1).tolist()
    d = np.load(os.path.join(GOLD, "dpm_solver_2m.npz"))
    for S in (8, 5):
        mt = (d[f"s{S}_t"] - 1.0 / 1000) * 1000.0
        mt[-1] = max(mt[-1], 0.0)
        r, _ = E.lms_coefficients(CFG, kind="dpmsolver++", order=2, solver_type="dpm_solver", lower_order_final=True, model_times=mt)
        # the fixture's alpha / sigma come from NoiseScheduleVP's float32 linspace t_array (one float32 ulp, 6e-8, on the
        # interpolation nodes); the rows interpolate between exact integers in fp64
        np.testing.assert_allclose(r[:, 0], d[f"s{S}_alpha"][:-1], rtol=2e-7)
        np.testing.assert_allclose(r[:, 1], d[f"s{S}_sigma"][:-1], rtol=2e-7)


def test_argument_errors():
    ts = [801, 601, 401, 201, 1]
    with pytest.raises(E.PdError, match="descending"):
        E.lms_coefficients(CFG, ts[::-1], kind="plms")
    with pytest.raises(E.PdError, match="descending"):
        E.lms_coefficients(CFG, ts[::-1], kind="dpmsolver++")
    for o in (0, 4):
        with pytest.raises(E.PdError, match="order"):
            E.lms_coefficients(CFG, ts, kind="dpmsolver++", order=o)
    with pytest.raises(E.PdError, match="outside"):
        E.lms_coefficients(CFG, [1000, 500], kind="plms")
    with pytest.raises(E.PdError, match="integer grid"):
        E.lms_coefficients(CFG, kind="plms", model_times=[999.0, 500.5, 0.0])
    with pytest.raises(NotImplementedError):
        SCH.PNDMScheduler(skip_prk_steps=False)
    with pytest.raises(NotImplementedError):
        SCH.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    with pytest.raises(ValueError):
        SCH.DPMSolverMultistepScheduler(solver_order=4)
    # the caller's own rows: a row may not read more history than was pushed
    rows, times = E.lms_coefficients(CFG, ts, kind="dpmsolver++", order=2)
    bad = rows.copy()
    bad[0, 13] = 1
    with pytest.raises(E.PdError, match="earlier outputs"):
        E.lms_coefficients(CFG, kind="rows", rows=bad, row_times=times, steps=len(ts))
    r2, t2 = E.lms_coefficients(CFG, kind="rows", rows=rows, row_times=times, steps=len(ts))
    assert np.array_equal(r2, rows) and np.array_equal(t2, times)


def test_exports_and_abi():
    lib = E.load_library()
    for name in ("pd_lms_coefficients", "pd_lms_sample", "pd_sample_begin_lms", "pd_sample_rows"):
        assert name in E.EXPORTS and hasattr(lib, name)
    assert lib.pd_abi_version() == 2


def test_double_timestep_embedding_bits():
    """The fractional-time embedding gives the int64 one's bits on 0..999 (both through the library's host functions)."""
    import ctypes as C
    lib = E.load_library()
    lib.pd_op_timestep_embedding_f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pd_op_timestep_embedding_i.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    for dim in (32, 320):
        ti = np.arange(1000, dtype=np.int64)
        tf = ti.astype(np.float64)
        a, b = np.zeros((1000, dim), np.float32), np.zeros((1000, dim), np.float32)
        assert lib.pd_op_timestep_embedding_i(ti.ctypes.data, 1000, dim, a.ctypes.data) == 0
        assert lib.pd_op_timestep_embedding_f(tf.ctypes.data, 1000, dim, b.ctypes.data) == 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a fractional time is not rounded to an integer on the way
        frac = np.zeros((1, dim), np.float32)
        assert lib.pd_op_timestep_embedding_f(np.asarray([799.2]).ctypes.data, 1, dim, frac.ctypes.data) == 0
        assert not np.array_equal(frac[0], a[799]) and not np.array_equal(frac[0], a[800])
        lo = np.float32(799.2) * np.float32(1.0)     # the first frequency is exp(0) = 1: cos / sin of (float)t itself
        np.testing.assert_allclose([frac[0, 0], frac[0, dim // 2]], [np.cos(np.float64(lo)), np.sin(np.float64(lo))], atol=1e-6)


@pytest.mark.parametrize("strength", [1.0, 0.9, 0.8, 0.35])
def test_pipeline_plan_follows_the_scheduler_after_set_begin_index(strength):
    """img2img / inpainting on the host path: PNDMScheduler rebuilds its tail in set_begin_index (the first step there takes
    two evaluations again), so the pipeline's evaluations, step grid and blend levels come from the scheduler afterwards."""
    from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
    s = SCH.PNDMScheduler()
    pipe = PromptDiffusionPipeline(None, scheduler=s)
    s.set_timesteps(10)
    full = [int(t) for t in s.timesteps]
    _, t_start = pipe.get_timesteps(full, strength)
    plan = pipe._eval_plan(t_start)
    assert plan["rows"] == [int(t) for t in s.timesteps[t_start:]]
    grid = plan["grid"]
    assert len(plan["rows"]) == len(grid) + 1 and all(a > b for a, b in zip(grid, grid[1:]))
    assert plan["rows"] == grid[:2] + grid[1:]                      # t0, t1, t1, t2, ...
    assert plan["ends"] == [False] + [True] * len(grid) and plan["step"] == [0, 0] + list(range(1, len(grid)))
    assert s.fused_lms(t_start)["timesteps"] == grid
    # the scheduler steps through exactly these evaluations
    x = np.zeros((1, 4, 2, 2))
    for i, t in enumerate(plan["rows"]):
        assert s.completes_step() == plan["ends"][i]
        x = s.step(np.ones_like(x), t, x, return_dict=False)[0]
    d = SCH.DPMSolverMultistepScheduler()
    pipe = PromptDiffusionPipeline(None, scheduler=d)
    d.set_timesteps(10)
    _, t0 = pipe.get_timesteps([int(t) for t in d.timesteps], strength)
    plan = pipe._eval_plan(t0)
    assert plan["rows"] == plan["grid"] == [int(t) for t in d.timesteps[t0:]] and all(plan["ends"])


def test_own_rows_must_fit_the_documented_buffers():
    """pd_lms_coefficients writes at most steps + 1 rows, the capacity its header documents, for the caller's rows too."""
    ts = [801, 601, 401, 201, 1]
    rows, times = E.lms_coefficients(CFG, ts, kind="plms")          # 6 rows for 5 steps
    r2, _ = E.lms_coefficients(CFG, kind="rows", rows=rows, row_times=times, steps=5)
    assert np.array_equal(r2, rows)
    extra = np.concatenate([rows[:1], rows])                        # 7 rows: a second non-completing evaluation
    import ctypes as C
    lib = E.load_library()
    u, keep = E._lms_args("rows", 2, "dpm_solver", True, None, extra, np.concatenate([times[:1], times]))
    out, tt, nr = np.full((6, E.PD_LMS_NCOEF), -7.0), np.full(6, -7.0), C.c_int32(0)
    c = E.make_config(CFG)
    assert lib.pd_lms_coefficients(C.byref(c), C.byref(u), None, 5, out.ctypes.data, tt.ctypes.data, C.byref(nr)) != 0
    assert b"do not fit" in lib.pd_last_error() and np.all(out == -7.0) and np.all(tt == -7.0)
