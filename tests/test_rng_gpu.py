"""Seeded noise on the GPU (pd_set_rng / pd_randn, PD_NOISE_FROM_SEED / PD_XT_FROM_SEED, PD_LMS_EULER_A, the seeded VAE
posterior): Engine.randn against the fp64 restatement of tests/rng_ref.py, and the draws made inside the update kernels
against the same loops fed Engine.randn's values as caller noise -- bit for bit, since a draw is a function of its address
(seed, sample, draw, stream, element) alone.

K_ULP, the bound of the fp32 Box-Muller against the restatement in units of 2^-24 * radius: the maximum over 2^22 draws
measured on the MI355X is 3.55; the bound is twice that, rounded up.  It has to stay at or
under 16: the error is a few ulp of logf, sqrtf, sincospif and two multiplies, and more than that means a fast-math form
crept in.

The networks are the tiny f32 ones at B = 2, 16x16 latents, 5 steps."""
import dataclasses

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import EngineGenerator
from prompt_diffusion_amd.schedulers import EulerAncestralDiscreteScheduler
from tests import rng_ref as R

pytestmark = pytest.mark.gpu

K_ULP = 8
FUSED_VS_HOST = 1e-5      # the bound tests/test_lms_gpu.py uses for a fused loop against its host plug-in, per step
B, H, Wd, S = 2, 16, 16, 5
SHAPE = (B, 4, H, Wd)
SEED = 0x1234_5678_9ABC_DEF0


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(W.TINY, precision="f32")
    e.load_state_dict(W.synth_state_dict(W.TINY))
    yield e
    e.close()


@pytest.fixture(scope="module")
def inp():
    i = W.synth_inputs(W.TINY, B, H, Wd)
    return dict(ctx_cond=i["ctx_cond"], ctx_uncond=i["ctx_uncond"], pair=i["pair"], query=i["query"]), i["x_T"]


def test_k_bound_is_sane():
    assert K_ULP <= 16


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("per", [1, 5, 1023, 4096])
def test_randn_matches_restatement(eng, per, nb):
    eng.set_rng(SEED, 0xFFFFFFFE)            # the sample index wraps at 2^32 inside the batch of 3
    assert eng.rng == (SEED, 0xFFFFFFFE)
    for stream, draw in (("step", 3), ("xt", 0), (E.PD_RNG_USER + 1, 7)):
        got = eng.randn((nb, per), stream, draw)
        ref, rad = R.randn(SEED, 0xFFFFFFFE, (nb, per), stream, draw)
        assert got.shape == (nb, per) and got.dtype == np.float32
        excess = np.abs(got.astype(np.float64) - ref) - K_ULP * 2.0 ** -24 * rad
        assert excess.max() <= 0.0, (stream, draw, float(np.abs(got - ref).max()))


def test_randn_distribution(eng):
    from scipy import stats
    n = 1 << 20
    eng.set_rng(R.DIST_SEED)
    z = eng.randn((1, n), "step", 0).reshape(-1).astype(np.float64)
    mean, var, d = z.mean(), z.var(), stats.kstest(z, "norm").statistic
    print(f"[rng] 2^20 draws: mean {mean:.3e}, var - 1 {var - 1:.3e}, KS D {d:.3e} (bound {1.63 / np.sqrt(n):.3e})")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / n)
    assert d < 1.63 / np.sqrt(n)


def test_shard_independence(eng):
    eng.set_rng(SEED, 0)
    both = eng.randn(SHAPE, "step", 2)
    eng.set_rng(SEED, 1)
    np.testing.assert_array_equal(eng.randn((1,) + SHAPE[1:], "step", 2), both[1:])
    assert not np.array_equal(both[0], both[1])


def _step_noise(eng, n=S):
    return np.stack([eng.randn(SHAPE, "step", i) for i in range(n)])


@pytest.mark.parametrize("case", ["plain", "temperature", "inpaint"])
def test_ddim_noise_drawn_in_the_kernel(eng, inp, case):
    kw, x_T = inp
    kw = dict(kw, x_T=x_T, steps=S, cfg_scale=4.0, eta=0.7)
    if case == "temperature":
        kw["temperature"] = 0.5
    if case == "inpaint":
        g = np.random.default_rng(3)
        kw["init_latents"] = g.standard_normal(SHAPE).astype(np.float32)
        kw["mask"] = (g.random((B, 1, H, Wd)) > 0.5).astype(np.float32)
    eng.set_rng(SEED + 1)
    l0 = eng.stat("launches")
    det = eng.ddim_sample(**dict(kw, eta=0.0))
    l1 = eng.stat("launches")
    got, inter = eng.ddim_sample(noise="engine", return_intermediates=True, **kw)
    want, winter = eng.ddim_sample(noise=_step_noise(eng), return_intermediates=True, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(inter, winter)
    assert not np.array_equal(got, det)
    l2 = eng.stat("launches")
    plain = eng.ddim_sample(noise="engine", **kw)
    l3 = eng.stat("launches")
    assert l3 - l2 == l1 - l0               # no launch added per step (the two runs between differ by the per-step copies only)
    np.testing.assert_array_equal(plain, got)


@pytest.mark.parametrize("img2img", [False, True])
def test_x_T_from_seed(eng, inp, img2img):
    kw, _ = inp
    kw = dict(kw, steps=S, cfg_scale=4.0, eta=0.0)
    if img2img:
        kw["init_latents"] = np.random.default_rng(4).standard_normal(SHAPE).astype(np.float32)
        kw["timesteps"] = [601, 401, 201, 1]
    eng.set_rng(SEED + 2)
    x_T = eng.randn(SHAPE, "xt")
    got, inter = eng.ddim_sample(x_T=None, seed_x_T=True, return_intermediates=True, **kw)
    want, winter = eng.ddim_sample(x_T=x_T, return_intermediates=True, **kw)
    np.testing.assert_array_equal(inter[0], x_T if not img2img else winter[0])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(inter, winter)


def test_captured_graph_replays_with_a_new_seed(eng, inp):
    kw, x_T = inp
    kw = dict(kw, x_T=x_T, steps=S, cfg_scale=4.0, eta=0.7, noise="engine")
    eng.set_rng(77)
    ref_a = eng.ddim_sample(**kw)
    eng.set_rng(78)
    ref_b = eng.ddim_sample(**kw)
    assert not np.array_equal(ref_a, ref_b)
    try:
        eng.set_option("graph", 1)
        c0, r0 = eng.stat("graph_captures"), eng.stat("graph_replays")
        eng.set_rng(77)
        g_a = eng.ddim_sample(**kw)              # captured
        assert (eng.stat("graph_captures"), eng.stat("graph_replays")) == (c0 + 1, r0)
        eng.set_rng(78)
        g_b = eng.ddim_sample(**kw)              # replayed: the seed is data the kernels read, not part of the graph
        assert (eng.stat("graph_captures"), eng.stat("graph_replays")) == (c0 + 1, r0 + 1)
    finally:
        eng.set_option("graph", 0)
    np.testing.assert_array_equal(g_a, ref_a)
    np.testing.assert_array_equal(g_b, ref_b)


@pytest.mark.parametrize("use_cfg", [True, False])
def test_euler_a_fused_matches_host_plugin(eng, inp, use_cfg):
    kw, x_T = inp
    args = dict(kw, x_T=x_T, cfg_scale=4.0 if use_cfg else 1.0, use_cfg=use_cfg)
    sched = EulerAncestralDiscreteScheduler()
    sched.set_timesteps(S)
    gen = EngineGenerator(SEED + 3).bind(eng)
    eng.sample_begin(steps=S, eta=0.0, **args)
    x = np.asarray(eng.sample_get(E.PD_GET_LATENTS))
    host = []
    for t in sched.timesteps:
        eps = np.asarray(eng.sample_eps_at(int(t)))
        x = sched.step(eps, t, x, generator=gen, return_dict=False)[0].astype(np.float32)
        host.append(x)
        eng.sample_set_latents(x)
    eng.sample_end()
    out, inter = eng.lms_sample(return_intermediates=True, **args, **sched.fused_lms())
    np.testing.assert_array_equal(inter[0], x_T)
    np.testing.assert_array_equal(inter[-1], out)
    errs = [relerr(inter[i + 1], host[i]) for i in range(S)]
    print(f"[euler_a fused vs host] cfg={use_cfg}: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) <= FUSED_VS_HOST
    eng.set_rng(SEED + 4)
    assert not np.array_equal(eng.lms_sample(**args, **sched.fused_lms()), out)     # the noise really enters


def test_own_rows_with_noise_follow_the_row(eng, inp):
    kw, x_T = inp
    grid = [801, 601, 401, 201, 1]
    rows, times = E.lms_coefficients(W.TINY, grid, kind="euler_a")
    rows = rows.copy()
    rows[:, 14] = [0.5, -0.25, 0.125, 0.0, 0.1]
    eng.set_rng(SEED + 5)
    n = eng.sample_begin_lms(kind="rows", rows=rows, row_times=times, steps=len(grid), noise="engine", x_T=x_T, cfg_scale=3.0, **kw)
    assert n == len(grid)
    for i in range(n):
        x = np.asarray(eng.sample_get(E.PD_GET_LATENTS)).astype(np.float64)
        eng.sample_step(i)
        eps = np.asarray(eng.sample_get(E.PD_GET_EPS)).astype(np.float64)
        z = eng.randn(SHAPE, "step", i).astype(np.float64)
        want = (rows[i, 3] * x + rows[i, 4] * eps) + rows[i, 14] * z
        np.testing.assert_array_equal(np.asarray(eng.sample_get(E.PD_GET_LATENTS)), want.astype(np.float32))
        np.testing.assert_array_equal(np.asarray(eng.sample_get(E.PD_GET_PRED_X0)), (rows[i, 8] * x + rows[i, 9] * eps).astype(np.float32))
    eng.sample_end()


def test_errors_leave_the_engine_usable(eng, inp):
    import ctypes as C
    kw, x_T = inp
    base = dict(kw, x_T=x_T, steps=S, cfg_scale=4.0)
    want = eng.ddim_sample(**base)
    grid = [801, 601, 401, 201, 1]
    rows, times = E.lms_coefficients(W.TINY, grid, kind="euler_a")
    with pytest.raises(E.PdError, match="PD_NOISE_FROM_SEED"):
        eng.lms_sample(kind="rows", rows=rows, row_times=times, steps=len(grid), x_T=x_T, cfg_scale=4.0, **kw)
    out = np.empty(SHAPE, np.float32)
    a, keep, _ = eng._args(noise=_step_noise(eng), eta=0.7, **base)
    a.init_flags |= E.PD_NOISE_FROM_SEED
    assert eng.lib.pd_ddim_sample(eng._h, C.byref(a), a.mem, out.ctypes.data, None) != 0
    assert "noise must be NULL" in eng.lib.pd_last_error().decode()
    a, keep, _ = eng._args(**base)
    a.init_flags |= E.PD_XT_FROM_SEED
    assert eng.lib.pd_ddim_sample(eng._h, C.byref(a), a.mem, out.ctypes.data, None) != 0
    assert "x_T must be NULL" in eng.lib.pd_last_error().decode()
    with pytest.raises(E.PdError, match="needs the noise draws"):
        eng.ddim_sample(eta=0.5, **base)
    np.testing.assert_array_equal(eng.ddim_sample(**base), want)


def test_vae_posterior_sample_from_seed():
    cfg = dataclasses.replace(W.TINY, vae_encoder=True)
    e = E.Engine(cfg, precision="f32")
    for n, a in W.synth_vae_encoder_state_dict(cfg).items():
        e.load_tensor(n, a)
    x = np.random.default_rng(8).uniform(-1.0, 1.0, (2, 3, 64, 64)).astype(np.float32)
    with pytest.raises(E.PdError, match="needs `noise`"):
        e.vae_encode(x, mode="sample")               # nobody chose a seed: as before
    e.set_rng(SEED + 6, 5)
    noise = e.randn((2, 4, 8, 8), "vae")
    want = e.vae_encode(x, mode="sample", noise=noise)
    np.testing.assert_array_equal(e.vae_encode(x, mode="sample"), want)
    np.testing.assert_array_equal(e.vae_encode(x, mode="sample", noise="engine"), want)
    assert not np.array_equal(want, e.vae_encode(x, mode="mean"))
    e.close()
