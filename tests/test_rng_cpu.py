"""Seeded noise without a GPU: the host Philox block against its known answers, the ABI additions, the Euler ancestral rows
(pd_lms_coefficients, PD_LMS_EULER_A) against the fp64 restatement in tests/rng_ref.py and against the identities that follow
from their formulas, and the host EulerAncestralDiscreteScheduler against the rows."""
import ctypes as C

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.schedulers import DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler
from tests import rng_ref as R

CFG = W.TINY
GRIDS = [[999, 800, 600, 400, 200, 50], [981, 1], [500], [801, 601, 401, 201, 1]]

KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = E.philox4x32_10(ctr, key)
    assert " ".join("%08x" % v for v in got) == want
    ref = R.philox4x32_10(ctr, key)                 # the restatement the GPU tests lean on gives the same block
    assert tuple(int(v) for v in ref) == got


def test_restatement_uniforms_and_tail():
    assert R.u01(0) == np.float32(2.0 ** -33) and R.u01(0xFFFFFFFF) == np.float32(1.0)
    z5, r5 = R.normals(7, 3, 2, "step", 5)
    z8, r8 = R.normals(7, 3, 2, "step", 8)
    assert np.array_equal(z5, z8[:5]) and np.array_equal(r5, r8[:5]) and r8[0] == r8[1] and r8[2] == r8[3]


def test_exports_and_struct_layouts_unchanged():
    lib = E.load_library()
    for name in ("pd_philox4x32_10", "pd_set_rng", "pd_get_rng", "pd_randn"):
        assert hasattr(lib, name) and name in E.EXPORTS
    assert lib.pd_abi_version() == 2
    assert (E.PD_INIT_PURE_NOISE, E.PD_NOISE_FROM_SEED, E.PD_XT_FROM_SEED) == (1, 2, 4)
    assert (E.PD_RNG_XT, E.PD_RNG_STEP, E.PD_RNG_VAE, E.PD_RNG_USER, E.PD_LMS_EULER_A) == (0, 1, 2, 16, 3)
    a, l = E.pd_sample_args, E.pd_lms_args
    assert C.sizeof(a) == 160 and C.sizeof(l) == 56
    assert (a.x_T.offset, a.noise.offset, a.timesteps.offset, a.init_latents.offset, a.mask.offset, a.init_flags.offset) == \
        (48, 120, 128, 136, 144, 152)
    assert (l.kind.offset, l.model_times.offset, l.rows.offset, l.row_times.offset, l.n_rows.offset) == (0, 16, 24, 32, 40)


@pytest.mark.parametrize("grid", GRIDS)
def test_euler_a_rows(grid):
    rows, times = E.lms_coefficients(CFG, grid, kind="euler_a")
    ac = E.alphas_cumprod(CFG)
    ref = R.euler_a_rows(ac, grid)
    assert rows.shape == ref.shape == (len(grid), E.PD_LMS_NCOEF) and np.array_equal(times, np.asarray(grid, np.float64))
    np.testing.assert_allclose(rows, ref, rtol=1e-12, atol=0)
    assert np.all(rows[:, 2] == E.PD_LMS_F_STEP) and np.all(rows[:, 13] == 0) and np.all(rows[:, 15] == 0)
    a = np.sqrt(np.append(ac[grid], 1.0))
    s = np.sqrt(1.0 - np.append(ac[grid], 1.0))
    for i in range(len(grid)):
        # the deterministic part lands on alpha_to, and drift + noise together keep the marginal variance sigma_to^2
        np.testing.assert_allclose(rows[i, 3] * a[i], a[i + 1], rtol=1e-12)
        np.testing.assert_allclose((rows[i, 3] * s[i] + rows[i, 4]) ** 2 + rows[i, 14] ** 2, s[i + 1] ** 2, rtol=1e-12, atol=1e-24)
    assert rows[-1, 14] == 0.0 and np.all(rows[:-1, 14] > 0.0)


def test_own_rows_accept_a_noise_coefficient():
    grid = GRIDS[0]
    rows, times = E.lms_coefficients(CFG, grid, kind="dpmsolver++", order=2)
    mine = rows.copy()
    mine[:, 14] = np.linspace(0.3, -0.1, len(grid))
    r2, t2 = E.lms_coefficients(CFG, kind="rows", rows=mine, row_times=times, steps=len(grid))
    assert np.array_equal(r2, mine) and np.array_equal(t2, times)
    for bad14 in (np.inf, np.nan):
        bad = mine.copy()
        bad[2, 14] = bad14
        with pytest.raises(E.PdError, match="non-finite"):
            E.lms_coefficients(CFG, kind="rows", rows=bad, row_times=times, steps=len(grid))
    bad = mine.copy()
    bad[1, 15] = 1e-3
    with pytest.raises(E.PdError, match=r"\[15\] must be zero"):
        E.lms_coefficients(CFG, kind="rows", rows=bad, row_times=times, steps=len(grid))
    with pytest.raises(E.PdError, match="integer grid"):
        E.lms_coefficients(CFG, kind="euler_a", model_times=[999.0, 500.5, 0.0])


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
def test_host_euler_a_scheduler_follows_the_rows(spacing):
    s = EulerAncestralDiscreteScheduler(timestep_spacing=spacing)
    s.set_timesteps(7)
    assert s.init_noise_sigma == 1.0 and len(s.timesteps) == 7 and np.all(np.diff(s.timesteps) < 0)
    fused = s.fused_lms()
    assert fused["kind"] == "euler_a"
    rows, _ = E.lms_coefficients(CFG, fused["timesteps"], kind="euler_a")
    shape = (2, 4, 8, 8)
    data = np.random.default_rng(5)
    x = data.standard_normal(shape)
    g_sched, g_ref = np.random.default_rng(11), np.random.default_rng(11)
    for i, t in enumerate(s.timesteps):
        eps = data.standard_normal(shape)
        want = rows[i, 3] * x + rows[i, 4] * eps
        if rows[i, 14] != 0.0:
            want = want + rows[i, 14] * g_ref.standard_normal(shape)
        got = s.step(eps, t, x, generator=g_sched, return_dict=False)[0]
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(s.pred_original_sample, rows[i, 8] * x + rows[i, 9] * eps, rtol=1e-12, atol=1e-14)
        x = got
    assert g_sched.standard_normal() == g_ref.standard_normal()     # the last step drew nothing


def test_sde_dpmsolver_still_refused():
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")


def test_distribution_seed_passes_on_the_restatement():
    """The fixed seed of the GPU distribution test, checked here on the fp64 restatement alone."""
    from scipy import stats
    n = 1 << 20
    z, _ = R.normals(R.DIST_SEED, 0, 0, "step", n)
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert stats.kstest(z, "norm").statistic < 1.63 / np.sqrt(n)

