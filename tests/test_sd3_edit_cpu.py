"""SD3 img2img / inpainting without a GPU: the truncation of the grid by `strength` (diffusers' SD3 img2img get_timesteps, restated in
include/pdengine.h), its two ValueErrors, and the invariants of the NumPy restatement tests/sd3_edit_ref.py that the GPU tests lean on."""
import numpy as np
import pytest

from oracle import sd3_oracle as O
from prompt_diffusion_amd import sd3
from tests import sd3_edit_ref as R

CFG = sd3.SD3_TINY


# t_start = int(max(n - min(n * strength, n), 0)), worked by hand; where n * strength is no integer, int() truncates the difference
@pytest.mark.parametrize("n,strength,want", [
    (28, 1.0, 0), (4, 1.0, 0), (28, 0.5, 14), (4, 0.5, 2), (4, 0.75, 1),
    (28, 0.6, 11),       # 28 - 16.8 = 11.2: 17 steps run
    (10, 0.33, 6),       # 10 - 3.3 = 6.7
    (7, 0.5, 3),         # 7 - 3.5 = 3.5
    (3, 0.4, 1),         # 3 - 1.2 = 1.8
    (4, 0.2, 3),         # 4 - 0.8 = 3.2: one step left
    (50, 0.02, 49),      # exactly one step left
])
def test_truncation(n, strength, want):
    assert sd3.img2img_start(n, strength) == want == R.t_start(n, strength)
    sig = sd3.flow_match_sigmas(n)
    kept = R.truncate(sig, strength)
    assert len(kept) - 1 == n - want and kept[-1] == 0.0 and np.array_equal(kept, sig[want:])


@pytest.mark.parametrize("f", [sd3.img2img_start, R.t_start])
def test_truncation_errors(f):
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            f(10, bad)
    for n, s in ((10, 0.0), (1, 0.0), (10, 1e-20)):      # nothing left to run (10 - 1e-19 is 10.0 in double)
        with pytest.raises(ValueError, match="step"):
            f(n, s)


def _case(B=1, h=8, w=8, S=4, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    C = CFG.in_channels
    a = dict(z0=f(B, C, h, w), eps=f(B, C, h, w), cond=f(B, C, h, w), pair=f(B, C, h, w), pe=f(B, S, CFG.joint_dim),
             npe=f(B, S, CFG.joint_dim), ppe=f(B, CFG.pooled_dim), nppe=f(B, CFG.pooled_dim))
    return a


def test_reference_invariants():
    """m = 0 returns z0 exactly, m = 1 is img2img exactly, and at strength 1 (sigma_0 = 1) the start state is eps: the loop then equals
    the oracle's plain sampling from eps."""
    sd = sd3.synth_sd3_state_dict(CFG)
    a = _case()
    vel = R.oracle_velocity(sd, CFG, a["pe"], a["npe"], a["ppe"], a["nppe"], a["cond"], a["pair"], 4.0)
    sig = R.truncate(O.flow_match_sigmas(3), 1.0)
    shape = (1, 1, 8, 8)
    img = R.sample(vel, sig, a["z0"], a["eps"])
    assert np.array_equal(R.sample(vel, sig, a["z0"], a["eps"], mask=np.zeros(shape, np.float32)), a["z0"])
    assert np.array_equal(R.sample(vel, sig, a["z0"], a["eps"], mask=np.ones(shape, np.float32)), img)
    assert sig[0] == 1.0 and np.array_equal(R.start_state(sig[0], a["eps"], a["z0"]), a["eps"])
    plain = O.sample(sd, CFG, a["eps"], a["pe"], a["npe"], a["ppe"], a["nppe"], a["cond"], a["pair"], 3, 4.0)
    assert np.array_equal(img, plain)
    # a half mask: kept pixels are z0, repainted ones are not
    m = np.zeros(shape, np.float32)
    m[..., 4:] = 1.0
    out = R.sample(vel, sig, a["z0"], a["eps"], mask=m)
    assert np.array_equal(out[..., :4], a["z0"][..., :4]) and not np.array_equal(out[..., 4:], a["z0"][..., 4:])


def test_blend_arithmetic_is_float32_in_the_written_order():
    rng = np.random.default_rng(3)
    z0, eps, x = (rng.standard_normal((2, 4, 6, 10)).astype(np.float32) for _ in range(3))
    m = rng.choice(np.array([0.0, 1.0, 0.25], np.float32), (2, 1, 6, 10))
    s = np.float32(0.37)
    one = np.float32(1.0)
    k = R.known(s, z0, eps)
    assert k.dtype == np.float32 and np.array_equal(k, (one - s) * z0 + s * eps)
    out = R.blend(m, k, x)
    assert out.dtype == np.float32 and np.array_equal(out, (one - m) * k + m * x)
    assert np.array_equal(R.known(0.0, z0, eps), z0)
    st = R.start_state(s, eps, z0)
    assert np.array_equal(st, s * eps + (one - s) * z0)
    # within half an ulp-scale bound of the fp64 value
    ref = float(s) * eps.astype(np.float64) + (1.0 - float(s)) * z0.astype(np.float64)
    assert np.all(np.abs(st - ref) <= 3 * 2.0 ** -24 * (np.abs(eps) + np.abs(z0)))


def test_package_exports_the_pipelines():
    import prompt_diffusion_amd as P
    from prompt_diffusion_amd import pipeline_sd3
    assert P.StableDiffusion3PromptDiffusionImg2ImgPipeline is pipeline_sd3.StableDiffusion3PromptDiffusionImg2ImgPipeline
    assert P.StableDiffusion3PromptDiffusionInpaintPipeline is pipeline_sd3.StableDiffusion3PromptDiffusionInpaintPipeline
    assert issubclass(P.StableDiffusion3PromptDiffusionInpaintPipeline, P.StableDiffusion3PromptDiffusionPipeline)
