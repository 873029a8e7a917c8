"""sd3_update_kernel alone (pd_op_sd3_update): the start state, the CFG + Euler update and the inpainting blend of the SD3 loop on a
caller's tensors, against the NumPy float32 restatement (tests/sd3_edit_ref.py: bit-equal where the arithmetic is pinned to separately
rounded fp32 operations) and against an fp64 evaluation under the rounding count of the expression."""
import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import sd3_edit_ref as R

pytestmark = pytest.mark.gpu

# 16 channels: 6 x 10 x 16 = 960 elements per sample is a multiple of neither the 1024-element footprint of a block nor of 256.
# The last two take the kernel's other paths: 5 x 5 x 3 = 75 (no multiple of 4: element-wise accesses, a 3-element last group) and
# 3 x 5 x 4 = 60 (vector accesses, but HW = 15: a group straddles channels and reads its mask values one by one).
SHAPES = [(16, 8, 8), (16, 8, 12), (16, 6, 10), (3, 5, 5), (4, 3, 5)]
G, DS, SIG = np.float32(4.5), np.float32(-0.3125 - 1e-3), np.float32(0.37)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(W.TINY, precision="f32")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case(B, C, H, Wd, cfg, seed=0):
    rng = np.random.default_rng(seed + 100 * B + C + H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    v = f((2 if cfg else 1) * B, C, H, Wd)
    x, z0, eps = f(B, C, H, Wd), f(B, C, H, Wd), f(B, C, H, Wd)
    # 0, 1 and 0.25, a pattern that differs per sample and per row (and is not symmetric in h, w)
    vals = np.array([0.0, 1.0, 0.25], np.float32)
    b, y, xx = np.meshgrid(np.arange(B), np.arange(H), np.arange(Wd), indexing="ij")
    m = vals[(2 * b + y + xx // 3) % 3][:, None]
    assert B == 1 or not np.array_equal(m[0], m[1])
    assert not np.array_equal(m[0, 0, 0], m[0, 0, 1])
    return v, x, z0, eps, np.ascontiguousarray(m)


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C,H,Wd", SHAPES)
def test_update(eng, C, H, Wd, B, cfg):
    v, x, z0, eps, m = case(B, C, H, Wd, cfg)
    shape = (B, C, H, Wd)
    kw = dict(use_cfg=cfg, guidance=G, dsigma=DS)
    # the Euler part alone, then the whole update
    x1, x1_in = eng.op_sd3_update(shape, v=v, x=x, want_x_in=True, **kw)
    out, out_in = eng.op_sd3_update(shape, v=v, x=x, z0=z0, mask=m, eps=eps, sigma=SIG, want_x_in=True, **kw)
    # blend: bit-equal to the float32 restatement applied to the kernel's own Euler result
    assert np.array_equal(bits(out), bits(R.blend(m, R.known(SIG, z0, eps), x1)))
    # both halves of the doubled input hold the new state
    for got, got_in in ((x1, x1_in), (out, out_in)):
        assert np.array_equal(bits(got_in[:B]), bits(got)) and np.array_equal(bits(got_in[B:]), bits(got))
    # the whole update against fp64, per element, under the rounding count of the expression
    d = lambda a: a.astype(np.float64)
    vn, vp = d(v[:B]), d(v[B:] if cfg else v[:B])
    g, ds, s = (float(G) if cfg else 0.0), float(DS), float(SIG)
    xe = d(x) + ds * (vn + g * (vp - vn))
    ref = (1.0 - d(m)) * ((1.0 - s) * d(z0) + s * d(eps)) + d(m) * xe
    scale = np.abs(x) + abs(ds) * (np.abs(vn) + abs(g) * (np.abs(vp) + np.abs(vn)))
    bound = 8 * 2.0 ** -24
    e1 = np.abs(x1 - xe) / scale
    e2 = np.abs(out - ref) / (scale + np.abs(z0) + np.abs(eps))
    print(f"[sd3_update] {shape} cfg={cfg}: euler {e1.max() / 2.0 ** -24:.2f}, whole {e2.max() / 2.0 ** -24:.2f} x 2^-24 (bound 8)")
    assert e1.max() <= bound and e2.max() <= bound
    # the last step of a schedule (sigma = 0): k is z0 itself, so m = 0 pixels hold z0 exactly
    last = eng.op_sd3_update(shape, v=v, x=x, z0=z0, mask=m, eps=eps, sigma=0.0, **kw)
    keep = np.broadcast_to(m == 0.0, shape)
    assert np.array_equal(last[keep], z0[keep])
    assert np.array_equal(bits(last), bits(R.blend(m, R.known(0.0, z0, eps), x1)))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C,H,Wd", SHAPES)
def test_start_state(eng, C, H, Wd, B):
    _, _, z0, eps, _ = case(B, C, H, Wd, False, seed=5)
    shape = (B, C, H, Wd)
    got, got_in = eng.op_sd3_update(shape, z0=z0, eps=eps, sigma=SIG, want_x_in=True)
    assert np.array_equal(bits(got), bits(R.start_state(SIG, eps, z0)))
    assert np.array_equal(bits(got_in[:B]), bits(got)) and np.array_equal(bits(got_in[B:]), bits(got))
    ref = float(SIG) * eps.astype(np.float64) + (1.0 - float(SIG)) * z0.astype(np.float64)
    assert np.all(np.abs(got - ref) <= 8 * 2.0 ** -24 * (np.abs(z0) + np.abs(eps)))
    assert np.array_equal(bits(eng.op_sd3_update(shape, z0=z0, eps=eps, sigma=SIG, pure=True)), bits(eps))
    assert np.array_equal(bits(eng.op_sd3_update(shape, eps=eps, sigma=SIG, pure=True)), bits(eps))
    # sigma_0 = 1 (strength 1): the start state is eps
    assert np.array_equal(eng.op_sd3_update(shape, z0=z0, eps=eps, sigma=1.0), eps)


@pytest.mark.parametrize("seed,base", [(1234, 0), (2 ** 40 + 17, 3)])
@pytest.mark.parametrize("C,H,Wd", SHAPES)
def test_seeded_mode_is_the_tensor_mode_fed_with_randn(eng, C, H, Wd, seed, base):
    B = 2
    v, x, z0, _, m = case(B, C, H, Wd, True, seed=9)
    shape = (B, C, H, Wd)
    eng.set_rng(seed, base)
    try:
        eps = eng.randn(shape, "xt", 0)
        kw = dict(use_cfg=True, guidance=G, dsigma=DS, sigma=SIG)
        a = eng.op_sd3_update(shape, v=v, x=x, z0=z0, mask=m, eps=eps, **kw)
        b = eng.op_sd3_update(shape, v=v, x=x, z0=z0, mask=m, seeded=True, **kw)
        assert np.array_equal(bits(a), bits(b))
        a = eng.op_sd3_update(shape, z0=z0, eps=eps, sigma=SIG)
        b = eng.op_sd3_update(shape, z0=z0, seeded=True, sigma=SIG)
        assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(eng.op_sd3_update(shape, seeded=True, pure=True)), bits(eps))     # the engine-drawn start latents
        # sample b of this call is sample base + b of an unsharded one
        eng.set_rng(seed, base + 1)
        assert np.array_equal(bits(eng.op_sd3_update((1, C, H, Wd), seeded=True, pure=True)), bits(eps[1:]))
    finally:
        eng.set_rng(0, 0)


def test_argument_errors(eng):
    shape = (1, 16, 8, 8)
    t = np.zeros(shape, np.float32)
    m = np.zeros((1, 1, 8, 8), np.float32)
    with pytest.raises(E.PdError, match="mask needs"):
        eng.op_sd3_update(shape, v=t, x=t, mask=m, eps=t)
    with pytest.raises(E.PdError, match="mask needs"):
        eng.op_sd3_update(shape, z0=t, mask=m, eps=t)
    with pytest.raises(E.PdError, match="exclude"):
        eng.op_sd3_update(shape, z0=t, eps=t, seeded=True)
    with pytest.raises(E.PdError, match="eps is required"):
        eng.op_sd3_update(shape, z0=t)
    with pytest.raises(E.PdError, match="needs z0"):
        eng.op_sd3_update(shape, eps=t)
    with pytest.raises(E.PdError, match="needs x"):
        eng.op_sd3_update(shape, v=t)
    with pytest.raises(E.PdError, match="bad shape"):
        eng.op_sd3_update((0, 16, 8, 8), eps=np.zeros((0, 16, 8, 8), np.float32), pure=True)
