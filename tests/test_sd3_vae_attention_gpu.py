"""The first stage's single-head attention on the flash kernel (vae_attention.hip, pd_op_vae_attention with option vae_flash 1)
against an fp64 NumPy softmax on inputs rounded to the compute type, next to the materialised three-launch path (vae_flash 0).

Bound: ATTN_TOL of tests/test_kernels_gpu.py (max |diff| / max |ref|: f16 2.5e-3, bf16 2e-2), 1.5x for the two adversarial inputs
like test_attention_peaked_softmax.  The materialised path meets the same bound on every input here (measured on an MI355X, flash /
materialised: f16 2.5e-4 .. 3.9e-4 / 3.6e-4 .. 5.1e-4, bf16 2.0e-3 .. 3.3e-3 / 3.1e-3 .. 5.1e-3), so no wider bound is in use.  Flash
and materialised outputs may differ by the sum of their two bounds."""
import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests.test_kernels_gpu import ATTN_TOL, relerr, round_like

pytestmark = pytest.mark.gpu

SHAPES = [(1, 40, 512),      # less than one 48-query block, one ragged key tile
          (1, 64, 512),
          (2, 240, 512),     # ragged last key tile (240 = 7.5 x 32), ragged last query block (240 = 5 x 48), batch stride
          (1, 1088, 512),    # 34 key tiles of 32 (17 of 64)
          (2, 240, 128)]     # the small instantiation: 64-query blocks


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng(request):
    e = E.Engine(W.TINY, precision=request.param)
    e.prec = request.param
    yield e
    e.close()


def attn_ref(q, k, v):
    """fp64 softmax(q k^T C^-0.5) v, one head over all channels."""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    s = np.einsum("bnc,bmc->bnm", q, k) * q.shape[-1] ** -0.5
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bnm,bmc->bnc", p, v)


def both_paths(eng, q, k, v):
    eng.set_option("vae_flash", 1)
    n0 = eng.stat("vae_flash_launches")
    fl = eng.op_vae_attention(q, k, v)
    assert eng.stat("vae_flash_launches") == n0 + 1        # one launch for the whole batch, and it was the flash kernel
    eng.set_option("vae_flash", 0)
    ma = eng.op_vae_attention(q, k, v)
    assert eng.stat("vae_flash_launches") == n0 + 1
    eng.set_option("vae_flash", -1)
    return fl, ma


def check(eng, q, k, v, factor, what):
    q, k, v = (round_like(a, eng.prec) for a in (q, k, v))
    ref = attn_ref(q, k, v)
    fl, ma = both_paths(eng, q, k, v)
    assert np.isfinite(fl).all() and np.isfinite(ma).all()
    tol = factor * ATTN_TOL[eng.prec]
    e_fl, e_ma = relerr(fl, ref), relerr(ma, ref)
    print(f"{what} {eng.prec}: flash {e_fl:.3e}, materialised {e_ma:.3e} (bound {tol:.3e})")
    assert e_fl < tol and e_ma < tol
    assert float(np.abs(fl - ma).max() / np.abs(ref).max()) < 2 * tol


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flash_matches_fp64(eng, shape):
    g = np.random.default_rng(sum(shape))
    q, k, v = (g.standard_normal(shape, dtype=np.float32) for _ in range(3))
    check(eng, q, k, v, 1.0, str(shape))


def test_flash_peaked(eng):
    """Logits scaled so that one key dominates each row: every key is a scaled copy of one query, whose logit |q|^2 * 0.35 / sqrt(C) is
    about 7.9 against N(0, 0.35^2) for the others -- some 0.9 of the row's mass on one key, the rest spread over 239.  Measured: f16
    flash 2.5e-4 / materialised 4.3e-4, bf16 2.0e-3 / 3.3e-3."""
    g = np.random.default_rng(11)
    B, N, C = 1, 240, 512
    q, k, v = (g.standard_normal((B, N, C), dtype=np.float32) for _ in range(3))
    k[0] = q[0, g.permutation(N)] * 0.35
    check(eng, q, k, v, 1.5, "peaked")


def test_flash_max_in_last_tile(eng):
    """Keys ordered so that the largest logit of every row falls in the LAST (ragged) key tile: every earlier tile's running sum and
    accumulator are rescaled by a tiny factor when it arrives.  Measured: f16 flash 3.4e-4 / materialised 5.1e-4, bf16 2.3e-3 / 5.1e-3."""
    g = np.random.default_rng(12)
    B, N, C = 1, 240, 512
    q, k, v = (g.standard_normal((B, N, C), dtype=np.float32) for _ in range(3))
    # all queries share the component u, and only the last tile's keys (tile 7 holds keys 224..239) have one along it: their logits sit
    # near 2 |u|^2 / sqrt(C) = 11.3, everybody else's are N(0, ~1.2)
    u = 0.5 * np.sign(g.standard_normal(C)).astype(np.float32)
    q[0] += u
    k[0, 224:] += 2.0 * u
    s = round_like(q, eng.prec).astype(np.float64)[0] @ round_like(k, eng.prec).astype(np.float64)[0].T
    assert (s.argmax(1) >= 224).all()
    check(eng, q, k, v, 1.5, "max in last tile")


def test_flash_refuses_what_it_does_not_build():
    """A missing kernel is an error, not a fall-back: fp32 storage, and a channel count without an instantiation."""
    x = np.zeros((1, 16, 64), np.float32)
    e = E.Engine(W.TINY, precision="f16")
    e.set_option("vae_flash", 1)
    with pytest.raises(E.PdError):
        e.op_vae_attention(x, x, x)                      # C = 64
    e.close()
    e = E.Engine(W.TINY, precision="f32")
    e.set_option("vae_flash", 1)
    y = np.zeros((1, 16, 128), np.float32)
    with pytest.raises(E.PdError):
        e.op_vae_attention(y, y, y)
    e.set_option("vae_flash", 0)
    assert np.isfinite(e.op_vae_attention(y, y, y)).all()   # the materialised path takes every mode
    e.close()
