"""Context lengths other than 77 at the block level: pd_op_spatial_transformer_ctx on the SD1.5 input_blocks.1.1. block (C = 320,
8 heads x 40) with synthetic weights, against oracle.spatial_transformer on a [B, L, 768] context.

In the 2-byte modes the 320-channel block takes the fused tail (csrc/st_tail.hip) for L <= 288: one, two or three 96-key windows with
an online softmax across them; L = 289 and token counts that are no multiple of 128 take the per-layer path.  L: 1; 77; 96 | 97 (the
window boundary); 154 and 192 (two windows, the second partly / completely full); 231 (three windows: the reference's long prompts);
288 (three full windows); 289 (per-layer).  Tolerances are tests/test_st_tail_gpu.py's (max-abs / max-abs of the block output)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W

pytestmark = pytest.mark.gpu
PRE = "model.diffusion_model."
BLK = "input_blocks.1.1."
TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 5e-3, "bf16": 4e-2}
LENGTHS = [1, 77, 96, 97, 154, 192, 231, 288, 289]
SHAPES = [(2, 16, 16), (1, 8, 48), (3, 8, 8)]   # two workgroups per sample; one sample of 384 tokens; 64 tokens: per-layer path


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def sd():
    return {n: W.synth_tensor(n, s, k) for n, s, k in W.param_spec(W.SD15) if n.startswith(PRE + BLK)}


@pytest.fixture(scope="module")
def engines(sd):
    made = {}

    def get(prec):
        if prec not in made:
            e = E.Engine(W.SD15, precision=prec)
            for n, a in sd.items():
                e.load_tensor(n, a)
            made[prec] = e
        return made[prec]
    yield get
    for e in made.values():
        e.close()


_cache = {}


def case(sd, B, H, Wd, L, boost=None):
    """inputs and the oracle's output, computed once per case and shared by the modes"""
    key = (B, H, Wd, L, boost)
    if key not in _cache:
        r = np.random.default_rng(1000 * L + 10 * H + B)
        x = r.standard_normal((B, 320, H, Wd), dtype=np.float32)
        ctx = r.standard_normal((B, L, 768), dtype=np.float32)
        if boost is not None:
            ctx[:, boost] *= 12.0    # this row's key dominates the softmax of most queries
        ref = O.spatial_transformer(O.Net(sd, PRE), BLK, x, ctx, heads=8)
        assert np.isfinite(ref).all()
        x.setflags(write=False); ctx.setflags(write=False); ref.setflags(write=False)
        _cache[key] = (x, ctx, ref)
    return _cache[key]


def run_counted(e, x, ctx):
    n0 = e.stat("launches")
    y = e.op_spatial_transformer(PRE + BLK, x, ctx)
    return y, e.stat("launches") - n0


@pytest.mark.parametrize("prec", ["f32", "f16x2", "f16", "bf16"])
@pytest.mark.parametrize("B,H,Wd", SHAPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_block_matches_oracle(engines, sd, prec, B, H, Wd, L):
    x, ctx, ref = case(sd, B, H, Wd, L)
    y = engines(prec).op_spatial_transformer(PRE + BLK, x, ctx)
    err = relerr(y, ref)
    print(f"L {L} {B}x{H}x{Wd} {prec}: relerr {err:.3e} (bound {TOL[prec]:g})")
    assert np.isfinite(y).all()
    assert err < TOL[prec], (prec, L, err)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("B,H,Wd", SHAPES[:2])
@pytest.mark.parametrize("L", LENGTHS)
def test_fused_against_per_layer_path(engines, sd, prec, B, H, Wd, L):
    """option st_fuse on / off on one engine: within the mode's bound of each other; by launch count, L <= 288 took the fused tail
    (12 launches became 5) and 289 did not"""
    x, ctx, ref = case(sd, B, H, Wd, L)
    e = engines(prec)
    y1, n_on = run_counted(e, x, ctx)
    e.set_option("st_fuse", 0)
    try:
        y0, n_off = run_counted(e, x, ctx)
    finally:
        e.set_option("st_fuse", 1)
    err = relerr(y1, y0)
    print(f"L {L} {B}x{H}x{Wd} {prec}: launches {n_on} / {n_off}, fused vs per-layer {err:.3e}")
    if L <= 288:
        assert n_on < n_off - 6, (L, n_on, n_off)
    else:
        assert n_on == n_off, (L, n_on, n_off)
    assert err < TOL[prec], (prec, L, err)
    assert relerr(y0, ref) < TOL[prec]


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("L,boost", [(231, 5), (231, 229), (154, 3), (154, 150)])
def test_dominant_key_in_first_and_last_window(engines, sd, prec, L, boost):
    """online softmax: a key that dominates sits in window 0 (later windows add almost nothing) or in the last window (everything
    accumulated before it is rescaled towards zero).  case() checks that the oracle itself is finite for these inputs."""
    x, ctx, ref = case(sd, 2, 16, 16, L, boost)
    y = engines(prec).op_spatial_transformer(PRE + BLK, x, ctx)
    err = relerr(y, ref)
    print(f"L {L} boost {boost} {prec}: relerr {err:.3e}")
    assert np.isfinite(y).all()
    assert err < TOL[prec], (prec, L, boost, err)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
def test_context_77_through_new_export_is_bit_identical_to_old(engines, sd, prec):
    """pd_op_spatial_transformer is now a call of pd_op_spatial_transformer_ctx with L = cfg.context_len, so this pins the wrapper's
    argument, not the kernel.  That L <= 96 computes what it did before rests on the NW = 1 instantiation compiling to the parent's
    instructions ("Long prompts") and on tests/test_st_tail_gpu.py and the golden trajectories, which are untouched."""
    x, ctx, _ = case(sd, 2, 16, 16, 77)
    e = engines(prec)
    y_new = e.op_spatial_transformer(PRE + BLK, x, ctx)
    y_old = np.empty_like(y_new)
    xa, ca = np.ascontiguousarray(x), np.ascontiguousarray(ctx)
    e._check(e.lib.pd_op_spatial_transformer(e._h, (PRE + BLK).encode(), xa.ctypes.data, ca.ctypes.data, 2, 16, 16, y_old.ctypes.data))
    np.testing.assert_array_equal(y_new, y_old)


def test_bad_context_length_is_refused(engines, sd):
    e = engines("f16")
    x, ctx, _ = case(sd, 2, 16, 16, 77)
    y = np.empty_like(x)
    for L in (0, -3, E.PD_MAX_CONTEXT_LEN + 1):
        rc = e.lib.pd_op_spatial_transformer_ctx(e._h, (PRE + BLK).encode(), np.ascontiguousarray(x).ctypes.data,
                                                 np.ascontiguousarray(ctx).ctypes.data, 2, 16, 16, L, y.ctypes.data)
        assert rc != 0 and str(L) in e.lib.pd_last_error().decode()
