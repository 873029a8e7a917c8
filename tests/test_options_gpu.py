"""The option table on an engine: options are per engine (two engines in one process do not see each other's gn_reg), every key reads
back what was stored, the three range checks keep their messages, and splitk_tiles is stored as given (per 256 CUs) whatever the device."""
import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests.test_norm_gpu import LDS_SLAB, REG_SHAPES, REGISTER

pytestmark = pytest.mark.gpu

# the on / off knobs (stored as value != 0); "vae_flash" is the one tri-state (value < 0 ? -1 : value != 0); the rest store the value
BOOL_KEYS = {"gn_single", "gn_reg", "graph", "conv_patch", "conv_patch2", "splitk_fused", "attn_legacy", "gn_fuse", "st_fuse", "two_streams",
             "cfg_share", "wide_tile", "patch_split", "patch4", "ups_fold", "big_tile", "tile192", "gemv"}
LEGAL = {"gemm_tile": 2, "gemm_splitk": 2, "patch_split_min": 2, "ln_fuse": 0, "sd3_fp8": 1, "ring": 1000}   # otherwise: default + 1


@pytest.fixture()
def eng():
    e = E.Engine(W.TINY, precision="f16")
    yield e
    e.close()


def test_gn_reg_belongs_to_one_engine(eng):
    shape = (2, 256, 8, 8)
    assert shape in REG_SHAPES
    rng = np.random.default_rng(5)
    x = rng.standard_normal(shape).astype(np.float32)
    ga, be = rng.standard_normal(shape[1]).astype(np.float32), rng.standard_normal(shape[1]).astype(np.float32)
    other = E.Engine(W.TINY, precision="f16")
    try:
        before = other.op_groupnorm(x, ga, be, 1e-5, False)
        assert other.stat("gn_kernel") == REGISTER
        eng.set_option("gn_reg", 0)
        eng.op_groupnorm(x, ga, be, 1e-5, False)
        assert eng.stat("gn_kernel") == LDS_SLAB
        after = other.op_groupnorm(x, ga, be, 1e-5, False)
        assert other.stat("gn_kernel") == REGISTER, "the other engine's GroupNorm kernel moved with this engine's option"
        assert other.option("gn_reg") == 1 and eng.option("gn_reg") == 0
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    finally:
        other.close()


def test_every_option_reads_back_what_was_stored(eng):
    table = [(k, d) for k, d in E.option_table() if k not in ("verbose", "profile")]
    assert len(table) >= 40 and BOOL_KEYS <= {k for k, _ in table}
    for key, default in table:
        assert eng.option(key) == default, key
    for key, default in table:
        if key in BOOL_KEYS:
            eng.set_option(key, 1 - default)
            assert eng.option(key) == 1 - default, key
            eng.set_option(key, 7 if default else 0)
            assert eng.option(key) == default, key
        elif key == "vae_flash":
            for v, stored in ((1, 1), (5, 1), (0, 0), (-7, -1)):
                eng.set_option(key, v)
                assert eng.option(key) == stored, (key, v)
        else:
            v = LEGAL.get(key, default + 1)
            assert v != default
            eng.set_option(key, v)
            assert eng.option(key) == v, key
    for key, bad, msg in (("gemm_tile", 5, r"option gemm_tile: -1 \(the plan's own\) or a tile 0 \.\. 4"),
                          ("gemm_splitk", 0, r"option gemm_splitk: -1 \(the plan's own\), 1 \(never\) or 2 \.\. 64 slices"),
                          ("patch_split_min", 0, r"patch_split_min must be >= 1")):
        held = eng.option(key)
        with pytest.raises(E.PdError, match=msg):
            eng.set_option(key, bad)
        assert eng.option(key) == held, key
    with pytest.raises(E.PdError, match="unknown option 'no_such_knob'"):
        eng.set_option("no_such_knob", 1)
    with pytest.raises(E.PdError, match="unknown option 'no_such_knob'"):
        eng.option("no_such_knob")


def test_splitk_tiles_is_stored_per_256_cus(eng):
    print(f"[options] ncu {eng.stat('ncu')}")
    assert eng.stat("ncu") >= 8
    assert eng.option("splitk_tiles") == 256
    rng = np.random.default_rng(9)
    x, w = rng.standard_normal((128, 1280)).astype(np.float32), rng.standard_normal((320, 1280)).astype(np.float32)
    plan = lambda: tuple(eng.stat(k) for k in ("gemm_family", "gemm_tile", "gemm_splitk"))
    y0 = eng.op_linear(x, w)
    p0 = plan()
    eng.set_option("splitk_tiles", eng.option("splitk_tiles"))
    assert eng.option("splitk_tiles") == 256
    y1 = eng.op_linear(x, w)
    assert plan() == p0
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32))
