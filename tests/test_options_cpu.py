"""The engine's option table (csrc/options.h) from the host: pd_option_info walks it without an engine, so the key set, the defaults
and the documentation can be checked without a GPU.  The literal list below is the option list of the strcmp chain the table replaced:
a dropped, renamed or re-defaulted key fails here.  Tile-count defaults are the numbers for a 256-CU part (splitk_tiles 256)."""
import ctypes as C
import os
import re

import pytest

from prompt_diffusion_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prompt-diffusion_amd", "csrc")

DEFAULTS = {
    "verbose": 0, "profile": 0, "gn_single": 1, "gn_reg": 1, "graph": 0, "conv_patch": 1, "conv_patch2": 1, "conv_patch2_tiles": 768,
    "splitk_fused": 0, "splitk_big": 0, "splitk_max": 16, "splitk_tiles": 256, "attn_legacy": 0, "gn_fuse": 0, "ln_fuse": -1, "st_fuse": 1,
    "two_streams": 1, "cfg_share": 1, "wide_tile": 1, "slab_gn": 1, "ring": 80, "ring_tile": -1, "ring_geglu": 1, "ring_small": 4,
    "short_k": 20, "patch_split": 1, "gemm_tile": -1, "gemm_splitk": -1, "ring_pp": 1, "patch4": 1, "patch_split_fill": 256,
    "patch_split_min": 4, "patch_split_tiles": 64, "ups_fold": 1, "vae_flash": -1, "ups_fold_tiles": -1, "dense_tiles": 128, "dense_k": 40,
    "big_tile": 1, "tile192": 1, "gemv": 1, "sd3_fp8": 0,
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


def test_table_is_the_option_list(lib):
    rows = E.option_table()
    keys = [k for k, _ in rows]
    assert len(keys) == len(set(keys)), "duplicate key"
    assert set(keys) == set(DEFAULTS)
    assert dict(rows) == DEFAULTS
    # past the end: non-zero, outputs untouched; a negative index likewise
    k, d = C.c_char_p(b"x"), C.c_int64(7)
    assert lib.pd_option_info(len(rows), C.byref(k), C.byref(d)) != 0 and lib.pd_option_info(-1, C.byref(k), C.byref(d)) != 0
    assert k.value == b"x" and d.value == 7
    assert "pd_get_option" in E.EXPORTS and "pd_option_info" in E.EXPORTS and lib.pd_abi_version() == 2


def test_every_key_is_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    end = hdr.index("int pd_set_option(")
    comment = hdr[hdr.rindex("/*", 0, end):end]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key, default in E.option_table():
        assert f'"{key}"' in comment, f"{key}: not in the pd_set_option comment of include/pdengine.h"
        assert f'"{key}"' in integ, f"{key}: not in INTEGRATION.md"
        # INTEGRATION.md's list is a table: the row of a key carries its default
        assert re.search(rf'^\| `"{key}"` \| {default} \|', integ, flags=re.M), f"{key}: INTEGRATION.md row without the default {default}"
    # ... and the comment's list (from "verbose" on, after the introduction) names them in the table's order
    start = comment.index('"verbose"')
    at = [comment.index(f'"{k}"', start) for k, _ in E.option_table()]
    assert at == sorted(at)


def test_null_engine_is_refused(lib):
    v = C.c_int64(0)
    assert lib.pd_set_option(None, b"ring", 1) != 0 and lib.pd_last_error() == b"null argument"
    assert lib.pd_get_option(None, b"ring", C.byref(v)) != 0 and lib.pd_last_error() == b"null argument"
    assert lib.pd_get_stat(None, b"ncu") == -1


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".hip", ".h")) or f == "Makefile":
            yield f, open(os.path.join(CSRC, f)).read()


def test_no_scattered_or_process_wide_option_state():
    """The options are pd_engine::opt and nothing else: no opt_ fields, no GroupNorm global, no CU-count static in the ring launcher;
    plan_gemm reads the CU count through ChipFill only."""
    for f, src in _sources():
        for word in ("opt_", "g_gn_reg", "ncu_of", "device_ncu"):
            assert word not in src, f"{word} in csrc/{f}"
    eng = open(os.path.join(CSRC, "engine.cpp")).read()
    body = eng[eng.index("GemmPlan pd_engine::plan_gemm("):]
    body = body[:body.index("\n}\n")]
    assert len(body) > 3000 and "fill.whole" in body
    assert not re.search(r"\bncu\b", body), "plan_gemm does CU arithmetic of its own"
    ses = open(os.path.join(CSRC, "session.cpp")).read()
    for fn in ("pd_set_option", "pd_get_option", "pd_option_info", "pd_get_stat", "pd_profile_read", "pd_profile_dump"):
        assert fn + "(" not in ses, f"{fn} belongs to options.cpp"
