"""The bound of tests/gemm_ref.py has teeth, and is not too tight: every mistake of gemm_ref.MUTANTS, applied to the fp64 reference itself,
exceeds it in bf16 and f16 at every shape of the GPU case list, on the input family meant for it; an independent NumPy evaluation in the
kernels' own fp32 arithmetic stays inside it on every GPU case of every mode.  No engine, no GPU.  Prints "[gemm-ref] ..." lines (pytest -s)."""
import numpy as np
import pytest

from tests import gemm_ref as R

S = R.Spec


def spec_for(mutant, B, tok, K, N):
    """the call that carries what the mistake is about, on the family built to magnify it"""
    vb = N // 2 // 4 * 4
    return {
        "gate_next_sample": S("per_sample", B, tok, K, N, gate=True, res_dt="S", out_dt="T"),
        "rowvec_next_sample": S("per_sample", B, tok, K, N, rowvec=True),
        "gate_after_residual": S("cancel", B, tok, K, N, gate=True, res_dt="T", out_dt="T"),
        "scale_after_residual": S("cancel", B, tok, K, N, scale=0.75, res_dt="T"),
        "c_row_off_dropped": S("per_sample", B, tok, K, N, gate=True, c_remap=True),
        "a_row_off_dropped": S("normal", B, tok, K, N, gate=True, a_remap=True),
        "vt_tok_off_dropped": S("normal", B, tok, K, N, out_dt="T", vt_begin=vb, vt_tok_off=R.REMAP, c_remap=True),
        "vt_token_off1": S("normal", B, tok, K, N, vt_begin=vb, vt_extra=8),
        "vt_first_group_skipped": S("normal", B, tok, K, N, out_dt="T", vt_begin=vb),
        "bias_n_plus_4": S("ragged_bias", B, tok, K, N, out_dt="T"),
        "residual_ldc": S("normal", B, tok, K, N, scale=0.75, res_dt="f32", out_dt="T", ldc_extra=28),
        "last_row_next_sample": S("per_sample", B, tok, K, N, rowvec=True, gate=True, out_dt="T"),
        "gelu_no_cubic": S("act_edges", B, tok, K, N, R.ACT_TANH, out_dt="T"),
        "truncate": S("per_sample", B, tok, K, N, rowvec=True, out_dt="T"),
    }[mutant]


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_every_mistake_exceeds_the_bound(mode):
    worst = {m: (np.inf, None) for m in R.MUTANTS}
    for B, tok, K, N in R.shapes(mode):
        for mutant in R.MUTANTS:
            spec = spec_for(mutant, B, tok, K, N)
            inp = R.make_inputs(spec, mode)
            ref, bound = R.gemm_ref(inp, spec, mode), R.gemm_bound(inp, spec, mode, splitk=4)     # the widest bound a GPU case of this shape gets
            r0, _ = R.check(ref, ref, bound)
            assert r0 == 0.0
            r, at = R.check(R.gemm_ref(inp, spec, mode, mutant), ref, bound)
            if r < worst[mutant][0]:
                worst[mutant] = (r, (B, tok, K, N))
            assert r > 1.0, f"{mode} {mutant} at {(B, tok, K, N)}: err / bound {r:.3f} -- the bound would let this mistake through"
    for mutant, (r, shp) in worst.items():
        print(f"[gemm-ref] {mode} {mutant}: smallest err / bound over the shapes {r:.3g} at (B, tokens, K, N) {shp}")


@pytest.mark.parametrize("mode", ["f32", "f16x2", "f16", "bf16"])
def test_fp32_evaluation_stays_inside(mode):
    worst = (0.0, None)
    for c in R.all_cases(mode):
        inp = R.make_inputs(c.spec, mode)
        ref, bound = R.gemm_ref(inp, c.spec, mode), R.gemm_bound(inp, c.spec, mode, splitk=c.splitk)
        r, at = R.check(R.gemm_emul(inp, c.spec, mode), ref, bound)
        assert r <= 1.0, f"{mode} {c}: the fp32 evaluation is at {r:.3f} of the bound at {at}: the model misses a term"
        if r > worst[0]:
            worst = (r, c)
    print(f"[gemm-ref] {mode} fp32 NumPy evaluation: worst err / bound {worst[0]:.3f} on {worst[1]}")


def test_case_families_do_what_they_are_for():
    for mode in ("f16", "bf16"):
        s = S("cancel", 3, 77, 200, 164, gate=True, scale=0.5, res_dt="T", out_dt="T")
        inp = R.make_inputs(s, mode)
        y, _ = R.gemm_ref(inp, s, mode)
        assert np.abs(y).max() < 2 * R.U_OUT[R.STORAGE[mode]] * np.abs(inp["residual"]).max()      # only the residual's rounding is left
        s = S("act_edges", 3, 77, 200, 320, R.ACT_TANH)
        inp = R.make_inputs(s, mode)
        z = inp["x"].astype(np.float64) @ inp["w"].astype(np.float64).T + inp["bias"]
        assert z.min() < -11 and z.max() > 11 and (np.abs(z) < 0.05).any()
        s = S("act_edges", 3, 77, 200, 320, R.ACT_GATED, out_dt="T")
        y, _ = R.gemm_ref(R.make_inputs(s, "f16"), s, "f16")
        assert (np.abs(y[1]) == R.F16_MAX).any() and np.abs(y).max() == R.F16_MAX                  # row 1 leaves the fp16 range and is saturated
        s = S("per_sample", 3, 77, 72, 164, rowvec=True, gate=True)
        inp = R.make_inputs(s, mode)
        assert np.abs(np.diff(inp["rowvec"], axis=0)).min() > 3 and np.abs(np.diff(inp["gate"], axis=0)).min() > 1


def test_stated_constants_against_the_fp32_formulas():
    """gelu_fast's erf and the three exp-based activations, evaluated in NumPy fp32 over [-13, 13], against fp64: inside ERF and act_error"""
    z = np.linspace(-13.0, 13.0, 200001).astype(np.float32)
    z8 = z.astype(np.float64)
    gf = R.gelu_fast_f32(z).astype(np.float64)
    erf_err = np.abs(gf - R.act_ref(z8, R.ACT_ERF)) / np.maximum(0.5 * np.abs(z8), 1e-30)
    print(f"[gemm-ref] gelu_fast in fp32: erf error {erf_err[np.abs(z8) > 1e-3].max():.3g} (stated 1.5e-7 + evaluation, taken {R.ERF:.3g})")
    for act in (R.ACT_SILU, R.ACT_QUICK, R.ACT_TANH, R.ACT_ERF):
        rel, ab = R.act_error(z8, act, False)
        ref = R.act_ref(z8, act)
        err = np.abs(R.act_f32(z, act).astype(np.float64) - ref)
        assert (err <= rel * np.abs(ref) + ab + 1e-300).all(), (act, float((err / (rel * np.abs(ref) + ab + 1e-300)).max()))


def test_case_list_covers_what_it_claims():
    for mode in ("f32", "f16x2", "f16", "bf16"):
        cs = R.all_cases(mode)
        ig = [c for c in cs if c.ring is None]
        assert {c.tile for c in ig} == set(R.TILES[mode])
        for t in R.TILES[mode]:
            tc = [c for c in ig if c.tile == t and c.spec.act == 0 and not c.spec.vt_begin]
            sp = [c.spec for c in tc]
            assert all(s.B == 3 and (s.tokens == 77) == (R.TILE_ROWS[t] == 128) and (s.B * s.tokens) % R.TILE_ROWS[t] for s in sp)
            assert all(s.tokens % R.TILE_ROWS[t] and s.tokens < R.TILE_ROWS[t] for s in sp)          # a tile straddles two samples
            assert {s.N for s in sp} == ({384} if t == 4 else {164, 320, 384}) and {s.K for s in sp} >= {72, 200, 320, 1280}
            assert {c.splitk for c in tc if c.spec.K == 1280} >= ({1, 4} if t < 2 else {1})
            assert any(s.rowvec and s.bias and not s.gate for s in sp)
            assert {s.res_dt for s in sp if s.scale != 1.0 and s.res_dt} == {"f32", "T", "S"}
            gated = [s for s in sp if s.gate and s.res_dt]
            if t == 3:      # no MM instantiation of the 256 x 320 tile: nothing here may ask for one
                assert not any(s.gate or s.c_remap or s.a_remap for s in sp)
            else:
                assert any(s.c_remap and s.a_remap for s in gated) and any(not s.c_remap and not s.a_remap for s in gated)
            assert {s.out_dt for s in sp} == {"f32", "T"} and {s.ldc_extra for s in sp} == {0, 28}
            assert {s.family for s in sp} >= {"normal", "per_sample", "cancel", "ragged_bias"}
        for t in R.TILES[mode]:
            vt = [c.spec for c in ig if c.spec.vt_begin and c.tile == t]
            assert {(s.N, s.vt_begin) for s in vt} == ({(384, 256), (384, 192)} if t == 4 else {(384, 256), (320, 160)}) and {s.tokens for s in vt} == {77, 64}
            assert {s.vt_extra for s in vt} == {0, 8} and {s.out_dt for s in vt} == {"f32", "T"} and all(s.vt_begin % 4 == 0 for s in vt)
            assert {s.vt_tok_off for s in vt} == ({0} if t == 3 else {0, R.REMAP}) and all(bool(s.vt_tok_off) == s.c_remap for s in vt)
        acts = {(c.spec.act, c.tile) for c in ig if c.spec.family == "act_edges"}
        assert {a for a, _ in acts} == {R.ACT_SILU, R.ACT_QUICK, R.ACT_TANH, R.ACT_ERF, R.ACT_RELU, R.ACT_GATED}
        assert {(R.ACT_RELU, 0), (R.ACT_RELU, 1), (R.ACT_GATED, 0), (R.ACT_GATED, 1)} <= acts
        assert {c.spec.out_dt for c in ig if c.spec.act == R.ACT_TANH} == {"f32", "T"}
        rg = [c for c in cs if c.ring is not None]
        if R.STORAGE[mode] == "f32":
            assert not rg
            continue
        assert {c.ring for c in rg} == {(0, 0), (0, 1), (1, 0), (1, 1), (4, 1)}
        assert {c.spec.K for c in rg} == {128, 320, 2560} and {c.spec.N for c in rg} == {164, 320} and {c.spec.B * c.spec.tokens for c in rg} == {231, 300}
        assert {R.ring_launched(c) for c in rg} == {0, 1, 2, 3, 4} and {c.spec.ldc_extra for c in rg} == {0, 28}      # both ping-pong forms really run
        for t in range(5):
            at = [c.spec for c in rg if R.ring_launched(c) == t]
            assert any(s.res_dt for s in at) and any(s.vt_begin for s in at) and any(s.act for s in at)
        assert any(c.spec.res_dt for c in rg) and any(c.spec.vt_begin for c in rg) and {c.spec.act for c in rg} == {0, R.ACT_SILU, R.ACT_QUICK}
        assert all(c.spec.out_dt == "T" and not c.spec.rowvec and not c.spec.gate for c in rg)
