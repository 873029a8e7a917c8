"""SD3 text encoders on the engine (CLIP-L, CLIP-G: text.cpp; T5: sd3_text.cpp) against tests/golden/sd3_text.npz -- computed by transformers itself,
tests/golden/make_golden_sd3_text.py -- and, at the T5 lengths the fixture does not hold, against the NumPy restatement that the CPU suite
pins to the same fixture (tests/sd3_text_ref.py).  Nothing here imports transformers.  Configuration: sd3.SD3_TINY_TEXT (why its T5 width
is 384: tests/test_sd3_text_cpu.py).

Bounds, max |got - ref| / max |ref| per tensor against the fp32 references:
  f32     1e-4: the bound tests/test_text_gpu.py holds the same GEMM and attention arithmetic to over 12 blocks.
  f16x2 / f16 / bf16: twice the largest value measured over every comparison of this file on an MI355X (these stacks are 2-4 blocks deep
          and box-to-box rounding differs little; f32 itself measured 8.2e-7); measured -> bound:
            f16x2  2.13e-6 (t5)                           -> 4.3e-6
            f16    1.08e-3 (clip_g hidden, skip 1)        -> 2.2e-3
            bf16   9.97e-3 (clip_l pooled at a moved EOS) -> 2.0e-2
"""
import ctypes as C

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as Pipe
from tests import sd3_text_ref as R

pytestmark = pytest.mark.gpu

TCFG = sd3.SD3_TINY_TEXT
NOT5 = sd3.SD3TextConfig(clip_l=TCFG.clip_l, clip_g=TCFG.clip_g, t5=None, joint_dim=TCFG.joint_dim)
NET = sd3.SD3Config(in_channels=4, out_channels=4, heads=2, head_dim=64, layers=2, cn_layers=1, joint_dim=TCFG.joint_dim,
                    pooled_dim=TCFG.pooled_dim, pos_embed_max_size=12, cn_pos_embed_max_size=10)
BOUND = {"f32": 1e-4, "f16x2": 4.3e-6, "f16": 2.2e-3, "bf16": 2.0e-2}
PRECS = ["f32", "f16x2", "f16", "bf16"]


def check(tag, got, ref, prec):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"[sd3_text] {prec:5s} {tag}: {err:.3e} (bound {BOUND[prec]:g})")
    assert err < BOUND[prec], (tag, prec, err)


@pytest.fixture(scope="module")
def gold():
    import os
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "sd3_text.npz")))


@pytest.fixture(scope="module")
def sd(gold):
    return sd3.synth_sd3_text_state_dict(TCFG, int(gold["seed"]))


@pytest.fixture(scope="module", params=PRECS)
def eng(request, sd):
    e = sd3.SD3Engine(NET, precision=request.param)
    e.configure_text(TCFG)
    e.load_state_dict(sd, strict=False)
    assert e.text_weights_missing() == 0
    e.prec = request.param
    yield e
    e.close()


@pytest.fixture(scope="module")
def t5_cases(sd):
    """ids and the NumPy reference for the T5 lengths of test 2, computed once: 20 (one ragged key tile, no multiple of 8), 136 (two query
    blocks, three key tiles with the last ragged, distances >= 128 in the saturated bucket), 256 (the default: whole tiles)."""
    out = {}
    for Lt in (20, 136, 256):
        ids = np.random.default_rng(Lt).integers(0, TCFG.t5.vocab, (2, Lt)).astype(np.int32)
        out[Lt] = (ids, R.t5_forward(sd, TCFG.t5, ids))
    return out


# 1 ---------------------------------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("skip", [0, 1])
def test_encoders_and_assembly_match_the_fixture(eng, gold, skip):
    rows = gold["clip_rows"]
    for tag, ids in (("l", gold["ids_l"]), ("g", gold["ids_g"])):
        hid, pooled = eng.text_encoder("clip_" + tag, ids, clip_skip=skip)
        check(f"clip_{tag} hidden skip{skip}", hid[:, rows], gold[f"hidden_{tag}_skip{skip}"], eng.prec)
        check(f"clip_{tag} pooled", pooled, gold[f"pooled_{tag}"], eng.prec)          # both EOS rules: l argmax, g first match
    check("t5", eng.text_encoder("t5", gold["ids_t5"]), gold["t5"], eng.prec)
    pe, pooled = eng.encode_prompt_ids(gold["ids_l"], gold["ids_g"], gold["ids_t5"], clip_skip=skip or None)
    assert pe.shape == (3, 77 + 20, TCFG.joint_dim) and pooled.shape == (3, TCFG.pooled_dim)
    check(f"prompt_embeds skip{skip}", pe[:, gold["pe_rows"]], gold[f"prompt_embeds_skip{skip}"], eng.prec)
    check("pooled", pooled, gold["pooled"], eng.prec)


# 2 ---------------------------------------------------------------------------------------------------- T5 lengths
@pytest.mark.parametrize("Lt", [20, 136, 256])
def test_t5_lengths(eng, t5_cases, Lt):
    ids, ref = t5_cases[Lt]
    got = eng.text_encoder("t5", ids)
    check(f"t5 Lt={Lt}", got, ref, eng.prec)
    if Lt == 136:   # bias indexing that leaked across samples or heads would not commute with a batch permutation
        assert np.array_equal(eng.text_encoder("t5", ids[::-1].copy()), got[::-1])


def test_t5_gated_product_beyond_the_fp16_range(sd):
    """T5-XXL's feed-forward is known to leave the fp16 range.  With wi_0 / wi_1 scaled until gelu_new(wi_0 x) * wi_1 x passes 65504 (a
    quarter of the products do) the fp16 engine must saturate on store, not write inf: the residual stream is fp32, so everything after
    stays finite.  (Finite is all that is claimed: whether f16 is USABLE with real T5-XXL weights is unmeasured)"""
    prec = "f16"
    big = {k: (v * np.float32(400.0) if "DenseReluDense.wi_" in k else v * np.float32(1e-4) if k.endswith("DenseReluDense.wo.weight") else v)
           for k, v in sd.items()}
    ids = np.random.default_rng(11).integers(0, TCFG.t5.vocab, (2, 24)).astype(np.int32)
    W = lambda n: np.asarray(big["text_encoder_3.encoder.block.0." + n], np.float64)
    x = np.asarray(big["text_encoder_3.shared.weight"], np.float64)[ids]
    ref = R.t5_forward(big, TCFG.t5, ids)
    e = sd3.SD3Engine(NET, precision=prec)
    try:
        e.configure_text(TCFG)
        e.load_state_dict(big, strict=False)
        got = e.text_encoder("t5", ids)
        assert got.shape == ref.shape and np.isfinite(got).all()
    finally:
        e.close()
    # the premise: the reference's own gated product does exceed the fp16 range with these weights
    h = x + 0.0   # (block 0's attention adds O(1); the product's size comes from the 400 x 400 scaling)
    h = W("layer.1.layer_norm.weight") * (h / np.sqrt((h * h).mean(-1, keepdims=True) + TCFG.t5.eps))
    prod = R._act(h @ W("layer.1.DenseReluDense.wi_0.weight").T, "gelu_new") * (h @ W("layer.1.DenseReluDense.wi_1.weight").T)
    assert np.abs(prod).max() > 65504.0


# 3 ---------------------------------------------------------------------------------------------------- assembly
def test_assembly_layout(eng, gold):
    ids_l, ids_g, ids_t5 = gold["ids_l"], gold["ids_g"], gold["ids_t5"]
    pe, pooled = eng.encode_prompt_ids(ids_l, ids_g, ids_t5)
    cl, cg = TCFG.clip_l.hidden, TCFG.clip_g.hidden
    assert np.all(pe[:, :77, cl + cg:] == 0.0)                                   # the pad columns ...
    assert np.all(pe[:, :77, :cl + cg] != 0.0) and np.all(pe[:, 77:] != 0.0)     # ... and nothing else
    hl, pl = eng.text_encoder("clip_l", ids_l)
    hg, pg = eng.text_encoder("clip_g", ids_g)
    assert np.array_equal(pe[:, :77, :cl], hl) and np.array_equal(pe[:, :77, cl:cl + cg], hg)
    assert np.array_equal(pe[:, 77:], eng.text_encoder("t5", ids_t5))
    assert np.array_equal(pooled, np.concatenate([pl, pg], 1))


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_without_t5_the_output_is_77_rows(prec, sd, gold):
    e = sd3.SD3Engine(NET, precision=prec)
    try:
        e.configure_text(NOT5)
        e.load_state_dict(sd, strict=False)     # text_encoder_3.* tensors are not this engine's: skipped
        assert e.text_weights_missing() == 0
        pe, pooled = e.encode_prompt_ids(gold["ids_l"], gold["ids_g"])
        assert pe.shape == (3, 77, TCFG.joint_dim) and pooled.shape == (3, TCFG.pooled_dim)
        ref, refp = R.encode_prompt(sd, NOT5, gold["ids_l"], gold["ids_g"])
        check("prompt_embeds without T5", pe, ref, prec)
        check("pooled without T5", pooled, refp, prec)
        assert e.encode_prompt_ids(gold["ids_l"], gold["ids_g"], zero_t5_rows=True)[0].shape == (3, 154, TCFG.joint_dim)
    finally:
        e.close()


# 4 ---------------------------------------------------------------------------------------------------- pooling
def test_pooled_row_follows_the_eos_token(eng, sd):
    rng = np.random.default_rng(3)
    for which, c, prefix in (("clip_l", TCFG.clip_l, "text_encoder."), ("clip_g", TCFG.clip_g, "text_encoder_2.")):
        eos = c.vocab - 1 if c.eos_token_id == 2 else c.eos_token_id
        body = rng.integers(8, c.vocab - 2, 76).astype(np.int32)
        def row(p, tail):   # BOS, body, EOS at position p, then `tail`
            r = np.concatenate([[c.vocab - 2], body[:p - 1], [eos], tail[:76 - p]]).astype(np.int32)
            assert r.shape == (77,)
            return r
        pad = np.full(76, eos, np.int32)
        junk = rng.integers(8, c.vocab - 2, 76).astype(np.int32)     # never the EOS value, never larger than it
        late = junk.copy()
        late[20] = eos                                               # a second EOS further on: not the first match, not a larger id
        ids = np.stack([row(9, pad), row(9, junk), row(9, late), row(30, pad)])
        _, pooled = eng.text_encoder(which, ids)
        # what follows the first EOS cannot reach its row (causal) nor move the choice of row: bit-identical
        assert np.array_equal(pooled[0], pooled[1]) and np.array_equal(pooled[0], pooled[2])
        assert not np.array_equal(pooled[0], pooled[3])              # moving the EOS moves the row
        assert R.eos_positions(ids, c.eos_token_id).tolist() == [9, 9, 9, 30]
        check(f"{which} pooled at moved EOS", pooled, R.clip_forward(sd, c, prefix, ids)[1], eng.prec)


# 4b --------------------------------------------------------------------------------------------------- where the stack stops
@pytest.fixture(scope="module")
def clip_refs(sd, gold):
    """(hidden_states, text_embeds) of the NumPy restatement for the fixture's CLIP ids, computed once."""
    return {which: R.clip_forward(sd, c, prefix, gold[key])
            for which, c, prefix, key in (("clip_l", TCFG.clip_l, "text_encoder.", "ids_l"), ("clip_g", TCFG.clip_g, "text_encoder_2.", "ids_g"))}


def test_capture_before_any_block(eng, gold, clip_refs):
    """clip_skip = layers - 1 asks for hidden_states[0]: the token + position embeddings, written before any block has run, while the
    pooled output still takes the whole stack and so does not depend on clip_skip."""
    for which, c, key in (("clip_l", TCFG.clip_l, "ids_l"), ("clip_g", TCFG.clip_g, "ids_g")):
        hs, pooled_ref = clip_refs[which]
        hid, pooled = eng.text_encoder(which, gold[key], clip_skip=c.layers - 1)
        check(f"{which} embeddings (skip {c.layers - 1})", hid, hs[0], eng.prec)
        check(f"{which} pooled (skip {c.layers - 1})", pooled, pooled_ref, eng.prec)
        assert np.array_equal(pooled, eng.text_encoder(which, gold[key], clip_skip=0)[1])


def test_one_output_only(eng, gold, clip_refs):
    """pd_sd3_text_encoder with pooled = NULL or hidden = NULL (the Python wrapper always asks for both): each output is the same bits as
    in the two-output call, and without the pooled output the stack stops at the capture layer, so fewer kernels are launched."""
    c, skip, base = TCFG.clip_l, 1, eng.base
    ids = np.ascontiguousarray(gold["ids_l"][:2], np.int32)

    def call(want_hidden, want_pooled):
        hid, po = np.zeros((2, 77, c.hidden), np.float32), np.zeros((2, c.proj_dim), np.float32)
        n0 = base.stat("launches")
        base._check(base.lib.pd_sd3_text_encoder(base._h, 0, ids.ctypes.data, 2, 77, skip, E.PD_MEM_HOST,
                                                 hid.ctypes.data if want_hidden else None, po.ctypes.data if want_pooled else None))
        return hid, po, base.stat("launches") - n0

    hid, po, n_both = call(True, True)
    hs, pooled_ref = clip_refs["clip_l"]
    check("clip_l hidden skip1, batch 2", hid, hs[-(skip + 2)][:2], eng.prec)
    check("clip_l pooled, batch 2", po, pooled_ref[:2], eng.prec)
    hid_only, untouched, n_hidden = call(True, False)
    assert np.array_equal(hid_only, hid) and not untouched.any()
    untouched, po_only, n_pooled = call(False, True)
    assert np.array_equal(po_only, po) and not untouched.any()
    print(f"[sd3_text] launches: both {n_both}, hidden only {n_hidden}, pooled only {n_pooled}")
    assert 0 < n_hidden < n_both and 0 < n_pooled <= n_both


# 5 ---------------------------------------------------------------------------------------------------- causality
def test_clip_is_causal_and_t5_is_not(eng, gold):
    for which, ids in (("clip_l", gold["ids_l"]), ("clip_g", gold["ids_g"])):
        other = ids.copy()
        other[:, 40:] = (other[:, 40:] + 5) % 90 + 8
        a, b = eng.text_encoder(which, ids)[0], eng.text_encoder(which, other)[0]
        assert np.array_equal(a[:, :40], b[:, :40]) and not np.array_equal(a[:, 40:], b[:, 40:])
    ids = np.random.default_rng(1).integers(0, TCFG.t5.vocab, (2, 64)).astype(np.int32)
    other = ids.copy()
    other[:, 40:] = (other[:, 40:] + 5) % TCFG.t5.vocab
    a, b = eng.text_encoder("t5", ids), eng.text_encoder("t5", other)
    assert not np.array_equal(a[:, 0], b[:, 0])                      # bidirectional: row 0 sees the change


# 6 ---------------------------------------------------------------------------------------------------- an engine that never configures text
def test_unconfigured_engine_is_unchanged(sd):
    net_sd = sd3.synth_sd3_state_dict(NET)
    plain, full = sd3.SD3Engine(NET, precision="f16"), sd3.SD3Engine(NET, precision="f16")
    try:
        full.configure_text(TCFG)
        plain.load_state_dict(net_sd)
        full.load_state_dict({**net_sd, **sd})
        names, fnames = plain.base.param_names(), full.base.param_names()
        assert not any(n.startswith("text_encoder") for n, _ in names)
        assert names == [x for x in fnames if not x[0].startswith("text_encoder")]
        assert sum(n.startswith("text_encoder") for n, _ in fnames) == len(sd3.sd3_text_spec(TCFG))
        # the C entry point itself refuses, with a message
        ids = np.zeros((1, 77), np.int32)
        a = sd3.pd_sd3_text_args()
        a.batch, a.t5_len, a.clip_skip, a.mem = 1, 0, 0, E.PD_MEM_HOST
        a.ids_clip_l = a.ids_clip_g = ids.ctypes.data
        pe, po = np.zeros((1, 77, NET.joint_dim), np.float32), np.zeros((1, NET.pooled_dim), np.float32)
        assert plain.base.lib.pd_sd3_encode_prompt(plain.base._h, C.byref(a), pe.ctypes.data, po.ctypes.data) != 0
        assert "pd_sd3_text_configure" in plain.base.lib.pd_last_error().decode()
        with pytest.raises(E.PdError, match="configure_text"):
            plain.encode_prompt_ids(ids, ids)
        rng = np.random.default_rng(0)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        x, ctx, pooled, t = f(2, 4, 8, 8), f(2, 7, NET.joint_dim), f(2, NET.pooled_dim), np.array([500.0, 20.0], np.float32)
        cond, pair = f(2, 4, 8, 8), f(2, 4, 8, 8)
        assert np.array_equal(plain.forward(x, t, ctx, pooled, cond, pair), full.forward(x, t, ctx, pooled, cond, pair))
    finally:
        plain.close()
        full.close()


# 7 ---------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_from_prompt_strings_equals_prompt_embeds(sd):
    e = sd3.SD3Engine(NET, precision="f16")
    try:
        e.configure_text(TCFG)
        e.load_state_dict({**sd3.synth_sd3_state_dict(NET), **sd})
        assert e.weights_missing() == 0

        def tok(vocab, eos):
            def f(texts, max_length):
                out = np.full((len(texts), max_length), eos, np.int32)
                for i, t in enumerate(texts):
                    w = [8 + (sum(map(ord, x)) % (vocab - 12)) for x in t.split()][:max_length - 2]
                    out[i, 0] = vocab - 2
                    out[i, 1:1 + len(w)] = w
                return out
            return f
        toks = (tok(100, 99), tok(100, TCFG.clip_g.eos_token_id), tok(100, 1))
        prompts, neg = ["a red house", "two cats on a mat"], ["blurry", ""]
        lat = np.random.default_rng(5).standard_normal((2, 4, 8, 8)).astype(np.float32)
        kw = dict(control_image=lat * 0.5, control_image_pair=lat * 0.25, latents=lat, num_inference_steps=2, guidance_scale=5.0,
                  output_type="latent", max_sequence_length=24)
        got = Pipe(e, tokenizers=toks)(prompt=prompts, negative_prompt=neg, clip_skip=1, **kw)["images"]
        pe, ppe = e.encode_prompt_ids(toks[0](prompts, 77), toks[1](prompts, 77), toks[2](prompts, 24), clip_skip=1)
        npe, nppe = e.encode_prompt_ids(toks[0](neg, 77), toks[1](neg, 77), toks[2](neg, 24))
        want = Pipe(e)(prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=nppe, **kw)["images"]
        assert pe.shape == (2, 77 + 24, NET.joint_dim) and np.isfinite(got).all()
        assert np.array_equal(got, want)
    finally:
        e.close()
