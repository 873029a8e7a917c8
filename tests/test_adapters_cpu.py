"""Adapter parsing (lora.parse_adapters / parse_sd3_adapters), the alpha / dim rules, the host folds, the declared symbols, the SD3
pipeline's bookkeeping on a stub engine, and the error budget of tests/adapter_ref.py against an fp32 emulation of the merge.  No GPU."""
import os
import re

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import lora as L
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as SD3Pipe
from tests import adapter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, T = W.UNET_PREFIX, W.TEXT_PREFIX
CFG = W.TINY
ATT = "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k"            # diffusers module
ATT_K = "lora_unet_" + ATT.replace(".", "_")                                   # kohya module
ATT_N = U + "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"          # engine tensor
CONV = "down_blocks.0.resnets.0.conv1"
CONV_N = U + "input_blocks.1.0.in_layers.2.weight"


def rnd(*shape, seed=0):
    return np.random.default_rng(seed + sum(shape)).standard_normal(shape).astype(np.float32)


def test_every_key_form_is_read():
    sd = {
        # kohya LoHa with alpha
        ATT_K + ".hada_w1_a": rnd(64, 4), ATT_K + ".hada_w1_b": rnd(4, 96), ATT_K + ".hada_w2_a": rnd(64, 4), ATT_K + ".hada_w2_b": rnd(4, 96),
        ATT_K + ".alpha": np.float32(2.0),
        # LyCORIS suffixes on a diffusers module path: Tucker LoCon under a dora_scale [N, 1, 1, 1]
        f"unet.{CONV}.lora_up.weight": rnd(64, 3, 1, 1), f"unet.{CONV}.lora_mid.weight": rnd(3, 3, 3, 3),
        f"unet.{CONV}.lora_down.weight": rnd(3, 64, 1, 1), f"unet.{CONV}.dora_scale": rnd(64, 1, 1, 1),
        # PEFT pair with its magnitude vector, on the text encoder
        "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight": rnd(2, 64),
        "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_B.weight": rnd(128, 2),
        "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_magnitude_vector": rnd(128),
        # kohya LoKr, w1 whole and w2 decomposed
        "lora_te_text_model_encoder_layers_1_self_attn_q_proj.lokr_w1": rnd(4, 2),
        "lora_te_text_model_encoder_layers_1_self_attn_q_proj.lokr_w2_a": rnd(16, 5),
        "lora_te_text_model_encoder_layers_1_self_attn_q_proj.lokr_w2_b": rnd(5, 32),
        "lora_te_text_model_encoder_layers_1_self_attn_q_proj.alpha": np.float32(10.0),
    }
    out = L.parse_adapters(sd, CFG)
    fc1, qp = T + "encoder.layers.0.mlp.fc1.weight", T + "encoder.layers.1.self_attn.q_proj.weight"
    assert set(out) == {ATT_N, CONV_N, fc1, qp}
    a = out[ATT_N]
    assert a.kind == "loha" and set(a.factors) == {"w1_a", "w1_b", "w2_a", "w2_b"} and a.alpha == 2.0 and a.magnitude is None
    assert L.effective_scale(a) == 0.5
    c = out[CONV_N]
    assert c.kind == "lora" and set(c.factors) == {"up", "mid", "down"} and c.alpha is None and c.magnitude.shape == (64,)
    assert L.effective_scale(c) == 1.0                                  # alpha missing: scale 1
    p = out[fc1]
    assert p.kind == "lora" and p.magnitude.shape == (128,) and p.factors["up"].shape == (128, 2)
    k = out[qp]
    assert k.kind == "lokr" and set(k.factors) == {"w1", "w2_a", "w2_b"} and L.effective_scale(k) == 2.0     # 10 / 5
    low = L.lower(k)
    assert low["kind"] == "kron" and low["up"].shape == (4, 2) and low["down"].shape == (16, 32)
    low = L.lower(c)
    assert low["kind"] == "pair" and low["up"].shape == (64, 3) and low["down"].shape == (3, 64, 3, 3) and low["magnitude"] is c.magnitude


def test_alpha_and_dim_rules():
    mk = lambda f, alpha: L.Adapter(kind="lokr", factors=f, alpha=alpha)
    assert L.effective_scale(mk(dict(w1=rnd(4, 2), w2=rnd(16, 32)), 7.0)) == 1.0          # nothing decomposed: 1 whatever alpha
    assert L.effective_scale(mk(dict(w1_a=rnd(4, 3), w1_b=rnd(3, 2), w2=rnd(16, 32)), 6.0)) == 2.0
    assert L.effective_scale(mk(dict(w1_a=rnd(4, 3), w1_b=rnd(3, 2), w2_a=rnd(16, 8), w2_b=rnd(8, 32)), 6.0)) == 0.75   # the last one
    assert L.effective_scale(mk(dict(w1=rnd(4, 2), t2=rnd(5, 5, 3, 3), w2_a=rnd(5, 16), w2_b=rnd(5, 32)), 10.0)) == 2.0
    assert L.effective_scale(mk(dict(w1_a=rnd(4, 3), w1_b=rnd(3, 2), w2=rnd(16, 32)), None)) == 1.0
    assert L.effective_scale(L.Adapter(kind="loha", factors=dict(w1_a=rnd(8, 4), w1_b=rnd(4, 8), w2_a=rnd(8, 4), w2_b=rnd(4, 8)))) == 1.0
    assert L.effective_scale(L.Adapter(kind="lora", factors=dict(up=rnd(8, 4), down=rnd(4, 8)), alpha=1.0)) == 0.25
    # the reference statement applies the same rules
    t = R.term("lokr", dict(w1=rnd(4, 2), w2=rnd(16, 32)), 7.0, 1.0, (64, 64))
    assert t["scale"] == 1.0
    t = R.term("lokr", dict(w1_a=rnd(4, 3), w1_b=rnd(3, 2), w2_a=rnd(16, 8), w2_b=rnd(8, 32)), 6.0, 1.0, (64, 64))
    assert t["scale"] == 0.75


@pytest.mark.parametrize("key,what", [
    ("lora_te1_text_model_encoder_layers_0_mlp_fc1.hada_w1_a", "SDXL text encoders"),
    ("text_encoder_2.text_model.encoder.layers.0.mlp.fc1.lora_A.weight", "SDXL text encoders"),
    ("controlnet.down_blocks.0.resnets.0.conv1.lokr_w1", "ControlNet"),
    ("transformer.transformer_blocks.0.attn.to_q.lora_A.weight", "SD3 transformer"),
    ("unet.down_blocks.0.resnets.0.conv9.hada_w1_a", "builds no tensor"),
    (ATT_K + ".hada_w3_a", "not an adapter factor"),
])
def test_refusals_name_the_first_offending_key(key, what):
    sd = {ATT_K + ".lora_up.weight": rnd(64, 2), ATT_K + ".lora_down.weight": rnd(2, 96), key: rnd(4, 4)}
    with pytest.raises(NotImplementedError, match=re.escape(f"'{key}'")) as ei:
        L.parse_adapters(sd, CFG)
    assert what in str(ei.value)


def test_magnitude_axes_and_incomplete_groups():
    pair = {ATT_K + ".lora_up.weight": rnd(64, 2), ATT_K + ".lora_down.weight": rnd(2, 96)}
    for shape in ((64,), (64, 1)):
        assert L.parse_adapters({**pair, ATT_K + ".dora_scale": rnd(*shape)}, CFG)[ATT_N].magnitude.shape == (64,)
    with pytest.raises(NotImplementedError, match=re.escape(f"'{ATT_K}.dora_scale'")):
        L.parse_adapters({**pair, ATT_K + ".dora_scale": rnd(1, 96)}, CFG)              # the input axis
    with pytest.raises(ValueError, match="dora_scale"):
        L.parse_adapters({**pair, ATT_K + ".dora_scale": rnd(63)}, CFG)
    with pytest.raises(ValueError, match="lacks a factor"):
        L.parse_adapters({ATT_K + ".hada_w1_a": rnd(64, 2), ATT_K + ".hada_w1_b": rnd(2, 96)}, CFG)
    with pytest.raises(ValueError, match="lacks lokr_w2"):
        L.parse_adapters({ATT_K + ".lokr_w1": rnd(4, 2)}, CFG)
    with pytest.raises(ValueError, match="mixes"):
        L.parse_adapters({**pair, ATT_K + ".lokr_w1": rnd(4, 2), ATT_K + ".lokr_w2": rnd(16, 48)}, CFG)


def test_parse_lora_is_still_strict():
    pair = {ATT_K + ".lora_up.weight": rnd(64, 2), ATT_K + ".lora_down.weight": rnd(2, 96)}
    assert set(L.parse_lora(pair, CFG)) == {ATT_N}
    for extra in (".hada_w1_a", ".lokr_w1", ".dora_scale", ".lora_mid.weight"):
        with pytest.raises(NotImplementedError, match=re.escape(f"'{ATT_K}{extra}'")):
            L.parse_lora({**pair, ATT_K + extra: rnd(4, 4)}, CFG)


def test_sd3_keys():
    cfg, tcfg = sd3.SD3_TINY, None
    q = "transformer.transformer_blocks.1.attn.to_q"
    sd = {q + ".lora_A.weight": rnd(4, 128), q + ".lora_B.weight": rnd(128, 4), q + ".alpha": np.float32(8.0),
          "transformer.transformer_blocks.1.norm1.linear.lokr_w1": rnd(6, 2),
          "transformer.transformer_blocks.1.norm1.linear.lokr_w2": rnd(128, 64),
          "transformer.transformer_blocks.0.attn.add_k_proj.hada_w1_a": rnd(128, 2),
          "transformer.transformer_blocks.0.attn.add_k_proj.hada_w1_b": rnd(2, 128),
          "transformer.transformer_blocks.0.attn.add_k_proj.hada_w2_a": rnd(128, 2),
          "transformer.transformer_blocks.0.attn.add_k_proj.hada_w2_b": rnd(2, 128),
          "transformer.transformer_blocks.0.attn.add_k_proj.dora_scale": rnd(128, 1)}
    out = L.parse_sd3_adapters(sd, cfg, tcfg)
    assert set(out) == {q + ".weight", "transformer.transformer_blocks.1.norm1.linear.weight",
                        "transformer.transformer_blocks.0.attn.add_k_proj.weight"}
    assert L.effective_scale(out[q + ".weight"]) == 2.0 and out[q + ".weight"].kind == "lora"
    assert out["transformer.transformer_blocks.0.attn.add_k_proj.weight"].magnitude.shape == (128,)
    g = "text_encoder_2.text_model.encoder.layers.1.mlp.fc1"
    te = {g + ".lora_A.weight": rnd(2, 192), g + ".lora_B.weight": rnd(320, 2)}
    assert set(L.parse_sd3_adapters(te, sd3.SD3_TINY, sd3.SD3_TINY_TEXT)) == {g + ".weight"}
    with pytest.raises(NotImplementedError, match="builds no tensor"):
        L.parse_sd3_adapters(te, cfg, None)                                   # an engine without text encoders
    for key, what in (("lora_unet_joint_blocks_0_x_block_attn_qkv.lora_up.weight", "kohya"),
                      ("text_encoder_3.encoder.block.0.layer.0.SelfAttention.q.lora_A.weight", "T5"),
                      ("controlnet.transformer_blocks.0.attn.to_q.lora_A.weight", "ControlNet"),
                      ("transformer.transformer_blocks.9.attn.to_q.lora_A.weight", "builds no tensor")):
        with pytest.raises(NotImplementedError, match=re.escape(f"'{key}'")) as ei:
            L.parse_sd3_adapters({**sd, key: rnd(4, 4)}, cfg, tcfg)
        assert what in str(ei.value)


def test_tucker_fold_equals_the_einsum():
    up, mid, down = rnd(16, 3), rnd(3, 5, 3, 3), rnd(5, 8)
    want = np.einsum("oi,ijyx,jc->ocyx", *(a.astype(np.float64) for a in (up, mid, down)))
    fold = L.tucker_fold(mid, down)
    assert fold.dtype == np.float32 and fold.shape == (3, 8, 3, 3)
    got = np.einsum("oi,icyx->ocyx", up.astype(np.float64), fold.astype(np.float64))
    assert np.abs(got - want).max() <= 2.0 ** -24 * (np.abs(up.astype(np.float64)) @ np.abs(fold.astype(np.float64)).reshape(3, -1)).max()
    np.testing.assert_array_equal(fold, R.tucker_fold(mid, down).astype(np.float32))
    # LoHa's Tucker form: P[o, c, y, x] = sum t[i, j, y, x] wa[i, o] wb[j, c]
    wa, wb, t = rnd(3, 16), rnd(5, 8), rnd(3, 5, 3, 3)
    low = L.lower(L.Adapter(kind="loha", factors=dict(w1_a=wa, w1_b=wb, t1=t, w2_a=wa, w2_b=wb, t2=t)))
    want = np.einsum("ijyx,io,jc->ocyx", *(a.astype(np.float64) for a in (t, wa, wb)))
    got = np.einsum("oi,icyx->ocyx", low["up"].astype(np.float64), low["down"].astype(np.float64))
    assert low["kind"] == "hada" and np.abs(got - want).max() < 1e-5 * np.abs(want).max()
    # a decomposed Kronecker factor with a Tucker core
    w2a, w2b = rnd(3, 4), rnd(5, 6)
    low = L.lower(L.Adapter(kind="lokr", factors=dict(w1=rnd(2, 2), t2=t, w2_a=w2a, w2_b=w2b)))
    want = np.einsum("ijyx,ip,jq->pqyx", *(a.astype(np.float64) for a in (t, w2a, w2b)))
    assert low["down"].shape == (4, 6, 3, 3) and np.abs(low["down"] - want).max() <= 2.0 ** -24 * np.abs(want).max()


def test_new_symbols_are_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    assert re.search(r"\bpd_lora_add_ex\s*\(", txt) and "pd_lora_factors" in txt
    assert "pd_lora_add_ex" in E.EXPORTS
    for m in ("lora_add_ex", "lora_add"):
        assert callable(getattr(E.Engine, m))
    for m in ("lora_add", "lora_add_ex", "lora_set_scales", "lora_remove", "read_weight"):
        assert callable(getattr(sd3.SD3Engine, m))
    assert [n for n, _ in E.LoraFactors._fields_] == ["kind", "rank", "rank2", "kron_a", "kron_b", "scale", "up", "down", "up2", "down2",
                                                      "magnitude"]


class _StubSD3Engine:
    cfg = sd3.SD3_TINY
    text_cfg = sd3.SD3_TINY_TEXT

    def __init__(self):
        self.calls = []

    def lora_add(self, aid, name, up, down, alpha=None):
        self.calls.append(("add", aid, name, alpha))

    def lora_add_ex(self, aid, name, kind, up, down, up2=None, down2=None, scale=1.0, magnitude=None):
        self.calls.append(("add_ex", aid, name, kind, scale, magnitude is not None))

    def lora_set_scales(self, s):
        self.calls.append(("scales", list(s)))

    def lora_remove(self, aid):
        self.calls.append(("remove", aid))


def _sd3_file(text=False):
    q, k = "transformer.transformer_blocks.1.attn.to_q", "transformer.transformer_blocks.0.ff.net.2"
    sd = {q + ".lora_A.weight": rnd(4, 128), q + ".lora_B.weight": rnd(128, 4), q + ".alpha": np.float32(2.0),
          k + ".lokr_w1": rnd(4, 4), k + ".lokr_w2": rnd(32, 128)}
    if text:
        g = "text_encoder_2.text_model.encoder.layers.1.mlp.fc1"
        sd.update({g + ".lora_A.weight": rnd(2, 192), g + ".lora_B.weight": rnd(320, 2), g + ".lora_magnitude_vector": rnd(320)})
    return sd


def test_sd3_pipeline_bookkeeping_on_a_stub_engine():
    eng = _StubSD3Engine()
    pipe = SD3Pipe(eng)
    pipe.load_lora_weights(_sd3_file(), adapter_name="a")
    pipe.load_lora_weights(_sd3_file(text=True))
    assert pipe.get_active_adapters() == ["a", "default_1"]
    assert pipe.get_list_adapters() == {"transformer": ["a", "default_1"], "text_encoder_2": ["default_1"]}
    adds = [c for c in eng.calls if c[0].startswith("add")]
    assert adds[0] == ("add", 0, "transformer.transformer_blocks.1.attn.to_q.weight", 2.0)           # plain pairs keep lora_add
    assert adds[1] == ("add_ex", 0, "transformer.transformer_blocks.0.ff.net.2.weight", "kron", 1.0, False)
    assert adds[-1] == ("add_ex", 1, "text_encoder_2.text_model.encoder.layers.1.mlp.fc1.weight", "pair", 1.0, True)
    assert not any(c[0] == "scales" for c in eng.calls)                   # nothing merged before a call
    assert pipe._lora_scales(0.5) == [0.5, 0.5]
    pipe.set_adapters(["default_1"], [0.25])
    pipe._lora_sync(2.0)
    assert eng.calls[-1] == ("scales", [0.0, 0.5])
    n = len(eng.calls)
    pipe._lora_sync(2.0)
    assert len(eng.calls) == n                                             # unchanged scales: no merge
    with pytest.raises(ValueError, match="already in use"):
        pipe.load_lora_weights(_sd3_file(), adapter_name="a")
    pipe.delete_adapters("a")
    assert eng.calls[-1] == ("remove", 0) and pipe.get_list_adapters() == {"transformer": ["default_1"], "text_encoder_2": ["default_1"]}
    pipe.unload_lora_weights()
    assert eng.calls[-1] == ("remove", -1) and pipe.get_list_adapters() == {}
    # text-encoder adapters next to an injected encode_prompt are refused; transformer-only ones are fine
    other = SD3Pipe(_StubSD3Engine(), encode_prompt=lambda *a, **k: None)
    with pytest.raises(ValueError, match="encode_prompt"):
        other.load_lora_weights(_sd3_file(text=True))
    other.load_lora_weights(_sd3_file())
    with pytest.raises(NotImplementedError, match="unsupported arguments"):
        other.load_lora_weights(_sd3_file(), weight_name="x.safetensors")


# ------------------------------------------------------------------------------------------------ the error budget
def _case(shape, seed):
    from tests.test_adapters_gpu import PAIRINGS, clean, magnitude, make, variant_for
    rng = np.random.default_rng(seed)
    w0 = (rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))).astype(np.float32)
    for (va, da), (vb, db) in PAIRINGS:
        ref_terms, dev_terms = [], []
        for v, d, r, s in ((va, da, 3, 0.7), (vb, db, 37, -1.3)):
            kind, f, alpha = make(variant_for(v, shape), shape, r, "c")
            f = clean(f)
            mag = magnitude(w0, "m") if d else None
            ref_terms.append(R.term(kind, f, alpha, s, shape, mag))
            low = L.lower(L.Adapter(kind=kind, factors=f, alpha=alpha, magnitude=mag))
            if low["kind"] == "kron" and low["down"].ndim == 2 and len(shape) == 4:
                low["down"] = low["down"].reshape(low["down"].shape[0], -1, *shape[2:])
            dev_terms.append(dict(low, s=s))
        yield (va, vb), w0, ref_terms, dev_terms


@pytest.mark.parametrize("shape", [(64, 64), (64, 32, 3, 3), (64, 4, 3, 3), (160, 64)])
def test_fp32_emulation_stays_inside_the_bounds(shape):
    """The merge in the device's operation order, in float32 NumPy, stays inside adapter_ref's budget for every pairing of the GPU
    test -- and the budget stays below 1e-4 of the weights, so that it separates the formulas from their near misses (below)."""
    for what, w0, ref_terms, dev_terms in _case(shape, 1):
        ref, tol = R.merge(w0, ref_terms)
        err = np.abs(R.merge_fp32(w0, dev_terms).astype(np.float64) - ref)
        assert (err <= tol).all(), (what, float((err / tol).max()))
        assert tol.max() < 1e-4 * np.abs(ref).max(), what


def test_near_misses_fall_outside_the_bounds():
    """A sum in place of the Hadamard product, a swapped Kronecker index, a wrong norm axis and a DoRA formed against the running
    sum instead of W0 all miss the bound (with an ulp of f16 added, the coarsest budget a GPU case uses on weights of this size)."""
    shape = (64, 64)
    w0 = (np.random.default_rng(2).standard_normal(shape) / 8).astype(np.float32)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)
    f64 = lambda x: np.asarray(x, np.float64)

    def misses(terms, wrong):
        ref, tol = R.merge(w0, terms)
        return not (np.abs(wrong - ref) <= tol + np.maximum(ulp(ref), ulp(wrong))).all()

    h = dict(kind="hada", up=rnd(64, 3), down=rnd(3, 64) / 8, up2=rnd(64, 3, seed=1), down2=rnd(3, 64, seed=2), scale=0.5, s=0.7)
    assert misses([h], w0 + 0.35 * (f64(h["up"]) @ f64(h["down"]) + f64(h["up2"]) @ f64(h["down2"])))
    k = dict(kind="kron", up=rnd(8, 2), down=rnd(8, 32) / 8, scale=1.0, s=0.7)
    assert misses([k], w0 + 0.7 * np.kron(f64(k["down"]), f64(k["up"])))
    assert misses([k], w0 + 0.7 * np.einsum("ij,pq->pijq", f64(k["up"]), f64(k["down"])).reshape(64, 64))
    m = np.linspace(0.5, 1.5, 64).astype(np.float32)
    d = dict(kind="pair", up=rnd(64, 4), down=rnd(4, 64) / 8, scale=1.0, s=0.7, magnitude=m)
    v = f64(w0) + 0.7 * f64(d["up"]) @ f64(d["down"])
    assert misses([d], f64(m)[None, :] / np.sqrt((v * v).sum(axis=0, keepdims=True)) * v)          # norm over the wrong axis
    p = dict(kind="pair", up=rnd(64, 2, seed=5), down=rnd(2, 64) / 8, scale=1.0, s=1.0)
    both, _ = R.merge(w0, [p, d])
    vp = v + f64(p["up"]) @ f64(p["down"])
    assert misses([p, d], f64(m)[:, None] / np.sqrt((vp * vp).sum(axis=1, keepdims=True)) * vp)     # DoRA on top of the other adapter
    assert not misses([p, d], both)
