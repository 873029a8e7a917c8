"""LoRA loading on the host: state-dict formats, diffusers -> LDM name mapping, rejections, the C ABI's new symbols and the
pipeline's adapter bookkeeping on a stub engine.  CPU only."""
import os
import re

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import lora as L
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = W.UNET_PREFIX
T = W.TEXT_PREFIX

# diffusers module -> engine tensor, written out by hand (SD1.5 layout)
PAIRS = [
    ("down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k", U + "input_blocks.4.1.transformer_blocks.0.attn2.to_k.weight"),
    ("down_blocks.0.attentions.1.transformer_blocks.0.ff.net.0.proj", U + "input_blocks.2.1.transformer_blocks.0.ff.net.0.proj.weight"),
    ("up_blocks.0.upsamplers.0.conv", U + "output_blocks.2.1.conv.weight"),
    ("up_blocks.1.upsamplers.0.conv", U + "output_blocks.5.2.conv.weight"),
    ("up_blocks.3.attentions.2.transformer_blocks.0.attn1.to_out.0", U + "output_blocks.11.1.transformer_blocks.0.attn1.to_out.0.weight"),
    ("down_blocks.2.resnets.1.conv1", U + "input_blocks.8.0.in_layers.2.weight"),
    ("down_blocks.1.resnets.0.conv_shortcut", U + "input_blocks.4.0.skip_connection.weight"),
    ("down_blocks.0.resnets.0.time_emb_proj", U + "input_blocks.1.0.emb_layers.1.weight"),
    ("down_blocks.2.downsamplers.0.conv", U + "input_blocks.9.0.op.weight"),
    ("up_blocks.2.resnets.2.conv2", U + "output_blocks.8.0.out_layers.3.weight"),
    ("mid_block.attentions.0.proj_in", U + "middle_block.1.proj_in.weight"),
    ("mid_block.resnets.1.conv2", U + "middle_block.2.out_layers.3.weight"),
    ("conv_in", U + "input_blocks.0.0.weight"),
    ("conv_out", U + "out.2.weight"),
    ("time_embedding.linear_2", U + "time_embed.2.weight"),
]
TE_PAIRS = [
    ("text_model.encoder.layers.3.self_attn.q_proj", T + "encoder.layers.3.self_attn.q_proj.weight"),
    ("text_model.encoder.layers.11.mlp.fc2", T + "encoder.layers.11.mlp.fc2.weight"),
]


def _rng(tag):
    return np.random.Generator(np.random.Philox(key=[7, sum(map(ord, tag))]))


def _pair(shape, r, tag):
    """seeded up [N, r] / down [r, *shape[1:]] for a tensor of this shape"""
    g = _rng(tag)
    return (g.standard_normal((shape[0], r), dtype=np.float32),
            g.standard_normal((r,) + tuple(shape[1:]), dtype=np.float32))


def test_name_pairs_by_hand():
    um, tm = L.unet_module_map(W.SD15), L.text_module_map(W.SD15)
    for d, n in PAIRS:
        assert um[d] == n, d
    for d, n in TE_PAIRS:
        assert tm[d] == n, d
    shapes = dict((n, s) for n, s, _ in W.unet_spec(W.SD15) + W.text_spec(W.SD15))
    sd = {}
    for d, n in PAIRS:
        up, down = _pair(shapes[n], 2, d)
        sd["lora_unet_" + d.replace(".", "_") + ".lora_up.weight"] = up
        sd["lora_unet_" + d.replace(".", "_") + ".lora_down.weight"] = down
    for d, n in TE_PAIRS:
        up, down = _pair(shapes[n], 2, d)
        sd["lora_te_" + d.replace(".", "_") + ".lora_up.weight"] = up
        sd["lora_te_" + d.replace(".", "_") + ".lora_down.weight"] = down
    out = L.parse_lora(sd, W.SD15)
    assert sorted(out) == sorted(n for _, n in PAIRS + TE_PAIRS)


@pytest.mark.parametrize("cfg", [W.SD15, W.TINY], ids=["sd15", "tiny"])
def test_every_in_scope_matrix_is_reachable(cfg):
    """Every UNet matrix (attention, feed-forward, proj, resnet convs, up/down samplers, time embedding, conv_in/out) and
    every CLIP attention / MLP matrix has exactly one diffusers module; kohya keys built from it parse back with the right
    up / down shapes."""
    um, tm = L.unet_module_map(cfg), L.text_module_map(cfg)
    spec = dict((n, s) for n, s, _ in W.unet_spec(cfg) + W.text_spec(cfg))
    want_u = {n for n, s, k in W.unet_spec(cfg) if k == "w" and len(s) >= 2}
    want_t = {n for n, s, k in W.text_spec(cfg) if k == "w" and "embeddings" not in n}
    assert set(um.values()) == want_u and len(um) == len(want_u)
    assert set(tm.values()) == want_t and len(tm) == len(want_t)
    sd = {}
    for d, n in list(um.items()) + list(tm.items()):
        pre = "lora_unet_" if n.startswith(U) else "lora_te_"
        k = pre + d.replace(".", "_")
        s = spec[n]
        sd[k + ".lora_up.weight"] = np.zeros((s[0], 4) + ((1, 1) if len(s) == 4 else ()), np.float32)
        sd[k + ".lora_down.weight"] = np.zeros((4,) + tuple(s[1:]), np.float32)
    out = L.parse_lora(sd, cfg)
    assert set(out) == want_u | want_t
    for n, (up, down, alpha) in out.items():
        assert up.shape == (spec[n][0], 4) and down.shape == (4,) + tuple(spec[n][1:]) and alpha == 4.0


def test_formats_parse_to_the_same_triples():
    d = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"
    te = "text_model.encoder.layers.0.self_attn.v_proj"
    up, down = _pair((640, 640), 4, "q")
    tup, tdown = _pair((768, 768), 4, "v")
    kohya = {"lora_unet_" + d.replace(".", "_") + ".lora_up.weight": up * np.float32(0.5),
             "lora_unet_" + d.replace(".", "_") + ".lora_down.weight": down,
             "lora_unet_" + d.replace(".", "_") + ".alpha": np.array(2.0, np.float32),
             "lora_te_" + te.replace(".", "_") + ".lora_up.weight": tup,
             "lora_te_" + te.replace(".", "_") + ".lora_down.weight": tdown}
    peft = {"unet." + d + ".lora_B.weight": up, "unet." + d + ".lora_A.weight": down,
            "text_encoder." + te + ".lora_B.weight": tup, "text_encoder." + te + ".lora_A.weight": tdown}
    legacy = {"down_blocks.1.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.up.weight": up,
              "down_blocks.1.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight": down}
    name = U + "input_blocks.4.1.transformer_blocks.0.attn1.to_q.weight"
    tname = T + "encoder.layers.0.self_attn.v_proj.weight"
    a, b, c = L.parse_lora(kohya), L.parse_lora(peft), L.parse_lora(legacy)
    assert sorted(a) == sorted(b) == sorted([name, tname]) and list(c) == [name]

    def eff(t):   # (alpha / r) * up @ down, the update each format stands for
        u, dn, al = t
        return (al / u.shape[1]) * (u.astype(np.float64) @ dn.reshape(dn.shape[0], -1))
    # kohya: (alpha 2 / rank 4) x (0.5 up) = 0.25 of the PEFT / legacy update (no alpha there: alpha = rank)
    np.testing.assert_allclose(eff(a[name]), 0.25 * eff(b[name]), rtol=1e-6)
    np.testing.assert_array_equal(eff(b[name]), eff(c[name]))
    np.testing.assert_array_equal(eff(a[tname]), eff(b[tname]))
    assert a[name][2] == 2.0 and b[name][2] == 4.0 and c[name][2] == 4.0


def test_safetensors_file_round_trip(tmp_path):
    from safetensors.numpy import save_file
    d = "mid_block.attentions.0.proj_out"
    up, down = _pair((1280, 1280, 1, 1), 8, "p")
    path = tmp_path / "x.safetensors"
    save_file({"unet." + d + ".lora_B.weight": up[:, :, None, None].copy(), "unet." + d + ".lora_A.weight": down}, str(path))
    out = L.parse_lora(str(path))
    u, dn, al = out[U + "middle_block.1.proj_out.weight"]
    np.testing.assert_array_equal(u, up)
    np.testing.assert_array_equal(dn, down)
    assert al == 8.0


@pytest.mark.parametrize("bad", [
    "lora_unet_down_blocks_0_attentions_0_proj_in.hada_w1_a",
    "lora_unet_down_blocks_0_attentions_0_proj_in.lokr_w1",
    "unet.down_blocks.0.attentions.0.proj_in.lora_magnitude_vector",
    "lora_unet_down_blocks_0_attentions_0_proj_in.dora_scale",
    "lora_te2_text_model_encoder_layers_0_mlp_fc1.lora_up.weight",
    "transformer.transformer_blocks.0.attn.to_q.lora_A.weight",
    "lora_unet_down_blocks_0_attentions_0_norm.lora_up.weight",
    "unet.down_blocks.3.attentions.0.proj_in.lora_A.weight",
])
def test_rejections_name_the_first_bad_key(bad):
    ok = "lora_unet_down_blocks_0_attentions_0_proj_in"
    sd = {ok + ".lora_up.weight": np.zeros((320, 2, 1, 1), np.float32), ok + ".lora_down.weight": np.zeros((2, 320, 1, 1), np.float32),
          bad: np.zeros((2, 2), np.float32), bad + "_second": np.zeros((2, 2), np.float32)}
    with pytest.raises(NotImplementedError, match=re.escape(f"'{bad}'")):
        L.parse_lora(sd)


def test_new_symbols_are_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    for n in ("pd_lora_add", "pd_lora_set_scales", "pd_lora_remove", "pd_read_weights"):
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in E.EXPORTS
    for m in ("lora_add", "lora_set_scales", "lora_remove", "read_weight"):
        assert callable(getattr(E.Engine, m))


# ------------------------------------------------------------------ pipeline on a stub engine
class _StubEngine:
    cfg = W.TINY

    def __init__(self):
        self.calls = []
        self.scales = None

    def lora_add(self, aid, name, up, down, alpha=None):
        self.calls.append(("add", aid, name))

    def lora_set_scales(self, s):
        self.calls.append(("scales", list(s)))
        self.scales = list(s)

    def lora_remove(self, aid):
        self.calls.append(("remove", aid))

    def num_ddim_steps(self, steps):
        return steps

    def ddim_sample(self, **kw):
        self.calls.append(("sample",))
        return np.zeros_like(kw["x_T"])


def _lora_sd(seed_tag, text=False):
    d = "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_v"
    up, down = _pair((128, 96), 2, seed_tag)
    sd = {"unet." + d + ".lora_B.weight": up, "unet." + d + ".lora_A.weight": down}
    if text:
        sd["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_B.weight"] = np.zeros((192, 2), np.float32)
        sd["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight"] = np.zeros((2, 96), np.float32)
    return sd


def _call(pipe, **kw):
    img = np.zeros((1, 64, 64, 3), np.float32)
    emb = np.zeros((1, 77, 96), np.float32)
    return pipe(prompt_embeds=emb, negative_prompt_embeds=emb, image=img, image_pair=[img, img], num_inference_steps=2,
                output_type="latent", **kw)


def test_pipeline_effective_scales_and_lazy_merges():
    eng = _StubEngine()
    pipe = PromptDiffusionPipeline(eng)
    with pytest.raises(NotImplementedError):
        _call(pipe, cross_attention_kwargs={"scale": 0.5})      # no adapter loaded yet
    pipe.load_lora_weights(_lora_sd("a"), adapter_name="a")
    pipe.load_lora_weights(_lora_sd("b", text=True))
    assert pipe.get_active_adapters() == ["a", "default_1"]
    assert pipe.get_list_adapters() == {"unet": ["a", "default_1"], "text_encoder": ["default_1"]}
    assert not any(c[0] == "scales" for c in eng.calls)         # nothing merged before a call
    with pytest.raises(NotImplementedError):
        _call(pipe, cross_attention_kwargs={"scale": 0.5, "other": 1})
    _call(pipe)
    assert eng.scales == [1.0, 1.0]
    n = len([c for c in eng.calls if c[0] == "scales"])
    _call(pipe)                                                 # same scales: no re-merge
    assert len([c for c in eng.calls if c[0] == "scales"]) == n
    pipe.set_adapters(["a", "default_1"], [0.5, 2.0])
    pipe.set_adapters(["default_1", "a"], [2.0, 0.5])           # the same state twice: still one merge at the call
    _call(pipe, cross_attention_kwargs={"scale": 0.5})
    assert eng.scales == [0.25, 1.0]
    assert len([c for c in eng.calls if c[0] == "scales"]) == n + 1
    pipe.set_adapters("a", 0.125)
    _call(pipe)
    assert eng.scales == [0.125, 0.0]
    pipe.delete_adapters("a")
    assert ("remove", 0) in eng.calls and pipe.get_active_adapters() == []
    pipe.unload_lora_weights()
    assert eng.calls[-1] == ("remove", -1) and pipe.get_list_adapters() == {}
    with pytest.raises(NotImplementedError):
        _call(pipe, cross_attention_kwargs={"scale": 0.5})


def test_pipeline_refuses_text_keys_with_a_caller_text_encoder():
    pipe = PromptDiffusionPipeline(_StubEngine(), text_encoder=lambda p: np.zeros((len(p), 77, 96), np.float32))
    with pytest.raises(ValueError, match="text_encoder"):
        pipe.load_lora_weights(_lora_sd("t", text=True))
    pipe.load_lora_weights(_lora_sd("u"))      # UNet-only adapters are fine
    with pytest.raises(ValueError):
        pipe.set_adapters("nope")
