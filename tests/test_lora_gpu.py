"""LoRA adapters merged on the device (pd_lora_*, csrc/lora.hip): merge accuracy against the fp64 host formula, refreshed
derived copies (folded LayerNorms, fused st_tail packs, captured graphs), bit-exact restore, path independence, base-weight
reloads, oracle parity, the pipeline surface and the refusals.  Inputs are synthetic and seeded."""
import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline

pytestmark = pytest.mark.gpu

U = W.UNET_PREFIX
T = W.TEXT_PREFIX
PRECS = ["f32", "f16x2", "f16", "bf16"]


def _factors(shape, r, tag, gain=1.0):
    """seeded up [N, r] / down [r, *shape[1:]], scaled so the update is of the order of the weight itself"""
    g = np.random.Generator(np.random.Philox(key=[11, sum(ord(c) * (i + 1) for i, c in enumerate(tag)) + r]))
    k = int(np.prod(shape[1:]))
    up = g.standard_normal((shape[0], r), dtype=np.float32) * np.float32(gain / np.sqrt(r))
    down = g.standard_normal((r,) + tuple(shape[1:]), dtype=np.float32) * np.float32(1.0 / np.sqrt(k))
    return up, down


def _ulp(x, prec):
    a = np.abs(np.asarray(x, np.float64))
    if prec == "f16":
        return np.spacing(a.astype(np.float16)).astype(np.float64)
    if prec == "bf16":
        return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 7)
    return np.spacing(a.astype(np.float32)).astype(np.float64)


def _host_merge(w0, terms):
    """fp64 W0 + sum s * up @ down, with the kernel's fp32 product s * up; and sum |U||D| for the error bound"""
    n = w0.shape[0]
    acc = w0.astype(np.float64).reshape(n, -1).copy()
    mag = np.zeros_like(acc)
    R = 0
    for s, up, down in terms:
        u = (np.float32(s) * up).astype(np.float64)
        d = down.reshape(down.shape[0], -1).astype(np.float64)
        acc += u @ d
        mag += np.abs(u) @ np.abs(d)
        R += up.shape[1]
    return acc.reshape(w0.shape), mag.reshape(w0.shape), R


def _check_merged(got, w0, terms, prec, what):
    ref, mag, R = _host_merge(w0, terms)
    tol = np.maximum(_ulp(ref, prec), _ulp(got, prec)) + R * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= tol).all(), (what, prec, float((err / tol).max()))


def _tiny_engine(prec, text=True):
    cfg = W.TINY
    e = E.Engine(cfg, precision=prec)
    for n, a in W.iter_synth(cfg):
        e.load_tensor(n, a)
    if text:
        e.load_state_dict(W.synth_text_state_dict(cfg), strict=False)
    return e


BLK = U + "input_blocks.1.1."          # TINY: 64 channels; SD1.5: 320 channels (the fused st_tail blocks)
TB = BLK + "transformer_blocks.0."
TINY_TARGETS = [TB + "attn1.to_q.weight", TB + "attn1.to_v.weight", TB + "attn2.to_k.weight", TB + "ff.net.0.proj.weight",
                BLK + "proj_in.weight", U + "input_blocks.1.0.in_layers.2.weight", U + "input_blocks.0.0.weight",
                T + "encoder.layers.0.self_attn.q_proj.weight", T + "encoder.layers.1.mlp.fc1.weight"]


@pytest.mark.parametrize("prec", PRECS)
def test_merge_accuracy_tiny(prec):
    """Two adapters (ranks 3 and 37: one partial LDS chunk, one spanning two) on linear rows of the fused q|k|v matrix, a
    context projection, GEGLU rows (TINY pads them), a 1x1 proj_in, a 3x3 resnet conv, conv_in (cin 4: padded columns) and
    text-encoder layers; the k rows next to the adapted q / v rows stay bit-exact."""
    e = _tiny_engine(prec)
    try:
        shapes = dict(e.param_names())
        base = {n: e.read_weight(n) for n in TINY_TARGETS + [TB + "attn1.to_k.weight"]}
        fac = {}
        for a, r in ((0, 3), (1, 37)):
            for n in TINY_TARGETS:
                fac[a, n] = _factors(shapes[n], r, f"{a}{n}")
                e.lora_add(a, n, *fac[a, n])
        for n in TINY_TARGETS:   # added but inactive: nothing changes
            np.testing.assert_array_equal(e.read_weight(n), base[n])
        e.lora_set_scales([0.7, -1.3])
        for n in TINY_TARGETS:
            _check_merged(e.read_weight(n), base[n], [(0.7, *fac[0, n]), (-1.3, *fac[1, n])], prec, n)
        np.testing.assert_array_equal(e.read_weight(TB + "attn1.to_k.weight"), base[TB + "attn1.to_k.weight"])
        e.lora_set_scales([0.0, 2.0])
        for n in TINY_TARGETS:
            _check_merged(e.read_weight(n), base[n], [(2.0, *fac[1, n])], prec, n)
    finally:
        e.close()


SD15_TARGETS = [TB + "attn1.to_q.weight", TB + "attn1.to_k.weight", TB + "attn1.to_v.weight", TB + "ff.net.0.proj.weight",
                TB + "ff.net.2.weight", TB + "attn2.to_v.weight", BLK + "proj_in.weight", U + "input_blocks.1.0.in_layers.2.weight"]


@pytest.mark.parametrize("prec", PRECS)
def test_merge_accuracy_sd15(prec):
    e = E.Engine(W.SD15, precision=prec)
    try:
        e.init_random_weights(5)
        shapes = dict(e.param_names())
        base = {n: e.read_weight(n) for n in SD15_TARGETS}
        fac = {n: _factors(shapes[n], 64, n) for n in SD15_TARGETS}
        for n in SD15_TARGETS:
            e.lora_add(3, n, *fac[n])
        e.lora_set_scales([0, 0, 0, 0.9])
        for n in SD15_TARGETS:
            _check_merged(e.read_weight(n), base[n], [(0.9, *fac[n])], prec, n)
    finally:
        e.close()


# every matrix of the SD1.5 320-channel blocks whose derived copies (folded LayerNorm, st_tail front / tail packs) are live
ST_MATS = ["attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_v", "attn2.to_out.0",
           "ff.net.0.proj", "ff.net.2"]
DERIVED_TARGETS = ([f"{U}{b}.transformer_blocks.0.{m}.weight" for b in ("input_blocks.1.1", "output_blocks.11.1") for m in ST_MATS]
                   + [U + "input_blocks.1.1.proj_in.weight", U + "output_blocks.11.1.proj_out.weight",
                      U + "input_blocks.2.0.out_layers.3.weight", U + "middle_block.1.transformer_blocks.0.attn1.to_q.weight",
                      T + "encoder.layers.0.self_attn.k_proj.weight", T + "encoder.layers.5.mlp.fc2.weight"])


def _sd15_kw(seed=9, steps=5):
    i = W.synth_inputs(W.SD15, 1, 16, 16, seed=seed)
    return dict(x_T=i["x_T"], ctx_cond=i["ctx_cond"], ctx_uncond=i["ctx_uncond"], pair=i["pair"], query=i["query"], steps=steps,
                cfg_scale=7.5)


def test_derived_copies_and_graphs_follow_the_merge_sd15_f16():
    """Engine A merges adapters; engine B gets A's merged weights through pd_load_weights.  5 DDIM steps at 16 x 16 latents
    (the fused st_tail blocks and the folded LayerNorms are live in f16) and text_encode are bit-identical, eager and with
    captured graphs.  A graph captured before a scale change is not replayed with stale weights."""
    a, b = E.Engine(W.SD15, precision="f16"), E.Engine(W.SD15, precision="f16")
    try:
        a.init_random_weights(21)
        b.init_random_weights(21)
        shapes = dict(a.param_names())
        kw = _sd15_kw()
        ids = W.synth_token_ids(W.SD15, 2)
        plain = a.ddim_sample(**kw)
        plain_text = a.text_encode(ids)
        for n in DERIVED_TARGETS:
            a.lora_add(0, n, *_factors(shapes[n], 16, n, gain=0.5))
        a.lora_set_scales([1.0])
        for n in DERIVED_TARGETS:
            b.load_tensor(n, a.read_weight(n))
        r1 = a.ddim_sample(**kw)
        assert np.isfinite(r1).all() and not np.array_equal(r1, plain)
        np.testing.assert_array_equal(b.ddim_sample(**kw), r1)
        t1 = a.text_encode(ids)
        assert not np.array_equal(t1, plain_text)
        np.testing.assert_array_equal(b.text_encode(ids), t1)
        a.set_option("graph", 1)
        b.set_option("graph", 1)
        np.testing.assert_array_equal(b.ddim_sample(**kw), r1)
        np.testing.assert_array_equal(a.ddim_sample(**kw), r1)     # captured at scale 1
        a.lora_set_scales([0.25])
        r2 = a.ddim_sample(**kw)                                   # same call after the change: not the old graph
        a.set_option("graph", 0)
        np.testing.assert_array_equal(a.ddim_sample(**kw), r2)
        assert not np.array_equal(r2, r1)
    finally:
        a.close()
        b.close()


def _tiny_kw(seed=4):
    i = W.synth_inputs(W.TINY, 2, 16, 16, seed=seed)
    return dict(x_T=i["x_T"], ctx_cond=i["ctx_cond"], ctx_uncond=i["ctx_uncond"], pair=i["pair"], query=i["query"], steps=4,
                cfg_scale=5.0)


@pytest.mark.parametrize("prec", PRECS)
def test_restore_is_exact_and_merges_do_not_depend_on_history(prec):
    e = _tiny_engine(prec, text=False)
    try:
        kw = _tiny_kw()
        plain = e.ddim_sample(**kw)
        shapes = dict(e.param_names())
        names = [n for n in TINY_TARGETS if n.startswith(U)] + [U + "middle_block.1.transformer_blocks.0.ff.net.2.weight"]
        base = {n: e.read_weight(n) for n in names}
        for a, r in ((0, 8), (1, 5)):
            for n in names[a::2] if a else names:
                e.lora_add(a, n, *_factors(shapes[n], r, f"{a}{n}"))
        e.lora_set_scales([0.8, 0.5])
        direct = {n: e.read_weight(n) for n in names}
        lat = e.ddim_sample(**kw)
        assert not np.array_equal(lat, plain)
        e.lora_set_scales([-2.0, 0.0])
        e.lora_set_scales([1.5, 3.0])
        e.lora_set_scales([0.8, 0.5])                   # s1 -> s2 -> s3 -> s1 == s1
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), direct[n])
        np.testing.assert_array_equal(e.ddim_sample(**kw), lat)
        e.lora_set_scales([0.0, 0.0])                   # scale 0 restores W0 bit-exactly
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), base[n])
        np.testing.assert_array_equal(e.ddim_sample(**kw), plain)
        e.lora_set_scales([0.8, 0.5])
        e.lora_remove(1)                                # one of two adapters: the other stays merged
        for n in names[0::2]:                           # (adapter 0 alone there)
            np.testing.assert_array_equal(e.read_weight(n), direct[n])
        e.lora_remove(-1)
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), base[n])
        np.testing.assert_array_equal(e.ddim_sample(**kw), plain)
        assert e.stat("lora_targets") == 0 and e.stat("lora_base_bytes") == 0
    finally:
        e.close()


def test_base_weight_reloads_reapply_the_merge():
    e = _tiny_engine("f32", text=False)
    try:
        n = TB + "attn1.to_k.weight"
        shapes = dict(e.param_names())
        fac = _factors(shapes[n], 6, n)
        e.lora_add(0, n, *fac)
        e.lora_set_scales([1.25])
        new = np.random.default_rng(1).standard_normal(shapes[n]).astype(np.float32) * np.float32(0.1)
        e.load_tensor(n, new)
        _check_merged(e.read_weight(n), new, [(1.25, *fac)], "f32", n)
        e.lora_remove(0)
        np.testing.assert_array_equal(e.read_weight(n), new)
        # pd_init_random_weights under an adapter: its values become the base
        e.lora_add(0, n, *fac)
        e.lora_set_scales([1.0])
        e.init_random_weights(77)
        e.lora_remove(-1)
        f = E.Engine(W.TINY, precision="f32")
        try:
            f.init_random_weights(77)
            np.testing.assert_array_equal(e.read_weight(n), f.read_weight(n))
        finally:
            f.close()
    finally:
        e.close()


def test_read_weight_inverts_load():
    e = E.Engine(W.TINY, precision="f32")
    try:
        sd = W.synth_state_dict(W.TINY)
        for n, a in sd.items():
            e.load_tensor(n, a)
        for n in [TB + "ff.net.0.proj.weight", TB + "ff.net.0.proj.bias", U + "input_blocks.0.0.weight", TB + "attn1.to_v.weight",
                  BLK + "norm.weight", U + "out.2.weight"]:
            np.testing.assert_array_equal(e.read_weight(n), sd[n])
    finally:
        e.close()


def test_oracle_parity_with_host_merged_weights():
    cfg = W.TINY
    e = _tiny_engine("f32", text=False)
    try:
        sd = W.synth_state_dict(cfg)
        shapes = dict(e.param_names())
        for n in TINY_TARGETS[:7]:
            up, down = _factors(shapes[n], 4, n)
            e.lora_add(2, n, up, down, alpha=2.0)
            ref, _, _ = _host_merge(sd[n], [(0.6 * 2.0 / 4, up, down)])
            sd[n] = ref.astype(np.float32)
        e.lora_set_scales([0, 0, 0.6])
        inp = W.synth_inputs(cfg, 1, 8, 8, seed=7)
        lay = O.make_layouts(cfg, W)
        cond = dict(c_crossattn=inp["ctx_cond"], example_pair=inp["pair"], query=inp["query"])
        unc = dict(c_crossattn=inp["ctx_uncond"], example_pair=inp["pair"], query=inp["query"])
        ref, _, _ = O.ddim_sampling(sd, cfg, lay, 4, inp["x_T"], cond, unc, 9.0)
        got = e.ddim_sample(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"],
                            query=inp["query"], steps=4, cfg_scale=9.0)
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) < 2e-4
        t = np.array([500], np.int64)
        eps = e.eps(inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
        eps_ref = O.apply_model(sd, cfg, lay, inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
        assert float(np.abs(eps - eps_ref).max() / np.abs(eps_ref).max()) < 1e-4
    finally:
        e.close()


def test_pipeline_load_lora_weights_end_to_end(tmp_path):
    from safetensors.numpy import save_file
    cfg = W.TINY
    e = _tiny_engine("f16")
    try:
        shapes = dict(e.param_names())
        sd = {}
        for d, n in (("down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k", TB + "attn2.to_k.weight"),
                     ("down_blocks.0.attentions.0.transformer_blocks.0.ff.net.0.proj", TB + "ff.net.0.proj.weight"),
                     ("mid_block.attentions.0.proj_in", U + "middle_block.1.proj_in.weight")):
            up, down = _factors(shapes[n], 4, n)
            sd[f"unet.{d}.lora_B.weight"], sd[f"unet.{d}.lora_A.weight"] = up, down
        up, down = _factors(shapes[T + "encoder.layers.0.mlp.fc1.weight"], 4, "fc1")
        sd["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_B.weight"] = up
        sd["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight"] = down
        path = tmp_path / "style.safetensors"
        save_file(sd, str(path))
        pipe = PromptDiffusionPipeline(e, tokenizer=lambda p: W.synth_token_ids(cfg, len(p)))
        img = np.random.default_rng(0).uniform(0, 1, (1, 64, 64, 3)).astype(np.float32)
        lat0 = np.random.default_rng(1).standard_normal((1, 4, 8, 8)).astype(np.float32)
        call = lambda **k: pipe(prompt="a", image=img, image_pair=[img, img[:, ::-1].copy()], num_inference_steps=4, latents=lat0,
                                output_type="latent", **k).images
        plain = call()
        pipe.load_lora_weights(str(path), adapter_name="style")
        assert pipe.get_list_adapters() == {"unet": ["style"], "text_encoder": ["style"]}
        full = call()
        assert not np.array_equal(full, plain)
        pipe.set_adapters("style", 0.5)
        half = call()
        pipe.set_adapters("style", 1.0)
        np.testing.assert_array_equal(call(cross_attention_kwargs={"scale": 0.5}), half)
        np.testing.assert_array_equal(call(), full)
        pipe.unload_lora_weights()
        np.testing.assert_array_equal(call(), plain)
    finally:
        e.close()


def test_refusals_name_the_tensor():
    e = _tiny_engine("f32", text=False)
    try:
        n = TB + "attn1.to_q.weight"
        shapes = dict(e.param_names())
        up, down = _factors(shapes[n], 4, n)
        with pytest.raises(E.PdError, match="unknown tensor 'nope'"):
            e.lora_add(0, "nope", up, down)
        with pytest.raises(E.PdError, match="vector parameter"):
            e.lora_add(0, TB + "norm1.weight", up[:, :1], down[:1, :1])
        with pytest.raises(E.PdError, match="up has 63 rows"):
            e.lora_add(0, n, up[:63], down)
        with pytest.raises(E.PdError, match="down must be"):
            e.lora_add(0, n, up, down[:, :60])
        with pytest.raises(E.PdError, match="down must be"):
            e.lora_add(0, U + "input_blocks.1.0.in_layers.2.weight", np.zeros((64, 4), np.float32), np.zeros((4, 64, 1, 9), np.float32))
        with pytest.raises(E.PdError, match="rank 0"):
            e.lora_add(0, n, up[:, :0], down[:0])
        with pytest.raises(E.PdError, match="non-finite values"):
            e.lora_add(0, n, up * np.float32(np.inf), down)
        e.lora_add(0, n, up, down)
        with pytest.raises(E.PdError, match="already has adapter 0"):
            e.lora_add(0, n, up, down)
        with pytest.raises(E.PdError, match="non-finite scale"):
            e.lora_set_scales([float("nan")])
        with pytest.raises(E.PdError, match="unknown adapter id 1"):
            e.lora_set_scales([1.0, 1.0])
        with pytest.raises(E.PdError, match="unknown adapter id 5"):
            e.lora_remove(5)
        e.sample_begin(**_tiny_kw())
        try:
            with pytest.raises(E.PdError, match="sampling session"):
                e.lora_add(1, TB + "attn1.to_k.weight", up, down)
            with pytest.raises(E.PdError, match="sampling session"):
                e.lora_set_scales([1.0])
            with pytest.raises(E.PdError, match="sampling session"):
                e.lora_remove(-1)
        finally:
            e.sample_end()
        e.lora_set_scales([1.0])       # the engine still works after every refusal
        e.lora_remove(-1)
    finally:
        e.close()
