"""LoHa, LoKr, Tucker and DoRA adapters merged on the device (pd_lora_add_ex, csrc/lora.hip) against the fp64 statement of
tests/adapter_ref.py, on the TINY engine in every storage type and on the reduced SD3 engine.

Bound of every comparison (adapter_ref.merge has the derivation): one ulp of the storage type on reference and result, plus
2^-23 x (fp32 operations on the path: the ranks, the two scale products, the Hadamard product, the K-long norm sum, the division,
the additions of the running sum) x the magnitude sums of the reference.  Inputs are synthetic and seeded."""
import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import lora as L
from prompt_diffusion_amd import weights as W
from tests import adapter_ref as R
from tests.test_lora_gpu import PRECS, TB, TINY_TARGETS, U, _factors, _tiny_engine, _tiny_kw, _ulp

pytestmark = pytest.mark.gpu

K_ROWS = TB + "attn1.to_k.weight"
CONV3 = U + "input_blocks.1.0.in_layers.2.weight"


def _rng(tag, r):
    return np.random.Generator(np.random.Philox(key=[23, sum(ord(c) * (i + 1) for i, c in enumerate(tag)) + r]))


def _n(g, shape, std):
    return g.standard_normal(shape, dtype=np.float32) * np.float32(std)


def make(variant, shape, r, tag):
    """(kind, factors, alpha) of one synthetic adapter in its file's key roles, scaled so its delta is of the order of the weight"""
    g = _rng(tag + variant, r)
    N, cin, tail = shape[0], shape[1], tuple(shape[2:])
    K = int(np.prod(shape[1:]))
    if variant == "lora":
        return "lora", dict(up=_n(g, (N, r), r ** -0.5), down=_n(g, (r,) + tuple(shape[1:]), K ** -0.5)), r / 2
    if variant == "locon_tucker":      # 3x3 convs only
        return "lora", dict(up=_n(g, (N, r, 1, 1), r ** -0.5), mid=_n(g, (r, r) + tail, 1.0 / r),
                            down=_n(g, (r, cin, 1, 1), (cin * 9) ** -0.5 * r ** 0.5)), float(r)
    if variant == "loha":
        return "loha", dict(w1_a=_n(g, (N, r), r ** -0.5), w1_b=_n(g, (r, K), K ** -0.5), w2_a=_n(g, (N, r), r ** -0.5),
                            w2_b=_n(g, (r, K), 1.0)), r / 2
    if variant == "loha_tucker":
        return "loha", dict(w1_a=_n(g, (r, N), 1.0), w1_b=_n(g, (r, cin), K ** -0.5), t1=_n(g, (r, r) + tail, 1.0 / r),
                            w2_a=_n(g, (r, N), 1.0), w2_b=_n(g, (r, cin), 1.0), t2=_n(g, (r, r) + tail, 1.0 / r)), None
    if variant.startswith("lokr"):
        a = {"lokr8": 8, "lokr1": 1, "lokrh": N // 2}.get(variant, 8)
        b = 2
        c, d = N // a, cin // b
        w1 = _n(g, (a, b), 1.0)
        if variant == "lokr_dec":      # decomposed w2 (and w1): alpha / r applies, r from w2_b
            return "lokr", dict(w1_a=_n(g, (a, 2), 1.0), w1_b=_n(g, (2, b), 1.0), w2_a=_n(g, (c, r), r ** -0.5),
                                w2_b=_n(g, (r, d * int(np.prod(tail or (1,)))), K ** -0.5)), 2.0 * r
        if variant == "lokr_4d":       # conv: w2 [c, d, kh, kw]; an undecomposed LoKr has scale 1 whatever its alpha
            return "lokr", dict(w1=w1, w2=_n(g, (c, d) + tail, K ** -0.5)), 123.0
        return "lokr", dict(w1=w1, w2=_n(g, (c, d) + tail if tail else (c, d), K ** -0.5)), None
    raise ValueError(variant)


def clean(f):
    return {k: v for k, v in f.items() if v is not None}


def magnitude(w0, tag):
    n = np.sqrt((w0.astype(np.float64).reshape(w0.shape[0], -1) ** 2).sum(axis=1))
    return (n * (1.0 + 0.2 * _rng(tag, 0).standard_normal(n.shape))).astype(np.float32)


class Loaded:
    """one adapter on one tensor: registered on the engine, and its fp64 term"""

    def __init__(self, e, aid, name, w0, variant, r, dora=False):
        kind, f, alpha = make(variant, w0.shape, r, f"{aid}{name}")
        f = clean(f)
        self.mag = magnitude(w0, name + variant) if dora else None
        L.add_to_engine(e, aid, name, L.Adapter(kind=kind, factors=f, alpha=alpha, magnitude=self.mag))
        self.args = (kind, f, alpha)

    def term(self, s, shape):
        kind, f, alpha = self.args
        return R.term(kind, f, alpha, s, shape, self.mag)


def check(got, w0, terms, prec, what):
    ref, tol32 = R.merge(w0, terms)
    tol = np.maximum(_ulp(ref, prec), _ulp(got, prec)) + tol32
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), (what, prec, float((err / tol).max()))
    return ref


def variant_for(v, shape):
    """the variant a tensor takes: Tucker and 4-D forms only exist on 3x3 convs"""
    conv3 = len(shape) == 4 and tuple(shape[2:]) == (3, 3)
    if v in ("loha_tucker", "locon_tucker", "lokr_4d") and not conv3:
        return {"loha_tucker": "loha", "locon_tucker": "lora", "lokr_4d": "lokr_dec"}[v]
    return v


# (variant of adapter 0 at rank 3, DoRA?), (variant of adapter 1 at rank 37, DoRA?)
PAIRINGS = [(("loha_tucker", False), ("lokr8", False)),
            (("lokr1", False), ("loha", False)),
            (("lokrh", False), ("locon_tucker", False)),
            (("lokr_4d", False), ("lora", True)),
            (("loha", True), ("lokr_dec", True))]


@pytest.mark.parametrize("prec", PRECS)
def test_each_kind_alone_and_in_pairs_tiny(prec):
    """Per pairing, adapter 0 (rank 3) and adapter 1 (rank 37) of different kinds sit on every tensor of the tiny target list (q and
    v rows of the fused q|k|v matrix, a context projection, GEGLU rows, a 1x1 proj_in, a 3x3 resnet conv, conv_in with cin 4, two
    text-encoder layers): each alone at 0.7 / -1.3, then both.  The k rows next to q and v stay bit-exact; scales back at 0 give W0
    bit for bit.  conv_in's pad columns are not visible through read_weight; every delta kernel writes them as exact zeros, and the
    derived-copy test below runs conv_in against a fresh engine."""
    e = _tiny_engine(prec)
    try:
        base = {n: e.read_weight(n) for n in TINY_TARGETS + [K_ROWS]}
        for (va, da), (vb, db) in PAIRINGS:
            ad = {}
            for n in TINY_TARGETS:
                shp = base[n].shape
                ad[n] = (Loaded(e, 0, n, base[n], variant_for(va, shp), 3, da), Loaded(e, 1, n, base[n], variant_for(vb, shp), 37, db))
            for n in TINY_TARGETS:   # added but inactive: nothing changes
                np.testing.assert_array_equal(e.read_weight(n), base[n])
            for sc in ([0.7, 0.0], [0.0, -1.3], [0.7, -1.3]):
                e.lora_set_scales(sc)
                for n in TINY_TARGETS:
                    terms = [ad[n][i].term(sc[i], base[n].shape) for i in range(2)]
                    ref = check(e.read_weight(n), base[n], terms, prec, (va, vb, sc, n))
                    assert np.abs(ref - base[n]).max() > 1e-3, (va, vb, n)    # the adapters do move the weights
                np.testing.assert_array_equal(e.read_weight(K_ROWS), base[K_ROWS])
            e.lora_set_scales([0.0, 0.0])
            for n in TINY_TARGETS:
                np.testing.assert_array_equal(e.read_weight(n), base[n])
            e.lora_remove(-1)
        assert e.stat("lora_targets") == 0 and e.stat("lora_bytes") == 0
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_mixtures_plain_hadamard_two_magnitudes_and_an_inactive_one(prec):
    """plain + LoHa on one tensor; two DoRA adapters on one tensor (each formed against W0 alone); an inactive adapter in between;
    removing the middle adapter leaves the same bytes as never having it active."""
    e = _tiny_engine(prec, text=False)
    try:
        names = [TB + "attn1.to_q.weight", TB + "ff.net.0.proj.weight", CONV3, U + "input_blocks.0.0.weight"]
        base = {n: e.read_weight(n) for n in names}
        ad = {n: [Loaded(e, 0, n, base[n], "lora", 37), Loaded(e, 1, n, base[n], "loha", 3), Loaded(e, 2, n, base[n], "lokr8", 5, True),
                  Loaded(e, 3, n, base[n], "lora", 4, True), Loaded(e, 4, n, base[n], "lora", 6)] for n in names}
        got = {}
        for sc in ([1.0, 0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.7, -1.3, 0.0], [0.7, -1.3, 0.0, 0.9, 1.1], [0.7, -1.3, 0.4, 0.9, 1.1]):
            e.lora_set_scales(sc)
            for n in names:
                got[n] = e.read_weight(n)
                check(got[n], base[n], [ad[n][i].term(sc[i], base[n].shape) for i in range(5)], prec, (sc, n))
        e.lora_set_scales([0.7, -1.3, 0.0, 0.9, 1.1])
        mid_off = {n: e.read_weight(n) for n in names}
        e.lora_set_scales([0.7, -1.3, 0.4, 0.9, 1.1])
        e.lora_remove(2)
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), mid_off[n])
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_a_zero_row_under_a_magnitude_stays_finite(prec):
    """W0 row 5 and the adapter's row 5 are both zero: the norm is 0, the factor is taken as 0 and the row stays exactly 0."""
    e = _tiny_engine(prec, text=False)
    try:
        n = TB + "attn2.to_k.weight"
        w0 = e.read_weight(n).copy()
        w0[5] = 0
        e.load_tensor(n, w0)
        w0 = e.read_weight(n)
        up, down = _factors(w0.shape, 4, n)
        up[5] = 0
        mag = magnitude(w0, n) + np.float32(0.5)
        e.lora_add_ex(0, n, "pair", up, down, scale=0.5, magnitude=mag)
        e.lora_set_scales([0.7])
        got = e.read_weight(n)
        assert np.isfinite(got).all() and not got[5].any()
        check(got, w0, [dict(kind="pair", up=up, down=down, scale=0.5, s=0.7, magnitude=mag)], prec, n)
    finally:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
def test_histories_restore_and_plain_only_targets(prec):
    """Two scale histories ending in the same scales give identical bytes; all scales at 0 give W0 bit for bit; a target that only
    carries plain pairs holds the bytes lora_add alone produces, whether the pair came through lora_add or lora_add_ex."""
    e, f = _tiny_engine(prec, text=False), _tiny_engine(prec, text=False)
    try:
        names = [n for n in TINY_TARGETS if n.startswith(U)]
        base = {n: e.read_weight(n) for n in names}
        for n in names:
            Loaded(e, 0, n, base[n], "loha", 5)
            Loaded(e, 1, n, base[n], "lora", 7, True)
            Loaded(e, 2, n, base[n], "lokr8", 3)
        e.lora_set_scales([0.8, 0.5, -0.6])
        direct = {n: e.read_weight(n) for n in names}
        e.lora_set_scales([-2.0, 0.0, 0.0])
        e.lora_set_scales([0.0, 3.0, 1.5])
        e.lora_set_scales([0.8, 0.5, -0.6])
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), direct[n])
        e.lora_set_scales([0.0, 0.0, 0.0])
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), base[n])
        e.lora_remove(-1)
        for n in names:     # plain pairs: engine e through lora_add_ex, engine f through lora_add
            up, down = _factors(base[n].shape, 9, n)
            e.lora_add_ex(0, n, "pair", up, down, scale=0.25)
            f.lora_add(0, n, up, down, alpha=0.25 * 9)
        Loaded(e, 1, K_ROWS, e.read_weight(K_ROWS), "loha", 3)     # a form elsewhere does not change the plain-only path
        e.lora_set_scales([0.9, 1.0])
        f.lora_set_scales([0.9])
        for n in names:
            np.testing.assert_array_equal(e.read_weight(n), f.read_weight(n))
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_derived_copies_follow_the_merge(prec):
    """eps after a merge equals, bit for bit, eps of a fresh engine loaded with the weights read back by read_weight (folded
    LayerNorms, conv_in's padded columns); text_encode likewise."""
    a, b = _tiny_engine(prec), _tiny_engine(prec)
    try:
        kw = _tiny_kw()
        t = np.array([500, 500], np.int64)
        ids = W.synth_token_ids(W.TINY, 2)
        run = lambda e: e.eps(kw["x_T"], t, kw["ctx_cond"], kw["pair"], kw["query"])
        plain, plain_text = run(a), a.text_encode(ids)
        for i, n in enumerate(TINY_TARGETS):
            Loaded(a, 0, n, a.read_weight(n), ("loha", "lokr8", "lora")[i % 3], 4, dora=i % 3 == 2)
        a.lora_set_scales([0.8])
        for n in TINY_TARGETS:
            b.load_tensor(n, a.read_weight(n))
        got = run(a)
        assert np.isfinite(got).all() and not np.array_equal(got, plain)
        np.testing.assert_array_equal(run(b), got)
        text = a.text_encode(ids)
        assert not np.array_equal(text, plain_text)
        np.testing.assert_array_equal(b.text_encode(ids), text)
    finally:
        a.close()
        b.close()


def test_refusals_name_the_tensor():
    e = _tiny_engine("f32", text=False)
    try:
        n = TB + "attn1.to_q.weight"
        up, down = _factors((64, 64), 4, n)
        with pytest.raises(E.PdError, match="unknown tensor 'nope'"):
            e.lora_add_ex(0, "nope", "hada", up, down, up, down)
        with pytest.raises(E.PdError, match="vector parameter"):
            e.lora_add_ex(0, TB + "norm1.weight", "pair", up, down)
        with pytest.raises(E.PdError, match=r"attn1.to_q.weight': up2 / down2"):
            e.lora_add_ex(0, n, "hada", up, down, up[:63], down)
        with pytest.raises(E.PdError, match=r"attn1.to_q.weight': w1 \(3, 2\).*a \* c = 64"):
            e.lora_add_ex(0, n, "kron", np.ones((3, 2), np.float32), np.ones((21, 32), np.float32))
        with pytest.raises(E.PdError, match="magnitude has 63 elements"):
            e.lora_add_ex(0, n, "pair", up, down, magnitude=np.ones(63, np.float32))
        with pytest.raises(E.PdError, match=r"attn1.to_q.weight': factors hold non-finite"):
            e.lora_add_ex(0, n, "hada", up, down, up * np.float32(np.nan), down)
        e.lora_add_ex(0, n, "hada", up, down, up, down)
        with pytest.raises(E.PdError, match="already has adapter 0"):
            e.lora_add_ex(0, n, "kron", np.ones((8, 2), np.float32), np.ones((8, 32), np.float32))
        with pytest.raises(E.PdError, match="already has adapter 0"):
            e.lora_add(0, n, up, down)
        e.sample_begin(**_tiny_kw())
        try:
            with pytest.raises(E.PdError, match="sampling session"):
                e.lora_add_ex(1, n, "hada", up, down, up, down)
        finally:
            e.sample_end()
        e.lora_set_scales([1.0])
        e.lora_remove(-1)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ SD3
from prompt_diffusion_amd import sd3  # noqa: E402
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as SD3Pipe  # noqa: E402
from tests.test_sd3_gpu import CFG as SD3CFG, inputs as sd3_inputs  # noqa: E402

B1 = "transformer.transformer_blocks.1."
MOD = "norm1.linear.weight"      # one stacked modulation matrix holds every block's rows
# tensor -> ((variant, DoRA) of adapter 0 at rank 3, of adapter 1 at rank 37)
SD3_TARGETS = {B1 + "attn.to_q.weight": (("loha", False), ("lokr8", False)),
               B1 + "attn.add_k_proj.weight": (("lokr_dec", False), ("lora", True)),
               B1 + "ff.net.0.proj.weight": (("loha", True), ("lora", False)),
               B1 + MOD: (("lokr1", False), ("loha", False))}
SD3_UNTOUCHED = ["transformer.transformer_blocks.0." + MOD, "transformer.transformer_blocks.2." + MOD, B1 + "attn.to_k.weight",
                 B1 + "attn.add_q_proj.weight"]


@pytest.mark.parametrize("fp8", [False, True])
def test_sd3_transformer_adapters_and_refreshed_copies(fp8):
    """Adapters on attn.to_q, attn.add_k_proj, ff.net.0.proj and norm1.linear of block 1 (f16 storage): read_weight within the bound,
    the other blocks' rows of the stacked modulation matrix and the neighbouring projections bit-exact, and forward bit-identical to
    a fresh engine loaded from the read-back weights -- with fp8=True that shows the e4m3 copies were rebuilt."""
    sd = sd3.synth_sd3_state_dict(SD3CFG)
    a, b = sd3.SD3Engine(SD3CFG, precision="f16", fp8=fp8), sd3.SD3Engine(SD3CFG, precision="f16", fp8=fp8)
    try:
        a.load_state_dict(sd)
        i = sd3_inputs(2, 8, 12, 5, seed=3)
        run = lambda e: e.forward(i["x"], i["t"], i["ctx"], i["pooled"], i["cond"], i["pair"], 0.8)
        plain = run(a)
        base = {n: a.read_weight(n) for n in list(SD3_TARGETS) + SD3_UNTOUCHED}
        ad = {n: [Loaded(a, k, n, base[n], v, r, d) for k, ((v, d), r) in enumerate(zip(vs, (3, 37)))] for n, vs in SD3_TARGETS.items()}
        sc = [0.7, -1.3]
        a.lora_set_scales(sc)
        back = {}
        for n in SD3_TARGETS:
            back[n] = a.read_weight(n)
            check(back[n], base[n], [ad[n][k].term(sc[k], base[n].shape) for k in range(2)], "f16", n)
        for n in SD3_UNTOUCHED:
            np.testing.assert_array_equal(a.read_weight(n), base[n])
        got = run(a)
        assert np.isfinite(got).all() and not np.array_equal(got, plain)
        b.load_state_dict({**sd, **back})
        np.testing.assert_array_equal(run(b), got)
        a.lora_set_scales([0.0, 0.0])
        np.testing.assert_array_equal(run(a), plain)
    finally:
        a.close()
        b.close()


def test_sd3_pipeline_load_lora_weights_end_to_end():
    """load_lora_weights on the SD3 pipeline (PEFT pair on the transformer, LoHa on a GEGLU-free MLP, LoKr on a CLIP-G layer), the
    adapter bookkeeping, and joint_attention_kwargs={"scale": s} against set_adapters(weight s); the CLIP-G matrix within the bound."""
    from tests.test_sd3_text_gpu import NET, TCFG
    e = sd3.SD3Engine(NET, precision="f16")
    try:
        e.configure_text(TCFG)
        e.load_state_dict({**sd3.synth_sd3_state_dict(NET), **sd3.synth_sd3_text_state_dict(TCFG, 3)})
        q, ff = "transformer.transformer_blocks.1.attn.to_q", "transformer.transformer_blocks.0.ff.net.0.proj"
        g = "text_encoder_2.text_model.encoder.layers.1.mlp.fc1"
        w0 = {m: e.read_weight(m + ".weight") for m in (q, ff, g)}
        file = {}
        _, f, _ = make("lora", w0[q].shape, 4, "q")
        file[q + ".lora_B.weight"], file[q + ".lora_A.weight"] = f["up"], f["down"]
        _, fh, _ = make("loha", w0[ff].shape, 3, "ff")
        file.update({f"{ff}.hada_{k}": v for k, v in fh.items()})
        file[ff + ".alpha"] = np.float32(1.5)
        _, fk, _ = make("lokr8", w0[g].shape, 3, "g")
        file.update({f"{g}.lokr_{k}": v for k, v in fk.items()})

        def tok(eos):
            def t(texts, max_length):
                out = np.full((len(texts), max_length), eos, np.int32)
                for r, s in enumerate(texts):
                    w = [8 + (sum(map(ord, x)) % 88) for x in s.split()][:max_length - 2]
                    out[r, 0] = 98
                    out[r, 1:1 + len(w)] = w
                return out
            return t
        pipe = SD3Pipe(e, tokenizers=(tok(99), tok(TCFG.clip_g.eos_token_id), tok(1)))
        lat = np.random.default_rng(5).standard_normal((1, 4, 8, 8)).astype(np.float32)
        call = lambda **k: pipe(prompt=["a red house"], negative_prompt=["blurry"], control_image=lat * 0.5, control_image_pair=lat * 0.25,
                                latents=lat, num_inference_steps=2, guidance_scale=5.0, output_type="latent", max_sequence_length=24,
                                **k)["images"]
        plain = call()
        with pytest.raises(NotImplementedError):
            call(joint_attention_kwargs={"scale": 0.5})      # no adapter loaded
        pipe.load_lora_weights(file, adapter_name="style")
        assert pipe.get_list_adapters() == {"transformer": ["style"], "text_encoder_2": ["style"]}
        full = call()
        assert np.isfinite(full).all() and not np.array_equal(full, plain)
        check(e.read_weight(g + ".weight"), w0[g], [R.term("lokr", fk, None, 1.0, w0[g].shape)], "f16", g)
        check(e.read_weight(ff + ".weight"), w0[ff], [R.term("loha", fh, 1.5, 1.0, w0[ff].shape)], "f16", ff)
        pipe.set_adapters("style", 0.5)
        half = call()
        assert not np.array_equal(half, full)
        pipe.set_adapters("style", 1.0)
        np.testing.assert_array_equal(call(joint_attention_kwargs={"scale": 0.5}), half)
        np.testing.assert_array_equal(call(), full)
        pipe.unload_lora_weights()
        np.testing.assert_array_equal(call(), plain)
    finally:
        e.close()


def test_st_tail_block_follows_a_loha_merge_sd15_f16():
    """The 320-channel block of SD1.5 in f16 (fused st_tail packs, folded LayerNorms live) with a LoHa adapter on every matrix of
    its transformer block: 5 DDIM steps at 16 x 16 latents equal those of an engine loaded with the read-back weights."""
    from tests.test_lora_gpu import ST_MATS, _sd15_kw
    a, b = E.Engine(W.SD15, precision="f16"), E.Engine(W.SD15, precision="f16")
    try:
        a.init_random_weights(21)
        b.init_random_weights(21)
        kw = _sd15_kw()
        plain = a.ddim_sample(**kw)
        names = [f"{TB}{m}.weight" for m in ST_MATS]
        for n in names:
            Loaded(a, 0, n, a.read_weight(n), "loha", 8)
        a.lora_set_scales([0.5])
        for n in names:
            b.load_tensor(n, a.read_weight(n))
        got = a.ddim_sample(**kw)
        assert np.isfinite(got).all() and not np.array_equal(got, plain)
        np.testing.assert_array_equal(b.ddim_sample(**kw), got)
    finally:
        a.close()
        b.close()
