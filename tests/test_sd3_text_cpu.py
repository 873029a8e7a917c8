"""SD3 text encoders, the parts that need no GPU: the host bucket function, the NumPy restatement the GPU tests lean on (pinned here by
tests/golden/sd3_text.npz, which transformers itself computed: tests/golden/make_golden_sd3_text.py), and the pipeline's argument
handling around the encoders (promptdiffusioncontrolnetpipeline_sd3.py:351-545) with a stub engine.

The tiny configuration is sd3.SD3_TINY_TEXT.  It departs from the first sketch of this feature in one place: T5's d_model and joint_dim
are both 384 (not 192 / 256).  The reference concatenates the padded CLIP rows and the T5 rows along the token axis, so T5's width IS
the joint width, and it must hold the 128 + 192 CLIP columns plus some pad columns to have any; heads * d_kv = 128 != d_model stays."""
import os

import numpy as np
import pytest

from prompt_diffusion_amd import sd3
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as Pipe

from tests import sd3_text_ref as R

CFG = sd3.SD3_TINY_TEXT
GOLD = os.path.join(os.path.dirname(__file__), "golden", "sd3_text.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def sd(gold):
    return sd3.synth_sd3_text_state_dict(CFG, int(gold["seed"]))


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_bucket_function_matches_transformers(gold):
    """Every distance below 512, both signs, 32 buckets / max distance 128: the host function and the fp64 restatement agree with
    transformers' float32 formula (no boundary case to special-case at these settings)."""
    want = gold["buckets_512"]
    got = sd3.t5_relative_buckets(512, 32, 128)
    assert got.shape == want.shape == (1023,)
    assert np.array_equal(got, want)
    assert np.array_equal(R.t5_bucket(np.arange(-511, 512), 32, 128), want)
    # a shorter call is the middle of the longer one
    assert np.array_equal(sd3.t5_relative_buckets(20, 32, 128), want[511 - 19:511 + 20])
    assert want[511] == 0 and want[0] == 15 and want[-1] == 31      # saturated buckets on both sides


def test_numpy_restatement_reproduces_fixture(gold, sd):
    rows, bound = gold["clip_rows"], 2e-5
    for tag, c, prefix, ids in (("l", CFG.clip_l, "text_encoder.", gold["ids_l"]), ("g", CFG.clip_g, "text_encoder_2.", gold["ids_g"])):
        hs, pooled = R.clip_forward(sd, c, prefix, ids)
        for k in (0, 1):
            assert relmax(hs[-(k + 2)][:, rows], gold[f"hidden_{tag}_skip{k}"]) < bound, (tag, k)
        assert relmax(pooled, gold[f"pooled_{tag}"]) < bound, tag
    assert relmax(R.t5_forward(sd, CFG.t5, gold["ids_t5"]), gold["t5"]) < bound
    for k in (0, 1):
        pe, pooled = R.encode_prompt(sd, CFG, gold["ids_l"], gold["ids_g"], gold["ids_t5"], clip_skip=k)
        assert pe.shape == (3, 77 + 20, CFG.joint_dim)
        assert relmax(pe[:, gold["pe_rows"]], gold[f"prompt_embeds_skip{k}"]) < bound, k
        assert relmax(pooled, gold["pooled"]) < bound


def test_both_eos_rules_are_in_the_fixture(gold):
    ids_l, ids_g = gold["ids_l"], gold["ids_g"]
    assert CFG.clip_l.eos_token_id == 2 and CFG.clip_g.eos_token_id != 2
    pl, pg = R.eos_positions(ids_l, 2), R.eos_positions(ids_g, CFG.clip_g.eos_token_id)
    assert len(set(pl.tolist())) > 1 and len(set(pg.tolist())) > 1           # different positions across rows
    assert ((ids_g == CFG.clip_g.eos_token_id).sum(1) >= 2).any()            # the eos value twice in a row: the FIRST match counts
    assert (ids_l[np.arange(3), pl] == ids_l.max(1)).all() and not (ids_l == 2).any()   # argmax rule: no token 2 anywhere


def test_synth_state_dict_is_deterministic_and_complete():
    a, b = sd3.synth_sd3_text_state_dict(CFG, 5), sd3.synth_sd3_text_state_dict(CFG, 5)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert "text_encoder_3.encoder.embed_tokens.weight" not in a
    names = {n for n, _, _ in sd3.sd3_text_spec(sd3.SD3_MEDIUM_TEXT)}
    for n in ("text_encoder.text_projection.weight", "text_encoder_2.text_model.encoder.layers.31.mlp.fc1.weight", "text_encoder_3.shared.weight",
              "text_encoder_3.encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
              "text_encoder_3.encoder.block.23.layer.1.DenseReluDense.wi_0.weight", "text_encoder_3.encoder.final_layer_norm.weight"):
        assert n in names
    assert "text_encoder_3.encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight" not in names


# ---------------------------------------------------------------------------------------------------- pipeline argument handling
class StubEngine:
    """Records what the pipeline asks of the engine; the "embedding" of a row is its first token id."""

    def __init__(self, t5=True):
        self.cfg = sd3.SD3Config(in_channels=4, out_channels=4, heads=2, head_dim=64, layers=1, cn_layers=1, joint_dim=CFG.joint_dim,
                                 pooled_dim=CFG.pooled_dim)
        self.text_cfg = CFG if t5 else sd3.SD3TextConfig(clip_l=CFG.clip_l, clip_g=CFG.clip_g, t5=None, joint_dim=CFG.joint_dim)
        self.calls, self.sampled = [], None

    def encode_prompt_ids(self, ids_l, ids_g, ids_t5=None, clip_skip=None):
        self.calls.append(dict(ids_l=np.array(ids_l), ids_g=np.array(ids_g), ids_t5=None if ids_t5 is None else np.array(ids_t5), clip_skip=clip_skip))
        B, Lt = ids_l.shape[0], 0 if ids_t5 is None else ids_t5.shape[1]
        pe = np.zeros((B, 77 + Lt, self.cfg.joint_dim), np.float32)
        pe[:, :, 0] = ids_l[:, :1]
        pe[:, :, 1] = ids_g[:, :1]
        if ids_t5 is not None:
            pe[:, 77:, 2] = ids_t5[:, :1]
        pooled = np.zeros((B, self.cfg.pooled_dim), np.float32)
        pooled[:, 0] = ids_l[:, 0]
        return pe, pooled

    def sample(self, latents, pe, ppe, npe, nppe, **kw):
        self.sampled = dict(pe=pe, ppe=ppe, npe=npe, nppe=nppe)
        return latents


VOCAB = {"": 0, "a cat": 11, "a dog": 12, "two": 22, "three": 33, "bad": 44, "bad2": 55, "bad3": 66}


def make_tok(log, tag):
    def tok(texts, max_length):
        assert isinstance(texts, list) and all(isinstance(t, str) for t in texts)
        log.append((tag, list(texts), max_length))
        return np.array([[VOCAB[t]] * max_length for t in texts], np.int32)
    return tok


def run(eng, log, **kw):
    toks = (make_tok(log, "l"), make_tok(log, "g"), make_tok(log, "t5") if eng.text_cfg.t5 is not None else None)
    pipe = Pipe(eng, tokenizers=toks)
    lat = np.zeros((1, 4, 4, 4), np.float32)
    bs = len(kw["prompt"]) if isinstance(kw["prompt"], list) else 1
    ctl, lat = np.repeat(lat, bs, 0), np.repeat(lat, bs * kw.get("num_images_per_prompt", 1), 0)   # control latents: one per prompt
    return pipe(control_image=ctl, control_image_pair=ctl, latents=lat, output_type="latent", num_inference_steps=1, **kw)


def test_pipeline_prompt_fallbacks_and_negative_pass():
    eng, log = StubEngine(), []
    run(eng, log, prompt="a cat", guidance_scale=7.0, clip_skip=1, max_sequence_length=40)
    # prompt_2 / prompt_3 fall back to prompt; the negative prompt defaults to "" for all three; CLIP ids are 77 long, T5's max_sequence_length
    assert log == [("l", ["a cat"], 77), ("g", ["a cat"], 77), ("t5", ["a cat"], 40), ("l", [""], 77), ("g", [""], 77), ("t5", [""], 40)]
    assert [c["clip_skip"] for c in eng.calls] == [1, None]                  # the negative pass uses clip_skip None
    assert eng.sampled["pe"].shape == (1, 77 + 40, CFG.joint_dim) and eng.sampled["npe"].shape == (1, 77 + 40, CFG.joint_dim)
    eng, log = StubEngine(), []
    run(eng, log, prompt="a cat", prompt_2="two", prompt_3="three", negative_prompt="bad", negative_prompt_3="bad3", guidance_scale=7.0)
    assert [(t, x) for t, x, _ in log] == [("l", ["a cat"]), ("g", ["two"]), ("t5", ["three"]), ("l", ["bad"]), ("g", ["bad"]), ("t5", ["bad3"])]
    assert log[2][2] == 256
    eng, log = StubEngine(), []
    run(eng, log, prompt="a cat", guidance_scale=1.0)                         # no guidance: no negative pass at all
    assert len(eng.calls) == 1 and eng.sampled["npe"] is None


def test_pipeline_negative_prompt_errors_carry_the_reference_texts():
    eng, log = StubEngine(), []
    with pytest.raises(ValueError, match=r"`negative_prompt`: \['bad'\] has batch size 1, but `prompt`: \['a cat', 'a dog'\] has batch size 2\. "
                                         r"Please make sure that passed `negative_prompt` matches the batch size of `prompt`\."):
        run(eng, log, prompt=["a cat", "a dog"], negative_prompt=["bad"], guidance_scale=7.0)
    with pytest.raises(TypeError, match=r"`negative_prompt` should be the same type to `prompt`, but got <class 'tuple'> != <class 'list'>\."):
        run(eng, log, prompt=["a cat", "a dog"], negative_prompt=("bad", "bad2"), guidance_scale=7.0)
    with pytest.raises(ValueError, match="`max_sequence_length` cannot be greater than 512 but is 513"):
        run(eng, log, prompt="a cat", max_sequence_length=513)


def test_pipeline_without_t5_gives_77_rows():
    eng, log = StubEngine(t5=False), []
    run(eng, log, prompt=["a cat", "a dog"], guidance_scale=7.0)
    assert [t for t, _, _ in log] == ["l", "g", "l", "g"] and all(c["ids_t5"] is None for c in eng.calls)
    assert eng.sampled["pe"].shape == (2, 77, CFG.joint_dim) and eng.sampled["npe"].shape == (2, 77, CFG.joint_dim)


def test_pipeline_repeats_each_prompt_per_image_in_place():
    eng, log = StubEngine(), []
    run(eng, log, prompt=["a cat", "a dog"], negative_prompt=["bad", "bad2"], num_images_per_prompt=3, guidance_scale=7.0)
    # repeat(1, n, 1).view(B * n, L, -1): cat cat cat dog dog dog
    assert eng.sampled["pe"][:, 0, 0].tolist() == [11, 11, 11, 12, 12, 12] and eng.sampled["ppe"][:, 0].tolist() == [11, 11, 11, 12, 12, 12]
    assert eng.sampled["npe"][:, 0, 0].tolist() == [44, 44, 44, 55, 55, 55] and eng.sampled["nppe"].shape == (6, CFG.pooled_dim)


def test_injected_encode_prompt_keeps_precedence():
    eng, log, seen = StubEngine(), [], []

    def enc(**kw):
        seen.append(kw)
        z = np.zeros((1, 5, CFG.joint_dim), np.float32), np.zeros((1, CFG.pooled_dim), np.float32)
        return z[0], z[0], z[1], z[1]
    pipe = Pipe(eng, encode_prompt=enc, tokenizers=(make_tok(log, "l"), make_tok(log, "g"), make_tok(log, "t5")))
    lat = np.zeros((1, 4, 4, 4), np.float32)
    pipe(prompt="a cat", control_image=lat, control_image_pair=lat, latents=lat, output_type="latent", num_inference_steps=1)
    assert len(seen) == 1 and seen[0]["prompt"] == "a cat" and not log and not eng.calls
    with pytest.raises(ValueError, match="text prompts need the `encode_prompt` callable"):     # neither: today's error
        Pipe(eng)(prompt="a cat", control_image=lat, control_image_pair=lat, latents=lat, output_type="latent", num_inference_steps=1)


def test_given_negative_embeddings_are_kept_next_to_prompt_strings():
    eng, log = StubEngine(), []
    npe, nppe = np.full((1, 77 + 256, CFG.joint_dim), 3.0, np.float32), np.full((1, CFG.pooled_dim), 4.0, np.float32)
    run(eng, log, prompt="a cat", guidance_scale=7.0, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=nppe)
    assert len(eng.calls) == 1 and [t for t, _, _ in log] == ["l", "g", "t5"]          # only the missing half is encoded (:473)
    assert np.array_equal(eng.sampled["npe"], npe) and np.array_equal(eng.sampled["nppe"], nppe)
