"""Long prompts on the host side (CPU only): the reference's window split (cldm/hack.py, _hacked_clip_forward) restated in
prompt_diffusion_amd.pipeline against the ids the reference itself fed its CLIP (tests/golden/long_prompt.npz), the clip_skip mapping
between the reference's and the engine's count, and check_inputs on embeddings of any equal length.  The multi-window maps of the
fused tail kernel are checked in tests/test_st_tail_mw_layout_cpu.py."""
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.ddim import ControlLDM
from prompt_diffusion_amd.pipeline import (PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline, PromptDiffusionPipeline,
                                           reference_clip_skip, split_long_prompt, tokenize_long)
from tests.long_prompt_stub import TOKEN_COUNTS, StubTokenizer, prompt_of

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_prompt.npz"))


class _NoEngine:
    cfg = W.TINY

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before input validation finished")


def test_fixture_covers_the_window_boundaries():
    assert tuple(GOLD["token_counts"]) == TOKEN_COUNTS == (0, 74, 75, 76, 150, 226, 300)
    assert GOLD["window_ids"].shape == (7, 3, 77) and GOLD["z"].shape == (7, 231, W.TINY.context_dim)
    assert tuple(GOLD["raw_len"]) == TOKEN_COUNTS


def test_window_split_reproduces_the_reference_ids():
    vocab = int(GOLD["vocab"])
    bos, eos, pad = vocab - 2, vocab - 1, vocab - 1
    for b, n in enumerate(GOLD["raw_len"]):
        raw = GOLD["raw_tokens"][b, :n]
        got = split_long_prompt(raw, bos, eos, pad, windows=3)
        np.testing.assert_array_equal(got, GOLD["window_ids"][b])
        # what the split means: BOS first, the run, EOS right behind it, padding after; tokens past 225 are dropped
        for f in range(3):
            run = raw[75 * f:75 * (f + 1)]
            assert got[f, 0] == bos and (got[f, 1:1 + len(run)] == run).all() and got[f, 1 + len(run)] == eos
            assert (got[f, 2 + len(run):] == pad).all()
    # other window counts: 1 window keeps 75 tokens, 4 windows reach 300
    raw = GOLD["raw_tokens"][6, :300]
    assert split_long_prompt(raw, bos, eos, pad, windows=1).shape == (1, 77)
    w4 = split_long_prompt(raw, bos, eos, pad, windows=4)
    assert w4.shape == (4, 77) and (w4[3, 1:76] == raw[225:300]).all()


def test_tokenize_long_through_the_stub_tokenizer_is_prompt_major():
    tok = StubTokenizer(int(GOLD["vocab"]))
    prompts = [prompt_of(n, 100 + i, tok.vocab) for i, n in enumerate(TOKEN_COUNTS)]
    ids = tokenize_long(tok, prompts, 3, 77)
    assert ids.dtype == np.int32
    np.testing.assert_array_equal(ids, GOLD["window_ids"].reshape(21, 77))      # 'b f i -> (b f) i'
    with pytest.raises(ValueError, match="bos_token_id"):
        tokenize_long(lambda p, **kw: {"input_ids": [[1]] * len(p)}, prompts, 3, 77)


def test_clip_skip_mapping():
    """hack.py: hidden_states[-c] for c > 1, last layer otherwise; the engine's text_encode(clip_skip=k): hidden_states[-(k + 1)]"""
    assert [reference_clip_skip(c) for c in (0, 1, 2, 3, 12)] == [0, 0, 1, 2, 11]
    for c in (2, 3, 5):
        assert -(reference_clip_skip(c) + 1) == -c
    with pytest.raises(ValueError):
        reference_clip_skip(-1)


@pytest.mark.parametrize("cls", [PromptDiffusionPipeline, PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline])
def test_check_inputs_takes_any_equal_length(cls):
    pipe = cls(_NoEngine())
    img = np.zeros((1, 64, 64, 3), np.float32)
    pair = [img.copy(), img.copy()]
    D = W.TINY.context_dim
    for L in (1, 40, 77, 154, 231, E.PD_MAX_CONTEXT_LEN):
        emb = np.zeros((1, L, D), np.float32)
        pipe.check_inputs(None, img, pair, None, None, emb, emb)
    with pytest.raises(ValueError, match="must have the same shape"):
        pipe.check_inputs(None, img, pair, None, None, np.zeros((1, 231, D), np.float32), np.zeros((1, 77, D), np.float32))
    with pytest.raises(ValueError, match="1 <= L <= 1024"):
        too_long = np.zeros((1, E.PD_MAX_CONTEXT_LEN + 1, D), np.float32)
        pipe.check_inputs(None, img, pair, None, None, too_long, too_long)


def test_long_prompt_switches():
    pipe = PromptDiffusionPipeline(_NoEngine(), tokenizer=StubTokenizer(W.TINY.text_vocab))
    assert pipe._long_windows == 0
    pipe.enable_long_prompts()
    assert pipe._long_windows == 3
    pipe.enable_long_prompts(windows=2)
    assert pipe._long_windows == 2
    pipe.disable_long_prompts()
    assert pipe._long_windows == 0
    tok = StubTokenizer(W.TINY.text_vocab)
    assert PromptDiffusionPipeline(_NoEngine(), tokenizer=tok, long_prompts=True)._long_windows == 3
    assert PromptDiffusionInpaintPipeline(_NoEngine(), tokenizer=tok, long_prompts=4)._long_windows == 4
    assert PromptDiffusionPipeline(_NoEngine(), long_prompts=False)._long_windows == 0
    # the switch belongs to the engine's own encoder: without a tokenizer, or with a text_encoder callable, it is refused
    for kw in (dict(), dict(tokenizer=tok, text_encoder=lambda prompts: None)):
        with pytest.raises(ValueError, match="engine's own text encoder"):
            PromptDiffusionPipeline(_NoEngine(), **kw).enable_long_prompts()
        with pytest.raises(ValueError, match="engine's own text encoder"):
            PromptDiffusionPipeline(_NoEngine(), long_prompts=True, **kw)
    with pytest.raises(ValueError, match="exceed PD_MAX_CONTEXT_LEN"):
        pipe.enable_long_prompts(windows=14)
    with pytest.raises(ValueError):
        pipe.enable_long_prompts(windows=0)
    m = ControlLDM(_NoEngine(), tokenizer=StubTokenizer(W.TINY.text_vocab))
    assert m.long_prompt_windows == 0 and m.clip_skip == 0
    m.hack_everything(clip_skip=2)
    assert m.long_prompt_windows == 3 and m.clip_skip == 2


def test_sample_args_carry_the_context_length():
    """the ABI field sits where reserved[0] sat: the struct keeps its size"""
    import ctypes as C
    a = E.pd_sample_args()
    assert a.context_len == 0
    assert E.pd_sample_args.context_len.offset == E.pd_sample_args.init_flags.offset + 4
    assert C.sizeof(E.pd_sample_args) == E.pd_sample_args.context_len.offset + 4
    assert E.PD_MAX_CONTEXT_LEN == 1024
    assert "pd_op_spatial_transformer_ctx" in E.EXPORTS and "pd_eps_ctx" in E.EXPORTS
