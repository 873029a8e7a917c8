"""Perturbed-attention guidance without a GPU: the layer-name grammar (prompt_diffusion_amd/pag.py), the restatement (tests/pag_ref.py)
and that the inputs of tests/test_pag_gpu.py have teeth, the adaptive scale, the pipelines' argument checks on a stub engine.

Teeth: every (layer set, latent size, mode) the GPU network tests use must move the restatement's conditional eps -- max |e_c - e_p| /
max |e_c| at t = 801 on W.TINY's synthetic weights -- by at least 5 x the tolerance that GPU test applies against the restatement.  The
set {0, 15, 6..14} reaches about 0.6, which is 5 x every bound but bf16's 1.5e-1 (0.75): bf16 is held to the margin it does reach, at
least 2 x, with the figure printed.  "mid" alone moves eps by 1.5e-2 at 16 x 16 (an f32 / f16x2 case only) and by exactly 0 at 8 x 8,
where the middle block has one token and the softmax over one key is the identity."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pag import PAGMixin, pag_block_table, parse_pag_layers
from tests import pag_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ORACLE = {"f32": 2e-4, "f16x2": 2e-4, "f16": 2e-2, "bf16": 1.5e-1}     # tests/test_cfg_share_gpu.py, against the oracle
TOL_PATH = {"f32": 2e-5, "f16x2": 2e-5, "f16": 1e-2, "bf16": 8e-2}         # ... engine path against engine path
T_EPS, B, HW, S, CFG_SCALE, PAG_SCALE = 801, 2, 16, 5, 7.5, 3.0
WIDE = (0, 15) + tuple(range(6, 15))       # block 0, the middle block, the nine decoder blocks
MID = (15,)
ALL = tuple(range(16))
# (layer set, B, h, w, modes) of the GPU network cases
GPU_CASES = [(MID, B, HW, HW, ("f32", "f16x2")), (WIDE, B, HW, HW, ("f32", "f16x2", "f16", "bf16")), (ALL, 1, 8, 24, ("f32",))]


@functools.lru_cache(maxsize=None)
def tiny():
    cfg = W.TINY
    return cfg, W.synth_state_dict(cfg), O.make_layouts(cfg, W)


def conds(inp):
    cond = dict(c_crossattn=inp["ctx_cond"], example_pair=inp["pair"], query=inp["query"])
    unc = dict(c_crossattn=inp["ctx_uncond"], example_pair=inp["pair"], query=inp["query"])
    return cond, unc


@functools.lru_cache(maxsize=None)
def branches(blocks, b, h, w, with_cfg=True):
    """(e_u, e_c, e_p) of the restatement at t = 801 on synth_inputs(TINY, b, h, w) (the default seed), once per case"""
    cfg, sd, lay = tiny()
    inp = W.synth_inputs(cfg, b, h, w)
    cond, unc = conds(inp)
    return PR.eps_branches(sd, cfg, lay, W, inp["x_T"], T_EPS, cond, unc if with_cfg else None, list(blocks))


def change(blocks, b, h, w):
    _, e_c, e_p = branches(blocks, b, h, w)
    return float(np.abs(e_c - e_p).max() / np.abs(e_c).max())


# ------------------------------------------------------------------------------------------------ the grammar
def test_block_table_is_diffusers_numbering():
    down, up, mid = pag_block_table(W.SD15)
    assert down == [[0, 1], [2, 3], [4, 5], []] and up == [[], [6, 7, 8], [9, 10, 11], [12, 13, 14]] and mid == 15
    assert PR.block_prefixes(W.SD15, W)[mid] == "middle_block.1." and len(PR.block_prefixes(W.SD15, W)) == 16
    from prompt_diffusion_amd import ip_adapter as IP
    assert PR.block_prefixes(W.SD15, W) == IP.block_prefixes(W.SD15, prefix="")


@pytest.mark.parametrize("names,blocks", [
    ("mid", [15]), ("down", range(6)), ("up", range(6, 15)), (["mid"], [15]),
    ("down.block_0", [0, 1]), ("down_blocks.0", [0, 1]), ("down.block_2", [4, 5]), ("down_blocks.2", [4, 5]),
    ("up.block_1", [6, 7, 8]), ("up_blocks.1", [6, 7, 8]), ("up.block_3", [12, 13, 14]), ("up_blocks.3", [12, 13, 14]),
    ("mid.block_0", [15]), ("mid_block", [15]),
    ("down.block_1.attentions_1", [3]), ("down_blocks.1.attentions.1", [3]), ("down.block_1.attentions.0", [2]),
    ("up.block_2.attentions_2", [11]), ("up_blocks.2.attentions.0", [9]), ("mid.block_0.attentions_0", [15]), ("mid_block.attentions.0", [15]),
    (["down.block_2", "mid", "up.block_1"], [4, 5, 15, 6, 7, 8]), (["mid", "mid_block"], [15]),
])
def test_grammar(names, blocks):
    assert parse_pag_layers(names, W.SD15) == sum(1 << j for j in set(blocks))
    assert parse_pag_layers(names, W.TINY) == sum(1 << j for j in set(blocks))      # same topology


@pytest.mark.parametrize("name", ["down.block_3", "down_blocks.3", "up.block_0", "up_blocks.0", "down.block_4", "up_blocks.7", "mid.block_1",
                                  "down.block_1.attentions_2", "up.block_1.attentions.3", "mid_block.attentions.1", "down.attentions_0",
                                  "middle", "down.block_", "blocks.1", "", "up.block_1.attn_0"])
def test_grammar_refusals(name):
    with pytest.raises(ValueError, match=re.escape(repr(name))):
        parse_pag_layers(["mid", name], W.SD15)


def test_grammar_refuses_other_types():
    with pytest.raises(ValueError):
        parse_pag_layers([15], W.SD15)


# ------------------------------------------------------------------------------------------------ the restatement
def test_guidance_restatement():
    r = np.random.default_rng(3)
    e_u, e_c, e_p = (r.standard_normal((2, 4, 8, 8)).astype(np.float32) for _ in range(3))
    two = (e_u + np.float32(7.5) * (e_c - e_u)).astype(np.float32)
    assert np.array_equal(PR.guide(e_u, e_c, e_p, 7.5, 0.0), two)
    assert np.array_equal(PR.guide(None, e_c, e_p, 1.0, 0.0), e_c)
    g = PR.guide(e_u, e_c, e_p, 7.5, 3.0)
    assert g.dtype == np.float32 and np.array_equal(g, two + np.float32(3.0) * (e_c - e_p))
    assert np.array_equal(PR.guide(None, e_c, e_p, 9.0, 0.37), e_c + np.float32(0.37) * (e_c - e_p))
    assert np.array_equal(PR.guide(e_u, e_c, e_c, 7.5, 3.0), two)      # an unperturbed branch adds nothing


def test_adaptive_scale():
    assert PR.pag_scale_at(3.0, 0.0, 1) == np.float32(3.0)
    a = float(np.float32(0.004))
    for t in (999, 801, 601, 401, 251, 250, 201, 1):
        want = max(3.0 - a * (1000.0 - t), 0.0)
        assert PR.pag_scale_at(3.0, 0.004, t) == np.float32(want), t
    assert PR.pag_scale_at(3.0, 0.004, 801) > 0 and PR.pag_scale_at(3.0, 0.004, 201) == 0      # the clamp: 3 - 0.004 * 799 < 0
    assert PR.pag_scale_at(3.0, 0.004, 1000) == np.float32(3.0)


@pytest.mark.parametrize("blocks,b,h,w,modes", GPU_CASES)
def test_gpu_cases_have_teeth(blocks, b, h, w, modes):
    c = change(blocks, b, h, w)
    print(f"[pag teeth] blocks {blocks} at {b} x {h} x {w}: max |e_c - e_p| / max |e_c| = {c:.3e}")
    for m in modes:
        need = 5 * TOL_ORACLE[m]
        if m == "bf16" and c < need:
            print(f"[pag teeth] bf16: {c / TOL_ORACLE[m]:.2f} x its bound {TOL_ORACLE[m]} (5 x is out of reach of every layer set)")
            need = 2 * TOL_ORACLE[m]
        assert c >= need, (m, c, need)


def test_no_layer_set_reaches_5x_bf16():
    """... which is why bf16 is held to 2 x: the set of every block moves eps by less than 0.75 too"""
    assert change(ALL, B, HW, HW) < 5 * TOL_ORACLE["bf16"]
    assert change(ALL, B, HW, HW) > change(MID, B, HW, HW)


def test_mid_at_8x8_is_exactly_the_plain_evaluation():
    e_u, e_c, e_p = branches(MID, B, 8, 8)
    assert np.array_equal(e_c, e_p)
    cfg, sd, lay = tiny()
    inp = W.synth_inputs(cfg, B, 8, 8)
    cond, unc = conds(inp)
    plain = PR.ddim_pag(sd, cfg, lay, W, S, inp["x_T"], cond, unc, CFG_SCALE, PAG_SCALE, [], steps_limit=2)
    got = PR.ddim_pag(sd, cfg, lay, W, S, inp["x_T"], cond, unc, CFG_SCALE, PAG_SCALE, list(MID), steps_limit=2)
    # (e_c - e_p is exactly 0 and adding p * 0 changes nothing: the trajectory is that of the restatement with no layer perturbed ...
    assert np.array_equal(got[-1], plain[-1])
    # ... which is the oracle's own CFG loop up to the summation order of a batch of three instead of two)
    ref, _, _ = O.ddim_sampling(sd, cfg, lay, S, inp["x_T"], cond, unc, CFG_SCALE, steps_limit=2)
    assert np.abs(got[-1] - ref).max() <= 2e-5 * np.abs(ref).max()


def test_restatement_without_layers_is_the_oracle():
    cfg, sd, lay = tiny()
    inp = W.synth_inputs(cfg, 1, 8, 8)
    cond, unc = conds(inp)
    e_u, e_c, e_p = PR.eps_branches(sd, cfg, lay, W, inp["x_T"], T_EPS, cond, unc, [])
    out = O.apply_model(sd, cfg, lay, np.concatenate([inp["x_T"]] * 2), np.full((2,), T_EPS, np.int64),
                        np.concatenate([inp["ctx_uncond"], inp["ctx_cond"]]), np.concatenate([inp["pair"]] * 2), np.concatenate([inp["query"]] * 2))
    assert np.array_equal(e_p, e_c)
    for got, ref in ((e_u, out[:1]), (e_c, out[1:])):      # (a batch of three against a batch of two: the summation order of the BLAS calls)
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


def test_guess_mode_restatement_perturbs_the_conditional_residuals():
    cfg, sd, lay = tiny()
    inp = W.synth_inputs(cfg, 1, 8, 8)
    cond, unc = conds(inp)
    g = PR.eps_branches(sd, cfg, lay, W, inp["x_T"], T_EPS, cond, unc, list(WIDE), guess_mode=True)
    n = PR.eps_branches(sd, cfg, lay, W, inp["x_T"], T_EPS, cond, unc, list(WIDE))
    assert not np.array_equal(g[0], n[0]) and np.array_equal(g[1], n[1]) and np.array_equal(g[2], n[2])


# ------------------------------------------------------------------------------------------------ the pipelines, on a stub engine
class _StubEngine:
    cfg = W.TINY

    def __init__(self):
        self.state, self.calls, self.ended = None, [], 0

    @property
    def pag(self):
        return self.state

    def set_pag(self, scale, layers, adaptive_scale=0.0):
        self.calls.append((scale, layers, adaptive_scale))
        self.state = (float(scale), float(adaptive_scale), int(layers)) if scale and layers else None

    def disable_pag(self):
        self.calls.append(None)
        self.state = None

    def sample_end(self):
        self.ended += 1


class _Pipe(PAGMixin):
    def __init__(self, layers="mid"):
        self.engine = _StubEngine()
        self.set_pag_applied_layers(layers)


def test_mixin_properties_and_bracket():
    p = _Pipe()
    assert p.pag_applied_layers == ["mid"] and p._pag_mask == 1 << 15
    assert (p.pag_scale, p.pag_adaptive_scale, p.do_perturbed_attention_guidance, p.do_pag_adaptive_scaling) == (0.0, 0.0, False, False)
    with p._pag_of_call(0.0, 0.0):
        assert p.engine.calls == []                      # the default leaves the engine alone
    with p._pag_of_call(3.0, 0.0):
        assert p.engine.pag == (3.0, 0.0, 1 << 15) and p.do_perturbed_attention_guidance and not p.do_pag_adaptive_scaling
    assert p.engine.pag is None
    with p._pag_of_call(3.0, 0.004):
        assert p.do_pag_adaptive_scaling and p.pag_adaptive_scale == 0.004
    p.engine.set_pag(1.5, 3, 0.25)                        # state set on the engine directly comes back after the call ...
    with p._pag_of_call(3.0, 0.0):
        assert p.engine.pag == (3.0, 0.0, 1 << 15)
    assert p.engine.pag == (1.5, 0.25, 3)
    with pytest.raises(RuntimeError):                      # ... also after a call that raised (and its session is ended first)
        with p._pag_of_call(2.0, 0.0):
            raise RuntimeError("boom")
    assert p.engine.pag == (1.5, 0.25, 3) and p.engine.ended == 1
    for bad in ((-1.0, 0.0), (3.0, -0.5), (float("nan"), 0.0)):
        n = len(p.engine.calls)
        with pytest.raises(ValueError, match="pag_scale"):
            with p._pag_of_call(*bad):
                pass
        assert len(p.engine.calls) == n
    p.set_pag_applied_layers(["down.block_2", "mid", "up.block_1"])
    assert p._pag_mask == (1 << 4 | 1 << 5 | 1 << 15 | 1 << 6 | 1 << 7 | 1 << 8)
    with pytest.raises(ValueError, match="up.block_0"):
        p.set_pag_applied_layers(["mid", "up.block_0"])
    assert p.pag_applied_layers == ["down.block_2", "mid", "up.block_1"]      # a refused list changes nothing


def test_sd15_pipelines_take_the_arguments():
    import inspect
    from prompt_diffusion_amd import pipeline as P
    for cls in (P.PromptDiffusionPipeline, P.PromptDiffusionImg2ImgPipeline, P.PromptDiffusionInpaintPipeline):
        sig = inspect.signature(cls.__call__).parameters
        assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0
        assert issubclass(cls, PAGMixin)
    assert inspect.signature(P.PromptDiffusionPipeline.__init__).parameters["pag_applied_layers"].default == "mid"
    pipe = P.PromptDiffusionPipeline(_StubEngine(), pag_applied_layers=["mid", "up.block_1"])
    assert pipe._pag_mask == (1 << 15 | 1 << 6 | 1 << 7 | 1 << 8)
    with pytest.raises(ValueError, match="down.block_3"):
        P.PromptDiffusionPipeline(_StubEngine(), pag_applied_layers="down.block_3")
    with pytest.raises(ValueError, match="pag_scale"):
        pipe(prompt_embeds=np.zeros((1, 77, 96), np.float32), pag_scale=-1.0)
    assert pipe.engine.calls == []


def test_sd3_pipeline_refuses():
    from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as P3
    with pytest.raises(NotImplementedError, match="pag_scale"):
        P3.__call__(None, prompt="x", pag_scale=3.0)


def test_header_documents_the_state():
    h = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    assert re.search(r"int pd_set_pag\(pd_engine\* e, float scale, float adaptive_scale, uint32_t layer_mask\);", h)
    assert re.search(r"int pd_get_pag\(pd_engine\* e, float out\[2\], uint32_t\* layer_mask\);", h)
    from prompt_diffusion_amd import engine as E
    assert "pag_fork" not in dict(E.option_table())       # a switch outside the enumerated table (options.h: kSwitches)
