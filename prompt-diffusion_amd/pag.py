"""Perturbed-attention guidance (PAG, arXiv:2403.17377) on the host side: diffusers' `pag_applied_layers` names -> the engine's block
mask (Engine.set_pag / pd_set_pag), and the per-call bracket of the SD1.5 pipelines.

The engine numbers the UNet's transformer blocks as pd_ip_adapter_configure does: the encoder's, then the decoder's, then the middle
block.  diffusers names them by module path; both of its generations are accepted:

    "mid", "down", "up"                              every block of that part
    "down.block_i"   or  "down_blocks.i"             the attentions of down block i
    "up.block_i"     or  "up_blocks.i"               the attentions of up block i
    "mid.block_0"    or  "mid_block"                 the middle block
    ... each optionally followed by ".attentions_j" or ".attentions.j": attention j of that block alone

In diffusers' numbering of this architecture `down_blocks` i holds num_res_blocks attentions where the resolution of level i is one
of cfg.attention_resolutions (SD1.5: down blocks 0-2, two each; down block 3 has none), and `up_blocks` i, counted from the lowest
resolution, holds num_res_blocks + 1 where level L-1-i is (SD1.5: up blocks 1-3, three each; up block 0 has none).  A name that
selects no self-attention is an error, as in diffusers.  Parity with diffusers is unpinned (it is not installed where the tests run):
the grammar and the block order are restated from its PAGMixin._set_pag_attn_processor and UNet2DConditionModel."""
import contextlib
import re
from typing import Iterable, List, Union

__all__ = ["parse_pag_layers", "pag_block_table", "PAGMixin"]


def pag_block_table(cfg):
    """(down, up, mid): down[i] / up[i] = the engine block indices of the attentions of diffusers' down_blocks[i] / up_blocks[i]
    (empty where the block has none), mid = the middle block's index."""
    levels = len(cfg.channel_mult)
    has = [(1 << l) in tuple(cfg.attention_resolutions) for l in range(levels)]
    down, up, j = [], [], 0
    for l in range(levels):
        n = cfg.num_res_blocks if has[l] else 0
        down.append(list(range(j, j + n)))
        j += n
    for i in range(levels):
        n = cfg.num_res_blocks + 1 if has[levels - 1 - i] else 0
        up.append(list(range(j, j + n)))
        j += n
    return down, up, j


_NAME = re.compile(r"^(?:(down|up)(?:\.block_(\d+)|_blocks\.(\d+))?|(mid)(?:\.block_(\d+))?|(mid_block))(?:\.attentions[_.](\d+))?$")


def parse_pag_layers(layers: Union[str, Iterable[str]], cfg) -> int:
    """The engine's layer mask of diffusers' pag_applied_layers (a name or a list of names; the grammar is in the module docstring).
    ValueError names the entry that is malformed or selects no self-attention."""
    if isinstance(layers, str):
        layers = [layers]
    layers = list(layers)
    down, up, mid = pag_block_table(cfg)
    mask = 0
    for name in layers:
        if not isinstance(name, str):
            raise ValueError(f"pag_applied_layers: expected layer names (str), got {name!r}")
        m = _NAME.match(name.strip())
        if not m:
            raise ValueError(f"pag_applied_layers: cannot parse {name!r}")
        part, i1, i2, midp, mid_i, midb, att = m.groups()
        if part:
            table = down if part == "down" else up
            idx = i1 if i1 is not None else i2
            if idx is None:
                if att is not None:
                    raise ValueError(f"pag_applied_layers: {name!r} names an attention without a block")
                sel = [j for blk in table for j in blk]
            else:
                i = int(idx)
                sel = table[i] if i < len(table) else []
        else:
            if mid_i is not None and int(mid_i) != 0:
                sel = []
            else:
                sel = [mid]
        if att is not None and (part or midp or midb):
            a = int(att)
            sel = sel[a:a + 1]
        if not sel:
            raise ValueError(f"pag_applied_layers: {name!r} selects no self-attention layer of this UNet")
        for j in sel:
            mask |= 1 << j
    return mask


class PAGMixin:
    """`pag_applied_layers`, the four properties of diffusers' PAGMixin and the bracket of a call (PromptDiffusionPipeline._run)."""
    _pag_scale = 0.0
    _pag_adaptive_scale = 0.0
    _pag_mask = None      # the engine's mask of pag_applied_layers; None: not parsed yet (a pipeline built around no engine configuration)
    pag_applied_layers: List[str] = []

    def set_pag_applied_layers(self, pag_applied_layers: Union[str, List[str]]):
        """The names are checked against the engine's UNet here where the pipeline has one, else at the first call that uses them."""
        names = [pag_applied_layers] if isinstance(pag_applied_layers, str) else list(pag_applied_layers)
        cfg = getattr(getattr(self, "engine", None), "cfg", None)
        mask = parse_pag_layers(names, cfg) if cfg is not None else None
        self._pag_mask, self.pag_applied_layers = mask, names

    def _pag_layer_mask(self) -> int:
        if self._pag_mask is None:
            self._pag_mask = parse_pag_layers(self.pag_applied_layers, self.engine.cfg)
        return self._pag_mask

    @property
    def pag_scale(self) -> float:
        return self._pag_scale

    @property
    def pag_adaptive_scale(self) -> float:
        return self._pag_adaptive_scale

    @property
    def do_pag_adaptive_scaling(self) -> bool:
        return self._pag_adaptive_scale > 0 and self._pag_scale > 0 and len(self.pag_applied_layers) > 0

    @property
    def do_perturbed_attention_guidance(self) -> bool:
        return self._pag_scale > 0 and len(self.pag_applied_layers) > 0

    @contextlib.contextmanager
    def _pag_of_call(self, pag_scale: float, pag_adaptive_scale: float):
        """The engine's PAG state for the duration of a call: set before the body, put back afterwards, exception or not.  A call
        with pag_scale 0 leaves the engine as it is (PAG set on the engine directly then applies, as FreeU does)."""
        pag_scale, pag_adaptive_scale = float(pag_scale), float(pag_adaptive_scale)
        if not pag_scale >= 0.0 or not pag_adaptive_scale >= 0.0:
            raise ValueError(f"`pag_scale` and `pag_adaptive_scale` must be >= 0, got {pag_scale} and {pag_adaptive_scale}")
        self._pag_scale, self._pag_adaptive_scale = pag_scale, pag_adaptive_scale
        if not self.do_perturbed_attention_guidance:
            yield
            return
        eng = self.engine
        before = eng.pag
        eng.set_pag(pag_scale, self._pag_layer_mask(), pag_adaptive_scale)
        try:
            yield
        except BaseException:
            try:
                eng.sample_end()    # a body that raised inside a session: the state below cannot be put back while one is active
            except Exception:
                pass
            raise
        finally:
            if before is None:
                eng.disable_pag()
            else:
                eng.set_pag(before[0], before[2], before[1])
