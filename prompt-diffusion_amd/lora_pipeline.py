"""The adapter surface both pipelines share (diffusers' LoraLoaderMixin / SD3LoraLoaderMixin): named adapters, the active set with
its weights, and the lazy merge on the device before a call.  A pipeline supplies ``self.engine`` (lora_add, lora_add_ex,
lora_set_scales, lora_remove) and two hooks: ``_lora_parse(src)`` -> {engine tensor name: lora.Adapter} and
``_lora_components(names)`` -> {component: bool}, which may refuse (a text-encoder adapter next to a caller-supplied encoder)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Union


class AdapterMixin:
    def _lora_init(self):
        # name -> {"id", <component>: bool ...}; the active set with its weights; the scales the engine holds merged (None: never merged)
        self._lora_adapters: Dict[str, Dict[str, Any]] = {}
        self._lora_active: Dict[str, float] = {}
        self._lora_next_id = 0
        self._lora_merged: Optional[List[float]] = None

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, **kwargs):
        """Load an adapter (dict of arrays or a local .safetensors file): plain LoRA pairs, Tucker LoCon, LoHa, LoKr, each
        optionally under a DoRA magnitude.  It joins the active set with weight 1.0; the weights are merged on the device at the
        next call."""
        from . import lora as L
        if kwargs:
            raise NotImplementedError(f"load_lora_weights: unsupported arguments {sorted(kwargs)}")
        name = adapter_name if adapter_name is not None else f"default_{self._lora_next_id}"
        if name in self._lora_adapters:
            raise ValueError(f"Adapter name {name} already in use")
        records = self._lora_parse(pretrained_model_name_or_path_or_dict)
        comps = self._lora_components(list(records))
        aid = self._lora_next_id
        added = False
        try:
            for k, rec in records.items():
                L.add_to_engine(self.engine, aid, k, rec)
                added = True
        except Exception:
            if added:
                self.engine.lora_remove(aid)
            raise
        self._lora_next_id += 1
        self._lora_adapters[name] = dict(id=aid, **comps)
        self._lora_active[name] = 1.0

    def set_adapters(self, adapter_names: Union[str, List[str]], adapter_weights: Optional[Union[float, List[float]]] = None):
        """Make exactly these adapters active, with these weights (default 1.0)."""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None:
            weights = [1.0] * len(names)
        elif isinstance(adapter_weights, (int, float)):
            weights = [float(adapter_weights)] * len(names)
        else:
            weights = [float(w) for w in adapter_weights]
        if len(weights) != len(names):
            raise ValueError(f"Length of adapter names {len(names)} is not equal to the length of their weights {len(weights)}.")
        for n in names:
            if n not in self._lora_adapters:
                raise ValueError(f"Adapter name(s) {n} not in the list of present adapters: {sorted(self._lora_adapters)}.")
        self._lora_active = dict(zip(names, weights))

    def get_active_adapters(self) -> List[str]:
        return list(self._lora_active)

    def get_list_adapters(self) -> Dict[str, List[str]]:
        out: Dict[str, List[str]] = {}
        for comp in self._lora_component_names:
            names = [n for n, a in self._lora_adapters.items() if a[comp]]
            if names:
                out[comp] = names
        return out

    def delete_adapters(self, adapter_names: Union[str, List[str]]):
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        for n in names:
            if n not in self._lora_adapters:
                raise ValueError(f"Adapter name {n} not in the list of present adapters: {sorted(self._lora_adapters)}.")
        for n in names:
            aid = self._lora_adapters.pop(n)["id"]
            self._lora_active.pop(n, None)
            self.engine.lora_remove(aid)
            if self._lora_merged is not None and aid < len(self._lora_merged):
                self._lora_merged[aid] = 0.0

    def unload_lora_weights(self):
        if self._lora_adapters:
            self.engine.lora_remove(-1)
        self._lora_adapters.clear()
        self._lora_active.clear()
        self._lora_merged = None

    def _lora_scales(self, scale: float) -> List[float]:
        """Effective multiplier per adapter id: its set_adapters weight x the call's scale (cross_attention_kwargs /
        joint_attention_kwargs; diffusers' scale_lora_layers); 0 for inactive ids."""
        out = [0.0] * self._lora_next_id
        for n, w in self._lora_active.items():
            out[self._lora_adapters[n]["id"]] = float(w) * float(scale)
        return out

    def _lora_sync(self, scale: float):
        """Merge on the device only when the effective scales differ from the merged ones."""
        want = self._lora_scales(scale)
        if self._lora_merged is None and not any(want):
            return
        if want != self._lora_merged:
            self.engine.lora_set_scales(want)
            self._lora_merged = want
