#!/usr/bin/env python3
"""Generate tests/golden/long_prompt.npz from the REFERENCE's long-prompt path (cldm/hack.py: hack_everything ->
_hacked_clip_forward), which tokenises without truncation, splits the ids into three 75-token windows, wraps each in BOS / EOS, pads to
77, runs them through CLIP as one batch and concatenates to a [B, 231, C] context.

Runs only where a checkout of the reference exists (--reference DIR).  _hacked_clip_forward is called unbound on a shim that carries
what it reads: a tokenizer (tests/long_prompt_stub.py -- the real vocabulary cannot be fetched offline), `transformer` (transformers'
CLIPTextModel built from the TINY config with the seeded weights of prompt-diffusion_amd/weights.py, as make_golden.py's clip case
does), clip_skip and device.  The window ids it feeds the transformer are recorded from that call.  Data only: token lists, window ids,
outputs (of the clip_skip run every second token row: `z_rows`).

Usage: python tests/golden/make_golden_long_prompt.py --reference DIR
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def load_weights_module():
    spec = importlib.util.spec_from_file_location("pd_weights", os.path.join(ROOT, "prompt-diffusion_amd", "weights.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["pd_weights"] = mod
    spec.loader.exec_module(mod)
    return mod


def tiny_clip(cfg, W):
    from transformers import CLIPTextConfig, CLIPTextModel
    tc = CLIPTextConfig(vocab_size=cfg.text_vocab, hidden_size=cfg.context_dim, intermediate_size=cfg.text_ff,
                        num_hidden_layers=cfg.text_layers, num_attention_heads=cfg.text_heads,
                        max_position_embeddings=cfg.context_len, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                        bos_token_id=cfg.text_vocab - 2, eos_token_id=cfg.text_vocab - 1, pad_token_id=cfg.text_vocab - 1)
    m = CLIPTextModel(tc).eval()
    own = m.state_dict()
    mapped = {}
    for k, v in W.synth_text_state_dict(cfg).items():
        kk = k[len(W.TEXT_PREFIX):]
        kk = kk if kk in own else "text_model." + kk
        mapped[kk] = torch.from_numpy(v)
    missing = [k for k in own if k not in mapped and "position_ids" not in k]
    assert not missing, missing
    m.load_state_dict(mapped, strict=False)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import transformers.models.clip.modeling_clip  # noqa: F401  (before the stubs: transformers probes torchvision while it imports)
    from transformers import CLIPTextModel, CLIPTokenizer, T5EncoderModel, T5Tokenizer  # noqa: F401
    from tests.golden.make_golden import install_stubs
    install_stubs()
    sys.modules.setdefault("open_clip", types.ModuleType("open_clip"))    # imported by ldm/modules/encoders/modules.py, unused here
    from cldm import hack
    from tests.long_prompt_stub import TOKEN_COUNTS, StubTokenizer, prompt_of

    W = load_weights_module()
    cfg = W.TINY
    tok = StubTokenizer(cfg.text_vocab)
    prompts = [prompt_of(n, 100 + i, cfg.text_vocab) for i, n in enumerate(TOKEN_COUNTS)]
    model = tiny_clip(cfg, W)
    fed = []

    class Recorder(torch.nn.Module):          # records the ids _hacked_clip_forward feeds, then the model itself
        def __init__(self, inner):
            super().__init__()
            self.inner = inner
            # (transformers 5 keeps final_layer_norm on the model itself, 4.x under text_model: the reference reads the latter)
            fln = [mod for name, mod in inner.named_modules() if name.endswith("final_layer_norm")][0]
            self.text_model = types.SimpleNamespace(final_layer_norm=fln)

        def forward(self, input_ids, **kw):
            fed.append(input_ids.detach().cpu().numpy().copy())
            return self.inner(input_ids=input_ids.long(), **kw)

    res = dict(token_counts=np.asarray(TOKEN_COUNTS, np.int64), vocab=np.int64(cfg.text_vocab))
    raw = tok(prompts, truncation=False, add_special_tokens=False)["input_ids"]
    res["raw_len"] = np.asarray([len(r) for r in raw], np.int64)
    res["raw_tokens"] = np.full((len(raw), max(TOKEN_COUNTS)), -1, np.int32)
    for b, r in enumerate(raw):
        res["raw_tokens"][b, :len(r)] = r
    for skip in (0, 3):                        # the reference's own count: 0 = last layer, 3 = hidden_states[-3]
        shim = types.SimpleNamespace(tokenizer=tok, transformer=Recorder(model), clip_skip=skip, device="cpu")
        with torch.no_grad():
            z = hack._hacked_clip_forward(shim, prompts).float().numpy()
        assert z.shape == (len(prompts), 231, cfg.context_dim)
        if skip == 0:
            res["z"] = z                             # the full [B, 231, C] output
        else:
            # the longest prompt, every second token row (all three windows stay covered; keeps the file at a few hundred KB)
            rows = np.arange(0, 231, 2)
            res["z_rows"] = rows.astype(np.int64)
            res["z_ref_clip_skip3"] = z[-1:, rows]
    ids = fed[0].reshape(len(prompts), 3, 77)
    assert all((f.reshape(ids.shape) == ids).all() for f in fed)
    res["window_ids"] = ids.astype(np.int32)
    path = os.path.join(a.out, "long_prompt.npz")
    np.savez_compressed(path, **res)
    print(f"[golden] long_prompt.npz: {os.path.getsize(path) / 1024:.0f} KB, |z| mean {np.abs(res['z']).mean():.4f}")


if __name__ == "__main__":
    main()
