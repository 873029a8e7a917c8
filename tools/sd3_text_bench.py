"""Times the SD3 text encoders on the engine at the real shapes with random weights: CLIP-L, CLIP-G, T5-XXL at Lt = 256 and the whole
encode_prompt, at B = 2 and B = 16.  If transformers is importable, the same three modules in torch on the same GPU, same dtype.

    python tools/sd3_text_bench.py [--precision bf16] [--batches 2,16] [--t5-len 256] [--min-seconds 0.5] [--no-torch]

Method: ids and outputs live on the device; every engine call ends in a stream synchronise, so a host clock around it times the device work
plus its launches.  Each case is warmed up (3 calls), then timed call by call until --min-seconds of work and at least 5 calls are in; the
figure is the median.  FLOP/s = the contraction FLOPs the model needs (2 M N K of every Linear, 4 L^2 dh per head for attention, causal
attention counted in full) over that time: an end-to-end rate, not a kernel's share of peak.  Compare numbers from one run on one box only."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prompt_diffusion_amd import sd3  # noqa: E402


def clip_flops(c, B):
    L = c.max_positions
    return B * L * c.layers * (2.0 * (4 * c.hidden * c.hidden + 2 * c.hidden * c.ff) + 4.0 * L * c.hidden) + 2.0 * B * c.hidden * c.proj_dim


def t5_flops(t, B, L):
    inner = t.heads * t.d_kv
    return B * L * t.layers * (2.0 * (4 * t.d_model * inner + 3 * t.d_model * t.d_ff) + 4.0 * L * inner)


def timed(fn, sync, min_seconds):
    for _ in range(3):
        fn()
    sync()
    ts, t_end = [], time.perf_counter() + min_seconds
    while len(ts) < 5 or (time.perf_counter() < t_end and len(ts) < 200):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--t5-len", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sd3_text_bench: no GPU; this tool only measures on one")
    cfg, Lt = sd3.SD3_MEDIUM_TEXT, a.t5_len
    net = sd3.SD3Config(heads=2, head_dim=64, layers=1, cn_layers=0, joint_dim=cfg.joint_dim, pooled_dim=cfg.pooled_dim, pos_embed_max_size=16)
    eng = sd3.SD3Engine(net, precision=a.precision)
    eng.configure_text(cfg)
    eng.init_random_weights(1)
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in [int(x) for x in a.batches.split(",")]:
        ids_l = torch.randint(0, cfg.clip_l.vocab, (B, 77), device="cuda", dtype=torch.int32, generator=g)
        ids_g = torch.randint(0, cfg.clip_g.vocab, (B, 77), device="cuda", dtype=torch.int32, generator=g)
        ids_t = torch.randint(0, cfg.t5.vocab, (B, Lt), device="cuda", dtype=torch.int32, generator=g)
        fl = {"clip_l": clip_flops(cfg.clip_l, B), "clip_g": clip_flops(cfg.clip_g, B), "t5": t5_flops(cfg.t5, B, Lt)}
        fl["encode_prompt"] = sum(fl.values())
        cases = {"clip_l": lambda: eng.text_encoder("clip_l", ids_l), "clip_g": lambda: eng.text_encoder("clip_g", ids_g),
                 "t5": lambda: eng.text_encoder("t5", ids_t), "encode_prompt": lambda: eng.encode_prompt_ids(ids_l, ids_g, ids_t)}
        for name, fn in cases.items():
            ms, n = timed(fn, lambda: None, a.min_seconds)      # the engine call itself ends in a stream synchronise
            rows.append(dict(impl="engine", precision=a.precision, case=name, B=B, Lt=Lt, ms=round(ms, 3), calls=n, tflops=round(fl[name] / ms / 1e9, 1)))
            print(json.dumps(rows[-1]), flush=True)
    eng.close()
    del eng
    if not a.no_torch:
        try:
            from transformers import CLIPTextConfig, CLIPTextModelWithProjection, T5Config, T5EncoderModel
        except Exception as ex:   # the torch columns are optional
            print(json.dumps(dict(impl="torch", skipped=f"transformers not importable: {ex}")))
            return
        dt = torch.bfloat16 if a.precision == "bf16" else torch.float16
        torch.cuda.empty_cache()

        def clip(c):
            with torch.device("cuda"):
                return CLIPTextModelWithProjection(CLIPTextConfig(
                    vocab_size=c.vocab, hidden_size=c.hidden, intermediate_size=c.ff, projection_dim=c.proj_dim, num_hidden_layers=c.layers,
                    num_attention_heads=c.heads, max_position_embeddings=c.max_positions, hidden_act=c.act, eos_token_id=c.eos_token_id)).to(dt).eval()
        t = cfg.t5
        mods = {"clip_l": lambda: clip(cfg.clip_l), "clip_g": lambda: clip(cfg.clip_g)}

        def t5():
            with torch.device("cuda"):
                return T5EncoderModel(T5Config(vocab_size=t.vocab, d_model=t.d_model, d_kv=t.d_kv, d_ff=t.d_ff, num_layers=t.layers, num_heads=t.heads,
                                               feed_forward_proj="gated-gelu", is_encoder_decoder=False, use_cache=False)).to(dt).eval()
        mods["t5"] = t5
        for name, make in mods.items():
            m = make()
            for B in [int(x) for x in a.batches.split(",")]:
                c = {"clip_l": cfg.clip_l, "clip_g": cfg.clip_g}.get(name)
                ids = torch.randint(0, (c.vocab if c else t.vocab), (B, 77 if c else Lt), device="cuda", generator=g)
                fl = clip_flops(c, B) if c else t5_flops(t, B, Lt)
                with torch.no_grad():
                    fn = (lambda: m(ids, output_hidden_states=True)) if c else (lambda: m(ids))
                    ms, n = timed(fn, torch.cuda.synchronize, a.min_seconds)
                rows.append(dict(impl="torch", precision=a.precision, case=name, B=B, Lt=Lt, ms=round(ms, 3), calls=n, tflops=round(fl / ms / 1e9, 1)))
                print(json.dumps(rows[-1]), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
