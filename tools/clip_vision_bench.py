"""CLIP image tower: preprocessing + tower + safety check per batch on seeded random weights, one MI355X.

    python tools/clip_vision_bench.py [--calls 20] [--warmup 3] [--timeout 300] [--out profiles/clip_vision_bench.json]

For the ViT-L/14 safety tower (CLIP_VIT_L14_SAFETY: uint8 pictures -> image_embeds -> flags) and the ViT-H/14 image encoder
(CLIP_VIT_H14: uint8 pictures -> image_embeds), B = 1 and 8 pictures of 512 x 512, f16 and bf16, each leg a child process under its
own time limit: the median wall time of the whole call (CUDA uint8 tensor in; the call ends in a stream synchronise), the launches per
call, and the same work in transformers' eager CLIPVisionModelWithProjection in the same process on the same GPU in the same dtype
(bicubic resize + crop + normalise in torch on the device standing in for the processor, the concept check in torch) where
transformers is importable -- "not measured" otherwise.  The two sides hold different random weights: only times are compared.
Prints one JSON line per leg and writes them all to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(run, sync, calls, warmup):
    for _ in range(warmup):
        run()
    sync()
    ts = []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        run()
        sync()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 4), round(1e3 * min(ts), 4), round(1e3 * max(ts), 4)


def child(args):
    import torch

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W

    cfg = W.CLIP_VIT_L14_SAFETY if args.tower == "safety" else W.CLIP_VIT_H14
    e = E.Engine(W.TINY, device=0, precision=args.precision)
    if args.tower == "safety":
        e.configure_safety_checker(cfg)
    else:
        e.configure_clip_vision(cfg)
    e._check(e.lib.pd_init_random_weights(e._h, 11))
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    sync = torch.cuda.synchronize
    run = (lambda: e.safety_check(x)) if args.tower == "safety" else (lambda: e.clip_vision(x, "embeds", prefix=cfg.prefix))
    run()
    l0 = e.stat("launches")
    run()
    launches = e.stat("launches") - l0
    med, lo, hi = _median_ms(run, sync, args.calls, args.warmup)
    prep = _median_ms(lambda: e.clip_preprocess(x, cfg.image_size, cfg.patch, what="patches"), sync, args.calls, args.warmup)[0]
    rec = dict(tower=args.tower, model="ViT-L/14" if args.tower == "safety" else "ViT-H/14", precision=args.precision, batch=B, picture=S,
               calls=args.calls, engine_ms=med, engine_ms_min=lo, engine_ms_max=hi, engine_preprocess_ms=prep, launches_per_call=int(launches),
               eager_ms="not measured")
    try:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    except ImportError:
        print(json.dumps(rec))
        return
    dt = torch.float16 if args.precision == "f16" else torch.bfloat16
    hc = CLIPVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.ff, projection_dim=cfg.proj_dim, num_hidden_layers=cfg.layers,
                          num_attention_heads=cfg.heads, image_size=cfg.image_size, patch_size=cfg.patch, hidden_act=cfg.act,
                          attn_implementation="eager")
    torch.manual_seed(0)
    m = CLIPVisionModelWithProjection(hc).eval().to("cuda", dt)
    mean = torch.tensor(cfg.mean, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(cfg.std, device="cuda").view(1, 3, 1, 1)
    concepts = torch.nn.functional.normalize(torch.randn(20, cfg.proj_dim, device="cuda"), dim=-1)
    thr = torch.full((20,), 0.5, device="cuda")

    def eager():
        with torch.no_grad():
            f = x.permute(0, 3, 1, 2).float()
            f = torch.nn.functional.interpolate(f, size=(cfg.image_size, cfg.image_size), mode="bicubic", antialias=True, align_corners=False)
            pv = ((f.round().clamp(0, 255) / 255 - mean) / std).to(dt)
            emb = m(pv).image_embeds.float()
            if args.tower == "safety":
                return ((torch.nn.functional.normalize(emb, dim=-1) @ concepts.T - thr) > 0).any(1).cpu()
            return emb

    rec["eager_ms"], rec["eager_ms_min"], rec["eager_ms_max"] = _median_ms(eager, sync, args.calls, args.warmup)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tower", default="safety")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = []
    for tower in ("safety", "image_encoder"):
        for prec in ("f16", "bf16"):
            for B in (1, 8):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tower", tower, "--precision", prec, "--batch", str(B),
                       "--calls", str(args.calls), "--warmup", str(args.warmup), "--size", str(args.size)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                except subprocess.TimeoutExpired:
                    print(f"leg {tower} {prec} B={B}: time limit; stopping", file=sys.stderr)
                    sys.exit(124)
                if r.returncode != 0:     # a failed leg ends the run: nothing more is started on the card
                    print(r.stderr[-2000:], file=sys.stderr)
                    sys.exit(r.returncode)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                legs.append(json.loads(line))
                print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_vision_bench.py", device="MI355X", picture=args.size, legs=legs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
