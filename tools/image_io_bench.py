"""The image ends (Engine.image_load / image_store, the pipelines' device_images switch): what they cost and what they save.

    python tools/image_io_bench.py                      # everything: the ends alone, then the three pipeline workloads
    python tools/image_io_bench.py --leg ends           # image_load of 24 pictures at 768² (native and from 1024²), image_store of
                                                        # 8 at 768², each against the host code it replaces, with bytes per second
    python tools/image_io_bench.py --leg c4-768 --switch on|off     # one rate, one process (what the default run starts)
    python tools/image_io_bench.py --parent DIR         # also time the same calls with the package (and library) of another tree

Pipeline workloads, SD1.5 random weights, bs 8, RGB PIL inputs, end to end through pipe(...):
  c4-768    config #4: 768², 20 UniPC steps fused, bf16, 768² inputs, output_type="latent"
  c4-1024   the same with 1024² inputs, which need the resize
  pil-512   512², 50 DDIM steps, f16, 512² inputs, output_type="pil"
Every rate comes from a fresh process (one warm-up call, then the median of --calls timed calls); the legs alternate, --rounds times
over.  Each child runs under its own time limit and a failing child ends the run.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {
    "c4-768": dict(size=768, src=768, steps=20, precision="bf16", sched="unipc", output_type="latent"),
    "c4-1024": dict(size=768, src=1024, steps=20, precision="bf16", sched="unipc", output_type="latent"),
    "pil-512": dict(size=512, src=512, steps=50, precision="f16", sched="ddim", output_type="pil"),
}
B = 8


def pil_images(n, size, seed):
    import numpy as np
    from PIL import Image
    a = np.random.default_rng(seed).integers(0, 256, (n, size, size, 3), dtype=np.uint8)
    return [Image.fromarray(x, "RGB") for x in a]


def timed(fn, calls, sync):
    out, ts = None, []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return out, ts


def leg_pipeline(args):
    import numpy as np
    import torch

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
    from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
    w = WORKLOADS[args.leg]
    e = E.Engine(W.SD15, precision=w["precision"])
    e.init_random_weights(1234)
    g = np.random.default_rng(0)
    kw = dict(prompt_embeds=g.standard_normal((B, 77, 768), dtype=np.float32), negative_prompt_embeds=g.standard_normal((B, 77, 768), dtype=np.float32),
              image=pil_images(B, w["src"], 1), image_pair=[pil_images(B, w["src"], 2), pil_images(B, w["src"], 3)],
              num_inference_steps=w["steps"], guidance_scale=7.5, latents=g.standard_normal((B, 4, w["size"] // 8, w["size"] // 8), dtype=np.float32),
              output_type=w["output_type"], height=w["size"], width=w["size"])
    if w["sched"] == "unipc":
        pipe = PromptDiffusionPipeline(e, scheduler=UniPCMultistepScheduler(), fuse_scheduler=True)
    else:
        pipe = PromptDiffusionPipeline(e)
    if args.switch == "on":
        pipe.enable_device_images()
    pipe(**kw)
    out, ts = timed(lambda: pipe(**kw).images, args.calls, torch.cuda.synchronize)
    a = np.asarray(out) if w["output_type"] == "latent" else np.stack([np.asarray(im) for im in out])
    dt = statistics.median(ts)
    print(json.dumps(dict(leg=args.leg, switch=args.switch, tree=args.tree, images_per_s=round(B / dt, 3), ms=round(1e3 * dt, 1),
                          ms_all=[round(1e3 * t, 1) for t in ts], checksum=int(np.frombuffer(a.tobytes(), np.uint8).astype(np.uint64).sum()))))
    e.close()


def leg_ends(args):
    """The two ends alone.  Bytes per output pixel (three channels), as DESIGN.md section 7 counts them:
      image_load, no resize: 3 read + 12 written per destination sample; with a resize the horizontal pass adds 3 Ws / W read per
        source row pixel and 3 written, the vertical pass reads 3 Hs / H; plus the 3-byte upload of the source over the bus
      image_store: 12 read + 3 written, plus the 3-byte download."""
    import numpy as np
    import torch
    from PIL import Image

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    e = E.Engine(W.TINY, precision="f32")
    sync = torch.cuda.synchronize
    n, size = 24, 768
    for src in (768, 1024):
        ims = pil_images(n, src, 5)

        def host_load():
            outs = []
            for im in ims:
                if im.size != (size, size):
                    im = im.resize((size, size), resample=Image.LANCZOS)
                outs.append((np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0).transpose(2, 0, 1)[None])
            return torch.from_numpy(np.concatenate(outs, axis=0)).cuda()          # the engine uploaded it as fp32

        def dev_load():
            return e.image_load(np.stack([np.asarray(im) for im in ims]), (size, size))

        dev_src = torch.from_numpy(np.stack([np.asarray(im) for im in ims])).cuda()
        for fn in (host_load, dev_load):
            fn()
        ref, th = timed(host_load, args.calls, sync)
        got, td = timed(dev_load, args.calls, sync)
        _, tk = timed(lambda: e.image_load(dev_src, (size, size)), args.calls * 4, sync)     # device source: the kernels alone
        assert torch.equal(ref, got)
        px = n * size * size
        kernel_bytes = px * 15 if src == size else n * src * src * 3 + n * src * size * 3 * 2 + px * 12
        tkm = statistics.median(tk)
        print(json.dumps(dict(leg="image_load", pictures=n, src=src, dst=size, host_ms=round(1e3 * statistics.median(th), 2),
                              device_ms=round(1e3 * statistics.median(td), 2), device_source_ms=round(1e3 * tkm, 3),
                              kernel_bytes=kernel_bytes, GBps=round(kernel_bytes / tkm / 1e9, 1), upload_bytes=n * src * src * 3,
                              host_upload_bytes=px * 12, identical=True)))
    x = torch.rand((B, 3, size, size), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 2.6 - 1.3

    def host_store():
        img = np.clip(x.cpu().numpy() / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
        return [Image.fromarray((im * 255).round().astype("uint8")) for im in img]

    def dev_store():
        return [Image.fromarray(im) for im in e.image_store(x, mul=0.5, add=0.5, host=True)]

    for fn in (host_store, dev_store):
        fn()
    ref, th = timed(host_store, args.calls, sync)
    got, td = timed(dev_store, args.calls, sync)
    _, tk = timed(lambda: e.image_store(x, mul=0.5, add=0.5), args.calls * 4, sync)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(ref, got))
    px = B * size * size
    tkm = statistics.median(tk)
    print(json.dumps(dict(leg="image_store", pictures=B, size=size, host_ms=round(1e3 * statistics.median(th), 2),
                          device_ms=round(1e3 * statistics.median(td), 2), device_source_ms=round(1e3 * tkm, 3), kernel_bytes=px * 15,
                          GBps=round(px * 15 / tkm / 1e9, 1), download_bytes=px * 3, host_download_bytes=px * 12, identical=True)))
    e.close()


def run_child(argv, root, timeout):
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "image_io_bench.py")] + argv, env=env, timeout=timeout, cwd=root)
    if r.returncode != 0:
        sys.exit(f"child {argv} failed with status {r.returncode}: stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["ends"] + sorted(WORKLOADS))
    ap.add_argument("--switch", choices=["on", "off"], default="off")
    ap.add_argument("--tree", default="this")
    ap.add_argument("--parent", help="root of another checkout (built) whose package runs the same calls, switch off")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--only", nargs="*", help="workloads of the default run (default: all)")
    args = ap.parse_args()
    if args.leg == "ends":
        return leg_ends(args)
    if args.leg:
        return leg_pipeline(args)
    common = ["--calls", str(args.calls)]
    if not args.only or "ends" in args.only:
        run_child(["--leg", "ends"] + common, ROOT, args.timeout)
    for leg in sorted(WORKLOADS):
        if args.only and leg not in args.only:
            continue
        for _ in range(args.rounds):
            run_child(["--leg", leg, "--switch", "off"] + common, ROOT, args.timeout)
            run_child(["--leg", leg, "--switch", "on"] + common, ROOT, args.timeout)
            if args.parent:
                run_child(["--leg", leg, "--switch", "off", "--tree", "parent"] + common, os.path.abspath(args.parent), args.timeout)


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("PYTHONPATH", "").split(os.pathsep)[0] or ROOT)
    main()
