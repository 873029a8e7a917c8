"""Writes tests/golden/clip_vision.npz: the CLIP image tower, its preprocessing and the safety checker, pinned on the CPU by the real
modules -- transformers' CLIPVisionModelWithProjection and CLIPImageProcessor (PIL backend) and PIL's Image.resize; nothing of the
engine is loaded.  Run once on a machine with transformers, torch and PIL:

    python tests/golden/make_golden_clip_vision.py

Weights, pixel_values and pictures are NOT stored: tests/clip_vision_ref.py draws them from seeded NumPy generators, for this file and
for the tests alike (the file stores their CRC-32 so that a changed generator is noticed).  Stored per tower configuration (A, B, C of
clip_vision_ref.CONFIGS): the module's float64 image_embeds, pooler_output and the HIDDEN_ROWS token rows of hidden_states[-2], and the
error (max-abs / max-abs) of the module's own CPU forward in float32, float16 and bfloat16 against that float64 run.  Per picture of
PREP_SHAPES: the PREP_ROWS crop rows of CLIPImageProcessor()'s pixel_values and of Image.resize(..., BICUBIC)'s bytes, and the CRC-32
of the whole cropped bytes / pixel_values.  For the checker: seeded embeddings, buffers and thresholds with the scores and flags of the
restatement that uses Python's round.

No score may lie within 1e-3 of the decision boundary 0.0005.  (A score that is positive only through the carried 0.01 lies within
0.01 of the boundary by construction, so a margin of 0.01 cannot hold for the batch this file must contain; 1e-3 is a hundred times
the 1e-5 to which the fp32 kernel's scores are held.)  Nothing here runs in the test suite: the tests read the .npz only."""
import os
import sys

import numpy as np
import torch
from PIL import Image
from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from prompt_diffusion_amd.weights import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD  # noqa: E402
from tests import clip_vision_ref as R  # noqa: E402


def make_module(cfg, sd, attn="eager"):
    hc = CLIPVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.ff, projection_dim=cfg.proj_dim, num_hidden_layers=cfg.layers,
                          num_attention_heads=cfg.heads, image_size=cfg.image_size, patch_size=cfg.patch, hidden_act=cfg.act,
                          layer_norm_eps=cfg.eps, attn_implementation=attn)
    m = CLIPVisionModelWithProjection(hc).eval()
    own = {k: torch.from_numpy(v) for k, v in R.module_state_dict(sd, cfg).items()}
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m


def run(m, pv, dtype):
    with torch.no_grad():
        r = m.to(dtype)(torch.from_numpy(pv).to(dtype), output_hidden_states=True)
    f = lambda t: t.double().numpy()
    return dict(image_embeds=f(r.image_embeds), hidden=f(r.hidden_states[-2]), hidden_all=[f(h) for h in r.hidden_states], last=f(r.last_hidden_state))


def main():
    out = dict(seed=np.int64(R.SEED))
    for name, (cfg, B) in R.CONFIGS.items():
        sd = R.synth_state_dict(cfg)
        pv = R.synth_pixel_values(name)
        # the float64 reference takes torch's scaled_dot_product_attention: transformers' eager attention computes its softmax in
        # float32 whatever the module's dtype, which would leave the "float64" outputs at 3e-8; the low-precision runs below are eager
        m = make_module(cfg, sd, "sdpa")
        ref = run(m, pv, torch.float64)
        with torch.no_grad():
            pooled = m.to(torch.float64).vision_model(torch.from_numpy(pv).double()).pooler_output.numpy()
        # the NumPy restatement against the module itself, in float64
        mine = R.forward(sd, cfg, pv)
        assert len(mine["hidden_states"]) == len(ref["hidden_all"]) == cfg.layers + 1
        for a, b in ((mine["image_embeds"], ref["image_embeds"]), (mine["pooler_output"], pooled), (mine["hidden_states"][-2], ref["hidden"]),
                     (mine["hidden_states"][-1], ref["last"])):
            assert R.relerr(a, b) < 1e-12, (name, R.relerr(a, b))
        out[f"{name}_image_embeds"] = ref["image_embeds"]
        out[f"{name}_pooler_output"] = pooled
        out[f"{name}_hidden_rows"] = R.HIDDEN_ROWS[name]
        out[f"{name}_hidden"] = ref["hidden"][:, R.HIDDEN_ROWS[name]]
        out[f"{name}_pv_crc"] = np.int64(R.crc(pv))
        out[f"{name}_sd_crc"] = np.int64(R.crc(np.concatenate([v.ravel() for v in sd.values()])))
        for tag, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
            low = run(make_module(cfg, sd), pv, dt)
            with torch.no_grad():
                low_pooled = make_module(cfg, sd).to(dt).vision_model(torch.from_numpy(pv).to(dt)).pooler_output.double().numpy()
            errs = np.array([R.relerr(low["image_embeds"], ref["image_embeds"]), R.relerr(low_pooled, pooled), R.relerr(low["hidden"], ref["hidden"])])
            out[f"{name}_err_{tag}"] = errs    # image_embeds, pooler_output, hidden_states[-2]
            print(name, tag, errs)

    proc = CLIPImageProcessor()
    assert tuple(np.float32(proc.image_mean)) == tuple(np.float32(OPENAI_CLIP_MEAN)) and tuple(np.float32(proc.image_std)) == tuple(np.float32(OPENAI_CLIP_STD))
    S = 224
    for (H, W) in R.PREP_SHAPES:
        img = R.synth_pictures((H, W))[0]
        pv = np.asarray(proc(Image.fromarray(img, "RGB"), return_tensors="np").pixel_values, np.float32)
        Hr, Wr, top, left = R.resize_geometry(H, W, S)
        full = np.asarray(Image.fromarray(img, "RGB").resize((Wr, Hr), resample=Image.BICUBIC))
        crop = np.ascontiguousarray(full[top:top + S, left:left + S])
        # the float32 value map restated in NumPy against the processor, on PIL's own bytes (the engine's tables are not needed here:
        # tests/test_clip_vision_cpu.py holds them to these bytes)
        p2 = R.normalize(crop[None], OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
        print((H, W), "->", (Hr, Wr), "crop", (top, left), "pixel_values vs restatement: ulp", R.ulp_diff(p2, pv), "max abs", float(np.abs(p2 - pv).max()))
        assert R.ulp_diff(p2, pv) <= 1
        k = f"prep_{H}x{W}"
        out[k + "_img_crc"] = np.int64(R.crc(img))
        out[k + "_geometry"] = np.array([Hr, Wr, top, left], np.int32)
        out[k + "_bytes_rows"] = crop[R.PREP_ROWS]
        out[k + "_bytes_crc"] = np.int64(R.crc(crop))
        out[k + "_pixel_values_rows"] = pv[0][:, R.PREP_ROWS]
        out[k + "_pixel_values_crc"] = np.int64(R.crc(pv))
        out[k + "_pixel_values_exact"] = np.int64(R.ulp_diff(p2, pv) == 0)
    out["prep_rows"] = R.PREP_ROWS

    s = R.synth_safety()
    scores, flags = R.safety_check(s["embeds"], s["special_care_embeds"], s["concept_embeds"], s["special_care_embeds_weights"], s["concept_embeds_weights"])
    assert np.abs(scores - 0.0005).min() >= 1e-3, np.abs(scores - 0.0005).min()
    pos = scores > 0.0005
    assert not flags[0] and not pos[0].any()                                   # clean
    assert flags[1] and pos[1, 3 + 3] and not pos[1, :3].any()                 # flagged directly, adj never raised
    assert flags[2] and pos[2, 0] and pos[2, 3 + 5] and scores[2, 3 + 5] - 0.01 < 0.0005 and pos[2, 3:].sum() == 1   # only through adj
    assert (s["embeds"][3] != 0).all() and pos[3, 0] and pos[3, 1] and scores[3, 1] - 0.01 < 0.0005
    print("safety flags", flags, "margin", np.abs(scores - 0.0005).min())
    for k, v in s.items():
        out["safety_" + k] = v
    out["safety_scores"] = scores
    out["safety_flags"] = flags

    path = os.path.join(ROOT, "tests", "golden", "clip_vision.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; limit", os.path.getsize(os.path.join(ROOT, "tests", "golden", "sd3_text.npz")))


if __name__ == "__main__":
    main()
