"""Writes tests/golden/sd3_text.npz: the SD3 text encoders on the tiny configuration (sd3.SD3_TINY_TEXT), computed on the CPU by
transformers' own CLIPTextModelWithProjection (x 2) and T5EncoderModel with synth_sd3_text_state_dict loaded into them, assembled with
the reference's own cat / pad lines (promptdiffusioncontrolnetpipeline_sd3.py:457-471).  Run once on a machine with transformers:

    python tests/golden/make_golden_sd3_text.py

Everything is fp32.  Nothing here runs in the test suite: the tests read the .npz only."""
import os
import sys

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModelWithProjection, T5Config, T5EncoderModel
from transformers.models.t5.modeling_t5 import T5Attention

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from prompt_diffusion_amd import sd3  # noqa: E402

CFG = sd3.SD3_TINY_TEXT
SEED, B, LT = 1234, 3, 20
# the file stays small (as clip_sd15_b2.npz does it): hidden states keep these token rows, the assembled prompt_embeds a handful of rows on
# both sides of the CLIP / T5 boundary; pooled outputs and the T5 output are whole
CLIP_ROWS = np.unique(np.concatenate([np.arange(0, 77, 3), [1, 39, 40, 41, 76]]))
PE_ROWS = np.array([0, 5, 17, 40, 76, 77, 78, 85, 96])


def make_clip(c, sd, prefix):
    hc = CLIPTextConfig(vocab_size=c.vocab, hidden_size=c.hidden, intermediate_size=c.ff, projection_dim=c.proj_dim,
                        num_hidden_layers=c.layers, num_attention_heads=c.heads, max_position_embeddings=c.max_positions,
                        hidden_act=c.act, eos_token_id=c.eos_token_id, bos_token_id=c.vocab - 2, pad_token_id=1,
                        attn_implementation="eager")
    m = CLIPTextModelWithProjection(hc).eval().float()
    own = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix)}
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m


def make_t5(t, sd, prefix="text_encoder_3."):
    hc = T5Config(vocab_size=t.vocab, d_model=t.d_model, d_kv=t.d_kv, d_ff=t.d_ff, num_layers=t.layers, num_heads=t.heads,
                  relative_attention_num_buckets=t.num_buckets, relative_attention_max_distance=t.max_distance,
                  layer_norm_epsilon=t.eps, feed_forward_proj="gated-gelu", dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    m = T5EncoderModel(hc).eval().float()
    own = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix)}
    own["encoder.embed_tokens.weight"] = own["shared.weight"]
    m.load_state_dict(own, strict=True)
    return m


def main():
    sd = sd3.synth_sd3_text_state_dict(CFG, SEED)
    ids_l, ids_g, ids_t5 = sd3.synth_sd3_token_ids(CFG, B, LT, seed=7)
    eos_g = (ids_g == CFG.clip_g.eos_token_id)
    assert (eos_g.sum(1) >= 2).any() and len(set(eos_g.argmax(1).tolist())) > 1   # twice in a row; different rows, different places
    out = dict(ids_l=ids_l, ids_g=ids_g, ids_t5=ids_t5, seed=np.int64(SEED), clip_rows=CLIP_ROWS, pe_rows=PE_ROWS)
    with torch.no_grad():
        clip = {}
        for tag, c, prefix, ids in (("l", CFG.clip_l, "text_encoder.", ids_l), ("g", CFG.clip_g, "text_encoder_2.", ids_g)):
            r = make_clip(c, sd, prefix)(torch.from_numpy(ids).long(), output_hidden_states=True)
            clip[tag] = r
            for k in (0, 1):
                out[f"hidden_{tag}_skip{k}"] = r.hidden_states[-(k + 2)].numpy()[:, CLIP_ROWS]
            out[f"pooled_{tag}"] = r[0].numpy()
        t5 = make_t5(CFG.t5, sd)(torch.from_numpy(ids_t5).long())[0]
        out["t5"] = t5.numpy()
        for k in (0, 1):
            # the reference's lines (:457, :466-471)
            clip_prompt_embeds = torch.cat([clip["l"].hidden_states[-(k + 2)], clip["g"].hidden_states[-(k + 2)]], dim=-1)
            clip_prompt_embeds = torch.nn.functional.pad(clip_prompt_embeds, (0, t5.shape[-1] - clip_prompt_embeds.shape[-1]))
            pe = torch.cat([clip_prompt_embeds, t5], dim=-2).numpy()
            assert pe.shape == (B, 77 + LT, CFG.joint_dim)
            out[f"prompt_embeds_skip{k}"] = pe[:, PE_ROWS]
        out["pooled"] = torch.cat([clip["l"][0], clip["g"][0]], dim=-1).numpy()
        # T5Attention._relative_position_bucket for the relative positions -(L - 1) .. L - 1, L = 512
        L = 512
        rel = torch.arange(-(L - 1), L, dtype=torch.long)
        out["buckets_512"] = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=CFG.t5.num_buckets,
                                                                   max_distance=CFG.t5.max_distance).numpy().astype(np.int32)
    out = {k: (np.ascontiguousarray(v, np.float32) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(ROOT, "tests", "golden", "sd3_text.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: tuple(np.shape(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
