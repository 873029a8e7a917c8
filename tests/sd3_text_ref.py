"""NumPy restatement (fp64 arithmetic, fp32 results) of the SD3 text encoders, for tests: transformers' CLIPTextModelWithProjection and
T5EncoderModel as the reference's encode_prompt drives them (promptdiffusioncontrolnetpipeline_sd3.py:238-545), over the checkpoint's
state-dict names.  tests/golden/sd3_text.npz (made with transformers itself) pins this file; the GPU tests then use it at shapes the
fixture does not hold."""
import math

import numpy as np


def _ln(x, g, b, eps=1e-5):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def _softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def _act(x, name):
    if name == "quick_gelu":
        return x / (1.0 + np.exp(-1.702 * x))
    if name == "gelu":
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    if name == "gelu_new":
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    raise ValueError(name)


def eos_positions(ids, eos_token_id):
    """CLIPTextTransformer's pooling row: argmax(ids) when eos_token_id == 2 (the legacy rule both SD3 configs fall under), else the
    first ids == eos_token_id."""
    ids = np.asarray(ids)
    if eos_token_id == 2:
        return ids.argmax(-1)
    return (ids == eos_token_id).astype(np.int32).argmax(-1)


def clip_forward(sd, c, prefix, ids):
    """-> (hidden_states list of layers + 1 arrays [B, L, hidden] (no final LayerNorm), text_embeds [B, proj_dim]), fp64."""
    W = lambda n: np.asarray(sd[prefix + n], np.float64)
    P = "text_model."
    ids = np.asarray(ids)
    B, L = ids.shape
    H, dh = c.heads, c.hidden // c.heads
    x = W(P + "embeddings.token_embedding.weight")[ids] + W(P + "embeddings.position_embedding.weight")[None, :L]
    mask = np.triu(np.full((L, L), -np.inf), 1)
    hs = [x]
    for i in range(c.layers):
        Lp = f"{P}encoder.layers.{i}."
        h = _ln(x, W(Lp + "layer_norm1.weight"), W(Lp + "layer_norm1.bias"))
        q, k, v = (h @ W(Lp + f"self_attn.{n}_proj.weight").T + W(Lp + f"self_attn.{n}_proj.bias") for n in "qkv")
        sp = lambda t: t.reshape(B, L, H, dh).transpose(0, 2, 1, 3)
        p = _softmax(sp(q) @ sp(k).transpose(0, 1, 3, 2) * dh ** -0.5 + mask)
        a = (p @ sp(v)).transpose(0, 2, 1, 3).reshape(B, L, c.hidden)
        x = x + a @ W(Lp + "self_attn.out_proj.weight").T + W(Lp + "self_attn.out_proj.bias")
        h = _ln(x, W(Lp + "layer_norm2.weight"), W(Lp + "layer_norm2.bias"))
        h = _act(h @ W(Lp + "mlp.fc1.weight").T + W(Lp + "mlp.fc1.bias"), c.act)
        x = x + h @ W(Lp + "mlp.fc2.weight").T + W(Lp + "mlp.fc2.bias")
        hs.append(x)
    last = _ln(x, W(P + "final_layer_norm.weight"), W(P + "final_layer_norm.bias"))
    pooled = last[np.arange(B), eos_positions(ids, c.eos_token_id)]
    return hs, pooled @ W("text_projection.weight").T


def t5_bucket(rel, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional, for integer relative positions key - query (fp64 logarithm)."""
    rel = np.asarray(rel, np.int64)
    nb = num_buckets // 2
    ret = (rel > 0).astype(np.int64) * nb
    n = np.abs(rel)
    max_exact = nb // 2
    with np.errstate(divide="ignore"):
        large = max_exact + (np.log(np.maximum(n, 1) / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).astype(np.int64)
    large = np.minimum(large, nb - 1)
    return ret + np.where(n < max_exact, n, large)


def t5_forward(sd, t, ids, prefix="text_encoder_3."):
    """T5EncoderModel(ids)[0] without an attention mask -> [B, L, d_model], fp64."""
    W = lambda n: np.asarray(sd[prefix + n], np.float64)
    rms = lambda x, w: w * (x / np.sqrt((x * x).mean(-1, keepdims=True) + t.eps))
    ids = np.asarray(ids)
    B, L = ids.shape
    H, dk = t.heads, t.d_kv
    x = W("shared.weight")[ids]
    pos = np.arange(L)
    bucket = t5_bucket(pos[None, :] - pos[:, None], t.num_buckets, t.max_distance)             # [query, key]
    bias = W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")[bucket].transpose(2, 0, 1)[None]   # [1, H, q, k]
    for i in range(t.layers):
        Bp = f"encoder.block.{i}."
        h = rms(x, W(Bp + "layer.0.layer_norm.weight"))
        q, k, v = (h @ W(Bp + f"layer.0.SelfAttention.{n}.weight").T for n in "qkv")
        sp = lambda a: a.reshape(B, L, H, dk).transpose(0, 2, 1, 3)
        p = _softmax(sp(q) @ sp(k).transpose(0, 1, 3, 2) + bias)
        a = (p @ sp(v)).transpose(0, 2, 1, 3).reshape(B, L, H * dk)
        x = x + a @ W(Bp + "layer.0.SelfAttention.o.weight").T
        h = rms(x, W(Bp + "layer.1.layer_norm.weight"))
        g = _act(h @ W(Bp + "layer.1.DenseReluDense.wi_0.weight").T, "gelu_new") * (h @ W(Bp + "layer.1.DenseReluDense.wi_1.weight").T)
        x = x + g @ W(Bp + "layer.1.DenseReluDense.wo.weight").T
    return rms(x, W("encoder.final_layer_norm.weight"))


def encode_prompt(sd, cfg, ids_l, ids_g, ids_t5=None, clip_skip=None):
    """The tensor half of encode_prompt (:443-471): (prompt_embeds [B, 77 + Lt, joint_dim], pooled [B, proj_l + proj_g]), fp32.  Without a
    T5 encoder: [B, 77, joint_dim] (the engine's convention; the reference appends a zero block of 77 more rows)."""
    k = int(clip_skip or 0)
    hl, pl = clip_forward(sd, cfg.clip_l, "text_encoder.", ids_l)
    hg, pg = clip_forward(sd, cfg.clip_g, "text_encoder_2.", ids_g)
    clip = np.concatenate([hl[-(k + 2)], hg[-(k + 2)]], -1)
    clip = np.pad(clip, ((0, 0), (0, 0), (0, cfg.joint_dim - clip.shape[-1])))
    if cfg.t5 is not None:
        clip = np.concatenate([clip, t5_forward(sd, cfg.t5, ids_t5)], -2)
    return clip.astype(np.float32), np.concatenate([pl, pg], -1).astype(np.float32)
