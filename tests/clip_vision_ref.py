"""What the CLIP image tower's fixture maker (tests/golden/make_golden_clip_vision.py) and its tests share: the tiny configurations,
seeded weights and inputs, and NumPy restatements of transformers' CLIPVisionModelWithProjection, of CLIPImageProcessor() and of
diffusers' StableDiffusionSafetyChecker.forward.  transformers / PIL themselves are the yardsticks (the maker runs them; the CPU tests
run them again where they are importable); these only let a test compute a reference without them."""
import math
import zlib

import numpy as np

from prompt_diffusion_amd.weights import (IMAGE_ENCODER_PREFIX, SAFETY_PREFIX, ClipVisionConfig, clip_vision_param_shapes)

SEED = 20240
# name -> (configuration, batch).  A: two blocks, B = 5 so that the projection's groups of four rows get a second group; B: the real
# sequence length 257 and its key padding to 264; C: ViT-H's head dimension 80 and erf-GELU.  A stands for the safety tower (the engine's
# stream type), B and C for image_encoder (fp32 stream).
CONFIGS = {
    "A": (ClipVisionConfig(hidden=128, layers=2, heads=2, ff=256, patch=14, image_size=56, proj_dim=64, act="quick_gelu",
                           prefix=SAFETY_PREFIX, stream_f32=False), 5),
    "B": (ClipVisionConfig(hidden=128, layers=1, heads=2, ff=256, patch=14, image_size=224, proj_dim=64, act="quick_gelu",
                           prefix=IMAGE_ENCODER_PREFIX, stream_f32=True), 2),
    "C": (ClipVisionConfig(hidden=160, layers=1, heads=2, ff=320, patch=14, image_size=56, proj_dim=64, act="gelu",
                           prefix=IMAGE_ENCODER_PREFIX, stream_f32=True), 2),
}
# token rows of hidden_states[-2] the fixture keeps (the file stays small): the class row, the first patches, the middle, the last
HIDDEN_ROWS = {"A": np.array([0, 1, 2, 8, 15, 16]), "B": np.array([0, 1, 2, 128, 255, 256]), "C": np.array([0, 1, 2, 8, 15, 16])}

# preprocessing: the pictures (H, W) and the crop rows whose processor output the fixture keeps
PREP_SHAPES = [(96, 160), (224, 224), (300, 231), (512, 512)]
PREP_ROWS = np.array([0, 1, 37, 111, 112, 186, 222, 223])
ENLARGE = ((40, 30), (224, 298))    # one enlargement for the table test: (H, W) -> Image.resize target (H, W)


def relerr(a, b):
    """max-abs / max-abs, the project's usual metric"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def crc(a) -> int:
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


# ------------------------------------------------------------------------------------------------ seeded weights and inputs
def synth_state_dict(cfg: ClipVisionConfig, seed: int = SEED):
    """float32 tensors under the registry's names (= the diffusers checkpoint's), drawn tensor by tensor from one seeded generator."""
    rng = np.random.default_rng([seed, cfg.hidden, cfg.layers, cfg.image_size])
    out = {}
    for name, shape in clip_vision_param_shapes(cfg).items():
        n = rng.standard_normal(shape)
        if name.endswith("class_embedding"):
            v = 0.5 * n
        elif name.endswith("position_embedding.weight"):
            v = 0.1 * n
        elif "norm" in name and name.endswith(".weight"):
            v = 1.0 + 0.1 * n
        elif "norm" in name and name.endswith(".bias"):
            v = 0.1 * n
        elif name.endswith(".bias"):
            v = 0.02 * n
        else:
            v = n / math.sqrt(int(np.prod(shape[1:])))
        out[name] = v.astype(np.float32)
    return out


def module_state_dict(sd, cfg: ClipVisionConfig):
    """The same tensors under CLIPVisionModelWithProjection.state_dict()'s own keys."""
    out = {}
    for k, v in sd.items():
        if k.startswith(cfg.prefix):
            out[k[len(cfg.prefix):]] = v
        else:
            out[k[len(cfg.outer_prefix):]] = v
    return out


def synth_pixel_values(name: str, seed: int = SEED):
    cfg, B = CONFIGS[name]
    rng = np.random.default_rng([seed, ord(name)])
    return rng.standard_normal((B, 3, cfg.image_size, cfg.image_size)).astype(np.float32)


def synth_pictures(hw, seed: int = SEED, batch: int = 1):
    """uint8 [batch, H, W, 3]: smooth gradients plus noise plus a hard-edged block, so that the bicubic lobes over- and undershoot"""
    H, W = hw
    rng = np.random.default_rng([seed, H, W])
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(y * 255.0 / max(H - 1, 1)), (x * 255.0 / max(W - 1, 1)), ((x + y) % 64) * 4.0], -1)
    img = base[None] + rng.normal(0, 40, (batch, H, W, 3))
    img[:, H // 4:H // 2, W // 3:2 * W // 3] = rng.integers(0, 2, (batch, 1, 1, 3)) * 255
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the tower
def _ln(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


_erf = np.vectorize(math.erf, otypes=[np.float64])


def _act(x, kind):
    if kind == "quick_gelu":
        return x / (1.0 + np.exp(-1.702 * x))
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def patches_from_pixel_values(pv, patch):
    """[B, 3, S, S] -> [B, (S / p)^2, 3 p^2], element c p^2 + py p + px: the rows the flattened Conv2d weight multiplies"""
    B, _, S, _ = pv.shape
    G = S // patch
    return pv.reshape(B, 3, G, patch, G, patch).transpose(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * patch * patch)


def patch_operand(pv, patch):
    """... zero-padded to the GEMM's row width (round_up(3 p^2, 8)) and flattened over the batch: pd_clip_preprocess's "patches" """
    p = patches_from_pixel_values(np.asarray(pv, np.float32), patch)
    kw = (3 * patch * patch + 7) // 8 * 8
    out = np.zeros((p.shape[0] * p.shape[1], kw), np.float32)
    out[:, :p.shape[2]] = p.reshape(-1, p.shape[2])
    return out


def forward(sd, cfg: ClipVisionConfig, pixel_values, dtype=np.float64):
    """CLIPVisionModelWithProjection(pixel_values, output_hidden_states=True) -> dict(image_embeds, pooler_output, hidden_states)"""
    w = lambda n: np.asarray(sd[n], dtype)
    V = cfg.prefix + "vision_model."
    C, H = cfg.hidden, cfg.heads
    dh = C // H
    x = patches_from_pixel_values(np.asarray(pixel_values, dtype), cfg.patch) @ w(V + "embeddings.patch_embedding.weight").reshape(C, -1).T
    B = x.shape[0]
    x = np.concatenate([np.broadcast_to(w(V + "embeddings.class_embedding"), (B, 1, C)), x], 1) + w(V + "embeddings.position_embedding.weight")
    x = _ln(x, w(V + "pre_layrnorm.weight"), w(V + "pre_layrnorm.bias"), cfg.eps)
    hs = [x]
    for i in range(cfg.layers):
        L = f"{V}encoder.layers.{i}."
        lin = lambda t, nm: t @ w(L + nm + ".weight").T + w(L + nm + ".bias")
        h = _ln(x, w(L + "layer_norm1.weight"), w(L + "layer_norm1.bias"), cfg.eps)
        split = lambda t: t.reshape(B, -1, H, dh).transpose(0, 2, 1, 3)
        q, k, v = split(lin(h, "self_attn.q_proj")) * dh ** -0.5, split(lin(h, "self_attn.k_proj")), split(lin(h, "self_attn.v_proj"))
        s = q @ k.transpose(0, 1, 3, 2)
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ v
        x = x + lin(a.transpose(0, 2, 1, 3).reshape(B, -1, C), "self_attn.out_proj")
        h = _ln(x, w(L + "layer_norm2.weight"), w(L + "layer_norm2.bias"), cfg.eps)
        x = x + lin(_act(lin(h, "mlp.fc1"), cfg.act), "mlp.fc2")
        hs.append(x)
    pooled = _ln(x[:, 0], w(V + "post_layernorm.weight"), w(V + "post_layernorm.bias"), cfg.eps)
    embeds = pooled @ w(cfg.outer_prefix + "visual_projection.weight").T
    return dict(image_embeds=embeds, pooler_output=pooled, hidden_states=hs)


# ------------------------------------------------------------------------------------------------ CLIPImageProcessor()
def resize_geometry(H, W, S):
    """(Hr, Wr, top, left): get_resize_output_image_size (shortest edge) and center_crop of transformers' image_transforms"""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(S * long_ / short)
    Hr, Wr = (new_long, S) if W <= H else (S, new_long)
    return Hr, Wr, (Hr - S) // 2, (Wr - S) // 2


def normalize(u8_nhwc, mean, std):
    """uint8 [B, S, S, 3] -> float32 [B, 3, S, S] = (v / 255 - mean) / std, every operation in float32 and rounded once"""
    v = np.asarray(u8_nhwc, np.uint8).astype(np.float32) / np.float32(255.0)
    v = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def preprocess(images_u8, S, coefficients, mean, std):
    """CLIPImageProcessor() on uint8 [B, H, W, 3] from the tables `coefficients(in, out, "bicubic") -> (bounds, kk)`: returns (the
    whole resized picture, its S x S crop, pixel_values)"""
    from tests.image_ref import resize_u8
    images_u8 = np.asarray(images_u8, np.uint8)
    Hr, Wr, top, left = resize_geometry(images_u8.shape[1], images_u8.shape[2], S)
    full = resize_u8(images_u8, (Hr, Wr), coefficients, "bicubic")
    crop = np.ascontiguousarray(full[:, top:top + S, left:left + S])
    return full, crop, normalize(crop, mean, std)


def ulp_diff(a, b):
    """largest distance in float32 units in the last place"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


# ------------------------------------------------------------------------------------------------ the safety checker
def safety_check(embeds, special, concepts, special_thr, concept_thr, dtype=np.float64):
    """StableDiffusionSafetyChecker.forward on image_embeds with Python's round(x, 3), as diffusers writes it: (scores [B, 20] before
    rounding -- 3 special-care, then 17 concept --, flags [B])"""
    norm = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    e = norm(np.asarray(embeds, dtype))
    cs, cc = e @ norm(np.asarray(special, dtype)).T, e @ norm(np.asarray(concepts, dtype)).T
    scores, flags = [], []
    for b in range(e.shape[0]):
        adj, row, bad = 0.0, [], False
        for j in range(cs.shape[1]):
            s = float(cs[b, j]) - float(special_thr[j]) + adj
            row.append(s)
            if round(s, 3) > 0:
                adj = 0.01
        for j in range(cc.shape[1]):
            s = float(cc[b, j]) - float(concept_thr[j]) + adj
            row.append(s)
            if round(s, 3) > 0:
                bad = True
        scores.append(row)
        flags.append(bad)
    return np.asarray(scores, np.float64), np.asarray(flags, bool)


def synth_safety(D=64, seed: int = SEED):
    """Four embeddings and the checker's buffers, thresholds chosen from the cosines so that the batch holds: 0 a clean image, 1 one
    flagged directly, 2 one flagged only because a special-care hit raised adj, 3 a zero-free embedding whose first special score is
    positive and whose second is positive only with the carried 0.01."""
    rng = np.random.default_rng([seed, D])
    concepts, special = rng.standard_normal((17, D)), rng.standard_normal((3, D))
    e = rng.standard_normal((4, D))
    e[1] = concepts[3] + 0.05 * rng.standard_normal(D)
    e[2] += 1.5 * special[0]
    e[3] += 1.5 * special[0]
    e[3][e[3] == 0] = 0.25
    e, concepts, special = (a.astype(np.float32) for a in (e, concepts, special))
    norm = lambda a: a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=-1, keepdims=True)
    cs, cc = norm(e) @ norm(special).T, norm(e) @ norm(concepts).T
    sthr, cthr = cs.max(0) + 0.05, cc.max(0) + 0.05
    sthr[0] = min(cs[2, 0], cs[3, 0]) - 0.05
    sthr[1] = cs[3, 1] + 0.005
    cthr[3] = 0.5
    cthr[5] = cc[2, 5] + 0.005
    return dict(embeds=e, concept_embeds=concepts, special_care_embeds=special, concept_embeds_weights=cthr.astype(np.float32),
                special_care_embeds_weights=sthr.astype(np.float32))


def with_thresholds(safety, value):
    """the same buffers with every threshold set to `value` (-1: everything flagged, +1: nothing)"""
    out = dict(safety)
    out["concept_embeds_weights"] = np.full(17, value, np.float32)
    out["special_care_embeds_weights"] = np.full(3, value, np.float32)
    return out

