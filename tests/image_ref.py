"""NumPy restatements of the image ends (include/pdengine.h, "Image ends") for the tests: Pillow's integer two-pass 8-bit
resampler evaluated from pd_resample_coefficients' tables, the float32 value map of pd_image_load and the uint8 map of
pd_image_store.  Pillow itself (Image.resize) is the yardstick of the resize; these only turn tables into pixels."""
import numpy as np

PRECISION_BITS = 22     # Pillow's Resample.c: 32 - 8 - 2

# H x W pairs of the checks: up- and down-scaling in both axes, one axis only, the overshooting checkerboard, 8x up, about 8x down,
# identity
SHAPES = [((37, 53), (64, 64)), ((64, 64), (37, 53)), ((100, 80), (64, 128)), ((50, 50), (50, 64)), ((129, 200), (64, 64)),
          ((16, 16), (128, 128)), ((511, 300), (64, 192)), ((64, 64), (64, 64))]
CHECKER = ((129, 200), (64, 64))    # this pair runs on a 0 / 255 checkerboard: Lanczos overshoots there, so the clip matters
PIL_FILTER = {"lanczos": 1, "box": 4}


def seeded_image(src_hw, seed=0, batch=None):
    """Seeded uint8 RGB picture(s) [H, W, 3] (or [batch, H, W, 3]); the CHECKER pair gets a 0 / 255 checkerboard of 8-pixel cells (sharp edges,
    where Lanczos over- and undershoots) whose phase differs per channel and per sample."""
    H, W = src_hw
    n = 1 if batch is None else batch
    if tuple(src_hw) == CHECKER[0]:
        y, x, c, b = np.arange(H)[None, :, None, None], np.arange(W)[None, None, :, None], np.arange(3)[None, None, None, :], \
            np.arange(n)[:, None, None, None]
        img = (((y // 8 + x // 8 + c // 2 + b + seed) % 2) * 255).astype(np.uint8)
    else:
        img = np.random.default_rng([seed, H, W]).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return img[0] if batch is None else img


def pass_1d(img, bounds, kk, axis):
    """One pass of the 8-bit resampler along `axis` of a uint8 array: out = clip8((2^21 + sum pixel * kk) >> 22) in int32 with an
    arithmetic shift; bounds [n_out, 2] = (xmin, count), kk [n_out, ksize]."""
    a = np.moveaxis(np.asarray(img, np.uint8), axis, 0).astype(np.int32)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for i, (xmin, cnt) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for j in range(cnt):
            acc = acc + a[xmin + j] * np.int32(kk[i, j])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, dst_hw, coefficients, filter="lanczos"):
    """Pillow's Image.resize on uint8 [..., H, W, 3] from the tables `coefficients(in, out, filter) -> (bounds, kk)`: the
    horizontal pass first, its uint8 result into the vertical pass; a pass whose sizes are equal is skipped."""
    img = np.asarray(img, np.uint8)
    Hs, Ws = img.shape[-3], img.shape[-2]
    H, W = dst_hw
    if Ws != W:
        img = pass_1d(img, *coefficients(Ws, W, filter), axis=img.ndim - 2)
    if Hs != H:
        img = pass_1d(img, *coefficients(Hs, H, filter), axis=img.ndim - 3)
    return img


def pil_resize(img, dst_hw, filter="lanczos"):
    """The yardstick: PIL's own Image.resize on uint8 [H, W, 3] or [B, H, W, 3]."""
    from PIL import Image
    img = np.asarray(img, np.uint8)
    if img.ndim == 4:
        return np.stack([pil_resize(im, dst_hw, filter) for im in img])
    return np.asarray(Image.fromarray(img, "RGB").resize((dst_hw[1], dst_hw[0]), resample=PIL_FILTER[filter]))


def load_value(u8_nhwc, mul, add):
    """pd_image_load's value map: uint8 [B, H, W, 3] -> float32 [B, 3, H, W] = (u8 / 255) * mul + add, every operation in
    float32 and rounded once -- what prepare_image's `/ 255` (and `* 2 - 1` for the init image) computes."""
    v = np.asarray(u8_nhwc, np.uint8).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray((v * np.float32(mul) + np.float32(add)).transpose(0, 3, 1, 2))


def store_value(x_nchw, mul, add, rounding):
    """pd_image_store's map: float32 [B, C, H, W] -> uint8 [B, H, W, C] = min(max(x * mul + add, 0), 1) * 255 in float32, then
    np.round (half to even; "nearest_even") or astype(uint8) (truncation; "trunc")."""
    x = np.asarray(x_nchw, np.float32)
    u = np.minimum(np.maximum(x * np.float32(mul) + np.float32(add), np.float32(0)), np.float32(1)) * np.float32(255.0)
    u = np.round(u) if rounding == "nearest_even" else u
    return np.ascontiguousarray(u.astype(np.uint8).transpose(0, 2, 3, 1))
