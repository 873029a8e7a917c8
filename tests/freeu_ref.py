"""NumPy restatement of FreeU (diffusers' apply_freeu / fourier_filter, arXiv:2309.11497) for the FreeU tests.

  fourier_filter      the FFT form: fftshift(fftn(x)), scale the [H//2-1 : H//2+1, W//2-1 : W//2+1] band, ifftn(...).real
  freeu_closed_form   the same filter without an FFT: the band is the frequencies {0, -1} per axis (what freeu.hip computes)
  apply_freeu         one decoder block's (h, skip) pair of stage 1 (s1, b1) or stage 2 (s2, b2)
  controlled_unet_forward   pd_oracle.controlled_unet_forward with FreeU, built from the oracle's own blocks
  enabled(...)        context manager: pd_oracle's apply_model / p_sample_ddim / ddim_sampling evaluate the FreeU UNet
"""
import contextlib

import numpy as np

from oracle import pd_oracle as O

F32 = np.float32


def is_on(freeu) -> bool:
    """diffusers applies FreeU only if `s1 and s2 and b1 and b2` is truthy."""
    return freeu is not None and all(float(v) != 0.0 for v in freeu)


def fourier_filter(x, threshold: int, scale: float):
    """diffusers.utils.torch_utils.fourier_filter over the last two axes (in float64, returned as float32)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    X = np.fft.fftshift(np.fft.fftn(x, axes=(-2, -1)), axes=(-2, -1))
    crow, ccol = H // 2, W // 2
    mask = np.ones((H, W))
    mask[crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale   # Python slice rules (H == 1: [-1:1])
    X = X * mask
    return np.fft.ifftn(np.fft.ifftshift(X, axes=(-2, -1)), axes=(-2, -1)).real.astype(F32)


def freeu_closed_form(x, scale: float):
    """fourier_filter(x, 1, scale) as 7 real sums per plane: Ky = {0, H-1} ({0} when H == 1), Kx likewise,
    y[n] = x[n] + (scale - 1) / (H W) * sum_{k in Ky x Kx} Re(X[k] e^{+2 pi i (ky ny / H + kx nx / W)})."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    ky = [0] if H == 1 else [0, H - 1]
    kx = [0] if W == 1 else [0, W - 1]
    my, mx = np.arange(H)[:, None], np.arange(W)[None, :]
    y = x.copy()
    for a in ky:
        for b in kx:
            # exact integer phases (k m) mod N
            ph = 2.0 * np.pi * (((a * my) % H) / H + ((b * mx) % W) / W)
            Xk = (x * np.exp(-1j * ph)).sum(axis=(-2, -1), keepdims=True)
            y = y + (scale - 1.0) / (H * W) * (Xk * np.exp(1j * ph)).real
    return y.astype(F32)


def apply_freeu(stage: int, h, skip, s1, s2, b1, b2):
    """diffusers.utils.torch_utils.apply_freeu for resolution_idx = stage (0 or 1)."""
    s, b = (s1, b1) if stage == 0 else (s2, b2)
    h = h.copy()
    half = h.shape[1] // 2
    h[:, :half] = h[:, :half] * F32(b)
    return h, fourier_filter(skip, 1, s)


def controlled_unet_forward(sd, cfg, layouts, x, t, context, control, only_mid_control=False, freeu=None):
    """ControlledUnetModel.forward (cldm/cldm.py:23-45) with diffusers' FreeU in up_blocks[0] / [1]: the decoder blocks i with
    i // (num_res_blocks + 1) == 0 / 1.  Per block, the skip gets its control residual first (diffusers adds
    down_block_additional_residuals before the up blocks), then FreeU, then the concat.  freeu = (s1, s2, b1, b2) or None."""
    on = is_on(freeu)
    p = O.Net(sd, "model.diffusion_model.")
    control = list(control) if control is not None else None
    emb = O.time_embed(p, t, cfg.model_channels)
    hs = []
    h = x
    for i, blk in enumerate(layouts["enc"]):
        h = O._input_block(p, i, blk, h, emb, context, cfg.num_heads)
        hs.append(h)
    h = O._middle(p, h, emb, context, cfg.num_heads)
    if control is not None:
        h = h + control.pop()
    for i, blk in enumerate(layouts["dec"]):
        if only_mid_control or control is None:
            skip = hs.pop()
        else:
            skip = hs.pop() + control.pop()
        stage = i // (cfg.num_res_blocks + 1)
        if on and stage < 2:
            h, skip = apply_freeu(stage, h, skip, *freeu)
        h = np.concatenate([h, skip], axis=1)
        pre = f"output_blocks.{i}."
        h = O.resblock(p, pre + "0.", h, emb)
        j = 1
        if blk["attn"]:
            h = O.spatial_transformer(p, pre + "1.", h, context, cfg.num_heads)
            j = 2
        if blk["up"]:
            h = np.repeat(np.repeat(h, 2, axis=2), 2, axis=3)
            h = O.conv2d(h, p(pre + f"{j}.conv.weight"), p(pre + f"{j}.conv.bias"))
    h = O.silu(O.group_norm(h, p("out.0.weight"), p("out.0.bias")))
    return O.conv2d(h, p("out.2.weight"), p("out.2.bias"))


@contextlib.contextmanager
def enabled(s1, s2, b1, b2):
    """Within the block, pd_oracle's apply_model (and so p_sample_ddim, ddim_sampling, ...) runs the FreeU UNet, as a
    diffusers pipeline does after unet.enable_freeu(s1, s2, b1, b2)."""
    orig = O.controlled_unet_forward

    def fwd(sd, cfg, layouts, x, t, context, control, only_mid_control=False):
        return controlled_unet_forward(sd, cfg, layouts, x, t, context, control, only_mid_control, (s1, s2, b1, b2))

    O.controlled_unet_forward = fwd
    try:
        yield
    finally:
        O.controlled_unet_forward = orig
