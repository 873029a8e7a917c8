"""A torch-functional restatement of the HED edge detector, for the tests (CPU, or any device the tensors live on).

Restates what annotator/hed/__init__.py computes -- ``Network.forward`` and the pre- and post-processing of
``HEDdetector.__call__`` -- from a flat state dict under ``hed.`` + ``Network``'s names (prompt-diffusion_amd/weights.py:
``hed_spec``).  tests/golden/hed.npz, which the reference's own ``Network`` wrote, pins it (tests/test_hed_cpu.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = (("One", (0, 2)), ("Two", (1, 3)), ("Thr", (1, 3, 5)), ("Fou", (1, 3, 5)), ("Fiv", (1, 3, 5)))
BGR_MEAN = (104.00698793, 116.66876762, 122.67891434)


def _t(sd, name, like):
    v = sd["hed." + name]
    v = v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))
    return v.to(device=like.device, dtype=like.dtype)


def forward_bgr(sd, x):
    """Network.forward: x [B, 3, H, W] BGR in [0, 1] -> (sides [B, 5, H, W], edge [B, 1, H, W])."""
    size = x.shape[2:]
    x = x * 255.0 - torch.tensor(BGR_MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    ups = []
    for s, (tag, idxs) in enumerate(STAGES):
        if s:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for i in idxs:
            x = F.relu(F.conv2d(x, _t(sd, f"netVgg{tag}.{i}.weight", x), _t(sd, f"netVgg{tag}.{i}.bias", x), padding=1))
        score = F.conv2d(x, _t(sd, f"netScore{tag}.weight", x), _t(sd, f"netScore{tag}.bias", x))
        ups.append(F.interpolate(score, size=size, mode="bilinear", align_corners=False))
    sides = torch.cat(ups, 1)
    edge = torch.sigmoid(F.conv2d(sides, _t(sd, "netCombine.0.weight", x), _t(sd, "netCombine.0.bias", x)))
    return sides, edge


def detect_rgb(sd, images, dtype=torch.float32, device="cpu"):
    """What the engine's ``hed`` computes: images [B, 3, H, W] RGB in [0, 1] (NumPy) -> (sides, edge) as float32 NumPy."""
    x = torch.from_numpy(np.ascontiguousarray(images)).to(device=device, dtype=dtype)
    with torch.no_grad():
        sides, edge = forward_bgr(sd, x.flip(1))
    return sides.float().cpu().numpy(), edge.float().cpu().numpy()


def to_uint8(edge):
    """HEDdetector.__call__'s last step on a float edge map."""
    return (np.asarray(edge, np.float32) * 255.0).clip(0, 255).astype(np.uint8)


def detector(sd, image_u8):
    """HEDdetector.__call__: uint8 HWC RGB -> uint8 HW."""
    bgr = image_u8[:, :, ::-1].copy()
    x = torch.from_numpy(bgr).float() / 255.0
    with torch.no_grad():
        _, edge = forward_bgr(sd, x.permute(2, 0, 1)[None])
    return to_uint8(edge[0].numpy())[0]
