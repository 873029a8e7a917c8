"""Annotators: photographs -> the condition maps Prompt-Diffusion takes as ``query`` and inside ``example_pair``.

``HEDdetector`` is the reference's ``annotator.hed.HEDdetector`` with the network on the engine (``Engine.hed``: the VGG trunk,
the five side outputs and their fusion are gfx950 kernels behind ``pd_hed_detect``); the uint8 ends stay on the host, or run on
the GPU as well with ``detect(..., device=True)``.
``CannyDetector`` is the reference's ``annotator.canny.CannyDetector`` (``cv2.Canny(img, low, high)``) with all of it on the engine
(``Engine.canny``: Sobel / non-maximum suppression, the hysteresis flood and the output are gfx950 kernels behind ``pd_canny``).  Its
arithmetic is integer and pinned byte for byte to a NumPy restatement of OpenCV's algorithm (tests/canny_ref.py), and to ``cv2`` itself
only where ``cv2`` is installed; neither this module nor the engine needs OpenCV.
``MLSDdetector`` is the reference's ``annotator.mlsd.MLSDdetector`` with all of it on the engine (``Engine.mlsd``: MobileNetV2's
depthwise convs, the decoder, the peak decode and the line rasteriser are gfx950 kernels behind ``pd_mlsd_detect``; only uint8 comes
back).  Its decode and rasteriser are pinned to a NumPy restatement (tests/mlsd_ref.py) and, through the fixture, to the reference's
own ``pred_lines``; byte parity of the rasteriser with ``cv2.line`` itself is checked only where ``cv2`` is installed.
``HWC3`` and ``resize_image`` restate ``annotator/util.py`` in NumPy + PIL.  ``nms`` (the scribble step of ``annotator/hed``, which
goes through cv2's float ``GaussianBlur``) and the annotators whose networks need packages that are not at hand (MiDaS: timm;
UniFormer: mmcv's compiled extension) are not built.
"""
from __future__ import annotations

import numpy as np


def HWC3(x: np.ndarray) -> np.ndarray:
    """uint8 HW, HW1, HW3 or HW4 -> HW3 (grey replicated; alpha composited over white), as annotator/util.py:9-25."""
    if x.dtype != np.uint8:
        raise ValueError("HWC3 expects uint8")
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3 or x.shape[2] not in (1, 3, 4):
        raise ValueError(f"HWC3 expects HW, HW1, HW3 or HW4, got {x.shape}")
    C = x.shape[2]
    if C == 3:
        return x
    if C == 1:
        return np.concatenate([x, x, x], axis=2)
    color = x[:, :, 0:3].astype(np.float32)
    alpha = x[:, :, 3:4].astype(np.float32) / 255.0
    y = color * alpha + 255.0 * (1.0 - alpha)
    return y.clip(0, 255).astype(np.uint8)


def resize_image(input_image: np.ndarray, resolution: int) -> np.ndarray:
    """The short side to `resolution`, both sides rounded to multiples of 64 (annotator/util.py:28-38).  The target size is the
    reference's; the pixels are not: the reference resamples with cv2 (INTER_LANCZOS4 up, INTER_AREA down), this uses PIL
    (LANCZOS up, BOX down), whose kernels and rounding differ.  Parity of the resize is unpinned."""
    from PIL import Image
    H, W = float(input_image.shape[0]), float(input_image.shape[1])
    k = float(resolution) / min(H, W)
    H = int(np.round(H * k / 64.0)) * 64
    W = int(np.round(W * k / 64.0)) * 64
    img = Image.fromarray(input_image).resize((W, H), Image.LANCZOS if k > 1 else Image.BOX)
    return np.asarray(img)


def edge_to_uint8(edge: np.ndarray) -> np.ndarray:
    """The reference's float -> uint8 step, ``(edge * 255.0).clip(0, 255).astype(np.uint8)`` (annotator/hed/__init__.py:113):
    float32 arithmetic, truncation towards zero."""
    return (np.asarray(edge, np.float32) * 255.0).clip(0, 255).astype(np.uint8)


class HEDdetector:
    """``annotator.hed.HEDdetector`` on an engine built with ``ModelConfig(hed=True)`` whose hed.* weights are loaded
    (``Engine.load_hed_state_dict``)."""

    def __init__(self, engine):
        self.engine = engine

    def detect(self, images, device: bool = False) -> np.ndarray:
        """Batched form: uint8 [B, H, W, 3] RGB -> uint8 [B, H, W]; H and W multiples of 16.  device: the uint8 ends on the GPU
        too -- Engine.image_load(1, 0), Engine.hed on the CUDA tensor, Engine.image_store(1, 0, "trunc") -- with the same bytes
        out; only uint8 crosses the bus."""
        x = np.asarray(images)
        if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
            raise ValueError(f"detect expects uint8 [B, H, W, 3], got {x.dtype} {x.shape}")
        if device:
            edge = self.engine.hed(self.engine.image_load(x, mul=1.0, add=0.0), what="edge")
            return self.engine.image_store(edge, mul=1.0, add=0.0, rounding="trunc", host=True)[:, :, :, 0]
        # the reference divides the float32 image by 255 on its way in (:109-111); the engine flips RGB -> BGR itself
        x = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)
        return edge_to_uint8(self.engine.hed(x, what="edge")[:, 0])

    def __call__(self, input_image: np.ndarray) -> np.ndarray:
        """uint8 HWC RGB -> uint8 HW, as the reference's ``__call__``."""
        if np.asarray(input_image).ndim != 3:
            raise ValueError("HEDdetector expects one HWC image")
        return self.detect(np.asarray(input_image)[None])[0]


class CannyDetector:
    """``annotator.canny.CannyDetector`` on an engine (any configuration: the detector has no weights)."""

    def __init__(self, engine):
        self.engine = engine

    def detect(self, images, low_threshold, high_threshold, device: bool = False):
        """Batched form: uint8 [B, H, W, 3], [B, H, W, 1] or [B, H, W] (NumPy, or a CPU / CUDA torch tensor) -> uint8 [B, H, W] of
        0 / 255.  device: the edge map stays on the GPU and comes back as a CUDA tensor (a CUDA tensor in then never leaves it);
        otherwise a NumPy array comes back."""
        if not device:
            return self.engine.canny(images, low_threshold, high_threshold, host=True)
        if not hasattr(images, "is_cuda"):
            import torch
            images = torch.from_numpy(np.array(images))   # (a copy: torch wants a writable array)
        return self.engine.canny(images, low_threshold, high_threshold)

    def __call__(self, img: np.ndarray, low_threshold, high_threshold) -> np.ndarray:
        """uint8 HW or HWC -> uint8 HW, as the reference's ``__call__``."""
        img = np.asarray(img)
        if img.ndim not in (2, 3):
            raise ValueError("CannyDetector expects one HW or HWC image")
        return self.detect(img[None], low_threshold, high_threshold)[0]


class MLSDdetector:
    """``annotator.mlsd.MLSDdetector`` on an engine built with ``ModelConfig(mlsd=True)`` whose mlsd.* weights are loaded
    (``Engine.load_mlsd_state_dict``)."""

    def __init__(self, engine):
        self.engine = engine

    def detect(self, images, thr_v, thr_d, device: bool = False):
        """Batched form: uint8 [B, H, W, 3] RGB (NumPy, or a CPU / CUDA torch tensor) -> uint8 [B, H, W] of 0 / 255; H and W
        multiples of 32.  Every image is handled on its own.  device: the line map stays on the GPU and comes back as a CUDA tensor
        (a CUDA tensor in then never leaves it); otherwise a NumPy array comes back."""
        sh = tuple(images.shape)
        if len(sh) != 4 or sh[3] != 3:
            raise ValueError(f"detect expects uint8 [B, H, W, 3], got {sh}")
        if not device:
            return self.engine.mlsd(images, thr_v, thr_d, what="lines", host=True)
        if not hasattr(images, "is_cuda"):
            import torch
            images = torch.from_numpy(np.array(images))   # (a copy: torch wants a writable array)
        return self.engine.mlsd(images, thr_v, thr_d, what="lines")

    def __call__(self, input_image: np.ndarray, thr_v, thr_d) -> np.ndarray:
        """uint8 HWC RGB -> uint8 HW, as the reference's ``__call__``."""
        img = np.asarray(input_image)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("MLSDdetector expects one HWC image with three channels")
        if img.dtype != np.uint8:
            raise ValueError("MLSDdetector expects uint8")
        return self.detect(img[None], thr_v, thr_d)[0]
