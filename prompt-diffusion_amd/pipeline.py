"""(D)-path host surface: ``PromptDiffusionPipeline.__call__(prompt, image, image_pair, ...)``.

Same keyword arguments, defaults, exception types and loop semantics as the reference's
``pipeline_prompt_diffusion.py:890-1321`` (diffusers naming): images in [0, 1], one float
``controlnet_conditioning_scale`` (or logspace(-1, 0, 13) x scale in guess mode,
promptdiffusioncontrolnet.py:371-375), ``controlnet_keep`` gating from ``control_guidance_start/end``
(:1196-1202), guess-mode zero residuals for the unconditional half (:1248-1253), ``[negative, positive]``
CFG order (:1108, :1269-1270).  The denoising loop itself runs in the HIP engine.

Either side of the hot path:
  * the text encoder: ``tokenizer=`` (a transformers CLIPTokenizer or a callable prompts -> ids [B, 77]) runs the CLIP text
    transformer inside the engine (``pd_text_encode``) when the checkpoint's ``cond_stage_model.*`` tensors are
    loaded; a ``text_encoder(list_of_prompts) -> [B, 77, 768]`` callable overrides it; with neither pass ``prompt_embeds`` /
    ``negative_prompt_embeds`` (the north star consumes the CLIP embedding as a fixed context tensor) -- of any equal length
    L <= 1024: the engine takes the context length per call.  ``enable_long_prompts()`` makes the engine's encoder build the
    reference's long-prompt context (cldm/hack.py: three 75-token windows -> [B, 231, 768]);
  * the VAE decoder: built into the engine (``pd_vae_decode``) when the checkpoint's ``first_stage_model.*``
    tensors are loaded; a ``vae_decode(latents / scaling_factor) -> images in [-1, 1]`` callable overrides it; with
    neither use ``output_type="latent"``.
"""
from __future__ import annotations

import dataclasses
import inspect
from typing import Any, Callable, Dict, List, Optional, Sequence, Union

import numpy as np

from . import engine as E
from .ip_adapter import IPAdapterMixin
from .lora_pipeline import AdapterMixin
from .pag import PAGMixin


@dataclasses.dataclass
class StableDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]] = None


def _is_pil(x) -> bool:
    return type(x).__module__.startswith("PIL")


def _to_numpy(x):
    if E._is_torch(x):
        return x.detach().float().cpu().numpy()
    return np.asarray(x)


def add_noise_coefficients(cfg, timesteps):
    """(sa, sb) = (sqrt(abar[t]), sqrt(1 - abar[t])) per entry of `timesteps`, fp32 from the engine's fp32 table -- what
    diffusers' add_noise takes from its float32 alphas_cumprod, and what the engine's start / blend kernels use."""
    ac = E.alphas_cumprod(cfg).astype(np.float32)[np.asarray(timesteps, np.int64)]
    return np.sqrt(ac), np.sqrt(np.float32(1.0) - ac)


def add_noise(z0, eps, sa, sb):
    """diffusers' scheduler.add_noise at one timestep, fp32: sa * z0 + sb * eps."""
    return np.float32(sa) * z0 + np.float32(sb) * eps


def blend_latents(known, x, mask):
    """The inpainting blend of a 4-channel UNet, fp32: (1 - m) * known + m * x (m = 1 repaints)."""
    return (np.float32(1.0) - mask) * known + mask * x


class EngineGenerator:
    """generator=EngineGenerator(seed, sample_base=0): every random number of a pipeline call comes from the engine's seeded
    Philox generator (Engine.set_rng) -- the start latents, the eta > 0 DDIM draws (drawn inside the update kernel, no noise
    tensor is made or uploaded), the img2img noise, the VAE posterior sample, and the draws of an Euler ancestral scheduler,
    fused or on the host.  A sample's numbers depend on (seed, sample_base + its index in the batch) alone, so a sharded run
    that passes each shard's first global index as sample_base reproduces the unsharded images."""

    def __init__(self, seed: int, sample_base: int = 0):
        self.seed, self.sample_base = int(seed), int(sample_base)
        self.engine = None

    def bind(self, engine: E.Engine) -> "EngineGenerator":
        self.engine = engine
        engine.set_rng(self.seed, self.sample_base)
        return self

    def randn(self, shape, stream="step", draw: int = 0):
        if self.engine is None:
            raise ValueError("EngineGenerator is not bound to an engine yet (the pipeline binds it at the start of a call)")
        return self.engine.randn(shape, stream=stream, draw=draw)


def split_long_prompt(raw_ids, bos: int, eos: int, pad: int, windows: int = 3, width: int = 77) -> np.ndarray:
    """The reference's long-prompt windows (cldm/hack.py, _hacked_clip_forward): the untruncated token ids of one prompt, without
    special tokens, are cut into `windows` runs of width - 2 (tokens past (width - 2) * windows are dropped, as its split() drops
    them); each run becomes [BOS] + run + [EOS], cut or padded to `width` with the pad token.  Every prompt gets all `windows`
    windows, empty ones included.  Returns int32 [windows, width]."""
    raw = [int(t) for t in raw_ids]
    run = width - 2
    out = np.empty((windows, width), np.int32)
    for f in range(windows):
        x = [bos] + raw[run * f:run * (f + 1)] + [eos]
        out[f] = x[:width] if len(x) >= width else x + [pad] * (width - len(x))
    return out


def reference_clip_skip(clip_skip: int) -> int:
    """cldm/hack.py's clip_skip -> the engine's (= diffusers'): the reference takes hidden_states[-clip_skip] for clip_skip > 1 (and
    the last layer for 0 and 1), the engine's text_encode(clip_skip=k) takes hidden_states[-(k + 1)] -- so c > 1 maps to c - 1
    and 0 / 1 map to 0."""
    c = int(clip_skip)
    if c < 0:
        raise ValueError(f"clip_skip must be >= 0, got {clip_skip}")
    return c - 1 if c > 1 else 0


def _window_count(value) -> int:
    """long_prompts= of the constructors: None / False -> 0 (off), True -> 3 (the reference's), n -> n"""
    if value is None or value is False:
        return 0
    n = 3 if value is True else int(value)
    if n < 1:
        raise ValueError(f"long prompts need at least one window, got {value}")
    return n


def tokenize_long(tokenizer, prompts: List[str], windows: int, width: int) -> np.ndarray:
    """prompts -> int32 [B * windows, width] window ids (split_long_prompt of every prompt, prompt-major: the reference's
    '(b f) i' batch).  The tokenizer is called as the reference calls it -- truncation=False, add_special_tokens=False -- and
    supplies bos_token_id / eos_token_id / pad_token_id."""
    for attr in ("bos_token_id", "eos_token_id", "pad_token_id"):
        if getattr(tokenizer, attr, None) is None:
            raise ValueError(f"long prompts need a tokenizer with {attr} (a transformers CLIPTokenizer has it)")
    raw = tokenizer(list(prompts), truncation=False, add_special_tokens=False)["input_ids"]
    if len(raw) != len(prompts):
        raise ValueError(f"tokenizer returned {len(raw)} id lists for {len(prompts)} prompts")
    return np.concatenate([split_long_prompt(r, tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.pad_token_id, windows, width)
                           for r in raw]) if len(raw) else np.zeros((0, width), np.int32)


def prepare_inpaint_mask(mask_image, width, height, batch_size, scale_factor):
    """diffusers' mask processor (grayscale, resize to the image size with LANCZOS, binarize at 0.5), then the
    nearest-neighbour downsample to the latent size -- pixel (f i, f j) for scale_factor f, F.interpolate's default -- and the
    duplication to the batch: [batch_size, 1, height / f, width / f] float32.  Arrays: [H, W], [H, W, 1], [B, H, W] or [B, H, W, 1]
    (NumPy), [H, W], [B, H, W] or [B, 1, H, W] (torch), in [0, 1] at the image size.  Shared by the SD1.5 and SD3 inpaint pipelines."""
    outs = []
    for im in (mask_image if isinstance(mask_image, list) else [mask_image]):
        if _is_pil(im):
            if im.size != (width, height):
                from PIL import Image
                im = im.resize((width, height), resample=Image.LANCZOS)
            a = (np.asarray(im.convert("L"), dtype=np.float32) / 255.0)[None, None]
        else:
            a = _to_numpy(im).astype(np.float32)
            if a.ndim == 2:
                a = a[None, None]
            elif a.ndim == 3:
                a = a.transpose(2, 0, 1)[None] if isinstance(im, np.ndarray) and a.shape[-1] == 1 else a[:, None]
            elif a.ndim == 4 and isinstance(im, np.ndarray):
                a = a.transpose(0, 3, 1, 2)
            if a.ndim != 4 or a.shape[1] != 1:
                raise ValueError(f"mask_image must have one channel, got an array of shape {_to_numpy(im).shape}")
        if a.shape[-2:] != (height, width):
            raise ValueError(f"mask_image is {a.shape[-1]}x{a.shape[-2]}, the image {width}x{height}")
        outs.append(a)
    m = np.concatenate(outs, axis=0)
    m = np.where(m < 0.5, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    f = scale_factor
    m = np.ascontiguousarray(m[:, :, ::f, ::f])
    return PromptDiffusionPipeline._tile(m, batch_size, "`mask_image`")


class PromptDiffusionPipeline(AdapterMixin, IPAdapterMixin, PAGMixin):
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]
    vae_scale_factor = 8
    vae_scaling_factor = 0.18215      # models/cldm_v15.yaml:17

    def __init__(self, engine: E.Engine, text_encoder: Optional[Callable] = None, vae_decode: Optional[Callable] = None,
                 scheduler: Any = None, tokenizer: Any = None, fuse_scheduler: bool = False, long_prompts=None,
                 device_images: bool = False, safety_checker: Any = None, feature_extractor: Any = None, image_encoder: Any = None,
                 requires_safety_checker: bool = False, pag_applied_layers: Union[str, List[str]] = "mid"):
        """pag_applied_layers: the layers perturbed-attention guidance perturbs when a call passes pag_scale > 0, under diffusers' names
        (prompt_diffusion_amd.pag.parse_pag_layers; set_pag_applied_layers changes them later).  One class serves both uses, so
        __call__'s pag_scale defaults to 0 = off, where diffusers' PAG pipelines default to 3.0.
        long_prompts: True / a window count = enable_long_prompts() at construction.
        safety_checker: None (the default, and what the reference's __call__ runs: it switches its checker off), True = the engine's
        checker (Engine.configure_safety_checker + its weights: the CLIP ViT-L/14 tower, preprocessing and the concept check on the
        GPU), or a callable with diffusers' signature safety_checker(images=, clip_input=) -> (images, has_nsfw_concept), which then
        needs feature_extractor (a CLIPImageProcessor-like callable).  With a checker and output_type != "latent", flagged images
        come back black and nsfw_content_detected is the list of flags.  image_encoder: True = the engine's tower under
        "image_encoder." (Engine.configure_clip_vision), or a callable pixel_values -> object with .image_embeds / .hidden_states,
        for encode_image.  requires_safety_checker is kept as the reference's config flag.
        device_images: True = enable_device_images() at construction (the image ends of a call on the GPU; off by default).
        prompt_embeds / negative_prompt_embeds of any equal length L <= engine.PD_MAX_CONTEXT_LEN are accepted by every path
        (fused DDIM, fuse_scheduler=True, host schedulers, callbacks): the engine takes the context length per call.
        clip_skip of __call__ has diffusers' meaning (the hidden state of layer -(clip_skip + 1)); the reference's own
        hack_everything(clip_skip=c) counts one higher -- reference_clip_skip(c) converts, and the (L) facade in ddim.py takes c.
        fuse_scheduler: run the update of a UniPCMultistepScheduler (pd_unipc_sample), DPMSolverMultistepScheduler or
        PNDMScheduler (pd_lms_sample) inside the engine's loop instead of on the host between eps evaluations; same grid, same
        controlnet_keep scales, same callback semantics."""
        self.engine = engine
        self.tokenizer = tokenizer
        if text_encoder is None and tokenizer is not None:
            # cond stage inside the engine (pd_text_encode): the caller only supplies the tokenizer -- a
            # transformers CLIPTokenizer, or any callable prompts -> token ids [B, context_len]
            text_encoder = self._engine_text_encoder
        self.text_encoder = text_encoder
        self.vae_decode = vae_decode
        self.scheduler = scheduler          # None = the engine's fused DDIM (DDIMScheduler semantics of SD1.5)
        self.fuse_scheduler = bool(fuse_scheduler)
        if self.fuse_scheduler:
            self._check_fusable()
        self._long_windows = 0
        if _window_count(long_prompts):
            self.enable_long_prompts(long_prompts)
        self._guidance_scale = 7.5
        self._device_images = bool(device_images)
        if safety_checker is None and requires_safety_checker:
            raise ValueError("requires_safety_checker=True needs a safety_checker (True for the engine's, or a callable)")
        if safety_checker is not None and safety_checker is not True and feature_extractor is None:
            raise ValueError("a safety_checker callable needs a feature_extractor (the reference raises the same)")
        self.safety_checker = safety_checker
        self.feature_extractor = feature_extractor
        self.image_encoder = image_encoder
        self.requires_safety_checker = bool(requires_safety_checker)
        self._lora_init()      # LoRA adapters (load_lora_weights; lora_pipeline.AdapterMixin)
        self.set_pag_applied_layers(pag_applied_layers)

    def _check_fusable(self):
        """The fused loops restate this package's schedulers on the engine's own noise schedule; anything else is refused."""
        from .schedulers import (DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, PNDMScheduler,
                                 UniPCMultistepScheduler)
        sched = self.scheduler
        if type(sched) not in (UniPCMultistepScheduler, DPMSolverMultistepScheduler, PNDMScheduler, EulerAncestralDiscreteScheduler):
            raise ValueError("fuse_scheduler=True needs prompt_diffusion_amd.schedulers.UniPCMultistepScheduler, "
                             f"DPMSolverMultistepScheduler or PNDMScheduler, got {type(sched)}")
        cfg = self.engine.cfg
        if sched.num_train_timesteps != cfg.timesteps:
            raise ValueError(f"fuse_scheduler=True: scheduler num_train_timesteps {sched.num_train_timesteps} != the engine's "
                             f"{cfg.timesteps}")
        ac = E.alphas_cumprod(cfg)
        if not np.allclose(sched.alphas_cumprod, ac, rtol=1e-12, atol=0):
            raise ValueError("fuse_scheduler=True: the scheduler's alphas_cumprod differ from the engine's noise schedule "
                             "(beta_start / beta_end / beta_schedule)")

    # ------------------------------------------------------------------ properties of the reference
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1     # pipeline_prompt_diffusion.py:878

    # ------------------------------------------------------------------ input validation
    def check_image(self, image, prompt, prompt_embeds):
        """pipeline_prompt_diffusion.py:722-757."""
        ok_single = _is_pil(image) or E._is_torch(image) or isinstance(image, np.ndarray)
        ok_list = isinstance(image, list) and len(image) > 0 and (
            _is_pil(image[0]) or E._is_torch(image[0]) or isinstance(image[0], np.ndarray))
        if not ok_single and not ok_list:
            raise TypeError("image must be passed and be one of PIL image, numpy array, torch tensor, list of PIL images, "
                            f"list of numpy arrays or list of torch tensors, but is {type(image)}")
        image_batch_size = 1 if _is_pil(image) else len(image)
        if prompt is not None and isinstance(prompt, str):
            prompt_batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            prompt_batch_size = len(prompt)
        else:
            prompt_batch_size = prompt_embeds.shape[0]
        if image_batch_size != 1 and image_batch_size != prompt_batch_size:
            raise ValueError("If image batch size is not 1, image batch size must be same as prompt batch size. "
                             f"image batch size: {image_batch_size}, prompt batch size: {prompt_batch_size}")

    def check_inputs(self, prompt, image, image_pair, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None, controlnet_conditioning_scale=1.0, control_guidance_start=0.0,
                     control_guidance_end=1.0, callback_on_step_end_tensor_inputs=None):
        """pipeline_prompt_diffusion.py:559-719 (single-ControlNet branches)."""
        if callback_steps is not None and (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found {bad}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if tuple(prompt_embeds.shape) != tuple(negative_prompt_embeds.shape):
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
        for name, emb in (("prompt_embeds", prompt_embeds), ("negative_prompt_embeds", negative_prompt_embeds)):
            # any context length the engine takes per call (pd_sample_args.context_len)
            if emb is not None and (len(emb.shape) != 3 or not 1 <= emb.shape[1] <= E.PD_MAX_CONTEXT_LEN):
                raise ValueError(f"`{name}` must be [batch, L, dim] with 1 <= L <= {E.PD_MAX_CONTEXT_LEN}, got {tuple(emb.shape)}.")
        self.check_image(image, prompt, prompt_embeds)
        if len(image_pair) == 2:
            for im in image_pair:
                self.check_image(im, prompt, prompt_embeds)
        else:
            raise ValueError(f"You have passed a list of images of length {len(image_pair)}.Make sure the list size equals to two.")
        if not isinstance(controlnet_conditioning_scale, float):
            raise TypeError("For single controlnet: `controlnet_conditioning_scale` must be type `float`.")
        starts = control_guidance_start if isinstance(control_guidance_start, (tuple, list)) else [control_guidance_start]
        ends = control_guidance_end if isinstance(control_guidance_end, (tuple, list)) else [control_guidance_end]
        if len(starts) != len(ends):
            raise ValueError(f"`control_guidance_start` has {len(starts)} elements, but `control_guidance_end` has {len(ends)} elements."
                             " Make sure to provide the same number of elements to each list.")
        for start, end in zip(starts, ends):
            if start >= end:
                raise ValueError(f"control guidance start: {start} cannot be larger or equal to control guidance end: {end}.")
            if start < 0.0:
                raise ValueError(f"control guidance start: {start} can't be smaller than 0.")
            if end > 1.0:
                raise ValueError(f"control guidance end: {end} can't be larger than 1.0.")

    # ------------------------------------------------------------------ safety checker / image encoder (pipeline :490-528)
    @staticmethod
    def _pictures_u8(image):
        """What the reference hands its feature_extractor, as one uint8 array [B, H, W, 3]: a torch tensor in [-1, 1] goes through
        postprocess(output_type="pil") (denormalize, clamp, round), an array in [0, 1] through numpy_to_pil ((x * 255).round()), PIL
        images / uint8 arrays are taken as they are; None when the pictures differ in size."""
        if E._is_torch(image) and str(image.dtype) == "torch.uint8":      # pictures already: [B, H, W, 3] (or one [H, W, 3])
            image = image.detach().cpu().numpy()
        nchw = isinstance(image, np.ndarray) and image.dtype != np.uint8 and image.ndim == 4 and image.shape[1] == 3 and image.shape[3] != 3
        if E._is_torch(image) or nchw:      # (a float array [B, 3, H, W] is read like the tensor it stands for)
            x = _to_numpy(image)
            return (np.clip(x / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1) * 255).round().astype("uint8")
        if isinstance(image, np.ndarray):
            if image.dtype == np.uint8:
                return image if image.ndim == 4 else image[None]
            x = image if image.ndim == 4 else image[None]
            return (x * 255).round().astype("uint8")
        items = image if isinstance(image, (list, tuple)) else [image]
        arrs = [np.asarray(im.convert("RGB")) if _is_pil(im) else np.asarray(im) for im in items]
        if len({a.shape for a in arrs}) != 1:
            return None
        return np.stack(arrs).astype(np.uint8, copy=False)

    def _host_pixel_values(self, u8_or_image):
        if self.feature_extractor is None:
            raise ValueError("these pictures need a feature_extractor: the engine's preprocessing refuses reductions beyond "
                             f"{E.PD_RESAMPLE_MAX_SCALE}x and pictures of unequal sizes")
        from PIL import Image
        pics = [Image.fromarray(im) for im in u8_or_image] if isinstance(u8_or_image, np.ndarray) else u8_or_image
        return _to_numpy(self.feature_extractor(pics, return_tensors="np").pixel_values).astype(np.float32)

    def run_safety_checker(self, image, device=None, dtype=None):
        """pipeline :515-527: (image with the flagged pictures zeroed, has_nsfw_concept) -- (image, None) without a checker.  image:
        a tensor / array [B, 3, H, W] in [-1, 1] or an array [B, H, W, 3] in [0, 1], as in the reference."""
        if self.safety_checker is None:
            return image, None
        u8 = self._pictures_u8(image)
        if self.safety_checker is True:
            if u8 is not None and E.clip_preprocess_supported(u8.shape[1], u8.shape[2], self._safety_size()):
                flags = self.engine.safety_check(u8)
            else:
                flags = self.engine.safety_check(self.engine.clip_vision(self._host_pixel_values(u8 if u8 is not None else image), "embeds",
                                                                         prefix=E.SAFETY_PREFIX))
            flags = [bool(f) for f in flags]
            if any(flags):
                image = image.clone() if E._is_torch(image) else np.array(image, copy=True)
                for i, f in enumerate(flags):
                    if f:
                        image[i] = 0
            return image, flags
        clip_input = self._host_pixel_values(u8 if u8 is not None else image)
        image, flags = self.safety_checker(images=image, clip_input=clip_input)
        return image, flags

    def _safety_size(self) -> int:
        cv = getattr(self.engine, "_clip_vision", {}).get(E.SAFETY_PREFIX)
        return cv.image_size if cv is not None else 224

    def encode_image(self, image, device=None, num_images_per_prompt: int = 1, output_hidden_states=None):
        """pipeline :490-512: (image_embeds, zeros_like) -- or, with output_hidden_states, hidden_states[-2] of the pictures and of an
        all-zero pixel_values batch -- each repeat_interleave'd num_images_per_prompt times.  image: PIL pictures / uint8 arrays (the
        engine preprocesses them) or float pixel_values [B, 3, S, S].  NumPy arrays come back."""
        if self.image_encoder is None:
            raise ValueError("encode_image needs an image_encoder (True for the engine's tower, or a callable)")
        is_pv = (E._is_torch(image) and str(image.dtype) != "torch.uint8") or (isinstance(image, np.ndarray) and image.dtype != np.uint8)
        if self.image_encoder is True:
            eng = self.engine
            cv = eng._clip_vision[E.IMAGE_ENCODER_PREFIX]
            if is_pv:
                x = _to_numpy(image).astype(np.float32)
            else:
                x = self._pictures_u8(image)
                if x is None or not E.clip_preprocess_supported(x.shape[1], x.shape[2], cv.image_size):
                    x = self._host_pixel_values(x if x is not None else image)
            if output_hidden_states:
                hid = _to_numpy(eng.clip_vision(x, "hidden", hidden_layer=-2, prefix=E.IMAGE_ENCODER_PREFIX))
                zeros = np.zeros((x.shape[0], 3, cv.image_size, cv.image_size), np.float32)
                unc = _to_numpy(eng.clip_vision(zeros, "hidden", hidden_layer=-2, prefix=E.IMAGE_ENCODER_PREFIX))
                return np.repeat(hid, num_images_per_prompt, axis=0), np.repeat(unc, num_images_per_prompt, axis=0)
            emb = np.repeat(_to_numpy(eng.clip_vision(x, "embeds", prefix=E.IMAGE_ENCODER_PREFIX)), num_images_per_prompt, axis=0)
            return emb, np.zeros_like(emb)
        if is_pv:
            pv = _to_numpy(image).astype(np.float32)
        else:
            u8 = self._pictures_u8(image)
            pv = self._host_pixel_values(u8 if u8 is not None else image)
        if output_hidden_states:
            hid = _to_numpy(self.image_encoder(pv, output_hidden_states=True).hidden_states[-2])
            unc = _to_numpy(self.image_encoder(np.zeros_like(pv), output_hidden_states=True).hidden_states[-2])
            return np.repeat(hid, num_images_per_prompt, axis=0), np.repeat(unc, num_images_per_prompt, axis=0)
        emb = np.repeat(_to_numpy(self.image_encoder(pv).image_embeds), num_images_per_prompt, axis=0)
        return emb, np.zeros_like(emb)

    # ------------------------------------------------------------------ image ends on the device
    def enable_device_images(self):
        """Both image ends of a call on the GPU (Engine.image_load / image_store), bit-identical to the host code they replace:
        mode-"RGB" PIL images given as `image`, `image_pair` or an img2img / inpainting init `image` are uploaded as uint8,
        resampled there as PIL's LANCZOS resize does it and written straight into the engine's float layout (the pair as one
        6-channel tensor); the other sampling inputs are uploaded once and the loop runs on device pointers; output_type="pil"
        decodes on the device and downloads uint8 only.  Every other kind of input (arrays, tensors, other PIL modes, masks, a
        reduction beyond engine.PD_RESAMPLE_MAX_SCALE) keeps the host code and is uploaded.  Applies where the loop runs inside
        the engine (fused DDIM, fuse_scheduler=True, img2img, inpainting); the per-step driver (host schedulers, callbacks)
        builds the tensors the same way and brings them to the host once.  "np" and "latent" outputs are unchanged."""
        self._device_images = True

    def disable_device_images(self):
        self._device_images = False

    def _device_image(self, image, width, height, batch_size, num_images_per_prompt, out=None, c_off=0, channels=3, mul=1.0,
                      add=0.0):
        """prepare_image on the device: a new CUDA tensor [B, channels, H, W], or `out`, with channels c_off .. c_off + 2
        written; None when the input is not the device path's kind -- the caller then takes prepare_image."""
        items = image if isinstance(image, list) else [image]
        if not items or not all(_is_pil(im) and im.mode == "RGB" for im in items) or len({im.size for im in items}) != 1:
            return None
        Ws, Hs = items[0].size
        H, W = (height, width) if height is not None and width is not None else (Hs, Ws)
        if not E.resample_supported((Hs, Ws), (H, W)):
            return None
        repeat_by = batch_size if len(items) == 1 else num_images_per_prompt
        B = len(items) * repeat_by
        if out is not None and (out.shape[0], out.shape[2], out.shape[3]) != (B, H, W):
            return None
        src = np.stack([np.asarray(im) for im in items])
        return self.engine.image_load(src, (H, W), out=out, c_off=c_off, channels=channels, batch=B, batch_mode="repeat", mul=mul,
                                      add=add)

    def _to_device(self, x):
        """A sampling input on the engine's GPU: arrays and CPU tensors are uploaded as float32, None / "engine" pass through."""
        if x is None or isinstance(x, str):
            return x
        import torch
        dev = torch.device("cuda", self.engine.device)
        if E._is_torch(x):
            return x.detach().to(device=dev, dtype=torch.float32)
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    # ------------------------------------------------------------------ host pre-processing
    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt):
        """VaeImageProcessor(do_normalize=False).preprocess + repeat (pipeline :236-238, :760-788): [B,3,H,W] in [0,1]."""
        items = image if isinstance(image, list) else [image]
        outs = []
        for im in items:
            if _is_pil(im):
                if height is not None and width is not None and im.size != (width, height):
                    from PIL import Image
                    im = im.resize((width, height), resample=Image.LANCZOS)
                a = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
                outs.append(a.transpose(2, 0, 1)[None])
            else:
                a = _to_numpy(im).astype(np.float32)
                if isinstance(im, np.ndarray):        # numpy images are [H,W,C] or [B,H,W,C] in [0,1]
                    a = a[None] if a.ndim == 3 else a
                    a = a.transpose(0, 3, 1, 2)
                else:                                 # torch tensors are [C,H,W] or [B,C,H,W]
                    a = a[None] if a.ndim == 3 else a
                outs.append(a)
        x = np.concatenate(outs, axis=0)
        repeat_by = batch_size if x.shape[0] == 1 else num_images_per_prompt
        return np.repeat(x, repeat_by, axis=0)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, generator, latents=None):
        """pipeline :791-806; init_noise_sigma of DDIM is 1."""
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            latents = self._randn(shape, generator)
        else:
            latents = _to_numpy(latents).astype(np.float32)
        sigma = float(getattr(self.scheduler, "init_noise_sigma", 1.0)) if self.scheduler is not None else 1.0
        return latents * np.float32(sigma)

    # ------------------------------------------------------------------ img2img / inpainting (the subclasses below)
    def get_timesteps(self, timesteps, strength):
        """diffusers' get_timesteps: the last min(int(S * strength), S) entries of the S-entry grid `timesteps` (sampling
        order) and the index of the first one, which the scheduler learns through set_begin_index when it has it."""
        S = len(timesteps)
        init_timestep = min(int(S * strength), S)
        t_start = max(S - init_timestep, 0)
        order = int(getattr(self.scheduler, "order", 1)) if self.scheduler is not None else 1
        grid = [int(t) for t in timesteps[t_start * order:]]
        if len(grid) < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"
                             f"steps is {len(grid)} which is < 1 and not appropriate for this pipeline.")
        if self.scheduler is not None and hasattr(self.scheduler, "set_begin_index"):
            self.scheduler.set_begin_index(t_start * order)
        return grid, t_start * order

    def _check_init(self, init):
        strength = init["strength"]
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        for key, what in (("image", "`image` (the init image)"), ("mask", "`mask_image`")):
            im = init[key]
            if im is None:
                if key == "image":
                    raise ValueError(f"{what} must be passed")
                continue
            items = im if isinstance(im, list) else [im]
            if not items or not all(_is_pil(x) or E._is_torch(x) or isinstance(x, np.ndarray) for x in items):
                raise TypeError(f"{what} must be a PIL image, numpy array, torch tensor or a list of them, but is {type(im)}")

    @staticmethod
    def _tile(x, batch_size, what):
        """diffusers' duplication of init latents / masks to the batch: whole-batch repeats (torch .repeat)."""
        if x.shape[0] == batch_size:
            return x
        if batch_size % x.shape[0] != 0:
            raise ValueError(f"Cannot duplicate {what} of batch size {x.shape[0]} to {batch_size} images; the batch size must "
                             "divide it.")
        if E._is_torch(x):
            return x.repeat((batch_size // x.shape[0],) + (1,) * (x.ndim - 1))
        return np.tile(x, (batch_size // x.shape[0],) + (1,) * (x.ndim - 1))

    def prepare_mask(self, mask_image, width, height, batch_size):
        """diffusers' mask processor (grayscale, resize to the image size with LANCZOS, binarize at 0.5), then the
        nearest-neighbour downsample to the latent size -- pixel (8i, 8j), F.interpolate's default -- and the duplication to the
        batch: [batch_size, 1, height / 8, width / 8] float32.  Arrays: [H, W], [H, W, 1], [B, H, W] or [B, H, W, 1] (NumPy),
        [H, W], [B, H, W] or [B, 1, H, W] (torch), in [0, 1] at the image size."""
        return prepare_inpaint_mask(mask_image, width, height, batch_size, self.vae_scale_factor)

    def _init_latents(self, image, width, height, batch_size, generator, device=False):
        """z0 = scaling_factor * the init image's latents, [batch_size, 4, height / 8, width / 8]: a 4-channel `image` is taken
        as latents; anything else is preprocessed as prepare_image does, mapped to [-1, 1] and encoded on the engine with a
        posterior sample (vae_encode mode "sample", a standard-normal draw from `generator`).  device: RGB PIL images go
        through Engine.image_load(2, -1) straight into vae_encode and z0 stays a CUDA tensor."""
        cfg = self.engine.cfg
        zc, f = cfg.in_channels, self.vae_scale_factor
        lat_hw = (height // f, width // f)
        if (E._is_torch(image) or isinstance(image, np.ndarray)) and image.ndim == 4 and image.shape[1] == zc:
            z = _to_numpy(image).astype(np.float32)
            if tuple(z.shape[2:]) != lat_hw:
                raise ValueError(f"latent `image` must be [B, {zc}, {lat_hw[0]}, {lat_hw[1]}], got {tuple(z.shape)}")
        else:
            x = self._device_image(image, width, height, 1, 1, mul=2.0, add=-1.0) if device else None
            on_device = x is not None
            if not on_device:
                x = self.prepare_image(image, width, height, 1, 1)
            if tuple(x.shape[-2:]) != (height, width):
                raise ValueError(f"`image` is {x.shape[-1]}x{x.shape[-2]}, the control image {width}x{height}")
            if not getattr(cfg, "vae_encoder", False) or self.engine.vae_encoder_weights_missing() != 0:
                raise ValueError("an init `image` needs the engine's VAE encoder (vae_encoder=True and the first_stage_model.encoder.* "
                                 "/ quant_conv.* weights), or pass its latents as a 4-channel `image`")
            if not on_device:
                x = np.ascontiguousarray(x * np.float32(2.0) - np.float32(1.0))
            Bi = x.shape[0]
            gen = generator[:Bi] if isinstance(generator, list) else generator
            # (an EngineGenerator: the posterior kernel draws at stream "vae" itself)
            noise = "engine" if isinstance(gen, EngineGenerator) else self._randn((Bi, zc) + lat_hw, gen)
            if on_device:
                return self._tile(self.engine.vae_encode(x, mode="sample", noise=self._to_device(noise)), batch_size, "`image`").contiguous()
            z = _to_numpy(self.engine.vae_encode(x, mode="sample", noise=noise)).astype(np.float32)
        return np.ascontiguousarray(self._tile(z, batch_size, "`image`"))

    @staticmethod
    def _randn(shape, generator):
        if generator is None:
            return np.random.standard_normal(shape).astype(np.float32)
        if isinstance(generator, EngineGenerator):     # the start latents / the img2img noise: stream "xt"
            return np.asarray(generator.randn(shape, stream="xt"), np.float32)
        if isinstance(generator, np.random.Generator):
            return generator.standard_normal(shape, dtype=np.float32)
        import torch
        if isinstance(generator, list):
            return np.concatenate([torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device).cpu().numpy()
                                   for g in generator])
        return torch.randn(shape, generator=generator, device=generator.device).cpu().numpy()

    def _tokenize(self, prompts: List[str]):
        """pipeline :386-392 / FrozenCLIPEmbedder.forward (modules.py:119-121): pad / truncate to context_len."""
        L = self.engine.cfg.context_len
        tok = self.tokenizer
        if hasattr(tok, "model_max_length") or hasattr(tok, "pad_token_id"):      # transformers tokenizer
            ids = tok(prompts, padding="max_length", max_length=L, truncation=True, return_tensors="np")["input_ids"]
        else:
            ids = tok(prompts)
        ids = np.asarray(_to_numpy(ids), np.int32)
        if ids.ndim != 2 or ids.shape != (len(prompts), L):
            raise ValueError(f"tokenizer must return ids of shape [{len(prompts)}, {L}], got {ids.shape}")
        return ids

    def enable_long_prompts(self, windows: int = 3):
        """Prompts longer than 77 tokens as the reference does them (cldm/hack.py, hack_everything -> _hacked_clip_forward): the
        tokenizer runs without truncation and special tokens, the ids are split into `windows` runs of 75, each wrapped in BOS / EOS
        and padded to 77 (split_long_prompt); the [B * windows, 77] ids go through the engine's CLIP in one text_encode call and
        are viewed as a [B, 77 * windows, D] context.  Every prompt, the negative one included, gets `windows` windows.  Needs the
        engine's own text encoder (a tokenizer, no text_encoder callable)."""
        n = _window_count(windows)
        if self.tokenizer is None or self.text_encoder != self._engine_text_encoder:
            raise ValueError("long prompts are built by the engine's own text encoder: construct the pipeline with `tokenizer=` and "
                             "without a `text_encoder` callable (or pass `prompt_embeds` of the long context)")
        if n * self.engine.cfg.context_len > E.PD_MAX_CONTEXT_LEN:
            raise ValueError(f"{n} windows of {self.engine.cfg.context_len} tokens exceed PD_MAX_CONTEXT_LEN {E.PD_MAX_CONTEXT_LEN}")
        self._long_windows = n

    def disable_long_prompts(self):
        self._long_windows = 0

    def _engine_text_encoder(self, prompts: List[str], clip_skip: Optional[int] = None):
        if self.engine.text_weights_missing() != 0:
            raise ValueError("a string `prompt` needs the cond_stage_model.transformer.text_model.* weights in the engine "
                             "(or a text_encoder callable, or `prompt_embeds`)")
        if self._long_windows:
            L, n = self.engine.cfg.context_len, self._long_windows
            z = self.engine.text_encode(tokenize_long(self.tokenizer, prompts, n, L), clip_skip=clip_skip or 0)
            return z.reshape(len(prompts), n * L, z.shape[-1])     # '(b f) i c -> b (f i) c'
        return self.engine.text_encode(self._tokenize(prompts), clip_skip=clip_skip or 0)

    def _encode_text(self, prompts: List[str], clip_skip: Optional[int]):
        """text_encoder(ids)[0], or with clip_skip the hidden state of layer -(clip_skip+1) through final_layer_norm
        (pipeline :398-413).  The conditional prompt honours clip_skip; the reference encodes the negative prompt without
        it (pipeline :455-459)."""
        if not clip_skip:
            return _to_numpy(self.text_encoder(prompts))
        if "clip_skip" not in set(inspect.signature(self.text_encoder).parameters.keys()):
            raise ValueError("clip_skip needs a text_encoder that accepts `clip_skip=` (the engine's own does); "
                             "or pass prompt_embeds computed with it")
        return _to_numpy(self.text_encoder(prompts, clip_skip=clip_skip))

    def encode_prompt(self, prompt, num_images_per_prompt, do_cfg, negative_prompt=None, prompt_embeds=None,
                      negative_prompt_embeds=None):
        """pipeline :308-487 reduced to its tensor contract: returns (prompt_embeds, negative_prompt_embeds) [B*n, L, D]."""
        if prompt_embeds is None:
            if self.text_encoder is None:
                raise ValueError("a string `prompt` needs a text_encoder; this engine consumes the CLIP embedding as a fixed "
                                 "context tensor -- pass `prompt_embeds` (and `negative_prompt_embeds`)")
            plist = [prompt] if isinstance(prompt, str) else list(prompt)
            prompt_embeds = self._encode_text(plist, getattr(self, "_clip_skip", None))
        pe = np.repeat(_to_numpy(prompt_embeds).astype(np.float32), num_images_per_prompt, axis=0)
        ne = None
        if do_cfg:
            if negative_prompt_embeds is None:
                if self.text_encoder is None:
                    raise ValueError("classifier-free guidance needs `negative_prompt_embeds` when no text_encoder is attached")
                bs = pe.shape[0] // num_images_per_prompt
                if negative_prompt is None:
                    neg = [""] * bs
                elif isinstance(negative_prompt, str):
                    neg = [negative_prompt] * bs
                else:
                    if len(negative_prompt) != bs:
                        raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: "
                                         f"{prompt} has batch size {bs}.")
                    neg = list(negative_prompt)
                negative_prompt_embeds = _to_numpy(self.text_encoder(neg))
            ne = np.repeat(_to_numpy(negative_prompt_embeds).astype(np.float32), num_images_per_prompt, axis=0)
        return pe, ne

    # ------------------------------------------------------------------ LoRA (diffusers LoraLoaderMixin surface; lora_pipeline.py)
    _lora_component_names = ("unet", "text_encoder")

    def _lora_parse(self, src):
        """kohya, diffusers/PEFT or legacy attention-processor keys -> the engine's UNet and text transformer tensors"""
        from . import lora as L
        return L.parse_adapters(src, self.engine.cfg)

    def _lora_components(self, names):
        from . import weights as W
        te = any(k.startswith(W.TEXT_PREFIX) for k in names)
        if te and self.text_encoder is not None and self.text_encoder != self._engine_text_encoder:
            raise ValueError("this LoRA has text-encoder layers, but a caller-supplied text_encoder is attached; only the engine's "
                             "own text transformer can take them")
        return dict(unet=any(k.startswith(W.UNET_PREFIX) for k in names), text_encoder=te)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        r"""Enables the FreeU mechanism as in https://arxiv.org/abs/2309.11497.

        The suffixes after the scaling factors represent the stages where they are being applied.

        Please refer to the [official repository](https://github.com/ChenyangSi/FreeU) for combinations of the values
        that are known to work well for different pipelines such as Stable Diffusion v1, v2, and Stable Diffusion XL.

        Args:
            s1 (`float`):
                Scaling factor for stage 1 to attenuate the contributions of the skip features. This is done to
                mitigate "oversmoothing effect" in the enhanced denoising process.
            s2 (`float`):
                Scaling factor for stage 2 to attenuate the contributions of the skip features. This is done to
                mitigate "oversmoothing effect" in the enhanced denoising process.
            b1 (`float`): Scaling factor for stage 1 to amplify the contributions of backbone features.
            b2 (`float`): Scaling factor for stage 2 to amplify the contributions of backbone features.
        """
        # engine state (Engine.set_freeu): every UNet evaluation of this engine applies it, whatever the scheduler path
        self.engine.set_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        """Disables the FreeU mechanism if enabled."""
        self.engine.disable_freeu()

    def _engine_vae(self, what: str):
        """The engine whose VAE the four switches below act on; ValueError where decoding is the caller's."""
        if self.vae_decode is not None and getattr(self.engine.cfg, "vae_ch", 0) <= 0:
            raise ValueError(f"{what} acts on the engine's VAE, but this pipeline decodes through the injected `vae_decode` callable and its "
                             "engine was built without one (vae_ch = 0): switch tiling / slicing on in that callable's own VAE")
        if getattr(self.engine.cfg, "vae_ch", 0) <= 0:
            raise ValueError(f"{what} needs an engine with a VAE (vae_ch > 0)")
        return self.engine

    def enable_vae_slicing(self):
        r"""
        Enable sliced VAE decoding. When this option is enabled, the VAE will split the input tensor in slices to
        compute decoding in several steps. This is useful to save some memory and allow larger batch sizes.
        """
        # engine state (Engine.set_vae_slicing): every later vae_decode / vae_encode of this engine, the device-image path included
        self._engine_vae("enable_vae_slicing").set_vae_slicing(True)

    def disable_vae_slicing(self):
        r"""
        Disable sliced VAE decoding. If `enable_vae_slicing` was previously enabled, this method will go back to
        computing decoding in one step.
        """
        self._engine_vae("disable_vae_slicing").set_vae_slicing(False)

    def enable_vae_tiling(self):
        r"""
        Enable tiled VAE decoding. When this option is enabled, the VAE will split the input tensor into tiles to
        compute decoding and encoding in several steps. This is useful for saving a large amount of memory and to allow
        processing larger images.
        """
        st = self._engine_vae("enable_vae_tiling").vae_tiling   # (keeps tile size, overlap and tile batch as set on the engine)
        self.engine.set_vae_tiling(True, st.tile_latent, st.overlap_factor, st.tile_batch)

    def disable_vae_tiling(self):
        r"""
        Disable tiled VAE decoding. If `enable_vae_tiling` was previously enabled, this method will go back to
        computing decoding in one step.
        """
        st = self._engine_vae("disable_vae_tiling").vae_tiling
        self.engine.set_vae_tiling(False, st.tile_latent, st.overlap_factor, st.tile_batch)

    # ------------------------------------------------------------------ the call
    def __call__(self, prompt: Union[str, List[str]] = None, image=None, image_pair: List = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 timesteps: List[int] = None, guidance_scale: float = 7.5,
                 negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 clip_skip: Optional[int] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 **kwargs):
        return self._run(prompt=prompt, image=image, image_pair=image_pair, height=height, width=width,
                         num_inference_steps=num_inference_steps, timesteps=timesteps, guidance_scale=guidance_scale,
                         negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator,
                         latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                         ip_adapter_image=ip_adapter_image, ip_adapter_image_embeds=ip_adapter_image_embeds, output_type=output_type,
                         return_dict=return_dict,
                         cross_attention_kwargs=cross_attention_kwargs, controlnet_conditioning_scale=controlnet_conditioning_scale,
                         guess_mode=guess_mode, control_guidance_start=control_guidance_start,
                         control_guidance_end=control_guidance_end, clip_skip=clip_skip, callback_on_step_end=callback_on_step_end,
                         callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, pag_scale=pag_scale,
                         pag_adaptive_scale=pag_adaptive_scale, kwargs=kwargs)

    def _run(self, *, ip_adapter_image=None, ip_adapter_image_embeds=None, pag_scale=0.0, pag_adaptive_scale=0.0, **body):
        """_run_body(**body) inside the IP-Adapter bracket of the call (IPAdapterMixin._ip_image_of_call): the image state is set in the
        engine before the body runs and cleared when it ends, with or without an exception.  Likewise the perturbed-attention guidance
        of the call (PAGMixin._pag_of_call): the engine's state is what it was once the call has ended.  The PAG bracket is the
        inner one: on an exception it ends the engine's session first (PAG cannot be switched on again inside one), then puts its state
        back, and only then does the IP bracket clear the image."""
        with self._ip_image_of_call(ip_adapter_image, ip_adapter_image_embeds, body["prompt"], body["prompt_embeds"],
                                    body["num_images_per_prompt"], body["guidance_scale"]), \
                self._pag_of_call(pag_scale, pag_adaptive_scale):
            return self._run_body(**body)

    def _run_body(self, prompt, image, image_pair, height, width, num_inference_steps, timesteps, guidance_scale, negative_prompt,
                  num_images_per_prompt, eta, generator, latents, prompt_embeds, negative_prompt_embeds, output_type,
                  return_dict, cross_attention_kwargs, controlnet_conditioning_scale, guess_mode, control_guidance_start,
                  control_guidance_end, clip_skip, callback_on_step_end, callback_on_step_end_tensor_inputs, kwargs, init=None):
        """The body of __call__.  `image` is the ControlNet query.  init (img2img / inpainting, the subclasses below):
        dict(image=init image, mask=mask image or None, strength=float); None runs the plain text-to-image loop."""
        callback = kwargs.pop("callback", None)
        callback_steps = kwargs.pop("callback_steps", None)
        lora_scale = 1.0
        if cross_attention_kwargs:
            if not self._lora_adapters:
                raise NotImplementedError("cross_attention_kwargs (LoRA scale) needs a LoRA loaded with load_lora_weights")
            extra = sorted(set(cross_attention_kwargs) - {"scale"})
            if extra:
                raise NotImplementedError(f"cross_attention_kwargs: only 'scale' is supported, got {extra}")
            lora_scale = float(cross_attention_kwargs.get("scale", 1.0))
        self._clip_skip = clip_skip
        # 0/1. defaults + checks (pipeline :1033-1062)
        if not isinstance(control_guidance_start, list) and isinstance(control_guidance_end, list):
            control_guidance_start = len(control_guidance_end) * [control_guidance_start]
        elif not isinstance(control_guidance_end, list) and isinstance(control_guidance_start, list):
            control_guidance_end = len(control_guidance_start) * [control_guidance_end]
        elif not isinstance(control_guidance_start, list) and not isinstance(control_guidance_end, list):
            control_guidance_start, control_guidance_end = [control_guidance_start], [control_guidance_end]
        self.check_inputs(prompt, image, image_pair, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds,
                          controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                          callback_on_step_end_tensor_inputs)
        if init is not None:
            self._check_init(init)
        self._guidance_scale = guidance_scale
        if self._lora_adapters or self._lora_merged is not None:
            self._lora_sync(lora_scale)     # adapters x cross_attention_kwargs scale, in the UNet and the text transformer
        # 2. call parameters
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        do_cfg = self.do_classifier_free_guidance
        # 3. text context
        pe, ne = self.encode_prompt(prompt, num_images_per_prompt, do_cfg, negative_prompt, prompt_embeds, negative_prompt_embeds)
        # 3.1 / 4. images: [B,6,H,W] example pair and [B,3,H,W] query, both in [0,1]
        B = batch_size * num_images_per_prompt
        # device_images: the image ends on the GPU.  in_engine: the loop runs inside the engine, so its inputs stay there
        dev_images = self._device_images
        in_engine = dev_images and callback_on_step_end is None and callback is None and (self.scheduler is None or self.fuse_scheduler)
        pair = query = None
        if dev_images:
            query = self._device_image(image, width, height, B, num_images_per_prompt)
            # both halves into one 6-channel tensor, no concat: the first call makes it, the second fills channels 3 .. 5
            pair = self._device_image(image_pair[0], width, height, B, num_images_per_prompt, channels=6)
            if pair is not None and self._device_image(image_pair[1], width, height, B, num_images_per_prompt, out=pair, c_off=3) is None:
                pair = None
        if pair is None:
            pair = np.concatenate([self.prepare_image(im, width, height, B, num_images_per_prompt) for im in image_pair], axis=1)
        if query is None:
            query = self.prepare_image(image, width, height, B, num_images_per_prompt)
        height, width = (int(v) for v in query.shape[-2:])
        if isinstance(generator, EngineGenerator):
            generator.bind(self.engine)
        # 6. latents (img2img / inpainting: the init image's latents first -- its posterior draw comes before the noise draw)
        if init is not None:
            m = self.prepare_mask(init["mask"], width, height, B) if init["mask"] is not None else None
            z0 = self._init_latents(init["image"], width, height, B, generator, device=dev_images)
        x_T = self.prepare_latents(B, self.engine.cfg.in_channels, height, width, generator, latents)
        # 7.2 controlnet_keep gating and per-step scales (pipeline :1196-1202, :1229-1235; controlnet :371-378)
        custom_ts = None
        if self.scheduler is not None:      # plug-in scheduler: its own time grid (retrieve_timesteps, pipeline :101-142, :1164)
            if timesteps is not None:
                if "timesteps" not in set(inspect.signature(self.scheduler.set_timesteps).parameters.keys()):
                    raise ValueError(f"The current scheduler class {self.scheduler.__class__}'s `set_timesteps` does not support custom"
                                     f" timestep schedules. Please check whether you are using the correct scheduler.")
                self.scheduler.set_timesteps(timesteps=timesteps)
            else:
                self.scheduler.set_timesteps(num_inference_steps)
            plan = self._eval_plan(0)
            n_steps = len(plan["grid"])
        else:
            # the engine's own DDIM loop with diffusers' DDIMScheduler grid for SD1.5 (timestep_spacing "leading",
            # steps_offset 1): exactly num_inference_steps entries arange(S) * (T // S) + 1.  For S dividing T this IS the
            # LDM grid of make_ddim_timesteps and the fused default runs; otherwise -- and for a caller-supplied list -- the
            # grid goes to the engine as custom timesteps.
            T = self.engine.cfg.timesteps
            if timesteps is not None:
                custom_ts = [int(t) for t in _to_numpy(timesteps).reshape(-1)]
            elif T % num_inference_steps != 0:
                custom_ts = [int(t) for t in (np.arange(num_inference_steps) * (T // num_inference_steps))[::-1] + 1]
            n_steps = len(custom_ts) if custom_ts is not None else self.engine.num_ddim_steps(num_inference_steps)
        t_start = 0
        if init is not None:
            # get_timesteps: the last int(S * strength) entries of the grid (the engine's DDIM takes them as custom timesteps)
            if self.scheduler is not None:
                full = [int(t) for t in self.scheduler.timesteps]
            elif custom_ts is not None:
                full = custom_ts
            else:
                full = [int(t) for t in self.engine.make_schedule(num_inference_steps)["ddim_timesteps"][::-1]]
            grid, t_start = self.get_timesteps(full, init["strength"])
            if self.scheduler is None:
                custom_ts = grid
            else:
                # set_begin_index ran: the evaluations and the step grid are what the scheduler holds from t_start on (a
                # scheduler with two evaluations in its first step rebuilds its tail there), not a slice of the old list
                plan = self._eval_plan(t_start)
                grid = plan["grid"]
            n_steps = len(grid)
            sa, sb = add_noise_coefficients(self.engine.cfg, grid)
            pure = bool(init["mask"] is not None and (init["strength"] == 1.0 or latents is not None))
        keep = [1.0 - float(i / n_steps < control_guidance_start[0] or (i + 1) / n_steps > control_guidance_end[0])
                for i in range(n_steps)]
        n_ctl = E.PD_NUM_CONTROL
        base = np.logspace(-1, 0, n_ctl).astype(np.float32) if guess_mode else np.ones(n_ctl, np.float32)
        scales_step = np.stack([base * np.float32(controlnet_conditioning_scale) * np.float32(k) for k in keep])
        noise = None
        if eta > 0.0:
            if self.scheduler is None and isinstance(generator, EngineGenerator):
                noise = "engine"         # drawn in the update kernel at (stream "step", draw = step): nothing to make or upload
            elif self.scheduler is None:   # a plug-in scheduler draws its own noise (`generator` is forwarded to step())
                noise = self._randn((n_steps,) + x_T.shape, generator if not isinstance(generator, list) else None)
        if in_engine:     # every pointer of pd_sample_args on the device: uploaded once, here
            x_T, pe, ne, pair, query, noise = (self._to_device(v) for v in (x_T, pe, ne, pair, query, noise))
            if init is not None:
                z0, m = self._to_device(z0), self._to_device(m)
        elif dev_images:  # the per-step driver works on the host: bring what was built on the device back once
            pair, query = _to_numpy(pair), _to_numpy(query)
            if init is not None:
                z0 = _to_numpy(z0)
        kw = dict(x_T=x_T, ctx_cond=pe, ctx_uncond=ne, pair=pair, query=query, steps=num_inference_steps,
                  cfg_scale=float(guidance_scale), eta=float(eta), use_cfg=do_cfg, guess_mode=guess_mode,
                  control_scales_step=scales_step, noise=noise)
        if custom_ts is not None:
            kw["timesteps"] = custom_ts
        host_blend = None
        if init is not None:
            if self.scheduler is not None and not self.fuse_scheduler:
                # a host plug-in scheduler: the start and the per-step blend in NumPy (the engine only evaluates eps)
                kw["x_T"] = x_T if pure else add_noise(z0, x_T, sa[0], sb[0])
                if m is not None:
                    host_blend = dict(z0=z0, eps=x_T, mask=m, sa=sa, sb=sb)
            else:
                kw.update(init_latents=z0, mask=m, init_pure_noise=pure)
        eng = self.engine
        if self.fuse_scheduler:
            # the scheduler's update inside the engine's loop: its grid, the per-step controlnet_keep scales; UniPC draws no noise
            self._check_fusable()
            sched = self.scheduler
            kw.update(eta=0.0, noise=None)
            if getattr(sched, "fused_lms", None) is not None and sched.fused_lms(t_start).get("kind") == "euler_a" \
                    and not isinstance(generator, EngineGenerator):
                raise ValueError("fuse_scheduler=True with EulerAncestralDiscreteScheduler draws its noise inside the engine: pass "
                                 "generator=EngineGenerator(seed)")
            if hasattr(sched, "fused_lms"):
                # a linear multistep scheduler: its step grid and options as pd_lms_args; one engine row per evaluation
                fused = dict(solver="lms", args=sched.fused_lms(t_start), rows=plan["rows"])
                kw.pop("timesteps", None)
                kw.pop("steps", None)
            else:
                kw.update(timesteps=[int(t) for t in sched.timesteps[t_start:]])
                # disable_corrector indexes the whole grid (as the host scheduler after set_begin_index does); the fused rows the tail
                fused = dict(solver="unipc", rows=plan["rows"],
                             args=dict(order=sched.solver_order, solver_type=sched.solver_type, lower_order_final=sched.lower_order_final,
                                       disable_corrector=[d - t_start for d in sched.disable_corrector if d - t_start >= 0]))
            if callback_on_step_end is None and callback is None:
                run = eng.lms_sample if fused["solver"] == "lms" else eng.unipc_sample
                lat = run(**kw, **fused["args"])
            else:
                lat = self._stepwise(kw, scales_step, callback_on_step_end, callback_on_step_end_tensor_inputs, callback,
                                     callback_steps, pe, ne, eta, generator, fused=fused)
        elif self.scheduler is None and callback_on_step_end is None and callback is None:
            lat = eng.ddim_sample(**kw)                                  # 8. the fused loop
        else:
            lat = self._stepwise(kw, scales_step, callback_on_step_end, callback_on_step_end_tensor_inputs, callback,
                                 callback_steps, pe, ne, eta, generator, host_blend=host_blend,
                                 plan=plan if self.scheduler is not None else None)
        # 9. post-processing (pipeline :1298-1321).  The reference's __call__ forces its checker off; here it runs when one was given
        nsfw = None
        if output_type == "latent":
            images = _to_numpy(lat) if in_engine else lat
        elif (self.safety_checker is True and dev_images and output_type == "pil" and self.vae_decode is None
              and getattr(self.engine.cfg, "vae_ch", 0) > 0 and self.engine.vae_weights_missing() == 0
              and E.clip_preprocess_supported(int(lat.shape[2]) * 8, int(lat.shape[3]) * 8, self._safety_size())):
            # as below, with the checker in between, all of it on the device: the stored bytes are what the reference's
            # feature_extractor would be handed; flagged images are overwritten with the value the store maps to black
            from PIL import Image
            dec = self.engine.vae_decode(self._to_device(lat))
            u8 = self.engine.image_store(dec, mul=0.5, add=0.5, rounding="nearest_even")
            nsfw = [bool(f) for f in self.engine.safety_check(u8)]
            if any(nsfw):
                self.engine.safety_blank(dec, nsfw, value=-1.0)
                u8 = self.engine.image_store(dec, mul=0.5, add=0.5, rounding="nearest_even")
            images = [Image.fromarray(im) for im in u8.cpu().numpy()]
        elif (self.safety_checker is None and dev_images and output_type == "pil" and self.vae_decode is None
              and getattr(self.engine.cfg, "vae_ch", 0) > 0 and self.engine.vae_weights_missing() == 0):
            # decode, denormalize, clip, round and the NHWC transpose on the device; only the uint8 pictures come back.  (Never with a
            # checker: a callable one, or pictures the device preprocessing refuses, take the host branch below, which checks them.)
            from PIL import Image
            u8 = self.engine.image_store(self.engine.vae_decode(self._to_device(lat)), mul=0.5, add=0.5, rounding="nearest_even",
                                         host=True)
            images = [Image.fromarray(im) for im in u8]
        else:
            if in_engine:
                lat = _to_numpy(lat)
            if self.vae_decode is not None:
                img = _to_numpy(self.vae_decode(lat / np.float32(self.vae_scaling_factor)))
            elif getattr(self.engine.cfg, "vae_ch", 0) > 0 and self.engine.vae_weights_missing() == 0:
                img = _to_numpy(self.engine.vae_decode(lat))      # divides by scaling_factor itself (ddpm.py:827)
            else:
                raise ValueError('output_type other than "latent" needs first-stage weights in the engine '
                                 "(first_stage_model.decoder.* / post_quant_conv.*) or a vae_decode callable")
            img = np.clip(img / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)      # denormalize, NHWC
            if self.safety_checker is not None:
                # (the reference checks before it denormalises and then skips the denormalisation of the zeroed images: black either way)
                img, nsfw = self.run_safety_checker(np.ascontiguousarray(img))
                img = _to_numpy(img)
                nsfw = None if nsfw is None else [bool(f) for f in nsfw]
                if nsfw is not None and any(nsfw):      # (diffusers' checker zeroes them itself; a callable that does not is not trusted to)
                    img = np.array(img, copy=True)
                    img[np.asarray(nsfw, bool)] = 0
            if output_type == "pil":
                from PIL import Image
                images = [Image.fromarray((im * 255).round().astype("uint8")) for im in img]
            else:
                images = img
        if not return_dict:
            return (images, nsfw)
        return StableDiffusionPipelineOutput(images=images, nsfw_content_detected=nsfw)

    # ------------------------------------------------------------------ per-step driver (callbacks / plug-in schedulers)
    def _eval_plan(self, t_start):
        """The evaluations the plug-in scheduler makes from timesteps[t_start] on, and the sampling steps they form.  Most
        schedulers take one evaluation per step; one that says otherwise through completes_step(index) (PNDMScheduler: two
        evaluations in its first step, at a repeated timestep) has fewer steps than evaluations.  rows: the timestep of every
        evaluation; ends: whether it completes a step; step: the step it belongs to; grid: one timestep per step.  The
        controlnet_keep scales and the inpainting blend follow steps, in the host loop as in the engine's."""
        sched = self.scheduler
        ts = sched.timesteps[t_start:]
        rows = [t.item() if hasattr(t, "item") else t for t in ts]
        rows = [int(t) if float(t) == int(t) else float(t) for t in rows]
        if hasattr(sched, "completes_step"):
            ends = [bool(sched.completes_step(t_start + i)) for i in range(len(rows))]
        else:
            ends = [True] * len(rows)
        step, grid, done = [], [], 0
        for i, e in enumerate(ends):
            if i == 0 or ends[i - 1]:
                grid.append(rows[i])     # the first evaluation of a step is at the step's own timestep
            step.append(done)
            done += int(e)
        return dict(rows=rows, ends=ends, step=step, grid=grid[:done])

    def _stepwise(self, kw, scales_step, cb_end, cb_inputs, cb_legacy, cb_steps, pe, ne, eta, generator, fused=None,
                  host_blend=None, plan=None):
        eng = self.engine
        sched = self.scheduler
        if fused is not None:       # the scheduler's update inside the engine: one engine row per evaluation of the scheduler
            sched = None
            begin = eng.sample_begin_lms if fused["solver"] == "lms" else eng.sample_begin_unipc
            n = begin(**kw, **fused["args"])
            assert n == len(fused["rows"])
            kw = dict(kw, timesteps=fused["rows"])
        elif sched is not None:     # the engine only evaluates eps at the scheduler's timesteps: no DDIM tables needed
            kw = {k: v for k, v in kw.items() if k not in ("control_scales_step", "noise")}
            kw["eta"] = 0.0
            n = eng.sample_begin(**kw)
        else:
            n = eng.sample_begin(**kw)
        if sched is not None:
            ts = plan["rows"]                                    # set_timesteps (and set_begin_index) ran in __call__
            extra = {}
            params = set(inspect.signature(sched.step).parameters.keys())
            if "eta" in params:
                extra["eta"] = eta
            if "generator" in params:
                extra["generator"] = generator
        elif kw.get("timesteps") is not None:
            ts = list(kw["timesteps"])
        else:
            ts = [int(t) for t in np.flip(eng.make_schedule(kw["steps"], kw["eta"])["ddim_timesteps"])]
        lat = None
        for i, t in enumerate(ts):
            if sched is None:
                eng.sample_step(i)
            else:
                # scheduler.scale_model_input is the identity for the DDIM / UniPC families used with SD1.5
                import torch
                j = plan["step"][i]                              # the sampling step this evaluation belongs to
                noise_pred = eng.sample_eps_at(t, scales_step[min(j, len(scales_step) - 1)])
                cur = eng.sample_get(E.PD_GET_LATENTS)
                out = sched.step(torch.from_numpy(np.asarray(noise_pred)), t, torch.from_numpy(np.asarray(cur)), **extra,
                                 return_dict=False)[0]
                out = out.numpy()
                if host_blend is not None and plan["ends"][i]:   # inpainting: the known region back at the next step's noise level
                    hb = host_blend
                    known = hb["z0"] if j == len(plan["grid"]) - 1 else add_noise(hb["z0"], hb["eps"], hb["sa"][j + 1], hb["sb"][j + 1])
                    out = blend_latents(known, out, hb["mask"])
                eng.sample_set_latents(out)
            if cb_end is not None:
                lat = eng.sample_get(E.PD_GET_LATENTS)
                cb_kwargs = {}
                for k in cb_inputs:
                    cb_kwargs[k] = {"latents": lat, "prompt_embeds": pe, "negative_prompt_embeds": ne}[k]
                outs = cb_end(self, i, t, cb_kwargs) or {}
                new = outs.pop("latents", None)
                if new is not None and new is not lat:
                    eng.sample_set_latents(_to_numpy(new))
            if cb_legacy is not None and i % (cb_steps or 1) == 0:
                cb_legacy(i, t, eng.sample_get(E.PD_GET_LATENTS))
        lat = eng.sample_get(E.PD_GET_LATENTS)
        eng.sample_end()
        return lat


class PromptDiffusionImg2ImgPipeline(PromptDiffusionPipeline):
    """Img2img with Prompt-Diffusion's ControlNet, under diffusers' StableDiffusionControlNetImg2ImgPipeline naming: `image` is
    the init image (or its 4-channel latents), `control_image` the query, `image_pair` the example pair.  The loop runs the
    last int(S * strength) steps of the grid from add_noise(z0, eps, t_first) -- strength 1 included.  A given `latents` is
    taken as that noise draw eps (diffusers ignores it).  Everything else is PromptDiffusionPipeline.__call__."""

    def __call__(self, prompt: Union[str, List[str]] = None, image=None, control_image=None, image_pair: List = None,
                 height: Optional[int] = None, width: Optional[int] = None, strength: float = 0.8, num_inference_steps: int = 50,
                 timesteps: List[int] = None, guidance_scale: float = 7.5,
                 negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 clip_skip: Optional[int] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 **kwargs):
        return self._run(prompt=prompt, image=control_image, image_pair=image_pair, height=height, width=width,
                         num_inference_steps=num_inference_steps, timesteps=timesteps, guidance_scale=guidance_scale,
                         negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator,
                         latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                         ip_adapter_image=ip_adapter_image, ip_adapter_image_embeds=ip_adapter_image_embeds, output_type=output_type,
                         return_dict=return_dict,
                         cross_attention_kwargs=cross_attention_kwargs, controlnet_conditioning_scale=controlnet_conditioning_scale,
                         guess_mode=guess_mode, control_guidance_start=control_guidance_start,
                         control_guidance_end=control_guidance_end, clip_skip=clip_skip, callback_on_step_end=callback_on_step_end,
                         callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, pag_scale=pag_scale,
                         pag_adaptive_scale=pag_adaptive_scale, kwargs=kwargs,
                         init=dict(image=image, mask=None, strength=strength))


class PromptDiffusionInpaintPipeline(PromptDiffusionPipeline):
    """Inpainting with Prompt-Diffusion's ControlNet and the 4-channel UNet, under diffusers'
    StableDiffusionControlNetInpaintPipeline naming: `image` is the init image (or its 4-channel latents), `mask_image` the
    region to repaint (white = 1 = repaint, binarized at 0.5), `control_image` the query.  After every step the kept region is
    put back at the next step's noise level (z0 itself after the last step); the loop starts from pure noise at strength 1 (or
    from a given `latents`, which is also the noise draw), from add_noise(z0, eps, t_first) otherwise.  Not built: 9-channel
    inpainting UNets (masked_image_latents) and padding_mask_crop."""

    def __call__(self, prompt: Union[str, List[str]] = None, image=None, mask_image=None, control_image=None,
                 image_pair: List = None, height: Optional[int] = None, width: Optional[int] = None, strength: float = 1.0,
                 num_inference_steps: int = 50, timesteps: List[int] = None, guidance_scale: float = 7.5,
                 negative_prompt: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0, control_guidance_end: Union[float, List[float]] = 1.0,
                 clip_skip: Optional[int] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 **kwargs):
        if kwargs.get("padding_mask_crop") is not None or kwargs.get("masked_image_latents") is not None:
            raise NotImplementedError("padding_mask_crop / masked_image_latents (9-channel inpainting UNets) are not supported")
        kwargs.pop("padding_mask_crop", None)
        kwargs.pop("masked_image_latents", None)
        if mask_image is None:
            raise ValueError("`mask_image` must be passed")
        return self._run(prompt=prompt, image=control_image, image_pair=image_pair, height=height, width=width,
                         num_inference_steps=num_inference_steps, timesteps=timesteps, guidance_scale=guidance_scale,
                         negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator,
                         latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                         ip_adapter_image=ip_adapter_image, ip_adapter_image_embeds=ip_adapter_image_embeds, output_type=output_type,
                         return_dict=return_dict,
                         cross_attention_kwargs=cross_attention_kwargs, controlnet_conditioning_scale=controlnet_conditioning_scale,
                         guess_mode=guess_mode, control_guidance_start=control_guidance_start,
                         control_guidance_end=control_guidance_end, clip_skip=clip_skip, callback_on_step_end=callback_on_step_end,
                         callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, pag_scale=pag_scale,
                         pag_adaptive_scale=pag_adaptive_scale, kwargs=kwargs,
                         init=dict(image=image, mask=mask_image, strength=strength))
