"""Host-side mirror of the reference's SD3 pipeline surface over the engine's SD3 path.

`StableDiffusion3PromptDiffusionPipeline.__call__` keeps the keyword names, defaults, argument normalisation and error
behaviour of promptdiffusioncontrolnetpipeline_sd3.py:853-1283 for everything that concerns the denoising path; what the
reference does with modules outside the path is injected as callables (the boundary of DESIGN.md §7 N4):

  encode_prompt(prompt, prompt_2, prompt_3, negative_prompt, negative_prompt_2, negative_prompt_3, do_classifier_free_guidance,
                num_images_per_prompt, clip_skip, max_sequence_length)
        -> (prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds)   (:1059-1082)
  vae_encode(images [B, 3, H, W] in [-1, 1]) -> latents [B, 16, H/8, W/8]      (vae.encode(...).latent_dist.sample(), :1126)
  vae_decode(latents) -> images in [-1, 1]                                       (vae.decode, :1270)
  down_proj(pair [B, 6, H, W]) -> [B, 3, H, W]                                   (controlnet.down_proj, encode_support_pair :189-198)

Without an injected `encode_prompt`, an engine with text encoders (`SD3Engine.configure_text`) and `tokenizers=(tok_l, tok_g, tok_t5)`
-- callables taking `(list[str], max_length)` and returning int ids `[B, max_length]`; `tok_t5` may be None on an engine without T5 --
make `prompt=` strings work: the pipeline does what the reference's encode_prompt (:351-545) does around the encoders (prompt_2 / prompt_3
fallbacks, the negative prompt with its checks, the negative pass at clip_skip None, the per-image repeat, max_sequence_length) and the
engine encodes (`SD3Engine.encode_prompt_ids`).  An injected `encode_prompt` keeps precedence.

Likewise the image ends: without injected `vae_encode` / `vae_decode` / `down_proj`, an engine with SD3's VAE (`SD3Engine.configure_vae`)
encodes `control_image` images and image pairs (`vae_encode(..., raw=True)`, `encode_support_pair`) and decodes for `output_type` "pil",
"np" and "pt" (`vae_decode(..., raw=True)`).  The shift / scaling arithmetic stays here in both cases, applied once; the two factors
default to the engine's VAE configuration.  Injected callables keep precedence; with neither, the ValueErrors below stay.

The three steps of the loop body (controlnet, transformer, CFG + scheduler.step; :1192-1245) run inside the engine
(`SD3Engine.sample`); with `callback_on_step_end` the loop is driven step by step from here (`SD3Engine.forward` + the same
Euler update) so that the callback can replace the latents or the embeddings (:1247-1258).  Arrays are NumPy (torch tensors
are converted).  Not supported, raising NotImplementedError like the SD1.5 mirror does for options outside the path:
`ip_adapter_image(_embeds)`.  `joint_attention_kwargs={"scale": s}` scales the adapters of `load_lora_weights`.

`StableDiffusion3PromptDiffusionImg2ImgPipeline(image=, strength=)` and `StableDiffusion3PromptDiffusionInpaintPipeline(image=,
mask_image=, strength=)` add diffusers' SD3 img2img and (16-channel) inpainting to the same call: the grid is truncated by `strength`,
the loop starts from sigma_0 eps + (1 - sigma_0) z0 and, with a mask, every step ends with (1 - m) k_i + m x (include/pdengine.h,
pd_sd3_loop_args) -- inside the engine's loop, or in NumPy float32 in the same order on the callback path.  `generator=EngineGenerator(seed)`
makes every draw the engine's (the start latents of the plain pipeline too); in the edited loops eps is then drawn inside the update kernel."""
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np

from . import engine as E
from .lora_pipeline import AdapterMixin
from .pipeline import EngineGenerator, prepare_inpaint_mask
from .sd3 import SD3Engine, flow_match_sigmas, img2img_start

_CALLBACK_TENSOR_INPUTS = ["latents", "prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds"]


def _np(x, dtype=np.float32):
    return None if x is None else np.ascontiguousarray(E._to_host(x), dtype=dtype)


def _image_array(x):
    """PIL images (one or a list) and uint8 arrays become float arrays in [0, 1] (VaeImageProcessor's pil_to_numpy); everything else
    passes through."""
    if isinstance(x, (list, tuple)) and x and hasattr(x[0], "convert"):
        return np.stack([np.asarray(i.convert("RGB"), np.float32) / 255.0 for i in x])
    if hasattr(x, "convert"):
        return np.asarray(x.convert("RGB"), np.float32)[None] / 255.0
    if isinstance(x, np.ndarray) and x.dtype == np.uint8:
        return x.astype(np.float32) / 255.0
    return x


class StableDiffusion3PromptDiffusionPipeline(AdapterMixin):
    _callback_tensor_inputs = _CALLBACK_TENSOR_INPUTS

    def __init__(self, engine: SD3Engine, encode_prompt: Optional[Callable] = None, vae_encode: Optional[Callable] = None,
                 vae_decode: Optional[Callable] = None, down_proj: Optional[Callable] = None, vae_scaling_factor: Optional[float] = None,
                 vae_shift_factor: Optional[float] = None, vae_scale_factor: int = 8, shift: float = 3.0, tokenizers=None,
                 tokenizer_max_length: int = 77):
        self.engine = engine
        self.tokenizers, self.tokenizer_max_length = tokenizers, tokenizer_max_length
        self.encode_prompt, self.vae_encode, self.vae_decode, self.down_proj = encode_prompt, vae_encode, vae_decode, down_proj
        vcfg = getattr(engine, "vae_cfg", None)   # None: the published SD3 values
        if vae_scaling_factor is None:
            vae_scaling_factor = vcfg.scaling_factor if vcfg is not None else 1.5305
        if vae_shift_factor is None:
            vae_shift_factor = vcfg.shift_factor if vcfg is not None else 0.0609
        self.vae_scaling_factor, self.vae_shift_factor, self.vae_scale_factor = vae_scaling_factor, vae_shift_factor, vae_scale_factor
        self.shift = shift
        self._guidance_scale, self._clip_skip, self._num_timesteps, self._interrupt = 7.0, None, 0, False
        self._lora_init()      # adapters (load_lora_weights; lora_pipeline.AdapterMixin)

    # ------------------------------------------------------------------ LoRA (diffusers SD3LoraLoaderMixin surface)
    _lora_component_names = ("transformer", "text_encoder", "text_encoder_2")

    def _lora_parse(self, src):
        """diffusers / PEFT keys (transformer., text_encoder., text_encoder_2.) -> the engine's tensors; T5 and the ControlNet are
        not targets"""
        from . import lora as L
        return L.parse_sd3_adapters(src, self.engine.cfg, getattr(self.engine, "text_cfg", None))

    def _lora_components(self, names):
        comps = {c: any(k.startswith(c + ".") for k in names) for c in self._lora_component_names}
        if (comps["text_encoder"] or comps["text_encoder_2"]) and self.encode_prompt is not None:
            raise ValueError("this LoRA has text-encoder layers, but an `encode_prompt` callable is attached; only the engine's own "
                             "text encoders can take them")
        return comps

    # ------------------------------------------------------------------ properties of the reference pipeline
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def clip_skip(self):
        return self._clip_skip

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def interrupt(self):
        return self._interrupt

    # ------------------------------------------------------------------ check_inputs (:541-633)
    def check_inputs(self, prompt, prompt_2, prompt_3, height, width, negative_prompt=None, negative_prompt_2=None,
                     negative_prompt_3=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                     negative_pooled_prompt_embeds=None, callback_on_step_end_tensor_inputs=None, max_sequence_length=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found {bad}")
        for name, p in (("prompt", prompt), ("prompt_2", prompt_2), ("prompt_3", prompt_3)):
            if p is not None and prompt_embeds is not None:
                raise ValueError(f"Cannot forward both `{name}`: {p} and `prompt_embeds`. Please make sure to only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        for name, p in (("prompt", prompt), ("prompt_2", prompt_2), ("prompt_3", prompt_3)):
            if p is not None and not isinstance(p, (str, list)):
                raise ValueError(f"`{name}` has to be of type `str` or `list` but is {type(p)}")
        for name, p in (("negative_prompt", negative_prompt), ("negative_prompt_2", negative_prompt_2), ("negative_prompt_3", negative_prompt_3)):
            if p is not None and negative_prompt_embeds is not None:
                raise ValueError(f"Cannot forward both `{name}`: {p} and `negative_prompt_embeds`. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None and tuple(prompt_embeds.shape) != tuple(negative_prompt_embeds.shape):
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but got: "
                             f"`prompt_embeds` {tuple(prompt_embeds.shape)} != `negative_prompt_embeds` {tuple(negative_prompt_embeds.shape)}.")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.")
        if negative_prompt_embeds is not None and negative_pooled_prompt_embeds is None:
            raise ValueError("If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed.")
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f"`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}")

    # ------------------------------------------------------------------ encode_prompt (:351-545) over the engine's encoders
    def _engine_encodes(self) -> bool:
        return self.tokenizers is not None and getattr(self.engine, "text_cfg", None) is not None

    def _encode_ids(self, prompt, prompt_2, prompt_3, clip_skip, max_sequence_length):
        """_get_clip_prompt_embeds x 2 + _get_t5_prompt_embeds + the cat / pad / cat of :457-471, for lists of strings."""
        tok_l, tok_g, tok_t5 = self.tokenizers
        ids_l = np.asarray(tok_l(prompt, self.tokenizer_max_length))
        ids_g = np.asarray(tok_g(prompt_2, self.tokenizer_max_length))
        ids_t5 = None
        if self.engine.text_cfg.t5 is not None:
            if tok_t5 is None:
                raise ValueError("the engine has a T5 encoder: `tokenizers` needs its tokenizer as third entry")
            ids_t5 = np.asarray(tok_t5(prompt_3, max_sequence_length))
        pe, pooled = self.engine.encode_prompt_ids(ids_l, ids_g, ids_t5, clip_skip=clip_skip)
        return _np(pe), _np(pooled)

    def _encode_prompt_engine(self, prompt, prompt_2, prompt_3, negative_prompt, negative_prompt_2, negative_prompt_3,
                              do_classifier_free_guidance, num_images_per_prompt, clip_skip, max_sequence_length, skip_negative=False):
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        prompt_2 = prompt_2 or prompt
        prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
        prompt_3 = prompt_3 or prompt
        prompt_3 = [prompt_3] if isinstance(prompt_3, str) else prompt_3
        pe, ppe = self._encode_ids(prompt, prompt_2, prompt_3, clip_skip, max_sequence_length)
        # repeat(1, n, 1).view(B * n, L, -1) (:289-290, :342-346): the copies of one prompt are neighbours
        pe, ppe = np.repeat(pe, num_images_per_prompt, 0), np.repeat(ppe, num_images_per_prompt, 0)
        npe = nppe = None
        if do_classifier_free_guidance and not skip_negative:
            negative_prompt = negative_prompt or ""
            negative_prompt_2 = negative_prompt_2 or negative_prompt
            negative_prompt_3 = negative_prompt_3 or negative_prompt
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
            negative_prompt_3 = batch_size * [negative_prompt_3] if isinstance(negative_prompt_3, str) else negative_prompt_3
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            npe, nppe = self._encode_ids(negative_prompt, negative_prompt_2, negative_prompt_3, None, max_sequence_length)
            npe, nppe = np.repeat(npe, num_images_per_prompt, 0), np.repeat(nppe, num_images_per_prompt, 0)
        return pe, npe, ppe, nppe

    # ------------------------------------------------------------------ host pieces of steps 3 and 5
    def prepare_image(self, image, batch_size, num_images_per_prompt):
        """prepare_image (:666-698) without the CFG doubling (the engine doubles internally): torch tensors pass unchanged
        like in the reference; other arrays ([B, H, W, 3] or [B, 3, H, W] in [0, 1]) get VaeImageProcessor's normalisation to
        [-1, 1].  Resizing is the caller's."""
        as_is = E._is_torch(image)
        img = _np(_image_array(image))
        if img.ndim == 3:
            img = img[None]
        if img.shape[-1] == 3 and img.shape[1] != 3:
            img = img.transpose(0, 3, 1, 2)
        if not as_is:
            img = 2.0 * img - 1.0
        repeat_by = batch_size if img.shape[0] == 1 else num_images_per_prompt
        return np.ascontiguousarray(np.repeat(img, repeat_by, axis=0), np.float32)

    # ------------------------------------------------------------------ the image ends: injected callables first, then the engine's VAE
    def _engine_has_vae(self, encoder: bool) -> bool:
        return getattr(self.engine, "vae_cfg", None) is not None and (not encoder or getattr(self.engine, "vae_has_encoder", False))

    def _engine_vae(self, what: str):
        """The engine whose VAE the four switches below act on; ValueError where the VAE is the caller's."""
        if not self._engine_has_vae(False):
            if self.vae_decode is not None or self.vae_encode is not None:
                raise ValueError(f"{what} acts on the engine's VAE, but this pipeline runs the injected `vae_decode` / `vae_encode` callables "
                                 "and its engine has no VAE (SD3Engine.configure_vae): switch tiling / slicing on in the callables' own VAE")
            raise ValueError(f"{what} needs an engine with SD3's VAE (SD3Engine.configure_vae)")
        return self.engine

    def enable_vae_slicing(self):
        """vae.enable_slicing(): each sample of a batch is decoded / encoded on its own (SD3Engine.set_vae_slicing)."""
        self._engine_vae("enable_vae_slicing").set_vae_slicing(True)

    def disable_vae_slicing(self):
        self._engine_vae("disable_vae_slicing").set_vae_slicing(False)

    def enable_vae_tiling(self):
        """vae.enable_tiling(): images above 1024 pixels per side are decoded / encoded in overlapping tiles (SD3Engine.set_vae_tiling)."""
        st = self._engine_vae("enable_vae_tiling").vae_tiling
        self.engine.set_vae_tiling(True, st.tile_latent, st.overlap_factor, st.tile_batch)

    def disable_vae_tiling(self):
        st = self._engine_vae("disable_vae_tiling").vae_tiling
        self.engine.set_vae_tiling(False, st.tile_latent, st.overlap_factor, st.tile_batch)

    def _vae_encode_fn(self):
        if self.vae_encode is not None:
            return self.vae_encode
        if self._engine_has_vae(True):
            return lambda x: self.engine.vae_encode(x, mode="sample", raw=True)   # shift and scaling are applied here
        return None

    def _vae_decode_fn(self):
        if self.vae_decode is not None:
            return self.vae_decode
        if self._engine_has_vae(False):
            return lambda z: self.engine.vae_decode(z, raw=True)
        return None

    def _to_latents(self, x, batch_size, num_images_per_prompt, shift, pair=False):
        """Control conditions: 16-channel arrays are taken as latents already; images go through (down_proj +) vae_encode and
        (x - shift_factor) * scaling_factor (:1112-1127)."""
        C = self.engine.cfg.in_channels
        if not pair:
            x, known_image = _image_array(x), _image_array(x) is not x      # a PIL / uint8 input is an image whatever its size
            a = _np(x)
            if not known_image and a.ndim == 4 and a.shape[1] == C:
                return np.ascontiguousarray(np.repeat(a, batch_size * num_images_per_prompt if a.shape[0] == 1 else num_images_per_prompt, axis=0))
            encode = self._vae_encode_fn()
            if encode is None:
                raise ValueError(f"`control_image` must be [{C}]-channel latents unless the pipeline was given `vae_encode`")
            lat = _np(encode(self.prepare_image(x, batch_size * num_images_per_prompt, num_images_per_prompt)))
            return ((lat - shift) * self.vae_scaling_factor).astype(np.float32)
        if not isinstance(x, (list, tuple)):
            a = _np(x)
            if a.ndim == 4 and a.shape[1] == C:
                return np.ascontiguousarray(np.repeat(a, batch_size * num_images_per_prompt if a.shape[0] == 1 else num_images_per_prompt, axis=0))
            raise ValueError("`control_image_pair` must be a list of two images (or pair latents)")
        if len(x) != 2:
            raise ValueError("`control_image_pair` must hold exactly two images")
        encode = self._vae_encode_fn()
        if encode is None or (self.down_proj is None and not self._engine_has_vae(True)):
            raise ValueError("image pairs need `vae_encode` and `down_proj`; pass pair latents otherwise")
        imgs = [self.prepare_image(i, batch_size * num_images_per_prompt, num_images_per_prompt) for i in x]
        if self.down_proj is not None:
            lat = _np(encode(_np(self.down_proj(np.concatenate(imgs, axis=1)))))      # encode_support_pair (:189-198)
        elif self.vae_encode is not None:
            lat = _np(encode(_np(self.engine.down_proj(imgs[0], imgs[1]))))
        else:
            lat = _np(self.engine.encode_support_pair(imgs[0], imgs[1]))              # down_proj, then vae_encode(raw=True)
        return ((lat - shift) * self.vae_scaling_factor).astype(np.float32)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, generator, latents=None):
        if latents is not None:
            return _np(latents)
        shape = (batch_size, num_channels_latents, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if generator is None:
            generator = np.random.default_rng()
        if isinstance(generator, list):
            return np.concatenate([self._randn(g, (1,) + shape[1:]) for g in generator], 0)
        return self._randn(generator, shape)

    @staticmethod
    def _randn(g, shape):
        if isinstance(g, EngineGenerator):          # bound by __call__; the start latents / the img2img noise: stream "xt"
            return np.asarray(g.randn(shape, stream="xt"), np.float32)
        if isinstance(g, np.random.Generator):
            return g.standard_normal(shape).astype(np.float32)
        import torch   # a torch.Generator, as the reference takes
        return torch.randn(shape, generator=g, device=g.device).float().cpu().numpy()

    def _init_z0(self, image, batch, height, width, generator):
        """z0 of img2img / inpainting, [batch, C, height / 8, width / 8]: C-channel arrays are latents and taken as they are (as diffusers
        does); images (PIL, uint8, float arrays in [0, 1]) are encoded -- by the injected `vae_encode`, else by the engine's VAE with a
        posterior sample drawn from `generator` -- and become (latents - shift_factor) * scaling_factor, always with the VAE's real
        shift factor.  Fewer images than `batch` are repeated as a whole (diffusers' torch.cat of the init latents)."""
        C, f = self.engine.cfg.in_channels, self.vae_scale_factor
        x = _image_array(image)
        a = _np(x)
        if x is image and a.ndim == 4 and a.shape[1] == C:
            z = a
        else:
            img = self.prepare_image(x, 1, 1)
            if tuple(img.shape[-2:]) != (height, width):
                raise ValueError(f"`image` is {img.shape[-1]}x{img.shape[-2]}, the control image {width}x{height}")
            if self.vae_encode is not None:
                lat = _np(self.vae_encode(img))
            elif self._engine_has_vae(True):
                gen = generator[:img.shape[0]] if isinstance(generator, list) else generator
                # an EngineGenerator: the posterior kernel draws at stream "vae" itself
                noise = None if isinstance(gen, EngineGenerator) else self.prepare_latents(img.shape[0], C, height, width, gen)
                lat = _np(self.engine.vae_encode(img, mode="sample", noise=noise, raw=True))
            else:
                raise ValueError(f"an init `image` needs `vae_encode` or an engine with SD3's VAE encoder; pass [{C}]-channel latents otherwise")
            z = ((lat - self.vae_shift_factor) * self.vae_scaling_factor).astype(np.float32)
        if tuple(z.shape[1:]) != (C, height // f, width // f):
            raise ValueError(f"`image` latents must be [B, {C}, {height // f}, {width // f}], got {list(z.shape)}")
        if z.shape[0] != batch:
            if batch % z.shape[0]:
                raise ValueError(f"Cannot duplicate `image` of batch size {z.shape[0]} to {batch} images; the batch size must divide it.")
            z = np.tile(z, (batch // z.shape[0], 1, 1, 1))
        return np.ascontiguousarray(z, np.float32)

    def _sigmas(self, num_inference_steps, sigmas):
        """retrieve_timesteps(scheduler, num_inference_steps, sigmas=sigmas) on FlowMatchEulerDiscreteScheduler: custom sigmas
        are shifted like the default grid and terminated with 0."""
        if sigmas is None:
            return flow_match_sigmas(num_inference_steps, self.shift), num_inference_steps
        s = np.asarray(sigmas, np.float64)
        s = self.shift * s / (1.0 + (self.shift - 1.0) * s)
        return np.concatenate([s, [0.0]]).astype(np.float32), len(s)

    # ------------------------------------------------------------------ __call__ (:853-1283)
    def __call__(self, prompt: Union[str, List[str]] = None, prompt_2=None, prompt_3=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 28, sigmas: Optional[List[float]] = None,
                 guidance_scale: float = 7.0, control_guidance_start: Union[float, List[float]] = 0.0,
                 control_guidance_end: Union[float, List[float]] = 1.0, control_image=None, control_image_pair=None,
                 controlnet_conditioning_scale: Union[float, List[float]] = 1.0, controlnet_pooled_projections=None,
                 negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None, num_images_per_prompt: Optional[int] = 1,
                 generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_pooled_prompt_embeds=None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                 clip_skip: Optional[int] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 256, _edit: Optional[dict] = None,
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0):
        """_edit: set by the img2img / inpaint subclasses -- {"image", "strength", "mask_image"}."""
        if pag_scale:
            raise NotImplementedError("pag_scale: perturbed-attention guidance is built for the SD1.5 pipelines only (not the MMDiT path)")
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            raise NotImplementedError("ip_adapter_image / ip_adapter_image_embeds are outside the engine's path")
        lora_scale = 1.0
        if joint_attention_kwargs:
            if not self._lora_adapters:
                raise NotImplementedError("joint_attention_kwargs (LoRA scale) needs a LoRA loaded with load_lora_weights")
            if set(joint_attention_kwargs) - {"scale"}:
                raise NotImplementedError(f"joint_attention_kwargs: only 'scale' is supported, got {sorted(joint_attention_kwargs)}")
            lora_scale = float(joint_attention_kwargs.get("scale", 1.0))
        if self._lora_adapters or self._lora_merged is not None:
            self._lora_sync(lora_scale)     # adapters x joint_attention_kwargs scale, in the transformer and the CLIP encoders
        cfg = self.engine.cfg
        if control_image is None or control_image_pair is None:
            raise ValueError("`control_image` and `control_image_pair` are required (the reference asserts a SD3PromptDiffusionModel)")
        # default size: the control latents / image decide (the reference overrides height, width from the control image, :1123)
        ci = _np(_image_array(control_image))
        if ci.ndim == 3:
            ci = ci[None]
        if _image_array(control_image) is not control_image:
            h_img, w_img = ci.shape[1:3]                                   # PIL / uint8: [B, H, W, 3]
        elif ci.shape[1] == cfg.in_channels:
            h_img, w_img = ci.shape[-2] * self.vae_scale_factor, ci.shape[-1] * self.vae_scale_factor
        elif ci.shape[1] == 3:
            h_img, w_img = ci.shape[-2:]
        else:
            h_img, w_img = ci.shape[1:3]
        height, width = height or h_img, width or w_img
        # align format for control guidance (:1016-1025); the single-ControlNet reference uses element 0
        if isinstance(control_guidance_start, list) or isinstance(control_guidance_end, list):
            if not isinstance(control_guidance_start, list):
                control_guidance_start = len(control_guidance_end) * [control_guidance_start]
            if not isinstance(control_guidance_end, list):
                control_guidance_end = len(control_guidance_start) * [control_guidance_end]
            control_guidance_start, control_guidance_end = control_guidance_start[0], control_guidance_end[0]
        if isinstance(controlnet_conditioning_scale, list):
            controlnet_conditioning_scale = controlnet_conditioning_scale[0]
        # 1. check inputs
        self.check_inputs(prompt, prompt_2, prompt_3, height, width, negative_prompt, negative_prompt_2, negative_prompt_3,
                          prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds,
                          callback_on_step_end_tensor_inputs, max_sequence_length)
        self._guidance_scale, self._clip_skip, self._interrupt = guidance_scale, clip_skip, False
        # 2. call parameters
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None:
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        cfg_on = self.do_classifier_free_guidance
        if prompt is not None:
            if self.encode_prompt is None and not self._engine_encodes():
                raise ValueError("text prompts need the `encode_prompt` callable; pass `prompt_embeds` / `pooled_prompt_embeds` otherwise")
            encode = self.encode_prompt if self.encode_prompt is not None else self._encode_prompt_engine
            given_negative = (negative_prompt_embeds, negative_pooled_prompt_embeds)
            extra = {"skip_negative": True} if self.encode_prompt is None and negative_prompt_embeds is not None else {}
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = encode(
                prompt=prompt, prompt_2=prompt_2, prompt_3=prompt_3, negative_prompt=negative_prompt, negative_prompt_2=negative_prompt_2,
                negative_prompt_3=negative_prompt_3, do_classifier_free_guidance=cfg_on, num_images_per_prompt=num_images_per_prompt,
                clip_skip=clip_skip, max_sequence_length=max_sequence_length, **extra)
            if self.encode_prompt is None and given_negative[0] is not None:
                # negative embeddings given next to prompt strings are returned as they came (:473: only a missing one is encoded)
                negative_prompt_embeds, negative_pooled_prompt_embeds = given_negative
            rep = 1
        else:
            rep = num_images_per_prompt          # encode_prompt repeats given embeddings per image (:397-399 of diffusers' encode_prompt)
        pe, ppe = np.repeat(_np(prompt_embeds), rep, 0), np.repeat(_np(pooled_prompt_embeds), rep, 0)
        if cfg_on:
            if negative_prompt_embeds is None or negative_pooled_prompt_embeds is None:
                raise ValueError("guidance_scale > 1 with `prompt_embeds` needs `negative_prompt_embeds` and `negative_pooled_prompt_embeds`")
            npe, nppe = np.repeat(_np(negative_prompt_embeds), rep, 0), np.repeat(_np(negative_pooled_prompt_embeds), rep, 0)
        else:
            npe = nppe = None
        B = batch_size * num_images_per_prompt
        # 3. control conditions (no shift factor under force_zeros_for_pooled_projection, :1084-1088)
        vshift = 0.0 if cfg.force_zeros_for_pooled_projection else self.vae_shift_factor
        pair_lat = self._to_latents(control_image_pair, batch_size, num_images_per_prompt, vshift, pair=True)
        cond_lat = self._to_latents(control_image, batch_size, num_images_per_prompt, vshift)
        if cond_lat.shape[0] != B or pair_lat.shape[0] != B:
            raise ValueError(f"control conditions have batch {cond_lat.shape[0]} / {pair_lat.shape[0]}, expected {B}")
        height, width = cond_lat.shape[-2] * self.vae_scale_factor, cond_lat.shape[-1] * self.vae_scale_factor
        # 4. timesteps
        sig, num_inference_steps = self._sigmas(num_inference_steps, sigmas)
        if _edit is not None:        # get_timesteps of diffusers' SD3 img2img: the loop runs on the tail of the grid
            t_start = img2img_start(num_inference_steps, _edit["strength"])
            sig, num_inference_steps = np.ascontiguousarray(sig[t_start:]), num_inference_steps - t_start
        self._num_timesteps = num_inference_steps
        # 5. latents
        if isinstance(generator, EngineGenerator):
            generator.bind(self.engine)
        z0 = mask = None
        from_seed = False
        if _edit is not None:
            # z0 first, then the noise, in the order diffusers' prepare_latents draws them; `latents`, when given, is the noise eps
            z0 = self._init_z0(_edit["image"], B, height, width, generator)
            if _edit.get("mask_image") is not None:
                mask = prepare_inpaint_mask(_edit["mask_image"], width, height, B, self.vae_scale_factor)
            # the engine's generator in the fused loop: eps is drawn inside the update kernel, no tensor is made
            from_seed = isinstance(generator, EngineGenerator) and latents is None and callback_on_step_end is None
            if tuple(z0.shape) != tuple(cond_lat.shape):
                raise ValueError(f"`image` latents {tuple(z0.shape)} and control latents {tuple(cond_lat.shape)} differ")
        if not from_seed:
            latents = self.prepare_latents(B, cfg.in_channels, height, width, generator, latents)
            if tuple(latents.shape) != tuple(cond_lat.shape):
                raise ValueError(f"latents {tuple(latents.shape)} and control latents {tuple(cond_lat.shape)} differ")
        cn_pooled = None
        if not cfg.force_zeros_for_pooled_projection and controlnet_pooled_projections is not None:
            cn_pooled = _np(controlnet_pooled_projections)
        # 8. denoising loop
        if callback_on_step_end is None:
            latents = self.engine.sample(latents, pe, ppe, npe, nppe, control_latents=cond_lat, pair_latents=pair_lat,
                                         num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                         controlnet_conditioning_scale=controlnet_conditioning_scale, sigmas=sig,
                                         control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                                         controlnet_pooled_projections=cn_pooled, init_latents=z0, mask=mask, from_seed=from_seed)
        else:
            n = num_inference_steps
            one = np.float32(1.0)
            if z0 is not None:       # the start state and, below, the blend: float32, in the order of the engine's update kernel
                eps = latents
                latents = sig[0] * eps + (one - sig[0]) * z0
            for i in range(n):
                if self._interrupt:
                    continue
                keep = 1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end)
                t = np.full((2 * B if cfg_on else B,), sig[i] * 1000.0, np.float32)
                x_in = np.concatenate([latents, latents]) if cfg_on else latents
                ctx = np.concatenate([npe, pe]) if cfg_on else pe
                pooled = np.concatenate([nppe, ppe]) if cfg_on else ppe
                dup = (lambda a: np.concatenate([a, a])) if cfg_on else (lambda a: a)
                v = self.engine.forward(x_in, t, ctx, pooled, dup(cond_lat), dup(pair_lat), controlnet_conditioning_scale * keep,
                                        controlnet_pooled_projections=cn_pooled)
                if cfg_on:
                    v = v[:B] + np.float32(guidance_scale) * (v[B:] - v[:B])
                latents = (latents + (sig[i + 1] - sig[i]) * v).astype(np.float32)
                if mask is not None:
                    known = (one - sig[i + 1]) * z0 + sig[i + 1] * eps
                    latents = (one - mask) * known + mask * latents
                kw = {k: {"latents": latents, "prompt_embeds": pe, "negative_prompt_embeds": npe,
                          "negative_pooled_prompt_embeds": nppe}[k] for k in callback_on_step_end_tensor_inputs}
                out = callback_on_step_end(self, i, float(sig[i] * 1000.0), kw) or {}
                latents = _np(out.pop("latents", latents))
                pe = _np(out.pop("prompt_embeds", pe))
                npe = _np(out.pop("negative_prompt_embeds", npe)) if cfg_on else npe
                nppe = _np(out.pop("negative_pooled_prompt_embeds", nppe)) if cfg_on else nppe
        # post
        if output_type == "latent":
            image = latents
        else:
            decode = self._vae_decode_fn()
            if decode is None:
                raise ValueError('output_type other than "latent" needs the `vae_decode` callable')
            image = _np(decode(latents / self.vae_scaling_factor + self.vae_shift_factor))
            image = np.clip(image / 2 + 0.5, 0.0, 1.0)            # postprocess (:823-851)
            if output_type != "pt":
                image = image.transpose(0, 2, 3, 1)
            if output_type == "pil":
                from PIL import Image
                image = [Image.fromarray((im * 255).round().astype("uint8")) for im in image]
        if not return_dict:
            return (image,)
        return {"images": image}


class StableDiffusion3PromptDiffusionImg2ImgPipeline(StableDiffusion3PromptDiffusionPipeline):
    """diffusers' StableDiffusion3Img2ImgPipeline on the Prompt-Diffusion ControlNet path: every argument of the base __call__, plus
    `image` (PIL, uint8 / float arrays, or [B, C, h, w] latents used as z0 directly) and `strength`: the loop runs the last
    int(min(n * strength, n)) steps of the grid from sigma_0 eps + (1 - sigma_0) z0.  `latents`, when given, is the noise eps."""

    def __call__(self, *args, image=None, strength: float = 0.6, **kwargs):
        if image is None:
            raise ValueError("`image` must be passed")
        return super().__call__(*args, _edit={"image": image, "strength": float(strength)}, **kwargs)


class StableDiffusion3PromptDiffusionInpaintPipeline(StableDiffusion3PromptDiffusionPipeline):
    """diffusers' StableDiffusion3InpaintPipeline for a 16-channel transformer (no masked_image_latents): the img2img pipeline plus
    `mask_image` (white = repaint; grayscale, binarised at 0.5, nearest resize to the latent grid, as the SD1.5 inpaint pipeline prepares
    it).  After every step the kept region is reset to z0 noised to the next sigma with the call's one eps; at the end it is z0."""

    def __call__(self, *args, image=None, mask_image=None, strength: float = 0.6, **kwargs):
        if image is None or mask_image is None:
            raise ValueError("`image` and `mask_image` must be passed")
        return super().__call__(*args, _edit={"image": image, "mask_image": mask_image, "strength": float(strength)}, **kwargs)
