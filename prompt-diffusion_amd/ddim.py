"""(L)-path host surface: ``ControlLDM`` + ``DDIMSampler`` look-alikes over the HIP engine.

Mirrors the reference call (run_prompt_diffusion.ipynb cell 5; cldm/ddim_hacked.py:55-120):

    model = ControlLDM(engine)                      # owns control_scales / only_mid_control (cldm/cldm.py:330-335)
    sampler = DDIMSampler(model)
    samples, intermediates = sampler.sample(S, batch_size, shape, cond, eta=0.0, x_T=x_T,
                                            unconditional_guidance_scale=9.0,
                                            unconditional_conditioning=un_cond, log_every_t=...)

``cond`` / ``un_cond`` are the reference's dicts: ``{"c_crossattn": [ctx], "example_pair": [pair], "query": [query]}``
(lists of tensors, cldm/cldm.py:372-378).  Images are in [-1, 1] like the notebook feeds them.  The loop is driven through the
asynchronous per-step export (``pd_sample_step``), so ``callback`` / ``img_callback`` / ``log_every_t`` behave like the
reference's; the host synchronises only when it reads latents back.
``ucg_schedule`` (per-step guidance, :159-161), ``noise_dropout`` (:232), ``make_schedule(ddim_discretize="quad")`` (util.py:49-50) and
``encode`` / ``stochastic_encode`` / ``decode`` (:237-318) are built on the same per-step export; ``score_corrector``,
``quantize_x0`` and ``dynamic_threshold`` raise ``NotImplementedError``.

The first stage runs on the engine too (``encode_first_stage`` / ``get_first_stage_encoding`` / ``decode_first_stage``; the
encoder needs an engine built with ``ModelConfig(vae_encoder=True)``), so the SD img2img recipe is

    init = model.get_first_stage_encoding(model.encode_first_stage(x))
    z = sampler.stochastic_encode(init, t_enc, noise=...)
    samples = model.decode_first_stage(sampler.decode(z, cond, t_enc, ...))

``c_crossattn`` tensors of any length L <= engine.PD_MAX_CONTEXT_LEN flow through every sampler and through ``encode`` / ``decode``
(the engine takes the context length per call); the conditional and the unconditional one must have the same L, as the reference's
``torch.cat`` of the two halves demands.  ``ControlLDM(engine, tokenizer)`` also has the cond stage: ``get_learned_conditioning`` on
the engine's CLIP, and ``hack_everything(clip_skip)`` for the reference's long prompts (cldm/hack.py: three 75-token windows ->
a [B, 231, 768] context) with the reference's clip_skip count.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import engine as E


def _cat(xs):
    """torch.cat(list, 1) for the reference's list-of-tensors conditioning (cldm/cldm.py:372,377)."""
    if len(xs) == 1:
        return xs[0]
    if E._is_torch(xs[0]):
        import torch
        return torch.cat(list(xs), 1)
    return np.concatenate(list(xs), 1)


def _np32(x):
    if E._is_torch(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float32)


class DiagonalGaussianDistribution:
    """The posterior of ldm/modules/distributions/distributions.py:24-62 over the engine's quant_conv moments [B, 2z, h, w]:
    logvar clamped to [-30, 20], std = exp(0.5 logvar), var = exp(logvar), mode() = mean (fp32 on the host)."""

    def __init__(self, parameters, deterministic: bool = False):
        self.parameters = _np32(parameters)
        self.mean, self.logvar = np.split(self.parameters, 2, axis=1)
        self.logvar = np.clip(self.logvar, np.float32(-30.0), np.float32(20.0))
        self.deterministic = deterministic
        self.std = np.exp(np.float32(0.5) * self.logvar)
        self.var = np.exp(self.logvar)
        if deterministic:
            self.var = self.std = np.zeros_like(self.mean)

    def sample(self, noise=None, generator: Optional[np.random.Generator] = None):
        """mean + std * noise; noise defaults to a standard normal draw from `generator` (or NumPy's global one)."""
        if noise is None:
            g = generator if generator is not None else np.random
            noise = g.standard_normal(self.mean.shape).astype(np.float32)
        return (self.mean + self.std * _np32(noise)).astype(np.float32)

    def mode(self):
        return self.mean


class ControlLDM:
    """The attributes of cldm.cldm.ControlLDM the sampler touches, backed by an Engine."""

    def __init__(self, engine: E.Engine, tokenizer=None, long_prompts=None, clip_skip: int = 0):
        """tokenizer: a transformers CLIPTokenizer (or a look-alike) for get_learned_conditioning.  long_prompts / clip_skip: as
        hack_everything(clip_skip) sets them -- clip_skip counts like the REFERENCE's (cldm/hack.py: hidden_states[-clip_skip] for
        clip_skip > 1, the last layer for 0 and 1), one higher than diffusers' / PromptDiffusionPipeline's clip_skip."""
        from .pipeline import _window_count
        self.engine = engine
        self.tokenizer = tokenizer
        self.long_prompt_windows = _window_count(long_prompts)
        self.clip_skip = int(clip_skip)
        self.control_scales = [1.0] * 13          # cldm/cldm.py:335
        self.only_mid_control = False             # cldm/cldm.py:334
        self.num_timesteps = engine.cfg.timesteps
        self.parameterization = "eps"
        self.scale_factor = engine.cfg.scale_factor   # cldm_v15.yaml:17
        # DDPM.register_schedule buffers q_sample reads (ddpm.py:138-163): fp64 schedule, stored fp32
        cfg = engine.cfg
        betas = np.linspace(cfg.linear_start ** 0.5, cfg.linear_end ** 0.5, cfg.timesteps, dtype=np.float64) ** 2
        ac = np.cumprod(1.0 - betas)
        self.sqrt_alphas_cumprod = np.sqrt(ac).astype(np.float32)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - ac).astype(np.float32)

    def q_sample(self, x_start, t, noise=None):
        """DDPM.q_sample, ldm/models/diffusion/ddpm.py:356-359 (host arithmetic; used by the inpainting blend)."""
        x_start = _np32(x_start)
        if noise is None:
            noise = np.random.standard_normal(x_start.shape).astype(np.float32)
        t = np.asarray(t, np.int64).reshape(-1)
        sa = self.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1)
        sb = self.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1)
        return (sa * x_start + sb * np.asarray(noise, np.float32)).astype(np.float32)

    def encode_first_stage(self, x):
        """LatentDiffusion.encode_first_stage (ddpm.py:831-832): the KL-VAE encoder on the engine -> the posterior."""
        return DiagonalGaussianDistribution(_np32(self.engine.vae_encode(x, mode="moments")))

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """ddpm.py:655-662: scale_factor * posterior.sample() (`noise`: the standard normal draw; default a fresh host draw),
        or scale_factor * tensor."""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(noise)
        elif E._is_torch(encoder_posterior) or isinstance(encoder_posterior, np.ndarray):
            z = _np32(encoder_posterior)
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return (np.float32(self.scale_factor) * z).astype(np.float32)

    def decode_first_stage(self, z):
        """LatentDiffusion.decode_first_stage (ddpm.py:820-828): 1 / scale_factor, post_quant_conv and the decoder, on the engine."""
        return self.engine.vae_decode(_np32(z))

    def hack_everything(self, clip_skip: int = 0, windows: int = 3):
        """cldm/hack.py hack_everything: long prompts (three 75-token windows, each BOS / EOS wrapped and padded to 77, encoded as one
        batch and concatenated to [B, 231, D]) and the reference's clip_skip for get_learned_conditioning."""
        from .pipeline import _window_count
        self.long_prompt_windows = _window_count(windows)
        self.clip_skip = int(clip_skip)

    def get_learned_conditioning(self, c):
        """LatentDiffusion.get_learned_conditioning (ddpm.py:555-565) with FrozenCLIPEmbedder.forward (modules.py:118-131) or, after
        hack_everything, _hacked_clip_forward: prompts -> [B, L, D] fp32 on the engine's CLIP text transformer."""
        from .pipeline import reference_clip_skip, tokenize_long
        if self.tokenizer is None:
            raise ValueError("get_learned_conditioning needs ControlLDM(engine, tokenizer=...)")
        prompts = [c] if isinstance(c, str) else list(c)
        L = self.engine.cfg.context_len
        if self.long_prompt_windows:
            n = self.long_prompt_windows
            z = self.engine.text_encode(tokenize_long(self.tokenizer, prompts, n, L), clip_skip=reference_clip_skip(self.clip_skip))
            return z.reshape(len(prompts), n * L, z.shape[-1])
        # (the unhacked FrozenCLIPEmbedder has no clip_skip: last_hidden_state)
        ids = self.tokenizer(prompts, truncation=True, max_length=L, padding="max_length", return_tensors="np")["input_ids"]
        return self.engine.text_encode(np.asarray(ids, np.int32))

    def apply_model(self, x_noisy, t, cond, *args, **kwargs):
        """eps = apply_model(x, t, cond), cldm/cldm.py:369-382 (one HIP pass through ControlNet + UNet)."""
        assert isinstance(cond, dict)
        assert cond["example_pair"] is not None
        if self.only_mid_control:
            raise NotImplementedError("only_mid_control is supported through DDIMSampler.sample only")
        return self.engine.eps(x_noisy, t, _cat(cond["c_crossattn"]), _cat(cond["example_pair"]), cond["query"][0],
                               scales=self.control_scales)


class DDIMSampler:
    """cldm/ddim_hacked.py:10 DDIMSampler over the HIP engine (sampling only)."""

    def __init__(self, model: ControlLDM, schedule: str = "linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        """cldm/ddim_hacked.py:23-52.  'uniform' comes from the engine (pd_make_schedule); 'quad' (util.py:49-50) is the same
        arithmetic on the host over the quadratic timestep grid, which the engine then samples as a custom grid."""
        eng = self.model.engine
        self.ddim_eta = float(ddim_eta)
        self._custom_ts = None
        if ddim_discretize == "uniform":
            s = eng.make_schedule(ddim_num_steps, ddim_eta)
        elif ddim_discretize == "quad":
            cfg = eng.cfg
            ts = ((np.linspace(0, np.sqrt(cfg.timesteps * .8), ddim_num_steps)) ** 2).astype(int) + 1
            betas = np.linspace(cfg.linear_start ** 0.5, cfg.linear_end ** 0.5, cfg.timesteps, dtype=np.float64) ** 2
            ac = np.cumprod(1.0 - betas).astype(np.float32)             # ddpm.py:155-157 registers float32 buffers
            al = ac[ts]                                                  # util.py:62-66
            ap = np.asarray([ac[0]] + ac[ts[:-1]].tolist(), np.float32)
            sg = ddim_eta * np.sqrt((1 - ap.astype(np.float64)) / (1 - al.astype(np.float64)) * (1 - al.astype(np.float64) / ap.astype(np.float64)))
            s = dict(ddim_timesteps=ts.astype(np.int64), ddim_alphas=al, ddim_alphas_prev=ap, ddim_sigmas=sg.astype(np.float32),
                     ddim_sqrt_one_minus_alphas=np.sqrt(np.float32(1.0) - al))
            self._custom_ts = ts.astype(np.int64)
        else:
            raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discretize}"')   # util.py:52
        self.ddim_timesteps = s["ddim_timesteps"]
        self.ddim_alphas = s["ddim_alphas"]
        self.ddim_alphas_prev = s["ddim_alphas_prev"]
        self.ddim_sigmas = s["ddim_sigmas"]
        self.ddim_sqrt_one_minus_alphas = s["ddim_sqrt_one_minus_alphas"]

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, noise=None, seed=None, **kwargs):
        """seed: seeds the engine's generator (Engine.set_rng, keeping its sample_base).  With eta > 0 and no `noise`, an
        engine whose generator the caller has seeded -- here or through set_rng -- draws the per-step noise in its update
        kernel instead of the host drawing and uploading it; noise_dropout keeps the host draw."""
        if conditioning is None or not isinstance(conditioning, dict):
            raise NotImplementedError("conditioning must be the ControlLDM dict (c_crossattn / example_pair / query)")
        for name, val in (("score_corrector", score_corrector), ("dynamic_threshold", dynamic_threshold)):
            if val is not None:
                raise NotImplementedError(f"{name} is not supported by the HIP sampler")
        if quantize_x0:
            raise NotImplementedError("quantize_x0 is not supported by the HIP sampler")
        ctmp = conditioning[list(conditioning.keys())[0]]
        while isinstance(ctmp, list):
            ctmp = ctmp[0]
        if ctmp.shape[0] != batch_size:   # the reference only prints (ddim_hacked.py:85-86)
            print(f"Warning: Got {ctmp.shape[0]} conditionings but batch-size is {batch_size}")
        C, H, W = shape
        if x_T is None:
            # torch.randn on the reference's device cannot be reproduced bit-exactly; draw on the host
            x_T = np.random.standard_normal((batch_size, C, H, W)).astype(np.float32)
        eng = self.model.engine
        n_steps = eng.num_ddim_steps(S)
        if seed is not None:
            eng.set_rng(seed, eng.rng[1])
        if eta > 0.0 and noise is None and eng._rng_set and not noise_dropout > 0.0:
            noise = "engine"
        if eta > 0.0 and noise is None:
            noise = np.random.standard_normal((n_steps, batch_size, C, H, W)).astype(np.float32)
        if eta > 0.0 and noise_dropout > 0.0:
            # torch.nn.functional.dropout(noise, p), ddim_hacked.py:231-232: zero with probability p, survivors scaled by 1/(1-p)
            noise = _np32(noise)
            keep_mask = (np.random.random_sample(noise.shape) >= noise_dropout).astype(np.float32)
            noise = noise * keep_mask * np.float32(1.0 / (1.0 - noise_dropout))
        if ucg_schedule is not None:
            assert len(ucg_schedule) == n_steps                      # ddim_hacked.py:160
        self.make_schedule(S, ddim_eta=eta, verbose=verbose)
        uc = unconditional_conditioning
        kw = dict(x_T=x_T, ctx_cond=_cat(conditioning["c_crossattn"]), pair=_cat(conditioning["example_pair"]),
                  query=conditioning["query"][0], steps=S, cfg_scale=float(unconditional_guidance_scale), eta=float(eta),
                  use_cfg=uc is not None, temperature=float(temperature), control_scales=self.model.control_scales,
                  only_mid_control=self.model.only_mid_control, noise=noise if eta > 0.0 else None,
                  ctx_uncond=_cat(uc["c_crossattn"]) if uc is not None else None)
        if uc is not None:
            # the reference concatenates EVERY cond key (ddim_hacked.py:190-191); pass differing images through
            if uc["example_pair"][0] is not conditioning["example_pair"][0]:
                kw["pair_uncond"] = _cat(uc["example_pair"])
            if uc["query"][0] is not conditioning["query"][0]:
                kw["query_uncond"] = uc["query"][0]
        every = log_every_t
        # per-step export (asynchronous launches; the host only syncs when it reads latents back)
        n = eng.sample_begin(**kw)
        x_inter, preds = [x_T], [x_T]
        if mask is not None:
            assert x0 is not None                          # ddim_hacked.py:155
            mask_np = _np32(mask)
            x0_np = _np32(x0)
        for i in range(n):
            if mask is not None:
                # inpainting blend, ddim_hacked.py:154-157: keep the known region at this step's noise level
                ts = np.full((batch_size,), int(self.ddim_timesteps[n - i - 1]), np.int64)
                img_orig = _np32(self.model.q_sample(x0_np, ts))
                cur = _np32(eng.sample_get(E.PD_GET_LATENTS))
                eng.sample_set_latents(img_orig * mask_np + (np.float32(1.0) - mask_np) * cur)
            if ucg_schedule is not None:
                eng.sample_set_guidance(float(ucg_schedule[i]))          # ddim_hacked.py:159-161
            eng.sample_step(i)
            index = n - i - 1
            if callback:
                callback(i)
            if img_callback:
                img_callback(eng.sample_get(E.PD_GET_PRED_X0), i)
            if index % every == 0 or index == n - 1:
                x_inter.append(eng.sample_get(E.PD_GET_LATENTS))
                preds.append(eng.sample_get(E.PD_GET_PRED_X0))
        samples = eng.sample_get(E.PD_GET_LATENTS)
        eng.sample_end()
        return samples, {"x_inter": x_inter, "pred_x0": preds}

    def _lms_call(self, conditioning, batch_size, shape, x_T, scale, uc, unsupported):
        """The engine arguments PLMSSampler / DPMSolverSampler share with sample() above; both apply guidance only when the
        scale differs from 1 (plms.py:185, dpm_solver.py:305)."""
        if conditioning is None or not isinstance(conditioning, dict):
            raise NotImplementedError("conditioning must be the ControlLDM dict (c_crossattn / example_pair / query)")
        for name, val in unsupported:
            if val:
                raise NotImplementedError(f"{name} is not supported by the HIP sampler")
        C, H, W = shape
        if x_T is None:
            x_T = np.random.standard_normal((batch_size, C, H, W)).astype(np.float32)
        cfg_on = uc is not None and float(scale) != 1.0
        kw = dict(x_T=x_T, ctx_cond=_cat(conditioning["c_crossattn"]), pair=_cat(conditioning["example_pair"]),
                  query=conditioning["query"][0], cfg_scale=float(scale), use_cfg=cfg_on, control_scales=self.model.control_scales,
                  only_mid_control=self.model.only_mid_control, ctx_uncond=_cat(uc["c_crossattn"]) if cfg_on else None)
        if cfg_on:
            if uc["example_pair"][0] is not conditioning["example_pair"][0]:
                kw["pair_uncond"] = _cat(uc["example_pair"])
            if uc["query"][0] is not conditioning["query"][0]:
                kw["query_uncond"] = uc["query"][0]
        return kw

    # ------------------------------------------------------------------ encode / decode (ddim_hacked.py:237-318)
    def _session(self, x, cond, uc, scale, timesteps, noise=None):
        """one engine session over a custom descending timestep list (context K/V, hint embedders and time embeddings hoisted once)"""
        kw = dict(noise=noise, x_T=x, ctx_cond=_cat(cond["c_crossattn"]), pair=_cat(cond["example_pair"]), query=cond["query"][0],
                  steps=len(timesteps), cfg_scale=float(scale), eta=self.ddim_eta, use_cfg=uc is not None, temperature=1.0,
                  control_scales=self.model.control_scales, only_mid_control=self.model.only_mid_control, timesteps=timesteps,
                  ctx_uncond=_cat(uc["c_crossattn"]) if uc is not None else None)
        if uc is not None:
            if uc["example_pair"][0] is not cond["example_pair"][0]:
                kw["pair_uncond"] = _cat(uc["example_pair"])
            if uc["query"][0] is not cond["query"][0]:
                kw["query_uncond"] = uc["query"][0]
        return self.model.engine.sample_begin(**kw)

    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None):
        """DDIM inversion exactly as ddim_hacked.py:237-282 runs it -- including its quirk of handing the LOOP INDEX i (not the
        DDIM timestep) to apply_model.  With guidance the reference concatenates the two conditioning dicts with torch.cat
        (:263), which raises TypeError for ControlLDM's dict conditioning; that path raises the same here."""
        if use_original_steps:
            raise NotImplementedError("use_original_steps needs the full 1000-step buffers of DDPM; not built")
        num_reference_steps = self.ddim_timesteps.shape[0]
        assert t_enc <= num_reference_steps
        if unconditional_guidance_scale != 1.0:
            assert unconditional_conditioning is not None
            raise TypeError("expected Tensor as element 0 in argument 0, but got dict")
        num_steps = t_enc
        alphas_next = self.ddim_alphas[:num_steps].astype(np.float32)
        alphas = self.ddim_alphas_prev[:num_steps].astype(np.float32)
        eng = self.model.engine
        x_next = _np32(x0)
        self._session(x_next, c, None, 1.0, [1])     # the session only hoists the conditioning; eps is asked for at explicit t
        intermediates, inter_steps = [], []
        one = np.float32(1.0)
        for i in range(num_steps):
            noise_pred = _np32(eng.sample_eps_at(i, self.model.control_scales))
            xt_weighted = np.sqrt(alphas_next[i] / alphas[i]) * x_next
            weighted_noise_pred = np.sqrt(alphas_next[i]) * (np.sqrt(one / alphas_next[i] - one) - np.sqrt(one / alphas[i] - one)) * noise_pred
            x_next = (xt_weighted + weighted_noise_pred).astype(np.float32)
            eng.sample_set_latents(x_next)
            if return_intermediates and i % (num_steps // return_intermediates) == 0 and i < num_steps - 1:
                intermediates.append(x_next)
                inter_steps.append(i)
            elif return_intermediates and i >= num_steps - 2:
                intermediates.append(x_next)
                inter_steps.append(i)
            if callback:
                callback(i)
        eng.sample_end()
        out = {"x_encoded": x_next, "intermediate_steps": inter_steps}
        if return_intermediates:
            out.update({"intermediates": intermediates})
        return x_next, out

    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim_hacked.py:284-299: q(x_t | x_0) on the DDIM grid; t indexes the DDIM schedule."""
        if use_original_steps:
            raise NotImplementedError("use_original_steps needs the full 1000-step buffers of DDPM; not built")
        x0 = _np32(x0)
        if noise is None:
            noise = np.random.standard_normal(x0.shape).astype(np.float32)
        t = np.asarray(t, np.int64).reshape(-1)
        sa = np.sqrt(self.ddim_alphas.astype(np.float32))[t].reshape(-1, 1, 1, 1)
        sb = self.ddim_sqrt_one_minus_alphas.astype(np.float32)[t].reshape(-1, 1, 1, 1)
        return (sa * x0 + sb * _np32(noise)).astype(np.float32)

    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, seed=None):
        """ddim_hacked.py:301-318: p_sample_ddim over the first t_start timesteps of the current schedule, in the engine's own
        step loop (custom timestep grid).  With eta > 0 the fresh noise of every step is the engine's own seeded draw: pass
        `seed`, or seed the engine's generator first (Engine.set_rng); otherwise eta > 0 raises as before."""
        if use_original_steps:
            raise NotImplementedError("use_original_steps needs the full 1000-step buffers of DDPM; not built")
        eng = self.model.engine
        if seed is not None:
            eng.set_rng(seed, eng.rng[1])
        if self.ddim_eta > 0.0 and not eng._rng_set:
            raise NotImplementedError("decode with eta > 0 draws fresh noise per step in the reference; pass eta = 0 to make_schedule")
        timesteps = np.asarray(self.ddim_timesteps)[:t_start]
        n = self._session(_np32(x_latent), cond, unconditional_conditioning, unconditional_guidance_scale,
                          [int(t) for t in np.flip(timesteps)], noise="engine" if self.ddim_eta > 0.0 else None)
        for i in range(n):
            eng.sample_step(i)
            if callback:
                callback(i)
        x_dec = eng.sample_get(E.PD_GET_LATENTS)
        eng.sample_end()
        return x_dec


class PLMSSampler(DDIMSampler):
    """ldm/models/diffusion/plms.py:12 PLMSSampler over the HIP engine: the whole loop runs inside the engine (pd_lms_sample,
    kind PLMS) on the grid of make_schedule.  Returns (samples, {'x_inter', 'pred_x0'}) like the reference.  Not built, as in
    DDIMSampler: quantize_x0, score_corrector, dynamic_threshold; also mask / x0 (the reference re-draws q_sample noise at
    every step) and eta != 0, which the reference refuses too (plms.py:26-27)."""

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")      # plms.py:26-27
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0.0, verbose=verbose)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, dynamic_threshold=None, **kwargs):
        kw = self._lms_call(conditioning, batch_size, shape, x_T, unconditional_guidance_scale, unconditional_conditioning,
                            (("quantize_x0", quantize_x0), ("score_corrector", score_corrector is not None),
                             ("dynamic_threshold", dynamic_threshold is not None), ("mask", mask is not None)))
        self.make_schedule(S, ddim_eta=eta, verbose=verbose)
        eng = self.model.engine
        grid = [int(t) for t in np.flip(self.ddim_timesteps)]
        rows, _ = eng.lms_coefficients(grid, kind="plms")
        n = eng.sample_begin_lms(kind="plms", timesteps=grid, **kw)
        total = len(grid)
        x_inter, preds, done = [kw["x_T"]], [kw["x_T"]], 0
        for r in range(n):
            eng.sample_step(r)
            if not int(rows[r, 2]) & E.PD_LMS_F_STEP:
                continue                                         # the first evaluation of the pseudo improved Euler step
            index = total - done - 1
            if callback:
                callback(done)
            if img_callback:
                img_callback(eng.sample_get(E.PD_GET_PRED_X0), done)
            if index % log_every_t == 0 or index == total - 1:
                x_inter.append(eng.sample_get(E.PD_GET_LATENTS))
                preds.append(eng.sample_get(E.PD_GET_PRED_X0))
            done += 1
        samples = eng.sample_get(E.PD_GET_LATENTS)
        eng.sample_end()
        return samples, {"x_inter": x_inter, "pred_x0": preds}


class DPMSolverSampler(DDIMSampler):
    """ldm/models/diffusion/dpm_solver/sampler.py:13 DPMSolverSampler over the HIP engine: DPM-Solver++ multistep, order 2,
    lower_order_final, on the reference's time-uniform continuous grid t = linspace(1, 1/N, S + 1), which reaches the UNet
    as the fractional model times (t - 1/N) * 1000 (pd_lms_args.model_times).  Returns (samples, None) like the reference,
    which ignores mask / x0 / callbacks / eta there as well; options that would change the result raise."""

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, **kwargs):
        kw = self._lms_call(conditioning, batch_size, shape, x_T, unconditional_guidance_scale, unconditional_conditioning,
                            (("quantize_x0", quantize_x0), ("score_corrector", score_corrector is not None)))
        N = self.ddpm_num_timesteps
        t = np.linspace(1.0, 1.0 / N, int(S) + 1)
        model_times = np.maximum((t - 1.0 / N) * 1000.0, 0.0)
        samples = self.model.engine.lms_sample(kind="dpmsolver++", order=2, solver_type="dpm_solver",
                                               lower_order_final=int(S) < 15, model_times=model_times, **kw)
        return samples, None
