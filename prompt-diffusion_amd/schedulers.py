"""Host-side scheduler plug-ins for `PromptDiffusionPipeline(scheduler=...)`.

The reference's README swaps the pipeline's scheduler for diffusers' `UniPCMultistepScheduler`
(`README.md:49`, `pipe.scheduler = UniPCMultistepScheduler.from_config(pipe.scheduler.config)`) and BASELINE config #4
(768x768, 20 steps) is quoted with it.  diffusers is not vendored in the reference tree, so this is a restatement of the
published algorithm -- UniPC, Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of
Diffusion Models", Alg. 5-8 (multistep UniP-p / UniC-p, data prediction, B(h) = e^h - 1 "bh2" or h "bh1") -- behind the
scheduler interface the pipeline drives (`set_timesteps`, `timesteps`, `scale_model_input`, `step(..., return_dict=False)`,
`init_noise_sigma`).  PARITY UNPINNED against diffusers (no source, no fixtures); it is cross-checked against an
independent fp64 closed-form restatement in `oracle/` and against the analytic probability-flow solution for Gaussian
data (`tests/test_schedulers_cpu.py`).

`DPMSolverMultistepScheduler` (DPM-Solver++ multistep; Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of
Diffusion Probabilistic Models") and `PNDMScheduler` (`skip_prk_steps=True`: PLMS; Liu et al. 2022, "Pseudo Numerical Methods
for Diffusion Models on Manifolds") sit behind the same interface.  Both solvers ship in the reference tree
(`ldm/models/diffusion/dpm_solver/dpm_solver.py`, `ldm/models/diffusion/plms.py`), so their UPDATE ARITHMETIC IS PINNED to
the reference's own code through `tests/golden/samplers_lms.npz` (`tests/test_lms_cpu.py`).  Their `set_timesteps` grids,
option names and order rules are diffusers' and, like UniPC's, UNPINNED.

All coefficient arithmetic is fp64 NumPy; the per-step update is O(latent size) host work (2 MB per step at 768x768,
bs 8) and stays on the host like the reference's scheduler does.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np


def _to_np(x):
    if isinstance(x, np.ndarray):
        return x, None
    import torch
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy(), x
    return np.asarray(x), None


class UniPCMultistepScheduler:
    """UniPC multistep predictor-corrector, epsilon-prediction model, data-prediction (x0) form.

    Defaults follow what `from_config(<SD1.5 scheduler config>)` yields in the reference's README flow:
    scaled-linear betas 0.00085..0.012 over 1000 steps, solver_order 2, `bh2`, lower_order_final, final sigma 0.
    """
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 predict_x0: bool = True, solver_type: str = "bh2", lower_order_final: bool = True,
                 disable_corrector: Optional[List[int]] = None, timestep_spacing: str = "linspace", steps_offset: int = 0,
                 thresholding: bool = False):
        if beta_schedule == "scaled_linear":
            betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        elif beta_schedule == "linear":
            betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule!r}")
        if prediction_type != "epsilon":
            raise NotImplementedError("the Prompt-Diffusion UNet predicts epsilon (ddpm.py:71)")
        if not predict_x0:
            raise NotImplementedError("noise-prediction form of UniPC")
        if thresholding:
            raise NotImplementedError("dynamic thresholding is for pixel-space models")
        if solver_type not in ("bh1", "bh2"):
            raise ValueError("solver_type must be 'bh1' or 'bh2'")
        if solver_order < 1 or solver_order > 3:
            raise ValueError("solver_order must be 1, 2 or 3")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}")
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.solver_order = solver_order
        self.solver_type = solver_type
        self.lower_order_final = lower_order_final
        self.disable_corrector = list(disable_corrector or [])
        self.timestep_spacing = timestep_spacing
        self.steps_offset = steps_offset
        self.timesteps = np.zeros((0,), np.int64)
        self._reset()

    def _reset(self):
        self.model_outputs = [None] * self.solver_order     # x0 predictions, oldest first
        self.timestep_list = [None] * self.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self._step_index = 0
        self.this_order = 1

    # ------------------------------------------------------------------ schedule
    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, int(num_inference_steps)
        if n < 1 or n > T:
            raise ValueError("num_inference_steps out of range")
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + self.steps_offset
        else:
            ts = np.arange(T, 0, -T / n).round() - 1
        self.timesteps = ts.astype(np.int64)
        a = self.alphas_cumprod[self.timesteps]
        # alpha_t = sqrt(abar), sigma_t = sqrt(1 - abar), lambda = log(alpha / sigma); the final point is sigma = 0
        self._alpha = np.concatenate([np.sqrt(a), [1.0]])
        self._sigma = np.concatenate([np.sqrt(1.0 - a), [0.0]])
        with np.errstate(divide="ignore"):
            self._lambda = np.log(self._alpha) - np.log(self._sigma)
        self.num_inference_steps = n
        self._reset()

    def set_begin_index(self, begin_index: int = 0):
        """diffusers' set_begin_index: after set_timesteps, stepping starts at timesteps[begin_index] with fresh solver state
        (img2img / inpainting run the tail of the grid).  disable_corrector keeps indexing the whole grid."""
        k = int(begin_index)
        if not 0 <= k < len(self.timesteps):
            raise ValueError(f"begin_index {k} outside the {len(self.timesteps)} timesteps")
        self._reset()
        self._step_index = k

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ------------------------------------------------------------------ coefficients (fp64)
    def _coeffs(self, i0: int, order: int, hist_idx: List[int]):
        """Quantities shared by UniP and UniC for the update from schedule point i0 to i0+1.
        hist_idx: schedule indices of the older model outputs, newest first (length order-1)."""
        lam0, lam1 = self._lambda[i0], self._lambda[i0 + 1]
        h = lam1 - lam0
        rks = [(self._lambda[j] - lam0) / h for j in hist_idx] + [1.0]
        hh = -h
        h_phi_1 = math.expm1(hh) if np.isfinite(hh) else -1.0
        h_phi_k = (h_phi_1 / hh - 1.0) if np.isfinite(hh) else -1.0
        B_h = h_phi_1 if self.solver_type == "bh2" else hh
        R, b, fact = [], [], 1.0
        for i in range(1, order + 1):
            R.append(np.power(rks, i - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = (h_phi_k / hh - 1.0 / fact) if np.isfinite(hh) else -1.0 / fact
        return dict(h_phi_1=h_phi_1, B_h=B_h, rks=np.asarray(rks), R=np.stack(R), b=np.asarray(b),
                    alpha1=self._alpha[i0 + 1], sig_ratio=self._sigma[i0 + 1] / self._sigma[i0])

    def _d1s(self, m0, hist, rks):
        return [(m - m0) / r for m, r in zip(hist, rks[:-1])]

    def _uni_p(self, x, i0, order):
        m0 = self.model_outputs[-1]
        hist = [self.model_outputs[-(k + 1)] for k in range(1, order)]
        hidx = [self.timestep_list[-(k + 1)] for k in range(1, order)]
        c = self._coeffs(i0, order, hidx)
        x_t = c["sig_ratio"] * x - c["alpha1"] * c["h_phi_1"] * m0
        if order > 1:
            D1s = self._d1s(m0, hist, c["rks"])
            rhos = np.array([0.5]) if order == 2 else np.linalg.solve(c["R"][:-1, :-1], c["b"][:-1])
            x_t = x_t - c["alpha1"] * c["B_h"] * sum(r * d for r, d in zip(rhos, D1s))
        return x_t

    def _uni_c(self, m_t, x_last, i0, order):
        """Corrector for the step i0 -> i0+1 that the predictor already took; m_t = x0 prediction at i0+1.
        Runs BEFORE m_t is pushed, so model_outputs[-1] is the output at i0."""
        m0 = self.model_outputs[-1]
        hist = [self.model_outputs[-(k + 1)] for k in range(1, order)]
        hidx = [self.timestep_list[-(k + 1)] for k in range(1, order)]
        c = self._coeffs(i0, order, hidx)
        rhos = np.array([0.5]) if order == 1 else np.linalg.solve(c["R"], c["b"])
        corr = 0.0
        if order > 1:
            D1s = self._d1s(m0, hist, c["rks"])
            corr = sum(r * d for r, d in zip(rhos[:-1], D1s))
        x_t = c["sig_ratio"] * x_last - c["alpha1"] * c["h_phi_1"] * m0
        return x_t - c["alpha1"] * c["B_h"] * (corr + rhos[-1] * (m_t - m0))

    # ------------------------------------------------------------------ one step
    def step(self, model_output, timestep, sample, return_dict: bool = True, **_):
        if len(self.timesteps) == 0:
            raise ValueError("call set_timesteps first")
        eps, like = _to_np(model_output)
        x, like_x = _to_np(sample)
        like = like_x if like_x is not None else like
        out_dtype = x.dtype
        eps = eps.astype(np.float64)
        x = x.astype(np.float64)
        i = self._step_index
        if int(timestep) != int(self.timesteps[i]):
            raise ValueError(f"step {i} expects timestep {int(self.timesteps[i])}, got {int(timestep)}")
        m_t = (x - self._sigma[i] * eps) / self._alpha[i]              # epsilon -> x0 prediction
        use_corrector = i > 0 and (i - 1) not in self.disable_corrector and self.last_sample is not None
        if use_corrector:
            x = self._uni_c(m_t, self.last_sample, i - 1, self.this_order)
        self.model_outputs = self.model_outputs[1:] + [m_t]
        self.timestep_list = self.timestep_list[1:] + [i]
        order = min(self.solver_order, len(self.timesteps) - i) if self.lower_order_final else self.solver_order
        self.this_order = min(order, self.lower_order_nums + 1)        # warm-up: orders 1, 2, ...
        if not np.isfinite(self._lambda[i + 1]):
            self.this_order = 1                                        # the step onto sigma = 0 is x0 itself
        self.last_sample = x
        prev = self._uni_p(x, i, self.this_order)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        prev = prev.astype(out_dtype)
        if like is not None:
            import torch
            prev = torch.from_numpy(prev).to(like.device)
        if not return_dict:
            return (prev,)
        return {"prev_sample": prev}


def _betas(beta_schedule, beta_start, beta_end, n):
    if beta_schedule == "scaled_linear":
        return np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float64) ** 2
    if beta_schedule == "linear":
        return np.linspace(beta_start, beta_end, n, dtype=np.float64)
    raise NotImplementedError(f"beta_schedule {beta_schedule!r}")


def _spaced_timesteps(spacing, T, n, steps_offset):
    """diffusers' three spacings, sampling order (descending), as UniPCMultistepScheduler.set_timesteps writes them."""
    if spacing == "linspace":
        ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1]
    elif spacing == "leading":
        ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1] + steps_offset
    elif spacing == "trailing":
        ts = np.arange(T, 0, -T / n).round() - 1
    else:
        raise ValueError(f"timestep_spacing {spacing!r}")
    return ts.astype(np.int64)


def _wrap_out(prev, out_dtype, like, return_dict):
    prev = prev.astype(out_dtype)
    if like is not None:
        import torch
        prev = torch.from_numpy(prev).to(like.device)
    if not return_dict:
        return (prev,)
    return {"prev_sample": prev}


class DPMSolverMultistepScheduler:
    """DPM-Solver++ multistep, epsilon-prediction model, data-prediction form, orders 1-3.

    The update is DPM_Solver.multistep_dpm_solver_update of the reference tree with predict_x0 (dpm_solver.py:469-501,
    723-825); `solver_type` "midpoint" is its "dpm_solver" second-order form and "heun" its "taylor" form, the mapping
    diffusers uses.  The order of a step is min(solver_order, steps taken + 1), lowered to the number of steps left with
    `lower_order_final` on grids of fewer than 15 points (dpm_solver.py:1062-1065), and 1 for the step onto sigma = 0.
    `set_timesteps` lands on sigma = 0 (diffusers' final_sigmas_type "zero"); `set_model_times` is this package's extension
    for the reference's continuous grid.
    """
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint", lower_order_final: bool = True,
                 timestep_spacing: str = "linspace", steps_offset: int = 0, thresholding: bool = False,
                 use_karras_sigmas: bool = False):
        if prediction_type != "epsilon":
            raise NotImplementedError("the Prompt-Diffusion UNet predicts epsilon (ddpm.py:71)")
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type {algorithm_type!r}: only the deterministic data-prediction solver is built")
        if thresholding or use_karras_sigmas:
            raise NotImplementedError("thresholding / use_karras_sigmas")
        if solver_type not in ("midpoint", "heun"):
            raise ValueError("solver_type must be 'midpoint' or 'heun'")
        if solver_order < 1 or solver_order > 3:
            raise ValueError("solver_order must be 1, 2 or 3")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}")
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = np.cumprod(1.0 - _betas(beta_schedule, beta_start, beta_end, num_train_timesteps))
        self.solver_order = solver_order
        self.solver_type = solver_type
        self.lower_order_final = lower_order_final
        self.timestep_spacing = timestep_spacing
        self.steps_offset = steps_offset
        self.timesteps = np.zeros((0,), np.int64)
        self.model_times = None
        self._reset()

    def _reset(self):
        self.model_outputs = []      # x0 predictions, newest last
        self._hist_idx = []
        self._step_index = 0
        self._begin = 0

    def _set_points(self, alpha, sigma):
        self._alpha, self._sigma = np.asarray(alpha, np.float64), np.asarray(sigma, np.float64)
        with np.errstate(divide="ignore"):
            self._lambda = np.log(self._alpha) - np.log(self._sigma)
        self.num_inference_steps = len(self._alpha) - 1
        self._reset()

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        T = self.num_train_timesteps
        if timesteps is not None:
            ts = np.asarray([int(t) for t in timesteps], np.int64)
        else:
            n = int(num_inference_steps)
            if n < 1 or n > T:
                raise ValueError("num_inference_steps out of range")
            ts = _spaced_timesteps(self.timestep_spacing, T, n, self.steps_offset)
        if len(ts) < 1 or np.any(np.diff(ts) >= 0) or ts.min() < 0 or ts.max() >= T:
            raise ValueError("timesteps must be strictly descending inside [0, num_train_timesteps)")
        self.timesteps = ts
        self.model_times = None
        a = self.alphas_cumprod[ts]
        self._set_points(np.concatenate([np.sqrt(a), [1.0]]), np.concatenate([np.sqrt(1.0 - a), [0.0]]))

    def set_model_times(self, model_times):
        """The reference's grid: steps + 1 strictly descending model times in [0, T - 1], fractional ones included, the last
        one the point the loop lands on; log(alpha) linear between the trained points (NoiseScheduleVP('discrete')).
        `timesteps` then holds the evaluation times as floats."""
        mt = np.asarray(model_times, np.float64).reshape(-1)
        if len(mt) < 2 or np.any(np.diff(mt) >= 0) or mt.min() < 0 or mt.max() > self.num_train_timesteps - 1:
            raise ValueError("model_times must be strictly descending inside [0, num_train_timesteps - 1]")
        la = np.interp(mt, np.arange(self.num_train_timesteps), 0.5 * np.log(self.alphas_cumprod))
        self.model_times = mt
        self.timesteps = mt[:-1].copy()
        self._set_points(np.exp(la), np.sqrt(1.0 - np.exp(2.0 * la)))

    def set_begin_index(self, begin_index: int = 0):
        k = int(begin_index)
        if not 0 <= k < len(self.timesteps):
            raise ValueError(f"begin_index {k} outside the {len(self.timesteps)} timesteps")
        self._reset()
        self._step_index = self._begin = k

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _lower_order_final(self) -> bool:
        return bool(self.lower_order_final) and len(self.timesteps) < 15

    def step(self, model_output, timestep, sample, return_dict: bool = True, **_):
        if len(self.timesteps) == 0:
            raise ValueError("call set_timesteps first")
        eps, like = _to_np(model_output)
        x, like_x = _to_np(sample)
        like = like_x if like_x is not None else like
        out_dtype = x.dtype
        eps, x = eps.astype(np.float64), x.astype(np.float64)
        i, n = self._step_index, len(self.timesteps)
        if float(timestep) != float(self.timesteps[i]):
            raise ValueError(f"step {i} expects timestep {self.timesteps[i]}, got {timestep}")
        m0 = (x - self._sigma[i] * eps) / self._alpha[i]
        self.model_outputs = (self.model_outputs + [m0])[-3:]
        self._hist_idx = (self._hist_idx + [i])[-3:]
        order = min(self.solver_order, len(self.model_outputs))
        if self._lower_order_final():
            order = min(order, n - i)
        lam = self._lambda
        h = lam[i + 1] - lam[i]
        if not np.isfinite(h):
            order = 1
        a1 = self._alpha[i + 1]
        phi = math.expm1(-h) if np.isfinite(h) else -1.0          # exp(-h) - 1
        prev = (self._sigma[i + 1] / self._sigma[i]) * x - (a1 * phi) * m0
        if order >= 2:
            m1 = self.model_outputs[-2]
            r0 = (lam[i] - lam[self._hist_idx[-2]]) / h
            D1_0 = (1.0 / r0) * (m0 - m1)
        if order == 2:
            if self.solver_type == "midpoint":
                prev = prev - 0.5 * (a1 * phi) * D1_0
            else:
                prev = prev + (a1 * (phi / h + 1.0)) * D1_0
        elif order == 3:
            m2 = self.model_outputs[-3]
            r1 = (lam[self._hist_idx[-2]] - lam[self._hist_idx[-3]]) / h
            D1_1 = (1.0 / r1) * (m1 - m2)
            D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
            D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
            prev = prev + (a1 * (phi / h + 1.0)) * D1 - (a1 * ((phi + h) / h ** 2 - 0.5)) * D2
        self.pred_original_sample = m0
        self._step_index += 1
        return _wrap_out(prev, out_dtype, like, return_dict)

    def fused_lms(self, t_start: int = 0):
        """Arguments of Engine.lms_sample that run this scheduler's remaining steps inside the engine."""
        kw = dict(kind="dpmsolver++", order=self.solver_order, solver_type=self.solver_type,
                  lower_order_final=self._lower_order_final())
        if self.model_times is not None:
            kw["model_times"] = self.model_times[t_start:]
        else:
            kw["timesteps"] = [int(t) for t in self.timesteps[t_start:]]
        return kw


class PNDMScheduler:
    """PLMS (`skip_prk_steps=True`): Adams-Bashforth of orders 1-4 over eps by warm-up, with PLMSSampler's pseudo improved
    Euler first step (plms.py:226-242).  `timesteps` repeats the second grid point -- t0, t1, t1, t2, ... -- because the first
    step evaluates the model twice; the second call redoes the step from the sample of the first.  a_prev of a step is
    alphas_cumprod at the next grid point and alphas_cumprod[0] after the last (1.0 with `set_alpha_to_one`), which is
    make_ddim_sampling_parameters' rule and, on the "leading" grid with steps_offset 1 of the SD1.5 config, diffusers' too.
    Defaults are that config's (`skip_prk_steps=True, set_alpha_to_one=False, steps_offset=1`).
    """
    order = 1
    init_noise_sigma = 1.0
    _AB = ((1.0,), (3.0 / 2.0, -1.0 / 2.0), (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0), (55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0))

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", skip_prk_steps: bool = True, set_alpha_to_one: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", steps_offset: int = 1):
        if not skip_prk_steps:
            raise NotImplementedError("skip_prk_steps=False (the Runge-Kutta warm-up) is not built; SD1.5 configs set it True")
        if prediction_type != "epsilon":
            raise NotImplementedError("the Prompt-Diffusion UNet predicts epsilon (ddpm.py:71)")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}")
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = np.cumprod(1.0 - _betas(beta_schedule, beta_start, beta_end, num_train_timesteps))
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.set_alpha_to_one = bool(set_alpha_to_one)
        self.timestep_spacing = timestep_spacing
        self.steps_offset = steps_offset
        self.timesteps = np.zeros((0,), np.int64)
        self._reset()

    def _reset(self):
        self.ets = []
        self.cur_sample = None
        self.counter = 0
        self._step_index = self._begin = 0

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        """`timesteps`: the grid itself, one entry per step, sampling order (the second entry is repeated here)."""
        T = self.num_train_timesteps
        if timesteps is not None:
            g = np.asarray([int(t) for t in timesteps], np.int64)
        else:
            n = int(num_inference_steps)
            if n < 1 or n > T:
                raise ValueError("num_inference_steps out of range")
            if self.timestep_spacing == "leading":
                g = ((np.arange(0, n) * (T // n)).round()[::-1] + self.steps_offset).astype(np.int64)
            else:
                g = _spaced_timesteps(self.timestep_spacing, T, n, self.steps_offset)
        if len(g) < 1 or np.any(np.diff(g) >= 0) or g.min() < 0 or g.max() >= T:
            raise ValueError("timesteps must be strictly descending inside [0, num_train_timesteps)")
        self.grid = g
        self.timesteps = np.concatenate([g[:1], g[min(1, len(g) - 1):][:1], g[1:]])
        self.num_inference_steps = len(g)
        self._reset()

    def set_begin_index(self, begin_index: int = 0):
        """Start at timesteps[begin_index] with fresh state: the remaining entries are taken as a grid of their own (a repeated
        leading entry collapses), so the first step there is again the two-evaluation one."""
        k = int(begin_index)
        if not 0 <= k < len(self.timesteps):
            raise ValueError(f"begin_index {k} outside the {len(self.timesteps)} timesteps")
        rest = [int(t) for t in self.timesteps[k:]]
        g = [t for j, t in enumerate(rest) if j == 0 or t != rest[j - 1]]
        head = self.timesteps[:k].copy()
        self.set_timesteps(timesteps=g)
        self.timesteps = np.concatenate([head, self.timesteps])
        self._step_index = self._begin = k

    def scale_model_input(self, sample, timestep=None):
        return sample

    def completes_step(self, index: Optional[int] = None) -> bool:
        """Whether the call at timesteps[index] (default: the next one) ends a sampling step; the first of a run does not."""
        return (self.counter if index is None else index - self._begin) != 0

    def _a_prev(self, j):
        return self.alphas_cumprod[self.grid[j + 1]] if j + 1 < len(self.grid) else self.final_alpha_cumprod

    def step(self, model_output, timestep, sample, return_dict: bool = True, **_):
        if len(self.timesteps) == 0:
            raise ValueError("call set_timesteps first")
        e_t, like = _to_np(model_output)
        x, like_x = _to_np(sample)
        like = like_x if like_x is not None else like
        out_dtype = x.dtype
        e_t, x = e_t.astype(np.float64), x.astype(np.float64)
        if int(timestep) != int(self.timesteps[self._step_index]):
            raise ValueError(f"step {self._step_index} expects timestep {int(self.timesteps[self._step_index])}, got {int(timestep)}")
        c = self.counter
        j = 0 if c < 2 else c - 1                 # grid index of the step this call works on
        if c == 0:
            self.cur_sample = x
            self.ets = [e_t]
            e_prime = e_t                         # the trial update of the pseudo improved Euler step
        elif c == 1:
            e_prime = (self.ets[-1] + e_t) / 2    # e_t is e_t_next; it never enters the history
            x = self.cur_sample
            self.cur_sample = None
        else:
            w = self._AB[min(len(self.ets), 3)]
            e_prime = sum(wk * ek for wk, ek in zip(w, [e_t] + self.ets[::-1]))
            self.ets = (self.ets + [e_t])[-3:]
        a_t, a_prev = self.alphas_cumprod[self.grid[j]], self._a_prev(j)
        pred_x0 = (x - np.sqrt(1.0 - a_t) * e_prime) / np.sqrt(a_t)
        prev = np.sqrt(a_prev) * pred_x0 + np.sqrt(1.0 - a_prev) * e_prime
        self.pred_original_sample = pred_x0
        self.counter += 1
        self._step_index += 1
        return _wrap_out(prev, out_dtype, like, return_dict)

    def fused_lms(self, t_start: int = 0):
        """Arguments of Engine.lms_sample that run this scheduler's remaining steps inside the engine."""
        rest = [int(t) for t in self.timesteps[t_start:]]
        return dict(kind="plms", timesteps=[t for j, t in enumerate(rest) if j == 0 or t != rest[j - 1]])


class EulerAncestralDiscreteScheduler:
    """Euler ancestral ("Euler a"): k-diffusion's sample_euler_ancestral with eta = 1, written in the VP variables the engine
    samples in, so `init_noise_sigma` is 1 and `scale_model_input` the identity.  With alpha = sqrt(abar), sigma = sqrt(1 - abar)
    and s = sigma / alpha, a step from t_i to t_{i+1} (s = 0 after the last) is
        s_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2),  s_down = sqrt(s_to^2 - s_up^2)
        x' = (alpha_to / alpha_from) x + alpha_to (s_down - s_from) eps + alpha_to s_up z,   z ~ N(0, 1)
    -- the rows of PD_LMS_EULER_A (include/pdengine.h).  No counterpart ships in the reference tree: the formula is
    k-diffusion's published one, UNPINNED like the other grids here.  `step(..., generator=)` draws z through whatever it is
    given: a NumPy Generator, a torch.Generator, or an object with randn(shape, stream=, draw=) such as the pipeline's
    EngineGenerator, which is asked for (stream "step", draw = the step's index from the first step run) -- the addresses the
    fused loop draws at.
    """
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", prediction_type: str = "epsilon", timestep_spacing: str = "leading",
                 steps_offset: int = 1):
        if prediction_type != "epsilon":
            raise NotImplementedError("the Prompt-Diffusion UNet predicts epsilon (ddpm.py:71)")
        if timestep_spacing not in ("leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: 'leading' or 'trailing'")
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = np.cumprod(1.0 - _betas(beta_schedule, beta_start, beta_end, num_train_timesteps))
        self.timestep_spacing = timestep_spacing
        self.steps_offset = steps_offset
        self.timesteps = np.zeros((0,), np.int64)
        self._step_index = self._begin = 0

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        T = self.num_train_timesteps
        if timesteps is not None:
            ts = np.asarray([int(t) for t in timesteps], np.int64)
        else:
            n = int(num_inference_steps)
            if n < 1 or n > T:
                raise ValueError("num_inference_steps out of range")
            if self.timestep_spacing == "leading":      # diffusers: arange(n) * (T // n) + steps_offset, descending
                ts = ((np.arange(0, n) * (T // n)).round()[::-1] + self.steps_offset).astype(np.int64)
            else:
                ts = _spaced_timesteps("trailing", T, n, 0)
        if len(ts) < 1 or np.any(np.diff(ts) >= 0) or ts.min() < 0 or ts.max() >= T:
            raise ValueError("timesteps must be strictly descending inside [0, num_train_timesteps)")
        self.timesteps = ts
        self.num_inference_steps = len(ts)
        self._step_index = self._begin = 0

    def set_begin_index(self, begin_index: int = 0):
        k = int(begin_index)
        if not 0 <= k < len(self.timesteps):
            raise ValueError(f"begin_index {k} outside the {len(self.timesteps)} timesteps")
        self._step_index = self._begin = k

    def scale_model_input(self, sample, timestep=None):
        return sample

    def coefficients(self, i: int):
        """(c_x, c_eps, c_z, alpha_from, sigma_from) of step i in fp64: x' = c_x x + c_eps eps + c_z z."""
        ac, ts = self.alphas_cumprod, self.timesteps
        a_from, sg_from = math.sqrt(ac[ts[i]]), math.sqrt(1.0 - ac[ts[i]])
        s_from = sg_from / a_from
        last = i + 1 == len(ts)
        a_to = 1.0 if last else math.sqrt(ac[ts[i + 1]])
        s_to = 0.0 if last else math.sqrt(1.0 - ac[ts[i + 1]]) / a_to
        s_up = math.sqrt(s_to * s_to * (s_from * s_from - s_to * s_to) / (s_from * s_from))
        s_down = math.sqrt(s_to * s_to - s_up * s_up)
        return a_to / a_from, a_to * (s_down - s_from), 0.0 if last else a_to * s_up, a_from, sg_from

    @staticmethod
    def _draw(shape, generator, draw):
        if generator is None:
            return np.random.standard_normal(shape)
        if isinstance(generator, np.random.Generator):
            return generator.standard_normal(shape)
        if hasattr(generator, "randn"):
            return np.asarray(generator.randn(shape, stream="step", draw=draw))
        import torch
        return torch.randn(tuple(shape), generator=generator, device=generator.device).cpu().numpy()

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, **_):
        if len(self.timesteps) == 0:
            raise ValueError("call set_timesteps first")
        eps, like = _to_np(model_output)
        x, like_x = _to_np(sample)
        like = like_x if like_x is not None else like
        out_dtype = x.dtype
        eps, x = eps.astype(np.float64), x.astype(np.float64)
        i = self._step_index
        if float(timestep) != float(self.timesteps[i]):
            raise ValueError(f"step {i} expects timestep {self.timesteps[i]}, got {timestep}")
        c_x, c_eps, c_z, a_from, sg_from = self.coefficients(i)
        prev = c_x * x + c_eps * eps
        if c_z != 0.0:
            z = np.asarray(self._draw(x.shape, generator, i - self._begin), np.float64)
            prev = prev + c_z * z
        self.pred_original_sample = (x - sg_from * eps) / a_from
        self._step_index += 1
        return _wrap_out(prev, out_dtype, like, return_dict)

    def fused_lms(self, t_start: int = 0):
        """Arguments of Engine.lms_sample that run this scheduler's remaining steps inside the engine (PD_LMS_EULER_A); the
        noise is the engine's own seeded draw."""
        return dict(kind="euler_a", timesteps=[int(t) for t in self.timesteps[t_start:]])
