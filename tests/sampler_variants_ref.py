"""Test-side reference of the sampler variants (not a test module): a float64 restatement of diffusers 0.28 `DDIMScheduler.step`
(eta = 0) for the three prediction types and of `rescale_noise_cfg`, a `DDIMSchedulerOracle` subclass that knows trailing / linspace
spacing, zero-terminal-SNR betas and the three prediction types, and a patch of `oracle.sd_oracle.denoise_one_step` that applies the
classifier-free-guidance rescale (the oracle's own function has no hook for the conditional half).  The step restatement is checked
from first principles in tests/test_sampler_variants.py, so it is not a second copy of the formulas under test."""
import contextlib

import numpy as np
import torch

from oracle import sd_oracle as O

PRED = {"epsilon": 0, "v_prediction": 1, "sample": 2}


def step_ref(pred, a, ap, z, m):
    """(x0, z') of one DDIM step, eta = 0, written as diffusers writes it: first (x0, eps) from the model output, then the update.
    Works on float64 tensors (or any dtype: the arithmetic is the caller's)."""
    sa, sb = a ** 0.5, (1 - a) ** 0.5
    if pred == "epsilon":
        x0, eps = (z - sb * m) / sa, m
    elif pred == "v_prediction":
        x0, eps = sa * z - sb * m, sa * m + sb * z
    elif pred == "sample":
        x0, eps = m, (z - sa * m) / sb
    else:
        raise ValueError(pred)
    return x0, ap ** 0.5 * x0 + (1 - ap) ** 0.5 * eps


def rescale_noise_cfg(m, c, phi):
    """diffusers `rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale)`: std over every dim but the batch, unbiased."""
    dims = list(range(1, m.ndim))
    std_c, std_m = c.std(dim=dims, keepdim=True), m.std(dim=dims, keepdim=True)
    return phi * (m * (std_c / std_m)) + (1 - phi) * m


def cfg_step_ref(pred, a, ap, s, phi, z, u, c):
    """CFG mix + optional rescale + step; returns (x0, z', k) with k the per-image factor m^ / m."""
    m = u + s * (c - u)
    k = None
    if phi:
        dims = list(range(1, m.ndim))
        k = phi * c.std(dim=dims) / m.std(dim=dims) + 1 - phi
        m = rescale_noise_cfg(m, c, phi)
    x0, zp = step_ref(pred, a, ap, z, m)
    return x0, zp, k


class VariantScheduler(O.DDIMSchedulerOracle):
    """DDIMSchedulerOracle + timestep_spacing trailing / linspace, rescale_betas_zero_snr, prediction_type v_prediction / sample
    (diffusers 0.28 DDIMScheduler; `step` keeps the parent's previous-timestep rule for every spacing, as diffusers does)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        s = self.cfg
        if s.rescale_betas_zero_snr:
            T = s.num_train_timesteps
            if s.beta_schedule == "scaled_linear":
                betas = torch.linspace(s.beta_start ** 0.5, s.beta_end ** 0.5, T, dtype=torch.float32) ** 2
            else:
                betas = torch.linspace(s.beta_start, s.beta_end, T, dtype=torch.float32)
            abs_ = torch.cumprod(1.0 - betas, dim=0).sqrt()
            a0, aT = abs_[0].clone(), abs_[-1].clone()
            abs_ = (abs_ - aT) * (a0 / (a0 - aT))
            bar = abs_ ** 2
            alphas = torch.cat([bar[0:1], bar[1:] / bar[:-1]])
            self.alphas_cumprod = torch.cumprod(1.0 - (1 - alphas), dim=0)
            self.final_alpha_cumprod = torch.tensor(1.0) if s.set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, n):
        s = self.cfg
        self.num_inference_steps = n
        T = s.num_train_timesteps
        if s.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.int64) + s.steps_offset
        elif s.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        elif s.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n).round()[::-1].copy().astype(np.int64)
        else:
            raise ValueError(s.timestep_spacing)
        self.timesteps = torch.from_numpy(ts)
        return self.timesteps

    def step(self, model_output, timestep, sample, return_dict=True, **kw):
        a_t, a_p = self.coefficients(timestep)
        x0, prev = step_ref(self.cfg.prediction_type, a_t, a_p, sample, model_output)
        return {"prev_sample": prev, "pred_original_sample": x0}


@contextlib.contextmanager
def oracle_guidance_rescale(phi):
    """Inside the block `oracle.sd_oracle.denoise_one_step` -- looked up at call time by transform_guidance / direct_guidance /
    expand_one -- applies rescale_noise_cfg(phi) between the CFG mix and scheduler.step."""
    orig = O.denoise_one_step

    def denoise_one_step(args, latents, scheduler, t, unet, prompt_embeds):
        x = scheduler.scale_model_input(torch.cat([latents] * 2), t)
        u, c = unet(x, t, prompt_embeds, class_labels=None, return_dict=False)[0].chunk(2)
        m = u + args.guidance_scale * (c - u)
        if phi:
            m = rescale_noise_cfg(m, c, phi)
        out = scheduler.step(m, t, latents, return_dict=True)
        return out["prev_sample"], out["pred_original_sample"]

    O.denoise_one_step = denoise_one_step
    try:
        yield
    finally:
        O.denoise_one_step = orig
