"""Host-side DDIM schedule tables (what the reference gets from diffusers' DDIMScheduler.from_pretrained +
retrieve_timesteps, generate_data.py:863, 1043-1044). Only tables live here; the per-element update runs in the
sampler-step HIP kernel (csrc/sampler_step.hip).  Same fp32 torch / float64 numpy arithmetic as diffusers 0.28:
`beta_schedule` scaled_linear | linear, `rescale_betas_zero_snr`, `timestep_spacing` leading | trailing | linspace."""
import numpy as np

from .config import SchedulerConfig


class DDIMSchedule:
    def __init__(self, cfg: SchedulerConfig = None):
        self.cfg = cfg or SchedulerConfig()
        c = self.cfg
        T = c.num_train_timesteps
        import torch  # same fp32 linspace / cumprod arithmetic as diffusers' DDIMScheduler.__init__ (host-side table only)
        if c.beta_schedule == "scaled_linear":
            betas = torch.linspace(c.beta_start ** 0.5, c.beta_end ** 0.5, T, dtype=torch.float32) ** 2
        elif c.beta_schedule == "linear":
            betas = torch.linspace(c.beta_start, c.beta_end, T, dtype=torch.float32)
        else:
            raise NotImplementedError(c.beta_schedule)
        if c.rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.final_alpha_cumprod = 1.0 if c.set_alpha_to_one else float(self.alphas_cumprod[0])
        self.timesteps = None

    def set_timesteps(self, n):
        c = self.cfg
        T = c.num_train_timesteps
        if c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":              # steps_offset applies to `leading` only
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        elif c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n).round()[::-1].astype(np.int64)
        else:
            raise NotImplementedError("timestep_spacing=%r" % (c.timestep_spacing,))
        self.timesteps = [int(t) for t in ts]
        return self.timesteps


def rescale_zero_terminal_snr(betas):
    """diffusers' rescale_zero_terminal_snr (Lin et al. 2023, algorithm 1): shift sqrt(alphas_cumprod) so that its last value is 0,
    rescale so that its first is unchanged, and turn the result back into betas.  The last alphas_cumprod is then exactly 0."""
    import torch
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = alphas_bar_sqrt[0].clone(), alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= last
    alphas_bar_sqrt *= first / (first - last)
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1 - alphas


def start_index(strength, n_steps):
    """generate_data.py:1174."""
    return int((1 - strength) * n_steps)


def guide_window(n_steps, guidance_step, guidance_period):
    """Index window of guide_timesteps = timesteps[n-guidance_step : n-guidance_step+guidance_period] (:1178)."""
    assert guidance_step >= 1
    first = n_steps - guidance_step
    assert 0 <= first and first + guidance_period <= n_steps
    return first, guidance_period
