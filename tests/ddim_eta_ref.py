"""Test-side reference of stochastic DDIM, eta in [0, 1] (not a test module): a float64 restatement of diffusers 0.28
`DDIMScheduler.step(eta=..., use_clipped_model_output=False, variance_noise=n)` written from (pred, a, a', eta, z, m, n) -- first (x0, eps)
from the model output by the three prediction types' formulas, then the update -- the linear coefficients read off that function by
probing it (it is linear in (z, m, n)), the DDPM posterior mean it has to reduce to at eta = 1, and a loop `expand_eta` that drives the
oracle's own `denoise_one_step` / `transform_guidance` / `direct_guidance` (which step with eta = 0) and turns the (z', x0) of every
stochastic step into the eta > 0 step with noise the caller passes in.  The library's form -- the linear step on coefficient rows with d
in place of sqrt(1 - a'), plus sigma n -- is checked against this one in tests/test_ddim_eta.py, so neither is a copy of the other."""
import math

import torch

import dpm_solver_ref as D
import sampler_variants_ref as R
from oracle import sd_oracle as O


def sigma_d(a, ap, eta):
    """(sigma, d): sigma = eta sqrt(var), var = (1 - a') / (1 - a) (1 - a / a') (diffusers `_get_variance`), d = sqrt(max(0, 1 - a' -
    sigma^2)).  diffusers has no max: at a = 0 and eta = 1 its radicand is +-1e-16 and the negative sign is a NaN there."""
    a, ap = float(a), float(ap)
    sigma = eta * math.sqrt((1.0 - ap) / (1.0 - a) * (1.0 - a / ap)) if eta else 0.0
    return sigma, math.sqrt(max(0.0, 1.0 - ap - sigma * sigma))


def step_eta_ref(pred, a, ap, eta, z, m, n):
    """(x0, z') of one step as diffusers writes it: x0 and eps from the model output, then sqrt(a') x0 + d eps + sigma n."""
    sa, sb = float(a) ** 0.5, (1.0 - float(a)) ** 0.5
    if pred == "epsilon":
        x0, eps = (z - sb * m) / sa, m
    elif pred == "v_prediction":
        x0, eps = sa * z - sb * m, sa * m + sb * z
    elif pred == "sample":
        x0, eps = m, (z - sa * m) / sb
    else:
        raise ValueError(pred)
    sigma, d = sigma_d(a, ap, eta)
    return x0, float(ap) ** 0.5 * x0 + d * eps + sigma * n


def coefs_eta_ref(pred, a, ap, eta):
    """(A_z, A_m, B_z, B_m, sigma) in float64, read off step_eta_ref: it is linear in (z, m, n), so its value at the unit inputs is the
    coefficient."""
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    xz, bz = step_eta_ref(pred, a, ap, eta, one, zero, zero)
    xm, bm = step_eta_ref(pred, a, ap, eta, zero, one, zero)
    _, sg = step_eta_ref(pred, a, ap, eta, zero, zero, one)
    return tuple(float(v) for v in (xz, xm, bz, bm, sg))


def posterior_mean(a, ap, x0, z):
    """Mean of the DDPM posterior q(z' | z, x0) between the levels a and a' (Ho et al. 2020, eq. 7, with alpha_t = a / a')."""
    a, ap = float(a), float(ap)
    return math.sqrt(ap) * (1.0 - a / ap) / (1.0 - a) * x0 + math.sqrt(a / ap) * (1.0 - ap) / (1.0 - a) * z


def make_stochastic(z0, x0, a, ap, eta, n):
    """The deterministic step's (z'_0, x0) -> the eta step: eps = (z'_0 - sqrt(a') x0) / sqrt(1 - a'), z' = sqrt(a') x0 + d eps + sigma n.
    At a' = 1 there is no eps to recover, and d and sigma are both 0: z' = z'_0."""
    a, ap = float(a), float(ap)
    if ap >= 1.0:
        return z0
    sigma, d = sigma_d(a, ap, eta)
    sap = math.sqrt(ap)
    return sap * x0 + d * (z0 - sap * x0) / math.sqrt(1.0 - ap) + sigma * n


def expand_eta(args, cfg, models, z, timesteps, start, gts, embeds, targets, e, b, Pc, Pg, eta, noises, phi=0.0):
    """The loop of dpm_solver_ref.expand_2m with second_order=False, every step of the main loop made stochastic: noises[i] is n_i
    [B,C,L,L] of step index i.  The look-ahead inside O.transform_guidance stays as the oracle has it (eta = 0); the step executed again
    after it is stochastic.  In direct guidance the oracle returns z'_0 - rho g and g: the eta step is taken on z'_0 and rho g subtracted
    from it, as dd_direct_guidance_n does.  eta = 0 is expand_2m(second_order=False) exactly (no arithmetic is added)."""
    unet, vae, guide, sched = models
    ts = [int(t) for t in timesteps]
    n = len(ts)
    tr = D.triples(sched.alphas_cumprod.double().numpy(), float(sched.final_alpha_cumprod), ts, sched.cfg.num_train_timesteps)
    gsz = cfg.guide.input_size
    score = None

    def stoch(i, z0, x0):
        return make_stochastic(z0, x0, tr[i][1], tr[i][2], eta, noises[i].to(z0.dtype)).to(z0.dtype) if eta else z0

    with R.oracle_guidance_rescale(phi):
        for i in range(start, n):
            t = ts[i]
            if gts and t == gts[0] and args.guidance_type == "transform_guidance":
                z, score, _ = O.transform_guidance(args, z, targets, gts, sched, unet, embeds, vae, guide, e, b, Pc, Pg, gsz)
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)
                z = stoch(i, z, x0)
            elif gts and t in gts and args.guidance_type == "direct_guidance":
                z, x0, score, g = O.direct_guidance(args, z, targets, t, sched, unet, embeds, vae, guide, Pc, Pg, gsz)
                if eta:
                    z = stoch(i, z + args.rho * g, x0) - args.rho * g
            else:
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)
                z = stoch(i, z, x0)
    with torch.no_grad():
        img = (vae.decode(z / vae.config.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    return z, img, score
