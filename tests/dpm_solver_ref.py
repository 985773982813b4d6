"""Test-side reference of the DPM-Solver++(2M) sampler (not a test module): a float64 restatement of the second-order update as
diffusers 0.28 `DPMSolverMultistepScheduler` writes it (algorithm_type dpmsolver++, solver_order 2, solver_type midpoint,
lower_order_final: lambda, h, r, D), the schedule's (a_{i-1}, a_i, a'_i) triples under the engine's previous-timestep rule, and a loop
`expand_2m` that drives the oracle's own `denoise_one_step` / `transform_guidance` / `direct_guidance` with
`sampler_variants_ref.VariantScheduler` and adds the second-order term under the engine's rules (no history at the first executed
step and at the step executed again after transform guidance; the final step first-order).  The library's form -- DDIM step +
c (x0 - x0_prev) -- is checked against this one in tests/test_dpm_solver.py, so neither is a copy of the other."""
import math

import torch

import sampler_variants_ref as R
from oracle import sd_oracle as O


def lam(a):
    """lambda(a) = ln(alpha / sigma) = ln(a / (1 - a)) / 2; -inf at a = 0, +inf at a = 1."""
    a = float(a)
    if a <= 0.0:
        return -math.inf
    if a >= 1.0:
        return math.inf
    return 0.5 * math.log(a / (1.0 - a))


def update_2m_ref(pred, a_before, a, ap, z, m, x0_prev):
    """(x0, z') of one second-order step in diffusers' form: z' = (sigma' / sigma) z - alpha' (e^-h - 1) D with
    D = x0 + (x0 - x0_prev) / (2 r), h = lambda' - lambda, r = (lambda - lambda_before) / h.  x0_prev None: D = x0 (first order)."""
    x0, _ = R.step_ref(pred, a, ap, z, m)
    h = lam(ap) - lam(a)
    D = x0
    if x0_prev is not None:
        r = (lam(a) - lam(a_before)) / h
        D = x0 + (x0 - x0_prev) / (2.0 * r)
    return x0, ((1.0 - ap) / (1.0 - a)) ** 0.5 * z - ap ** 0.5 * math.expm1(-h) * D


def coef_2m_ref(i, n, a_before, a, ap):
    """c_i in float64: sqrt(a') (1 - e^-h) / (2 r); 0 at i = 0, at i = n - 1 and wherever a lambda is not finite."""
    if i <= 0 or i >= n - 1:
        return 0.0
    l0, l1, l2 = lam(a_before), lam(a), lam(ap)
    if not all(math.isfinite(x) for x in (l0, l1, l2)):
        return 0.0
    h = l2 - l1
    r = (l1 - l0) / h
    return float(ap) ** 0.5 * -math.expm1(-h) / (2.0 * r)


def triples(alphas_cumprod, final_alpha_cumprod, timesteps, num_train=1000):
    """[(a_{i-1} or None, a_i, a'_i)] as float64, a' by the rule dd_set_schedule uses: t - num_train // n, final_alpha_cumprod below 0."""
    n = len(timesteps)
    out = []
    for i, t in enumerate(timesteps):
        prev = int(t) - num_train // n
        ap = float(alphas_cumprod[prev]) if prev >= 0 else float(final_alpha_cumprod)
        out.append((float(alphas_cumprod[int(timesteps[i - 1])]) if i else None, float(alphas_cumprod[int(t)]), ap))
    return out


def coefs_2m_ref(alphas_cumprod, final_alpha_cumprod, timesteps, num_train=1000):
    n = len(timesteps)
    return [coef_2m_ref(i, n, ab if ab is not None else 0.0, a, ap)
            for i, (ab, a, ap) in enumerate(triples(alphas_cumprod, final_alpha_cumprod, timesteps, num_train))]


def expand_2m(args, cfg, models, z, timesteps, start, gts, embeds, targets, e, b, Pc, Pg, phi=0.0, second_order=True):
    """The main loop of oracle.sd_oracle.expand_one from the latent `z` at timesteps[start:], with the second-order term.  gts: the
    guide timesteps ([] = none); args.guidance_type says which guidance.  second_order=False is the DDIM loop (the same code with
    c = 0).  Returns (latents, image in [0, 1], score)."""
    unet, vae, guide, sched = models
    ts = [int(t) for t in timesteps]
    n = len(ts)
    cs = coefs_2m_ref(sched.alphas_cumprod.double().numpy(), float(sched.final_alpha_cumprod), ts, sched.cfg.num_train_timesteps)
    gsz = cfg.guide.input_size
    score, hist = None, None
    with R.oracle_guidance_rescale(phi):
        for i in range(start, n):
            t = ts[i]
            c = cs[i] if (second_order and hist is not None and i != n - 1) else 0.0
            if gts and t == gts[0] and args.guidance_type == "transform_guidance":
                z, score, _ = O.transform_guidance(args, z, targets, gts, sched, unet, embeds, vae, guide, e, b, Pc, Pg, gsz)
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)        # off the history's trajectory: first-order
            elif gts and t in gts and args.guidance_type == "direct_guidance":
                z, x0, score, _ = O.direct_guidance(args, z, targets, t, sched, unet, embeds, vae, guide, Pc, Pg, gsz)
                if c:
                    z = z + c * (x0 - hist)
            else:
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)
                if c:
                    z = z + c * (x0 - hist)
            hist = x0
    with torch.no_grad():
        img = (vae.decode(z / vae.config.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    return z, img, score
