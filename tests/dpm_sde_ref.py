"""Test-side reference of SDE-DPM-Solver++(2M) (not a test module): a float64 restatement of the update as diffusers 0.28
`DPMSolverMultistepScheduler` (algorithm_type sde-dpmsolver++, solver_order 2, solver_type midpoint, lower_order_final) and k-diffusion
`sample_dpmpp_2m_sde` write it, with k-diffusion's eta as `s` (diffusers is s = 1):

    z' = (sigma'/sigma) e^(-s h) z + alpha' (1 - e^(-(1+s) h)) x0 + 1/2 alpha' (1 - e^(-(1+s) h)) (x0 - x0_prev) / r
         + sigma' sqrt(1 - e^(-2 s h)) n

the linear coefficients read off that function by probing it, the coefficient of the history term, and a loop `expand_sde`: the fp32
oracle loop of dpm_solver_ref.expand_2m made stochastic and second-order on the test side, with the rules of the engine (no history at the
first executed step and at the step executed again after transform guidance, the final step first-order, the look-ahead inside
transform guidance deterministic, direct guidance's rho g outside the stochastic step).  The library's form -- the linear step on rows
with d = sigma' e^(-s h) in place of sqrt(1 - a'), plus c_sde (x0 - x0_prev), plus sigma_n n -- is checked against this one in
tests/test_dpm_sde.py, so neither is a copy of the other."""
import math

import torch

import dpm_solver_ref as D
import sampler_variants_ref as R
from oracle import sd_oracle as O

lam = D.lam


def x0_of(pred, a, z, m):
    sa, sb = float(a) ** 0.5, (1.0 - float(a)) ** 0.5
    if pred == "epsilon":
        return (z - sb * m) / sa
    if pred == "v_prediction":
        return sa * z - sb * m
    if pred == "sample":
        return m
    raise ValueError(pred)


def update_sde_ref(pred, a_before, a, ap, s, z, m, x0_prev, n):
    """(x0, z') of one step in the diffusers / k-diffusion form above; x0_prev None: first order.  Needs 0 < a < 1 and a' < 1."""
    a, ap = float(a), float(ap)
    x0 = x0_of(pred, a, z, m)
    h = lam(ap) - lam(a)
    sig, sigp, alp = math.sqrt(1.0 - a), math.sqrt(1.0 - ap), math.sqrt(ap)
    g = -math.expm1(-(1.0 + s) * h)                        # 1 - e^(-(1+s) h)
    zp = sigp / sig * math.exp(-s * h) * z + alp * g * x0 + sigp * math.sqrt(-math.expm1(-2.0 * s * h)) * n
    if x0_prev is not None:
        r = (lam(a) - lam(a_before)) / h
        zp = zp + 0.5 * alp * g * (x0 - x0_prev) / r
    return x0, zp


def sigma_d(a, ap, s):
    """(sigma_n, d) with the limits the issue states: s = 0 or a' = a -> (0, sqrt(1-a')); a' = 1 -> (0, 0); a = 0 -> (sqrt(1-a'), 0)."""
    a, ap = float(a), float(ap)
    sbp = math.sqrt(1.0 - ap)
    if not s or ap >= 1.0:
        return 0.0, sbp
    if a <= 0.0:
        return sbp, 0.0
    h = lam(ap) - lam(a)
    if not h > 0.0:
        return 0.0, sbp
    return sbp * math.sqrt(-math.expm1(-2.0 * s * h)), sbp * math.exp(-s * h)


def coefs_sde_ref(pred, a, ap, s):
    """(A_z, A_m, B_z, B_m, sigma_n) in float64.  On a regular step (0 < a < a' < 1) read off update_sde_ref, which is linear in (z, m,
    n); on the limit steps from the limits of (sigma_n, d) in the form sqrt(a') x0 + d eps + sigma_n n."""
    a, ap = float(a), float(ap)
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    if 0.0 < a < ap < 1.0:
        f = lambda z, m, n: update_sde_ref(pred, None, a, ap, s, z, m, None, n)
    else:
        sg, d = sigma_d(a, ap, s)

        def f(z, m, n):
            sa, sb = a ** 0.5, (1.0 - a) ** 0.5
            x0 = x0_of(pred, a, z, m)
            eps = m if pred == "epsilon" else (sa * m + sb * z if pred == "v_prediction" else (z - sa * m) / sb)
            return x0, ap ** 0.5 * x0 + d * eps + sg * n
    xz, bz = f(one, zero, zero)
    xm, bm = f(zero, one, zero)
    _, sg = f(zero, zero, one)
    return tuple(float(v) for v in (xz, xm, bz, bm, sg))


def coef_2m_sde_ref(i, n, a_before, a, ap, s):
    """c_sde in float64: sqrt(a') (1 - e^(-(1+s) h)) / (2 r); 0 at i = 0, at i = n - 1 and wherever a lambda is not finite."""
    if i <= 0 or i >= n - 1:
        return 0.0
    l0, l1, l2 = lam(a_before), lam(a), lam(ap)
    if not all(math.isfinite(x) for x in (l0, l1, l2)):
        return 0.0
    h = l2 - l1
    r = (l1 - l0) / h
    return float(ap) ** 0.5 * -math.expm1(-(1.0 + s) * h) / (2.0 * r)


def make_stochastic(z0, x0, hist, i, n, a_before, a, ap, s, noise):
    """The deterministic first-order step's (z'_0, x0) -> the SDE step: eps = (z'_0 - sqrt(a') x0) / sqrt(1 - a'), then
    z' = sqrt(a') x0 + d eps + c_sde (x0 - hist) + sigma_n n.  At a' = 1 there is no eps to recover, d = sigma_n = 0 and c_sde = 0.
    Where sigma_n = 0 the engine takes the deterministic step, c of DPM-Solver++(2M) included."""
    a, ap = float(a), float(ap)
    sg, d = sigma_d(a, ap, s)
    if sg == 0.0:
        c = D.coef_2m_ref(i, n, a_before if a_before is not None else 0.0, a, ap) if hist is not None else 0.0
        return z0 + c * (x0 - hist) if c else z0
    sap = math.sqrt(ap)
    c = coef_2m_sde_ref(i, n, a_before if a_before is not None else 0.0, a, ap, s) if hist is not None else 0.0
    zp = sap * x0 + d * (z0 - sap * x0) / math.sqrt(1.0 - ap) + sg * noise
    return zp + c * (x0 - hist) if c else zp


def expand_sde(args, cfg, models, z, timesteps, start, gts, embeds, targets, e, b, Pc, Pg, s, noises, phi=0.0):
    """dpm_solver_ref.expand_2m with every step of the main loop made stochastic: noises[i] is n_i [B,C,L,L] of step index i
    (dd_randn_units(seed, 16 + i, ...)).  s = 0 is expand_2m (no arithmetic is added)."""
    if not s:
        return D.expand_2m(args, cfg, models, z, timesteps, start, gts, embeds, targets, e, b, Pc, Pg, phi=phi)
    unet, vae, guide, sched = models
    ts = [int(t) for t in timesteps]
    n = len(ts)
    tr = D.triples(sched.alphas_cumprod.double().numpy(), float(sched.final_alpha_cumprod), ts, sched.cfg.num_train_timesteps)
    gsz = cfg.guide.input_size
    score, hist = None, None

    def stoch(i, z0, x0, h):
        ab, a, ap = tr[i]
        return make_stochastic(z0, x0, h, i, n, ab, a, ap, s, noises[i].to(z0.dtype)).to(z0.dtype)

    with R.oracle_guidance_rescale(phi):
        for i in range(start, n):
            t = ts[i]
            h = hist if i != n - 1 else None
            if gts and t == gts[0] and args.guidance_type == "transform_guidance":
                z, score, _ = O.transform_guidance(args, z, targets, gts, sched, unet, embeds, vae, guide, e, b, Pc, Pg, gsz)
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)
                z = stoch(i, z, x0, None)                                       # off the history's trajectory: noise and no history
            elif gts and t in gts and args.guidance_type == "direct_guidance":
                z, x0, score, g = O.direct_guidance(args, z, targets, t, sched, unet, embeds, vae, guide, Pc, Pg, gsz)
                z = stoch(i, z + args.rho * g, x0, h) - args.rho * g
            else:
                with torch.no_grad():
                    z, x0 = O.denoise_one_step(args, z, sched, t, unet, embeds)
                z = stoch(i, z, x0, h)
            hist = x0
    with torch.no_grad():
        img = (vae.decode(z / vae.config.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    return z, img, score

