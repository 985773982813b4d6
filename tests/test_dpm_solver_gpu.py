"""GPU checks of the DPM-Solver++(2M) sampler (dd_set_schedule_s, solver 1): the fused step kernel at op level against float64, the
first-order cases as the DDIM kernels bit for bit, dd_expand against the step-by-step calls with an explicit history, direct guidance,
the defaults, the refusals, the whole loop against the fp32 oracle driven by tests/dpm_solver_ref.py::expand_2m, and the CLI.

Engine fixtures as in tests/test_sd2_engine_gpu.py: tiny_sd2_config (v-prediction) and tiny_config (epsilon), B = 2, L = 16, a 10-step
schedule, start index 5, guide window = steps 6 and 7.

Loop parity against the fp32 oracle, measured on an MI355X (latents rel L2 / image max abs / score rel); LOOP_BOUNDS are 1.5 x the 2M
figures (the box-to-box and build-to-build spread of these quantities: DESIGN.md 4.2) and are asserted to stay under the caps of
tests/test_noise_rng_gpu.py (0.06 / 0.16 / 0.01).  The DDIM figures are the same loops with solver="ddim" on both sides:
    (a) epsilon, leading, half schedule from image latents, transform guidance
            2M 0.0370 / 0.0802 / 0.000019 (bound 0.0555 / 0.1204 / 0.000029)    DDIM 0.0272 / 0.0531 / 0.000019
    (b) v-prediction, trailing, zero terminal SNR, phi = 0.7, text_to_img:
        guidance off
            2M 0.0142 / 0.0275 / -        (bound 0.0213 / 0.0413 / -)           DDIM 0.0134 / 0.0245 / -
        transform guidance
            2M 0.0334 / 0.0662 / 0.00047  (bound 0.0501 / 0.0993 / 0.00071)     DDIM 0.0168 / 0.0303 / 0.00014
The second-order term extrapolates along x0_i - x0_{i-1}, so it carries the bf16 engine's distance from the fp32 oracle in x0 further
than the DDIM step does; every bound stays under its cap.  In (a) the first guided step follows the first executed step, which has no
history: its score is the DDIM loop's."""
import contextlib
import ctypes as C
import dataclasses
import os

import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as D
import sampler_variants_ref as R

pytestmark = pytest.mark.gpu

ARGS = dict(guidance_scale=7.5, gs=1.0, ls=1.0, rho=10.0, guidance_period=2, guidance_step=4, constraint_value=0.2, strength=0.5,
            guidance_type="transform_guidance", num_inference_steps=10)
N_STEPS, START, FIRST = 10, 5, 6          # guide window = steps 6, 7 (guidance_step 4, guidance_period 2)
S = 7.5
CAPS = (0.06, 0.16, 0.01)
# (latents rel L2, image max abs, score rel), 1.5 x the figures in the module docstring
LOOP_BOUNDS = {("eps", "transform_guidance"): (0.0555, 0.1204, 0.000029), ("sd2", None): (0.0213, 0.0413, None),
               ("sd2", "transform_guidance"): (0.0501, 0.0993, 0.00071)}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def close(got, ref, what=""):
    """The op-level bound of tests/test_sampler_step_gpu.py: max|err| <= 1e-5 + 1e-5 max|ref|."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err, lim = (got - ref).abs().max().item(), 1e-5 + 1e-5 * ref.abs().max().item()
    assert err <= lim, "%s: max err %.4g > %.4g (ref max %.4g)" % (what, err, lim, ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
A_BEFORE, A, AP = 0.45, 0.64, 0.81
OP_SHAPES = [(2, 4, 64), (3, 4, 300), (2, 4, 9216)]       # (B, C, HW): one partial block; B != 2, a partial last block; 36 blocks


class Op:
    """One (prediction type, phi, shape) on the device: inputs, coefficient rows, scratch; m2 lives in 8-wide fp32 rows with 1e30 in
    the padding columns, so a kernel that lets padding into a result shows it."""

    def __init__(self, L, pred, phi, shape, seed=11):
        self.L, self.pred, self.code, self.phi = L, pred, R.PRED[pred], phi
        self.B, self.Cc, self.HW = shape
        g = torch.Generator().manual_seed(seed)
        self.z = torch.randn(self.B, self.Cc, self.HW, generator=g)
        self.m2 = torch.randn(2 * self.B, self.Cc, self.HW, generator=g)
        self.xp = torch.randn(self.B, self.Cc, self.HW, generator=g)
        rows = torch.full((2 * self.B * self.HW, 8), 1e30)
        rows[:, :self.Cc] = self.m2.permute(0, 2, 1).reshape(-1, self.Cc)
        self.d_rows, self.d_z = rows.cuda(), self.z.cuda()
        self.coef = torch.tensor([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, (1 - AP) ** 0.5]).cuda()
        out = (C.c_float * 4)()
        assert L.dd_op_step_coefs(self.code, A, AP, out) == 0
        self.lin = torch.tensor(list(out)).cuda()
        self.stats = torch.zeros(self.B, 8, device="cuda")
        self.part = torch.zeros(int(L.dd_op_sampler_step_scratch_floats(self.B, self.HW)), device="cuda")
        self.c = L.dd_op_step_coef_2m(3, 10, A_BEFORE, A, AP)
        assert self.c > 0.0

    def step_2m(self, x0_prev, c, x0=None):
        """-> (x0, z'); x0 given: written there (x0_prev itself = the in-place call)."""
        zp = torch.full_like(self.d_z, float("nan"))
        x0 = torch.full_like(self.d_z, float("nan")) if x0 is None else x0
        rc = self.L.dd_op_sampler_step_2m(P(self.d_rows), 8, P(self.d_z), P(x0_prev), c, P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef),
                                          P(self.lin), self.code, self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def step_ddim(self):
        zp, x0 = torch.full_like(self.d_z, float("nan")), torch.full_like(self.d_z, float("nan"))
        rc = self.L.dd_op_sampler_step(P(self.d_rows), 8, P(self.d_z), P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef), P(self.lin),
                                       self.code, self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def ref(self):
        """float64, in diffusers' form (dpm_solver_ref.update_2m_ref) on the CFG-mixed, rescaled model output."""
        u, c = self.m2.double().chunk(2)
        m = u + S * (c - u)
        if self.phi:
            m = R.rescale_noise_cfg(m, c, self.phi)
        return D.update_2m_ref(self.pred, A_BEFORE, A, AP, self.z.double(), m, self.xp.double())


@pytest.fixture(scope="module")
def L(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


@pytest.mark.parametrize("shape", OP_SHAPES)
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_op_step_2m_vs_float64(L, pred, phi, shape):
    op = Op(L, pred, phi, shape)
    # the library's c against the triple's float64 value, then the kernel with it against the diffusers form
    assert abs(op.c - D.coef_2m_ref(3, 10, A_BEFORE, A, AP)) <= 1e-6 * op.c
    x0, zp = op.step_2m(op.xp.cuda(), op.c)
    rx0, rzp = op.ref()
    close(x0, rx0, "%s phi %.1f x0" % (pred, phi))
    close(zp, rzp, "%s phi %.1f z'" % (pred, phi))
    # x0 is what the guidance calls differentiate: the bits of the first-order step, for every type
    assert torch.equal(x0, op.step_ddim()[0])
    # in place: the history buffer is read and written by the same call
    buf = op.xp.cuda()
    x0i, zpi = op.step_2m(buf, op.c, x0=buf)
    assert x0i is buf and torch.equal(buf, x0) and torch.equal(zpi, zp)


@pytest.mark.parametrize("pred,phi", [("epsilon", 0.0), ("epsilon", 0.7), ("v_prediction", 0.0), ("v_prediction", 0.7), ("sample", 0.0)])
def test_op_without_history_is_the_ddim_step_bitwise(L, pred, phi):
    op = Op(L, pred, phi, OP_SHAPES[1])
    x0, zp = op.step_ddim()
    nan = torch.full_like(op.d_z, float("nan"))
    for hist, c in ((None, op.c), (nan, 0.0), (None, 0.0)):              # no history; c = 0 with a history that must not be read
        gx0, gzp = op.step_2m(hist, c)
        assert torch.equal(gx0, x0) and torch.equal(gzp, zp)
    if pred == "epsilon" and phi == 0.0:                                   # and that is the cfg_ddim kernel
        zp2, x02 = torch.empty_like(zp), torch.empty_like(x0)
        assert L.dd_op_cfg_ddim(P(op.d_rows), 8, P(op.d_z), P(zp2), P(x02), op.B, op.Cc, op.HW, P(op.coef), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(zp2, zp) and torch.equal(x02, x0)
    # refused before any launch: a row stride the 16-byte loads cannot take, no x0 to write, a c that is not finite
    xp = op.xp.cuda()
    out = torch.empty_like(op.d_z)
    bad = [dict(ld=4), dict(x0=None), dict(c=float("inf")), dict(c=float("nan")), dict(code=3)]
    for kw in bad:
        rc = L.dd_op_sampler_step_2m(P(op.d_rows), kw.get("ld", 8), P(op.d_z), P(xp), kw.get("c", op.c), P(out), P(kw.get("x0", out)), op.B, op.Cc,
                                     op.HW, P(op.coef), P(op.lin), kw.get("code", op.code), op.phi, P(op.stats), P(op.part), None)
        assert rc != 0, kw


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def make_setup(kind):
    """kind 'sd2': tiny_sd2_config (v-prediction); 'eps': tiny_config (epsilon).  -> dict(cfg, eng, models, O, fx)."""
    from distdiff_amd.config import tiny_config, tiny_sd2_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.weights import synthetic_weights
    from oracle import sd_oracle as O
    cfg = (tiny_sd2_config if kind == "sd2" else tiny_config)(max_batch=2)
    g = torch.Generator().manual_seed(21 if kind == "sd2" else 22)
    B, Ls, T, Dm, W = 2, cfg.latent_size, cfg.text_len, cfg.guide.feature_dim, cfg.unet.cross_attention_dim
    fx = dict(z=torch.randn(B, 4, Ls, Ls, generator=g), lat=torch.randn(B, 4, Ls, Ls, generator=g) * 0.9,
              noise=torch.randn(B, 4, Ls, Ls, generator=g), e=torch.rand(B, 4, 1, 1, generator=g), b=torch.randn(B, 4, 1, 1, generator=g),
              prompt=torch.randn(B, T, W, generator=g), negative=torch.randn(1, T, W, generator=g).expand(B, -1, -1).contiguous(),
              Pc=F.normalize(torch.randn(5, Dm, generator=g), dim=-1), Pg=F.normalize(torch.randn(5, 3, Dm, generator=g), dim=-1),
              targets=torch.tensor([1, 3]))
    fx["emb"] = torch.cat([fx["negative"], fx["prompt"]])
    w = synthetic_weights(cfg, seed=0, num_classes=5)
    eng = Engine(cfg, w, enable_grad=True, max_guidance_period=2)
    try:
        eng.set_prototypes(fx["Pc"], fx["Pg"])
        eng.set_prompt(fx["emb"].cuda())
        unet, vae, guide, _ = O.build_models(cfg, w)
        yield dict(kind=kind, cfg=cfg, eng=eng, models=(unet, vae, guide), O=O, fx=fx)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def sd2(hip_lib):
    with make_setup("sd2") as s:
        yield s


@pytest.fixture(scope="module")
def eps(hip_lib):
    with make_setup("eps") as s:
        yield s


# the two sampler configurations of this module
V_TRAILING = dict(pred="v_prediction", spacing="trailing", phi=0.7)
EPS_LEADING = dict(pred="epsilon", spacing="leading", phi=0.0)


def schedule(s, solver="dpmsolver++", pred=None, spacing="leading", phi=0.0, zero_snr=False, default_solver=False):
    """Puts the same sampler on the engine and on the oracle; returns (oracle models incl. scheduler, timesteps, c_i of every step)."""
    from distdiff_amd.scheduler import DDIMSchedule
    cfg, eng = s["cfg"], s["eng"]
    sc = dataclasses.replace(cfg.scheduler, prediction_type=pred or cfg.scheduler.prediction_type, timestep_spacing=spacing,
                             rescale_betas_zero_snr=zero_snr)
    sched = DDIMSchedule(sc)
    ts = sched.set_timesteps(N_STEPS)
    a = ARGS
    kw = {} if default_solver else dict(solver=solver)
    eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                     rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"],
                     prediction_type=sc.prediction_type, guidance_rescale=phi, **kw)
    osched = R.VariantScheduler(sc)
    assert osched.set_timesteps(N_STEPS).tolist() == ts
    tr = D.triples(sched.alphas_cumprod, sched.final_alpha_cumprod, ts)
    cs = [eng.L.dd_op_step_coef_2m(i, N_STEPS, ab if ab is not None else 0.0, a_, ap) for i, (ab, a_, ap) in enumerate(tr)]
    return s["models"] + (osched,), ts, cs


def expand(s, gt, **kw):
    fx = s["fx"]
    return s["eng"].expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, gt, FIRST, 2, **kw)


def step_by_step(s, gt):
    """dd_expand's loop through the step-level calls, the history passed explicitly (a fresh tensor per step: out of place)."""
    eng, fx = s["eng"], s["fx"]
    zc = eng.add_noise(fx["lat"], fx["noise"], START)
    h, sc = None, None
    for i in range(START, N_STEPS):
        hp = None if i == N_STEPS - 1 else h
        if gt == "transform_guidance" and i == FIRST:
            zc, sc, _ = eng.transform_guidance(zc, fx["targets"], fx["e"], fx["b"], FIRST, 2)
            zc, h = eng.denoise_step(zc, i)
        elif gt == "direct_guidance" and FIRST <= i < FIRST + 2:
            zc, h, sc, _ = eng.direct_guidance(zc, fx["targets"], i, x0_prev=hp)
        else:
            zc, h = eng.denoise_step(zc, i, x0_prev=hp)
    return zc, sc


def test_first_order_cases_are_the_ddim_step_bitwise(sd2):
    eng, fx = sd2["eng"], sd2["fx"]
    _, ts, cs = schedule(sd2, **V_TRAILING)
    assert cs[0] == 0.0 and cs[-1] == 0.0 and all(c > 0.0 for c in cs[1:-1])
    z = fx["z"]
    for i in (0, 4, N_STEPS - 1):
        want = eng.denoise_step(z, i)
        got = eng.denoise_step(z, i, x0_prev=None)
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    nan = torch.full_like(z, float("nan"))
    for i in (0, N_STEPS - 1):                                             # c = 0 there: the history is not read
        want, got = eng.denoise_step(z, i), eng.denoise_step(z, i, x0_prev=nan)
        assert torch.isfinite(got[0]).all() and torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    # the same bits as under the DDIM solver, and an interior step with a history is another step
    first_order = eng.denoise_step(z, 4)
    second = eng.denoise_step(z, 4, x0_prev=fx["lat"])
    schedule(sd2, solver="ddim", **V_TRAILING)
    ddim = eng.denoise_step(z, 4)
    assert torch.equal(first_order[0], ddim[0]) and torch.equal(first_order[1], ddim[1])
    assert torch.equal(second[1], ddim[1]) and not torch.equal(second[0], ddim[0])
    close(second[0] - ddim[0], cs[4] * (ddim[1].double().cpu() - fx["lat"].double()), "z'_2M - z'_DDIM = c (x0 - x0_prev)")


@pytest.mark.parametrize("gt", [None, "transform_guidance", "direct_guidance"])
@pytest.mark.parametrize("which", ["sd2", "eps"])
def test_expand_is_the_step_by_step_calls_bitwise(request, which, gt):
    s = request.getfixturevalue(which)
    eng = s["eng"]
    schedule(s, **(V_TRAILING if which == "sd2" else EPS_LEADING))
    z, img, score = expand(s, gt)
    zc, sc = step_by_step(s, gt)
    assert torch.isfinite(z).all() and torch.equal(zc, z), "dd_expand and the step-by-step calls with an explicit history differ"
    assert torch.equal(eng.decode(zc), img)
    if gt:
        assert torch.equal(sc, score)
    z2, img2, score2 = expand(s, gt)                                      # the history buffer of the last call is not read
    assert torch.equal(z, z2) and torch.equal(img, img2) and torch.equal(score, score2)
    # generated inputs (noise_mode 1) take the same loop
    ids = [7, (3 << 32) | 2]
    za = expand(s, gt, seed=5, unit_ids=ids)[0]
    zb = expand(s, gt, seed=5, unit_ids=ids)[0]
    assert torch.isfinite(za).all() and torch.equal(za, zb) and not torch.equal(za, z)


@pytest.mark.parametrize("which", ["sd2", "eps"])
def test_direct_guidance_with_a_history(request, which):
    """The gradient flows through x0 alone, which does not depend on the history: g and x0 keep the bits of the DDIM call, and z_next
    moves by c (x0 - x0_prev)."""
    s = request.getfixturevalue(which)
    eng, fx = s["eng"], s["fx"]
    kw = V_TRAILING if which == "sd2" else EPS_LEADING
    _, ts, cs = schedule(s, **kw)
    zn2, x02, s2, g2 = eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"])
    zn0, x00, s0, g0 = eng.direct_guidance(fx["z"], fx["targets"], FIRST)             # no history: first-order
    schedule(s, solver="ddim", **kw)
    zn1, x01, s1, g1 = eng.direct_guidance(fx["z"], fx["targets"], FIRST)
    assert torch.isfinite(g2).all() and float(g2.abs().max()) > 0
    assert torch.equal(g2, g1) and torch.equal(x02, x01) and torch.equal(s2, s1)
    assert torch.equal(zn0, zn1) and torch.equal(g0, g1)
    assert cs[FIRST] > 0.0
    close(zn2 - zn1, cs[FIRST] * (x01.double().cpu() - fx["lat"].double()), "z_next_2M - z_next_DDIM")


def test_default_solver_is_ddim_bitwise(eps):
    schedule(eps, default_solver=True, **EPS_LEADING)
    want = expand(eps, "transform_guidance")
    schedule(eps, solver="ddim", **EPS_LEADING)
    got = expand(eps, "transform_guidance")
    for w_, g_ in zip(want, got):
        assert torch.isfinite(g_).all() and torch.equal(w_, g_)
    schedule(eps, solver="dpmsolver++", **EPS_LEADING)
    assert not torch.equal(expand(eps, "transform_guidance")[0], want[0])


def test_refusals(sd2):
    from distdiff_amd.engine import DDSamplerParams
    from distdiff_amd.scheduler import DDIMSchedule
    eng, fx = sd2["eng"], sd2["fx"]
    schedule(sd2, solver="ddim", **V_TRAILING)
    want = eng.denoise_step(fx["z"], 3)
    with pytest.raises(RuntimeError, match=r"\(-3\).*DPM-Solver"):                # DD_ERR_STATE
        eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"])
    with pytest.raises(RuntimeError, match=r"\(-3\).*DPM-Solver"):
        eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"])
    got = eng.denoise_step(fx["z"], 3)                                          # the engine stays usable
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    sched = DDIMSchedule(sd2["cfg"].scheduler)
    ts = sched.set_timesteps(N_STEPS)
    with pytest.raises(NotImplementedError, match="solver"):
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, solver="euler")
    import numpy as np
    tsa = np.asarray(ts, dtype=np.int32)
    for bad in (2, -1):                                                        # at the C level
        sp = DDSamplerParams(7.5, 1.0, 1.0, 10.0, 0.2, 1, 1, 2, 1, 0.0)
        rc = eng.L.dd_set_schedule_s(eng._h, tsa.ctypes.data_as(C.c_void_p), len(tsa), sched.alphas_cumprod.ctypes.data_as(C.c_void_p),
                                     len(sched.alphas_cumprod), float(sched.final_alpha_cumprod), C.byref(sp), bad)
        assert rc != 0 and b"solver" in eng.L.dd_last_error(eng._h)
    got = eng.denoise_step(fx["z"], 3)                                          # ... which left the schedule that was set
    assert torch.equal(want[0], got[0])


def loop_errors(s, case, gt, solver="dpmsolver++"):
    """(latents rel L2, image max abs, score rel or None) of dd_expand against the fp32 oracle's loop under the same solver.
    case 'half': from image latents at START (leading); 'full': text_to_img over the whole schedule (trailing, zero terminal SNR,
    phi = 0.7)."""
    eng, fx, O, cfg = s["eng"], s["fx"], s["O"], s["cfg"]
    if case == "half":
        phi = 0.0
        models, ts, _ = schedule(s, solver=solver, **EPS_LEADING)
        z, img, score = expand(s, gt)
        start, z0 = START, models[3].add_noise(fx["lat"], fx["noise"], ts[START])
    else:
        phi = 0.7
        models, ts, cs = schedule(s, solver=solver, zero_snr=True, **V_TRAILING)
        assert ts[0] == 999 and float(models[3].alphas_cumprod[999]) == 0.0 and cs[1] == 0.0
        z, img, score = eng.expand(None, fx["noise"], fx["e"], fx["b"], fx["targets"], 0, gt, FIRST, 2, text_to_img=True)
        start, z0 = 0, fx["noise"].clone()
    args = O.SamplerArgs(**{**ARGS, "guidance_type": gt})
    gts = ts[FIRST:FIRST + 2] if gt else []
    zr, imr, sr = D.expand_2m(args, cfg, models, z0, ts, start, gts, fx["emb"], fx["targets"], fx["e"], fx["b"], fx["Pc"], fx["Pg"], phi=phi,
                              second_order=solver == "dpmsolver++")
    assert torch.isfinite(z).all() and torch.isfinite(img).all()
    lat_err = float((z.cpu() - zr).norm() / zr.norm())
    img_err = float((img.cpu() - imr).abs().max())
    sc_err = abs(score.item() - float(sr)) / abs(float(sr)) if gt else None
    print("loop parity %s %s %s %s: latents rel %.4f, image max abs %.4f, score rel %s"
          % (s["kind"], case, gt, solver, lat_err, img_err, "%.5f" % sc_err if gt else "-"))
    return lat_err, img_err, sc_err


@pytest.mark.parametrize("which,case,gt", [("eps", "half", "transform_guidance"), ("sd2", "full", None), ("sd2", "full", "transform_guidance")])
def test_loop_vs_oracle(request, which, case, gt):
    """dd_expand under DPM-Solver++(2M) against the fp32 oracle's loop with the second-order term added on the test side
    (dpm_solver_ref.expand_2m).  Measured on an MI355X (latents rel L2 / image max abs / score rel): 0.0370 / 0.0802 / 0.000019 on the
    half schedule with transform guidance (epsilon); 0.0142 / 0.0275 / - and 0.0334 / 0.0662 / 0.00047 on the whole zero-SNR schedule
    (v-prediction) without and with transform guidance.  LOOP_BOUNDS are 1.5 x that; the DDIM figures are in the module docstring."""
    s = request.getfixturevalue(which)
    lat_err, img_err, sc_err = loop_errors(s, case, gt)
    bl, bi, bs = LOOP_BOUNDS[which, gt]
    assert bl <= CAPS[0] and bi <= CAPS[1] and (bs is None or bs <= CAPS[2])
    assert lat_err < bl and img_err < bi
    if gt:
        assert sc_err < bs


def test_cli_sampler_end_to_end(hip_lib, tmp_path):
    from distdiff_amd import generate_data as G

    def run(name, sampler):
        out = str(tmp_path / name)
        argv = ["--synthetic", "4", "--tiny", "--synthetic_classes", "2", "--output_dir", out, "--train_batch_size", "1", "--engine_batch", "4",
                "--steps", "10", "--strength", "0.5", "--total_split", "1", "--split", "0", "--num_images_per_prompt", "1", "--guidance_type",
                "transform_guidance", "--guidance_step", "4", "--guidance_period", "2", "--constraint_value", "0.2", "--optimize_targets",
                "global_prototype-local_prototype", "--K", "3", "--sampler", sampler]
        assert G.main(argv) == 0
        files = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs)
        assert sorted(os.path.basename(f) for f in files) == ["image_%04d_expand_0.png" % i for i in range(4)]
        return [open(f, "rb").read() for f in files]

    a, b, d = run("a", "dpmsolver++"), run("b", "dpmsolver++"), run("d", "ddim")
    assert a == b                                                            # deterministic
    assert all(x != y for x, y in zip(a, d))                                  # and another sampler than DDIM
