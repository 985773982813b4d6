"""GPU checks of SDE-DPM-Solver++(2M) (dd_set_schedule_sde, sde_eta = s in (0, 1]): the step kernel's HIST + NOISE form at op level
against float64 with explicit noise, the noise generated in registers against dd_randn_units' tensor bit for bit, the degenerate forms
against the kernels they must be, dd_expand against the step-by-step dd_*_hn calls bit for bit, direct guidance, transform guidance,
the defaults, packing independence, the fp16 library, the refusals, and the whole loop against the fp32 oracle driven by
tests/dpm_sde_ref.py::expand_sde.

Engine fixtures as in tests/test_dpm_solver_gpu.py: tiny_sd2_config (v-prediction) and tiny_config (epsilon), B = 2, L = 16, a 10-step
schedule, start index 5, guide window = steps 6 and 7.

Loop parity against the fp32 oracle (latents rel L2 / image max abs / score rel), s > 0 beside the same loop with s = 0 (dpmsolver++) on
both sides; the bound of each s > 0 figure is 2 x its s = 0 figure (the noise puts the loop on another trajectory; the score gets
max(2 x, 1e-3)), and under the caps of tests/test_noise_rng_gpu.py (0.06 / 0.16 / 0.01).  The figures measured on an MI355X are in
DESIGN.md section 15."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import dpm_sde_ref as SD
import dpm_solver_ref as D
import sampler_variants_ref as R
import test_dpm_solver_gpu as T

pytestmark = pytest.mark.gpu

ARGS, N_STEPS, START, FIRST, S, CAPS = T.ARGS, T.N_STEPS, T.START, T.FIRST, T.S, T.CAPS
P, close = T.P, T.close
A_BEFORE, A, AP = T.A_BEFORE, T.A, T.AP
# (B, C, HW): one partial block; B != 2 and a partial last block; HW % 4 != 0, so Philox blocks straddle channels; B past the 16 ids of
# one launch; 36 blocks
OP_SHAPES = [(2, 4, 64), (3, 4, 300), (2, 4, 49), (17, 4, 64), (2, 4, 9216)]
SEED, STREAM = 0x1234567899, 16 + 3


def unit_ids(B):
    return [(k * 7919 + 5) | ((k % 3) << 32) for k in range(B)]


class Op:
    """One (prediction type, phi, shape, s) on the device, as tests/test_ddim_eta_gpu.py::Op with a history: m2 in 8-wide fp32 rows with
    1e30 in the padding columns; coef / lin are the SDE rows (d in place of sqrt(1 - a')), c the SDE c of step 3 of 10."""

    def __init__(self, L, pred, phi, shape, s, z=None, m2=None, xp=None):
        self.L, self.pred, self.code, self.phi, self.s = L, pred, R.PRED[pred], phi, s
        self.B, self.Cc, self.HW = shape
        g = torch.Generator().manual_seed(11)
        self.z = torch.randn(self.B, self.Cc, self.HW, generator=g) if z is None else z
        self.m2 = torch.randn(2 * self.B, self.Cc, self.HW, generator=g) if m2 is None else m2
        self.xp = torch.randn(self.B, self.Cc, self.HW, generator=g) if xp is None else xp
        self.noise = torch.randn(self.B, self.Cc, self.HW, generator=g)
        rows = torch.full((2 * self.B * self.HW, 8), 1e30)
        rows[:, :self.Cc] = self.m2.permute(0, 2, 1).reshape(-1, self.Cc)
        self.d_rows, self.d_z = rows.cuda(), self.z.cuda()
        out = (C.c_float * 5)()
        assert L.dd_op_step_coefs_sde(self.code, A, AP, s, out) == 0
        self.sigma = float(out[4])
        self.lin = torch.tensor(list(out)[:4]).cuda()
        self.coef = torch.tensor([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, SD.sigma_d(A, AP, s)[1]]).cuda()
        cc = (C.c_float * 1)()
        assert L.dd_op_step_coef_2m_sde(3, 10, A_BEFORE, A, AP, s, cc) == 0
        self.c = float(cc[0])
        assert self.c > 0.0
        out4 = (C.c_float * 4)()
        assert L.dd_op_step_coefs(self.code, A, AP, out4) == 0
        self.lin0 = torch.tensor(list(out4)).cuda()
        self.coef0 = torch.tensor([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, (1 - AP) ** 0.5]).cuda()
        self.stats = torch.zeros(self.B, 8, device="cuda")
        self.part = torch.zeros(int(L.dd_op_sampler_step_scratch_floats(self.B, self.HW)), device="cuda")

    def step(self, x0_prev="xp", c=None, noise=None, ids=None, sigma=None, seed=SEED, stream=STREAM, x0=None, rc_want=0):
        """-> (x0, z') of dd_op_sampler_step_2m_n on the SDE rows: history `x0_prev` (device; default the op's own, None = none), explicit
        `noise` (device) or generated from `ids`; x0 given: written there (x0_prev itself = the in-place call)."""
        hist = self.xp.cuda() if isinstance(x0_prev, str) else x0_prev
        zp = torch.full_like(self.d_z, float("nan"))
        x0 = torch.full_like(self.d_z, float("nan")) if x0 is None else x0
        arr = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64)) if ids is not None else None
        rc = self.L.dd_op_sampler_step_2m_n(P(self.d_rows), 8, P(self.d_z), P(hist), self.c if c is None else c, P(noise),
                                            self.sigma if sigma is None else sigma, seed, stream,
                                            arr.ctypes.data_as(C.c_void_p) if arr is not None else None, P(zp), P(x0), self.B, self.Cc, self.HW,
                                            P(self.coef), P(self.lin), self.code, self.phi, P(self.stats), P(self.part), None)
        torch.cuda.synchronize()
        assert (rc == 0) == (rc_want == 0), rc
        return x0, zp

    def step_2m(self, x0_prev, c):
        """dd_op_sampler_step_2m on the same SDE rows."""
        zp, x0 = torch.full_like(self.d_z, float("nan")), torch.full_like(self.d_z, float("nan"))
        rc = self.L.dd_op_sampler_step_2m(P(self.d_rows), 8, P(self.d_z), P(x0_prev), c, P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef),
                                          P(self.lin), self.code, self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def step_n(self, noise=None, ids=None):
        """dd_op_sampler_step_n on the same SDE rows."""
        zp, x0 = torch.full_like(self.d_z, float("nan")), torch.full_like(self.d_z, float("nan"))
        arr = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64)) if ids is not None else None
        rc = self.L.dd_op_sampler_step_n(P(self.d_rows), 8, P(self.d_z), P(noise), self.sigma, SEED, STREAM,
                                         arr.ctypes.data_as(C.c_void_p) if arr is not None else None, P(zp), P(x0), self.B, self.Cc, self.HW,
                                         P(self.coef), P(self.lin), self.code, self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def step_ddim(self):
        zp, x0 = torch.full_like(self.d_z, float("nan")), torch.full_like(self.d_z, float("nan"))
        rc = self.L.dd_op_sampler_step(P(self.d_rows), 8, P(self.d_z), P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef0), P(self.lin0),
                                       self.code, self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def ref(self, noise):
        """float64, in the diffusers / k-diffusion form (dpm_sde_ref.update_sde_ref) on the CFG-mixed, rescaled model output."""
        u, c = self.m2.double().chunk(2)
        m = u + S * (c - u)
        if self.phi:
            m = R.rescale_noise_cfg(m, c, self.phi)
        return SD.update_sde_ref(self.pred, A_BEFORE, A, AP, self.s, self.z.double(), m, self.xp.double(), noise.double())


@pytest.fixture(scope="module")
def L(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module")
def sd2(hip_lib):
    with T.make_setup("sd2") as s:
        yield s


@pytest.fixture(scope="module")
def eps(hip_lib):
    with T.make_setup("eps") as s:
        yield s


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OP_SHAPES)
@pytest.mark.parametrize("s", [0.5, 1.0])
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_op_explicit_noise_vs_float64(L, pred, phi, s, shape):
    op = Op(L, pred, phi, shape, s)
    assert op.sigma > 0.0 and abs(op.c - SD.coef_2m_sde_ref(3, 10, A_BEFORE, A, AP, s)) <= 1e-6 * op.c
    nz = op.noise.cuda()
    x0, zp = op.step(noise=nz)
    rx0, rzp = op.ref(op.noise)
    close(x0, rx0, "%s phi %.1f s %.1f x0" % (pred, phi, s))
    close(zp, rzp, "%s phi %.1f s %.1f z'" % (pred, phi, s))
    # x0 depends neither on s nor on n nor on the history: the bits of the deterministic first-order step
    dx0, dzp = op.step_ddim()
    assert torch.equal(x0, dx0) and not torch.equal(zp, dzp)
    # the rounding statement: z'(n) = z' of the history kernel on the same rows and c, + sigma * n, the product rounded, then the sum
    hx0, hzp = op.step_2m(op.xp.cuda(), op.c)
    assert torch.equal(hx0, x0) and torch.equal(zp, hzp + nz * op.sigma)
    # in place: the history buffer is read and written by the same call
    buf = op.xp.cuda()
    x0i, zpi = op.step(x0_prev=buf, noise=nz, x0=buf)
    assert x0i is buf and torch.equal(buf, x0) and torch.equal(zpi, zp)


@pytest.mark.parametrize("shape", OP_SHAPES)
@pytest.mark.parametrize("pred,phi", [("epsilon", 0.0), ("v_prediction", 0.7), ("sample", 0.0)])
def test_op_generated_equals_explicit_bitwise(L, eps, pred, phi, shape):
    """The noise generated in registers is the tensor dd_randn_units writes for (seed, stream, unit id): same z' bit for bit, at every
    shape -- HW % 4 != 0 (blocks straddle channels), more than 16 rows (two launches over row ranges, the statistics computed once) --
    out of place and in place."""
    op = Op(L, pred, phi, shape, 1.0)
    ids = unit_ids(op.B)
    nz = eps["eng"].randn_units(SEED, STREAM, ids, op.Cc * op.HW).view(op.B, op.Cc, op.HW)
    ex0, ezp = op.step(noise=nz)
    gx0, gzp = op.step(ids=ids)
    assert torch.isfinite(gzp).all() and torch.equal(gzp, ezp) and torch.equal(gx0, ex0)
    buf = op.xp.cuda()
    ix0, izp = op.step(x0_prev=buf, ids=ids, x0=buf)
    assert torch.equal(izp, ezp) and torch.equal(buf, ex0)
    assert not torch.equal(op.step(ids=ids, stream=STREAM + 1)[1], gzp) and not torch.equal(op.step(ids=ids, seed=SEED + 1)[1], gzp)
    # position independence: the last row of the call alone, as a one-row call for that unit id
    k = op.B - 1
    one = Op(L, pred, phi, (1, op.Cc, op.HW), 1.0, z=op.z[k:k + 1].clone(), m2=op.m2[[k, op.B + k]].clone(), xp=op.xp[k:k + 1].clone())
    assert torch.equal(one.step(ids=[ids[k]])[1][0], gzp[k])


@pytest.mark.parametrize("pred,phi", [("epsilon", 0.0), ("epsilon", 0.7), ("v_prediction", 0.7), ("sample", 0.0)])
def test_op_degenerate_forms_bitwise(L, pred, phi):
    """sigma = 0 or no noise source: dd_op_sampler_step_2m; no history or c = 0 with noise: dd_op_sampler_step_n -- on the same rows."""
    op = Op(L, pred, phi, OP_SHAPES[1], 1.0)
    xp, nz = op.xp.cuda(), op.noise.cuda()
    nan = torch.full_like(op.d_z, float("nan"))
    ids = unit_ids(op.B)
    hx0, hzp = op.step_2m(xp, op.c)
    for kw in (dict(noise=nan, sigma=0.0), dict(ids=ids, sigma=0.0), dict()):        # a noise tensor that must not be read
        gx0, gzp = op.step(**kw)
        assert torch.equal(gx0, hx0) and torch.equal(gzp, hzp), kw
    for src in (dict(noise=nz), dict(ids=ids)):
        nx0, nzp = op.step_n(**src)
        for hk in (dict(x0_prev=None), dict(x0_prev=nan, c=0.0), dict(x0_prev=None, c=0.0)):   # a history that must not be read
            gx0, gzp = op.step(**hk, **src)
            assert torch.isfinite(gzp).all() and torch.equal(gx0, nx0) and torch.equal(gzp, nzp), (hk, list(src))
    # refused before any launch: a sigma or a c that is not finite, a reserved stream
    for kw in (dict(noise=nan, sigma=float("nan")), dict(noise=nan, sigma=float("inf")), dict(noise=nz, c=float("nan")),
               dict(noise=nz, c=float("inf")), dict(ids=ids, stream=7), dict(ids=ids, stream=2)):
        op.step(rc_want=1, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
V_TRAILING = dict(pred="v_prediction", spacing="trailing", phi=0.7, zero_snr=True)
EPS_LEADING = dict(pred="epsilon", spacing="leading", phi=0.0)
IDS = [7, (3 << 32) | 2]


def schedule(s, sde_eta=None, pred=None, spacing="leading", phi=0.0, zero_snr=False, solver="dpmsolver++", eta=None, n=N_STEPS):
    """Puts the same sampler on the engine (sde_eta None: set_schedule without the keyword) and on the oracle; returns (oracle models
    incl. scheduler, timesteps, (a_before, a, a') of every step)."""
    from distdiff_amd.scheduler import DDIMSchedule
    cfg, eng = s["cfg"], s["eng"]
    sc = dataclasses.replace(cfg.scheduler, prediction_type=pred or cfg.scheduler.prediction_type, timestep_spacing=spacing,
                             rescale_betas_zero_snr=zero_snr)
    sched = DDIMSchedule(sc)
    ts = sched.set_timesteps(n)
    a = ARGS
    kw = {} if sde_eta is None else dict(sde_eta=sde_eta)
    if eta is not None:
        kw["eta"] = eta
    eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                     rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"],
                     prediction_type=sc.prediction_type, guidance_rescale=phi, solver=solver, **kw)
    osched = R.VariantScheduler(sc)
    assert osched.set_timesteps(n).tolist() == ts
    return s["models"] + (osched,), ts, D.triples(sched.alphas_cumprod, sched.final_alpha_cumprod, ts)


def step_noise(s, i, seed=5, ids=IDS):
    eng, cfg = s["eng"], s["cfg"]
    Ls = cfg.latent_size
    return eng.randn_units(seed, 16 + i, ids, 4 * Ls * Ls).view(len(ids), 4, Ls, Ls)


def step_by_step(s, gt, z0, e, b, seed=5, ids=IDS, targets=None):
    """dd_expand's loop under sde_eta > 0 through the step-level calls: the history (a fresh tensor per step) and the noise of every step
    passed explicitly."""
    eng, fx = s["eng"], s["fx"]
    tg = fx["targets"] if targets is None else targets
    zc, h, sc = z0, None, None
    for i in range(START, N_STEPS):
        nz = step_noise(s, i, seed, ids)
        hp = None if i == N_STEPS - 1 else h
        if gt == "transform_guidance" and i == FIRST:
            zc, sc, _ = eng.transform_guidance(zc, tg, e, b, FIRST, 2)
            zc, h = eng.denoise_step(zc, i, step_noise=nz)                       # noise and no history
        elif gt == "direct_guidance" and FIRST <= i < FIRST + 2:
            zc, h, sc, _ = eng.direct_guidance(zc, tg, i, x0_prev=hp, step_noise=nz)
        else:
            zc, h = eng.denoise_step(zc, i, x0_prev=hp, step_noise=nz)
    return zc, sc


@pytest.mark.parametrize("gt", [None, "transform_guidance", "direct_guidance"])
@pytest.mark.parametrize("which", ["sd2", "eps"])
def test_expand_is_the_step_by_step_calls_bitwise(request, which, gt):
    s = request.getfixturevalue(which)
    eng, fx = s["eng"], s["fx"]
    kw = V_TRAILING if which == "sd2" else EPS_LEADING
    schedule(s, sde_eta=1.0, **kw)
    Ls = s["cfg"].latent_size

    def expand(seed, generate_inputs):
        return eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, gt, FIRST, 2, seed=seed, unit_ids=IDS,
                          generate_inputs=generate_inputs)

    # noise_mode 0: the caller's noise / e / b; seed and unit ids key the step noise alone
    z, img, score = expand(5, False)
    zc, sc = step_by_step(s, gt, eng.add_noise(fx["lat"], fx["noise"], START), fx["e"], fx["b"])
    assert torch.isfinite(z).all() and torch.equal(zc, z), "dd_expand and the step-by-step calls with explicit history and noise differ"
    assert torch.equal(eng.decode(zc), img)
    if gt:
        assert torch.equal(sc, score)
    z2, img2, score2 = expand(5, False)                                     # two runs: the history buffer of the last call is not read
    assert torch.equal(z, z2) and torch.equal(img, img2) and torch.equal(score, score2)
    assert not torch.equal(expand(6, False)[0], z)                          # another seed: other step noise on the same first latent
    # noise_mode 1: the first latent, e and b generated as well
    za = expand(5, True)[0]
    n0 = eng.randn_units(5, 0, IDS, 4 * Ls * Ls).view(2, 4, Ls, Ls)
    zg, _ = step_by_step(s, gt, eng.add_noise(fx["lat"], n0, START), eng.randn_units(5, 2, IDS, 4), eng.randn_units(5, 3, IDS, 4))
    assert torch.isfinite(za).all() and torch.equal(zg, za) and not torch.equal(za, z)
    assert torch.equal(expand(5, True)[0], za)
    # and the loop is neither the deterministic second-order one nor the first-order stochastic one
    schedule(s, **kw)
    zd = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, gt, FIRST, 2)[0]
    schedule(s, solver="ddim", eta=1.0, **kw)
    assert not torch.equal(zd, z) and not torch.equal(expand(5, False)[0], z)


@pytest.mark.parametrize("which", ["sd2", "eps"])
def test_direct_guidance_with_history_and_noise(request, which):
    """The gradient flows through x0 alone, which depends on neither s, n nor the history: g, x0 and the score keep the bits of the
    deterministic _h call, and z_next + rho g is the SDE step of the float64 reference on the first-order call's (z'_0, x0)."""
    s = request.getfixturevalue(which)
    eng, fx = s["eng"], s["fx"]
    kw = V_TRAILING if which == "sd2" else EPS_LEADING
    _, ts, tr = schedule(s, sde_eta=1.0, **kw)
    nz = step_noise(s, FIRST)
    zn1, x01, s1, g1 = eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"], step_noise=nz)
    znh, x0h, sh, gh = eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"])      # no noise: the dpmsolver++ step
    schedule(s, **kw)
    zn0, x00, s0, g0 = eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"])
    znf, x0f, _, gf = eng.direct_guidance(fx["z"], fx["targets"], FIRST)                          # first-order, deterministic
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(g1, g0) and torch.equal(x01, x00) and torch.equal(s1, s0)
    assert torch.equal(znh, zn0) and torch.equal(gh, g0) and torch.equal(x0h, x00) and not torch.equal(zn1, zn0)
    rho = ARGS["rho"]
    det = znf.double().cpu() + rho * gf.double().cpu()
    ab, a, ap = tr[FIRST]
    ref = SD.make_stochastic(det, x0f.double().cpu(), fx["lat"].double(), FIRST, N_STEPS, ab, a, ap, 1.0, nz.double().cpu())
    close(zn1.double().cpu() + rho * g1.double().cpu(), ref, "z_next + rho g under sde_eta = 1")


def test_transform_guidance_stays_deterministic(eps):
    eng, fx = eps["eng"], eps["fx"]
    schedule(eps, sde_eta=1.0, **EPS_LEADING)
    got = eng.transform_guidance(fx["z"], fx["targets"], fx["e"], fx["b"], FIRST, 2)
    schedule(eps, **EPS_LEADING)
    want = eng.transform_guidance(fx["z"], fx["targets"], fx["e"], fx["b"], FIRST, 2)
    for w_, g_ in zip(want, got):
        assert torch.isfinite(g_).all() and torch.equal(w_, g_)


def test_default_sde_eta_is_zero_bitwise(eps):
    eng, fx = eps["eng"], eps["fx"]
    schedule(eps, **EPS_LEADING)                                              # set_schedule() without sde_eta
    want = T.expand(eps, "transform_guidance")
    step = eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"])
    schedule(eps, sde_eta=0.0, **EPS_LEADING)
    got = T.expand(eps, "transform_guidance")
    for w_, g_ in zip(want, got):
        assert torch.isfinite(g_).all() and torch.equal(w_, g_)
    # seed and unit ids without generated inputs change nothing under sde_eta = 0
    got = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, "transform_guidance", FIRST, 2, seed=5, unit_ids=IDS,
                     generate_inputs=False)
    assert torch.equal(got[0], want[0])
    # without a noise source a step on an SDE schedule is the dpmsolver++ step
    schedule(eps, sde_eta=1.0, **EPS_LEADING)
    again = eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"])
    assert torch.equal(again[0], step[0]) and torch.equal(again[1], step[1])
    noisy = eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"], step_noise=fx["noise"])
    assert torch.equal(noisy[1], step[1]) and not torch.equal(noisy[0], step[0])


def test_unit_results_do_not_depend_on_row_or_batch(eps):
    """The final latents of a unit are a function of (seed, unit id) and its own inputs: the same unit in row 0 and in row 1, next to
    another neighbour, bit for bit; two unit ids differ."""
    eng, fx = eps["eng"], eps["fx"]
    schedule(eps, sde_eta=1.0, **EPS_LEADING)

    def run(ids, rows):
        r = torch.tensor(rows)
        eng.set_prompt(torch.cat([fx["negative"], fx["prompt"][r]]).cuda())   # the prompt travels with the unit's inputs
        return eng.expand(fx["lat"][r], None, None, None, fx["targets"][r], START, None, FIRST, 2, seed=5, unit_ids=ids)[0]

    try:
        a = run([7, 9], [0, 1])
        b = run([11, 7], [1, 0])
        assert torch.isfinite(a).all() and torch.equal(a[0], b[1]) and not torch.equal(a[1], b[0])
        c = run([7, 9], [0, 0])
        assert torch.equal(c[0], a[0]) and not torch.equal(c[0], c[1])      # the same inputs under two unit ids
    finally:
        eng.set_prompt(fx["emb"].cuda())


def test_fp16_library_expand_is_the_step_by_step_calls_bitwise(hip_lib):
    from distdiff_amd.config import tiny_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.weights import synthetic_weights
    cfg = tiny_config(max_batch=2)
    g = torch.Generator().manual_seed(22)
    Ls, Tn, Dm, W = cfg.latent_size, cfg.text_len, cfg.guide.feature_dim, cfg.unet.cross_attention_dim
    fx = dict(lat=torch.randn(2, 4, Ls, Ls, generator=g) * 0.9, noise=torch.randn(2, 4, Ls, Ls, generator=g),
              e=torch.rand(2, 4, 1, 1, generator=g), b=torch.randn(2, 4, 1, 1, generator=g), targets=torch.tensor([1, 3]))
    emb = torch.randn(4, Tn, W, generator=g)
    Pc = torch.nn.functional.normalize(torch.randn(5, Dm, generator=g), dim=-1)
    Pg = torch.nn.functional.normalize(torch.randn(5, 3, Dm, generator=g), dim=-1)
    eng = Engine(cfg, synthetic_weights(cfg, seed=0, num_classes=5), enable_grad=True, max_guidance_period=2, act_dtype="fp16")
    try:
        eng.set_prototypes(Pc, Pg)
        eng.set_prompt(emb.cuda())
        s = dict(cfg=cfg, eng=eng, fx=fx, models=(None, None, None))
        schedule(s, sde_eta=1.0, **EPS_LEADING)
        z, img, score = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, "direct_guidance", FIRST, 2, seed=5,
                                   unit_ids=IDS, generate_inputs=False)
        zc, sc = step_by_step(s, "direct_guidance", eng.add_noise(fx["lat"], fx["noise"], START), fx["e"], fx["b"])
        assert torch.isfinite(z).all() and torch.equal(zc, z) and torch.equal(sc, score)
    finally:
        eng.close()


def test_refusals(sd2):
    from distdiff_amd.engine import DDSamplerParams
    from distdiff_amd.scheduler import DDIMSchedule
    eng, fx = sd2["eng"], sd2["fx"]
    schedule(sd2, **V_TRAILING)                                               # dpmsolver++, deterministic
    want = eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"])

    def unchanged():
        got = eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"])
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])

    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"\(-1\).*sde_eta must be in \[0, 1\]"):
            schedule(sd2, sde_eta=bad, **V_TRAILING)
        unchanged()
    with pytest.raises(RuntimeError, match=r"\(-1\).*sde_eta.*solver"):
        schedule(sd2, sde_eta=0.5, solver="ddim", **V_TRAILING)
    unchanged()
    for solver in ("ddim", "dpmsolver++"):
        with pytest.raises(RuntimeError, match=r"\(-1\).*sde_eta > 0 needs eta = 0"):
            schedule(sd2, sde_eta=0.5, solver=solver, eta=0.5, **V_TRAILING)
        unchanged()
    with pytest.raises(RuntimeError, match="eta > 0.*solver"):                 # as before: eta alone does not go with solver 1
        schedule(sd2, eta=0.5, **V_TRAILING)
    unchanged()
    # more than 4096 steps, at the C level (a list no spacing produces)
    sched = DDIMSchedule(sd2["cfg"].scheduler)
    tsa = np.zeros(4097, dtype=np.int32) + 500
    sp = DDSamplerParams(7.5, 1.0, 1.0, 10.0, 0.2, 1, 1, 2, 1, 0.0)
    rc = eng.L.dd_set_schedule_sde(eng._h, tsa.ctypes.data_as(C.c_void_p), len(tsa), sched.alphas_cumprod.ctypes.data_as(C.c_void_p),
                                   len(sched.alphas_cumprod), float(sched.final_alpha_cumprod), C.byref(sp), 1, 0.0, 0.5)
    assert rc == -1 and b"sde_eta" in eng.L.dd_last_error(eng._h) and b"4096" in eng.L.dd_last_error(eng._h)
    unchanged()
    # step noise on a deterministic schedule: DD_ERR_STATE, with and without a history; in Python the pair is refused first
    with pytest.raises(RuntimeError, match=r"\(-3\).*eta = 0"):
        eng.denoise_step(fx["z"], 3, step_noise=fx["noise"])
    nz, hp, zp, x0 = fx["noise"].cuda(), fx["lat"].cuda(), torch.empty(2, 4, 16, 16, device="cuda"), torch.empty(2, 4, 16, 16, device="cuda")
    zc = fx["z"].cuda()
    assert eng.L.dd_denoise_step_hn(eng._h, P(zc), 3, P(hp), P(nz), P(zp), P(x0), 2, None) == -3
    assert b"eta = 0" in eng.L.dd_last_error(eng._h)
    with pytest.raises(ValueError, match="go together"):
        eng.denoise_step(fx["z"], 3, x0_prev=fx["lat"], step_noise=fx["noise"])
    with pytest.raises(ValueError, match="go together"):
        eng.direct_guidance(fx["z"], fx["targets"], FIRST, x0_prev=fx["lat"], step_noise=fx["noise"])
    unchanged()
    # either pointer of the _hn call may be NULL: the deterministic _h call
    assert eng.L.dd_denoise_step_hn(eng._h, P(zc), 3, P(hp), None, P(zp), P(x0), 2, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(zp, want[0]) and torch.equal(x0, want[1])
    # dd_expand under sde_eta > 0 needs unit_ids
    schedule(sd2, sde_eta=0.5, **V_TRAILING)
    with pytest.raises(RuntimeError, match=r"dd_expand failed \(-1\).*sde_eta.*unit_ids"):
        T.expand(sd2, None)
    unchanged()                                                               # without noise: the dpmsolver++ step


# ---------------------------------------------------------------------------------------------------------------------------------
# whole loop against the fp32 oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def loop_errors(s, case, gt, sde):
    """(latents rel L2, image max abs, score rel or None) of dd_expand against dpm_sde_ref.expand_sde with the n_i of dd_randn_units.
    case 'half': from image latents at START (epsilon, leading); 'full': text_to_img over the whole schedule (v-prediction, trailing,
    zero terminal SNR, phi = 0.7).  sde 0: the deterministic dpmsolver++ loop on both sides (set_schedule without sde_eta, no seed)."""
    eng, fx, O, cfg = s["eng"], s["fx"], s["O"], s["cfg"]
    kw = dict(seed=5, unit_ids=IDS, generate_inputs=False) if sde else {}
    if case == "half":
        phi = 0.0
        models, ts, _ = schedule(s, sde_eta=sde or None, **EPS_LEADING)
        z, img, score = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, gt, FIRST, 2, **kw)
        start, z0 = START, models[3].add_noise(fx["lat"], fx["noise"], ts[START])
    else:
        phi = 0.7
        models, ts, _ = schedule(s, sde_eta=sde or None, **V_TRAILING)
        assert ts[0] == 999 and float(models[3].alphas_cumprod[999]) == 0.0
        z, img, score = eng.expand(None, fx["noise"], fx["e"], fx["b"], fx["targets"], 0, gt, FIRST, 2, text_to_img=True, **kw)
        start, z0 = 0, fx["noise"].clone()
    noises = {i: step_noise(s, i).cpu() for i in range(start, N_STEPS)} if sde else {}
    args = O.SamplerArgs(**{**ARGS, "guidance_type": gt})
    gts = ts[FIRST:FIRST + 2] if gt else []
    zr, imr, sr = SD.expand_sde(args, cfg, models, z0, ts, start, gts, fx["emb"], fx["targets"], fx["e"], fx["b"], fx["Pc"], fx["Pg"], sde,
                                noises, phi=phi)
    assert torch.isfinite(z).all() and torch.isfinite(img).all()
    lat_err = float((z.cpu() - zr).norm() / zr.norm())
    img_err = float((img.cpu() - imr).abs().max())
    sc_err = abs(score.item() - float(sr)) / abs(float(sr)) if gt else None
    print("loop parity %s %s %s sde_eta %.1f: latents rel %.4f, image max abs %.4f, score rel %s"
          % (s["kind"], case, gt, sde, lat_err, img_err, "%.6f" % sc_err if gt else "-"))
    return lat_err, img_err, sc_err


@pytest.mark.parametrize("which,case,gt,sde", [("eps", "half", "transform_guidance", 1.0), ("sd2", "full", None, 1.0),
                                               ("eps", "half", "direct_guidance", 0.5)])
def test_loop_vs_oracle(request, which, case, gt, sde):
    """dd_expand under sde_eta > 0 against the fp32 oracle's loop made stochastic and second-order on the test side, beside the same loop
    under sde_eta = 0 (dpmsolver++).  Each of latents rel L2 and image max abs stays under 2 x its s = 0 figure and under the caps; the
    score under max(2 x its s = 0 figure, 1e-3).  Measured on an MI355X: DESIGN.md section 15."""
    s = request.getfixturevalue(which)
    l0, i0, s0 = loop_errors(s, case, gt, 0.0)
    l1, i1, s1 = loop_errors(s, case, gt, sde)
    assert l1 < min(2 * l0, CAPS[0]) and i1 < min(2 * i0, CAPS[1])
    if gt:
        assert s1 < min(max(2 * s0, 1e-3), CAPS[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_sde_eta_end_to_end(hip_lib, tmp_path):
    """--sampler dpmsolver++ --sde_eta 1 with counter-based inputs: a unit's PNG does not depend on how the run is packed (another row,
    other neighbours, the same --engine_batch: bit for bit), the expansions of one image differ from each other, and every image is
    another than under --sde_eta 0.  Against another --engine_batch the engine inputs are the same (tests/test_dpm_sde.py) and the PNGs
    are compared and reported only, as in tests/test_noise_rng_gpu.py: the GEMM tiling depends on the batch."""
    import os

    from PIL import Image

    from distdiff_amd import generate_data as G

    def run(name, sde, eb, extra=()):
        out = str(tmp_path / name)
        argv = ["--synthetic", "4", "--tiny", "--synthetic_classes", "2", "--output_dir", out, "--train_batch_size", "1", "--engine_batch", eb,
                "--steps", "20", "--strength", "0.5", "--total_split", "1", "--split", "0", "--num_images_per_prompt", "2", "--guidance_type",
                "transform_guidance", "--guidance_step", "8", "--guidance_period", "2", "--constraint_value", "0.2", "--optimize_targets",
                "global_prototype-local_prototype", "--K", "3", "--sampler", "dpmsolver++", "--sde_eta", sde, "--noise_rng", "philox"]
        assert G.main(argv + list(extra)) == 0
        return {f: os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs}

    raw = lambda path: open(path, "rb").read()
    px = lambda path: np.asarray(Image.open(path)).astype(np.int32)

    names = sorted("image_%04d_expand_%d.png" % (i, j) for i in range(4) for j in range(2))
    a, d = run("a", "1", "4"), run("d", "0", "4")
    assert sorted(a) == names and sorted(d) == names
    assert all(raw(a["image_%04d_expand_0.png" % i]) != raw(a["image_%04d_expand_1.png" % i]) for i in range(4))
    assert all(raw(a[k]) != raw(d[k]) for k in a)
    # the second expansions alone: one batch of (image 0..3, expand 1) where the full run had (image, expand) pairs of two images
    b = run("b", "1", "4", ["--first_image_index", "1"])
    assert sorted(b) == [k for k in names if k.endswith("_expand_1.png")] and all(raw(b[k]) == raw(a[k]) for k in b)
    c = run("c", "1", "8")
    diff = [int(np.abs(px(a[k]) - px(c[k])).max()) for k in names]
    print("sde_eta 1 PNGs, --engine_batch 4 vs 8: max abs difference per image (of 255):", diff)

