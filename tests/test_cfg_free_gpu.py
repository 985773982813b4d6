"""GPU checks of the CFG-free mode (dd_set_cfg_free / Engine(cfg_free=True): one UNet pass per step, on the conditional prompt alone).

Op level, bit for bit, on both libraries: dd_op_sampler_step1 on c against the two-half entry point on m2 = [c; c] at s = 7.5
(fmaf(s, c - c, c) == c for finite c), dd_op_sampler_step1_bwd against dd_op_sampler_step_bwd at coef[0] = 1 (1 * g and fmaf(1, g, 0)
are g).  Engine level: every entry point of a CFG-free tiny engine against the fp32 oracle run with
SamplerArgs(do_classifier_free_guidance=False), under the bounds tests/test_engine_gpu.py uses for the same quantity of the two-pass
engine (the network is the same, on half the rows, without the 7.5 x mix); denoise_step against dd_op_sampler_step1 on the engine's own
UNet output for every solver and noise mode, bit for bit; determinism; a two-pass engine beside it; the CLI."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

import ddim_eta_ref as E
import dpm_sde_ref as SD
import dpm_solver_ref as D
import sampler_variants_ref as R

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(__file__), "golden", "tiny_fixture.pt")
S = 7.5
A_BEFORE, A, AP = 0.45, 0.64, 0.81
SEED, STREAM = 0x1234567899, 16 + 3


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.isfinite(a).all()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def unit_ids(B):
    return [(k * 7919 + 5) | ((k % 3) << 32) for k in range(B)]


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def L(request, hip_lib):
    from distdiff_amd import _lib
    assert torch.cuda.is_available()
    if request.param == "fp16" and not os.path.exists(_lib.LIB_PATH_F16):
        pytest.skip("libdistdiff_hip_f16.so is not built")
    return _lib.lib(request.param)


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
def nhwc_rows(x, ld, fill):
    """[N, C, HW] -> fp32 rows [N*HW, ld], `fill` in the padding columns."""
    n, c, hw = x.shape
    rows = torch.full((n * hw, ld), fill, dtype=torch.float32)
    rows[:, :c] = x.permute(0, 2, 1).reshape(-1, c)
    return rows


class Fwd:
    """c ~ N(0,1) on the device as [B*HW, ld] rows and twice as [2B*HW, ld] rows, z, a history, a noise tensor; coefficient rows with
    s = 7.5 in coef[0].  1e30 in the padding columns: a kernel that lets padding into a result shows it."""

    def __init__(self, L, pred, shape):
        self.L, self.code = L, R.PRED[pred]
        self.B, self.Cc, self.HW, self.ld = shape
        g = torch.Generator().manual_seed(31)
        B, Cc, HW = self.B, self.Cc, self.HW
        c = torch.randn(B, Cc, HW, generator=g)
        self.z, self.xp, self.noise = (torch.randn(B, Cc, HW, generator=g).cuda() for _ in range(3))
        self.rows1 = nhwc_rows(c, self.ld, 1e30).cuda()
        self.rows2 = nhwc_rows(torch.cat([c, c]), self.ld, 1e30).cuda()
        self.coef = torch.tensor([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, 0.3]).cuda()
        out = (C.c_float * 4)()
        assert L.dd_op_step_coefs(self.code, A, AP, out) == 0
        self.lin = torch.tensor(list(out)).cuda()
        self.ids = np.ascontiguousarray(np.asarray(unit_ids(B), dtype=np.uint64))

    def run(self, one, hist, noise):
        """-> (x0, z') of dd_op_sampler_step1 (one) or dd_op_sampler_step_2m_n on [c; c]; noise: None | 'tensor' | 'generated'."""
        zp, x0 = torch.full_like(self.z, float("nan")), torch.full_like(self.z, float("nan"))
        xp, c2m = (self.xp, 0.37) if hist else (None, 0.0)
        nz = self.noise if noise == "tensor" else None
        ids = self.ids.ctypes.data_as(C.c_void_p) if noise == "generated" else None
        sigma = 0.21 if noise else 0.0
        head = (P(xp), c2m, P(nz), sigma, SEED, STREAM, ids, P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef), P(self.lin), self.code)
        if one:
            rc = self.L.dd_op_sampler_step1(P(self.rows1), self.ld, P(self.z), *head, None)
        else:
            rc = self.L.dd_op_sampler_step_2m_n(P(self.rows2), self.ld, P(self.z), *head, 0.0, None, None, None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return x0, zp


MODES = [(False, None), (True, None), (False, "tensor"), (False, "generated"), (True, "tensor"), (True, "generated")]


@pytest.mark.parametrize("hist,noise", MODES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", [(3, 4, 300, 8), (2, 8, 64, 16)])
def test_forward_op_is_the_two_half_op_on_c_c_bitwise(L, shape, pred, hist, noise):
    """(3, 4, 300, 8): a ragged last 256-block; (2, 8, 64, 16): both 16-byte loads of a row, padding columns beyond them.  The generated
    noise runs on B = 17: two launches over row ranges."""
    if noise == "generated":
        shape = (17,) + shape[1:]
    op = Fwd(L, pred, shape)
    x1, z1 = op.run(True, hist, noise)
    x2, z2 = op.run(False, hist, noise)
    assert torch.isfinite(z1).all() and torch.isfinite(x1).all()
    assert torch.equal(x1, x2) and torch.equal(z1, z2)
    # and the mode was taken: the history and the noise move z'
    x0, z0 = op.run(True, False, None)
    assert torch.equal(x0, x1) and (torch.equal(z0, z1) == (not hist and not noise))


@pytest.mark.parametrize("which", ["x0", "zprev", "both"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", [(3, 4, 300, 16), (2, 8, 64, 16), (3, 4, 300, 8)])
def test_backward_op_is_the_two_half_op_at_s_1_bitwise(L, shape, pred, which):
    """g_z identical, g_m the conditional rows of the two-half call at coef[0] = 1, every column written and the padding zero."""
    B, Cc, HW, ld = shape
    code = R.PRED[pred]
    g = torch.Generator().manual_seed(32)
    gx0 = torch.randn(B, Cc, HW, generator=g).cuda() if which != "zprev" else None
    gzp = torch.randn(B, Cc, HW, generator=g).cuda() if which != "x0" else None
    coef1 = torch.tensor([1.0, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, (1 - AP) ** 0.5]).cuda()
    coef_nan = coef1.clone()
    coef_nan[0] = float("nan")                      # the one-half kernel does not read coef[0]
    out = (C.c_float * 4)()
    assert L.dd_op_step_coefs(code, A, AP, out) == 0
    lin = torch.tensor(list(out)).cuda()
    junk = 0x7FC1                                   # a NaN pattern in both 16-bit formats: a column that is not written shows
    gm1 = torch.full((B * HW, ld), junk, dtype=torch.int16, device="cuda")
    gm2 = torch.full((2 * B * HW, ld), junk, dtype=torch.int16, device="cuda")
    gz1, gz2 = (torch.full((B, Cc, HW), float("nan"), device="cuda") for _ in range(2))
    assert L.dd_op_sampler_step1_bwd(P(gx0), P(gzp), P(gm1), ld, P(gz1), B, Cc, HW, P(coef_nan), P(lin), code, None) == 0
    assert L.dd_op_sampler_step_bwd(P(gx0), P(gzp), P(gm2), ld, P(gz2), B, Cc, HW, P(coef1), P(lin), code, 0.0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gz1).all() and torch.equal(gz1, gz2)
    assert torch.equal(gm1, gm2[B * HW:])
    assert not (gm1 == junk).any() and (gm1[:, Cc:] == 0).all() and (gm1[:, :Cc] != 0).any()
    assert (gm2[:B * HW, :Cc] & 0x7FFF == 0).all()      # (1 - s) g_m = 0 on the unconditional rows at s = 1


def test_op_refusals(L):
    """What the launchers refuse in front of any launch holds for the one-half entry points: outputs untouched."""
    op = Fwd(L, "epsilon", (2, 4, 64, 8))
    zp, x0 = torch.full_like(op.z, 7.0), torch.full_like(op.z, 7.0)
    bad = [dict(ld=4), dict(code=3), dict(Cc=9), dict(sigma=float("nan"), noise=True), dict(c2m=float("inf"), hist=True)]
    for kw in bad:
        rc = L.dd_op_sampler_step1(P(op.rows1), kw.get("ld", 8), P(op.z), P(op.xp) if kw.get("hist") else None, kw.get("c2m", 0.0),
                                   P(op.noise) if kw.get("noise") else None, kw.get("sigma", 0.0), SEED, STREAM, None, P(zp), P(x0), op.B,
                                   kw.get("Cc", op.Cc), op.HW, P(op.coef), P(op.lin), kw.get("code", op.code), None)
        assert rc != 0, kw
    gm = torch.full((2 * 64, 8), 0x7FC1, dtype=torch.int16, device="cuda")
    assert L.dd_op_sampler_step1_bwd(P(op.z), None, P(gm), 4, P(zp), 2, 4, 64, P(op.coef), P(op.lin), 0, None) != 0
    torch.cuda.synchronize()
    assert (zp == 7.0).all() and (x0 == 7.0).all() and (gm == 0x7FC1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level: the tiny fixture of tests/test_engine_gpu.py on a CFG-free engine, the oracle run with CFG off
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return torch.load(FIX, weights_only=False)


def make_engine(fx, cfg_free, **kw):
    from distdiff_amd.config import tiny_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    cfg = tiny_config(max_batch=2)
    w = synthetic_weights(cfg, seed=0, num_classes=5)
    eng = Engine(cfg, w, enable_grad=True, max_guidance_period=2, cfg_free=cfg_free, **kw)
    sched = DDIMSchedule(cfg.scheduler)
    ts = sched.set_timesteps(fx["n_steps"])
    assert ts == fx["timesteps"].tolist()
    a = fx["args"]
    eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                     rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"])
    eng.set_prototypes(fx["Pc"], fx["Pg"])
    eng.set_prompt((fx["prompt_embeds"] if cfg_free else torch.cat([fx["negative_embeds"], fx["prompt_embeds"]])).cuda())
    return cfg, w, eng, sched, ts


@pytest.fixture(scope="module")
def setup(hip_lib, fx):
    from oracle import sd_oracle as O
    cfg, w, eng, sched, ts = make_engine(fx, True)
    assert eng.L.dd_cfg_free(eng._h) == 1
    models = O.build_models(cfg, w)
    models[3].set_timesteps(fx["n_steps"])
    args = O.SamplerArgs(**{**fx["args"], "do_classifier_free_guidance": False})
    yield dict(cfg=cfg, eng=eng, models=models, O=O, args=args, sched=sched, ts=ts)
    eng.close()


def first_index(fx):
    return fx["timesteps"].tolist().index(fx["guide_timesteps"][0])


def test_unet_forward_and_denoise_step_vs_oracle(setup, fx):
    eng, O, args = setup["eng"], setup["O"], setup["args"]
    unet, vae, guide, sched = setup["models"]
    first = first_index(fx)
    with torch.no_grad():
        eps = unet(fx["z"], fx["timesteps"][5].item(), fx["prompt_embeds"])[0]
        rzp, rx0 = O.denoise_one_step(args, fx["z"], sched, fx["guide_timesteps"][0], unet, fx["prompt_embeds"])
    got = eng.unet_forward(fx["z"], 5)
    assert got.shape == fx["z"].shape                    # B images, not 2B
    zp, x0 = eng.denoise_step(fx["z"], first)
    fig = (rel(got, eps), rel(zp, rzp), rel(x0, rx0))
    print("cfg_free vs oracle: unet_forward %.4f, denoise_step z' %.4f x0 %.4f" % fig)
    assert fig[0] < 0.03 and fig[1] < 0.03 and fig[2] < 0.04
    with pytest.raises(AssertionError):                  # the prompt of a CFG-free engine is [B, T, D]
        eng.set_prompt(torch.cat([fx["negative_embeds"], fx["prompt_embeds"]]).cuda())


def test_unet_vjp_vs_autograd(setup, fx):
    eng = setup["eng"]
    unet = setup["models"][0]
    g = torch.Generator().manual_seed(11)
    gg = torch.randn(2, 4, setup["cfg"].latent_size, setup["cfg"].latent_size, generator=g)
    zr = fx["z"].clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(unet(zr, fx["timesteps"][5].item(), fx["prompt_embeds"])[0], zr, gg)
    r = rel(eng.unet_vjp(fx["z"], 5, gg), gz)
    print("cfg_free vs oracle: unet_vjp %.4f" % r)
    assert r < 0.05


def test_direct_guidance_vs_oracle(setup, fx):
    cfg, eng, O, args = setup["cfg"], setup["eng"], setup["O"], setup["args"]
    unet, vae, guide, sched = setup["models"]
    rzn, rx0, rs, _ = O.direct_guidance(args, fx["z"], fx["targets"], fx["guide_timesteps"][0], sched, unet, fx["prompt_embeds"], vae, guide,
                                        fx["Pc"], fx["Pg"], cfg.guide.input_size)
    zn, x0, score, gz = eng.direct_guidance(fx["z"], fx["targets"], first_index(fx))
    fig = (rel(zn, rzn), rel(x0, rx0), abs(score.item() - float(rs)) / abs(float(rs)))
    print("cfg_free vs oracle: direct_guidance z' %.4f x0 %.4f score rel %.6f" % fig)
    assert fig[0] < 0.03 and fig[1] < 0.04 and fig[2] < 0.01
    assert float(gz.abs().max()) > 0


def test_transform_guidance_vs_oracle(setup, fx):
    cfg, eng, O, args = setup["cfg"], setup["eng"], setup["O"], setup["args"]
    unet, vae, guide, sched = setup["models"]
    pe = fx["prompt_embeds"]
    rz, rs, _ = O.transform_guidance(args, fx["z"], fx["targets"], fx["guide_timesteps"], sched, unet, pe, vae, guide, fx["e"], fx["b"],
                                     fx["Pc"], fx["Pg"], cfg.guide.input_size)
    z, score, gz0 = eng.transform_guidance(fx["z"], fx["targets"], fx["e"], fx["b"], first_index(fx), 2)
    s_rel, z_rel = abs(score.item() - float(rs)) / abs(float(rs)), rel(z, rz)
    assert float((z.cpu() - fx["z"]).abs().max()) <= fx["args"]["constraint_value"] + 1e-5       # the L-inf ball, exactly
    # the gradients at the same image: the oracle's guide evaluated at the engine's decoded images (its images_at hook)
    imgs = [eng.guided_image(0), eng.guided_image(1)]
    _, s_at, (ge, gb) = O.transform_guidance(args, fx["z"], fx["targets"], fx["guide_timesteps"], sched, unet, pe, vae, guide, fx["e"], fx["b"],
                                             fx["Pc"], fx["Pg"], cfg.guide.input_size, images_at=imgs)
    ge_h = (gz0.cpu() * fx["z"]).sum((2, 3), keepdim=True)
    gb_h = gz0.cpu().sum((2, 3), keepdim=True)
    print("cfg_free vs oracle: transform_guidance score rel %.6f latents %.4f, gradients at the same image ge %.4f gb %.4f"
          % (s_rel, z_rel, rel(ge_h, ge), rel(gb_h, gb)))
    assert s_rel < 0.005 and z_rel < 0.07
    assert rel(ge_h, ge) < 0.08 and rel(gb_h, gb) < 0.08


@pytest.mark.parametrize("gt", ["transform_guidance", "direct_guidance", None])
def test_expand_vs_oracle_and_determinism(setup, fx, gt):
    cfg, eng, O = setup["cfg"], setup["eng"], setup["O"]
    args = O.SamplerArgs(**{**fx["args"], "do_classifier_free_guidance": False, "guidance_type": gt})
    zr, imr, sr = O.expand_one(args, cfg, setup["models"], fx["lat"], fx["noise"], fx["e"], fx["b"], fx["prompt_embeds"], None, fx["targets"],
                               fx["Pc"], fx["Pg"])
    first = first_index(fx)
    z, img, score = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], fx["start_index"], gt, first, 2)
    z_rel, i_err = rel(z, zr), float((img.cpu() - imr).abs().max())
    print("cfg_free vs oracle: expand %s latents %.4f image max abs %.4f" % (gt, z_rel, i_err))
    assert z_rel < 0.03 and i_err < 0.08
    if gt:
        assert abs(score.item() - float(sr)) < 0.005 * abs(float(sr))
    z2, img2, score2 = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], fx["start_index"], gt, first, 2)
    assert torch.equal(z, z2) and torch.equal(img, img2) and torch.equal(score, score2)


# ---------------------------------------------------------------------------------------------------------------------------------
# every solver and noise mode: denoise_step is dd_op_sampler_step1 on the engine's own UNet output with the schedule's row
# ---------------------------------------------------------------------------------------------------------------------------------
def schedule_row(Lb, code, mode, i, n, tr):
    """(coef, lin, sigma, c) of step i as dd_set_schedule_sde forms them (kernels.h: sampler_step_row), from the library's own host ops."""
    ab, a, ap = tr[i]
    ab = 0.0 if ab is None else ab
    out5, c1 = (C.c_float * 5)(), (C.c_float * 1)()
    if mode == "eta":
        assert Lb.dd_op_step_coefs_eta(code, a, ap, 0.5, out5) == 0
        d, c = E.sigma_d(a, ap, 0.5)[1], 0.0
    elif mode == "sde_eta":
        assert Lb.dd_op_step_coefs_sde(code, a, ap, 0.5, out5) == 0
        assert Lb.dd_op_step_coef_2m_sde(i, n, ab, a, ap, 0.5, c1) == 0
        d, c = SD.sigma_d(a, ap, 0.5)[1], float(c1[0])
    else:
        assert Lb.dd_op_step_coefs(code, a, ap, out5) == 0
        out5[4] = 0.0
        d, c = (1 - ap) ** 0.5, (Lb.dd_op_step_coef_2m(i, n, ab, a, ap) if mode == "dpmsolver++" else 0.0)
    coef = torch.tensor([float("nan"), a ** 0.5, (1 - a) ** 0.5, ap ** 0.5, d]).cuda()      # coef[0] is not read
    return coef, torch.tensor(list(out5)[:4]).cuda(), float(out5[4]), c


@pytest.mark.parametrize("mode", ["ddim", "dpmsolver++", "eta", "sde_eta"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_denoise_step_is_the_one_half_op_bitwise(setup, fx, pred, mode):
    """epsilon: the division form on coef; v_prediction (the same weights read as a v-model): the linear form on lin."""
    from distdiff_amd.scheduler import DDIMSchedule
    cfg, eng = setup["cfg"], setup["eng"]
    n, i = fx["n_steps"], 3
    sc = dataclasses.replace(cfg.scheduler, prediction_type=pred)
    sched = DDIMSchedule(sc)
    ts = sched.set_timesteps(n)
    a = fx["args"]
    kw = dict(solver="dpmsolver++" if mode in ("dpmsolver++", "sde_eta") else "ddim")
    if mode in ("eta", "sde_eta"):
        kw[mode] = 0.5
    try:
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                         rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"], prediction_type=pred, **kw)
        Ls = cfg.latent_size
        HW = Ls * Ls
        z = fx["z"].cuda()
        hist = fx["lat"].cuda() if mode in ("dpmsolver++", "sde_eta") else None
        nz = fx["noise"].cuda() if mode in ("eta", "sde_eta") else None
        zp, x0 = eng.denoise_step(z, i, x0_prev=hist, step_noise=nz)
        m = eng.unet_forward(z, i)
        rows = nhwc_rows(m.reshape(2, 4, HW).cpu(), 8, 0.0).cuda()
        coef, lin, sigma, c = schedule_row(eng.L, R.PRED[pred], mode, i, n, D.triples(sched.alphas_cumprod, sched.final_alpha_cumprod, ts))
        assert (sigma != 0.0) == (nz is not None) and (c != 0.0) == (hist is not None)
        ozp, ox0 = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
        rc = eng.L.dd_op_sampler_step1(P(rows), 8, P(z), P(hist), c, P(nz), sigma, 0, 0, None, P(ozp), P(ox0), 2, 4, HW, P(coef), P(lin),
                                       R.PRED[pred], None)
        torch.cuda.synchronize()
        assert rc == 0 and torch.isfinite(zp).all()
        assert torch.equal(x0, ox0) and torch.equal(zp, ozp)
        base = eng.denoise_step(z, i)                       # and the mode was taken
        assert torch.equal(base[1], x0) and (torch.equal(base[0], zp) == (mode == "ddim"))
    finally:
        restore_schedule(setup, fx)


def restore_schedule(setup, fx):
    eng, sched, a = setup["eng"], setup["sched"], fx["args"]
    eng.set_schedule(setup["ts"], sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                     rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"])


def test_guidance_rescale_is_refused_and_launches_nothing(setup, fx):
    """phi != 0 has no one-half form: dd_set_schedule* refuses it with a message and the engine keeps the schedule it had."""
    eng, sched, a = setup["eng"], setup["sched"], fx["args"]
    want = eng.denoise_step(fx["z"], 3)
    with pytest.raises(RuntimeError, match="guidance_rescale != 0 on a CFG-free engine"):
        eng.set_schedule(setup["ts"], sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], guidance_rescale=0.7)
    got = eng.denoise_step(fx["z"], 3)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


def test_guidance_scale_is_not_read(setup, fx):
    eng, sched, a = setup["eng"], setup["sched"], fx["args"]
    want = eng.denoise_step(fx["z"], 3)
    try:
        eng.set_schedule(setup["ts"], sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=1.0, gs=a["gs"], ls=a["ls"],
                         rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"])
        got = eng.denoise_step(fx["z"], 3)
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    finally:
        restore_schedule(setup, fx)


def test_two_pass_engine_in_the_same_process(setup, fx):
    """A default engine created beside the CFG-free one still gives the fixture step of tests/test_engine_gpu.py; its conditional half
    against the CFG-free UNet output is printed, not gated: the tile plans may differ at half the rows."""
    _, _, two, _, _ = make_engine(fx, False)
    try:
        assert two.L.dd_cfg_free(two._h) == 0
        zp, x0 = two.denoise_step(fx["z"], first_index(fx))
        assert rel(zp, fx["ref_denoise_z_prev"]) < 0.03 and rel(x0, fx["ref_denoise_x0"]) < 0.04
        both = two.unet_forward(fx["z"], 5)
        one = setup["eng"].unet_forward(fx["z"], 5)
        assert both.shape[0] == 2 * one.shape[0]
        d = (one - both[2:]).abs().max().item()
        print("cfg_free unet_forward vs the conditional half of a two-pass engine: rel L2 %.6f, max abs %.3g, bitwise %s"
              % (rel(one, both[2:]), d, torch.equal(one, both[2:])))
    finally:
        two.close()


def test_fp16_library_engine(hip_lib, fx):
    """The CFG-free engine of the fp16 library: finite, deterministic, and within the forward bound of the fp32 oracle's step."""
    from distdiff_amd import _lib
    if not os.path.exists(_lib.LIB_PATH_F16):
        pytest.skip("libdistdiff_hip_f16.so is not built")
    from oracle import sd_oracle as O
    cfg, w, eng, sched, ts = make_engine(fx, True, act_dtype="fp16")
    try:
        unet, vae, guide, osched = O.build_models(cfg, w)
        osched.set_timesteps(fx["n_steps"])
        args = O.SamplerArgs(**{**fx["args"], "do_classifier_free_guidance": False})
        with torch.no_grad():
            rzp, rx0 = O.denoise_one_step(args, fx["z"], osched, fx["guide_timesteps"][0], unet, fx["prompt_embeds"])
        zp, x0 = eng.denoise_step(fx["z"], first_index(fx))
        assert rel(zp, rzp) < 0.03 and rel(x0, rx0) < 0.04
        first = first_index(fx)
        a = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], fx["start_index"], "transform_guidance", first, 2)
        b = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], fx["start_index"], "transform_guidance", first, 2)
        assert all(torch.isfinite(t).all() and torch.equal(t, u) for t, u in zip(a, b))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_cfg_free_end_to_end(hip_lib, tmp_path):
    from distdiff_amd import generate_data as G

    def run(name, extra=()):
        out = str(tmp_path / name)
        argv = ["--synthetic", "4", "--tiny", "--synthetic_classes", "2", "--output_dir", out, "--train_batch_size", "1", "--engine_batch", "4",
                "--steps", "20", "--strength", "0.5", "--total_split", "1", "--split", "0", "--num_images_per_prompt", "2", "--guidance_type",
                "transform_guidance", "--guidance_step", "8", "--guidance_period", "2", "--constraint_value", "0.2", "--optimize_targets",
                "global_prototype-local_prototype", "--K", "3", "--seed", "0"]
        assert G.main(argv + list(extra)) == 0
        return {f: open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(out) for f in fs}

    names = sorted("image_%04d_expand_%d.png" % (i, j) for i in range(4) for j in range(2))
    a, b = run("a", ["--cfg_free"]), run("b", ["--cfg_free"])
    assert sorted(a) == names and sorted(b) == names
    assert all(a[k] == b[k] for k in names)
    c = run("c")                                            # and it is another sampler than the two-pass one
    assert sorted(c) == names and any(a[k] != c[k] for k in names)
