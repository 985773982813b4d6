"""Engine-level parity of the SD-2.x family (config.tiny_sd2_config: head dim 64 on every level, linear projections, a cross-attention
width that differs from the UNet's; v-prediction) and of the sampler variants, against the fp32 oracle with the test-side scheduler of
tests/sampler_variants_ref.py in models[3].  Classifier-free-guidance rescale on the oracle's side: sampler_variants_ref.
oracle_guidance_rescale patches oracle.sd_oracle.denoise_one_step.

Bounds are those of tests/test_engine_gpu.py (tiny column) for the same quantities: forward tensors <= 3 %, scores
<= 0.5 %, energy gradient at the SAME image <= 5 % (g_z of direct guidance) and 5 % / 8 % (ge / gb of two chained steps), latents after the
transform update <= 7 % and == the update rule on the engine's own gradient to 2e-4, UNet VJP with random cotangents <= 5 %.
The whole loop from pure noise (text_to_img, trailing, zero terminal SNR, v-prediction, phi = 0.7: the configuration that meets
alphas_cumprod = 0) has no bound of its own to inherit: T2I_BOUNDS are 1.5 x the figures measured on an MI355X, under the caps of
tests/test_noise_rng_gpu.py (6 % / 0.16 / 1 %)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import sampler_variants_ref as R

pytestmark = pytest.mark.gpu

ARGS = dict(guidance_scale=7.5, gs=1.0, ls=1.0, rho=10.0, guidance_period=2, guidance_step=4, constraint_value=0.2, strength=0.5,
            guidance_type="transform_guidance", num_inference_steps=10)
N_STEPS, FIRST = 10, 6          # guide window = steps 6, 7 (guidance_step 4, guidance_period 2)
T2I_CAPS = (0.06, 0.16, 0.01)
# measured (latents rel L2, image max abs, score rel): guidance off 0.0134 / 0.0245 / -; transform guidance 0.0168 / 0.0303 / 0.00014
T2I_BOUNDS = {None: (0.0201, 0.0368, None), "transform_guidance": (0.0252, 0.0455, 0.00021)}


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.isfinite(a).all()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


@pytest.fixture(scope="module")
def fx():
    g = torch.Generator().manual_seed(21)
    B, L, T, D, W = 2, 16, 13, 256, 128
    return dict(z=torch.randn(B, 4, L, L, generator=g), lat=torch.randn(B, 4, L, L, generator=g) * 0.9, noise=torch.randn(B, 4, L, L, generator=g),
                e=torch.rand(B, 4, 1, 1, generator=g), b=torch.randn(B, 4, 1, 1, generator=g),
                prompt=torch.randn(B, T, W, generator=g), negative=torch.randn(1, T, W, generator=g).expand(B, -1, -1).contiguous(),
                Pc=F.normalize(torch.randn(5, D, generator=g), dim=-1), Pg=F.normalize(torch.randn(5, 3, D, generator=g), dim=-1),
                targets=torch.tensor([1, 3]))


@pytest.fixture(scope="module")
def setup(hip_lib, fx):
    from distdiff_amd.config import tiny_sd2_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.weights import synthetic_weights
    from oracle import sd_oracle as O
    cfg = tiny_sd2_config(max_batch=2)
    assert cfg.guide.feature_dim == fx["Pc"].shape[1]
    w = synthetic_weights(cfg, seed=0, num_classes=5)
    eng = Engine(cfg, w, enable_grad=True, max_guidance_period=2)
    eng.set_prototypes(fx["Pc"], fx["Pg"])
    eng.set_prompt(torch.cat([fx["negative"], fx["prompt"]]).cuda())
    unet, vae, guide, _ = O.build_models(cfg, w)
    yield cfg, eng, (unet, vae, guide), O
    eng.close()


def schedule(setup, phi=0.0, spacing="leading", zero_snr=False, pred="v_prediction", **kw):
    """Puts the same sampler on both sides; returns the oracle's models tuple and the timesteps."""
    import dataclasses
    from distdiff_amd.scheduler import DDIMSchedule
    cfg, eng, (unet, vae, guide), O = setup
    sc = dataclasses.replace(cfg.scheduler, prediction_type=pred, timestep_spacing=spacing, rescale_betas_zero_snr=zero_snr)
    sched = DDIMSchedule(sc)
    ts = sched.set_timesteps(N_STEPS)
    a = ARGS
    if kw.get("plain_call"):
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                         rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"])
    else:
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                         rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"], prediction_type=pred,
                         guidance_rescale=phi)
    osched = R.VariantScheduler(sc)
    assert osched.set_timesteps(N_STEPS).tolist() == ts
    assert torch.equal(osched.alphas_cumprod, torch.from_numpy(sched.alphas_cumprod))
    return (unet, vae, guide, osched), ts


def test_one_step_v_prediction(setup, fx):
    cfg, eng, _, O = setup
    models, ts = schedule(setup)
    emb = torch.cat([fx["negative"], fx["prompt"]])
    zp, x0 = eng.denoise_step(fx["z"], FIRST)
    with torch.no_grad():
        rzp, rx0 = O.denoise_one_step(O.SamplerArgs(**ARGS), fx["z"], models[3], ts[FIRST], models[0], emb)
    print("one step v-prediction: z' rel %.4f, x0 rel %.4f" % (rel(zp, rzp), rel(x0, rx0)))
    assert rel(zp, rzp) < 0.03 and rel(x0, rx0) < 0.03


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guidance_v_prediction_at_the_same_image(setup, fx, phi):
    cfg, eng, _, O = setup
    models, ts = schedule(setup, phi)
    unet, vae, guide, sched = models
    args = O.SamplerArgs(**ARGS)
    emb = torch.cat([fx["negative"], fx["prompt"]])
    gts = ts[FIRST:FIRST + 2]
    z0 = fx["z"]
    with R.oracle_guidance_rescale(phi):
        # direct guidance: per-pixel g_z
        zn, x0, score, gz = eng.direct_guidance(z0, fx["targets"], FIRST)
        img = eng.guided_image(0)
        rzn, rx0, sc_ref, g_ref = O.direct_guidance(args, z0, fx["targets"], gts[0], sched, unet, emb, vae, guide, fx["Pc"], fx["Pg"],
                                                    cfg.guide.input_size, image_at=img)
        d_sc, d_g = abs(score.item() - float(sc_ref)) / abs(float(sc_ref)), rel(gz, g_ref)
        # transform guidance: two chained steps
        z, score, gz0 = eng.transform_guidance(z0, fx["targets"], fx["e"], fx["b"], FIRST, 2)
        imgs = [eng.guided_image(0), eng.guided_image(1)]
        z_ref, s_ref, (ge, gb) = O.transform_guidance(args, z0, fx["targets"], gts, sched, unet, emb, vae, guide, fx["e"], fx["b"], fx["Pc"],
                                                      fx["Pg"], cfg.guide.input_size, images_at=imgs)
    t_sc = abs(score.item() - float(s_ref)) / abs(float(s_ref))
    g0 = gz0.cpu()
    ge_h, gb_h = (g0 * z0).sum((2, 3), keepdim=True), g0.sum((2, 3), keepdim=True)
    print("phi %.1f: direct score rel %.2e, g_z rel %.4f, x0 rel %.4f | transform score rel %.2e, (ge, gb) rel %.4f %.4f, latents rel %.4f"
          % (phi, d_sc, d_g, rel(x0, rx0), t_sc, rel(ge_h, ge), rel(gb_h, gb), rel(z, z_ref)))
    assert d_sc < 0.005 and t_sc < 0.005
    assert rel(x0, rx0) < 0.03
    assert d_g < 0.05
    assert rel(ge_h, ge) < 0.05 and rel(gb_h, gb) < 0.08
    # the update rule itself on the engine's own gradient (generate_data.py:696, :721-728), then against the oracle's latents
    a = ARGS
    e2 = fx["e"] - a["rho"] * ge_h
    b2 = fx["b"] - a["rho"] * gb_h
    new = z0 * (1 + e2) + b2
    lo, hi = z0 - a["constraint_value"], z0 + a["constraint_value"]
    new = torch.where(new < lo, lo, new)
    new = torch.where(new > hi, hi, new)
    assert (z.cpu() - new).abs().max().item() < 2e-4
    assert rel(z, z_ref) < 0.07


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_step_vjp_through_the_unet(setup, fx, phi):
    """Random cotangents on (x0, z') through the new backward kernels (op level, on the engine's own UNet output) and the engine's UNet
    VJP, against autograd of the oracle's denoise_one_step."""
    cfg, eng, _, O = setup
    models, ts = schedule(setup, phi)
    unet, vae, guide, sched = models
    Lb = eng.L
    B, Cc, Ls = 2, 4, cfg.latent_size
    HW = Ls * Ls
    g = torch.Generator().manual_seed(5)
    gx0, gzp = torch.randn(B, Cc, Ls, Ls, generator=g), torch.randn(B, Cc, Ls, Ls, generator=g)
    z0 = fx["z"]
    emb = torch.cat([fx["negative"], fx["prompt"]])
    zr = z0.clone().requires_grad_(True)
    with R.oracle_guidance_rescale(phi):
        rzp, rx0 = O.denoise_one_step(O.SamplerArgs(**ARGS), zr, sched, ts[FIRST], unet, emb)
    (g_ref,) = torch.autograd.grad([rx0, rzp], zr, [gx0, gzp])
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    t = ts[FIRST]
    a, ap = float(sched.alphas_cumprod[t]), float(sched.alphas_cumprod[t - 1000 // N_STEPS])
    coef = torch.tensor([ARGS["guidance_scale"], a ** 0.5, (1 - a) ** 0.5, ap ** 0.5, (1 - ap) ** 0.5]).cuda()
    out = (C.c_float * 4)()
    assert Lb.dd_op_step_coefs(1, a, ap, out) == 0
    lin = torch.tensor(list(out)).cuda()
    m2 = eng.unet_forward(z0, FIRST)                                             # [2B, 4, L, L] fp32, the engine's own model output
    rows = torch.zeros(2 * B * HW, 8, device="cuda")
    rows[:, :Cc] = m2.permute(0, 2, 3, 1).reshape(-1, Cc)
    stats = torch.zeros(B, 8, device="cuda")
    part = torch.zeros(int(Lb.dd_op_sampler_step_scratch_floats(B, HW)), device="cuda")
    d_z, d_gx0, d_gzp = z0.cuda(), gx0.cuda(), gzp.cuda()
    zp, x0 = torch.empty_like(d_z), torch.empty_like(d_z)
    assert Lb.dd_op_sampler_step(P(rows), 8, P(d_z), P(zp), P(x0), B, Cc, HW, P(coef), P(lin), 1, phi, P(stats), P(part), None) == 0
    g_m2 = torch.zeros(2 * B * HW, 8, device="cuda", dtype=torch.bfloat16)
    g_z = torch.empty_like(d_z)
    assert Lb.dd_op_sampler_step_bwd(P(d_gx0), P(d_gzp), P(g_m2), 8, P(g_z), B, Cc, HW, P(coef), P(lin), 1, phi, P(rows), P(stats), P(part), None) == 0
    torch.cuda.synchronize()
    assert rel(x0, rx0) < 0.03 and rel(zp, rzp) < 0.03
    g_eps2 = g_m2.float()[:, :Cc].reshape(2 * B, Ls, Ls, Cc).permute(0, 3, 1, 2).contiguous()
    got = g_z + eng.unet_vjp(z0, FIRST, g_eps2)
    print("phi %.1f: step + UNet VJP with random cotangents, rel %.4f" % (phi, rel(got, g_ref)))
    assert rel(got, g_ref) < 0.05


def _expand(eng, fx, gt, **kw):
    return eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], 5, gt, FIRST, 2, **kw)


def test_expand_is_the_step_by_step_calls_bitwise(setup, fx):
    """dd_expand under v-prediction + trailing + phi = 0.7 against the same loop through the step-level ABI."""
    cfg, eng, _, O = setup
    schedule(setup, 0.7, spacing="trailing")
    z, img, score = _expand(eng, fx, "transform_guidance")
    zc = eng.add_noise(fx["lat"], fx["noise"], 5)
    for i in range(5, N_STEPS):
        if i == FIRST:
            zc, sc, _ = eng.transform_guidance(zc, fx["targets"], fx["e"], fx["b"], FIRST, 2)
        zc, _ = eng.denoise_step(zc, i)
    assert torch.isfinite(z).all() and torch.equal(zc, z), "dd_expand and the step-by-step ABI calls differ"
    assert torch.equal(eng.decode(zc), img) and torch.equal(sc, score)
    z2, img2, _ = _expand(eng, fx, "transform_guidance")
    assert torch.equal(z, z2) and torch.equal(img, img2)                      # deterministic with the rescale reductions in
    schedule(setup, 0.0, spacing="trailing")
    assert not torch.equal(_expand(eng, fx, "transform_guidance")[0], z)        # and phi does something


def test_default_arguments_are_the_old_call_bitwise(setup, fx):
    """set_schedule without the new arguments == with them at their defaults, and both run the cfg_ddim kernels (epsilon)."""
    cfg, eng, _, O = setup
    schedule(setup, pred="epsilon", plain_call=True)
    want = _expand(eng, fx, "transform_guidance")
    schedule(setup, 0.0, pred="epsilon")
    got = _expand(eng, fx, "transform_guidance")
    for w_, g_ in zip(want, got):
        assert torch.isfinite(g_).all() and torch.equal(w_, g_)
    schedule(setup, 0.0)                                                       # v-prediction reads the same UNet output differently
    assert not torch.equal(_expand(eng, fx, "transform_guidance")[0], want[0])


def test_unbuilt_sampler_settings_are_refused(setup, fx):
    from distdiff_amd.scheduler import DDIMSchedule
    import dataclasses
    cfg, eng, _, O = setup
    sc = dataclasses.replace(cfg.scheduler, timestep_spacing="trailing", rescale_betas_zero_snr=True)
    sched = DDIMSchedule(sc)
    ts = sched.set_timesteps(N_STEPS)
    for phi in (0.0, 0.5):                                                     # epsilon at alphas_cumprod = 0: x0 is undefined
        with pytest.raises(RuntimeError, match="zero terminal SNR"):
            eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, prediction_type="epsilon", guidance_rescale=phi)
    with pytest.raises(RuntimeError, match="guidance_rescale"):
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, prediction_type="v_prediction", guidance_rescale=1.5)
    schedule(setup)                                                            # a refusal leaves the engine usable
    assert torch.isfinite(eng.denoise_step(fx["z"], 0)[0]).all()


@pytest.mark.parametrize("gt", [None, "transform_guidance"])
def test_text_to_img_zero_snr_vs_oracle(setup, fx, gt):
    """The whole 10-step schedule from pure noise: text_to_img, trailing, zero terminal SNR (alphas_cumprod = 0 at the first step),
    v-prediction, phi = 0.7, engine against the fp32 oracle.  Measured on an MI355X (latents rel L2 / image max abs / score rel):
    0.0134 / 0.0245 / - without guidance, 0.0168 / 0.0303 / 0.00014 with transform guidance; T2I_BOUNDS are 1.5 x that."""
    cfg, eng, _, O = setup
    phi = 0.7
    models, ts = schedule(setup, phi, spacing="trailing", zero_snr=True)
    unet, vae, guide, sched = models
    assert ts[0] == 999 and float(sched.alphas_cumprod[999]) == 0.0
    args = O.SamplerArgs(**{**ARGS, "guidance_type": gt})
    emb = torch.cat([fx["negative"], fx["prompt"]])
    z, img, score = eng.expand(None, fx["noise"], fx["e"], fx["b"], fx["targets"], 0, gt, FIRST, 2, text_to_img=True)
    gts = ts[FIRST:FIRST + 2] if gt else []
    zr, sr = fx["noise"].clone(), None
    with R.oracle_guidance_rescale(phi):
        for t in ts:
            if gts and t == gts[0]:
                zr, sr, _ = O.transform_guidance(args, zr, fx["targets"], gts, sched, unet, emb, vae, guide, fx["e"], fx["b"], fx["Pc"], fx["Pg"],
                                                 cfg.guide.input_size)
            with torch.no_grad():
                zr, _ = O.denoise_one_step(args, zr, sched, t, unet, emb)
    with torch.no_grad():
        imr = (vae.decode(zr / vae.config.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    lat_err = float((z.cpu() - zr).norm() / zr.norm())
    img_err = float((img.cpu() - imr).abs().max())
    sc_err = abs(score.item() - float(sr)) / abs(float(sr)) if gt else None
    print("text_to_img zero-SNR v-prediction %s: latents rel %.4f, image max abs %.4f, score rel %s"
          % (gt, lat_err, img_err, "%.5f" % sc_err if gt else "-"))
    assert torch.isfinite(z).all() and torch.isfinite(img).all()
    bl, bi, bs = T2I_BOUNDS[gt]
    assert bl <= T2I_CAPS[0] and bi <= T2I_CAPS[1] and (bs is None or bs <= T2I_CAPS[2])
    assert lat_err < bl and img_err < bi
    if gt:
        assert sc_err < bs
