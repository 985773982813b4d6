"""A bf16 and an fp16 engine (Engine(act_dtype=...): libdistdiff_hip.so / libdistdiff_hip_f16.so) side by side in one process, tiny config,
B = 2, the inputs of smoke(), against the fp32 oracle on the CPU.

Forward (dd_unet_forward, dd_denoise_step, dd_decode, dd_vae_encode, dd_text_encode, the ViT dd_guide_encode), rel-L2 against the fp32 oracle:
the yardstick is the ORACLE ITSELF run with its weights and inputs rounded to fp16 (every activation is then fp16 too), as
tests/test_oracle.py::test_reduced_precision_floor_of_the_oracle_loop does.  The fp16 engine must be within 2 x that floor -- it
accumulates in fp32 and should sit below it; the factor covers summation order -- and below half the bf16 engine's error on the same inputs.
VJPs (dd_unet_vjp, dd_decode_vjp, random cotangents) against oracle autograd: the bounds of tests/test_engine_gpu.py (5 % / 3 %), below the
bf16 engine's error, and the promise of the power-of-two cotangent normalisation: the result for the cotangent x 2^-20 and x 2^10 is
2^-20 / 2^10 times the result for the cotangent, bitwise; a cotangent of zeros gives zeros.
Guided loop (transform guidance P = 2, direct guidance): the bounds of smoke(), everything finite.  Not "better than bf16": the guided loop
re-draws the guide's masks.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
B = 2
N_STEPS = 10
VIT = dict(kind="vit", input_size=64, vit_width=64, vit_layers=2, vit_heads=2, vit_patch=16, vit_mlp=128, vit_out=32)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.isfinite(a).all()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def half_weights(w):
    return {k: {n: (t.half() if t.is_floating_point() else t) for n, t in v.items()} for k, v in w.items()}


@pytest.fixture(scope="module")
def S(hip_lib):
    """inputs, both engines, the fp32 oracle's outputs and the fp16-rounded oracle's distance from them, computed once"""
    from types import SimpleNamespace
    from distdiff_amd.config import GuideConfig, tiny_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    from oracle import sd_oracle as O
    s = SimpleNamespace(O=O)
    cfg = s.cfg = tiny_config(max_batch=B)
    w = s.w = synthetic_weights(cfg, seed=0, num_classes=5, encoders=True)
    g = torch.Generator().manual_seed(1)                       # smoke()'s draws, in its order
    L, D = cfg.latent_size, cfg.guide.feature_dim
    s.lat = torch.randn(B, 4, L, L, generator=g) * 0.9
    s.noise = torch.randn(B, 4, L, L, generator=g)
    s.e, s.b = torch.rand(B, 4, 1, 1, generator=g), torch.randn(B, 4, 1, 1, generator=g)
    s.pe = torch.randn(B, cfg.text_len, cfg.unet.cross_attention_dim, generator=g)
    s.ne = torch.randn(1, cfg.text_len, cfg.unet.cross_attention_dim, generator=g).expand(B, -1, -1)
    s.Pc = F.normalize(torch.randn(5, D, generator=g), dim=-1)
    s.Pg = F.normalize(torch.randn(5, 3, D, generator=g), dim=-1)
    s.tg = torch.tensor([1, 3])
    s.emb = torch.cat([s.ne, s.pe])
    s.images = torch.rand(B, 3, 8 * L, 8 * L, generator=g) * 2 - 1
    s.ids = torch.randint(0, cfg.text.vocab_size, (2 * B, cfg.text_len), generator=g).int()
    s.gg = torch.randn(2 * B, 4, L, L, generator=g)
    s.gim = torch.randn(B, 3, 8 * L, 8 * L, generator=g)
    sched = DDIMSchedule(cfg.scheduler)
    s.ts = sched.set_timesteps(N_STEPS)
    s.step = 5
    s.z = s.lat * 0.7 + s.noise * 0.7

    def engine(c, ww, dt, grad=True):
        eng = Engine(c, ww, enable_grad=grad, max_guidance_period=2, act_dtype=dt)
        eng.set_schedule(s.ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_period=2)
        return eng
    s.eng = {dt: engine(cfg, w, dt) for dt in ("bf16", "fp16")}
    for eng in s.eng.values():
        eng.set_prototypes(s.Pc, s.Pg)
        eng.set_prompt(s.emb.cuda())
    # the ViT guide: its own pair of engines (the guide of the tiny config is the fp32 ResNet, which has no 16-bit activations)
    from copy import deepcopy
    vcfg = s.vcfg = deepcopy(cfg)
    vcfg.guide = GuideConfig(**VIT)
    vw = s.vw = synthetic_weights(vcfg, seed=0, num_classes=5)
    s.veng = {dt: engine(vcfg, vw, dt, grad=False) for dt in ("bf16", "fp16")}
    s.gimg = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1

    def oracle(ww, vww, cast):
        unet, vae, guide, osched = O.build_models(cfg, ww)
        osched.set_timesteps(N_STEPS)
        t = s.ts[s.step]
        with torch.no_grad():
            eps2 = unet(cast(torch.cat([s.z, s.z])), t, cast(s.emb))[0]
            zp, x0 = O.denoise_one_step(O.SamplerArgs(), cast(s.z), osched, t, unet, cast(s.emb))
            img = vae.decode(cast(s.z) / cfg.vae.scaling_factor)[0]
            lat, mom = O.vae_encode(cfg, ww["vae"], cast(s.images), None)
            # the oracle builds its causal mask in the default dtype, which would promote the scores of the rounded run to fp32
            torch.set_default_dtype(cast(torch.zeros(1)).dtype)
            try:
                txt = O.clip_text_encode(cfg, ww["text"], s.ids)
            finally:
                torch.set_default_dtype(torch.float32)
            vit = O.GuideOracleViT(vcfg, vww["guide"]).encode_image(cast(s.gimg))
        return dict(unet=eps2.float(), z_prev=zp.float(), x0=x0.float(), decode=img.float(), vae_encode=mom.float(), text=txt.float(), vit=vit.float())
    s.ref = oracle(w, vw, lambda t: t)
    h = oracle(half_weights(w), half_weights(vw), lambda t: t.half())
    s.floor = {k: rel(h[k], s.ref[k]) for k in s.ref}
    s.models = O.build_models(cfg, w)
    yield s
    for eng in list(s.eng.values()) + list(s.veng.values()):
        eng.close()


def _forward(s, dt):
    eng, veng = s.eng[dt], s.veng[dt]
    zp, x0 = eng.denoise_step(s.z, s.step)
    _lat, mom = eng.vae_encode(s.images, None, return_moments=True)
    return dict(unet=eng.unet_forward(s.z, s.step), z_prev=zp, x0=x0, decode=eng.decode(s.z, denormalize=False), vae_encode=mom,
                text=eng.text_encode(s.ids), vit=veng.guide_encode(s.gimg))


def test_two_libraries_in_one_process(S):
    assert S.eng["bf16"].L is not S.eng["fp16"].L
    assert S.eng["bf16"].L.dd_act_dtype() == 0 and S.eng["fp16"].L.dd_act_dtype() == 1
    assert S.eng["fp16"].act_dtype == "fp16"


@pytest.mark.parametrize("what", ["unet", "z_prev", "x0", "decode", "vae_encode", "text", "vit"])
def test_forward_against_the_fp16_floor_of_the_oracle(S, what):
    if not hasattr(S, "fwd"):
        S.fwd = {dt: _forward(S, dt) for dt in ("bf16", "fp16")}
    e16, ebf, floor = rel(S.fwd["fp16"][what], S.ref[what]), rel(S.fwd["bf16"][what], S.ref[what]), S.floor[what]
    print("%s: fp16 engine %.3e, bf16 engine %.3e, all-fp16 oracle %.3e (vs the fp32 oracle)" % (what, e16, ebf, floor))
    assert e16 <= 2.0 * floor
    assert e16 < 0.5 * ebf


def _vjp_refs(S):
    if hasattr(S, "vjp_ref"):
        return S.vjp_ref
    unet, vae, _guide, _sched = S.models
    zr = S.z.clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(unet(torch.cat([zr, zr]), S.ts[S.step], S.emb)[0], zr, S.gg)
    xr = S.z.clone().requires_grad_(True)
    (gv,) = torch.autograd.grad(vae.decode(xr / S.cfg.vae.scaling_factor)[0], xr, S.gim)
    S.vjp_ref = (gz, gv)
    return S.vjp_ref


def test_vjps_against_autograd(S):
    gz, gv = _vjp_refs(S)
    eu = {dt: rel(S.eng[dt].unet_vjp(S.z, S.step, S.gg), gz) for dt in ("bf16", "fp16")}
    ev = {dt: rel(S.eng[dt].decode_vjp(S.z, S.gim), gv) for dt in ("bf16", "fp16")}
    print("unet_vjp: fp16 %.3e bf16 %.3e; decode_vjp: fp16 %.3e bf16 %.3e" % (eu["fp16"], eu["bf16"], ev["fp16"], ev["bf16"]))
    assert eu["fp16"] < 0.05 and ev["fp16"] < 0.03
    assert eu["fp16"] < eu["bf16"] and ev["fp16"] < ev["bf16"]


@pytest.mark.parametrize("k", [-20, 10])
def test_vjp_scale_invariance_is_bitwise(S, k):
    eng = S.eng["fp16"]
    f = 2.0 ** k
    a = eng.unet_vjp(S.z, S.step, S.gg)
    assert torch.equal(eng.unet_vjp(S.z, S.step, S.gg * f), a * f)
    c = eng.decode_vjp(S.z, S.gim)
    assert torch.equal(eng.decode_vjp(S.z, S.gim * f), c * f)
    assert float(a.abs().max()) > 0 and float(c.abs().max()) > 0


def test_zero_cotangent_gives_zeros(S):
    eng = S.eng["fp16"]
    a = eng.unet_vjp(S.z, S.step, torch.zeros_like(S.gg))
    c = eng.decode_vjp(S.z, torch.zeros_like(S.gim))
    assert torch.count_nonzero(a).item() == 0 and torch.count_nonzero(c).item() == 0


@pytest.mark.parametrize("gt", ["transform_guidance", "direct_guidance"])
def test_guided_loop_meets_the_bounds_of_smoke(S, gt):
    from distdiff_amd.scheduler import guide_window, start_index
    O, cfg = S.O, S.cfg
    eng = S.eng["fp16"]
    first, cnt = guide_window(N_STEPS, 4, 2)
    z, img, score = eng.expand(S.lat, S.noise, S.e, S.b, S.tg, start_index(0.5, N_STEPS), gt, first, cnt)
    torch.cuda.synchronize()
    args = O.SamplerArgs(guidance_type=gt, num_inference_steps=N_STEPS, guidance_step=4, guidance_period=2, strength=0.5)
    zr, imr, sr = O.expand_one(args, cfg, O.build_models(cfg, S.w), S.lat, S.noise, S.e, S.b, S.pe, S.ne, S.tg, S.Pc, S.Pg)
    assert torch.isfinite(z).all() and torch.isfinite(img).all() and torch.isfinite(score).all()
    r, ir = rel(z, zr), (img.cpu() - imr).abs().max().item()
    print("%s: latents %.4f, image max abs %.4f, score %.5f (oracle %.5f)" % (gt, r, ir, score.item(), float(sr)))
    assert r < 0.035 and ir < 0.08 and abs(score.item() - float(sr)) < 0.005 * abs(float(sr))


def test_fp16_engine_refuses_fp8_attention(S):
    from distdiff_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine(S.cfg, S.w, act_dtype="fp16", attn_fp8=True)
