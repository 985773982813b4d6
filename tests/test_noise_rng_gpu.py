"""GPU checks of the counter-based device noise (rng.hip through dd_randn_units / dd_expand's noise_mode 1) and of text-to-image:
the kernel against the Philox / Box-Muller restatement that tests/test_noise_rng.py pins to the Random123 known answers, position
independence, moments, generated == explicit (bitwise), text-to-image against the fp32 oracle, and the CLI.

Text-to-image parity (test_text_to_img_vs_oracle): the whole 10-step schedule of the tiny configuration from pure noise, engine (bf16
UNet / VAE) against the fp32 oracle composed from the oracle's own functions.  Measured on an MI355X: latents within 1.49 % / 1.52 %
(guidance off / transform guidance), image max abs error 0.037 / 0.036, score within 0.086 %; the error does not grow over the steps
(1.62 % after the first, 1.49 % after the tenth).  The bounds below are 1.5 x those figures and stay under twice
the bounds of the half-schedule loop test (test_engine_gpu.py::test_expand_loop_vs_golden: 3 % latents, 0.08 image, 0.5 % score)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_noise_rng as R  # noqa: E402  (the restatement and its known-answer tests)

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(__file__), "golden", "tiny_fixture.pt")

SEEDS = [0, 42, (1 << 40) + 12345]
UNITS = [0, 7, (3 << 32) | 2, (1 << 63) + 5]
TOL = 2e-5          # absolute, on values up to |6.8|: about 40 fp32 ulp at the extreme (log, sqrt and the angle reduction cost a few each)

# text-to-image vs the fp32 oracle: 1.5 x measured, capped at twice the half-schedule loop bounds
T2I_CAPS = (0.06, 0.16, 0.01)
# measured (latents rel L2, image max abs, score rel): guidance off 0.0149 / 0.0374 / -; transform guidance 0.0152 / 0.0360 / 0.00086
T2I_BOUNDS = {None: (0.0224, 0.0561, None), "transform_guidance": (0.0228, 0.0540, 0.0013)}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIX, weights_only=False)


@pytest.fixture(scope="module")
def setup(hip_lib, fx):
    from distdiff_amd.config import tiny_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    from oracle import sd_oracle as O
    cfg = tiny_config(max_batch=2)
    w = synthetic_weights(cfg, seed=0, num_classes=5)
    eng = Engine(cfg, w, enable_grad=True, max_guidance_period=2)
    sched = DDIMSchedule(cfg.scheduler)
    ts = sched.set_timesteps(fx["n_steps"])
    a = fx["args"]
    eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=a["guidance_scale"], gs=a["gs"], ls=a["ls"],
                     rho=a["rho"], constraint_value=a["constraint_value"], guidance_period=a["guidance_period"])
    eng.set_prototypes(fx["Pc"], fx["Pg"])
    eng.set_prompt(torch.cat([fx["negative_embeds"], fx["prompt_embeds"]]).cuda())
    models = O.build_models(cfg, w)
    models[3].set_timesteps(fx["n_steps"])
    yield cfg, eng, models, O
    eng.close()


def test_randn_units_vs_restatement(setup):
    cfg, eng, _, _ = setup
    worst = {0: 0.0, 1: 0.0, 3: 0.0}
    for seed in SEEDS:
        for stream, n in ((0, 1003), (1, 1003), (2, 1003), (3, 1003), (0, 4096), (2, 4), (3, 4), (0, 1)):
            got = eng.randn_units(seed, stream, UNITS, n).cpu().numpy()
            assert got.shape == (len(UNITS), n) and got.dtype == np.float32
            for row, uid in enumerate(UNITS):
                ref = R.unit_values(seed, stream, uid, n)
                if stream == 2:
                    assert np.array_equal(got[row], ref.astype(np.float32)), (seed, uid, n)      # 24-bit integers scaled by 2^-24: exact
                    assert got[row].min() >= 0.0 and got[row].max() < 1.0
                else:
                    err = float(np.abs(got[row].astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max())
                    worst[stream] = max(worst[stream], err)
    print("randn_units vs float64 restatement, max abs error per normal stream:", worst)
    assert max(worst.values()) <= TOL, worst


def test_position_independence_bitwise(setup):
    cfg, eng, _, _ = setup
    seed, uid, n = SEEDS[2], UNITS[2], 4 * cfg.latent_size ** 2
    for stream in range(4):
        alone = eng.randn_units(seed, stream, [uid], n)
        row5 = eng.randn_units(seed, stream, [11, 12, 13, 14, 15, uid, 16, 17], n)
        row17 = eng.randn_units(seed, stream, list(range(100, 117)) + [uid, 1, 2], n)          # past the 16 ids of one launch
        again = eng.randn_units(seed, stream, [uid], n)
        assert torch.equal(alone[0], row5[5]) and torch.equal(alone[0], row17[17]) and torch.equal(alone, again)
        assert not torch.equal(alone[0], row5[4])                                                  # another unit id
        assert not torch.equal(alone, eng.randn_units(seed, stream, [uid ^ (1 << 32)], n))         # ... in the high word
        assert not torch.equal(alone, eng.randn_units(seed + 1, stream, [uid], n))                 # another seed
        assert not torch.equal(alone, eng.randn_units(seed ^ (1 << 40), stream, [uid], n))         # ... in the high word
        assert not torch.equal(alone, eng.randn_units(seed, (stream + 1) % 4, [uid], n))           # another stream


def test_moments_of_one_call(setup):
    cfg, eng, _, _ = setup
    N = R.MOMENT_N
    x = eng.randn_units(R.MOMENT_SEED, 0, [5], N).cpu().numpy()[0]
    assert np.isfinite(x).all()
    m, v, k = R.moments(x)
    bm, bv, bk = R.moment_bounds(N)
    ref = R.unit_values(R.MOMENT_SEED, 0, 5, N)
    err = np.abs(x.astype(np.float64) - ref)
    print("moments of %d normals: mean %.3e (bound %.3e), var-1 %.3e (%.3e), kurt-3 %.3e (%.3e); max |x| %.3f; vs restatement: max abs "
          "err %.3e at |ref| = %.3f" % (N, m, bm, v - 1, bv, k - 3, bk, np.abs(x).max(), err.max(), abs(ref[err.argmax()])))
    assert abs(m) <= bm and abs(v - 1) <= bv and abs(k - 3) <= bk
    assert err.max() <= TOL + 2.0 ** -24 * np.abs(ref).max()          # the same 2e-5 over 4 M values (+ the fp32 rounding of the result itself)
    e = eng.randn_units(R.MOMENT_SEED, 2, [5], 1 << 16).cpu().numpy()
    assert e.min() >= 0.0 and e.max() < 1.0 and abs(e.mean() - 0.5) <= 5 / np.sqrt(12.0 * e.size)


@pytest.mark.parametrize("gt", [None, "transform_guidance", "direct_guidance"])
def test_generated_equals_explicit_bitwise(setup, fx, gt):
    """expand(seed, unit_ids) == expand(noise, e, b) given the generator's own outputs as explicit tensors: the fused first op writes
    the bits of add_noise's kernel on the materialised noise, and e / b are used where the caller's are."""
    cfg, eng, _, _ = setup
    L, seed, ids = cfg.latent_size, SEEDS[2], [UNITS[2], UNITS[3]]
    first = fx["timesteps"].tolist().index(fx["guide_timesteps"][0])
    n0 = eng.randn_units(seed, 0, ids, 4 * L * L).view(2, 4, L, L)
    off = eng.randn_units(seed, 1, ids, 4).view(2, 4, 1, 1)
    e, b = eng.randn_units(seed, 2, ids, 4), eng.randn_units(seed, 3, ids, 4)
    for offset_noise in (False, True):
        noise = n0 + 0.1 * off if offset_noise else n0
        want = eng.expand(fx["lat"], noise, e, b, fx["targets"], fx["start_index"], gt, first, 2)
        got = eng.expand(fx["lat"], None, None, None, fx["targets"], fx["start_index"], gt, first, 2, seed=seed, unit_ids=ids,
                         offset_noise=offset_noise)
        for w_, g_ in zip(want, got):
            assert torch.isfinite(g_).all() and torch.equal(w_, g_), (gt, offset_noise)
    # text-to-image: the noise itself is the first latent, generated or passed
    want = eng.expand(None, n0, e, b, fx["targets"], 0, gt, first, 2, text_to_img=True)
    got = eng.expand(None, None, None, None, fx["targets"], 0, gt, first, 2, seed=seed, unit_ids=ids, offset_noise=True, text_to_img=True)
    for w_, g_ in zip(want, got):
        assert torch.isfinite(g_).all() and torch.equal(w_, g_), gt
    assert not torch.equal(want[0], eng.expand(fx["lat"], n0, e, b, fx["targets"], 0, gt, first, 2)[0])


def _oracle_text_to_img(O, cfg, models, fx, gt, noise, e, b):
    """The reference's text-to-image branch as it is meant (generate_data.py:1150-1158, 1199-1228), from the oracle's own functions:
    z = noise * init_noise_sigma (1), every timestep, guidance at the window."""
    unet, vae, guide, sched = models
    args = O.SamplerArgs(**{**fx["args"], "guidance_type": gt})
    ts = [int(t) for t in sched.set_timesteps(fx["n_steps"])]
    gts = O.guide_timesteps(ts, args.guidance_step, args.guidance_period) if gt else []
    emb = torch.cat([fx["negative_embeds"], fx["prompt_embeds"]])
    z, score, trail = noise.clone(), None, []
    for t in ts:
        if gts and t == gts[0] and gt == "transform_guidance":
            z, score, _ = O.transform_guidance(args, z, fx["targets"], gts, sched, unet, emb, vae, guide, e, b, fx["Pc"], fx["Pg"],
                                               cfg.guide.input_size)
        with torch.no_grad():
            z, _ = O.denoise_one_step(args, z, sched, t, unet, emb)
        trail.append(z.clone())
    with torch.no_grad():
        img = (vae.decode(z / vae.config.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    return z, img, score, trail


@pytest.mark.parametrize("gt", [None, "transform_guidance"])
def test_text_to_img_vs_oracle(setup, fx, gt):
    cfg, eng, models, O = setup
    L, seed, ids = cfg.latent_size, SEEDS[1], [UNITS[1], UNITS[2]]
    first = fx["timesteps"].tolist().index(fx["guide_timesteps"][0])
    noise = eng.randn_units(seed, 0, ids, 4 * L * L).view(2, 4, L, L).cpu()
    e = eng.randn_units(seed, 2, ids, 4).view(2, 4, 1, 1).cpu()
    b = eng.randn_units(seed, 3, ids, 4).view(2, 4, 1, 1).cpu()
    z, img, score = eng.expand(None, None, None, None, fx["targets"], 0, gt, first, 2, seed=seed, unit_ids=ids, text_to_img=True)
    zr, imr, sr, trail = _oracle_text_to_img(O, cfg, models, fx, gt, noise, e, b)
    # per-step error growth of the plain schedule (the step-level ABI from the same noise)
    growth = []
    if gt is None:
        cur = noise.cuda()
        for i in range(fx["n_steps"]):
            cur, _ = eng.denoise_step(cur, i)
            growth.append(float((cur.cpu() - trail[i]).norm() / trail[i].norm()))
        assert torch.equal(cur, z)
    lat_err = float((z.cpu() - zr).norm() / zr.norm())
    img_err = float((img.cpu() - imr).abs().max())
    sc_err = abs(score.item() - float(sr)) / abs(float(sr)) if gt else None
    print("text_to_img %s: latents rel %.4f, image max abs %.4f, score rel %s; per-step latent error %s"
          % (gt, lat_err, img_err, "%.5f" % sc_err if gt else "-", " ".join("%.4f" % g for g in growth)))
    bl, bi, bs = T2I_BOUNDS[gt]
    assert bl <= T2I_CAPS[0] and bi <= T2I_CAPS[1] and (bs is None or bs <= T2I_CAPS[2])
    assert lat_err < bl and img_err < bi
    if gt:
        assert sc_err < bs


def test_text_to_img_needs_start_index_zero(setup, fx):
    cfg, eng, _, _ = setup
    with pytest.raises(RuntimeError, match=r"dd_expand failed \(-1\)"):          # DD_ERR_ARG
        eng.expand(None, None, None, None, fx["targets"], 3, None, 0, 0, seed=1, unit_ids=[1, 2], text_to_img=True)
    with pytest.raises(RuntimeError, match=r"dd_expand failed \(-1\)"):          # latents are needed without text_to_img
        eng.expand(None, None, None, None, fx["targets"], 3, None, 0, 0, seed=1, unit_ids=[1, 2])


def test_cli_text_to_img_philox(hip_lib, tmp_path):
    """--text_to_img --noise_rng philox with transform guidance writes its PNGs; a second run with another --engine_batch gets the same
    engine inputs (tests/test_noise_rng.py) -- the PNGs are only compared and reported: the GEMM tiling depends on the batch."""
    from PIL import Image
    from distdiff_amd import generate_data as G
    outs = []
    for eb in (4, 8):
        out = str(tmp_path / ("eb%d" % eb))
        argv = ["--synthetic", "8", "--tiny", "--synthetic_classes", "2", "--output_dir", out, "--train_batch_size", "1", "--engine_batch", str(eb),
                "--steps", "10", "--total_split", "1", "--split", "0", "--num_images_per_prompt", "1", "--guidance_type", "transform_guidance",
                "--guidance_step", "4", "--guidance_period", "2", "--constraint_value", "0.2", "--optimize_targets",
                "global_prototype-local_prototype", "--K", "3", "--text_to_img", "--noise_rng", "philox", "--seed", "7"]
        assert G.main(argv) == 0
        files = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs)
        assert len(files) == 8 and all(f.endswith("_expand_0.png") for f in files)
        outs.append([np.asarray(Image.open(f)).astype(np.int32) for f in files])
        assert all(im.shape == (128, 128, 3) and im.std() > 0 for im in outs[-1])
    diff = [int(np.abs(a - b).max()) for a, b in zip(*outs)]
    print("text_to_img philox PNGs, --engine_batch 4 vs 8: max abs difference per image (of 255):", diff)
