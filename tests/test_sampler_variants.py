"""CPU checks of the sampler variants (no GPU call): timestep tables and the zero-terminal-SNR table against known answers computed
from the diffusers 0.28 formulas, config.from_model_dir(sampler_variants=True), the SD-2.x configs, the host-side step coefficients of
the library, the CLI plumbing, and the float64 step restatement of tests/sampler_variants_ref.py from first principles."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import sampler_variants_ref as R
from distdiff_amd import generate_data as G
from distdiff_amd.config import SchedulerConfig, from_model_dir, sd21_config, tiny_config, tiny_sd2_config
from distdiff_amd.scheduler import DDIMSchedule
from distdiff_amd.weights import synthetic_weights
from test_checkpoints import write_model_dir


@pytest.mark.parametrize("spacing,n,head,tail", [
    ("trailing", 50, [999, 979, 959, 939], [59, 39, 19]),
    ("trailing", 30, [999, 966, 932, 899], [99, 66, 32]),
    ("linspace", 50, [999, 979, 958, 938], [41, 20, 0]),
    ("linspace", 30, [999, 965, 930, 896], [69, 34, 0]),
    ("leading", 50, [981, 961, 941, 921], [41, 21, 1]),
])
def test_timestep_known_answers(spacing, n, head, tail):
    ts = DDIMSchedule(SchedulerConfig(timestep_spacing=spacing)).set_timesteps(n)
    assert len(ts) == n and ts[:4] == head and ts[-3:] == tail
    assert all(isinstance(t, int) and 0 <= t < 1000 for t in ts) and ts == sorted(ts, reverse=True)
    # the test-side scheduler (the GPU tests' reference) agrees
    assert R.VariantScheduler(SchedulerConfig(timestep_spacing=spacing)).set_timesteps(n).tolist() == ts


def test_unknown_spacing_is_refused():
    with pytest.raises(NotImplementedError, match="timestep_spacing"):
        DDIMSchedule(SchedulerConfig(timestep_spacing="karras")).set_timesteps(10)


def test_zero_terminal_snr_table():
    plain = DDIMSchedule(SchedulerConfig()).alphas_cumprod
    ac = DDIMSchedule(SchedulerConfig(rescale_betas_zero_snr=True)).alphas_cumprod
    assert ac.dtype == np.float32 and ac.shape == (1000,)
    assert abs(float(ac[0]) - 0.99914998) <= 1e-6 * 0.99914998 and abs(float(ac[0]) - float(plain[0])) <= 1e-6
    assert float(ac[-1]) == 0.0
    assert abs(float(ac[-2]) - 1.968e-7) <= 1e-3 * 1.968e-7, float(ac[-2])
    assert (np.diff(ac) <= 0).all()
    assert float(plain[-1]) > 0                                      # the plain table never reaches zero SNR
    assert torch.equal(R.VariantScheduler(SchedulerConfig(rescale_betas_zero_snr=True)).alphas_cumprod, torch.from_numpy(ac))


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_step_restatement_from_first_principles(pred):
    """Any (x0, eps) at noise level a gives z = sqrt(a) x0 + sqrt(1-a) eps; the model output that encodes it under each prediction
    type must give back x0 and z' = sqrt(a') x0 + sqrt(1-a') eps."""
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 4, 5, 5, generator=g, dtype=torch.float64)
    eps = torch.randn(2, 4, 5, 5, generator=g, dtype=torch.float64)
    for a, ap in ((0.3, 0.45), (0.9, 0.999), (0.02, 0.05)):
        sa, sb = a ** 0.5, (1 - a) ** 0.5
        z = sa * x0 + sb * eps
        m = {"epsilon": eps, "v_prediction": sa * eps - sb * x0, "sample": x0}[pred]
        gx0, gzp = R.step_ref(pred, a, ap, z, m)
        assert (gx0 - x0).abs().max() < 1e-12
        assert (gzp - (ap ** 0.5 * x0 + (1 - ap) ** 0.5 * eps)).abs().max() < 1e-12
    # v-prediction never divides: a = 0 (first trailing step of a zero-SNR table) gives x0 = -m
    z = torch.randn(2, 4, 5, 5, generator=g, dtype=torch.float64)
    gx0, gzp = R.step_ref("v_prediction", 0.0, 0.01, z, eps)
    assert torch.isfinite(gx0).all() and torch.isfinite(gzp).all() and torch.equal(gx0, -eps)


def test_library_step_coefficients_match_the_restatement(tmp_path):
    """dd_op_step_coefs (host code of the library, what dd_set_schedule fills its table with): x0 = A_z z + A_m m, z' = B_z z + B_m m."""
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    L = _lib.lib()
    out = (C.c_float * 4)()
    z, m = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([0.0, 1.0], dtype=torch.float64)
    for pred, code in R.PRED.items():
        for a, ap in ((0.3, 0.45), (0.9, 0.999), (1.968e-7, 0.0047), (0.0, 0.0047)):
            if a == 0.0 and pred == "epsilon":
                assert L.dd_op_step_coefs(code, a, ap, out) == -1                  # x0 is undefined there: refused
                continue
            assert L.dd_op_step_coefs(code, a, ap, out) == 0
            x0, zp = R.step_ref(pred, a, ap, z, m)
            ref = [float(x0[0]), float(x0[1]), float(zp[0]), float(zp[1])]
            for got, want in zip(list(out), ref):
                assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (pred, a, ap, list(out), ref)
    assert L.dd_op_step_coefs(3, 0.5, 0.6, out) == -1 and L.dd_op_step_coefs(2, 1.0, 1.0, out) == -1


def test_sd2_configs():
    c = sd21_config()
    assert c.latent_size == 96 and c.unet.block_out_channels == (320, 640, 1280, 1280) and c.unet.level_heads == (5, 10, 20, 20)
    assert all(w // h == 64 for w, h in zip(c.unet.block_out_channels, c.unet.level_heads))
    assert c.unet.cross_attention_dim == 1024 and c.unet.use_linear_projection
    t = c.text
    assert (t.hidden_size, t.intermediate_size, t.num_hidden_layers, t.num_attention_heads, t.hidden_act) == (1024, 4096, 23, 16, "gelu")
    assert c.text_hidden_layer == 0 and c.text2 is None and c.scheduler.prediction_type == "v_prediction"
    assert sd21_config(64, 2, v_prediction=False).scheduler.prediction_type == "epsilon"
    t2 = tiny_sd2_config()
    assert t2.latent_size == 16 and t2.max_batch == 2 and t2.unet.block_out_channels == (64, 128, 128, 128)
    assert t2.unet.level_heads == (1, 2, 2, 2) and t2.unet.cross_attention_dim == 128 and t2.unet.layers_per_block == 1
    assert t2.unet.norm_num_groups == 8 and t2.unet.use_linear_projection
    assert (t2.text.hidden_size, t2.text.num_attention_heads, t2.text.num_hidden_layers, t2.text.hidden_act, t2.text_len) == (128, 2, 3, "gelu", 13)
    w = synthetic_weights(t2, seed=0, num_classes=2, encoders=True)
    assert tuple(w["unet"]["down_blocks.0.attentions.0.proj_in.weight"].shape) == (64, 64)                       # nn.Linear
    assert tuple(w["unet"]["mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight"].shape) == (128, 128)
    assert tuple(w["text"]["text_model.encoder.layers.2.mlp.fc1.weight"].shape) == (256, 128)


def _sd2_dir(tmp_path, scheduler, cfg=None):
    cfg = cfg or tiny_sd2_config()
    root = str(tmp_path / "m")
    write_model_dir(root, cfg, synthetic_weights(cfg, seed=0, num_classes=2, encoders=True), scheduler=scheduler)
    if cfg.unet.level_heads:          # the SD-2.x unet/config.json fields
        p = os.path.join(root, "unet", "config.json")
        u = json.load(open(p))
        u.update({"attention_head_dim": list(cfg.unet.level_heads), "use_linear_projection": True, "upcast_attention": True})
        json.dump(u, open(p, "w"))
    return root, cfg


def test_sd2_model_dir_round_trip(tmp_path):
    root, cfg = _sd2_dir(tmp_path, {"prediction_type": "v_prediction"})
    with pytest.raises(NotImplementedError, match="prediction_type"):
        from_model_dir(root, cfg.latent_size, 2)                     # called as before: the strict SD-1.x reader
    got = from_model_dir(root, cfg.latent_size, 2, sampler_variants=True)
    for part in ("unet", "vae", "text", "scheduler"):
        assert getattr(got, part) == getattr(cfg, part), part
    assert got.text_len == cfg.text_len and got.text2 is None and got.text_hidden_layer == 0


@pytest.mark.parametrize("sc", [{"prediction_type": "v_prediction"}, {"prediction_type": "sample"}, {"timestep_spacing": "trailing"},
                                {"timestep_spacing": "linspace"}, {"beta_schedule": "linear"},
                                {"rescale_betas_zero_snr": True, "prediction_type": "v_prediction", "timestep_spacing": "trailing"}])
def test_from_model_dir_accepts_the_variants(tmp_path, sc):
    root, cfg = _sd2_dir(tmp_path, sc, tiny_config())
    got = from_model_dir(root, sampler_variants=True).scheduler
    assert got == dataclasses.replace(SchedulerConfig(), **sc)
    with pytest.raises(NotImplementedError):
        from_model_dir(root)


@pytest.mark.parametrize("sc,key", [({"clip_sample": True}, "clip_sample"), ({"thresholding": True}, "thresholding"),
                                    ({"prediction_type": "flow"}, "prediction_type"), ({"timestep_spacing": "karras"}, "timestep_spacing"),
                                    ({"beta_schedule": "squaredcos_cap_v2"}, "beta_schedule")])
def test_from_model_dir_refuses_by_key(tmp_path, sc, key):
    root, cfg = _sd2_dir(tmp_path, sc, tiny_config())
    for kw in ({}, {"sampler_variants": True}):
        with pytest.raises(NotImplementedError, match=key):
            from_model_dir(root, **kw)


class RecordingEngine:
    """Stand-in for engine.Engine behind generate_data.build_engine: records the constructor's config and set_schedule's arguments."""
    last = None

    def __init__(self, cfg, weights, **kw):
        self.cfg, self.B, self.device, self.schedule = cfg, cfg.max_batch, torch.device("cpu"), None
        RecordingEngine.last = self

    def set_schedule(self, timesteps, alphas_cumprod, final_alpha_cumprod, **kw):
        self.schedule = (list(timesteps), np.asarray(alphas_cumprod), float(final_alpha_cumprod), kw)


def _build(monkeypatch, extra):
    from distdiff_amd import engine
    monkeypatch.setattr(engine, "Engine", RecordingEngine)
    args = G.parse_args(["--synthetic", "4", "--tiny", "--engine_batch", "2", "--steps", "10"] + extra)
    cfg, eng, sched = G.build_engine(args, device="cpu")
    return args, cfg, eng, sched


def test_cli_defaults_are_the_sd1_sampler(monkeypatch):
    a = G.parse_args([])
    assert (a.guidance_rescale, a.prediction_type, a.timestep_spacing, a.rescale_betas_zero_snr, a.synthetic_arch) == (0.0, None, None, False, "sd15")
    args, cfg, eng, sched = _build(monkeypatch, [])
    ts, ac, fa, kw = eng.schedule
    assert ts == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    assert kw["prediction_type"] == "epsilon" and kw["guidance_rescale"] == 0.0
    assert cfg.unet.cross_attention_dim == 64 and not cfg.unet.use_linear_projection


def test_cli_flags_reach_set_schedule(monkeypatch):
    args, cfg, eng, sched = _build(monkeypatch, ["--synthetic_arch", "sd21", "--guidance_rescale", "0.7", "--timestep_spacing", "trailing",
                                                 "--rescale_betas_zero_snr"])
    assert cfg.unet.level_heads == (1, 2, 2, 2) and cfg.text.hidden_act == "gelu" and cfg.max_batch == 2        # tiny_sd2_config
    ts, ac, fa, kw = eng.schedule
    assert ts == [999, 899, 799, 699, 599, 499, 399, 299, 199, 99] and sched.timesteps == ts
    assert float(ac[-1]) == 0.0 and kw["prediction_type"] == "v_prediction" and kw["guidance_rescale"] == pytest.approx(0.7)
    assert cfg.scheduler.rescale_betas_zero_snr and cfg.scheduler.timestep_spacing == "trailing"
    # --prediction_type overrides the architecture's own
    args, cfg, eng, sched = _build(monkeypatch, ["--synthetic_arch", "sd21", "--prediction_type", "epsilon", "--timestep_spacing", "linspace"])
    assert eng.schedule[3]["prediction_type"] == "epsilon" and eng.schedule[0][0] == 999 and eng.schedule[0][-1] == 0
    assert float(eng.schedule[1][-1]) > 0
    for bad in (["--guidance_rescale", "1.5"], ["--prediction_type", "flow"], ["--timestep_spacing", "karras"]):
        with pytest.raises(SystemExit):
            G.parse_args(bad)


def test_engine_set_schedule_refuses_an_unknown_prediction_type():
    from distdiff_amd.engine import DDSamplerParams, Engine, PREDICTION_TYPES
    assert PREDICTION_TYPES == R.PRED
    assert [f[0] for f in DDSamplerParams._fields_][-2:] == ["prediction_type", "guidance_rescale"]
    eng = Engine.__new__(Engine)               # no library call is reached
    with pytest.raises(NotImplementedError, match="prediction_type"):
        eng.set_schedule([1], [0.5], 1.0, prediction_type="flow")
