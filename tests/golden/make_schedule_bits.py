"""Records the bits of Engine.expand under every kind of schedule on ONE build as tests/golden/schedule_bits.npz;
tests/test_schedule_bits_gpu.py replays the same loops on the current build and compares.

    python tests/golden/make_schedule_bits.py            # needs a GPU; DD_LIB= / DD_LIB_F16= record another build of the libraries

Run it on the build whose loop is to be pinned (the commit BEFORE a change to how the engine holds or reads its schedule), never to
make a failing test pass.  The file holds, per case, the SHA-256 of the raw bytes of z_out, of the decoded image and of score_out.

Engines: the two tiny engines of tests/test_dpm_solver_gpu.py::make_setup -- 'eps' (tiny_config, epsilon, leading: the division form
of the step) and 'sd2' (tiny_sd2_config, v-prediction, trailing, guidance_rescale 0.7: the linear form and the statistics kernels) --,
B = 2, L = 16, 10 steps, start index 5, guide window = steps 6 and 7: the smallest setup in which a history, a guide window and a last
first-order step all occur.  Each in the bf16 and in the fp16 library.
Cases per engine: {ddim, ddim eta = 0.5, dpmsolver++, dpmsolver++ sde_eta = 0.7} x {no guidance, transform guidance, direct guidance};
on 'sd2' also the four schedules on the zero-terminal-SNR trailing table from step 0 (text_to_img, transform guidance), so that the
a = 0 rows reach the device tables.

The loop is bitwise deterministic at a fixed engine batch: every case runs twice in this process and once in a fresh process, and the
file is not written unless the three digests of every case agree."""
import dataclasses
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "schedule_bits.npz")
N_STEPS, START, FIRST, COUNT = 10, 5, 6, 2
SEED, IDS = 5, [7, (3 << 32) | 2]
SCHEDULES = {"ddim": dict(solver="ddim"), "ddim_eta0.5": dict(solver="ddim", eta=0.5),
             "dpm": dict(solver="dpmsolver++"), "dpm_sde0.7": dict(solver="dpmsolver++", sde_eta=0.7)}
GUIDANCE = {"none": None, "transform": "transform_guidance", "direct": "direct_guidance"}
ENGINES = [(kind, act) for act in ("bf16", "fp16") for kind in ("eps", "sd2")]
SAMPLER = {"eps": dict(pred="epsilon", spacing="leading", phi=0.0), "sd2": dict(pred="v_prediction", spacing="trailing", phi=0.7)}
OUTPUTS = ("z_out", "image", "score")


def case_names(kind, act):
    names = ["%s/%s/%s/%s" % (act, kind, sc, gt) for sc in SCHEDULES for gt in GUIDANCE]
    if kind == "sd2":
        names += ["%s/sd2/%s/zero_snr_transform" % (act, sc) for sc in SCHEDULES]
    return names


ALL_CASES = [n for kind, act in ENGINES for n in case_names(kind, act)]


def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def make_engine(kind, act):
    """The engine and inputs of tests/test_dpm_solver_gpu.py::make_setup (same seeds), without the oracle's models, in library `act`."""
    import torch
    import torch.nn.functional as F
    from distdiff_amd.config import tiny_config, tiny_sd2_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.weights import synthetic_weights
    cfg = (tiny_sd2_config if kind == "sd2" else tiny_config)(max_batch=2)
    g = torch.Generator().manual_seed(21 if kind == "sd2" else 22)
    B, Ls, T, Dm, W = 2, cfg.latent_size, cfg.text_len, cfg.guide.feature_dim, cfg.unet.cross_attention_dim
    fx = dict(z=torch.randn(B, 4, Ls, Ls, generator=g), lat=torch.randn(B, 4, Ls, Ls, generator=g) * 0.9,
              noise=torch.randn(B, 4, Ls, Ls, generator=g), e=torch.rand(B, 4, 1, 1, generator=g), b=torch.randn(B, 4, 1, 1, generator=g),
              prompt=torch.randn(B, T, W, generator=g), negative=torch.randn(1, T, W, generator=g).expand(B, -1, -1).contiguous(),
              Pc=F.normalize(torch.randn(5, Dm, generator=g), dim=-1), Pg=F.normalize(torch.randn(5, 3, Dm, generator=g), dim=-1),
              targets=torch.tensor([1, 3]))
    eng = Engine(cfg, synthetic_weights(cfg, seed=0, num_classes=5), enable_grad=True, max_guidance_period=2, act_dtype=act)
    eng.set_prototypes(fx["Pc"], fx["Pg"])
    eng.set_prompt(torch.cat([fx["negative"], fx["prompt"]]).cuda())
    return cfg, eng, fx


def replay(kind, act):
    """Every case of one engine -> {"<case>/<output>": sha256 hex}."""
    import torch
    from distdiff_amd.scheduler import DDIMSchedule
    cfg, eng, fx = make_engine(kind, act)
    got = {}
    try:
        for name in case_names(kind, act):
            sc_name, gt_name = name.split("/")[2:]
            zero_snr = gt_name == "zero_snr_transform"
            sm, kw = SAMPLER[kind], SCHEDULES[sc_name]
            sc = dataclasses.replace(cfg.scheduler, prediction_type=sm["pred"], timestep_spacing=sm["spacing"], rescale_betas_zero_snr=zero_snr)
            sched = DDIMSchedule(sc)
            ts = sched.set_timesteps(N_STEPS)
            assert not zero_snr or float(sched.alphas_cumprod[ts[0]]) == 0.0
            eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=7.5, gs=1.0, ls=1.0, rho=10.0,
                             constraint_value=0.2, guidance_period=2, prediction_type=sm["pred"], guidance_rescale=sm["phi"], **kw)
            # a stochastic schedule keys the noise of its steps by (seed, unit ids); the inputs stay the given tensors
            noisy = dict(seed=SEED, unit_ids=IDS, generate_inputs=False) if ("eta" in kw or "sde_eta" in kw) else {}
            if zero_snr:
                out = eng.expand(None, fx["noise"], fx["e"], fx["b"], fx["targets"], 0, "transform_guidance", FIRST, COUNT, text_to_img=True, **noisy)
            else:
                out = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, GUIDANCE[gt_name], FIRST, COUNT, **noisy)
            torch.cuda.synchronize()
            assert all(torch.isfinite(t).all() for t in out), name
            for o, t in zip(OUTPUTS, out):
                got[name + "/" + o] = digest(t)
    finally:
        eng.close()
    return got


def replay_all():
    got = {}
    for kind, act in ENGINES:
        got.update(replay(kind, act))
    return got


def load():
    with np.load(PATH) as f:
        return dict(zip(f["names"].tolist(), f["sha256"].tolist()))


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    if "--print" in sys.argv:                       # the fresh process of the record: digests as one JSON line
        print("DIGESTS " + json.dumps(replay_all()))
        return
    # the fresh process first, while this one has not touched the GPU
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--print"], capture_output=True, text=True, check=True)
    fresh = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")][-1][len("DIGESTS "):])
    first, second = replay_all(), replay_all()
    assert sorted(first) == sorted(n + "/" + o for n in ALL_CASES for o in OUTPUTS)
    unstable = sorted({k.rsplit("/", 1)[0] for k in first if not (first[k] == second[k] == fresh.get(k))})
    if unstable:
        raise SystemExit("not written: %d of %d cases do not reproduce on this build: %s" % (len(unstable), len(ALL_CASES), ", ".join(unstable)))
    names = sorted(first)
    np.savez_compressed(PATH, names=np.array(names), sha256=np.array([first[n] for n in names]))
    from distdiff_amd import _lib
    print("wrote %s: %d cases, %d digests, %d bytes, libraries %s %s" % (PATH, len(ALL_CASES), len(names), os.path.getsize(PATH),
                                                                          _lib.LIB_PATH, _lib.LIB_PATH_F16))


if __name__ == "__main__":
    main()
