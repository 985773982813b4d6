"""Times `Engine.expand` at the benchmark shape (SD-1.x structure, 512 x 512, synthetic weights, strength 0.5, transform guidance with
P = 2 chained steps, decode included) under the two samplers at the step counts they are meant for: DDIM on a 50-step schedule (25
executed steps; the script of record) and DPM-Solver++(2M) on a 20-step schedule (10 executed steps).  The guide window starts 3/5
through the schedule in both (guidance_step 20 of 50, 8 of 20), as scripts/exps/expand_diff.sh places it.

    python tools/bench_solver.py [--out profiles/dpmpp_2m.json] [--rounds 3] [--batch 0]
    python tools/bench_solver.py --eta 1 [--out ...]      # instead: DDIM on the 50-step schedule with eta = 0 against eta = ETA
    python tools/bench_solver.py --sde_eta 1 [--out profiles/dpmpp_2m_sde.json]   # instead: dpmsolver++ on the 20-step schedule, s = 0 / S

One engine; the two settings alternate inside every round (set_schedule between them, outside the timed window); the window is a host
clock around one `expand` of a fresh batch that ends in a device synchronise.  Reported: the median over the rounds of seconds per
batch, images/s, and milliseconds per executed step = batch time / executed schedule steps (the guidance call, the step executed again
after it and the decode are inside the batch time, so they are spread over the steps: over 25 of them and over 10).  The ratio of the
two batch times follows from the executed step counts; there is no gate on it.  What this does NOT measure: image quality at 20
against 50 steps -- the weights are synthetic.  With --eta the two settings are the script of record's DDIM loop under eta = 0 and under
eta = ETA (stochastic DDIM: the step noise is generated inside the step kernel from (seed, unit id, step), so `expand` gets a seed and
unit ids and still reads the batch's noise / e / b).  With --sde_eta they are DPM-Solver++(2M) on the 20-step schedule under sde_eta = 0 and
under sde_eta = S (SDE-DPM-Solver++(2M): the same generator inside the step kernel's history form)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SETTINGS = [dict(name="ddim_50", solver="ddim", steps=50, guidance_step=20), dict(name="dpmsolver++_20", solver="dpmsolver++", steps=20, guidance_step=8)]
STRENGTH, P = 0.5, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="0 = the largest of 32 / 16 / 8 that fits the free HBM (bench.py's rule)")
    ap.add_argument("--config", default="sd15", choices=["sd15", "tiny"], help="tiny: a rehearsal of the script, not a measurement")
    ap.add_argument("--eta", type=float, default=None, help="time DDIM 50 under eta = 0 against eta = ETA instead of the two solvers")
    ap.add_argument("--sde_eta", type=float, default=None, help="time dpmsolver++ 20 under sde_eta = 0 against sde_eta = S instead of the two solvers")
    a = ap.parse_args()
    if a.eta is not None and a.sde_eta is not None:
        raise SystemExit("--eta and --sde_eta are two measurements: one at a time")
    settings = SETTINGS if a.eta is None else [dict(SETTINGS[0], name="ddim_50_eta0", eta=0.0), dict(SETTINGS[0], name="ddim_50_eta", eta=a.eta)]
    if a.sde_eta is not None:
        settings = [dict(SETTINGS[1], name="dpmsolver++_20_s0", sde_eta=0.0), dict(SETTINGS[1], name="dpmsolver++_20_s", sde_eta=a.sde_eta)]
    from distdiff_amd.config import sd15_config, tiny_config
    from distdiff_amd.engine import Engine, batch_for_free_hbm
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    dev = torch.device("cuda:0")
    B = a.batch or (batch_for_free_hbm(torch.cuda.mem_get_info(dev)[0], guided=True) if a.config == "sd15" else 4)
    cfg = (sd15_config if a.config == "sd15" else tiny_config)(max_batch=B)
    C_cls, K, Dm, L = 10, 3, cfg.guide.feature_dim, cfg.latent_size
    eng = Engine(cfg, synthetic_weights(cfg, seed=0, num_classes=C_cls), enable_grad=True, max_guidance_period=P)
    g = torch.Generator().manual_seed(3)
    eng.set_prototypes(torch.nn.functional.normalize(torch.randn(C_cls, Dm, generator=g), dim=-1),
                       torch.nn.functional.normalize(torch.randn(C_cls, K, Dm, generator=g), dim=-1))
    eng.set_prompt(torch.randn(2 * B, cfg.text_len, cfg.unet.cross_attention_dim, generator=g).to(dev))
    sched = DDIMSchedule(cfg.scheduler)

    def batch(seed):
        gd = torch.Generator().manual_seed(seed)
        return ((torch.randn(B, 4, L, L, generator=gd) * 0.18215 * 5).to(dev), torch.randn(B, 4, L, L, generator=gd).to(dev),
                torch.rand(B, 4, generator=gd).to(dev), torch.randn(B, 4, generator=gd).to(dev), torch.randint(0, C_cls, (B,), generator=gd).to(dev))

    def run(s, seed):
        ts = sched.set_timesteps(s["steps"])
        eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=7.5, gs=1.0, ls=1.0, rho=10.0, constraint_value=0.2,
                         guidance_period=P, solver=s["solver"], eta=s.get("eta", 0.0), sde_eta=s.get("sde_eta", 0.0))
        lat, noise, e, b, tg = batch(seed)
        si = int((1 - STRENGTH) * len(ts))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = dict(seed=seed, unit_ids=list(range(B)), generate_inputs=False) if s.get("eta") or s.get("sde_eta") else {}
        z, img, _ = eng.expand(lat, noise, e, b, tg, si, "transform_guidance", len(ts) - s["guidance_step"], P, want_image=True, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(z).all() and torch.isfinite(img).all()
        return dt, len(ts) - si

    for s in settings:                                  # warm-up: every shape and kernel of both settings once
        run(s, 1)
    times = {s["name"]: [] for s in settings}
    execd = {}
    for r in range(a.rounds):
        for s in settings:
            dt, execd[s["name"]] = run(s, 100 + r)
            times[s["name"]].append(dt)
    res = {"workload": "%s structure, %dx%d, batch %d, synthetic weights, strength %.1f, transform guidance P = %d, decode included"
                       % (a.config, 8 * L, 8 * L, B, STRENGTH, P),
           "rounds": a.rounds, "unit": "median over the rounds (min, max); the two settings alternate inside every round",
           "device": torch.cuda.get_device_name(dev)}
    for s in settings:
        v, n = times[s["name"]], execd[s["name"]]
        med = statistics.median(v)
        res[s["name"]] = {"solver": s["solver"], "schedule_steps": s["steps"], "executed_steps": n, "guidance_step": s["guidance_step"],
                          "eta": s.get("eta", 0.0), "sde_eta": s.get("sde_eta", 0.0), "s_per_batch": round(med, 4), "s_per_batch_min": round(min(v), 4),
                          "s_per_batch_max": round(max(v), 4), "images_per_s": round(B / med, 3), "ms_per_executed_step": round(1e3 * med / n, 2)}
    if a.sde_eta is not None:
        res["batch_time_ratio_s_over_s0"] = round(res["dpmsolver++_20_s"]["s_per_batch"] / res["dpmsolver++_20_s0"]["s_per_batch"], 4)
        res["not_measured"] = "image quality and diversity under sde_eta > 0: the weights are synthetic"
    elif a.eta is None:
        res["batch_time_ratio_ddim50_over_2m20"] = round(res["ddim_50"]["s_per_batch"] / res["dpmsolver++_20"]["s_per_batch"], 3)
        res["not_measured"] = "image quality at 20 against 50 steps: the weights are synthetic"
    else:
        res["batch_time_ratio_eta_over_eta0"] = round(res["ddim_50_eta"]["s_per_batch"] / res["ddim_50_eta0"]["s_per_batch"], 4)
        res["not_measured"] = "image quality and diversity under eta > 0: the weights are synthetic"
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    eng.close()


if __name__ == "__main__":
    main()
