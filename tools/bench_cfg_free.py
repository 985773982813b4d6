"""Times the CFG-free engine (Engine(cfg_free=True): one UNet pass per step, on the conditional prompt alone) against the default
two-pass engine, on the same build and the same box, interleaved.  Two figures per engine at the benchmark shape (SD-1.x structure,
512 x 512, batch 32, synthetic weights):

  plain step    `denoise_step` (UNet forward without a stash + the sampler step), a window of --plain_steps calls
  guided batch  `expand` of the script of record: 50-step DDIM schedule, strength 0.5 (25 executed steps), transform guidance with P = 2
                chained steps at guidance_step 20, decode included -- bench.py's workload

    python tools/bench_cfg_free.py [--out profiles/cfg_free.json] [--rounds 2] [--batches 2] [--plain_steps 10] [--batch 32]

Two guided engines of 32 images do not fit one MI355X together (186.7 GB for the two-pass one alone), so the engines alternate by
visit: every round builds the two-pass engine, warms it up, times it and closes it, then the CFG-free one -- A B A B on one process, one
set of host weights.  A window is a host clock around work that ends in a device synchronise; every shape of a window runs once before
it.  Reported: the median over all windows of a kind (min, max), images/s = batch / time, the workspace of both engines, and the
ratios two-pass / CFG-free.  No ratio is expected in advance: the two-pass engine already runs the layers in front of the first
cross-attention once (the shared CFG prefix), and half the rows change the tile counts per CU.  Not measured: image quality -- the
weights are synthetic, base checkpoints trained for classifier-free guidance give poor images without it, and no distilled checkpoint
is run here."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STEPS, STRENGTH, GUIDANCE_STEP, P, PLAIN_INDEX = 50, 0.5, 20, 2, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=2, help="visits per engine")
    ap.add_argument("--batches", type=int, default=2, help="timed guided batches per visit")
    ap.add_argument("--plain_steps", type=int, default=10, help="denoise_step calls per plain window (two windows per visit)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--config", default="sd15", choices=["sd15", "tiny"], help="tiny: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    from distdiff_amd.config import sd15_config, tiny_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    B = a.batch
    cfg = (sd15_config if a.config == "sd15" else tiny_config)(max_batch=B)
    C_cls, K, Dm, L = 10, 3, cfg.guide.feature_dim, cfg.latent_size
    weights = synthetic_weights(cfg, seed=0, num_classes=C_cls)
    g = torch.Generator().manual_seed(3)
    Pc = torch.nn.functional.normalize(torch.randn(C_cls, Dm, generator=g), dim=-1)
    Pg = torch.nn.functional.normalize(torch.randn(C_cls, K, Dm, generator=g), dim=-1)
    prompt = torch.randn(2 * B, cfg.text_len, cfg.unet.cross_attention_dim, generator=g)        # negative half first
    sched = DDIMSchedule(cfg.scheduler)
    ts = sched.set_timesteps(STEPS)
    si, gfirst = int((1 - STRENGTH) * len(ts)), len(ts) - GUIDANCE_STEP

    def batch(seed):
        gd = torch.Generator().manual_seed(seed)
        return ((torch.randn(B, 4, L, L, generator=gd) * 0.18215 * 5).to(dev), torch.randn(B, 4, L, L, generator=gd).to(dev),
                torch.rand(B, 4, generator=gd).to(dev), torch.randn(B, 4, generator=gd).to(dev), torch.randint(0, C_cls, (B,), generator=gd).to(dev))

    def visit(cfg_free, seed):
        """One engine, built, warmed up, timed and closed -> (plain window times per step, guided batch times, workspace bytes)."""
        eng = Engine(cfg, weights, enable_grad=True, max_guidance_period=P, cfg_free=cfg_free)
        try:
            eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_scale=7.5, gs=1.0, ls=1.0, rho=10.0, constraint_value=0.2,
                             guidance_period=P)
            eng.set_prototypes(Pc, Pg)
            eng.set_prompt((prompt[B:] if cfg_free else prompt).to(dev))
            lat, noise, e, b, tg = batch(1)

            def guided(inputs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                z, img, _ = eng.expand(*inputs[:4], inputs[4], si, "transform_guidance", gfirst, P, want_image=True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert torch.isfinite(z).all() and torch.isfinite(img).all()
                return dt

            def plain(z):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.plain_steps):
                    z, _ = eng.denoise_step(z, PLAIN_INDEX)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.plain_steps

            plain(noise)                                   # warm-up: every shape and kernel of both windows once
            guided((lat, noise, e, b, tg))
            pl = [plain(noise)]
            gd = [guided(batch(seed + k)) for k in range(a.batches)]
            pl.append(plain(noise))
            return pl, gd, eng.workspace_bytes()
        finally:
            eng.close()
            torch.cuda.empty_cache()

    modes = [("two_pass", False), ("cfg_free", True)]
    plain_t, guided_t, ws = {m: [] for m, _ in modes}, {m: [] for m, _ in modes}, {}
    for r in range(a.rounds):
        for name, flag in modes:
            pl, gd, ws[name] = visit(flag, 100 + 10 * r)
            plain_t[name] += pl
            guided_t[name] += gd
            print("round %d %s: plain %s ms/step, guided %s s/batch" % (r, name, ["%.1f" % (1e3 * t) for t in pl], ["%.3f" % t for t in gd]), flush=True)

    def stat(v, scale=1.0, nd=4):
        return {"median": round(scale * statistics.median(v), nd), "min": round(scale * min(v), nd), "max": round(scale * max(v), nd), "windows": len(v)}

    res = {"workload": "%s structure, %dx%d, batch %d, synthetic weights; plain: denoise_step at step index %d of a %d-step DDIM schedule; guided: "
                       "expand, strength %.1f (%d executed steps), transform guidance P = %d at guidance_step %d, decode included"
                       % (a.config, 8 * L, 8 * L, B, PLAIN_INDEX, STEPS, STRENGTH, len(ts) - si, P, GUIDANCE_STEP),
           "how": "one process, one build; the engines alternate by visit (build, warm up, time, close), two_pass then cfg_free in each of %d "
                  "rounds; host clock around work that ends in a device synchronise; per visit two plain windows of %d steps around %d guided "
                  "batches" % (a.rounds, a.plain_steps, a.batches),
           "device": torch.cuda.get_device_name(dev)}
    for name, _ in modes:
        pm, gm = statistics.median(plain_t[name]), statistics.median(guided_t[name])
        res[name] = {"plain_ms_per_step": stat(plain_t[name], 1e3, 2), "plain_images_per_s_per_step": round(B / pm, 2),
                     "guided_s_per_batch": stat(guided_t[name]), "guided_images_per_s": round(B / gm, 3), "workspace_gb": round(ws[name] / 1e9, 2)}
    res["plain_step_time_ratio_two_pass_over_cfg_free"] = round(res["two_pass"]["plain_ms_per_step"]["median"] / res["cfg_free"]["plain_ms_per_step"]["median"], 3)
    res["guided_batch_time_ratio_two_pass_over_cfg_free"] = round(res["two_pass"]["guided_s_per_batch"]["median"] / res["cfg_free"]["guided_s_per_batch"]["median"], 3)
    res["not_measured"] = ("image quality: the weights are synthetic; a base (non-distilled) checkpoint without classifier-free guidance gives poor "
                           "images, and no guidance-distilled checkpoint is run here.  The automatic batch (batch_for_free_hbm) keeps its two-pass figures")
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
