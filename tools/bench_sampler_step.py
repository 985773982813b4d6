"""Times the sampler-step kernels at the bench shape (B = 32: 64 images' worth of UNet output rows, 64 x 64 latents, C = 4) through the
op-level ABI, forward and backward: the division form of (epsilon, no rescale) -- the `cfg_ddim_*` variants, named after the entry points
that are this mode --, the linear form (v-prediction) and the linear form with CFG rescale (which adds the two-stage statistics pass in
front of the forward and the dot-product pass in front of the backward).

    python tools/bench_sampler_step.py [--out FILE.json] [--launches 2000] [--rounds 5]

Device events around `--launches` back-to-back launches per variant, the variants alternating inside every round; the figure is the
median over the rounds, in microseconds per call.  Every buffer was just written and fits the last-level cache, as in the engine, where
the step follows the UNet's conv_out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--latent", type=int, default=64)
    a = ap.parse_args()
    from distdiff_amd import _lib
    L = _lib.lib()
    B, Cc, HW = a.batch, 4, a.latent * a.latent
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    g = torch.Generator().manual_seed(0)
    m2 = torch.zeros(2 * B * HW, 8)
    m2[:, :Cc] = torch.randn(2 * B * HW, Cc, generator=g)
    m2, z = m2.cuda(), torch.randn(B, Cc, HW, generator=g).cuda()
    gx0, gzp = torch.randn(B, Cc, HW, generator=g).cuda(), torch.randn(B, Cc, HW, generator=g).cuda()
    zp, x0, gz = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    gm = torch.zeros(2 * B * HW, 8, device="cuda", dtype=torch.bfloat16)
    al, ap_ = 0.64, 0.81
    coef = torch.tensor([7.5, al ** 0.5, (1 - al) ** 0.5, ap_ ** 0.5, (1 - ap_) ** 0.5]).cuda()
    out4 = (C.c_float * 4)()
    assert L.dd_op_step_coefs(1, al, ap_, out4) == 0
    lin = torch.tensor(list(out4)).cuda()
    stats = torch.zeros(B, 8, device="cuda")
    part = torch.zeros(int(L.dd_op_sampler_step_scratch_floats(B, HW)), device="cuda")

    def fwd(pred, phi):
        return lambda: L.dd_op_sampler_step(P(m2), 8, P(z), P(zp), P(x0), B, Cc, HW, P(coef), P(lin), pred, phi, P(stats), P(part), None)

    def bwd(pred, phi):
        return lambda: L.dd_op_sampler_step_bwd(P(gx0), P(gzp), P(gm), 8, P(gz), B, Cc, HW, P(coef), P(lin), pred, phi, P(m2), P(stats), P(part), None)

    variants = {"cfg_ddim_fwd": fwd(0, 0.0), "step_fwd_v": fwd(1, 0.0), "step_fwd_v_rescale": fwd(1, 0.7),
                "cfg_ddim_bwd": bwd(0, 0.0), "step_bwd_v": bwd(1, 0.0), "step_bwd_v_rescale": bwd(1, 0.7)}
    for f in variants.values():                       # warm-up: code objects, clocks
        for _ in range(50):
            assert f() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    # bytes the single-pass kernels move: both halves of the fp32 rows + z in, x0 + z' out (forward); two cotangents in, g_z + both bf16 rows out
    res = {"shape": {"B": B, "C": Cc, "HW": HW, "row_floats": 8}, "launches_per_window": a.launches, "rounds": a.rounds,
           "unit": "microseconds per call, median over the rounds (min, max)",
           "bytes_fwd": 2 * B * HW * 32 + 3 * B * Cc * HW * 4, "bytes_bwd": 3 * B * Cc * HW * 4 + 2 * B * HW * 16}
    for k, v in times.items():
        res[k] = {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3)}
    res["rescale_extra_fwd_us"] = round(res["step_fwd_v_rescale"]["median_us"] - res["step_fwd_v"]["median_us"], 3)
    res["rescale_extra_bwd_us"] = round(res["step_bwd_v_rescale"]["median_us"] - res["step_bwd_v"]["median_us"], 3)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
