"""Records the bits of the sampler-step ops (dd_op_cfg_ddim*, dd_op_sampler_step*, dd_op_sampler_step_2m) of ONE build as
tests/golden/sampler_step_bits.npz; tests/test_sampler_step_bits_gpu.py replays the same calls on the current build and compares.

    python tests/golden/make_sampler_step_bits.py            # needs a GPU; DD_LIB=... records another build of the library

Run it on the build whose arithmetic is to be pinned (the commit BEFORE a change to the step's kernels), never to make a failing test
pass.  Only dd_op_* symbols of ABI 9 are used.  The file holds the inputs themselves (not seeds), the coefficient rows, and for every
case the SHA-256 of the raw bytes of each output.

Shapes (B, C, HW, ld): (3, 4, 300, 8) odd batch, two 256-pixel blocks with a ragged last one, a real second stage of the rescale merge;
(1, 8, 70, 8) both 16-byte halves of the row; (2, 3, 40, 16) C < 4 and gradient columns >= 8 that must come out zero.  The padding
columns of m2 hold 1e30; g_m2 is pre-filled with NaN so that an unwritten column shows."""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "sampler_step_bits.npz")
SHAPES = [(3, 4, 300, 8), (1, 8, 70, 8), (2, 3, 40, 16)]
S, A_BEFORE, A, AP = 7.5, 0.45, 0.64, 0.81
MODES = [(pt, phi) for pt in (0, 1, 2) for phi in (0.0, 0.7)]
INPUTS = ("z", "m2", "x0_prev", "g_x0", "g_zprev")


def tag(shape):
    return "B%d_C%d_HW%d_ld%d" % shape


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def draw(L):
    """The arrays of the fixture apart from the digests: inputs per shape, coefficient rows, c."""
    g = torch.Generator().manual_seed(20)
    fx = {}
    for shape in SHAPES:
        B, Cc, HW, ld = shape
        rows = torch.full((2 * B * HW, ld), 1e30)
        rows[:, :Cc] = torch.randn(2 * B * HW, Cc, generator=g)
        fx[tag(shape) + "/m2"] = rows.numpy()
        for name in ("z", "x0_prev", "g_x0", "g_zprev"):
            fx[tag(shape) + "/" + name] = torch.randn(B, Cc, HW, generator=g).numpy()
    fx["coef"] = np.array([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, (1 - AP) ** 0.5], dtype=np.float32)
    lin = np.zeros((3, 4), dtype=np.float32)
    for pt in range(3):
        out = (C.c_float * 4)()
        assert L.dd_op_step_coefs(pt, A, AP, out) == 0
        lin[pt] = list(out)
    fx["lin"] = lin
    fx["c2m"] = np.array([L.dd_op_step_coef_2m(3, 10, A_BEFORE, A, AP)], dtype=np.float32)
    assert fx["c2m"][0] > 0
    return fx


def replay(L, fx, shape):
    """Every case of `shape` on library L with the stored inputs -> {"<shape>/<case>/<output>": sha256 hex}."""
    B, Cc, HW, ld = shape
    t = {k: torch.from_numpy(fx[tag(shape) + "/" + k]).cuda() for k in INPUTS}
    coef, c2m = torch.from_numpy(fx["coef"]).cuda(), float(fx["c2m"][0])
    lins = [torch.from_numpy(fx["lin"][pt]).cuda() for pt in range(3)]
    part = torch.zeros(int(L.dd_op_sampler_step_scratch_floats(B, HW)), device="cuda")
    got = {}

    def put(case, **outs):
        torch.cuda.synchronize()
        for k, v in outs.items():
            got["%s/%s/%s" % (tag(shape), case, k)] = digest(v)

    def nan(dtype=torch.float32, n=None):
        return torch.full((B, Cc, HW) if n is None else n, float("nan"), device="cuda", dtype=dtype)

    for with_x0 in (True, False):
        zp, x0 = nan(), nan()
        assert L.dd_op_cfg_ddim(P(t["m2"]), ld, P(t["z"]), P(zp), P(x0) if with_x0 else None, B, Cc, HW, P(coef), None) == 0
        put("cfg_ddim" if with_x0 else "cfg_ddim_no_x0", z_prev=zp, **({"x0": x0} if with_x0 else {}))
    for case, gx, gp in (("both", t["g_x0"], t["g_zprev"]), ("no_g_x0", None, t["g_zprev"]), ("no_g_zprev", t["g_x0"], None)):
        g_z, g_m2 = nan(), nan(torch.bfloat16, (2 * B * HW, ld))
        assert L.dd_op_cfg_ddim_bwd(P(gx), P(gp), P(g_m2), ld, P(g_z), B, Cc, HW, P(coef), None) == 0
        put("cfg_ddim_bwd_" + case, g_z=g_z, g_m2=g_m2)
    for pt, phi in MODES:
        mode = "pt%d_phi%.1f" % (pt, phi)
        stats = torch.zeros(B, 8, device="cuda")
        zp, x0 = nan(), nan()
        assert L.dd_op_sampler_step(P(t["m2"]), ld, P(t["z"]), P(zp), P(x0), B, Cc, HW, P(coef), P(lins[pt]), pt, phi, P(stats), P(part), None) == 0
        put("step_" + mode, x0=x0, z_prev=zp, **({"stats": stats[:, :7]} if phi else {}))
        # the backward runs on the statistics this forward left
        g_z, g_m2 = nan(), nan(torch.bfloat16, (2 * B * HW, ld))
        assert L.dd_op_sampler_step_bwd(P(t["g_x0"]), P(t["g_zprev"]), P(g_m2), ld, P(g_z), B, Cc, HW, P(coef), P(lins[pt]), pt, phi, P(t["m2"]),
                                        P(stats), P(part), None) == 0
        put("step_bwd_" + mode, g_z=g_z, g_m2=g_m2)
        for in_place in (False, True):
            hist = t["x0_prev"].clone()
            zp, x0 = nan(), (hist if in_place else nan())
            assert L.dd_op_sampler_step_2m(P(t["m2"]), ld, P(t["z"]), P(hist), c2m, P(zp), P(x0), B, Cc, HW, P(coef), P(lins[pt]), pt, phi,
                                           P(stats), P(part), None) == 0
            put("step_2m_%s_%s" % (mode, "in_place" if in_place else "out_of_place"), x0=x0, z_prev=zp)
    return got


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from distdiff_amd import _lib
    L = _lib.lib()
    fx = draw(L)
    got = {}
    for shape in SHAPES:
        got.update(replay(L, fx, shape))
        again = replay(L, fx, shape)
        assert all(got[k] == v for k, v in again.items()), "the build is not deterministic on %s" % (shape,)
    names = sorted(got)
    fx["case_names"] = np.array(names)
    fx["case_sha256"] = np.array([got[n] for n in names])
    np.savez_compressed(PATH, **fx)
    print("wrote %s: %d outputs, %d bytes, library %s" % (PATH, len(names), os.path.getsize(PATH), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
