"""Records what the host coefficient functions of the sampler step return on ONE build as tests/golden/step_row_bits.npz;
tests/test_step_row_bits.py replays the same calls on the current build and compares integers.

    python tests/golden/make_step_row_bits.py            # no GPU; DD_LIB=... records another build of the library

Run it on the build whose numbers are to be pinned (the commit BEFORE a change to the host part of sampler_step.hip), never to make a
failing test pass.  Only the five dd_op_step_coef* symbols are called.  Every case is one call: its return code and the raw uint32
patterns of its five-float output buffer, which is filled with FILL before the call -- a float the call did not write (the fifth of
dd_op_step_coefs, everything on a refusal in front of the arithmetic, *out of a refused dd_op_step_coef_2m_sde) is recorded as FILL,
a refusal behind the arithmetic leaves what it had written by then.  dd_op_step_coef_2m returns its float: code 0, word 0.

The grid: prediction types 0, 1, 2 on the leading, trailing and zero-terminal-SNR trailing schedules of tests/test_dpm_solver.py
(the last has a = 0 exactly at its first step) with n = 1, 2, 10, 50 steps, every step (c is 0 at the first and the last);
eta in {0, 0.3, 1}, s in {0, 0.5, 1}; out of range eta = -0.1, s = 1.5 and prediction type 3; the limit inputs a' = 1, a' = a and
a = 1e-80 (the last gives a row that is not finite: the deterministic rule returns it with code 0, the stochastic rules refuse it)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "step_row_bits.npz")
FILL = 0xDEADBEEF
FNS = ("dd_op_step_coefs", "dd_op_step_coefs_eta", "dd_op_step_coefs_sde", "dd_op_step_coef_2m", "dd_op_step_coef_2m_sde")
ETAS, SS = (0.0, 0.3, 1.0), (0.0, 0.5, 1.0)
SCHEDULES = (("leading", False), ("trailing", False), ("trailing", True))
NS = (1, 2, 10, 50)
LIMITS = ((0.3, 0.5, 1.0), (0.3, 0.5, 0.5), (0.3, 1e-80, 0.5))          # (a_before, a, a'): a' = 1, a' = a, a = 1e-80
# per (schedule, n, step, type) 1 + 3 + 3 + 1 + 3 calls; 5 out-of-range calls per step of the leading schedules; per limit triple and type
# the same with one more eta and s, and 3 calls with type 3
N_CASES = 3 * len(SCHEDULES) * sum(NS) * 11 + sum(NS) * 5 + len(LIMITS) * (3 * 14 + 3)


def cases():
    """[(fn index, prediction type, i, n, a_before, a, a', eta or s)] in a fixed order; what a function does not take is 0."""
    sys.path.insert(0, os.path.join(HERE, ".."))
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from test_dpm_solver import _schedule
    out = []

    def triple(pt, i, n, ab, a, ap, etas, ss):
        out.append((0, pt, 0, 0, 0.0, a, ap, 0.0))
        out.extend((1, pt, 0, 0, 0.0, a, ap, e) for e in etas)
        out.extend((2, pt, 0, 0, 0.0, a, ap, s) for s in ss)
        out.append((3, 0, i, n, ab, a, ap, 0.0))
        out.extend((4, 0, i, n, ab, a, ap, s) for s in ss)

    for spacing, zero_snr in SCHEDULES:
        for n in NS:
            tr = _schedule(spacing, zero_snr, n)[2]
            assert len(tr) == n and (not zero_snr or tr[0][1] == 0.0)
            for i, (ab, a, ap) in enumerate(tr):
                for pt in (0, 1, 2):
                    triple(pt, i, n, 0.0 if ab is None else float(ab), float(a), float(ap), ETAS, SS)
                if spacing == "leading":                                     # out of range, on real triples
                    ab = 0.0 if ab is None else float(ab)
                    out.extend([(0, 3, 0, 0, 0.0, float(a), float(ap), 0.0), (1, 3, 0, 0, 0.0, float(a), float(ap), 0.3),
                                (2, 3, 0, 0, 0.0, float(a), float(ap), 0.5), (1, 1, 0, 0, 0.0, float(a), float(ap), -0.1),
                                (2, 1, 0, 0, 0.0, float(a), float(ap), 1.5)])
    for ab, a, ap in LIMITS:
        for pt in (0, 1, 2):
            triple(pt, 3, 10, ab, a, ap, ETAS + (-0.1,), SS + (1.5,))
        out.extend([(0, 3, 0, 0, 0.0, a, ap, 0.0), (1, 3, 0, 0, 0.0, a, ap, 1.0), (2, 3, 0, 0, 0.0, a, ap, 1.0)])
    return out


def replay(L, cs):
    """Every case on library L -> (return codes int32 [N], words uint32 [N, 5])."""
    rc, bits = np.zeros(len(cs), dtype=np.int32), np.zeros((len(cs), 5), dtype=np.uint32)
    for k, (fn, pt, i, n, ab, a, ap, s) in enumerate(cs):
        buf = np.full(5, FILL, dtype=np.uint32)
        p = buf.ctypes.data_as(C.c_void_p)
        if fn == 0:
            rc[k] = L.dd_op_step_coefs(pt, a, ap, p)
        elif fn == 1:
            rc[k] = L.dd_op_step_coefs_eta(pt, a, ap, s, p)
        elif fn == 2:
            rc[k] = L.dd_op_step_coefs_sde(pt, a, ap, s, p)
        elif fn == 3:
            buf[0] = np.array([L.dd_op_step_coef_2m(i, n, ab, a, ap)], dtype=np.float32).view(np.uint32)[0]
        else:
            rc[k] = L.dd_op_step_coef_2m_sde(i, n, ab, a, ap, s, p)
        bits[k] = buf
    return rc, bits


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from distdiff_amd import _lib
    L = _lib.lib()
    cs = cases()
    assert len(cs) == N_CASES, (len(cs), N_CASES)
    rc, bits = replay(L, cs)
    np.savez_compressed(PATH, cases=np.array(cs, dtype=np.float64), rc=rc, bits=bits)
    print("wrote %s: %d cases (%d refused), %d bytes, library %s" % (PATH, len(cs), int((rc != 0).sum()), os.path.getsize(PATH), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
