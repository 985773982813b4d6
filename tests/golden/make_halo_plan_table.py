"""Records what the launcher does with every halo 3x3 problem of the test tables BEYOND the kernel's bits: tile geometry, address table,
LDS bytes and grid (dd_op_conv_halo_plan) -> tests/golden/halo_plan_table.npz.  No GPU is needed.

    python tests/golden/make_halo_plan_table.py

None of these fields changes an output bit -- another tile width, a dropped address table or another grid only change the speed -- so the
bit records (tests/test_pingpong_bits_gpu.py, tests/test_conv_exact_gpu.py) and tests/golden/conv_plan_table.npz (kind, form, split,
narrow) cannot see them move.  The committed table was recorded on the decision code of commit e7e9c93, BEFORE the host side of
conv_halo.hip was reorganised into one plan (the query was written on that commit's unchanged functions).  Re-record only when a decision
is changed on purpose, and say which.

Problems:
  * every row of tests/conv_plan_cases.py whose recorded kind in tests/golden/conv_plan_table.npz is conv_halo or conv_halo_persist;
  * conv_exact_cases.HALO_CASES and the 3x3 cases of make_pingpong_bits.CONV;
  * EXTRA: two non-square problems.  By the launcher's arithmetic every default geometry of a square image fits the one-tile kernel's
    address table into the 160 KB of LDS; an image of 4 (2) rows x 128 pixels does not take 512-pixel tiles, runs 256 x 320 tiles at
    tw = 128, th = 2, and its table does not fit (149 824 B without, 166 464 B with it): table = 0 without DD_HALO_TAB=0.

The file holds, per library (bf16, fp16), the distinct 12-field answers (`outcomes_*`) and the answer of every problem (`index_*`), the
block names and row numbers of the conv_plan_cases rows, the names of the other problems and `commit`.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import conv_plan_cases as cases  # noqa: E402

PATH = os.path.join(HERE, "halo_plan_table.npz")
FIELDS = ("kind", "form", "tw", "th", "tiles_x", "tiles_y", "images_per_tile", "table", "lds_bytes", "grid_x", "grid_y", "persist")
F = {n: i for i, n in enumerate(FIELDS)}
LIBS = ("bf16", "fp16")
EXTRA = (("extra_4x128_table_does_not_fit", 48, 64, 640, 4, 128), ("extra_2x128_table_does_not_fit", 96, 64, 640, 2, 128))


def plan_case_rows():
    """[(block name, row numbers, rows)]: the rows of conv_plan_cases whose RECORDED kind is a halo kernel"""
    t = np.load(os.path.join(HERE, "conv_plan_table.npz"))
    kind = t["outcomes"][t["index"]][:, 0]
    out, off = [], 0
    for name, rows in cases.blocks():
        at = np.nonzero((kind[off:off + len(rows)] == 1) | (kind[off:off + len(rows)] == 2))[0]
        off += len(rows)
        if len(at):
            out.append((name, at.astype(np.int32), rows[at]))
    assert off == len(kind), "tests/conv_plan_cases.py no longer generates the cases conv_plan_table.npz was recorded for"
    return out


def params_of_rows(rows):
    """ConvGemmParams blocks (numpy struct array) and scratch capacities of conv_plan_cases rows, filled as conv_plan_cases.evaluate
    fills them (halo problems: no mask / raw / LayerNorm fold / row statistics)"""
    from distdiff_amd._lib import ConvGemmParams
    c, ptr = cases.COL, 1 << 12
    p = np.zeros(len(rows), dtype=np.dtype(ConvGemmParams))
    for name in ("B", "H", "W", "Ho", "Wo", "stride", "shift", "parity", "cin", "ntaps", "M", "N", "K", "ksplit", "flags", "force_small",
                 "wgroup_rows", "x_ld", "y_ld", "res_ld", "raw_ld", "rowpart_ld"):
        p[name] = rows[:, c[name]]
    flags = rows[:, c["flags"]]
    assert not (flags & ~(cases.BIAS | cases.RES | cases.RELU | cases.OUT_F32 | cases.STATS)).any() and not rows[:, c["drop"]].any()
    p["alpha"] = rows[:, c["alpha_q"]] / 4.0
    for name in ("x", "w", "taptab", "y"):
        p[name] = ptr
    p["bias"], p["res"] = np.where(flags & cases.BIAS, ptr, 0), np.where(flags & cases.RES, ptr, 0)
    p["stats"], p["stats_ld"] = np.where(flags & cases.STATS, ptr, 0), np.where(flags & cases.STATS, rows[:, c["y_ld"]], 0)
    p["bias_sel"] = np.where(rows[:, c["bias_sel"]], ptr, 0)
    scratch = rows[:, c["scratch"]]
    p["partial"] = np.where(scratch, ptr, 0)
    caps = np.where(scratch == 1, 16, np.where(scratch == 2, 2, 0)) * rows[:, c["M"]] * rows[:, c["N"]] * 4
    return p, caps.tolist()


def named_problems():
    """[(name, Problem)]: the halo cases of the exact tests (CASES and STAT_CASES), the 3x3 cases of the ping-pong bit record, EXTRA"""
    import conv_exact_cases as T
    from exact_ref import Problem
    out = [("exact:" + c[0].name, c[0]) for c in T.HALO_CASES]
    out += [("exact:" + c[0].name, c[0]) for c in T.STAT_CASES if c[1][0] in (T.HALO, T.PERSIST)]
    rec = T.record_problems()
    out += [("pp:" + c[0], rec["pp:" + c[0]][0]) for c in T.pp.CONV]
    out += [(e[0], Problem(*e)) for e in EXTRA]
    return out


def params_of_problems(probs):
    import torch
    import conv_exact_cases as T
    from distdiff_amd import ops
    from distdiff_amd._lib import ConvGemmParams
    p, caps = np.zeros(len(probs), dtype=np.dtype(ConvGemmParams)), []
    for i, (_name, prob) in enumerate(probs):
        pk, x, kw, _out = T.launch_args(ops, prob, torch.bfloat16)
        q, cap, _y, _keep = ops._conv_gemm_params(x, pk, *prob.geom, dry=True, **kw)
        p[i:i + 1] = np.frombuffer(bytes(q), dtype=p.dtype)
        caps.append(cap)
    return p, caps


def evaluate(lib_path, p, caps):
    """the 12 FIELDS of every problem as int32 [n, 12]; all zero where the launcher runs no halo kernel"""
    L = C.CDLL(lib_path)                                         # a handle of its own: plain addresses as arguments
    fn = L.dd_op_conv_halo_plan
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_void_p], C.c_int
    out = np.zeros((len(p), len(FIELDS)), dtype=np.int32)
    a0, o0, step = p.ctypes.data, out.ctypes.data, p.dtype.itemsize
    for i, cap in enumerate(caps):
        if fn(a0 + i * step, cap, o0 + i * 4 * len(FIELDS)) != 1:
            out[i] = 0
    return out


def problems():
    """(labels, params, caps, block names, block sizes, row numbers, names) of the whole table, in the recorded order"""
    blks, named = plan_case_rows(), named_problems()
    p1, c1 = params_of_rows(np.concatenate([r for _n, _a, r in blks]))
    p2, c2 = params_of_problems(named)
    labels = ["%s[%d]" % (n, i) for n, at, _r in blks for i in at] + [n for n, _p in named]
    return (labels, np.concatenate([p1, p2]), c1 + c2, [n for n, _a, _r in blks], [len(a) for _n, a, _r in blks],
            np.concatenate([a for _n, a, _r in blks]), [n for n, _p in named])


def lib_paths():
    from distdiff_amd import _lib
    _lib.lib(), _lib.lib("fp16")
    return {"bf16": _lib.LIB_PATH, "fp16": _lib.LIB_PATH_F16}


def main():
    labels, p, caps, bnames, bsizes, rownos, names = problems()
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=HERE).stdout.strip()
    save = dict(fields=np.array(FIELDS), block_names=np.array(bnames), block_sizes=np.array(bsizes, dtype=np.int64), rows=rownos.astype(np.int32),
                names=np.array(names), commit=np.array(commit))
    for dt, path in lib_paths().items():
        res = evaluate(path, p, caps)
        assert (res[:, 0] > 0).all(), "%s: the launcher runs no halo kernel on %s" % (dt, labels[int(np.argmin(res[:, 0] > 0))])
        outcomes, index = np.unique(res, axis=0, return_inverse=True)
        assert len(outcomes) < 65536
        save["outcomes_" + dt], save["index_" + dt] = outcomes.astype(np.int32), index.reshape(-1).astype(np.uint16)
        print("%s: %d problems, %d distinct plans" % (dt, len(res), len(outcomes)))
        for n in names[-len(EXTRA):]:
            print("  ", n, dict(zip(FIELDS, res[labels.index(n)].tolist())))
    np.savez_compressed(PATH, **save)
    print("%d bytes -> %s (decision code of %s)" % (os.path.getsize(PATH), PATH, commit))


if __name__ == "__main__":
    main()
