"""Deterministic problems for the conv / GEMM launcher's decision (dd_op_conv_gemm_plan: which kernel, which form, which split; or the
refusal).  The planner only tests pointers for null and reads no device, so the whole table is answered on a CPU.

blocks() yields (name, rows): rows is an int64 array with one problem per row, columns FIELDS.  Pointers are not fields: a buffer is
present exactly when the flag that needs it is set (bias, res, mask, raw, stats, ln_stats + ln_c1, rowpart), unless `drop` removes it;
`scratch` says how much split-K workspace there is (0 none, 1 ample: 16 M N floats, 2 tight: 2 M N floats).  alpha = alpha_q / 4.

tests/golden/make_conv_plan_table.py records the outcomes, tests/test_conv_plan_table.py compares a build against the record.
"""
import ctypes as C
import hashlib

import numpy as np

FIELDS = ("B", "H", "W", "Ho", "Wo", "stride", "shift", "parity", "cin", "ntaps", "M", "N", "K", "ksplit", "flags", "alpha_q",
          "force_small", "wgroup_rows", "x_ld", "y_ld", "res_ld", "raw_ld", "rowpart_ld", "bias_sel", "scratch", "drop")
COL = {n: i for i, n in enumerate(FIELDS)}
BIAS, RES, RELU, GEGLU, OUT_F32, MASK, RES_F32, RAW, STATS, LNFOLD, ROWSTATS = 1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 2048
DROP_STATS, DROP_ROWPART, DROP_LN = 1, 2, 4

BATCHES = (1, 2, 4, 16, 32)
SIDES = (8, 16, 24, 32, 48, 64, 96, 128, 256, 512)
CINS = (8, 64, 128, 256, 320, 512, 640, 1280, 2560)
NS = (4, 64, 128, 256, 320, 512, 640, 1280, 2560, 5120)
TAPS = (1, 9)
GEOMS = ((1, 0), (2, 0), (1, 1))       # (stride, shift): same size, stride-2 downsample, fused nearest-2x upsample
KSPLITS = (0, 1, 4)
SCRATCH = (0, 1, 2)
# every flag combination the engine issues; the sets of MAIN_FLAGS run the whole grid in the same order (block i of one set is the same
# problem as block i of another: the test pairs BIAS with BIAS | STATS), MORE_FLAGS a thinner one (ksplit 0, ample scratch)
MAIN_FLAGS = (BIAS, BIAS | RES, BIAS | RELU, BIAS | STATS, BIAS | OUT_F32, BIAS | MASK, BIAS | RES | RES_F32, BIAS | GEGLU,
              BIAS | GEGLU | RAW, BIAS | LNFOLD)
MORE_FLAGS = (0, BIAS | RES | RELU, BIAS | RES | STATS, BIAS | RELU | STATS, BIAS | GEGLU | LNFOLD, BIAS | GEGLU | RAW | LNFOLD,
              BIAS | STATS | ROWSTATS, BIAS | RES | ROWSTATS, BIAS | LNFOLD | ROWSTATS)
ROWPART_DIVS = (40, 64, 80, 160)       # rowpart_ld = N / d: the span count shows through the refusal of rowpart_ld < spans


def _product(*axes):
    g = np.meshgrid(*[np.asarray(a, dtype=np.int64) for a in axes], indexing="ij")
    return [x.reshape(-1) for x in g]


def _rows(B, side, cin, N, taps, geom, ksplit, scratch, flags, rowpart_ld=None):
    """Square images of `side` stored pixels; geom indexes GEOMS.  Leading dimensions as ops.py sets them for contiguous rows."""
    n = B.shape[0]
    r = np.zeros((n, len(FIELDS)), dtype=np.int64)
    stride = np.asarray([g[0] for g in GEOMS], dtype=np.int64)[geom]
    shift = np.asarray([g[1] for g in GEOMS], dtype=np.int64)[geom]
    out = (side << shift) // stride
    ncols = np.where(flags & GEGLU, N // 2, N)
    for name, v in (("B", B), ("H", side), ("W", side), ("Ho", out), ("Wo", out), ("stride", stride), ("shift", shift), ("cin", cin),
                    ("ntaps", taps), ("M", B * out * out), ("N", N), ("K", (taps * cin + 63) // 64 * 64), ("ksplit", ksplit),
                    ("flags", flags), ("x_ld", cin), ("y_ld", ncols), ("scratch", scratch)):
        r[:, COL[name]] = v
    r[:, COL["alpha_q"]] = 4
    r[:, COL["res_ld"]] = np.where(flags & RES, ncols, 0)
    r[:, COL["raw_ld"]] = np.where(flags & RAW, N, 0)
    if rowpart_ld is not None:
        r[:, COL["rowpart_ld"]] = rowpart_ld
    return r


def _set(rows, **kw):
    r = rows.copy()
    for k, v in kw.items():
        r[:, COL[k]] = v
    return r


def _base():
    """A small spread of problems that reaches every path, for the variations that the grid lacks"""
    B, side, cin, N, taps, geom, flags = _product((2, 16), (8, 32, 64), (64, 320, 640), (4, 128, 320, 640, 1280), TAPS, (0,),
                                                  (BIAS, BIAS | STATS, BIAS | RES, BIAS | OUT_F32))
    return _rows(B, side, cin, N, taps, geom, 0 * B, 0 * B + 1, flags)


def _extras():
    b = _base()
    c = COL
    yield "parity", _set(b, shift=1, parity=1, Ho=2 * b[:, c["H"]], Wo=2 * b[:, c["W"]], M=4 * b[:, c["M"]])   # stride-2 dgrad
    yield "force_small", _set(b, force_small=1)
    yield "bias_sel", _set(b, bias_sel=1)
    yield "alpha", _set(b, alpha_q=2)
    for name in ("x_ld", "y_ld", "res_ld"):                      # leading dimensions that are not multiples of 8, and one that is
        yield name + "+4", _set(b, **{name: b[:, c[name]] + 4})
        yield name + "+2", _set(b, **{name: b[:, c[name]] + 2})
        yield name + "+8", _set(b, **{name: b[:, c[name]] + 8})
    pw = b[(b[:, c["ntaps"]] == 1)]
    for fl in (0, BIAS, OUT_F32, BIAS | OUT_F32, BIAS | RELU):   # grouped GEMMs: good and bad multiples of the tile, and flags they refuse
        for wg in (64, 96, 128, 256, 384, 1024):
            yield "wgroup%d_%d" % (wg, fl), _set(pw, wgroup_rows=wg, flags=fl, res_ld=0)
        yield "wgroup_img_%d" % fl, _set(pw, wgroup_rows=pw[:, c["M"]] // pw[:, c["B"]], flags=fl, res_ld=0)
    yield "wgroup_taps", _set(b[b[:, c["ntaps"]] == 9], wgroup_rows=256, flags=BIAS, res_ld=0)
    yield "M0", _set(b, M=0, B=0)
    yield "Mneg", _set(b, M=-64)
    yield "N0", _set(b, N=0)
    yield "K+8", _set(b, K=b[:, c["K"]] + 8)
    yield "K+32", _set(b, K=b[:, c["K"]] + 32)
    # inputs at the 32-bit limits: element offsets of the whole input (0xFFFF0000), byte offsets of the whole input (0xF0000000: the
    # row-statistics forms and the big kernel's fast staging), byte offsets of one image (halo), of 256 / 64 rows (pps / ws)
    px = b[:, c["B"]] * b[:, c["H"]] * b[:, c["W"]]
    for name, lim, per in (("elem", 0xFFFF0000, px), ("byte", 0xF0000000 // 2, px), ("image", 0xF0000000 // 2, b[:, c["H"]] * b[:, c["W"]]),
                           ("rows256", 0xF0000000 // 2, 256 + 0 * px), ("rows64", 0xF0000000 // 2, 64 + 0 * px)):
        edge = (lim + per - 1) // per
        edge = (edge + 7) // 8 * 8
        for d in (-8, 0, 8):
            yield "x_ld_%s%+d" % (name, d), _set(b, x_ld=np.maximum(edge + d, 8))
    rs = _set(pw, flags=BIAS | ROWSTATS, res_ld=0)
    for d in ROWPART_DIVS:
        rsd = _set(rs, rowpart_ld=rs[:, c["N"]] // d)
        edge = ((0xF0000000 // 2 + px[b[:, c["ntaps"]] == 1] - 1) // px[b[:, c["ntaps"]] == 1] + 7) // 8 * 8
        yield "rowstats_x_ld_byte_%d" % d, _set(rsd, x_ld=edge)
        yield "rowstats_x_ld_byte-8_%d" % d, _set(rsd, x_ld=edge - 8)
    # a GEGLU projection whose weights are exactly / just below 0xF0000000 bytes (pps byte offsets of the weight matrix)
    B, side, cin, N = _product((12,), (64,), (49152, 49088), (40960, 40704))
    yield "weights_byte", _rows(B, side, cin, N, 0 * B + 1, 0 * B, 0 * B, 0 * B + 1, 0 * B + (BIAS | GEGLU))
    # a flag without its buffer
    yield "no_stats_buffer", _set(b, flags=BIAS | STATS, res_ld=0, drop=DROP_STATS)
    yield "no_rowpart_buffer", _set(rs, rowpart_ld=rs[:, c["N"]] // 40, drop=DROP_ROWPART)
    yield "no_ln_buffers", _set(pw, flags=BIAS | LNFOLD, res_ld=0, drop=DROP_LN)
    yield "lnfold_taps", _set(b[b[:, c["ntaps"]] == 9], flags=BIAS | LNFOLD, res_ld=0)


def blocks():
    grid = _product(BATCHES, SIDES, CINS, NS, TAPS, range(len(GEOMS)), KSPLITS, SCRATCH)
    for fl in MAIN_FLAGS:
        yield "grid_%d" % fl, _rows(*grid, 0 * grid[0] + fl)
    thin = _product(BATCHES, SIDES, CINS, NS, TAPS, range(len(GEOMS)), (0,), (1,))
    for fl in MORE_FLAGS:
        rp = thin[3] // 40 if fl & ROWSTATS else None
        yield "thin_%d" % fl, _rows(*thin, 0 * thin[0] + fl, rowpart_ld=rp)
    # CF_ROWSTATS: rowpart_ld innermost, so that rows 4 i .. 4 i + 3 are one problem at N / 40, N / 64, N / 80, N / 160
    *g, div = _product(BATCHES, SIDES, CINS, NS, TAPS, range(len(GEOMS)), KSPLITS, (0, 1), ROWPART_DIVS)
    yield "rowstats", _rows(*g, 0 * g[0] + (BIAS | ROWSTATS), rowpart_ld=g[3] // div)
    yield from _extras()


def cases_hash(blks):
    h = hashlib.sha256(repr(FIELDS).encode())
    for name, rows in blks:
        h.update(name.encode())
        h.update(np.ascontiguousarray(rows, dtype="<i8").tobytes())
    return h.hexdigest()


_PTR_FLAG = (("bias", BIAS), ("res", RES), ("mask", MASK), ("raw", RAW))
_NOT_READ = 1 << 12       # stands for a buffer: the planner tests pointers for null and never follows them


def evaluate(lib_path, rows):
    """(kind, form, split, narrow) of every row as an int16 [n, 4] array; a refusal is (-1, 0, 0, 0)"""
    from distdiff_amd._lib import ConvGemmParams
    L = C.CDLL(lib_path)                                         # a handle of its own: plain addresses as arguments
    fn = L.dd_op_conv_gemm_plan
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_void_p], C.c_int
    n = rows.shape[0]
    p = np.zeros(n, dtype=np.dtype(ConvGemmParams))
    for name in ("B", "H", "W", "Ho", "Wo", "stride", "shift", "parity", "cin", "ntaps", "M", "N", "K", "ksplit", "flags", "force_small",
                 "wgroup_rows", "x_ld", "y_ld", "res_ld", "raw_ld", "rowpart_ld"):
        p[name] = rows[:, COL[name]]
    p["alpha"] = rows[:, COL["alpha_q"]] / 4.0
    flags, drop = rows[:, COL["flags"]], rows[:, COL["drop"]]
    for name in ("x", "w", "taptab", "y"):
        p[name] = _NOT_READ
    for name, f in _PTR_FLAG:
        p[name] = np.where(flags & f, _NOT_READ, 0)
    p["mask_ld"] = np.where(flags & MASK, rows[:, COL["y_ld"]], 0)
    p["stats"] = np.where((flags & STATS != 0) & (drop & DROP_STATS == 0), _NOT_READ, 0)
    p["stats_ld"] = np.where(flags & STATS, rows[:, COL["y_ld"]], 0)
    p["rowpart"] = np.where((flags & ROWSTATS != 0) & (drop & DROP_ROWPART == 0), _NOT_READ, 0)
    ln = np.where((flags & LNFOLD != 0) & (drop & DROP_LN == 0), _NOT_READ, 0)
    p["ln_stats"], p["ln_c1"] = ln, ln
    p["bias_sel"] = np.where(rows[:, COL["bias_sel"]], _NOT_READ, 0)
    scratch = rows[:, COL["scratch"]]
    p["partial"] = np.where(scratch, _NOT_READ, 0)
    mn = np.maximum(rows[:, COL["M"]], 0) * np.maximum(rows[:, COL["N"]], 0) * 4
    caps = (np.where(scratch == 1, 16, np.where(scratch == 2, 2, 0)) * mn).tolist()
    out = np.zeros((n, 4), dtype=np.int32)
    out[:, 0] = -1
    a0, o0, step = p.ctypes.data, out.ctypes.data, p.dtype.itemsize
    for i, cap in enumerate(caps):
        fn(a0 + i * step, cap, o0 + i * 16)
    return out.astype(np.int16)


def describe(rows, i):
    return ", ".join("%s=%d" % (n, rows[i, COL[n]]) for n in FIELDS)
