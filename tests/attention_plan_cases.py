"""Deterministic problems for the attention launcher's decision (dd_op_attention_plan: which route, which tile form, which flags, how many
images per GEMM group, and grid / block / dynamic LDS of every launch; or the refusal).  The planner only tests pointers for null and
reads no device, so the whole table is answered on a CPU.

blocks() yields (name, rows): rows is an int64 array with one problem per row, columns FIELDS.  Pointers are not fields: q, k, v, o are
always present; lse and delta unless `drop` removes them; d_o, dq (and dk, dv when `dkv` is set) in backward problems.  `ws_images` is the
scratch offered, in units of dd_op_attention_gemm_workspace(Nq, Nk, D, bwd) (0: none -- what the engine passes for a cross-attention op).
scale = ln 2 for a prescaled problem, else 1 / sqrt(D).

Not in the grid: backward problems with scratch but without dk / dv.  The engine never issues them (self-attention always wants dk / dv,
cross-attention gets no scratch); the planner sends them to the flash kernels.

tests/golden/make_attention_plan_table.py records the outcomes, tests/test_attention_plan_table.py compares a build against the record.
"""
import ctypes as C
import hashlib

import numpy as np

FIELDS = ("B", "H", "Nq", "Nk", "D", "causal", "prescaled", "fp8", "no_shortk", "bwd", "dkv", "ws_images", "drop",
          "ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv")
COL = {n: i for i, n in enumerate(FIELDS)}
DROP_LSE, DROP_DELTA = 1, 2

# the outcome of one problem (int32): OUT_FIELDS, then (grid x, y, z, block, dynamic LDS bytes) of up to three launches.  A refusal is
# route -1 and zeros.  The GEMM route reports route and group only (its launches are the conv planner's business).
OUT_FIELDS = ("route", "d", "qt", "kt", "dsplit", "ktw", "qtl", "waves", "bits", "group", "launches")
OCOL = {n: i for i, n in enumerate(OUT_FIELDS)}
OUT_N = len(OUT_FIELDS) + 15
ROUTE_GEMM, ROUTE_SHORTK, ROUTE_DMA, ROUTE_STREAM, ROUTE_FLASH_BWD = 0, 1, 2, 3, 4
ROUTES = ("gemm", "shortk", "dma", "stream", "flash_bwd")
BIT_LAZY, BIT_PRESCALED, BIT_CAUSAL, BIT_FP8 = 1, 2, 4, 8      # prescaled: the backward's PS instantiations

DS = (32, 40, 48, 64, 80, 160, 256, 512)
NS = (1, 16, 31, 32, 50, 64, 77, 80, 81, 96, 200, 256, 1024, 2304, 4096, 9216)
HS = (1, 8)
BS = (1, 2, 9)
FWD_FLAGS = ((), ("causal",), ("prescaled",), ("fp8",), ("no_shortk",), ("prescaled", "no_shortk"), ("prescaled", "fp8"), ("causal", "prescaled"),
             ("causal", "fp8"))
BWD_FLAGS = (("dkv",), ("dkv", "prescaled"), (), ("prescaled",))


def _product(*axes):
    g = np.meshgrid(*[np.asarray(a, dtype=np.int64) for a in axes], indexing="ij")
    return [x.reshape(-1) for x in g]


def _rows(B, H, Nq, Nk, D, flags=(), bwd=0, ws_images=0, qkv_ld=1):
    """Contiguous outputs and gradients; q, k, v rows qkv_ld * H * D wide (3: column views of a fused projection)"""
    n = B.shape[0]
    r = np.zeros((n, len(FIELDS)), dtype=np.int64)
    for name, v in (("B", B), ("H", H), ("Nq", Nq), ("Nk", Nk), ("D", D), ("bwd", bwd), ("ws_images", ws_images)):
        r[:, COL[name]] = v
    for f in flags:
        r[:, COL[f]] = 1
    c = H * D
    for name in ("ldq", "ldk", "ldv"):
        r[:, COL[name]] = qkv_ld * c
    r[:, COL["ldo"]] = c
    if bwd:
        r[:, COL["lddo"]] = c
        r[:, COL["lddq"]] = qkv_ld * c
        r[:, COL["lddk"]] = np.where(r[:, COL["dkv"]], qkv_ld * c, 0)
        r[:, COL["lddv"]] = r[:, COL["lddk"]]
    return r


def _set(rows, **kw):
    r = rows.copy()
    for k, v in kw.items():
        r[:, COL[k]] = v
    return r


def _tag(flags):
    return "+".join(flags) if flags else "plain"


def _base(bwd):
    """A small spread that reaches every route, for the variations the grid lacks"""
    B, H, Nq, Nk, D = _product((2,), HS, (64, 256, 4096), (77, 256, 4096), (40, 64, 160, 512))
    out = [_rows(B, H, Nq, Nk, D, fl, bwd) for fl in ((("dkv",), ("dkv", "prescaled")) if bwd else ((), ("prescaled",), ("fp8",)))]
    out.append(_rows(B, H, Nq, Nk, D, ("dkv",) if bwd else (), bwd, ws_images=8))
    return np.concatenate(out)


def _engine():
    """The attention ops the model builders produce: (B, H, Nq, Nk, D, flags, self-attention (scratch offered, dk / dv wanted))"""
    ops = []
    for B in (2, 32, 64):
        for heads, ds, toks in ((8, (40, 80, 160, 160), (4096, 1024, 256, 64)),):                       # SD-1.5, 64 x 64 latents
            for d, n in zip(ds, toks):
                ops += [(B, heads, n, n, d, ("prescaled",), 1), (B, heads, n, 77, d, ("prescaled",), 0)]
        for heads, n in ((5, 4096), (10, 1024), (20, 256), (20, 64), (10, 4096), (20, 1024)):            # SD-2.x and SDXL: d = 64
            ops += [(B, heads, n, n, 64, ("prescaled",), 1), (B, heads, n, 77, 64, ("prescaled",), 0), (B, heads, n, n, 64, ("prescaled", "fp8"), 1)]
    for B in (1, 2, 8, 9, 32):
        for px in (512, 384, 640, 768):                                                                  # AutoencoderKL mid block
            ops.append((B, 1, (px // 8) ** 2, (px // 8) ** 2, 512, (), 1))
    for B in (1, 2):
        for heads in (12, 16, 20):                                                                       # CLIP text towers: causal 77 x 77
            ops.append((B, heads, 77, 77, 64, ("causal",), 1))
    for B in (1, 32):
        ops.append((B, 12, 50, 50, 64, (), 1))                                                           # ViT guide
    return ops


ENGINE_OPS = _engine()


def _engine_rows(bwd):
    out = []
    for B, H, Nq, Nk, D, flags, self_attn in ENGINE_OPS:
        if bwd and "causal" in flags:
            continue                                                                                     # the text towers run forward only
        one = [np.asarray([x], dtype=np.int64) for x in (B, H, Nq, Nk, D)]
        fl = tuple(f for f in flags if not (bwd and f == "fp8")) + (("dkv",) if bwd and self_attn else ())
        for ws in ((0, min(B, 8)) if self_attn else (0,)):
            out.append(_rows(*one, fl, bwd, ws_images=ws, qkv_ld=3 if self_attn else 1))
    return np.concatenate(out)


def _ld_edge(n, d):
    """The row stride (a multiple of 8) at which n rows reach 0xF0000000 bytes, plus d"""
    edge = (0xF0000000 // 2 + n - 1) // n
    return np.maximum((edge + 7) // 8 * 8 + d, 8)


def blocks():
    grid = _product(BS, HS, NS, NS, DS)
    for fl in FWD_FLAGS:
        yield "fwd_" + _tag(fl), _rows(*grid, fl)
    for fl in BWD_FLAGS:
        yield "bwd_" + _tag(fl), _rows(*grid, fl, 1)
    # row strides wider than the heads (column views)
    yield "fwd_wide", _rows(*grid, (), qkv_ld=3)
    yield "fwd_wide_prescaled", _rows(*grid, ("prescaled",), qkv_ld=3)
    yield "bwd_wide", _rows(*grid, ("dkv",), 1, qkv_ld=3)
    # scratch for one image and for eight
    for ws in (1, 8):
        yield "fwd_ws%d" % ws, _rows(*grid, (), 0, ws)
        yield "fwd_ws%d_causal" % ws, _rows(*grid, ("causal",), 0, ws)
        yield "fwd_ws%d_wide" % ws, _rows(*grid, (), 0, ws, qkv_ld=3)
        yield "bwd_ws%d" % ws, _rows(*grid, ("dkv",), 1, ws)
    for bwd in (0, 1):
        b = _base(bwd)
        d = "bwd" if bwd else "fwd"
        c = COL
        # one misaligned stride at a time (& 7; & 3 is what the flash kernels ask of o, dq, dk, dv)
        for name in ("ldq", "ldk", "ldv", "ldo") + (("lddo", "lddq", "lddk", "lddv") if bwd else ()):
            for add in (4, 2):
                yield "%s_%s+%d" % (d, name, add), _set(b, **{name: b[:, c[name]] + add})
        # key / value rows (and the short-key kernel's query rows) at the end of the 32-bit byte offsets of one image
        for add in (-8, 0, 8):
            yield "%s_ldk_edge%+d" % (d, add), _set(b, ldk=_ld_edge(b[:, c["Nk"]], add))
            yield "%s_ldv_edge%+d" % (d, add), _set(b, ldv=_ld_edge(b[:, c["Nk"]], add))
            yield "%s_ldq_edge%+d" % (d, add), _set(b, ldq=_ld_edge(b[:, c["Nq"]], add))
        yield d + "_no_lse", _set(b, drop=DROP_LSE)
        if bwd:
            yield "bwd_no_delta", _set(b, drop=DROP_DELTA)
        yield d + "_engine", _engine_rows(bwd)


def cases_hash(blks):
    h = hashlib.sha256(repr(FIELDS).encode())
    for name, rows in blks:
        h.update(name.encode())
        h.update(np.ascontiguousarray(rows, dtype="<i8").tobytes())
    return h.hexdigest()


_NOT_READ = 1 << 12       # stands for a buffer: the planner tests pointers for null and never follows them


def evaluate(lib_path, rows):
    """The outcome of every row as an int32 [n, OUT_N] array (see OUT_FIELDS)"""
    from distdiff_amd._lib import AttnParams
    L = C.CDLL(lib_path)                                         # a handle of its own: plain addresses as arguments
    fn, wsf = L.dd_op_attention_plan, L.dd_op_attention_gemm_workspace
    fn.argtypes, fn.restype = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p], C.c_int
    wsf.argtypes, wsf.restype = [C.c_int] * 4, C.c_size_t
    n = rows.shape[0]
    p = np.zeros(n, dtype=np.dtype(AttnParams))
    for name in ("B", "H", "Nq", "Nk", "D", "causal", "no_shortk", "ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv"):
        p[name] = rows[:, COL[name]]
    p["q_prescaled"], p["pv_fp8"] = rows[:, COL["prescaled"]], rows[:, COL["fp8"]]
    p["scale"] = np.where(rows[:, COL["prescaled"]], 0.6931471805599453, 1.0 / np.sqrt(rows[:, COL["D"]]))
    bwd, drop = rows[:, COL["bwd"]], rows[:, COL["drop"]]
    for name in ("q", "k", "v", "o"):
        p[name] = _NOT_READ
    p["lse"] = np.where(drop & DROP_LSE, 0, _NOT_READ)
    p["delta"] = np.where((bwd == 0) | (drop & DROP_DELTA != 0), 0, _NOT_READ)
    p["d_o"] = p["dq"] = np.where(bwd, _NOT_READ, 0)
    p["dk"] = p["dv"] = np.where(rows[:, COL["dkv"]], _NOT_READ, 0)
    out = np.zeros((n, OUT_N), dtype=np.int32)
    a0, o0, step = p.ctypes.data, out.ctypes.data, p.dtype.itemsize
    key = rows[:, [COL["Nq"], COL["Nk"], COL["D"], COL["bwd"]]]
    per = {tuple(k): wsf(*k) for k in np.unique(key, axis=0).tolist()}
    for i, (k, w, b) in enumerate(zip(key.tolist(), rows[:, COL["ws_images"]].tolist(), bwd.tolist())):
        fn(a0 + i * step, per[tuple(k)] * w, b, o0 + i * 4 * OUT_N)
    return out


def describe(rows, i):
    return ", ".join("%s=%d" % (n, rows[i, COL[n]]) for n in FIELDS)
