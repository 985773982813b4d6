"""Records the bits of the flash attention kernels (attn_fwd_kernel, attn_fwd_dma_kernel, attn_fwd_shortk_kernel, attn_delta_kernel,
attn_bwd_dq_kernel, attn_bwd_dkv_kernel: every instantiation the planner can reach below 3.7 GB of K / V, every path of their tile loops)
of ONE build, for both storage formats, as tests/golden/attention_bits.npz; tests/test_attention_bits_gpu.py replays the same calls on the
current build and compares.

    DD_LIB=ab/parent.so DD_LIB_F16=ab/parent_f16.so python tests/golden/make_attention_bits.py      # needs a GPU
    python tests/golden/make_attention_bits.py --plan                                               # no GPU: plans and preconditions only

Run it on a build of the commit BEFORE a change to these kernels (PARENT below; both libraries of that build, loaded with DD_LIB and
DD_LIB_F16), never on the code under test and never to make a failing test pass.  It runs every case twice and refuses to write if the
two runs differ.

Inputs come from a closed integer formula (lattice(): uint32 arithmetic on the element index and a per-tensor constant, no library
generator): unscaled q, k, v and dO are multiples of 1/16 in [-2, 2) with scale = 1 / sqrt(D); a prescaled q is multiples of 1/64 in
[-1/2, 1/2) with scale = ln 2 -- all exact in bf16 and in half.  The file holds, per library and output buffer (O, LSE, and for the
backward cases dQ, dK, dV), the SHA-256 of its raw bytes.  Every output buffer is pre-filled with NaN and hashed whole, and every row
stride is H * D + 8 elements, so an element that is not written, or one written into the 8 padding columns, shows.  Each case first
asserts (ops._attention_plan) route, tile form, waves and the lazy / prescaled / causal / fp8 flags the planner gives it.

Shapes: the smallest that still reach each instantiation and each path; the comments of CASES say which.  The runaway cases set column 0
of q to 12 and column 0 of key j to 0.75 * (j // 16): every row's maximum then lies more than 2^64 above its first tile's (asserted on
the CPU), the optimistic sweep of the lazy kernel is rejected and the safe sweep rebases."""
import hashlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "attention_bits.npz")
PARENT = "51fd84f"          # the commit whose build made the record
LIBS = ("bf16", "fp16")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# forward tile forms (qt, kt) and backward (dq_qt, dq_kt, ktw, qtl) per head dim: csrc/attention_dispatch.h, ATTN_FORMS
FWD_FORM = {32: (2, 64), 40: (2, 64), 64: (2, 64), 80: (2, 64), 160: (2, 64), 512: (4, 32)}
BWD_FORM = {32: (2, 64, 2, 64), 40: (2, 64, 2, 64), 64: (2, 64, 2, 64), 80: (1, 64, 1, 64), 160: (1, 64, 1, 64), 512: (1, 32, 1, 32)}

# (name, B, H, Nq, Nk, D, flags, forward route, waves).  flags: p prescaled q, c causal, 8 pv_fp8, n no_shortk, r runaway scores,
# b backward too, x backward without dK / dV
CASES = [
    ("dma_d40_nw8_lazy", 1, 2, 256, 200, 40, "p", "dma", 8),                 # ONES; first tile, full tiles, 8-key ragged tile
    ("dma_d40_nw4_lazy_ragged_q", 2, 2, 200, 128, 40, "p", "dma", 4),        # rows past Nq, no ragged tile
    ("dma_d40_nw8_online", 1, 2, 256, 200, 40, "", "dma", 8),                # non-lazy branch with ONES
    ("dma_d40_one_partial_tile", 1, 2, 128, 77, 40, "pn", "dma", 4),         # nfull == 0
    ("dma_d32_nw8_lazy", 1, 2, 256, 96, 32, "p", "dma", 8),                  # one MFMA per score tile, shuffled row sum
    ("dma_d32_nw4_online", 1, 2, 96, 96, 32, "", "dma", 4),
    ("dma_d64_lazy", 1, 2, 200, 200, 64, "p", "dma", 4),                     # 160-byte rows
    ("dma_d64_online", 1, 2, 200, 200, 64, "", "dma", 4),
    ("dma_d80_lazy", 1, 2, 128, 150, 80, "p", "dma", 4),                     # KS = 3, no ONES
    ("dma_d80_online", 1, 2, 128, 150, 80, "", "dma", 4),
    ("dma_d40_runaway", 1, 2, 256, 256, 40, "pr", "dma", 8),                 # optimistic sweep rejected, safe sweep with rebase
    ("dma_d80_runaway", 1, 2, 128, 256, 80, "pr", "dma", 4),
    ("fp8_d64", 1, 2, 256, 200, 64, "8", "dma", 8),                          # bf16 library only
    ("fp8_d64_one_tile", 1, 2, 256, 77, 64, "8", "dma", 8),
    ("stream_d160", 1, 2, 100, 150, 160, "", "stream", 4),                   # register-staged, prefetch, ragged both ways
    ("stream_d512", 1, 1, 80, 80, 512, "", "stream", 4),                     # DSPLIT 4, direct staging, 32-key tiles
    ("stream_causal_d64", 1, 2, 130, 130, 64, "c", "stream", 4),
    ("stream_causal_d40", 1, 2, 100, 100, 40, "c", "stream", 4),             # causal mask with ONES
    ("bwd_d40", 1, 2, 200, 150, 40, "b", "dma", 4),                          # dQ and dK/dV, ragged keys and queries
    ("bwd_d40_ps", 1, 2, 200, 150, 40, "bp", "dma", 4),
    ("bwd_d32_ps", 1, 2, 100, 100, 32, "bp", "dma", 4),
    ("bwd_d64", 1, 2, 100, 100, 64, "b", "dma", 4),
    ("bwd_d80_ps", 1, 2, 100, 100, 80, "bp", "dma", 4),
    ("bwd_d160", 1, 2, 100, 100, 160, "b", "stream", 4),
    ("bwd_d512_ps", 1, 1, 80, 80, 512, "bp", "stream", 4),                   # DSPLIT 4
    ("bwd_cross_d40", 1, 2, 128, 77, 40, "x", "shortk", 8),                  # dQ alone
    ("shortk_d40", 1, 2, 512, 77, 40, "", "shortk", 8),                      # kfull 4
    ("shortk_d40_full", 1, 2, 512, 80, 40, "", "shortk", 8),                 # kfull 5
    ("shortk_d40_one_key", 1, 2, 512, 1, 40, "", "shortk", 8),               # kfull 0
    ("shortk_d64_one_tile", 2, 2, 32, 16, 64, "p", "shortk", 4),
    ("shortk_d80", 1, 4, 96, 65, 80, "", "shortk", 4),
    # the Q ring and the counted waits: by the planner's arithmetic the smallest B * H that leaves two tiles per wave (about 170 MB)
    ("shortk_d40_two_tiles_per_wave", 16, 8, 4096, 77, 40, "p", "shortk", 8),
]
NAMES = [c[0] for c in CASES]


def cases_of(lib):
    return [c[0] for c in CASES if lib == "bf16" or "8" not in c[6]]


def lattice(shape, salt):
    """integers in [-32, 32) from the element index and `salt`"""
    h = np.arange(int(np.prod(shape)), dtype=np.uint32) * np.uint32(2654435761) + np.uint32((salt * 40503 + 977) & 0xffffffff)
    h ^= h >> np.uint32(15)
    h *= np.uint32(2246822519)
    h ^= h >> np.uint32(13)
    return torch.from_numpy((((h >> np.uint32(7)) & np.uint32(63)).astype(np.int32) - 32).astype(np.float32).reshape(shape))


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


_inputs = {}


def inputs(name):
    """fp32 q, k, v, dO [rows, H * D + 8] of case `name` (the last case's are kept: both libraries replay it)"""
    if name not in _inputs:
        _inputs.clear()
        _, B, H, Nq, Nk, D, fl, _, _ = CASES[NAMES.index(name)]
        salt, ld = NAMES.index(name) * 8, H * D + 8
        q = lattice((B * Nq, ld), salt) / (64 if "p" in fl else 16)
        k, v, do = lattice((B * Nk, ld), salt + 1) / 16, lattice((B * Nk, ld), salt + 2) / 16, lattice((B * Nq, ld), salt + 3) / 16
        if "r" in fl:
            q[:, 0:H * D:D] = 12.0
            k[:, 0:H * D:D] = (0.75 * (torch.arange(B * Nk) % Nk // 16).float())[:, None]
            # CPU-side precondition: every row's maximum lies more than 64 (log2 domain: q is prescaled) above that of its first 64 keys
            for h in range(H):
                s = q[:Nq, h * D:(h + 1) * D].double() @ k[:Nk, h * D:(h + 1) * D].double().T
                assert ((s.max(dim=1).values - s[:, :64].max(dim=1).values) > 64).all(), name
        _inputs[name] = (q, k, v, do)
    return _inputs[name]


def check_plan(name, plan, bwd):
    _, B, H, Nq, Nk, D, fl, route, waves = CASES[NAMES.index(name)]
    what = "%s (%s): the planner gives %r" % (name, "backward" if bwd else "forward", plan)
    if bwd:
        dq_qt, dq_kt, ktw, qtl = BWD_FORM[D]
        dkv = "b" in fl
        assert plan["route"] == "flash_bwd" and plan["d"] == D and plan["waves"] == 4 and plan["dsplit"] == (4 if D == 512 else 1), what
        assert (plan["qt"], plan["kt"], plan["ktw"], plan["qtl"]) == (dq_qt, dq_kt, ktw if dkv else 0, qtl if dkv else 0), what
        assert plan["prescaled"] == ("p" in fl) and len(plan["launches"]) == (3 if dkv else 2), what
        return
    assert plan["route"] == route and plan["d"] == D and plan["waves"] == waves, what
    assert plan["lazy"] == (route == "dma" and ("p" in fl or "8" in fl)) and plan["fp8"] == ("8" in fl), what
    assert plan["causal"] == ("c" in fl and route == "stream"), what
    if route == "shortk":
        # the planner's arithmetic (attention_plan): workgroups per (image, head), at most 8 tiles per wave while the chip stays full
        sk_tiles, per = Nq // 32, 8
        wgs = -(-sk_tiles // waves)
        while per > 1 and -(-wgs // per) * H * B < 1024:
            per >>= 1
        sk_wgs = -(-wgs // per)
        assert plan["launches"][0][0] == ((B * sk_wgs + 7) & ~7) * H, what
        # the last case alone has more tiles than waves (every wave walks two: the Q ring, the counted waits)
        assert (sk_wgs * waves < sk_tiles) == (name == "shortk_d40_two_tiles_per_wave"), what
    else:
        assert (plan["qt"], plan["kt"]) == ((2, 128) if "8" in fl else FWD_FORM[D]) and plan["dsplit"] == (4 if D == 512 else 1), what


def replay(ops, name, lib="bf16", plan_only=False):
    """Case `name` on the `lib` library ops uses -> {"<lib>/<name>/<output>": sha256 hex} (plan_only: {} after the plan checks, nothing
    touches a device)."""
    from distdiff_amd._lib import AttnParams, check
    _, B, H, Nq, Nk, D, fl, _, _ = CASES[NAMES.index(name)]
    dt, dev = DTYPES[lib], "cpu" if plan_only else "cuda"
    q, k, v, do = (t.to(dt).to(dev) for t in inputs(name))
    ld = H * D + 8
    nan = lambda shape, dtype=dt: torch.full(shape, float("nan"), dtype=dtype, device=dev)
    outs = {"o": nan((B * Nq, ld)), "lse": nan((B, H, Nq), torch.float32)}
    p = AttnParams()
    p.q, p.k, p.v, p.o, p.lse = ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(outs["o"]), ops._ptr(outs["lse"])
    p.ldq = p.ldk = p.ldv = p.ldo = ld
    p.B, p.H, p.Nq, p.Nk, p.D = B, H, Nq, Nk, D
    p.scale = math.log(2.0) if "p" in fl else 1.0 / math.sqrt(D)
    p.q_prescaled, p.causal, p.pv_fp8, p.no_shortk = int("p" in fl), int("c" in fl), int("8" in fl), int("n" in fl)
    check_plan(name, ops._attention_plan(p, 0, False, dt), False)
    L = ops._L(dt)
    if not plan_only:
        check(L.dd_op_attention_fwd(ops.C.byref(p), ops._stream()), "attn_fwd")
    if "b" in fl or "x" in fl:
        outs["dq"] = nan((B * Nq, ld))
        delta = torch.empty((B, H, Nq), dtype=torch.float32, device=dev)
        p.d_o, p.dq, p.delta, p.lddo, p.lddq = ops._ptr(do), ops._ptr(outs["dq"]), ops._ptr(delta), ld, ld
        if "b" in fl:
            outs["dk"], outs["dv"] = nan((B * Nk, ld)), nan((B * Nk, ld))
            p.dk, p.dv, p.lddk, p.lddv = ops._ptr(outs["dk"]), ops._ptr(outs["dv"]), ld, ld
        check_plan(name, ops._attention_plan(p, 0, True, dt), True)
        if not plan_only:
            check(L.dd_op_attention_bwd(ops.C.byref(p), ops._stream()), "attn_bwd")
    if plan_only:
        return {}
    torch.cuda.synchronize()
    for n, t in outs.items():        # every element of the head columns is written and finite, the padding columns keep their NaN
        assert torch.isfinite(t if n == "lse" else t[:, :H * D]).all() and (n == "lse" or torch.isnan(t[:, H * D:]).all()), (lib, name, n)
    return {"%s/%s/%s" % (lib, name, n): digest(t) for n, t in outs.items()}


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from distdiff_amd import _lib, ops
    plan_only = "--plan" in sys.argv
    assert plan_only or (os.environ.get("DD_LIB") and os.environ.get("DD_LIB_F16")), "record from a build of %s: set DD_LIB and DD_LIB_F16" % PARENT
    got = {}
    for lib in LIBS:
        for name in cases_of(lib):
            first = replay(ops, name, lib, plan_only)
            if not plan_only:
                assert replay(ops, name, lib) == first, "the build is not deterministic on %s (%s)" % (name, lib)
            got.update(first)
            print("ok" if plan_only else len(first), lib, name, flush=True)
    if plan_only:
        return
    names = sorted(got)
    np.savez_compressed(PATH, parent_commit=np.array(PARENT), case_names=np.array(names), case_sha256=np.array([got[n] for n in names]))
    print("wrote %s: %d outputs, %d bytes, libraries %s %s" % (PATH, len(names), os.path.getsize(PATH), _lib.LIB_PATH, _lib.LIB_PATH_F16))


if __name__ == "__main__":
    main()
