"""Records the bits of the norm kernels (norm.hip: gn_partial_kernel, the two finalize kernels, gn_finalize_chan_kernel, gn_apply_kernel,
ln_rows_kernel, the LayerNorm backward, ln_rowpart_finalize_kernel: every path of their launch arithmetic) of ONE build, for both storage
formats, as tests/golden/norm_bits.npz; tests/test_norm_bits_gpu.py replays the same calls on the current build and compares.

    DD_LIB=ab/parent.so DD_LIB_F16=ab/parent_f16.so python tests/golden/make_norm_bits.py      # needs a GPU
    python tests/golden/make_norm_bits.py --cases                                               # no GPU: inputs and the path of every case

Run it on a build of the commit BEFORE a change to these kernels (PARENT below; both libraries of that build, made outside git with
DD_BUILD_OBJ / DD_BUILD_LIB and loaded with DD_LIB and DD_LIB_F16), never on the code under test and never to make a failing test pass.
It runs every case twice and refuses to write if the two runs differ.

Calls go through ops.groupnorm, ops.layernorm and ops.layernorm_stats; the library follows the tensor dtype.  Inputs come from the closed
integer formula of the other records (make_pingpong_bits.lattice): x, dy and prev are multiples of 1/16 in [-2, 2), gamma and beta
multiples of 1/64 in [-1/2, 1/2) -- all exact in bf16 and in half.  Channel partials (norm_ref.chan_partials) and row partials are
computed from those inputs in float64 on the CPU and rounded to fp32.  The file holds the SHA-256 of every input tensor (as fp32, on the
CPU: the test compares these first, so a generator difference reads as "inputs differ" and not as a kernel change) and, per library and
output buffer, the SHA-256 of its raw bytes.  y, dx and dx with `accumulate` on top of prev are column views (column offsets 8 and 32) of
wider buffers pre-filled with NaN, the statistics the head of a longer NaN-filled buffer; each is hashed whole, so an element that is not
written, or one written beside the view, shows.  x and dy are column views too (row strides C + 24, C + 40 against C + 16, C + 56 of y,
dx), the channel partials a view with part_ld = C + 16, the row partials one with rowpart_ld = spans + 3.  The statistics-only forward
returns its own buffer, which is hashed as it is.

Shapes: the tables of tests/norm_ref.py (the smallest that reach each path; the comments there say which), without their input kinds.
paths() is a Python mirror of the launch arithmetic of norm.hip; tests/test_norm_bits_cases.py asserts on the CPU that the table as a
whole reaches every path."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import norm_ref as nr  # noqa: E402
from make_pingpong_bits import digest, lattice, nan  # noqa: E402

PATH = os.path.join(HERE, "norm_bits.npz")
PARENT = "6266c73"          # the commit whose build made the record
LIBS = ("bf16", "fp16")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ROWPART_M, ROWPART_C = 300, 320

# (name, kind, shape).  gn: forward, backward, backward-accumulate; part: forward from channel partials; ln: forward, statistics-only
# forward, backward, backward-accumulate; rowpart: statistics from row partials.  gn / part shapes (C, G, HW, B, eps, silu), ln (C, M)
CASES = [("gn_" + n, "gn", c[:6]) for n, c in nr.GN_CASES.items()] + [("gn_gridcap", "gn", nr.GRIDCAP)]
CASES += [("part_" + n, "part", c[:6]) for n, c in nr.PART_CASES.items()]
CASES += [("ln_C%d_M%d" % cm, "ln", cm) for cm in dict.fromkeys(c[:2] for c in nr.LN_CASES)]
CASES += [("rowpart_spans%d" % s, "rowpart", (ROWPART_C, ROWPART_M, s)) for s in (1, 4, 8, 16)]
NAMES = [c[0] for c in CASES]

GN_THREADS, APPLY_TOTAL, CHAN_MAXP, LN_RPW = 256, 4096, 12 * 256, 4


def paths(name):
    """The path case `name` takes, from the launch arithmetic of norm.hip (gn_launch, gn_split, gn_apply_blocks, gn_finalize_chan_kernel,
    launch_layernorm_fwd)."""
    _, kind, shape = CASES[NAMES.index(name)]
    if kind in ("gn", "part"):
        C, G, HW, B = shape[:4]
        VC, cpg = C // 8, C // G
        VCt = min(VC, GN_THREADS)
        R = GN_THREADS // VCt
        want = max((HW * VC + GN_THREADS * 8 - 1) // (GN_THREADS * 8), 1)
        cap = APPLY_TOTAL // B + 1
        d = dict(kind=kind, VC=VC, VCt=VCt, R=R, idle=GN_THREADS - R * VCt, second_sweep=VC > VCt, cpg=cpg, straddle=cpg % 8 != 0 and 8 % cpg != 0,
                 apply_wanted=want, apply_allowed=cap, apply_capped=want > cap)
        if kind == "part":
            d.update(P=(HW // 64) * cpg, P_in_registers=(HW // 64) * cpg <= CHAN_MAXP)
        else:
            S = nr.gn_split(HW, C)
            rows_per = (HW + S - 1) // S
            rows = [max(min(HW, (s + 1) * rows_per) - s * rows_per, 0) for s in range(S)]
            d.update(S=S, rows_per=rows_per, ragged=sum(0 < r < rows_per for r in rows), empty=sum(r == 0 for r in rows),
                     S_capped=S == nr.GN_MAX_SPLIT and (HW + max(32768 // C, 4) - 1) // max(32768 // C, 4) > S, R_over_rows=R > rows_per)
        return d
    if kind == "ln":
        C, M = shape
        VC = C // 8
        return dict(kind=kind, VC=VC, VI=(VC + 63) // 64, idle_lanes=64 * ((VC + 63) // 64) - VC, M=M, row_tail=M % (4 * LN_RPW),
                    blocks=(M + 4 * LN_RPW - 1) // (4 * LN_RPW))
    C, M, spans = shape
    return dict(kind=kind, spans=spans, M=M, blocks=(M + 255) // 256, row_tail=M % 256)


_inputs = {}


def inputs(name):
    """fp32 CPU inputs of case `name` as a dict (the last case's are kept: both libraries replay it)"""
    if name not in _inputs:
        _inputs.clear()
        i = NAMES.index(name)
        _, kind, shape = CASES[i]
        salt = i * 8
        if kind in ("gn", "part"):
            C, G, HW, B = shape[:4]
            I = dict(x=lattice((B * HW, C), salt) / 16, gamma=lattice((C,), salt + 3) / 64, beta=lattice((C,), salt + 4) / 64)
            if kind == "gn":
                I.update(dy=lattice((B * HW, C), salt + 1) / 16, prev=lattice((B * HW, C), salt + 2) / 16)
            else:
                I["chan_part"] = nr.chan_partials(I["x"].view(B, HW, C)).float()
        elif kind == "ln":
            C, M = shape
            I = dict(x=lattice((M, C), salt) / 16, dy=lattice((M, C), salt + 1) / 16, prev=lattice((M, C), salt + 2) / 16,
                     gamma=lattice((C,), salt + 3) / 64, beta=lattice((C,), salt + 4) / 64)
        else:
            C, M, spans = shape
            x = lattice((M, C), salt) / 16
            xs = x.double().view(M, spans, C // spans)
            I = dict(x=x, rowpart=torch.stack([xs.sum(2), (xs * xs).sum(2)], -1).float())
        _inputs[name] = I
    return _inputs[name]


def input_digests(name):
    I = inputs(name)
    if "digests" not in I:              # kept with the inputs: hashed once for both libraries
        I["digests"] = {"%s/%s" % (name, k): digest(v) for k, v in I.items()}
    return I["digests"]


def _view(t, extra, off, dt):
    """fp32 CPU [rows, C] -> a device column view at column `off` of a zero buffer with ld = C + extra"""
    rows, C = t.shape
    buf = torch.zeros((rows, C + extra), dtype=dt, device="cuda")
    v = buf[:, off:off + C]
    v.copy_(t.to(dt))
    return v


def _out(rows, C, extra, off, dt, fill=None):
    """a NaN buffer with ld = C + extra and its column view at `off` (holding `fill`, if given) -> (view, buffer)"""
    buf = nan((rows, C + extra), dt)
    v = buf[:, off:off + C]
    if fill is not None:
        v.copy_(fill.to(dt))
    return v, buf


def _stats(n):
    """a NaN buffer of 2 n + 16 floats and its head [n, 2] -> (head, buffer)"""
    buf = nan((2 * n + 16,), torch.float32)
    return buf[:2 * n].view(n, 2), buf


def replay(ops, name, lib="bf16"):
    """Case `name` on the `lib` library ops uses -> {"<lib>/<name>/<output>": sha256 hex}"""
    _, kind, shape = CASES[NAMES.index(name)]
    dt, I, outs, views = DTYPES[lib], inputs(name), {}, []
    if kind in ("gn", "part"):
        C, G, HW, B, eps, silu = shape
        rows = B * HW
        x, ga, be = _view(I["x"], 24, 8, dt), I["gamma"].cuda(), I["beta"].cuda()
        y, outs["y"] = _out(rows, C, 16, 8, dt)
        st, outs["stats"] = _stats(B * G)
        st = st.view(B, G, 2)
        views += [(y, outs["y"], 8)]
        kw = {}
        if kind == "part":
            pbuf = nan((I["chan_part"].shape[0], C + 16, 2), torch.float32)
            pbuf[:, 8:8 + C] = I["chan_part"].cuda()
            kw["chan_part"] = pbuf[:, 8:8 + C]
        ops.groupnorm(x, ga, be, B, HW, G, eps, silu, y=y, stats=st, **kw)
        if kind == "gn":
            dy = _view(I["dy"], 40, 16, dt)
            dx, outs["dx"] = _out(rows, C, 56, 32, dt)
            acc, outs["dx_acc"] = _out(rows, C, 56, 32, dt, I["prev"])
            views += [(dx, outs["dx"], 32), (acc, outs["dx_acc"], 32)]
            ops.groupnorm(x, ga, be, B, HW, G, eps, silu, dy=dy, stats=st, dx=dx)
            ops.groupnorm(x, ga, be, B, HW, G, eps, silu, dy=dy, stats=st, accumulate_into=acc)
    elif kind == "ln":
        C, M = shape
        x, dy, ga, be = _view(I["x"], 24, 8, dt), _view(I["dy"], 40, 16, dt), I["gamma"].cuda(), I["beta"].cuda()
        y, outs["y"] = _out(M, C, 16, 8, dt)
        dx, outs["dx"] = _out(M, C, 56, 32, dt)
        acc, outs["dx_acc"] = _out(M, C, 56, 32, dt, I["prev"])
        st, outs["stats"] = _stats(M)
        views += [(y, outs["y"], 8), (dx, outs["dx"], 32), (acc, outs["dx_acc"], 32)]
        ops.layernorm(x, ga, be, nr.LN_EPS, y=y, stats=st)
        outs["stats_only"] = ops.layernorm_stats(x, nr.LN_EPS)
        ops.layernorm(x, ga, be, nr.LN_EPS, dy=dy, stats=st, dx=dx)
        ops.layernorm(x, ga, be, nr.LN_EPS, dy=dy, stats=st, accumulate_into=acc)
    else:
        C, M, spans = shape
        pbuf = nan((M, spans + 3, 2), torch.float32)
        pbuf[:, :spans] = I["rowpart"].cuda()
        outs["stats"] = ops.layernorm_stats(I["x"].to(dt).cuda(), nr.LN_EPS, rowpart=pbuf[:, :spans], spans=spans)
    torch.cuda.synchronize()
    for v, buf, off in views:          # every element of the view is written and finite, the padding columns keep their NaN
        assert torch.isfinite(v).all() and torch.isnan(buf[:, :off]).all() and torch.isnan(buf[:, off + v.shape[1]:]).all(), (lib, name)
    for k in ("stats", "stats_only"):
        if k in outs:
            t = outs[k].flatten()
            n = t.numel() - (16 if kind != "rowpart" and k == "stats" else 0)
            assert torch.isfinite(t[:n]).all() and torch.isnan(t[n:]).all(), (lib, name, k)
    return {"%s/%s/%s" % (lib, name, k): digest(v) for k, v in outs.items()}


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def _file_sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    if "--cases" in sys.argv:
        for name in NAMES:
            d = input_digests(name)
            print(name, " ".join("%s=%s" % kv for kv in paths(name).items()), "inputs:", " ".join("%s=%s" % (k.split("/")[1], v[:8]) for k, v in d.items()),
                  flush=True)
        return
    from distdiff_amd import _lib, ops
    assert os.environ.get("DD_LIB") and os.environ.get("DD_LIB_F16"), "record from a build of %s: set DD_LIB and DD_LIB_F16" % PARENT
    got, ins = {}, {}
    for name in NAMES:
        ins.update(input_digests(name))
        for lib in LIBS:
            first = replay(ops, name, lib)
            assert replay(ops, name, lib) == first, "the build is not deterministic on %s (%s)" % (name, lib)
            got.update(first)
            print(len(first), lib, name, flush=True)
    names, inames = sorted(got), sorted(ins)
    np.savez_compressed(PATH, parent_commit=np.array(PARENT), case_names=np.array(names), case_sha256=np.array([got[n] for n in names]),
                        input_names=np.array(inames), input_sha256=np.array([ins[n] for n in inames]),
                        library_sha256=np.array([_file_sha256(_lib.LIB_PATH), _file_sha256(_lib.LIB_PATH_F16)]))
    print("wrote %s: %d outputs, %d inputs, %d bytes, libraries %s %s" % (PATH, len(names), len(inames), os.path.getsize(PATH), _lib.LIB_PATH, _lib.LIB_PATH_F16))


if __name__ == "__main__":
    main()
