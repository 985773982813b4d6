"""Records the bits of the HBM-bound side kernels that exist for bf16 and for fp32 rows (add / copy, ReLU masks, 3x3 s2 max-pool, bicubic
resize, global pooling, NCHW -> NHWC; each with its transpose) of ONE build as tests/golden/side_kernel_bits.npz;
tests/test_side_kernel_bits_gpu.py replays the same calls on the current build and compares.

    python tests/golden/make_side_kernel_bits.py            # needs a GPU; DD_LIB=... records another build of the library

Run it on the build whose arithmetic is to be pinned (the commit BEFORE a change to these kernels), never to make a failing test pass.
Only dd_op_* symbols of ABI 9 are used.  The file holds the inputs themselves (not seeds; bf16 as uint16) and for every case the SHA-256
of the raw bytes of each output buffer.  Every output buffer is pre-filled with NaN (argmax: -1) and hashed whole, row padding included,
so an element that is not written, or one written outside the C columns, shows.

Shapes: the smallest at which each kernel can still go wrong (the grid-wrapping shapes are in tests/test_reverse_ops_gpu.py).
  rows     M = 37, C = 24 (bf16: 3 vectors) / 12 (fp32: 3 vectors), row strides C + 1, 2, 3 vectors; NaN, +-inf and -0 among the addends;
           masks drawn from 0, -0, 6, its two neighbours in the format, +inf and ordinary values; hi 0 (ReLU) and 6 (ReLU6) for fp32
  maxpool  B = 2, 6 x 10 -> 3 x 5, C = 16 / 8 (2 vectors): values from {0, 1, 2} so that most windows are tied (asserted), one NaN
  bicubic  16 x 16 -> 7 x 7 (the 512 -> 224 ratio) and 18 x 12 -> 8 x 5; B = 2, C = 3, Cpad = 8; rows of 8 (bf16) / 4 (fp32) elements
  gap      B = 3, HW = 49, C = 20: average (both formats), maximum + argmax on tied maxima (fp32); transposes with / without the
           ReLU mask (bf16) and the argmax (fp32)
  layout   B = 2, C = 3, 5 x 7, Cpad = 8, ld = 8: bf16 with dup 0 / 1 and scale 1 / 0.18215, fp32"""
import ctypes as C
import hashlib
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "side_kernel_bits.npz")
GROUPS = ("rows", "maxpool", "bicubic", "gap", "layout")
# outputs per group: see replay()
COUNTS = {"rows": 2 * 3 + 2 + 4, "maxpool": 4, "bicubic": 2 * 5, "gap": 2 + 2 + 2 + 2, "layout": 5}
BF, F32 = torch.bfloat16, torch.float32
M_ROWS = 37
POOL = (2, 6, 10)
BICUBIC = ((16, 16, 7, 7), (18, 12, 8, 5))
GAP = (3, 49, 20)
LAYOUT = (2, 3, 5, 7, 8, 8)
SENTINEL = 7.0


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def to_np(t):
    """a CPU tensor as the array the file holds: bf16 as its uint16 bits"""
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF else t.numpy()


def to_dev(a):
    return (torch.from_numpy(a.view(np.int16)).view(BF) if a.dtype == np.uint16 else torch.from_numpy(a)).cuda()


def sfx(dt):
    return "bf16" if dt == BF else "f32"


def draw():
    """The inputs of every case, as {"<group>/<name>_<format>": array}."""
    g = torch.Generator().manual_seed(41)
    fx = {}

    def keep(name, t, dt):
        fx["%s_%s" % (name, sfx(dt))] = to_np(t.to(dt).contiguous())

    def sprinkle(t, values):
        flat = t.reshape(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:2 * len(values)]
        flat[idx] = torch.tensor(values + values)
        return t

    six = torch.tensor(6.0)
    for dt, Cc in ((BF, 24), (F32, 12)):
        specials = [float("nan"), float("inf"), float("-inf"), -0.0]
        keep("rows/a", sprinkle(torch.randn(M_ROWS, Cc, generator=g), specials), dt)
        keep("rows/b", sprinkle(torch.randn(M_ROWS, Cc, generator=g), specials), dt)
        keep("rows/dy", sprinkle(torch.randn(M_ROWS, Cc, generator=g), specials), dt)
        if dt == BF:       # neighbours of 6 in bf16 (8 bits of significand: spacing 2^-5 above 4)
            below, above = 6.0 - 2.0 ** -5, 6.0 + 2.0 ** -5
        else:
            below, above = float(torch.nextafter(six, torch.tensor(0.0))), float(torch.nextafter(six, torch.tensor(9.0)))
        pal = torch.tensor([0.0, -0.0, 6.0, below, above, float("inf"), 1e-30, -1e-30])
        mask = torch.randn(M_ROWS, Cc, generator=g) * 4
        sel = torch.randint(0, 16, (M_ROWS, Cc), generator=g)
        for j in range(pal.numel()):
            mask[sel == j] = pal[j]
            assert bool((sel == j).any())
        mask = mask.to(dt)
        assert float(mask.float()[sel == 3].max()) < 6.0 < float(mask.float()[sel == 4].min())
        keep("rows/mask", mask, dt)

    B, H, W = POOL
    for dt, Cc in ((BF, 16), (F32, 8)):
        x = torch.randint(0, 3, (B, Cc, H, W), generator=g).float()
        win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(B, Cc, 9, -1)
        assert ((win == win.max(2, keepdim=True).values).sum(2) >= 2).float().mean().item() >= 0.5
        x[1, 3, 2, 5] = float("nan")
        keep("maxpool/x", x.permute(0, 2, 3, 1).reshape(-1, Cc), dt)
        keep("maxpool/dy", torch.randn(B * (H // 2) * (W // 2), Cc, generator=g), dt)

    for Hs, Ws, Hd, Wd in BICUBIC:
        for dt in (BF, F32):
            keep("bicubic/src_%dx%d" % (Hs, Ws), torch.randn(2 * Hs * Ws, 3, generator=g), dt)
            keep("bicubic/ddst_%dx%d" % (Hd, Wd), torch.randn(2 * Hd * Wd, 3, generator=g), dt)

    B, HW, Cc = GAP
    for dt in (BF, F32):
        keep("gap/x", torch.randn(B * HW, Cc, generator=g), dt)
    xt = torch.randint(0, 3, (B, HW, Cc), generator=g).float()
    assert ((xt == xt.max(1, keepdim=True).values).sum(1) >= 2).float().mean().item() >= 0.5
    keep("gap/x_tied", xt.reshape(-1, Cc), F32)
    keep("gap/gf", torch.randn(B, Cc, generator=g), F32)
    mask = torch.randn(B * HW, Cc, generator=g)
    mask[torch.rand(B * HW, Cc, generator=g) < 0.2] = 0.0
    mask[torch.rand(B * HW, Cc, generator=g) < 0.05] = -0.0
    keep("gap/mask", mask, BF)

    B, Cc, H, W, _Cpad, _ld = LAYOUT
    keep("layout/x", torch.randn(B, Cc, H, W, generator=g), F32)
    return fx


def padded(t, ld):
    """device rows [M, C] -> a buffer [M, ld] whose padding columns hold SENTINEL"""
    buf = torch.full((t.shape[0], ld), SENTINEL, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf


def nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device="cuda")


def replay(L, fx, group):
    """Every case of `group` on library L with the stored inputs -> {"<group>/<case>/<output>": sha256 hex}."""
    got = {}

    def inp(name, dt):
        return to_dev(fx["%s/%s_%s" % (group, name, sfx(dt))])

    def put(case, **outs):
        torch.cuda.synchronize()
        for k, v in outs.items():
            got["%s/%s/%s" % (group, case, k)] = digest(v)

    def ok(err):
        assert err == 0, err

    if group == "rows":
        for dt in (BF, F32):
            s, V = sfx(dt), 8 if dt == BF else 4
            a, b, dy, mask = (inp(n, dt) for n in ("a", "b", "dy", "mask"))
            M, Cc = a.shape
            lda, ldb, ldy = Cc + V, Cc + 2 * V, Cc + 3 * V
            ab, bb = padded(a, lda), padded(b, ldb)
            y = nan((M, ldy), dt)
            ok(getattr(L, "dd_op_add_" + s)(P(ab), lda, P(bb), ldb, P(y), ldy, M, Cc, None))
            put("add_" + s, y=y)
            y = nan((M, ldy), dt)
            ok(getattr(L, "dd_op_copy_" + s)(P(ab), lda, P(y), ldy, M, Cc, None))
            put("copy_" + s, y=y)
            ok(getattr(L, "dd_op_add_" + s)(P(ab), lda, P(bb), ldb, P(ab), lda, M, Cc, None))      # y == a
            put("add_in_place_" + s, y=ab)
            mb = padded(mask, ldb)
            for hi in ((None,) if dt == BF else (0.0, 6.0)):
                tail = () if hi is None else (hi,)
                case = "mask_" + s + ("" if hi is None else "_hi%g" % hi)
                db, y = padded(dy, lda), nan((M, ldy), dt)
                ok(getattr(L, "dd_op_mask_" + s)(P(db), lda, P(mb), ldb, P(y), ldy, M, Cc, *tail, None))
                put(case, y=y)
                ok(getattr(L, "dd_op_mask_" + s)(P(db), lda, P(mb), ldb, P(db), lda, M, Cc, *tail, None))      # y == dy
                put(case + "_in_place", y=db)
    elif group == "maxpool":
        B, H, W = POOL
        for dt in (BF, F32):
            tail = "" if dt == BF else "_f32"
            x, dy = inp("x", dt), inp("dy", dt)
            y, dx = nan(tuple(dy.shape), dt), nan(tuple(x.shape), dt)
            ok(getattr(L, "dd_op_maxpool3x3s2" + tail)(P(x), P(y), B, H, W, x.shape[1], None))
            ok(getattr(L, "dd_op_maxpool3x3s2_bwd" + tail)(P(x), P(dy), P(dx), B, H, W, x.shape[1], None))
            put("maxpool_" + sfx(dt), y=y, dx=dx)
    elif group == "bicubic":
        B, Cc, Cpad = 2, 3, 8
        for Hs, Ws, Hd, Wd in BICUBIC:
            geo = "%dx%d_to_%dx%d" % (Hs, Ws, Hd, Wd)
            dims = (B, Hs, Ws, Hd, Wd, Cc)
            for dt in (BF, F32):
                ld = 8 if dt == BF else 4
                src, ddst = padded(inp("src_%dx%d" % (Hs, Ws), dt), ld), padded(inp("ddst_%dx%d" % (Hd, Wd), dt), ld)
                dst, dsrc = nan((B * Hd * Wd, Cpad + ld), dt), nan((B * Hs * Ws, ld), dt)
                if dt == BF:
                    ok(L.dd_op_bicubic(P(src), ld, P(dst), Cpad + ld, *dims, Cpad, None))
                    ok(L.dd_op_bicubic_bwd(P(ddst), ld, P(dsrc), ld, *dims, None))
                else:
                    ok(L.dd_op_bicubic_f32(P(src), ld, P(dst), Cpad + ld, *dims, Cpad, None))
                    ok(L.dd_op_bicubic_bwd_f32(P(ddst), ld, P(dsrc), 0, ld, *dims, None))
                    slab = nan((B * Hs * Ws, 8), BF)              # fp32 gradient -> bf16 rows
                    ok(L.dd_op_bicubic_bwd_f32(P(ddst), ld, P(slab), 1, 8, *dims, None))
                    put("%s_bwd_f32_to_bf16" % geo, dsrc=slab)
                put("%s_%s" % (geo, sfx(dt)), dst=dst, dsrc=dsrc)
    elif group == "gap":
        B, HW, Cc = GAP
        ld = Cc + 4
        gf = inp("gf", F32)
        f = nan((B, Cc), F32)
        ok(L.dd_op_gap(P(padded(inp("x", BF), ld)), ld, P(f), B, HW, Cc, None))
        put("gap_bf16", f=f)
        f = nan((B, Cc), F32)
        ok(L.dd_op_gap_f32(P(padded(inp("x", F32), ld)), ld, P(f), None, B, HW, Cc, 0, None))
        put("gap_f32_avg", f=f)
        f, arg = nan((B, Cc), F32), torch.full((B, Cc), -1, dtype=torch.int32, device="cuda")
        ok(L.dd_op_gap_f32(P(padded(inp("x_tied", F32), ld)), ld, P(f), P(arg), B, HW, Cc, 1, None))
        put("gap_f32_max", f=f, argmax=arg)
        mb = padded(inp("mask", BF), ld + 8)
        for m in (None, mb):
            dx = nan((B * HW, ld), BF)
            ok(L.dd_op_gap_bwd(P(gf), P(dx), ld, B, HW, Cc, P(m), ld + 8, None))
            put("gap_bwd_bf16" + ("_mask" if m is not None else ""), dx=dx)
        for a in (None, arg):
            dx = nan((B * HW, ld), F32)
            ok(L.dd_op_gap_bwd_f32(P(gf), P(dx), ld, B, HW, Cc, P(a), None))
            put("gap_bwd_f32" + ("_argmax" if a is not None else ""), dx=dx)
    elif group == "layout":
        B, Cc, H, W, Cpad, ld = LAYOUT
        x = inp("x", F32)
        for dup in (0, 1):
            for scale in (1.0, 0.18215):
                y = nan(((2 if dup else 1) * B * H * W, ld), BF)
                ok(L.dd_op_nchw_f32_to_nhwc_bf16(P(x), P(y), B, Cc, H, W, Cpad, ld, dup, scale, None))
                put("nchw_to_nhwc_bf16_dup%d_scale%g" % (dup, scale), y=y)
        y = nan((B * H * W, ld), F32)
        ok(L.dd_op_nchw_to_nhwc_f32(P(x), P(y), B, Cc, H, W, Cpad, ld, None))
        put("nchw_to_nhwc_f32", y=y)
    assert len(got) == COUNTS[group], (group, len(got))
    return got


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from distdiff_amd import _lib
    L = _lib.lib()
    fx = draw()
    got = {}
    for group in GROUPS:
        got.update(replay(L, fx, group))
        again = replay(L, fx, group)
        assert all(got[k] == v for k, v in again.items()), "the build is not deterministic on %s" % group
    names = sorted(got)
    fx["case_names"] = np.array(names)
    fx["case_sha256"] = np.array([got[n] for n in names])
    np.savez_compressed(PATH, **fx)
    print("wrote %s: %d outputs, %d bytes, library %s" % (PATH, len(names), os.path.getsize(PATH), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
