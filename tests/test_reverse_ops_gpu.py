"""The forms the reverse pass (engine_exec.cpp: run_bwd) launches that no other op-level test reaches, each against a plain float64
torch computation on the CPU of the same operation on the same (bf16- or fp32-rounded) inputs.

A. In-place accumulating input-gradients: a tensor with several consumers gets `y = gx, res = gx` (the residual ALIASES the output) on
   whichever kernel launch_conv_gemm / launch_conv_f32 picks.  Each case runs the same launch out of place (y = empty, res = g_prev)
   and in place (y = g_prev.clone(), res = y): the two results must be BIT-identical (same kernel, inputs and summation order -- only
   the aliasing differs, so no tolerance is involved), the out-of-place one must match float64 autograd + g_prev, and
   ops.conv_gemm_kind of the very same arguments must name the kernel the case is about.
B. The `accumulate` forms of GroupNorm / LayerNorm backward, sumpool2x2, act_bwd, select_rows_bwd and add with y == a.
C. The side kernels that have no other op-level test, at a small ragged shape and at one whose thread count exceeds one grid pass
   (8192 blocks x 256 threads: the grid-stride loop wraps), through strided row views where the launcher takes row strides.

Tolerances.  bf16 kernels with arithmetic: assert_close defaults of test_kernels_gpu.py (one bf16 rounding of an fp32 accumulation).
GroupNorm / LayerNorm backward: rtol 2e-2, atol 2e-3 as in test_groupnorm / test_layernorm.  fp32 additive kernels: 2e-5 of max|ref|
(test_guide_f32_gpu.py).  Selection / re-layout kernels: exact.  Bicubic fp32: see test_bicubic_f32.
Every accumulating case draws the previous gradient with 0.5 <= rms(prev) / rms(fresh) <= 2 (asserted on the reference): a dropped or
doubled accumulation is then an error of the order of max|ref| / 3, far outside every tolerance here.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import assert_close, bf

pytestmark = pytest.mark.gpu

WRAP = 8192 * 256          # threads of one grid pass of the side kernels (elementwise.hip / guide_f32.hip: nblocks)
SENTINEL = 7.0             # fills the columns around a strided view; must come back unchanged


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distdiff_amd import ops as o
    assert torch.cuda.is_available()
    return o


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call(name, *args):
    """one dd_op_* launch on the default stream, checked and waited for"""
    from distdiff_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)
    torch.cuda.synchronize()


def close32(got, ref, what, tol=2e-5):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    assert err <= tol * max(ref.abs().max().item(), 1e-6), "%s: max err %.3g (ref max %.3g)" % (what, err, ref.abs().max().item())


def exact(got, ref, what):
    assert_close(got, ref, rtol=0, atol=0, what=what)


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


def prev_like(gref, g):
    """a previous gradient of the fresh gradient's magnitude (condition of the accumulating cases, asserted)"""
    prev = bf(torch.randn(gref.shape, generator=g) * rms(gref))
    ratio = rms(prev) / rms(gref)
    assert 0.5 <= ratio <= 2.0, ratio
    return prev


def dev_rows(t, ld=None, off=0, dtype=torch.bfloat16):
    """CPU rows [M, C] -> (device buffer [M, ld] full of SENTINEL, its column view [:, off:off + C] holding t)"""
    M, Cc = t.shape
    buf = torch.full((M, ld or Cc), SENTINEL, dtype=dtype, device="cuda")
    v = buf[:, off:off + Cc]
    v.copy_(t.to(dtype))
    return buf, v


def untouched(buf, off, Cc, what):
    out = torch.cat([buf[:, :off], buf[:, off + Cc:]], dim=1).float()
    assert out.numel() == 0 or float((out - SENTINEL).abs().max()) == 0.0, what + ": wrote outside the row view"


def bit_diff(a, b):
    """'' when a and b are bit-identical, else where they differ (rows / columns / 256-row tiles)"""
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    a, b = a.contiguous().view(it), b.contiguous().view(it)
    if torch.equal(a, b):
        return ""
    d = (a != b).nonzero().cpu()
    rows, cols = d[:, 0].unique(), d[:, 1].unique()
    return "%d elements differ; first (row, col) %s; %d rows (first %s, 256-row tiles %s), %d columns (first %s)" % (
        d.shape[0], d[:5].tolist(), rows.numel(), rows[:8].tolist(), (rows // 256).unique()[:8].tolist(), cols.numel(), cols[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# A. in-place accumulating dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [
    # name, kind (ops.CONV_GEMM_KINDS), form inside kind "general" and split (ops.conv_gemm_plan), B, Cin, Cout, H, W, k, stride, ksplit,
    # y is a column view of a wider gradient buffer.  The dgrad's GEMM is M = B H W, N = Cin, K = k k Cout; "linear" = 1x1 on M x 1 pixels.
    # ksplit = 0 leaves the choice to the launcher, which keeps conv_gemm_big_kernel only with >= 192 work items (tiles x split);
    # ksplit >= 1 fixes the split and keeps the big kernel's configuration whenever the shape has one (M >= 1024).
    # conv_gemm_kernel, 256 x 64 and 128 x 128 tiles, generic epilogue, explicit and automatic split-K (the reduce kernel reads res == y)
    ("small_256x64_linear_ksplit1", "general", "small_256x64", 1, 1, 320, 640, 300, 1, 1, 1, 1, False),
    ("small_256x64_linear_ksplit3_reduce_reads_res", "general", "small_256x64", 3, 1, 320, 640, 300, 1, 1, 1, 3, False),
    ("small_256x64_auto_splitk_ragged_m", "general", "small_256x64", 9, 2, 320, 320, 24, 25, 3, 1, 0, False),
    ("small_256x64_auto_splitk_stride2_dgrad", "general", "small_256x64", 6, 2, 64, 256, 64, 64, 3, 2, 0, False),
    ("small_128x128_auto_splitk_ragged_m", "general", "small_128x128", 11, 3, 128, 384, 20, 21, 3, 1, 0, False),
    # conv_gemm_big_kernel (persistent): every configuration, batched epilogue (split 1) and split-K + reduce; rows beyond a ragged M are
    # clamped reads of row M - 1
    ("big_128x160_two_workgroups_ragged_m", "general", "big_128x160_two_workgroups", 1, 2, 320, 320, 24, 25, 3, 1, 1, False),
    ("big_128x160_two_workgroups_ksplit3_reduce_reads_res", "general", "big_128x160_two_workgroups", 3, 2, 320, 320, 24, 25, 3, 1, 3, False),
    ("big_128x160_two_workgroups_auto_288_items", "general", "big_128x160_two_workgroups", 1, 2, 320, 320, 96, 96, 3, 1, 0, False),
    ("big_256x128_stride2_dgrad", "general", "big_256x128", 1, 2, 64, 256, 64, 64, 3, 2, 1, False),          # shift = 1, parity = 1
    ("big_256x128_ragged_m_54_ksteps", "general", "big_256x128", 1, 3, 128, 384, 20, 21, 3, 1, 1, False),
    ("big_128x128_two_workgroups_ragged_m", "general", "big_128x128_two_workgroups", 1, 3, 384, 128, 20, 21, 3, 1, 1, False),
    ("big_128x256", "general", "big_128x256", 1, 2, 256, 256, 32, 32, 3, 1, 1, False),
    ("big_256x160_180_ksteps", "general", "big_256x160", 1, 2, 320, 1280, 24, 24, 3, 1, 1, False),
    ("halo_n320_32x32", "conv_halo", None, 1, 48, 320, 320, 32, 32, 3, 1, 0, False),
    ("halo_persist_n256_64x64", "conv_halo_persist", None, 1, 12, 256, 256, 64, 64, 3, 1, 0, False),   # <= 8 chunks: the persistent 512 x 128 form
    ("halo_n256_64x64_10_chunks", "conv_halo", None, 1, 12, 256, 640, 64, 64, 3, 1, 0, False),          # 10 chunks: conv_halo_kernel, N = 256
    ("halo_n320_width96_not_a_power_of_two", "conv_halo", None, 1, 12, 320, 320, 96, 96, 3, 1, 0, False),
    ("halo_8x8_chunk_split_fp32_partials", "conv_halo", None, 4, 64, 1280, 1280, 8, 8, 3, 1, 0, False),
    ("halo_persist_ragged_288_tiles", "conv_halo_persist", None, 1, 9, 128, 128, 128, 128, 3, 1, 0, False),
    ("gemm_pps_linear", "gemm_pps", None, 1, 1, 1280, 640, 49152, 1, 1, 1, 1, False),
    # the gradient of a channel concat: y_ld = res_ld > N, the columns outside the view must come back bit-unchanged
    ("small_256x64_auto_splitk_ragged_m_column_view", "general", "small_256x64", 9, 2, 320, 320, 24, 25, 3, 1, 0, True),
    ("big_128x160_two_workgroups_ragged_m_column_view", "general", "big_128x160_two_workgroups", 1, 2, 320, 320, 24, 25, 3, 1, 1, True),
    ("halo_n320_32x32_column_view", "conv_halo", None, 1, 48, 320, 320, 32, 32, 3, 1, 0, True),
]
# kernel kinds whose two OUT-OF-PLACE runs differ bitwise (then the in-place run can only be held to the float64 reference): none --
# every kind reduces in a fixed order (split-K and the 8 x 8 chunk split go through fp32 partials and a reduce kernel, no atomics)
NOT_DETERMINISTIC = ()


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_dgrad_accumulates_in_place(ops, case):
    name, kind, form, split, B, Cin, Cout, H, W, k, stride, ksplit, view = case
    if kind != "general" and torch.cuda.mem_get_info()[0] < 12e9:         # the halo / ping-pong shapes (up to 2.3 GB of split-K scratch)
        pytest.skip("needs 12 GB of free HBM")
    g = torch.Generator().manual_seed(len(name) * 7 + Cin)
    pad = k // 2
    w = bf(torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = bf(torch.randn(B, Cout, Ho, Wo, generator=g))
    x0 = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    (gref,) = torch.autograd.grad(F.conv2d(x0, w.double(), None, stride=stride, padding=pad), x0, dy.double())
    prev = prev_like(gref, g)
    want = ops.to_nhwc_bf16(prev, Cin).double() + gref.permute(0, 2, 3, 1).reshape(-1, Cin)        # rows [M, Cin]
    M, N = B * H * W, Cin
    dyd = ops.to_nhwc_bf16(dy, Cout).cuda()
    pkd = ops.PackedConv(w, pad, mode=1)
    kw = dict(stride=1, shift=1 if stride == 2 else 0, parity=1 if stride == 2 else 0, ksplit=ksplit)
    if ksplit != 1:      # one split-K scratch for every launch of the case (its size is part of the launcher's decision)
        kw["partial"] = torch.empty((max(ksplit, 16) * M * N,), device="cuda", dtype=torch.float32)
    ld, off = (N + 64, 64) if view else (N, 0)
    prev_rows = ops.to_nhwc_bf16(prev, Cin)

    def launch(in_place):
        buf, y = dev_rows(prev_rows, ld, off)            # in place: y holds g_prev and is its own residual
        if in_place:
            res = y
        else:
            _rbuf, res = dev_rows(prev_rows, ld, off)
            y.fill_(-3.0)
        assert ops.CONV_GEMM_KINDS[ops.conv_gemm_kind(dyd, pkd, B, Ho, Wo, H, W, y=y, res=res, **kw)] == kind
        plan = ops.conv_gemm_plan(dyd, pkd, B, Ho, Wo, H, W, y=y, res=res, **kw)
        assert plan == (kind, form, split), "%s runs as %s, the case is about %s" % (name, plan, (kind, form, split))
        ops.conv_gemm(dyd, pkd, B, Ho, Wo, H, W, y=y, res=res, **kw)
        torch.cuda.synchronize()
        untouched(buf, off, N, name)
        return y

    out1, out2, inp = launch(False), launch(False), launch(True)
    assert_close(out1, want, what=name + " out of place")
    twice = bit_diff(out1, out2)
    if kind in NOT_DETERMINISTIC:
        assert_close(inp, want, what=name + " in place")
        return
    assert not twice, "%s: two out-of-place runs differ (%s)" % (name, twice)
    d = bit_diff(out1, inp)
    assert not d, "%s: res == y changes the result: %s" % (name, d)


F32_DGRAD_CASES = [      # of tests/test_guide_f32_gpu.py: name, B, Cin, Cout, H, W, k, stride, pad, groups
    ("3x3", 2, 64, 64, 14, 14, 3, 1, 1, 1),
    ("3x3_groups32_stride2", 1, 256, 256, 14, 14, 3, 2, 1, 32),
    ("stem7x7_narrow_dgrad", 2, 3, 64, 96, 96, 7, 2, 3, 1),
]


@pytest.mark.parametrize("case", F32_DGRAD_CASES, ids=[c[0] for c in F32_DGRAD_CASES])
def test_dgrad_f32_accumulates_in_place(ops, case):
    """launch_conv_f32 with res == y (engine_exec.cpp: run_conv_f32_bwd, op.x_acc), general and one-thread-per-pixel kernel."""
    name, B, Cin, Cout, H, W, k, stride, pad, groups = case
    g = torch.Generator().manual_seed(5)
    w = torch.randn(Cout, Cin // groups, k, k, generator=g) / (Cin // groups * k * k) ** 0.5
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = torch.randn(B, Cout, Ho, Wo, generator=g)
    x0 = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    (gref,) = torch.autograd.grad(F.conv2d(x0, w.double(), None, stride=stride, padding=pad, groups=groups), x0, gy.double())
    prev = torch.randn(B, Cin, H, W, generator=g) * rms(gref)
    assert 0.5 <= rms(prev) / rms(gref) <= 2.0
    ld = (Cin + 3) // 4 * 4

    def rows(x, width):
        r = torch.zeros(x.shape[0] * x.shape[2] * x.shape[3], width)
        r[:, :x.shape[1]] = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        return r.cuda()

    pkb = ops.PackedConvF32(w, pad, mode=1, groups=groups)
    gyd = rows(gy, (Cout + 3) // 4 * 4)
    kw = dict(stride=1, shift=1 if stride == 2 else 0, parity=1 if stride == 2 else 0)
    out = ops.conv_f32(gyd, pkb, B, Ho, Wo, H, W, res=rows(prev, ld), **kw)
    buf = rows(prev, ld)
    inp = ops.conv_f32(gyd, pkb, B, Ho, Wo, H, W, res=buf, y=buf, **kw)
    torch.cuda.synchronize()
    want = (gref + prev.double()).permute(0, 2, 3, 1).reshape(-1, Cin)
    close32(out, want, name + " out of place")
    d = bit_diff(out.contiguous(), inp.contiguous())
    assert not d, "%s: res == y changes the result: %s" % (name, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. accumulate forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,G,HW,silu,eps", [(320, 32, 256, True, 1e-5), (128, 32, 1024, True, 1e-6), (64, 8, 100, False, 1e-6),
                                               (2560, 32, 64, True, 1e-5)])
def test_groupnorm_backward_accumulates(ops, Cc, G, HW, silu, eps):
    g = torch.Generator().manual_seed(5)
    B = 2
    x = bf(torch.randn(B, Cc, HW, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    xr = x.double().requires_grad_(True)
    ref = F.group_norm(xr, G, gamma.double(), beta.double(), eps)
    if silu:
        ref = F.silu(ref)
    dy = bf(torch.randn(B, Cc, HW, generator=g))
    (gx,) = torch.autograd.grad(ref, xr, dy.double())
    prev = prev_like(gx, g)
    to_rows = lambda t: t.permute(0, 2, 1).reshape(B * HW, Cc).to(torch.bfloat16).cuda()
    xd = to_rows(x)
    _y, stats = ops.groupnorm(xd, gamma.cuda(), beta.cuda(), B, HW, G, eps, silu)
    dx = to_rows(prev)
    out = ops.groupnorm(xd, gamma.cuda(), beta.cuda(), B, HW, G, eps, silu, dy=to_rows(dy), stats=stats, accumulate_into=dx)
    torch.cuda.synchronize()
    assert out.data_ptr() == dx.data_ptr()
    assert_close(dx.float().cpu().reshape(B, HW, Cc).permute(0, 2, 1), gx + prev.double(), rtol=2e-2, atol=2e-3, what="gn bwd accumulate")


@pytest.mark.parametrize("Cc", [320, 1280, 2048])     # multi-row kernel (1 and 3 vectors per lane), one-row kernel beyond 1536
def test_layernorm_backward_accumulates(ops, Cc):
    g = torch.Generator().manual_seed(6)
    M = 77
    x = bf(torch.randn(M, Cc, generator=g) * 1.5 + 0.3)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    xr = x.double().requires_grad_(True)
    ref = F.layer_norm(xr, (Cc,), gamma.double(), beta.double(), 1e-5)
    dy = bf(torch.randn(M, Cc, generator=g))
    (gx,) = torch.autograd.grad(ref, xr, dy.double())
    prev = prev_like(gx, g)
    xd = x.to(torch.bfloat16).cuda()
    _y, stats = ops.layernorm(xd, gamma.cuda(), beta.cuda(), 1e-5)
    dx = prev.to(torch.bfloat16).cuda()
    ops.layernorm(xd, gamma.cuda(), beta.cuda(), 1e-5, dy=dy.to(torch.bfloat16).cuda(), stats=stats, accumulate_into=dx)
    torch.cuda.synchronize()
    assert_close(dx, gx + prev.double(), rtol=2e-2, atol=2e-3, what="ln bwd accumulate")


@pytest.mark.parametrize("B,H,W,Cc", [(1, 3, 5, 24), (3, 64, 64, 1408)], ids=["small_ragged", "grid_wraps"])
def test_sumpool2x2_accumulates_into_a_strided_view(ops, B, H, W, Cc):
    """launch_sumpool2x2(..., accumulate = 1): the transpose of the fused nearest-2x upsample added to a gradient that is already
    there (engine_exec.cpp, op.up && op.x_acc), the destination a column view of wider rows; and the first-write form."""
    g = torch.Generator().manual_seed(21)
    src = bf(torch.randn(B, 2 * H, 2 * W, Cc, generator=g))
    fresh = src.double().reshape(B, H, 2, W, 2, Cc).sum((2, 4)).reshape(B * H * W, Cc)
    prev = prev_like(fresh, g)
    if B * H * W * (Cc // 8) <= WRAP:
        assert B == 1, "the large case must wrap the grid-stride loop"
    _sbuf, sd = dev_rows(src.reshape(-1, Cc), Cc + 8, 8)
    for acc in (1, 0):
        buf, dst = dev_rows(prev, Cc + 24, 16)
        call("dd_op_sumpool2x2", P(sd), sd.stride(0), P(dst), dst.stride(0), B, H, W, Cc, acc)
        assert_close(dst, fresh + prev.double() * acc, what="sumpool accumulate=%d" % acc)
        untouched(buf, 16, Cc, "sumpool")


@pytest.mark.parametrize("M,Cc", [(37, 24), (4100, 4096)], ids=["small_ragged", "grid_wraps"])
def test_add_and_copy_bf16(ops, M, Cc):
    """launch_add_bf16 / launch_copy_bf16 on strided views, and the accumulate form of the reverse pass: output == first input."""
    g = torch.Generator().manual_seed(22)
    assert M * (Cc // 8) > WRAP or M < 100
    a, b = bf(torch.randn(M, Cc, generator=g)), bf(torch.randn(M, Cc, generator=g))
    _ab, ad = dev_rows(a, Cc + 8, 8)
    _bb, bd = dev_rows(b, Cc + 16, 0)
    yb, yd = dev_rows(torch.zeros(M, Cc), Cc + 24, 16)
    call("dd_op_add_bf16", P(ad), ad.stride(0), P(bd), bd.stride(0), P(yd), yd.stride(0), M, Cc)
    assert_close(yd, a.double() + b.double(), what="add")
    untouched(yb, 16, Cc, "add")
    call("dd_op_add_bf16", P(ad), ad.stride(0), P(bd), bd.stride(0), P(ad), ad.stride(0), M, Cc)         # y == a
    assert_close(ad, a.double() + b.double(), what="add in place")
    untouched(_ab, 8, Cc, "add in place")
    call("dd_op_copy_bf16", P(bd), bd.stride(0), P(yd), yd.stride(0), M, Cc)
    exact(yd, b, "copy")
    untouched(yb, 16, Cc, "copy")


@pytest.mark.parametrize("M,Cc", [(37, 20), (2100, 1000)], ids=["small_ragged", "grid_wraps"])
@pytest.mark.parametrize("kind", [0, 1], ids=["quick_gelu", "erf_gelu"])
def test_act_forward_backward_and_accumulate(ops, M, Cc, kind):
    g = torch.Generator().manual_seed(23)
    assert M * Cc > WRAP or M < 100
    x = bf(torch.randn(M, Cc, generator=g) * 2)
    xr = x.double().requires_grad_(True)
    ref = xr * torch.sigmoid(1.702 * xr) if kind == 0 else F.gelu(xr)
    dy = bf(torch.randn(M, Cc, generator=g))
    (gx,) = torch.autograd.grad(ref, xr, dy.double())
    prev = prev_like(gx, g)
    _xb, xd = dev_rows(x, Cc + 4, 4)
    yb, yd = dev_rows(torch.zeros(M, Cc), Cc + 6, 2)
    call("dd_op_act_bf16", P(xd), xd.stride(0), P(yd), yd.stride(0), M, Cc, kind)
    assert_close(yd, ref.detach(), what="act fwd")
    untouched(yb, 2, Cc, "act fwd")
    _db, dyd = dev_rows(dy, Cc + 2, 1)
    for acc in (0, 1):
        gb, gd = dev_rows(prev, Cc + 10, 3)
        call("dd_op_act_bwd_bf16", P(xd), xd.stride(0), P(dyd), dyd.stride(0), P(gd), gd.stride(0), M, Cc, kind, acc)
        assert_close(gd, gx + prev.double() * acc, what="act bwd accumulate=%d" % acc)
        untouched(gb, 3, Cc, "act bwd")


@pytest.mark.parametrize("B,stride,Cc", [(3, 5, 20), (9, 257, 1000)], ids=["small_ragged", "grid_wraps"])
def test_select_rows_forward_backward_and_accumulate(ops, B, stride, Cc):
    """the class token of every image (rows b * stride) and its VJP: zero (or the gradient already there) everywhere else"""
    g = torch.Generator().manual_seed(24)
    assert B * stride * Cc > WRAP or B < 5
    x = bf(torch.randn(B * stride, Cc, generator=g))
    _xb, xd = dev_rows(x, Cc + 4, 4)
    yb, yd = dev_rows(torch.zeros(B, Cc), Cc + 6, 2)
    call("dd_op_select_rows", P(xd), xd.stride(0), P(yd), yd.stride(0), B, stride, Cc)
    exact(yd, x[::stride], "select_rows")
    untouched(yb, 2, Cc, "select_rows")
    if B > 5:      # the forward runs B * C threads: its own wrapping shape (every second row of 4400)
        Bw = 2200
        assert Bw * Cc > WRAP
        xw = bf(torch.randn(2 * Bw, Cc, generator=g))
        _wb, xwd = dev_rows(xw, Cc + 4, 4)
        ywb, ywd = dev_rows(torch.zeros(Bw, Cc), Cc + 6, 2)
        call("dd_op_select_rows", P(xwd), xwd.stride(0), P(ywd), ywd.stride(0), Bw, 2, Cc)
        exact(ywd, xw[::2], "select_rows, wrapping forward")
        untouched(ywb, 2, Cc, "select_rows, wrapping forward")
    dy = bf(torch.randn(B, Cc, generator=g))
    fresh = torch.zeros(B * stride, Cc, dtype=torch.float64)
    fresh[::stride] = dy.double()
    prev = bf(torch.randn(B * stride, Cc, generator=g))            # same magnitude as dy
    _db, dyd = dev_rows(dy, Cc + 2, 1)
    gb, gd = dev_rows(prev, Cc + 10, 3)
    call("dd_op_select_rows_bwd", P(dyd), dyd.stride(0), P(gd), gd.stride(0), B, stride, Cc, 0)
    exact(gd, fresh, "select_rows bwd")
    untouched(gb, 3, Cc, "select_rows bwd")
    gb, gd = dev_rows(prev, Cc + 10, 3)
    call("dd_op_select_rows_bwd", P(dyd), dyd.stride(0), P(gd), gd.stride(0), B, stride, Cc, 1)
    assert_close(gd, fresh + prev.double(), what="select_rows bwd accumulate")
    assert 0.5 <= rms(prev[::stride]) / rms(dy) <= 2.0
    exact(gd.float().cpu()[torch.arange(B * stride) % stride != 0], prev[torch.arange(B * stride) % stride != 0], "unselected rows")
    untouched(gb, 3, Cc, "select_rows bwd accumulate")


# ---------------------------------------------------------------------------------------------------------------------------------
# C. side kernels against plain references
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cc", [(37, 24), (4100, 4096)], ids=["small_ragged", "grid_wraps"])
def test_mask_bf16(ops, M, Cc):
    """y = dy * (mask > 0): ReLU backward from the stored forward output (zeros of either sign and negative values block)"""
    g = torch.Generator().manual_seed(25)
    assert M * (Cc // 8) > WRAP or M < 100
    dy = bf(torch.randn(M, Cc, generator=g))
    pal = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.5, -2.0, 3.0])
    mask = pal[torch.randint(0, pal.numel(), (M, Cc), generator=g)]
    mask[0, :7] = pal
    xr = mask.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.relu(xr), xr, dy)
    _db, dd = dev_rows(dy, Cc + 8, 8)
    _mb, md = dev_rows(mask, Cc + 16, 0)
    assert torch.equal(md.float().cpu(), mask) and bool((torch.signbit(md.float().cpu()) & (mask == 0)).any())      # -0 survives
    yb, yd = dev_rows(torch.zeros(M, Cc), Cc + 24, 16)
    call("dd_op_mask_bf16", P(dd), dd.stride(0), P(md), md.stride(0), P(yd), yd.stride(0), M, Cc)
    exact(yd, ref, "mask_bf16")
    untouched(yb, 16, Cc, "mask_bf16")
    call("dd_op_mask_bf16", P(dd), dd.stride(0), P(md), md.stride(0), P(dd), dd.stride(0), M, Cc)       # in place, as run_bwd calls it
    exact(dd, ref, "mask_bf16 in place")


@pytest.mark.parametrize("M,Cc", [(37, 12), (4100, 2048)], ids=["small_ragged", "grid_wraps"])
@pytest.mark.parametrize("hi", [0.0, 6.0], ids=["relu", "relu6"])
def test_mask_f32(ops, M, Cc, hi):
    """launch_mask_f32 against autograd of F.relu / F.hardtanh(x, 0, 6) at the kinks: exact 0, -0, exact 6 and its fp32 neighbours"""
    g = torch.Generator().manual_seed(26)
    assert M * (Cc // 4) > WRAP or M < 100
    six = torch.tensor(6.0)
    below, above = torch.nextafter(six, torch.tensor(0.0)), torch.nextafter(six, torch.tensor(9.0))
    special = torch.stack([torch.tensor(0.0), torch.tensor(-0.0), six, below, above])
    assert float(below) < 6.0 < float(above)
    mask = torch.randn(M, Cc, generator=g) * 4
    sel = torch.randint(0, 10, (M, Cc), generator=g)
    for j in range(5):
        mask[sel == j] = special[j]
        assert bool((sel == j).any())
    assert bool(torch.signbit(mask[mask == 0]).any()) and bool((~torch.signbit(mask[mask == 0])).any())
    for v in (six, below, above):
        assert bool((mask == v).any())
    dy = torch.randn(M, Cc, generator=g)
    xr = mask.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.relu(xr) if hi == 0.0 else F.hardtanh(xr, 0.0, 6.0), xr, dy)
    _db, dd = dev_rows(dy, Cc + 4, 4, torch.float32)
    _mb, md = dev_rows(mask, Cc + 8, 0, torch.float32)
    yb, yd = dev_rows(torch.zeros(M, Cc), Cc + 12, 8, torch.float32)
    call("dd_op_mask_f32", P(dd), dd.stride(0), P(md), md.stride(0), P(yd), yd.stride(0), M, Cc, hi)
    exact(yd, ref, "mask_f32")
    untouched(yb, 8, Cc, "mask_f32")


@pytest.mark.parametrize("M,Cc", [(37, 12), (4100, 2048)], ids=["small_ragged", "grid_wraps"])
def test_add_and_copy_f32(ops, M, Cc):
    g = torch.Generator().manual_seed(27)
    assert M * (Cc // 4) > WRAP or M < 100
    a, b = torch.randn(M, Cc, generator=g), torch.randn(M, Cc, generator=g)
    ab, ad = dev_rows(a, Cc + 4, 4, torch.float32)
    _bb, bd = dev_rows(b, Cc + 8, 0, torch.float32)
    yb, yd = dev_rows(torch.zeros(M, Cc), Cc + 12, 8, torch.float32)
    call("dd_op_add_f32", P(ad), ad.stride(0), P(bd), bd.stride(0), P(yd), yd.stride(0), M, Cc)
    close32(yd, a.double() + b.double(), "add_f32")
    untouched(yb, 8, Cc, "add_f32")
    call("dd_op_copy_f32", P(bd), bd.stride(0), P(yd), yd.stride(0), M, Cc)
    exact(yd, b, "copy_f32")
    untouched(yb, 8, Cc, "copy_f32")
    call("dd_op_add_f32", P(ad), ad.stride(0), P(bd), bd.stride(0), P(ad), ad.stride(0), M, Cc)          # y == a (op.res_acc)
    close32(ad, a.double() + b.double(), "add_f32 in place")
    untouched(ab, 4, Cc, "add_f32 in place")


def _tied_fraction(x):
    """fraction of the 3x3 / stride 2 / pad 1 windows of x [B, C, H, W] whose maximum occurs more than once"""
    B, Cc, H, W = x.shape
    win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(B, Cc, 9, -1)
    return ((win == win.max(2, keepdim=True).values).sum(2) >= 2).float().mean().item()


@pytest.mark.parametrize("B,H,W,Cc", [(2, 6, 10, 24), (8, 64, 64, 2056)], ids=["small_ragged", "grid_wraps"])
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
def test_maxpool_forward_and_vjp_with_tied_maxima(ops, B, H, W, Cc, f32):
    """Inputs from {0, 1, 2} (as after a ReLU): most windows hold their maximum several times, and the whole gradient of a window goes
    to the FIRST maximum in (ky, kx) scan order -- torch's max_pool2d rule on the CPU.  A wrong tie-break moves whole dy values."""
    g = torch.Generator().manual_seed(28)
    vec = 4 if f32 else 8
    assert B * (H // 2) * (W // 2) * (Cc // vec) > WRAP or B == 2
    x = torch.randint(0, 3, (B, Cc, H, W), generator=g).float()
    assert _tied_fraction(x[:2, :24]) >= 0.5          # (i.i.d. values: a slice stands for the whole tensor)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    dy = torch.randn(B, Cc, H // 2, W // 2, generator=g)
    dy = dy if f32 else bf(dy)
    (gx,) = torch.autograd.grad(ref, xr, dy)
    dt = torch.float32 if f32 else torch.bfloat16
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cc).to(dt).cuda()
    xd, dyd = rows(x), rows(dy)
    yd = torch.empty((B * (H // 2) * (W // 2), Cc), device="cuda", dtype=dt)
    dxd = torch.empty_like(xd)
    sfx = "_f32" if f32 else ""
    call("dd_op_maxpool3x3s2" + sfx, P(xd), P(yd), B, H, W, Cc)
    exact(ops.from_nhwc(yd, B, H // 2, W // 2), ref.detach(), "maxpool fwd")
    call("dd_op_maxpool3x3s2_bwd" + sfx, P(xd), P(dyd), P(dxd), B, H, W, Cc)
    got = ops.from_nhwc(dxd, B, H, W)
    if f32:
        close32(got, gx, "maxpool bwd f32")          # up to four windows' dy summed in fp32
    else:
        assert_close(got, gx, rtol=1e-2, what="maxpool bwd bf16")      # the bound of test_bicubic_maxpool_gap_energy
    # pixels that get no gradient at all must be exactly zero (which pixels get gradient is what a wrong tie-break changes)
    assert float(got[gx == 0].abs().max()) == 0.0


@pytest.mark.parametrize("B,HW,Cc", [(2, 35, 20), (1030, 4, 2048)], ids=["small_ragged", "grid_wraps"])
def test_gap_f32_avg_and_max_with_argmax(ops, B, HW, Cc):
    g = torch.Generator().manual_seed(29)
    assert B * Cc > WRAP or B == 2
    x = torch.randn(B, HW, Cc, generator=g)
    xb, xd = dev_rows(x.reshape(-1, Cc), Cc + 4, 4, torch.float32)
    f = torch.empty((B, Cc), device="cuda")
    call("dd_op_gap_f32", P(xd), xd.stride(0), P(f), None, B, HW, Cc, 0)
    close32(f, x.double().mean(1), "gap_f32 avg")
    gf = torch.randn(B, Cc, generator=g)
    gfd = gf.cuda()
    db, dxd = dev_rows(torch.zeros(B * HW, Cc), Cc + 8, 4, torch.float32)
    call("dd_op_gap_bwd_f32", P(gfd), P(dxd), dxd.stride(0), B, HW, Cc, None)
    close32(dxd.reshape(B, HW, Cc), (gf.double() / HW)[:, None, :].expand(B, HW, Cc), "gap_bwd_f32 avg")
    untouched(db, 4, Cc, "gap_bwd_f32 avg")
    # max form on tied maxima: value, argmax (first maximum in scan order) and the VJP, all exact
    xt = torch.randint(0, 3, (B, HW, Cc), generator=g).float()
    tied = ((xt == xt.max(1, keepdim=True).values).sum(1) >= 2).float().mean().item()
    assert tied >= 0.5, tied
    xr = xt.permute(0, 2, 1).reshape(B, Cc, HW, 1).clone().requires_grad_(True)
    mref, iref = F.adaptive_max_pool2d(xr, 1, return_indices=True)
    (gxr,) = torch.autograd.grad(mref, xr, gf.reshape(B, Cc, 1, 1))
    _tb, td = dev_rows(xt.reshape(-1, Cc), Cc + 4, 4, torch.float32)
    arg = torch.full((B, Cc), -1, device="cuda", dtype=torch.int32)
    call("dd_op_gap_f32", P(td), td.stride(0), P(f), P(arg), B, HW, Cc, 1)
    exact(f, mref.reshape(B, Cc).detach(), "gap_f32 max")
    assert torch.equal(arg.cpu().long(), iref.reshape(B, Cc)), "gap_f32 argmax is not the first maximum"
    db, dxd = dev_rows(torch.zeros(B * HW, Cc), Cc + 8, 4, torch.float32)
    call("dd_op_gap_bwd_f32", P(gfd), P(dxd), dxd.stride(0), B, HW, Cc, P(arg))
    exact(dxd.reshape(B, HW, Cc), gxr.reshape(B, Cc, HW).permute(0, 2, 1), "gap_bwd_f32 max")
    untouched(db, 4, Cc, "gap_bwd_f32 max")


@pytest.mark.parametrize("B,HW,Cc", [(2, 35, 20), (9, 257, 1000)], ids=["small_ragged", "grid_wraps"])
def test_gap_bwd_bf16_with_and_without_mask(ops, B, HW, Cc):
    g = torch.Generator().manual_seed(30)
    assert B * HW * Cc > WRAP or B == 2
    gf = torch.randn(B, Cc, generator=g)
    gfd = gf.cuda()
    mask = bf(torch.randn(B * HW, Cc, generator=g))
    mask[torch.rand(B * HW, Cc, generator=g) < 0.2] = 0.0
    _mb, md = dev_rows(mask, Cc + 6, 2)
    ref = (gf.double() / HW)[:, None, :].expand(B, HW, Cc).reshape(B * HW, Cc)
    for m in (None, md):
        db, dxd = dev_rows(torch.zeros(B * HW, Cc), Cc + 10, 3)
        call("dd_op_gap_bwd", P(gfd), P(dxd), dxd.stride(0), B, HW, Cc, P(m), md.stride(0))
        want = ref if m is None else ref * (mask > 0)
        assert_close(dxd, want, what="gap_bwd mask=%s" % (m is not None))
        if m is not None:
            assert float(dxd.float().cpu()[mask <= 0].abs().max()) == 0.0
        untouched(db, 3, Cc, "gap_bwd")


@pytest.mark.parametrize("B,Cc,H,W,Cpad,ld", [(2, 3, 5, 7, 4, 8), (3, 3, 512, 512, 4, 4)], ids=["small_ragged", "grid_wraps"])
def test_layout_changes(ops, B, Cc, H, W, Cpad, ld):
    """NCHW <-> NHWC: launch_nchw_to_nhwc_f32, dd_op_nchw_f32_to_nhwc_bf16 (plain, duplicated batch, scaled), dd_op_nhwc_to_nchw_f32
    (fp32 and bf16 source; exact with scale 1 / shift 0, and the affine + clamp form of the decoder's output stage)."""
    g = torch.Generator().manual_seed(31)
    assert B * H * W * Cpad > WRAP or B == 2
    x = torch.randn(B, Cc, H, W, generator=g)
    xd = x.cuda()
    nhwc = torch.zeros(B * H * W, Cpad)
    nhwc[:, :Cc] = x.permute(0, 2, 3, 1).reshape(-1, Cc)
    buf, v = dev_rows(torch.zeros(B * H * W, Cpad), ld, 0, torch.float32)
    call("dd_op_nchw_to_nhwc_f32", P(xd), P(v), B, Cc, H, W, Cpad, ld)
    exact(v, nhwc, "nchw_to_nhwc_f32")
    untouched(buf, 0, Cpad, "nchw_to_nhwc_f32")
    back = torch.empty((B, Cc, H, W), device="cuda")
    call("dd_op_nhwc_to_nchw_f32", P(v), 1, P(back), B, Cc, H, W, ld, 1.0, 0.0, 0, 0.0, 0.0)
    exact(back, x, "nhwc_to_nchw_f32 (fp32 rows)")
    call("dd_op_nhwc_to_nchw_f32", P(v), 1, P(back), B, Cc, H, W, ld, 0.5, 0.5, 1, 0.0, 1.0)
    close32(back, (x.double() * 0.5 + 0.5).clamp(0, 1), "nhwc_to_nchw_f32 affine + clamp")
    for dup, scale in ((0, 1.0), (1, 1.0), (0, 0.5)):
        rows = B * H * W * (2 if dup else 1)
        bb, bv = dev_rows(torch.zeros(rows, Cpad), ld, 0)
        call("dd_op_nchw_f32_to_nhwc_bf16", P(xd), P(bv), B, Cc, H, W, Cpad, ld, dup, scale)
        want = bf(nhwc * scale)
        exact(bv, torch.cat([want, want]) if dup else want, "nchw_f32_to_nhwc_bf16 dup=%d scale=%g" % (dup, scale))
        untouched(bb, 0, Cpad, "nchw_f32_to_nhwc_bf16")
        if not dup and scale == 1.0:
            call("dd_op_nhwc_to_nchw_f32", P(bv), 0, P(back), B, Cc, H, W, ld, 1.0, 0.0, 0, 0.0, 0.0)
            exact(back, bf(x), "nhwc_to_nchw_f32 (bf16 rows)")


@pytest.mark.parametrize("B,Cc,HW", [(2, 4, 35), (3, 4, 512 * 512)], ids=["small_ragged", "grid_wraps"])
def test_dup_bwd_sub_scaled_affine(ops, B, Cc, HW):
    g = torch.Generator().manual_seed(32)
    assert B * Cc * HW > WRAP or B == 2
    ld = 8
    gin = bf(torch.randn(2 * B * HW, Cc, generator=g))
    _gb, gd = dev_rows(gin, ld, 0)
    rows = gin.double().reshape(2, B, HW, Cc).permute(0, 1, 3, 2)            # [half, B, C, HW]
    prev = torch.randn(B, Cc, HW, generator=g)
    for halves in (1, 2):
        for acc in (0, 1):
            gz = prev.cuda()
            call("dd_op_dup_bwd", P(gd), ld, P(gz), B, Cc, HW, acc, halves)
            want = rows[0] + (rows[1] if halves == 2 else 0) + prev.double() * acc
            close32(gz, want, "dup_bwd halves=%d accumulate=%d" % (halves, acc))
    assert 0.5 <= rms(prev) / rms(rows[0]) <= 2.0
    a, gg = torch.randn(B * Cc * HW, generator=g), torch.randn(B * Cc * HW, generator=g)
    ad, ggd, out = a.cuda(), gg.cuda(), torch.empty(B * Cc * HW, device="cuda")
    call("dd_op_sub_scaled", P(ad), P(ggd), P(out), C.c_size_t(a.numel()), 0.37)
    close32(out, a.double() - 0.37 * gg.double(), "sub_scaled")
    z, e, b = torch.randn(B * Cc, HW, generator=g), torch.rand(B * Cc, generator=g), torch.randn(B * Cc, generator=g)
    zd, ed, bd, od = z.cuda(), e.cuda(), b.cuda(), torch.empty((B * Cc, HW), device="cuda")
    call("dd_op_affine", P(zd), P(ed), P(bd), P(od), B * Cc, HW)
    close32(od, z.double() * (1 + e.double()[:, None]) + b.double()[:, None], "affine")


@pytest.mark.parametrize("normalize", [0, 1])
def test_energy_with_sample_weights_and_image_scores(ops, normalize):
    """Two train_batch_size groups of different size packed into one batch: w_i = 1 / |group of i| (the reference's .mean() runs per
    group), score_out += weight * sum_i w_i E_i, image_scores[i] += weight * E_i on a non-zero start value, gf = d score / d f."""
    g = torch.Generator().manual_seed(33)
    B, D, K, Ccls = 5, 256, 3, 7
    gs, ls, weight = 1.0, 0.7, 0.5
    f0 = torch.randn(B, D, generator=g).abs()
    Pc = F.normalize(torch.randn(Ccls, D, generator=g), dim=-1)
    Pg = F.normalize(torch.randn(Ccls, K, D, generator=g), dim=-1)
    tg = torch.tensor([3, 1, 6, 0, 3], dtype=torch.int32)
    wts = torch.tensor([1 / 2, 1 / 2, 1 / 3, 1 / 3, 1 / 3])
    f = f0.double().requires_grad_(True)
    fh = f / f.norm(dim=-1, keepdim=True) if normalize else f
    lp = Pg.double()[tg.long()]
    idx = torch.argmax(torch.bmm(fh.unsqueeze(1), lp.permute(0, 2, 1)), -1).squeeze(1)
    E = gs * torch.norm(fh - Pc.double()[tg.long()], dim=1) + ls * torch.norm(fh - lp[torch.arange(B), idx], dim=1)
    total = weight * (wts.double() * E).sum()
    (gf_ref,) = torch.autograd.grad(total, f)
    start_score, start_img = 0.25, torch.linspace(1.0, 2.0, B)
    score = torch.full((1,), start_score, device="cuda")
    img = start_img.cuda()
    gf = torch.empty((B, D), device="cuda")
    fd, dPc, dPg, dtg, dw = f0.cuda(), Pc.cuda(), Pg.cuda(), tg.cuda(), wts.cuda()
    call("dd_op_energy_weighted", P(fd), P(dPc), P(dPg), P(dtg), B, D, K, gs, ls, 1, 1, normalize, weight, P(dw), P(score), P(img), P(gf))
    assert_close(score, (total.detach() + start_score).reshape(1), rtol=1e-5, atol=1e-6, what="energy score")
    assert_close(img, start_img.double() + weight * E.detach(), rtol=1e-5, atol=1e-6, what="image scores")
    assert_close(gf, gf_ref, rtol=1e-4, atol=1e-7, what="energy grad")
    # without weights the same entry is dd_op_energy: w_i = 1 / B
    score.zero_()
    call("dd_op_energy_weighted", P(fd), P(dPc), P(dPg), P(dtg), B, D, K, gs, ls, 1, 1, normalize, weight, None, P(score), None, P(gf))
    assert_close(score, (weight * E.detach().mean()).reshape(1), rtol=1e-5, atol=1e-6, what="energy score, uniform weights")


@pytest.mark.parametrize("B,S,p,Cc,ld", [(2, 12, 4, 3, 4), (3, 512, 16, 3, 4)], ids=["small_ragged", "grid_wraps"])
def test_patchify_and_its_transpose(ops, B, S, p, Cc, ld):
    g = torch.Generator().manual_seed(34)
    assert B * S * S * Cc > WRAP or B == 2
    img = torch.randn(B, Cc, S, S, generator=g)
    ib, iv = dev_rows(img.permute(0, 2, 3, 1).reshape(-1, Cc), ld, 0, torch.float32)
    n, K = (S // p) ** 2, Cc * p * p
    out = torch.empty((B * n, K), device="cuda", dtype=torch.bfloat16)
    call("dd_op_patchify", P(iv), ld, P(out), B, S, p, Cc)
    exact(out, bf(F.unfold(img, p, stride=p).transpose(1, 2).reshape(B * n, K)), "patchify")
    gout = bf(torch.randn(B * n, K, generator=g))
    gd = gout.to(torch.bfloat16).cuda()
    gb, gv = dev_rows(torch.zeros(B * S * S, Cc), ld, 0, torch.float32)
    call("dd_op_patchify_bwd", P(gd), P(gv), ld, B, S, p, Cc)
    want = F.fold(gout.reshape(B, n, K).transpose(1, 2), (S, S), p, stride=p)
    exact(gv, want.permute(0, 2, 3, 1).reshape(-1, Cc), "patchify bwd")
    untouched(gb, 0, Cc, "patchify bwd")


@pytest.mark.parametrize("B,np_,Wd", [(2, 9, 20), (9, 256, 1000)], ids=["small_ragged", "grid_wraps"])
def test_vit_embed_and_its_transpose(ops, B, np_, Wd):
    g = torch.Generator().manual_seed(35)
    assert B * np_ * Wd > WRAP or B == 2
    patches = bf(torch.randn(B * np_, Wd, generator=g))
    cls, pos = torch.randn(Wd, generator=g), torch.randn(np_ + 1, Wd, generator=g)
    _pb, pd = dev_rows(patches, Wd + 4, 4)
    ob, od = dev_rows(torch.zeros(B * (np_ + 1), Wd), Wd + 6, 2)
    cd, psd = cls.cuda(), pos.cuda()
    call("dd_op_vit_embed", P(pd), pd.stride(0), P(cd), P(psd), P(od), od.stride(0), B, np_, Wd)
    want = torch.cat([cls.double().expand(B, 1, Wd), patches.double().reshape(B, np_, Wd)], dim=1) + pos.double()
    assert_close(od, want.reshape(-1, Wd), what="vit_embed")
    untouched(ob, 2, Wd, "vit_embed")
    gout = bf(torch.randn(B * (np_ + 1), Wd, generator=g))
    _gb, gd = dev_rows(gout, Wd + 2, 1)
    qb, qd = dev_rows(torch.zeros(B * np_, Wd), Wd + 10, 3)
    call("dd_op_vit_embed_bwd", P(gd), gd.stride(0), P(qd), qd.stride(0), B, np_, Wd)
    exact(qd, gout.reshape(B, np_ + 1, Wd)[:, 1:].reshape(-1, Wd), "vit_embed bwd")
    untouched(qb, 3, Wd, "vit_embed bwd")


# the shipped geometries: 512 / 384 / 640 / 768 / 1024-pixel images -> the guides' 224; the tiny configs (latent 4 -> 32 pixels up to 56,
# latent 16 -> 128 pixels to 56 and, for the tiny MobileNetV2 / ViT guides, to 64); a non-square one; 512 -> 224 at a batch that wraps
BICUBIC_GEOMETRIES = [(1, 512, 512, 224, 224), (1, 384, 384, 224, 224), (1, 640, 640, 224, 224), (1, 768, 768, 224, 224),
                      (1, 1024, 1024, 224, 224), (2, 32, 32, 56, 56), (2, 128, 128, 56, 56), (2, 128, 128, 64, 64), (2, 96, 352, 56, 224),
                      (42, 512, 512, 224, 224)]
_GEO_IDS = ["%dx%dx%d_to_%dx%d" % geo for geo in BICUBIC_GEOMETRIES]


def _nhwc(t, ld, dtype):
    B, Cc, H, W = t.shape
    return dev_rows(t.permute(0, 2, 3, 1).reshape(-1, Cc), ld, 0, dtype)


@pytest.mark.parametrize("geo", BICUBIC_GEOMETRIES, ids=_GEO_IDS)
def test_bicubic_f32(ops, geo):
    """launch_bicubic_f32 and its transpose (fp32 and bf16 output) against F.interpolate(mode="bicubic") and its autograd transpose IN
    FLOAT64.  The source coordinate scale * (o + 0.5) - 0.5 is formed in fp32 by torch's fp32 path and by the kernel alike, which alone
    costs up to 1e-4 of max|ref| against float64 (1024 -> 224), so the file's 2e-5 cannot hold.  The bound is taken from the reference's
    own fp32 error on the same input: floor = max|interp_fp32_cpu - interp_fp64|, and
        max|kernel - interp_fp64| <= 2 * floor + 2e-5 * max|ref|
    (factor 2: one more fp32 evaluation of the same formula).  The measured err / floor is printed per geometry.
    Measured on an MI355X, err / floor forward | transpose (floor as a fraction of max|ref| in brackets):
        512 -> 224   1.00 | 1.00  (6.4e-5)      384 -> 224   1.00 | 1.00  (2.2e-5)      640 -> 224   1.00 | 1.00  (6.2e-5)
        768 -> 224   1.00 | 1.00  (5.7e-5)     1024 -> 224   1.00 | 1.00  (1.1e-4)       32 -> 56    0.98 | 1.00  (3.4e-6)
        128 -> 56    1.00 | 1.00  (1.5e-5)      128 -> 64    1.00 | 0.78  (1.3e-7: scale 2 is exact)
        96 x 352 -> 56 x 224   1.00 | 1.00      512 -> 224, 42 images   1.00 | 1.00
    i.e. the kernels reproduce torch's own fp32 evaluation; the whole error against float64 is the fp32 source coordinate.
    """
    B, Hs, Ws, Hd, Wd = geo
    g = torch.Generator().manual_seed(36)
    assert B * Hd * Wd > WRAP or B <= 2
    img = torch.randn(B, 3, Hs, Ws, generator=g)
    i64 = img.double().requires_grad_(True)
    ref = F.interpolate(i64, size=(Hd, Wd), mode="bicubic")
    dd = torch.randn(B, 3, Hd, Wd, generator=g)
    (gref,) = torch.autograd.grad(ref, i64, dd.double())
    i32 = img.clone().requires_grad_(True)
    r32 = F.interpolate(i32, size=(Hd, Wd), mode="bicubic")
    (g32,) = torch.autograd.grad(r32, i32, dd)
    ref = ref.detach()
    floor_f = (r32.detach().double() - ref).abs().max().item()
    floor_b = (g32.double() - gref).abs().max().item()
    _sb, sv = _nhwc(img, 4, torch.float32)
    db, dv = dev_rows(torch.zeros(B * Hd * Wd, 8), 12, 0, torch.float32)
    call("dd_op_bicubic_f32", P(sv), 4, P(dv), dv.stride(0), B, Hs, Ws, Hd, Wd, 3, 8)
    got = dv.double().cpu().reshape(B, Hd, Wd, 8).permute(0, 3, 1, 2)
    err_f = (got[:, :3] - ref).abs().max().item()
    assert float(got[:, 3:].abs().max()) == 0.0, "channels C .. Cpad must be zero-filled"
    untouched(db, 0, 8, "bicubic_f32")
    _gb, gv = _nhwc(dd, 4, torch.float32)
    ob, ov = dev_rows(torch.zeros(B * Hs * Ws, 3), 4, 0, torch.float32)
    call("dd_op_bicubic_bwd_f32", P(gv), 4, P(ov), 0, 4, B, Hs, Ws, Hd, Wd, 3)
    gotb = ov.double().cpu().reshape(B, Hs, Ws, 3).permute(0, 3, 1, 2)
    err_b = (gotb - gref).abs().max().item()
    untouched(ob, 0, 3, "bicubic_bwd_f32")
    print("bicubic f32 %s: forward err %.3g floor %.3g ratio %.2f | transpose err %.3g floor %.3g ratio %.2f"
          % ("%dx%dx%d->%dx%d" % geo, err_f, floor_f, err_f / max(floor_f, 1e-30), err_b, floor_b, err_b / max(floor_b, 1e-30)))
    assert err_f <= 2 * floor_f + 2e-5 * ref.abs().max().item(), (err_f, floor_f)
    assert err_b <= 2 * floor_b + 2e-5 * gref.abs().max().item(), (err_b, floor_b)
    hb, hv = dev_rows(torch.zeros(B * Hs * Ws, 3), 8, 0)                   # bf16 rows: the VAE decoder's gradient slab
    call("dd_op_bicubic_bwd_f32", P(gv), 4, P(hv), 1, 8, B, Hs, Ws, Hd, Wd, 3)
    assert_close(hv.float().cpu().reshape(B, Hs, Ws, 3).permute(0, 3, 1, 2), gref, what="bicubic_bwd_f32, bf16 output")
    untouched(hb, 0, 3, "bicubic_bwd_f32 bf16 output")


@pytest.mark.parametrize("geo", BICUBIC_GEOMETRIES, ids=_GEO_IDS)
def test_bicubic_bf16(ops, geo):
    """the bf16 resize (the bf16 guides: CLIP ViT) and its transpose at the same geometries; bf16 rounding dominates: assert_close defaults"""
    B, Hs, Ws, Hd, Wd = geo
    g = torch.Generator().manual_seed(37)
    img = bf(torch.randn(B, 3, Hs, Ws, generator=g))
    i64 = img.double().requires_grad_(True)
    ref = F.interpolate(i64, size=(Hd, Wd), mode="bicubic")
    dd = bf(torch.randn(B, 3, Hd, Wd, generator=g))
    (gref,) = torch.autograd.grad(ref, i64, dd.double())
    _sb, sv = _nhwc(img, 8, torch.bfloat16)
    db, dv = dev_rows(torch.zeros(B * Hd * Wd, 8), 16, 0)
    call("dd_op_bicubic", P(sv), 8, P(dv), dv.stride(0), B, Hs, Ws, Hd, Wd, 3, 8)
    got = ops.from_nhwc(dv, B, Hd, Wd)
    assert_close(got[:, :3], ref.detach(), what="bicubic bf16 fwd")
    assert float(got[:, 3:].abs().max()) == 0.0
    untouched(db, 0, 8, "bicubic bf16")
    _gb, gv = _nhwc(dd, 8, torch.bfloat16)
    ob, ov = dev_rows(torch.zeros(B * Hs * Ws, 3), 8, 0)
    call("dd_op_bicubic_bwd", P(gv), 8, P(ov), 8, B, Hs, Ws, Hd, Wd, 3)
    assert_close(ops.from_nhwc(ov, B, Hs, Ws), gref, what="bicubic bf16 bwd")
    untouched(ob, 0, 3, "bicubic bf16 bwd")
