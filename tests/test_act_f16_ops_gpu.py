"""The fp16 library (libdistdiff_hip_f16.so: the kernels compiled with -DDD_ACT_F16) op by op against float64, one case per kernel.  This is
where a conversion site that still speaks bf16 shows: the tiny engine never reaches the halo / pps / ws kernels.

Inputs are drawn in fp32 and rounded to fp16; the reference is torch float64 on the rounded inputs (computed on the device).

Convolution / GEMM, per element:   |y - ref| <= 2^-11 |ref| + K 2^-24 A,   A = the same conv on absolute values (bias and residual included)
    -- one RNE store, and the worst case of a K-term fp32 accumulation in any order.  Derived, not measured.  GEGLU's polynomial GELU adds
    its stated 5e-5 absolute (times |hidden|: the product is hidden * gelu(gate)).  CF_STATS partials are compared with the statistics of
    the STORED values to 1e-5 (of max(1, largest |value| of the block) for the mean, of max(1, sum of squares) for M2).
Attention forward:   every element within 2^-10 max|v| of the reference (p and O rounded once each to half; scores are exact products
    accumulated in fp32; the hardware exp2 takes the factor 2).
Forward norms:   rel-L2 <= 5e-4 (one RNE store: rms 2^-11 / sqrt 3 = 2.8e-4).
Backward kernels (attention dQ / dK / dV, GroupNorm, LayerNorm):   rel-L2 against float64, bound = 2 x the worst value measured on an MI355X
    (BWD_BOUND below, the measured values beside it), and the same problem through the bf16 library (inputs rounded to bf16) must be at
    least 2 x further from its own reference (three more mantissa bits predict about 8 x).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_ref as nr

pytestmark = pytest.mark.gpu
H16, B16 = torch.float16, torch.bfloat16
F64 = torch.float64
GELU_POLY_ABS = 5e-5


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distdiff_amd import _lib, ops
    assert _lib.lib("fp16").dd_act_dtype() == 1 and _lib.lib("bf16").dd_act_dtype() == 0
    return ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.to(F64).cpu(), b.to(F64).cpu()
    assert torch.isfinite(a).all()
    return ((a - b).norm() / b.norm()).item()


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution / GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_bound_check(name, y, ref, absref, K, extra=None):
    tol = 2.0 ** -11 * ref.abs() + K * 2.0 ** -24 * absref
    if extra is not None:
        tol = tol + extra
    err = (y.to(F64) - ref).abs()
    assert torch.isfinite(y.float()).all(), name
    worst = torch.where(tol > 0, err / tol, err * float("inf")).nan_to_num(nan=0.0).max().item()      # bound 0 (masked out): exactly 0
    print("%s: worst error / bound %.3f, rel-L2 %.2e" % (name, worst, (err.norm() / ref.norm()).item()))
    assert worst <= 1.0, "%s: %d elements beyond the bound, worst %.3f of it" % (name, int((err > tol).sum()), worst)


def stats_errors(part, vals):
    """CF_STATS partials [M / 64, N, 2] = (mean, M2) per 64-row block and channel against those of vals [M, N]: the largest error of the
    mean as a fraction of max(1, largest |value| of the block), of M2 as a fraction of max(1, sum of squares of the block)"""
    rows = vals.to(F64).view(-1, 64, vals.shape[1])
    mean, m2 = rows.mean(1), ((rows - rows.mean(1, keepdim=True)) ** 2).sum(1)
    em = (part[..., 0].to(F64) - mean).abs() / rows.abs().amax(1).clamp(min=1.0)
    e2 = (part[..., 1].to(F64) - m2).abs() / (rows ** 2).sum(1).clamp(min=1.0)
    return em.max().item(), e2.max().item()


def conv_inputs(seed, B, H, W, Cin, Cout, k=3, mode=0):
    g = gen(seed)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(H16)
    b = torch.randn(Cout, generator=g) * 0.5 if mode == 0 else None
    xc = Cin if mode == 0 else Cout
    x = torch.randn(B, xc, H, W, generator=g).to(H16)
    return x, w, b


def nhwc(t):                    # [B, C, H, W] -> [B*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def conv_ref(x, w, b, stride=1, mode=0, res=None):
    """float64 conv (or, mode 1, its input-gradient form: conv_transpose of the same weight) on the device, and the same on absolute values"""
    xd, wd = x.cuda().to(F64), w.cuda().to(F64)
    f = (lambda a, ww: F.conv2d(a, ww, stride=stride, padding=w.shape[-1] // 2)) if mode == 0 else \
        (lambda a, ww: F.conv_transpose2d(a, ww, stride=1, padding=w.shape[-1] // 2))
    ref, ab = nhwc(f(xd, wd)), nhwc(f(xd.abs(), wd.abs()))
    if b is not None:
        ref, ab = ref + b.cuda().to(F64), ab + b.cuda().to(F64).abs()
    if res is not None:
        ref, ab = ref + res.to(F64), ab + res.to(F64).abs()
    return ref, ab


CONV3 = {   # name: (kind, B, H, W, Cin, Cout, stride, mode, flags, ksplit)   flags: r residual, s CF_STATS, f fp32 output, m mask
    "halo_bias_res_stats": (1, 6, 128, 128, 64, 160, 1, 0, "rs", 0),
    "halo_persist_bias_res_stats": (2, 6, 128, 128, 128, 128, 1, 0, "rs", 0),
    "halo_narrow_n4_f32": (1, 6, 128, 128, 64, 4, 1, 0, "f", 1),
    "halo_8x8_chunk_split": (1, 8, 8, 8, 256, 320, 1, 0, "", 0),
    "general_stride2": (0, 1, 64, 64, 64, 128, 2, 0, "", 0),
    "general_stride2_f32": (0, 1, 64, 64, 64, 128, 2, 0, "f", 1),
    "general_stride2_mask_big": (0, 1, 64, 64, 64, 128, 2, 0, "m", 4),
    "general_stride2_splitk_big": (0, 1, 64, 64, 64, 128, 2, 0, "", 4),
    "general_small_m256": (0, 1, 16, 16, 64, 128, 1, 0, "", 0),
    "general_big_stride2_stats": (0, 8, 64, 64, 64, 128, 2, 0, "s", 1),             # conv_gemm_big_kernel's own CF_STATS epilogue
    "halo_dgrad_128_to_160": (1, 6, 128, 128, 160, 128, 1, 1, "", 0),      # transposed + flipped packing: 128 gradient channels -> 160
}


def run_conv3x3(ops, name):
    """one case of CONV3 against its bound -> (CF_STATS partials or None, y, float64 reference)"""
    kind, B, H, W, Cin, Cout, stride, mode, fl, ksplit = CONV3[name]
    x, w, b = conv_inputs(sum(map(ord, name)), B, H, W, Cin, Cout, mode=mode)
    pk = ops.PackedConv(w.float(), 1, mode=mode, bias=b, dtype=H16)
    assert pk.w.dtype == H16
    Ho, Wo = H // stride, W // stride
    M, N = B * Ho * Wo, pk.N
    g = gen(7)
    kw = dict(stride=stride, ksplit=ksplit, out_f32="f" in fl)
    res = torch.randn(M, N, generator=g).to(H16).cuda() if "r" in fl else None
    mask = (torch.randn(M, N, generator=g) * 1.0).to(H16).cuda() if "m" in fl else None
    stats = torch.full((M // 64, N, 2), float("nan"), device="cuda") if "s" in fl else None
    kw.update(res=res, stats=stats)
    if mask is not None:
        kw["mask"] = mask
    xd = nhwc(x).cuda()
    plan = ops.conv_gemm_plan(xd, pk, B, H, W, Ho, Wo, **{k: (True if (k in ("res", "stats") and v is not None) else v) for k, v in kw.items()})
    assert ops.CONV_GEMM_KINDS.index(plan[0]) == kind, plan
    if name == "halo_8x8_chunk_split":
        assert plan[2] > 1, plan                  # the chunk split with its splitk_reduce
    if name.endswith("_big") or "_big_" in name:
        assert plan[1].startswith("big_"), plan   # conv_gemm_big_kernel
    if N < 8:                                     # the narrow form writes into 8-wide rows
        ybuf = torch.full((M, 8), float("nan"), device="cuda")
        kw["y"] = ybuf[:, :N]
    y = ops.conv_gemm(xd, pk, B, H, W, Ho, Wo, **kw)
    torch.cuda.synchronize()
    assert y.dtype == (torch.float32 if "f" in fl else H16)
    ref, ab = conv_ref(x, w, b, stride, mode, res)
    if mask is not None:
        keep = (mask.float() > 0).to(F64)
        ref, ab = ref * keep, ab * keep
    conv_bound_check(name, y, ref, ab, pk.K)
    return stats, y, ref


@pytest.mark.parametrize("name", list(CONV3))
def test_conv3x3(ops, name):
    run_conv3x3(ops, name)


@pytest.mark.parametrize("name", [n for n, c in CONV3.items() if "s" in c[8]])
def test_conv_stats_partials(ops, name):
    """CF_STATS against the statistics of the STORED values, to 1e-5: the fp16 build sums the rounded values (common.h DD_STORED4), so what
    is left is the fp32 arithmetic of 64-term sums and of M2 = sq - sa * mean (64 x 2^-24 = 3.8e-6 of the sum of squares at worst).  (Summed
    in front of the store, as the bf16 build does, the same partials sit 5e-5 / 3.9e-4 from the stored values' statistics.)"""
    stats, y, _ref = run_conv3x3(ops, name)
    em, e2 = stats_errors(stats, y)
    print("%s: CF_STATS against the stored values: mean %.2e, M2 %.2e (of 1e-5)" % (name, em, e2))
    assert em <= 1e-5 and e2 <= 1e-5


GEMM = {    # name: (kind, M, K, N, geglu, flags)   flags: r residual, l LayerNorm folded, g GEGLU raw stash
    "ws_bias": (3, 32768, 320, 320, False, ""),
    "ws_geglu_raw": (3, 32768, 320, 512, True, "g"),
    "pps_bias_res": (4, 49152, 256, 320, False, "r"),
    "pps_lnfold": (4, 49152, 256, 320, False, "l"),
}


@pytest.mark.parametrize("name", list(GEMM))
def test_pointwise_gemm(ops, name):
    kind, M, K, N, geglu, fl = GEMM[name]
    g = gen(sum(map(ord, name)))
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(H16)
    b = torch.randn(N, generator=g) * 0.5
    x = torch.randn(M, K, generator=g).to(H16)
    pk = ops.PackedConv(w.float(), 0, geglu=geglu, bias=b, dtype=H16)
    kw = dict(ksplit=1)
    xd, wd, bd = x.cuda().to(F64), w.cuda().to(F64), b.cuda().to(F64)
    acc, ab = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if "l" in fl:                                   # out = rstd (acc - mean c1) + b: x is the raw LayerNorm input, c1 the column sums
        ln = torch.stack((torch.randn(M, generator=g) * 0.5, torch.rand(M, generator=g) + 0.5), dim=1)
        c1 = w.float().sum(1)
        kw.update(ln_stats=ln.cuda(), ln_c1=c1.cuda())
        mean, rstd, c1d = ln[:, 0].cuda().to(F64)[:, None], ln[:, 1].cuda().to(F64)[:, None], c1.cuda().to(F64)[None, :]
        ref, ab = rstd * (acc - mean * c1d) + bd, rstd * (ab + mean.abs() * c1d.abs()) + bd.abs()
    else:
        ref, ab = acc + bd, ab + bd.abs()
    if "r" in fl:
        res = torch.randn(M, N, generator=g).to(H16).cuda()
        kw["res"] = res
        ref, ab = ref + res.to(F64), ab + res.to(F64).abs()
    if "g" in fl:
        kw["raw"] = torch.full((M, N), float("nan"), dtype=H16, device="cuda")
    plan = ops.conv_gemm_plan(None, pk, 1, M, 1, M, 1, **{k: (True if k in ("res", "ln_stats") else v) for k, v in kw.items()})
    assert ops.CONV_GEMM_KINDS.index(plan[0]) == kind, plan
    y = ops.conv_gemm(x.cuda(), pk, 1, M, 1, M, 1, **kw)
    torch.cuda.synchronize()
    assert y.dtype == H16
    if geglu:                                        # diffusers GEGLU: hidden * gelu(gate), (hidden | gate) = the two halves of the projection
        Fh = N // 2
        hid, gate = ref[:, :Fh], ref[:, Fh:]
        out = hid * F.gelu(gate)
        # first-order propagation of the two fp32 sums' errors through the product, plus the polynomial's 5e-5 on gelu(gate)
        e = K * 2.0 ** -24 * ab
        dgelu = 0.5 * (1 + torch.erf(gate / math.sqrt(2))) + gate * torch.exp(-gate * gate / 2) / math.sqrt(2 * math.pi)
        extra = e[:, :Fh] * F.gelu(gate).abs() + hid.abs() * (e[:, Fh:] * dgelu.abs() + GELU_POLY_ABS)
        conv_bound_check(name, y, out, torch.zeros_like(out), K, extra=extra * 1.01)
        # the raw stash holds the rounded projection in packed order: 32-column groups of 16 hidden | 16 gate
        raw = kw["raw"].to(F64).view(M, N // 32, 2, 16)
        conv_bound_check(name + " raw hidden", raw[:, :, 0].reshape(M, Fh), hid, ab[:, :Fh], K)
        conv_bound_check(name + " raw gate", raw[:, :, 1].reshape(M, Fh), gate, ab[:, Fh:], K)
    else:
        conv_bound_check(name, y, ref, ab, K)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def attn_inputs(seed, B, H, Nq, Nk, D, dt=H16, spread=1.0):
    g = gen(seed)
    q = (torch.randn(B * Nq, H * D, generator=g) * spread).to(dt)
    k = (torch.randn(B * Nk, H * D, generator=g) * spread).to(dt)
    v = torch.randn(B * Nk, H * D, generator=g).to(dt)
    do = torch.randn(B * Nq, H * D, generator=g).to(dt)
    return q, k, v, do


def attn_ref(q, k, v, B, H, Nq, Nk, D, scale, causal=False, do=None):
    """float64 on the device: o [B*Nq, H*D] (and dq, dk, dv with do)"""
    def heads(t, n):
        return t.cuda().to(F64).view(B, n, H, D).permute(0, 2, 1, 3)
    qh, kh, vh = heads(q, Nq), heads(k, Nk), heads(v, Nk)
    if do is not None:
        qh, kh, vh = qh.requires_grad_(True), kh.requires_grad_(True), vh.requires_grad_(True)
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device="cuda").triu(1), float("-inf"))
    o = torch.softmax(s, -1) @ vh
    flat = lambda t, n: t.permute(0, 2, 1, 3).reshape(B * n, H * D)
    if do is None:
        return flat(o, Nq)
    gq, gk, gv = torch.autograd.grad(o, (qh, kh, vh), heads(do, Nq))
    return flat(o.detach(), Nq), flat(gq, Nq), flat(gk, Nk), flat(gv, Nk)


ATTN_FWD = {    # name: (B, H, Nq, Nk, D, flags)   p: prescaled queries, c: causal, g: GEMM route (scratch offered)
    "d40_256": (1, 2, 256, 256, 40, ""),
    "d40_256_prescaled": (1, 2, 256, 256, 40, "p"),
    "d40_q96_ragged": (1, 2, 96, 256, 40, ""),
    "shortk_d40": (1, 2, 64, 77, 40, ""),
    "shortk_d64": (1, 2, 64, 77, 64, ""),
    "shortk_d80": (1, 2, 64, 77, 80, ""),
    "d64_128": (1, 2, 128, 128, 64, ""),
    "d160_64": (1, 2, 64, 64, 160, ""),
    "causal_d64_77": (1, 2, 77, 77, 64, "c"),
    "gemm_d512_256": (1, 1, 256, 256, 512, "g"),
}


@pytest.mark.parametrize("name", list(ATTN_FWD))
def test_attention_forward(ops, name):
    B, H, Nq, Nk, D, fl = ATTN_FWD[name]
    q, k, v, _ = attn_inputs(sum(map(ord, name)), B, H, Nq, Nk, D)
    scale = 1.0 / math.sqrt(D)
    qd = q
    kw, sc = {}, scale
    if "p" in fl:           # the producer folds scale * log2(e) into q (one more rounding: the reference takes the rounded product)
        qd = (q.float() * (scale * math.log2(math.e))).to(H16)
        kw, sc = dict(q_prescaled=True), math.log(2.0)
    ref = attn_ref(qd if "p" in fl else q, k, v, B, H, Nq, Nk, D, (math.log(2.0) if "p" in fl else scale), causal="c" in fl)
    if "g" in fl:
        (o, lse), plans = ops.attention_planned(qd.cuda(), k.cuda(), v.cuda(), B, H, Nq, Nk, D, sc, ws_images=1)
        assert plans[0]["route"] == "gemm", plans
    else:
        (o, lse), plans = ops.attention_planned(qd.cuda(), k.cuda(), v.cuda(), B, H, Nq, Nk, D, sc, causal="c" in fl, **kw)
        if name.startswith("shortk"):
            assert plans[0]["route"] == "shortk", plans
        if "p" in fl:
            assert plans[0]["lazy"], plans
    torch.cuda.synchronize()
    assert o.dtype == H16 and torch.isfinite(o.float()).all()
    err = (o.to(F64) - ref).abs().max().item()
    bound = 2.0 ** -10 * v.float().abs().max().item()
    print("%s (%s): max error %.3e, bound %.3e" % (name, plans[0]["route"], err, bound))
    assert err <= bound


def test_attention_lazy_reference_runs_away_in_fp16(ops):
    """The lazy-reference softmax exponentiates later tiles against the first tile's maximum.  Keys whose scores climb by far more than
    2^16 above it overflow p in half: the kernel must notice (inf / NaN in O) and repeat with the per-tile maximum, p <= 2^8."""
    B, H, Nq, Nk, D = 1, 2, 256, 512, 40
    q, k, v, _ = attn_inputs(5, B, H, Nq, Nk, D)
    k = (k.float() * torch.linspace(0.2, 6.0, Nk).repeat_interleave(1)[:, None]).to(H16)      # later keys score higher and higher
    q = (q.float() * 3.0).to(H16)
    scale = 1.0 / math.sqrt(D)
    qd = (q.float() * (scale * math.log2(math.e))).to(H16)
    ref = attn_ref(qd, k, v, B, H, Nq, Nk, D, math.log(2.0))
    (o, lse), plans = ops.attention_planned(qd.cuda(), k.cuda(), v.cuda(), B, H, Nq, Nk, D, math.log(2.0), q_prescaled=True)
    assert plans[0]["lazy"]
    s = (qd.float().view(Nq, H, D).permute(1, 0, 2) @ k.float().view(Nk, H, D).permute(1, 2, 0))
    climb = (s[:, :, 128:].amax(-1) - s[:, :, :128].amax(-1)).max().item()      # against the first tile (64 or 128 keys: at least this)
    assert climb > 17.0, climb                                   # log2 domain: some row does leave the half range of the optimistic pass
    err = (o.to(F64) - ref).abs().max().item()
    print("runaway rows: climb 2^%.1f, max error %.3e" % (climb, err))
    assert torch.isfinite(o.float()).all() and err <= 2.0 ** -10 * v.float().abs().max().item()


def test_fp8_pv_is_refused(ops):
    q, k, v, _ = attn_inputs(3, 1, 2, 128, 128, 64)
    with pytest.raises(RuntimeError):
        ops.attention(q.cuda(), k.cuda(), v.cuda(), 1, 2, 128, 128, 64, 0.125, pv_fp8=True)
    o, _ = ops.attention(q.to(B16).cuda(), k.to(B16).cuda(), v.to(B16).cuda(), 1, 2, 128, 128, 64, 0.125, pv_fp8=True)   # the bf16 library still has it
    assert o.dtype == B16


# ---- backward kernels: measured bounds ---------------------------------------------------------------------------------------------
# rel-L2 of the fp16 library against float64, measured on an MI355X (gfx950); the bound is twice the worst value of its row.
#   attention d40 self 256x256 (dq dk dv):   fp16 3.01e-4 2.95e-4 2.93e-4      bf16 library 2.41e-3 2.35e-3 2.36e-3
#   attention d40 cross 64x77 (dq):          fp16 3.00e-4                      bf16 2.46e-3
#   attention d512 GEMM route (dq dk dv):    fp16 2.93e-4 2.92e-4 2.96e-4      bf16 2.39e-3 2.37e-3 2.35e-3
#   GroupNorm(+SiLU) backward, the 15 cases of nr.GN_CASES:   fp16 1.80e-4 .. 2.10e-4 (worst: eps1e-6)      bf16 1.58e-3 .. 1.68e-3
#   LayerNorm backward, the 20 cases of nr.LN_CASES:          fp16 1.99e-4 .. 2.19e-4 (worst: C8_M17)       bf16 1.56e-3 .. 1.96e-3
# (the figures repeat bit for bit from run to run; the forward norms measure 2.0e-4 .. 2.3e-4 against their 5e-4)
BWD_BOUND = {"attn_self": 6.03e-4, "attn_cross": 6.0e-4, "attn_gemm": 5.91e-4, "gn_bwd": 4.21e-4, "ln_bwd": 4.39e-4}


def _bwd_verdict(key, name, e16, ebf):
    print("%s: fp16 rel-L2 %s, bf16 %s" % (name, " ".join("%.3e" % e for e in e16), " ".join("%.3e" % e for e in ebf)))
    for a, b in zip(e16, ebf):
        assert b >= 2.0 * a, "%s: the bf16 library (%.3e) is not 2 x further from its reference than the fp16 one (%.3e)" % (name, b, a)
    assert BWD_BOUND[key] is not None, "no measured bound recorded for %s" % key
    assert max(e16) <= BWD_BOUND[key], "%s: %.3e beyond the bound %.3e" % (name, max(e16), BWD_BOUND[key])


def _attn_bwd(ops, dt, B, H, Nq, Nk, D, cross, gemm):
    q, k, v, do = attn_inputs(29, B, H, Nq, Nk, D, dt)
    scale = 1.0 / math.sqrt(D)
    _, gq, gk, gv = attn_ref(q, k, v, B, H, Nq, Nk, D, scale, do=do)
    if gemm:
        out = ops.attention_gemm(q.cuda(), k.cuda(), v.cuda(), B, H, Nq, Nk, D, scale, d_o=do.cuda(), ws_images=1)
    else:
        out = ops.attention(q.cuda(), k.cuda(), v.cuda(), B, H, Nq, Nk, D, scale, d_o=do.cuda(), need_dkv=not cross)
    torch.cuda.synchronize()
    assert out[2].dtype == dt
    return [rel(out[2], gq)] if cross else [rel(out[2], gq), rel(out[3], gk), rel(out[4], gv)]


@pytest.mark.parametrize("key,shape", [("attn_self", (1, 2, 256, 256, 40, False, False)), ("attn_cross", (1, 2, 64, 77, 40, True, False)),
                                       ("attn_gemm", (1, 1, 256, 256, 512, False, True))])
def test_attention_backward(ops, key, shape):
    _bwd_verdict(key, key, _attn_bwd(ops, H16, *shape), _attn_bwd(ops, B16, *shape))


def _gn(ops, dt, case, bwd):
    I = nr.gn_inputs(case)
    x, dy = I.x.to(dt), I.dy.to(dt)
    R = nr.reference(x, I.gamma, I.beta, I.G, I.eps, I.silu, dy if bwd else None)
    xd = x.view(-1, I.C).cuda()
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    y, stats = ops.groupnorm(xd, ga, be, I.B, I.HW, I.G, I.eps, I.silu)
    if not bwd:
        return rel(y.view(I.B, I.HW, I.C), R.ref)
    dx = ops.groupnorm(xd, ga, be, I.B, I.HW, I.G, I.eps, I.silu, dy=dy.view(-1, I.C).cuda(), stats=stats)
    return rel(dx.view(I.B, I.HW, I.C), R.dx)


def _ln(ops, dt, case, bwd):
    I = nr.ln_inputs(case)
    x, dy = I.x.to(dt), I.dy.to(dt)
    R = nr.layernorm_reference(x, I.gamma, I.beta, nr.LN_EPS, dy if bwd else None)
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    y, stats = ops.layernorm(x.cuda(), ga, be, nr.LN_EPS)
    if not bwd:
        return rel(y, R.ref[:, 0])
    return rel(ops.layernorm(x.cuda(), ga, be, nr.LN_EPS, dy=dy.cuda(), stats=stats), R.dx[:, 0])


# The norm cases are those of tests/norm_ref.py (the shapes of tests/test_norm_*): their inputs are bf16-valued, hence exact in half too, so
# both libraries are given the very same problem.
@pytest.mark.parametrize("name", list(nr.GN_CASES))
def test_groupnorm_forward(ops, name):
    e = _gn(ops, H16, nr.GN_CASES[name], False)
    print("GroupNorm forward %s: rel-L2 %.3e" % (name, e))
    assert e <= 5e-4


@pytest.mark.parametrize("case", nr.LN_CASES, ids=nr.ln_id)
def test_layernorm_forward(ops, case):
    e = _ln(ops, H16, case, False)
    print("LayerNorm forward %s: rel-L2 %.3e" % (nr.ln_id(case), e))
    assert e <= 5e-4


def test_groupnorm_backward(ops):
    e16 = [_gn(ops, H16, c, True) for c in nr.GN_CASES.values()]
    ebf = [_gn(ops, B16, c, True) for c in nr.GN_CASES.values()]
    for n, a, b in zip(nr.GN_CASES, e16, ebf):
        print("GroupNorm backward %s: fp16 %.3e bf16 %.3e" % (n, a, b))
    _bwd_verdict("gn_bwd", "GroupNorm backward", e16, ebf)


def test_layernorm_backward(ops):
    e16 = [_ln(ops, H16, c, True) for c in nr.LN_CASES]
    ebf = [_ln(ops, B16, c, True) for c in nr.LN_CASES]
    for c, a, b in zip(nr.LN_CASES, e16, ebf):
        print("LayerNorm backward %s: fp16 %.3e bf16 %.3e" % (nr.ln_id(c), a, b))
    _bwd_verdict("ln_bwd", "LayerNorm backward", e16, ebf)
