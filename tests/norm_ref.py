"""Reference side of the norm-kernel tests: float64 GroupNorm(+SiLU) / LayerNorm, an fp32 emulation of the documented statistic schemes,
and per-element tolerances derived from the arithmetic.  Plain torch on the CPU; nothing here calls or knows the compiled library.

Layout: x is [B, HW, C] ("rows", NHWC) float64 holding bf16-representable values; GroupNorm has G groups of cpg = C / G adjacent
channels and one (mu, rho) per (image, group); LayerNorm is the same operation with B = M rows, HW = 1, G = 1, no activation.

    mu = mean(x), var = mean((x - mu)^2), sigma = sqrt(var), rho = (var + eps)^-1/2, xhat = (x - mu) rho
    pre = xhat gamma_c + beta_c,  ref = act(pre),  act = SiLU or identity
    d = dy act'(pre) gamma_c,  s1 = mean(d),  s2 = mean(d xhat),  dx = rho (d - s1 - xhat s2)

THE FP32 FLOOR.  emu_* below evaluate the kernels' documented statistic schemes in float32 on the CPU: GroupNorm one-pass
(n, mean, M2 = sumsq - sum * mean) per split of ceil(HW / gn_split) rows merged by Chan's formula; the fused form over equal-count
partials (mean = avg(mean_p), M2 = sum M2_p + 64 sum (mean_p - mean)^2); LayerNorm two-pass; row partials one-pass q / C - mean^2.
floor_mu = max |mu_emu - mu|, floor_rho = max |rho_emu - rho| / rho against float64 on the same inputs: what fp32 costs THIS scheme on
THIS input.  It is computed from the inputs alone, so it cannot follow a binary.

STATISTIC BOUNDS (stat_bounds).  r = max |mu| / sigma over the case's groups with sigma > 0.
    d_rho (relative, one per case)  = clamp(4 floor_rho, 2^-20, 2^-18 (1 + r^2))
    d_mu  (absolute, per group)     = max(4 floor_mu, 2^-22 (|mu| + sigma))
4 covers a summation order that differs between emulation and kernel (both are sums of the same rounded terms; a different tree moves
the error by a small factor, not by an order of magnitude).  The lower values are two / four fp32 ulps of the quantity itself.  The upper
clamp is a condition: one-pass variance loses about (1 + r^2) 2^-24 relative, 2^-18 (1 + r^2) is 64 x that, and a kernel that needs more
has a finding, not a case for a higher clamp.

FORWARD TOLERANCE, per element (fwd_tol).  The kernel computes fl(x a + b), a = rho' gamma, b = beta - mu' a (GroupNorm) or
fl((x - mu') rho' gamma + beta) (LayerNorm) with its own statistics mu' = mu + dmu, rho' = rho (1 + drho):
    pre' - pre = gamma rho (x - mu) drho - gamma rho dmu + (fp32 rounding of 3-4 operations on terms of size gamma rho |x|, gamma rho |mu|, |beta|)
so  |pre' - pre| <= |gamma| rho |x - mu| d_rho + |gamma| rho d_mu + 2^-21 (|gamma| rho (|x| + |mu|) + |beta|)      =: e_pre
(2^-21 = 8 half-ulps: each of at most four roundings acts on a partial result no larger than the sum of the magnitudes; factor 2 spare).
The activation multiplies an argument error by at most max |SiLU'| = 1.0998 < 1.1 and adds its own relative error eps_act (1 + |pre|):
v_exp_f32 and v_rcp_f32 are 1 ulp each, 1 + e is rounded once, and the scaling of the argument by log2(e) moves the exponent by
|pre| 2^-24 log2(e), a relative error |pre| ulps of the result; eps_act = 2^-20 = 16 ulps covers the four with a factor 4.  One bf16
RNE store adds at most half a bf16 ulp, 2^-8 |ref| (attained on ties, hence <=).  Nothing scales with max |ref|:
    tol = 2^-8 |ref| + 1.1 e_pre + eps_act (1 + |pre|) |ref|            (eps_act = 0 without SiLU)

BACKWARD TOLERANCE, per element (bwd_bounds, bwd_tol).  With the same (dmu, drho):
    e_x   = |xhat| d_rho + rho d_mu                                   error of xhat' = (x - mu') rho'
    e_d   = |dy gamma| (0.5 |gamma| e_x + 1.1 eps_act (1 + |pre|))    SiLU only: max |SiLU''| = 0.5, |SiLU'| <= 1.1; 0 without SiLU
    e_s1  = mean(e_d) + d_s1,   e_s2 = mean(e_d |xhat| + |d| e_x) + d_s2
    tol   = 2^-8 |ref + prev| + rho (e_d + e_s1 + |xhat| e_s2 + e_x |s2|) + d_rho |ref| + 2^-21 rho (|d| + |s1| + |xhat s2|)
d_s1 = max(4 floor_s1, 2^-22 mean |d|) and d_s2 = max(4 floor_s2, 2^-22 mean |d xhat|) are the fp32 floors of the two backward sums,
built like d_mu from the emulation (emu_bwd) with exact statistics; the propagated statistic error is the mean(...) part.  d_rho |ref|
is the leading factor rho'.  The last term is the fp32 evaluation of rho (d - s1 - xhat s2) (three roundings on partial results bounded
by the sum of magnitudes, as above).  With `accumulate` the previous gradient prev (bf16) is added in fp32 in front of the single
rounding, so the store term is 2^-8 |ref + prev|.
"""
from types import SimpleNamespace

import torch

F64 = torch.float64
EPS_ACT = 2.0 ** -20          # SiLU: v_exp_f32 + v_rcp_f32 + 1 + e + argument scaling, see the docstring (measured: below 2^-22)
GN_MAX_SPLIT = 256


def bf(t):
    """Round to bf16 (RNE) and return as float64."""
    return t.to(torch.bfloat16).to(F64)


def gn_split(HW, C):
    """Splits of the GroupNorm statistics pass (norm.hip gn_split): about 32K elements per split, at most 256."""
    rows = max(32768 // C, 4)
    return min(max((HW + rows - 1) // rows, 1), GN_MAX_SPLIT)


def silu64(p):
    return p * torch.sigmoid(p)


def dsilu64(p):
    s = torch.sigmoid(p)
    return s * (1 + p * (1 - s))


def _pg(v, cpg):
    """[B, G] per-group values -> [B, 1, C] per channel."""
    return v.repeat_interleave(cpg, dim=1)[:, None, :]


def _gmean(t, G):
    """mean over (rows, channels of the group) of [B, HW, C] -> [B, G]"""
    B, HW, C = t.shape
    return t.view(B, HW, G, C // G).mean((1, 3))


def reference(x, gamma, beta, G, eps, silu, dy=None):
    """float64 forward (and, with dy, the float64 autograd input gradient) from bf16-rounded inputs.  x, dy [B, HW, C]; gamma, beta [C]."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    B, HW, C = x.shape
    cpg = C // G
    xr = x.clone().requires_grad_(dy is not None)
    mu = _gmean(xr, G)
    var = _gmean((xr - _pg(mu, cpg)) ** 2, G)
    rho = (var + eps).rsqrt()
    xhat = (xr - _pg(mu, cpg)) * _pg(rho, cpg)
    pre = xhat * gamma + beta
    out = silu64(pre) if silu else pre
    R = SimpleNamespace(x=x, gamma=gamma, beta=beta, G=G, cpg=cpg, eps=eps, silu=silu, mu=mu.detach(), var=var.detach(), rho=rho.detach(),
                        sigma=var.detach().sqrt(), xhat=xhat.detach(), pre=pre.detach(), ref=out.detach())
    if dy is not None:
        dy = dy.to(F64)
        (R.dx,) = torch.autograd.grad(out, xr, dy)
        R.dy = dy
        R.d = dy * (dsilu64(R.pre) if silu else 1.0) * gamma
        R.s1 = _gmean(R.d, G)
        R.s2 = _gmean(R.d * R.xhat, G)
    return R


def layernorm_reference(x, gamma, beta, eps, dy=None):
    """LayerNorm over the channels of [M, C] rows: GroupNorm with one group per row."""
    return reference(x[:, None, :], gamma, beta, 1, eps, False, None if dy is None else dy[:, None, :])


# ---------------------------------------------------------------- fp32 emulation of the documented schemes

def emu_gn_stats(x, G, eps, drop_row=False):
    """One-pass (n, mean, M2 = sumsq - sum * mean) per split, Chan merge in split order; float32 throughout.  -> (mu, rho) [B, G].
    drop_row: the last row of the first split is left out (a perturbation for the tests of the bounds)."""
    x32 = x.to(torch.float32)
    B, HW, C = x32.shape
    cpg = C // G
    S = gn_split(HW, C)
    rows_per = (HW + S - 1) // S
    n = torch.zeros((), dtype=torch.float32)
    mean = torch.zeros(B, G, dtype=torch.float32)
    M2 = torch.zeros(B, G, dtype=torch.float32)
    for s in range(S):
        r0, r1 = s * rows_per, min(HW, (s + 1) * rows_per)
        if drop_row and s == 0:
            r1 -= 1
        if r1 <= r0:
            continue
        blk = x32[:, r0:r1].reshape(B, r1 - r0, G, cpg)
        t0, t1 = blk.sum((1, 3)), (blk * blk).sum((1, 3))
        nb = torch.tensor(float((r1 - r0) * cpg), dtype=torch.float32)
        m = t0 / nb
        M2b = (t1 - t0 * m).clamp_min(0)
        nn = n + nb
        d = m - mean
        mean = mean + d * (nb / nn)
        M2 = M2 + M2b + d * d * (n * nb / nn)
        n = nn
    return mean, torch.rsqrt(M2 / n + torch.tensor(eps, dtype=torch.float32))


def chan_partials(x):
    """float64 (mean, M2) of every (64-row block, channel) of [B, HW, C], as the convolution epilogues emit them: [B * HW / 64, C, 2]."""
    B, HW, C = x.shape
    blk = x.to(F64).view(B, HW // 64, 64, C)
    m = blk.mean(2)
    M2 = ((blk - m[:, :, None, :]) ** 2).sum(2)
    return torch.stack([m, M2], -1).view(B * (HW // 64), C, 2)


def emu_gn_stats_fused(part32, B, G, eps):
    """Merge of equal-count partials [B * nb, C, 2] (float32): mean = avg(mean_p), M2 = sum M2_p + 64 sum (mean_p - mean)^2."""
    nbB, C, _ = part32.shape
    nb, cpg = nbB // B, C // G
    pm = part32[..., 0].reshape(B, nb, G, cpg).to(torch.float32)
    pM = part32[..., 1].reshape(B, nb, G, cpg).to(torch.float32)
    P = torch.tensor(float(nb * cpg), dtype=torch.float32)
    mean = pm.sum((1, 3)) / P
    d = pm - mean[:, None, :, None]
    M2 = (pM + 64.0 * d * d).sum((1, 3))
    return mean, torch.rsqrt(M2.clamp_min(0) / (64.0 * P) + torch.tensor(eps, dtype=torch.float32))


def emu_ln_stats(x, eps, divisor=None):
    """Two-pass float32 statistics of [M, C] rows -> (mu, rho) [M, 1].  divisor: C - 1 for the perturbation test."""
    x32 = x.to(torch.float32)
    C = x32.shape[1]
    mean = x32.sum(1, keepdim=True) / C
    v = ((x32 - mean) ** 2).sum(1, keepdim=True) / (divisor or C)
    return mean, torch.rsqrt(v + torch.tensor(eps, dtype=torch.float32))


def emu_ln_stats_rowpart(part32, C, eps):
    """One-pass statistics from (sum, sum^2) row partials [M, spans, 2] (float32): var = q / C - mean^2."""
    a, q = part32[..., 0].to(torch.float32).sum(1, keepdim=True), part32[..., 1].to(torch.float32).sum(1, keepdim=True)
    mean = a / C
    var = (q / C - mean * mean).clamp_min(0)
    return mean, torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def emu_fwd(x, gamma, beta, mu, rho, G, silu, form="gn", gidx=None):
    """float32 x * a + b (GroupNorm) or (x - mu) rho gamma + beta (LayerNorm), SiLU, one bf16 rounding.  gidx: channel -> group map."""
    x32, ga, be = x.to(torch.float32), gamma.to(torch.float32), beta.to(torch.float32)
    C = x32.shape[2]
    if gidx is None:
        gidx = torch.arange(C) // (C // G)
    m, r = mu.to(torch.float32)[:, gidx][:, None, :], rho.to(torch.float32)[:, gidx][:, None, :]
    if form == "gn":
        a = r * ga
        y = x32 * a + (be - m * a)
    else:
        y = (x32 - m) * r * ga + be
    if silu:
        y = y / (1 + torch.exp(-y))
    return y.to(torch.bfloat16)


def emu_bwd(x, dy, gamma, beta, mu, rho, G, silu, prev=None, drop_s2=False):
    """float32 backward from given statistics -> (dx bf16, s1, s2)."""
    x32, dy32, ga, be = x.to(torch.float32), dy.to(torch.float32), gamma.to(torch.float32), beta.to(torch.float32)
    cpg = x32.shape[2] // G
    m, r = _pg(mu.to(torch.float32), cpg), _pg(rho.to(torch.float32), cpg)
    xh = (x32 - m) * r
    d = dy32
    if silu:
        p = xh * ga + be
        s = 1 / (1 + torch.exp(-p))
        d = d * (s * (1 + p * (1 - s)))
    d = d * ga
    s1, s2 = _gmean(d, G), _gmean(d * xh, G)
    out = r * (d - _pg(s1, cpg) - (0 if drop_s2 else xh * _pg(s2, cpg)))
    if prev is not None:
        out = out + prev.to(torch.float32)
    return out.to(torch.bfloat16), s1, s2


# ---------------------------------------------------------------- bounds

def stat_bounds(R, emu_mu, emu_rho):
    """-> SimpleNamespace(d_mu [B, G], d_rho, r, floor_mu, floor_rho, live [B, G]) from the emulation's error against float64."""
    live = R.sigma > 0
    r = float((R.mu.abs() / R.sigma)[live].max())
    floor_rho = float(((emu_rho.to(F64) - R.rho).abs() / R.rho)[live].max())
    floor_mu = float((emu_mu.to(F64) - R.mu).abs().max())
    d_rho = min(max(4 * floor_rho, 2.0 ** -20), 2.0 ** -18 * (1 + r * r))
    d_mu = torch.clamp_min(2.0 ** -22 * (R.mu.abs() + R.sigma), 4 * floor_mu)
    return SimpleNamespace(d_mu=d_mu, d_rho=d_rho, r=r, floor_mu=floor_mu, floor_rho=floor_rho, live=live)


def fwd_tol(R, sb):
    ga, cpg = R.gamma.abs(), R.cpg
    rho, mu = _pg(R.rho, cpg), _pg(R.mu, cpg)
    e_pre = ga * rho * (R.x - mu).abs() * sb.d_rho + ga * rho * _pg(sb.d_mu, cpg) + 2.0 ** -21 * (ga * rho * (R.x.abs() + mu.abs()) + R.beta.abs())
    tol = 2.0 ** -8 * R.ref.abs() + 1.1 * e_pre
    if R.silu:
        tol = tol + EPS_ACT * (1 + R.pre.abs()) * R.ref.abs()
    return tol


def bwd_bounds(R, emu_s1, emu_s2):
    """fp32 floors of the two backward sums, per group [B, G]."""
    f1 = float((emu_s1.to(F64) - R.s1).abs().max())
    f2 = float((emu_s2.to(F64) - R.s2).abs().max())
    d_s1 = torch.clamp_min(2.0 ** -22 * _gmean(R.d.abs(), R.G), 4 * f1)
    d_s2 = torch.clamp_min(2.0 ** -22 * _gmean((R.d * R.xhat).abs(), R.G), 4 * f2)
    return SimpleNamespace(d_s1=d_s1, d_s2=d_s2, floor_s1=f1, floor_s2=f2)


def bwd_tol(R, sb, bb, prev=None):
    cpg, G = R.cpg, R.G
    rho = _pg(R.rho, cpg)
    axh = R.xhat.abs()
    e_x = axh * sb.d_rho + rho * _pg(sb.d_mu, cpg)
    if R.silu:
        e_d = (R.dy * R.gamma).abs() * (0.5 * R.gamma.abs() * e_x + 1.1 * EPS_ACT * (1 + R.pre.abs()))
    else:
        e_d = torch.zeros_like(e_x)
    e_s1 = _pg(_gmean(e_d, G) + bb.d_s1, cpg)
    e_s2 = _pg(_gmean(e_d * axh + R.d.abs() * e_x, G) + bb.d_s2, cpg)
    s1, s2 = _pg(R.s1, cpg), _pg(R.s2, cpg)
    stored = R.dx if prev is None else R.dx + prev.to(F64)
    return (2.0 ** -8 * stored.abs() + rho * (e_d + e_s1 + axh * e_s2 + e_x * s2.abs()) + sb.d_rho * R.dx.abs()
            + 2.0 ** -21 * rho * (R.d.abs() + s1.abs() + (R.xhat * s2).abs()))


# ---------------------------------------------------------------- assertions (shared by the CPU and the GPU tests)

def assert_stats(mu, rho, R, sb, what=""):
    """The statistics buffer against float64: |mu' - mu| <= d_mu everywhere, |rho' / rho - 1| <= d_rho where sigma > 0.
    -> (worst mu error / d_mu, worst relative rho error)"""
    mu, rho = mu.detach().cpu().to(F64).reshape(R.mu.shape), rho.detach().cpu().to(F64).reshape(R.rho.shape)
    assert torch.isfinite(mu).all() and torch.isfinite(rho).all(), what + ": non-finite statistics"
    e = (mu - R.mu).abs()
    e = torch.where(e > 0, e / sb.d_mu, torch.zeros_like(e))               # d_mu == 0 only for an all-zero group with an exact emulation
    emu, i = e.max().item(), int(e.argmax())
    assert emu <= 1, "%s: mean of (image, group) %s off by %.3g, %.3g x d_mu" % (what, divmod(i, R.mu.shape[1]), (mu - R.mu).abs().flatten()[i].item(), emu)
    rel = ((rho - R.rho).abs() / R.rho)
    rel = torch.where(sb.live, rel, torch.zeros_like(rel))
    i = int(rel.argmax())
    assert rel.max().item() <= sb.d_rho, "%s: rstd of (image, group) %s off by %.3g relative, d_rho %.3g (r = %.3g, fp32 floor %.3g)" % (
        what, divmod(i, R.rho.shape[1]), rel.max().item(), sb.d_rho, sb.r, sb.floor_rho)
    return emu, rel.max().item()


def assert_elems(got, ref, tol, what=""):
    """Every element within its own tolerance; on failure the worst element's (image, row, channel), err / tol and the fraction over.
    -> worst err / tol"""
    got = got.detach().cpu().to(F64).reshape(ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / tol, torch.zeros_like(err))        # tol == 0 only where an exact zero is required
    worst = ratio.max().item()
    if not worst <= 1:
        i = int(ratio.argmax())
        b, rem = divmod(i, ref.shape[1] * ref.shape[2])
        row, c = divmod(rem, ref.shape[2])
        raise AssertionError("%s: (image %d, row %d, channel %d) got %.6g, reference %.6g, err / tol = %.3g; %.3g %% of the elements over tol"
                             % (what, b, row, c, got.flatten()[i].item(), ref.flatten()[i].item(), worst, 100.0 * (ratio > 1).double().mean().item()))
    return worst


# ---------------------------------------------------------------- the cases (inputs seeded on the CPU; shared by both test files)

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _affine(C, g):
    return torch.randn(C, generator=g, dtype=F64).float().to(F64), torch.randn(C, generator=g, dtype=F64).float().to(F64)   # fp32 values


# name: (C, G, HW, B, eps, silu, input kind)
GN_CASES = {
    "c320_hw64": (320, 32, 64, 2, 1e-5, True, "plain"),          # cpg 10: vectors straddle groups; 40 vector columns, 16 idle threads
    "c320_hw100": (320, 32, 100, 2, 1e-6, False, "plain"),
    "c960_hw72": (960, 32, 72, 2, 1e-5, True, "plain"),
    "c1920_hw64": (1920, 32, 64, 2, 1e-6, False, "plain"),
    "c2560_hw64": (2560, 32, 64, 2, 1e-5, True, "plain"),        # 320 vector columns: a second sweep with 64 threads
    "c8_g1_hw5": (8, 1, 5, 2, 1e-5, True, "plain"),              # one column, 256 row slots, fewer rows than slots
    "c32_cpg1_hw16": (32, 32, 16, 2, 1e-6, False, "plain"),
    "split4": (128, 32, 1024, 2, 1e-6, True, "plain"),
    "split17_ragged": (512, 32, 1030, 2, 1e-5, False, "plain"),
    "split256_cap": (512, 32, 16400, 1, 1e-5, True, "plain"),    # 257 splits wanted: 256 of 65 rows, the last ones ragged / empty
    "far50": (320, 32, 4096, 2, 1e-5, True, "far50"),
    "far8": (512, 32, 1024, 2, 1e-6, False, "far8"),
    "ramp4": (320, 32, 256, 2, 1e-5, True, "ramp"),
    "eps1e-5": (128, 32, 256, 2, 1e-5, True, "tiny"),
    "eps1e-6": (128, 32, 256, 2, 1e-6, True, "tiny"),
}
GRIDCAP = (640, 32, 4096, 32, 1e-5, True)                        # 160 apply blocks wanted, 4096 / 32 + 1 = 129 allowed
GRIDCAP_CHECKED = (0, 1, 15, 31)
# GroupNorm from channel partials: P = (HW / 64) * cpg partials per group; 12 per thread are held in registers (P <= 3072), the rest re-read
PART_CASES = {
    "P4": (128, 32, 64, 2, 1e-5, True, "plain"),
    "P3072_far50": (128, 32, 49152, 2, 1e-6, False, "far50"),
    "P3080": (1280, 32, 4928, 2, 1e-5, True, "plain"),
    "P4096": (128, 32, 65536, 1, 1e-6, True, "plain"),
}
LN_C = (8, 64, 320, 512, 520, 768, 1024, 1032, 1280, 1536, 1544, 2048)
# (C, M, input kind): every C sees M = 17, every M sees C = 320 and 1544, rows at mean 50 sigma for C = 320 and 2048
LN_CASES = [(c, 17, "plain") for c in LN_C] + [(c, m, "plain") for c in (320, 1544) for m in (1, 15, 77)] + [(320, 17, "far50"), (2048, 17, "far50")]
LN_EPS = 1e-5


def ln_id(case):
    return "C%d_M%d_%s" % case


def make_rows(kind, B, HW, C, G, g):
    """bf16-rounded [B, HW, C] float64 input of a case."""
    cpg = C // G
    z = torch.randn(B, HW, C, generator=g)
    if kind == "plain":
        x = z * 2 + 0.5
    elif kind in ("far50", "far8"):                     # groups at +- 50 (8) sigma, the sign alternating with image + group
        k = 50.0 if kind == "far50" else 8.0
        sign = ((torch.arange(B)[:, None] + torch.arange(G)[None, :]) % 2) * 2.0 - 1.0
        x = z + k * sign.repeat_interleave(cpg, dim=1)[:, None, :]
    elif kind == "ramp":                                # per-channel means on a smooth ramp inside each group, total spread 4 sigma
        ramp = (torch.arange(C) % cpg).float() / max(cpg - 1, 1) * 4.0 - 2.0
        x = z + ramp
    elif kind == "tiny":                                # variance about eps
        x = z * 3e-3
    else:
        raise ValueError(kind)
    return bf(x)


def gn_inputs(case, seed=11):
    """-> SimpleNamespace(x, dy, prev [B, HW, C] float64 bf16-valued, gamma, beta [C] float64 fp32-valued, C, G, HW, B, eps, silu)"""
    C, G, HW, B, eps, silu, kind = case
    g = _gen(seed + C + HW)
    x = make_rows(kind, B, HW, C, G, g)
    gamma, beta = _affine(C, g)
    dy = bf(torch.randn(B, HW, C, generator=g))
    prev = bf(torch.randn(B, HW, C, generator=g))
    return SimpleNamespace(x=x, dy=dy, prev=prev, gamma=gamma, beta=beta, C=C, G=G, HW=HW, B=B, eps=eps, silu=silu)


def degenerate_inputs():
    """(320, 32, 64): group 3 of image 0 all zero, group 7 of image 1 a non-zero constant; forward only."""
    I = gn_inputs((320, 32, 64, 2, 1e-5, True, "plain"), seed=23)
    I.x[0, :, 30:40] = 0.0
    I.x[1, :, 70:80] = 3.0
    return I


def gridcap_images(images, seed=31):
    """Images of the B = 32 case: 8 seeded base images, image b = bf16(base[b % 8] * scale_b + offset_b).  -> x, dy [len(images), HW, C] bf16"""
    C, G, HW, B, eps, silu = GRIDCAP
    g = _gen(seed)
    base = torch.randn(8, HW, C, generator=g)
    dbase = torch.randn(8, HW, C, generator=g)
    x = torch.stack([(base[b % 8] * (1.0 + 0.05 * b) + (0.3 * b - 4.0)).to(torch.bfloat16) for b in images])
    dy = torch.stack([(dbase[(b + 3) % 8] * (1.0 + 0.02 * b)).to(torch.bfloat16) for b in images])
    return x, dy, _affine(C, g)


def ln_inputs(case, seed=41):
    C, M, kind = case
    g = _gen(seed + C + M)
    z = torch.randn(M, C, generator=g)
    if kind == "far50":
        sign = (torch.arange(M) % 2) * 2.0 - 1.0
        x = bf(z + 50.0 * sign[:, None])
    else:
        x = bf(z * 1.5 + 0.3)
    gamma, beta = _affine(C, g)
    return SimpleNamespace(x=x, dy=bf(torch.randn(M, C, generator=g)), prev=bf(torch.randn(M, C, generator=g)), gamma=gamma, beta=beta, C=C, M=M)


def rowpart_inputs(spans, far, seed=53):
    """Row partials of M = 300 rows of C = 320 fp32 values (the producing GEMM sums in front of the bf16 rounding): float64 (sum, sum^2)
    per column span, rounded to fp32.  -> x [M, C] float64, part [M, spans, 2] float32"""
    M, C = 300, 320
    g = _gen(seed + spans)
    x = torch.randn(M, C, generator=g).to(F64) * 1.5 + (8.0 * 1.5 * ((torch.arange(M) % 2) * 2.0 - 1.0)[:, None] if far else 0.3)
    xs = x.view(M, spans, C // spans)
    return x, torch.stack([xs.sum(2), (xs * xs).sum(2)], -1).float()
