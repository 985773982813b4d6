"""GroupNorm(+SiLU) / LayerNorm kernels (norm.hip) against the float64 reference of tests/norm_ref.py: the statistics buffer within
(d_mu, d_rho) of float64, every output element within its own tolerance -- both derived from the arithmetic and the fp32 floor of the
documented statistic scheme on the case's own input (norm_ref's docstring), nothing scaled by max|ref|.  Every case runs forward, backward
and backward with `accumulate`.  tests/test_norm_bounds.py shows on the CPU that these assertions fail for a 0.4 % error in rstd and six
other perturbations.  Each case prints one `NORMFIG` line with its measured figures (pytest -s).
"""
import pytest
import torch

import norm_ref as nr

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B          # bit pattern of the bytes around a strided view (a finite bf16, 1.5e16)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distdiff_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _fig(name, **kw):
    print("NORMFIG %s %s" % (name, " ".join("%s=%.3g" % kv for kv in kw.items())))


def _dev(t):
    """[.., C] float64 holding bf16 values -> [rows, C] bf16 on the device"""
    return t.reshape(-1, t.shape[-1]).to(torch.bfloat16).cuda()


def _view(t, ld_extra, off):
    """t [rows, C] bf16 (device) as a column view at column `off` of a sentinel-filled buffer with ld = C + ld_extra; -> (view, buffer)"""
    rows, C = t.shape
    buf = torch.full((rows, C + ld_extra), SENTINEL, dtype=torch.int16, device=t.device).view(torch.bfloat16)
    v = buf[:, off:off + C]
    v.copy_(t)
    return v, buf


def _outside_unchanged(buf, C, off, what, inside_too=None):
    """every byte of `buf` outside the view is still the sentinel (and, for an input, the view still holds `inside_too`)"""
    b = buf.view(torch.int16)
    assert bool((b[:, :off] == SENTINEL).all()) and bool((b[:, off + C:] == SENTINEL).all()), what + ": bytes outside the view were written"
    if inside_too is not None:
        assert torch.equal(buf[:, off:off + C].view(torch.int16), inside_too.view(torch.int16)), what + ": an input was modified"


def _run_gn(ops, name, I, chan_part=False, strided=False, backward=True):
    """forward / backward / backward-accumulate of one GroupNorm case against float64; -> the figures"""
    B, HW, C, G = I.B, I.HW, I.C, I.G
    R = nr.reference(I.x, I.gamma, I.beta, G, I.eps, I.silu, I.dy if backward else None)
    if chan_part:
        part = nr.chan_partials(I.x).float()                                     # float64 partials, rounded to fp32
        emu_mu, emu_rho = nr.emu_gn_stats_fused(part, B, G, I.eps)
    else:
        emu_mu, emu_rho = nr.emu_gn_stats(I.x, G, I.eps)
    sb = nr.stat_bounds(R, emu_mu, emu_rho)
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    xd, dyd, pvd = _dev(I.x), _dev(I.dy), _dev(I.prev)
    kw, yv, dxv, bufs = {}, None, None, None
    if strided:           # four buffers, four row strides, four column offsets (multiples of 8)
        (xv, xb), (dyv, dyb) = _view(xd, 24, 8), _view(dyd, 40, 16)
        (yv, yb), (dxv, dxb) = _view(torch.zeros_like(xd), 8, 0), _view(pvd, 56, 32)
        bufs = (xb, dyb, yb, dxb)
        xin, dyin = xv, dyv
        kw["y"] = yv
    else:
        xin, dyin = xd, dyd
    if chan_part:
        pbuf = torch.full((part.shape[0], C + 16, 2), float("nan"), device="cuda")   # the partials as a column view, part_ld = C + 16 > C
        pbuf[:, 8:8 + C] = part.cuda()
        kw["chan_part"] = pbuf[:, 8:8 + C]
    y, stats = ops.groupnorm(xin, ga, be, B, HW, G, I.eps, I.silu, **kw)
    torch.cuda.synchronize()
    fig = {"r": sb.r, "floor_rho": sb.floor_rho, "floor_mu": sb.floor_mu, "d_rho": sb.d_rho}
    fig["mu_err/d_mu"], fig["rho_err"] = nr.assert_stats(stats[..., 0], stats[..., 1], R, sb, name + " statistics")
    fig["fwd"] = nr.assert_elems(y.contiguous().view(B, HW, C), R.ref, nr.fwd_tol(R, sb), name + " forward")
    if backward:
        bb = nr.bwd_bounds(R, *nr.emu_bwd(I.x, I.dy, I.gamma, I.beta, R.mu, R.rho, G, I.silu)[1:])
        if strided:
            acc = dxv
        else:
            dx = ops.groupnorm(xin, ga, be, B, HW, G, I.eps, I.silu, dy=dyin, stats=stats)
            fig["bwd"] = nr.assert_elems(dx.view(B, HW, C), R.dx, nr.bwd_tol(R, sb, bb), name + " backward")
            acc = pvd.clone()
        out = ops.groupnorm(xin, ga, be, B, HW, G, I.eps, I.silu, dy=dyin, stats=stats, accumulate_into=acc)
        assert out.data_ptr() == acc.data_ptr()
        fig["acc"] = nr.assert_elems(acc.contiguous().view(B, HW, C), R.dx + I.prev, nr.bwd_tol(R, sb, bb, I.prev), name + " backward accumulate")
        if strided:       # the plain backward into the same strided dx
            ops.groupnorm(xin, ga, be, B, HW, G, I.eps, I.silu, dy=dyin, stats=stats, dx=dxv)
            fig["bwd"] = nr.assert_elems(dxv.contiguous().view(B, HW, C), R.dx, nr.bwd_tol(R, sb, bb), name + " backward")
    if strided:
        torch.cuda.synchronize()
        _outside_unchanged(bufs[0], C, 8, name + " x", xd)
        _outside_unchanged(bufs[1], C, 16, name + " dy", dyd)
        _outside_unchanged(bufs[2], C, 0, name + " y")
        _outside_unchanged(bufs[3], C, 32, name + " dx")
    _fig(name, **fig)
    return fig


@pytest.mark.parametrize("name", list(nr.GN_CASES))
def test_groupnorm_case(ops, name):
    _run_gn(ops, name, nr.gn_inputs(nr.GN_CASES[name]))


def test_groupnorm_degenerate_groups(ops):
    """An all-zero group and a constant group: the forward result is act(beta) within tol and finite (no backward claim at zero variance);
    rstd is asserted for the other groups only, the mean for all."""
    I = nr.degenerate_inputs()
    fig = _run_gn(ops, "degenerate", I, backward=False)
    assert fig["fwd"] <= 1


def test_groupnorm_strided_views(ops):
    """x, y, dy, dx are column views at different column offsets of four buffers with four different row strides; every byte outside
    the views keeps its sentinel."""
    _run_gn(ops, "strided", nr.gn_inputs(nr.GN_CASES["c320_hw100"], seed=17), strided=True)


@pytest.mark.parametrize("name", list(nr.PART_CASES))
def test_groupnorm_from_channel_partials(ops, name):
    """gn_finalize_chan_kernel alone: the partials are computed in float64 from x here and rounded to fp32; bounds from the fused-form emulation"""
    _run_gn(ops, name, nr.gn_inputs(nr.PART_CASES[name]), chan_part=True)


def test_silu_activation_alone_on_a_grid(ops):
    """eps_act measured: SiLU on a 1-D grid of 32768 pre-activations in about [-12, 12], separated from the statistics.  The kernel's affine
    is rebuilt from ITS OWN statistics buffer (a = fl(rho' gamma), b = fl(beta - fl(mu' a)), pre = x a + b in float64), so what remains
    between the output and RNE_bf16(SiLU_64(pre)) is the fp32 evaluation of x a + b (at most 2^-22 (|x a| + |b|), through a slope <= 1.1)
    and the activation's own error.  An output that is NOT the correctly rounded value shows that the computed value was on the other side
    of a bf16 rounding boundary: the exact value's distance to that boundary is a lower bound of the error there, and it must be within
    eps_act (1 + |pre|) |ref| + the affine term -- for every such element.  Prints the largest such distance as a multiple of
    (1 + |pre|) |ref| (the measured eps_act: a lower estimate, 0 when every output is correctly rounded; with 32768 points, each within half a bf16 ulp =
    2^-9 .. 2^-8 relative of a boundary, an error of 2^-22 relative leaves about 5 outputs on the wrong side)."""
    HW, C = 4096, 8
    x = nr.bf(torch.linspace(-10.0, 10.0, HW * C, dtype=nr.F64)[torch.randperm(HW * C, generator=torch.Generator().manual_seed(71))].view(1, HW, C))
    gamma = (4.0 + 0.37 * torch.arange(C, dtype=nr.F64)).float().to(nr.F64)       # eight affines: eight times the distinct pre-activations
    beta = (0.11 * torch.arange(C, dtype=nr.F64) - 0.4).float().to(nr.F64)
    y, stats = ops.groupnorm(_dev(x), gamma.float().cuda(), beta.float().cuda(), 1, HW, 1, 1e-5, True)
    mu, rho = stats[0, 0, 0].cpu().float(), stats[0, 0, 1].cpu().float()
    a = rho * gamma.float()
    b = beta.float() - mu * a
    pre = x * a.to(nr.F64) + b.to(nr.F64)
    ref, got = nr.silu64(pre), y.cpu().to(nr.F64).view(1, HW, C)
    want = nr.bf(ref)
    wrong = got != want
    assert bool(((got - want).abs() <= 2.0 ** -7 * ref.abs())[wrong].all()), "an output is more than one bf16 ulp from the correctly rounded value"
    dist = (ref - (got + want) / 2).abs()[wrong]                     # exact value to the rounding boundary between the two candidates
    scale = ((1 + pre.abs()) * ref.abs())[wrong]
    bound = nr.EPS_ACT * scale + 1.1 * 2.0 ** -22 * ((x * a.to(nr.F64)).abs() + b.to(nr.F64).abs())[wrong]
    measured = float((dist / scale).max()) if bool(wrong.any()) else 0.0
    print("NORMFIG silu_grid wrong=%d of=%d measured_eps_act=%.3g eps_act=%.3g pre_max=%.3g" % (int(wrong.sum()), HW * C, measured, nr.EPS_ACT, float(pre.abs().max())))
    assert bool((dist <= bound).all()), "activation error above eps_act: %.3g x (1 + |pre|) |ref|" % measured


# ---------------------------------------------------------------- apply-grid cap, B = 32

@pytest.fixture(scope="module")
def gridcap(ops):
    """One forward + backward + backward-accumulate run of (640, 32, 4096) at B = 32, shared by the two tests below (read-only)."""
    C, G, HW, B, eps, silu = nr.GRIDCAP
    x, dy, (gamma, beta) = nr.gridcap_images(range(B))
    ga, be = gamma.float().cuda(), beta.float().cuda()
    xd, dyd = x.view(B * HW, C).cuda(), dy.view(B * HW, C).cuda()
    y, stats = ops.groupnorm(xd, ga, be, B, HW, G, eps, silu)
    dx = ops.groupnorm(xd, ga, be, B, HW, G, eps, silu, dy=dyd, stats=stats)
    acc = dyd.view(B, HW, C).roll(1, 0).reshape(B * HW, C).contiguous()        # the previous gradient of image b is dy of image b - 1
    ops.groupnorm(xd, ga, be, B, HW, G, eps, silu, dy=dyd, stats=stats, accumulate_into=acc)
    torch.cuda.synchronize()
    return nr.SimpleNamespace(x=x, dy=dy, gamma=gamma, beta=beta, ga=ga, be=be, y=y.view(B, HW, C), stats=stats, dx=dx.view(B, HW, C), acc=acc.view(B, HW, C))


def test_groupnorm_apply_grid_cap(ops, gridcap):
    """B = 32 at 64x64: 160 apply blocks per image wanted, 4096 / 32 + 1 = 129 allowed, so every block walks a second round of rows.
    All 32 images finite; images 0, 1, 15, 31 against float64."""
    C, G, HW, B, eps, silu = nr.GRIDCAP
    Z = gridcap
    for t in (Z.y, Z.dx, Z.acc, Z.stats):
        assert bool(torch.isfinite(t).all())
    ids = list(nr.GRIDCAP_CHECKED)
    prev = torch.stack([Z.dy[(b - 1) % B] for b in ids]).to(nr.F64)
    R = nr.reference(Z.x[ids].to(nr.F64), Z.gamma, Z.beta, G, eps, silu, Z.dy[ids].to(nr.F64))
    sb = nr.stat_bounds(R, *nr.emu_gn_stats(R.x, G, eps))
    bb = nr.bwd_bounds(R, *nr.emu_bwd(R.x, R.dy, Z.gamma, Z.beta, R.mu, R.rho, G, silu)[1:])
    fig = {"r": sb.r, "floor_rho": sb.floor_rho, "floor_mu": sb.floor_mu, "d_rho": sb.d_rho}
    fig["mu_err/d_mu"], fig["rho_err"] = nr.assert_stats(Z.stats[ids][..., 0], Z.stats[ids][..., 1], R, sb, "gridcap statistics")
    fig["fwd"] = nr.assert_elems(Z.y[ids], R.ref, nr.fwd_tol(R, sb), "gridcap forward")
    fig["bwd"] = nr.assert_elems(Z.dx[ids], R.dx, nr.bwd_tol(R, sb, bb), "gridcap backward")
    fig["acc"] = nr.assert_elems(Z.acc[ids], R.dx + prev, nr.bwd_tol(R, sb, bb, prev), "gridcap backward accumulate")
    _fig("gridcap", **fig)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what + ": %d elements differ" % int((_bits(a) != _bits(b)).sum())


def test_groupnorm_image_alone_has_the_bits_it_has_in_the_batch_of_32(ops, gridcap):
    """The apply grid is capped by B (4096 / B + 1 blocks), the statistics splits are not a function of B: image 31 run alone (uncapped
    grid) must give the bits it gives inside the batch of 32 (a PNG does not depend on the engine batch)."""
    C, G, HW, B, eps, silu = nr.GRIDCAP
    Z = gridcap
    xd, dyd = Z.x[31].cuda(), Z.dy[31].cuda()
    y, stats = ops.groupnorm(xd, Z.ga, Z.be, 1, HW, G, eps, silu)
    dx = ops.groupnorm(xd, Z.ga, Z.be, 1, HW, G, eps, silu, dy=dyd, stats=stats)
    _same_bits(stats[0], Z.stats[31], "statistics of image 31")
    _same_bits(y, Z.y[31], "forward of image 31")
    _same_bits(dx, Z.dx[31], "backward of image 31")


def test_groupnorm_deterministic_and_batch_invariant(ops):
    """(320, 32, 4096), B = 4: the same call twice gives the same bits (no float atomics anywhere), and every image run alone gives the
    bits it gives inside the batch."""
    I = nr.gn_inputs((320, 32, 4096, 4, 1e-5, True, "plain"), seed=61)
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    xd, dyd = _dev(I.x), _dev(I.dy)

    def run(x, dy, B):
        y, st = ops.groupnorm(x, ga, be, B, I.HW, I.G, I.eps, I.silu)
        return y, st, ops.groupnorm(x, ga, be, B, I.HW, I.G, I.eps, I.silu, dy=dy, stats=st)
    first, second = run(xd, dyd, I.B), run(xd, dyd, I.B)
    for a, b, what in zip(first, second, ("forward", "statistics", "backward")):
        _same_bits(a, b, what + ", second run")
    for b in range(I.B):
        rows = slice(b * I.HW, (b + 1) * I.HW)
        y1, st1, dx1 = run(xd[rows], dyd[rows], 1)
        _same_bits(y1, first[0][rows], "forward of image %d alone" % b)
        _same_bits(st1[0], first[1][b], "statistics of image %d alone" % b)
        _same_bits(dx1, first[2][rows], "backward of image %d alone" % b)


# ---------------------------------------------------------------- LayerNorm

@pytest.mark.parametrize("case", nr.LN_CASES, ids=nr.ln_id)
def test_layernorm_case(ops, case):
    """Forward (1-4 vectors per lane on the multi-row kernel; row tails M % 16), statistics-only forward bit-identical, backward, backward
    accumulating into a strided dx."""
    I = nr.ln_inputs(case)
    M, C, name = I.M, I.C, "ln " + nr.ln_id(case)
    R = nr.layernorm_reference(I.x, I.gamma, I.beta, nr.LN_EPS, I.dy)
    sb = nr.stat_bounds(R, *nr.emu_ln_stats(I.x, nr.LN_EPS))
    x3, dy3, pv3 = I.x[:, None, :], I.dy[:, None, :], I.prev[:, None, :]
    bb = nr.bwd_bounds(R, *nr.emu_bwd(x3, dy3, I.gamma, I.beta, R.mu, R.rho, 1, False)[1:])
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    xd, dyd, pvd = _dev(I.x), _dev(I.dy), _dev(I.prev)
    y, stats = ops.layernorm(xd, ga, be, nr.LN_EPS)
    fig = {"r": sb.r, "floor_rho": sb.floor_rho, "floor_mu": sb.floor_mu, "d_rho": sb.d_rho}
    fig["mu_err/d_mu"], fig["rho_err"] = nr.assert_stats(stats[:, 0], stats[:, 1], R, sb, name + " statistics")
    fig["fwd"] = nr.assert_elems(y, R.ref, nr.fwd_tol(R, sb), name + " forward")
    _same_bits(ops.layernorm_stats(xd, nr.LN_EPS), stats, name + " statistics-only forward")
    dx = ops.layernorm(xd, ga, be, nr.LN_EPS, dy=dyd, stats=stats)
    fig["bwd"] = nr.assert_elems(dx, R.dx, nr.bwd_tol(R, sb, bb), name + " backward")
    acc, buf = _view(pvd, 24, 16)
    ops.layernorm(xd, ga, be, nr.LN_EPS, dy=dyd, stats=stats, accumulate_into=acc)
    fig["acc"] = nr.assert_elems(acc.contiguous(), R.dx + pv3, nr.bwd_tol(R, sb, bb, pv3), name + " backward accumulate")
    _outside_unchanged(buf, C, 16, name + " dx")
    _fig(name.replace(" ", "_"), **fig)


def test_layernorm_strided_views(ops):
    """x, y, dy, dx as column views of four buffers with four row strides; the bits of the contiguous call, nothing written outside."""
    I = nr.ln_inputs((520, 17, "plain"), seed=43)
    ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
    xd, dyd = _dev(I.x), _dev(I.dy)
    y0, st0 = ops.layernorm(xd, ga, be, nr.LN_EPS)
    dx0 = ops.layernorm(xd, ga, be, nr.LN_EPS, dy=dyd, stats=st0)
    (xv, xb), (dyv, dyb) = _view(xd, 24, 8), _view(dyd, 40, 16)
    (yv, yb), (dxv, dxb) = _view(torch.zeros_like(xd), 8, 0), _view(torch.zeros_like(xd), 56, 32)
    _, st = ops.layernorm(xv, ga, be, nr.LN_EPS, y=yv)
    ops.layernorm(xv, ga, be, nr.LN_EPS, dy=dyv, stats=st, dx=dxv)
    torch.cuda.synchronize()
    _same_bits(st, st0, "statistics")
    _same_bits(yv, y0, "forward")
    _same_bits(dxv, dx0, "backward")
    _outside_unchanged(xb, 520, 8, "x", xd)
    _outside_unchanged(dyb, 520, 16, "dy", dyd)
    _outside_unchanged(yb, 520, 0, "y")
    _outside_unchanged(dxb, 520, 32, "dx")


@pytest.mark.parametrize("spans,far", [(1, False), (4, False), (8, True), (16, False)])
def test_layernorm_row_partial_finalize(ops, spans, far):
    """ln_rowpart_finalize_kernel alone: synthetic (sum, sum^2) partials from float64, rowpart_ld = spans + 3 with NaN beside them, M = 300
    (two blocks, a ragged last one); one case with rows at mean 8 sigma."""
    x, part = nr.rowpart_inputs(spans, far)
    M, C = x.shape
    R = nr.layernorm_reference(x, torch.ones(C), torch.zeros(C), nr.LN_EPS)
    sb = nr.stat_bounds(R, *nr.emu_ln_stats_rowpart(part, C, nr.LN_EPS))
    buf = torch.full((M, spans + 3, 2), float("nan"), device="cuda")
    buf[:, :spans] = part.cuda()
    stats = ops.layernorm_stats(_dev(x), nr.LN_EPS, rowpart=buf[:, :spans], spans=spans)
    e_mu, e_rho = nr.assert_stats(stats[:, 0], stats[:, 1], R, sb, "row partials, %d spans" % spans)
    _fig("rowpart_spans%d%s" % (spans, "_far8" if far else ""), r=sb.r, floor_rho=sb.floor_rho, floor_mu=sb.floor_mu, d_rho=sb.d_rho, **{"mu_err/d_mu": e_mu, "rho_err": e_rho})


def test_layernorm_deterministic_and_row_invariant(ops):
    """The same call twice gives the same bits; a row run alone gives the bits it gives inside its block of rows (forward at 1 and at 4
    vectors per lane, backward)."""
    for C in (320, 1544):
        I = nr.ln_inputs((C, 77, "plain"), seed=47)
        ga, be = I.gamma.float().cuda(), I.beta.float().cuda()
        xd, dyd = _dev(I.x), _dev(I.dy)

        def run(x, dy):
            y, st = ops.layernorm(x, ga, be, nr.LN_EPS)
            return y, st, ops.layernorm(x, ga, be, nr.LN_EPS, dy=dy, stats=st)
        first, second = run(xd, dyd), run(xd, dyd)
        for a, b, what in zip(first, second, ("forward", "statistics", "backward")):
            _same_bits(a, b, "C %d %s, second run" % (C, what))
        for row in (0, 6, 76):
            alone = run(xd[row:row + 1], dyd[row:row + 1])
            for a, b, what in zip(alone, first, ("forward", "statistics", "backward")):
                _same_bits(a, b[row:row + 1], "C %d %s of row %d alone" % (C, what, row))
