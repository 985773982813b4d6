"""The norm bounds of tests/norm_ref.py have teeth (CPU only, no kernel runs here).

For every case of tests/test_norm_gpu.py the fp32 emulation of the documented arithmetic, rounded to bf16 once, must PASS the statistic
and per-element assertions, and emulations perturbed the way a subtly wrong kernel would be must FAIL at least one of them: rstd x 1.004,
mean moved by 0.004 sigma, eps 1e-5 for 1e-6, one row missing from the statistics, the group index taken per 8-channel vector, LayerNorm
dividing by C - 1, the backward without its s2 term.  (The old bound atol + 1.5e-2 max|ref| sees the first of these at 0.33-0.41 of its limit.)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import norm_ref as nr


@functools.lru_cache(maxsize=2)
def _gn(name):
    """inputs, float64 reference, emulated statistics and the bounds of one GroupNorm case"""
    if name == "gridcap":
        C, G, HW, B, eps, silu = nr.GRIDCAP
        x, dy, (gamma, beta) = nr.gridcap_images(nr.GRIDCAP_CHECKED)
        I = nr.SimpleNamespace(x=x.to(nr.F64), dy=dy.to(nr.F64), prev=nr.bf(torch.randn(x.shape, generator=torch.Generator().manual_seed(3))),
                               gamma=gamma, beta=beta, C=C, G=G, HW=HW, B=len(nr.GRIDCAP_CHECKED), eps=eps, silu=silu)
    elif name in nr.PART_CASES:
        I = nr.gn_inputs(nr.PART_CASES[name])
    else:
        I = nr.gn_inputs(nr.GN_CASES[name])
    R = nr.reference(I.x, I.gamma, I.beta, I.G, I.eps, I.silu, I.dy)
    if name in nr.PART_CASES:
        mu, rho = nr.emu_gn_stats_fused(nr.chan_partials(I.x).float(), I.B, I.G, I.eps)
    else:
        mu, rho = nr.emu_gn_stats(I.x, I.G, I.eps)
    sb = nr.stat_bounds(R, mu, rho)
    _, s1, s2 = nr.emu_bwd(I.x, I.dy, I.gamma, I.beta, R.mu, R.rho, I.G, I.silu)
    bb = nr.bwd_bounds(R, s1, s2)
    return I, R, mu, rho, sb, bb


def _check_all(I, R, sb, bb, mu, rho, form="gn", gidx=None, drop_s2=False):
    """every assertion the GPU test makes, on an emulated result computed from the statistics (mu, rho); -> the worst ratios"""
    out = {}
    out["mu"], out["rho"] = nr.assert_stats(mu, rho, R, sb, "stats")
    out["fwd"] = nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu, rho, I.G, I.silu, form, gidx), R.ref, nr.fwd_tol(R, sb), "fwd")
    dx, _, _ = nr.emu_bwd(I.x, I.dy, I.gamma, I.beta, mu, rho, I.G, I.silu, drop_s2=drop_s2)
    out["bwd"] = nr.assert_elems(dx, R.dx, nr.bwd_tol(R, sb, bb), "bwd")
    dxa, _, _ = nr.emu_bwd(I.x, I.dy, I.gamma, I.beta, mu, rho, I.G, I.silu, prev=I.prev, drop_s2=drop_s2)
    out["acc"] = nr.assert_elems(dxa, R.dx + I.prev, nr.bwd_tol(R, sb, bb, I.prev), "bwd accumulate")
    return out


ALL_GN = list(nr.GN_CASES) + ["gridcap"] + list(nr.PART_CASES)


@pytest.mark.parametrize("name", ALL_GN)
def test_groupnorm_emulation_passes_and_perturbations_fail(name):
    I, R, mu, rho, sb, bb = _gn(name)
    assert sb.r <= 60, sb.r                                    # no case goes beyond 50 sigma (at 100 the one-pass form itself loses 1.4e-3)
    assert 4 * sb.floor_rho <= 2.0 ** -18 * (1 + sb.r ** 2)     # the upper clamp does not bind on the emulation
    got = _check_all(I, R, sb, bb, mu, rho)
    print("%s: r %.3g floor_rho %.3g floor_mu %.3g d_rho %.3g worst err/tol fwd %.3f bwd %.3f acc %.3f"
          % (name, sb.r, sb.floor_rho, sb.floor_mu, sb.d_rho, got["fwd"], got["bwd"], got["acc"]))
    sig = R.sigma.float()
    tol_f, tol_b = nr.fwd_tol(R, sb), nr.bwd_tol(R, sb, bb)
    # rstd x 1.004: the statistics assertion AND the forward element assertion each see it on their own
    with pytest.raises(AssertionError):
        nr.assert_stats(mu, rho * 1.004, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu, rho * 1.004, I.G, I.silu), R.ref, tol_f)
    # mean moved by 0.004 sigma
    with pytest.raises(AssertionError):
        nr.assert_stats(mu + 0.004 * sig, rho, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu + 0.004 * sig, rho, I.G, I.silu), R.ref, tol_f)
    # backward without the s2 term (right statistics)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_bwd(I.x, I.dy, I.gamma, I.beta, mu, rho, I.G, I.silu, drop_s2=True)[0], R.dx, tol_b)


def test_eps_1e5_for_1e6_fails():
    I, R, mu, rho, sb, bb = _gn("eps1e-6")
    mu5, rho5 = nr.emu_gn_stats(I.x, I.G, 1e-5)
    with pytest.raises(AssertionError):
        nr.assert_stats(mu5, rho5, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu5, rho5, I.G, I.silu), R.ref, nr.fwd_tol(R, sb))


def test_one_row_left_out_of_the_statistics_fails():
    I, R, mu, rho, sb, bb = _gn("c320_hw64")
    mu1, rho1 = nr.emu_gn_stats(I.x, I.G, I.eps, drop_row=True)
    with pytest.raises(AssertionError):
        nr.assert_stats(mu1, rho1, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu1, rho1, I.G, I.silu), R.ref, nr.fwd_tol(R, sb))


def test_group_index_per_vector_fails():
    """cpg = 10: a kernel that takes one group index per 8-channel vector reads its neighbour group's statistics in 2 channels of 10"""
    I, R, mu, rho, sb, bb = _gn("c320_hw64")
    gidx = (torch.arange(I.C) // 8 * 8) // (I.C // I.G)
    assert (gidx != torch.arange(I.C) // (I.C // I.G)).any()
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu, rho, I.G, I.silu, gidx=gidx), R.ref, nr.fwd_tol(R, sb))


def test_degenerate_groups_emulation_passes():
    I = nr.degenerate_inputs()
    R = nr.reference(I.x, I.gamma, I.beta, I.G, I.eps, I.silu)
    mu, rho = nr.emu_gn_stats(I.x, I.G, I.eps)
    sb = nr.stat_bounds(R, mu, rho)
    assert int((~sb.live).sum()) == 2
    nr.assert_stats(mu, rho, R, sb)
    nr.assert_elems(nr.emu_fwd(I.x, I.gamma, I.beta, mu, rho, I.G, I.silu), R.ref, nr.fwd_tol(R, sb))
    act_beta = nr.silu64(I.beta)
    assert torch.equal(R.ref[0, :, 30:40], act_beta[30:40].expand(I.HW, 10)) and torch.equal(R.ref[1, :, 70:80], act_beta[70:80].expand(I.HW, 10))


@pytest.mark.parametrize("case", nr.LN_CASES, ids=nr.ln_id)
def test_layernorm_emulation_passes_and_perturbations_fail(case):
    I = nr.ln_inputs(case)
    R = nr.layernorm_reference(I.x, I.gamma, I.beta, nr.LN_EPS, I.dy)
    mu, rho = nr.emu_ln_stats(I.x, nr.LN_EPS)
    sb = nr.stat_bounds(R, mu, rho)
    x3, I3 = I.x[:, None, :], nr.SimpleNamespace(x=I.x[:, None, :], dy=I.dy[:, None, :], prev=I.prev[:, None, :], gamma=I.gamma, beta=I.beta, G=1, silu=False)
    _, s1, s2 = nr.emu_bwd(x3, I3.dy, I.gamma, I.beta, R.mu, R.rho, 1, False)
    bb = nr.bwd_bounds(R, s1, s2)
    got = _check_all(I3, R, sb, bb, mu, rho, form="ln")
    print("%s: r %.3g floor_rho %.3g d_rho %.3g fwd %.3f bwd %.3f acc %.3f" % (nr.ln_id(case), sb.r, sb.floor_rho, sb.d_rho, got["fwd"], got["bwd"], got["acc"]))
    tol_f = nr.fwd_tol(R, sb)
    mu1, rho1 = nr.emu_ln_stats(I.x, nr.LN_EPS, divisor=I.C - 1)          # unbiased variance
    with pytest.raises(AssertionError):
        nr.assert_stats(mu1, rho1, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(x3, I.gamma, I.beta, mu1, rho1, 1, False, "ln"), R.ref, tol_f)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(x3, I.gamma, I.beta, mu, rho * 1.004, 1, False, "ln"), R.ref, tol_f)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_fwd(x3, I.gamma, I.beta, mu + 0.004 * R.sigma.float(), rho, 1, False, "ln"), R.ref, tol_f)
    with pytest.raises(AssertionError):
        nr.assert_elems(nr.emu_bwd(x3, I3.dy, I.gamma, I.beta, mu, rho, 1, False, drop_s2=True)[0], R.dx, nr.bwd_tol(R, sb, bb))


@pytest.mark.parametrize("spans,far", [(1, False), (4, False), (8, True), (16, False)])
def test_row_partial_emulation_passes(spans, far):
    x, part = nr.rowpart_inputs(spans, far)
    C = x.shape[1]
    R = nr.layernorm_reference(x, torch.ones(C), torch.zeros(C), nr.LN_EPS)
    mu, rho = nr.emu_ln_stats_rowpart(part, C, nr.LN_EPS)
    sb = nr.stat_bounds(R, mu, rho)
    assert (7 < sb.r < 10) if far else sb.r < 1
    nr.assert_stats(mu, rho, R, sb)
    with pytest.raises(AssertionError):
        nr.assert_stats(mu, rho * 1.004, R, sb)


def test_reference_equals_torch_float64():
    """norm_ref's float64 forward is F.group_norm / F.layer_norm in float64 to 1e-12, its analytic backward is autograd's"""
    I = nr.gn_inputs(nr.GN_CASES["c320_hw100"])
    R = nr.reference(I.x, I.gamma, I.beta, I.G, 1e-5, True, I.dy)
    nchw = I.x.permute(0, 2, 1).contiguous()
    want = F.silu(F.group_norm(nchw, I.G, I.gamma, I.beta, 1e-5)).permute(0, 2, 1)
    assert (R.ref - want).abs().max().item() <= 1e-12
    cpg = I.C // I.G
    dx = nr._pg(R.rho, cpg) * (R.d - nr._pg(R.s1, cpg) - R.xhat * nr._pg(R.s2, cpg))
    assert (dx - R.dx).abs().max().item() <= 1e-12
    L = nr.ln_inputs((520, 17, "plain"))
    RL = nr.layernorm_reference(L.x, L.gamma, L.beta, nr.LN_EPS)
    assert (RL.ref[:, 0] - F.layer_norm(L.x, (520,), L.gamma, L.beta, nr.LN_EPS)).abs().max().item() <= 1e-12
    assert (RL.mu[:, 0] - L.x.mean(1)).abs().max().item() <= 1e-12
    assert (RL.rho[:, 0] - (L.x.var(1, unbiased=False) + nr.LN_EPS).rsqrt()).abs().max().item() <= 1e-9 * RL.rho.max().item()
