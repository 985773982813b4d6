"""CPU checks of SDE-DPM-Solver++(2M) (sde_eta = s in (0, 1]): the library's host coefficients (dd_op_step_coefs_sde,
dd_op_step_coef_2m_sde: what dd_set_schedule_sde fills its tables with) against the float64 restatement of tests/dpm_sde_ref.py on the
real schedules, s = 0 against the deterministic tables bit for bit, s = 1 against the eta = 1 DDIM step, the identity the kernel rests on
(linear step on the SDE rows + c_sde (x0 - x0_prev) + sigma_n n == the update as diffusers / k-diffusion write it), the zero cases, the
order of convergence on a model with a known answer, the ABI surface and the CLI flag.  No GPU call.

Order of convergence, relative error of the standard deviation of z on the Gaussian model (float64, the library's coefficients):
    s = 1    first order 5.10e-2 (n = 20), 2.24e-2 (40), 1.06e-2 (80); second order 6.65e-3, 1.70e-3, 3.95e-4
    s = 0.5  first order 3.82e-2, 1.67e-2; second order 3.77e-3, 9.31e-4"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import ddim_eta_ref as E
import dpm_sde_ref as SD
import dpm_solver_ref as D
import sampler_variants_ref as R
import test_noise_rng as RNG
from test_dpm_solver import _schedule

PREDS = ["epsilon", "v_prediction", "sample"]
SCHEDULES = list(itertools.product(["leading", "trailing", "linspace"], [False, True], [10, 20, 50]))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    return _lib.lib()


def coefs_sde(L, pred, a, ap, s):
    out = (C.c_float * 5)(*([float("nan")] * 5))
    rc = L.dd_op_step_coefs_sde(R.PRED[pred], a, ap, s, out)
    return rc, [float(v) for v in out]


def coef_2m_sde(L, i, n, ab, a, ap, s):
    out = (C.c_float * 1)(float("nan"))
    rc = L.dd_op_step_coef_2m_sde(i, n, ab if ab is not None else 0.0, a, ap, s, out)
    return rc, float(out[0])


def bits(xs):
    return np.array(list(xs), np.float32).view(np.uint32)


@pytest.mark.parametrize("spacing,zero_snr,n", SCHEDULES)
def test_library_coefficients_match_the_restatement(L, spacing, zero_snr, n):
    """Formed in double, rounded to fp32 once (6e-8): relative error <= 1e-6 per coefficient wherever the restatement is not 0, exactly
    0 where it is -- the bound dd_op_step_coef_2m and dd_op_step_coefs_eta are held to."""
    _, ts, tr = _schedule(spacing, zero_snr, n)
    worst, worst_c, checked, nonzero = 0.0, 0.0, 0, 0
    for s in (0.3, 1.0):
        for i, (ab, a, ap) in enumerate(tr):
            rc, c = coef_2m_sde(L, i, n, ab, a, ap, s)
            ref = SD.coef_2m_sde_ref(i, n, ab if ab is not None else 0.0, a, ap, s)
            assert rc == 0 and math.isfinite(c)
            if ref == 0.0:
                assert c == 0.0, (s, ts[i], c)
            else:
                nonzero += 1
                worst_c = max(worst_c, abs(c - ref) / abs(ref))
            for pred in PREDS:
                rc, got = coefs_sde(L, pred, a, ap, s)
                if pred == "epsilon" and a == 0.0:                         # x0 is undefined there: the singular step of dd_op_step_coefs
                    assert rc == -1, (ts[i], rc)
                    continue
                assert rc == 0 and all(math.isfinite(v) for v in got), (pred, s, ts[i], rc, got)
                for g_, r_ in zip(got, SD.coefs_sde_ref(pred, a, ap, s)):
                    if r_ == 0.0:
                        assert g_ == 0.0, (pred, s, ts[i], got)
                    else:
                        worst = max(worst, abs(g_ - r_) / abs(r_))
                checked += 1
                assert 0.0 <= got[4] <= 1.0
    print("%s zero_snr=%s n=%d: %d rows, worst relative error %.2e; %d second-order c, worst %.2e" % (spacing, zero_snr, n, checked, worst, nonzero, worst_c))
    assert nonzero == 2 * (n - 2 - (1 if zero_snr and ts[0] == 999 else 0))
    assert checked >= 5 * n and worst <= 1e-6 and worst_c <= 1e-6


def test_s_zero_is_the_deterministic_table_bitwise(L):
    for spacing, zero_snr, n in SCHEDULES:
        _, ts, tr = _schedule(spacing, zero_snr, n)
        for i, (ab, a, ap) in enumerate(tr):
            rc, c = coef_2m_sde(L, i, n, ab, a, ap, 0.0)
            assert rc == 0 and np.array_equal(bits([c]), bits([L.dd_op_step_coef_2m(i, n, ab if ab is not None else 0.0, a, ap)]))
            for pred in PREDS:
                want = (C.c_float * 4)()
                rc4 = L.dd_op_step_coefs(R.PRED[pred], a, ap, want)
                rc, got = coefs_sde(L, pred, a, ap, 0.0)
                assert rc == rc4
                if rc == 0:
                    assert np.array_equal(bits(got[:4]), bits(want))
                    assert got[4] == 0.0 and not math.copysign(1.0, got[4]) < 0


def test_s_one_first_order_is_the_eta_one_ddim_step(L):
    """At s = 1 d = sigma' e^-h and sigma_n = sigma' sqrt(1 - e^-2h) are d and sigma of DDIMScheduler.step(eta = 1): the five floats agree
    within 1e-6 of the largest of them (both are double expressions rounded once; B_m cancels, hence relative to the largest)."""
    worst = 0.0
    for (spacing, zero_snr, n), pred in itertools.product(SCHEDULES, PREDS):
        _, ts, tr = _schedule(spacing, zero_snr, n)
        for _, a, ap in tr:
            rc, got = coefs_sde(L, pred, a, ap, 1.0)
            out = (C.c_float * 5)()
            rce = L.dd_op_step_coefs_eta(R.PRED[pred], a, ap, 1.0, out)
            assert rc == rce
            if rc == 0:
                big = max(abs(float(v)) for v in out)
                worst = max(worst, max(abs(g_ - float(e_)) for g_, e_ in zip(got, out)) / big)
    print("s = 1 against eta = 1: worst difference relative to the largest coefficient %.2e" % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("pred", PREDS)
def test_linear_form_is_the_diffusers_update(pred):
    """(A_z z + A_m m, [sqrt(a') x0 + d eps] + c_sde (x0 - x0_prev) + sigma_n n) on the issue's expressions == the diffusers /
    k-diffusion form, float64, within 1e-10."""
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for (spacing, n), s in itertools.product((("leading", 10), ("trailing", 20), ("linspace", 50)), (0.3, 0.5, 1.0)):
        _, ts, tr = _schedule(spacing, False, n)
        for i in range(1, n - 1):
            ab, a, ap = tr[i]
            z, m, xp, nz = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(4))
            sa, sb, sap, sbp = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(1 - ap)
            h = D.lam(ap) - D.lam(a)
            r = (D.lam(a) - D.lam(ab)) / h
            d, sg = sbp * math.exp(-s * h), sbp * math.sqrt(-math.expm1(-2 * s * h))
            c = sap * -math.expm1(-(1 + s) * h) / (2 * r)
            assert abs(d * d + sg * sg - (1 - ap)) <= 1e-14
            if pred == "epsilon":
                Az, Am, Bz, Bm = 1 / sa, -sb / sa, sap / sa, d - sap * sb / sa
            elif pred == "v_prediction":
                Az, Am, Bz, Bm = sa, -sb, sap * sa + d * sb, d * sa - sap * sb
            else:
                Az, Am, Bz, Bm = 0.0, 1.0, d / sb, sap - d * sa / sb
            x0 = Az * z + Am * m
            zp = Bz * z + Bm * m + c * (x0 - xp) + sg * nz
            rx0, rzp = SD.update_sde_ref(pred, ab, a, ap, s, z, m, xp, nz)
            worst = max(worst, float((x0 - rx0).abs().max() / rx0.abs().max()), float((zp - rzp).abs().max() / rzp.abs().max()))
            # without a history: the first-order SDE step
            z1 = Bz * z + Bm * m + sg * nz
            r1 = SD.update_sde_ref(pred, ab, a, ap, s, z, m, None, nz)[1]
            worst = max(worst, float((z1 - r1).abs().max() / r1.abs().max()))
    print("%s: worst relative difference of the two forms %.2e" % (pred, worst))
    assert worst <= 1e-10


def test_zero_cases(L):
    """a' = 1: d = sigma_n = c = 0; a' = a: d = sqrt(1-a'), sigma_n = 0.0f, the floats of dd_op_step_coefs; a = 0: d = 0, sigma_n =
    sqrt(1-a'), c = 0.  Finite everywhere, exact zeros, d^2 + sigma_n^2 = 1 - a' to 1e-6."""
    def d_of(got, a, ap):        # v-prediction: B_z = sqrt(a') sqrt(a) + d sqrt(1-a), B_m = d sqrt(a) - sqrt(a') sqrt(1-a)
        sa, sb, sap = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap)
        return (got[2] - sap * sa) * sb + (got[3] + sap * sb) * sa
    for s in (0.3, 0.5, 1.0):
        # a' = 1
        for pred in ("epsilon", "v_prediction"):
            rc, got = coefs_sde(L, pred, 0.5, 1.0, s)
            assert rc == 0 and got[4] == 0.0 and all(math.isfinite(v) for v in got)
        rc, got = coefs_sde(L, "v_prediction", 0.5, 1.0, s)
        assert abs(d_of(got, 0.5, 1.0)) <= 1e-6
        assert coef_2m_sde(L, 3, 10, 0.2, 0.5, 1.0, s) == (0, 0.0)
        # a' = a
        for pred in PREDS:
            rc, got = coefs_sde(L, pred, 0.3, 0.3, s)
            want = (C.c_float * 4)()
            assert rc == 0 and L.dd_op_step_coefs(R.PRED[pred], 0.3, 0.3, want) == 0
            assert np.array_equal(bits(got[:4]), bits(want)) and got[4] == 0.0 and not math.copysign(1.0, got[4]) < 0
        assert coef_2m_sde(L, 3, 10, 0.2, 0.3, 0.3, s) == (0, 0.0)
        # a = 0
        for ap in (0.3, 1e-4):
            rc, got = coefs_sde(L, "v_prediction", 0.0, ap, s)
            assert rc == 0 and all(math.isfinite(v) for v in got)
            assert abs(got[4] - math.sqrt(1 - ap)) <= 1e-6 and got[2] == 0.0 and abs(got[3] + math.sqrt(ap)) <= 1e-6
            rc, got = coefs_sde(L, "sample", 0.0, ap, s)
            assert rc == 0 and got[2] == 0.0 and abs(got[4] - math.sqrt(1 - ap)) <= 1e-6
            assert coefs_sde(L, "epsilon", 0.0, ap, s)[0] == -1
        assert coef_2m_sde(L, 3, 10, 0.2, 0.0, 0.3, s) == (0, 0.0) and coef_2m_sde(L, 1, 10, 0.0, 0.2, 0.3, s) == (0, 0.0)
        # c = 0 for the first and the last step, and where dd_op_step_coef_2m is 0
        for args in ((0, 10, 0.2, 0.4, 0.6), (9, 10, 0.2, 0.4, 0.6), (1, 2, 0.2, 0.4, 0.6), (3, 10, 0.4, 0.4, 0.6),
                     (3, 10, float("nan"), 0.4, 0.6), (3, 10, 0.2, 0.4, 1.5), (3, 10, -0.1, 0.4, 0.6)):
            assert coef_2m_sde(L, *args, s) == (0, 0.0), args
        assert coef_2m_sde(L, 3, 10, 0.2, 0.4, 0.6, s)[1] > L.dd_op_step_coef_2m(3, 10, 0.2, 0.4, 0.6) > 0.0
        # d^2 + sigma_n^2 = 1 - a' on regular and limit steps; never NaN or inf
        for pred in PREDS:
            for a, ap in ((0.0, 0.3), (0.0, 1e-4), (0.5, 1.0), (0.999, 1.0), (1e-6, 2e-6), (0.3, 0.3), (1.0, 1.0), (0.6, 0.4), (0.0, 0.0),
                          (0.2, 0.0), (0.2, 0.7), (1e-9, 0.999999)):
                rc, got = coefs_sde(L, pred, a, ap, s)
                assert rc in (0, -1)
                if rc == 0:
                    assert all(math.isfinite(v) for v in got), (pred, s, a, ap, got)
                    if pred == "v_prediction" and ap <= 1.0:
                        d = d_of(got, a, ap)
                        assert abs(d * d + got[4] * got[4] - (1 - ap)) <= 1e-6, (s, a, ap, d, got)
    # the real tables: the first trailing step of a zero-terminal-SNR table, and the t = 0 step of linspace (a' = a)
    _, ts, tr = _schedule("trailing", True, 10)
    assert tr[0][1] == 0.0
    rc, got = coefs_sde(L, "v_prediction", tr[0][1], tr[0][2], 1.0)
    assert rc == 0 and got[2] == 0.0 and abs(got[4] - math.sqrt(1 - tr[0][2])) <= 1e-6
    # refusals: s outside [0, 1] or not finite, an unknown type, no output
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert coefs_sde(L, "v_prediction", 0.5, 0.7, bad)[0] == -1
        rc, c = coef_2m_sde(L, 3, 10, 0.2, 0.4, 0.6, bad)
        assert rc == -1 and math.isnan(c)                                   # not written
    assert L.dd_op_step_coefs_sde(3, 0.5, 0.7, 0.5, (C.c_float * 5)()) == -1 and L.dd_op_step_coefs_sde(1, 0.5, 0.7, 0.5, None) == -1
    assert L.dd_op_step_coef_2m_sde(3, 10, 0.2, 0.4, 0.6, 0.5, None) == -1


def _gaussian_model_error(L, n, s, second_order):
    """The setup of tests/test_dpm_solver.py: data N(0, s2) per element, s2 = 0.25, exact denoiser x0 = sqrt(a) s2 / V(a) z with V(a) =
    a s2 + 1 - a; SD-1.x betas, leading, steps 0 .. n - n/5 - 1 as an epsilon model with the library's coefficients, float64.  The sampler
    is linear in (z, x0_prev) and the noise is independent of both, so their 2 x 2 covariance is propagated exactly -- no sampling:
        x0 = k z, m = (z - sqrt(a) x0) / sqrt(1-a) = q z,  z' = (B_z + B_m q + c k) z - c x0_prev + sigma_n n,  x0_prev' = k z.
    Starts from the exact marginal Var z = V(a_0); returns the relative error of std(z) against sqrt(V(a_end))."""
    s2 = 0.25
    V = lambda a: a * s2 + 1 - a
    _, ts, tr = _schedule("leading", False, n)
    last = n - n // 5 - 1
    P = np.array([[V(tr[0][1]), 0.0], [0.0, 0.0]])                           # covariance of (z, x0_prev)
    have_hist = False
    for i in range(last + 1):
        ab, a, ap = tr[i]
        rc, (Az, Am, Bz, Bm, sg) = coefs_sde(L, "epsilon", a, ap, s)
        assert rc == 0
        k = math.sqrt(a) * s2 / V(a)
        q = (1 - math.sqrt(a) * k) / math.sqrt(1 - a)
        c = coef_2m_sde(L, i, n, ab, a, ap, s)[1] if (second_order and have_hist) else 0.0
        M = np.array([[Bz + Bm * q + c * k, -c], [k, 0.0]])
        P = M @ P @ M.T + np.array([[sg * sg, 0.0], [0.0, 0.0]])
        have_hist = True
    exact = math.sqrt(V(tr[last][2]))
    return abs(math.sqrt(P[0, 0]) - exact) / exact


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_order_of_convergence_on_a_gaussian_model(L, s):
    """The three inequalities of tests/test_dpm_solver.py's order test, on the standard deviation of z (figures: module docstring)."""
    err = {(n, so): _gaussian_model_error(L, n, s, so) for n in (20, 40, 80) for so in (False, True)}
    print("s = %.1f  first order: n=20 %.3e, n=40 %.3e, n=80 %.3e   second order: %.3e, %.3e, %.3e   ratios 20/40: %.2f, %.2f"
          % (s, err[20, False], err[40, False], err[80, False], err[20, True], err[40, True], err[80, True],
             err[20, False] / err[40, False], err[20, True] / err[40, True]))
    assert err[40, True] < err[40, False] / 10
    assert err[20, True] / err[40, True] > 3
    assert err[20, False] / err[40, False] < 3


def test_abi_surface():
    from distdiff_amd import _lib, engine
    assert _lib.ABI_VERSION == 11
    for name in ("dd_set_schedule_sde", "dd_denoise_step_hn", "dd_direct_guidance_hn"):
        assert name in _lib.ENGINE_SYMBOLS
    for name in ("dd_op_step_coefs_sde", "dd_op_step_coef_2m_sde", "dd_op_sampler_step_2m_n"):
        assert name in _lib.OPS_SYMBOLS
    assert "sde_eta" not in [f[0] for f in engine.DDSamplerParams._fields_]      # an argument of dd_set_schedule_sde, not a struct field
    assert engine.SOLVERS == {"ddim": 0, "dpmsolver++": 1}


def test_cli_sde_eta_flag(tmp_path):
    from distdiff_amd import generate_data as G
    assert G.parse_args([]).sde_eta == 0.0
    a = G.parse_args(["--sde_eta", "0.5", "--sampler", "dpmsolver++"])
    assert a.sde_eta == 0.5 and a.sampler == "dpmsolver++" and a.eta == 0.0
    assert G.parse_args(["--sde_eta", "1", "--sampler", "dpmsolver++"]).sde_eta == 1.0
    assert G.parse_args(["--sde_eta", "0"]).sampler == "ddim"
    dp = ["--sampler", "dpmsolver++"]
    for bad in (["--sde_eta", "0.5"], ["--sde_eta", "0.5", "--sampler", "ddim"], ["--sde_eta", "0.5", "--eta", "0.5"],
                ["--sde_eta", "0.5", "--eta", "0.5"] + dp, ["--sde_eta", "1.5"] + dp, ["--sde_eta", "-0.1"] + dp, ["--sde_eta", "nan"] + dp,
                ["--eta", "0.5"] + dp):
        with pytest.raises(SystemExit):
            G.parse_args(bad)
    # --sde_eta 0: the call sequence of today, argument for argument (no keyword reaches the engine in stream mode)
    one = ["--total_split", "1", "--split", "0"] + dp
    base, calls0 = RNG._run(tmp_path, "a", one, EB=2)
    same, calls1 = RNG._run(tmp_path, "b", one + ["--sde_eta", "0"], EB=2)
    assert base == same and len(calls0) == len(calls1) == 7
    for c0, c1 in zip(calls0, calls1):
        assert c1["kw"] == {} and torch.equal(c0["noise"], c1["noise"]) and c0["si"] == c1["si"] and c0["gt"] == c1["gt"]
    # --sde_eta > 0, stream: the host's noise is still drawn and handed over; seed and unit ids key the step noise alone
    handed, calls = RNG._run(tmp_path, "c", one + ["--sde_eta", "0.5"], EB=2)
    assert sorted(u for _, u in handed.values()) == sorted(G.unit_id(i, j) for i in range(7) for j in range(2))
    for c0, c in zip(calls0, calls):
        assert torch.equal(c0["noise"], c["noise"]) and c["kw"]["seed"] == 1234 and c["kw"]["generate_inputs"] is False
        assert set(c["kw"]) == {"seed", "unit_ids", "generate_inputs"}
    # --sde_eta > 0, philox: the keywords of --noise_rng philox, nothing else
    _, callsp = RNG._run(tmp_path, "d", one + ["--sde_eta", "0.5", "--noise_rng", "philox"], EB=2)
    assert all(c["noise"] is None and set(c["kw"]) == {"seed", "unit_ids", "offset_noise"} for c in callsp)


def test_make_stochastic_at_s_one_is_the_eta_one_step():
    """The loop reference's per-step transform, first order, against tests/ddim_eta_ref.py's at eta = 1: float64, 1e-12."""
    g = torch.Generator().manual_seed(9)
    _, ts, tr = _schedule("leading", False, 10)
    for i, (ab, a, ap) in enumerate(tr):
        z0, x0, nz = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(3))
        got = SD.make_stochastic(z0, x0, None, i, 10, ab, a, ap, 1.0, nz)
        want = E.make_stochastic(z0, x0, a, ap, 1.0, nz)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
