"""CPU checks of stochastic DDIM (eta > 0): the library's host coefficients (dd_op_step_coefs_eta, what dd_set_schedule_e fills its eta
tables with) against the float64 restatement of tests/ddim_eta_ref.py on the real schedules, their eta = 0 and singular cases, the
identity the kernel rests on (the linear step with d in place of sqrt(1 - a'), plus sigma n == the update as diffusers writes it), the
DDPM posterior mean at eta = 1, the independence of the per-step noise streams, and the CLI flag.  No GPU call."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import ddim_eta_ref as E
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


def coefs_eta(L, pred, a, ap, eta):
    out = (C.c_float * 5)(*([float("nan")] * 5))
    rc = L.dd_op_step_coefs_eta(R.PRED[pred], a, ap, eta, out)
    return rc, [float(v) for v in out]


@pytest.mark.parametrize("spacing,zero_snr,n", SCHEDULES)
def test_library_coefficients_match_the_restatement(L, spacing, zero_snr, n):
    """Formed in double, rounded to fp32 once (6e-8): relative error <= 1e-6 per coefficient, the bound dd_op_step_coef_2m is held to."""
    _, ts, tr = _schedule(spacing, zero_snr, n)
    worst, checked, sig = 0.0, 0, []
    for pred, eta in itertools.product(PREDS, (0.3, 1.0)):
        for i, (_, a, ap) in enumerate(tr):
            rc, got = coefs_eta(L, pred, a, ap, eta)
            if pred == "epsilon" and a == 0.0:                             # x0 is undefined there: the singular step of dd_op_step_coefs
                assert rc == -1, (ts[i], rc)
                continue
            assert rc == 0 and all(math.isfinite(v) for v in got), (pred, eta, ts[i], rc, got)
            ref = E.coefs_eta_ref(pred, a, ap, eta)
            for g_, r_ in zip(got, ref):
                if r_ == 0.0:
                    assert g_ == 0.0, (pred, eta, ts[i], got, ref)
                else:
                    worst = max(worst, abs(g_ - r_) / abs(r_))
            checked += 1
            assert 0.0 <= got[4] < 1.0                                      # 0 where a' = a: the t = 0 step of linspace
            if pred == "v_prediction" and eta == 1.0:
                sig.append(got[4])
    print("%s zero_snr=%s n=%d: %d steps, worst relative error %.2e, sigma at eta = 1 from %.3f to %.3f" % (spacing, zero_snr, n, checked, worst, sig[0], sig[-1]))
    assert checked >= 5 * n and worst <= 1e-6


def test_eta_zero_is_the_deterministic_table_bitwise(L):
    for (spacing, zero_snr, n), pred in itertools.product(SCHEDULES, PREDS):
        _, ts, tr = _schedule(spacing, zero_snr, n)
        for _, a, ap in tr:
            want = (C.c_float * 4)()
            rc4 = L.dd_op_step_coefs(R.PRED[pred], a, ap, want)
            rc, got = coefs_eta(L, pred, a, ap, 0.0)
            assert rc == rc4
            if rc == 0:
                assert np.array_equal(np.array(got[:4], np.float32).view(np.uint32), np.array(list(want), np.float32).view(np.uint32))
                assert got[4] == 0.0 and not math.copysign(1.0, got[4]) < 0


def test_never_nan_or_inf(L):
    """Every answer is five finite floats or -1: a = 0 at eta = 1 (the radicand of d is +-1e-16 there), a' = 1 (sigma = d = 0), the
    singular steps, eta outside [0, 1], and a schedule that is not monotone (a negative variance)."""
    for pred, eta in itertools.product(PREDS, (0.0, 0.5, 1.0)):
        for a, ap in ((0.0, 0.3), (0.0, 1e-4), (0.5, 1.0), (0.999, 1.0), (1e-6, 2e-6), (0.3, 0.3), (1.0, 1.0), (0.6, 0.4), (0.0, 0.0), (0.2, 0.0)):
            rc, got = coefs_eta(L, pred, a, ap, eta)
            assert rc in (0, -1)
            if rc == 0:
                assert all(math.isfinite(v) for v in got), (pred, eta, a, ap, got)
    rc, got = coefs_eta(L, "v_prediction", 0.0, 0.3, 1.0)                   # the first trailing step of a zero-terminal-SNR table
    assert rc == 0 and abs(got[4] - math.sqrt(0.7)) <= 1e-6 and abs(got[2]) <= 1e-7 and abs(got[3] + math.sqrt(0.3)) <= 1e-6
    rc, got = coefs_eta(L, "v_prediction", 0.5, 1.0, 1.0)                   # a' = 1: no noise, no direction
    assert rc == 0 and got[4] == 0.0
    assert coefs_eta(L, "epsilon", 0.0, 0.3, 1.0)[0] == -1 and coefs_eta(L, "sample", 1.0, 1.0, 0.5)[0] == -1
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert coefs_eta(L, "v_prediction", 0.5, 0.7, bad)[0] == -1
    assert coefs_eta(L, "v_prediction", 0.6, 0.4, 0.5)[0] == -1             # a > a': var < 0
    assert L.dd_op_step_coefs_eta(3, 0.5, 0.7, 0.5, (C.c_float * 5)()) == -1 and L.dd_op_step_coefs_eta(1, 0.5, 0.7, 0.5, None) == -1


@pytest.mark.parametrize("pred", PREDS)
def test_linear_form_is_the_diffusers_update(L, pred):
    """(A_z z + A_m m, B_z z + B_m m + sigma n) on the issue's coefficient expressions, in float64 == diffusers' form within 1e-10; and
    at eta = 1 the deterministic part is the DDPM posterior mean."""
    g = torch.Generator().manual_seed(5)
    worst, worst_pm = 0.0, 0.0
    for (spacing, n), eta in itertools.product((("leading", 10), ("trailing", 20), ("linspace", 50)), (0.0, 0.5, 1.0)):
        _, ts, tr = _schedule(spacing, False, n)
        for _, a, ap in tr:
            z, m, nz = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(3))
            sa, sb, sap = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap)
            sigma, d = E.sigma_d(a, ap, eta)
            if pred == "epsilon":
                Az, Am, Bz, Bm = 1 / sa, -sb / sa, sap / sa, d - sap * sb / sa
            elif pred == "v_prediction":
                Az, Am, Bz, Bm = sa, -sb, sap * sa + d * sb, d * sa - sap * sb
            else:
                Az, Am, Bz, Bm = 0.0, 1.0, d / sb, sap - d * sa / sb
            x0, zp = Az * z + Am * m, Bz * z + Bm * m + sigma * nz
            rx0, rzp = E.step_eta_ref(pred, a, ap, eta, z, m, nz)
            worst = max(worst, float((x0 - rx0).abs().max() / rx0.abs().max()), float((zp - rzp).abs().max() / rzp.abs().max()))
            if eta == 0.0:                                                  # and the restatement at eta = 0 is the one of the eta = 0 tests
                assert torch.equal(rzp, R.step_ref(pred, a, ap, z, m)[1])
            if eta == 1.0:
                pm = E.posterior_mean(a, ap, rx0, z)
                worst_pm = max(worst_pm, float((zp - sigma * nz - pm).abs().max() / pm.abs().max()))
    print("%s: worst relative difference of the two forms %.2e, of the eta = 1 mean from the DDPM posterior mean %.2e" % (pred, worst, worst_pm))
    assert worst <= 1e-10 and worst_pm <= 1e-10


def test_step_streams_are_independent():
    """tests/test_noise_rng.py::unit_values(seed, 16 + i, uid, n) is the restatement the GPU tests hold dd_randn_units and the fused
    generator to: streams 16 and 17 of one unit are N(0,1) and uncorrelated within 5 / sqrt(N), and neither is the initial noise."""
    N = 1 << 16
    x, y, z0 = (RNG.unit_values(RNG.MOMENT_SEED, st, 5, N) for st in (16, 17, 0))
    bm, bv, bk = RNG.moment_bounds(N)
    for v in (x, y):
        m, var, k = RNG.moments(v)
        assert abs(m) <= bm and abs(var - 1) <= bv and abs(k - 3) <= bk
    for u, v in ((x, y), (x, z0), (y, z0)):
        assert abs(float(np.corrcoef(u, v)[0, 1])) <= 5 / math.sqrt(N)
    assert not np.array_equal(x, RNG.unit_values(RNG.MOMENT_SEED, 16, 6, N))


def test_abi_surface():
    from distdiff_amd import _lib, engine
    assert _lib.ABI_VERSION >= 10
    for name in ("dd_set_schedule_e", "dd_denoise_step_n", "dd_direct_guidance_n"):
        assert name in _lib.ENGINE_SYMBOLS
    for name in ("dd_op_step_coefs_eta", "dd_op_sampler_step_n"):
        assert name in _lib.OPS_SYMBOLS
    assert "eta" not in [f[0] for f in engine.DDSamplerParams._fields_]          # an argument of dd_set_schedule_e, not a struct field


def test_cli_eta_flag(tmp_path):
    from distdiff_amd import generate_data as G
    assert G.parse_args([]).eta == 0.0
    assert G.parse_args(["--eta", "0.5"]).eta == 0.5 and G.parse_args(["--eta", "1"]).eta == 1.0
    for bad in (["--eta", "1.5"], ["--eta", "-0.1"], ["--eta", "nan"], ["--eta", "0.5", "--sampler", "dpmsolver++"]):
        with pytest.raises(SystemExit):
            G.parse_args(bad)
    assert G.parse_args(["--eta", "0", "--sampler", "dpmsolver++"]).sampler == "dpmsolver++"
    # --eta 0: the call sequence of today, argument for argument (no keyword reaches the engine in stream mode)
    one = ["--total_split", "1", "--split", "0"]
    base, calls0 = RNG._run(tmp_path, "a", one, EB=2)
    same, calls1 = RNG._run(tmp_path, "b", one + ["--eta", "0"], EB=2)
    assert base == same and len(calls0) == len(calls1) == 7
    for c0, c1 in zip(calls0, calls1):
        assert c1["kw"] == {} and torch.equal(c0["noise"], c1["noise"]) and c0["si"] == c1["si"] and c0["gt"] == c1["gt"]
    # --eta > 0, stream: the host's noise is still drawn and handed over; seed and unit ids key the step noise alone
    handed, calls = RNG._run(tmp_path, "c", one + ["--eta", "0.5"], EB=2)
    assert sorted(u for _, u in handed.values()) == sorted(G.unit_id(i, j) for i in range(7) for j in range(2))
    for c0, c in zip(calls0, calls):
        assert torch.equal(c0["noise"], c["noise"]) and c["kw"]["seed"] == 1234 and c["kw"]["generate_inputs"] is False
        assert set(c["kw"]) == {"seed", "unit_ids", "generate_inputs"}
    # --eta > 0, philox: the keywords of --noise_rng philox, nothing else
    _, callsp = RNG._run(tmp_path, "d", one + ["--eta", "0.5", "--noise_rng", "philox"], EB=2)
    assert all(c["noise"] is None and set(c["kw"]) == {"seed", "unit_ids", "offset_noise"} for c in callsp)
