"""CPU checks of the DPM-Solver++(2M) sampler: the library's host coefficient (dd_op_step_coef_2m, what dd_set_schedule fills its
table with) against the float64 restatement of tests/dpm_solver_ref.py on the real schedules, its zero cases, the identity the kernel
rests on (DDIM step + c (x0 - x0_prev) == the update as diffusers writes it), the order of convergence on a model with a known answer,
and the CLI flag.  No GPU call."""
import dataclasses
import itertools
import math

import pytest
import torch

import dpm_solver_ref as D
import sampler_variants_ref as R


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    return _lib.lib()


def _schedule(spacing="leading", zero_snr=False, n=10):
    from distdiff_amd.config import SchedulerConfig
    from distdiff_amd.scheduler import DDIMSchedule
    sc = dataclasses.replace(SchedulerConfig(), timestep_spacing=spacing, rescale_betas_zero_snr=zero_snr)
    assert sc.beta_schedule == "scaled_linear" and sc.steps_offset == 1 and sc.num_train_timesteps == 1000      # the SD-1.x file
    s = DDIMSchedule(sc)
    ts = s.set_timesteps(n)
    return s, ts, D.triples(s.alphas_cumprod, s.final_alpha_cumprod, ts)


SCHEDULES = list(itertools.product(["leading", "trailing", "linspace"], [False, True], [10, 20, 50]))


@pytest.mark.parametrize("spacing,zero_snr,n", SCHEDULES)
def test_library_coefficient_matches_the_restatement(L, spacing, zero_snr, n):
    """Formed in double, rounded to fp32 once (6e-8): relative error <= 1e-6 wherever the restatement is not 0, exactly 0 where it is."""
    _, ts, tr = _schedule(spacing, zero_snr, n)
    worst, nonzero = 0.0, 0
    for i, (ab, a, ap) in enumerate(tr):
        got = L.dd_op_step_coef_2m(i, n, ab if ab is not None else 0.0, a, ap)
        ref = D.coef_2m_ref(i, n, ab if ab is not None else 0.0, a, ap)
        assert math.isfinite(got)
        if ref == 0.0:
            assert got == 0.0, (i, ts[i], got)
        else:
            nonzero += 1
            worst = max(worst, abs(got - ref) / abs(ref))
    print("%s zero_snr=%s n=%d: %d second-order steps, worst relative error %.2e" % (spacing, zero_snr, n, nonzero, worst))
    # every interior step is second-order, but the one behind a = 0 of a zero-terminal-SNR table that starts at t = 999
    assert nonzero == n - 2 - (1 if zero_snr and ts[0] == 999 else 0)
    assert worst <= 1e-6


def test_zero_cases_are_exactly_zero(L):
    c = L.dd_op_step_coef_2m
    a0, a1, a2 = 0.2, 0.4, 0.6
    assert c(3, 10, a0, a1, a2) > 0.0                                      # the same triple inside a schedule is a second-order step
    for got in (c(0, 10, a0, a1, a2),                                       # i = 0: nothing before it
                c(9, 10, a0, a1, a2),                                       # i = n - 1: the final step is first-order
                c(1, 2, a0, a1, a2), c(0, 1, a0, a1, a2),                   # ... also of a one- or two-step schedule
                c(1, 10, 0.0, a1, a2),                                      # a_{i-1} = 0 (zero terminal SNR): lambda = -inf
                c(3, 10, a0, 0.0, a2),
                c(3, 10, a0, a1, 1.0),                                      # a' = 1 (set_alpha_to_one): lambda = +inf
                c(3, 10, a0, a1, a1),                                       # h = 0
                c(3, 10, a1, a1, a2),                                       # r = 0: c would be inf
                c(3, 10, float("nan"), a1, a2), c(3, 10, a0, a1, 1.5), c(3, 10, -0.1, a1, a2)):
        assert got == 0.0 and not math.isnan(got), got
    for spacing, zero_snr, n in SCHEDULES:                                  # and on the real tables: first, last, behind a = 0
        _, ts, tr = _schedule(spacing, zero_snr, n)
        for i in (0, n - 1) + ((1,) if tr[0][1] == 0.0 else ()):
            ab, a, ap = tr[i]
            assert c(i, n, ab if ab is not None else 0.0, a, ap) == 0.0


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_ddim_step_plus_correction_is_the_diffusers_update(pred):
    """DDIM step (eta = 0) + c (x0 - x0_prev) == (sigma'/sigma) z - alpha' (e^-h - 1) D, D = x0 + (x0 - x0_prev) / (2 r), in float64."""
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for spacing, n in (("leading", 10), ("trailing", 20), ("linspace", 50)):
        _, ts, tr = _schedule(spacing, False, n)
        for i in range(1, n - 1):
            ab, a, ap = tr[i]
            z, m, xp = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(3))
            x0, zp = R.step_ref(pred, a, ap, z, m)
            got = zp + D.coef_2m_ref(i, n, ab, a, ap) * (x0 - xp)
            rx0, ref = D.update_2m_ref(pred, ab, a, ap, z, m, xp)
            assert torch.equal(rx0, x0)
            worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
            # and without a history the diffusers form is the DDIM step
            assert float((D.update_2m_ref(pred, ab, a, ap, z, m, None)[1] - zp).abs().max() / zp.abs().max()) <= 1e-10
    print("%s: worst relative difference of the two forms %.2e" % (pred, worst))
    assert worst <= 1e-10


def _gaussian_model_error(L, n, second_order):
    """Data N(0, s^2) per element, s^2 = 0.25: the exact denoiser is x0 = sqrt(a) s^2 / V(a) z with V(a) = a s^2 + 1 - a, and the exact
    probability-flow solution z_end / z_start = sqrt(V(a_end) / V(a_start)).  Runs steps 0 .. n - n/5 - 1 of the n-step leading schedule
    as an epsilon model, with the library's own coefficients, and returns the relative error at the a' of the last executed step."""
    import ctypes as C
    s2 = 0.25
    V = lambda a: a * s2 + 1 - a
    _, ts, tr = _schedule("leading", False, n)
    z, x0_prev = 1.0, None
    last = n - n // 5 - 1
    lin = (C.c_float * 4)()
    for i in range(last + 1):
        ab, a, ap = tr[i]
        assert L.dd_op_step_coefs(0, a, ap, lin) == 0
        Az, Am, Bz, Bm = (float(x) for x in lin)
        x0_true = math.sqrt(a) * s2 / V(a) * z
        m = (z - math.sqrt(a) * x0_true) / math.sqrt(1 - a)                 # what an exact epsilon model returns
        x0 = Az * z + Am * m
        c = L.dd_op_step_coef_2m(i, n, ab if ab is not None else 0.0, a, ap) if (second_order and x0_prev is not None) else 0.0
        z = Bz * z + Bm * m + (c * (x0 - x0_prev) if c else 0.0)
        x0_prev = x0
    exact = math.sqrt(V(tr[last][2]) / V(tr[0][1]))
    return abs(z - exact) / exact


def test_order_of_convergence_on_a_gaussian_model(L):
    """Relative errors in float64: DDIM 2.53e-2 (n = 20), 1.10e-2 (n = 40); 2M 1.76e-3, 4.25e-4.  Halving the step divides the DDIM
    error by 2.29 (first order) and the 2M error by 4.15 (second order).  The whole schedule is not asserted on: its error is that of
    the first-order final step."""
    err = {(n, so): _gaussian_model_error(L, n, so) for n in (20, 40) for so in (False, True)}
    print("relative error  n=20: DDIM %.3e, 2M %.3e   n=40: DDIM %.3e, 2M %.3e   ratios: DDIM %.2f, 2M %.2f, DDIM/2M at 40 %.1f"
          % (err[20, False], err[20, True], err[40, False], err[40, True], err[20, False] / err[40, False], err[20, True] / err[40, True],
             err[40, False] / err[40, True]))
    assert err[40, True] < err[40, False] / 10
    assert err[20, True] / err[40, True] > 3
    assert err[20, False] / err[40, False] < 3


def test_cli_sampler_flag(capsys):
    from distdiff_amd import generate_data as G
    from distdiff_amd import engine
    assert G.parse_args([]).sampler == "ddim"
    assert G.parse_args(["--sampler", "dpmsolver++"]).sampler == "dpmsolver++"
    with pytest.raises(SystemExit):
        G.parse_args(["--sampler", "euler"])
    assert "invalid choice" in capsys.readouterr().err
    assert engine.SOLVERS == {"ddim": 0, "dpmsolver++": 1}
    assert "solver" not in [f[0] for f in engine.DDSamplerParams._fields_]        # an argument of dd_set_schedule_s, not a struct field
