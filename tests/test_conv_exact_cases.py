"""The exact-input case table (tests/conv_exact_cases.py) on the CPU: what the launcher plans for every case, what the table covers, and
what the exact comparison sees that the tolerance test does not.

dd_op_conv_gemm_plan tests pointers for null and reads no device, so routing drift of the cases of tests/test_conv_exact_gpu.py fails
here, without a GPU, for both libraries.  Coverage: every distinct non-refused (kind, form, narrow, split > 1, CF_STATS, CF_ROWSTATS,
CF_LNFOLD, GEGLU) among the recorded outcomes of tests/golden/conv_plan_table.npz is the plan of at least one exact case of CASES or
STAT_CASES; the list of combinations without a closed form is asserted whole and is empty.  What the launcher must refuse of the
statistics flags is asserted as refused.

Seven more mutants (exact_ref.STAT_MUTANTS) stand for faults of the statistics, fold and GEGLU epilogues; each must show in the exact
comparison of the whole buffers on every case it applies to, and what the tolerance tests of tests/test_kernels_gpu.py make of the same
mutant on their own kind of inputs is printed beside it.

Sensitivity: three mutants of the reference (tests/exact_ref.py: one 8-channel vector of one tap dropped at the last image column, two
taps swapped, the first 64-channel chunk used twice) must show as mismatches of the exact comparison on every ternary case they apply to;
at the K = 23040 shape of the 8 x 8 level the first of them stays inside the limit of tests/test_kernels_gpu.py::assert_close on that
test's own kind of inputs (both numbers are printed).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as T
import conv_plan_cases as plan_cases
import exact_ref as X
from test_conv_plan_table import TABLE


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import ops as o
    return o


def raw_plan(ops, prob, dtype=torch.bfloat16, rowspan=0):
    """(kind, form, split, narrow) as dd_op_conv_gemm_plan returns them"""
    pk, x, kw, _out = T.launch_args(ops, prob, dtype, rowspan=rowspan)
    p, cap, _y, _keep = ops._conv_gemm_params(x, pk, *prob.geom, dry=True, **kw)
    out4 = (C.c_int * 4)()
    kind = ops._L(pk).dd_op_conv_gemm_plan(C.byref(p), cap, out4)
    return kind, out4[1], out4[2], out4[3]


def test_case_names_are_unique():
    assert len(set(T.NAMES)) == len(T.NAMES)
    assert len(set(T.STAT_NAMES)) == len(T.STAT_NAMES) and not set(T.STAT_NAMES) & set(T.NAMES)


def test_every_case_plans_as_stated(ops):
    bad = []
    for prob, plan, f16, rowspan in [c + (0,) for c in T.CASES] + [c[:4] for c in T.STAT_CASES]:
        for dtype in (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,):
            try:
                got = T.plan_of(ops, prob, dtype, rowspan=rowspan)
            except RuntimeError as e:
                got = "refused (%s)" % e
            if got != plan:
                bad.append("%s (%s): planned %s, the case is about %s" % (prob.name, dtype, got, plan))
    assert not bad, "\n".join(bad)


def test_statistics_refusals_are_refused(ops):
    """what the launcher must refuse is asserted here and never launched"""
    for prob, rowspan in T.STAT_REFUSALS:
        for dtype in (torch.bfloat16, torch.float16):
            with pytest.raises(RuntimeError, match="refuses"):
                T.plan_of(ops, prob, dtype, rowspan=rowspan)


def test_every_kind_and_form_runs_on_the_fp16_library():
    want = {(k, f) for _p, (k, f, _s), _h in T.CASES if "goes_general" not in _p.name}
    assert {(k, f) for _p, (k, f, _s), h in T.CASES if h} == want
    kind_of = lambda p: "".join(sorted(c for c in p.fl.replace("G", "g") if c in "swlg"))
    want = {(k, f, kind_of(p)) for p, (k, f, _s), *_r in T.STAT_CASES}
    assert {(k, f, kind_of(p)) for p, (k, f, _s), h, *_r in T.STAT_CASES if h} >= {w for w in want if len(w[2]) == 1}     # one per form and statistics kind


def test_record_cases_plan_as_their_records_state(ops):
    for key, (prob, _salt, span, plan) in T.record_problems().items():
        if not T.closed_form_outputs(prob):
            continue
        got = T.plan_of(ops, prob, rowspan=span)
        if isinstance(plan, tuple):
            assert got == plan, (key, got, plan)
        else:
            assert got[0] == ops.CONV_GEMM_KINDS[plan], (key, got, plan)


def test_table_covers_every_recorded_plan(ops):
    t = np.load(TABLE)
    rows = np.concatenate([r for _n, r in plan_cases.blocks()])
    want = t["outcomes"][t["index"]]
    assert len(rows) == len(want)
    flags = rows[:, plan_cases.COL["flags"]]
    # an empty problem (M <= 0 or N <= 0) is accepted and launches nothing: no kernel, no output, nothing to compare
    keep = (want[:, 0] >= 0) & (rows[:, plan_cases.COL["M"]] > 0) & (rows[:, plan_cases.COL["N"]] > 0)
    w, f = want[keep].astype(np.int64), flags[keep]
    bit = lambda b: ((f & b) != 0).astype(np.int64)
    key = np.stack([w[:, 0], w[:, 1], w[:, 3], (w[:, 2] > 1).astype(np.int64), bit(plan_cases.STATS), bit(plan_cases.ROWSTATS), bit(plan_cases.LNFOLD),
                    bit(plan_cases.GEGLU)], axis=1)
    need = set(map(tuple, np.unique(key, axis=0).tolist()))
    assert len(need) >= 60, sorted(need)
    have = set()
    for prob, rowspan in [(c[0], 0) for c in T.CASES] + [(c[0], c[3]) for c in T.STAT_CASES]:
        kind, form, split, narrow = raw_plan(ops, prob, rowspan=rowspan)
        fl = prob.fl
        have.add((kind, form, narrow, int(split > 1), int("s" in fl), int("w" in fl), int("l" in fl), int("g" in fl or "G" in fl)))
    assert NO_CLOSED_FORM == [], "every statistics, fold and GEGLU output has a closed form on ternary inputs"
    missing = need - have - set(NO_CLOSED_FORM)
    assert not missing, "recorded (kind, form, narrow, split > 1, stats, rowstats, lnfold, geglu) that no exact case runs: %s" % sorted(missing)


NO_CLOSED_FORM = []      # recorded combinations that cannot be compared exactly: none


def _one_image(prob):
    """the case with its batch cut to one image (a GEMM: to 4096 rows): what a mutant changes depends on the taps, the channels, the depth
    of K and the epilogue, not on how many rows there are, and the halo kinds need hundreds of thousands of them"""
    return prob._replace(B=1, H=min(prob.H, 4096) if prob.W == 1 else prob.H)


def _geometry(prob):
    return prob[1:10]         # B Cin Cout H W k stride pad up


def test_mutants_of_the_reference_show_on_every_ternary_case():
    """per distinct forward geometry: the epilogue variants of one geometry share its sums, and each is compared"""
    seen = {}
    for i, (prob, _plan, _f16) in enumerate(T.CASES):
        if prob.dgrad or "g" in prob.fl:
            continue
        prob = _one_image(prob)
        seen.setdefault(_geometry(prob), []).append((i, prob))
    assert len(seen) >= 25
    quiet, applied = [], {name: 0 for name, _fn, _a in X.MUTANTS}
    for group in seen.values():
        i0, p0 = group[0]
        inp0 = X.make_inputs(p0, "ternary", i0)
        acc = X.accumulate(p0, inp0["x"], inp0["w"])
        deltas = [(name, X.mutant_rows(p0, inp0, fn)) for name, fn, applies in X.MUTANTS if applies(p0)]
        for i, prob in group:
            inp = dict(X.make_inputs(prob, "ternary", i), x=inp0["x"], w=inp0["w"])
            want = X.finish(prob, acc, inp)
            X.check_conditions(prob, inp, "ternary", ref=want)
            assert X.mismatch_report(prob, want, want) is None
            for name, d in deltas:
                applied[name] += 1
                rep = X.mismatch_report(prob, X.finish(prob, acc + d, inp), want)
                if rep is None:
                    quiet.append((prob.name, name))
                elif name == "dropped_vector":
                    assert "all on an image border: True" in rep, rep
    print("mutants applied (cases): %s" % applied)
    assert not quiet, "mutants the exact comparison did not see: %s" % quiet
    assert min(applied.values()) >= 25


def test_dropped_vector_passes_the_tolerance_test_at_k23040():
    """Cin 2560 -> Cout 1280 at 8 x 8, 8 images, on inputs of the kind tests/test_kernels_gpu.py::test_conv_forward_and_dgrad draws: the
    largest error of a dropped vector against that test's limit atol + 1.5 % max|ref|, for each of the six taps that read inside the image
    at the last column and four vectors each; and what the exact comparison counts on ternary inputs of the same shape"""
    prob = X.Problem("k23040", 8, 2560, 1280, 8, 8)
    g = torch.Generator().manual_seed(0)
    bf = lambda t: t.to(torch.bfloat16).float()
    x = bf(torch.randn(prob.B * 64, 2560, generator=g))
    w = bf(torch.randn(1280, 2560, 3, 3, generator=g) / math.sqrt(23040))
    bias = torch.randn(1280, generator=g)
    inp = dict(x=x, w=w)
    ref = X.accumulate(prob, x, w) + bias[None, :]
    lim = 1e-3 + 1.5e-2 * float(ref.abs().max())
    noise = float((bf(ref) - ref).abs().max())
    errs = []
    for tap in (0, 1, 3, 4, 6, 7):
        for c0 in (0, 8, 16, 24):
            mut = lambda p, xx, ww: X.mutant_dropped_vector(p, xx, ww, tap=tap, first_ch=c0)
            errs.append(float((bf(ref + X.mutant_rows(prob, inp, mut)) - ref).abs().max()))
    everywhere = float((bf(ref + X.mutant_rows(prob, inp, lambda p, xx, ww: X.mutant_dropped_vector(p, xx, ww, last_column_only=False))) - ref).abs().max())
    ti = X.make_inputs(prob, "ternary", 7)
    acc = X.accumulate(prob, ti["x"], ti["w"])
    want = X.finish(prob, acc, ti)
    X.check_conditions(prob, ti, "ternary", ref=want)
    wrong = int((X.bits(X.finish(prob, acc + X.mutant_rows(prob, ti, X.mutant_dropped_vector), ti)) != X.bits(want)).sum())
    print("K = 23040: assert_close limit %.4f; the correct result's own bf16 rounding %.4f; one vector of one tap dropped at the last column: "
          "largest error %.4f .. %.4f over 24 vectors, %d of them inside the limit; dropped at every pixel %.4f; exact comparison on ternary "
          "inputs: %d of %d border outputs wrong, largest |y| %d"
          % (lim, noise, min(errs), max(errs), sum(e <= lim for e in errs), everywhere, wrong, prob.B * 8 * 1280, int(want.float().abs().max())))
    assert all(e > noise for e in errs)
    assert any(e <= lim for e in errs), "no dropped vector passes the tolerance test any more: %r against %.4f" % (errs, lim)
    assert wrong > 1000


# ---- the statistics / fold / GEGLU outputs: mutants of the reference, and what the tolerance tests make of them ----------------------

def _gaussian_inputs(prob):
    """operands of the kind tests/test_kernels_gpu.py draws for a GEMM case (test_layernorm_folded_into_linear under "l", else
    test_linear_emits_layernorm_row_partials / test_conv_emits_groupnorm_partials), and the rows' own (mean, rstd)"""
    g = torch.Generator().manual_seed(77)
    bf = lambda t: t.to(torch.bfloat16).float()
    M, K, N = prob.M, prob.Cin, prob.N
    x = bf(torch.randn(M, K, generator=g) * 1.7 + torch.randn(M, 1, generator=g) * 0.8) if "l" in prob.fl else bf(torch.randn(M, K, generator=g))
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if "l" in prob.fl:
        w = w * (1.0 + 0.3 * torch.randn(K, generator=g))[None, :]
    res = bf(torch.randn(M, N, generator=g)) if "r" in prob.fl else None
    st = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)
    return dict(x=x, w=bf(w)[:, :, None, None], bias=torch.randn(N, generator=g), res=res, mask=None, ln_stats=st)


def _tolerance_view(name):
    """(largest error, limit, note): what the assertion of tests/test_kernels_gpu.py that guards the mutant's output computes for it on
    that test's kind of Gaussian inputs (limit = atol + rtol * max|ref|, its assert_close); None, None and a fact where the test has no
    assertion that could see the mutant"""
    close = lambda got, ref, rtol, atol: (float((got - ref).abs().max()), atol + rtol * float(ref.abs().max()))
    if name in ("last_row_of_a_block_twice", "stats_in_front_of_the_relu"):
        prob = X.Problem("gauss", 1, 320, 320, 4096, 1, k=1, fl="brus" if "relu" in name else "brs")
        inp = _gaussian_inputs(prob)
        acc = X.accumulate(prob, inp["x"], inp["w"])
        slot_of = X.slots_m64(prob)
        ref = X.expected_stats(prob, X.epilogue(prob, acc, inp), slot_of)
        sv = X.epilogue(prob._replace(fl="brs"), acc, inp) if "relu" in name else X.epilogue(prob, acc, inp)
        mut = X.expected_stats(prob, sv, slot_of, name if "relu" not in name else None)
        e1, l1 = close(mut[:, :, 0], ref[:, :, 0], 2e-3, 2e-3)
        e2, l2 = close(mut[:, :, 1], ref[:, :, 1], 2e-2, 2e-2)
        note = "partial mean %.4f against %.4f, partial M2 %.3f against %.3f" % (e1, l1, e2, l2)
        if "relu" in name:
            note += " (and test_conv_emits_groupnorm_partials has no case with a ReLU)"
        return max(e1 / l1, e2 / l2), 1.0, note
    if name == "narrow_halo_tile_in_slot_m64":
        import test_kernels_gpu as K
        narrow = [c[0] for c in K.STATS_CASES if K.STATS_PLANS[c[0]][0].startswith("conv_halo") and X.halo_tile_width(X.Problem(c[0], *c[1:6])) < 64
                  and c[5] // X.halo_tile_width(X.Problem(c[0], *c[1:6])) > 1]
        return None, None, ("%d of the cases of test_conv_emits_groupnorm_partials that run a halo kernel have several tiles narrower than 64 pixels per "
                            "image row: the block map never runs there" % len(narrow))
    if name == "span_sums_in_the_neighbouring_span":
        return 0.0, None, "test_linear_emits_layernorm_row_partials and test_weight_stationary_gemm sum the partials over the spans: a permutation of spans changes nothing they look at"
    geglu = name != "ln_stats_of_the_neighbouring_row"
    fl = "bG" if name == "last_gate_group_with_the_previous_hidden" else ("bGl" if geglu else "bl")
    prob = X.Problem("gauss", 1, 320, 2560 if geglu else 960, 1500 if fl == "bG" else 4096, 1, k=1, fl=fl)
    inp = _gaussian_inputs(prob)
    acc = X.accumulate(prob, inp["x"], inp["w"])

    def y(mutant):
        v = X.epilogue(prob, acc, inp, mutant)
        if not geglu:
            return v
        grp = v.reshape(prob.M, prob.N // 32, 2, 16)
        h, gate = grp[:, :, 0].clone(), grp[:, :, 1]
        if mutant == "last_gate_group_with_the_previous_hidden":
            h[:, -1] = h[:, -2]
        return (h * F.gelu(gate)).reshape(prob.M, prob.N // 2)
    err, lim = close(y(name), y(None), 1.5e-2, 2e-2 if "l" in fl else 1e-3)
    return err, lim, "largest error %.4f against the limit %.4f" % (err, lim)


def test_mutants_of_the_statistics_outputs_show_on_every_case():
    """Seven mutants of the reference's statistics, fold and GEGLU epilogues (exact_ref.STAT_MUTANTS), each on every case of STAT_CASES it
    applies to, cut to one image or 4096 rows: the exact comparison of the whole buffers must see every one.  What the tolerance tests
    of tests/test_kernels_gpu.py compute for the same mutant on their kind of inputs is printed beside it, not asserted."""
    quiet, applied = [], {name: 0 for name, _fl, _a in X.STAT_MUTANTS}
    for i, (prob, _plan, _f16, rowspan, slots) in enumerate(T.STAT_CASES):
        prob = _one_image(prob)
        muts = [name for name, need, applies in X.STAT_MUTANTS if all(c in prob.fl for c in need) and applies(prob)
                and (slots == "halo" or name != "narrow_halo_tile_in_slot_m64")]          # the block map is the halo kernels'
        if not muts:
            continue
        inp = X.make_inputs(prob, "ternary", i)
        acc = X.accumulate(prob, inp["x"], inp["w"])
        want, _found = T.stat_expected(prob, acc, inp, torch.bfloat16, rowspan, slots)
        for name in muts:
            applied[name] += 1
            got, _f = T.stat_expected(prob, acc, inp, torch.bfloat16, rowspan, slots, mutant=name, check=False)
            if all(X.mismatch_report(prob, got[k], want[k]) is None for k in want if k != "v"):
                quiet.append((prob.name, name))
    print("statistics mutants applied (cases): %s" % applied)
    for name, _fl, _a in X.STAT_MUTANTS:
        err, lim, note = _tolerance_view(name)
        verdict = "no assertion looks" if lim is None else ("inside its limit" if err <= lim else "outside its limit")
        print("  %s: exact comparison sees it on %d of %d cases; tolerance test: %s -- %s" % (name, applied[name] - sum(n == name for _p, n in quiet), applied[name], verdict, note))
    assert not quiet, "mutants the exact comparison did not see: %s" % quiet
    assert min(applied.values()) >= 2, applied


def test_gelu_emulation_equals_the_oracle_evaluation_on_the_gate_table():
    """exact_ref's gelu (every fma formed exactly, rounded once) against the evaluation of tests/test_oracle.py::test_gelu_polynomial
    (float64 product and sum, then one rounding to fp32: a double rounding) on the multiples of 1 / 8 inside the clamp: where the two
    differ it is printed, and the exact one is what the GPU comparison uses"""
    clamp, c = X.gelu_literals()
    _clamp, table = X.gate_table()
    t = np.arange(-int(clamp * X.GATE_LATTICE), int(clamp * X.GATE_LATTICE) + 1, dtype=np.float32) / np.float32(X.GATE_LATTICE)
    c = np.array(c, dtype=np.float32)
    u = (t * t).astype(np.float32)
    p = np.full_like(u, c[9])
    for k in range(8, -1, -1):
        p = (p.astype(np.float64) * u + c[k]).astype(np.float32)
    phi = (t.astype(np.float64) * p + 0.5).astype(np.float32)
    differ = np.nonzero(phi.view(np.int32) != table.numpy().view(np.int32))[0]
    for i in differ:
        print("gate %g: float64 evaluation %r, exact fmas %r" % (t[i], float(phi[i]), float(table[i])))
    print("gelu on the gate table: %d of %d values differ between the float64 evaluation and the exact one" % (len(differ), len(t)))
    assert len(t) == 73 and np.abs(phi.astype(np.float64) - table.numpy().astype(np.float64)).max() <= 2.0 ** -23      # a last place at most
    assert float(table[0]) >= 0.0 and abs(float(table[-1]) - 1.0) <= 2e-6 and float(table[len(t) // 2]) == 0.5


# ---- tests/test_kernels_gpu.py: the plan dicts of the statistics / fold / weight-stationary tests, answered here without a device --------

def test_tolerance_test_plan_dicts_hold(ops):
    import test_kernels_gpu as K
    z, e = torch.zeros, torch.empty
    assert set(K.WS_PLANS) == {c[0] for c in K.WS_CASES} and set(K.STATS_PLANS) == {c[0] for c in K.STATS_CASES}
    for name, M, N, res, lnfold, rowstats, geglu in K.WS_CASES:
        views = "views" in name
        ncols = N // 2 if geglu else N
        pk = ops.PackedConv(z(N, 320), 0, geglu=geglu, bias=z(N), device="cpu")
        kw = dict(y=e(M, ncols + (32 if views else 0), dtype=torch.bfloat16)[:, :ncols], ksplit=1, x_ld=320 + (64 if views else 0), res=True if res else None,
                  ln_stats=True if lnfold else None, rowpart=e(M, N // 40, 2) if rowstats else None, raw=e(M, N, dtype=torch.bfloat16) if geglu and lnfold else None)
        got = ops.conv_gemm_plan(None, pk, 1, M, 1, M, 1, **kw)
        assert got == K.WS_PLANS[name], (name, got)
        for word, kind in (("pingpong", "gemm_pps"), ("two_workgroup", "general")):      # a name that states a kernel states the one that runs
            assert word not in name or got[0] == kind, (name, got)
    for (M, Cc, N, geglu), plan in K.LNFOLD_PLANS.items():
        pk = ops.PackedConv(z(N, Cc), 0, geglu=geglu, bias=z(N), device="cpu")
        assert ops.conv_gemm_plan(None, pk, 1, M, 1, M, 1, ksplit=1, ln_stats=True) == plan, (M, Cc, N, geglu)
    for (M, Kk, N), plan in K.ROWPART_PLANS.items():
        pk = ops.PackedConv(z(N, Kk), 0, bias=z(N), device="cpu")
        assert ops.conv_gemm_plan(None, pk, 1, M, 1, M, 1, res=True, ksplit=1, rowpart=e(M, N // 40, 2)) == plan, (M, Kk, N)
    for case in K.STATS_CASES:
        name, B, Cin, Cout, H, W, k, with_res = case[:8]
        pk = ops.PackedConv(z(Cout, Cin, k, k), k // 2, bias=z(Cout), device="cpu")
        y, st = e(B * H * W, Cout + 64, dtype=torch.bfloat16)[:, 64:], e(B * H * W // 64, Cout + 64, 2)[:, 64:]
        got = ops.conv_gemm_plan(None, pk, B, H, W, H, W, res=True if with_res else None, y=y, stats=st)
        assert got == K.STATS_PLANS[name], (name, got)
        assert not name.startswith("halo") or got[0].startswith("conv_halo"), (name, got)


# ---- tests/test_kernels_gpu.py::CONV_CASES: the names say what runs -----------------------------------------------------------------

_STATES_A_PLAN = ("big", "halo", "n3_", "n4_")
_FORMS = ("128x256", "256x160", "256x128", "128x160", "128x128")


def _form_in(text):
    found = [f for f in _FORMS if f in text]
    return found[0] if found else None


def test_conv_case_names_say_what_runs(ops):
    import test_kernels_gpu as K
    names = [c[0] for c in K.CONV_CASES]
    assert len(set(names)) == len(names)
    stating = [c for c in K.CONV_CASES if c[0].startswith(_STATES_A_PLAN)]
    assert {c[0] for c in stating} == set(K.CONV_PLANS), "CONV_PLANS must hold exactly the cases whose names state a kernel or a form"
    assert {f for c in stating for f in [_form_in(c[0].split("_dgrad_")[0])] if f} == set(_FORMS)      # every big form forward ...
    assert {_form_in(c[0].split("_dgrad_")[1]) for c in stating if "_dgrad_" in c[0]} >= {"128x256", "256x128", "128x160", "128x128"}   # ... and as an input gradient
    for case in K.CONV_CASES:
        name, _B, Cin, Cout, _H, _W, k, _stride, pad = case[:9]
        (fgeom, fkw), (dgeom, dkw) = K.conv_case_launches(case)
        w = torch.zeros(Cout, Cin, k, k)
        fwd = ops.conv_gemm_plan(None, ops.PackedConv(w, pad, mode=0, bias=torch.zeros(Cout), device="cpu"), *fgeom, **fkw)
        dgrad = ops.conv_gemm_plan(None, ops.PackedConv(w, pad, mode=1, device="cpu"), *dgeom, **dkw)
        for part in name.split("_"):
            if part.startswith("split") and part[5:].isdigit():
                assert fwd[2] == int(part[5:]), (name, fwd)
        if not name.startswith(_STATES_A_PLAN):
            if "small" in name:                                 # the small kernel, and no split unless the name has one
                assert fwd[1].startswith("small") and (fwd[2] == 1 or "_split" in name), (name, fwd)
            continue
        assert (fwd, dgrad) == K.CONV_PLANS[name], "%s: planned %s, CONV_PLANS says %s" % (name, (fwd, dgrad), K.CONV_PLANS[name])
        head, _, tail = name.partition("_dgrad_")
        if name.startswith("big"):
            assert fwd[0] == "general" and fwd[1].startswith("big_")
            assert _form_in(head) is None or _form_in(head) in fwd[1], (name, fwd)
            assert ("ks1" in name) == (len(case) > 10 and case[10] == 1) and ("ks1" not in name or fwd[2] == 1)
        if name.startswith("halo_persist"):
            assert fwd[0] == "conv_halo_persist", (name, fwd)
        elif name.startswith("halo"):
            assert fwd[0] in ("conv_halo", "conv_halo_persist"), (name, fwd)
        if name.startswith(("n3_", "n4_")):
            assert fwd[1] == "small_256x64", (name, fwd)
        if tail:
            assert _form_in(tail) in dgrad[1], (name, dgrad)
