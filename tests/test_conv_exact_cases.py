"""The exact-input case table (tests/conv_exact_cases.py) on the CPU: what the launcher plans for every case, what the table covers, and
what the exact comparison sees that the tolerance test does not.

dd_op_conv_gemm_plan tests pointers for null and reads no device, so routing drift of the cases of tests/test_conv_exact_gpu.py fails
here, without a GPU, for both libraries.  Coverage: every distinct non-refused (kind, form, narrow, split > 1) among the recorded outcomes
of tests/golden/conv_plan_table.npz for problems without CF_STATS / CF_LNFOLD / CF_ROWSTATS is the plan of at least one exact case.

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


def test_every_case_plans_as_stated(ops):
    bad = []
    for prob, plan, f16 in T.CASES:
        for dtype in (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,):
            got = T.plan_of(ops, prob, dtype)
            if got != plan:
                bad.append("%s (%s): planned %s, the case is about %s" % (prob.name, dtype, got, plan))
    assert not bad, "\n".join(bad)


def test_every_kind_and_form_runs_on_the_fp16_library():
    want = {(k, f) for _p, (k, f, _s), _h in T.CASES if "goes_general" not in _p.name}
    assert {(k, f) for _p, (k, f, _s), h in T.CASES if h} == want


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
    keep = (want[:, 0] >= 0) & ((flags & (plan_cases.STATS | plan_cases.LNFOLD | plan_cases.ROWSTATS)) == 0)
    w = want[keep].astype(np.int64)
    need = set(map(tuple, np.unique(np.stack([w[:, 0], w[:, 1], w[:, 3], (w[:, 2] > 1).astype(np.int64)], axis=1), axis=0).tolist()))
    assert len(need) >= 19, sorted(need)
    have = set()
    for prob, _plan, _f16 in T.CASES:
        kind, form, split, narrow = raw_plan(ops, prob)
        have.add((kind, form, narrow, int(split > 1)))
    assert not need - have, "recorded (kind, form, narrow, split > 1) that no exact case runs: %s" % sorted(need - have)


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
