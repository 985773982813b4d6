"""The conv / GEMM kernels (conv_gemm.hip, conv_gemm2.hip, conv_halo.hip, gemm_ws.hip, gemm_pps.hip) on exact inputs, bit for bit.

On the two input families of tests/exact_ref.py every product and partial sum is exact in fp32, so a kernel's output is the closed form
in any order of summation -- chunk splits, split-K and its reduce kernel included -- and is compared with NO tolerance: the int16 / int32
view of the whole output buffer, the NaN prefill beyond the N valid columns included, must equal the reference's.  A dropped operand
vector, a swapped tap or a stage that was not refilled changes thousands of elements (tests/test_conv_exact_cases.py shows it on the CPU),
where the 1.5 % tolerance of tests/test_kernels_gpu.py lets some of them pass at deep K.  tests/test_bit_records_exact.py derives the
recorded MI355X bits from the same reference.

test_conv_gemm_stat_outputs_exact does the same for the outputs that have closed forms on ternary inputs only: the GroupNorm partials
(CF_STATS), the LayerNorm row partials (CF_ROWSTATS), the output of a GEMM with the LayerNorm folded in (CF_LNFOLD) and the GEGLU product,
each buffer whole, with its NaN prefill.

Every case first asserts the (kind, form, split) it is about through ops.conv_gemm_plan (tests/conv_exact_cases.py; the same table is
walked on the CPU).  A failure prints exact_ref.mismatch_report: how many elements, the first eight as (image, oy, ox, n), whether they
all lie on an image border, their row index modulo the tile height.
"""
import os
import subprocess
import sys

import pytest
import torch

import conv_exact_cases as T
import exact_ref as X

pytestmark = pytest.mark.gpu
FAMILIES = ("lattice", "ternary")


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distdiff_amd import ops as o
    assert torch.cuda.is_available()
    return o


_SUMS = {}      # (geometry, dgrad, family) -> (operands, accumulate()): the epilogue variants of one geometry share the CPU conv; the last two kept


def shared_sums(prob, family):
    key = (prob[1:11], family)
    if key not in _SUMS:
        while len(_SUMS) >= 2:
            _SUMS.pop(next(iter(_SUMS)))
        inp = X.make_inputs(prob._replace(fl=""), family, salt=sum(prob[1:10]) % 251)
        _SUMS[key] = dict(x=inp["x"], w=inp["w"], dx=inp["dx"], dw=inp["dw"]), X.accumulate(prob, inp["x"], inp["w"])
    return _SUMS[key]


def run_exact(ops, prob, plan, family, dtypes, salt, rowspan=0, shared=True):
    inp = X.make_inputs(prob, family, salt)
    if shared:
        operands, acc = shared_sums(prob, family)
        inp.update(operands)
    else:
        acc = X.accumulate(prob, inp["x"], inp["w"])
    for dtype in dtypes:
        want = X.finish(prob, acc, inp, dtype)
        X.check_conditions(prob, inp, family, dtype, ref=want)
        pk, x, kw, out = T.launch_args(ops, prob, dtype, inp, "cuda", rowspan=rowspan)
        got = ops.conv_gemm_plan(x, pk, *prob.geom, **kw)
        if isinstance(plan, tuple):
            assert got == plan, "%s (%s): the launcher plans %s, the case is about %s" % (prob.name, dtype, got, plan)
        else:
            assert got[0] == ops.CONV_GEMM_KINDS[plan], (prob.name, got, plan)
        ops.conv_gemm(x, pk, *prob.geom, **kw)
        torch.cuda.synchronize()
        rep = X.mismatch_report(prob, out, want)
        assert rep is None, "%s inputs, %s, plan %s\n%s" % (family, dtype, got, rep)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", T.CASES, ids=T.NAMES)
def test_conv_gemm_exact(ops, case, family):
    prob, plan, f16 = case
    if plan[0] == T.PERSIST and os.environ.get("DD_HALO_PERSIST") == "0":     # the child process of test_halo_switch_fallbacks_stay_exact
        plan = (T.HALO, None, plan[2])
    run_exact(ops, prob, plan, family, (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,), salt=T.NAMES.index(prob.name))


@pytest.mark.parametrize("case", T.STAT_CASES, ids=T.STAT_NAMES)
def test_conv_gemm_stat_outputs_exact(ops, case):
    """CF_STATS, CF_ROWSTATS, CF_LNFOLD and the GEGLU product on ternary inputs (tests/exact_ref.py: expected_buffers), bit for bit: the
    plan, then y, then the WHOLE partials / row-partials / raw buffer -- the NaN prefill in front of the op's channels and in the three
    spare span slots included.  The (mean, rstd) rows of the fold are synthetic (small integers, powers of two): the kernels only read them."""
    prob, plan, f16, rowspan, slots = case
    if plan[0] == T.PERSIST and os.environ.get("DD_HALO_PERSIST") == "0":     # the child process of test_halo_switch_fallbacks_stay_exact
        plan = (T.HALO, None, plan[2])
    inp = X.make_inputs(prob, "ternary", T.STAT_NAMES.index(prob.name))
    operands, acc = shared_sums(prob, "ternary")
    inp.update(operands)
    for dtype in (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,):
        want, _found = T.stat_expected(prob, acc, inp, dtype, rowspan, slots)
        got = {}
        pk, x, kw, _out = T.launch_args(ops, prob, dtype, inp, "cuda", rowspan=rowspan, bufs=got)
        planned = ops.conv_gemm_plan(x, pk, *prob.geom, **kw)
        assert planned == plan, "%s (%s): the launcher plans %s, the case is about %s" % (prob.name, dtype, planned, plan)
        ops.conv_gemm(x, pk, *prob.geom, **kw)
        torch.cuda.synchronize()
        assert set(got) == set(want) - {"v"}, (sorted(got), sorted(want))
        for name in ("y", "raw", "stats", "rowpart"):
            if name in got:
                rep = X.mismatch_report(prob, got[name], want[name])
                assert rep is None, "%s of %s, ternary inputs, %s, plan %s\n%s" % (name, prob.name, dtype, planned, rep)


RECORDS = {k: v for k, v in T.record_problems().items() if T.closed_form_outputs(v[0])}


@pytest.mark.parametrize("key", sorted(RECORDS))
def test_record_case_equals_the_closed_form(ops, key):
    """the cases of the two bit records that have a closed form, on the record's own inputs: a failure names a place instead of a hash"""
    prob, salt, span, plan = RECORDS[key]
    run_exact(ops, prob, plan, "lattice", (torch.bfloat16,), salt, rowspan=span, shared=False)


def test_halo_switch_fallbacks_stay_exact():
    """`DD_HALO_TAB=0` (per-piece address arithmetic instead of the address table) and `DD_HALO_PERSIST=0` (decoder levels on the one-tile
    form) select code the default configuration never runs; they are read once per process.  The halo cases once more in a child process
    with both set (with DD_HALO_PERSIST=0 the launcher's kind query answers conv_halo for the persistent cases)."""
    env = dict(os.environ, DD_HALO_TAB="0", DD_HALO_PERSIST="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "(test_conv_gemm_exact and (halo_ or persist_) and not goes_general) or "
                          "(test_conv_gemm_stat_outputs_exact and (s_halo_ or s_persist_))"], capture_output=True, text=True, timeout=900, env=env,
                         cwd=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-1000:]
