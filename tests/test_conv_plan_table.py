"""The conv / GEMM launcher's decision, case by case, against the table recorded at commit 691758c (tests/golden/conv_plan_table.npz:
written by tests/golden/make_conv_plan_table.py before the decision code was reorganised into one planner).  dd_op_conv_gemm_plan only
tests pointers for null and touches no device (without one the CU count keeps its default, 256: the MI355X's own), so this runs on a CPU.

Every problem of tests/conv_plan_cases.py must give the recorded (kind, form, split, narrow), refusals included.  The second test checks, on
the recorded data alone, that the table is not vacuous: every kind, every general form, both splits, the flag-dependent path and every
row-span width are in it.
"""
import os

import numpy as np
import pytest

import conv_plan_cases as cases

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.npz")


@pytest.fixture(scope="module")
def table():
    t = np.load(TABLE)
    blks = list(cases.blocks())
    assert str(t["cases_sha256"]) == cases.cases_hash(blks), "tests/conv_plan_cases.py no longer generates the cases the table was recorded for"
    assert [n for n, _r in blks] == [str(n) for n in t["block_names"]] and [len(r) for _n, r in blks] == t["block_sizes"].tolist()
    want = t["outcomes"][t["index"]]
    offs = np.concatenate([[0], np.cumsum(t["block_sizes"])])
    return {n: (rows, want[offs[i]:offs[i + 1]]) for i, (n, rows) in enumerate(blks)}


def test_every_case_plans_as_recorded(table):
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    _lib.lib()
    bad, lines = 0, []
    for name, (rows, want) in table.items():
        got = cases.evaluate(_lib.LIB_PATH, rows)
        diff = np.nonzero((got != want).any(axis=1))[0]
        bad += len(diff)
        for i in diff[:max(0, 12 - len(lines))]:
            lines.append("%s[%d]: recorded %s, got %s  (%s)" % (name, i, want[i].tolist(), got[i].tolist(), cases.describe(rows, i)))
    if bad:
        print("\n".join(lines))
    assert bad == 0, "%d cases plan differently from the record; (kind, form, split, narrow) of the first:\n%s" % (bad, "\n".join(lines))


def test_recorded_table_covers_the_decision(table):
    c = cases.COL
    rows = np.concatenate([r for r, _w in table.values()])
    want = np.concatenate([w for _r, w in table.values()])
    kind, form, split, narrow = want.T
    flags = rows[:, c["flags"]]
    for k in (-1, 0, 1, 2, 3, 4):
        assert (kind == k).sum() >= 1000, "kind %d" % k
    for f in range(6):                                           # the general forms: conv_gemm_kernel 128 x 128, conv_gemm_big_kernel 1 .. 5
        assert ((kind == 0) & (form == f) & (narrow == 0)).sum() >= 1000, "general form %d" % f
    assert ((kind == 0) & (form == 0) & (narrow == 1)).sum() >= 1000                 # conv_gemm_kernel 256 x 64
    assert ((kind == 0) & (split > 1)).sum() >= 1000                                 # split-K
    assert ((kind == 1) & (split > 1)).sum() >= 100                                  # chunk split of the halo 8 x 8 level
    st = (flags & cases.STATS) != 0
    assert (st & (kind == 1)).any() and (st & (kind == 2)).any() and (st & (kind == 4)).any() and (st & (kind == 0) & (form > 0)).any()
    assert (st & (kind == -1)).any()
    # the flag-dependent path: the same problem is gemm_ws without CF_STATS and gemm_pps with it
    plain, stats = table["grid_%d" % cases.BIAS][1], table["grid_%d" % (cases.BIAS | cases.STATS)][1]
    assert ((plain[:, 0] == 3) & (stats[:, 0] == 4)).any()
    # every row-span width: accepted at rowpart_ld = N / d, refused at the next narrower one
    w = table["rowstats"][1].reshape(-1, len(cases.ROWPART_DIVS), 4)      # [problem][N / 40, N / 64, N / 80, N / 160]
    k4, f4 = w[:, :, 0], w[:, :, 1]
    assert ((k4[:, 0] == 3) & (k4[:, 1] == -1)).any()                                 # ws: N / 40 spans
    assert ((k4[:, 2] == 4) & (k4[:, 3] == -1)).any()                                 # pps: N / 80
    assert ((k4[:, 2] == 0) & (f4[:, 2] == 4) & (k4[:, 3] == -1)).any()               # big form 4: N / 80
    assert ((k4[:, 1] == 0) & (f4[:, 1] == 5) & (k4[:, 2] == -1)).any()               # big form 5: N / 64
