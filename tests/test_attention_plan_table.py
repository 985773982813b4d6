"""The attention launcher's decision, case by case, against the table recorded at commit cbe2388 (tests/golden/attention_plan_table.npz,
from that commit's own dispatch code with the kernel launches intercepted, before the decision was reorganised into one planner:
tests/golden/make_attention_plan_table.py says how).  dd_op_attention_plan only tests pointers for null and touches no device, so this
runs on a CPU.

Every problem of tests/attention_plan_cases.py must give the recorded route, tile form, flags, images per GEMM group and the grid / block /
dynamic LDS of every launch, refusals included.  The second test checks, on the recorded data alone, that the table is not vacuous.  The
third: the scratch the graph builder asks the planner for is what Builder::attn computed itself at that commit, for the engine's shapes.
"""
import ctypes as C
import os

import numpy as np
import pytest

import attention_plan_cases as cases

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_plan_table.npz")


@pytest.fixture(scope="module")
def table():
    t = np.load(TABLE)
    blks = list(cases.blocks())
    assert str(t["cases_sha256"]) == cases.cases_hash(blks), "tests/attention_plan_cases.py no longer generates the cases the table was recorded for"
    assert [n for n, _r in blks] == [str(n) for n in t["block_names"]] and [len(r) for _n, r in blks] == t["block_sizes"].tolist()
    want = t["outcomes"][t["index"]]
    assert want.shape[1] == cases.OUT_N
    offs = np.concatenate([[0], np.cumsum(t["block_sizes"])])
    return {n: (rows, want[offs[i]:offs[i + 1]]) for i, (n, rows) in enumerate(blks)}


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    _lib.lib()
    return _lib.LIB_PATH


def test_every_case_plans_as_recorded(table, lib_path):
    bad, lines = 0, []
    for name, (rows, want) in table.items():
        got = cases.evaluate(lib_path, rows)
        diff = np.nonzero((got != want).any(axis=1))[0]
        bad += len(diff)
        for i in diff[:max(0, 12 - len(lines))]:
            lines.append("%s[%d]: recorded %s, got %s  (%s)" % (name, i, want[i].tolist(), got[i].tolist(), cases.describe(rows, i)))
    if bad:
        print("\n".join(lines))
    assert bad == 0, "%d cases plan differently from the record; %s + launches of the first:\n%s" % (bad, cases.OUT_FIELDS, "\n".join(lines))


def test_recorded_table_covers_the_decision(table):
    c, o = cases.COL, cases.OCOL
    rows = np.concatenate([r for r, _w in table.values()])
    want = np.concatenate([w for _r, w in table.values()])
    route, bits, waves = want[:, o["route"]], want[:, o["bits"]], want[:, o["waves"]]
    bwd = rows[:, c["bwd"]] != 0
    for r in (cases.ROUTE_GEMM, cases.ROUTE_SHORTK, cases.ROUTE_DMA, cases.ROUTE_STREAM):
        assert ((route == r) & ~bwd).sum() >= 1000, "forward route %s" % cases.ROUTES[r]
    assert ((route == cases.ROUTE_GEMM) & bwd).sum() >= 500 and ((route == cases.ROUTE_FLASH_BWD) & bwd).sum() >= 1000
    assert not ((route == cases.ROUTE_FLASH_BWD) & ~bwd).any()
    dma = route == cases.ROUTE_DMA
    for w in (4, 8):
        assert (dma & (waves == w)).sum() >= 1000, "LDS-DMA kernel on %d waves" % w
    for lazy in (0, cases.BIT_LAZY):
        assert (dma & (bits & cases.BIT_LAZY == lazy)).sum() >= 1000
    fp8 = dma & (bits & cases.BIT_FP8 != 0)
    assert fp8.sum() >= 100 and (want[fp8][:, o["kt"]] == 128).all() and (rows[fp8][:, c["fp8"]] == 1).all()
    assert ((route == cases.ROUTE_STREAM) & (bits & cases.BIT_CAUSAL != 0)).sum() >= 1000
    assert ((route == cases.ROUTE_FLASH_BWD) & (bits & cases.BIT_PRESCALED != 0)).sum() >= 1000
    assert ((route == cases.ROUTE_FLASH_BWD) & (want[:, o["launches"]] == 2)).sum() >= 1000          # dQ only
    assert ((route == cases.ROUTE_FLASH_BWD) & (want[:, o["launches"]] == 3)).sum() >= 1000
    assert (want[:, o["dsplit"]] == 4).sum() >= 100 and (want[:, o["dsplit"]] == 1).sum() >= 1000
    for d in (32, 40, 64, 80, 160, 512):
        assert ((want[:, o["d"]] == d) & ~bwd).any() and ((want[:, o["d"]] == d) & bwd).any(), "form of d = %d" % d
    for g in (1, 2, 8):
        assert ((route == cases.ROUTE_GEMM) & (want[:, o["group"]] == g)).sum() >= 10, "GEMM groups of %d" % g

    # short keys refused by each of its conditions: the same problem is short-key in the plain block and not in the other
    def differs(a, b, cond=None):
        (ra, wa), (rb, wb) = table[a], table[b]
        m = (wa[:, 0] == cases.ROUTE_SHORTK) & (wb[:, 0] != cases.ROUTE_SHORTK) & (wb[:, 0] >= 0)
        return (m if cond is None else m & cond(ra, rb)).any()
    assert differs("fwd_plain", "fwd_no_shortk") and differs("fwd_plain", "fwd_causal") and differs("fwd_plain", "fwd_fp8")
    plain_r, plain_w = table["fwd_plain"]
    sk = plain_w[:, 0] == cases.ROUTE_SHORTK
    assert set(np.unique(plain_r[sk][:, c["D"]]).tolist()) == {40, 64, 80}
    assert plain_r[sk][:, c["Nk"]].max() == 80 and (plain_r[sk][:, c["Nq"]] % 32 == 0).all()
    ok = plain_w[:, 0] >= 0
    assert (ok & ~sk & (plain_r[:, c["Nk"]] == 81) & (plain_r[:, c["Nq"]] == 64) & (plain_r[:, c["D"]] == 40)).any()      # too many keys
    assert (ok & ~sk & (plain_r[:, c["Nk"]] == 77) & (plain_r[:, c["Nq"]] == 50) & (plain_r[:, c["D"]] == 40)).any()      # ragged queries
    assert (ok & ~sk & (plain_r[:, c["Nk"]] == 77) & (plain_r[:, c["Nq"]] == 64) & (plain_r[:, c["D"]] == 160)).any()     # no kernel for d
    for below, at in (("fwd_ldq_edge-8", "fwd_ldq_edge+0"), ("fwd_ldk_edge-8", "fwd_ldk_edge+0"), ("fwd_ldv_edge-8", "fwd_ldv_edge+0")):
        assert differs(below, at), at                                                                                     # 32-bit offsets
    # ... and the same limit moves the LDS-DMA kernel to the register-staged one
    (_r, wa), (_r2, wb) = table["fwd_ldk_edge-8"], table["fwd_ldk_edge+0"]
    assert ((wa[:, 0] == cases.ROUTE_DMA) & (wb[:, 0] == cases.ROUTE_STREAM)).any()

    # one refusal per reason
    def refused(name, cond=None):
        r, w = table[name]
        m = w[:, 0] < 0
        return (m if cond is None else m & cond(r)).any()
    assert refused("fwd_plain", lambda r: r[:, c["D"]] == 48) and refused("fwd_plain", lambda r: r[:, c["D"]] == 256)     # no form, no scratch
    assert refused("bwd_dkv", lambda r: r[:, c["D"]] == 48)
    for name in ("ldq", "ldk", "ldv"):
        assert refused("fwd_%s+4" % name) and refused("bwd_%s+4" % name), name
    assert not refused("fwd_ldo+4") and (table["fwd_ldo+4"][1][:, 0] != cases.ROUTE_GEMM).all()      # o rows & 3: only the GEMM route wants & 7
    assert refused("fwd_ldo+2") and refused("bwd_ldo+2") and refused("bwd_lddo+4") and refused("bwd_lddq+2") and refused("bwd_lddk+2") and refused("bwd_lddv+2")
    assert refused("bwd_lddq+4", lambda r: r[:, c["ws_images"]] > 0) and not refused("bwd_lddq+4", lambda r: r[:, c["ws_images"]] == 0)   # & 7: GEMM only
    assert refused("bwd_no_lse") and refused("bwd_no_delta")
    assert refused("fwd_no_lse", lambda r: r[:, c["ws_images"]] > 0) and not refused("fwd_no_lse", lambda r: r[:, c["ws_images"]] == 0)
    # scratch too small for the GEMM route is no refusal where a flash form exists: d = 512 without scratch streams
    assert (plain_w[plain_r[:, c["D"]] == 512][:, 0] == cases.ROUTE_STREAM).all()


def test_scratch_bytes_match_the_graph_builder(lib_path):
    """attention_scratch_bytes against the expression Builder::attn carried before the planner:
    D >= 256 && cross_slot < 0 && !causal  ->  attention_gemm_workspace(Nq, Nk, D, want_grad) * (heads == 1 ? min(B, 8) : 1)"""
    L = C.CDLL(lib_path)
    L.dd_op_attention_scratch_bytes.argtypes, L.dd_op_attention_scratch_bytes.restype = [C.c_int] * 8, C.c_size_t
    L.dd_op_attention_gemm_workspace.argtypes, L.dd_op_attention_gemm_workspace.restype = [C.c_int] * 4, C.c_size_t
    wide = 0
    for B, H, Nq, Nk, D, flags, self_attn in cases.ENGINE_OPS:
        causal = "causal" in flags
        for grad in (0, 1):
            want = 0
            if D >= 256 and self_attn and not causal:
                want = L.dd_op_attention_gemm_workspace(Nq, Nk, D, grad) * (min(B, 8) if H == 1 else 1)
                wide += 1
            assert L.dd_op_attention_scratch_bytes(B, H, Nq, Nk, D, int(causal), int(not self_attn), grad) == want, (B, H, Nq, Nk, D, flags, grad)
    assert wide >= 8
