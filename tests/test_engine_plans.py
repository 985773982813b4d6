"""The engine's plans, pinned on the CPU: every case of tests/golden/make_engine_plans.py is planned on this build (dd_debug_plan_only: fake
device addresses, no GPU) and compared record by record with tests/golden/engine_plans.npz, recorded before engine_graph.cpp, the engine
object and the plan switches were reorganised.  What is compared: every tensor (offsets, shapes, gradient intervals, transient slots) and
op (operands, backward plan, fusion plan) of the six programs, their totals, the workspace size and the packed-weight layout."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_engine_plans as M  # noqa: E402

K = {n: i for i, n in enumerate(M.OP_KINDS)}
OF = {n: i for i, n in enumerate(M.OP_FIELDS)}
TF = {n: i for i, n in enumerate(M.TENSOR_FIELDS)}


@pytest.fixture(scope="module")
def record():
    return M.load()


def _first_differences(name, want, got, fields, limit=5):
    if want.shape != got.shape:
        return ["%s: %d records recorded, %d now" % (name, len(want), len(got))]
    rows = np.flatnonzero((want != got).any(axis=1))
    out = ["%s: %d of %d records differ" % (name, len(rows), len(want))] if len(rows) else []
    for r in rows[:limit]:
        out.append("  %s[%d]: " % (name, r) + ", ".join("%s %d -> %d" % (fields[c], want[r, c], got[r, c]) for c in np.flatnonzero(want[r] != got[r])))
    return out


@pytest.mark.parametrize("name", list(M.CASES))
def test_plans_are_the_recorded_ones(hip_lib, record, name):
    got = M.plan(name)
    diff = []
    w, g = record[name + "/engine"], got["engine"]
    for i, f in enumerate(("total_bytes", "partial_cap", "tmp_cap", "packed buffers")):
        if w[i] != g[i]:
            diff.append("engine: %s %d -> %d" % (f, w[i], g[i]))
    if len(w) != len(g) or (w[4:] != g[4:]).any():
        at = next((i for i, (a, b) in enumerate(zip(w[4:], g[4:])) if a != b), min(len(w), len(g)) - 4)
        diff.append("engine: the packed weight buffers differ from buffer %d on" % at)
    diff += _first_differences("programs", record[name + "/programs"], got["programs"], M.PROGRAM_FIELDS, limit=6)
    if name + "/sha256" in record:
        now = M.digests(got)
        diff += ["%s: tensor / op records differ (digest only)" % M.PROGRAMS[p] for p in range(6) if now[p] != record[name + "/sha256"][p]]
    else:
        for p, prog in enumerate(M.PROGRAMS):
            diff += _first_differences(prog + ".t", record["%s/tensors%d" % (name, p)], got["tensors%d" % p], M.TENSOR_FIELDS)
            diff += _first_differences(prog + ".ops", record["%s/ops%d" % (name, p)], got["ops%d" % p], M.OP_FIELDS)
    print("\n".join(diff))
    assert not diff, "%s: the plan differs from the recorded one:\n%s" % (name, "\n".join(diff[:40]))


def _raw(record, what):
    return [record[k] for k in record if k.rsplit("/", 1)[-1].startswith(what)]


def test_the_record_is_not_vacuous(record):
    """On the recorded data alone: the table holds every case, every op kind, both outcomes of every planning decision, and every plan
    switch moves at least one field of the configuration it was recorded on."""
    assert all(n + "/engine" in record and n + "/programs" in record for n in M.CASES)
    assert all(n + "/sha256" in record or n + "/ops0" in record for n in M.CASES)
    ops, ts = np.concatenate(_raw(record, "ops")), np.concatenate(_raw(record, "tensors"))
    assert sorted(set(ops[:, OF["kind"]].tolist())) == list(range(len(M.OP_KINDS)))
    conv, cat = ops[ops[:, OF["kind"]] == K["CONV"]], ops[ops[:, OF["kind"]] == K["CONCAT"]]
    gn, ln = ops[ops[:, OF["kind"]] == K["GN"]], ops[(ops[:, OF["kind"]] == K["LN"]) & (ops[:, OF["ln_fold"]] == 1)]
    for f in ("x_acc", "res_acc", "res_alias"):
        assert set(conv[:, OF[f]].tolist()) == {0, 1}, f
    assert set(cat[:, OF["fused"]].tolist()) == {0, 1}
    assert set(gn[:, OF["gn_fused"]].tolist()) == {0, 1} and set(conv[conv[:, OF["part"]] == 1][:, OF["gn_fused"]].tolist()) == {0, 1}
    assert (ln[:, OF["row_spans"]] == 0).any() and (ln[:, OF["row_spans"]] > 0).any()
    assert (conv[:, OF["row_spans"]] > 0).any() and (conv[conv[:, OF["rowstat_emit"]] == 1][:, OF["row_spans"]] == 0).any()
    assert set(ts[ts[:, TF["transient"]] == 1][:, TF["tr_slot"]].tolist()) == {0, 1}
    assert (ts[:, TF["glo"]] >= 0).any() and (ts[:, TF["parent"]] != np.concatenate([np.arange(len(t)) for t in _raw(record, "tensors")])).any()
    assert (record["tiny_nograd/programs"][:3, 3] == 0).all() and (record["tiny/programs"][:3, 3] > 0).all()      # grad_bytes
    assert (record["tiny_sdxl_enc/programs"][:, 1] > 0).all()                                                   # all six programs
    for sw in M.SWITCHES:
        for base in ("tiny", "sd15_L64_B32"):
            keys = [k[len(base) + 1:] for k in record if k.startswith(base + "/") and k.count("/") == 1]
            moved = [k for k in keys if record["%s/%s" % (base, k)].shape != record["%s/%s/%s" % (base, sw, k)].shape or
                     (record["%s/%s" % (base, k)] != record["%s/%s/%s" % (base, sw, k)]).any()]
            assert moved, "%s does not change the plan of %s" % (sw, base)
