"""The case table of tests/golden/make_norm_bits.py reaches every path of the norm kernels' launch arithmetic: asserted on the CPU from
make_norm_bits.paths(), a Python mirror of gn_split, gn_apply_blocks, the column map of the GroupNorm passes, the register budget of
gn_finalize_chan_kernel and the VI switch of launch_layernorm_fwd."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_norm_bits as M  # noqa: E402

P = {n: M.paths(n) for n in M.NAMES}


def _any(kind, pred):
    return any(p["kind"] in kind and pred(p) for p in P.values())


def test_case_names_are_unique_and_of_every_kind():
    assert len(set(M.NAMES)) == len(M.NAMES)
    assert {p["kind"] for p in P.values()} == {"gn", "part", "ln", "rowpart"}


def test_groupnorm_column_map():
    assert _any(("gn",), lambda p: p["VC"] < 256 and p["idle"] > 0) and _any(("gn",), lambda p: p["VC"] > 256 and p["second_sweep"])
    assert _any(("gn",), lambda p: p["cpg"] == 1) and _any(("gn",), lambda p: p["cpg"] == 10 and p["straddle"])
    assert _any(("gn",), lambda p: p["cpg"] % 8 == 0)
    assert _any(("gn",), lambda p: p["R_over_rows"])


def test_groupnorm_splits():
    assert _any(("gn",), lambda p: p["S"] == 1) and _any(("gn",), lambda p: 1 < p["S"] <= 64) and _any(("gn",), lambda p: p["S"] > 64)
    assert _any(("gn",), lambda p: p["S_capped"] and p["S"] == 256 and p["empty"] > 0 and p["ragged"] > 0)
    assert _any(("gn",), lambda p: p["ragged"] > 0 and p["empty"] == 0)


def test_groupnorm_apply_cap():
    assert _any(("gn",), lambda p: p["apply_capped"]) and _any(("gn", "part"), lambda p: not p["apply_capped"])
    capped = [n for n, p in P.items() if p["kind"] == "gn" and p["apply_capped"]]
    assert capped == ["gn_gridcap"] and (P["gn_gridcap"]["apply_wanted"], P["gn_gridcap"]["apply_allowed"]) == (160, 129)


def test_channel_partials():
    assert _any(("part",), lambda p: p["P"] <= 3072 and p["P_in_registers"]) and _any(("part",), lambda p: p["P"] > 3072)
    assert _any(("part",), lambda p: p["P"] == 3072)


def test_layernorm_paths():
    assert {p["VI"] for p in P.values() if p["kind"] == "ln"} == {1, 2, 3, 4}
    assert _any(("ln",), lambda p: p["row_tail"] != 0) and _any(("ln",), lambda p: p["M"] == 1)
    assert _any(("ln",), lambda p: p["idle_lanes"] > 0) and _any(("ln",), lambda p: p["idle_lanes"] == 0)
    assert _any(("rowpart",), lambda p: p["spans"] == 1) and _any(("rowpart",), lambda p: p["spans"] > 1)
    assert _any(("rowpart",), lambda p: p["blocks"] > 1 and p["row_tail"] != 0)


def test_record_matches_the_table():
    """The record names the parent commit and holds, for both libraries, every output of every case, and every input digest."""
    rec = M.load()
    assert str(rec["parent_commit"]) == M.PARENT == "6266c73"
    outs = {"gn": ("y", "stats", "dx", "dx_acc"), "part": ("y", "stats"), "ln": ("y", "stats", "stats_only", "dx", "dx_acc"), "rowpart": ("stats",)}
    want = sorted("%s/%s/%s" % (lib, n, o) for lib in M.LIBS for n, k, _ in M.CASES for o in outs[k])
    assert rec["case_names"].tolist() == want and len(rec["case_sha256"]) == len(want)
    assert all(len(d) == 64 for d in rec["case_sha256"].tolist() + rec["input_sha256"].tolist() + rec["library_sha256"].tolist())
    ins = dict(zip(rec["input_names"].tolist(), rec["input_sha256"].tolist()))
    for n in (n for n in M.NAMES if n.startswith(("ln_", "rowpart_"))):    # the generator gives the recorded inputs (GroupNorm: the GPU test)
        got = M.input_digests(n)
        assert got and all(ins[k] == v for k, v in got.items()), n
    assert sorted(ins) == sorted(k for n in M.NAMES for k in _input_names(n))


def _input_names(name):
    kind = M.CASES[M.NAMES.index(name)][1]
    t = {"gn": ("x", "dy", "prev", "gamma", "beta"), "part": ("x", "gamma", "beta", "chan_part"), "ln": ("x", "dy", "prev", "gamma", "beta"),
         "rowpart": ("x", "rowpart")}[kind]
    return ["%s/%s" % (name, k) for k in t]
