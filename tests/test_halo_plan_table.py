"""What the launcher does with a halo 3x3 problem beyond the bits: tile geometry, address table, LDS bytes and grid of every halo problem of
the test tables against tests/golden/halo_plan_table.npz (tests/golden/make_halo_plan_table.py says what is in it and when it was
recorded).  dd_op_conv_halo_plan tests pointers for null and touches no device (without one the CU count keeps its default, 256: the
MI355X's own), so this runs on a CPU, for both libraries.

A tile width, the table decision and the grid change no output bit, only the speed: this table is the one check that sees the host side
of conv_halo.hip pick another tiling.  The second test checks, on the recorded data alone, that the table is not vacuous.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_halo_plan_table as R  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with np.load(R.PATH) as f:
        return {k: f[k] for k in f.files}


def test_every_halo_problem_plans_as_recorded(table):
    import __graft_entry__ as g
    g.build()
    assert tuple(str(n) for n in table["fields"]) == R.FIELDS
    labels, p, caps, bnames, bsizes, rownos, names = R.problems()
    assert bnames == [str(n) for n in table["block_names"]] and bsizes == table["block_sizes"].tolist() and (rownos == table["rows"]).all()
    assert names == [str(n) for n in table["names"]], "the halo cases of the test tables are not the recorded ones: re-record, and say why"
    for dt, path in R.lib_paths().items():
        want = table["outcomes_" + dt][table["index_" + dt]]
        got = R.evaluate(path, p, caps)
        diff = np.nonzero((got != want).any(axis=1))[0]
        lines = ["%s: %s" % (labels[i], ", ".join("%s recorded %d got %d" % (R.FIELDS[j], want[i, j], got[i, j]) for j in np.nonzero(got[i] != want[i])[0]))
                 for i in diff[:12]]
        assert not len(diff), "%s library: %d halo problems plan differently from the record of %s; the first:\n%s" % (
            dt, len(diff), table["commit"], "\n".join(lines))


def test_recorded_table_covers_the_decision(table):
    for dt in R.LIBS:
        w = table["outcomes_" + dt][table["index_" + dt]].astype(np.int64)
        col = lambda n: w[:, R.F[n]]
        assert len(w) == table["block_sizes"].sum() + len(table["names"]) and (col("kind") > 0).all()
        assert set(np.unique(col("form")).tolist()) == {1, 2, 4, 5, 6}                   # every HALO_FORMS id
        assert set(np.unique(col("kind")).tolist()) == {1, 2}                            # conv_halo_kernel, conv_halo_persist_kernel
        assert ((col("persist") == 1) == (col("kind") == 2)).all()
        assert (col("grid_y") > 1).any() and ((col("grid_y") > 1) <= (col("images_per_tile") == 4)).all()     # the chunk split of the 8 x 8 level
        assert set(np.unique(col("images_per_tile")).tolist()) == {1, 4}
        assert {16, 32, 64, 128} <= set(np.unique(col("tw")).tolist())
        assert set(np.unique(col("table")).tolist()) == {0, 1}
        # the table is dropped where it does not FIT (not only where a form never has it: the multi-image tiles)
        assert ((col("table") == 0) & (col("images_per_tile") == 1) & (col("lds_bytes") + ((col("tw") + 2) * (col("th") + 2) + 7) // 8 * 256 > 163840)).any()
        assert (col("lds_bytes") <= 163840).all() and (col("tw") * col("th") * col("images_per_tile") % 256 == 0).all()
