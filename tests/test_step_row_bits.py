"""The host numbers of the sampler step, pinned: every call of tests/golden/make_step_row_bits.py replayed on this build and compared,
return code by return code and word by word, with tests/golden/step_row_bits.npz -- recorded from the build that had seven
coefficient functions (sampler_step_coefs, _coefs_eta, _eta_d, _coefs_sde, _sde_d, _coef_2m, _coef_2m_sde) behind the five dd_op_step_coef*
symbols.  Integers are compared, not floats: a refused call must return the recorded code and leave the buffer as recorded (the
unwritten *out of dd_op_step_coef_2m_sde, the row a stochastic rule had written before it found it not finite).  No GPU call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_step_row_bits as M  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    return _lib.lib()


def test_the_grid_is_the_recorded_one():
    fx, cs = M.load(), M.cases()
    assert len(cs) == M.N_CASES == 6687 and fx["rc"].shape == (6687,) and fx["bits"].shape == (6687, 5)
    assert np.array_equal(fx["cases"], np.array(cs, dtype=np.float64))
    # the record holds what it is there for: refusals of every kind, and the deterministic row that is not finite with code 0
    rc, bits, c = fx["rc"], fx["bits"], fx["cases"]
    assert set(rc.tolist()) == {0, -1}
    for fn in (0, 1, 2, 4):
        assert (rc[c[:, 0] == fn] == -1).any() and (rc[c[:, 0] == fn] == 0).any()
    tiny = (c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 5] == 1e-80)
    assert tiny.sum() == 1 and rc[tiny][0] == 0 and not np.isfinite(bits[tiny][0, :4].view(np.float32)).any()
    assert (bits[(c[:, 0] == 4) & (rc == -1)] == M.FILL).all()


def test_numbers_are_the_recorded_ones(L):
    fx = M.load()
    cs = [tuple(int(v) for v in row[:4]) + tuple(float(v) for v in row[4:]) for row in fx["cases"]]
    rc, bits = M.replay(L, cs)
    bad_rc = np.flatnonzero(rc != fx["rc"])
    assert bad_rc.size == 0, "%d return codes differ, first: case %s gives %d, recorded %d" % (
        bad_rc.size, cs[bad_rc[0]], rc[bad_rc[0]], fx["rc"][bad_rc[0]])
    bad = np.flatnonzero((bits != fx["bits"]).any(axis=1))
    assert bad.size == 0, "%d of %d buffers differ, first: case %s gives %s, recorded %s" % (
        bad.size, len(cs), cs[bad[0]], [hex(w) for w in bits[bad[0]]], [hex(w) for w in fx["bits"][bad[0]]])
