"""The bits of the sampling loop under every kind of schedule, pinned: every case of tests/golden/make_schedule_bits.py replayed on this
build and compared with the SHA-256 digests of tests/golden/schedule_bits.npz, recorded from the build in which the engine kept its
schedule as loose fields (coef_table, step_table, their eta twins, c2m, c2m_sde, sigma, eta, sde_eta, solver) filled by seven coefficient
functions.  tests/test_dpm_solver_gpu.py, test_ddim_eta_gpu.py and test_dpm_sde_gpu.py show within one build that `expand` is the
step-by-step calls bit for bit; this file compares the build with the record."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_schedule_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_record_holds_every_case():
    # per library 12 cases on 'eps' and 12 + 4 on 'sd2', three outputs each
    assert len(M.ALL_CASES) == 2 * (12 + 16) == 56
    assert sorted(M.load()) == sorted(n + "/" + o for n in M.ALL_CASES for o in M.OUTPUTS)


@pytest.mark.parametrize("kind,act", M.ENGINES, ids=["%s-%s" % e for e in M.ENGINES])
def test_bits_are_the_recorded_ones(hip_lib, kind, act):
    assert torch.cuda.is_available()
    rec = M.load()
    want = {k: v for k, v in rec.items() if k.startswith("%s/%s/" % (act, kind))}
    assert len(want) == 3 * (16 if kind == "sd2" else 12)
    got = M.replay(kind, act)
    assert sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
