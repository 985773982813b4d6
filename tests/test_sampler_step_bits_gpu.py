"""The bits of the sampler step, pinned: every case of tests/golden/make_sampler_step_bits.py replayed on this build from the stored
inputs and compared, output by output, with the SHA-256 digests recorded in tests/golden/sampler_step_bits.npz from the build that had
one kernel per mode (cfg_ddim, sampler_step, sampler_step_2m<EPS> and their two backward kernels).  The bitwise tests of
tests/test_sampler_step_gpu.py and tests/test_dpm_solver_gpu.py compare one entry point with another of the same build; this one
compares the build with the record."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_sampler_step_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(hip_lib):
    assert torch.cuda.is_available()
    return M.load()


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.tag)
def test_bits_are_the_recorded_ones(hip_lib, fx, shape):
    want = {n: d for n, d in zip(fx["case_names"].tolist(), fx["case_sha256"].tolist()) if n.startswith(M.tag(shape) + "/")}
    # 2 + 3 cfg_ddim cases, and per mode a forward, a backward and two history steps
    assert len(want) == 3 + 6 + 6 * (2 + 2 + 4) + 3
    got = M.replay(hip_lib, fx, shape)
    assert sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
