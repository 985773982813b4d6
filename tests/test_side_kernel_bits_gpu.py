"""The bits of the side kernels that serve bf16 and fp32 rows, pinned: every case of tests/golden/make_side_kernel_bits.py replayed on
this build from the stored inputs and compared, output by output, with the SHA-256 digests recorded in
tests/golden/side_kernel_bits.npz from the build that had one hand-written kernel per format (commit 34efcaf: add_kernel /
add_f32_kernel, mask_kernel / mask_f32_kernel, ... in elementwise.hip and guide_f32.hip), on an MI355X.  tests/test_reverse_ops_gpu.py
compares the same kernels with float64 references within a tolerance and holds the grid-wrapping shapes; this one compares the build
with the record, bit for bit."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_side_kernel_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(hip_lib):
    assert torch.cuda.is_available()
    return M.load()


@pytest.mark.parametrize("group", M.GROUPS)
def test_bits_are_the_recorded_ones(hip_lib, fx, group):
    want = {n: d for n, d in zip(fx["case_names"].tolist(), fx["case_sha256"].tolist()) if n.startswith(group + "/")}
    assert len(want) == M.COUNTS[group]
    got = M.replay(hip_lib, fx, group)
    assert sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
