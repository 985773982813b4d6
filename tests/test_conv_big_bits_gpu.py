"""The bits of conv_gemm_big_kernel (conv_gemm2.hip), pinned: every case of tests/golden/make_conv_big_bits.py replayed on this build
from the same generated inputs and compared, output by output, with the SHA-256 digests recorded in tests/golden/conv_big_bits.npz on an
MI355X from the build of commit 31f7888, before the tile description and the dispatcher were taken out of the kernel and its launchers.
tests/test_kernels_gpu.py and tests/test_reverse_ops_gpu.py compare the same kernel with torch references within a tolerance; this one
compares the build with the record, bit for bit."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_conv_big_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record(hip_lib):
    assert torch.cuda.is_available()
    rec = M.load()
    assert str(rec["parent_commit"]) == M.PARENT
    return dict(zip(rec["case_names"].tolist(), rec["case_sha256"].tolist()))


@pytest.mark.parametrize("case", M.CASES)
def test_bits_are_the_recorded_ones(hip_lib, record, case):
    from distdiff_amd import ops
    want = {n: d for n, d in record.items() if n.startswith(case + "/")}
    got = M.replay(ops, case)
    assert got and sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
