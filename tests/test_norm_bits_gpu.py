"""The bits of the norm kernels (norm.hip: GroupNorm(+SiLU) in its three passes and from channel partials, LayerNorm forward, statistics-only
forward, backward and row-partial finalize), pinned: every case of tests/golden/make_norm_bits.py replayed on this build, on the bf16 and
on the fp16 library, from the same generated inputs and compared, output by output (y, statistics, dx, dx accumulated on a previous
gradient: NaN-prefilled buffers wider than the views the kernels write, hashed whole), with the SHA-256 digests recorded in
tests/golden/norm_bits.npz on an MI355X from the build in which LayerNorm still had two forward kernels and the GroupNorm passes each
spelled their row walk and backward element by hand (commit 6266c73).  The input digests are compared first: a generator that differs
reads as "inputs differ", not as a kernel change.  tests/test_norm_gpu.py compares the same kernels with float64 within per-element
bounds; this one compares the build with the record, bit for bit."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_norm_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record(hip_lib):
    assert torch.cuda.is_available()
    rec = M.load()
    assert str(rec["parent_commit"]) == M.PARENT
    return dict(zip(rec["case_names"].tolist(), rec["case_sha256"].tolist())), dict(zip(rec["input_names"].tolist(), rec["input_sha256"].tolist()))


@pytest.mark.parametrize("lib", M.LIBS)            # the library varies fastest: both replay a case from one generated set of inputs
@pytest.mark.parametrize("case", M.NAMES)
def test_bits_are_the_recorded_ones(hip_lib, record, lib, case):
    from distdiff_amd import ops
    outs, ins = record
    have = M.input_digests(case)
    assert have and sorted(have) == sorted(n for n in ins if n.startswith(case + "/"))
    differ = [n for n in sorted(have) if have[n] != ins[n]]
    assert not differ, "inputs differ from the recorded ones (the generator, not a kernel): %s" % ", ".join(differ)
    want = {n: d for n, d in outs.items() if n.startswith("%s/%s/" % (lib, case))}
    got = M.replay(ops, case, lib)
    assert got and sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
