"""The bits of the flash attention kernels (attn_fwd_kernel, attn_fwd_dma_kernel, attn_fwd_shortk_kernel, attn_delta_kernel,
attn_bwd_dq_kernel, attn_bwd_dkv_kernel), pinned: every case of tests/golden/make_attention_bits.py replayed on this build, on the bf16
and on the fp16 library, from the same generated inputs and compared, output by output (O, LSE, dQ, dK, dV: NaN-prefilled buffers with 8
padding columns per row, hashed whole), with the SHA-256 digests recorded in tests/golden/attention_bits.npz on an MI355X from the build
in which each kernel still spelled its tile staging, softmax and row epilogue by hand (commit 51fd84f).  tests/test_kernels_gpu.py and
tests/test_act_f16_ops_gpu.py compare the same kernels with torch references within a tolerance; this one compares the build with the
record, bit for bit.

Not covered: the non-causal instantiations of attn_fwd_kernel at d <= 80.  The planner sends a non-causal problem of those head dims there
only when its K / V rows exceed the 32-bit offsets of the LDS-DMA loads, which needs more than 3.7 GB; they are the same template as the
causal cases (stream_causal_d64, stream_causal_d40), whose full-tile loop they add."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_attention_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record(hip_lib):
    assert torch.cuda.is_available()
    rec = M.load()
    assert str(rec["parent_commit"]) == M.PARENT
    return dict(zip(rec["case_names"].tolist(), rec["case_sha256"].tolist()))


@pytest.mark.parametrize("lib", M.LIBS)            # the library varies fastest: both replay a case from one generated set of inputs
@pytest.mark.parametrize("case", M.NAMES)
def test_bits_are_the_recorded_ones(hip_lib, record, lib, case):
    from distdiff_amd import ops
    if case not in M.cases_of(lib):
        with pytest.raises(RuntimeError):                      # the fp16 library has no fp8 P.V form: its planner refuses
            M.replay(ops, case, lib, plan_only=True)
        return
    want = {n: d for n, d in record.items() if n.startswith("%s/%s/" % (lib, case))}
    got = M.replay(ops, case, lib)
    assert got and sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if got[n] != want[n]]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
