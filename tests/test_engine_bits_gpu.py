"""The bits of every engine entry point that runs a program, pinned: every engine of tests/golden/make_engine_bits.py replayed on this build
and compared with tests/golden/engine_bits.npz, recorded from the build in which run_fwd / run_bwd were two switch statements and the
gradient fan-out was written at every site.  The engines are the smallest that run every op kind and both reverse paths; each takes seconds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_engine_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_record_holds_every_engine():
    rec = M.load()
    for kind, act in M.ENGINES:
        names = {k.split("/", 2)[2] for k in rec if k.startswith("%s/%s/" % (act, kind))}
        # 13 outputs of the guided, plain and VJP calls and decode, 9 of the three expands, and the encoders where the engine has them
        assert len(names) == 13 + 9 + {"tiny": 3, "tiny_sdxl": 5}.get(kind, 0), (kind, act, sorted(names))
    assert len(rec) == 2 * (4 * 22 + 3 + 5)


@pytest.mark.parametrize("kind,act", M.ENGINES, ids=["%s-%s" % e for e in M.ENGINES])
def test_bits_are_the_recorded_ones(hip_lib, kind, act):
    assert torch.cuda.is_available()
    rec = M.load()
    want = {k: v for k, v in rec.items() if k.startswith("%s/%s/" % (act, kind))}
    got = M.replay(kind, act)
    assert sorted(got) == sorted(want)
    differ = [n for n in sorted(want) if not np.array_equal(got[n], want[n])]
    assert not differ, "%d of %d outputs differ from the recorded bits: %s" % (len(differ), len(want), ", ".join(differ))
