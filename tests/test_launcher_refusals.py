"""Host-side argument checks of the vectorised row kernels (status only: a refused call returns before any HIP call, so no GPU is needed).

The 8-wide bf16 kernels (add, copy, mask, sumpool2x2, maxpool, geglu_bwd) move uint4 vectors and the 4-wide fp32 ones float4: with a
channel count that is not a multiple of the vector width they would silently drop the channel tail (C >> 3 / C >> 2), with such a row
stride the 16-byte accesses would be misaligned.  maxpool3x3s2* pools to H / 2 x W / 2, which is torch's (H - 1) / 2 + 1 for even sizes
only.  All of these are hipErrorInvalidValue.  Only refused argument sets are passed here: nothing is ever launched.

The norm launchers (norm.hip) refuse, in front of any launch and of any division by G: empty or negative extents, B beyond a grid's y
extent, C that is no multiple of 8 or of G, C > 2048 for LayerNorm, any row stride that is no multiple of 8, channel partials with
HW % 64, a forward with neither y nor stats, row partials with spans < 1 or rowpart_ld < spans, a backward without stats.
"""
import pytest

INVALID = 1     # hipErrorInvalidValue

# name, argument list with null pointers, the positions whose value is made invalid one at a time (-> value)
BF16 = [
    ("dd_op_add_bf16", [None, 16, 1, 16, None, 16, 4, 16], {1: 12, 3: 12, 5: 12, 7: 12}),
    ("dd_op_copy_bf16", [None, 16, None, 16, 4, 16], {1: 12, 3: 12, 5: 12}),
    ("dd_op_mask_bf16", [None, 16, None, 16, None, 16, 4, 16], {1: 12, 3: 12, 5: 12, 7: 12}),
    ("dd_op_sumpool2x2", [None, 16, None, 16, 1, 2, 2, 16, 0], {1: 12, 3: 12, 7: 12}),
    ("dd_op_geglu_bwd", [None, 32, None, 16, None, 32, 4, 16], {1: 36, 3: 12, 5: 36, 7: 12}),
    ("dd_op_maxpool3x3s2", [None, None, 1, 4, 4, 16], {3: 5, 4: 5, 5: 12}),
    ("dd_op_maxpool3x3s2_bwd", [None, None, None, 1, 4, 4, 16], {4: 5, 5: 5, 6: 12}),
]
F32 = [
    ("dd_op_add_f32", [None, 8, 1, 8, None, 8, 4, 8], {1: 6, 3: 6, 5: 6, 7: 6}),
    ("dd_op_copy_f32", [None, 8, None, 8, 4, 8], {1: 6, 3: 6, 5: 6}),
    ("dd_op_mask_f32", [None, 8, None, 8, None, 8, 4, 8, 6.0], {1: 6, 3: 6, 5: 6, 7: 6}),
    ("dd_op_maxpool3x3s2_f32", [None, None, 1, 4, 4, 8], {3: 5, 4: 5, 5: 6}),
    ("dd_op_maxpool3x3s2_bwd_f32", [None, None, None, 1, 4, 4, 8], {4: 5, 5: 5, 6: 6}),
]


@pytest.mark.parametrize("case", BF16 + F32, ids=[c[0] for c in BF16 + F32])
def test_vector_width_and_odd_size_refusals(case):
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    name, args, bad = case
    fn = getattr(_lib.lib(), name)
    for pos, value in bad.items():
        a = list(args)
        a[pos] = value
        assert fn(*a, None) == INVALID, "%s accepted argument %d = %r" % (name, pos, value)


def test_other_arguments_are_still_checked_when_b_is_null():
    """launch_copy_* is launch_add_* with b = null: the first operand's stride, the output's and C are checked all the same (that such
    a call is ACCEPTED whatever ldb holds needs a launch: tests/test_reverse_ops_gpu.py calls dd_op_copy_* on a GPU)"""
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    L = _lib.lib()
    assert L.dd_op_add_bf16(None, 12, None, 5, None, 16, 4, 16, None) == INVALID        # lda
    assert L.dd_op_add_f32(None, 8, None, 5, None, 8, 4, 6, None) == INVALID            # C


PTR = 0x1000        # stands for a non-null pointer: every call below is refused before anything is dereferenced or launched
GN_OK = dict(x_ld=64, y_ld=64, dy_ld=64, dx_ld=64, B=1, HW=64, C=64, G=8, eps=1e-5)
GN_FWD_BAD = [dict(G=0), dict(G=-1), dict(HW=0), dict(HW=-64), dict(B=0), dict(B=-1), dict(B=65536), dict(C=60, G=4), dict(C=0), dict(G=7),
              dict(x_ld=60), dict(y_ld=60), dict(chan_part=PTR, part_ld=64, HW=100)]
GN_BWD_BAD = [dict(G=0), dict(HW=0), dict(B=0), dict(B=65536), dict(C=60, G=4), dict(G=7), dict(x_ld=60), dict(dy_ld=60), dict(dx_ld=60)]
LN_OK = dict(x_ld=64, y_ld=64, dy_ld=64, dx_ld=64, M=4, C=64, eps=1e-5, y=PTR, stats=PTR)
LN_FWD_BAD = [dict(M=0), dict(M=-1), dict(C=60), dict(C=0), dict(C=2056, x_ld=2056, y_ld=2056), dict(x_ld=60), dict(y_ld=60), dict(y=None, stats=None),
              dict(y=None, rowpart=PTR, spans=0, rowpart_ld=4), dict(y=None, rowpart=PTR, spans=4, rowpart_ld=3)]
LN_BWD_BAD = [dict(stats=None), dict(M=0), dict(C=60), dict(C=2056, x_ld=2056, dy_ld=2056, dx_ld=2056), dict(x_ld=60), dict(dy_ld=60), dict(dx_ld=60)]


def _ident(d):
    return ",".join("%s=%s" % kv for kv in d.items())


NORM_REFUSALS = [(f, s, o, b) for f, s, o, cases in (
    ("dd_op_groupnorm_fwd", "GroupNormParams", GN_OK, GN_FWD_BAD), ("dd_op_groupnorm_bwd", "GroupNormParams", GN_OK, GN_BWD_BAD),
    ("dd_op_layernorm_fwd", "LayerNormParams", LN_OK, LN_FWD_BAD), ("dd_op_layernorm_bwd", "LayerNormParams", LN_OK, LN_BWD_BAD)) for b in cases]


@pytest.mark.parametrize("fn,struct,ok,bad", NORM_REFUSALS, ids=["%s:%s" % (c[0][6:], _ident(c[3])) for c in NORM_REFUSALS])
def test_norm_launcher_refusals(fn, struct, ok, bad):
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    p = getattr(_lib, struct)()            # zero-initialised: every pointer null unless the case names it
    for k, v in dict(ok, **bad).items():
        setattr(p, k, v)
    assert getattr(_lib.lib(), fn)(C.byref(p), None) == INVALID, "%s accepted %s" % (fn, bad)
