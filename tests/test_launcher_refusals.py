"""Host-side argument checks of the vectorised row kernels (status only: a refused call returns before any HIP call, so no GPU is needed).

The 8-wide bf16 kernels (add, copy, mask, sumpool2x2, maxpool, geglu_bwd) move uint4 vectors and the 4-wide fp32 ones float4: with a
channel count that is not a multiple of the vector width they would silently drop the channel tail (C >> 3 / C >> 2), with such a row
stride the 16-byte accesses would be misaligned.  maxpool3x3s2* pools to H / 2 x W / 2, which is torch's (H - 1) / 2 + 1 for even sizes
only.  All of these are hipErrorInvalidValue.  Only refused argument sets are passed here: nothing is ever launched.
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
