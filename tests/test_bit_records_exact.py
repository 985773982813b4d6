"""The bit records of the conv / GEMM kernels (tests/golden/conv_big_bits.npz, pingpong_bits.npz) against a closed form, on the CPU.

The records pin what a parent build wrote on lattice() inputs.  Those inputs make every product and every partial sum exact in fp32
(tests/exact_ref.py), so wherever the epilogue is a chain of exact operations and one rounding, the recorded bits can be derived without
a device: a plain fp32 conv / matmul, bias, residual, ReLU, one RNE rounding, hashed.  This test does that for every recorded output that
has such a closed form and asserts the recorded SHA-256; it turns "what a build did" into "what is right", and it validates the reference
that tests/test_conv_exact_gpu.py compares the kernels with.  Every other recorded output is named in NO_CLOSED_FORM with the reason, and
the list is asserted whole: a recorded output that is neither checked nor listed fails.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import exact_ref as X  # noqa: E402
from conv_exact_cases import closed_form_outputs, record_problems  # noqa: E402
import make_conv_big_bits as big  # noqa: E402
import make_pingpong_bits as pp  # noqa: E402

ORDER = "depends on the order of summation or holds quantities fp32 does not represent exactly"
ACT = "depends on rstd / GELU"
# outputs of the two records without a closed form ON THE RECORDS' INPUTS: {"record:case/output": reason}.  The reason is the lattice, not
# the outputs: sums of squares of multiples of 1 / 1024 are not exact in fp32, and the (mean, rstd) rows of the recorded folds are those
# of the lattice rows, so their products are rounded.  On ternary inputs with synthetic (mean, rstd) the same outputs (partials, row
# partials, the folded and the GEGLU y) are compared bit for bit by tests/test_conv_exact_gpu.py::test_conv_gemm_stat_outputs_exact;
# the split-K partial buffers stay what they are, scratch whose layout is the kernel's own.
NO_CLOSED_FORM = {
    "big:f4_stats/stats": ORDER, "big:f1_ragged_n_tile_stats/stats": ORDER, "big:f5_3x3_stride2_fast_padding_taps_stats/stats": ORDER,
    "big:f4_rowstats/rowpart": ORDER, "big:f5_rowstats/rowpart": ORDER,
    "big:f2_splitk3/partial": ORDER, "big:f4_splitk2/partial": ORDER,
    "big:f4_lnfold/y": ACT, "big:f4_lnfold_rings_wrap/y": ACT, "big:f4_lnfold_generic_k128/y": ACT,
    "big:f5_geglu_raw/y": ACT, "big:f5_geglu/y": ACT, "big:f5_geglu_lnfold/y": ACT, "big:f1_geglu_raw_deep_k/y": ACT,
    "pp:halo_5_2_three_tiles_per_row_res_stats/stats": ORDER, "pp:persist_two_tiles_per_workgroup_res_stats/stats": ORDER,
    "pp:halo_4_4_res_stats/stats": ORDER, "pp:pps_5_stats/stats": ORDER, "pp:pps_5_rowstats/rowpart": ORDER,
    "pp:halo_5_4_multi_image_chunk_split/partial": ORDER,
    "pp:pps_5_lnfold/y": ACT, "pp:pps_4_geglu_raw/y": ACT, "pp:pps_4_geglu_lnfold/y": ACT,
}


def recorded():
    rec = {}
    for tag, mod in (("big", big), ("pp", pp)):
        t = mod.load()
        rec.update({"%s:%s" % (tag, n): str(h) for n, h in zip(t["case_names"].tolist(), t["case_sha256"].tolist())})
    return rec


def test_recorded_outputs_equal_the_closed_form():
    rec = recorded()
    checked, wrong = [], []
    for key, (prob, salt, _span, _plan) in record_problems().items():
        outs = closed_form_outputs(prob)
        if not outs:
            continue
        inp = X.make_inputs(prob, "lattice", salt)
        assert (inp["dx"], inp["dw"]) == (16, 64), key              # the record's own scaling
        X.check_conditions(prob, inp, "lattice")
        want = X.expected(prob, inp)
        name = "%s/%s" % (key, outs[0])
        checked.append(name)
        if X.digest(want) != rec[name]:
            wrong.append(name)
    assert not wrong, "the closed form does not give the recorded bits of: %s" % wrong
    print("%d recorded outputs verified against the closed form" % len(checked))
    assert len(checked) >= 31, len(checked)
    assert set(checked) | set(NO_CLOSED_FORM) == set(rec) and not set(checked) & set(NO_CLOSED_FORM), \
        (sorted(set(rec) - set(checked) - set(NO_CLOSED_FORM)), sorted((set(checked) | set(NO_CLOSED_FORM)) - set(rec)))


def test_skip_list_is_what_has_no_closed_form():
    probs = record_problems()
    rec = recorded()
    want = {}
    for name in rec:
        key, out = name.rsplit("/", 1)
        prob = probs[key][0]
        if out in closed_form_outputs(prob):
            continue
        want[name] = ACT if out == "y" else ORDER
    assert want == NO_CLOSED_FORM
