"""The attention kernels (attention.hip, attention_shortk.hip, attention_gemm.hip) on exact inputs, against closed-form bits.

tests/attention_exact_ref.py: one-hot queries and per-class integer keys make every score an integer (graded family, log2 domain) or
0 / "masked" (mask family, any scale), every probability a power of two (or 1 / 0) and, with small-integer values, O l and l exact in fp32
in any order -- under any reference the lazy softmax picks, across the rescales of the online softmax, through the ring buffer, the ragged
tile's mask, the ones-column row sum at d = 40 and the e4m3 packing of the fp8 P.V.  O is compared bit for bit wherever the exact quotient
acc / l is further than 2^-18 (relative) from a rounding boundary of the stored format (the kernels multiply by a rounded reciprocal), else
either neighbour is admitted; at most 2 % of a case's elements may be of that kind.  The LSE is compared against (max + log2 l) ln 2 within
1e-5 max(1, |lse|) (never more than a tenth of what one lost key moves a flat row).  The whole output buffer is compared: the kernels write
into a column view of a wider NaN-prefilled buffer and the columns on either side must keep the prefill.  Backward cases compare dQ, dK and
dV with no tolerance at all, and the dK / dV rows of keys no query sees must be +0.

Every case first asserts the plan it is about (tests/attention_exact_cases.py; the same table is walked on the CPU).  A failure prints
attention_exact_ref.mismatch_report: how many elements, the first eight as (image, head, query, column), the query index modulo 16 and
32, whether every wrong row sees keys of a single key tile only.

Observed on the MI355X, bf16 and fp16 storage builds (the test prints the figures of every case with -s):
  * the hardware exp2 returns exact powers of two for integral arguments: no element of any case differed from the round-to-nearest-even
    of the exact quotient, the indeterminate ones included (none "took the other neighbour"), so every route is BIT-EXACT on the family
    it runs, not only exact within 2^-18: the short-key kernel, the lazy LDS-DMA kernel (optimistic and safe sweep) and the fp8 P.V on the
    graded family; the online-softmax LDS-DMA kernel, the register-staged kernel (d = 160, d = 512, causal) on both families; the GEMM
    route on the mask family with power-of-two key counts; dQ, dK, dV of the flash backward (plain and PS) and of the GEMM route.
  * largest indeterminate share (bf16 / fp16): short-key 0.06 % / 0.58 %, LDS-DMA lazy 0.14 % / 0.40 %, fp8 P.V 0 %, LDS-DMA online 0 % / 0 %,
    register-staged 0.03 % / 1.37 % (d = 512, mask family: thirds and fifths against 11 significand bits), GEMM route 0 % (power-of-two row
    sums: every quotient is exact).
  * largest LSE error: 8.6e-7 (flash kernels, 1064 and 4096 keys), 1.5e-8 (GEMM route): at most 0.034 of the tolerance.
"""

import pytest
import torch

import attention_exact_cases as T
import attention_exact_ref as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distdiff_amd import ops as o
    assert torch.cuda.is_available()
    return o


RUNS = [(i, dt) for i, c in enumerate(T.CASES) for dt in ((torch.bfloat16, torch.float16) if c.f16 else (torch.bfloat16,))]
IDS = [T.CASES[i].name + ("-fp16" if dt == torch.float16 else "") for i, dt in RUNS]


def check_plans(ops, case, dtype):
    for bwd, want in ((False, case.fwd), (True, case.bwd)):
        if want is not None:
            diff = T.plan_differences(T.plan_of(ops, case, bwd, dtype), want)
            assert not diff, "%s (%s, %s): planned / the case is about: %s" % (case.name, dtype, "backward" if bwd else "forward", diff)


def launch(ops, case, q, k, v, d_o, o):
    args = (q, k, v, case.B, case.H, case.Nq, case.Nk, case.D, case.scale)
    if case.api == "gemm":
        return ops.attention_gemm(*args, d_o=d_o, ws_images=case.ws_images, o=o)
    flags = dict(case.flags, q_prescaled=case.prescaled, o=o)
    flags["pv_fp8"] = flags.pop("fp8", False)
    if case.api == "planned":
        out, plans = ops.attention_planned(*args, d_o=d_o, need_dkv=case.need_dkv, ws_images=case.ws_images, **flags)
        for got, want in zip(plans, (case.fwd, case.bwd)):
            assert not T.plan_differences(got, want), (case.name, got, want)
        return out
    return ops.attention(*args, d_o=d_o, need_dkv=case.need_dkv, **flags)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_attention_exact(ops, run):
    i, dtype = run
    case = T.CASES[i]
    inp = X.make_inputs(case, i)
    fw = X.forward(case, inp, dtype)
    assert fw.share <= X.CAP, "%s: %.2f %% of the elements are indeterminate" % (case.name, 100 * fw.share)
    check_plans(ops, case, dtype)
    q, k, v, d_o = X.rows(case, inp, dtype, "cuda")
    c = case.H * case.D
    obuf = torch.full((case.B * case.Nq, c + 2 * T.O_PAD), float("nan"), dtype=dtype, device="cuda")
    prefill = int(X.bits(obuf)[0, 0])
    o = obuf[:, T.O_PAD:T.O_PAD + c]
    out = launch(ops, case, q, k, v, d_o, o)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == o.data_ptr()
    # ---- O: the whole buffer
    pads = torch.cat([obuf[:, :T.O_PAD], obuf[:, T.O_PAD + c:]], 1)
    assert bool((X.bits(pads) == prefill).all()), "%s: %d elements beside the H * D output columns were written" % (case.name, int((X.bits(pads) != prefill).sum()))
    got = X.bits(o)
    wrong = X.wrong_elements(got, fw)
    if bool(wrong.any()):
        want = X.expand(fw.want, fw.idx)
        pytest.fail("%s, plan %s\n%s" % (dtype, T.plan_of(ops, case, False, dtype), X.mismatch_report(case, inp, wrong, got.cpu().view(dtype), want.view(dtype))))
    other = int((got != X.expand(fw.want.cuda(), fw.idx.cuda())).sum())
    # ---- LSE
    lse_want = X.expand(fw.lse, fw.idx)
    err = (out[1].double().cpu() - lse_want).abs() / X.lse_tolerance(lse_want, case.Nk)
    print("%s (%s): indeterminate share %.4f %%, %d elements took the other neighbour, largest LSE error %.3f of its tolerance (%.2g absolute)"
          % (case.name, dtype, 100 * fw.share, other, float(err.max()), float((out[1].double().cpu() - lse_want).abs().max())))
    if not bool((err <= 1).all()):
        bad = (err > 1).nonzero()
        b, h, r = bad[0].tolist()
        pytest.fail("%s LSE: %d of %d rows beyond 1e-5 max(1, |lse|); first (image %d, head %d, query %d): got %.8g want %.8g; query index mod 16: %s"
                    % (case.name, len(bad), err.numel(), b, h, r, float(out[1][b, h, r]), float(lse_want[b, h, r]), (bad[:, 2] % 16).unique().tolist()))
    # ---- dQ, dK, dV
    if case.bwd is None:
        return
    bw = X.backward(case, inp, fw, dtype)
    dq, dk, dv = out[2:]
    assert (dk is None) == (dv is None) == (not case.need_dkv)
    for what, g_, w_, rows_are in (("dQ", dq, bw.dq, "query"), ("dK", dk, bw.dk, "key"), ("dV", dv, bw.dv, "key")):
        if g_ is not None:
            g_ = g_.cpu()
            rep = X.mismatch_report(case, inp, X.bits(g_) != X.bits(w_), g_, w_, what, rows_are)
            assert rep is None, "%s, plan %s\n%s" % (dtype, T.plan_of(ops, case, True, dtype), rep)
