"""The exact-input attention cases (tests/attention_exact_cases.py) on the CPU: what the launcher plans for every case, what the table
covers, the exactness conditions the closed form rests on, and what the exact comparison sees that the tolerance tests do not.

dd_op_attention_plan tests pointers for null and reads no device, so routing drift of the cases of tests/test_attention_exact_gpu.py
fails here, without a GPU, for both libraries.  Coverage: every distinct (route, d, qt, kt, dsplit, ktw, qtl, waves, bits) the fwd_engine
and bwd_engine blocks of tests/attention_plan_cases.py produce is the plan of at least one exact case, or is named in SKIP with its reason.

Sensitivity: five mutants of the reference (tests/attention_exact_ref.py: one key dropped, the ragged tile unmasked, the next head's V,
no rescale after tile 0, the row sum rounded to 16 bits) must change DETERMINATE elements of every case they apply to; the dropped key
stays inside the limits of tests/test_kernels_gpu.py::assert_close on the Gaussian inputs of test_attention_4096_keys_peaky_logits (the
numbers are printed).
"""
import math

import pytest
import torch

import attention_exact_cases as T
import attention_exact_ref as X
import attention_plan_cases as A

# engine plans no exact case runs: {(route, d, qt, kt, dsplit, ktw, qtl, waves, bits): reason}
SKIP = {}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import ops as o
    return o


_REF = {}


def ref_of(i, dtype=torch.bfloat16):
    """(inputs, Forward) of case i: computed once, shared and never changed"""
    if (i, dtype) not in _REF:
        case = T.CASES[i]
        inp = X.make_inputs(case, i)
        _REF[i, dtype] = inp, X.forward(case, inp, dtype)
    return _REF[i, dtype]


def dtypes_of(case):
    return (torch.bfloat16, torch.float16) if case.f16 else (torch.bfloat16,)


def test_case_names_are_unique():
    assert len(set(T.NAMES)) == len(T.NAMES)


def test_every_case_plans_as_stated(ops):
    bad = []
    for case in T.CASES:
        for dtype in dtypes_of(case):
            for bwd, want in ((False, case.fwd), (True, case.bwd)):
                if want is not None:
                    diff = T.plan_differences(T.plan_of(ops, case, bwd, dtype), want)
                    if diff:
                        bad.append("%s (%s, %s): planned / the case is about: %s" % (case.name, dtype, "backward" if bwd else "forward", diff))
    assert not bad, "\n".join(bad)


def test_table_covers_every_plan_of_the_engine(ops):
    from distdiff_amd import _lib
    need = {}
    for name, rows in A.blocks():
        if name in ("fwd_engine", "bwd_engine"):
            out = A.evaluate(_lib.LIB_PATH, rows)
            assert (out[:, 0] >= 0).all(), name
            for i, o in enumerate(out):
                need.setdefault(tuple(int(x) for x in o[:9]), A.describe(rows, i))
    assert len(need) >= 20, sorted(need)
    have = set()
    for case in T.CASES:
        have.add(T.plan_tuple(T.plan_of(ops, case)))
        if case.bwd is not None:
            have.add(T.plan_tuple(T.plan_of(ops, case, True)))
    left = {k: v for k, v in need.items() if k not in have}
    assert set(left) == set(SKIP), "engine plans no exact case runs, against the skip list %s:\n%s" % (sorted(SKIP), "\n".join("%s  %s" % kv for kv in sorted(left.items())))


def test_table_covers_the_stated_edges():
    fwd = [c for c in T.CASES if c.bwd is None]
    assert {c.Nk for c in T.CASES} >= {1, 13, 16, 64, 65, 77, 80, 81, 130, 200, 1064, 4096}
    assert any((c.Nq, c.Nk, c.D) == (512, 4096, 40) and c.fwd["route"] == "dma" for c in fwd)
    assert {c.Nq for c in T.CASES} >= {50, 77, 200, 300, 256, 512}
    assert {c.D for c in T.CASES} == {32, 40, 64, 80, 160, 256, 512}
    assert {c.Nk for c in T.CASES if c.causal} == {77, 130}
    for flag in ("prescaled", "fp8", "no_shortk", "wide"):
        assert any(getattr(c, flag) for c in fwd), flag
    assert {(c.ws_images, c.fwd["group"]) for c in fwd if c.api == "gemm"} >= {(1, 2), (2, 5), (8, 8)}
    assert any(c.B == 5 and c.fwd["group"] == 2 for c in fwd)
    # (the short-key grid is ((B * workgroups per (image, head) + 7) & ~7) * H)
    wgs = lambda c: min(w for w in range(1, 129) if ((c.B * w + 7) & ~7) * c.H == c.fwd["grid"])
    tiles_per_wave = {c.Nq // 32 // (wgs(c) * c.fwd["waves"]) for c in T.CASES if c.fwd["route"] == "shortk" and "grid" in c.fwd}
    assert tiles_per_wave >= {1, 4, 8}, tiles_per_wave
    # backward: plain and PS, ragged last tile, need_dkv off, the GEMM route at D = 256 with an explicit power-of-two scale
    bwd = [c for c in T.CASES if c.bwd is not None]
    assert {c.bwd["prescaled"] for c in bwd if c.bwd["route"] == "flash_bwd"} == {True, False}
    assert any(c.Nk % c.kt for c in bwd) and any(not c.need_dkv for c in bwd)
    assert all((c.D, c.scale) == (256, 2.0 ** -4) for c in bwd if c.bwd["route"] == "gemm") and any(c.bwd["route"] == "gemm" for c in bwd)
    assert all(c.bwd is None for c in T.CASES if c.D == 512 and c.fwd["route"] == "gemm")      # 1 / sqrt(512): forward only


def test_fp16_library_runs_every_route_once():
    routes = lambda cs: {c.fwd["route"] + ("_lazy" if c.fwd["lazy"] else "") for c in cs} | {c.bwd["route"] + "_bwd" for c in cs if c.bwd is not None}
    assert routes([c for c in T.CASES if c.f16]) == routes([c for c in T.CASES if not c.fp8])      # (the fp16 build has no fp8 P.V)


def test_exactness_conditions_and_caps():
    """forward() and backward() assert the conditions; here also the cap on the indeterminate share, per case and storage format"""
    worst = {}
    for i, case in enumerate(T.CASES):
        for dtype in dtypes_of(case):
            inp, fw = ref_of(i, dtype)
            assert fw.share <= X.CAP, "%s (%s): %.2f %% of the elements are indeterminate" % (case.name, dtype, 100 * fw.share)
            worst[case.fwd["route"]] = max(worst.get(case.fwd["route"], 0.0), fw.share)
            if case.family == "mask":
                assert inp["a"] * inp["b"] * case.scale >= 256 and bool((fw.m == 0).all())
            if case.bwd is not None:
                bw = X.backward(case, inp, fw, dtype)
                assert int(bw.unseen.sum()) > 0, case.name
                if case.need_dkv:
                    rows = bw.unseen.permute(0, 2, 1)[..., None].expand(-1, -1, -1, case.D).reshape(case.B * case.Nk, -1)
                    assert not bool(X.bits(bw.dk)[rows].any()) and not bool(X.bits(bw.dv)[rows].any())          # +0, not -0
            elif case.fwd["route"] != "gemm" and case.Nq >= case.C and not case.causal:
                assert bool(inp["vis"].any(-1).all()), "%s: a key no query row sees" % case.name
    print("largest indeterminate share per route: %s" % {k: "%.3f %%" % (100 * v) for k, v in worst.items()})


def test_gemm_cases_see_power_of_two_key_counts():
    for i, case in enumerate(T.CASES):
        if case.fwd["route"] == "gemm":
            assert bool(X.is_pow2(ref_of(i)[1].l).all()), case.name


def test_sweeps_of_the_lazy_kernel():
    """one case the optimistic sweep alone carries, one that needs the safe sweep (attention.hip: a row sum at or beyond 2^64)"""
    i = T.NAMES.index("dma_d64_pre_k200_optimistic_sweep_suffices")
    assert not bool(X.needs_safe_sweep(T.CASES[i], ref_of(i)[0]).any())
    i = T.NAMES.index("dma_d80_pre_q77_k1064_needs_safe_sweep")
    case, (inp, fw) = T.CASES[i], ref_of(i)
    need = torch.gather(X.needs_safe_sweep(case, inp), 2, fw.idx)                   # per query row
    assert bool(need.any(-1).all()), "a workgroup of some (image, head) stays on the optimistic sweep"
    assert not bool(need.all()), "no row is left that the optimistic sweep would have carried"
    # rows whose maximum rises with every tile (the riser classes): the online softmax rescales in each of the first tiles
    i = T.NAMES.index("dma_d40_w8_ln2_q256_k200")
    case, (inp, _fw) = T.CASES[i], ref_of(i)
    s, _idx = X.scores(case, inp)
    run = torch.cummax(torch.stack([c.max(-1).values for c in s.split(case.kt, -1)], -1), -1).values
    assert bool((run[:, :, 0, 1:] > run[:, :, 0, :-1]).all())


def test_lse_tolerance_sees_one_missing_key():
    """at least 10 x below log(Nk / (Nk - 1)) of the largest case, whatever the row's LSE"""
    big = max(T.CASES, key=lambda c: c.Nk)
    assert big.Nk == 4096
    _inp, fw = ref_of(T.CASES.index(big))
    assert float(X.lse_tolerance(fw.lse, big.Nk).max()) * 10 <= math.log(big.Nk / (big.Nk - 1.0))
    assert X.lse_tolerance(torch.tensor([0.5, 16.0], dtype=torch.float64), 77).tolist() == pytest.approx([1e-5, 16e-5], rel=1e-12)


def _seen(fw, fm):
    """the GPU test's comparison on the mutant's bits: elements wrong AND determinate"""
    return (fm.want != fw.want) & (fm.want != fw.alt) & ~fw.ind


def test_mutants_of_the_reference_show_on_every_case():
    quiet, applied = [], {name: 0 for name, _fn in X.MUTANTS}
    for i, case in enumerate(T.CASES):
        inp, fw = ref_of(i)
        for name, fn in X.MUTANTS:
            fm = X.forward(case, inp, mutant=fn)
            if fm is None:
                continue
            applied[name] += 1
            if not bool(_seen(fw, fm).any()):
                quiet.append((case.name, name))
    print("mutants applied (cases): %s" % applied)
    assert not quiet, "mutants the exact comparison did not see: %s" % quiet
    assert applied["dropped_key"] == len(T.CASES) - 1 and applied["next_heads_v"] >= len(T.CASES) - 2 and min(applied.values()) >= 8, applied


def test_mismatch_report_names_the_place():
    i = T.NAMES.index("dma_d40_w4_pre_q300_k130")
    case, (inp, fw) = T.CASES[i], ref_of(i)
    want = X.expand(fw.want, fw.idx)
    assert X.mismatch_report(case, inp, X.wrong_elements(want, fw)) is None
    fm = X.forward(case, inp, mutant=X.mutant_unmasked_ragged_tile)
    got = X.expand(fm.want, fm.idx)
    rep = X.mismatch_report(case, inp, X.wrong_elements(got, fw), got.view(torch.bfloat16), want.view(torch.bfloat16))
    print(rep)
    assert "elements differ" in rep and "(image 0, head 0, query " in rep and "mod 16" in rep and "mod 32" in rep and "single key tile only: False" in rep
    # a fault of the last tile alone: the rows that see nothing but that tile
    cls = torch.gather(inp["vis"][:, :, :128].any(2), 2, inp["g"])                      # rows that see a key of the first two tiles
    only_last = (~cls).permute(0, 2, 1)[..., None].expand(-1, -1, -1, case.D).reshape(got.shape)
    rep = X.mismatch_report(case, inp, X.wrong_elements(torch.where(only_last, got, want), fw))
    assert "single key tile only: True" in rep and "/ [2]" in rep, rep


def test_dropped_key_passes_the_tolerance_test_at_4096_keys():
    """The Gaussian inputs of tests/test_kernels_gpu.py::test_attention_4096_keys_peaky_logits (d = 40, the first 256 of its 4096
    queries), one key lost: the largest O and LSE errors against that test's limits, for 16 keys; and the same fault on the exact 4096-key
    case."""
    B, Nq, Nk, H, D = 1, 4096, 4096, 8, 40
    g = torch.Generator().manual_seed(41)
    bf = lambda t: t.to(torch.bfloat16).float()
    q = bf(torch.randn(B, Nq, H, D, generator=g) * 2.0)
    k = bf(torch.randn(B, Nk, H, D, generator=g) * 2.0)
    u = torch.randn(H, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    a = math.sqrt(12.0 * math.sqrt(D))
    q = bf(q + a * u)[:, :256]
    k = bf(k + (torch.linspace(0, 1, Nk)[None, :, None, None] * a) * u)
    v = bf(torch.randn(B, Nk, H, D, generator=g))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D)
    ref, lse = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v), torch.logsumexp(s, -1)
    lim_o, lim_l = 2e-3 + 2e-2 * float(ref.abs().max()), 2e-3 + 1e-3 * float(lse.abs().max())
    noise = float((bf(ref) - ref).abs().max())
    errs = []
    for j in range(0, Nk, 256):
        sm = s.clone()
        sm[..., j] = -math.inf
        errs.append((float((bf(torch.einsum("bhqk,bkhd->bqhd", sm.softmax(-1), v)) - ref).abs().max()), float((torch.logsumexp(sm, -1) - lse).abs().max())))
    inside = sum(eo <= lim_o and el <= lim_l for eo, el in errs)
    i = T.NAMES.index("dma_d40_w8_pre_q512_k4096_ring")
    case, (inp, fw) = T.CASES[i], ref_of(i)
    fm = X.forward(case, inp, mutant=X.mutant_dropped_key)
    wrong = int(torch.gather(_seen(fw, fm).sum(-1), 2, fw.idx).sum())
    lse_moved = int((torch.gather((fm.lse - fw.lse).abs() > X.lse_tolerance(fw.lse, case.Nk), 2, fw.idx)).sum())
    print("4096 keys, one key lost: assert_close limits O %.4f LSE %.4f; the right result's own bf16 rounding %.4f; largest O error %.5f .. %.4f, "
          "LSE error %.2g .. %.2g over 16 keys, %d of them inside both limits; exact comparison on the 4096-key case: %d determinate O elements "
          "wrong, %d of %d LSE rows beyond their tolerance" % (lim_o, lim_l, noise, min(e[0] for e in errs), max(e[0] for e in errs), min(e[1] for e in errs),
                                                               max(e[1] for e in errs), inside, wrong, lse_moved, fw.idx.numel()))
    assert inside >= 1, "no dropped key passes the tolerance test any more: %r" % (errs,)
    assert wrong > 1000 and lse_moved > 0
