"""Records the bits of conv_gemm_big_kernel (the general persistent implicit-GEMM kernel of conv_gemm2.hip: every tile form, both staging
paths, every store path of its epilogue) of ONE build as tests/golden/conv_big_bits.npz; tests/test_conv_big_bits_gpu.py replays the same
calls on the current build and compares.

    DD_LIB=/path/to/parent.so python tests/golden/make_conv_big_bits.py      # needs a GPU
    python tests/golden/make_conv_big_bits.py --plan                         # no GPU: only asks the launcher what each case gets

Run it on a build of the commit BEFORE a change to this kernel (PARENT below; a variant library made with DD_BUILD_OBJ / DD_BUILD_LIB and
loaded with DD_LIB), never on the code under test and never to make a failing test pass.  It runs every case twice and refuses to write
if the two runs differ.

Conventions of make_pingpong_bits.py: inputs from its closed integer formula lattice() (activations, residuals, biases and LayerNorm
means multiples of 1/16 in [-2, 2), weights and c1 multiples of 1/64 in [-1/2, 1/2), rstd multiples of 1/64 in [1/2, 3/2): exact in
bf16); every output buffer (y, the CF_STATS partials, the CF_ROWSTATS partials, the GEGLU raw stash, the fp32 split-K partial sums) is
pre-filled with NaN and hashed whole with SHA-256.  Each case first asserts through ops.conv_gemm_plan that the launcher gives it kind
"general", the intended tile form and the intended split.

Each case is the smallest shape that reaches one path of the kernel.  Two workgroup forms (4: 128 x 160, 5: 128 x 128): the batched
epilogue in its plain, CF_STATS, CF_ROWSTATS and CF_LNFOLD instantiations, ragged M (residual row clamp), the odd last tile of TN = 5,
GEGLU with / without the raw stash and with the fold, the fold refused its own instantiation (K < 192: generic epilogue), both LDS
rings wrapping (four items per workgroup against a bias ring of three and a c1 / statistics ring of two), split-K.  Eight-wave forms
(1: 128 x 256, 2: 256 x 160, 3: 256 x 128): a K loop deeper than 100 steps, a ragged last n-tile (generic epilogue beside batched tiles),
fp32 output, split-K 3 with the partial sums hashed.  3x3: stride 2 with padding taps on the fast staging path, Cin % 64 != 0 and the
fused 2x upsample on the general one, the input gradient of a stride-2 conv (shift = 1, parity = 1, packing mode 1).
ops.conv_gemm cannot set grouped weights (wgroup_rows) or bias_sel.  Grouped weights reach this kernel through the attention GEMM route:
tests/test_kernels_gpu.py::test_attention_gemm_path runs them.  Nothing in the package sets bias_sel
on a launch (only tests/test_conv_plan_table.py puts it into the planner's input); the loader keeps the line as it was."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pingpong_bits import digest, lattice, nan  # noqa: E402

PATH = os.path.join(HERE, "conv_big_bits.npz")
PARENT = "31f7888"          # the commit whose build made the record
F1, F2, F3, F4, F5 = "big_128x256", "big_256x160", "big_256x128", "big_128x160_two_workgroups", "big_128x128_two_workgroups"
SPAN = {F4: 80, F5: 64}     # CF_ROWSTATS: columns per (sum, sum^2) pair (BigForm::rowstat_span)

# pointwise cases: (name, form, ksplit, M, K, N, geglu, flags).  flags: b bias, r residual, u ReLU, s CF_STATS, w CF_ROWSTATS, l CF_LNFOLD,
# g CF_GEGLU_RAW, f fp32 output, p split-K partial sums hashed
GEMM = [
    ("f4_plain_odd_tile_ragged_m_res_relu", F4, 1, 1100, 192, 160, False, "bru"),
    ("f4_stats", F4, 1, 1152, 192, 160, False, "brs"),
    ("f4_rowstats", F4, 1, 1100, 192, 320, False, "bw"),
    ("f4_lnfold", F4, 1, 1100, 192, 320, False, "bl"),
    ("f4_lnfold_rings_wrap", F4, 1, 131072, 192, 320, False, "bl"),
    ("f4_plain_rings_wrap", F4, 1, 131072, 192, 320, False, "br"),
    ("f4_lnfold_generic_k128", F4, 1, 1100, 128, 160, False, "bl"),
    ("f5_geglu_raw", F5, 1, 1100, 192, 256, True, "bg"),
    ("f5_geglu", F5, 1, 1100, 192, 256, True, "b"),
    ("f5_geglu_lnfold", F5, 1, 1100, 192, 256, True, "bl"),
    ("f5_rowstats", F5, 1, 1100, 192, 128, False, "bw"),
    ("f1_geglu_raw_deep_k", F1, 1, 1100, 1600, 512, True, "bg"),
    ("f1_ragged_n_tile_stats", F1, 1, 1152, 128, 1032, False, "brs"),
    ("f3_f32_out", F3, 1, 1100, 1600, 128, False, "bf"),
    ("f2_101_ksteps", F2, 1, 1024, 6464, 320, False, "br"),
    ("f2_splitk3", F2, 3, 1024, 6464, 320, False, "brp"),
    ("f4_splitk2", F4, 2, 1100, 384, 160, False, "bp"),
]
# 3x3 cases: (name, form, B, stored H = W, stride, shift, parity, Cout, Cin of the forward weight, mode, flags).  mode 1 (input-gradient
# packing) maps Cout -> Cin; its stored input is the stride-2 conv's output.
CONV = [
    ("f5_3x3_stride2_fast_padding_taps_stats", F5, 2, 64, 2, 0, 0, 256, 64, 0, "bs"),
    ("f4_3x3_cin160_general_staging", F4, 2, 32, 1, 0, 0, 320, 160, 0, "b"),
    ("f5_3x3_upsample_general_staging", F5, 2, 16, 1, 1, 0, 256, 64, 0, "b"),
    ("f3_3x3_stride2_dgrad", F3, 2, 32, 1, 1, 1, 256, 64, 1, "r"),
]
CASES = [c[0] for c in GEMM] + [c[0] for c in CONV]


def replay(ops, name, plan_only=False):
    """Case `name` on the library ops uses -> {"<name>/<output>": sha256 hex} (plan_only: {} after the plan check, nothing touches a device)."""
    salt = CASES.index(name) * 16
    dev = "cpu" if plan_only else "cuda"
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    present = lambda make: True if plan_only else make()
    outs = {}
    conv = [c for c in CONV if c[0] == name]
    if conv:
        _, form, B, H, stride, shift, parity, Cout, Cin, mode, fl = conv[0]
        pk = ops.PackedConv(lattice((Cout, Cin, 3, 3), salt) / 64, 1, mode=mode, bias=lattice((Cin if mode else Cout,), salt + 1) / 16 if "b" in fl else None,
                            device=dev)
        Ho = ((H << shift) + 2 - 3) // stride + 1
        M, N, geglu, ksplit = B * Ho * Ho, pk.N, False, 1
        geom = (B, H, H, Ho, Ho)
        kw = dict(stride=stride, shift=shift, parity=parity, ksplit=1)
        x = None if plan_only else bf(lattice((B * H * H, pk.cin), salt + 2) / 16)
    else:
        _, form, ksplit, M, K, N, geglu, fl = [c for c in GEMM if c[0] == name][0]
        pk = ops.PackedConv(lattice((N, K), salt) / 64, 0, geglu=geglu, bias=lattice((N,), salt + 1) / 16, device=dev)
        geom = (1, M, 1, M, 1)
        kw = dict(ksplit=ksplit, relu="u" in fl, out_f32="f" in fl)
        x = None if plan_only else bf(lattice((M, K), salt + 2) / 16)
    ncols = N // 2 if geglu else N
    y = None
    if not plan_only:
        y = outs["y"] = nan((M, ncols), torch.float32 if "f" in fl else torch.bfloat16)
    if "r" in fl:
        kw["res"] = present(lambda: bf(lattice((M, N), salt + 3) / 16))
    if "s" in fl:
        kw["stats"] = present(lambda: outs.setdefault("stats", nan((M // 64, N, 2), torch.float32)))
    if "w" in fl:
        kw["rowpart"] = torch.empty((M, N // SPAN[form], 2)) if plan_only else outs.setdefault("rowpart", nan((M, N // SPAN[form], 2), torch.float32))
    if "l" in fl:
        kw["ln_stats"] = present(lambda: torch.stack((lattice((M,), salt + 4) / 16, lattice((M,), salt + 5) / 64 + 1.0), dim=1).contiguous().to(dev))
        if not plan_only:
            kw["ln_c1"] = (lattice((N,), salt + 6) / 64).to(dev)
    if "g" in fl:
        kw["raw"] = torch.empty((M, N), dtype=torch.bfloat16) if plan_only else outs.setdefault("raw", nan((M, N)))
    if "p" in fl and not plan_only:
        kw["partial"] = outs["partial"] = nan((16 * M * N,), torch.float32)
    plan = ops.conv_gemm_plan(x, pk, *geom, y=y, **kw)
    assert plan == ("general", form, ksplit), "%s: the launcher plans %s, the case is about %s" % (name, plan, ("general", form, ksplit))
    if plan_only:
        return {}
    ops.conv_gemm(x, pk, *geom, y=y, **kw)
    torch.cuda.synchronize()
    return {"%s/%s" % (name, k): digest(v) for k, v in outs.items()}


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from distdiff_amd import _lib, ops
    if "--plan" in sys.argv:
        for name in CASES:
            replay(ops, name, plan_only=True)
            print("ok", name)
        return
    got = {}
    for name in CASES:
        first = replay(ops, name)
        assert replay(ops, name) == first, "the build is not deterministic on %s" % name
        got.update(first)
        print(name, len(first), flush=True)
    names = sorted(got)
    np.savez_compressed(PATH, parent_commit=np.array(PARENT), case_names=np.array(names), case_sha256=np.array([got[n] for n in names]))
    print("wrote %s: %d outputs, %d bytes, library %s" % (PATH, len(names), os.path.getsize(PATH), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
