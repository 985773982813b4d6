"""Records the bits of the three ping-pong kernels (conv_halo_kernel, conv_halo_persist_kernel, gemm_pps_kernel: every instantiation, every
epilogue and everything their shared K loop varies in) of ONE build as tests/golden/pingpong_bits.npz; tests/test_pingpong_bits_gpu.py
replays the same calls on the current build and compares.

    DD_LIB=/path/to/parent.so python tests/golden/make_pingpong_bits.py      # needs a GPU
    python tests/golden/make_pingpong_bits.py --plan                         # no GPU: only asks the launcher which kernel each case gets

Run it on a build of the commit BEFORE a change to these kernels (PARENT below; a variant library made with DD_BUILD_OBJ / DD_BUILD_LIB
and loaded with DD_LIB), never on the code under test and never to make a failing test pass.  It runs every case twice and refuses to
write if the two runs differ.

The inputs are too large to store, so they come from a closed integer formula (lattice(): uint32 arithmetic on the element index and a
per-tensor constant, no library generator): activations, residuals, biases and LayerNorm means are multiples of 1/16 in [-2, 2), weights
and c1 multiples of 1/64 in [-1/2, 1/2), rstd multiples of 1/64 in [1/2, 3/2) -- all exact in bf16.  The file holds the case names and,
per output buffer, the SHA-256 of its raw bytes.  Every output buffer (y, the CF_STATS partials, the CF_ROWSTATS partials, the GEGLU raw
stash, the fp32 split-K partial sums of the 8 x 8 form) is pre-filled with NaN and hashed whole, so an element that is not written, or
one written outside the N columns, shows.  Each case first asserts (ops.conv_gemm_kind) that the launcher sends it to the intended kernel;
the tile form named in a case is what conv_halo_plan / launch_conv_halo give for its N.

Shapes: the smallest that still reach each instantiation (>= 192 tiles wherever the planner asks for most of the chip) and each path of
the shared loop: more tiles than workgroups (persistent walks of two tiles), an odd number of K-steps per tile (the weight-stage parity
flips between tiles), two chunks (one halo refill), nine chunks (not persistent), the fused 2x upsample, the input-gradient packing, three
tiles per image row (halo_stats_block), multi-image tiles with the chunk split, the narrow outputs, every GEMM epilogue flag.
The input-gradient packing of 160 -> 128 channels (64 x 64, 24 images) does not reach a halo kernel: its 160 input channels are not whole
64-channel chunks and the launcher sends it to the general kernel.  The two nearest shapes that do stand in for it: 128 -> 128 (N = 128 at
two chunks: conv_halo_persist_kernel) and 128 -> 160 (conv_halo_kernel<5, 2>)."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "pingpong_bits.npz")
PARENT = "bc98f8a"          # the commit whose build made the record
HALO, PERSIST, PPS = 1, 2, 4      # ops.CONV_GEMM_KINDS

# 3x3 cases: (name, kind, B, stored H = W, shift, Cout, Cin of the forward weight, mode, flags).  mode 1 (input-gradient packing) maps Cout -> Cin.
# flags: b bias, r residual, s CF_STATS, u ReLU, f fp32 output into 8-wide rows, n bf16 output into 8-wide rows, p split-K partial sums hashed
CONV = [
    ("halo_5_2_three_tiles_per_row_res_stats", HALO, 11, 96, 0, 160, 128, 0, "brs"),
    ("halo_5_2_upsample", HALO, 24, 32, 1, 160, 128, 0, "b"),
    ("halo_5_2_dgrad_128_to_160", HALO, 24, 64, 0, 128, 160, 1, ""),
    ("persist_dgrad_128_to_128", PERSIST, 24, 64, 0, 128, 128, 1, ""),
    ("persist_two_tiles_per_workgroup_res_stats", PERSIST, 20, 64, 0, 256, 128, 0, "brs"),
    ("persist_9_ksteps_stage_parity_flips", PERSIST, 20, 64, 0, 256, 64, 0, "b"),
    ("persist_upsample", PERSIST, 20, 32, 1, 256, 128, 0, "b"),
    ("halo_4_2_one_tile_9_chunks", HALO, 24, 64, 0, 128, 576, 0, "b"),
    ("halo_5_4_relu", HALO, 192, 16, 0, 320, 128, 0, "bu"),
    ("halo_4_4_res_stats", HALO, 192, 16, 0, 256, 128, 0, "brs"),
    ("halo_5_4_multi_image_chunk_split", HALO, 8, 8, 0, 320, 256, 0, "bp"),
    ("halo_narrow_n4_f32", HALO, 6, 128, 0, 4, 128, 0, "bf"),
    ("halo_narrow_n3_bf16", HALO, 6, 128, 0, 3, 64, 0, "bn"),
]
# pointwise cases: (name, M, K, N, geglu, flags).  flags: b bias, r residual, s CF_STATS, w CF_ROWSTATS, l CF_LNFOLD, g CF_GEGLU_RAW
GEMM = [
    ("pps_5_res", 40960, 256, 640, False, "br"),
    ("pps_5_stats", 40960, 256, 640, False, "bs"),
    ("pps_5_rowstats", 40960, 256, 640, False, "bw"),
    ("pps_5_lnfold", 40960, 256, 640, False, "bl"),
    ("pps_4_geglu_raw", 40960, 256, 512, True, "bg"),
    ("pps_4_geglu_lnfold", 40960, 256, 512, True, "bl"),
]
CASES = [c[0] for c in CONV] + [c[0] for c in GEMM]


def lattice(shape, salt):
    """integers in [-32, 32) from the element index and `salt`"""
    h = np.arange(int(np.prod(shape)), dtype=np.uint32) * np.uint32(2654435761) + np.uint32((salt * 40503 + 977) & 0xffffffff)
    h ^= h >> np.uint32(15)
    h *= np.uint32(2246822519)
    h ^= h >> np.uint32(13)
    return torch.from_numpy((((h >> np.uint32(7)) & np.uint32(63)).astype(np.int32) - 32).astype(np.float32).reshape(shape))


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def nan(shape, dt=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dt, device="cuda")


def replay(ops, name, plan_only=False):
    """Case `name` on the library ops uses -> {"<name>/<output>": sha256 hex} (plan_only: {} after the kind check, nothing touches a device)."""
    salt = CASES.index(name) * 16
    dev = "cpu" if plan_only else "cuda"
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    outs = {}
    conv = [c for c in CONV if c[0] == name]
    if conv:
        _, kind, B, H, shift, Cout, Cin, mode, fl = conv[0]
        pk = ops.PackedConv(lattice((Cout, Cin, 3, 3), salt) / 64, 1, mode=mode, bias=lattice((Cout,), salt + 1) / 16 if "b" in fl else None, device=dev)
        Ho = H << shift
        M, N = B * Ho * Ho, pk.N
        geom = (B, H, H, Ho, Ho)
        kw = dict(shift=shift, relu="u" in fl, out_f32="f" in fl)
        if "f" in fl or "n" in fl:
            kw["ksplit"] = 1
        if plan_only:
            x, y = None, None
            kw.update(res=True if "r" in fl else None, stats=True if "s" in fl else None)
        else:
            x = bf(lattice((B * H * H, pk.cin), salt + 2) / 16)
            outs["y"] = nan((M, 8 if ("f" in fl or "n" in fl) else N), torch.float32 if "f" in fl else torch.bfloat16)
            y = outs["y"][:, :N]
            part = nan((16 * M * N,), torch.float32) if "p" in fl else torch.empty(1 << 20, dtype=torch.float32, device="cuda")
            if "p" in fl:
                outs["partial"] = part
            if "s" in fl:
                outs["stats"] = nan((M // 64, N, 2), torch.float32)
            kw.update(res=bf(lattice((M, N), salt + 3) / 16) if "r" in fl else None, stats=outs.get("stats"), partial=part)
    else:
        _, M, K, N, geglu, fl = [c for c in GEMM if c[0] == name][0]
        kind = PPS
        pk = ops.PackedConv(lattice((N, K), salt) / 64, 0, geglu=geglu, bias=lattice((N,), salt + 1) / 16, device=dev)
        geom = (1, M, 1, M, 1)
        kw = dict(ksplit=1)
        ncols = N // 2 if geglu else N
        if plan_only:
            x, y = None, None
            kw.update(res=True if "r" in fl else None, stats=True if "s" in fl else None, rowpart=True if "w" in fl else None,
                      ln_stats=True if "l" in fl else None)
            if "g" in fl:
                kw["raw"] = torch.empty((M, N), dtype=torch.bfloat16)
        else:
            x = bf(lattice((M, K), salt + 2) / 16)
            y = outs["y"] = nan((M, ncols))
            if "r" in fl:
                kw["res"] = bf(lattice((M, N), salt + 3) / 16)
            if "s" in fl:
                kw["stats"] = outs["stats"] = nan((M // 64, N, 2), torch.float32)
            if "w" in fl:
                kw["rowpart"] = outs["rowpart"] = nan((M, N // 40, 2), torch.float32)
            if "l" in fl:
                ln = torch.stack((lattice((M,), salt + 4) / 16, lattice((M,), salt + 5) / 64 + 1.0), dim=1)
                kw.update(ln_stats=ln.contiguous().to(dev), ln_c1=(lattice((N,), salt + 6) / 64).to(dev))
            if "g" in fl:
                kw["raw"] = outs["raw"] = nan((M, N))
    got = ops.CONV_GEMM_KINDS[ops.conv_gemm_kind(x, pk, *geom, **kw)]
    assert got == ops.CONV_GEMM_KINDS[kind], "%s: the launcher sends this case to %s, not to %s" % (name, got, ops.CONV_GEMM_KINDS[kind])
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
