"""The bench step's deep 3x3 convolutions (engine batch 32: CFG batch 64 for the UNet, 32 images for the VAE) through the op-level ABI,
for A/B of the halo-resident kernel: DD_CONV_HALO=0 python tools/bench_halo.py vs DD_CONV_HALO=1.

    python tools/bench_halo.py --resolution     # the 3x3 levels of 384 / 640 / 768-pixel images (widths 48 / 80 / 96 ... 768: several
                                                # power-of-two tiles per image row), forward and input-gradient, with the kernel each gets
                                                # (profiles/resolution_per_shape.txt: DD_CONV_HALO=0 = the general kernels, interleaved)"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from distdiff_amd import ops


def run(name, B, H, Cin, Cout, res=False, iters=6):
    g = torch.Generator().manual_seed(0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    pk = ops.PackedConv(w, 1, bias=torch.randn(Cout, generator=g))
    M = B * H * H
    x = torch.randn(M, Cin, device="cuda").to(torch.bfloat16)
    y = torch.empty(M, Cout, dtype=torch.bfloat16, device="cuda")
    r = torch.randn(M, Cout, device="cuda").to(torch.bfloat16) if res else None
    part = torch.empty(16 * 1024 * 1024, dtype=torch.float32, device="cuda")
    f = lambda: ops.conv_gemm(x, pk, B, H, H, H, H, y=y, res=r, partial=part)
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / iters
    return "%s %.0f us %.0f TF/s" % (name, us, 2.0 * M * Cout * Cin * 9 / us / 1e6)


def run_resolution(B, Cin, Cout, H, up, iters=5):
    """One 3x3 layer of a non-power-of-two level: forward (with the fused nearest-2x upsample when `up`) and input-gradient."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    Ho = H << up
    part = torch.empty(16 * 1024 * 1024, dtype=torch.float32, device="cuda")
    res = []
    for what, pk, h, sh in (("fwd", ops.PackedConv(w, 1, bias=torch.randn(Cout, generator=g)), H, up), ("dgrad", ops.PackedConv(w, 1, mode=1), Ho, 0)):
        x = torch.randn(B * h * h, pk.cin, device="cuda").to(torch.bfloat16)
        y = torch.empty(B * Ho * Ho, pk.N, dtype=torch.bfloat16, device="cuda")
        kind = ops.CONV_GEMM_KINDS[ops.conv_gemm_kind(x, pk, B, h, h, Ho, Ho, shift=sh, y=y, partial=part)]
        f = lambda: ops.conv_gemm(x, pk, B, h, h, Ho, Ho, shift=sh, y=y, partial=part)
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000 / iters
        res.append("%s %s %.0f us %.0f TF/s" % (what, kind, us, 2.0 * B * Ho * Ho * Cout * Cin * 9 / us / 1e6))
    return "%d x %d>%d@%d%s: %s" % (B, Cin, Cout, H, "(up2)" if up else "", ", ".join(res))


tag = "halo=" + os.environ.get("DD_CONV_HALO", "1")
if "--resolution" in sys.argv:
    shapes = [(32, 320, 320, 96, 0), (32, 640, 640, 48, 0), (32, 320, 320, 80, 0), (32, 320, 320, 48, 1),
              (8, 128, 128, 768, 0), (8, 256, 256, 384, 0), (8, 512, 512, 192, 0), (8, 256, 256, 96, 1)]
    for sh in shapes:
        print(tag, run_resolution(*sh), flush=True)
    sys.exit(0)
out = [run("960>320@64", 64, 64, 960, 320), run("320>320@64", 64, 64, 320, 320, True), run("640>320@64", 64, 64, 640, 320), run("640>640@32", 64, 32, 640, 640, True),
       run("1280>640@32", 64, 32, 1280, 640), run("1280>1280@16", 64, 16, 1280, 1280, True), run("2560>1280@16", 64, 16, 2560, 1280),
       run("512>512@64", 32, 64, 512, 512, True, 3), run("512>512@128", 32, 128, 512, 512, True, 2), run("256>256@256", 8, 256, 256, 256, True, 2), run("128>128@512", 8, 512, 128, 128, True, 2), run("256>128@512", 8, 512, 256, 128, False, 2)]
print(tag, " | ".join(out))
