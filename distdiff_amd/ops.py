"""Pythonic wrappers over the op-level C ABI (include/distdiff_hip_ops.h) on torch device tensors.

Used by the parity tests and for debugging; the production loop goes through distdiff_amd.engine.
Tensors are NHWC bf16 (a [pixels, C] matrix) unless stated. Nothing here computes on the CPU.

The 16-bit storage format is a property of the library (libdistdiff_hip.so: bf16, libdistdiff_hip_f16.so: IEEE half).  Every wrapper
picks the library from the dtype of its activation tensor (torch.bfloat16 / torch.float16; packed weights: PackedConv(dtype=)), and
outputs take that dtype; the plan queries without a tensor take it from the packed weights or a `dtype` keyword.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (CF_BIAS, CF_GEGLU, CF_GEGLU_RAW, CF_LNFOLD, CF_MASK, CF_OUT_F32, CF_RELU, CF_RES, CF_RES_F32, CF_ROWSTATS, CF_STATS, AttnParams,
                   ConvGemmParams, GroupNormParams, LayerNormParams, check)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L(t):
    """the library whose storage format is the dtype of t (a tensor, a PackedConv or a torch dtype)"""
    return _lib.lib(t if isinstance(t, torch.dtype) else t.dtype)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class PackedConv:
    """Device copy of pre-packed weights for one conv/linear (forward or dgrad form)."""

    def __init__(self, w_oihw, pad, mode=0, geglu=False, bias=None, device="cuda", dtype=torch.bfloat16):
        self.dtype = dtype                        # torch.bfloat16 | torch.float16: packed (host side, RNE) by the library of that format
        w = w_oihw.detach().float().contiguous().cpu()
        if w.dim() == 2:
            w = w[:, :, None, None].contiguous()
        Cout, Cin, KH, KW = w.shape
        out4 = (C.c_int * 4)()
        L = _L(dtype)
        L.dd_pack_conv_weight(C.c_void_p(w.data_ptr()), Cout, Cin, KH, KW, pad, mode, int(geglu), None, None, out4)
        self.N, self.K, self.cin, self.ntaps = out4[0], out4[1], out4[2], out4[3]
        wp = np.zeros((self.N, self.K), dtype=np.uint16)
        tt = np.zeros((self.ntaps,), dtype=np.int32)
        L.dd_pack_conv_weight(C.c_void_p(w.data_ptr()), Cout, Cin, KH, KW, pad, mode, int(geglu),
                              wp.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p), out4)
        self.w = torch.from_numpy(wp.view(np.int16)).to(device).view(dtype)
        self.taptab = torch.from_numpy(tt).to(device)
        self.taptab_host = tt.copy()              # host copy: contract checks without a device round trip (conv_gemm); read-only
        self.taptab_host.setflags(write=False)
        self.geglu = bool(geglu) and mode == 0   # in dgrad form the permutation applies to K only
        self.bias = None
        if bias is not None:
            b = bias.detach().float().cpu()
            if geglu:
                F = Cout // 2
                perm = [(p // 32) * 16 + (p % 32) if (p % 32) < 16 else F + (p // 32) * 16 + (p % 32 - 16) for p in range(Cout)]
                b = b[perm]
            self.bias = b.to(device)


class PackedConvF32:
    """fp32 packing of one guide conv (forward or dgrad form) for dd_op_conv_f32; w is [Cout][Cin/groups][KH][KW]."""

    def __init__(self, w, pad, mode=0, groups=1, bias=None, device="cuda"):
        w = w.detach().float().contiguous().cpu()
        Cout, Cg, KH, KW = w.shape
        Cin = Cg * groups
        out4 = (C.c_int * 4)()
        L = _lib.lib()
        L.dd_pack_conv_weight_f32(C.c_void_p(w.data_ptr()), Cout, Cin, KH, KW, pad, mode, groups, None, None, out4)
        self.N, self.K, self.cin, self.ntaps = out4[0], out4[1], out4[2], out4[3]
        wp = np.zeros((self.N, self.K), dtype=np.float32)
        tt = np.zeros((self.ntaps,), dtype=np.int32)
        L.dd_pack_conv_weight_f32(C.c_void_p(w.data_ptr()), Cout, Cin, KH, KW, pad, mode, groups,
                                  wp.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p), out4)
        self.w = torch.from_numpy(wp).to(device)
        self.taptab = torch.from_numpy(tt).to(device)
        self.groups = groups
        gi, go = Cin // groups, Cout // groups
        self.cpg_in, self.cpg_out = (go, gi) if mode else (gi, go)
        self.bias = bias.detach().float().to(device) if bias is not None else None


def conv_f32(x, pk, B, H, W, Ho, Wo, stride=1, shift=0, parity=0, res=None, mask=None, relu=False, y=None):
    """x: fp32 [B*H*W, ld] (ld % 4 == 0); returns fp32 y [B*Ho*Wo, roundup(N, 4)].  y: the output rows to write (at least N columns);
    res may be that same tensor (the accumulating input-gradient of the reverse pass)."""
    from ._lib import ConvF32Params
    p = ConvF32Params()
    M = B * Ho * Wo
    if y is None:
        y = torch.zeros((M, (pk.N + 3) // 4 * 4), device=x.device, dtype=torch.float32)
    p.x, p.w, p.taptab, p.y = _ptr(x), _ptr(pk.w), _ptr(pk.taptab), _ptr(y)
    p.x_ld, p.y_ld = x.stride(0), y.stride(0)
    flags = 0
    if pk.bias is not None:
        flags |= CF_BIAS
        p.bias = _ptr(pk.bias)
    if res is not None:
        flags |= CF_RES
        p.res, p.res_ld = _ptr(res), res.stride(0)
    if mask is not None:
        flags |= CF_MASK
        p.mask, p.mask_ld = _ptr(mask), mask.stride(0)
    if relu:
        flags |= CF_RELU
    p.B, p.H, p.W, p.Ho, p.Wo, p.stride, p.shift, p.parity = B, H, W, Ho, Wo, stride, shift, parity
    p.cin, p.ntaps, p.M, p.N, p.K = pk.cin, pk.ntaps, M, pk.N, pk.K
    p.groups, p.cpg_in, p.cpg_out, p.flags = pk.groups, pk.cpg_in, pk.cpg_out, flags
    check(_lib.lib().dd_op_conv_f32(C.byref(p), _stream()), "conv_f32")
    return y[:, :pk.N]


_NOT_READ = 1 << 12     # stands for a buffer in conv_gemm_kind: the decision tests pointers for null and never follows them


def _dry_ptr(t):
    return C.c_void_p(_NOT_READ) if t is True else _ptr(t)


def _dry_ld(t, ncols):
    return ncols if t is True else t.stride(0)


def _conv_gemm_params(x, pk, B, H, W, Ho, Wo, stride=1, shift=0, parity=0, res=None, mask=None, relu=False, out_f32=False,
                      ksplit=0, alpha=1.0, raw=None, y=None, x_ld=None, partial=None, force_small=False, stats=None, ln_stats=None, ln_c1=None,
                      rowpart=None, dry=False):
    """The ConvGemmParams block of one launch: (p, partial_cap_bytes, y, buffers to keep alive).  dry (conv_gemm_kind): nothing is
    allocated; x / y may be None (contiguous rows assumed) and res / stats / ln_stats / rowpart may be True for "present"."""
    p = ConvGemmParams()
    M = B * Ho * Wo
    ncols = pk.N // 2 if pk.geglu else pk.N
    # pointwise contract of dd_op_conv_gemm: a one-tap, stride-1, same-size launch does not read its tap table (it IS the centre tap);
    # checked here on the host copy kept at pack time, so the launch itself stays stream-asynchronous
    if pk.ntaps == 1 and stride == 1 and (H, W) == (Ho, Wo) and shift == 0 and int(pk.taptab_host[0]) != ((32 << 6) | 32):
        raise RuntimeError("conv_gemm: a one-tap stride-1 launch must be the centre tap (got %#x)" % int(pk.taptab_host[0]))
    if y is None and not dry:
        y = torch.empty((M, ncols), device=x.device, dtype=torch.float32 if out_f32 else pk.dtype)
    p.x, p.w, p.taptab, p.y = _ptr(x), _ptr(pk.w), _ptr(pk.taptab), _ptr(y)
    p.x_ld = x_ld if x_ld is not None else (x.stride(0) if x is not None else pk.cin)
    p.y_ld = y.stride(0) if y is not None else ncols
    flags = 0
    if pk.bias is not None:
        flags |= CF_BIAS
        p.bias = _ptr(pk.bias)
    if res is not None:
        flags |= CF_RES
        if res is not True and res.dtype == torch.float32:
            flags |= CF_RES_F32
        p.res, p.res_ld = _dry_ptr(res), _dry_ld(res, ncols)
    if mask is not None:
        flags |= CF_MASK
        p.mask, p.mask_ld = _ptr(mask), mask.stride(0)
    if relu:
        flags |= CF_RELU
    if out_f32:
        flags |= CF_OUT_F32
    if pk.geglu:
        flags |= CF_GEGLU
        if raw is not None:
            flags |= CF_GEGLU_RAW
            p.raw, p.raw_ld = _ptr(raw), raw.stride(0)
    cap = 0
    if ksplit != 1:
        if partial is None and not dry:
            partial = torch.empty((max(ksplit, 16) * M * pk.N,), device=x.device, dtype=torch.float32)
        p.partial = _dry_ptr(True if partial is None else partial)
        cap = (max(ksplit, 16) * M * pk.N if partial is None else partial.numel()) * 4
    p.B, p.H, p.W, p.Ho, p.Wo, p.stride, p.shift, p.parity = B, H, W, Ho, Wo, stride, shift, parity
    p.cin, p.ntaps, p.M, p.N, p.K = pk.cin, pk.ntaps, M, pk.N, pk.K
    if stats is not None:
        flags |= CF_STATS
        p.stats, p.stats_ld = _dry_ptr(stats), _dry_ld(stats, 2 * ncols) // 2
    if ln_stats is not None:      # CF_LNFOLD: x is the raw LayerNorm input, pk holds gamma o W, ln_c1 its column sums (packed order)
        flags |= CF_LNFOLD
        p.ln_stats, p.ln_c1 = _dry_ptr(ln_stats), _dry_ptr(True if ln_stats is True else ln_c1)
    if rowpart is not None:       # CF_ROWSTATS: fp32 [M, spans, 2] (sum, sum of squares) per row and column span
        flags |= CF_ROWSTATS
        p.rowpart, p.rowpart_ld = _dry_ptr(rowpart), _dry_ld(rowpart, 2 * ((ncols + 39) // 40)) // 2
    p.ksplit, p.flags, p.alpha = ksplit, flags, alpha
    p.force_small = int(force_small)
    return p, cap, y, (partial,)


def conv_gemm(x, pk, B, H, W, Ho, Wo, *args, check_device_taps=False, **kw):
    """x: bf16 [B*H*W, x_ld]; returns y [B*Ho*Wo, N(or N/2 for GEGLU)].  stats: fp32 [M/64, C, 2] buffer (or a column view of one) to
    receive the per-(64-row block, channel) partial (mean, M2) of the stored values (CF_STATS; the launch fails if the kernel the
    launcher picks for this shape cannot emit them).  Keywords: _conv_gemm_params."""
    p, cap, y, _keep = _conv_gemm_params(x, pk, B, H, W, Ho, Wo, *args, **kw)
    if check_device_taps:      # synchronous: the tap contract against the DEVICE table (dd_op_conv_gemm_check)
        check(_L(pk).dd_op_conv_gemm_check(C.byref(p), _stream()), "conv_gemm tap table check")
    check(_L(pk).dd_op_conv_gemm(C.byref(p), cap, _stream()), "conv_gemm")
    return y


CONV_GEMM_KINDS = ("general", "conv_halo", "conv_halo_persist", "gemm_ws", "gemm_pps")


def conv_gemm_kind(x, pk, B, H, W, Ho, Wo, *args, **kw):
    """Which kernel conv_gemm would run for the same arguments, as an index into CONV_GEMM_KINDS (dd_op_conv_gemm_kind: the launcher's
    own decision, nothing is launched or allocated).  Buffers may be left out: x / y = None mean contiguous rows, res / stats /
    ln_stats / rowpart = True mean "present".  Raises for a problem the launcher refuses."""
    p, cap, _y, _keep = _conv_gemm_params(x, pk, B, H, W, Ho, Wo, *args, dry=True, **kw)
    kind = _L(pk).dd_op_conv_gemm_kind(C.byref(p), cap)
    if kind < 0:
        raise RuntimeError("conv_gemm_kind: the launcher refuses this problem (status %d)" % kind)
    return kind


# the forms inside kind "general" (dd_op_conv_gemm_plan): conv_gemm_kernel's two tile shapes, then conv_gemm_big_kernel's configurations
CONV_GEMM_FORMS = ("small_128x128", "big_128x256", "big_256x160", "big_256x128", "big_128x160_two_workgroups", "big_128x128_two_workgroups")


def conv_gemm_plan(x, pk, B, H, W, Ho, Wo, *args, **kw):
    """(kind, form, split) of the launch conv_gemm would make for the same arguments (nothing is launched; buffers as for conv_gemm_kind):
    kind as conv_gemm_kind; form names the kernel form inside kind "general" (CONV_GEMM_FORMS, or "small_256x64"), None for the other
    kinds; split is the split-K (the chunk split at the 8 x 8 halo level) in use, 1 = none."""
    p, cap, _y, _keep = _conv_gemm_params(x, pk, B, H, W, Ho, Wo, *args, dry=True, **kw)
    out4 = (C.c_int * 4)()
    kind = _L(pk).dd_op_conv_gemm_plan(C.byref(p), cap, out4)
    if kind < 0:
        raise RuntimeError("conv_gemm_plan: the launcher refuses this problem (status %d)" % kind)
    form = None
    if kind == 0:
        form = "small_256x64" if (out4[1] == 0 and out4[3]) else CONV_GEMM_FORMS[out4[1]]
    return CONV_GEMM_KINDS[kind], form, out4[2]


def groupnorm(x, gamma, beta, B, HW, G, eps, silu, dy=None, stats=None, chan_part=None, accumulate_into=None, y=None, dx=None):
    """Forward (y, stats), or with dy the input-gradient dx.  accumulate_into: a dx buffer that already holds a gradient -- the result
    is added to it in place (GroupNormParams.accumulate) and it is returned.  y / dx: write the forward result / the gradient there (a
    column view of a wider buffer is fine) instead of into a fresh tensor."""
    Cc = x.shape[1]
    L = _L(x)
    p = GroupNormParams()
    if y is None:
        y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    scratch = torch.empty((L.dd_op_groupnorm_scratch_bytes(B, G) // 4,), device=x.device, dtype=torch.float32)
    if stats is None:
        stats = torch.empty((B, G, 2), device=x.device, dtype=torch.float32)
    p.x, p.x_ld, p.y, p.y_ld = _ptr(x), x.stride(0), _ptr(y), y.stride(0)
    p.gamma, p.beta, p.stats, p.scratch = _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(scratch)
    p.B, p.HW, p.C, p.G, p.eps, p.silu = B, HW, Cc, G, eps, int(silu)
    if chan_part is not None:     # [B*HW/64, C_total, 2] partials emitted by the producing convolutions (a column view is fine)
        p.chan_part, p.part_ld = _ptr(chan_part), chan_part.stride(0) // 2
    if dy is None:
        check(L.dd_op_groupnorm_fwd(C.byref(p), _stream()), "gn_fwd")
        return y, stats
    if accumulate_into is not None:
        dx = accumulate_into
    elif dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    p.dy, p.dy_ld, p.dx, p.dx_ld, p.accumulate = _ptr(dy), dy.stride(0), _ptr(dx), dx.stride(0), int(accumulate_into is not None)
    check(L.dd_op_groupnorm_bwd(C.byref(p), _stream()), "gn_bwd")
    return dx


def layernorm_stats(x, eps, rowpart=None, spans=0):
    """(mean, rstd) [M, 2] only (a LayerNorm folded into the GEMM that follows): from x, or from a GEMM's row partials."""
    M, Cc = x.shape
    p = LayerNormParams()
    stats = torch.empty((M, 2), device=x.device, dtype=torch.float32)
    p.x, p.x_ld, p.stats, p.M, p.C, p.eps = _ptr(x), x.stride(0), _ptr(stats), M, Cc, eps
    if rowpart is not None:
        p.rowpart, p.rowpart_ld, p.spans = _ptr(rowpart), rowpart.stride(0) // 2, spans
    check(_L(x).dd_op_layernorm_fwd(C.byref(p), _stream()), "ln_stats")
    return stats


def layernorm(x, gamma, beta, eps, dy=None, stats=None, accumulate_into=None, y=None, dx=None):
    """Forward (y, stats), or with dy the input-gradient dx; accumulate_into, y and dx as for groupnorm (LayerNormParams.accumulate)."""
    M, Cc = x.shape
    L = _L(x)
    p = LayerNormParams()
    if y is None:
        y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    if stats is None:
        stats = torch.empty((M, 2), device=x.device, dtype=torch.float32)
    p.x, p.x_ld, p.y, p.y_ld = _ptr(x), x.stride(0), _ptr(y), y.stride(0)
    p.gamma, p.beta, p.stats, p.M, p.C, p.eps = _ptr(gamma), _ptr(beta), _ptr(stats), M, Cc, eps
    if dy is None:
        check(L.dd_op_layernorm_fwd(C.byref(p), _stream()), "ln_fwd")
        return y, stats
    if accumulate_into is not None:
        dx = accumulate_into
    elif dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    p.dy, p.dy_ld, p.dx, p.dx_ld, p.accumulate = _ptr(dy), dy.stride(0), _ptr(dx), dx.stride(0), int(accumulate_into is not None)
    check(L.dd_op_layernorm_bwd(C.byref(p), _stream()), "ln_bwd")
    return dx


def _attn_fwd_params(q, k, v, B, H, Nq, Nk, D, scale, causal=False, q_prescaled=False, pv_fp8=False, no_shortk=False, o=None):
    """o: write the output there (B * Nq rows, H * D columns: a column view of a wider buffer, as the engine passes it) instead of into a
    fresh tensor"""
    p = AttnParams()
    if o is None:
        o = torch.zeros((B * Nq, H * D), device=q.device, dtype=q.dtype)
    elif tuple(o.shape) != (B * Nq, H * D) or o.dtype != q.dtype or o.stride(1) != 1:
        raise ValueError("attention: o must be %s rows of %d unit-stride columns of %s" % (B * Nq, H * D, q.dtype))
    lse = torch.empty((B, H, Nq), device=q.device, dtype=torch.float32)
    p.q, p.k, p.v, p.o, p.lse = _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse)
    p.ldq, p.ldk, p.ldv, p.ldo = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    p.B, p.H, p.Nq, p.Nk, p.D, p.scale = B, H, Nq, Nk, D, scale
    p.causal = 1 if causal else 0
    p.q_prescaled = 1 if q_prescaled else 0
    p.pv_fp8 = 1 if pv_fp8 else 0
    p.no_shortk = 1 if no_shortk else 0       # diagnostics: <= 80 keys on the streaming kernel (accuracy A/B)
    return p, o, lse


def _attn_bwd_params(p, o, d_o, need_dkv=True):
    """adds the backward's buffers to p; returns (dq, dk, dv, delta): delta only has to stay alive"""
    dq = torch.zeros_like(o)
    dk = torch.zeros((p.B * p.Nk, p.H * p.D), device=o.device, dtype=o.dtype) if need_dkv else None
    dv = torch.zeros_like(dk) if need_dkv else None
    delta = torch.empty((p.B, p.H, p.Nq), device=o.device, dtype=torch.float32)
    p.d_o, p.lddo, p.dq, p.lddq, p.delta = _ptr(d_o), d_o.stride(0), _ptr(dq), dq.stride(0), _ptr(delta)
    if need_dkv:
        p.dk, p.dv, p.lddk, p.lddv = _ptr(dk), _ptr(dv), dk.stride(0), dv.stride(0)
    return dq, dk, dv, delta


def _attn_scratch(q, Nq, Nk, D, ws_images):
    """(workspace, bytes, tap1x1, partial, bytes) of the dd_op_attention* argument lists, and the tensors behind them"""
    L = _L(q)
    L.dd_op_attention_gemm_workspace.restype = C.c_size_t
    if ws_images <= 0:
        return (None, C.c_size_t(0), None, None, C.c_size_t(0)), None
    ws = torch.empty(L.dd_op_attention_gemm_workspace(Nq, Nk, D, 1) * ws_images, device=q.device, dtype=torch.uint8)
    tap = torch.tensor([(32 << 6) | 32], device=q.device, dtype=torch.int32)
    part = torch.empty(32 * 1024 * 1024, device=q.device, dtype=torch.float32)
    return (_ptr(ws), C.c_size_t(ws.numel()), _ptr(tap), _ptr(part), C.c_size_t(part.numel() * 4)), (ws, tap, part)


def attention_gemm(q, k, v, B, H, Nq, Nk, D, scale, d_o=None, ws_images=8, o=None):
    """wide-head attention through the GEMM kernel (dd_op_attention_gemm_*): same arguments / results as `attention`.  ws_images: scratch
    for that many images (single-head layers then run min(ws_images, 8, B) images per launch)."""
    L = _L(q)
    p, o, lse = _attn_fwd_params(q, k, v, B, H, Nq, Nk, D, scale, o=o)
    sc, _keep = _attn_scratch(q, Nq, Nk, D, max(1, ws_images))
    check(L.dd_op_attention_gemm_fwd(C.byref(p), *sc, _stream()), "attn_gemm_fwd")
    if d_o is None:
        return o, lse
    dq, dk, dv, _delta = _attn_bwd_params(p, o, d_o)
    check(L.dd_op_attention_gemm_bwd(C.byref(p), *sc, _stream()), "attn_gemm_bwd")
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def attention(q, k, v, B, H, Nq, Nk, D, scale, d_o=None, need_dkv=True, **flags):
    """q [B*Nq, >=H*D], k/v [B*Nk, >=H*D] bf16 (row strides taken from the tensors), on the flash kernels.  flags: causal; q_prescaled: q
    already carries 1/sqrt(D) * log2(e) (the engine folds it into the to_q weights); pass scale = ln 2 then.  pv_fp8 (D = 64, forward): the
    P.V product on the block-scaled fp8 MFMA (e4m3 probabilities and values); no_shortk."""
    L = _L(q)
    p, o, lse = _attn_fwd_params(q, k, v, B, H, Nq, Nk, D, scale, **flags)
    check(L.dd_op_attention_fwd(C.byref(p), _stream()), "attn_fwd")
    if d_o is None:
        return o, lse
    dq, dk, dv, _delta = _attn_bwd_params(p, o, d_o, need_dkv)
    check(L.dd_op_attention_bwd(C.byref(p), _stream()), "attn_bwd")
    return o, lse, dq, dk, dv


ATTENTION_ROUTES = ("gemm", "shortk", "dma", "stream", "flash_bwd")      # dd_op_attention_plan


def _attention_plan(p, ws_bytes, bwd, dtype=torch.bfloat16):
    out = (C.c_int * 26)()
    route = _L(dtype).dd_op_attention_plan(C.byref(p), ws_bytes, int(bwd), out)
    if route < 0:
        raise RuntimeError("attention_plan: the launcher refuses this problem (status %d)" % route)
    return {"route": ATTENTION_ROUTES[route], "d": out[1], "qt": out[2], "kt": out[3], "dsplit": out[4], "ktw": out[5], "qtl": out[6],
            "waves": out[7], "lazy": bool(out[8] & 1), "prescaled": bool(out[8] & 2), "causal": bool(out[8] & 4), "fp8": bool(out[8] & 8),
            "group": out[9], "launches": [tuple(out[11 + 5 * j:16 + 5 * j]) for j in range(out[10])]}


def attention_planned(q, k, v, B, H, Nq, Nk, D, scale, d_o=None, need_dkv=True, ws_images=0, **flags):
    """The launcher's one entry (dd_op_attention): `attention` with scratch for ws_images images offered (0: none), so that the planner
    may take the GEMM route.  Returns the results of `attention` and the plans (dd_op_attention_plan, asked with the same arguments) of
    the forward and, with d_o, the backward: dicts of route (ATTENTION_ROUTES), tile form, flags, group and launches."""
    L = _L(q)
    p, o, lse = _attn_fwd_params(q, k, v, B, H, Nq, Nk, D, scale, **flags)
    sc, _keep = _attn_scratch(q, Nq, Nk, D, ws_images)
    plans = [_attention_plan(p, sc[1], False, q.dtype)]
    check(L.dd_op_attention(C.byref(p), *sc, 0, _stream()), "attention fwd")
    if d_o is None:
        return (o, lse), plans
    dq, dk, dv, _delta = _attn_bwd_params(p, o, d_o, need_dkv)
    plans.append(_attention_plan(p, sc[1], True, q.dtype))
    check(L.dd_op_attention(C.byref(p), *sc, 1, _stream()), "attention bwd")
    torch.cuda.synchronize()
    return (o, lse, dq, dk, dv), plans


def to_nhwc_bf16(x_nchw, cpad=None, dtype=torch.bfloat16):
    """host/torch-side helper for tests: NCHW fp32 -> [B*H*W, Cpad] bf16 (or `dtype`), zero padded."""
    B, Cc, H, W = x_nchw.shape
    cpad = cpad or Cc
    y = torch.zeros((B, H, W, cpad), dtype=torch.float32)
    y[..., :Cc] = x_nchw.permute(0, 2, 3, 1)
    return y.reshape(B * H * W, cpad).to(dtype)


def from_nhwc(y, B, H, W):
    return y.float().reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()
