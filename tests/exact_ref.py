"""Closed-form reference for the conv / GEMM kernels on EXACT inputs (CPU only, no library call).

On inputs whose products and partial sums are all exact in fp32 the accumulator of an implicit-GEMM kernel holds the mathematical sum in
ANY order of summation (split-K and chunk splits included), so the stored value is that sum through the epilogue, rounded once (RNE) to
the stored format: a plain torch fp32 conv / matmul on the CPU gives the same bits, and a comparison needs no tolerance.

Two input families:
  lattice   tests/golden/make_pingpong_bits.py: activations, residuals and biases multiples of 1/16 in [-2, 2), weights multiples of 1/64
            in [-1/2, 1/2) (the scaling of the bit records, so their cases can be replayed); for deep K a coarser lattice (1/4 and 1/8)
            keeps every partial sum exact.
  ternary   x and w in {-1, 0, 1} with non-zero density min(1, sqrt(400 / K)), integer bias in [-8, 8], integer residual in [-16, 16]:
            every output is a small integer, exact in bf16 up to 256 and in fp16 up to 2048, so no rounding can hide a wrong element.

A Problem names the FORWARD convolution (a pointwise GEMM is B = 1, H = M, W = 1, k = 1); dgrad = True is its input gradient (packing
mode 1: Cout -> Cin channels at the forward input's logical size, F.conv_transpose2d).  check_conditions() asserts what the argument
above needs before anything is compared.
"""
import collections
import hashlib
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_pingpong_bits import lattice  # noqa: E402

# flags: b bias, r 16-bit residual, R fp32 residual, u ReLU, m mask, f fp32 output, n output into NaN-prefilled 8-wide rows,
#        g GEGLU with the raw stash, a alpha = 0.5, v strided x / y views (64 / 32 columns wider), s CF_STATS and w CF_ROWSTATS buffers
#        (their contents have no closed form; y has); G GEGLU without the stash and l CF_LNFOLD appear in the bit records only (no closed
#        form for y)
_Problem = collections.namedtuple("Problem", "name B Cin Cout H W k stride pad up dgrad fl ksplit")


class Problem(_Problem):
    __slots__ = ()

    def __new__(cls, name, B, Cin, Cout, H, W, k=3, stride=1, pad=None, up=0, dgrad=False, fl="b", ksplit=0):
        return super().__new__(cls, name, B, Cin, Cout, H, W, k, stride, k // 2 if pad is None else pad, up, dgrad, fl, ksplit)

    @property
    def fwd_in(self):            # logical (upsampled) input size of the forward conv
        return self.H << self.up, self.W << self.up

    @property
    def fwd_out(self):
        h, w = self.fwd_in
        return (h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1

    @property
    def in_hw(self):             # stored size of the launch's input rows
        return self.fwd_out if self.dgrad else (self.H, self.W)

    @property
    def out_hw(self):
        return self.fwd_in if self.dgrad else self.fwd_out

    @property
    def in_ch(self):
        return self.Cout if self.dgrad else self.Cin

    @property
    def N(self):
        return self.Cin if self.dgrad else self.Cout

    @property
    def ncols(self):             # stored output columns
        return self.N // 2 if ("g" in self.fl or "G" in self.fl) else self.N

    @property
    def M(self):
        return self.B * self.out_hw[0] * self.out_hw[1]

    @property
    def depth(self):             # products per output element
        return self.k * self.k * self.in_ch

    @property
    def alpha(self):
        return 0.5 if "a" in self.fl else 1.0

    @property
    def geom(self):              # (B, H, W, Ho, Wo) of the launch
        return (self.B,) + tuple(self.in_hw) + tuple(self.out_hw)

    @property
    def launch_kw(self):         # stride / shift / parity of the launch
        if self.dgrad:
            return dict(stride=1, shift=1, parity=1) if self.stride == 2 else dict(stride=1)
        return dict(stride=self.stride, shift=self.up)


def pad8(c):
    return (c + 7) // 8 * 8


def _ternary(shape, p, g):
    keep = torch.rand(shape, generator=g) < p
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (keep * sign).float()


def _integers(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def lattice_denominators(prob):
    """(dx, dw): the record's 1/16 and 1/64 where every partial sum stays exact, else the coarser 1/4 and 1/8"""
    return (16, 64) if prob.depth * 1024 * (2 if "a" in prob.fl else 1) + 2 * 2048 * 2 < (1 << 24) else (4, 8)


def make_inputs(prob, family, salt=0):
    """{"w": OIHW fp32, "bias": [N] | None, "x": rows [M_in, pad8(channels)], "res": rows [M, ncols] | None, "mask": rows | None,
    "dx", "dw", "db": the denominators of x, of w and of bias / res}.  lattice with salt = 16 * (case index) is the input of the bit records."""
    ih, iw = prob.in_hw
    m_in, cin = prob.B * ih * iw, pad8(prob.in_ch)
    wshape = (prob.Cout, prob.Cin, prob.k, prob.k)
    if family == "lattice":
        dx, dw = lattice_denominators(prob)
        lx = lambda shape, s: torch.floor(lattice(shape, s) / (16 // dx)) / dx
        w = torch.floor(lattice(wshape, salt) / (64 // dw)) / dw
        x = lx((m_in, cin), salt + 2)
        bias = lattice((prob.N,), salt + 1) / 16 if "b" in prob.fl else None
        res = lattice((prob.M, prob.ncols), salt + 3) / 16 if ("r" in prob.fl or "R" in prob.fl) else None
        mask = lattice((prob.M, prob.ncols), salt + 7) / 16 if "m" in prob.fl else None
    else:
        assert family == "ternary"
        dx = dw = 1
        g = torch.Generator().manual_seed(1000 + salt)
        p = min(1.0, (400.0 / prob.depth) ** 0.5)
        w = _ternary(wshape, p, g)
        x = _ternary((m_in, cin), p, g)
        bias = _integers((prob.N,), 8, g) if "b" in prob.fl else None
        res = _integers((prob.M, prob.ncols), 16, g) if ("r" in prob.fl or "R" in prob.fl) else None
        mask = _integers((prob.M, prob.ncols), 2, g) if "m" in prob.fl else None
    if cin != prob.in_ch:
        x[:, prob.in_ch:] = 0
    return dict(w=w, bias=bias, x=x, res=res, mask=mask, dx=dx, dw=dw, db=16 if family == "lattice" else 1)


GEGLU_PERM_CACHE = {}


def geglu_perm(n):
    """packed column q of a GEGLU projection holds natural column geglu_perm(n)[q] (16 hidden, 16 gate columns interleaved)"""
    if n not in GEGLU_PERM_CACHE:
        f2 = n // 2
        GEGLU_PERM_CACHE[n] = torch.tensor([(q // 32) * 16 + (q % 32) if (q % 32) < 16 else f2 + (q // 32) * 16 + (q % 32 - 16) for q in range(n)])
    return GEGLU_PERM_CACHE[n]


def accumulate(prob, x_rows, w, mutant=None):
    """the sum over taps and channels as fp32 rows [M, N] (no epilogue).  mutant: one of the mutants below, standing for a wrong kernel"""
    ih, iw = prob.in_hw
    x = x_rows[:, :prob.in_ch].float().reshape(prob.B, ih, iw, prob.in_ch).permute(0, 3, 1, 2)
    if prob.dgrad:
        oh, ow = prob.out_hw
        op = (oh - ((ih - 1) * prob.stride - 2 * prob.pad + prob.k), ow - ((iw - 1) * prob.stride - 2 * prob.pad + prob.k))
        y = F.conv_transpose2d(x, w, stride=prob.stride, padding=prob.pad, output_padding=op)
    else:
        if prob.up:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        y = F.conv2d(x, w, stride=prob.stride, padding=prob.pad)
        if mutant is not None:
            y = y + mutant(prob, x, w)
    assert tuple(y.shape[2:]) == tuple(prob.out_hw), (prob.name, y.shape, prob.out_hw)
    return y.permute(0, 2, 3, 1).reshape(prob.M, prob.N)


def epilogue(prob, acc, inp):
    """fp32 rows before the one rounding: mask(relu(alpha * acc + bias + res)); with "g" the pre-activations in packed column order"""
    v = acc * prob.alpha if prob.alpha != 1.0 else acc
    if inp["bias"] is not None:
        v = v + inp["bias"][None, :]
    if "g" in prob.fl:
        return v[:, geglu_perm(prob.N)]
    if inp["res"] is not None:
        v = v + inp["res"]
    if "u" in prob.fl:
        v = v.clamp_min(0)
    if inp["mask"] is not None:
        v = torch.where(inp["mask"] > 0, v, torch.zeros(()))
    return v + 0.0                             # a zero is +0, as a sum that starts from +0 leaves it


def store_dtype(prob, dtype):
    return torch.float32 if "f" in prob.fl else dtype


def stored_width(prob):
    """columns of the whole output buffer: 8-wide rows for the narrow outputs, 32 more for the strided views"""
    n = prob.N if "g" in prob.fl else prob.ncols
    return 8 if "n" in prob.fl else n + (32 if "v" in prob.fl else 0)


def finish(prob, acc, inp, dtype=torch.bfloat16):
    """accumulate()'s rows through the epilogue and the one rounding, as the WHOLE output buffer (the raw stash with "g") the kernel must
    leave: [M, stored_width] in the stored format, NaN wherever the kernel must not write"""
    v = epilogue(prob, acc, inp)
    dt = store_dtype(prob, dtype)
    out = torch.full((prob.M, stored_width(prob)), float("nan"), dtype=dt)
    out[:, :v.shape[1]] = v.to(dt)              # torch rounds to nearest even
    return out


def expected(prob, inp, dtype=torch.bfloat16, mutant=None):
    return finish(prob, accumulate(prob, inp["x"], inp["w"], mutant), inp, dtype)


def mutant_rows(prob, inp, mutant):
    """what a mutant adds to accumulate()'s rows"""
    x = inp["x"][:, :prob.Cin].float().reshape(prob.B, prob.H, prob.W, prob.Cin).permute(0, 3, 1, 2)
    if prob.up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return mutant(prob, x, inp["w"]).permute(0, 2, 3, 1).reshape(prob.M, prob.N)


def check_conditions(prob, inp, family, dtype=torch.bfloat16, ref=None):
    """Asserts that every partial sum of the case is exact in fp32 in every order and, for ternary, that the outputs are exact in the
    stored format.  Units: 1 / (dx dw) (halved by alpha = 0.5)."""
    unit = inp["dx"] * inp["dw"] * (2 if prob.alpha == 0.5 else 1)
    assert unit % inp["db"] == 0
    for k, d in (("x", inp["dx"]), ("w", inp["dw"]), ("bias", inp["db"]), ("res", inp["db"])):
        if inp[k] is not None:
            assert torch.equal(inp[k] * d, torch.round(inp[k] * d)), "%s: %s is not on its lattice" % (prob.name, k)
            assert torch.equal(inp[k].to(dtype).float(), inp[k]), "%s: %s is not exact in %s" % (prob.name, k, dtype)
    mx = lambda t: 0.0 if t is None else float(t.abs().max())
    bound = prob.depth * mx(inp["x"]) * mx(inp["w"]) * unit + (mx(inp["bias"]) + mx(inp["res"])) * unit
    assert bound < (1 << 24), "%s: partial sums up to %d units are not exact in fp32" % (prob.name, bound)
    if family == "ternary" and ref is not None:
        lim = (2048 if store_dtype(prob, dtype) == torch.float16 else 256) * prob.alpha      # alpha = 0.5: half-integers
        if store_dtype(prob, dtype) != torch.float32:
            big = float(torch.nan_to_num(ref.float(), nan=0.0).abs().max())
            assert big <= lim, "%s: |output| %g is not exact in the stored format" % (prob.name, big)
    return bound


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def mismatch_report(prob, got, want, tile_rows=256):
    """None if got and want hold the same bits (NaN prefill included), else a text: the count of wrong elements, the first eight as
    (image, oy, ox, n) with got / want, whether all lie on an image border, their row index modulo the tile height"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (prob.name, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(bits(got), bits(want)):
        return None
    bad = (bits(got) != bits(want)).nonzero()
    oh, ow = prob.out_hw
    rows, cols = bad[:, 0], bad[:, 1]
    oy, ox = (rows // ow) % oh, rows % ow
    border = (oy == 0) | (oy == oh - 1) | (ox == 0) | (ox == ow - 1)
    lines = ["%s: %d of %d elements differ (%d rows, %d columns touched)" % (prob.name, len(bad), got.numel(), rows.unique().numel(), cols.unique().numel())]
    for r, c in bad[:8].tolist():
        lines.append("  (image %d, oy %d, ox %d, n %d): got %r want %r" % (r // (oh * ow), (r // ow) % oh, r % ow, c, float(got[r, c]), float(want[r, c])))
    lines.append("  all on an image border: %s (%d of %d)" % (bool(border.all()), int(border.sum()), len(bad)))
    mods = (rows % tile_rows).unique().tolist()
    lines.append("  row index mod %d: %s%s" % (tile_rows, mods[:16], " ..." if len(mods) > 16 else ""))
    lines.append("  columns: %s%s" % (cols.unique().tolist()[:16], " ..." if cols.unique().numel() > 16 else ""))
    return "\n".join(lines)


# ---- mutants of the reference: each stands for a fault of a kernel's staging that the exact comparison must see ----------------------
# A mutant is a function (prob, x NCHW at the conv's logical input size, w) -> what the faulty kernel ADDS to the right sums (NCHW); each
# costs a fraction of the conv (only the channels / taps concerned are convolved).  Forward problems only.

def _conv(prob, x, w):
    return F.conv2d(x, w, stride=prob.stride, padding=prob.pad)


def _tap_window(prob, x, tap):
    """the pixels tap `tap` reads, one per output pixel (zero padding included)"""
    ky, kx = divmod(tap % (prob.k * prob.k), prob.k)
    oh, ow = prob.fwd_out
    xp = F.pad(x, (prob.pad,) * 4)
    return xp[:, :, ky:ky + (oh - 1) * prob.stride + 1:prob.stride, kx:kx + (ow - 1) * prob.stride + 1:prob.stride]


def _tap_weight(prob, w, tap):
    ky, kx = divmod(tap % (prob.k * prob.k), prob.k)
    return w[:, :, ky, kx][:, :, None, None]


def mutant_dropped_vector(prob, x, w, tap=3, first_ch=8, last_column_only=True):
    """one 16-byte vector (8 channels) of one tap is not staged, at the last image column only (or at every pixel); the default tap reads
    the pixel to the left, which is inside the image at the last column"""
    c0 = min(first_ch, max(prob.Cin - 8, 0))
    d = -F.conv2d(_tap_window(prob, x[:, c0:c0 + 8], tap), _tap_weight(prob, w[:, c0:c0 + 8], tap))
    if last_column_only:
        d[:, :, :, :-1] = 0
    return d


def mutant_swapped_taps(prob, x, w, a=1, b=7):
    """two entries of the tap table swapped: tap a reads the pixels of tap b and back (needs more than one tap)"""
    return F.conv2d(_tap_window(prob, x, a) - _tap_window(prob, x, b), _tap_weight(prob, w, b) - _tap_weight(prob, w, a))


def mutant_chunk_twice(prob, x, w):
    """the first 64-channel chunk of the input is used in place of the second as well (a stage that was not refilled; Cin >= 128)"""
    return _conv(prob, x[:, :64] - x[:, 64:128], w[:, 64:128])


MUTANTS = (("dropped_vector", mutant_dropped_vector, lambda p: True), ("swapped_taps", mutant_swapped_taps, lambda p: p.k > 1),
           ("chunk_twice", mutant_chunk_twice, lambda p: p.Cin >= 128))
