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

On the ternary family the statistics epilogues, the LayerNorm fold and GEGLU have closed forms too (expected_buffers; conditions in
check_stat_conditions).  CF_STATS: plain sums a, q of the integers of a 64-row block, mean = a / 64, M2 = max(q - a * mean, 0), exact
while a^2 and q stay below 2^24.  CF_ROWSTATS: (sum, sum of squares) over a wave's column span.  CF_LNFOLD: the kernels only read
(mean, rstd), so the test supplies small integer means and power-of-two rstd, and alpha * rstd * (acc - mean * c1) + b' is one exact
number in either spelling the kernels use.  GEGLU: gelu_poly_f is a clamp, multiplications and fmas; each is formed exactly here and
rounded once (gelu_phi), on a table of the multiples of 1 / 8 inside the clamp.  The lattice family has none of these: its squares are
not exact.
"""
import collections
import fractions
import hashlib
import os
import re
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_pingpong_bits import lattice  # noqa: E402

# flags: b bias, r 16-bit residual, R fp32 residual, u ReLU, m mask, f fp32 output, n output into NaN-prefilled 8-wide rows,
#        g GEGLU with the raw stash, G GEGLU without it, a alpha = 0.5, v strided x / y views (64 / 32 columns wider), s CF_STATS and
#        w CF_ROWSTATS buffers, l CF_LNFOLD.
# s, w, l, G and the y of g have closed forms on the TERNARY family only (expected_stats, expected_rowpart, fold(), geglu_product()): the
# sums of squares of the lattice family (units of 1 / 2^20) are not exact in fp32, and neither are its folded or gated values, so on lattice
# inputs -- the bit records -- those outputs are not derived here.
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
    "dx", "dw", "db": the denominators of x, of w and of bias / res, "ln_stats": [M, 2] (mean, rstd) with "l" (ternary only) | None}.
    lattice with salt = 16 * (case index) is the input of the bit records."""
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
    ln_stats = None
    if "l" in prob.fl:
        # the kernels only READ ln_stats[m] = (mean, rstd): small integer means and power-of-two rstd keep rstd * (acc - mean * c1) + b' one
        # exact real number in both spellings of the fold (a generator of its own: the other operands do not depend on the flag)
        assert family == "ternary" and prob.k == 1 and not prob.dgrad
        g2 = torch.Generator().manual_seed(5000 + salt)
        mean = torch.randint(LN_MEAN[0], LN_MEAN[1] + 1, (prob.M,), generator=g2).float()
        rstd = torch.tensor(LN_RSTD)[torch.randint(0, len(LN_RSTD), (prob.M,), generator=g2)]
        ln_stats = torch.stack([mean, rstd], dim=1)
    return dict(w=w, bias=bias, x=x, res=res, mask=mask, dx=dx, dw=dw, db=16 if family == "lattice" else 1, ln_stats=ln_stats)


LN_MEAN, LN_RSTD = (-3, 3), (0.25, 0.5, 1.0, 2.0)


def ln_c1(inp):
    """CF_LNFOLD: the column sums of the (folded) weights in natural column order; the packer permutes them for GEGLU"""
    return inp["w"].sum(dim=(1, 2, 3))


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


def epilogue(prob, acc, inp, mutant=None):
    """fp32 rows before the one rounding: mask(relu(alpha * fold(acc) + bias + res)), fold(acc) = rstd[m] * (acc - mean[m] * c1[n]) with
    "l"; with "g" / "G" the pre-activations in packed column order (geglu_product() makes y of them).  mutant: see STAT_MUTANTS"""
    v = acc
    if "l" in prob.fl:
        st, c1 = inp["ln_stats"], ln_c1(inp)
        if mutant == "ln_stats_of_the_neighbouring_row":
            st = st.clone()
            tail = torch.arange(prob.M - 64, prob.M)
            st[tail] = inp["ln_stats"][tail ^ 1]
        if mutant == "c1_in_natural_order":          # the kernel indexes c1 by PACKED column: natural values at packed positions
            assert "g" in prob.fl or "G" in prob.fl
            inv = torch.empty(prob.N, dtype=torch.long)
            inv[geglu_perm(prob.N)] = torch.arange(prob.N)
            c1 = c1[inv]                             # natural column perm[q] gets c1[q]
        v = st[:, 1:2] * (v - st[:, 0:1] * c1[None, :])
    v = v * prob.alpha if prob.alpha != 1.0 else v
    if inp["bias"] is not None:
        v = v + inp["bias"][None, :]
    if "g" in prob.fl or "G" in prob.fl:
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


# ---- the statistics epilogues, the LayerNorm fold and GEGLU on the ternary family -----------------------------------------------------

def _round32(fr):
    """a Fraction rounded to the nearest fp32 (ties to even), as a Fraction; normal range only"""
    if fr == 0:
        return fr
    e = 0
    a = abs(fr)
    while a >= (1 << 24):
        a /= 2
        e += 1
    while a < (1 << 23):
        a *= 2
        e -= 1
    assert e >= -149, "subnormal"
    return (round(a) * fractions.Fraction(2) ** e) * (1 if fr > 0 else -1)          # round(Fraction) rounds half to even


def gelu_literals():
    """(clamp, the ten coefficients) of gelu_poly_f, read from distdiff_amd/csrc/common.h as tests/test_oracle.py::test_gelu_polynomial does"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distdiff_amd", "csrc", "common.h")).read()
    clamp = float(re.search(r"#define\s+DD_GELU_CLAMP\s+([0-9.]+)f", src).group(1))
    body = re.search(r"#define\s+DD_GELU_POLY\s*\{(.*?)\}", src, re.S).group(1).replace("\\", " ")
    c = [float(torch.tensor(float(v.strip().rstrip("f")), dtype=torch.float32)) for v in body.split(",")]
    assert len(c) == 10
    return clamp, c


_PHI = {}


def gelu_phi(t):
    """Phi~(t) of gelu_poly_f for one clamped gate value t (a float that is exact in fp32): u = t * t, nine fmas, fma(t, p, 0.5), every
    operation formed exactly (fractions.Fraction; math.fma where Python has it gives the same) and rounded once to fp32"""
    if t not in _PHI:
        if "lit" not in _PHI:
            _PHI["lit"] = gelu_literals()
        clamp, c = _PHI["lit"]
        assert abs(t) <= clamp
        Fr = fractions.Fraction
        ft = Fr(t)
        u = _round32(ft * ft)
        p = Fr(c[9])
        for k in range(8, -1, -1):
            p = _round32(p * u + Fr(c[k]))
        _PHI[t] = float(_round32(ft * p + Fr(1, 2)))
    return _PHI[t]


GATE_LATTICE = 8            # the gate table: the multiples of 1 / 8 inside the clamp (integers; quarters under "l", eighths with alpha = 0.5)


def gate_table():
    """(clamp, Phi~ of every multiple of 1 / 8 in [-clamp, clamp] as fp32)"""
    if "table" not in _PHI:
        clamp = gelu_literals()[0]
        n = int(clamp * GATE_LATTICE)
        assert n == clamp * GATE_LATTICE
        _PHI["table"] = clamp, torch.tensor([gelu_phi(i / GATE_LATTICE) for i in range(-n, n + 1)], dtype=torch.float32)
    return _PHI["table"]


def gelu_exact(g):
    """gelu_poly_f on fp32 gates of the table's lattice: g * Phi~(clamp(g)), one fp32 rounding per operation (the product of two fp32
    numbers is exact in float64)"""
    clamp, table = gate_table()
    t = g.clamp(-clamp, clamp)
    idx = (t + clamp) * GATE_LATTICE
    assert torch.equal(idx, torch.round(idx)), "gate values outside the table (not multiples of 1 / %d)" % GATE_LATTICE
    return (g.double() * table[idx.long()].double()).float()


def geglu_product(prob, v, mutant=None):
    """y rows [M, N / 2] in fp32 of the packed pre-activations v (16 hidden | 16 gate columns per group of 32): round32(h * gelu_poly(g)).
    A zero keeps the sign of the product (a negative hidden value times gelu(0) = +0 is -0, and the kernels store that)"""
    M = v.shape[0]
    grp = v.reshape(M, prob.N // 32, 2, 16)
    h, g = grp[:, :, 0], grp[:, :, 1]
    if mutant == "last_gate_group_with_the_previous_hidden":
        h = h.clone()
        h[:, -1] = h[:, -2]
    return (h.double() * gelu_exact(g).double()).float().reshape(M, prob.N // 2)


def halo_tile_width(prob):
    """the halo kernels' tile width: the largest power-of-two factor of the output width (capped at 64 or 128 by the tile form; below 64
    the cap does not matter)"""
    wo = prob.out_hw[1]
    return wo & -wo


def slots_m64(prob):
    """CF_STATS slot of every output row: m >> 6 (every kernel but the narrow-tile halo forms)"""
    return torch.arange(prob.M) >> 6


def slots_halo(prob):
    """CF_STATS slot of every output row on the halo kernels: with tiles narrower than 64 pixels a block is 64 / tw image rows by tw
    pixels, slot (image's first row >> 6) + (oy // (64 / tw)) * tiles_x + ox // tw; from 64 pixels on it is m >> 6"""
    tw = halo_tile_width(prob)
    if tw >= 64:
        return slots_m64(prob)
    oh, ow = prob.out_hw
    m = torch.arange(prob.M)
    img, oy, ox = m // (oh * ow), (m // ow) % oh, m % ow
    return (img * oh * ow >> 6) + (oy // (64 // tw)) * (ow // tw) + ox // tw


def _block_sums(v, slot_of, mutant=None):
    """(a, q): [slots, N] float64 sums and sums of squares of the 64 rows of every slot"""
    M, N = v.shape
    nslots = M // 64
    assert M % 64 == 0 and torch.equal(torch.bincount(slot_of, minlength=nslots), torch.full((nslots,), 64)), "the slot map is not one-to-one"
    order = torch.argsort(slot_of, stable=True)
    blocks = v[order].double().reshape(nslots, 64, N)
    if mutant == "last_row_of_a_block_twice":
        blocks = blocks.clone()
        blocks[:, 62] = blocks[:, 63]
    return blocks.sum(1), (blocks * blocks).sum(1), order


def expected_stats(prob, v, slot_of, mutant=None):
    """CF_STATS: [M / 64, N, 2] fp32 (mean, M2) of the 64 rows of every slot, formed in fp32 as the emitters do: a = sum v, q = sum v^2,
    mean = a * (1 / 64), M2 = max(q - a * mean, 0).  v: epilogue()'s rows; slot_of: slots_m64 / slots_halo"""
    a64, q64, order = _block_sums(v, slot_of, mutant)
    a, q = a64.float(), q64.float()
    mean = a * (1.0 / 64.0)
    m2 = (q - a * mean).clamp_min(0)
    out = torch.stack([mean, m2], dim=2) + 0.0
    if mutant == "narrow_halo_tile_in_slot_m64":       # each block's partials land in slot (its first row >> 6): collisions, holes stay NaN
        first = order.reshape(-1, 64).min(1).values >> 6
        moved = torch.full_like(out, float("nan"))
        moved[first] = out
        return moved
    return out


def expected_rowpart(prob, v, spans, mutant=None):
    """CF_ROWSTATS: [M, len(spans), 2] fp32 (sum v, sum v^2) of every row over consecutive column spans of the given widths"""
    assert sum(spans) == v.shape[1] and "g" not in prob.fl and "G" not in prob.fl
    parts = torch.split(v.double(), list(spans), dim=1)
    out = torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], dim=1) for p in parts], dim=1).float()
    if mutant == "span_sums_in_the_neighbouring_span":
        out = out[:, torch.arange(len(spans)) ^ 1]
    return out


STATS_PAD, SPAN_PAD = 64, 3      # channels in front of the op's range in the partials buffer; spare span slots behind the op's spans


def expected_buffers(prob, acc, inp, dtype=torch.bfloat16, spans=None, slot_of=None, mutant=None):
    """{"y", "raw", "stats", "rowpart"}: every WHOLE buffer the launch of tests/conv_exact_cases.py::launch_args leaves, NaN wherever the
    kernel must not write, and "v", the fp32 rows the statistics are taken of.  stats: [M / 64, 64 + N, 2] with the partials in channels
    [64, 64 + N); rowpart: [M, len(spans) + 3, 2]"""
    fl = prob.fl
    nan = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt)
    v = epilogue(prob, acc, inp, mutant)
    out = dict(v=v)
    dt = store_dtype(prob, dtype)
    if "g" in fl or "G" in fl:
        yrows = geglu_product(prob, v, mutant)
        if "g" in fl:
            out["raw"] = v.to(dtype)
        out["y"] = yrows.to(dt)
    else:
        out["y"] = nan((prob.M, stored_width(prob)), dt)
        out["y"][:, :v.shape[1]] = v.to(dt)
    if "s" in fl:
        sv = epilogue(prob._replace(fl=fl.replace("u", "")), acc, inp) if mutant == "stats_in_front_of_the_relu" else v
        out["stats"] = nan((prob.M // 64, STATS_PAD + prob.N, 2), torch.float32)
        out["stats"][:, STATS_PAD:STATS_PAD + prob.N] = expected_stats(prob, sv, slot_of, mutant)
    if "w" in fl:
        out["rowpart"] = nan((prob.M, len(spans) + SPAN_PAD, 2), torch.float32)
        out["rowpart"][:, :len(spans)] = expected_rowpart(prob, v, spans, mutant)
    return out


# mutants of the statistics / fold / GEGLU epilogues (expected_buffers(mutant=...)): name, the flags a case needs, a further condition
STAT_MUTANTS = (
    ("last_row_of_a_block_twice", "s", lambda p: True),
    ("stats_in_front_of_the_relu", "su", lambda p: True),
    ("narrow_halo_tile_in_slot_m64", "s", lambda p: p.k == 3 and halo_tile_width(p) < 64 and p.out_hw[1] // halo_tile_width(p) > 1),
    ("ln_stats_of_the_neighbouring_row", "l", lambda p: True),
    ("c1_in_natural_order", "l", lambda p: "g" in p.fl or "G" in p.fl),
    ("last_gate_group_with_the_previous_hidden", "", lambda p: "g" in p.fl or "G" in p.fl),
    ("span_sums_in_the_neighbouring_span", "w", lambda p: True),
)


def check_stat_conditions(prob, inp, bufs, dtype=torch.bfloat16, spans=None, slot_of=None):
    """What the closed forms of the statistics outputs need, asserted per case (ternary): returns the bounds found"""
    fl, v = prob.fl, bufs["v"]
    found = {}
    lattice = 1 if "l" not in fl else (8 if "a" in fl else 4)
    if "a" in fl and "l" not in fl:
        lattice = 2
    assert torch.equal(v * lattice, torch.round(v * lattice)), "%s: v is not on the lattice 1 / %d" % (prob.name, lattice)
    found["max|v|"] = float(v.abs().max())
    assert found["max|v|"] * lattice < (1 << 24)
    if "l" in fl:
        st, c1 = inp["ln_stats"], ln_c1(inp)
        assert torch.equal(st[:, 0], torch.round(st[:, 0])) and LN_MEAN[0] <= st[:, 0].min() and st[:, 0].max() <= LN_MEAN[1]
        assert all(float(r) in LN_RSTD for r in st[:, 1].unique())
        # acc - mean * c1 is an integer below 2^24; rstd a power of two: exact in both spellings of the fold
        bound = prob.depth + LN_MEAN[1] * float(c1.abs().max())
        assert bound * max(LN_RSTD) * 8 < (1 << 24)
        found["fold bound"] = bound
    if "g" in fl or "G" in fl:
        g = v.reshape(prob.M, prob.N // 32, 2, 16)[:, :, 1]
        assert torch.equal(g * GATE_LATTICE, torch.round(g * GATE_LATTICE)), "%s: gates outside the table" % prob.name
        found["max|gate|"] = float(g.abs().max())
    if "s" in fl:
        assert lattice == 1 and torch.equal(v.to(dtype).float(), v), "%s: v is not exact in the stored format" % prob.name
        a, q, _o = _block_sums(v, slot_of)
        found["max|a|"], found["max q"] = float(a.abs().max()), float(q.max())
        assert found["max|a|"] ** 2 < (1 << 24) and found["max q"] < (1 << 24), (prob.name, found)
    if "w" in fl:
        assert lattice <= 2
        rp = expected_rowpart(prob, v, spans).double()
        found["max|span sum|"], found["max span sum of squares"] = float(rp[:, :, 0].abs().max()), float(rp[:, :, 1].max())
        assert found["max|span sum|"] * lattice < (1 << 24) and found["max span sum of squares"] * lattice * lattice < (1 << 24), (prob.name, found)
    return found


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
    (image, oy, ox, n) with got / want, whether all lie on an image border, their row index modulo the tile height; for a statistics
    buffer (three dimensions) the first eight as (block, channel) or (row, span) and which of the pair"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (prob.name, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(bits(got), bits(want)):
        return None
    bad = (bits(got) != bits(want)).nonzero()
    if got.dim() == 3:       # a statistics buffer [blocks | rows, channels | spans, 2]
        what = ("row", "span") if got.shape[0] == prob.M else ("block", "channel")
        lines = ["%s: %d of %d statistics differ (%d %ss, %d %ss touched)"
                 % (prob.name, len(bad), got.numel(), bad[:, 0].unique().numel(), what[0], bad[:, 1].unique().numel(), what[1])]
        for r, c, e in bad[:8].tolist():
            lines.append("  (%s %d, %s %d, %s): got %r want %r" % (what[0], r, what[1], c, ("first", "second")[e], float(got[r, c, e]), float(want[r, c, e])))
        lines.append("  %ss: %s%s" % (what[0], bad[:, 0].unique().tolist()[:16], " ..." if bad[:, 0].unique().numel() > 16 else ""))
        lines.append("  %ss: %s%s" % (what[1], bad[:, 1].unique().tolist()[:16], " ..." if bad[:, 1].unique().numel() > 16 else ""))
        return "\n".join(lines)
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
