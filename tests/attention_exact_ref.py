"""Closed-form reference for the attention kernels on EXACT inputs (CPU only, no library call).

Queries are one-hot, q_i = a e_g(i) with class g(i) < C <= min(D, 32) in the first C head dimensions, and keys carry one integer per
class, k_j[c] = t[j, c] (columns C .. D - 1 of K hold small integers no query reads), so q_i . k_j = a t[j, g(i)] exactly.  Every
(image, head) has its own t, g and v: a swapped head, image, row stride or column view changes the answer.  Two families:

  graded   a = 1, t in {0, -1 .. -depth} or INVISIBLE = -256, scale = ln 2 (fp32 ln 2 * fp32 log2 e is exactly 1.0f, so the kernels that
           scale the scores themselves and the ones that get a prescaled query see the same integers).  p = 2^(s - ref) is an exact power
           of two whatever reference the kernel uses (the running maximum, the lazy kernel's first-tile maximum, a rebased one) and
           2^-256 is 0 in fp32, so O l and l are exact in fp32 in every kernel and in every order.
  mask     t in {0, -b}, a and b powers of two with a b scale >= 256: the row maximum is 0 and every probability exactly 1 or 0 at any
           scale (the model's 1 / sqrt(D) included).

Values are integers in [-4, 4] (forward) or ternary (backward cases).  forward() computes acc and l in fp64, asserts they are exact in
fp32 and returns the stored bits of acc / l.  The kernels compute acc * (1.f / l): an element is DETERMINATE unless its exact quotient
lies within TAU = 2^-18 (relative) of a rounding boundary of the stored format (eight times the 2^-21 an online-softmax kernel's
fma(s, scale log2 e, -m) could leave in a row sum; the reciprocal and the product add 2^-23) -- exact ties with l a power of two stay
determinate (the kernel's quotient is exact then).  Determinate elements must match bit for bit, the others may be either neighbour.

Rows that do not depend on the query index (no causal mask) are computed once per class: the reference of a case with a thousand heads
is a few thousand softmax rows.

Backward cases (Case.bwd): every row's l is a power of two and every normalised probability >= 2^-G, v and dO are ternary with at most
DO_NONZEROS non-zeros per row and head; then O, delta, dP, dS = P (dP - delta) (at most 8 significant bits: the kernels' one rounding of
an approximate dS to the stored format has a unique result) and dV are exact, and dQ = scale dS K, dK = scale dS^T Q are exact sums through
one fp32 multiply and one rounding.  backward() asserts all of it.
"""
import collections
import math

import numpy as np
import torch

LN2 = 0.6931471805599453
INVISIBLE = -256
TAU = 2.0 ** -18
CAP = 0.02                      # largest share of indeterminate elements of a case
LSE_RTOL = 1e-5                 # |lse error| <= LSE_RTOL * max(1, |lse|): one hardware log2, one add, one multiply (about 5 fp32 ulps at 16)
LZ_LIMIT = 2.0 ** 64            # attention.hip, attn_fwd_dma_kernel: a row sum of the optimistic sweep at or beyond it sends the workgroup to the safe sweep
G = 3                           # backward cases: normalised probabilities >= 2^-G
DO_NONZEROS = 12                # ... and non-zeros of a dO row per head: |dP - delta| <= 24 < 2^(8 - G)
PATTERNS = ("riser", "late", "ragged", "single", "dense", "sparse")

# api: "attention" | "gemm" | "planned" (ops.attention / attention_gemm / attention_planned).  kt: keys per tile of the kernel the case is
# about (where the visibility patterns put their tile edges).  late: whether classes whose first tile is all invisible exist.  wide: q, k, v
# are column views of one fused projection (row stride 3 H D).  fwd / bwd: the plan the case is about (a dict of the fields of
# ops._attention_plan that matter, None: no backward).
_Case = collections.namedtuple("Case", "name api B H Nq Nk D family scale causal prescaled fp8 no_shortk wide ws_images need_dkv depth kt late "
                                        "f16 fwd bwd")


class Case(_Case):
    __slots__ = ()

    def __new__(cls, name, B, H, Nq, Nk, D, fwd, bwd=None, api="attention", family="graded", scale=None, causal=False, prescaled=False, fp8=False,
                no_shortk=False, wide=False, ws_images=0, need_dkv=True, depth=None, kt=64, late=True, f16=False):
        if scale is None:
            scale = LN2 if family == "graded" else 1.0 / math.sqrt(D)
        if depth is None:
            depth = 0 if family == "mask" else 2 if bwd is not None else 5 if fp8 else 7
        return super().__new__(cls, name, api, B, H, Nq, Nk, D, family, scale, causal, prescaled, fp8, no_shortk, wide, ws_images, need_dkv, depth, kt,
                               late, f16, fwd, bwd)

    @property
    def C(self):
        return min(self.D, 16)

    @property
    def flags(self):
        return {k: True for k in ("causal", "fp8", "no_shortk") if getattr(self, k)}


def mask_amplitudes(scale):
    """(a, b): powers of two, a b scale >= 256, both exact in bf16 and fp16"""
    e = math.ceil(math.log2(256.0 / scale) - 1e-9)
    return float(2 ** ((e + 1) // 2)), float(2 ** (e // 2))


def _force(vis, rng, where=None):
    """every (image, head) gets at least one visible key: a random one (among `where`) is switched on"""
    B, H, Nk = vis.shape
    w = rng.random((B, H, Nk))
    if where is not None:
        w = np.where(where, w, -1.0)
    j = w.argmax(-1)
    np.put_along_axis(vis, j[..., None], True, axis=-1)
    return j


def make_inputs(case, seed):
    """{"t": int64 [B, H, Nk, C] (INVISIBLE / -b: not visible), "g": int64 [B, H, Nq], "v": fp64 [B, H, Nk, D], "junk": fp64 [B, H, Nk, D - C]
    (K columns no query reads), "a", "b", and for backward cases "d_o": fp64 [B, H, Nq, D]}"""
    B, H, Nq, Nk, D, C = case.B, case.H, case.Nq, case.Nk, case.D, case.C
    rng = np.random.default_rng(seed)
    a, b = (1.0, 256.0) if case.family == "graded" else mask_amplitudes(case.scale)
    g = rng.integers(0, C, (B, H, Nq))
    n = min(C, Nq)
    g[:, :, :n] = np.argsort(rng.random((B, H, C)), -1)[:, :, :n]       # every class has a query wherever Nq allows
    tile = np.arange(Nk) // case.kt
    last = tile == tile[-1]
    lev = rng.integers(0, case.depth + 1, (B, H, Nk, C))
    vis = np.zeros((B, H, Nk, C), dtype=bool)
    if case.bwd is not None or case.fwd["route"] == "gemm":
        # power-of-two row sums: 2^m keys at level 0, or (graded) the ladder 0, -1, -2, -2; in backward cases one key in eight is seen by no class
        seen = rng.random((B, H, Nk, 1)) >= (0.125 if case.bwd is not None else 0.0)
        seen[:, :, 0] = seen[:, :, -1] = True
        r = rng.random((B, H, Nk, C))
        r[:, :, -1, 1::2] = -1.0                 # every other class sees the last key: the ragged edge of the backward kernels' tiles
        rank = np.argsort(np.argsort(np.where(seen, r, 2.0), 2), 2)
        avail = int(seen.sum(2).min())
        top = min(G if case.bwd is not None else 12, int(math.log2(avail)))
        for c in range(C):
            if case.family == "graded" and c % 4 == 2 and avail >= 4:
                vis[..., c] = rank[..., c] < 4
                lev[..., c] = np.minimum(rank[..., c], 2)
            else:
                vis[..., c] = rank[..., c] < (1 << (c % (top + 1)))
                lev[..., c] = 0
    else:
        pats = [p if (p != "late" or case.late) else "sparse" for p in PATTERNS]
        for c in range(C):
            pat = pats[c % len(pats)]
            if pat == "late" and tile[-1] == 0:
                pat = "single"
            if pat == "riser":           # the row maximum rises by one with every tile (the first key of a tile carries the tile's top level)
                topl = np.maximum(0, case.depth - tile)[None, None, :]
                lev[..., c] = topl + (lev[..., c] % (case.depth - topl + 1))
                vis[..., c] = rng.random((B, H, Nk)) < 0.5
                first = np.arange(Nk) % case.kt == 0
                vis[..., first, c] = True
                lev[..., first, c] = np.broadcast_to(topl, (B, H, Nk))[..., first]
            elif pat == "late":          # the first tile is all invisible
                v = (rng.random((B, H, Nk)) < 0.5) & (tile >= 1)
                _force(v, rng, np.broadcast_to(tile >= 1, (B, H, Nk)))
                vis[..., c] = v
            elif pat == "ragged":        # only keys of the last (ragged) tile
                vis[..., c] = last
            elif pat == "single":
                v = np.zeros((B, H, Nk), dtype=bool)
                _force(v, rng)
                vis[..., c] = v
            elif pat == "dense":
                vis[..., c] = True
            else:
                v = rng.random((B, H, Nk)) < 0.125
                _force(v, rng)
                vis[..., c] = v
        if case.causal or not case.late:
            vis[:, :, 0, :] = True       # every causal row sees key 0; late = False: no class at all whose first tile is all invisible
    t = np.where(vis, -lev * (1 if case.family == "graded" else 0), INVISIBLE if case.family == "graded" else -int(b))
    if case.bwd is not None:
        v = rng.integers(-1, 2, (B, H, Nk, D))
        nz = min(DO_NONZEROS, D // 2)
        d_o = (np.argsort(np.argsort(rng.random((B, H, Nq, D)), -1), -1) < nz) * (rng.integers(0, 2, (B, H, Nq, D)) * 2 - 1)
    else:
        v = rng.integers(-4, 5, (B, H, Nk, D))
        d_o = None
    junk = rng.integers(-4, 5, (B, H, Nk, D - C))
    T = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    return dict(t=T(t.astype(np.int64)), g=T(g.astype(np.int64)), v=T(v.astype(np.float64)), junk=T(junk.astype(np.float64)), a=a, b=b,
                d_o=T(None if d_o is None else d_o.astype(np.float64)), vis=T(vis))


def rows(case, inp, dtype=torch.bfloat16, device="cpu"):
    """the kernels' operands: q [B Nq, H D], k, v [B Nk, H D] (and d_o) in the stored format; with case.wide column views of one
    [rows, 3 H D] buffer (Nq == Nk)"""
    B, H, Nq, Nk, D, C = case.B, case.H, case.Nq, case.Nk, case.D, case.C
    g = inp["g"].to(device)
    q = torch.zeros((B, H, Nq, D), dtype=dtype, device=device)
    q.scatter_(3, g[..., None], inp["a"])
    k = torch.cat([inp["t"].to(dtype), inp["junk"].to(dtype)], -1).to(device)
    v = inp["v"].to(dtype).to(device)
    flat = lambda x, n: x.permute(0, 2, 1, 3).reshape(B * n, H * D)
    q, k, v = flat(q, Nq), flat(k, Nk), flat(v, Nk)
    if case.wide:
        assert Nq == Nk
        w = torch.cat([q, k, v], 1)
        q, k, v = w[:, :H * D], w[:, H * D:2 * H * D], w[:, 2 * H * D:]
    else:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    d_o = None if inp["d_o"] is None else flat(inp["d_o"].to(dtype).to(device), Nq).contiguous()
    return q, k, v, d_o


def scores(case, inp):
    """(s fp64 [B, H, U, Nk] in units of the raw score (masked: -inf), idx int64 [B, H, Nq]): row idx[b, h, i] of s is query i's.  Without a
    causal mask U = C (one row per class), with one U = Nq"""
    s = inp["a"] * inp["t"].double().transpose(2, 3)
    if not case.causal:
        return s, inp["g"]
    s = torch.gather(s, 2, inp["g"][..., None].expand(-1, -1, -1, case.Nk))
    hidden = torch.ones(case.Nq, case.Nk).triu(1).bool()
    return s.masked_fill(hidden, -math.inf), torch.arange(case.Nq).expand(case.B, case.H, -1)


def _probs(case, s, m):
    e = s - m[..., None]
    if case.family == "graded":
        assert bool(((e >= -case.depth) | (e <= -150)).all()), case.name
        return torch.where(e >= -case.depth, torch.exp2(e), torch.zeros(()).double())
    assert bool(((e == 0) | (e * case.scale <= -256)).all()), case.name
    return (e == 0).double()


# ---- mutants of the reference: each stands for a fault of a kernel that the exact comparison must see -------------------------------------
# mutant(case, inp, s, v) -> (m, acc, l) of the faulty kernel, or None where it does not apply

def _sums(case, s, v, m=None):
    m = s.max(-1).values if m is None else m
    p = _probs(case, s, m)
    return m, p @ v, p.sum(-1)


def most_seen_key(case, inp):
    n = inp["vis"][0, 0].sum(-1)
    if case.causal and case.Nk > 1:
        n[0] = -1                     # (key 0 is all the first causal row has)
    return int(n.argmax())


def mutant_dropped_key(case, inp, s, v):
    """one key (the one most classes of the first head see) never reaches the softmax"""
    s = s.clone()
    s[:, :, :, most_seen_key(case, inp)] = -math.inf
    if bool(torch.isinf(s.max(-1).values).any()):
        return None
    return _sums(case, s, v)


def mutant_unmasked_ragged_tile(case, inp, s, v):
    """the keys behind Nk in the last tile are not masked: zero rows of K (score 0) and of V"""
    pad = -case.Nk % case.kt
    if pad == 0:
        return None
    s = torch.cat([s, torch.zeros(s.shape[:-1] + (pad,)).double()], -1)
    v = torch.cat([v, torch.zeros(v.shape[:-2] + (pad, v.shape[-1])).double()], -2)
    m = s.max(-1).values
    e = s - m[..., None]
    p = torch.where(e > -150, torch.exp2(e), torch.zeros(()).double()) if case.family == "graded" else (e == 0).double()
    return m, p @ v, p.sum(-1)


def mutant_next_heads_v(case, inp, s, v):
    """P.V reads the value rows of the next head (of the next image where there is one head)"""
    if case.H == 1 and case.B == 1:
        return None
    return _sums(case, s, torch.roll(v, -1, 1 if case.H > 1 else 0))


def mutant_no_rescale(case, inp, s, v):
    """the online softmax never rescales what it has when the maximum moves after tile 0: every tile's terms stay relative to the running
    maximum of their own tile"""
    if case.Nk <= case.kt:
        return None
    run = torch.cummax(torch.stack([c.max(-1).values for c in s.split(case.kt, -1)], -1), -1).values        # [B, H, U, tiles]
    if bool((run[..., 0] == run[..., -1]).all()):
        return None
    acc, l = 0.0, 0.0
    for i, (sc, vc) in enumerate(zip(s.split(case.kt, -1), v.split(case.kt, -2))):
        e = sc - run[..., i, None]
        p = torch.where(e > -150, torch.exp2(e), torch.zeros(()).double()) if case.family == "graded" else (e == 0).double()
        acc, l = acc + p @ vc, l + p.sum(-1)
    return run[..., -1], acc, l


def mutant_rounded_row_sum(case, inp, s, v):
    """the row sum is kept in the 16-bit format where the kernel keeps fp32 (every term is a power of two and survives the rounding: what
    can go wrong is the sum itself)"""
    m, acc, l = _sums(case, s, v)
    lr = l.float().to(torch.bfloat16).double()
    return None if bool((lr == l).all()) else (m, acc, lr)


MUTANTS = (("dropped_key", mutant_dropped_key), ("unmasked_ragged_tile", mutant_unmasked_ragged_tile), ("next_heads_v", mutant_next_heads_v),
           ("no_rescale", mutant_no_rescale), ("rounded_row_sum", mutant_rounded_row_sum))


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

def _from_bits(mag, dtype):
    return mag.to(torch.int16).view(dtype)


def round_stored(x, l_pow2, dtype):
    """x fp64 (the exact quotients) -> (want, alt, indeterminate): the stored bits (int16), the other admissible neighbour (= want where the
    element is determinate) and the mask of the indeterminate elements"""
    want = x.float().to(dtype)
    bits = want.view(torch.int16).to(torch.int32) & 0xffff
    mag, sign = bits & 0x7fff, bits & 0x8000
    ax, y = x.abs(), want.double().abs()
    up, dn = _from_bits(mag + 1, dtype).double(), _from_bits((mag - 1).clamp_min(0), dtype).double()
    du, dd = ((y + up) / 2 - ax).abs(), (ax - (y + dn) / 2).abs()
    dist = torch.minimum(du, dd)
    ind = (dist <= TAU * ax) & (ax > 0) & ~((dist == 0) & l_pow2)
    alt = torch.where(ind, torch.where(du <= dd, mag + 1, mag - 1) | sign, bits)
    tr = lambda b: torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
    return tr(bits), tr(alt), ind


def is_pow2(l):
    return torch.frexp(l)[0] == 0.5


Forward = collections.namedtuple("Forward", "want alt ind lse idx m acc l share")


def forward(case, inp, dtype=torch.bfloat16, mutant=None):
    """want, alt int16 [B, H, U, D], ind bool, lse fp64 [B, H, U], idx [B, H, Nq] (scores()), m / acc / l the exact sums, share: the
    indeterminate share of the case's elements (every query row counted).  Asserts the exactness conditions."""
    s, idx = scores(case, inp)
    v = inp["v"]
    if mutant is None:
        m, acc, l = _sums(case, s, v)
        unit = 2.0 ** case.depth
        big = max(float((_probs(case, s, m) @ v.abs()).max()), float(l.max()))
        assert big * unit < 2 ** 24, "%s: sums up to %g units of 2^-%d are not exact in fp32" % (case.name, big * unit, case.depth)
        assert bool((l >= 1).all())
    else:
        out = mutant(case, inp, s, v)
        if out is None:
            return None
        m, acc, l = out
    want, alt, ind = round_stored(acc / l[..., None], is_pow2(l)[..., None], dtype)
    lse = m * case.scale + torch.log(l)                       # (max + log2 l) ln 2 for the graded family
    share = float(torch.gather(ind.double().mean(-1), 2, idx).mean())
    return Forward(want, alt, ind, lse, idx, m, acc, l, share)


def expand(table, idx):
    """per-row table [B, H, U, ...] -> rows of the kernels' layout: [B Nq, H * D] (or [B, H, Nq] for a table without columns)"""
    B, H, Nq = idx.shape
    if table.dim() == 3:
        return torch.gather(table, 2, idx)
    D = table.shape[-1]
    full = torch.gather(table, 2, idx[..., None].expand(-1, -1, -1, D))
    return full.permute(0, 2, 1, 3).reshape(B * Nq, H * D)


def lse_tolerance(lse, Nk):
    """LSE_RTOL * max(1, |lse|), and never more than a tenth of log(Nk / (Nk - 1)), the least a flat row's LSE moves when one key is lost
    (that only bites beyond 4000 keys)"""
    tol = LSE_RTOL * lse.abs().clamp_min(1.0)
    return tol if Nk < 2 else tol.clamp_max(math.log(Nk / (Nk - 1.0)) / 10)


def needs_safe_sweep(case, inp):
    """bool [B, H, U]: rows whose optimistic row sum -- the reference is the first tile's maximum and never moves -- reaches LZ_LIMIT (or
    overflows), so that attn_fwd_dma_kernel<.., LZ = true> must repeat the sweep with the per-tile maximum"""
    s, _idx = scores(case, inp)
    ref = s[..., :case.kt].max(-1).values
    return ~(torch.exp2(s - ref[..., None]).sum(-1) < LZ_LIMIT)


def wrong_elements(got_bits, fw):
    """bool [B Nq, H D]: elements of the kernel's output (int16 bits) that are neither the stored value nor, where indeterminate, its neighbour"""
    want, alt = expand(fw.want.to(got_bits.device), fw.idx.to(got_bits.device)), expand(fw.alt.to(got_bits.device), fw.idx.to(got_bits.device))
    return (got_bits != want) & (got_bits != alt)


def mismatch_report(case, inp, wrong, got=None, want=None, what="O", rows_are="query"):
    """None if nothing is wrong, else a text: the count of wrong elements, the first eight as (image, head, query, column) with got / want,
    the query index modulo 16 and 32, and whether every wrong row sees keys of a single key tile only"""
    wrong = wrong.cpu()
    if not bool(wrong.any()):
        return None
    n = wrong.shape[0] // case.B
    bad = wrong.nonzero()
    r, c = bad[:, 0], bad[:, 1]
    img, row, head, col = r // n, r % n, c // case.D, c % case.D
    lines = ["%s %s: %d of %d elements differ (%d rows, %d heads touched)" % (case.name, what, len(bad), wrong.numel(), r.unique().numel(), (img * case.H + head).unique().numel())]
    for i in range(min(8, len(bad))):
        extra = "" if got is None else ": got %r want %r" % (float(got[r[i], c[i]]), float(want[r[i], c[i]]))
        lines.append("  (image %d, head %d, %s %d, column %d)%s" % (img[i], head[i], rows_are, row[i], col[i], extra))
    mods = lambda n: (lambda u: "all %d residues" % n if len(u) == n else str(u))((row % n).unique().tolist())
    lines.append("  %s index mod 16: %s   mod 32: %s" % (rows_are, mods(16), mods(32)))
    if rows_are == "query":
        vis = inp["vis"][img, head, :, inp["g"][img, head, row]]                       # [wrong elements, Nk]
        if case.causal:
            vis = vis & (torch.arange(case.Nk)[None, :] <= row[:, None])
        tile = torch.arange(case.Nk) // case.kt
        lo = torch.where(vis, tile, tile[-1] + 1).min(-1).values
        hi = torch.where(vis, tile, -1).max(-1).values
        lines.append("  every wrong row sees keys of a single key tile only: %s (tiles of %d keys; first / last visible tile of the wrong rows: %s / %s)"
                     % (bool((lo == hi).all()), case.kt, lo.unique().tolist()[:12], hi.unique().tolist()[:12]))
    else:
        lines.append("  key tiles of %d: %s" % (case.kt, (row // case.kt).unique().tolist()[:16]))
    return "\n".join(lines)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------

Backward = collections.namedtuple("Backward", "dq dk dv unseen")


def backward(case, inp, fw, dtype=torch.bfloat16):
    """dq [B Nq, H D], dk, dv [B Nk, H D] in the stored format (the bits are the reference), unseen bool [B, H, Nk]: keys no query sees
    (their dK and dV rows are +0).  Asserts the conditions of the module docstring."""
    B, H, Nq, Nk, D, C = case.B, case.H, case.Nq, case.Nk, case.D, case.C
    assert not case.causal and not bool(fw.ind.any())
    assert bool(is_pow2(fw.l).all()), "%s: a row sum is no power of two" % case.name
    ex = lambda tab: torch.gather(tab, 2, fw.idx[..., None].expand(-1, -1, -1, tab.shape[-1]))
    s, _ = scores(case, inp)
    P = ex(_probs(case, s, fw.m) / fw.l[..., None])                                        # [B, H, Nq, Nk]
    assert bool(((P == 0) | (P >= 2.0 ** -G)).all()), "%s: a probability below 2^-%d" % (case.name, G)
    O = ex(fw.want.view(dtype).double())
    assert torch.equal(O, ex(fw.acc / fw.l[..., None])), "%s: O is not exact in %s" % (case.name, dtype)
    v, d_o = inp["v"], inp["d_o"]
    assert bool((v.abs() <= 1).all()) and bool((d_o.abs() <= 1).all()) and int((d_o != 0).sum(-1).max()) <= DO_NONZEROS
    dP = d_o @ v.transpose(2, 3)
    delta = (d_o * O).sum(-1, keepdim=True)
    assert float((dP - delta).abs().max()) < 2.0 ** (8 - G)
    dS = P * (dP - delta)
    assert torch.equal(dS.float().to(dtype).double(), dS), "%s: dS has more than 8 significant bits" % case.name
    K = torch.cat([inp["t"].double(), inp["junk"]], -1)
    Q = torch.zeros((B, H, Nq, D), dtype=torch.float64).scatter_(3, inp["g"][..., None], inp["a"])
    unit = 4.0 ** G
    for a_, b_ in ((dS.abs(), K.abs()), (dS.abs().transpose(2, 3), Q.abs()), (P.transpose(2, 3), d_o.abs())):
        assert float((a_ @ b_).max()) * unit < 2 ** 24, "%s: a gradient sum is not exact in fp32" % case.name
    if case.api == "gemm" or case.bwd.get("route") == "gemm":
        assert math.frexp(case.scale)[0] == 0.5, "the GEMM route scales dS before its rounding: only a power-of-two scale leaves the bits unique"
    sc = torch.tensor(case.scale, dtype=torch.float32)
    flat = lambda x, n: ((x + 0.0).permute(0, 2, 1, 3).reshape(B * n, H * D))
    dq = flat(((dS @ K).float() * sc).to(dtype), Nq)
    dk = flat(((dS.transpose(2, 3) @ Q).float() * sc).to(dtype), Nk)
    dv = flat((P.transpose(2, 3) @ d_o).float().to(dtype), Nk)
    unseen = ~(P > 0).any(2)
    return Backward(dq, dk, dv, unseen)


def bits(t):
    return t.contiguous().view(torch.int16)
