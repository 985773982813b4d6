"""CPU checks of the counter-based noise (--noise_rng philox) and of --text_to_img on the host side: a pure-Python / numpy restatement of
Philox4x32-10 pinned to the published Random123 known answers (the GPU tests hold the kernel to this restatement), the CLI flags, and
the packing independence of what the loop hands to the engine, against a recording fake engine (no GPU)."""
import os

import numpy as np
import pytest
import torch

from distdiff_amd import generate_data as G
from distdiff_amd.config import tiny_config
from distdiff_amd.scheduler import DDIMSchedule

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Salmon et al., Random123: 10 rounds of (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
    key bumped by the Weyl constants after each round.  Plain Python integers."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_words(seed, stream, uid, n_blocks):
    """The same, vectorised over blocks q = 0 .. n_blocks-1 of one unit: uint32 [n_blocks, 4], counter (q, stream, uid lo, uid hi),
    key (seed lo, seed hi)."""
    c0 = np.arange(n_blocks, dtype=np.uint64) & MASK
    c1 = np.full(n_blocks, stream, dtype=np.uint64)
    c2 = np.full(n_blocks, uid & MASK, dtype=np.uint64)
    c3 = np.full(n_blocks, (uid >> 32) & MASK, dtype=np.uint64)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def unit_values(seed, stream, uid, n):
    """float64 values of one unit's tensor of n elements, as include/distdiff_hip.h (dd_randn_units) defines them: stream 2 uniform
    (w >> 8) 2^-24, else Box-Muller on the word pairs (w0, w1) and (w2, w3) with u = (w + 0.5) 2^-32."""
    w = philox_words(seed, stream, uid, (n + 3) // 4)
    if stream == 2:
        v = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    else:
        u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
        v = np.empty(w.shape, np.float64)
        for a in (0, 2):
            r = np.sqrt(-2.0 * np.log(u[:, a]))
            v[:, a], v[:, a + 1] = r * np.cos(2 * np.pi * u[:, a + 1]), r * np.sin(2 * np.pi * u[:, a + 1])
    return v.reshape(-1)[:n]


MOMENT_SEED = 20240917          # test_noise_rng_gpu.py holds the kernel to the same three bounds at this seed
MOMENT_N = 1 << 22


def moments(x):
    x = np.asarray(x, np.float64)
    m = x.mean()
    v = ((x - m) ** 2).mean()
    return m, v, ((x - m) ** 4).mean() / v ** 2


def moment_bounds(n):
    """Five standard errors of the sample mean, variance and kurtosis of n independent N(0,1) draws."""
    return 5 / np.sqrt(n), 5 * np.sqrt(2.0 / n), 5 * np.sqrt(24.0 / n)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((MASK,) * 4, (MASK, MASK), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % w for w in philox4x32_10(ctr, key)) == want
    # the vectorised form the GPU tests use is the same function
    seed, uid = 0x299f31d0a4093822, (0x03707344 << 32) | 0x13198a2e
    w = philox_words(seed, 0x85a308d3, uid, 0x243f6a88 % 1000 + 1)
    for q in (0, 1, 17, w.shape[0] - 1):
        assert tuple(int(x) for x in w[q]) == philox4x32_10((q, 0x85a308d3, uid & MASK, uid >> 32), (seed & MASK, seed >> 32))


def test_restatement_moments_at_the_gpu_tests_seed():
    x = unit_values(MOMENT_SEED, 0, 5, MOMENT_N)
    m, v, k = moments(x)
    bm, bv, bk = moment_bounds(MOMENT_N)
    print("restatement moments: mean %.3e (bound %.3e), var-1 %.3e (%.3e), kurt-3 %.3e (%.3e)" % (m, bm, v - 1, bv, k - 3, bk))
    assert abs(m) <= bm and abs(v - 1) <= bv and abs(k - 3) <= bk
    e = unit_values(MOMENT_SEED, 2, 5, 4096)
    assert e.min() >= 0.0 and e.max() < 1.0


def test_cli_flags():
    a = G.parse_args([])
    assert a.noise_rng == "stream" and a.text_to_img is False
    a = G.parse_args(["--text_to_img", "--synthetic", "4", "--tiny"])          # was refused with SystemExit
    assert a.text_to_img is True and a.noise_rng == "stream"
    assert G.parse_args(["--noise_rng", "philox"]).noise_rng == "philox"
    with pytest.raises(SystemExit):
        G.parse_args(["--noise_rng", "mt19937"])


def test_unit_id_is_injective():
    assert G.unit_id(0, 0) == 0 and G.unit_id(1, 0) == 1 << 32 and G.unit_id(0, 1) == 1 and G.unit_id(3, 7) == (3 << 32) | 7
    rng = np.random.default_rng(0)
    edge = [0, 1, 2, 2 ** 16, 2 ** 31 - 2, 2 ** 31 - 1]
    pairs = {(i, j) for i in edge for j in edge} | {(int(i), int(j)) for i, j in rng.integers(0, 2 ** 31, (4000, 2))}
    ids = {G.unit_id(i, j) for i, j in pairs}
    assert len(ids) == len(pairs) and all(0 <= u < 2 ** 64 for u in ids)
    # and it inverts: the pair can be read back from the id
    assert all((G.unit_id(i, j) >> 32, G.unit_id(i, j) & MASK) == (i, j) for i, j in pairs)
    with pytest.raises(ValueError):
        G.unit_id(-1, 0)


class RecordingEngine:
    """test_cli.py's FakeEngine with the new keywords: records, per row that is written, what the engine was asked to generate from."""
    device = torch.device("cpu")

    def __init__(self, B):
        self.B, self.calls = B, []

    def set_prompt(self, emb):
        pass

    def expand(self, lat, noise, e, b, tg, si, gt, gfirst, gcount, want_image=True, **kw):
        self.calls.append(dict(lat=lat, noise=noise, e=e, b=b, si=si, gt=gt, kw=kw))
        return (lat.clone() if lat is not None else None), torch.rand(self.B, 3, 16, 16), torch.tensor([1.25])


def _run(tmp_path, name, extra, EB, n=7, existing=()):
    cfg = tiny_config(max_batch=EB)
    ds = G.ExpansionDataset.synthetic(cfg, n=n, n_classes=2, seed=0)
    sched = DDIMSchedule(cfg.scheduler)
    sched.set_timesteps(50)
    out = str(tmp_path / name)
    args = G.parse_args(["--synthetic", str(n), "--output_dir", out, "--train_batch_size", "1", "--num_images_per_prompt", "2",
                         "--guidance_type", "transform_guidance", "--guidance_step", "20", "--guidance_period", "2", "--strength", "0.5",
                         "--seed", "1234"] + extra)
    for rel in existing:
        p = os.path.join(out, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "wb").close()
    eng = RecordingEngine(EB)
    written = []
    G.run_expansion(args, eng, sched, ds, writer=lambda img, p: written.append(os.path.relpath(p, out)))
    handed = {}
    for c, paths in zip(eng.calls, [written[k:k + EB] for k in range(0, len(written), EB)]):
        for row, p in enumerate(paths):
            assert p not in handed
            handed[p] = (c["kw"].get("seed"), c["kw"]["unit_ids"][row] if "unit_ids" in c["kw"] else None)
    return handed, eng.calls


def test_packing_independence_of_engine_inputs(tmp_path):
    ph = ["--noise_rng", "philox", "--total_split", "1", "--split", "0"]
    base, calls = _run(tmp_path, "a", ph, EB=2)
    assert len(base) == 14 and all(s == 1234 for s, _ in base.values())
    assert sorted(u for _, u in base.values()) == sorted(G.unit_id(i, j) for i in range(7) for j in range(2))
    assert all(c["noise"] is None and c["kw"]["offset_noise"] is False and "text_to_img" not in c["kw"] for c in calls)
    # (a) another engine batch
    assert _run(tmp_path, "b", ph, EB=4)[0] == base
    # (b) as two shards
    halves = {}
    for k in (0, 1):
        part = _run(tmp_path, "c%d" % k, ["--noise_rng", "philox", "--total_split", "2", "--split", str(k)], EB=2)[0]
        assert not set(part) & set(halves)
        halves.update(part)
    assert halves == base
    # (c) resumed: half of the PNGs exist, the rest get exactly the pairs of the fresh run
    done = sorted(base)[::3]
    rest = _run(tmp_path, "d", ph, EB=2, existing=done)[0]
    assert set(rest) == set(base) - set(done) and all(rest[p] == base[p] for p in rest)
    # --first_image_index leaves the later units alone as well
    later = _run(tmp_path, "e", ph + ["--first_image_index", "1"], EB=4)[0]
    assert later == {p: v for p, v in base.items() if p.endswith("_expand_1.png")}


def test_stream_mode_calls_are_todays(tmp_path):
    """Default mode: no new keyword reaches the engine (test_cli.py's FakeEngine takes none), and the host draws are the ones of the parent
    commit's loop -- restated here: one generator seeded with --seed, one randn of the batch shape per engine batch."""
    handed, calls = _run(tmp_path, "s", ["--total_split", "1", "--split", "0"], EB=2)
    assert len(calls) == 7 and all(c["kw"] == {} for c in calls) and all(v == (None, None) for v in handed.values())
    g = torch.Generator().manual_seed(1234)
    L = tiny_config(max_batch=2).latent_size
    for c in calls:
        assert torch.equal(c["noise"], torch.randn((2, 4, L, L), generator=g)) and c["si"] == 25 and c["lat"] is not None


def test_text_to_img_loop(tmp_path):
    for extra, philox in ((["--text_to_img"], False), (["--text_to_img", "--noise_rng", "philox", "--offset_noise"], True)):
        handed, calls = _run(tmp_path, "t%d" % philox, extra + ["--total_split", "1", "--split", "0"], EB=4)
        assert len(handed) == 14 and len(calls) == 4
        for c in calls:
            assert c["si"] == 0 and c["lat"] is None and c["kw"]["text_to_img"] is True and c["gt"] == "transform_guidance"
            if philox:
                assert c["noise"] is None and c["kw"]["seed"] == 1234 and len(c["kw"]["unit_ids"]) == 4 and c["kw"]["offset_noise"] is False
            else:
                L = tiny_config(max_batch=4).latent_size
                assert tuple(c["noise"].shape) == (4, 4, L, L)
                assert "seed" not in c["kw"]
