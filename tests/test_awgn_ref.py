"""The test of the tests of the noise: tests/awgn_ref.py, the float64 twin of the AWGN channel, the modulator's noise and the random source,
on the CPU --

a. its Philox4x32-10 against the three known answers of Random123's kat_vectors, its float32 uniforms against exact integer arithmetic;
b. the distribution it claims, on fixed seeds and 2^22 samples and more per statistic, every bar 4.5 standard errors of the statistic under
   N(0, 1) (the seeds are fixed: a condition verified once, not a flake rate);
c. the bars of tests/test_awgn_gpu.py (awgn_ref.check) against twelve mistakes a kernel could make, each put into a copy of the TWIN that then
   stands in for the device, rounded to float32: without a mistake every bar is met, with any of them a named bar is missed;
d. the edge-seed fixture tests/golden/awgn_edge_seeds.json (tools/awgn_edges.py) re-derived entry by entry;
e. the share of near-1 samples in every case of the GPU test, which is a property of its seeds alone."""
import json
import math
import os

import numpy as np
import pytest

import awgn_ref as R

SE = 4.5
S0 = (7 << 40) + (3 << 8) + 5                    # the simulator's form of a seed: both key halves in use
EDGES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "awgn_edge_seeds.json")))


# ---------------------------------------------------------------------------------------------------------------- a
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in R.philox4x32_10(ctr, key)) == want
    # vectorised over counters and keys alike, and the seed's halves go where the kernels put them
    ctr = [np.array([k[0][i] for k in KAT], np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT], np.uint64) for i in range(2)]
    got = np.stack(R.philox4x32_10(ctr, key)).T
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]
    seed = (0x299f31d0 << 32) | 0xa4093822
    w = R.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), R.STAGES["key"](seed))
    assert tuple(int(v) for v in w) == KAT[2][2]
    assert tuple(int(v[3, 5]) for v in R.words(2, 8, 4, seed)) == tuple(int(v) for v in R.philox4x32_10((5, 3, 2, 0), (0xa4093822, 0x299f31d0)))


def _rne24(n):
    """the integer n rounded to 24 significant bits, ties to even: what a float32 holds of it"""
    if n < 1 << 24:
        return n
    sh = n.bit_length() - 24
    q, rem = divmod(n, 1 << sh)
    if rem > 1 << (sh - 1) or (rem == 1 << (sh - 1) and q & 1):
        q += 1
    return q << sh


def test_uniforms_are_the_kernels_float32_bit_for_bit():
    rng = np.random.default_rng(1)
    ws = [0, 1, 2, 199, 200, 255, 256, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 31) - 64, (1 << 31) + 128, (1 << 31) + 384,
          2 ** 32 - 385, 2 ** 32 - 384, 2 ** 32 - 383, 2 ** 32 - 257, 2 ** 32 - 256, 2 ** 32 - 255, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 127, 2 ** 32 - 1]
    ws += [int(v) for v in rng.integers(0, 2 ** 32, 2000)]
    w = np.array(ws, np.uint64)
    u1, u2 = R.STAGES["u_radius"](w), R.STAGES["u_angle"](w)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    for i, v in enumerate(ws):
        assert float(u1[i]) * 2.0 ** 32 == _rne24(_rne24(v) + 1), v
        assert float(u2[i]) * 2.0 ** 32 == _rne24(v), v
    assert float(u1.min()) == 2.0 ** -32 and u1.max() == 1 and u2.min() == 0 and u2.max() == 1
    top = np.arange(2 ** 32 - 400, 2 ** 32, dtype=np.uint64)
    one = top >= np.uint64(2 ** 32 - 128)                               # 2^32 - 128 is the tie between 2^32 - 256 and 2^32, and goes to the even 2^32
    assert np.array_equal(R.STAGES["u_radius"](top) == 1, one) and np.array_equal(R.STAGES["u_angle"](top) == 1, one)
    below = R.edge_class("A2", top)                                      # (2^32 - 384 is a tie as well, and goes down to the even 2^32 - 512)
    assert np.all(R.STAGES["u_radius"](top)[below] == np.float32(1 - 2.0 ** -24)) and np.all(R.STAGES["u_radius"](top)[~below & ~one] < np.float32(1 - 2.0 ** -24))
    # the ends of the map: no noise at u1 = 1, the largest radius at word 0, a whole revolution at u2 = 1
    z, rad = R.normals(2, 4, 1, 0, dict(R.STAGES, u_radius=lambda w: np.array([[1.0, 2.0 ** -32, 0.5, 0.5]], np.float32), u_angle=lambda w: np.array([[0.3, 0.0, 1.0, 0.25]], np.float32)))
    assert rad[0, 0] == 0 and not z[0, :2].any() and rad[0, 1] == R.RAD_MAX and z[0, 2] == R.RAD_MAX and z[0, 3] == 0
    assert np.allclose(z[0, 4:], [rad[0, 2], 0, 0, rad[0, 3]], atol=1e-15) and abs(R.RAD_MAX - 6.66) < 0.01
    assert rad[0, 2] == math.sqrt(2 * math.log(2))


def test_entry_points_agree():
    x = np.random.default_rng(2).standard_normal((3, 14)).astype(np.float32)
    sg = np.array([0.5, 0.0, 2.0], np.float32)
    z, rad = R.normals(2, 7, 3, S0)
    y = R.awgn(x, sg, S0)
    assert y.dtype == np.float64 and np.array_equal(y, x.astype(np.float64) + sg.astype(np.float64)[:, None] * z) and np.array_equal(y[1], x[1])
    assert np.array_equal(rad, R.radius(2, 7, 3, S0)) and np.allclose(np.hypot(z[:, 0::2], z[:, 1::2]), rad, rtol=1e-14)
    t = R.tx_noise(7, 3, sg, S0)                                         # an odd frame: the last pair gives one symbol
    z1, _ = R.normals(1, 7, 3, S0)
    assert t.shape == (3, 14) and np.array_equal(t, sg.astype(np.float64)[:, None] * z1) and np.array_equal(R.tx_noise(8, 3, sg, S0)[:, :14], t)
    w = R.words(1, 4, 3, S0)
    wr, wa = R.sample_words(1, 7, 3, S0)
    assert np.array_equal(wr[:, 0::2], w[0]) and np.array_equal(wr[:, 1::2], w[2][:, :3]) and np.array_equal(wa[:, 0::2], w[1]) and np.array_equal(wa[:, 1::2], w[3][:, :3])
    b = R.source_bits(70, 3, S0)
    w0 = R.words(0, 1, 3, S0)
    assert b.dtype == np.int32 and b.shape == (3, 70) and set(np.unique(b)) <= {0, 1}
    for f in range(3):
        for k in range(70):
            assert b[f, k] == (int(w0[k // 32][f, 0]) >> (k % 32)) & 1
    assert np.array_equal(R.source_bits(14232, 2, 5)[:, :9552], R.source_bits(9552, 2, 5)) and np.array_equal(R.source_bits(9552, 3, 5)[:2], R.source_bits(9552, 2, 5))
    assert np.array_equal(R.source_bits(32 * 9, 1, 5)[0, 128:160], (int(R.philox4x32_10((1, 0, 0, 0), (5, 0))[0]) >> np.arange(32)) & 1)      # word 4 is word x of counter 1


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.fixture(scope="module")
def D():
    """the samples every statistic is taken from, drawn once"""
    class D:
        pass
    D.ch, D.ch_rad = R.normals(2, 2 ** 18, 16, S0)                        # channel: 16 frames of 2^18 complex samples, 2^23 reals
    D.tx, _ = R.normals(1, 2 ** 19, 8, S0)                                # modulator, same seed: 8 frames of 2^19 symbols, 2^18 counters a frame
    D.ch1, _ = R.normals(2, 2 ** 18, 8, S0 + 1)                           # channel, the next seed
    D.bits = R.source_bits(2 ** 20, 4, S0)                                # payload, same seed: bit k of frame f against real k of the modulator's frame f
    return D


def _within(name, stat, se, extra=0.0):
    print("%-58s %+.3e = %+.2f standard errors of %.3e" % (name, stat, stat / se, se))
    assert abs(stat) <= SE * se + extra, name


def _corr(name, a, b):
    a, b = np.ravel(a), np.ravel(b)
    assert a.size == b.size >= 2 ** 22
    _within("correlation " + name, float(np.mean(a * b) / math.sqrt(np.mean(a * a) * np.mean(b * b))), 1.0 / math.sqrt(a.size))


def test_twin_moments(D):
    for name, z in (("channel", D.ch), ("modulator", D.tx)):
        assert z.size >= 2 ** 22
        _within(name + " mean", float(np.mean(z)), 1.0 / math.sqrt(z.size))
        _within(name + " variance - 1", float(np.mean(z * z)) - 1.0, math.sqrt(2.0 / z.size))


def _chi2(name, p, bins=64):
    """p should be uniform on [0, 1): chi-square over equiprobable bins, 63 degrees of freedom (mean 63, variance 126)"""
    assert p.size >= 2 ** 22
    c = np.bincount(np.minimum((p * bins).astype(np.int64), bins - 1), minlength=bins)
    chi2 = float(np.sum((c - p.size / bins) ** 2) / (p.size / bins))
    _within("chi-square " + name + " - 63", chi2 - (bins - 1), math.sqrt(2.0 * (bins - 1)))


def test_twin_radius_and_angle(D):
    _chi2("rad^2 / 2 against Exp(1)", -np.expm1(-0.5 * D.ch_rad.ravel() ** 2))
    _chi2("angle against uniform", (np.arctan2(D.ch[:, 1::2], D.ch[:, 0::2]).ravel() / (2 * np.pi)) % 1.0)
    z = D.tx.reshape(8, -1, 2)
    _chi2("modulator rad^2 / 2 against Exp(1)", -np.expm1(-0.5 * (z[..., 0] ** 2 + z[..., 1] ** 2).ravel()))
    _chi2("modulator angle against uniform", (np.arctan2(z[..., 1], z[..., 0]).ravel() / (2 * np.pi)) % 1.0)


def test_twin_tails(D):
    """|n| > 3, 4, 5 against erfc(t / sqrt 2).  The 2^-32 grid of u1 ends the radius at 6.66: what a continuous radius would put beyond is 2^-32 of
    the samples, so the truncation moves an expected count by at most N 2^-32 (0.004 here), which the bar takes on top."""
    z = np.concatenate([D.ch.ravel(), D.tx.ravel()])
    assert z.size == 2 ** 24 and np.max(np.abs(z)) <= R.RAD_MAX
    for t in (3.0, 4.0, 5.0):
        p = math.erfc(t / math.sqrt(2.0))
        n = int(np.count_nonzero(np.abs(z) > t))
        print("|n| > %g: %d, expected %.1f" % (t, n, z.size * p))
        _within("count of |n| > %g less the normal tail's" % t, n - z.size * p, math.sqrt(z.size * p * (1 - p)), extra=z.size * 2.0 ** -32)


def test_twin_correlations(D):
    ch = D.ch.reshape(16, -1, 2)
    tx = D.tx.reshape(8, -1, 2)
    _corr("re and im of a sample", ch[..., 0], ch[..., 1])
    _corr("neighbouring samples", ch[:, :-1], ch[:, 1:])
    _corr("re of a sample and im of the next, im and re", ch[:, :-1], ch[:, 1:, ::-1])
    _corr("sample k of frames f and f + 1", ch[:-1], ch[1:])
    _corr("the modulator's even and odd symbol of a pair", tx[:, 0::2], tx[:, 1::2])
    _corr("the modulator's even symbol, re, and odd symbol, im; im and re", tx[:, 0::2], tx[:, 1::2, ::-1])
    _corr("streams 1 (even symbol) and 2 of a counter", tx[:, 0::2], ch[:8])
    _corr("streams 1 (odd symbol) and 2 of a counter", tx[:, 1::2], ch[:8])
    _corr("seeds s and s + 1", D.ch1, D.ch[:8])
    _corr("payload bits and the stream-1 noise of the frame", 2.0 * D.bits - 1.0, D.tx[:4])
    _within("payload mean bit - 1/2", float(np.mean(D.bits)) - 0.5, 0.5 / math.sqrt(D.bits.size))


# ---------------------------------------------------------------------------------------------------------------- c
ST = R.STAGES
_f32 = R._f32
MUTANTS = {
    "sin and cos swapped": {"unit": lambda u: ST["unit"](u)[::-1]},
    "radius uniform without the + 1": {"u_radius": lambda w: _f32(w) * R.TWO_M32},
    "uniforms from the top 24 bits only": {"u_radius": lambda w: (_f32(w >> np.uint64(8)) + np.float32(1.0)) * np.float32(2.0 ** -24), "u_angle": lambda w: _f32(w >> np.uint64(8)) * np.float32(2.0 ** -24)},
    "stream id 1 <-> 2": {"counter": lambda p, f, s: (p, f, np.uint64(3) - s, 0)},
    "frame and pair index swapped in the counter": {"counter": lambda p, f, s: (f, p, s, 0)},
    "key halves swapped": {"key": lambda seed: (seed >> 32, seed & 0xFFFFFFFF)},
    "9 rounds": {"rounds": 9},
    "the modulator reusing words x / y for the odd symbol": {"odd_words": (0, 1)},
    "sigma[0] used for every frame": {"sigma": lambda sg: np.full_like(sg, sg[0])},
    "a logarithm with 1e-4 relative error": {"log": lambda u: ST["log"](u) * (1.0 + 1e-4)},
    "a gain error of 3e-5": {"gain": 1.0 + 3e-5},
    "NaN for the zero noise at u1 == 1": {"radius": lambda u, log: np.where(u == 1, np.nan, ST["radius"](u, log))},
}


def _cases():
    """(name, stream, x, sigma, seed, systematic): a channel call and a transmitter call of the GPU test's kind, small, and the first fixture
    entry of every class and generator in the call the GPU test makes for it"""
    yield "channel 2^16 pairs", 2, np.zeros((5, 2 ** 17), np.float32), R.CH_SIGMA, S0, True
    yield "modulator 8370 symbols", 1, np.zeros((3, 2 * 8370), np.float32), R.TX_SIGMA, S0, False
    seen = set()
    for e in EDGES:
        k = (e["stream"], e["word"] & 2, e["class"])
        if k not in seen:
            seen.add(k)
            yield "edge %s stream %d word %d" % (e["class"], e["stream"], e["word"]), e["stream"], np.tile(np.array([1.0, 0.5], np.float32), 64)[None, :], np.float32(0.5), e["seed"], False


def _device(stream, x, sigma, seed, st):
    """what a kernel with the stages `st` would return: the twin's arithmetic, rounded to float32 once at the end"""
    F, n2 = x.shape
    with np.errstate(all="ignore"):
        return R._scaled(stream, x, n2 // 2, F, sigma, seed, st).astype(np.float32)


def test_every_mistake_is_seen_by_a_bar():
    cases = list(_cases())
    assert len(cases) == 2 + 12
    for name, stream, x, sigma, seed, systematic in cases:              # the twin itself, rounded to float32, meets every bar
        r = R.check(_device(stream, x, sigma, seed, ST), x, sigma, stream, seed, systematic=systematic, cap=not name.startswith("edge"))
        print(R.describe("twin: " + name, r))
        assert not r["broken"], (name, r["broken"])
    for mname, change in MUTANTS.items():
        st = dict(ST, **change)
        seen = {}
        for name, stream, x, sigma, seed, systematic in cases:
            r = R.check(_device(stream, x, sigma, seed, st), x, sigma, stream, seed, systematic=systematic, cap=False)
            for bar in r["broken"]:
                seen.setdefault(bar, []).append(name)
        print("mutation: %s" % mname)
        for bar, where in sorted(seen.items()):
            print("    %-7s %2d of %2d cases, e.g. %s" % (bar, len(where), len(cases), "; ".join(where[:3])))
        assert seen, mname
        if mname == "a gain error of 3e-5":
            assert "gain" in seen
        if mname.startswith("NaN"):
            assert "finite" in seen


# ---------------------------------------------------------------------------------------------------------------- d
def test_edge_fixture_is_what_the_twin_says():
    count = {}
    for e in EDGES:
        assert set(e) == {"stream", "seed", "frame", "pair", "word", "class", "r"} and e["frame"] == 0 and 0 <= e["pair"] < 64
        assert (e["stream"], e["word"] & 2) in R.EDGE_GENERATORS and (e["word"] & 1) == (1 if e["class"] == "C" else 0)
        w = R.philox4x32_10((e["pair"], e["frame"], e["stream"], 0), R.STAGES["key"](e["seed"]))
        assert int(w[e["word"]]) == e["r"] and bool(R.edge_class(e["class"], e["r"])), e
        k = R.edge_sample(e)
        wr, wa = R.sample_words(e["stream"], k + 1, 1, e["seed"])
        assert int((wa if e["class"] == "C" else wr)[0, k]) == e["r"]
        z, rad = R.normals(e["stream"], k + 1, 1, e["seed"])
        if e["class"] == "A":
            assert rad[0, k] == 0 and not z[0, 2 * k:2 * k + 2].any()
        elif e["class"] == "A2":
            assert rad[0, k] == math.sqrt(-2.0 * math.log(1.0 - 2.0 ** -24)) and 0 < rad[0, k] < 2.0 ** -10
        elif e["class"] == "B":
            assert 5.8 < rad[0, k] <= R.RAD_MAX
        else:
            assert z[0, 2 * k] == rad[0, k] and abs(z[0, 2 * k + 1]) < 1e-14
        count[(e["stream"], e["word"] & 2, e["class"])] = count.get((e["stream"], e["word"] & 2, e["class"]), 0) + 1
    assert set(count) == {(s, rw, c) for (s, rw) in R.EDGE_GENERATORS for c in R.EDGE_CLASSES} and min(count.values()) >= 4


# ---------------------------------------------------------------------------------------------------------------- e
def test_near_one_share_of_the_gpu_cases(P):
    """at most 2^-12 of a case's samples have a radius below 2^-6 (expected 1.2e-4): true of the seeds the GPU test uses, at every size"""
    F = len(R.CH_SIGMA)
    for seed in R.CH_SEEDS:
        rad = R.radius(2, max(R.CH_PAIRS), F, seed)
        for pairs in R.CH_PAIRS:
            n = int(np.count_nonzero(rad[:, :pairs] < R.NEAR_ONE))
            print("channel seed %#x pairs %6d: %3d of %d near 1" % (seed, pairs, n, F * pairs))
            assert n <= R.NEAR_ONE_CAP * F * pairs
    for modcod in R.TX_MODCODS:
        pl = P.get_modcod(modcod).pl_frame
        n = int(np.count_nonzero(R.radius(1, pl, len(R.TX_SIGMA), R.TX_SEED) < R.NEAR_ONE))
        print("modulator %s: %d of %d near 1" % (modcod, n, 3 * pl))
        assert n <= R.NEAR_ONE_CAP * 3 * pl
    n = int(np.count_nonzero(R.radius(2, 1000, 7, (5 << 40) + 9) < R.NEAR_ONE))
    assert n <= R.NEAR_ONE_CAP * 7000
