"""The float64 twin of the project's noise generator and random source, and the bars a device output is held to against it.

dvbs2_amd/csrc/k_tx.hip draws everything random from Philox4x32-10, key = (seed & 0xffffffff, seed >> 32):
    stream 0  payload     counter (w >> 2, f, 0, 0), word w & 3 is the packed payload word w of frame f (bit b of it is payload bit 32 w + b)
    stream 1  modulator   counter (pair, f, 1, 0): words x / y give PL symbol 2 pair, words z / w give PL symbol 2 pair + 1 (tx_mod_kernel)
    stream 2  channel     counter (pair, f, 2, 0): words x / y give complex sample `pair` of frame f (awgn_kernel)
One complex sample is one Box-Muller pair: u1 = (float(r) + 1) 2^-32 and u2 = float(r') 2^-32 IN FLOAT32 -- three correctly rounded IEEE
operations, so they belong to the definition and are restated bit for bit (r >= 2^32 - 128 gives 1.0f in both) -- and from there float64:
rad = sqrt(-2 ln u1), n = rad (cos 2 pi u2, sin 2 pi u2), y = x + sigma[f] n.  The largest radius is sqrt(64 ln 2) = 6.66.

Integer Philox is exact, so this is a sample-by-sample reference and not a statistical one; the statistics are done once, on the CPU, on the
twin (tests/test_awgn_ref.py).  The stages are the entries of STAGES: a mistake is the same dictionary with one entry replaced.
NumPy only: no GPU, no oracle."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
TWO_M32 = np.float32(2.0 ** -32)
RAD_MAX = math.sqrt(64.0 * math.log(2.0))
NEAR_ONE = 2.0 ** -6                                       # radius below which u1 is within 1.2e-4 of 1: the second zone of the per-sample bar
NEAR_ONE_CAP = 2.0 ** -12                                  # the share of a case's samples that may lie there (expected: 1 - exp(-2^-13) = 1.2e-4)


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & M32


def philox4x32(ctr, key, rounds=10):
    """Philox4x32: ctr = four and key = two arrays (or scalars) of 32-bit values, broadcast together -> four uint64 arrays below 2^32.
    The round of k_tx.hip's philox4x32: (x, y, z, w) <- (hi(M1 z) ^ y ^ k0, lo(M1 z), hi(M0 x) ^ w ^ k1, lo(M0 x)), then the key is bumped."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in ctr])
    k0, k1 = _u64(key[0]), _u64(key[1])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                              # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def philox4x32_10(ctr, key):
    return philox4x32(ctr, key, 10)


def _f32(w):
    return np.asarray(w, dtype=np.uint64).astype(np.uint32).astype(np.float32)      # uint32 -> float32, round to nearest even


# ---------------------------------------------------------------------------------------------------------------- the stages
STAGES = {
    "rounds": 10,
    "key": lambda seed: (seed & 0xFFFFFFFF, seed >> 32),
    "counter": lambda pair, frame, stream: (pair, frame, stream, 0),
    "odd_words": (2, 3),                                               # the modulator's odd symbol of a pair: words z / w
    "u_radius": lambda w: (_f32(w) + np.float32(1.0)) * TWO_M32,        # float32, in (0, 1]
    "u_angle": lambda w: _f32(w) * TWO_M32,                             # float32, in [0, 1]: revolutions
    "log": lambda u: np.log(u.astype(np.float64)),
    "radius": lambda u, log: np.sqrt(-2.0 * log(u)),
    "unit": lambda u: (np.cos(2.0 * np.pi * u.astype(np.float64)), np.sin(2.0 * np.pi * u.astype(np.float64))),
    "gain": 1.0,
    "sigma": lambda sigma: sigma,                                       # the [F] vector the frames are scaled with
}


def words(stream, n_ctr, F, seed, st=STAGES, frame0=0):
    """the four words of counters 0 .. n_ctr - 1 of frames frame0 .. frame0 + F - 1 -> uint64 [4, F, n_ctr]"""
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    pair = np.arange(n_ctr, dtype=np.uint64)[None, :]
    frame = np.arange(frame0, frame0 + F, dtype=np.uint64)[:, None]
    return np.stack(philox4x32(st["counter"](pair, frame, np.uint64(stream)), st["key"](seed), st["rounds"]))


def sample_words(stream, n, F, seed, st=STAGES):
    """(radius word, angle word) of complex samples 0 .. n - 1 of every frame -> two uint64 [F, n]"""
    if stream == 2:
        w = words(2, n, F, seed, st)
        return w[0], w[1]
    assert stream == 1
    w = words(1, (n + 1) // 2, F, seed, st)
    o = st["odd_words"]
    wr = np.stack([w[0], w[o[0]]], axis=-1).reshape(F, -1)[:, :n]
    wa = np.stack([w[1], w[o[1]]], axis=-1).reshape(F, -1)[:, :n]
    return wr, wa


def normals(stream, n, F, seed, st=STAGES):
    """unit-variance noise of complex samples 0 .. n - 1 -> (float64 [F, 2 n] interleaved re, im; the radius float64 [F, n])"""
    wr, wa = sample_words(stream, n, F, seed, st)
    rad = st["radius"](st["u_radius"](wr), st["log"])
    c, s = st["unit"](st["u_angle"](wa))
    z = st["gain"] * np.stack([rad * c, rad * s], axis=-1).reshape(F, 2 * n)
    return z, rad


def radius(stream, n, F, seed):
    """the twin's Box-Muller radius of every complex sample, float64 [F, n]: what the per-sample bar scales with"""
    return STAGES["radius"](STAGES["u_radius"](sample_words(stream, n, F, seed)[0]), STAGES["log"])


def _scaled(stream, x, n, F, sigma, seed, st):
    sg = np.asarray(st["sigma"](np.broadcast_to(np.asarray(sigma, dtype=np.float32), (F,)))).astype(np.float64)
    z, _ = normals(stream, n, F, seed, st)
    return sg[:, None] * z if x is None else np.asarray(x, dtype=np.float32).astype(np.float64).reshape(F, 2 * n) + sg[:, None] * z


def awgn(x, sigma, seed, st=STAGES):
    """Channel_AWGN::add_noise as awgn_kernel restates it: x float32 [F, 2 n] (n complex samples a frame), sigma [F] -> float64 [F, 2 n]"""
    x = np.asarray(x)
    F, n2 = x.shape
    assert n2 % 2 == 0
    return _scaled(2, x, n2 // 2, F, sigma, seed, st)


def tx_noise(pl_frame, F, sigma, seed, st=STAGES):
    """what tx_bb with a sigma socket adds to its F PL frames of pl_frame symbols: float64 [F, 2 pl_frame]"""
    return _scaled(1, None, pl_frame, F, sigma, seed, st)


def source_bits(K, F, seed, st=STAGES):
    """the random payload of tx_bb: int32 [F, K]"""
    nw = (K + 31) // 32
    seed = int(seed)
    w = np.arange(nw, dtype=np.uint64)[None, :]
    frame = np.arange(F, dtype=np.uint64)[:, None]
    r = np.stack(philox4x32(st["counter"](w >> np.uint64(2), frame, np.uint64(0)), st["key"](seed), st["rounds"]))      # [4, F, nw]
    word = np.take_along_axis(r, np.broadcast_to((w & np.uint64(3)).astype(np.int64), (F, nw))[None], axis=0)[0]
    bits = (word[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)                         # little-endian inside a word
    return bits.reshape(F, nw * 32)[:, :K].astype(np.int32)                                                            # the tail of the last word is dropped


# ---------------------------------------------------------------------------------------------------------------- the edge classes
def edge_class(which, w):
    """does the 32-bit word w belong to edge class `which`?  A, A2, B speak of a radius word, C of an angle word."""
    w = np.asarray(w, dtype=np.uint64)
    if which == "A":
        return w >= np.uint64(2 ** 32 - 128)                            # u1 == 1.0f: no noise at all
    if which == "A2":
        return (w >= np.uint64(2 ** 32 - 383)) & (w <= np.uint64(2 ** 32 - 129))      # u1 = 1 - 2^-24, the largest float below 1 (2^32 - 384 ties to even, 2^32 - 512)
    if which == "B":
        return w < np.uint64(EDGE_B)                                    # rad >= 5.8: the deep tail
    if which == "C":
        return w >= np.uint64(2 ** 32 - 128)                            # u2 == 1.0f: a whole revolution
    raise ValueError(which)


# (a radius word below 256 gives rad >= sqrt(48 ln 2) = 5.77 only; rad >= 5.8 needs u1 <= exp(-5.8^2 / 2), a word of at most 211)
EDGE_B = 200
EDGE_CLASSES = ("A", "A2", "B", "C")
EDGE_GENERATORS = ((2, 0), (1, 0), (1, 2))                              # (stream, radius word): the channel's x / y, the modulator's x / y and z / w


def edge_sample(e):
    """fixture entry -> index of the complex sample inside the frame it speaks of"""
    return e["pair"] if e["stream"] == 2 else 2 * e["pair"] + (1 if e["word"] >= 2 else 0)


# ---------------------------------------------------------------------------------------------------------------- the cases of tests/test_awgn_gpu.py
CH_SIGMA = np.array([0.05, 0.3, 1.0, 4.0, 0.0], np.float32)
CH_PAIRS = (1, 255, 256, 257, 16741, 2 ** 17)                            # one lane, a workgroup less one, one, one and a lane, no multiple of anything, 512 workgroups a frame
CH_SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1, (7 << 40) + (3 << 8) + 5)         # either key half zero, both all ones, the simulator's form
TX_MODCODS = ("QPSK-S_8/9", "8PSK-S_3/5", "32APSK-S_3/4", "QPSK-N_8/9")   # tx_mod_kernel<2, false>, <3, true>, <5, true>, a normal frame
TX_SIGMA = np.array([0.2, 0.0, 0.7], np.float32)
TX_SEED = 11

# ---------------------------------------------------------------------------------------------------------------- the bars
EPS = 1e-5                 # per sample, relative to sigma max(1, rad); and the systematic gain and mean
ROUND = 2.0 ** -22         # of max(|x|, |y|): the one fp32 rounding of x + sigma n, contracted into an FMA or not
NEAR_ONE_BAR = 2.0 ** -10  # of sigma, where rad < NEAR_ONE
SYSTEMATIC_MIN = 2 ** 17   # real samples a frame needs for the systematic bar


def check(y_dev, x, sigma, stream, seed, systematic=False, cap=True, twin=None):
    """Holds a device output [F, 2 n] to the twin: x is the noiseless input (None: zero), sigma [F].  -> dict with the measurements and
    "broken", the names of the bars missed: finite, sample (either zone), share (of the near-1 zone), gain, mean (the systematic pair,
    only where asked for: x has to be zero there and every frame with sigma > 0 needs SYSTEMATIC_MIN real samples)."""
    y_dev = np.asarray(y_dev)
    F, n2 = y_dev.shape
    n = n2 // 2
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (F,)).astype(np.float64)
    z, rad = twin if twin is not None else normals(stream, n, F, seed)
    x64 = np.zeros((F, n2)) if x is None else np.asarray(x, dtype=np.float32).astype(np.float64).reshape(F, n2)
    y = x64 + sg[:, None] * z
    out = {"broken": [], "samples": F * n}
    finite = np.isfinite(y_dev)
    out["finite"] = bool(finite.all())
    if not out["finite"]:
        out["broken"].append("finite")
    e = np.where(finite, y_dev.astype(np.float64) - y, np.inf)
    r2 = np.repeat(rad, 2, axis=1)
    near = r2 < NEAR_ONE
    rnd = ROUND * np.maximum(np.abs(x64), np.abs(y))
    scale = sg[:, None] * np.where(near, NEAR_ONE_BAR, EPS * np.maximum(1.0, r2))
    if not np.all(np.abs(e) <= scale + rnd):
        out["broken"].append("sample")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sg[:, None] > 0, np.abs(e) / (sg[:, None] * np.maximum(1.0, r2)), 0.0)        # |e| in units of sigma max(1, rad), the rounding of x + sigma n included
    out["worst_far"] = float(np.max(np.where(near, 0.0, ratio), initial=0.0))
    out["worst_near"] = float(np.max(np.where(near, ratio, 0.0), initial=0.0))
    out["share"] = float(np.count_nonzero(rad < NEAR_ONE)) / (F * n)
    if cap and out["share"] > NEAR_ONE_CAP:
        out["broken"].append("share")
    if systematic:
        assert not x64.any()
        gains, means = [], []
        for f in range(F):
            if sg[f] == 0:
                continue
            assert n2 >= SYSTEMATIC_MIN
            ef = e[f] / sg[f]
            gains.append(float(np.sum(ef * z[f]) / np.sum(z[f] * z[f])))
            means.append(float(np.mean(ef)))
        out["gain"], out["mean"] = gains, means
        if not all(abs(g) <= EPS for g in gains):
            out["broken"].append("gain")
        if not all(abs(m) <= EPS for m in means):
            out["broken"].append("mean")
    return out


def describe(tag, r):
    s = "%-46s n %7d  |e| / (sigma max(1, r)): far %.3e near %.3e  share %.2e" % (tag, r["samples"], r["worst_far"], r["worst_near"], r["share"])
    if "gain" in r:
        s += "  gain %s  mean %s" % (" ".join("%+.2e" % g for g in r["gain"]), " ".join("%+.2e" % m for m in r["mean"]))
    return s + ("  BROKEN: " + ",".join(r["broken"]) if r["broken"] else "")
