"""The AWGN channel (awgn_kernel: add_noise), the modulator's noise (the tail of tx_mod_kernel: tx_bb with a sigma socket) and the random source
(tx_src_kernel) against their float64 twin, tests/awgn_ref.py, sample by sample.

The bars (awgn_ref.check; e = y_gpu - y_twin, r = the twin's radius of the sample):
    r >= 2^-6:  |e| <= sigma 1e-5 max(1, r) + 2^-22 max(|x|, |y_twin|)
    r <  2^-6:  |e| <= sigma 2^-10 + 2^-22 max(|x|, |y_twin|), on at most 2^-12 of a case's samples (a property of the seed: asserted on
                the CPU for every case of this file by tests/test_awgn_ref.py::test_near_one_share_of_the_gpu_cases)
    systematic, x = 0, a frame of at least 2^17 real samples:  |sum(e n)| / sum(n^2) <= 1e-5 and |mean(e)| <= 1e-5 sigma
1e-5 is a requirement: around the waterfall d ln FER / d ln sigma is about 200 and a per-sample error of eps sigma max(1, r), even fully
systematic, moves sigma by at most 1.6 eps, so 1e-5 moves a FER by 0.3 %, a seventh of what the pooled comparison resolves.  That tests/
test_awgn_ref.py shows on the CPU which of twelve mistakes each bar rejects.  Measured values: results/awgn/README.md (every test prints its
figures before it asserts).

(The 2^17-pair case of the channel is one call of F = 5 frames, 1.25 x 2^20 floats: the case list fixes both numbers.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import awgn_ref as R

pytestmark = pytest.mark.gpu

SIGMA5, PAIRS, SEEDS = R.CH_SIGMA, R.CH_PAIRS, R.CH_SEEDS
TX_MODCODS, TX_SIGMA, TX_SEED = R.TX_MODCODS, R.TX_SIGMA, R.TX_SEED
EDGES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "awgn_edge_seeds.json")))


def gaussian_x(F, n, seed=77):
    """unit-power complex Gaussian, float32 [F, 2 n]"""
    return (np.random.default_rng(seed).standard_normal((F, 2 * n)) * np.sqrt(0.5)).astype(np.float32)


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


@pytest.fixture(scope="module")
def ch(Rx):
    rx = Rx("QPSK-S_8/9", max_frames=8)
    yield rx
    rx.close()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- add_noise against the twin
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("pairs", PAIRS)
def test_add_noise_against_the_twin(ch, pairs, seed):
    F = len(SIGMA5)
    twin = R.normals(2, pairs, F, seed)
    xg = gaussian_x(F, pairs)
    xg[4, 0] = -0.0                                                      # bit for bit includes the sign of a zero
    for kind, x in (("zero", np.zeros((F, 2 * pairs), np.float32)), ("gauss", xg)):
        y = ch.add_noise(SIGMA5, x, seed=seed, n_frames=F).reshape(F, 2 * pairs)
        r = R.check(y, x, SIGMA5, 2, seed, systematic=(kind == "zero" and pairs == 2 ** 17), twin=twin)
        print(R.describe("add_noise %s pairs %d seed %#x" % (kind, pairs, seed), r))
        assert bits_equal(y[4], x[4]), "the sigma = 0 frame is not its input"
        assert not r["broken"], r["broken"]


# ---------------------------------------------------------------------------------------------------------------- geometry and form
class Dev:
    """a device buffer of the handle's own (dvbs2hip_malloc and the memcpy helpers)"""
    def __init__(self, rx, host):
        self.rx, self.p, self.host = rx, C.c_void_p(), np.ascontiguousarray(host)
        assert rx.L.dvbs2hip_malloc(rx.h, C.byref(self.p), max(self.host.nbytes, 4)) == 0
        self.put(self.host)

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert self.rx.L.dvbs2hip_memcpy_h2d(self.rx.h, self.p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def get(self):
        out = np.empty_like(self.host)
        assert self.rx.L.dvbs2hip_memcpy_d2h(self.rx.h, out.ctypes.data_as(C.c_void_p), self.p, out.nbytes) == 0
        return out

    def free(self):
        self.rx.L.dvbs2hip_free(self.rx.h, self.p)


def test_noise_does_not_depend_on_the_call_geometry(ch):
    seed, n = (5 << 40) + 9, 1000
    x = gaussian_x(7, n, seed=3)
    sg = np.array([0.3, 1.0, 0.0, 2.0, 0.5, 0.7, 0.1], np.float32)
    y7 = ch.add_noise(sg, x, seed=seed, n_frames=7).reshape(7, -1)
    y3 = ch.add_noise(sg[:3], x[:3], seed=seed, n_frames=3).reshape(3, -1)
    assert bits_equal(y3, y7[:3])                                        # frame f of a call is frame f of a longer call
    m = 300
    ys = ch.add_noise(sg, np.ascontiguousarray(x[:, :2 * m]), seed=seed, n_frames=7).reshape(7, -1)
    assert bits_equal(ys, y7[:, :2 * m])                                 # the first pairs do not depend on n_elmts
    assert not R.check(y7, x, sg, 2, seed)["broken"]
    # the device form, out of place and in place
    dx, dy, ds = Dev(ch, x), Dev(ch, np.zeros_like(x)), Dev(ch, sg)
    ch.add_noise_dev(ds.p.value, dx.p.value, dy.p.value, seed, 2 * n, 7)
    assert bits_equal(dy.get(), y7)
    ch.add_noise_dev(ds.p.value, dx.p.value, dx.p.value, seed, 2 * n, 7)
    assert bits_equal(dx.get(), y7)
    # odd and empty sockets: an error, and nothing written
    from dvbs2_amd.lib_binding import Dvbs2HipError
    mark = np.full_like(x, 7.25)
    dy.put(mark)
    for bad in (2 * n - 1, 3, 1, 0, -2):
        with pytest.raises(Dvbs2HipError):
            ch.add_noise_dev(ds.p.value, dx.p.value, dy.p.value, seed, bad, 7)
        out = np.full(7 * max(bad, 0), 7.25, np.float32)
        xin = np.zeros(7 * max(bad, 0), np.float32)
        rc = ch.L.dvbs2hip_add_noise(ch.h, sg.ctypes.data_as(C.c_void_p), xin.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), seed, bad, 7)
        assert rc != 0 and (out == 7.25).all()
    assert bits_equal(dy.get(), mark)
    for d in (dx, dy, ds):
        d.free()


@pytest.mark.parametrize("F", [128, 1024])
def test_host_form_on_registered_sockets_is_one_call(Rx, F):
    """the pinned-socket pipeline cuts a per-frame task into 4 (F >= 128) or 8 (F >= 1024) chunks; add_noise must not go that way, since
    every chunk would restart at frame 0 and repeat the noise: registered and unregistered calls agree, and both are the twin's frames"""
    n, seed = 64, 2 ** 32 + 17
    rx = Rx("QPSK-S_8/9", max_frames=F)
    x = gaussian_x(F, n, seed=F)
    sg = np.linspace(0.1, 2.0, F).astype(np.float32)
    plain = rx.add_noise(sg, x, seed=seed, n_frames=F).reshape(F, 2 * n)
    y = np.zeros_like(x)
    for a in (sg, x, y):
        rx.host_register(a)
    assert rx.L.dvbs2hip_add_noise(rx.h, sg.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), seed, 2 * n, F) == 0
    for a in (sg, x, y):
        rx.host_unregister(a)
    rx.close()
    assert bits_equal(y, plain)
    r = R.check(y, x, sg, 2, seed, cap=False)
    print(R.describe("host form registered F %d" % F, r))
    assert not r["broken"], r["broken"]


# ---------------------------------------------------------------------------------------------------------------- tx_bb against the twin
def layout(rx):
    """masks over the PL symbols of a frame: header, pilots"""
    i = np.arange(rx.pl_frame)
    j = i - 90
    n_pil = rx.N_xfec // 1440
    blk, off = j // 1476, j % 1476
    return i < 90, (i >= 90) & (blk < n_pil) & (off >= 1440)


@pytest.mark.parametrize("modcod", TX_MODCODS)
def test_tx_bb_noise_against_the_twin(Rx, modcod):
    F, seed = 3, TX_SEED
    rx = Rx(modcod, max_frames=5)
    s1, p1 = rx.tx_bb(F, seed=seed)
    sn, pn = rx.tx_bb(F, seed=seed, sigma=TX_SIGMA)
    _, p0 = rx.tx_bb(F, seed=seed, sigma=np.zeros(F, np.float32))
    s5, p5 = rx.tx_bb(5, seed=seed, sigma=np.concatenate([TX_SIGMA, [1.5, 0.4]]).astype(np.float32))
    assert np.array_equal(s1, sn) and bits_equal(p0, p1)
    assert bits_equal(pn[1], p1[1]), "the sigma = 0 frame is not the noiseless one"
    assert bits_equal(p5[:F], pn) and np.array_equal(s5[:F], sn)         # frame f does not depend on F
    r = R.check(pn, p1, TX_SIGMA, 1, seed)
    print(R.describe("tx_bb %s" % modcod, r))
    assert not r["broken"], r["broken"]
    # header and pilots get noise like data: check() above held them to the twin with every other symbol; here, that the mask is the right one
    # and that each of those symbols did move
    hdr, pil = layout(rx)
    got = (pn.astype(np.float64) - p1).reshape(F, -1, 2)
    assert hdr.sum() == 90 and pil.sum() == 36 * (rx.N_xfec // 1440) and np.allclose(np.abs(p1.reshape(F, -1, 2)[:, pil]), np.sqrt(0.5), atol=1e-6)
    for mask in (hdr, pil):
        for f in (0, 2):
            assert np.all(np.any(got[f, mask] != 0, axis=1))
    if modcod == "QPSK-N_8/9":
        # the systematic bar: x is the frame here and not zero, so e carries the one rounding of p1 + sigma n as well -- random, at most 2^-24 |y|
        # a sample, far below the bar once averaged.  A frame has 66564 reals: the two noisy frames are pooled, in units of their sigma
        z, _ = R.normals(1, rx.pl_frame, F, seed)
        e = np.concatenate([(pn[f].astype(np.float64) - p1[f]) / float(TX_SIGMA[f]) - z[f] for f in (0, 2)])
        zz = np.concatenate([z[0], z[2]])
        assert e.size >= R.SYSTEMATIC_MIN
        gain, mean = float(np.sum(e * zz) / np.sum(zz * zz)), float(np.mean(e))
        print("tx_bb %s systematic over %d reals: gain %+.3e mean %+.3e" % (modcod, e.size, gain, mean))
        assert abs(gain) <= R.EPS and abs(mean) <= R.EPS
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- the random payload
@pytest.mark.parametrize("modcod", ["QPSK-S_8/9", "QPSK-S_3/5", "QPSK-N_8/9"])
def test_random_payload_is_the_twins(Rx, modcod):
    rx = Rx(modcod, max_frames=5)
    for seed in (0, 2 ** 64 - 1):
        s3, _ = rx.tx_bb(3, seed=seed)
        s5, _ = rx.tx_bb(5, seed=seed)
        want = R.source_bits(rx.K_bch, 5, seed)
        assert s5.dtype == np.int32 and np.array_equal(s5, want), (modcod, seed, int((s5 != want).sum()))
        assert np.array_equal(s3, want[:3])
    print("payload %s: K_bch %d, K %% 32 = %d" % (modcod, rx.K_bch, rx.K_bch % 32))
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- edge seeds
@pytest.mark.parametrize("stream", [2, 1])
def test_edge_seeds(Rx, ch, stream):
    entries = [e for e in EDGES if e["stream"] == stream]
    assert len(entries) >= (16 if stream == 2 else 32)
    sigma = np.float32(0.5)
    rx = ch
    for e in entries:
        k = R.edge_sample(e)
        if stream == 2:
            n = 64
            x = np.tile(np.array([1.0, 0.5], np.float32), n)[None, :]
            y = rx.add_noise(sigma, x, seed=e["seed"], n_frames=1).reshape(1, -1)
        else:
            n = rx.pl_frame
            _, x = rx.tx_bb(1, seed=e["seed"])
            _, y = rx.tx_bb(1, seed=e["seed"], sigma=sigma)
        z, rad = R.normals(stream, n, 1, e["seed"])
        r = R.check(y, x, sigma, stream, e["seed"], cap=False, twin=(z, rad))
        print(R.describe("edge %s stream %d word %d seed %d pair %d" % (e["class"], stream, e["word"], e["seed"], e["pair"]), r))
        assert not r["broken"], (e, r["broken"])
        noise = y[0, 2 * k:2 * k + 2].astype(np.float64) - x[0, 2 * k:2 * k + 2]
        bar = float(sigma) * R.EPS * max(1.0, rad[0, k]) + R.ROUND * np.maximum(np.abs(x[0, 2 * k:2 * k + 2]), np.abs(y[0, 2 * k:2 * k + 2])).astype(np.float64)
        if e["class"] in ("A", "A2"):
            assert rad[0, k] < R.NEAR_ONE
            if e["class"] == "A":
                assert bits_equal(y[0, 2 * k:2 * k + 2], x[0, 2 * k:2 * k + 2]), e
            else:
                assert np.all(np.isfinite(noise)) and np.max(np.abs(noise)) <= float(sigma) * 2.0 ** -10, (e, noise)
        elif e["class"] == "B":
            assert rad[0, k] >= 5.8 and np.hypot(noise[0], noise[1]) >= 5.8 * float(sigma), (e, noise)
        else:
            assert abs(noise[1]) <= bar[1] and abs(noise[0] - float(sigma) * rad[0, k]) <= bar[0], (e, noise, rad[0, k])
