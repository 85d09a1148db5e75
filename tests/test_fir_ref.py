"""The test of the tests: tests/fir_ref.py (float64 references, the CPU model of the matrix-core kernels' three-part split) and the bars of
tests/test_fir_fp64_gpu.py and of the correlator tests in tests/test_sync_gpu.py, on the CPU.

What the model shows, product by product (tap part, sample part; x = seen: the model with that product left out breaks the family's bar,
while the model with all six meets it):

    family                          (0,0)  (0,1)  (1,0)  (0,2)  (1,1)  (2,0)
    impulse gives the taps            x             x                    x       the sample is (1, 0, 0): products with x2, x3 are zero
    delta tap gives a delayed copy    x      x             x                     the tap is (b, 0, 0): products with b2, b3 are zero
    one tap 1 + 2^-10                 x      x      x      x      x              b3 = 0; (2,0) is seen by the impulse and random families
    random input against float64      x      x      x      x      x      x      every case of RANDOM_FIR / RANDOM_UPFIR
    power-of-two gain, call cuts                                                 see no product (they pin staging, seams, filter memory)

No product goes unseen, and each is seen by at least two families.  The correlators have one tap part (+-1 is exact in bf16) and three sample
parts: the random-input bar there (2 x the oracle chain's error) sees the third part, the {1, j, -1, -j} family the first.
"""
import numpy as np
import pytest

import fir_ref as R

SIX = sorted(R.ALL_SIX)


def _without(p):
    return tuple(q for q in R.ALL_SIX if q != p)


# ---------------------------------------------------------------------------------------------------------------- the references themselves
def test_split3_is_exact():
    rng = np.random.default_rng(1)
    edge = np.array([1 - 2.0 ** -24, 1 + 2.0 ** -23, 1 - 2.0 ** -9, 1 + 2.0 ** -8, 1 - 2.0 ** -17, 2 - 2.0 ** -23, 0.5 + 2.0 ** -24, 2.0 ** -9 - 2.0 ** -33,
                     255.5, 256.5, 257.0, 3.0 * 2.0 ** -40, 1.0, 0.0], np.float32)
    for v in (rng.standard_normal(1000000).astype(np.float32), R.srrc(81), R.srrc(41), np.concatenate([edge, -edge]),
              (rng.standard_normal(100000) * 2.0 ** rng.integers(-20, 21, 100000)).astype(np.float32)):
        p1, p2, p3 = R.split3(v)
        for p in (p1, p2, p3):
            assert not (p.view(np.uint32) & np.uint32(0xffff)).any()                  # bf16 values
        assert np.array_equal((p1 + p2) + p3, v) and np.array_equal(p3 + p2 + p1, v)  # float32 sums, either order
        assert np.array_equal(p1.astype(np.float64) + p2 + p3, v.astype(np.float64))
    assert np.array_equal(R.bf16_rne(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23], np.float32)),
                          np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7], np.float32))  # ties to even, above a tie up


def test_fir64_and_upfir64_against_numpy():
    rng = np.random.default_rng(2)
    for T, n in ((1, 50), (2, 7), (17, 300), (81, 40000), (98, 1000)):
        taps, hist, x = rng.standard_normal(T), rng.standard_normal(2 * (T - 1)), rng.standard_normal(2 * n)
        y, ya = R.fir64(taps, hist, x)
        for pl in range(2):
            ext = np.concatenate([hist[pl::2], x[pl::2]])
            assert np.allclose(y[pl::2], np.convolve(ext, taps)[T - 1:T - 1 + n], rtol=0, atol=1e-12)
            assert np.allclose(ya[pl::2], np.convolve(np.abs(ext), np.abs(taps))[T - 1:T - 1 + n], rtol=0, atol=1e-12)
        for osf in (2, 4):
            Hin = (T - 1) // osf
            hin = rng.standard_normal(2 * Hin)
            up = np.zeros((n, osf, 2)); up[:, 0] = x.reshape(-1, 2)
            uh = np.zeros((Hin + 1, osf, 2)); uh[1:, 0] = hin.reshape(-1, 2)              # the zero-stuffed past, cut to its last T - 1 samples
            uh = uh.reshape(-1, 2)[uh.shape[0] * osf - (T - 1):].reshape(-1)
            yu, yua = R.upfir64(taps, osf, hin, x)
            yz, yza = R.fir64(taps, uh, up.reshape(-1))
            assert np.allclose(yu, yz, rtol=0, atol=1e-12) and np.allclose(yua, yza, rtol=0, atol=1e-12)


def test_corr64_against_numpy(O):
    sof, plsc = O.sync_frame_taps()
    assert sof.size == 25 and plsc.size == 64 and set(np.abs(sof)) == {1.0} and set(np.abs(plsc)) <= {0.0, 1.0}
    rng = np.random.default_rng(3)
    x, zp = rng.standard_normal(2 * 500), rng.standard_normal(64) + 1j * rng.standard_normal(64)
    z = np.concatenate([zp, R.c_of(x)])
    d = np.concatenate([[0], z[:-1] * np.conj(z[1:])])
    for taps in (sof, plsc):
        assert np.allclose(R.corr64(x, taps, zp), np.convolve(d, taps)[64:64 + 500], rtol=0, atol=1e-12)


def test_impulse_stream_reaches_every_phase_and_seam():
    at = np.array(R.IMPULSE_AT)
    assert np.all(np.diff(at) >= 96) and set(at % 16) == set(range(16))
    for seam in (2048, 4096, 6144, R.IMPULSE_CUT):
        assert np.any((at >= seam - 80) & (at < seam)), seam
    assert R.IMPULSE_CUT % 16 == 0 and R.N3 == 3 * 2048 + 5


# ---------------------------------------------------------------------------------------------------------------- which bar sees which product
def _random_cases(O):
    """(name, taps, osf, x, y64, yabs, oracle chain's output): the GPU tests' inputs, the calls of a case as one stream from a reset handle
    (srrc81: its first call only -- the statistics do not need three)"""
    for table, osf in ((R.RANDOM_FIR, 1), (R.RANDOM_UPFIR, 2)):
        for name, (taps_fn, _, seed, calls) in table.items():
            taps = taps_fn()
            x = np.concatenate(R.gauss_calls(seed, calls)[:1 if name == "srrc81" else None])
            H = taps.size - 1
            if osf == 1:
                y64, yabs = R.fir64(taps, np.zeros(2 * H, np.float32), x)
                yo = O.fir(taps, np.zeros(2 * H, np.float32), x)
            else:
                y64, yabs = R.upfir64(taps, osf, np.zeros(2 * (H // osf), np.float32), x)
                yo = O.upfir(taps, osf, np.zeros(2 * H, np.float32), x)
            yield ("filter " if osf == 1 else "shape_filter ") + name, taps, osf, x, y64, yabs, yo


@pytest.fixture(scope="module")
def random_cases(O):
    return list(_random_cases(O))


def test_oracle_chain_stays_inside_its_own_bound(random_cases):
    """a chain of T fp32 fmas is within T 2^-24 sum |b| |x| of the exact sum; the yardstick is held to twice that, the bar of the GPU tests"""
    for name, taps, osf, x, y64, yabs, yo in random_cases:
        assert np.all(np.abs(yo - y64) <= taps.size * 2.0 ** -23 * yabs), name
        e = R.err_stats(yo, y64)
        assert 0 < e.rms < e.max < 1e-5, (name, e)


def _meets_random_bar(y, y64, yabs, yo, T):
    eg, er = R.err_stats(y, y64), R.err_stats(yo, y64)
    return bool(np.all(np.abs(y - y64) <= T * 2.0 ** -23 * yabs) and eg.max <= er.max and eg.rms <= er.rms)


def _seen(full_ok, ok_without):
    """the products a family sees; the model with all six has to meet its bar"""
    assert full_ok
    return {p for p in SIX if not ok_without(p)}


def test_every_product_is_seen_by_the_bars(random_cases):
    """the table of the module's docstring, from the model"""
    seen = {}
    # impulse: equality with the taps
    x = R.impulse_stream()
    sets = [R.srrc(81), R.srrc(41)] + [R.random_taps(T) for T in (1, 2, 16, 17, 49, 80, 81)]
    seen["impulse"] = _seen(all(np.array_equal(R.model_mfma(t, x), R.impulse_response(t)) for t in sets),
                            lambda p: all(np.array_equal(R.model_mfma(t, x, _without(p)), R.impulse_response(t)) for t in sets))
    for T in (2, 3, 81, 96, 97, 98, 99):
        t = R.random_taps(T)
        assert np.array_equal(R.model_mfma(t, x, osf=2), R.impulse_response(t, osf=2))
    # delta taps: equality with the delayed copy
    x = np.random.default_rng(40).standard_normal(2 * R.N3).astype(np.float32)
    cases = [(j, s) for j in (0, 47, 80) for s in (1.0, -0.5)]
    seen["delta"] = _seen(all(np.array_equal(R.model_mfma(R.delta_taps(81, j, s), x), R.delayed(x, j, s)) for j, s in cases),
                          lambda p: all(np.array_equal(R.model_mfma(R.delta_taps(81, j, s), x, _without(p)), R.delayed(x, j, s)) for j, s in cases))
    for j in (0, 47, 48, 96):
        assert np.array_equal(R.model_mfma(R.delta_taps(97, j, -0.5), x, osf=2), R.delayed(x, j, -0.5, osf=2))
    # one tap 1 + 2^-10: 2^-22 |y64| (the model has no fp32 additions: its full form is 2^-28 off, the dropped b2 x3)
    taps = np.array([1.0 + 2.0 ** -10], np.float32)
    x = np.random.default_rng(43).standard_normal(2 * 100000).astype(np.float32)
    y64, _ = R.fir64(taps, np.zeros(0, np.float32), x)
    rel = lambda prods: np.max(np.abs(R.model_mfma(taps, x, prods) - y64) / np.abs(y64))
    assert rel(R.ALL_SIX) <= 2.0 ** -27
    assert 2.0 ** -19 < rel(_without((1, 1))) <= 2.0 ** -18                 # b2 x2 <= 2^-10 2^-8 |x|: eight times the bar and more
    seen["one tap"] = _seen(True, lambda p: rel(_without(p)) <= 2.0 ** -22)
    # random input: the three bars of _float64_bars, every case on its own
    for name, taps, osf, x, y64, yabs, yo in random_cases:
        seen[name] = _seen(_meets_random_bar(R.model_mfma(taps, x, osf=osf), y64, yabs, yo, taps.size),
                           lambda p: _meets_random_bar(R.model_mfma(taps, x, _without(p), osf=osf), y64, yabs, yo, taps.size))
    for k, v in seen.items():
        print("%-24s %s" % (k, " ".join("(%d,%d)" % p if p in v else "  .  " for p in SIX)))
    assert seen["impulse"] == {(0, 0), (1, 0), (2, 0)}
    assert seen["delta"] == {(0, 0), (0, 1), (0, 2)}
    assert seen["one tap"] == set(SIX) - {(2, 0)}
    for name, *_ in random_cases:
        assert seen[name] == set(SIX), name


def test_power_of_two_gain_and_cuts_see_no_product():
    """why those two families are in no column of the table: the model answers them the same with a product missing"""
    x = np.random.default_rng(41).standard_normal(2 * 5000).astype(np.float32)
    for p in SIX:
        y = R.model_mfma(R.srrc(81), x, _without(p))
        assert np.array_equal(R.model_mfma(R.srrc(81), np.float32(2.0 ** 20) * x, _without(p)), 2.0 ** 20 * y)
        a = R.model_mfma(R.srrc(81), x[:4000], _without(p))
        b = R.model_mfma(R.srrc(81), x[4000:], _without(p), hist=R.tail(x[:4000], 80))
        assert np.allclose(np.concatenate([a, b]), y, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the correlators
def test_correlator_bar_sees_the_third_sample_part(O):
    """32APSK-S, two calls of 5 frames: the model (d formed in fp32 as the kernels form it, one tap part, sums in float64) with its three sample
    parts is inside 2 x the oracle chain's error against corr64, for each correlation and each call; with the third part left out it is
    outside, max and rms"""
    modcod, F = R.SYNC_SHAPES[0]
    stream, n = R.sync_stream(O, modcod, F)
    flat = stream.reshape(-1)
    ref = R.oracle_corr(O, n, stream.reshape(2 * F, -1))
    d = R.diff32(flat, 1.0)
    for taps, yo in zip(O.sync_frame_taps(), ref):
        c64 = np.concatenate([R.corr64(stream[0].reshape(-1), taps, R.Z0), R.corr64(stream[1].reshape(-1), taps, R.c_of(stream[0].reshape(-1))[-64:])])
        assert np.allclose(c64, R.corr64(flat, taps, R.Z0), rtol=0, atol=1e-12)         # the memory of 64 samples is all a second call needs
        full = R.c_of(R.model_mfma(taps, d, ((0, 2), (0, 1), (0, 0))))
        two = R.c_of(R.model_mfma(taps, d, ((0, 1), (0, 0))))
        for call in range(2):
            s = slice(call * F * n, (call + 1) * F * n)
            er, ef, e2 = R.err_stats(yo[s], c64[s]), R.err_stats(full[s], c64[s]), R.err_stats(two[s], c64[s])
            assert 0 < er.rms and ef.max <= 2 * er.max and ef.rms <= 2 * er.rms, (call, ef, er)
            assert e2.max > 2 * er.max and e2.rms > 2 * er.rms, (call, e2, er)


def test_unit_stream_correlations_are_whole_numbers(O):
    x = R.unit_stream(3000)
    assert np.array_equal(R.diff32(x, 1.0).astype(np.float64), np.stack([(z := np.concatenate([[1.0], R.c_of(x)[:-1]]) * np.conj(R.c_of(x))).real, z.imag], 1).reshape(-1))
    for taps in O.sync_frame_taps():
        c = R.corr64(x, taps, R.Z0)
        assert np.array_equal(c, np.round(c)) and np.max(np.abs(c)) < 64 and np.max(np.abs(c)) > 8
        assert np.array_equal(R.c_of(R.model_mfma(taps, R.diff32(x, 1.0), ((0, 0),))), c)
