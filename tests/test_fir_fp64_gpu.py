"""The streaming filters against float64 (tests/fir_ref.py), both kernels behind dvbs2hip_filter / dvbs2hip_shape_filter: the matrix-core
form (k_fir_mfma.hip: three bf16 parts per operand, six products) and the fp32 vector form (k_fir.hip).

tests/test_fir_gpu.py holds both to 1e-4 of the oracle's fp32 chain, a bar that does not see the three products of weight 2^-16 (a kernel
that lost one of them is 3e-6 .. 2e-5 off).  Here:

  bit-exact families   an impulse gives the taps back (sees the products b1 x1, b2 x1, b3 x1), a delta tap gives a delayed copy (b1 x1,
                       b1 x2, b1 x3), a power-of-two gain and a cut of the stream into calls change no bit (these two see no product: they
                       pin the staging, the tile seams and the filter memory).
  a derived bar        one tap 1 + 2^-10: sees b2 x2 (up to 2^-18 |y| against a bar of 2^-22 |y|) and everything larger.
  random input         max and rms error against float64 no larger than the oracle's fp32 chain on the same input (sees all six), and
                       every element inside T 2^-23 sum |b| |x|.

tests/test_fir_ref.py shows on the CPU model that each bar sees the products listed; results/fir_fp64/README.md has the measured figures.
"""
import numpy as np
import pytest

import fir_ref as R

pytestmark = pytest.mark.gpu
KERNELS = ("mfma", "valu")


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


def _rx(Rx, taps, kernel, osf=2, max_frames=1):
    """a handle that filters with `taps` through the asked kernel family"""
    from dvbs2_amd import lib_binding as B
    rx = Rx("QPSK-S_8/9", max_frames=max_frames, fir_taps=taps, fir_osf=osf)
    if kernel == "valu":
        rx.set_filter_kernel(B.FIR_VALU)
    elif len(taps) <= 81:
        rx.set_filter_kernel(B.FIR_MFMA)
    # (more than 81 taps: the matched filter has no matrix-core form and FIR_MFMA is refused; the shaping filter takes it by itself when its
    #  branches fit -- the default)
    return rx


def _in_calls(fn, x, cuts, osf=1):
    """the stream x (interleaved) through fn in calls cut at `cuts` (complex samples)"""
    e = [0] + list(cuts) + [x.size // 2]
    return np.concatenate([fn(x[2 * a:2 * b]) for a, b in zip(e[:-1], e[1:]) if b > a])


# ---------------------------------------------------------------------------------------------------------------- bit-exact families
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("taps_of", ["srrc81", "srrc41", 1, 2, 16, 17, 49, 80, 81])
def test_impulse_gives_the_taps_back(Rx, kernel, taps_of):
    """x = 1 has the parts (1, 0, 0), so the sum is (b3 + b2) + b1, two exact additions: the response is the taps, bit for bit, in both
    planes, at every block phase, across the tile seams and across a call boundary"""
    taps = R.srrc(int(taps_of[4:])) if isinstance(taps_of, str) else R.random_taps(taps_of)
    rx = _rx(Rx, taps, kernel)
    y = _in_calls(lambda v: rx.filter(v, 1), R.impulse_stream(), (R.IMPULSE_CUT,))
    rx.close()
    assert np.array_equal(y, R.impulse_response(taps))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T", [2, 3, 81, 96, 97, 98, 99])
def test_shaping_impulse_gives_the_taps_back(Rx, kernel, T):
    """the two polyphase branches interleaved are the taps; 98 taps are the last the matrix-core form takes (branches of 49: it leaves out the
    band's first K step), 99 go to the vector kernel"""
    taps = R.srrc(81) if T == 81 else R.random_taps(T)
    rx = _rx(Rx, taps, kernel)
    y = _in_calls(lambda v: rx.shape_filter(v, 1, osf=2), R.impulse_stream(), (R.IMPULSE_CUT,))
    rx.close()
    assert np.array_equal(y, R.impulse_response(taps, osf=2))


@pytest.fixture(scope="module")
def full_mantissa():
    return np.random.default_rng(40).standard_normal(2 * R.N3).astype(np.float32)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("j", [0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80])
def test_delta_tap_gives_a_delayed_copy(Rx, full_mantissa, kernel, j):
    """1 and -0.5 have the parts (b, 0, 0): the sum is (x3 + x2) + x1 scaled by a power of two, exact: y[n] = s x[n - j] bit for bit"""
    for s in (1.0, -0.5):
        rx = _rx(Rx, R.delta_taps(81, j, s), kernel)
        y = _in_calls(lambda v: rx.filter(v, 1), full_mantissa, (2051,))
        rx.close()
        assert np.array_equal(y, R.delayed(full_mantissa, j, s)), s


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("j", [0, 47, 48, 96])
def test_shaping_delta_tap_gives_a_delayed_copy(Rx, full_mantissa, kernel, j):
    """97 taps, branches of 49 and 48: the branch of the tap's parity is the scaled, delayed input, the other branch zero"""
    for s in (1.0, -0.5):
        rx = _rx(Rx, R.delta_taps(97, j, s), kernel)
        y = _in_calls(lambda v: rx.shape_filter(v, 1, osf=2), full_mantissa, (2051,))
        rx.close()
        assert np.array_equal(y, R.delayed(full_mantissa, j, s, osf=2)), s


@pytest.mark.parametrize("kernel", KERNELS)
def test_power_of_two_gain_changes_no_bit(Rx, kernel):
    x = np.random.default_rng(41).standard_normal(2 * 5000).astype(np.float32)
    rx = _rx(Rx, R.srrc(81), kernel)
    y = rx.filter(x, 1)
    for k in (-20, 20):
        rx.filter_reset()
        g = np.float32(2.0 ** k)
        assert np.array_equal(rx.filter(g * x, 1), g * y), k
    rx.close()


def _float64_bars(kernel, name, y, y64, yabs, yo, T):
    """the random-input bars: every element inside T 2^-23 sum |b| |x|; max and rms error no larger than the oracle's fp32 chain's on the
    same input (the vector kernel, a chain of the same length in another order: 1.25 x the max, 1.1 x the rms)"""
    eg, er = R.err_stats(y, y64), R.err_stats(yo, y64)
    print("fir_fp64 %-22s %-4s gpu %r | oracle chain %r" % (name, kernel, eg, er))
    assert np.all(np.abs(y - y64) <= T * 2.0 ** -23 * yabs), name
    fm, fr = (1.0, 1.0) if kernel == "mfma" else (1.25, 1.1)
    assert eg.max <= fm * er.max and eg.rms <= fr * er.rms, (name, eg, er)


@pytest.mark.parametrize("kernel", KERNELS)
def test_cutting_the_stream_into_calls_changes_no_bit(O, Rx, kernel):
    """cuts at multiples of 16 keep every sample at its place in the matrix-core kernel's blocks: same bits.  Any other cut moves the block
    phase (another order of the same additions): the vector kernel, one chain per output, still gives the same bits, the matrix-core kernel
    is held to the float64 bars."""
    taps = R.srrc(81)
    x = np.random.default_rng(42).standard_normal(2 * R.N3).astype(np.float32)
    rx = _rx(Rx, taps, kernel)
    whole = rx.filter(x, 1)
    rx.filter_reset()
    assert np.array_equal(_in_calls(lambda v: rx.filter(v, 1), x, (16, 2048, 2048 + 80, 4112)), whole)
    rx.filter_reset()
    odd = _in_calls(lambda v: rx.filter(v, 1), x, (1, 7, 2049))
    rx.close()
    if kernel == "valu":
        assert np.array_equal(odd, whole)
    else:
        y64, yabs = R.fir64(taps, np.zeros(160, np.float32), x)
        _float64_bars(kernel, "srrc81 cut at 1, 7, 2049", odd, y64, yabs, O.fir(taps, np.zeros(160, np.float32), x), 81)


# ---------------------------------------------------------------------------------------------------------------- a derived bar
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_tap_with_two_parts(Rx, kernel):
    """b = 1 + 2^-10 = (1, 2^-10, 0).  The matrix-core sum b2 x2 + b1 x3 + b2 x1 + b1 x2 + b1 x1 is five fp32 additions of which only the last
    two act on terms above 2^-8 |y|, each within 2^-23 of its partial sum whether the unit rounds or truncates; b2 x3 (2^-28 |y|) is
    dropped: |y - y64| <= 2^-22 |y64|.  (Without b2 x2 the model is up to 2^-18 |y| off.)  The vector kernel is one fma: 2^-24 |y64|."""
    taps = np.array([1.0 + 2.0 ** -10], np.float32)
    x = np.random.default_rng(43).standard_normal(2 * 100000).astype(np.float32)
    rx = _rx(Rx, taps, kernel)
    y = rx.filter(x, 1)
    rx.close()
    y64, _ = R.fir64(taps, np.zeros(0, np.float32), x)
    rel = np.max(np.abs(y - y64) / np.abs(y64))
    print("fir_fp64 one tap 1 + 2^-10     %-4s max |y - y64| / |y64| = 2^%.2f" % (kernel, np.log2(rel) if rel > 0 else -np.inf))
    assert np.all(np.abs(y - y64) <= 2.0 ** (-22 if kernel == "mfma" else -24) * np.abs(y64))


# ---------------------------------------------------------------------------------------------------------------- random input against float64
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", list(R.RANDOM_FIR))
def test_matched_filter_against_float64(O, Rx, kernel, case):
    taps_fn, osf, seed, calls = R.RANDOM_FIR[case]
    taps = taps_fn()
    T = taps.size
    rx = _rx(Rx, taps, kernel, osf=osf, max_frames=max(F for _, F in calls))
    xs = R.gauss_calls(seed, calls)
    ohist = np.zeros(2 * (T - 1), np.float32)
    out = [[], [], [], []]
    for i, ((n, F), x) in enumerate(zip(calls, xs)):
        y = rx.filter(x, n_frames=F)
        y64, yabs = R.fir64(taps, R.tail(np.concatenate(xs[:i] + [np.zeros(0, np.float32)]), T - 1), x)
        for o, v in zip(out, (y, y64, yabs, O.fir(taps, ohist, x))):
            o.append(v)
    rx.close()
    _float64_bars(kernel, "filter " + case, *[np.concatenate(o) for o in out], T)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", list(R.RANDOM_UPFIR))
def test_shaping_filter_against_float64(O, Rx, kernel, case):
    taps_fn, osf, seed, calls = R.RANDOM_UPFIR[case]
    taps = taps_fn()
    T = taps.size
    rx = _rx(Rx, taps, kernel, osf=osf, max_frames=max(F for _, F in calls))
    xs = R.gauss_calls(seed, calls)
    ohist = np.zeros(2 * (T - 1), np.float32)
    out = [[], [], [], []]
    for i, ((n, F), x) in enumerate(zip(calls, xs)):
        y = rx.shape_filter(x, n_frames=F, osf=osf)
        y64, yabs = R.upfir64(taps, osf, R.tail(np.concatenate(xs[:i] + [np.zeros(0, np.float32)]), (T - 1) // osf), x)
        for o, v in zip(out, (y, y64, yabs, O.upfir(taps, osf, ohist, x))):
            o.append(v)
    rx.close()
    _float64_bars(kernel, "shape_filter " + case, *[np.concatenate(o) for o in out], T)


def test_long_stream_four_tiles_per_workgroup_against_float64(O, Rx, tmp_path):
    """3073 tiles in one call: the matrix-core kernel's workgroups take four tiles each (three carries of the overlap inside LDS), the last one
    a single ragged tile -- as `plan_probe fir` (fir_choose, dvbs2_amd/csrc/rx_dispatch.h) says of this call"""
    from test_plan_digest import build_probe
    from test_rx_dispatch import ask
    build_probe(str(tmp_path / "plan_probe"))
    line = ask(str(tmp_path / "plan_probe"), "fir", [(81, R.LONG_N, 1, 16, 16, 1)], inherit=True)[0]
    print("fir_fp64 long stream: " + line)
    assert line == "fir_mfma_kernel<1> | grid %d x 1 tiles_per_wg 4" % -(-(-(-R.LONG_N // 2048)) // 4) and -(-R.LONG_N // 2048) % 4 == 1
    taps = R.srrc(81)
    x = np.random.default_rng(44).standard_normal(2 * R.LONG_N).astype(np.float32)
    rx = _rx(Rx, taps, "mfma")
    y = rx.filter(x, 1)
    rx.close()
    hist = np.zeros(160, np.float32)
    y64, _ = R.fir64(taps, hist, x, with_abs=False)
    eg, er = R.err_stats(y, y64), R.err_stats(O.fir(taps, hist, x), y64)
    print("fir_fp64 %-22s %-4s gpu %r | oracle chain %r" % ("filter srrc81 long", "mfma", eg, er))
    assert eg.max <= er.max and eg.rms <= er.rms, (eg, er)
