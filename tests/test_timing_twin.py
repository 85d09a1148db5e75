"""The CPU twin of the timing synchronizer (tests/timing_twin.c): pinned by a pure-Python restatement, locking on a delayed stream, the reference's loop gains.
No GPU needed: these hold the yardstick that tests/test_timing_gpu.py holds libdvbs2hip's kernels to."""
import numpy as np
import pytest

import timing_ref as TR
import twin_build
from dvbs2_amd import params as P

PL = P.get_modcod("QPSK-S_8/9").pl_frame          # 8370 symbols, 16740 complex samples per frame at osf = 2


QPSK = np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2)


def qpsk_stream(F, D, noise, seed):
    """F frames of the timing loop's input: QPSK shaped, delayed by the twin's channel, noisy, matched-filtered"""
    return TR.shaped_stream(F * 2 * PL, QPSK, D, noise, np.random.default_rng(seed)).reshape(F, -1)


def test_twin_equals_the_python_restatement_bit_for_bit():
    X = qpsk_stream(2, 4.5, 0.05, seed=3)
    kp, ki = TR.gains()
    n = 700
    y, b, mu, _ = TR.py_synchronize(X.ravel()[:2 * n].view(np.complex64), kp, ki)
    Y, B, MU = TR.Timing(PL).synchronize(X)
    assert np.array_equal(Y.ravel()[:2 * n].view(np.complex64), y)
    assert np.array_equal(B.ravel()[0:2 * n:2], b) and np.array_equal(B.ravel()[1:2 * n:2], b)
    assert b.sum() > n // 2 - 2                                   # about one strobe every other sample
    # and the stream carries on bit for bit across calls of one frame each
    t = TR.Timing(PL)
    Ya, Ba, MUa = t.synchronize(X[:1])
    Yb, Bb, MUb = t.synchronize(X[1:])
    assert np.array_equal(np.concatenate([Ya.ravel(), Yb.ravel()]), Y.ravel()) and np.array_equal(np.concatenate([Ba.ravel(), Bb.ravel()]), B.ravel())
    assert np.array_equal(np.concatenate([MUa, MUb]), MU)


def test_twin_equals_the_restatement_through_stuffing_and_skipping():
    """a fast loop (nbw 2e-2) on a noisy stream: the strobe history takes all four values (stuffing h = 3 and skipping h = 0 included) and the loop filter moves;
    the twin's Y, B and mu after the frame equal the restatement's bit for bit over a whole frame"""
    X = TR.shaped_stream(2 * PL, QPSK, 5.0, 0.3, np.random.default_rng(3)).reshape(1, -1)
    t = TR.Timing(PL, 1, np.float32(0.5 ** 0.5), 2e-2, 2.0)
    y, b, mu, h = TR.py_synchronize(X.ravel().view(np.complex64), t.kp, t.ki)
    assert (np.bincount(h, minlength=4) > 50).all(), np.bincount(h)
    Y, B, MU = t.synchronize(X)
    assert np.array_equal(Y.ravel().view(np.complex64), y) and np.array_equal(B.ravel()[0::2], b)
    assert MU.view(np.uint32)[0] == np.float32(mu).view(np.uint32)
    assert t.st[0].lf_prev_in != 0.0


def test_loop_gains_are_the_reference_formula():
    """Synchronizer_Gardner_fast_osf2::set_loop_filter_coeffs (.cpp:188-198) for the factory defaults sqrt(0.5), 5e-5, 2"""
    kp, ki = TR.gains()
    z, bn, g = 0.5 ** 0.5, 5e-5, 2.0
    th = bn / 2 / (z + 0.25 / z)
    d = (1 + 2 * z * th + th * th) * -1 * g
    assert abs(kp - 4 * z * th / d) <= 1e-6 * abs(kp) and abs(ki - 4 * th * th / d) <= 1e-6 * abs(ki)
    assert kp < 0 and ki < 0 and abs(kp) == pytest.approx(3.3332e-5, rel=1e-3)


@pytest.mark.parametrize("D", [4.0, 4.5, 4.25])
def test_loop_locks_behind_the_channel_delay(D):
    """at high SNR the loop settles on the symbol instants: mu at the delay's fractional phase ((-D) mod 1: the channel's Farrow delays by 2 - frac(D) after a line of
    floor(D) - 2 samples) and the extracted symbols on the QPSK points"""
    F = 64                                                        # ~64 k symbols = 3.2 / nbw to lock, then the ringing settles (from the unstable point at D = 4)
    X = qpsk_stream(F, D, 0.05, seed=int(D * 100))
    t = TR.Timing(PL)
    Y, B, MU = t.synchronize(X)
    Y2, UFW, RDY = t.extract(Y, B)
    assert RDY.tolist() == [1] and not UFW.any()
    want = (-D) % 1.0
    err = np.abs((MU[-6:] - want + 0.5) % 1.0 - 0.5)
    assert err.max() < 0.07, (MU[-6:], want)
    s = Y2[-2:].ravel().view(np.complex64).astype(complex)
    s = s / (np.abs(s.real).mean() * np.sqrt(2))
    ideal = (np.sign(s.real) + 1j * np.sign(s.imag)) / np.sqrt(2)
    evm = np.sqrt(np.mean(np.abs(s - ideal) ** 2))
    assert evm < 0.15, evm


def test_twin_extract_holds_an_underflowing_stream_and_releases_it():
    """a stream with fewer strobes than output slots: not ready, everything kept in the carry buffer, the underflow counted on the frame reached; the next call
    puts the held reals first"""
    N = 2 * PL
    t = TR.Timing(PL)
    Y = np.arange(2 * N, dtype=np.float32).reshape(1, -1)
    B = np.zeros((1, 2 * N), np.int32)
    B[0, : N - 10] = 1                                           # 10 reals short of one frame's output
    Y2, UFW, RDY = t.extract(Y, B)
    assert RDY.tolist() == [0] and UFW.tolist() == [1] and t.head == [N - 10]
    B2 = np.ones((1, 2 * N), np.int32)
    Y2b, UFW2, RDY2 = t.extract(Y + 1e5, B2)
    assert RDY2.tolist() == [1] and UFW2.tolist() == [1]           # reported once by the ready call, then cleared
    assert np.array_equal(Y2b[0, : N - 10], Y[0, : N - 10]) and np.array_equal(Y2b[0, N - 10:], Y[0, :10] + 1e5)
    assert t.head == [2 * N - 10]                                  # 2N strobed reals, 10 of them emitted: 2N - 10 held
    _, UFW3, _ = t.extract(Y, B2)
    assert UFW3.tolist() == [0]


def test_channel_delay_twin_is_a_delay_line_then_the_farrow_filter():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(2 * 1000).astype(np.float32)
    for D in (2.0, 4.0, 7.0):                                     # integer D: floor(D) - 2 samples of delay line + the Farrow filter's two at mu = 0
        y = TR.ChannelDelay(D)(x)
        k = int(D)
        assert np.array_equal(y[2 * k:], x[: x.size - 2 * k]) and not y[: 2 * k].any()
    ch = TR.ChannelDelay(4.5)
    whole = ch(x)
    ch2 = TR.ChannelDelay(4.5)
    parts = np.concatenate([ch2(x[:6]), ch2(x[6:800]), ch2(x[800:])])      # history across calls, including a call shorter than the history
    assert np.array_equal(whole, parts)


def test_twin_cache_key_covers_the_included_headers(tmp_path):
    """an edit to a header a twin includes must not reuse the cached shared object: on copies of timing_twin.c and gardner_twin.h, a comment appended to the header
    changes the key and the file the loader builds"""
    import os
    import shutil
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ("timing_twin.c", "gardner_twin.h"):
        shutil.copy(os.path.join(here, f), tmp_path / f)
    src = str(tmp_path / "timing_twin.c")
    assert twin_build.sources(src) == [src, str(tmp_path / "gardner_twin.h")]
    k0, so0 = twin_build.key(src), twin_build.load(src)._name
    assert k0 == twin_build.key(os.path.join(here, "timing_twin.c")) and k0 in so0
    with open(tmp_path / "gardner_twin.h", "a") as f:
        f.write("/* edited */\n")
    k1, so1 = twin_build.key(src), twin_build.load(src)._name
    assert k1 != k0 and so1 != so0 and k1 in so1
