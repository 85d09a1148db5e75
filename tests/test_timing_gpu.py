"""The timing synchronizer and the channel's delay tasks on the GPU against the CPU twin (tests/timing_twin.c), bit for bit: Y_N1, B_N1, MU, Y_N2, UFW, RDY over three
consecutive calls (the loop state and the carry buffers cross call boundaries), 1 to 1000 streams per call with ragged delays, an underflowing stream, reset and the
stream-count check."""
import numpy as np
import pytest

import timing_ref as TR
from dvbs2_amd import params as P

pytestmark = pytest.mark.gpu


def streams(mc, S, Fs, calls, seed):
    """S streams of calls * Fs frames each: windows of four base signals (channel delays 2, 2.25, 2.5, 2.75) at ragged sample offsets -> [calls] arrays of S * Fs frames"""
    N = 2 * mc.pl_frame
    rng = np.random.default_rng(seed)
    pts = P.normalise_constellation(P.load_constellation(mc.cstl_file))
    pts = pts[:, 0] + 1j * pts[:, 1] if pts.ndim == 2 else pts
    L = calls * Fs * N
    span = 4000
    bases = [TR.shaped_stream(L + span, pts, D, 0.05, rng) for D in (2.0, 2.25, 2.5, 2.75)]
    out = np.empty((S, 2 * L), np.float32)
    for s in range(S):
        off = (s * 37 + s // 4) % span
        out[s] = bases[s % 4][2 * off: 2 * (off + L)]
    return [np.ascontiguousarray(out[:, 2 * c * Fs * N: 2 * (c + 1) * Fs * N]).reshape(S * Fs, 2 * N) for c in range(calls)]


@pytest.mark.parametrize("modcod,S,Fs", [("QPSK-S_8/9", 1, 3), ("QPSK-S_8/9", 7, 2), ("QPSK-S_8/9", 64, 1), ("QPSK-S_8/9", 1000, 1),
                                         ("16APSK-S_8/9", 1, 2), ("16APSK-S_8/9", 7, 1), ("16APSK-S_8/9", 64, 1)])
def test_synchronize_and_extract_match_the_twin(modcod, S, Fs):
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod(modcod)
    xs = streams(mc, S, Fs, 3, seed=S + Fs)
    rx = Dvbs2Hip(modcod, max_frames=S * Fs)
    if S > 1:
        rx.sync_timing_set_streams(S)
    tw = TR.Timing(mc.pl_frame, S)
    for c, X in enumerate(xs):
        Y, B, MU = rx.sync_timing_synchronize(X)
        Yt, Bt, MUt = tw.synchronize(X)
        assert np.array_equal(B, Bt), (c, np.argwhere(B != Bt)[:4])
        assert np.array_equal(Y.view(np.uint32), Yt.view(np.uint32)), (c, np.argwhere(Y != Yt)[:4])
        assert np.array_equal(MU.view(np.uint32), MUt.view(np.uint32)), c
        Y2, UFW, RDY = rx.sync_timing_extract(Y, B)
        Y2t, UFWt, RDYt = tw.extract(Yt, Bt)
        assert np.array_equal(RDY, RDYt) and np.array_equal(UFW, UFWt), c
        assert np.array_equal(Y2.view(np.uint32), Y2t.view(np.uint32)), c
    assert 0.02 < float(np.abs(MU).mean()) < 0.98 or S == 1            # the loops are running
    rx.close()


def test_extract_underflow_holds_the_symbols_and_releases_them_next_call():
    """seven streams of two frames; stream 3 strobes slower than nominal (a stream sampled faster than its symbol rate) and runs short; the others are nominal or ahead"""
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod("QPSK-S_8/9")
    N, S, Fs = 2 * mc.pl_frame, 7, 2
    rng = np.random.default_rng(11)
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=S * Fs)
    rx.sync_timing_set_streams(S)
    tw = TR.Timing(mc.pl_frame, S)
    held = None
    for c in range(3):
        Y = rng.standard_normal((S * Fs, 2 * N)).astype(np.float32)
        B = np.zeros((S * Fs, N), np.int32)
        B[:, 1::2] = 1                                                        # one strobe every other sample: exactly N reals per frame
        Bs = B.reshape(S, -1)
        Bs[1, 5::4001] = 1                                                    # stream 1 strobes a little more often: its carry buffer grows
        Bs[2, 8] = 1; Bs[2, 9] = 0                                          # stream 2: one strobe moved
        if c == 0:
            Bs[3, 1:2 * 4001:4001 // 2 * 2] = 0                              # stream 3 misses a few strobes: underflow
        B = np.repeat(Bs.reshape(S * Fs, N), 2, axis=1)                       # both reals of a sample
        Y2, UFW, RDY = rx.sync_timing_extract(Y, B)
        Y2t, UFWt, RDYt = tw.extract(Y, B)
        assert np.array_equal(RDY, RDYt) and np.array_equal(UFW, UFWt), c
        assert np.array_equal(Y2.view(np.uint32), Y2t.view(np.uint32)), c
        if c == 0:
            assert RDY.tolist() == [1, 1, 1, 0, 1, 1, 1]
            assert UFW.reshape(S, Fs)[3].tolist() == [0, 1] and UFW.sum() == 1       # the output reached the second frame
            Ys, Bsx = Y.reshape(S, -1), B.reshape(S, -1)
            held = Ys[3][Bsx[3] != 0]
            assert held.size < Fs * N
        if c == 1:
            assert RDY.tolist() == [1] * S
            assert UFW.reshape(S, Fs)[3].tolist() == [0, 1]                      # reported by the ready call
            assert np.array_equal(Y2.reshape(S, -1)[3][: held.size], held)       # the held reals come out first
        if c == 2:
            assert not UFW.any()
    rx.close()


def test_reset_returns_the_first_calls_output_and_streams_must_divide_the_batch():
    from dvbs2_amd.receiver import Dvbs2Hip
    from dvbs2_amd.lib_binding import Dvbs2HipError
    mc = P.get_modcod("QPSK-S_8/9")
    X0, X1 = streams(mc, 2, 1, 2, seed=5)
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=4)
    rx.sync_timing_set_streams(2)
    first = rx.sync_timing_synchronize(X0)
    e1 = rx.sync_timing_extract(first[0], first[1])
    second = rx.sync_timing_synchronize(X1)
    assert not np.array_equal(second[0], first[0])
    rx.sync_timing_reset()
    again = rx.sync_timing_synchronize(X0)
    e2 = rx.sync_timing_extract(again[0], again[1])
    for a, b in zip(first + e1, again + e2):
        assert np.array_equal(a, b)
    with pytest.raises(Dvbs2HipError) as ei:
        rx.sync_timing_synchronize(np.zeros((3, 4 * mc.pl_frame), np.float32))      # 3 frames, 2 streams
    assert ei.value.code == -1
    with pytest.raises(Dvbs2HipError) as ei:
        rx.sync_timing_set_streams(5)                                               # more streams than frames per call
    assert ei.value.code == -1
    rx.close()


def test_gains_are_the_twins():
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip("QPSK-S_8/9")
    assert rx.sync_timing_gains() == tuple(float(g) for g in TR.gains())
    rx.sync_timing_set_params(0.9, 1e-3, 1.5)
    assert rx.sync_timing_gains() == tuple(float(g) for g in TR.gains(np.float32(0.9), 1e-3, 1.5))
    rx.close()


@pytest.mark.parametrize("D", [2.0, 4.5, 4.25, 5.0, 40000.7])
def test_channel_delay_matches_the_twin(D):
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod("QPSK-S_8/9")
    rng = np.random.default_rng(int(D * 10))
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=3)
    rx.channel_set_delay(D)
    tw = TR.ChannelDelay(D)
    for F in (1, 3, 2):
        X = rng.standard_normal((F, 4 * mc.pl_frame)).astype(np.float32)
        Y = rx.channel_delay(X)
        assert np.array_equal(Y.view(np.uint32), tw(X).view(np.uint32).reshape(Y.shape))
    with pytest.raises(Exception):
        rx.channel_set_delay(1.5)                                                  # DVBS2.cpp:129-133
    rx.close()
