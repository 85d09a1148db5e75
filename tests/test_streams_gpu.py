"""dvbs2hip_set_streams on the GPU: S independent streams per call through the block-wise matched filter, the frame synchronizer and L&R (stream s = frames
[s F/S, (s+1) F/S) of a call).  Every task is held to two things: S instances of the CPU oracle's objects at the bars the single-stream tests use (tests/test_fir_gpu.py,
tests/test_sync_gpu.py), and S single-stream handles fed stream by stream in the same calls, bit for bit -- per stream the operations are the same."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_pl_frames, rot as _rot

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
FIR_TOL = 1e-4        # tests/test_fir_gpu.py
SYNC_TOL = 2e-4       # tests/test_sync_gpu.py


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def _split(a, S):
    """socket of F frames -> [S, F/S, ...]"""
    a = np.asarray(a)
    return a.reshape((S, a.shape[0] // S) + a.shape[1:])


def _code(fn, *a):
    from dvbs2_amd import lib_binding as B
    with pytest.raises(B.Dvbs2HipError) as e:
        fn(*a)
    return e.value.code


# ------------------------------------------------------------------ matched filter
@pytest.mark.parametrize("kernel", ["valu", "mfma"])
@pytest.mark.parametrize("S,calls", [(3, (3, 6, 3)), (5, (5,))])
def test_filter_streams_against_the_oracle_and_single_stream_handles(O, Rx, P, kernel, S, calls):
    """32APSK-S_3/4 at two samples per symbol (n_cplx = 6804: 3.3 tiles of 2048 per frame), the handle's 81 taps.  Calls of F/S = 1, 2, 1 frames per stream, and one call
    with more streams (5) than tiles per stream (4).  Stream 1 is all zeros in the first call: a sample of stream 0's tail read as stream 1's head would show as a non-zero
    output."""
    from dvbs2_amd import lib_binding as B
    kern = B.FIR_VALU if kernel == "valu" else B.FIR_MFMA
    taps = P.rrc_taps(0.2, 2, 20)
    n = 6804
    rng = np.random.default_rng(50 + S)
    rx = Rx("32APSK-S_3/4", max_frames=max(calls))
    rx.set_filter_kernel(kern)
    rx.set_streams(S)
    singles = [Rx("32APSK-S_3/4", max_frames=max(calls) // S) for _ in range(S)]
    hist = [np.zeros(2 * 80, np.float32) for _ in range(S)]
    for one in singles:
        one.set_filter_kernel(kern)
    for c, F in enumerate(calls):
        Fs = F // S
        x = rng.standard_normal((S, Fs * 2 * n)).astype(np.float32)
        if c == 0:
            x[1] = 0.0
        y = rx.filter(x, n_frames=F).reshape(S, -1)
        for s in range(S):
            yo = O.fir(taps, hist[s], x[s])
            assert np.max(np.abs(y[s] - yo)) <= FIR_TOL * max(1.0, float(np.abs(yo).max())), (c, s)
            ys = singles[s].filter(x[s], n_frames=Fs)
            assert np.array_equal(_bits(y[s]), _bits(ys)), (c, s)
        if c == 0:
            assert not y[1].any()
            assert np.abs(y[0][:2 * 40]).max() > 0.1 and np.abs(y[2][:2 * 40]).max() > 0.1
    rx.close()
    for one in singles:
        one.close()


# ------------------------------------------------------------------ frame synchronizer
_sync_cache = {}


def _sync_streams(O, modcod):
    """four streams of 12 frames, [4, 12, 2 n]: offset 777 that jumps to 877 after frame 6 (the delay line's "delay moved" branches run inside a batch), offset 0,
    offset n - 1, noise only; and per stream the oracle's DEL, TRI, FLG, Y_N2 frame by frame (computed once per mod-cod, read only)"""
    if modcod in _sync_cache:
        return _sync_cache[modcod]
    frames = 12
    xs = []
    n = None
    for s, off in enumerate((777, 0, -1)):
        _, pl, _, _ = make_pl_frames(O, modcod, frames + 1, 8.0, seed=60 + s)
        n = pl.shape[1] // 2
        off = n - 1 if off < 0 else off
        st = np.concatenate([np.zeros(2 * off, np.float32), pl.reshape(-1)])[:frames * 2 * n].reshape(frames, 2 * n).copy()
        if s == 0:
            moved = np.concatenate([np.zeros(2 * (off + 100), np.float32), pl.reshape(-1)])[:frames * 2 * n].reshape(frames, 2 * n)
            st[6:] = moved[6:]
        xs.append(st)
    xs.append((0.3 * np.random.default_rng(63).standard_normal((frames, 2 * n))).astype(np.float32))
    xs = np.stack(xs)
    ref = []
    for s in range(4):
        sf = O.SyncFrame(n, alpha=0.9, trigger=30.0, vec_width=8)
        rows = []
        for f in range(frames):
            d, Y = sf.synchronize(xs[s, f])
            rows.append((int(d), float(sf.metric), bool(sf.packet_flag), Y.copy()))
        ref.append(rows)
    assert len({r[0] for r in ref[0][6:]}) > 1                          # the jump is followed inside the run
    assert ref[0][8][0] != ref[0][9][0] and ref[1][-1][2] and ref[2][-1][2] and not any(r[2] for r in ref[3])      # (the delay moves at frame 9: inside the call of frames 8 .. 10)
    xs.setflags(write=False)
    _sync_cache[modcod] = (xs, ref, n)
    return _sync_cache[modcod]


@pytest.mark.parametrize("form", ["fused", "unfused", "valu"])
@pytest.mark.parametrize("modcod", ["32APSK-S_3/4", "QPSK-S_8/9"])
def test_frame_synchronizer_streams_against_the_oracle_and_single_stream_handles(O, Rx, monkeypatch, modcod, form):
    """S = 4 streams of 12 frames in calls of F/S = 1, 2, 3, 2, 3, 1 (32APSK-S_3/4: n = 3402 is no multiple of vec_width 8, so the unaveraged tail positions are in
    play), the one-task form, DVBS2HIP_SYNC_UNFUSED and DVBS2HIP_SYNC=valu.  Per stream against its own O.SyncFrame: DEL exact, Y_N2 bit-exact, TRI within
    2e-4 max(1, metric), FLG and get_metric[s] equal.  Against four single-stream handles: DEL, FLG, Y_N2 identical and TRI bit for bit -- at these frame counts the
    single-stream handle takes the single walk of the average over frames (a call is cut into segments only from F >= 1536 frames on: rx_dispatch.h, sync_choose),
    which is the recurrence the S-stream kernel runs."""
    monkeypatch.delenv("DVBS2HIP_SYNC", raising=False)
    monkeypatch.delenv("DVBS2HIP_SYNC_UNFUSED", raising=False)
    if form == "valu":
        monkeypatch.setenv("DVBS2HIP_SYNC", "valu")
    if form == "unfused":
        monkeypatch.setenv("DVBS2HIP_SYNC_UNFUSED", "1")
    xs, ref, n = _sync_streams(O, modcod)
    S = 4
    rx = Rx(modcod, max_frames=3 * S)
    rx.set_streams(S)
    singles = [Rx(modcod, max_frames=3) for _ in range(S)]
    f0 = 0
    for Fs in (1, 2, 3, 2, 3, 1):
        x = np.ascontiguousarray(xs[:, f0:f0 + Fs]).reshape(S * Fs, 2 * n)
        d, flg, tri, Y = (_split(a, S) for a in rx.sync_frame_synchronize(x, with_flags=True))
        m, flag = rx.sync_frame_metric()
        assert m.shape == (S,) and flag.shape == (S,)
        for s in range(S):
            for k in range(Fs):
                do, mo, fo, Yo = ref[s][f0 + k]
                assert d[s, k] == do, (s, f0 + k, d[s, k], do)
                assert np.array_equal(_bits(Y[s, k]), _bits(Yo)), (s, f0 + k)
                assert abs(tri[s, k] - mo) <= SYNC_TOL * max(1.0, mo) and bool(flg[s, k]) == fo, (s, f0 + k)
            mo, fo = ref[s][f0 + Fs - 1][1:3]
            assert abs(m[s] - mo) <= SYNC_TOL * max(1.0, mo) and bool(flag[s]) == fo, s
            d1, f1, t1, Y1 = singles[s].sync_frame_synchronize(xs[s, f0:f0 + Fs], with_flags=True)
            assert np.array_equal(d[s], d1) and np.array_equal(flg[s], f1) and np.array_equal(_bits(Y[s]), _bits(Y1)), (s, f0)
            assert np.array_equal(_bits(tri[s]), _bits(t1)), (s, f0)
        f0 += Fs
    assert not flg[3].any()                                             # noise only: no lock, packet flag clear
    rx.close()
    for one in singles:
        one.close()


def test_frame_synchronizer_two_task_form_equals_the_one_task_form_at_two_streams(O, Rx, monkeypatch):
    monkeypatch.delenv("DVBS2HIP_SYNC", raising=False)
    monkeypatch.delenv("DVBS2HIP_SYNC_UNFUSED", raising=False)
    xs, _, n = _sync_streams(O, "32APSK-S_3/4")
    a, b = Rx("32APSK-S_3/4", max_frames=6), Rx("32APSK-S_3/4", max_frames=6)
    a.set_streams(2); b.set_streams(2)
    f0 = 0
    for Fs in (1, 3, 2):
        x = np.ascontiguousarray(xs[:2, f0:f0 + Fs]).reshape(2 * Fs, 2 * n)
        d1, g1, t1, Y1 = a.sync_frame_synchronize(x, with_flags=True)
        cs, cp = b.sync_frame_synchronize1(x)
        d2, g2, t2, Y2 = b.sync_frame_synchronize2(x, cs, cp, with_flags=True)
        assert np.array_equal(d1, d2) and np.array_equal(g1, g2) and np.array_equal(_bits(t1), _bits(t2)) and np.array_equal(_bits(Y1), _bits(Y2)), f0
        f0 += Fs
    a.close(); b.close()


# ------------------------------------------------------------------ L&R
def test_lr_streams_against_the_oracle_and_single_stream_handles(O, Rx, monkeypatch):
    """QPSK-S_8/9, S = 3, calls of F/S = 1, 4, 1, every stream with a carrier offset of its own on PL-descrambled pilots.  Per stream against O.SyncLR: FRQ within 1e-6,
    Y within 4e-3 (the bars of tests/test_sync_gpu.py, test_fine_synchronizers_match_oracle); FRQ and Y bit for bit those of three single-stream handles in the
    three-kernel form (DVBS2HIP_LR=unfused), which is the form S > 1 always takes; no launch is counted as repeated."""
    modcod, S = "QPSK-S_8/9", 3
    _, pl, _, _ = make_pl_frames(O, modcod, 6, 10.0, seed=71)
    n = pl.shape[1] // 2
    xs = np.stack([np.stack([_rot(O, pl[(f + s) % 6], (1e-4, -2.5e-4, 4e-5)[s], 0.1 * f + 0.3 * s) for f in range(6)]) for s in range(S)])
    rx = Rx(modcod, max_frames=4 * S)
    rx.set_streams(S)
    rx.sync_lr_set_alpha(0.9)
    singles = [Rx(modcod, max_frames=4) for _ in range(S)]
    lrs = [O.SyncLR(n, alpha=0.9) for _ in range(S)]
    for one in singles:
        one.sync_lr_set_alpha(0.9)
    f0 = 0
    for Fs in (1, 4, 1):
        x = np.ascontiguousarray(xs[:, f0:f0 + Fs]).reshape(S * Fs, 2 * n)
        monkeypatch.delenv("DVBS2HIP_LR", raising=False)
        FRQ, PHS, Y = (_split(a, S) for a in rx.sync_lr_synchronize(x))
        monkeypatch.setenv("DVBS2HIP_LR", "unfused")
        for s in range(S):
            for k in range(Fs):
                fo, _, Yo = lrs[s].synchronize(xs[s, f0 + k])
                assert abs(FRQ[s, k] - fo) <= 1e-6 and PHS[s, k] == 0.0, (s, f0 + k)
                assert np.max(np.abs(Y[s, k] - Yo)) <= 4e-3, (s, f0 + k)
            F1, _, Y1 = singles[s].sync_lr_synchronize(xs[s, f0:f0 + Fs])
            assert np.array_equal(_bits(FRQ[s]), _bits(F1)) and np.array_equal(_bits(Y[s]), _bits(Y1)), (s, f0)
        f0 += Fs
    assert len({float(v) for v in FRQ[:, -1]}) == S                     # three carriers, three estimates
    assert rx.sync_lr_timeouts() == 0
    rx.close()
    for one in singles:
        one.close()


# ------------------------------------------------------------------ the entry's rules
def test_rules_of_the_entry(O, Rx, P):
    import torch
    modcod = "QPSK-S_8/9"
    rng = np.random.default_rng(80)
    rx = Rx(modcod, max_frames=6)
    n = rx.pl_frame
    assert _code(rx.set_streams, 0) == EINVAL
    rx.set_streams(3)
    x4 = rng.standard_normal((4, 2 * n)).astype(np.float32)
    assert _code(rx.filter, x4, 4) == EINVAL and "multiple of the stream count" in rx.L.dvbs2hip_last_error(rx.h).decode()
    assert _code(rx.sync_frame_synchronize, x4) == EINVAL
    assert _code(rx.sync_lr_synchronize, x4) == EINVAL
    assert rx.L.dvbs2hip_graph_begin(rx.h) == 0
    rc = rx.L.dvbs2hip_set_streams(rx.h, 2)
    g = C.c_int32(-1)
    assert rx.L.dvbs2hip_graph_end(rx.h, C.byref(g)) == 0
    if g.value >= 0:
        rx.graph_destroy(g.value)
    assert rc == EINVAL
    # set_streams(2) after calls at S = 3: what a handle that starts at S = 2 gives
    _, pl, _, _ = make_pl_frames(O, modcod, 6, 9.0, seed=81)
    stream = np.concatenate([np.zeros(2 * 55, np.float32), pl.reshape(-1)])[:6 * 2 * n].reshape(6, 2 * n)
    desc = np.stack([_rot(O, pl[f], 2e-4, 0.05 * f) for f in range(6)])
    for x in (stream, stream[::-1].copy()):
        rx.filter(x, 6); rx.sync_frame_synchronize(x); rx.sync_lr_synchronize(desc)
    rx.set_streams(2)
    fresh = Rx(modcod, max_frames=6)
    fresh.set_streams(2)
    for h in (rx, fresh):
        h.out = [h.filter(stream[:4], 4), h.sync_frame_synchronize(stream[:4], with_flags=True), h.sync_lr_synchronize(desc[:4]), h.sync_frame_metric()]
    for a, b in zip([rx.out[0], *rx.out[1], *rx.out[2], *rx.out[3]], [fresh.out[0], *fresh.out[1], *fresh.out[2], *fresh.out[3]]):
        assert _same(a, b)
    # the located form stays one stream per handle
    t = dict(X=torch.zeros(2 * 2 * n, dtype=torch.float32, device="cuda"), D=torch.zeros(2, dtype=torch.int32, device="cuda"), G=torch.zeros(2, dtype=torch.int32, device="cuda"),
             T=torch.zeros(2, dtype=torch.float32, device="cuda"), S=torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert rx.L.dvbs2hip_sync_frame_locate_dev(rx.h, t["X"].data_ptr(), t["D"].data_ptr(), t["G"].data_ptr(), t["T"].data_ptr(), t["S"].data_ptr(), 2) == EUNSUPPORTED
    rx.close(); fresh.close()
    # sync_timing_set_streams alone leaves the block-wise tasks at one stream: two frames are ONE stream, frame 1's head is read from frame 0's tail
    rx = Rx("32APSK-S_3/4", max_frames=2)
    rx.sync_timing_set_streams(2)
    x = rng.standard_normal(2 * 2 * 6804).astype(np.float32)
    y = rx.filter(x, 2)
    taps = P.rrc_taps(0.2, 2, 20)
    yo = O.fir(taps, np.zeros(160, np.float32), x)
    assert np.max(np.abs(y - yo)) <= FIR_TOL * max(1.0, float(np.abs(yo).max()))
    alone = O.fir(taps, np.zeros(160, np.float32), x[2 * 6804:])
    assert np.max(np.abs(y[2 * 6804:2 * 6804 + 80] - alone[:80])) > 0.1          # (not frame 1 filtered from an empty memory)
    rx.close()


def test_stream_count_changed_on_a_live_handle_back_to_one_stream(O, Rx, monkeypatch):
    """QPSK-S_8/9, one handle: set_streams(3) and two calls of 3 frames through filter, sync_frame_synchronize and L&R, then set_streams(1) and two calls of 2 frames.
    The one-stream calls -- back on the one-stream filter memory and in the one-stream launch forms, the second call continuing from the state the first left -- are bit
    for bit those of a fresh handle that never called the entry, sync_frame_metric included."""
    for v in ("DVBS2HIP_SYNC", "DVBS2HIP_SYNC_UNFUSED", "DVBS2HIP_LR"):
        monkeypatch.delenv(v, raising=False)
    modcod = "QPSK-S_8/9"
    _, pl, _, _ = make_pl_frames(O, modcod, 6, 9.0, seed=82)
    n = pl.shape[1] // 2
    stream = np.concatenate([np.zeros(2 * 55, np.float32), pl.reshape(-1)])[:6 * 2 * n].reshape(6, 2 * n)
    desc = np.stack([_rot(O, pl[f], 2e-4, 0.05 * f) for f in range(6)])
    rx, fresh = Rx(modcod, max_frames=3), Rx(modcod, max_frames=3)
    rx.set_streams(3)
    for f0 in (0, 3):
        rx.filter(stream[f0:f0 + 3], 3); rx.sync_frame_synchronize(stream[f0:f0 + 3]); rx.sync_lr_synchronize(desc[f0:f0 + 3])
    rx.set_streams(1)
    for f0 in (1, 3):
        outs = []
        for h in (rx, fresh):
            x, p = stream[f0:f0 + 2], desc[f0:f0 + 2]
            outs.append([h.filter(x, 2), *h.sync_frame_synchronize(x, with_flags=True), *h.sync_lr_synchronize(p), *h.sync_frame_metric()])
        assert len(outs[0]) == len(outs[1]) == 10
        for k, (a, b) in enumerate(zip(*outs)):
            assert _same(a, b), (f0, k)
        assert np.abs(outs[0][0]).max() > 0.1 and np.abs(outs[0][4]).max() > 0.1          # (the filter's and the synchronizer's outputs are not empty)
    assert rx.sync_lr_timeouts() == 0 and fresh.sync_lr_timeouts() == 0
    rx.close(); fresh.close()


# ------------------------------------------------------------------ the hand-over between the coarse-frequency loop and the block-wise filter
def test_hand_over_from_step_mf_to_the_filter_per_stream(O):
    """S = 2 after dvbs2hip_set_streams: step_mf for 6 calls of one frame per stream, then sync_coarse_synchronize -> filter (the shape of
    tests/test_stepmf_gpu.py, test_seams_into_the_block_wise_tasks_share_state).  Each stream's first 40 filtered samples -- the ones that read the handed-over
    memory -- are within the matched filter's 1e-4 bar of O.fir continued from that stream's ring of the CPU twin (tests/stepmf_ref.py), and they are not near zero."""
    import stepmf_ref as SR
    import timing_ref as TR
    from test_stepmf_gpu import MODCOD, PL, N, streams
    from dvbs2_amd.receiver import Dvbs2Hip
    S, k = 2, 6
    xs = streams(S, k + 1, seed=91)
    rx = Dvbs2Hip(MODCOD, max_frames=S)
    rx.set_streams(S)
    rx.sync_coarse_set_pll(1, 0.5 ** 0.5, 1e-3)
    tm = TR.Timing(PL, S)
    sm = SR.StepMf(PL, S, tm)
    sm.set_pll(1, np.float32(0.5 ** 0.5), 1e-3)
    for c in range(k):
        X = np.ascontiguousarray(xs[:, c]).reshape(S, 2 * N)
        D = [(131 * c) % PL, (977 * c + 5) % PL]
        MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize(D, X)
        MUt, FRQt, _, Yt, Bt = sm.synchronize(D, X)
        rx.sync_timing_extract(Y, B); tm.extract(Yt, Bt)
        assert np.array_equal(_bits(Y), _bits(Yt)), c
    X = np.ascontiguousarray(xs[:, k]).reshape(S, 2 * N)
    _, _, Z = rx.sync_coarse_synchronize(X, n_frames=S)
    M = rx.filter(Z, n_frames=S).reshape(S, -1)
    Z = Z.reshape(S, -1)
    for s in range(S):
        cf = sm.cf[s]
        Zt, _ = O.nco(X[s], np.float32(cf.nu_k) / np.float32(1e6), float(cf.n))
        assert np.max(np.abs(Z[s] - Zt)) <= 2e-6 * max(1.0, float(np.abs(Zt).max())), s
        Mt = O.fir(sm.taps, sm.ring[s], Zt)
        head = slice(0, 2 * 40)
        assert np.max(np.abs(M[s, head] - Mt[head])) <= FIR_TOL * max(1.0, float(np.abs(Mt).max())), s
        assert np.abs(Mt[head]).max() > 0.1 and np.abs(M[s, head]).max() > 0.1, s
    rx.close()


# ------------------------------------------------------------------ one chained case
def test_chain_of_the_three_tasks_equals_single_stream_handles(O, Rx, P, monkeypatch):
    """32APSK-S_3/4 at 12 dB, S = 3, F/S = 2, two calls: shaped streams (the oracle's upfir, per stream) -> filter -> every second sample (numpy) -> agc ->
    sync_frame_synchronize -> pl_descramble -> sync_lr_synchronize -> sync_freq_phase_synchronize, against the same calls on three single-stream handles (L&R in its
    three-kernel form there too): identical arrays."""
    monkeypatch.setenv("DVBS2HIP_LR", "unfused")
    monkeypatch.delenv("DVBS2HIP_SYNC", raising=False)
    monkeypatch.delenv("DVBS2HIP_SYNC_UNFUSED", raising=False)
    modcod, S, Fs, calls = "32APSK-S_3/4", 3, 2, 2
    taps = P.rrc_taps(0.2, 2, 20)
    shaped = []
    for s in range(S):
        _, pl, _, _ = make_pl_frames(O, modcod, Fs * calls, 12.0, seed=100 + s)
        n = pl.shape[1] // 2
        sym = np.concatenate([np.zeros(2 * (211 * s + 17), np.float32), pl.reshape(-1)])[:Fs * calls * 2 * n]
        shaped.append(O.upfir(taps, 2, np.zeros(160, np.float32), sym).reshape(calls, Fs * 4 * n))
    rx = Rx(modcod, max_frames=S * Fs)
    rx.set_streams(S)
    singles = [Rx(modcod, max_frames=Fs) for _ in range(S)]

    def chain(h, x, F):
        y = h.filter(x, n_frames=F).reshape(-1, 2)[::2].reshape(F, 2 * n)
        z = h.agc(y, n_frames=F).reshape(F, 2 * n)
        d, flg, tri, a = h.sync_frame_synchronize(z, with_flags=True)
        p = h.pl_descramble(a)
        f1, _, q = h.sync_lr_synchronize(p)
        f2, p2, r = h.sync_freq_phase_synchronize(q)
        return d, flg, _bits(tri), _bits(f1), _bits(f2), _bits(p2), _bits(r)

    for c in range(calls):
        x = np.stack([shaped[s][c] for s in range(S)])
        got = [_split(a, S) for a in chain(rx, x, S * Fs)]
        for s in range(S):
            one = chain(singles[s], x[s], Fs)
            for name, a, b in zip(("DEL", "FLG", "TRI", "FRQ lr", "FRQ fp", "PHS fp", "Y"), got, one):
                assert np.array_equal(a[s].reshape(b.shape), b), (c, s, name)
    rx.close()
    for one in singles:
        one.close()
