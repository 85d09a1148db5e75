"""Row N4, the frame synchronizer's delay line driven through every branch.

sync_vdelay_batch_kernel (k_sync.hip) does not copy frame after frame as Variable_delay_cc_naive::_filter does: every lane derives, from the
table of delays alone, which earlier input sample its output sample is (vd_source_fast / vd_source / vd_buff), and the seams between calls
(delay line, last output frame, {head2, first_time}, the 64 cor_SOF values) are derived as well.  In lock none of the walks takes a step, so
the delays here are CHOSEN: synchronize2 takes the two correlations as sockets, and with alpha = 0 one real peak A in cor_PLSC at complex
index idx gives delay (n + idx - 89) % n and metric A (tests/test_sync_delay_line.py pins that, and the four copies, on the oracle alone).
The input samples are seeded standard_normal floats -- every complex sample distinct -- and every comparison of Y is an equality of copied samples.

The helpers of both files live here; the tests of this file need the GPU."""
import ctypes
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import make_pl_frames

pytestmark = pytest.mark.gpu
TOL = 2e-4        # the metric's bar of tests/test_sync_gpu.py (sums of up to 64 products of unit-power samples in another order)
TRIGGER = 30.0
N_TAPS = 25 + 64  # corr_SOF + corr_PLSC: the arg max sits this far behind the frame start (Synchronizer_frame_DVBS2_fast.cpp:296)


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


# ---------------------------------------------------------------- crafted correlations
def idx_of_q(n, q):
    """the arg max that makes the delay line's delay (n - delay) % n equal to q (D = 2 q floats)"""
    return ((n - q) % n + N_TAPS) % n


def first_idx(idx):
    return 0 if idx is None else int(idx) if np.isscalar(idx) else min(idx)      # no value above 0: index 0; equal values: the first


def expected_delays(n, idxs):
    return np.array([(n + first_idx(i) - N_TAPS) % n for i in idxs], np.int32)


def craft(n, idxs, amps, sof=False):
    """cor_SOF, cor_PLSC [F, 2n] float32, zero except one real peak amps[f] per frame: in cor_PLSC at complex index idxs[f], or (sof) in cor_SOF
    64 samples earlier IN THE STREAM -- the previous frame when idxs[f] < 64.  idxs[f] = None: an all-zero frame; a tuple: equal peaks at each."""
    F = len(idxs)
    cs, cp = np.zeros((F, 2 * n), np.float32), np.zeros((F, 2 * n), np.float32)
    flat = cs.reshape(-1)
    for f, (idx, a) in enumerate(zip(idxs, amps)):
        if idx is None:
            continue
        for i in ((idx,) if np.isscalar(idx) else idx):
            assert 0 <= i < n
            if sof:
                g = f * n + i - 64
                assert g >= 0, "the peak of frame 0 would fall into the frame before the stream"
                flat[2 * g] = a
            else:
                cp[f, 2 * i] = a
    return cs, cp


def script(name, n, F=None):
    """A delay script -> idxs (one entry per frame, see craft), amps, sof, alpha, vec_width, prefix (frames run as a call of their own and followed by
    sync_frame_reset()).  Written as q = D / 2 = (n - delay) % n wherever the script is about the delay line; raw indices where it is about the arg max."""
    Q = lambda q: idx_of_q(n, int(q) % n)
    step = n // 7 + 1
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sc = SimpleNamespace(name=name, sof=False, alpha=0.0, vec_width=8, prefix=0, amps=None)
    if name == "constant":
        sc.idxs = [Q(1234)] * (F or 6)
    elif name == "up1":
        sc.idxs = [Q(100 + f) for f in range(F or 40)]
    elif name == "down1":
        sc.idxs = [Q(5000 % n - f) for f in range(F or 40)]
    elif name == "up_n7":          # grows by about n / 7 per frame, through the wrap
        sc.idxs = [Q(f * step) for f in range(F or 10)]
    elif name == "down_n7":
        sc.idxs = [Q(n - 1 - f * step) for f in range(F or 10)]
    elif name == "alt_0_max":
        sc.idxs = [Q(0), Q(n - 1)] * 6
    elif name == "zigzag":         # 0, n - 1, 0, 1, n - 2, 2, n - 3, ..
        sc.idxs = [Q(0), Q(n - 1), Q(0)] + [Q(v) for k in range(1, 9) for v in (k, n - 1 - k)]
    elif name == "odd_even":       # odd q: D = 2 (mod 4) floats, the lanes' pairs of complex samples straddle the copies' bounds (8-byte path)
        sc.idxs = [Q(q) for q in (7, 8, 8, 11, 11, 2, 3, 3, 4, 101, 100, 99, 99, 64, 1, 1)]
    elif name == "zeros_between":  # D = 0 leaves buff2 untouched
        sc.idxs = [Q(q) for q in (n - 5, n - 5, 0, 0, 0, 0, n - 7, n - 7, 3)]
    elif name == "random":
        sc.idxs = [Q(q) for q in rng.integers(0, n, F or 130)]
    elif name == "reset_large":    # after the reset: first_time's zero fill with a large D, then growth (those frames find the zeros in "previous output")
        sc.prefix = 3
        sc.idxs = [Q(q) for q in (50, 60, 60, n // 2, n // 2 + 500, n // 2 + 1500, n - 1, n - 1, 5)]
    elif name == "zero_frames":
        sc.idxs = [Q(300), Q(300), None, None, Q(700), None, Q(20), Q(20)]
    elif name == "ties":           # 64 positions per workgroup, 16 per lane of the thirteen-wave arg max: same lane, same workgroup, two workgroups, both ends
        sc.idxs = [Q(10), (650, 643), (643, 680), Q(500), (5000, 100), (n - 1, 0), (4000, 4001), (n - 1, n - 2)]
    elif name.startswith("tail_vw"):      # "tail_vw16", "tail_vw1000_a": maxima in the un-averaged tail i >= (n / vec_width) * vec_width; "_a": with the average on
        sc.vec_width = int(name[7:].split("_")[0])
        t0 = (n // sc.vec_width) * sc.vec_width
        assert t0 < n - 1
        sc.idxs = [t0, 50, n - 1, n - 1, t0 - 1, t0, 5, n - 1, t0 + (n - t0) // 2, t0 - 1, n - 2]
        if name.endswith("_a"):
            sc.alpha = 0.5
            sc.amps = (3.0 ** np.arange(len(sc.idxs))).astype(np.float32)
    elif name == "sof_seam":       # cor_SOF peaks in the last 64 positions of a frame belong to the NEXT frame's first 64: frames 1, 3, F - 1 start a call in the splits below
        sc.sof = True
        sc.idxs = [500, 10, 7000 % n, 0, 63, 64, n - 1, 33]
    elif name == "alpha_half":     # the recurrence on the path: amplitudes 3^f keep the newest peak the largest
        sc.alpha = 0.5
        sc.idxs = [Q(q) for q in rng.integers(0, n, 30)]
        sc.amps = (3.0 ** np.arange(30)).astype(np.float32)
    elif name == "mixed12":        # the long frame (four-wave arg max, a frame over many workgroups)
        sc.idxs = [Q(0), Q(n - 1), Q(0), Q(5), Q(4), Q(n // 2), Q(n // 2 + 1), None, (n - 282, 70), (6403, 6440), Q(3), Q(3)]
    else:
        raise KeyError(name)
    if sc.amps is None:
        sc.amps = rng.uniform(1.0, 60.0, len(sc.idxs)).astype(np.float32)
    # one more call with a fixed frame after every script: q = n - 1 reads the whole delay line and, unless the script ended there, "previous output"
    sc.idxs = list(sc.idxs) + [Q(n - 1)]
    sc.amps = np.concatenate([sc.amps, [np.float32(45.0) if sc.alpha == 0.0 else 3.0 * sc.amps.max()]]).astype(np.float32)
    return sc


SHORT, APSK, LONG = "QPSK-S_8/9", "32APSK-S_3/4", "QPSK-N_8/9"
CASES = [(SHORT, s, None) for s in ("constant", "up1", "down1", "up_n7", "down_n7", "alt_0_max", "zigzag", "odd_even", "zeros_between", "random", "reset_large",
                                    "zero_frames", "ties", "tail_vw16", "tail_vw16_a", "tail_vw1000", "tail_vw1000_a", "sof_seam", "alpha_half")]
CASES += [(APSK, s, 100) for s in ("random", "up_n7", "down_n7")]       # one whole chunk of 96 frames + four
CASES += [(LONG, "mixed12", None)]
CASE_IDS = ["%s-%s" % (m.split("_")[0], s) for m, s, _ in CASES]


def case_inputs(P, modcod, name, F):
    n = P.get_modcod(modcod).pl_frame
    sc = script(name, n, F)
    cs, cp = craft(n, sc.idxs, sc.amps, sc.sof)
    X = np.random.default_rng(zlib.crc32(name.encode()) + 1).standard_normal((len(sc.idxs), 2 * n)).astype(np.float32)
    return n, sc, X, cs, cp


def oracle_run(O, n, sc, X, cs, cp):
    """the oracle frame by frame -> DEL, FLG, TRI, Y"""
    T = len(sc.idxs)
    sf = O.SyncFrame(n, alpha=sc.alpha, trigger=TRIGGER, vec_width=sc.vec_width)
    DEL, FLG, TRI, Y = np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty_like(X)
    for f in range(T):
        if sc.prefix and f == sc.prefix:
            sf.reset()
        DEL[f], Y[f] = sf.synchronize2(X[f], cs[f], cp[f])
        FLG[f], TRI[f] = sf.packet_flag, sf.metric
    return DEL, FLG, TRI, Y


def splits(sc):
    """the script's frames as one call, and cut into calls (the fixed frame is always a call of its own)"""
    F = len(sc.idxs) - 1 - sc.prefix
    assert F >= 4
    return [(F, 1), (1, 2, F - 3, 1), (F - 1, 1, 1), (F // 2, 1, F - F // 2 - 1, 1)]


def first_diff(a, b):
    w = np.argwhere(a != b)
    return "equal" if not len(w) else "first difference at (frame, float) %s: %r != %r" % (tuple(w[0]), a[tuple(w[0])], b[tuple(w[0])])


# ---------------------------------------------------------------- a stream whose frame start moves every frame
MOVING_LOCK = 6      # frames of the last, in-lock call


@functools.lru_cache(maxsize=2)
def moving_reference(O, modcod, F):
    """Clean PL frames, each followed by a gap of seeded noise whose length is drawn from {0, 1, 2, 3, 17, 64, n / 3, n - 1}, cut into two calls of F frames;
    then a call of MOVING_LOCK frames without gaps.  With alpha = 0 the delay follows the frame start from frame to frame.  -> the stream [2 F + MOVING_LOCK, 2 n],
    the oracle's DEL / FLG / TRI / Y of every frame, and per frame the relative margin of the largest metric over the runner-up outside +-1 position, from
    the oracle's correlations (synchronize1, the 64-sample delay and the metric in float64)."""
    _, pl, _, _ = make_pl_frames(O, modcod, 6, 20.0, seed=41)
    n = pl.shape[1] // 2
    rng = np.random.default_rng(43)
    # (the gap 0 once, the others three times per round: a frame behind a gap of 0 keeps its delay and is read in place, and more than 64 of a call's
    # 70 frames have to be materialized)
    bag = [0] + 3 * [1, 2, 3, 17, 64, n // 3, n - 1]
    parts, tot, k, gaps = [], 0, 0, []
    while tot < 2 * F * 2 * n:
        if not gaps:
            gaps = list(rng.permutation(bag))
        g = int(gaps.pop())
        parts += [pl[k % 6], (0.05 * rng.standard_normal(2 * g)).astype(np.float32)]
        tot += 2 * n + 2 * g
        k += 1
    x = np.concatenate([np.concatenate(parts)[:2 * F * 2 * n], np.tile(pl.reshape(-1), 2)[:MOVING_LOCK * 2 * n]]).reshape(-1, 2 * n)
    T = x.shape[0]
    sf = O.SyncFrame(n, alpha=0.0, trigger=TRIGGER, vec_width=8)
    DEL, FLG, TRI, Y, margin = np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty_like(x), np.empty(T)
    sof_prev = np.zeros(64, complex)
    for f in range(T):
        c1, c2 = sf.synchronize1(x[f])
        DEL[f], Y[f] = sf.synchronize2(x[f], c1, c2)
        FLG[f], TRI[f] = sf.packet_flag, sf.metric
        sof = c1[0::2].astype(np.float64) + 1j * c1[1::2]
        plsc = c2[0::2].astype(np.float64) + 1j * c2[1::2]
        s = np.concatenate([sof_prev, sof[:n - 64]])
        sof_prev = sof[n - 64:]
        m = np.maximum(np.abs(plsc + s), np.abs(s - plsc))
        i = int(np.argmax(m))
        top = m[i]
        m[max(i - 1, 0):i + 2] = 0.0
        margin[f] = (top - m.max()) / top
    for a in (x, DEL, FLG, TRI, Y, margin):
        a.setflags(write=False)
    return SimpleNamespace(n=n, x=x, DEL=DEL, FLG=FLG, TRI=TRI, Y=Y, margin=margin)


def materialized(DEL, n, F):
    """frames of a call of F frames that the located form cannot read in place: the first, the last, and every frame whose delay moved"""
    D = (n - DEL.astype(np.int64)) % n
    need = np.ones(F, bool)
    need[1:F - 1] = D[1:F - 1] != D[0:F - 2]
    return need


# ---------------------------------------------------------------- GPU: the two-task form with crafted correlations
def gpu_run(Rx, modcod, sc, X, cs, cp, cuts):
    calls = ([sc.prefix] if sc.prefix else []) + list(cuts)
    assert sum(calls) == len(sc.idxs)
    rx = Rx(modcod, max_frames=max(calls))
    rx.sync_frame_set_params(alpha=sc.alpha, trigger=TRIGGER, vec_width=sc.vec_width)
    outs, pos = [], 0
    for i, c in enumerate(calls):
        outs.append(rx.sync_frame_synchronize2(X[pos:pos + c], cs[pos:pos + c], cp[pos:pos + c], with_flags=True))
        pos += c
        if sc.prefix and i == 0:
            rx.sync_frame_reset()
    rx.close()
    return [np.concatenate([o[k] for o in outs]) for k in range(4)]


@pytest.mark.parametrize("modcod,name,F", CASES, ids=CASE_IDS)
def test_delay_script_in_one_call_and_split_into_calls_against_the_oracle(O, Rx, P, modcod, name, F):
    """Every delay script as ONE call (the batched walks see every change of the delay inside the call), as the same frames cut into calls (1, 2, F - 3), (F - 1, 1)
    and (F / 2, 1, rest) -- the walks then end in the previous call's delay line and last output frame, and a call of one frame starts its state row's walk at frame -1 --
    and on the oracle frame by frame; one more call with a fixed frame after each.  DEL and FLG exact, Y bit for bit, TRI the copied amplitude (alpha = 0) or within
    the metric's bar (alpha = 0.5), and the split runs bit for bit what the one call gives on all four sockets."""
    n, sc, X, cs, cp = case_inputs(P, modcod, name, F)
    DELo, FLGo, TRIo, Yo = oracle_run(O, n, sc, X, cs, cp)
    assert np.array_equal(DELo, expected_delays(n, sc.idxs))       # the script drives the delay line as written
    runs = splits(sc)
    DEL, FLG, TRI, Y = gpu_run(Rx, modcod, sc, X, cs, cp, runs[0])
    assert np.array_equal(DEL, DELo), first_diff(DEL, DELo)
    assert np.array_equal(FLG, FLGo), first_diff(FLG, FLGo)
    if sc.alpha == 0.0:
        assert np.array_equal(TRI, TRIo), first_diff(TRI, TRIo)
    else:
        assert np.all(np.abs(TRI - TRIo) <= TOL * np.maximum(1.0, TRIo)), first_diff(TRI, TRIo)
    assert np.array_equal(Y, Yo), first_diff(Y, Yo)
    for cuts in runs[1:]:
        d2, f2, t2, Y2 = gpu_run(Rx, modcod, sc, X, cs, cp, cuts)
        assert np.array_equal(d2, DEL), (cuts, first_diff(d2, DEL))
        assert np.array_equal(f2, FLG), (cuts, first_diff(f2, FLG))
        assert np.array_equal(t2.view(np.uint32), TRI.view(np.uint32)), (cuts, first_diff(t2, TRI))
        assert np.array_equal(Y2, Y), (cuts, first_diff(Y2, Y))


# ---------------------------------------------------------------- GPU: the one-task form and the located form, the real correlators
@pytest.mark.parametrize("kernel", ["mfma", "valu"])
@pytest.mark.parametrize("F", [70, 130])
def test_one_task_and_located_forms_on_a_stream_whose_frame_start_moves(O, Rx, monkeypatch, F, kernel):
    """alpha = 0 and a stream of PL frames with gaps between them: the real correlators (matrix cores, and DVBS2HIP_SYNC=valu) move the delay in nearly every frame,
    so the located form materializes more than 64 of a call's frames: the rows of its grid take a second and a third entry of the list (`red` reused between them,
    the state row as a later entry).  (a) synchronize = the oracle's delays and Y, bit for bit; (b) locate on a second handle = the same DEL / FLG / TRI bits;
    (c) the 2 n floats behind every SRC[f] = row f of (a); (d) at least 65 pointers outside the input; (e) one more call, in lock, agrees as well (the carried state).
    The arg max cannot legitimately differ from the oracle's: in every frame the largest metric leads the runner-up outside +-1 position by 1e-3 relative (asserted
    from the oracle's correlations), against the 4e-6 by which the correlator kernels differ."""
    import torch
    if kernel == "valu":
        monkeypatch.setenv("DVBS2HIP_SYNC", "valu")
    else:
        monkeypatch.delenv("DVBS2HIP_SYNC", raising=False)
    ref = moving_reference(O, SHORT, F)
    n = ref.n
    assert ref.margin.min() >= 1e-3, (int(np.argmin(ref.margin)), ref.margin.min())
    a, b = Rx(SHORT, max_frames=F), Rx(SHORT, max_frames=F)
    for rx in (a, b):
        rx.sync_frame_set_params(alpha=0.0, trigger=TRIGGER, vec_width=8)
    dev = torch.device("cuda")
    row, pos = np.empty(2 * n, np.float32), 0
    for call, Fc in enumerate((F, F, MOVING_LOCK)):
        x = ref.x[pos:pos + Fc]
        d, flg, tri, Y = a.sync_frame_synchronize(x, with_flags=True)
        DELo, FLGo, TRIo, Yo = (v[pos:pos + Fc] for v in (ref.DEL, ref.FLG, ref.TRI, ref.Y))
        assert np.array_equal(d, DELo), (call, first_diff(d, DELo))                                    # (a)
        assert np.array_equal(Y, Yo), (call, first_diff(Y, Yo))
        assert np.array_equal(flg, FLGo) and np.all(np.abs(tri - TRIo) <= TOL * np.maximum(1.0, TRIo)), call
        xd = torch.from_numpy(x.copy()).to(dev)
        DEL = torch.empty(Fc, dtype=torch.int32, device=dev); FLG = torch.empty_like(DEL); TRI = torch.empty(Fc, dtype=torch.float32, device=dev)
        SRC = torch.zeros(Fc, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        b.sync_frame_locate_dev(xd.data_ptr(), DEL.data_ptr(), FLG.data_ptr(), TRI.data_ptr(), SRC.data_ptr(), Fc)
        b.synchronize()
        assert np.array_equal(DEL.cpu().numpy(), d) and np.array_equal(FLG.cpu().numpy(), flg), call   # (b)
        assert np.array_equal(TRI.cpu().numpy().view(np.uint32), tri.view(np.uint32)), call
        p = SRC.cpu().numpy()
        assert (p % 8 == 0).all()
        for f in range(Fc):                                                                            # (c), before the next call on this handle
            assert b.L.dvbs2hip_memcpy_d2h(b.h, row.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(int(p[f])), row.nbytes) == 0
            assert np.array_equal(row, Y[f]), (call, f, first_diff(row[None], Y[f][None]))
        inside = (p >= xd.data_ptr()) & (p < xd.data_ptr() + xd.numel() * 4)
        assert np.array_equal(~inside, materialized(d, n, Fc)), call
        if call < 2:
            assert int((~inside).sum()) >= 65, (call, int((~inside).sum()))                            # (d)
        else:
            assert int(inside.sum()) == Fc - 2                                                         # (e): in lock, read in place
        pos += Fc
    a.close(); b.close()
