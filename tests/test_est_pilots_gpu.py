"""dvbs2hip_estimate_pilots[_dev | _located_dev], _set_alpha, _reset (dvbs2_amd/csrc/k_est_pilots.hip, api_est_pilots.hip) against the float64 reference of
tests/est_pilots_ref.py on the same float32 samples.  The bar is the M2M4 estimator's, 1e-4 max(1, |x|) on each of SIG, Eb_N0 and Es_N0: the residual form has no
cancellation, so the fp32 error is of the order L 2^-24 (5e-5 relative at L = 882 in the worst case).  The kernel adds in an order of its own; what is bit-exact here is
the kernel against itself: scrambled against descrambled input, the located against the plain form, the host against the device form, calls split in two."""
import ctypes as C

import numpy as np
import pytest

import est_pilots_ref as R
from dvbs2_amd import params as P

pytestmark = pytest.mark.gpu

TOL = 1e-4
EINVAL = -1
SMALL = "32APSK-S_3/4"
SHAPES = {"QPSK-S_8/9": 270, "8PSK-S_3/5": 198, SMALL: 162, "QPSK-N_8/9": 882, "16APSK-N_8/9": 486}      # MODCOD -> known symbols L
MAXF = 12


def make_frames(mc, F, esn0_db, rng, phase=0.3, signal=1.0):
    """F PL frames as the frame synchronizer delivers them (header copied, the rest PL-scrambled) with unit-power data symbols, turned by `phase`, at Es/N0 -> float32[F, 2 n]"""
    n = mc.pl_frame
    pos, val = R.positions(mc.N_xfec), R.values(mc.pls, mc.N_xfec)
    c = np.exp(2j * np.pi * rng.uniform(0, 1, (F, n)))
    c[:, pos] = val
    c[:, 90:] *= np.exp(0.5j * np.pi * R.pl_sequence()[:n - 90])
    sig = np.sqrt(10 ** (-esn0_db / 10) / 2) if esn0_db is not None else 0.0
    c = signal * c * np.exp(1j * phase) + sig * (rng.standard_normal((F, n)) + 1j * rng.standard_normal((F, n)))
    x = np.empty((F, 2 * n), np.float32)
    x[:, 0::2], x[:, 1::2] = c.real, c.imag
    return x


def within_bar(got, want, what):
    worst = max(float((np.abs(np.asarray(g, np.float64) - w) / np.maximum(1.0, np.abs(w))).max()) for g, w in zip(got, want))
    print("%s: largest |fp32 - float64| / max(1, |x|) = %.3g (bar %.0e)" % (what, worst, TOL))
    for g, w, name in zip(got, want, ("SIG", "Eb_N0", "Es_N0")):
        assert (np.abs(np.asarray(g, np.float64) - w) <= TOL * np.maximum(1.0, np.abs(w))).all(), (what, name)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(u).view(np.uint32), np.asarray(v).view(np.uint32)) for u, v in zip(a, b))


@pytest.fixture(scope="module")
def handles():
    """one handle per MODCOD for the whole module; every test leaves it at alpha = 0, one stream, reset"""
    from dvbs2_amd.receiver import Dvbs2Hip
    made = {}

    def get(modcod):
        if modcod not in made:
            made[modcod] = Dvbs2Hip(modcod, max_frames=MAXF)
        return made[modcod]
    yield get
    for rx in made.values():
        rx.close()


def dev_call(rx, x, scrambled=1, located=None):
    """the device form on a copy of x (or the located form on the table `located`) -> three float32 arrays"""
    import torch
    F = len(x) if located is None else len(located)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda() if located is None else None
    out = torch.full((3, F), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if located is None:
        rx.estimate_pilots_dev(xd.data_ptr(), scrambled, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), F)
    else:
        rx.estimate_pilots_located_dev(located.data_ptr(), scrambled, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), F)
    rx.synchronize()
    return tuple(out.cpu().numpy())


@pytest.mark.parametrize("esn0", [0.0, 10.0, 25.0])
@pytest.mark.parametrize("modcod", list(SHAPES))
def test_shapes_and_frame_counts_against_float64(handles, modcod, esn0):
    rx, mc = handles(modcod), P.get_modcod(modcod)
    assert mc.pl_frame - mc.N_xfec == SHAPES[modcod] == len(R.positions(mc.N_xfec))
    x = make_frames(mc, 9, esn0, np.random.default_rng(int(10 * esn0) + mc.pl_frame))
    want = R.estimate(x, mc, scrambled=True)
    assert (np.abs(want[2] - esn0) < 3.0).all()                                      # the reference measures what was put in
    all9 = rx.estimate_pilots(x)
    within_bar(all9, want, "%s at %g dB" % (modcod, esn0))
    for F in (1, 3, 4, 5):                                                           # around one workgroup of four waves
        assert same_bits(rx.estimate_pilots(x[:F]), [v[:F] for v in all9]), F
    assert same_bits(dev_call(rx, x), all9)                                          # whole frames on the device against the host form's staged known symbols
    # each output may be NULL
    es = np.full(9, -7.0, np.float32)
    rx._chk(rx.L.dvbs2hip_estimate_pilots(rx.h, x.ctypes.data_as(C.c_void_p), 1, None, None, es.ctypes.data_as(C.c_void_p), 9))
    assert same_bits([es], [all9[2]])


@pytest.mark.parametrize("modcod", [SMALL, "QPSK-N_8/9"])
def test_scrambled_and_descrambled_input_give_the_same_bits(handles, modcod):
    rx, mc = handles(modcod), P.get_modcod(modcod)
    x = make_frames(mc, 5, 10.0, np.random.default_rng(2))
    d = rx.pl_descramble(x)
    a, b = rx.estimate_pilots(x, scrambled=True), rx.estimate_pilots(d, scrambled=False)
    assert same_bits(a, b) and same_bits(dev_call(rx, x, 1), dev_call(rx, d, 0)) and same_bits(a, dev_call(rx, d, 0))
    within_bar(b, R.estimate(d, mc, scrambled=False), modcod + " descrambled")
    assert not same_bits(a, rx.estimate_pilots(x, scrambled=False))                  # (the flag is read)


def test_located_form_on_the_synchronizers_table_and_on_odd_complex_offsets(handles):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod(SMALL)
    n, F = mc.pl_frame, 6
    rng = np.random.default_rng(6)
    x = make_frames(mc, 2 * F + 1, 12.0, rng)
    # (a) the table dvbs2hip_sync_frame_locate_dev fills, against the delayed copy of dvbs2hip_sync_frame_synchronize_dev: two calls on a stream that starts mid-frame
    stream = np.concatenate([np.zeros(2 * 701, np.float32), x.reshape(-1)])
    a, b = Dvbs2Hip(SMALL, max_frames=F), Dvbs2Hip(SMALL, max_frames=F)
    in_place = 0
    for call in range(2):
        xd = torch.from_numpy(stream[call * F * 2 * n:(call + 1) * F * 2 * n].copy()).cuda()
        DEL = torch.empty(F, dtype=torch.int32, device="cuda"); FLG = torch.empty_like(DEL); TRI = torch.empty(F, dtype=torch.float32, device="cuda")
        Y, SRC = torch.empty_like(xd), torch.zeros(F, dtype=torch.int64, device="cuda")
        oa, ob = torch.full((3, F), -7.0, device="cuda"), torch.full((3, F), -7.0, device="cuda")
        torch.cuda.synchronize()
        a.sync_frame_synchronize_dev(xd.data_ptr(), DEL.data_ptr(), FLG.data_ptr(), TRI.data_ptr(), Y.data_ptr(), F)
        a.estimate_pilots_dev(Y.data_ptr(), 1, oa[0].data_ptr(), oa[1].data_ptr(), oa[2].data_ptr(), F)
        b.sync_frame_locate_dev(xd.data_ptr(), DEL.data_ptr(), FLG.data_ptr(), TRI.data_ptr(), SRC.data_ptr(), F)
        b.estimate_pilots_located_dev(SRC.data_ptr(), 1, ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr(), F)
        a.synchronize(); b.synchronize()
        assert same_bits(oa.cpu().numpy(), ob.cpu().numpy()), call
        p = SRC.cpu().numpy()
        in_place += int(((p >= xd.data_ptr()) & (p < xd.data_ptr() + xd.numel() * 4)).sum())
        if call == 1:                                                                # in lock: the aligned frames are transmitted ones, and float64 reads them the same
            want = R.estimate(Y.cpu().numpy(), mc)
            locked = want[2] > 5.0
            assert locked.sum() >= F - 2, want[2]
            within_bar([v[locked] for v in ob.cpu().numpy()], [v[locked] for v in want], "located, in lock")
    assert in_place >= F - 2                                                         # (frames read where they lie in the input, at whatever 8-byte address that is)
    a.close(); b.close()
    # (b) a hand-built table: frame k starts 2 k + 1 complex samples behind k (n + 16), an odd complex offset -- 8-byte aligned and not 16 -- in shuffled order
    rx = handles(SMALL)
    F = 7
    buf = torch.from_numpy(rng.standard_normal(2 * (F * (n + 16) + 2 * F + 1)).astype(np.float32)).cuda()
    assert buf.data_ptr() % 16 == 0
    order = rng.permutation(F)
    off = np.array([k * (n + 16) + 2 * k + 1 for k in range(F)])
    for k in range(F):
        buf[2 * off[k]:2 * (off[k] + n)] = torch.from_numpy(x[order[k]]).cuda()
    table = buf.data_ptr() + 8 * off[np.argsort(order)]
    assert (table % 16 == 8).all()
    SRC = torch.from_numpy(table.astype(np.int64)).cuda()
    for scr in (1, 0):
        assert same_bits(dev_call(rx, x[:F], scr), dev_call(rx, None, scr, located=SRC)), scr


def test_no_noise_saturates_at_100_db_and_noise_alone_reads_no_signal(handles):
    rx, mc = handles("8PSK-S_3/5"), P.get_modcod("8PSK-S_3/5")
    rng = np.random.default_rng(8)
    clean = make_frames(mc, 2, None, rng)
    noise = make_frames(mc, 6, 0.0, rng, signal=0.0)
    zero = np.zeros((1, 2 * mc.pl_frame), np.float32)
    sig, eb, es = rx.estimate_pilots(np.concatenate([clean, noise, zero]))
    print("noise alone: Es_N0 =", es[2:8])
    assert (es[:2] == 100.0).all() and np.allclose(sig[:2], np.sqrt(0.5e-10), rtol=1e-4, atol=0)
    assert ((es[2:8] <= -10.0) | (es[2:8] == -100.0)).all() and np.isfinite(sig).all() and np.isfinite(eb).all()
    assert es[8] == -100.0
    want = R.estimate(np.concatenate([clean, zero]), mc)
    assert (want[2] == [100.0, 100.0, -100.0]).all()


@pytest.mark.parametrize("alpha", [0.9, 0.99])
def test_averaging_carries_from_call_to_call_and_reset_starts_over(handles, alpha):
    rx, mc = handles(SMALL), P.get_modcod(SMALL)
    x = make_frames(mc, 12, 10.0, np.random.default_rng(12))
    per_frame = rx.estimate_pilots(x)
    try:
        rx.estimate_pilots_set_alpha(alpha)
        rx.estimate_pilots_reset()
        whole = rx.estimate_pilots(x)
        rx.estimate_pilots_reset()
        split = [np.concatenate(v) for v in zip(rx.estimate_pilots(x[:5]), rx.estimate_pilots(x[5:]))]
        assert same_bits(whole, split)                                               # the state carries
        want = R.estimate(x, mc, alpha=alpha)
        within_bar(whole, want[:3], "alpha %g" % alpha)
        assert same_bits([v[:1] for v in whole], [v[:1] for v in per_frame]) and not same_bits(whole, per_frame)
        assert whole[2][1:].std() < per_frame[2][1:].std()
        # without a reset the next call goes on from the state; after one it starts over; dvbs2hip_reset resets it too
        on = rx.estimate_pilots(x[:3])
        assert not same_bits(on, [v[:3] for v in whole])
        within_bar(on, R.estimate(x[:3], mc, alpha=alpha, state=want[3])[:3], "alpha %g, a third call" % alpha)
        rx.estimate_pilots_reset()
        assert same_bits(rx.estimate_pilots(x[:3]), [v[:3] for v in whole])
        rx.reset()
        assert same_bits(dev_call(rx, x[:3]), [v[:3] for v in whole])
        # back to 0: every frame on its own again, whatever the state holds
        rx.estimate_pilots_set_alpha(0.0)
        assert same_bits(rx.estimate_pilots(x), per_frame)
    finally:
        rx.estimate_pilots_set_alpha(0.0)
        rx.estimate_pilots_reset()


def test_three_streams_are_three_one_stream_handles(handles):
    from dvbs2_amd.receiver import Dvbs2Hip
    rx, mc = handles(SMALL), P.get_modcod(SMALL)
    x = make_frames(mc, 12, 8.0, np.random.default_rng(3))
    alone = []
    for s in range(3):
        one = Dvbs2Hip(SMALL, max_frames=4)
        one.estimate_pilots_set_alpha(0.9)
        alone.append([np.concatenate(v) for v in zip(one.estimate_pilots(x[4 * s:4 * s + 2]), one.estimate_pilots(x[4 * s + 2:4 * s + 4]))])
        one.close()
    try:
        rx.set_streams(3)
        rx.estimate_pilots_set_alpha(0.9)
        got = rx.estimate_pilots(x)                                                  # stream s = frames [4 s, 4 s + 4)
        assert same_bits(got, [np.concatenate(v) for v in zip(*alone)])
        within_bar(got, R.estimate(x, mc, alpha=0.9, streams=3)[:3], "three streams")
        # the state is per stream across calls: 6 frames = two of each stream, then the other six
        rx.estimate_pilots_reset()
        idx = np.array([0, 1, 4, 5, 8, 9])
        first, second = rx.estimate_pilots(x[idx]), rx.estimate_pilots(x[idx + 2])
        both = [np.empty(12, np.float32) for _ in range(3)]
        for v, u, w in zip(both, first, second):
            v[idx], v[idx + 2] = u, w
        assert same_bits(both, got)
        assert rx.L.dvbs2hip_estimate_pilots(rx.h, x.ctypes.data_as(C.c_void_p), 1, None, None, None, 4) == EINVAL and b"multiple" in rx.L.dvbs2hip_last_error(rx.h)
        rx.estimate_pilots_set_alpha(0.0)
        assert len(rx.estimate_pilots(x[:4])[0]) == 4                                # without averaging frames are just frames
    finally:
        rx.estimate_pilots_set_alpha(0.0)
        rx.set_streams(1)


def test_errors_leave_the_handle_usable(handles):
    rx, mc = handles(SMALL), P.get_modcod(SMALL)
    x = make_frames(mc, 3, 10.0, np.random.default_rng(4))
    want = rx.estimate_pilots(x)
    out = np.zeros(3, np.float32)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    err = lambda: rx.L.dvbs2hip_last_error(rx.h)
    for fn in (rx.L.dvbs2hip_estimate_pilots, rx.L.dvbs2hip_estimate_pilots_dev, rx.L.dvbs2hip_estimate_pilots_located_dev):
        assert fn(rx.h, xp, 1, op, None, None, 0) == EINVAL and b"n_frames" in err()
        assert fn(rx.h, xp, 1, op, None, None, MAXF + 1) == EINVAL and b"max_frames" in err()
        assert fn(rx.h, None, 1, op, None, None, 3) == EINVAL and b"null" in err()
        assert fn(rx.h, xp, 2, op, None, None, 3) == EINVAL and b"scrambled" in err()
        assert fn(rx.h, xp, -1, op, None, None, 3) == EINVAL
        assert fn(None, xp, 1, op, None, None, 3) == EINVAL
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert rx.L.dvbs2hip_estimate_pilots_set_alpha(rx.h, bad) == EINVAL and b"alpha" in err()
    assert rx.L.dvbs2hip_estimate_pilots_set_alpha(None, 0.5) == EINVAL and rx.L.dvbs2hip_estimate_pilots_reset(None) == EINVAL
    assert same_bits(rx.estimate_pilots(x), want)                                    # alpha is still 0, the handle works


def test_a_recorded_call_replays_on_new_input(handles):
    import torch
    rx, mc = handles(SMALL), P.get_modcod(SMALL)
    F = 9
    rng = np.random.default_rng(9)
    xd = torch.zeros((F, 2 * mc.pl_frame), dtype=torch.float32, device="cuda")
    out = torch.full((3, F), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def once():
        rx.estimate_pilots_dev(xd.data_ptr(), 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), F)

    once(); rx.synchronize()
    gid = rx.graph_capture(once)
    for k in range(2):
        x = make_frames(mc, F, 5.0 + 10 * k, rng)
        xd.copy_(torch.from_numpy(x)); torch.cuda.synchronize()
        once(); rx.synchronize()
        want = out.clone()
        out.fill_(-7.0); torch.cuda.synchronize()
        rx.graph_launch(gid); rx.synchronize()
        assert torch.equal(out, want)
        within_bar(out.cpu().numpy(), R.estimate(x, mc), "replay %d" % k)
    rx.graph_destroy(gid)
