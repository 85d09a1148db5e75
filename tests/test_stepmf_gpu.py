"""The coarse-frequency loop on the GPU (k_stepmf.hip) against the CPU twin (tests/stepmf_twin.c), bit for bit: Y_N1, B_N1, MU, FRQ and the state over runs of at
least 20 frames (so that nu moves), 1, 3 and 64 + 1 streams, one and several frames per call, host and device forms; the seams into the block-wise tasks (coarse shift ->
filter -> timing synchronize) with shared state; the channel's frequency shift against the oracle's sample-by-sample NCO."""
import ctypes as C

import numpy as np
import pytest

import stepmf_ref as SR
import timing_ref as TR
from dvbs2_amd import params as P

pytestmark = pytest.mark.gpu

MODCOD = "QPSK-S_8/9"
PL = P.get_modcod(MODCOD).pl_frame
N = 2 * PL


def streams(S, frames, seed):
    """S streams of `frames` frames: windows at ragged sample offsets of four received streams with different carrier offsets and channel delays -> [S, frames, 2 N]"""
    span = 3
    bases = [SR.received_stream(MODCOD, frames + span, f, 6.0, seed=seed + i, off=100 * i, D=D).reshape(-1)
             for i, (f, D) in enumerate(((0.02, 4.5), (-0.013, 2.25), (0.05, 4.0), (0.0031, 2.75)))]
    out = np.empty((S, frames, 2 * N), np.float32)
    for s in range(S):
        off = (s * 373 + s // 4) % (span * N)
        out[s] = bases[s % 4][2 * off: 2 * (off + frames * N)].reshape(frames, 2 * N)
    return out


def dels(S, Fs, call):
    return ((np.arange(S * Fs) * 131 + call * 977) % PL).astype(np.int32)


def check_state(rx, sm, S):
    est, nu = rx.sync_coarse_get_freq()
    assert np.array_equal(est.view(np.uint32), np.array([c.est for c in sm.cf], np.float32).view(np.uint32))
    assert np.array_equal(nu.view(np.uint32), np.array([np.float32(c.nu_k) / np.float32(1e6) for c in sm.cf], np.float32).view(np.uint32))


@pytest.mark.parametrize("S,Fs,calls,dev", [(1, 1, 20, False), (1, 5, 4, False), (1, 4, 5, True), (3, 1, 20, False), (3, 7, 3, True), (65, 1, 20, False)])
def test_step_mf_matches_the_twin(S, Fs, calls, dev):
    from dvbs2_amd.receiver import Dvbs2Hip
    xs = streams(S, Fs * calls, seed=10 * S + Fs)
    rx = Dvbs2Hip(MODCOD, max_frames=S * Fs)
    if S > 1:
        rx.sync_timing_set_streams(S)
    rx.sync_coarse_set_pll(1, 0.5 ** 0.5, 1e-3)                       # a fast PLL: nu moves from the first pilot block on
    tm = TR.Timing(PL, S)
    sm = SR.StepMf(PL, S, tm)
    sm.set_pll(1, np.float32(0.5 ** 0.5), 1e-3)
    assert rx.sync_coarse_gains() == (float(sm.pg), float(sm.ig))
    F = S * Fs
    if dev:
        import torch
        t = dict(X=torch.empty(F * 2 * N, dtype=torch.float32, device="cuda"), Y=torch.empty(F * 2 * N, dtype=torch.float32, device="cuda"),
                 B=torch.empty(F * 2 * N, dtype=torch.int32, device="cuda"), D=torch.empty(F, dtype=torch.int32, device="cuda"),
                 M=torch.empty(3 * F, dtype=torch.float32, device="cuda"), Y2=torch.zeros(F * N, dtype=torch.float32, device="cuda"),
                 U=torch.empty(F, dtype=torch.int32, device="cuda"), R=torch.empty(S, dtype=torch.int32, device="cuda"))
    moved = set()
    for c in range(calls):
        X = np.ascontiguousarray(xs[:, c * Fs:(c + 1) * Fs]).reshape(F, 2 * N)
        D = dels(S, Fs, c)
        MUt, FRQt, PHSt, Yt, Bt = sm.synchronize(D, X)
        if dev:
            t["X"].copy_(torch.from_numpy(X.ravel())); t["D"].copy_(torch.from_numpy(D))
            torch.cuda.synchronize()
            m = t["M"].data_ptr()
            rx.sync_step_mf_synchronize_dev(t["D"].data_ptr(), t["X"].data_ptr(), m, m + 4 * F, m + 8 * F, t["Y"].data_ptr(), t["B"].data_ptr(), F)
            rx.sync_timing_extract_dev(t["Y"].data_ptr(), t["B"].data_ptr(), t["Y2"].data_ptr(), t["U"].data_ptr(), t["R"].data_ptr(), F)
            rx.synchronize()
            M = t["M"].cpu().numpy()
            MU, FRQ, PHS = M[:F], M[F:2 * F], M[2 * F:]
            Y, B = t["Y"].cpu().numpy().reshape(F, -1), t["B"].cpu().numpy().reshape(F, -1)
            Y2, RDY = t["Y2"].cpu().numpy().reshape(F, -1), t["R"].cpu().numpy()
        else:
            MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize(D, X)
            Y2, _, RDY = rx.sync_timing_extract(Y, B)
        Y2t, _, RDYt = tm.extract(Yt, Bt)                              # (the carry buffer's fill is the loop's last_delay at the next call)
        assert np.array_equal(B, Bt), (c, np.argwhere(B != Bt)[:4])
        assert np.array_equal(Y.view(np.uint32), Yt.view(np.uint32)), (c, np.argwhere(Y != Yt)[:4])
        assert np.array_equal(MU.view(np.uint32), MUt.view(np.uint32)) and np.array_equal(FRQ.view(np.uint32), FRQt.view(np.uint32)), c
        assert not PHS.any()
        assert np.array_equal(RDY, RDYt)
        if RDY.all():
            assert np.array_equal(Y2.view(np.uint32), Y2t.view(np.uint32)), c
        moved.update(FRQt.tolist())
    assert len(moved) > 10 * min(S, 4)                                  # the estimate, and nu with it, moved from frame to frame
    check_state(rx, sm, S)
    rx.close()


def test_seams_into_the_block_wise_tasks_share_state():
    """step_mf for k calls, then sync_coarse_synchronize -> filter -> sync_timing_synchronize: FRQ and the timing state continue bit for bit (the timing loop is fed the
    twin's filtered frame), the shifted and filtered first frame after the switch matches the twin continued with shared state within the matched filter's 1e-4 bar
    (tests/test_fir_gpu.py), and step_mf carries on from the block-wise tasks again"""
    from dvbs2_amd.receiver import Dvbs2Hip
    from oracle import oracle as O
    k, F = 24, 1
    xs = streams(1, k + 3, seed=77)[0]
    rx = Dvbs2Hip(MODCOD, max_frames=F)
    rx.sync_coarse_set_pll(1, 0.5 ** 0.5, 1e-4)
    tm = TR.Timing(PL, 1)
    sm = SR.StepMf(PL, 1, tm)
    d = 0
    for c in range(k):
        MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize([d], xs[c:c + 1])
        MUt, FRQt, _, Yt, Bt = sm.synchronize([d], xs[c:c + 1])
        rx.sync_timing_extract(Y, B); tm.extract(Yt, Bt)
        d = (d + 517) % PL
        assert np.array_equal(Y.view(np.uint32), Yt.view(np.uint32))
    cf = sm.cf[0]
    assert cf.nu_k != 0
    for c in range(k, k + 2):
        # the switch: the shift at the learned frequency with a continuous sample counter
        FRQ2, PHS2, Z = rx.sync_coarse_synchronize(xs[c], n_frames=1)
        assert FRQ2.view(np.uint32)[0] == FRQt.view(np.uint32)[-1] and PHS2[0] == 0          # FRQ continues: estimated_freq as the loop left it
        Zt, n_after = O.nco(xs[c], np.float32(cf.nu_k) / np.float32(1e6), float(cf.n))
        cf.n = int(n_after)
        assert np.max(np.abs(Z - Zt)) <= 2e-6 * max(1.0, float(np.abs(Zt).max()))             # nco_kernel's bar
        M = rx.filter(Z, n_frames=1)                                                          # the block-wise filter carries on from the loop's ring
        Mt = O.fir(sm.taps, sm.ring[0], Zt)
        assert np.max(np.abs(M - Mt)) <= 1e-4 * max(1.0, float(np.abs(Mt).max()))
        # the timing loop carries on from step_mf's state: on the same input, bit for bit
        Y, B, MU = rx.sync_timing_synchronize(Mt.reshape(1, -1))
        Yt, Bt, MUt2 = tm.synchronize(Mt.reshape(1, -1))
        assert np.array_equal(Y.view(np.uint32), Yt.view(np.uint32)) and np.array_equal(B, Bt) and np.array_equal(MU.view(np.uint32), MUt2.view(np.uint32))
        rx.sync_timing_extract(Y, B); tm.extract(Yt, Bt)
    # and back: the ring is the block-wise filter's memory (of the GPU's shifted samples: equal to the twin's within the NCO's bar, so Y is compared at the filter's bar)
    MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize([d], xs[k + 2:k + 3])
    MUt, FRQt, _, Yt, Bt = sm.synchronize([d], xs[k + 2:k + 3])
    head = slice(0, 2 * 40)                                                                  # the samples that read the handed-over memory
    assert np.max(np.abs(Y[0, head] - Yt[0, head])) <= 1e-4 * max(1.0, float(np.abs(Yt).max()))
    assert np.abs(Yt[0, head]).max() > 0.1
    rx.close()


def test_resets_and_set_freq_keep_their_meaning():
    from dvbs2_amd.receiver import Dvbs2Hip
    xs = streams(2, 3, seed=5)
    rx = Dvbs2Hip(MODCOD, max_frames=2)
    rx.sync_timing_set_streams(2)
    rx.sync_coarse_set_pll(1, 0.5 ** 0.5, 1e-3)
    X0 = np.ascontiguousarray(xs[:, 0]).reshape(2, -1)
    first = rx.sync_step_mf_synchronize([5, 6], X0)
    rx.sync_step_mf_synchronize([5, 6], np.ascontiguousarray(xs[:, 1]).reshape(2, -1))
    est, nu = rx.sync_coarse_get_freq()
    assert est.any() and np.allclose(nu, -est, atol=1.1e-6)
    rx.sync_step_mf_reset()
    est, nu = rx.sync_coarse_get_freq()
    assert not est.any() and not nu.any()
    again = rx.sync_step_mf_synchronize([5, 6], X0)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rx.sync_coarse_set_freq(0.0125)                                    # all streams
    est, nu = rx.sync_coarse_get_freq()
    assert np.allclose(nu, -0.0125, atol=1.1e-6) and nu[0] == nu[1]
    rx.close()


def test_a_new_stream_count_starts_every_stream_over_filter_memory_included():
    """5 streams run a call, then set_streams(3): the three streams give what a fresh handle gives (PLL, timing and the per-stream matched-filter memories all cleared)"""
    from dvbs2_amd.receiver import Dvbs2Hip
    xs = streams(5, 2, seed=31)
    rx = Dvbs2Hip(MODCOD, max_frames=5)
    rx.sync_timing_set_streams(5)
    rx.sync_step_mf_synchronize(dels(5, 1, 0), np.ascontiguousarray(xs[:, 0]).reshape(5, -1))
    rx.sync_timing_set_streams(3)
    X = np.ascontiguousarray(xs[:3, 1]).reshape(3, -1)
    got = rx.sync_step_mf_synchronize(dels(3, 1, 1), X)
    sm = SR.StepMf(PL, 3, TR.Timing(PL, 3))
    want = sm.synchronize(dels(3, 1, 1), X)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rx.close()


@pytest.mark.parametrize("f", [0.05, -0.0123456])
def test_channel_freq_shift_matches_the_oracles_nco(f):
    """Multiplier_sine_ccc_naive built with f / Fs floored to six decimals (DVBS2.cpp:624-626): against the oracle's sample-by-sample NCO at nco_kernel's 2e-6, the
    stream position carried across calls and over the counter's wrap"""
    from dvbs2_amd.receiver import Dvbs2Hip
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    rx = Dvbs2Hip(MODCOD, max_frames=24)
    rx.channel_set_freq_shift(f)
    nu = np.floor(np.float32(f) * np.float32(1e6)) / np.float32(1e6)
    n = 0.0
    for F in (1, 24, 24, 13):                                          # 62 frames of 16740 samples: past 1e6
        X = rng.standard_normal((F, 2 * N)).astype(np.float32)
        Y = rx.channel_freq_shift(X)
        Yt, n = O.nco(X, nu, n)
        assert np.max(np.abs(Y.ravel() - Yt)) <= 2e-6 * float(np.abs(Yt).max())
    rx.close()
