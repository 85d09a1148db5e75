"""The one-wave-per-stream form of the coarse-frequency loop on the GPU (k_stepmf_wave.hip, dvbs2hip_sync_step_mf_set_kernel) against the CPU twin (tests/stepmf_twin.c), bit
for bit: Y_N1, B_N1, MU, FRQ, RDY / Y_N2 after extract and the coarse state, over the cases of tests/stepmf_wave_ref.py -- whose inputs cut a chunk at every lane position,
on the first and the last sample of a call and in a ragged last chunk, and run past the sample counter's wrap (asserted on the CPU, tests/test_stepmf_wave_twin.py) --; a
handle that changes form between calls; the seams into the block-wise tasks; the setter's rules; the file workflow with --smf-kernel WAVE."""
import io
import os

import numpy as np
import pytest

import stepmf_ref as SR
import stepmf_wave_ref as WR
import timing_ref as TR
from test_stepmf_gpu import check_state, streams

pytestmark = pytest.mark.gpu

MODCOD, PL, N = WR.MODCOD, WR.PL, WR.N


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Runner:
    """a handle and the twins beside it, call by call: step_mf -> extract on both, everything compared bit for bit"""

    def __init__(self, S, Fs, dev=False, kernel="WAVE"):
        from dvbs2_amd.receiver import Dvbs2Hip
        self.S, self.Fs, self.F, self.dev = S, Fs, S * Fs, dev
        self.rx = Dvbs2Hip(MODCOD, max_frames=self.F)
        if S > 1:
            self.rx.sync_timing_set_streams(S)
        self.rx.sync_coarse_set_pll(*WR.PLL)
        if kernel is not None:
            self.rx.sync_step_mf_set_kernel(kernel)
        self.tm, self.sm = WR.twins(S)
        assert self.rx.sync_coarse_gains() == (float(self.sm.pg), float(self.sm.ig))
        if dev:
            import torch
            F = self.F
            e = lambda n, t: torch.empty(n, dtype=t, device="cuda")
            self.t = dict(X=e(F * 2 * N, torch.float32), Y=e(F * 2 * N, torch.float32), B=e(F * 2 * N, torch.int32), D=e(F, torch.int32), M=e(3 * F, torch.float32),
                          Y2=torch.zeros(F * N, dtype=torch.float32, device="cuda"), U=e(F, torch.int32), R=e(S, torch.int32))

    def gpu(self, D, X):
        """-> MU, FRQ, PHS, Y, B, Y2, RDY of one call on the handle"""
        rx, F = self.rx, self.F
        if not self.dev:
            MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize(D, X)
            Y2, _, RDY = rx.sync_timing_extract(Y, B)
            return MU, FRQ, PHS, Y, B, Y2, RDY
        import torch
        t = self.t
        t["X"].copy_(torch.from_numpy(X.ravel())); t["D"].copy_(torch.from_numpy(D))
        torch.cuda.synchronize()
        m = t["M"].data_ptr()
        rx.sync_step_mf_synchronize_dev(t["D"].data_ptr(), t["X"].data_ptr(), m, m + 4 * F, m + 8 * F, t["Y"].data_ptr(), t["B"].data_ptr(), F)
        rx.sync_timing_extract_dev(t["Y"].data_ptr(), t["B"].data_ptr(), t["Y2"].data_ptr(), t["U"].data_ptr(), t["R"].data_ptr(), F)
        rx.synchronize()
        M = t["M"].cpu().numpy()
        return (M[:F], M[F:2 * F], M[2 * F:], t["Y"].cpu().numpy().reshape(F, -1), t["B"].cpu().numpy().reshape(F, -1), t["Y2"].cpu().numpy().reshape(F, -1),
                t["R"].cpu().numpy())

    def call(self, D, X, tag):
        MU, FRQ, PHS, Y, B, Y2, RDY = got = self.gpu(D, X)
        MUt, FRQt, _, Yt, Bt = self.sm.synchronize(D, X)
        Y2t, _, RDYt = self.tm.extract(Yt, Bt)                         # (the carry buffer's fill is the loop's last_delay at the next call)
        assert np.array_equal(B, Bt), (tag, np.argwhere(B != Bt)[:4])
        assert np.array_equal(bits(Y), bits(Yt)), (tag, np.argwhere(bits(Y) != bits(Yt))[:4])
        assert np.array_equal(bits(MU), bits(MUt)) and np.array_equal(bits(FRQ), bits(FRQt)), tag
        assert not PHS.any()
        assert np.array_equal(RDY, RDYt)
        if RDY.all():
            assert np.array_equal(bits(Y2), bits(Y2t)), tag
        return got

    def close(self):
        check_state(self.rx, self.sm, self.S)
        self.rx.close()


@pytest.mark.parametrize("S,Fs,calls,dev,seed", WR.CASES, ids=lambda v: str(v))
def test_wave_matches_the_twin(S, Fs, calls, dev, seed):
    xs = WR.case_inputs(S, Fs, calls, seed)
    r = Runner(S, Fs, dev)
    moved = set()
    for c in range(calls):
        D, X = WR.call_inputs(xs, S, Fs, c)
        moved.update(r.call(D, X, c)[1].tolist())
    assert len(moved) > 10 * min(S, 4)                                  # the estimate, and nu with it, moved from frame to frame
    if Fs * calls * N > 1000000:
        assert r.sm.cf[0].n == Fs * calls * N - 1000000                 # the counter went round once
    r.close()


def test_a_handle_changes_form_between_calls_and_the_forms_agree():
    """five calls LANE, five WAVE, five LANE on one stream, the twin beside it throughout; and the two forms on fresh handles over the same calls, output against output"""
    xs = WR.case_inputs(1, 1, 15, 11)
    r = Runner(1, 1, kernel=None)                                       # never set: LANE
    for c in range(15):
        if c in (5, 10):
            r.rx.sync_step_mf_set_kernel("WAVE" if c == 5 else "LANE")
        r.call(*WR.call_inputs(xs, 1, 1, c), tag=c)
    r.close()
    lane, wave = Runner(1, 1, kernel="LANE"), Runner(1, 1, kernel=1)
    for c in range(3):
        D, X = WR.call_inputs(xs, 1, 1, c)
        for a, b in zip(lane.gpu(D, X), wave.gpu(D, X)):
            assert np.array_equal(bits(a), bits(b)), c
    est_l, est_w = lane.rx.sync_coarse_get_freq(), wave.rx.sync_coarse_get_freq()
    assert np.array_equal(bits(est_l[0]), bits(est_w[0])) and np.array_equal(bits(est_l[1]), bits(est_w[1])) and est_w[0].any()
    lane.rx.close(); wave.rx.close()


def test_seams_into_the_block_wise_tasks_share_state_with_wave():
    """tests/test_stepmf_gpu.py's seam test with WAVE selected: step_mf for k calls, then sync_coarse_synchronize -> filter -> sync_timing_synchronize, and back, at the
    same bars: FRQ and the timing state continue bit for bit, the shifted and filtered frames match the twin continued with shared state within the matched filter's 1e-4,
    and step_mf carries on from the block-wise filter's memory"""
    from dvbs2_amd.receiver import Dvbs2Hip
    from oracle import oracle as O
    k, F = 24, 1
    xs = streams(1, k + 3, seed=77)[0]
    rx = Dvbs2Hip(MODCOD, max_frames=F)
    rx.sync_coarse_set_pll(1, 0.5 ** 0.5, 1e-4)
    rx.sync_step_mf_set_kernel("WAVE")
    tm = TR.Timing(PL, 1)
    sm = SR.StepMf(PL, 1, tm)
    d = 0
    for c in range(k):
        MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize([d], xs[c:c + 1])
        MUt, FRQt, _, Yt, Bt = sm.synchronize([d], xs[c:c + 1])
        rx.sync_timing_extract(Y, B); tm.extract(Yt, Bt)
        d = (d + 517) % PL
        assert np.array_equal(bits(Y), bits(Yt))
    cf = sm.cf[0]
    assert cf.nu_k != 0
    for c in range(k, k + 2):
        FRQ2, PHS2, Z = rx.sync_coarse_synchronize(xs[c], n_frames=1)
        assert bits(FRQ2)[0] == bits(FRQt)[-1] and PHS2[0] == 0         # FRQ continues: estimated_freq as the loop left it
        Zt, n_after = O.nco(xs[c], np.float32(cf.nu_k) / np.float32(1e6), float(cf.n))
        cf.n = int(n_after)
        assert np.max(np.abs(Z - Zt)) <= 2e-6 * max(1.0, float(np.abs(Zt).max()))             # nco_kernel's bar
        M = rx.filter(Z, n_frames=1)                                                          # the block-wise filter carries on from the loop's window
        Mt = O.fir(sm.taps, sm.ring[0], Zt)
        assert np.max(np.abs(M - Mt)) <= 1e-4 * max(1.0, float(np.abs(Mt).max()))
        Y, B, MU = rx.sync_timing_synchronize(Mt.reshape(1, -1))                              # the timing loop carries on from step_mf's state: bit for bit
        Yt, Bt, MUt2 = tm.synchronize(Mt.reshape(1, -1))
        assert np.array_equal(bits(Y), bits(Yt)) and np.array_equal(B, Bt) and np.array_equal(bits(MU), bits(MUt2))
        rx.sync_timing_extract(Y, B); tm.extract(Yt, Bt)
    MU, FRQ, PHS, Y, B = rx.sync_step_mf_synchronize([d], xs[k + 2:k + 3])
    MUt, FRQt, _, Yt, Bt = sm.synchronize([d], xs[k + 2:k + 3])
    head = slice(0, 2 * 40)                                                                  # the samples that read the handed-over memory
    assert np.max(np.abs(Y[0, head] - Yt[0, head])) <= 1e-4 * max(1.0, float(np.abs(Yt).max()))
    assert np.abs(Yt[0, head]).max() > 0.1
    rx.close()


def kernel_ms(rx, D, X, reps=3):
    """device time of one step_mf call on the handle (hipEvent, the shortest of `reps`), from the reset state every time"""
    import ctypes as C
    from dvbs2_amd import lib_binding as LB
    rx.L.dvbs2hip_timing_enable(rx.h, 1)
    out = []
    for _ in range(reps):
        rx.sync_step_mf_reset()
        rx.L.dvbs2hip_timing_reset(rx.h)
        rx.sync_step_mf_synchronize(D, X)
        tot, n = C.c_double(), C.c_int64()
        rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
        out.append(tot.value)
    rx.L.dvbs2hip_timing_enable(rx.h, 0)
    return min(out)


def test_the_setters_rules():
    from dvbs2_amd.lib_binding import Dvbs2HipError
    from dvbs2_amd.receiver import Dvbs2Hip
    xs = WR.case_inputs(1, 1, 2, 11)
    D, X = WR.call_inputs(xs, 1, 1, 0)
    rx = Dvbs2Hip(MODCOD, max_frames=2)
    rx.sync_coarse_set_pll(*WR.PLL)
    for bad in (2, -1):
        with pytest.raises(Dvbs2HipError) as ei:
            rx.sync_step_mf_set_kernel(bad)
        assert ei.value.code == -1                                      # DVBS2HIP_EINVAL
    # every condition of the loop holds with WAVE selected: ULTRA is still refused
    rx.sync_step_mf_set_kernel("WAVE")
    rx.sync_timing_set_type("ULTRA", 101)
    with pytest.raises(Dvbs2HipError) as ei:
        rx.sync_step_mf_synchronize(D, X)
    assert ei.value.code == -4                                          # DVBS2HIP_EUNSUPPORTED
    rx.sync_timing_set_type("FAST")
    # The choice survives sync_step_mf_reset and set_streams.  The two forms give the same bits, so which one ran shows only in the kernel's time: one stream is one lane
    # walking 81 taps per sample against 64 lanes sharing them, several times apart (results/coarse/README.md).  A call after the resets has to take WAVE's time, not
    # LANE's: below the geometric mean of the two, both measured here on the same frame.
    t_wave = kernel_ms(rx, D, X)
    rx.sync_step_mf_set_kernel("LANE")
    t_lane = kernel_ms(rx, D, X)
    print("step_mf, one frame of one stream: LANE %.2f ms, WAVE %.2f ms" % (t_lane, t_wave))
    assert t_wave < 0.5 * t_lane, (t_wave, t_lane)
    rx.sync_step_mf_set_kernel("WAVE")
    rx.sync_step_mf_reset()
    rx.sync_timing_set_streams(2)
    rx.sync_timing_set_streams(1)
    rx.sync_coarse_set_pll(*WR.PLL)
    t_after = kernel_ms(rx, D, X)
    assert t_after < (t_wave * t_lane) ** 0.5, (t_after, t_wave, t_lane)
    # ... and clears nothing: a change of form between two calls leaves the stream where it was (the twin runs on)
    rx.sync_step_mf_reset()
    tm, sm = WR.twins(1)
    for c, kern in enumerate(("LANE", "WAVE")):
        rx.sync_step_mf_set_kernel(kern)
        D, X = WR.call_inputs(xs, 1, 1, c)
        got, want = rx.sync_step_mf_synchronize(D, X), sm.synchronize(D, X)
        rx.sync_timing_extract(got[3], got[4]); tm.extract(want[3], want[4])
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b)), kern
    rx.close()


def test_the_file_workflow_with_wave_gives_the_lane_runs_bytes(tmp_path):
    """tests/test_acquire_files_gpu.py's workflow -- tx -> ch with a carrier offset and a delay -> rx --wl-phases -- once as it is and once with --smf-kernel WAVE: the same
    acquisition and the same sink file, byte for byte; without --wl-phases the flag is refused"""
    from dvbs2_amd import ch, rx, tx
    from dvbs2_amd.srcfile import save_src
    from test_acquire_files_gpu import FRAMES, FREQ, GOLD, LEARN, rx_argv
    b = np.unpackbits(np.load(os.path.join(GOLD, "src_K_14232.npy")))[:14232].astype(np.int32)
    src, f_tx, f_noisy = (str(tmp_path / n) for n in ("K_14232.src", "out_tx.bin", "out_tx_noisy.bin"))
    save_src(src, b)
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-type", "USER_BIN", "--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "USER", "--src-path", src,
                                                "--mod-cod", "QPSK-S_8/9", "--n-frames", str(FRAMES)]), out=log) == FRAMES
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", "QPSK-S_8/9",
                                                "-m", "8", "--chn-max-delay", "4.5", "--chn-max-freq-shift", str(FREQ)]), out=log) == FRAMES
    os.remove(f_tx)
    res = {}
    for name, extra in (("lane", []), ("wave", ["--smf-kernel", "WAVE"])):
        snk = str(tmp_path / (name + ".u8"))
        st = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--wl-phases", "--wl-frames"] + list(LEARN) + extra), out=log)
        res[name] = (st, open(snk, "rb").read())
    (sl, bl), (sw, bw) = res["lane"], res["wave"]
    assert sw["acquisition"] == sl["acquisition"] and sw["acquisition"]["acquired"], (sl["acquisition"], sw["acquisition"])
    assert len(bw) >= 64 * 14232 // 8 and bw == bl
    assert sw["frames"] == sl["frames"] and sw["be"] == 0 and sw["fe"] == 0
    with pytest.raises(ValueError, match="--wl-phases"):
        rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, str(tmp_path / "no.u8")) + ["--smf-kernel", "WAVE"]), out=log)
