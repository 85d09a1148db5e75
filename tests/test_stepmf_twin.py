"""The CPU twin of the coarse-frequency loop (tests/stepmf_twin.c): the written-out cos / sin routine pinned against double precision, the twin pinned by a pure-Python
restatement through every branch, its pull-in on a noisy stream with a carrier offset, and dvbs2_amd/acquire.py driving a stand-in handle through the phases.
No GPU needed: these hold the yardstick that tests/test_stepmf_gpu.py holds k_stepmf.hip to."""
import ctypes as C

import numpy as np

import stepmf_ref as SR
import timing_ref as TR
from dvbs2_amd import params as P

MODCOD = "QPSK-S_8/9"
PL = P.get_modcod(MODCOD).pl_frame          # 8370 symbols, 16740 complex samples per frame at osf = 2


def test_turn_cos_sin_is_within_the_nco_bar_over_all_arguments():
    """dvbs2_amd/csrc/nco_turn.h against double-precision cos / sin over all 1e6 arguments: the bar is the 2e-6 nco_kernel is held to (docs/kernels.md); measured 9.3e-8"""
    worst = SR.lib().twin_nco_turn_worst()
    print("nco_turn_cs: worst |error| over 1e6 arguments = %.3e" % worst)
    assert worst < 2e-6
    assert worst < 1.5e-7                                            # and, recorded: it is an fp32 rounding or two, not a truncation error
    c, s = C.c_float(), C.c_float()
    for p in (0, 1, 124999, 125000, 125001, 250000, 333333, 500000, 624999, 750000, 875001, 999999):
        SR.lib().twin_nco_turn(p, C.byref(c), C.byref(s))
        pc, ps = SR.py_turn_cs(p)
        assert np.float32(c.value).view(np.uint32) == np.float32(pc).view(np.uint32) and np.float32(s.value).view(np.uint32) == np.float32(ps).view(np.uint32), p
    SR.lib().twin_nco_turn(0, C.byref(c), C.byref(s))
    assert (c.value, s.value) == (1.0, 0.0)
    for k, n in ((-50000, 999999), (123456, 654321), (-1, 1), (999999, 999999), (-1500000, 7)):
        assert SR.lib().twin_nco_index(k, n) == (k * n) % 1000000


def test_pll_gains_are_the_reference_formula():
    """set_PLL_coeffs (Synchronizer_freq_coarse_DVBS2_aib.cpp:94-113) for the phases' (1, 1/sqrt 2, 1e-4) and (.., 5e-5)"""
    for nbw in (1e-4, 5e-5):
        pg, ig = SR.pll_gains(1, np.float32(0.5 ** 0.5), nbw)
        z = 0.5 ** 0.5
        th = nbw / (z + 0.25 / z)
        d = 1 + 2 * z * th + th * th
        assert abs(pg - 4 * z * th / d / 2) <= 1e-6 * pg and abs(ig - 4 * th * th / d / 2) <= 1e-6 * ig


def test_twin_equals_the_python_restatement_bit_for_bit_through_every_branch():
    """two noisy frames with a carrier offset, fast loops (timing nbw 2e-2, PLL nbw 2e-2), the sample counter started 5000 short of its wrap, nu started off zero,
    non-zero DEL and last_delay: Y, B, MU, FRQ and the state equal the restatement's; the run is checked to have gone through both PLL branches, curr_idx < 1530, nu
    crossing 1e-6 steps, the counter's wrap and all four strobe histories"""
    F = 2
    X = SR.received_stream(MODCOD, F, 0.013, 6.0, seed=5, off=777, D=4.3)
    DEL = [4321, 4322]
    n0, k0, ld, carry = 1000000 - 5000, -12000, 11, 7
    tm = TR.Timing(PL, 1, np.float32(0.5 ** 0.5), 2e-2, 2.0)
    sm = SR.StepMf(PL, 1, tm)
    sm.set_pll(1, np.float32(0.5 ** 0.5), 2e-2)
    sm.cf[0].n, sm.cf[0].nu_k, sm.cf[0].last_delay = n0, k0, ld
    tm.head[0] = 2 * carry
    MU, FRQ, PHS, Y, B = sm.synchronize(DEL, X)
    r = SR.py_stepmf(X, DEL, PL, sm.taps, sm.P, tm.kp, tm.ki, sm.pg, sm.ig, n0=n0, nu_k0=k0, last_delay=ld, carry_cplx=carry)
    # the coverage
    assert min(r["sfc"].branches) > 0, r["sfc"].branches                                  # pilot window, the clearing at rem_pos 90, neither (curr_idx < 1530 among them)
    assert r["sfc"].branches[0] > 100
    assert (np.bincount(r["hist"], minlength=4) > 0).all(), np.bincount(r["hist"])         # all four strobe histories
    assert np.unique(r["nu_k"]).size > 50                                                  # nu crossed 1e-6 steps
    assert r["sfc"].mult.n == (n0 + F * 2 * PL) % 1000000 and n0 + F * 2 * PL > 1000000    # the counter wrapped
    # bit for bit
    assert np.array_equal(B.ravel()[0::2], r["B"]) and np.array_equal(B.ravel()[1::2], r["B"])
    assert np.array_equal(Y.ravel().view(np.complex64).view(np.uint64), r["Y"].view(np.uint64))
    assert np.array_equal(MU.view(np.uint32), r["MU"].view(np.uint32)) and np.array_equal(FRQ.view(np.uint32), r["FRQ"].view(np.uint32))
    assert not PHS.any()
    c, s = sm.cf[0], r["sfc"]
    assert (c.n, c.nu_k, c.curr_idx, c.last_delay) == (s.mult.n, s.mult.k, s.curr_idx, r["last_delay"])
    for a, b in ((c.lfs, s.lfs), (c.ifs, s.ifs), (c.dds, s.dds), (c.est, s.est), (c.prev[0], s.prev[0]), (c.pprev[1], s.pprev[1]), (tm.st[0].nco, r["stm"].nco),
                 (tm.st[0].lf_prev_in, r["stm"].lfp), (tm.st[0].mu, r["stm"].mu)):
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
    # and the stream carries on bit for bit across calls of one frame each
    tm2 = TR.Timing(PL, 1, np.float32(0.5 ** 0.5), 2e-2, 2.0)
    sm2 = SR.StepMf(PL, 1, tm2)
    sm2.set_pll(1, np.float32(0.5 ** 0.5), 2e-2)
    sm2.cf[0].n, sm2.cf[0].nu_k, sm2.cf[0].last_delay = n0, k0, ld
    tm2.head[0] = 2 * carry
    a = sm2.synchronize(DEL[:1], X[:1])
    b = sm2.synchronize(DEL[1:], X[1:])
    assert np.array_equal(np.concatenate([a[3].ravel(), b[3].ravel()]), Y.ravel()) and np.array_equal(np.concatenate([a[1], b[1]]), FRQ)


# the pull-in: offset, Eb/N0, seed (results/coarse/README.md records them with the residual reached, and what the traces' own 3.8 dB gives)
PULL_IN = dict(freq=0.05, ebn0=15.0, seed=1)


def run_phases_on_the_twin(freq, ebn0, seed, F=300, D=4.5):
    """waiting is left out (the loops start from reset on a stream that is there from the first sample): 150 frames at 1e-4, 150 at 5e-5, the frame synchronizer's delay
    fed back by one call -> estimated_freq after every frame"""
    from oracle import oracle as O
    X = SR.received_stream(MODCOD, F, freq, ebn0, seed=seed, off=1234, D=D)
    sm, sf = SR.StepMf(PL), O.SyncFrame(PL)
    d, est = 0, []
    for f in range(F):
        if f == 150:
            sm.set_pll(1, np.float32(0.5 ** 0.5), 5e-5)
        MU, FRQ, PHS, Y, B = sm.synchronize([d], X[f:f + 1])
        Y2, UFW, RDY = sm.tm.extract(Y, B)
        if RDY[0]:
            d, _ = sf.synchronize(O.agc(Y2[0], 1.0))
        est.append(float(FRQ[0]))
    return np.array(est), sf


def test_twin_pulls_in_a_carrier_offset_with_the_reference_constants():
    """a noisy QPSK-S 8/9 stream from the oracle's TX mirror, 0.05 cycles per sample off, the channel's delay 4.5, the reference's PLL constants (1, 1/sqrt 2, 1e-4 then
    5e-5) and Gardner defaults: after learning 2 the estimate is within 5e-4 cycles per SYMBOL of the truth (the range the fine synchronizers are shown to remove,
    DESIGN.md section 2).  The Gardner step is Synchronizer_Gardner_fast_osf2::step's form: the loop locks with it."""
    est, sf = run_phases_on_the_twin(**PULL_IN)
    residual = (est[-1] - PULL_IN["freq"]) * 2.0                    # cycles per sample -> per symbol (osf = 2)
    print("pull-in: offset %.3f cycles/sample, Eb/N0 %.1f dB, seed %d -> residual %.3e cycles/symbol; frame-end estimates of learning 2: mean %.6f, std %.2e" % (
        PULL_IN["freq"], PULL_IN["ebn0"], PULL_IN["seed"], residual, est[150:].mean(), est[150:].std()))
    assert abs(residual) < 5e-4
    assert sf.packet_flag


def test_acquire_drives_the_phases_in_the_reference_order():
    """dvbs2_amd/acquire.py on a stand-in handle (the twins and the oracle): waiting until the packet flag, the three resets, learning 1 and 2 with their bandwidths,
    learning 3 with the PLL frozen, DEL fed back by one call; a source that never shows a frame makes the waiting phase give up"""
    from dvbs2_amd.acquire import acquire
    from dvbs2_amd.iqfile import ProcessingAborted
    X = SR.received_stream(MODCOD, 80, 0.02, 12.0, seed=9, off=500, D=4.5)
    it = iter(X)

    def receive():
        try:
            return next(it)[None, :]
        except StopIteration:
            raise ProcessingAborted()

    h = SR.TwinHandle(MODCOD)
    res = acquire(h, receive, n_frames=1, learn1=20, learn2=20, learn3=6, wait_max=30)
    assert res["flag"] and res["acquired"]
    fr = res["frames"]
    assert 1 <= fr["waiting"] <= 30 and (fr["learning1"], fr["learning2"], fr["learning3"]) == (20, 20, 6)
    assert abs(res["freq"][0] - 0.02) < 5e-3 and abs(res["nu"][0] + res["freq"][0]) <= 1.1e-6
    names = [e[0] for e in h.log]
    i_reset = names.index("reset_step_mf")
    assert names[0] == "set_pll" and h.log[0][1:] == (1, 1e-4)
    assert names[i_reset:i_reset + 4] == ["reset_step_mf", "reset_frame", "reset_timing", "set_pll"]
    assert names[:i_reset].count("step_mf") == fr["waiting"]
    plls = [e for e in h.log if e[0] == "set_pll"]
    assert [p[2] for p in plls] == [1e-4, 1e-4, 5e-5]
    i_pll2 = len(h.log) - 1 - h.log[::-1].index(plls[2])
    assert names[i_reset:i_pll2].count("step_mf") == 20 and names[i_pll2:].count("step_mf") == 20
    # DEL is the frame synchronizer's delay of the call before
    last = 0
    for e in h.log:
        if e[0] == "step_mf":
            assert e[1] == last
        if e[0] == "frame":
            last = e[1]
    # learning 3: the shift alone, at the frequency the loop left, then the block-wise tasks up to the fine synchronizer
    i_l3 = names.index("shift")
    assert "step_mf" not in names[i_l3:] and names[i_l3:].count("shift") == 6 and names[i_l3:].count("timing") == 6 and names[i_l3:].count("fine") >= 5
    assert len({e[1] for e in h.log if e[0] == "shift"}) == 1
    # a source without a signal: the waiting phase gives up and says so
    rng = np.random.default_rng(1)
    h2 = SR.TwinHandle(MODCOD)
    res2 = acquire(h2, lambda: rng.standard_normal((1, 4 * PL)).astype(np.float32), n_frames=1, learn1=2, learn2=2, learn3=1, wait_max=5)
    assert not res2["flag"] and not res2["acquired"] and res2["frames"]["waiting"] == 5 and res2["frames"]["learning1"] == 0
