"""The CPU twin of the held Gardner loop (tests/timing_ultra_twin.c, `--stm-type ULTRA`): pinned bit for bit by the block-parallel NumPy restatement
(tests/timing_ultra_ref.py), consistent across call boundaries, equal to the plain loop when no block fits, the reference's gains, locked behind a channel delay once `act` is
set, and run over inputs that put every strobe history at the head of a hold block.  No GPU needed: these hold the yardstick that tests/test_timing_ultra_gpu.py holds
libdvbs2hip's stm_ultra_kernel to."""
import numpy as np
import pytest

import timing_ref as TR
import timing_ultra_ref as UR
from dvbs2_amd import params as P

PL = P.get_modcod("32APSK-S_3/4").pl_frame           # 3402 symbols, 6804 complex samples per frame: the shortest frame the library has
N = 2 * PL


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


@pytest.fixture(scope="module")
def traces():
    """(H, first_hist) of every act-on twin run of the parametrised comparison below, for the coverage condition"""
    return []


@pytest.mark.parametrize("H", UR.HOLD_SIZES)
def test_twin_equals_the_block_parallel_restatement_bit_for_bit(H, traces):
    """the fast noisy loop: one frame with act off from the reset state, then two frames with act on (the carried history, buffer and NCO are whatever the loop left);
    and act on from the reset state"""
    assert N // H >= 1
    X = UR.noisy_frames(PL, 3, seed=H)
    tw = UR.UltraTiming(PL, H, **UR.NOISY)
    st = UR.PyState()
    for act, x in ((False, X[:1]), (True, X[1:])):
        tw.act = act
        Y, B, MU = tw.synchronize(x)
        Yp, Bp, MUp = UR.py_synchronize(st, x, N, H, act, tw.kp, tw.ki)
        assert np.array_equal(B, Bp), (act, np.flatnonzero(B.ravel() != Bp.ravel())[:4])
        assert np.array_equal(bits(Y), bits(Yp)), (act, np.flatnonzero(bits(Y).ravel() != bits(Yp).ravel())[:4])
        assert np.array_equal(bits(MU), bits(MUp)), act
    assert 0.4 < B.mean() < 0.6 and tw.st[0].lf_prev_in != 0.0              # the loop is running
    traces.append((H, np.concatenate(tw.first_hist)))
    tw2 = UR.UltraTiming(PL, H, act=True, **UR.NOISY)
    assert same(tw2.synchronize(X[:1]), UR.py_synchronize(UR.PyState(), X[:1], N, H, True, tw2.kp, tw2.ki))
    traces.append((H, np.concatenate(tw2.first_hist)))


def test_every_strobe_history_heads_a_hold_block(traces):
    """the coverage condition, on the twin's own trace: over the runs above each of the four histories occurs at a block's first held sample at least 3 times, and at least
    once where a block holds more than 64 samples (H = 69, 101: the kernel's second pass over the lanes)"""
    assert sorted({H for H, _ in traces}) == sorted(UR.HOLD_SIZES)
    UR.assert_coverage(traces)


@pytest.mark.parametrize("H,act", [(101, True), (68, True), (101, False)])
def test_one_call_of_four_frames_equals_four_calls_and_two_plus_two(H, act):
    X = UR.noisy_frames(PL, 4, seed=40 + H)

    def run(cuts):
        t = UR.UltraTiming(PL, H, act=act, **UR.NOISY)
        out = [t.synchronize(X[a:b]) for a, b in cuts]
        return [np.concatenate([o[k].ravel() for o in out]) for k in range(3)]

    whole = run([(0, 4)])
    assert same(whole, run([(0, 1), (1, 2), (2, 3), (3, 4)]))
    assert same(whole, run([(0, 2), (2, 4)]))


def test_a_hold_size_no_frame_can_fit_is_the_plain_loop():
    X = UR.noisy_frames(PL, 2, seed=7)
    on = UR.UltraTiming(PL, N + 1, act=True, **UR.NOISY)
    off = UR.UltraTiming(PL, N + 1, act=False, **UR.NOISY)
    plain = off.synchronize(X)
    assert same(on.synchronize(X), plain)
    assert on.first_hist[0].size == 0
    fits = UR.UltraTiming(PL, N, act=True, **UR.NOISY)                       # one block, no tail: it does differ
    assert not same(fits.synchronize(X), plain)


def test_loop_gains_are_the_reference_formula():
    """Synchronizer_Gardner_ultra_osf2::set_loop_filter_coeffs (.cpp:341-351): FAST's formula, for the factory defaults sqrt(0.5), 5e-5, 2"""
    kp, ki = UR.gains()
    z, bn, g = 0.5 ** 0.5, 5e-5, 2.0
    th = bn / 2 / (z + 0.25 / z)
    d = (1 + 2 * z * th + th * th) * -1 * g
    assert abs(kp - 4 * z * th / d) <= 1e-6 * abs(kp) and abs(ki - 4 * th * th / d) <= 1e-6 * abs(ki)
    assert (kp, ki) == TR.gains()
    assert UR.gains(np.float32(0.9), 1e-3, 1.5) == TR.gains(np.float32(0.9), 1e-3, 1.5)


def test_loop_stays_locked_behind_the_channel_delay_once_it_holds():
    """high SNR, a channel delay of 4.5 samples, the factory loop: 56 frames with act off (the learning phases), then 8 with act on and the default hold size.  mu stays
    within the band test_loop_locks_behind_the_channel_delay sets for FAST (0.07 around the delay's fractional phase) and the extracted symbols lie on the QPSK points"""
    D, F_learn, F_hold = 4.5, 56, 8
    qpsk = np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2)
    plq = P.get_modcod("QPSK-S_8/9").pl_frame
    X = TR.shaped_stream((F_learn + F_hold) * 2 * plq, qpsk, D, 0.05, np.random.default_rng(450)).reshape(F_learn + F_hold, -1)
    t = UR.UltraTiming(plq, 101)
    Y, B, MU = t.synchronize(X[:F_learn])
    t.extract(Y, B)
    t.act = True
    Y, B, MU = t.synchronize(X[F_learn:])
    Y2, UFW, RDY = t.extract(Y, B)
    assert RDY.tolist() == [1] and not UFW.any()
    assert (np.bincount(np.concatenate(t.first_hist[1:]), minlength=4)[[0, 3]] == 0).all()      # locked: no stuffing, no skipping
    want = (-D) % 1.0
    err = np.abs((MU - want + 0.5) % 1.0 - 0.5)
    assert err.max() < 0.07, (MU, want)
    s = Y2[-2:].ravel().view(np.complex64).astype(complex)
    s = s / (np.abs(s.real).mean() * np.sqrt(2))
    ideal = (np.sign(s.real) + 1j * np.sign(s.imag)) / np.sqrt(2)
    evm = np.sqrt(np.mean(np.abs(s - ideal) ** 2))
    assert evm < 0.15, evm
