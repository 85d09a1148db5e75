"""The held Gardner loop on the GPU (`--stm-type ULTRA`, stm_ultra_kernel: a wave per stream) against the CPU twin (tests/timing_ultra_twin.c), bit for bit: Y_N1, B_N1, MU,
and behind them extract's Y_N2, UFW, RDY, over calls with act off, on, on, off (the state is seen through the call that follows); hold sizes from one held sample to no
block at all, 1 to 65 streams, call boundaries, the host and the device form, the setters' errors, and FAST untouched on a fresh handle.  The inputs are the fast noisy
loop's of tests/test_timing_ultra_twin.py, and the coverage condition is asserted on the twin's trace here too."""
import numpy as np
import pytest

import timing_ref as TR
import timing_ultra_ref as UR
from dvbs2_amd import params as P

pytestmark = pytest.mark.gpu

MODCOD = "32APSK-S_3/4"                               # pl_frame 3402, 6804 complex samples per frame: the shortest frame the library has
PL = P.get_modcod(MODCOD).pl_frame
N = 2 * PL
# 1 and 2 held samples; 64 and 65 (the lanes wrap); the default; two wraps; one block with no tail; no block at all
HOLD_SIZES = (5, 6, 68, 69, 101, 133, N, N + 1)
ACTS = (False, True, True, False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def base():
    """one long noisy stream; the streams of a case are windows of it at ragged offsets"""
    return UR.noisy_frames(PL, len(ACTS) * 2 + 1, seed=1).ravel()


def windows(base, S, Fs, calls, salt):
    span = base.size // 2 - calls * Fs * N
    out = np.stack([base[2 * o: 2 * (o + calls * Fs * N)] for o in ((s * 97 + salt * 13) % span for s in range(S))])
    return [np.ascontiguousarray(out[:, 2 * c * Fs * N: 2 * (c + 1) * Fs * N]).reshape(S * Fs, 2 * N) for c in range(calls)]


def handle(S, Fs, H=None):
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(MODCOD, max_frames=S * Fs)
    rx.sync_timing_set_params(float(UR.NOISY["damping"]), UR.NOISY["nbw"], UR.NOISY["dg"])
    if S > 1:
        rx.sync_timing_set_streams(S)
    if H is not None:
        rx.sync_timing_set_type("ULTRA", H)
    return rx


def check(got, want, what):
    for name, g, w in zip(("Y", "B", "MU"), got, want):
        g, w = bits(g).ravel(), bits(w).ravel()
        assert np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:4], int((g != w).sum()))


@pytest.fixture(scope="module")
def traces():
    return []


@pytest.mark.parametrize("S", [1, 3, 65])
@pytest.mark.parametrize("H", HOLD_SIZES)
def test_synchronize_and_extract_match_the_twin(H, S, base, traces):
    Fs = 2
    xs = windows(base, S, Fs, len(ACTS), salt=H)
    rx = handle(S, Fs, H)
    tw = UR.UltraTiming(PL, H, S, **UR.NOISY)
    for c, (act, X) in enumerate(zip(ACTS, xs)):
        rx.sync_timing_set_act(act)
        tw.act = act
        got, want = rx.sync_timing_synchronize(X), tw.synchronize(X)
        check(got, want, (H, S, c))
        Y2, UFW, RDY = rx.sync_timing_extract(got[0], got[1])
        Y2t, UFWt, RDYt = tw.extract(want[0], want[1])
        assert np.array_equal(RDY, RDYt) and np.array_equal(UFW, UFWt), (H, S, c)
        assert np.array_equal(bits(Y2), bits(Y2t)), (H, S, c)
    rx.close()
    if H <= N:
        traces.append((H, np.concatenate(tw.first_hist)))


def test_every_strobe_history_heads_a_hold_block(traces):
    """the coverage condition of tests/test_timing_ultra_twin.py on the runs above, read from the twin's trace"""
    assert {H for H, _ in traces} >= set(UR.HOLD_SIZES)
    UR.assert_coverage(traces)


@pytest.mark.parametrize("H", [101, 68])
def test_one_call_of_four_frames_equals_four_calls_of_one(H, base):
    X = windows(base, 1, 4, 1, salt=3)[0]
    tw = UR.UltraTiming(PL, H, act=True, **UR.NOISY)
    want = tw.synchronize(X)
    a = handle(1, 4, H)
    a.sync_timing_set_act(True)
    check(a.sync_timing_synchronize(X), want, "1 x 4")
    a.close()
    b = handle(1, 1, H)
    b.sync_timing_set_act(True)
    parts = [b.sync_timing_synchronize(X[f:f + 1]) for f in range(4)]
    check([np.concatenate([p[k] for p in parts]) for k in range(3)], want, "4 x 1")
    b.close()


def test_device_form_matches_the_twin(base):
    import torch
    S, Fs, H = 3, 2, 101
    xs = windows(base, S, Fs, 2, salt=5)
    rx = handle(S, Fs, H)
    tw = UR.UltraTiming(PL, H, S, **UR.NOISY)
    F = S * Fs
    dev = torch.device("cuda:0")
    Yd, Bd, MU = torch.empty(F, 2 * N, dtype=torch.float32, device=dev), torch.empty(F, 2 * N, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.float32, device=dev)
    Y2, UFW, RDY = torch.zeros(F, N, dtype=torch.float32, device=dev), torch.empty(F, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    for act, X in zip((False, True), xs):
        rx.sync_timing_set_act(act)
        tw.act = act
        Xd = torch.from_numpy(X).to(dev)
        torch.cuda.synchronize()
        rx.sync_timing_synchronize_dev(Xd.data_ptr(), Yd.data_ptr(), Bd.data_ptr(), MU.data_ptr(), F)
        rx.sync_timing_extract_dev(Yd.data_ptr(), Bd.data_ptr(), Y2.data_ptr(), UFW.data_ptr(), RDY.data_ptr(), F)
        rx.synchronize()
        want = tw.synchronize(X)
        check((Yd.cpu().numpy(), Bd.cpu().numpy(), MU.cpu().numpy()), want, ("dev", act))
        Y2t, UFWt, RDYt = tw.extract(want[0], want[1])
        assert np.array_equal(RDY.cpu().numpy(), RDYt) and np.array_equal(UFW.cpu().numpy(), UFWt)
        assert np.array_equal(bits(Y2.cpu().numpy()), bits(Y2t))
    rx.close()


def test_set_type_clears_the_state_and_reset_clears_act(base):
    H = 101
    X0, X1 = windows(base, 1, 2, 2, salt=9)
    rx = handle(1, 2, H)
    rx.sync_timing_set_act(True)
    first = rx.sync_timing_synchronize(X0)
    assert not np.array_equal(rx.sync_timing_synchronize(X1)[0], first[0])
    rx.sync_timing_set_type("ULTRA", H)                                       # the state starts over; act is clear again
    tw = UR.UltraTiming(PL, H, **UR.NOISY)
    check(rx.sync_timing_synchronize(X0), tw.synchronize(X0), "after set_type: act off from the reset state")
    rx.sync_timing_set_type("ULTRA", H)
    rx.sync_timing_set_act(True)
    check(rx.sync_timing_synchronize(X0), first, "after set_type and set_act")
    rx.sync_timing_reset()                                                    # Synchronizer_timing::reset clears act
    tw.reset()
    check(rx.sync_timing_synchronize(X0), tw.synchronize(X0), "after reset")
    rx.close()


def test_setters_refuse_what_the_reference_refuses(base):
    from dvbs2_amd.lib_binding import Dvbs2HipError
    rx = handle(1, 1)
    for hold in (4, 0, -3):
        with pytest.raises(Dvbs2HipError) as ei:
            rx.sync_timing_set_type("ULTRA", hold)
        assert ei.value.code == -1                                            # DVBS2HIP_EINVAL
    with pytest.raises(Dvbs2HipError) as ei:
        rx.sync_timing_set_type(2, 101)
    assert ei.value.code == -1
    rx.sync_timing_set_type("ULTRA", 5)
    X = windows(base, 1, 1, 1, salt=2)[0]
    with pytest.raises(Dvbs2HipError) as ei:
        rx.sync_step_mf_synchronize(np.zeros(1, np.int32), X)
    assert ei.value.code == -4                                                # DVBS2HIP_EUNSUPPORTED: the coarse loop steps FAST's detector
    rx.sync_timing_set_type("FAST")
    rx.sync_step_mf_synchronize(np.zeros(1, np.int32), X)
    rx.close()


def test_fast_on_a_fresh_handle_is_still_the_fast_twin(base):
    """a handle that never calls set_type, one that sets act, and one that comes back from ULTRA: all the FAST twin bit for bit"""
    S, Fs = 3, 2
    X = windows(base, S, Fs, 1, salt=4)[0]
    want = TR.Timing(PL, S, **UR.NOISY).synchronize(X)
    for prep in (lambda rx: None, lambda rx: rx.sync_timing_set_act(True), lambda rx: (rx.sync_timing_set_type("ULTRA", 101), rx.sync_timing_set_type("FAST"))):
        rx = handle(S, Fs)
        prep(rx)
        check(rx.sync_timing_synchronize(X), want, "FAST")
        rx.close()
