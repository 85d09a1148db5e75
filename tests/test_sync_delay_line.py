"""What tests/test_sync_delay_line_gpu.py assumes of its inputs, checked on the CPU oracle alone: the crafted correlations put the delay where the
script says, the oracle's output is the four copies of Variable_delay_cc_naive::_filter driven by those delays, and the gapped stream moves the
delay in nearly every frame with an arg max that no rounding can move."""
import numpy as np
import pytest

from test_sync_delay_line_gpu import (CASES, CASE_IDS, MOVING_LOCK, SHORT, TRIGGER, case_inputs, expected_delays, first_diff, first_idx, materialized,
                                      moving_reference, oracle_run, splits)


class FourCopies:
    """Variable_delay_cc_naive(N, N / 2, N / 2) restated: _filter (Variable_delay_cc_naive.cpp:56-79), set_delay (:91-95), reset (:81-88).
    The output buffer is kept between calls, as the reference's socket buffer is."""

    def __init__(self, n):
        self.N, self.size = 2 * n, n + 1
        self.buff2 = np.zeros(4 * self.size, np.float32)
        self.Y = np.zeros(self.N, np.float32)
        self.head2, self.first_time = 0, True

    def reset(self):
        self.buff2[:] = 0
        self.head2, self.first_time = 0, True

    def filter(self, X, delay):
        N, D, head2 = self.N, 2 * min(delay, self.size - 1), self.head2
        start_Y = D - head2 if D > head2 else 0
        start_buff = head2 - D if D < head2 else 0
        end_buff = min(start_buff + D, self.buff2.size)
        if end_buff - start_buff > N - start_Y:
            end_buff -= (end_buff - start_buff) - (N - start_Y)
        if start_Y and not self.first_time:
            self.Y[:start_Y] = self.Y[N - start_Y:].copy()
        else:
            self.Y[:start_Y] = 0
        self.Y[start_Y:start_Y + end_buff - start_buff] = self.buff2[start_buff:end_buff]
        self.Y[D:] = X[:N - D]
        self.buff2[:D] = X[N - D:]
        self.first_time, self.head2 = False, D
        return self.Y.copy()


@pytest.mark.parametrize("modcod,name,F", CASES, ids=CASE_IDS)
def test_crafted_correlations_drive_the_oracles_delay_line_as_scripted(O, P, modcod, name, F):
    n, sc, X, cs, cp = case_inputs(P, modcod, name, F)
    assert np.unique(X.view(np.complex64)).size == X.size // 2      # every complex sample is distinct: a misplaced one cannot compare equal
    assert all(sum(cuts) + sc.prefix == len(sc.idxs) and min(cuts) >= 1 for cuts in splits(sc))
    DEL, FLG, TRI, Y = oracle_run(O, n, sc, X, cs, cp)
    want = expected_delays(n, sc.idxs)
    assert np.array_equal(DEL, want), first_diff(DEL, want)
    if sc.alpha == 0.0:                                     # the metric is a copy of the amplitude; no value above 0: metric 0
        amp = np.array([0.0 if i is None else a for i, a in zip(sc.idxs, sc.amps)], np.float32)
        assert np.array_equal(TRI, amp), first_diff(TRI, amp)
        assert np.array_equal(FLG, (amp > TRIGGER).astype(np.int32)) and 0 < FLG.sum() < FLG.size
    vd = FourCopies(n)
    for f in range(len(sc.idxs)):
        if sc.prefix and f == sc.prefix:
            vd.reset()
        Yf = vd.filter(X[f], (n - int(want[f])) % n)
        assert np.array_equal(Yf, Y[f]), (f, first_diff(Yf[None], Y[f][None]))


def test_no_frame_reads_further_back_than_the_frame_before_it():
    """What the four copies can reach, over every pair (head2, D) of a small frame: set_delay keeps D <= N - 2, so (1) the part of the delay line that survives in
    the output lies below head2 -- it is the tail of the frame before, never an older one -- and (2) the samples taken from "previous output" come from its part
    at or beyond head2, which that frame copied from ITS input.  So an output sample is a sample of input f, of input f - 1, or a zero of first_time, however the
    delay moves: the deeper steps of the kernel's walks (vd_source beyond one frame, vd_buff beyond frame f - 1) only ever produce delay-line entries at or beyond
    head2, which nothing reads.  A wrong deeper step is therefore not observable in any socket, here or on the GPU."""
    n = 6
    N = 2 * n
    for head2 in range(0, N - 1, 2):
        for D in range(0, N - 1, 2):
            start_Y = D - head2 if D > head2 else 0
            start_buff = head2 - D if D < head2 else 0
            end_buff = min(start_buff + D, 4 * (n + 1))
            if end_buff - start_buff > N - start_Y:
                end_buff -= (end_buff - start_buff) - (N - start_Y)
            surviving = min(start_Y + end_buff - start_buff, D) - start_Y      # the input's copy overwrites the output from D on
            assert surviving == min(D, head2) and start_buff + surviving <= head2, (head2, D)      # (1)
            assert N - start_Y >= head2, (head2, D)                                                # (2)


def test_scripts_reach_the_inputs_that_never_occur_in_lock(P):
    """delay 0, the largest delay, a jump between them, all-zero frames, ties, and a maximum in the un-averaged tail are all in the list"""
    n = P.get_modcod(SHORT).pl_frame
    seen = {}
    for modcod, name, F in CASES:
        if modcod == SHORT:
            sc = case_inputs(P, modcod, name, F)[1]
            seen[name] = (sc, (n - expected_delays(n, sc.idxs).astype(np.int64)) % n)
    q = seen["alt_0_max"][1]
    assert set(q[:-1]) == {0, n - 1} and np.all(np.abs(np.diff(q[:12])) == n - 1)
    assert np.all(np.diff(seen["up1"][1][:40]) == 1) and np.all(np.diff(seen["down1"][1][:40]) == -1)
    assert any(i is None for i in seen["zero_frames"][0].idxs) and any(not np.isscalar(i) and i is not None for i in seen["ties"][0].idxs)
    assert np.any(seen["odd_even"][1] % 2 == 1) and np.any(seen["odd_even"][1] % 2 == 0)
    for name, vw in (("tail_vw16", 16), ("tail_vw1000", 1000), ("tail_vw16_a", 16), ("tail_vw1000_a", 1000)):
        sc = seen[name][0]
        assert sc.vec_width == vw and sum(first_idx(i) >= (n // vw) * vw for i in sc.idxs) >= 5 and sum(first_idx(i) < (n // vw) * vw for i in sc.idxs) >= 4
    sc = seen["sof_seam"][0]
    F = len(sc.idxs) - 1
    assert sc.sof and all(sc.idxs[f] < 64 for f in (1, 3, F - 1))        # the frames that start a call in the splits
    assert seen["reset_large"][0].prefix == 3 and seen["reset_large"][1][3] >= n // 2


@pytest.mark.parametrize("F", [70, 130])
def test_gapped_stream_moves_the_delay_with_an_unambiguous_arg_max(O, F):
    ref = moving_reference(O, SHORT, F)
    n = ref.n
    assert ref.x.shape == (2 * F + MOVING_LOCK, 2 * n)
    assert ref.margin.min() >= 1e-3, (int(np.argmin(ref.margin)), ref.margin.min())
    for call in range(2):                                   # more than 64 frames of each call are not one run of the input stream
        need = materialized(ref.DEL[call * F:(call + 1) * F], n, F)
        assert need.sum() >= 65, (call, int(need.sum()))
        assert len(set(ref.DEL[call * F:(call + 1) * F])) >= F // 2
    assert np.all(ref.DEL[2 * F:] == ref.DEL[2 * F])        # the last call is in lock
