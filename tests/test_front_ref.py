"""CPU half of the fused front end's float64 check (tests/front_ref.py; the kernels' half is tests/test_front_fp64_gpu.py).

Two questions, neither of which needs a GPU.  Is the twin right: stage by stage against the oracle chain, on the inputs the GPU tests use, with the
oracle inside every bar the device will be held to.  Are the bars worth having: each of eleven mistakes a front-end kernel could make is put into
the twin's own answer -- a faultless device's sockets -- and judge() has to name a bar it breaks."""
import numpy as np
import pytest

import front_ref as R
from helpers import chain

ALL = R.modcods()


def _mc(O, modcod):
    return chain(O, modcod).mc


@pytest.mark.parametrize("modcod", ALL)
def test_twin_matches_the_oracle_chain_stage_by_stage(O, modcod):
    """PL sequence, constellation and interleaver table bit for bit; the payload symbols bit for bit; the oracle's fp32 estimates and LLRs inside
    the device's bars (sigma 1e-4 relative, 2e-3 dB, 1e-4 max(1, |L|)) against the twin: the reference alone stays inside them."""
    ch = chain(O, modcod)
    mc = ch.mc
    assert np.array_equal(R.pl_seq(), O.pl_rand_seq(0))
    assert np.array_equal(R.constellation(mc).ravel(), ch.cstl.ravel())
    assert np.array_equal(R.itl_table(mc), ch.lut)
    _, pl, _, sigma = R.frames(O, modcod)
    F = pl.shape[0]
    sig = R.sigmas(sigma, F)
    LLRo, ESTo = np.empty((F, mc.N_ldpc), np.float32), np.empty((F, 3), np.float32)
    for f in range(F):
        xo = O.framer_remove_plh(O.pl_scramble(pl[f], 90, False), mc.N_xfec)
        x = R.xfec(pl[f], mc)
        assert np.array_equal(x.ravel().view(np.uint32), xo.view(np.uint32))
        ESTo[f] = O.estimate(xo, mc.code_rate, mc.bps)
        e64 = R.estimate64(x, mc)
        assert abs(ESTo[f, 0] - e64[0]) <= 0.5 * R.SIGMA_BAR * e64[0]              # (the inputs leave the reference inside the bar by a factor of two)
        assert abs(ESTo[f, 1] - e64[1]) <= R.DB_BAR and abs(ESTo[f, 2] - e64[2]) <= R.DB_BAR
        Lo = O.demodulate(ch.cstl, mc.bps, sig[f], xo)
        L64 = R.llr64(x, sig[f], mc)
        assert np.all(R.norm_err(Lo.reshape(L64.shape), L64) <= R.LLR_BAR)
        LLRo[f, ch.lut] = O.demodulate(ch.cstl, mc.bps, ESTo[f, 0], xo)
    # the oracle chain as a device under judge(), sigma estimated: every bar holds (the tight one by construction: it is its own yardstick)
    rows = R.judge(mc, pl, LLRo, ESTo, None, R.oracle_rms_of(O, modcod))
    assert not R.broken(rows), rows
    # and the twin's own sockets, both ways
    for s in (None, sig):
        rows = R.judge(mc, pl, *R.twin_call(mc, pl, s), s, R.oracle_rms_of(O, modcod))
        assert not R.broken(rows), rows


@pytest.mark.parametrize("modcod", R.HIGH_SNR["modcods"])
def test_high_snr_inputs_keep_the_oracle_inside_the_bar_and_reach_both_paths(O, modcod):
    """Case E's inputs (30 dB frames demapped with sigma 0.05, 0.1, 0.2): the oracle's pairwise max* stays inside the contract bar there as well, the
    signs are the sent code word, the call holds symbols on both sides of the far-path threshold, and the fp32 model of the kernel's two forms
    (near32 / far32) passes the bars the device will be held to."""
    ch = chain(O, modcod)
    mc = ch.mc
    H = R.HIGH_SNR
    _, pl, cw, _ = R.frames(O, modcod, 3, H["ebn0"], H["seed"])
    sig = np.array(H["sigmas"], np.float32)
    n_far = 0
    LLRm = np.empty((3, mc.N_ldpc), np.float32)
    for f in range(3):
        x = R.xfec(pl[f], mc)
        L64 = R.llr64(x, sig[f], mc)
        Lo = O.demodulate(ch.cstl, mc.bps, sig[f], x.ravel()).reshape(L64.shape)
        assert np.all(R.norm_err(Lo, L64) <= R.LLR_BAR)
        assert np.array_equal((R.deinterleave(L64, mc) < 0).astype(np.int32), cw[f])
        n_far += int(R.far_symbols(x, sig[f], mc).sum())
        LLRm[f] = R.deinterleave(R.model32(x, sig[f], mc), mc)
    assert 0 < n_far < 3 * mc.N_xfec
    EST = np.zeros((3, 3), np.float32)
    EST[:, 0] = sig
    assert not R.broken(R.judge(mc, pl, LLRm, EST, sig, R.oracle_rms_of(O, modcod)))


@pytest.mark.parametrize("modcod", ALL)
def test_fp32_model_of_the_general_demapper_is_inside_the_tight_bar(O, modcod):
    """The derivation of TIGHT_MARGIN (results/front_fp64/README.md) as a test: the general demapper's arithmetic with every fp32 operation rounded
    correctly stays below HALF the margin on every frame of the GPU tests' inputs, sigma given and at the M2M4 estimate's sigma (the other half is
    for v_exp / v_log, good to one ulp where a correct rounding is good to half) -- and needs more than 4x the oracle's rms, which is the finding."""
    mc = _mc(O, modcod)
    _, pl, _, sigma = R.frames(O, modcod)
    sig = R.sigmas(sigma, 3)
    worst = 0.0
    for s in (sig, np.array([R.estimate64(R.xfec(pl[f], mc), mc)[0] for f in range(3)], np.float32)):
        LLR = np.stack([R.deinterleave(R.model32(R.xfec(pl[f], mc), s[f], mc), mc) for f in range(3)]).astype(np.float32)
        EST = np.zeros((3, 3), np.float32)
        EST[:, 0] = s
        rows = R.judge(mc, pl, LLR, EST, s, R.oracle_rms_of(O, modcod), margin=R.TIGHT_MARGIN / 2)
        assert not R.broken(rows), rows
        worst = max(worst, max(r["rms_e"] / r["rms_oracle"] for r in rows))
    assert worst >= 4.0          # the offset of 120 in the exponent and in the log2 costs bits: see the README


# ---------------------------------------------------------------------------------------------------------------- the mistakes
def _natural(mc, pl, sig, xfec_hooks=None, deitl_hooks=None, sigma_of=None):
    """a call's LLR socket from the twin with hooks in its maps"""
    F = pl.shape[0]
    out = np.empty((F, mc.N_ldpc), np.float32)
    for f in range(F):
        x = R.xfec(pl[f], mc, **(xfec_hooks or {}))
        out[f] = R.deinterleave(R.llr64(x, sig[sigma_of(f) if sigma_of else f], mc), mc, **(deitl_hooks or {}))
    return out


def _given(O, modcod, F=3):
    mc = _mc(O, modcod)
    _, pl, _, sigma = R.frames(O, modcod, F)
    sig = R.sigmas(sigma, F)
    EST = np.zeros((F, 3), np.float32)
    EST[:, 0] = sig
    return mc, pl, sig, EST


def _seam_trip(mc, pl, sig):
    """32APSK-S at three slices of 1280 symbols: the first 256-symbol trip of the second slice written from the last trip of the first"""
    LLR = np.empty((pl.shape[0], mc.N_ldpc), np.float32)
    for f in range(pl.shape[0]):
        L = R.llr64(R.xfec(pl[f], mc), sig[f], mc)
        L[1280:1536] = L[1024:1280]
        LLR[f] = R.deinterleave(L, mc)
    return LLR


MISTAKES = [
    # name, MODCOD, what the kernel would have done, the bar that has to see it
    ("a_pilot_skip_off_by_one_from_the_second_block", "QPSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, dict(pilot_slip=1)), "contract"),
    ("b_pl_sequence_shifted_by_one", "QPSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, dict(seq_shift=1)), "contract"),
    ("c_two_derotation_quadrants_exchanged", "8PSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, dict(swap_quadrants=True)), "contract"),
    ("d_column_order_mirrored_top_left", "8PSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, None, dict(mirror=True)), "contract"),
    ("d_column_order_mirrored_top_right", "8PSK-S_3/5", lambda mc, pl, sig: _natural(mc, pl, sig, None, dict(mirror=True)), "contract"),
    ("e_bit_order_inside_a_symbol_reversed", "16APSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, None, dict(reverse_bits=True)), "contract"),
    ("f_symbols_of_a_pair_exchanged", "QPSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, None, dict(swap_pairs=True)), "contract"),
    ("g_last_symbol_not_written", "32APSK-S_3/4", lambda mc, pl, sig: _natural(mc, pl, sig, None, dict(drop_last=True)), "nan"),
    ("h_next_frames_sigma", "16APSK-S_8/9", lambda mc, pl, sig: _natural(mc, pl, sig, sigma_of=lambda f: (f + 1) % 3), "contract"),
    ("j_trip_at_a_slice_seam_from_the_neighbouring_slice", "32APSK-S_3/4", _seam_trip, "contract"),
]


@pytest.mark.parametrize("name,modcod,make,bar", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_bars_reject_the_mistake(O, name, modcod, make, bar):
    """sigma given, three frames with three sigmas: the twin's answer passes, the same answer with the mistake in it breaks the named bar"""
    mc, pl, sig, EST = _given(O, modcod)
    yard = R.oracle_rms_of(O, modcod)
    assert not R.broken(R.judge(mc, pl, *R.twin_call(mc, pl, sig), sig, yard))
    rows = R.judge(mc, pl, make(mc, pl, sig), EST, sig, yard)
    assert bar in R.broken(rows), (name, rows)
    assert all(r["broken"] for r in rows), (name, rows)                   # in every frame, not by the luck of one


@pytest.mark.parametrize("modcod,lanes_x_spt", [("QPSK-S_8/9", 8192), ("8PSK-N_8/9", 22528), ("QPSK-N_8/9", 32768)])
def test_bars_reject_i_moments_divided_by_the_lane_count(O, modcod, lanes_x_spt):
    """(i) the register-resident kernels' padding lanes counted: moment sums over 1024 lanes x 8, 22 or 32 symbols instead of n_sym.  The LLRs follow
    the wrong sigma consistently, so only the estimate's bars can see it: all three must."""
    mc = _mc(O, modcod)
    _, pl, _, _ = R.frames(O, modcod)
    assert mc.N_xfec < lanes_x_spt < mc.N_xfec + 1024
    LLR, EST = R.twin_call(mc, pl, None)
    yard = R.oracle_rms_of(O, modcod)
    assert not R.broken(R.judge(mc, pl, LLR, EST, None, yard))
    for f in range(pl.shape[0]):
        EST[f] = R.estimate64(R.xfec(pl[f], mc), mc, divisor=lanes_x_spt)
        LLR[f] = R.front64(pl[f], mc, EST[f, 0])
    rows = R.judge(mc, pl, LLR, EST, None, yard)
    assert all({"sigma", "ebn0", "esn0"} <= r["broken"] for r in rows), rows


def test_bars_reject_an_estimate_echoed_from_the_wrong_frame(O):
    """(h), the other half: EST has to echo sigma_in frame by frame, bit for bit"""
    mc, pl, sig, EST = _given(O, "QPSK-S_8/9")
    LLR, _ = R.twin_call(mc, pl, sig)
    assert "echo" in R.broken(R.judge(mc, pl, LLR, np.roll(EST, 1, axis=0), sig, R.oracle_rms_of(O, "QPSK-S_8/9")))


@pytest.mark.parametrize("modcod", R.HIGH_SNR["modcods"])
def test_bars_reject_k_far_path_replaced_by_the_near_form(O, modcod):
    """(k) on case E's inputs: the symbols past the far-path threshold demapped by the near form after all, whose weaker subset has left fp32's
    range.  The frame with sigma 0.05 holds such symbols for every one of the four constellations; its contract bar has to break, while the
    model with the far path in place passes (test_high_snr_inputs_...)."""
    mc = _mc(O, modcod)
    H = R.HIGH_SNR
    _, pl, _, _ = R.frames(O, modcod, 3, H["ebn0"], H["seed"])
    sig = np.array(H["sigmas"], np.float32)
    EST = np.zeros((3, 3), np.float32)
    EST[:, 0] = sig
    with np.errstate(invalid="ignore"):
        LLR = np.stack([R.deinterleave(R.near32(R.xfec(pl[f], mc), sig[f], mc), mc) for f in range(3)]).astype(np.float32)
        rows = R.judge(mc, pl, LLR, EST, sig, R.oracle_rms_of(O, modcod))
    assert "contract" in rows[0]["broken"], rows


def test_tight_bar_sees_a_sigma_off_in_the_fifth_digit(O):
    """what the tight bar is for: LLRs scaled as by a sigma wrong by 2e-5 pass the contract bar and break the tight one"""
    mc, pl, sig, EST = _given(O, "16APSK-S_8/9")
    LLR, _ = R.twin_call(mc, pl, sig * np.float32(1 + 2e-5))
    rows = R.judge(mc, pl, LLR, EST, sig, R.oracle_rms_of(O, "16APSK-S_8/9"))
    assert all(r["broken"] == {"tight"} for r in rows), rows
