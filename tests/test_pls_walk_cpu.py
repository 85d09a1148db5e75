"""The PLHEADER walk without a GPU: the twin of tests/pls_walk_ref.py against hand-made chains whose answers are written out here, dvbs2_amd.params.find_vcm_start
against the twin run from every offset, the VCM length table, and the argument errors of `tx --mod-cod-seq` and `rx --mod-cod VCM` (raised before any handle is made)."""
import numpy as np
import pytest

import pls_walk_ref as W

NOISE = 99                                                                           # a value the table below gives no length
LEN = np.zeros(256, np.int32)
LEN[10], LEN[20], LEN[50] = 180, 360, 90
LEN[30], LEN[40] = 100, 72                                                           # no multiple of 18; below 90: both count as 0
Q_MIN = 0.5


def scan_of(n_sym, headers):
    """(PLS, MET, ENE) of a scan of n_sym symbols: q = 1 / 90 and NOISE everywhere but at {offset: value or (value, MET)}, where q = MET^2 / 90 (MET 9: 0.9)"""
    K = n_sym - 89
    PLS, MET, ENE = np.full(K, NOISE, np.int32), np.ones(K, np.float32), np.ones(K, np.float32)
    for k, v in headers.items():
        if k < K:                                                                    # (a header the buffer cuts off is in no scan)
            PLS[k], MET[k] = v if isinstance(v, tuple) else (v, 9.0)
    return PLS, MET, ENE


def run(n_sym, headers, start, max_out=100, LEN=LEN):
    OFF, VAL, Q, RES = W.walk_scan(*scan_of(n_sym, headers), start, LEN, Q_MIN, max_out)
    return OFF.tolist(), VAL.tolist(), RES.tolist()


CHAIN = {7: 10, 187: 20, 547: 10, 727: 50, 817: 20}                                  # lengths 180, 360, 180, 90, 360: the next header would be at 1177


def test_end_behind_the_last_whole_frame():
    assert run(1177 + 89, CHAIN, 7) == ([7, 187, 547, 727, 817], [10, 20, 10, 50, 20], [5, 1177, W.END, 0])      # 89 symbols left: no header fits
    assert run(1177, CHAIN, 7)[2] == [5, 1177, W.END, 0]                             # the last frame ends exactly at n_sym: NEXT = n_sym


def test_end_on_a_frame_the_buffer_cuts_off():
    assert run(1176, CHAIN, 7) == ([7, 187, 547, 727], [10, 20, 10, 50], [4, 817, W.END, 0])                     # one symbol of the last frame is missing
    assert run(817 + 90, CHAIN, 7)[2] == [4, 817, W.END, 0]                          # its header is all there is of it
    assert run(817 + 89, CHAIN, 7)[2] == [4, 817, W.END, 0]                          # and not even that: step 1


def test_lost_on_a_weak_header_and_on_a_value_without_a_length():
    weak = dict(CHAIN); weak[547] = (10, 6.0)                                        # q = 0.4 < q_min
    assert run(2000, weak, 7) == ([7, 187], [10, 20], [2, 547, W.LOST, 0])
    edge = dict(CHAIN); edge[547] = (10, float(np.sqrt(np.float32(45.0))))           # q within an ulp of q_min: the comparison is the fp32 one, whichever way it falls
    q = np.float32(edge[547][1]) * np.float32(edge[547][1]) / (np.float32(90) * np.float32(1))
    assert run(2000, edge, 7)[2][0] == (5 if q >= np.float32(Q_MIN) else 2)
    assert run(2000, CHAIN, 7)[2] == [5, 1177, W.LOST, 0]                            # noise where the sixth header would be
    for v in (30, 40, NOISE):                                                        # 100 symbols, 72 symbols, no entry
        bad = dict(CHAIN); bad[187] = v
        assert run(2000, bad, 7) == ([7], [10], [1, 187, W.LOST, 0])
    nan = scan_of(2000, CHAIN)
    nan[1][187] = np.nan                                                             # not q >= q_min
    assert W.walk_scan(*nan, 7, LEN, Q_MIN, 100)[3].tolist() == [1, 187, W.LOST, 0]
    zero = scan_of(2000, CHAIN)
    zero[1][187] = zero[2][187] = 0                                                  # ENE = 0: q = 0
    assert W.walk_scan(*zero, 7, LEN, Q_MIN, 100)[3].tolist() == [1, 187, W.LOST, 0]


def test_full_and_the_order_of_the_stops():
    assert run(2000, CHAIN, 7, max_out=3) == ([7, 187, 547], [10, 20, 10], [3, 727, W.FULL, 0])
    assert run(2000, CHAIN, 7, max_out=1)[2] == [1, 187, W.FULL, 0]
    assert run(2000, CHAIN, 7, max_out=5)[2] == [5, 1177, W.LOST, 0]                 # max_out frames and then no header: steps 1 to 4 come before 5
    assert run(1177, CHAIN, 7, max_out=5)[2] == [5, 1177, W.END, 0]
    assert run(1176, CHAIN, 7, max_out=4)[2] == [4, 817, W.END, 0]                   # the frame past max_out is cut off: END, not FULL


def test_starts():
    assert run(2000, CHAIN, 187)[0] == [187, 547, 727, 817]
    assert run(2000, CHAIN, 0)[2] == [0, 0, W.LOST, 0]
    assert run(2000, CHAIN, 2000)[2] == [0, 2000, W.END, 0]                          # start = n_sym
    assert run(2000, CHAIN, 1911)[2] == [0, 1911, W.END, 0]                          # 89 symbols behind start
    assert run(2000, CHAIN, 1910)[2] == [0, 1910, W.LOST, 0]                         # 90: a header's worth, of noise


def test_group():
    CNT, IDX = W.group([10, 20, 10, 50, 20, 0])
    assert IDX.tolist() == [5, 0, 2, 1, 4, 3]
    assert CNT.sum() == 6 and (CNT[0], CNT[10], CNT[20], CNT[50]) == (1, 2, 2, 1)
    CNT, IDX = W.group([])
    assert CNT.sum() == 0 and len(IDX) == 0


def test_every_vcm_frame_length_is_a_multiple_of_18(P):
    T = P.VCM_FRAME_SYMBOLS
    assert T.shape == (256,) and T.dtype == np.int32
    assert (T % 18 == 0).all() and ((T == 0) | (T >= 90)).all()
    assert T[0] == 3330 and T[1] == 0                                                # the dummy frame without pilots; the one with the pilot bit is left out
    assert np.array_equal(T[1:], P.PLS_FRAME_SYMBOLS[1:]) and P.PLS_FRAME_SYMBOLS[0] == 0
    assert np.array_equal(W.clean_len(T), T)
    for mc in P.MODCODS.values():
        assert T[P.pls_value(mc)] == mc.pl_frame and T[P.pls_value(mc, False)] == 0  # pilot-less data frames are left out


@pytest.mark.parametrize("n_sym, headers, want", [
    (1400, CHAIN, 7),                                                                # the chain, against single headers elsewhere
    (1400, {**CHAIN, 100: 20}, 7),                                                   # a lone header in front of nothing
    (1400, {k: v for k, v in CHAIN.items() if k != 7}, 187),
    (1400, {7: 10, 187: 20, 50: 50, 140: 50}, 7),                                    # ties: 7 -> 187 and 50 -> 140, two headers each
    (1400, {300: 10, 480: 10, 30: 20, 390: 20}, 30),                                 # ties again, the later chain first in the dict
    (700, {7: 10, 187: 20, 547: 10}, 7),                                             # 187's frame whole, 547's cut off at 700: its header counts
    (500, {7: 10, 187: 20}, 7),                                                      # one frame and the header of a cut-off one
    (500, {7: 10}, None),                                                            # a single header
    (500, {}, None),
    (1400, {400: 10, 580: 10}, None),                                                # a chain, but behind max(LEN) = 360: no offset below that leads into it
])
def test_find_vcm_start(P, n_sym, headers, want):
    scan = scan_of(n_sym, headers)
    assert W.best_start(*scan, LEN, Q_MIN) == want
    assert P.find_vcm_start(*scan, LEN, Q_MIN) == want


def test_find_vcm_start_on_random_chains(P):
    rng = np.random.default_rng(5)
    for _ in range(20):
        headers = {int(k): (int(rng.choice([10, 20, 30, 40, 50, NOISE])), float(rng.choice([9.0, 6.0]))) for k in rng.integers(0, 60, 25) * 18 + rng.integers(0, 3)}
        scan = scan_of(1200, headers)
        assert P.find_vcm_start(*scan, LEN, Q_MIN) == W.best_start(*scan, LEN, Q_MIN)


def _tx_args(*extra):
    from dvbs2_amd import tx
    return tx.build_parser().parse_args(["--rad-tx-file-path", "/dev/null", "--n-frames", "4"] + list(extra))


def _rx_args(*extra):
    from dvbs2_amd import rx
    return rx.build_parser().parse_args(["--rad-rx-file-path", "/dev/null", "--rad-rx-no-loop", "--src-type", "NONE"] + list(extra))


@pytest.mark.parametrize("extra, text", [
    (["--mod-cod-seq", "QPSK-S_8/9"], "NAME:COUNT"),
    (["--mod-cod-seq", "QPSK-S_8/9:0"], "at least 1"),
    (["--mod-cod-seq", "QPSK-S_8/9:two"], "NAME:COUNT"),
    (["--mod-cod-seq", "QAM-1/2:2"], "not supported"),
    (["--mod-cod-seq", ""], "NAME:COUNT"),
    (["--mod-cod-seq", "QPSK-S_8/9:1", "--src-type", "TS", "--src-path", "x"], "--src-type"),
    (["--mod-cod-seq", "QPSK-S_8/9:1", "--src-type", "USER", "--src-path", "x"], "--src-type"),
    (["--mod-cod-seq", "QPSK-S_8/9:1", "--tx-tasks"], "--tx-tasks"),
])
def test_mod_cod_seq_argument_errors(extra, text):
    from dvbs2_amd import tx
    with pytest.raises(ValueError, match=text):
        tx.run(_tx_args(*extra))


def test_mod_cod_seq_is_parsed():
    from dvbs2_amd.vcm import parse_schedule
    assert parse_schedule("QPSK-S_3/5:3,16APSK-S_8/9:2") == [("QPSK-S_3/5", 3), ("16APSK-S_8/9", 2)]


@pytest.mark.parametrize("extra, text", [
    (["--wl-phases", "--stm-type", "FAST"], "--wl-phases"),
    (["--sync-fine"], "--sync-fine"),
    (["--snk-type", "TS"], "--snk-type TS"),
    (["--pls-check"], "--pls-check"),
])
def test_mod_cod_vcm_argument_errors(extra, text):
    from dvbs2_amd import rx
    with pytest.raises(ValueError, match=text):
        rx.run(_rx_args("--mod-cod", "VCM", *extra))


def test_mod_cod_vcm_excludes_a_pattern_source():
    from dvbs2_amd import rx
    args = rx.build_parser().parse_args(["--rad-rx-file-path", "/dev/null", "--rad-rx-no-loop", "--mod-cod", "VCM", "--src-type", "USER", "--src-path", "x"])
    with pytest.raises(ValueError, match="--src-type USER"):
        rx.run(args)
