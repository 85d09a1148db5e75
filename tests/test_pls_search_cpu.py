"""The PLHEADER search without a GPU: the chain rule of include/dvbs2hip.h on hand-made arrays, the library's length table, the float64 twin (tests/pls_search_ref.py) on
frames of the oracle's transmitter at each short-frame MODCOD's lowest operating point, find_modcod's threshold on buffers without a header, and the rx parser."""
import io

import numpy as np
import pytest

import pls_search_ref as R


def table(**lengths):
    """LEN with the entries given as v23=100"""
    LEN = np.zeros(256, np.int32)
    for k, L in lengths.items():
        LEN[int(k[1:])] = L
    return LEN


def arrays(K, q=0.0, value=0):
    """K offsets that all decode to `value` with quality q (MET^2 = 90 q, ENE = 1)"""
    return np.full(K, value, np.int32), np.full(K, np.sqrt(90.0 * q), np.float32), np.ones(K, np.float32)


def put(PLS, MET, k, value, q):
    PLS[k], MET[k] = value, np.float32(np.sqrt(90.0 * q))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chain_rule_on_hand_made_arrays(dtype):
    LEN = table(v23=100, v43=150)
    # one chain of three headers 100 apart among offsets that are no candidates (value 0, LEN 0)
    PLS, MET, ENE = arrays(350)
    for k in (20, 120, 220, 320):
        put(PLS, MET, k, 23, 0.5)
    res, score = R.chain(PLS, MET, ENE, LEN, dtype)
    assert res.tolist() == [20, 23, 4, 4] and abs(float(score) - 2.0) < 1e-5 and score.dtype == dtype
    # a slot whose value differs adds 0 and is not counted, but it is a slot
    put(PLS, MET, 120, 43, 0.9)
    res, score = R.chain(PLS, MET, ENE, LEN, dtype)
    assert res.tolist() == [20, 23, 3, 4] and abs(float(score) - 1.5) < 1e-5
    # ... and starts a chain of its own frame length: 120, 270 -- 270 holds value 0, so COUNT = 1 and 0.9 loses to 1.5
    assert R.chain(PLS, MET, ENE, table(v43=150), dtype)[0].tolist() == [120, 43, 1, 2]


def test_the_tie_between_two_starts_goes_to_the_smaller_offset():
    PLS, MET, ENE = arrays(300)
    for k in (70, 170, 30, 130):                                                     # two chains of the same two qualities, the later one written first
        put(PLS, MET, k, 23, 0.25)
    res, score = R.chain(PLS, MET, ENE, table(v23=100))
    q = R.quality(MET[[30]], ENE[[30]])[0]
    assert res.tolist() == [30, 23, 2, 3] and score == np.float32(np.float32(q + q) + np.float32(0)) and abs(score - 0.5) < 1e-6
    put(PLS, MET, 170, 23, 0.2500001)                                                # one ulp and more on the other side
    assert R.chain(PLS, MET, ENE, table(v23=100))[0].tolist() == [70, 23, 2, 3]


def test_a_start_at_L_minus_1_and_none_at_L():
    PLS, MET, ENE = arrays(400)
    put(PLS, MET, 99, 23, 0.3); put(PLS, MET, 199, 23, 0.3)
    assert R.chain(PLS, MET, ENE, table(v23=100))[0].tolist() == [99, 23, 2, 4]      # slots 99, 199, 299, 399
    PLS, MET, ENE = arrays(400)
    put(PLS, MET, 100, 23, 0.3); put(PLS, MET, 200, 23, 0.3)
    res, score = R.chain(PLS, MET, ENE, table(v23=100))                              # k = L is not a start: the header at 100 belongs to a chain that would start at 0
    assert res.tolist() == [-1, 0, 0, 0] and score == 0


def test_no_start_and_len_entries_below_90():
    PLS, MET, ENE = arrays(500, q=0.5, value=23)
    assert R.chain(PLS, MET, ENE, np.zeros(256, np.int32))[0].tolist() == [-1, 0, 0, 0]
    for L in (1, 89, -5):
        assert R.chain(PLS, MET, ENE, table(v23=L))[0].tolist() == [-1, 0, 0, 0], L
    res, score = R.chain(PLS, MET, ENE, table(v23=90))                               # 90 is a length: slots 0, 90, .., 450
    want = np.float32(0)
    for _ in range(6):
        want = np.float32(want + R.quality(MET[[0]], ENE[[0]])[0])                   # the sum is serial from 0
    assert res.tolist() == [0, 23, 6, 6] and score == want and abs(score - 3.0) < 1e-5
    # an energy of zero gives q = 0, not a division
    ENE[:] = 0
    res, score = R.chain(PLS, MET, ENE, table(v23=90))
    assert res.tolist() == [0, 23, 6, 6] and score == 0


def test_pls_frame_symbols_is_the_tables_frame_lengths_pilots_on(P):
    want = np.zeros(256, np.int32)
    for mc in P.MODCODS.values():
        assert P.pls_frame_symbols(P.pls_value(mc, True)) == mc.pl_frame
        assert P.pls_frame_symbols(P.pls_value(mc, False)) == 0                      # the library builds no frame without pilots
        want[P.pls_value(mc, True)] = mc.pl_frame
    assert np.array_equal(P.PLS_FRAME_SYMBOLS, want) and P.PLS_FRAME_SYMBOLS.dtype == np.int32 and (want > 0).sum() == len(P.MODCODS) == 9
    assert sorted(set(want[want > 0].tolist())) == [3402, 4212, 5598, 8370, 16686, 22230, 33282]      # the library's own lengths (8PSK-N: its 15 pilot blocks)
    for bad in (-1, 256, 1 << 20):
        assert P.pls_frame_symbols(bad) == 0
    from dvbs2_amd import lib_binding as B
    L = B.load()
    assert [L.dvbs2hip_pls_frame_symbols(v) for v in range(-1, 258)] == [0] + want.tolist() + [0, 0]


def test_binding_lists_the_five_entries():
    from dvbs2_amd import lib_binding as B
    from dvbs2_amd.receiver import Dvbs2Hip
    for name in ("pls_scan", "pls_scan_dev", "pls_search", "pls_search_dev"):
        assert "dvbs2hip_" + name in B.ABI and callable(getattr(Dvbs2Hip, name))
    assert "dvbs2hip_pls_frame_symbols" in B.ABI


@pytest.mark.parametrize("modcod", R.SHORT)
def test_the_float64_twin_finds_offset_and_value_at_the_lowest_operating_point(O, P, modcod):
    b = R.short_frame_buffer(O, P, modcod)
    n = b["mc"].pl_frame
    assert len(b["x"]) // 2 <= 3 * n and 0 < b["offset"] < n
    res, score = b["res"], b["score"]
    print("%s at %.2f dB: RES %s, SCORE %.4f, per slot %.4f" % (modcod, b["esn0"], res.tolist(), score, score / res[3]))
    assert res.tolist() == [b["offset"], b["value"], 2, 2]
    found = P.find_modcod(res, score)
    assert found is not None and found[0].name == modcod and found[1] is True and found[2] == b["offset"]
    # the two true headers decode to the value sent, and no other offset comes near them
    PLS, MET, ENE = b["scan"]
    q = R.quality(MET, ENE, np.float64)
    true = [b["offset"], b["offset"] + n]
    assert (PLS[true] == b["value"]).all()
    rest = np.delete(q, true)
    assert q[true].min() > 1.5 * rest.max()


def test_find_modcod_rejects_20_noise_only_seeds_with_the_measured_q_min(P):
    assert 0.05 < P.PLS_SEARCH_Q_MIN < 0.6
    worst = 0.0
    for seed in range(20):
        x = R.header_free_buffer(np.random.default_rng([7, seed]), 2 * 3402 + 90, "noise")
        res, score = R.search64(x, P.PLS_FRAME_SYMBOLS)
        worst = max(worst, float(score) / max(1, int(res[3])))
        assert P.find_modcod(res, score) is None, (seed, res.tolist(), float(score))
    print("largest per-slot score of 20 noise-only buffers: %.4f, q_min %.4f" % (worst, P.PLS_SEARCH_Q_MIN))


def test_find_modcod_asks_for_two_headers_the_threshold_and_a_modcod_of_the_table(P):
    v = P.pls_value(P.get_modcod("QPSK-S_3/5"))
    q = P.PLS_SEARCH_Q_MIN
    assert P.find_modcod([5, v, 2, 2], 2 * q + 1e-3)[0].name == "QPSK-S_3/5" and P.find_modcod([5, v, 2, 2], 2 * q + 1e-3)[1:] == (True, 5)
    assert P.find_modcod([5, v, 2, 2], 2 * q - 1e-3) is None                         # SCORE < q_min SLOTS
    assert P.find_modcod([5, v, 1, 2], 2.0) is None                                  # a single header
    assert P.find_modcod([-1, 0, 0, 0], 0.0) is None
    assert P.find_modcod([5, 128 + v, 3, 3], 3.0) is None                            # no MODCOD of the table (a caller's LEN may name one)
    assert P.find_modcod([5, v, 2, 8], 1.0, q_min=0.1) is not None and P.find_modcod([5, v, 2, 8], 1.0, q_min=0.2) is None
    assert P.find_modcod([5, v, 2, 2], float("nan")) is None


def test_rx_parser_takes_auto_and_auto_excludes_the_learning_phases(tmp_path):
    from dvbs2_amd import rx
    iq = str(tmp_path / "in.bin")
    np.zeros(16, np.float32).tofile(iq)
    ap = rx.build_parser()
    assert ap.parse_args(["--rad-rx-file-path", iq, "--mod-cod", "AUTO"]).mod_cod == "AUTO"
    args = ap.parse_args(["--rad-rx-file-path", iq, "--rad-rx-no-loop", "--mod-cod", "AUTO", "--wl-phases", "--stm-type", "FAST"])
    with pytest.raises(ValueError, match="AUTO.*--wl-phases|--wl-phases.*AUTO"):
        rx.run(args, out=io.StringIO())
