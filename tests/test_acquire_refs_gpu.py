"""The coarse-frequency loop and the learning phases in the reference's full chain, against the reference's own traces with a carrier offset
(refs/TX_RX/QPSK_8_9_freq_005_delay_{40,45}.txt in tests/golden/refs_tx_rx.json, run with --chn-max-freq-shift 0.05): tools/sync_in_loop.py --wl-phases
--chn-max-freq-shift 0.05 --stm-type FAST at 3.8 dB, to at least 100 frame errors or the frame cap tests/test_timing_refs_gpu.py uses.  FER <= 2.5 x the trace's row (the
reference CI's band); at D = 4.0 it may not be below the genie-timed loop's by more than 4 sigma of the counting error.  No lower bound against the trace is fixed: the
ratio is recorded in results/coarse/trace_comparison.json."""
import json
import math
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def point(D, wl, max_frames=60000, fe=100):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sync_in_loop as S
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    # wl: the phases take the first 3 calls of 256 frames and more (waiting, learning 1, 2, 3: one call each at F = 256) and nothing of them is counted; the frames of
    # the first transmission call, in which the frame synchronizer's delay line settles, are skipped as in the timing test
    a = types.SimpleNamespace(F=256, off=1234, phase=0.0, freq=0.0, seed=7, fe=fe, max_frames=max_frames, skip=256 if wl else 32, est_perfect=False, agc=True,
                              chn_max_delay=D, stm_type="FAST" if wl else "PERFECT", chn_max_freq_shift=0.05 if wl else None, wl_phases=wl)
    r = S.run_point(Dvbs2Hip, P, P.get_modcod("QPSK-S_8/9"), 3.8, "fine" if wl else "frame", a)
    out = os.environ.get("DVBS2_ACQUIRE_REFS_JSON")
    if out:
        rows = json.load(open(out)) if os.path.exists(out) else []
        rows.append(dict(D=D, wl=wl, fer=r["fer"], fe=r["fe"], counted=r["counted"], acquisition=r.get("acquisition"), seconds=r["seconds"]))
        json.dump(rows, open(out, "w"), indent=1)
    return r


@pytest.fixture(scope="module")
def genie():
    return point(None, False)


def trace_row(trace, ebn0):
    return [r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "refs_tx_rx.json")))[trace]["rows"] if round(r["ebn0"], 2) == ebn0][0]


def test_acquired_loop_at_delay_40_against_the_genie_and_the_trace(genie):
    row = trace_row("QPSK_8_9_freq_005_delay_40.txt", 3.8)
    r = point(4.0, True)
    print("D 4.00: FER %.4e (FE %d / %d), genie %.4e (FE %d / %d), trace %.4e, FER / trace %.3f, acquisition %r" % (
        r["fer"], r["fe"], r["counted"], genie["fer"], genie["fe"], genie["counted"], row["fer"], r["fer"] / row["fer"], r["acquisition"]))
    assert r["fe"] >= 100 or r["counted"] >= 60000
    assert genie["fe"] >= 100
    sig = math.sqrt(1.0 / max(r["fe"], 1) + 1.0 / genie["fe"])
    assert math.log(max(r["fer"], 1e-12) / genie["fer"]) > -4.0 * sig, (r, genie)
    assert r["fer"] <= 2.5 * row["fer"], (r, row)


def test_acquired_loop_at_delay_45_against_the_trace():
    row = trace_row("QPSK_8_9_freq_005_delay_45.txt", 3.8)
    r = point(4.5, True, max_frames=20480)
    print("D 4.50: FER %.4e (FE %d / %d), trace %.4e, FER / trace %.3f, acquisition %r" % (r["fer"], r["fe"], r["counted"], row["fer"], r["fer"] / row["fer"], r["acquisition"]))
    assert r["fe"] >= 100 or r["counted"] >= 20480
    assert r["fer"] <= 2.5 * row["fer"], (r, row)
