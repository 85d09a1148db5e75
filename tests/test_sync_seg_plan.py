"""How the frame synchronizer cuts a call's frames into segments for the average over frames (CPU; `plan_probe syncseg` links the library's host code and prints what
sync_segment_plan -- the function sync_choose of dvbs2_amd/csrc/rx_dispatch.h calls, with the cap DVBS2HIP_SYNC_SEGMENTS gives at that call -- answers): the nine MODCODs' PL frame lengths, call lengths on both sides of every threshold,
every cap.  tests/test_sync_seg_gpu.py asks the same probe whether its cases are cut at all."""
import subprocess

import pytest

from test_plan_digest import build_probe

PL_FRAMES = (3402, 4212, 5598, 8370, 16686, 22230, 33282)      # 32APSK-S, 16APSK-S, 8PSK-S, QPSK-S, 32APSK-N / 16APSK-N, 8PSK-N, QPSK-N
FRAMES = (1, 767, 768, 1535, 1536, 1537, 2303, 2304, 2400, 3071, 3072, 4096, 8192)
CAPS = tuple(range(1, 9))
MAX_SEG, MAX_WG, MIN_SEG_F, SUB = 8, 256, 768, 64


def segment_plans(exe, triples):
    """[(n, F, cap)] -> [(nseg, seg_F)] as the library's sync_segment_plan gives them"""
    args = [str(v) for t in triples for v in t]
    out = subprocess.run([exe, "syncseg"] + args, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * len(triples)
    return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(len(triples))]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sync_seg_plan") / "plan_probe")
    build_probe(exe)
    return exe


def test_the_pl_frame_lengths_are_the_modcods(P):
    assert sorted({P.get_modcod(m).pl_frame for m in P.MODCODS}) == sorted(PL_FRAMES)


def test_segments_of_every_frame_length_call_length_and_cap(probe):
    triples = [(n, F, cap) for n in PL_FRAMES for F in FRAMES for cap in CAPS]
    largest = {}
    for (n, F, cap), (nseg, seg_F) in zip(triples, segment_plans(probe, triples)):
        nwg = -(-n // 64)
        case = (n, F, cap, nseg, seg_F)
        assert (nseg == 1) == (min(cap, MAX_SEG, MAX_WG // nwg, F // MIN_SEG_F) <= 1), case
        if nseg > 1:
            assert seg_F % 192 == 0 and (nseg - 1) * seg_F < F <= nseg * seg_F and nwg * nseg <= MAX_WG, case
            assert (nseg - 1) * (seg_F // SUB) <= -(-F // SUB), case              # the {A, B} scratch the handle allocated for max_frames >= F
        else:
            assert seg_F == F, case
        if cap == 1:
            assert nseg == 1, case
        largest[n] = max(largest.get(n, 1), nseg)
    assert largest == {3402: 4, 4212: 3, 5598: 2, 8370: 1, 16686: 1, 22230: 1, 33282: 1}
