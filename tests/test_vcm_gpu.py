"""dvbs2_amd.vcm: a stream whose MODCOD changes from frame to frame, from VcmTransmitter through VcmReceiver, noise-free at one sample per symbol.

21 frames of the schedule QPSK-S_8/9:2, 16APSK-S_8/9:1, 32APSK-S_3/4:3, 8PSK-S_3/5:1 go into VcmReceiver(max_frames=2, NMS, 10 iterations) in three unequal pieces -- one
cut inside a frame's payload, one inside a PLHEADER -- and every frame has to come out once, in order, with the sent bits and both flags up.  The same with a dummy frame
spliced in (stepped over and counted), and with one header overwritten: one loss of lock, and only the frames between that header and the chain the twin's acquisition
finds from there are missing -- the one frame whose header it was."""
import numpy as np
import pytest

import pls_walk_ref as W

pytestmark = pytest.mark.gpu

SCHEDULE = [("QPSK-S_8/9", 2), ("16APSK-S_8/9", 1), ("32APSK-S_3/4", 3), ("8PSK-S_3/5", 1)]
FRAMES = 21


@pytest.fixture(scope="module")
def sent(P):
    """dict(frames: [(name, bits)], x float32 not to be written to, off: every frame's first symbol and the stream's end)"""
    from dvbs2_amd.vcm import VcmTransmitter
    tx = VcmTransmitter(SCHEDULE, seed=3)
    frames, x = tx.frames(FRAMES)
    tx.close()
    off = np.concatenate([[0], np.cumsum([P.get_modcod(n).pl_frame for n, _ in frames])]).tolist()
    assert [n for n, _ in frames[:8]] == ["QPSK-S_8/9"] * 2 + ["16APSK-S_8/9"] + ["32APSK-S_3/4"] * 3 + ["8PSK-S_3/5", "QPSK-S_8/9"] and off[-1] == x.size // 2
    x.setflags(write=False)
    return dict(frames=frames, x=x, off=off)


@pytest.fixture(scope="module")
def receiver():
    from dvbs2_amd.vcm import VcmReceiver
    r = VcmReceiver(max_frames=2, n_ite=10, implem="NMS")
    yield r
    r.close()


def push_in_pieces(receiver, x, cuts):
    receiver.reset()
    out, edges = [], [0] + [2 * c for c in cuts] + [x.size]
    for a, b in zip(edges, edges[1:]):
        out += receiver.push(x[a:b])
    return out


def check(P, got, frames, off):
    """got: the receiver's frames; frames, off: what was sent and where"""
    assert [g[0] for g in got] == list(off), "every frame once, in order"
    for g, (name, bits), o in zip(got, frames, off):
        assert g[1] == P.pls_value(P.get_modcod(name)) and g[2] == name
        assert np.array_equal(g[3], bits), (name, o)
        assert g[4] == 1 and g[5] == 1, (name, o)


def test_every_frame_comes_out_once_in_order_with_the_sent_bits(P, sent, receiver):
    off = sent["off"]
    cuts = [off[5] + 1000, off[13] + 40]                                             # inside frame 6's payload; 40 symbols into frame 14's header
    got = push_in_pieces(receiver, sent["x"], cuts)
    check(P, got, sent["frames"], off[:-1])
    assert receiver.stats == dict(frames={"QPSK-S_8/9": 6, "16APSK-S_8/9": 3, "32APSK-S_3/4": 9, "8PSK-S_3/5": 3}, skipped=0, losses=0, ldpc_down=0, bch_down=0)
    assert receiver.locked and receiver.tail.size == 0 and receiver.pos == off[-1]
    assert sorted(receiver.h) == sorted(n for n, _ in SCHEDULE)                      # one handle per MODCOD met, the base handle among them
    assert all(h.stream == receiver.base.stream for h in receiver.h.values())


def test_a_dummy_frame_is_stepped_over_and_counted(P, sent, receiver):
    off, x = sent["off"], sent["x"]
    at = off[9]
    y = np.concatenate([x[:2 * at], W.dummy(np.random.default_rng(4)), x[2 * at:]])
    where = [o if o < at else o + 3330 for o in off[:-1]]
    got = push_in_pieces(receiver, y, [off[5] + 1000, at + 50])                      # the second cut inside the dummy frame's header
    check(P, got, sent["frames"], where)
    assert receiver.stats["skipped"] == 1 and receiver.stats["losses"] == 0 and sum(receiver.stats["frames"].values()) == FRAMES


def test_an_overwritten_header_costs_one_loss_of_lock_and_one_frame(P, sent, receiver):
    from dvbs2_amd.vcm import ACQ_SYMBOLS
    off, x = sent["off"], sent["x"]
    j = 10
    y = x.copy()
    y[2 * off[j]:2 * (off[j] + 90)] = (np.random.default_rng(5).standard_normal(180) * np.sqrt(0.5)).astype(np.float32)
    # the twin: the walk is LOST at that header, and acquisition from there finds the chain with the most headers in its window
    scan = receiver.base.pls_scan(y[2 * off[j]:2 * (off[j] + ACQ_SYMBOLS)])
    resume = off[j] + W.best_start(*scan, P.VCM_FRAME_SYMBOLS, P.PLS_SEARCH_Q_MIN)
    lost = [f for f, o in enumerate(off[:-1]) if off[j] <= o < resume]
    assert lost == [j]                                                               # the next good header is the next frame's: one frame
    got = push_in_pieces(receiver, y, [])
    keep = [f for f in range(FRAMES) if f not in lost]
    check(P, got, [sent["frames"][f] for f in keep], [off[f] for f in keep])
    assert receiver.stats["losses"] == 1 and receiver.stats["skipped"] == 0 and sum(receiver.stats["frames"].values()) == FRAMES - 1
    assert receiver.locked
