"""The BBFRAME layer on the GPU against its twin (tests/bbframe_ref.py), every comparison exact: bbframe_build bit for bit whatever the call sizes and the last frame's
length; bbframe_parse's packets, statuses, headers and counters on clean frames and on frames damaged on the host, in the host and the device form and across call
borders; the parser recorded in a graph; and the whole way, bbframe_build -> tx_bb -> rx_bb_up, against the sent stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bbframe_ref as BR                                                              # noqa: E402

pytestmark = pytest.mark.gpu

K35, D35 = 9552, 1184                                                                 # QPSK-S_3/5: 47 frames are 296 packets


@pytest.fixture(scope="module")
def h35():
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip("QPSK-S_3/5", max_frames=48, n_ite=10, implem="NMS")
    yield rx
    rx.close()


@pytest.fixture(scope="module")
def h89():
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=8, n_ite=10, implem="NMS")
    yield rx
    rx.close()


@pytest.fixture(scope="module")
def ref35():
    """50 frames of QPSK-S_3/5 from reset: (stream, twin's bits)"""
    stream = BR.ts_stream(50 * D35 // 188 + 1, seed=35)[:50 * D35]
    return stream, BR.build(stream, K35, BR.tx_state())[0]


def stats_list(rx):
    s = rx.bbframe_stats()
    return [s[k] for k in ("frames_taken", "frames_dropped", "packets_ok", "packets_bad", "bytes_discarded")]


def parse_dev(rx, bits, valid=None):
    import torch
    F = len(bits)
    cap = rx.bbframe_max_packets(F)
    uplb = getattr(rx, "uplb", 188)
    V = torch.from_numpy(np.ascontiguousarray(bits, np.int32)).cuda()
    va = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.int8)).cuda()
    UP, ST = torch.zeros(cap * uplb, dtype=torch.uint8, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    N, HDR = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros((F, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rx.bbframe_parse_dev(V.data_ptr(), None if va is None else va.data_ptr(), UP.data_ptr(), ST.data_ptr(), N.data_ptr(), HDR.data_ptr(), F)
    rx.synchronize()
    n = int(N.item())
    assert n <= cap
    return UP.cpu().numpy().reshape(cap, uplb)[:n], ST.cpu().numpy()[:n], HDR.cpu().numpy()


def same(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ------------------------------------------------------------------ build
def test_build_is_the_twin_over_all_phases(h35, ref35):
    stream, want = ref35
    h35.bbframe_reset()
    got = h35.bbframe_build(stream[:48 * D35], 48)
    assert got.dtype == np.int32 and np.array_equal(got, want[:48])
    syncd = np.packbits(got[:, 56:72].astype(np.uint8), axis=1).astype(int) @ [256, 1]
    assert len(set(syncd[:47])) == 47 and syncd[47] == 0 and syncd[46] != 65535              # all 47 phases; frame 46 ends on a packet's last byte
    nxt = h35.bbframe_build(stream[48 * D35:], 2)                                              # the state behind the call
    assert np.array_equal(nxt, want[48:])
    h35.bbframe_reset()
    parts, at = [], 0
    for n in (1, 2, 5, 40, 2):
        parts.append(h35.bbframe_build(stream[at * D35:(at + n) * D35], n)); at += n
    assert np.array_equal(np.concatenate(parts), want)


@pytest.mark.parametrize("rest", [1, 188 - D35 % 188, D35])
def test_build_short_last_frame(h35, rest):
    stream = BR.ts_stream(30, seed=rest)
    n0 = D35 + rest
    a, st = BR.build(stream[:n0], K35, BR.tx_state())
    b, _ = BR.build(stream[n0:n0 + 2 * D35], K35, st)
    h35.bbframe_reset()
    assert np.array_equal(h35.bbframe_build(stream[:n0], 2), a)
    assert np.array_equal(h35.bbframe_build(stream[n0:n0 + 2 * D35], 2), b)                    # pos and both CRC registers carried over
    hdr = np.packbits(a[1, :80].astype(np.uint8)).astype(int)
    # frame 1 starts 56 bytes into a packet: the next one starts at its byte 132, which only the full frame has
    assert hdr[4] << 8 | hdr[5] == 8 * rest and (hdr[7] << 8 | hdr[8]) == (8 * 132 if rest > 132 else 65535) and not a[1, 80 + 8 * rest:].any()


def test_build_and_parse_with_another_packet_length(h35):
    p = BR.params(upl=64, sync=0xB8)
    stream = BR.ts_stream(5 * D35 // 8 + 1, seed=64, upl=64, sync=0xB8)[:5 * D35 - 3]
    want, _ = BR.build(stream, K35, BR.tx_state(), p)
    try:
        h35.bbframe_set_params(upl_bits=64, sync=0xB8)
        assert np.array_equal(h35.bbframe_build(stream, 5), want)
        same(h35.bbframe_parse(want), BR.parse(want, None, BR.rx_state(), p)[:3])
        assert h35.bbframe_parse(want[:1])[0].shape[1] == 8
    finally:
        h35.bbframe_set_params()


def test_build_refuses_what_it_cannot_take(h35):
    from dvbs2_amd.lib_binding import Dvbs2HipError
    stream = BR.ts_stream(20)
    for n_bytes, F in ((D35, 2), (2 * D35 + 1, 2), (0, 1)):
        with pytest.raises(Dvbs2HipError) as e:
            h35.bbframe_build(stream[:n_bytes], F)
        assert e.value.code == -1
    for upl in (0, 8, 1500, K35 - 72):
        with pytest.raises(Dvbs2HipError) as e:
            h35.bbframe_set_params(upl_bits=upl)
        assert e.value.code == -4
    with pytest.raises(Dvbs2HipError, match=r"'n_frames' has to be in \[1, max_frames\]") as e:
        h35.bbframe_build(BR.ts_stream(49 * D35 // 188 + 1)[:49 * D35], 49)
    assert e.value.code == -1
    h35.bbframe_reset()
    assert np.array_equal(h35.bbframe_build(stream[:D35], 1), BR.build(stream[:D35], K35, BR.tx_state())[0])      # none of it touched the task


def test_normal_frames():
    from dvbs2_amd.receiver import Dvbs2Hip
    K = 57472
    stream = BR.ts_stream(3 * 7174 // 188 + 1, seed=3)[:2 * 7174 + 500]
    want, _ = BR.build(stream, K, BR.tx_state())
    rx = Dvbs2Hip("QPSK-N_8/9", max_frames=3, n_ite=10, implem="NMS")
    try:
        got = rx.bbframe_build(stream, 3)
        assert np.array_equal(got, want)
        ref = BR.parse(want, None, BR.rx_state())
        same(rx.bbframe_parse(got), ref[:3])
        assert stats_list(rx) == ref[3] and len(ref[0]) == (2 * 7174 + 500 - 1) // 188
    finally:
        rx.close()


# ------------------------------------------------------------------ parse, clean frames
def test_parse_is_the_twin_on_clean_frames(h35, ref35):
    stream, bits = ref35
    bits = bits[:48]
    whole = BR.parse(bits, None, BR.rx_state())
    assert np.array_equal(whole[0].ravel(), stream[:len(whole[0]) * 188]) and not whole[1].any()
    for form in (h35.bbframe_parse, lambda b: parse_dev(h35, b)):
        h35.bbframe_reset()
        same(form(bits), whole[:3])
        assert stats_list(h35) == whole[3]
    for cuts in ((1, 47), (46, 2), (47, 1)):                                                   # the pending packet crosses a call; at 47 | 1 it waits whole for its slot
        for form in (h35.bbframe_parse, lambda b: parse_dev(h35, b)):
            h35.bbframe_reset()
            st, at, pk = BR.rx_state(), 0, []
            for n in cuts:
                ref = BR.parse(bits[at:at + n], None, st)
                got = form(bits[at:at + n])
                same(got, ref[:3])
                assert stats_list(h35) == ref[3] and len(got[0]) <= h35.bbframe_max_packets(n)
                if cuts == (1, 47) and n == 47:
                    assert len(got[0]) == h35.bbframe_max_packets(47) == 296                   # the bound is reached
                if n == 46:
                    assert len(ref[4]["buf"]) == 132                                           # the border case, frame 46 then 47, inside the second call
                if cuts == (47, 1) and n == 47:
                    assert len(ref[4]["buf"]) == 188
                st, at = ref[4], at + n
                pk.append(got[0])
            assert np.array_equal(np.concatenate(pk), whole[0])


# ------------------------------------------------------------------ parse, damaged frames
def set_header(bits, f, **kw):
    """rewrites fields of frame f's BBHEADER and its CRC-8"""
    h = bytearray(np.packbits(bits[f, :72].astype(np.uint8)).tobytes())
    for k, v in kw.items():
        i = dict(upl=2, dfl=4, syncd=7)[k]
        h[i], h[i + 1] = v >> 8, v & 255
    h.append(BR.crc8(h))
    bits[f, :80] = np.unpackbits(np.frombuffer(bytes(h), np.uint8))


def flip(f, bit):
    def m(bits, valid):
        bits[f, bit] ^= 1
    return m


def hdr_bits(*frames):
    def m(bits, valid):
        for f in frames:
            bits[f, 17] ^= 1
    return m


def syncd_plus_8(bits, valid):
    set_header(bits, 2, syncd=608 + 8)


def other_upl(bits, valid):
    set_header(bits, 5, upl=1496)


def invalid(bits, valid):
    valid[4] = 0


DAMAGE = {
    "a header bit": (hdr_bits(3), lambda hdr: hdr[3, 0] == 1),
    "SYNCD + 8, CRC right": (syncd_plus_8, lambda hdr: hdr[2, 0] == 0 and hdr[2, 5] == 616),
    "another UPL, CRC right": (other_upl, lambda hdr: hdr[5, 0] == 2),
    "VALID = 0": (invalid, lambda hdr: hdr[4, 0] == 3),
    "first frame": (hdr_bits(0), lambda hdr: hdr[0, 0] == 1),
    "last frame": (hdr_bits(7), lambda hdr: hdr[7, 0] == 1),
    "two frames in a row": (hdr_bits(3, 4), lambda hdr: hdr[3, 0] == 1 and hdr[4, 0] == 1),
    "a packet body bit": (flip(1, 80 + 8 * 300 + 3), lambda hdr: not hdr[:, 0].any()),
    "a CRC slot bit": (flip(1, 80 + 1056 + 2), lambda hdr: not hdr[:, 0].any()),
}


MARKED = ("a packet body bit", "a CRC slot bit", "SYNCD + 8, CRC right")                      # the cases with a wrong packet: once more with mark_tei


@pytest.mark.parametrize("name,mark_tei", [(n, False) for n in DAMAGE] + [(n, True) for n in MARKED])
def test_parse_is_the_twin_on_damaged_frames(h35, ref35, name, mark_tei):
    damage, check = DAMAGE[name]
    bits, valid = ref35[1][:10].copy(), np.ones(10, np.int8)
    damage(bits, valid)
    p = BR.params(mark_tei=mark_tei)
    ref = BR.parse(bits[:8], valid[:8], BR.rx_state(), p)
    nxt = BR.parse(bits[8:], None, ref[4], p)                                                  # a good call behind it: what the damaged one left pending
    assert check(ref[2])
    clean = BR.parse(ref35[1][:8], None, BR.rx_state())
    if name in ("a packet body bit", "a CRC slot bit"):
        assert ref[1].sum() == 1 and len(ref[0]) == len(clean[0])
        hit = int(np.flatnonzero(ref[1])[0])
        assert not mark_tei or ref[0][hit, 1] & 0x80                                          # the transport_error_indicator of the packet that is wrong
    else:
        assert len(ref[0]) < len(clean[0]) and ref[3][4] > 0
    try:
        if mark_tei:
            h35.bbframe_set_params(mark_tei=True)
        for form in (lambda b, v: h35.bbframe_parse(b, v), lambda b, v: parse_dev(h35, b, v)):
            h35.bbframe_reset()
            same(form(bits[:8], valid[:8]), ref[:3])
            assert stats_list(h35) == ref[3]
            same(form(bits[8:], None), nxt[:3])
            assert stats_list(h35) == nxt[3]
    finally:
        if mark_tei:
            h35.bbframe_set_params()


def test_a_padding_bit_changes_nothing(h35):
    stream = BR.ts_stream(20, seed=9)[:2 * D35 + 700]
    bits, _ = BR.build(stream, K35, BR.tx_state())
    ref = BR.parse(bits, None, BR.rx_state())
    bits[2, 80 + 8 * 700 + 5] ^= 1
    assert np.array_equal(BR.parse(bits, None, BR.rx_state())[0], ref[0])
    h35.bbframe_reset()
    same(h35.bbframe_parse(bits), ref[:3])
    assert stats_list(h35) == ref[3]


# ------------------------------------------------------------------ graph
def test_parse_recorded_in_a_graph(h35, ref35):
    import torch
    F = 6
    inputs = [ref35[1][:F].copy(), ref35[1][:F].copy()]
    inputs[1][2, 17] ^= 1                                                                      # a dropped frame in the second
    cap = h35.bbframe_max_packets(F)
    V = torch.zeros((F, K35), dtype=torch.int32, device="cuda")
    UP, ST = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    N, HDR = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros((F, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def once():
        h35.bbframe_parse_dev(V.data_ptr(), None, UP.data_ptr(), ST.data_ptr(), N.data_ptr(), HDR.data_ptr(), F)

    h35.bbframe_reset()
    once()                                                                                     # allocates
    h35.synchronize()
    h35.bbframe_reset()
    gid = h35.graph_capture(once)
    h35.bbframe_reset()                                                                        # the recorded call reads the state of the moment of recording: the reset one
    try:
        for bits in inputs:
            V.copy_(torch.from_numpy(bits)); torch.cuda.synchronize()
            h35.graph_launch(gid)
            h35.synchronize()
            ref = BR.parse(bits, None, BR.rx_state())
            n = int(N.item())
            same((UP.cpu().numpy().reshape(cap, 188)[:n], ST.cpu().numpy()[:n], HDR.cpu().numpy()), ref[:3])
    finally:
        h35.graph_destroy(gid)
        h35.bbframe_reset()


# ------------------------------------------------------------------ end to end
def test_packets_through_the_chain(h89):
    from dvbs2_amd import params as P
    F, K, D = 8, 14232, 1769
    mc = P.get_modcod("QPSK-S_8/9")
    sigma = P.esn0_to_sigma(P.ebn0_to_esn0(8.0, mc.K_bch / mc.N_ldpc, mc.bps))
    stream = BR.ts_stream(F * D // 188 + 1, seed=89)[:F * D]
    h89.bbframe_reset()
    bits = h89.bbframe_build(stream, F)
    sent, pl = h89.tx_bb(F, info=bits, seed=5, sigma=sigma)
    assert np.array_equal(sent, bits)
    info, c0, c1 = h89.rx_bb(pl, sigma=sigma)
    be = int((info != bits).sum())
    assert be == 0, "bit errors at Eb/N0 = 8 dB: %d" % be
    pk, status, hdr, u0, u1 = h89.rx_bb_up(pl, sigma=sigma)
    n = (F * D - 1) // 188
    assert pk.shape == (n, 188) and np.array_equal(pk.ravel(), stream[:n * 188]) and not status.any() and not hdr[:, 0].any()
    assert np.array_equal(u0, c0) and np.array_equal(u1, c1)
    h89.bbframe_reset()
    same(h89.bbframe_parse(info), (pk, status, hdr))
