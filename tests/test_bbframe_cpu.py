"""The BBFRAME layer without a GPU: the known answers of the format pin the twin (tests/bbframe_ref.py), the twin's transmitter and receiver are inverse whatever the
call sizes, the transport-stream source and sink, the command lines' new flags, what the receiver calls on its handle with and without --snk-type TS, and the entries'
answer to a null handle."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bbframe_ref as BR                                                              # noqa: E402
import stepmf_ref as SR                                                               # noqa: E402

K_ALL = (14232, 9552, 57472, 11712)


def test_crc8_known_answers():
    assert BR.crc8(b"123456789") == 0xBC
    null = bytes([0x1F, 0xFF, 0x10]) + bytes([0xFF] * 184)
    assert len(null) == 187 and BR.crc8(null) == 0xAF
    assert BR._crc8_fast(null) == 0xAF and BR._crc8_fast(b"123456789") == 0xBC
    from dvbs2_amd.srcfile import TS_NULL
    assert bytes(TS_NULL[1:]) == null and TS_NULL[0] == 0x47 and TS_NULL.size == 188


@pytest.mark.parametrize("K,want", [(14232, "F20005E0374847 0000 E5"), (9552, "F20005E0250047 0000 2F"), (57472, "F20005E0E03047 0000 73"), (11712, "F20005E02D7047 0000 54")])
def test_header_of_a_full_frame_at_stream_start(K, want):
    assert BR.header(BR.DEFAULTS, K - 80, 0) == bytes.fromhex(want)
    bits, _ = BR.build(BR.ts_stream(40)[:(K - 80) // 8], K, BR.tx_state())
    assert bits.shape == (1, K) and np.packbits(bits[0, :80].astype(np.uint8)).tobytes() == bytes.fromhex(want)


def test_syncd_walks_through_its_period():
    K, D = 9552, 1184
    stream = BR.ts_stream(48 * D // 188 + 1, seed=1)[:48 * D]
    bits, st = BR.build(stream, K, BR.tx_state())
    hdr = np.packbits(bits[:, :80].astype(np.uint8), axis=1).astype(int)
    syncd = hdr[:, 7] << 8 | hdr[:, 8]
    assert list(syncd[:4]) == [0, 1056, 608, 160]
    assert 47 * D % 188 == 0 and syncd[47] == 0 and (syncd[1:47] != 0).all()                   # frame 46 ends on a packet's last byte
    assert (46 * D + 1183 + 1) % 188 == 0 and st["pos"] == 48 * D % 188
    # K = 14232: the period is 188 frames (D = 1769 and 188 share no factor)
    assert [f for f in range(1, 189) if f * 1769 % 188 == 0] == [188]
    # the first slot carries 0, every later one the CRC-8 of the packet before it
    data = np.packbits(bits[:, 80:].astype(np.uint8), axis=1).ravel()
    assert data[0] == 0 and data[188] == BR.crc8(stream[1:188]) and data[2 * 188] == BR.crc8(stream[189:2 * 188])
    assert np.array_equal(np.delete(data, np.arange(0, data.size, 188)), np.delete(stream, np.arange(0, stream.size, 188)))


@pytest.mark.parametrize("K", K_ALL)
@pytest.mark.parametrize("upl,sync", [(1504, 0x47), (64, 0xB8)])
def test_twin_round_trip_whatever_the_call_sizes(K, upl, sync):
    p = BR.params(upl=upl, sync=sync)
    uplb, D = upl // 8, (K - 80) // 8
    stream = BR.ts_stream(8 * D // uplb + 1, seed=K + upl, upl=upl, sync=sync)[:8 * D]
    one, st_one = BR.build(stream, K, BR.tx_state(), p)
    parts, st = [], BR.tx_state()
    for n in (1, 2, 5):
        b, st = BR.build(stream[sum(len(x) for x in parts) * D:][:n * D], K, st, p)
        parts.append(b)
    assert np.array_equal(np.concatenate(parts), one) and st == st_one
    pk, status, hdr, ctr, rst = BR.parse(one, None, BR.rx_state(), p)
    n = len(pk)
    assert n in (8 * D // uplb, 8 * D // uplb - 1) and not status.any() and not hdr[:, 0].any() and ctr == [8, 0, n, 0, 0]
    assert np.array_equal(pk.ravel(), stream[:n * uplb])                                        # everything but the pending last packet
    assert rst["have"] and len(rst["buf"]) == 8 * D - n * uplb
    got, rst2 = [], BR.rx_state()
    for a, b in ((0, 1), (1, 3), (3, 8)):
        q, s2, _, _, rst2 = BR.parse(one[a:b], None, rst2, p)
        got.append(q)
    assert np.array_equal(np.concatenate(got), pk) and rst2 == rst


def test_source_ts_and_sink_ts(tmp_path):
    from dvbs2_amd.srcfile import SinkTS, SourceDone, SourceTS
    K, D = 14232, 1769
    data = BR.ts_stream(30, seed=5)
    f_in, f_out = str(tmp_path / "in.ts"), str(tmp_path / "out.ts")
    data.tofile(f_in)
    once = SourceTS(f_in, D, auto_reset=False)
    tx, rx, snk, calls = BR.tx_state(), BR.rx_state(), SinkTS(f_out), []
    while True:
        try:
            stream, n = once.generate(2)
        except SourceDone:
            break
        calls.append((len(stream), n))
        bits = np.zeros((2, K), np.int32)
        if n:
            bits[:n], tx = BR.build(stream, K, tx)
        pk, status, hdr, _, rx = BR.parse(bits, None, rx)
        assert not status.any()
        snk.send(pk)
    snk.close()
    assert calls == [(2 * D, 2), (31 * 188 - 2 * D, 2), (0, 0)]                                # the file and one null packet, the last frame short; then the flush
    assert open(f_out, "rb").read() == data.tobytes()                                         # ... which never comes out: nothing follows it
    loop = SourceTS(f_in, D)
    a, n = loop.generate(4)
    assert n == 4 and np.array_equal(a, np.tile(data, 2)[:4 * D]) and np.array_equal(loop.generate(1)[0], np.tile(data, 2)[4 * D:5 * D])
    data[:-3].tofile(f_in)
    with pytest.raises(ValueError, match="offset %d" % (29 * 188)):
        SourceTS(f_in, D)
    bad = data.copy(); bad[7 * 188] = 0x48; bad[9 * 188] = 0
    bad.tofile(f_in)
    with pytest.raises(ValueError, match="offset %d" % (7 * 188)):
        SourceTS(f_in, D)


def test_the_parsers_take_the_new_flags():
    from dvbs2_amd import rx, tx
    a = tx.build_parser().parse_args(["--rad-tx-file-path", "x", "--src-type", "TS", "--src-path", "v.ts", "--src-no-loop"])
    assert a.src_type == "TS" and a.src_no_loop
    assert rx.build_parser().parse_args(["--rad-rx-file-path", "x"]).snk_type == "BITS"
    assert rx.build_parser().parse_args(["--rad-rx-file-path", "x", "--snk-type", "TS"]).snk_type == "TS"
    with pytest.raises(SystemExit):
        rx.build_parser().parse_args(["--rad-rx-file-path", "x", "--snk-type", "PES"])


class Spy(SR.RecordingHandle):
    """the recording handle of tests/test_rx_sequence.py with the two calls that hand out packets"""
    made = None

    def _out(self, s, F):
        return np.tile(BR.ts_stream(1), (3, 1)), np.zeros(3, np.uint8), np.zeros((F, 8), np.int32)

    def rx_bb_up(self, pl_frames, sigma=None):
        F = np.asarray(pl_frames).reshape(-1, 2 * self.n).shape[0]
        return self._out(self._rec("rx_bb_up", [sigma], pl_frames), F) + (np.ones(F, np.int8), np.ones(F, np.int8))

    def bbframe_parse(self, bits, valid=None):
        return self._out(self._rec("bbframe_parse", [valid], bits), len(bits))


PACKET_CALLS = ("rx_bb_up", "bbframe_parse", "bbframe_build", "bbframe_set_params", "bbframe_reset", "bbframe_stats", "bbframe_max_packets")


@pytest.mark.parametrize("extra", [[], ["--sync-fine"], ["--stm-type", "FAST"]])
def test_rx_hands_out_packets_only_when_asked(extra, tmp_path, monkeypatch):
    from dvbs2_amd import receiver, rx
    F, N = 2, 8370
    iq = str(tmp_path / "in.bin")
    SR.RecordingHandle._fill(11, (5 * F, 4 * N)).tofile(iq)
    logs, printed, sinks = [], [], []
    for flag in ([], ["--snk-type", "TS"]):
        H = type("S", (Spy,), dict(made=[], not_ready=(1,)))
        monkeypatch.setattr(receiver, "Dvbs2Hip", H)
        snk = str(tmp_path / ("snk%d" % len(logs)))
        args = rx.build_parser().parse_args(["--rad-rx-file-path", iq, "--rad-rx-no-loop", "-F", str(F), "--src-type", "NONE", "--snk-path", snk] + extra + flag)
        out = io.StringIO()
        rx.run(args, out=out)
        assert len(H.made) == 1
        logs.append(H.made[0].log); printed.append(out.getvalue().strip()); sinks.append(open(snk, "rb").read())
    plain, ts = logs
    assert not [e for e in plain if e[0] in PACKET_CALLS or e[0].startswith("bbframe_")]
    batches = [e[0] for e in plain].count("sync_frame_synchronize")
    assert batches >= 3 and [e[0] for e in ts if e[0] in PACKET_CALLS or e[0].startswith("bbframe_")] == [("bbframe_parse" if "--sync-fine" in extra else "rx_bb_up")] * batches
    if "--sync-fine" in extra:                                                                 # the parser behind the BB descrambler, nothing else moves
        assert [e for e in ts if e[0] != "bbframe_parse"] == plain
        assert all(ts[i - 1][0] == "bb_descramble" for i, e in enumerate(ts) if e[0] == "bbframe_parse")
    else:                                                                                      # the fused call in the fused call's place, same arguments
        assert [["rx_bb"] + e[1:] if e[0] == "rx_bb_up" else e for e in ts] == plain
    assert "BBFRAME" not in printed[0] and printed[1] == printed[0] + " | BBFRAMEs dropped 0 | packets %d | CRC-8 errors 0" % (3 * batches)
    assert sinks[1] == BR.ts_stream(1).tobytes() * (3 * batches) and len(sinks[0]) > 0 and len(sinks[0]) % (14232 // 8) == 0


def test_a_pattern_cannot_be_counted_against_packets(tmp_path):
    from dvbs2_amd import rx
    from dvbs2_amd.srcfile import save_src
    src = str(tmp_path / "p.src")
    save_src(src, np.zeros((1, 14232), np.int32))
    with pytest.raises(ValueError, match="--snk-type TS"):
        rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", src, "--rad-rx-no-loop", "--src-type", "USER", "--src-path", src, "--snk-type", "TS"]), out=io.StringIO())


def test_a_null_handle_is_an_invalid_argument():
    from dvbs2_amd import lib_binding as B
    L = B.load()
    n32, buf = ctypes.c_int32(), (ctypes.c_uint8 * 64)()
    assert L.dvbs2hip_bbframe_set_params(None, 0xF2, 0, 1504, 0x47, 0) == -1
    assert L.dvbs2hip_bbframe_reset(None) == -1
    assert L.dvbs2hip_bbframe_get_stats(None, buf) == -1
    assert L.dvbs2hip_bbframe_max_packets(None, 1, ctypes.byref(n32)) == -1
    for fn in (L.dvbs2hip_bbframe_build, L.dvbs2hip_bbframe_build_dev):
        assert fn(None, buf, 1, buf, 1) == -1
    for fn in (L.dvbs2hip_bbframe_parse, L.dvbs2hip_bbframe_parse_dev):
        assert fn(None, buf, None, buf, buf, buf, None, 1) == -1
    for fn in (L.dvbs2hip_rx_bb_up, L.dvbs2hip_rx_bb_up_dev):
        assert fn(None, buf, None, buf, buf, buf, None, None, None, 1) == -1
