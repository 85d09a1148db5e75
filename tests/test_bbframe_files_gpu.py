"""A transport stream through the files (made as tests/test_tx_ch_rx_files_gpu.py makes them): `dvbs2_tx --src-type TS --src-no-loop` -> `dvbs2_ch` -> `dvbs2_rx --snk-type TS`
returns the stream's packets -- none before the lock, none wrong, and the file's last packet is the last one out; with the default sink the receiver does what it did."""
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bbframe_ref as BR                                                              # noqa: E402

MODCOD, K = "QPSK-S_8/9", 14232


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """600 random transport packets, sent once at 8 dB -> (the packets, noisy IQ file, directory)"""
    from dvbs2_amd import ch, tx
    d = tmp_path_factory.mktemp("bbframe")
    f_in, f_tx, f_noisy = (str(d / n) for n in ("video.ts", "out_tx.bin", "out_tx_noisy.bin"))
    data = BR.ts_stream(600, seed=600)
    data.tofile(f_in)
    log = io.StringIO()
    n = tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "TS", "--src-path", f_in, "--src-no-loop", "--mod-cod", MODCOD]), out=log)
    assert n == 72                                                                             # 601 packets are 63.9 data fields: 8 calls, and the call that flushes
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", MODCOD, "-m", "8.0"]), out=log) == n
    return data.reshape(600, 188), f_noisy, d


def rx_run(f_noisy, snk, extra):
    from dvbs2_amd import rx
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(["--src-type", "NONE", "--rad-rx-file-path", f_noisy, "-F", "8", "--mod-cod", MODCOD, "--dec-implem", "NMS", "--dec-ite", "10",
                                              "--snk-path", snk, "--rad-rx-no-loop"] + extra), out=log)
    return st, log.getvalue()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--sync-fine"]])
def test_the_transport_stream_comes_back(files, extra):
    sent, f_noisy, d = files
    f_snk = str(d / ("output%d.ts" % len(extra)))
    st, printed = rx_run(f_noisy, f_snk, ["--snk-type", "TS"] + extra)
    out = np.fromfile(f_snk, dtype=np.uint8)
    assert out.size > 0 and out.size % 188 == 0, printed
    out = out.reshape(-1, 188)
    n = len(out)
    assert n >= 400 and np.array_equal(out, sent[600 - n:]), printed                           # a contiguous run that ends with the file's last packet; the null packet stays inside
    m = re.search(r"\| BBFRAMEs dropped (\d+) \| packets (\d+) \| CRC-8 errors (\d+)$", printed.strip())
    assert m and int(m.group(2)) == n == st["packets"] and int(m.group(3)) == 0 == st["crc8_errors"], printed
    # the head that is missing is the frames the synchronizer needed: they were dropped, not written, like the padding behind the stream; the frames that held the
    # n packets were not
    assert 0 < st["bbframes_dropped"] == int(m.group(1)) <= st["frames"] - n * 188 // 1769, printed


@pytest.mark.gpu
def test_the_default_sink_is_what_it_was(files):
    sent, f_noisy, d = files
    st0, printed0 = rx_run(f_noisy, str(d / "plain.u8"), [])
    st1, printed1 = rx_run(f_noisy, str(d / "bits.u8"), ["--snk-type", "BITS"])
    assert printed1 == printed0 and st1 == st0 and "BBFRAME" not in printed0 and "packets" not in st0
    raw = open(str(d / "plain.u8"), "rb").read()
    assert raw == open(str(d / "bits.u8"), "rb").read() and len(raw) == st0["frames"] * K // 8
    # every frame's K_bch bits, noise before the lock included: the twin's parser finds the same packets in them that --snk-type TS writes
    bits = np.unpackbits(np.frombuffer(raw, np.uint8).reshape(-1, K // 8), axis=1, bitorder="little").astype(np.int32)
    pk, status, _, _, _ = BR.parse(bits, None, BR.rx_state())
    assert not status.any() and len(pk) >= 400 and np.array_equal(pk, sent[600 - len(pk):])
