"""`dvbs2_tx --mod-cod-seq` and `dvbs2_rx --mod-cod VCM` through a raw IQ file: 20 frames of QPSK-S_3/5:3,16APSK-S_8/9:2, noise added to the file with NumPy at the level of
12 dB Eb/N0 of 16APSK-S_8/9 (the point of tests/test_pls_search_files_gpu.py, clear of the ten min-sum iterations' threshold), received with -F 4, NMS, 10 iterations and
the pilot-aided estimator.  The frames behind the acquisition decode to the sent bits in order, the sink holds exactly their bits; at most the frames of the first two
-F 4 reads of the probe (8 x 8370 symbols) may be missing.  Measured: none is -- all 20 frames come out (the default timing offset drops the two filters' group delays,
not a symbol of the first header; the transmitter ends its file with 40 zero symbols through the shaping filter, and the receiver pads the last read with noise, so the
last frame's last symbols leave the two filters)."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEQ = "QPSK-S_3/5:3,16APSK-S_8/9:2"
FRAMES = 20
MISSING = 0                                                                          # frames in front of the acquisition (see above)


def test_a_vcm_file_is_received_frame_by_frame(tmp_path):
    from dvbs2_amd import params as P
    from dvbs2_amd import rx, tx
    from dvbs2_amd.vcm import VcmTransmitter, parse_schedule
    f_tx, f_noisy, f_snk = (str(tmp_path / n) for n in ("out_tx.bin", "out_tx_noisy.bin", "snk.u8"))
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", f_tx, "-F", "4", "--mod-cod-seq", SEQ, "--n-frames", str(FRAMES)]), out=log) == FRAMES
    assert log.getvalue() == "(II) 20 frames (QPSK-S_3/5: 12, 16APSK-S_8/9: 8) written in '%s'\n" % f_tx
    # what was sent: the same transmitter, called as tx.py calls it
    again = VcmTransmitter(parse_schedule(SEQ), seed=0)
    sent = [f for _ in range(FRAMES // 4) for f in again.frames(4)[0]]
    again.close()
    assert [n for n, _ in sent[:6]] == ["QPSK-S_3/5"] * 3 + ["16APSK-S_8/9"] * 2 + ["QPSK-S_3/5"]
    x = np.fromfile(f_tx, np.float32)
    assert x.size == 2 * 2 * (sum(P.get_modcod(n).pl_frame for n, _ in sent) + 40)   # two samples per symbol; 40 symbols flush the two filters' group delays
    mc = P.get_modcod("16APSK-S_8/9")
    sigma = P.esn0_to_sigma(P.ebn0_to_esn0(12.0, mc.K_bch / mc.N_ldpc, mc.bps))
    (x + (sigma * np.random.default_rng(12).standard_normal(x.size)).astype(np.float32)).tofile(f_noisy)
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", f_noisy, "-F", "4", "--mod-cod", "VCM", "--dec-implem", "NMS", "--dec-ite", "10", "--est-type", "PILOTS",
                                              "--snk-path", f_snk, "--rad-rx-no-loop", "--src-type", "NONE"]), out=log)
    print(log.getvalue())
    got = st["frames"]
    print("frames in front of the acquisition: %d of %d" % (FRAMES - got, FRAMES))
    first_two_reads = sum(1 for o in np.cumsum([0] + [P.get_modcod(n).pl_frame for n, _ in sent[:-1]]) if o < 8 * 8370)
    assert FRAMES - got <= first_two_reads
    assert FRAMES - got == MISSING
    want = sent[FRAMES - got:]
    snk = open(f_snk, "rb").read()
    packed, at = [np.packbits(b.astype(np.uint8), bitorder="little").tobytes() for _, b in want], 0
    for f, p in enumerate(packed):                                                   # (frame by frame first, to say which one it is)
        assert snk[at:at + len(p)] == p, "frame %d (%s) of the decoded ones differs from what was sent" % (f, want[f][0])
        at += len(p)
    per = {}
    for n, _ in want:
        per[n] = per.get(n, 0) + 1
    assert st == dict(frames=got, per_modcod=per, skipped=0, losses=0, ldpc_down=0, bch_down=0)
    assert log.getvalue() == "# VCM: frames %d (%s) | skipped 0 | losses of lock 0 | LDPC flag down 0 | BCH flag down 0\n" % (got, ", ".join("%s: %d" % kv for kv in per.items()))
    assert snk == b"".join(packed)                                                   # the decoded frames' bits, nothing else
