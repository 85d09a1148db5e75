"""`dvbs2_rx --pls-check` through raw IQ files (made as tests/test_tx_ch_rx_files_gpu.py makes them): a stream of another MODCOD of the same frame length, on which the
frame synchronizer locks just as well, is named and refused; a matching stream decodes as without the flag; and without the flag the receiver makes no pls_* call."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stepmf_ref as SR                                                            # noqa: E402

SENT = "QPSK-S_3/5"                                                                  # 8370 symbols per PL frame, like QPSK-S_8/9
K = 9552


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """32 frames of SENT through tx and the channel at 8 dB -> (pattern file, noisy IQ file, directory)"""
    from dvbs2_amd import ch, tx
    from dvbs2_amd.srcfile import save_src
    d = tmp_path_factory.mktemp("pls")
    src, f_tx, f_noisy = (str(d / n) for n in ("K_9552.src", "out_tx.bin", "out_tx_noisy.bin"))
    save_src(src, np.random.default_rng(3).integers(0, 2, K).astype(np.int32))
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "USER", "--src-path", src, "--mod-cod", SENT, "--n-frames", "32"]), out=log) == 32
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", SENT, "-m", "8.0"]), out=log) == 32
    return src, f_noisy, d


def rx_run(modcod, f_noisy, snk, extra):
    from dvbs2_amd import rx
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", f_noisy, "-F", "8", "--mod-cod", modcod, "--dec-implem", "NMS", "--dec-ite", "10", "--snk-path", snk,
                                              "--rad-rx-no-loop"] + extra), out=log)
    return st, log.getvalue()


@pytest.mark.gpu
def test_a_stream_of_another_modcod_is_named_and_refused(files):
    _, f_noisy, d = files
    with pytest.raises(ValueError, match=r"stream carries QPSK-S_3/5 \(PLS 23, pilots on\); the receiver was built for QPSK-S_8/9 \(PLS 43\)"):
        rx_run("QPSK-S_8/9", f_noisy, str(d / "wrong.u8"), ["--src-type", "NONE", "--pls-check"])
    # without the flag the same run goes through to the end and hands the sink its frames: nothing says why they are noise
    st, printed = rx_run("QPSK-S_8/9", f_noisy, str(d / "wrong.u8"), ["--src-type", "NONE"])
    assert st["frames"] >= 24 and "PLS" not in printed and "pls_mismatches" not in st


@pytest.mark.gpu
def test_a_matching_stream_decodes_as_without_the_flag(files):
    src, f_noisy, d = files
    user = ["--src-type", "USER", "--src-path", src]
    st0, printed0 = rx_run(SENT, f_noisy, str(d / "plain.u8"), user)
    st1, printed1 = rx_run(SENT, f_noisy, str(d / "check.u8"), user + ["--pls-check"])
    assert st0["locked_frames"] >= 24 and st0["be"] == 0 and st0["fe"] == 0, printed0
    assert printed1.rstrip().endswith("| PLS mismatches 0") and printed1.rstrip() == printed0.rstrip() + " | PLS mismatches 0"
    assert st1.pop("pls_mismatches") == 0 and st1 == st0
    assert open(str(d / "plain.u8"), "rb").read() == open(str(d / "check.u8"), "rb").read()


class Spy(SR.RecordingHandle):
    """the recording handle of tests/test_rx_sequence.py with the PLS decoder's two methods"""
    made = None

    def pls_expected(self):
        self._rec("pls_expected")
        return 43

    def pls_decode(self, X_N1):
        F = np.asarray(X_N1).reshape(-1, 2 * self.n).shape[0]
        self._rec("pls_decode", (), X_N1)
        return np.full(F, 43, np.int32), np.full(F, 90.0, np.float32), np.full(F, 90.0, np.float32)


@pytest.mark.parametrize("extra", [[], ["--sync-fine"], ["--stm-type", "FAST"]])
def test_without_the_flag_rx_makes_no_pls_call(extra, tmp_path, monkeypatch):
    """no GPU: the calls rx.run makes on its handle, with and without --pls-check -- the flag adds one pls_expected and a pls_decode of the aligned frames behind every
    frame synchronizer call, and nothing else moves"""
    from dvbs2_amd import receiver, rx
    from dvbs2_amd.srcfile import save_src
    F, N = 2, 8370
    iq, src = str(tmp_path / "in.bin"), str(tmp_path / "pattern.src")
    SR.RecordingHandle._fill(11, (5 * F, 4 * N)).tofile(iq)
    save_src(src, SR.RecordingHandle._fill(12, (2, 14232), np.int32))
    logs, sts = [], []
    for flag in ([], ["--pls-check"]):
        H = type("S", (Spy,), dict(made=[], not_ready=(1,)))
        monkeypatch.setattr(receiver, "Dvbs2Hip", H)
        args = rx.build_parser().parse_args(["--rad-rx-file-path", iq, "--rad-rx-no-loop", "-F", str(F), "--src-type", "USER", "--src-path", src] + extra + flag)
        sts.append(rx.run(args, out=io.StringIO()))
        assert len(H.made) == 1
        logs.append(H.made[0].log)
    plain, check = logs
    assert not [e for e in plain if e[0].startswith("pls_")]
    assert [e for e in check if not e[0].startswith("pls_")] == plain
    names = [e[0] for e in check]
    assert names.count("pls_expected") == 1 and names.count("pls_decode") == names.count("sync_frame_synchronize") >= 3
    for i, e in enumerate(check):
        if e[0] == "pls_decode":
            assert check[i - 1][0] == "sync_frame_synchronize"
    assert sts[1].pop("pls_mismatches") == 0 and sts[1] == sts[0]
