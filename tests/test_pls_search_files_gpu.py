"""`dvbs2_rx --mod-cod AUTO` through raw IQ files (made as tests/test_pls_files_gpu.py makes them): the receiver reads the MODCOD and the frame start from the PLHEADERs
of the head of the file, says so in one line, and then runs exactly as with the MODCOD named; a file of noise is refused."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 32


def make(d, modcod, K):
    from dvbs2_amd import ch, tx
    from dvbs2_amd.srcfile import save_src
    src, f_tx, f_noisy = (str(d / n) for n in ("pattern.src", "out_tx.bin", "out_tx_noisy.bin"))
    save_src(src, np.random.default_rng(K).integers(0, 2, K).astype(np.int32))
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", f_tx, "-F", "4", "--src-type", "USER", "--src-path", src, "--mod-cod", modcod, "--n-frames", str(FRAMES)]), out=log) == FRAMES
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "4", "--mod-cod", modcod, "-m", "12.0"]), out=log) == FRAMES     # (Eb/N0: clear of the ten min-sum iterations' threshold on 16APSK 8/9)
    return src, f_noisy


def rx_run(modcod, src, f_noisy, snk):
    from dvbs2_amd import rx
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", f_noisy, "-F", "4", "--mod-cod", modcod, "--dec-implem", "NMS", "--dec-ite", "10", "--snk-path", snk, "--rad-rx-no-loop",
                                              "--est-type", "PILOTS", "--src-type", "USER", "--src-path", src]), out=log)
    return st, log.getvalue()


@pytest.mark.parametrize("modcod,K,value", [("QPSK-S_3/5", 9552, 23), ("16APSK-S_8/9", 14232, 91)])
def test_auto_finds_the_modcod_and_then_runs_as_with_it_named(tmp_path, modcod, K, value):
    from dvbs2_amd import params as P
    assert P.pls_value(P.get_modcod(modcod)) == value
    src, f_noisy = make(tmp_path, modcod, K)
    named, printed0 = rx_run(modcod, src, f_noisy, str(tmp_path / "named.u8"))
    auto, printed1 = rx_run("AUTO", src, f_noisy, str(tmp_path / "auto.u8"))
    assert named["locked_frames"] >= FRAMES - 8 and named["be"] == 0 and named["fe"] == 0, printed0
    found = auto.pop("auto")
    assert auto == named and "auto" not in named
    n = P.get_modcod(modcod).pl_frame
    slots = -(-(found["symbols"] - 89 - found["offset"]) // n)
    assert found["modcod"] == modcod and found["value"] == value and found["pilots"] is True and 0 <= found["offset"] < n
    assert found["symbols"] >= 2 * 33282 + 90 and found["slots"] == slots and found["count"] == slots and found["score"] > 0.8 * slots
    first, rest = printed1.split("\n", 1)
    assert first == "# AUTO: %s (PLS %d, pilots on) | header at symbol %d | %d of %d headers | score %.2f" % (modcod, value, found["offset"], slots, slots, found["score"])
    assert rest == printed0
    assert open(str(tmp_path / "named.u8"), "rb").read() == open(str(tmp_path / "auto.u8"), "rb").read()


def test_auto_on_a_file_of_noise_raises(tmp_path):
    from dvbs2_amd import rx
    iq = str(tmp_path / "noise.bin")
    (np.random.default_rng(5).standard_normal(2 * 3 * 4 * 8370 * 2) * 0.5).astype(np.float32).tofile(iq)     # three -F 4 reads of the probe: whole frames of them, past 2 x 33282 + 90 symbols
    args = rx.build_parser().parse_args(["--rad-rx-file-path", iq, "-F", "4", "--mod-cod", "AUTO", "--src-type", "NONE", "--rad-rx-no-loop"])
    with pytest.raises(ValueError, match=r"--mod-cod AUTO: no chain of PLHEADERs in the first (8|9|10)\d{4} symbols .*best chain: "):
        rx.run(args, out=io.StringIO())
