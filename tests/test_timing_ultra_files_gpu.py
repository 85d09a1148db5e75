"""The reference's README file workflow with a channel delay the receiver is not told, through the held Gardner loop: dvbs2_tx -> dvbs2_ch --chn-max-delay 4.5 ->
dvbs2_rx --stm-type ULTRA, where the whole loop finds the sampling phase over the learning frames and then holds mu over its hold blocks; and the same file through the C++
graph, host/dvbs2_rx_bb --matched-filter --stm-type ULTRA."""
import io
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARN = 24                                               # frames of the whole loop before it holds: three calls of -F 8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from dvbs2_amd import ch, tx
    from dvbs2_amd.srcfile import save_src
    d = tmp_path_factory.mktemp("stmu")
    bits = np.unpackbits(np.load(os.path.join(GOLD, "src_K_14232.npy")))[:14232].astype(np.int32)
    src = str(d / "K_14232.src")
    save_src(src, bits)
    f_tx, f_noisy = str(d / "out_tx.bin"), str(d / "out_tx_noisy.bin")
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-type", "USER_BIN", "--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "USER", "--src-path", src,
                                                "--mod-cod", "QPSK-S_8/9", "--n-frames", "64"]), out=log) == 64
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", "QPSK-S_8/9",
                                                "-m", "8", "--chn-max-delay", "4.5"]), out=log) == 64
    return src, f_noisy, bits


def rx_argv(src, f_noisy, snk):
    return ["--src-type", "USER", "--src-path", src, "--rad-type", "USER_BIN", "--rad-rx-file-path", f_noisy, "-F", "8", "--mod-cod", "QPSK-S_8/9",
            "--dec-implem", "NMS", "--dec-ite", "10", "--snk-path", snk, "--rad-rx-no-loop", "--no-wl-phases"]


@pytest.mark.parametrize("hold", [None, 64])
def test_ultra_timing_decodes_a_delayed_file(files, tmp_path, hold):
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    log = io.StringIO()
    extra = ["--stm-type", "ULTRA", "--stm-learn-frames", str(LEARN)] + (["--stm-hold-size", str(hold)] if hold else [])
    st = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, str(tmp_path / "ultra.u8")) + extra), out=log)
    assert st["locked_frames"] >= 16 and st["be"] == 0 and st["fe"] == 0, log.getvalue()
    got = np.unpackbits(np.fromfile(str(tmp_path / "ultra.u8"), dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert got.shape[0] >= 48 and (got[-24:] == bits[None, :]).all()          # the frames decoded while the loop holds


def test_wl_phases_with_ultra_is_refused(files, tmp_path):
    from dvbs2_amd import rx
    src, f_noisy, _ = files
    argv = [a for a in rx_argv(src, f_noisy, str(tmp_path / "x.u8")) if a != "--no-wl-phases"] + ["--stm-type", "ULTRA", "--wl-phases"]
    with pytest.raises(ValueError, match="ULTRA"):
        rx.run(rx.build_parser().parse_args(argv), out=io.StringIO())


def test_cpp_rx_graph_with_the_held_loop_gives_the_same_bits(files, tmp_path):
    """host/dvbs2_rx_bb --matched-filter --stm-type ULTRA binds Synchronizer_timing_hip with the lines it uses for FAST and sets act after the learning frames: the delayed
    file decodes to the bits dvbs2_amd.rx --stm-type ULTRA gives, and the monitor counts no error once the loops have locked"""
    import subprocess
    from dvbs2_amd import build as B
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    B.build_lib()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    psrc, pout = str(tmp_path / "src.i32"), str(tmp_path / "out.i32")
    np.tile(bits, (64, 1)).astype(np.int32).tofile(psrc)
    r = subprocess.run([os.path.join(ROOT, "host", "dvbs2_rx_bb"), "--matched-filter", "--stm-type", "ULTRA", "--stm-learn-frames", str(LEARN), "--mod-cod", "QPSK-S_8/9",
                        "-F", "8", "--dec-implem", "NMS", "--dec-ite", "10", "--in", f_noisy, "--src", psrc, "--src-delay", "1", "--mon-skip", "4", "--out", pout],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " FE 0\n" in r.stdout and "timing ULTRA hold size 101, holding after %d frames" % LEARN in r.stdout, r.stdout
    cpp = np.fromfile(pout, dtype=np.int32).reshape(-1, 14232)
    snk = str(tmp_path / "py.u8")
    rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--stm-type", "ULTRA", "--stm-learn-frames", str(LEARN)]), out=io.StringIO())
    py = np.unpackbits(np.fromfile(snk, dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert cpp.shape[0] == py.shape[0] and cpp.shape[0] >= 48
    assert np.array_equal(cpp[-16:], py[-16:]) and (cpp[-16:] == bits[None, :]).all()
    bad = subprocess.run([os.path.join(ROOT, "host", "dvbs2_rx_bb"), "--matched-filter", "--stm-type", "ULTRA", "--stm-hold-size", "4", "--in", f_noisy], capture_output=True, text=True)
    assert bad.returncode == 2 and "--stm-hold-size" in bad.stderr
