"""The reference's README file workflow with a channel delay the receiver is not told: dvbs2_tx -> dvbs2_ch --chn-max-delay 4.5 -> dvbs2_rx --stm-type FAST, where the
Gardner loop on the GPU finds the sampling phase; the default PERFECT extraction, half a sample off, does not decode the same file."""
import io
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from dvbs2_amd import ch, tx
    from dvbs2_amd.srcfile import save_src
    d = tmp_path_factory.mktemp("stm")
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


def test_fast_timing_decodes_a_delayed_file_and_perfect_timing_does_not(files, tmp_path):
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, str(tmp_path / "fast.u8")) + ["--stm-type", "FAST"]), out=log)
    assert st["locked_frames"] >= 16 and st["be"] == 0 and st["fe"] == 0, log.getvalue()
    got = np.unpackbits(np.fromfile(str(tmp_path / "fast.u8"), dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert (got[-8:] == bits[None, :]).all()
    pf = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, str(tmp_path / "perfect.u8"))), out=log)
    assert pf["fe"] > pf["locked_frames"] // 2 or pf["locked_frames"] < 8, log.getvalue()


def test_channel_delay_flag_leaves_the_default_output_unchanged(files, tmp_path):
    """without --chn-max-delay the channel writes what it wrote before; --chn-max-delay 4.0 delays the stream by four samples (two symbols)"""
    from dvbs2_amd import ch
    from dvbs2_amd.iqfile import RadioUserBinary
    N = 2 * 8370
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4, 2 * N)).astype(np.float32)
    src = str(tmp_path / "in.bin")
    RadioUserBinary(N, output_filename=src).send(x)
    outs = {}
    for name, extra in (("plain", []), ("d4", ["--chn-max-delay", "4.0"])):
        dst = str(tmp_path / (name + ".bin"))
        ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", src, "--rad-tx-file-path", dst, "--rad-rx-no-loop", "-F", "2", "-m", "200"] + extra), out=io.StringIO())
        outs[name] = RadioUserBinary(N, input_filename=dst, n_frames=4).receive().reshape(-1)
    assert np.allclose(outs["plain"], x.reshape(-1), atol=1e-6)
    assert np.allclose(outs["d4"][8:], x.reshape(-1)[:-8], atol=1e-6) and np.allclose(outs["d4"][:8], 0, atol=1e-6)


def test_cpp_rx_graph_with_the_timing_module_gives_the_same_bits(files, tmp_path):
    """host/dvbs2_rx_bb --matched-filter --stm-type FAST binds Synchronizer_timing_hip where the reference binds its timing synchronizer (RX/main_sched.cpp:202-204):
    the same delayed file decodes to the bits dvbs2_amd.rx --stm-type FAST gives, and the monitor counts no error once the loops have locked"""
    import subprocess
    from dvbs2_amd import build as B
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B.build_lib()
    subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s"])
    psrc, pout = str(tmp_path / "src.i32"), str(tmp_path / "out.i32")
    np.tile(bits, (64, 1)).astype(np.int32).tofile(psrc)
    r = subprocess.run([os.path.join(root, "host", "dvbs2_rx_bb"), "--matched-filter", "--stm-type", "FAST", "--mod-cod", "QPSK-S_8/9", "-F", "8", "--dec-implem", "NMS",
                        "--dec-ite", "10", "--in", f_noisy, "--src", psrc, "--src-delay", "1", "--mon-skip", "4", "--out", pout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " FE 0\n" in r.stdout and "timing FAST" in r.stdout, r.stdout
    cpp = np.fromfile(pout, dtype=np.int32).reshape(-1, 14232)
    snk = str(tmp_path / "py.u8")
    rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--stm-type", "FAST"]), out=io.StringIO())
    py = np.unpackbits(np.fromfile(snk, dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert cpp.shape[0] == py.shape[0] and cpp.shape[0] >= 48
    assert np.array_equal(cpp[-16:], py[-16:]) and (cpp[-16:] == bits[None, :]).all()
    r0 = subprocess.run([os.path.join(root, "host", "dvbs2_rx_bb"), "--matched-filter", "--mod-cod", "QPSK-S_8/9", "-F", "8", "--dec-implem", "NMS",
                         "--dec-ite", "10", "--in", f_noisy, "--src", psrc, "--src-delay", "1", "--mon-skip", "4"], capture_output=True, text=True)
    assert r0.returncode == 0 and " FE 0\n" not in r0.stdout, r0.stdout                # the stand-in at a known phase, half a sample off: frames are lost
