"""The file workflow with a carrier offset and a channel delay the receiver is not told: dvbs2_tx -> dvbs2_ch --chn-max-freq-shift f --chn-max-delay 4.5 ->
dvbs2_rx --wl-phases --stm-type FAST, where the waiting and learning phases find the offset with the coarse-frequency loop on the GPU.  Without the phases (and without
--coarse-freq) the same file does not decode."""
import io
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu

FREQ = 0.05            # cycles per sample: the reference traces' --chn-max-freq-shift
# Learning counts below the reference's 150 / 150 / 200 keep the file short.  Picked on the CPU with the twin (tests/test_stepmf_twin.py, run_phases_on_the_twin): the
# packet flag comes within 11 frames even at 3.8 dB, and at bandwidth 1e-4 the estimate is within a few 1e-3 cycles per sample of the offset after 25 frames and rings
# at that amplitude until about frame 75 (results/coarse/README.md).  48 + 48 frames end inside that ringing, which is all learning 3 needs: the L&R synchronizer that
# takes over is unambiguous to +-1 / (Lp / 2 + 1) = +-0.1 cycles per symbol (18 of a block's pilots, 9 lags), and 32 frames let its average (alpha 0.999) and the frame
# synchronizer settle.  Multiples of -F 8.
LEARN = ("48", "48", "32")
FRAMES = 256


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from dvbs2_amd import ch, tx
    from dvbs2_amd.srcfile import save_src
    d = tmp_path_factory.mktemp("acq")
    bits = np.unpackbits(np.load(os.path.join(GOLD, "src_K_14232.npy")))[:14232].astype(np.int32)
    src = str(d / "K_14232.src")
    save_src(src, bits)
    f_tx, f_noisy = str(d / "out_tx.bin"), str(d / "out_tx_noisy.bin")
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-type", "USER_BIN", "--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "USER", "--src-path", src,
                                                "--mod-cod", "QPSK-S_8/9", "--n-frames", str(FRAMES)]), out=log) == FRAMES
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", "QPSK-S_8/9",
                                                "-m", "8", "--chn-max-delay", "4.5", "--chn-max-freq-shift", str(FREQ)]), out=log) == FRAMES
    os.remove(f_tx)
    return src, f_noisy, bits


def rx_argv(src, f_noisy, snk):
    return ["--src-type", "USER", "--src-path", src, "--rad-type", "USER_BIN", "--rad-rx-file-path", f_noisy, "-F", "8", "--mod-cod", "QPSK-S_8/9",
            "--dec-implem", "NMS", "--dec-ite", "10", "--snk-path", snk, "--rad-rx-no-loop", "--stm-type", "FAST"]


def test_the_phases_decode_a_file_with_a_carrier_offset_and_nothing_else_does(files, tmp_path):
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    log = io.StringIO()
    snk = str(tmp_path / "wl.u8")
    st = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--wl-phases", "--wl-frames"] + list(LEARN)), out=log)
    acq = st["acquisition"]
    print(log.getvalue())
    assert acq["flag"] and acq["acquired"], log.getvalue()
    # (this checks the hand-over to L&R, not the PLL's accuracy: with 48 + 48 frames the freeze falls inside the loop's ringing; the pull-in test on the CPU covers the accuracy)
    assert abs(acq["freq"][0] - FREQ) < 1e-2, acq                      # a fifth of what L&R can take over: +-0.1 cycles per symbol = +-0.05 cycles per sample
    used = sum(acq["frames"].values())
    assert st["frames"] >= FRAMES - used - 16 and st["frames"] >= 64     # what is left of the file comes out (a call or two are held back by the timing loop's carry buffer)
    got = np.unpackbits(np.fromfile(snk, dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert got.shape[0] == st["frames"]
    assert (got == bits[None, :]).all(), (got != bits[None, :]).sum(axis=1)      # EVERY frame after the phases, the first one included
    assert st["be"] == 0 and st["fe"] == 0 and st["locked_frames"] >= st["frames"] - 4
    # the file needs the loop: the same receiver without the phases and without --coarse-freq loses most frames
    plain = rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, str(tmp_path / "plain.u8")) + ["--no-wl-phases"]), out=log)
    got0 = np.unpackbits(np.fromfile(str(tmp_path / "plain.u8"), dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    lost = int((got0 != bits[None, :]).any(axis=1).sum())
    assert lost > got0.shape[0] // 2, (lost, got0.shape[0])
    with pytest.raises(ValueError):
        rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--wl-phases", "--coarse-freq", "0.05"]), out=log)
    with pytest.raises(SystemExit):
        rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--wl-phases", "--no-wl-phases"])


def test_freq_shift_flag_leaves_the_default_output_unchanged(tmp_path):
    """without --chn-max-freq-shift the channel writes what it wrote before; with it the stream is rotated by exp(j 2 pi f n)"""
    from dvbs2_amd import ch
    from dvbs2_amd.iqfile import RadioUserBinary
    N = 2 * 8370
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4, 2 * N)).astype(np.float32)
    src = str(tmp_path / "in.bin")
    RadioUserBinary(N, output_filename=src).send(x)
    outs = {}
    for name, extra in (("plain", []), ("shift", ["--chn-max-freq-shift", "0.05"])):
        dst = str(tmp_path / (name + ".bin"))
        ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", src, "--rad-tx-file-path", dst, "--rad-rx-no-loop", "-F", "2", "-m", "200"] + extra), out=io.StringIO())
        outs[name] = RadioUserBinary(N, input_filename=dst, n_frames=4).receive().reshape(-1)
    assert np.allclose(outs["plain"], x.reshape(-1), atol=1e-6)
    # the task restates the reference's fp32 phase omega * n (Multiplier_sine_ccc_naive.cpp:71), whose rounding grows with n: the yardstick is the oracle's sample-by-sample
    # NCO in the same arithmetic, at nco_kernel's 2e-6 (plus the 1e-6 the channel's vanishing noise is given above)
    from oracle import oracle as O
    z, _ = O.nco(x.reshape(-1), np.floor(np.float32(0.05) * np.float32(1e6)) / np.float32(1e6), 0.0)
    assert np.max(np.abs(outs["shift"] - z)) <= 2e-6 * float(np.abs(z).max()) + 1e-6
    turn = (outs["shift"][0::2] + 1j * outs["shift"][1::2])[:100] / (x.reshape(-1)[0::2] + 1j * x.reshape(-1)[1::2])[:100]
    assert np.allclose(turn, np.exp(2j * np.pi * 0.05 * np.arange(100)), atol=1e-4)          # exp(+j 2 pi f n)


def test_cpp_rx_graph_with_the_phases_gives_the_same_bits(files, tmp_path):
    """host/dvbs2_rx_bb --matched-filter --stm-type FAST --wl-phases binds Synchronizer_step_mf_hip as RX/main_sched.cpp:428-432 does and runs the phases through it: the
    same file decodes to the bits dvbs2_amd.rx --wl-phases gives, and the monitor counts no error"""
    import subprocess
    from dvbs2_amd import build as B
    from dvbs2_amd import rx
    src, f_noisy, bits = files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B.build_lib()
    subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s"])
    psrc, pout = str(tmp_path / "src.i32"), str(tmp_path / "out.i32")
    np.tile(bits, (FRAMES, 1)).astype(np.int32).tofile(psrc)
    r = subprocess.run([os.path.join(root, "host", "dvbs2_rx_bb"), "--matched-filter", "--stm-type", "FAST", "--wl-phases", "--wl-frames"] + list(LEARN) +
                       ["--mod-cod", "QPSK-S_8/9", "-F", "8", "--dec-implem", "NMS", "--dec-ite", "10", "--in", f_noisy, "--src", psrc, "--src-delay", "1", "--mon-skip", "1",
                        "--out", pout], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " FE 0\n" in r.stdout and "wl phases" in r.stdout, r.stdout
    cpp = np.fromfile(pout, dtype=np.int32).reshape(-1, 14232)
    snk = str(tmp_path / "py.u8")
    rx.run(rx.build_parser().parse_args(rx_argv(src, f_noisy, snk) + ["--wl-phases", "--wl-frames"] + list(LEARN)), out=io.StringIO())
    py = np.unpackbits(np.fromfile(snk, dtype=np.uint8), bitorder="little").reshape(-1, 14232)
    assert cpp.shape[0] >= 64 and abs(cpp.shape[0] - py.shape[0]) <= 16
    assert (cpp == bits[None, :]).all() and (py == bits[None, :]).all()          # the same bits: every frame either path puts out is the payload
    k = min(cpp.shape[0], py.shape[0])
    assert np.array_equal(cpp[-k:], py[-k:])
