"""dvbs2_tx with --tx-tasks: the IQ file made by the seven task calls is the file made by the fused tx_bb, byte for byte."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def run_tx(tmp_path, name, argv):
    from dvbs2_amd import tx
    path = str(tmp_path / name)
    n = tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", path, "-F", "4", "--n-frames", "8"] + argv), out=io.StringIO())
    assert n == 8
    return open(path, "rb").read()


def test_user_source_qpsk_same_file_with_and_without_tx_tasks(tmp_path):
    from dvbs2_amd.srcfile import save_src
    bits = np.unpackbits(np.load(os.path.join(GOLD, "src_K_14232.npy")))[:14232].astype(np.int32)
    src = str(tmp_path / "K_14232.src")
    save_src(src, bits)
    argv = ["--src-type", "USER", "--src-path", src, "--mod-cod", "QPSK-S_8/9"]
    fused, tasks = run_tx(tmp_path, "fused.bin", argv), run_tx(tmp_path, "tasks.bin", argv + ["--tx-tasks"])
    assert len(fused) == 8 * 2 * 8370 * 2 * 4 and tasks == fused


def test_azcw_8psk_same_file_with_and_without_tx_tasks(tmp_path):
    argv = ["--src-type", "AZCW", "--mod-cod", "8PSK-S_3/5"]
    fused, tasks = run_tx(tmp_path, "fused.bin", argv), run_tx(tmp_path, "tasks.bin", argv + ["--tx-tasks"])
    assert len(fused) > 0 and tasks == fused


def test_tx_tasks_with_the_random_source_raises(tmp_path):
    from dvbs2_amd import tx
    with pytest.raises(ValueError):
        tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", str(tmp_path / "x.bin"), "--tx-tasks", "--src-type", "RAND", "--n-frames", "4"]), out=io.StringIO())
