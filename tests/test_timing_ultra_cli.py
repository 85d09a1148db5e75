"""The command lines take the held Gardner loop's options (no GPU: parsing only), and the defaults are what they were."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rx_parses_the_ultra_options():
    from dvbs2_amd import rx
    a = rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin", "--stm-type", "ULTRA", "--stm-hold-size", "64"])
    assert (a.stm_type, a.stm_hold_size, a.stm_learn_frames) == ("ULTRA", 64, None)
    a = rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin", "--stm-type", "ULTRA", "--stm-learn-frames", "24"])
    assert (a.stm_hold_size, a.stm_learn_frames) == (101, 24)
    d = rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin"])
    assert (d.stm_type, d.stm_hold_size) == ("PERFECT", 101) and sum(d.wl_frames) == 500          # the learning frames' default: the phases' total


def test_sync_in_loop_parses_the_ultra_options():
    spec = importlib.util.spec_from_file_location("sync_in_loop", os.path.join(ROOT, "tools", "sync_in_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a = m.build_parser().parse_args(["--stm-type", "ULTRA", "--stm-hold-size", "64"])
    assert (a.stm_type, a.stm_hold_size, a.stm_learn_frames) == ("ULTRA", 64, 500)
    d = m.build_parser().parse_args([])
    assert (d.stm_type, d.stm_hold_size) == ("PERFECT", 101)
