"""dvbs2_amd/rx_sequence.py: the three callers of the transmission-phase sequence (dvbs2_amd/rx.py::run, tools/sync_in_loop.py::run_point, dvbs2_amd/acquire.py) make the
calls they made before the sequence was written once -- the same tasks in the same order on the same data with the same scalars, through every branch.  No GPU: the
handle is stepmf_ref.RecordingHandle, whose outputs are a function of each call's name and inputs alone; tests/golden/rx_sequence_calls.json holds the logs (and the
returned dicts) of the three callers as they were before, made by `python tests/test_rx_sequence.py --write` at that commit (results/rx_sequence/README.md).

One difference is allowed and stated here: before, the tool asked `filter` and then `sync_timing_set_act`, rx.py the other way round; the sequence keeps rx.py's order (the
reference sets act ahead of the whole task sequence, main_sched.cpp:655), so in the tool's logs every `filter` directly followed by `sync_timing_set_act` is transposed
-- `set_act_before_filter` below, applied to the recorded log, nothing else.  set_act touches the timing task's state alone, so the filter's output is the same."""
import hashlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stepmf_ref as SR                                                            # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "rx_sequence_calls.json")
MODCOD = "QPSK-S_8/9"
N = 8370                                                                           # pl_frame
KEEP = 40


def compact(log):
    """a long log (the tool's 500 learning frames) keeps its first and last KEEP entries; what lies between becomes its length and its SHA-256, so equality still
    means every entry"""
    if len(log) <= 2 * KEEP + 1:
        return log
    mid = log[KEEP:-KEEP]
    return log[:KEEP] + [["elided", [len(mid)], [hashlib.sha256(json.dumps(mid).encode()).hexdigest()]]] + log[-KEEP:]


def set_act_before_filter(log):
    """the one transposition (module docstring)"""
    log = [list(e) for e in log]
    for i in range(len(log) - 1):
        if log[i][0] == "filter" and log[i + 1][0] == "sync_timing_set_act":
            log[i], log[i + 1] = log[i + 1], log[i]
    return log


def handle(**script):
    return type("Scripted", (SR.RecordingHandle,), dict(script, made=[]))


def plain(o):
    return json.loads(json.dumps(o, default=float))


def record(H, fn):
    """-> dict(log, result | raises)"""
    try:
        out = dict(result=plain(fn()))
    except Exception as e:                                                          # (the parent's tool without stm_learn_frames: see CASES)
        out = dict(raises=type(e).__name__)
    logs = [h.log for h in H.made]
    assert len(logs) == 1
    return dict(out, log=compact(plain(logs[0])))


# ------------------------------------------------------------------ the three drivers
def run_rx(tmp, F, extra, calls, monkeypatch_setattr, **script):
    from dvbs2_amd import receiver, rx
    from dvbs2_amd.srcfile import save_src
    iq, src, snk = (os.path.join(tmp, n) for n in ("in.bin", "pattern.src", "out.u8"))
    SR.RecordingHandle._fill(11, (calls * F, 4 * N)).tofile(iq)
    save_src(src, SR.RecordingHandle._fill(12, (2, 14232), np.int32))
    H = handle(**script)
    monkeypatch_setattr(receiver, "Dvbs2Hip", H)
    args = rx.build_parser().parse_args(["--rad-rx-file-path", iq, "--rad-rx-no-loop", "-F", str(F), "--src-type", "USER", "--src-path", src, "--snk-path", snk] + extra)

    def go():
        log = io.StringIO()
        st = rx.run(args, out=log)
        return dict(st=st, printed=log.getvalue(), sink=hashlib.sha256(open(snk, "rb").read()).hexdigest())
    return record(H, go)


def tool():
    spec = importlib.util.spec_from_file_location("sync_in_loop", os.path.join(ROOT, "tools", "sync_in_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_tool(F, variant, script=None, **opts):
    from dvbs2_amd import params as P
    a = types.SimpleNamespace(**dict(dict(F=F, off=5, phase=0.3, freq=1e-4, seed=3, fe=10 ** 9, max_frames=3 * F, skip=F, est_perfect=False, agc=False), **opts))
    H = handle(**(script or {}))

    def go():
        r = tool().run_point(H, P, P.get_modcod(MODCOD), 3.8, variant, a)
        del r["seconds"]
        return r
    return record(H, go)


def run_acquire(F, give_up=False):
    from dvbs2_amd.acquire import acquire
    from dvbs2_amd.iqfile import ProcessingAborted
    H = handle(not_ready=(1, 9, 46), flag_from=10 ** 9 if give_up else 3)
    h = H(MODCOD, max_frames=F)
    left, seen = [60], []

    def receive():
        if not left[0]:
            raise ProcessingAborted()
        left[0] -= 1
        return SR.RecordingHandle._fill(20 + left[0], (F, 4 * N))

    def go():
        kw = dict(learn1=2, learn2=2, learn3=1, wait_max=5) if give_up else dict(learn1=20, learn2=20, learn3=6, wait_max=30)
        res = acquire(h, receive, n_frames=F, on_frames=lambda phase, n: seen.append([phase, n, len(h.log)]), **kw)
        return dict(res=res, on_frames=seen)
    return record(H, go)


GARDNER = dict(not_ready=(1,))
WL = dict(not_ready=(1, 100, 254, 504), flag_from=1, delay_moves=(2,))
TOOL_WL = dict(stm_type="FAST", wl_phases=True, chn_max_delay=4.0, chn_max_freq_shift=0.05, agc=True)
# name -> (driver, arguments); the numbers are the issue's configurations
CASES = {
    "01_rx_default": ("rx", dict(extra=[], calls=4)),
    "02_rx_sync_fine": ("rx", dict(extra=["--sync-fine"], calls=4, delay_moves=(2,))),
    "03_rx_no_agc_coarse": ("rx", dict(extra=["--no-agc", "--coarse-freq", "0.05", "--timing-offset", "0"], calls=4)),
    "04_rx_fast": ("rx", dict(extra=["--stm-type", "FAST"], calls=5, **GARDNER)),
    "05_rx_ultra_learn_2": ("rx", dict(extra=["--stm-type", "ULTRA", "--stm-learn-frames", "2", "--stm-hold-size", "64"], calls=5, **GARDNER)),
    "06_rx_wl_phases": ("rx", dict(extra=["--stm-type", "FAST", "--wl-phases", "--wl-frames", "2", "2", "1"], calls=14, not_ready=(1, 6, 9, 11), flag_from=1)),
    "07_tool_frame_agc": ("tool", dict(variant="frame", agc=True)),
    "08_tool_fine_est_perfect": ("tool", dict(variant="fine", est_perfect=True, script=dict(delay_moves=(2,)))),
    # 09: before, run_point read a.stm_learn_frames without a default and a namespace without it ended in AttributeError behind the first filter; that log is kept as
    # `..._absent_before`.  The issue wants the case to run: the attribute is optional now, with the parser's default, so the log to reproduce is the parser's default's
    "09_tool_ultra_absent_before": ("tool", dict(variant="frame", stm_type="ULTRA", stm_hold_size=64, script=GARDNER)),
    "09_tool_ultra_500": ("tool", dict(variant="frame", stm_type="ULTRA", stm_hold_size=64, stm_learn_frames=500, script=GARDNER)),
    "09b_tool_ultra_learn_2": ("tool", dict(variant="frame", stm_type="ULTRA", stm_hold_size=64, stm_learn_frames=2, agc=True, script=GARDNER)),
    "10_tool_wl_phases": ("tool", dict(variant="fine", script=WL, **TOOL_WL)),
    "11_acquire": ("acquire", dict()),
    "11_acquire_gives_up": ("acquire", dict(give_up=True)),
}


def run_case(name, F, tmp, setattr_):
    kind, kw = CASES[name]
    if kind == "rx":
        return run_rx(tmp, F, monkeypatch_setattr=setattr_, **kw)
    return run_tool(F, **kw) if kind == "tool" else run_acquire(F, **kw)


@pytest.fixture(scope="module")
def before():
    return json.load(open(FIXTURE))["cases"]


@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("name", [n for n in CASES if n != "09_tool_ultra_absent_before"])
def test_the_callers_make_the_calls_they_made_before(name, F, before, tmp_path, monkeypatch):
    want = before["%s F=%d" % (name, F)]
    if name == "09_tool_ultra_500":                                                # the namespace WITHOUT stm_learn_frames gives what 500 gave
        kind, kw = CASES[name]
        got = run_tool(F, **{k: v for k, v in kw.items() if k != "stm_learn_frames"})
        cut = before["09_tool_ultra_absent_before F=%d" % F]
        assert cut["raises"] == "AttributeError" and cut["log"] == want["log"][:len(cut["log"])]      # before: the same calls up to the error
    else:
        got = run_case(name, F, str(tmp_path), monkeypatch.setattr)
    log = set_act_before_filter(want["log"]) if CASES[name][0] == "tool" else want["log"]
    names = [e[0] for e in got["log"]]
    if name == "09b_tool_ultra_learn_2":
        assert log != want["log"]                                                   # the transposition is exercised
    if name in ("05_rx_ultra_learn_2", "09b_tool_ultra_learn_2"):
        # set_act at the first call that finds fed >= 2 frames -- the third at F = 1, the second at F = 2 -- and at every call after it, not before
        first = 2 // F
        assert [names[:i].count("filter") for i, n in enumerate(names) if n == "sync_timing_set_act"] == list(range(first, 5))
    for i, (g, w) in enumerate(zip(got["log"], log)):
        assert g == w, "call %d: %r, before %r" % (i, g, w)
    assert len(got["log"]) == len(log)
    assert got.get("result") == want.get("result") and "raises" not in got


def test_perfect_timing_at_offset_0_is_every_osf_th_sample():
    """what sync_in_loop wrote as mf[0::2]: offset 0, a call of exactly F pl_frame osf samples -> mf[0::osf], nothing carried"""
    from dvbs2_amd.rx_sequence import RxSequence
    for F, osf in ((1, 2), (2, 2), (2, 4)):
        h = SR.RecordingHandle(MODCOD, max_frames=F)
        seq = RxSequence(h, F, osf, pl_frame=N, timing="PERFECT", timing_offset=0)
        for call in range(2):
            x = h._fill(30 + call, (F, 2 * N * osf))
            sym = seq.symbols(x)
            mf = h.filter(x, n_frames=F).reshape(-1, 2)
            assert sym.shape == (F, 2 * N) and np.array_equal(sym.reshape(-1, 2), mf[0::osf]) and seq.tail.shape[0] == 0
    # with an offset the first call of F = 1 gives nothing and the tail carries on
    h = SR.RecordingHandle(MODCOD, max_frames=1)
    seq = RxSequence(h, 1, 2, pl_frame=N, timing="PERFECT", timing_offset=80)
    x = h._fill(40, (1, 4 * N))
    assert seq.symbols(x) is None and seq.tail.shape[0] == 2 * N - 80
    mf = h.filter(x).reshape(-1, 2)
    assert np.array_equal(seq.symbols(x).reshape(-1, 2), np.concatenate([mf[80:], mf])[0:2 * N:2]) and seq.tail.shape[0] == 2 * N - 80


def test_lock_tracker_counts_what_the_two_loops_counted():
    from dvbs2_amd.rx_sequence import LockTracker
    lk = LockTracker()
    stable = [lk.update(d) for d in (7, 7, 7, 9, 9, 9, 9, 9, 9, 4, 4, 5)]
    assert stable == [0, 1, 2, 0, 1, 2, 3, 4, 5, 0, 1, 0]                        # frames since the delay last moved; the first frame has nothing to compare with
    assert (lk.frames, lk.delay, lk.stable, lk.moved) == (12, 5, 0, 2)              # moves within the first 8 frames are the acquisition's


def test_the_sequence_takes_exactly_one_decoder():
    from dvbs2_amd.rx_sequence import RxSequence
    with pytest.raises(ValueError, match="fused"):
        RxSequence(None, 1, fine=True, fused=True)


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    import subprocess
    import tempfile
    cases = {}
    for name in CASES:
        for F in (1, 2):
            with tempfile.TemporaryDirectory() as tmp:
                cases["%s F=%d" % (name, F)] = run_case(name, F, tmp, setattr)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    json.dump(dict(commit=commit, cases=cases), open(FIXTURE, "w"), separators=(",", ":"))
    print("%s: %d cases, %d bytes" % (FIXTURE, len(cases), os.path.getsize(FIXTURE)))
