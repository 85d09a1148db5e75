"""The one-wave-per-stream form of the coarse-frequency loop, on the CPU: the chunked twin (tests/stepmf_wave_twin.c: rotation and matched filter of up to 64 samples
ahead, the serial steps behind, a cut where the PLL changes nu) against stepmf_twin.c bit for bit on the inputs of every GPU case; what those inputs exercise, read from
the twin's cut list; and the new entry through the layers that need no GPU: header, library, binding, the three command lines, acquire()."""
import os
import subprocess

import numpy as np
import pytest

import stepmf_ref as SR
import stepmf_wave_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = WR.N

_runs = {}


def run_case(case):
    """both twins over a case, call by call, compared as they go -> (the chunked twin's cuts, the sample counter per stream before every call); computed once"""
    if case not in _runs:
        S, Fs, calls, _, seed = case
        xs = WR.case_inputs(S, Fs, calls, seed)
        tm, sm = WR.twins(S)
        tw, sw = WR.twins(S, WR.StepMfWave)
        n_before = []
        for c in range(calls):
            D, X = WR.call_inputs(xs, S, Fs, c)
            n_before.append([cf.n for cf in sw.cf])
            want, got = sm.synchronize(D, X), sw.synchronize(D, X)
            for name, a, b in zip(("MU", "FRQ", "PHS", "Y", "B"), want, got):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, c, name, np.argwhere(a != b)[:4])
            Y2, _, R = tm.extract(want[3], want[4])
            Y2w, _, Rw = tw.extract(got[3], got[4])
            assert np.array_equal(R, Rw) and np.array_equal(Y2.view(np.uint32), Y2w.view(np.uint32))
            assert WR.state_bits(sm) == WR.state_bits(sw), (case, c)                # the PLL, nu, n, curr_idx, last_delay, the timing loop, the filter's memory
        assert len({cf.nu_k for cf in sm.cf}) >= min(S, 4) and all(cf.nu_k != 0 for cf in sm.cf)
        _runs[case] = (sw.cuts, n_before)
    return _runs[case]


@pytest.mark.parametrize("case", WR.CASES, ids=lambda c: "S%d-Fs%d-calls%d" % c[:3])
def test_chunked_order_gives_the_twins_bits(case):
    cuts, _ = run_case(case)
    assert cuts                                                                     # nu moved, so the chunked order was not the plain one


def test_the_sample_counter_wraps_inside_a_case():
    """the last case runs one stream past n = 999999: the call that holds the wrap is cut like every other, on either side of it"""
    case = WR.CASES[-1]
    S, Fs, calls, _, _ = case
    assert S == 1 and Fs * calls * N > 1000000
    cuts, n_before = run_case(case)
    wrap_call = next(c for c in range(1, calls) if n_before[c][0] < n_before[c - 1][0])
    at = 1000000 - n_before[wrap_call - 1][0]                                       # the sample of that call at which n is 0 again
    assert 0 < at < Fs * N
    in_call = sorted(a for c, _, a, _ in cuts if c == wrap_call - 1)
    assert in_call[0] < at < in_call[-1]
    # and a chunk holds the wrap in its middle: the last cut before it ends the chunk before, so the wrap is at position at - (that cut + 1) mod 64 of its chunk
    before = max(a for a in in_call if a < at)
    assert (at - (before + 1)) % WR.CHUNK != 0


def test_what_the_gpu_cases_exercise():
    """a condition on the INPUTS of tests/test_stepmf_wave_gpu.py, read from the chunked twin's cut list: a cut at every lane position, on the last and on the first
    sample of a call, and in a ragged last chunk"""
    every = []
    for case in WR.CASES:
        S, Fs, calls, _, _ = case
        L = Fs * N
        every += [(L, a, p) for _, _, a, p in run_case(case)[0]]
    assert {p for _, _, p in every} == set(range(64)), sorted(set(range(64)) - {p for _, _, p in every})
    assert any(a == L - 1 for L, a, _ in every)                                     # the call's last sample changes nu: the next call starts with it
    assert any(a == 0 for L, a, _ in every)                                         # ... and its first: a chunk of one final sample
    # a ragged last chunk: it starts at a - p, less than 64 samples before the call's end
    assert any(L - (a - p) < WR.CHUNK for L, a, p in every)
    assert all(0 <= p < 64 and p <= a < L for L, a, p in every)


# ------------------------------------------------------------------ the entry through the layers above the kernel
def test_header_library_and_binding_have_the_entry():
    import ctypes
    from dvbs2_amd import build as B
    from dvbs2_amd import lib_binding
    text = open(os.path.join(ROOT, "include", "dvbs2hip.h")).read()
    assert "int dvbs2hip_sync_step_mf_set_kernel(dvbs2hip_t *h, int32_t kernel);" in text
    assert "enum { DVBS2HIP_SMF_LANE = 0, DVBS2HIP_SMF_WAVE = 1 };" in text
    L = ctypes.CDLL(B.build_lib())
    assert hasattr(L, "dvbs2hip_sync_step_mf_set_kernel")
    assert "dvbs2hip_sync_step_mf_set_kernel" in lib_binding.ABI
    assert L.dvbs2hip_sync_step_mf_set_kernel(None, 1) == -1                         # no handle: DVBS2HIP_EINVAL, before anything is touched
    from dvbs2_amd.receiver import Dvbs2Hip
    assert Dvbs2Hip.SMF_KERNELS == {"LANE": 0, "WAVE": 1} and callable(Dvbs2Hip.sync_step_mf_set_kernel)


def test_the_wave_kernel_is_in_the_library_within_the_register_rules():
    import sys
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no ROCm LLVM tools in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dvbs2_amd import build as B
    B.build_lib()
    import kernel_regs
    ks = {k["name"]: k for k in kernel_regs.kernels()}
    k = ks["dvbs2::stepmf_wave_kernel"]
    assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 8 * (80 + 64)
    assert "dvbs2::stepmf_kernel" in ks


def test_the_python_command_lines_take_the_flag_and_refuse_it_without_the_phases():
    import sys
    from dvbs2_amd import params as P
    from dvbs2_amd import rx
    a = rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin", "--smf-kernel", "WAVE", "--wl-phases", "--stm-type", "FAST"])
    assert a.smf_kernel == "WAVE"
    assert rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin"]).smf_kernel is None
    with pytest.raises(SystemExit):
        rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin", "--smf-kernel", "BLOCK"])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sync_in_loop as T
    t = T.build_parser().parse_args(["--smf-kernel", "WAVE", "--wl-phases", "--stm-type", "FAST"])
    assert t.smf_kernel == "WAVE" and T.build_parser().parse_args([]).smf_kernel is None

    # without --wl-phases both refuse, with a sentence, and no handle has been asked for anything but its construction
    class Made(SR.RecordingHandle):
        made = []
    with pytest.raises(ValueError, match="--wl-phases"):
        T.run_point(Made, P, P.get_modcod("QPSK-S_8/9"), 3.8, "fine", T.build_parser().parse_args(["--smf-kernel", "WAVE", "-F", "1"]))
    import dvbs2_amd.receiver as R
    real = R.Dvbs2Hip
    R.Dvbs2Hip = Made
    try:
        with pytest.raises(ValueError, match="--wl-phases"):
            rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", "x.bin", "--rad-rx-no-loop", "--smf-kernel", "WAVE", "--stm-type", "FAST"]))
    finally:
        R.Dvbs2Hip = real
    assert all("set_kernel" not in e[0] for h in Made.made for e in h.log)


def test_the_host_program_takes_the_flag_and_refuses_it_without_the_phases():
    from dvbs2_amd import build as B
    B.build_lib()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    exe = os.path.join(ROOT, "host", "dvbs2_rx_bb")
    wl = ["--matched-filter", "--stm-type", "FAST", "--wl-phases"]
    # parsed and accepted: the run goes on to the mod-cod check (exit status 3), not to the parser's (2)
    r = subprocess.run([exe, "--smf-kernel", "WAVE", "--mod-cod", "QPSK-S_1/2", "--in", "/dev/null"] + wl, capture_output=True, text=True)
    assert r.returncode == 3 and "mod-cod scheme not supported" in r.stderr, r.stderr
    r = subprocess.run([exe, "--smf-kernel", "WAVE", "--mod-cod", "QPSK-S_1/2", "--in", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 2 and "--wl-phases" in r.stderr
    r = subprocess.run([exe, "--smf-kernel", "BLOCK", "--in", "/dev/null"] + wl, capture_output=True, text=True)
    assert r.returncode == 2 and "LANE or WAVE" in r.stderr
    assert "void set_kernel(int kernel)" in open(os.path.join(ROOT, "host", "dvbs2hip_modules.hpp")).read()


def test_acquire_calls_the_setter_only_when_asked():
    """smf_kernel=None on the recording handle, which has no such method: the calls are those without the argument; with it, the setter is the first call"""
    from dvbs2_amd.acquire import acquire
    from dvbs2_amd.iqfile import ProcessingAborted

    def run(handle, **kw):
        k = [0]

        def receive():
            k[0] += 1
            if k[0] > 12:
                raise ProcessingAborted()
            return SR.RecordingHandle._fill(k[0], (1, 2 * N))

        acquire(handle, receive, n_frames=1, learn1=2, learn2=2, learn3=2, **kw)
        return handle.log

    assert not hasattr(SR.RecordingHandle, "sync_step_mf_set_kernel")
    plain, none = run(SR.RecordingHandle()), run(SR.RecordingHandle(), smf_kernel=None)
    assert plain == none and len(plain) > 20

    class WithSetter(SR.RecordingHandle):
        def sync_step_mf_set_kernel(self, kernel="LANE"):
            self._rec("sync_step_mf_set_kernel", [kernel])

    wave = run(WithSetter(), smf_kernel="WAVE")
    assert wave[1] == ["sync_step_mf_set_kernel", ["WAVE"], []] and wave[:1] + wave[2:] == plain
    with pytest.raises(AttributeError):
        run(SR.RecordingHandle(), smf_kernel="WAVE")
