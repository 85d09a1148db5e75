"""Which kernel a call of the receive path runs on, outside the LDPC decoder (CPU; tools/plan_probe.cpp `front`, `fir`, `upfir`, `sync`, `lr` and `walk` link the library's
host code): the choosers of dvbs2_amd/csrc/rx_dispatch.h are the one place that decides it, and what they say is held here against a restatement of each rule on both sides
of every threshold, against every knob (read at each call, so the probe takes them from its environment), and against the kernel symbols of the built code objects.
The fp64 GPU tests ask the same probe which form their cases reach (front_form, fir_form, sync_forms, lr_form below)."""
import os
import re
import subprocess

import pytest

from test_plan_digest import build_probe
from test_sync_seg_plan import FRAMES, PL_FRAMES, segment_plans

KNOBS = ("DVBS2HIP_FRONT_TWO_SWEEP", "DVBS2HIP_FRONT_SINGLE", "DVBS2HIP_FIR", "DVBS2HIP_FIR_WGS", "DVBS2HIP_SYNC", "DVBS2HIP_SYNC_UNFUSED", "DVBS2HIP_SYNC_ARGMAX4",
         "DVBS2HIP_SYNC_SEGMENTS", "DVBS2HIP_LR", "DVBS2HIP_LR_TIMEOUT_US", "DVBS2HIP_PLS_WALK_FORM", "DVBS2HIP_BCH_GRID")
WIDE, THREADS = 1024, 256                 # FRONT_WIDE, FRONT_THREADS
FM_TILE, FIR_TILE = 2048, 2048
# (bps, sep, itl_cols, n_sym, pl_frame) of the nine MODCODs as dvbs2hip_create sets them up (tests/test_sync_seg_plan.py holds the lengths against dvbs2_amd/params.py)
MODCODS = {"QPSK-S_8/9": (2, 1, 1, 8100, 8370), "QPSK-S_3/5": (2, 1, 1, 8100, 8370), "QPSK-N_8/9": (2, 1, 1, 32400, 33282), "8PSK-S_3/5": (3, 0, 3, 5400, 5598),
           "8PSK-S_8/9": (3, 0, 3, 5400, 5598), "8PSK-N_8/9": (3, 0, 3, 21600, 22230), "16APSK-S_8/9": (4, 0, 4, 4050, 4212), "16APSK-N_8/9": (4, 0, 4, 16200, 16686),
           "32APSK-S_3/4": (5, 0, 5, 3240, 3402)}


def ask(exe, mode, cases, env=None, inherit=False):
    """the probe's lines for `cases` (tuples of integers); the knobs are those of `env` alone, or with inherit those of this process and then `env`"""
    base = {k: v for k, v in os.environ.items() if inherit or k not in KNOBS}
    r = subprocess.run([exe, mode] + [str(int(v)) for c in cases for v in c], env=dict(base, **(env or {})), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases) and all(l.startswith(mode + ": ") for l in out), r.stdout
    return [l[len(mode) + 2:] for l in out]


def front_form(exe, modcod, F, align_pl=16, align_llr=16, located=False, sep=None, env=None, inherit=True):
    """the name front_choose gives the fused front end of a call, the knobs as this process has them now (monkeypatch.setenv included)"""
    bps, s, cols, n_sym, pl = MODCODS[modcod]
    return ask(exe, "front", [(bps, s if sep is None else sep, cols, n_sym, pl, F, align_pl, align_llr, located, 1, 1)], env, inherit)[0].split(" | ")[0]


def fir_form(exe, T, n_per, S=1, align_x=16, align_y=16, have_frag=True, env=None):
    return ask(exe, "fir", [(T, n_per, S, align_x, align_y, have_frag)], env, True)[0].split(" | ")[0]


def sync_forms(exe, n, Fs, S=1, align_x=16, one_task=True, located=False, env=None):
    """(correlator kernel, arg-max kernel) of a frame synchronizer call"""
    m = SYNC.match(ask(exe, "sync", [(n, Fs, S, align_x, 1, 1, one_task, located)], env, True)[0])
    return m[1], m[5]


def lr_form(exe, S, n, align_x=16, align_y=16, env=None):
    return ask(exe, "lr", [(S, n, align_x, align_y)], env, True)[0].split(" | ")[0]


FRONT = re.compile(r"^(.*?) \| block (\d+) grid (\d+) x (\d+) slice_chunk (\d+)$")
FIR = re.compile(r"^(.*?) \| grid (\d+) x (\d+) tiles_per_wg (\d+)$")
SYNC = re.compile(r"^(\S+) grid (\d+) x (\d+) fused (\d) \| (\S+) nwg (\d+) nseg (\d+) seg_F (\d+) \| delay line grid (\d+) x (\d+) x (\d+)$")
LR = re.compile(r"^(\S+) \| launches (\d) timeout_us (\d+) workgroups per frame (\d+) rotation (\S+)$")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rx_dispatch") / "plan_probe")
    build_probe(path)
    return path


# ------------------------------------------------------------------------------------------------------------------------ front end
def front_rule(bps, sep, cols, n_sym, pl, F, apl, allr, located, from_pl, deitl, two_sweep=False, single=False):
    """-> (name, block, grid_y, slice_chunk): the rule of k_front.hip as the parent commit had it in front_reg_try and front_dispatch"""
    if from_pl and not two_sweep:
        small, mid, big = n_sym <= 8 * WIDE, n_sym <= 22 * WIDE, n_sym <= 32 * WIDE
        pair = bps == 2 and sep and cols <= 1 and n_sym % 2 == 0 and pl % 2 == 0 and not single and (located or apl >= 16) and allr >= 16
        for ok, name in ((pair and small, "front_reg2_kernel<4>"), (pair and big, "front_reg2_kernel<16>"), (bps == 2 and sep and small, "front_reg_kernel<2, 8, true>"),
                         (bps == 2 and sep and big, "front_reg_kernel<2, 32, true>"), (bps == 2 and small, "front_reg_kernel<2, 8, false>"),
                         (bps == 3 and small, "front_reg_kernel<3, 8, false>"), (bps == 3 and mid, "front_reg_kernel<3, 22, false>")):
            if ok:
                return name, WIDE, 1, 0
    gy = chunk = 0
    if F < 512:
        trip = (4 if bps <= 3 else 1) * THREADS
        slices = min(-(-n_sym // trip), 1024 // F)
        if slices > 1:
            chunk = -(-(-(-n_sym // slices)) // trip) * trip
            gy = -(-n_sym // chunk)
    b = lambda v: "true" if v else "false"
    return "front_kernel<%d, %s, %s>%s" % (bps, b(from_pl), b(from_pl or deitl), " sliced" if chunk else ""), THREADS, max(gy, 1), chunk


def front_cases():
    out = []
    for bps, sep, cols in ((2, 1, 1), (2, 0, 1), (2, 1, 2), (3, 0, 3), (4, 0, 4), (5, 0, 5), (1, 0, 1)):
        for k in (8, 22, 32):
            for n_sym in (k * WIDE - 2, k * WIDE - 1, k * WIDE, k * WIDE + 1, k * WIDE + 2):
                out.append((bps, sep, cols, n_sym, n_sym + 90, 3, 16, 16, 0, 1, 1))
    out += [(1, 0, 1, 16200, 16290, 3, 16, 16, 0, 0, deitl) for deitl in (0, 1)]        # one bit per symbol through the stand-alone demapper
    for bps, sep, cols, n_sym, pl in MODCODS.values():
        for F in (1, 3, 300, 511, 512, 513):
            out.append((bps, sep, cols, n_sym, pl, F, 16, 16, 0, 1, 1))
            for deitl in (0, 1):
                out.append((bps, sep, cols, n_sym, pl, F, 16, 16, 0, 0, deitl))         # the stand-alone demapper: never a register-resident form
        for apl, allr, located in ((8, 16, 0), (16, 8, 0), (8, 8, 0), (4, 16, 0), (8, 16, 1), (16, 8, 1)):
            out.append((bps, sep, cols, n_sym, pl, 3, apl, allr, located, 1, 1))
        out.append((bps, 0, cols, n_sym, pl, 3, 16, 16, 0, 1, 1))                       # sep off (DVBS2HIP_DEMAP_GENERAL at create)
        out.append((bps, sep, cols, n_sym, pl + 1, 3, 16, 16, 0, 1, 1))                 # an odd PL frame: no pairs
    return out


@pytest.mark.parametrize("env,kw", [({}, {}), ({"DVBS2HIP_FRONT_TWO_SWEEP": "1"}, dict(two_sweep=True)), ({"DVBS2HIP_FRONT_SINGLE": "1"}, dict(single=True))], ids=["default", "two_sweep", "single"])
def test_front_end_form_slices_and_grid(exe, env, kw):
    cases = front_cases()
    seen = set()
    for c, line in zip(cases, ask(exe, "front", cases, env)):
        m = FRONT.match(line)
        assert m, line
        name, block, gy, chunk = front_rule(*c, **kw)
        assert (m[1], int(m[2]), int(m[3]), int(m[4]), int(m[5])) == (name, block, c[5], gy, chunk), (c, line)
        if chunk:      # whole trips per slice, every symbol in a slice, no more workgroups than 1024 / F per frame
            trip = (4 if c[0] <= 3 else 1) * THREADS
            assert chunk % trip == 0 and (gy - 1) * chunk < c[3] <= gy * chunk and 1 < gy <= 1024 // c[5], (c, line)
        seen.add(name)
    if not env:
        assert {"front_reg2_kernel<4>", "front_reg2_kernel<16>", "front_reg_kernel<2, 8, true>", "front_reg_kernel<2, 32, true>", "front_reg_kernel<2, 8, false>",
                "front_reg_kernel<3, 8, false>", "front_reg_kernel<3, 22, false>", "front_kernel<5, true, true> sliced", "front_kernel<5, true, true>",
                "front_kernel<4, false, false>", "front_kernel<2, false, true> sliced"} <= seen


def test_front_end_forms_the_fp64_test_documents(exe):
    """what tests/test_front_fp64_gpu.py's case A reaches: three frames, aligned sockets, no knob"""
    got = {m: front_form(exe, m, 3, inherit=False) for m in MODCODS}
    assert got == {"QPSK-S_8/9": "front_reg2_kernel<4>", "QPSK-S_3/5": "front_reg2_kernel<4>", "QPSK-N_8/9": "front_reg2_kernel<16>",
                   "8PSK-S_3/5": "front_reg_kernel<3, 8, false>", "8PSK-S_8/9": "front_reg_kernel<3, 8, false>", "8PSK-N_8/9": "front_reg_kernel<3, 22, false>",
                   "16APSK-S_8/9": "front_kernel<4, true, true> sliced", "16APSK-N_8/9": "front_kernel<4, true, true> sliced", "32APSK-S_3/4": "front_kernel<5, true, true> sliced"}
    assert front_form(exe, "32APSK-S_3/4", 300, inherit=False) == "front_kernel<5, true, true> sliced" and front_form(exe, "32APSK-S_3/4", 512, inherit=False) == "front_kernel<5, true, true>"
    assert ask(exe, "front", [(6, 0, 6, 3240, 3402, 3, 16, 16, 0, 1, 1)])[0].startswith("no front_kernel for 6 bits per symbol")


# ------------------------------------------------------------------------------------------------------------------------ FIR
def tiles_rule(n, max_wg=0):
    n_tiles = -(-n // FM_TILE)
    per = -(-n_tiles // max_wg) if max_wg > 0 else 4 if n_tiles >= 4096 else -(-n_tiles // 1024)
    return -(-n_tiles // per), per


def fir_rule(T, n_per, S, ax, ay, frag, valu=False, max_wg=0):
    if frag and not valu and T <= 81 and n_per >= 2 and (S == 1 or n_per % 2 == 0) and ax >= 16 and ay >= 16:
        gx, per = tiles_rule(n_per, max_wg)
        return "fir_mfma_kernel<%d>" % (5 if S > 1 else 1), gx, S, per
    return "fir_ccr_kernel<%d, %s>" % (81 if T == 81 else 0, "true" if S > 1 else "false"), -(-n_per // FIR_TILE), S, 0


def fir_cases():
    out = []
    for T in (1, 80, 81, 82, 257):
        for n_per in (1, 2, 1024, 2048, 2049, 4095 * FM_TILE, 4095 * FM_TILE + 1, 4096 * FM_TILE, 4096 * FM_TILE + 2, 1025 * FM_TILE):
            for S, ax, ay, frag in ((1, 16, 16, 1), (1, 8, 16, 1), (1, 16, 8, 1), (1, 16, 16, 0), (3, 16, 16, 1)):
                out.append((T, n_per, S, ax, ay, frag))
        out += [(T, 1025, 2, 16, 16, 1), (T, 1026, 2, 16, 16, 1), (T, 3 * FM_TILE + 1, 4, 16, 16, 1)]          # S > 1 with odd n_per: a stream would start on 8 bytes
    return out


@pytest.mark.parametrize("env,kw", [({}, {}), ({"DVBS2HIP_FIR": "valu"}, dict(valu=True)), ({"DVBS2HIP_FIR_WGS": "7"}, dict(max_wg=7)), ({"DVBS2HIP_FIR_WGS": "1024"}, dict(max_wg=1024))],
                         ids=["default", "valu", "wgs7", "wgs1024"])
def test_matched_filter_family_instantiation_and_grid(exe, env, kw):
    cases = fir_cases()
    seen = set()
    for c, line in zip(cases, ask(exe, "fir", cases, env)):
        m = FIR.match(line)
        assert m and (m[1], int(m[2]), int(m[3]), int(m[4])) == fir_rule(*c, **kw), (c, line)
        seen.add(m[1])
    assert seen == ({"fir_mfma_kernel<1>", "fir_mfma_kernel<5>"} if not kw.get("valu") else set()) | {"fir_ccr_kernel<81, false>", "fir_ccr_kernel<81, true>", "fir_ccr_kernel<0, false>", "fir_ccr_kernel<0, true>"}
    for bad in ((0, 1024, 1, 16, 16, 1), (258, 1024, 1, 16, 16, 1), (81, 0, 1, 16, 16, 1), (81, 1024, 0, 16, 16, 1), (81, 1024, 65536, 16, 16, 1)):
        assert ask(exe, "fir", [bad], env)[0].startswith("FIR: a parameter out of range")


def test_shaping_filter_takes_the_same_tile_rule_and_no_matched_filter_knob(exe):
    cases = [(T, 2, n, ax, ay, frag) for T in (1, 97, 98, 99, 100, 257) for n in (1, 2, 2048, 4095 * FM_TILE, 4096 * FM_TILE) for ax, ay, frag in ((16, 16, 1), (8, 16, 1), (16, 8, 1), (16, 16, 0))]
    cases += [(81, osf, 4096, 16, 16, 1) for osf in (1, 3, 4, 16)]
    for env in ({}, {"DVBS2HIP_FIR": "valu", "DVBS2HIP_FIR_WGS": "7"}):      # (the two knobs are the matched filter's)
        for c, line in zip(cases, ask(exe, "upfir", cases, env)):
            T, osf, n, ax, ay, frag = c
            m = FIR.match(line)
            if frag and osf == 2 and (T - 1) // 2 + 1 <= 49 and n >= 2 and ax >= 16 and ay >= 16:      # branches of 49 taps: T = 97 and 98; 50: T = 99
                want = ("fir_mfma_kernel<2>",) + tiles_rule(n)[:1] + (1,) + tiles_rule(n)[1:]
            else:
                want = ("upfir_kernel", -(-n // (256 // osf)), 1, 0)
            assert m and (m[1], int(m[2]), int(m[3]), int(m[4])) == want, (c, line)
    assert ask(exe, "upfir", [(81, 17, 4096, 16, 16, 1)])[0].startswith("FIR: a parameter out of range")


# ------------------------------------------------------------------------------------------------------------------------ frame synchronizer
def sync_rule(n, Fs, S, ax, frag, seg, one_task, located, valu=False, unfused=False, four=False):
    n_per = n * Fs
    mfma = frag and not valu and ax >= 16 and (S == 1 or n_per % 2 == 0)
    fused = bool(one_task and (located or not unfused))
    one = one_task and fused
    if mfma:
        corr = "sync_corr_mfma_%skernel<%s>" % ("streams_" if S > 1 else "", "true" if one else "false")
    else:
        corr = "%s<%s>" % ("sync_corr_m_kernel" if one else "sync_corr_kernel", "true" if S > 1 else "false")
    nwg = -(-n // 64)
    arg = "sync_average_argmax_streams_kernel" if S > 1 else "sync_metric_argmax_kernel<96>" if nwg <= 256 and not four else "sync_metric_argmax4_kernel"
    tot = (max(4 * (n + 1), 2 * n) + 3) // 4
    return corr, -(-n_per // (2048 if mfma else 1024)), S, int(fused), arg, nwg, -(-tot // 512), min(Fs + 1, 64) if located else Fs + 1, S


def sync_cases():
    out = []
    for n in PL_FRAMES + (16384, 16385):
        for Fs in (1, 62, 63, 64, 768, 1536, 4096):
            for S, ax, frag, seg, one_task, located in ((1, 16, 1, 1, 1, 0), (1, 16, 1, 1, 1, 1), (1, 16, 1, 1, 0, 0), (1, 8, 1, 1, 1, 0), (1, 16, 0, 1, 1, 0), (1, 16, 1, 0, 1, 0),
                                                        (2, 16, 1, 1, 1, 0), (3, 16, 1, 1, 0, 0), (2, 8, 1, 1, 1, 0)):
                out.append((n, Fs, S, ax, frag, seg, one_task, located))
    out += [(3401, 3, 2, 16, 1, 1, 1, 0), (3401, 4, 2, 16, 1, 1, 1, 0)]      # S > 1 and an odd number of samples per stream: a stream would start on 8 bytes
    return out


@pytest.mark.parametrize("env,kw", [({}, {}), ({"DVBS2HIP_SYNC": "valu"}, dict(valu=True)), ({"DVBS2HIP_SYNC_UNFUSED": "1"}, dict(unfused=True)), ({"DVBS2HIP_SYNC_ARGMAX4": "1"}, dict(four=True))],
                         ids=["default", "valu", "unfused", "argmax4"])
def test_synchronizer_correlators_arg_max_and_delay_line(exe, env, kw):
    cases = sync_cases()
    arg_of = {}
    for c, line in zip(cases, ask(exe, "sync", cases, env)):
        m = SYNC.match(line)
        assert m, line
        want = sync_rule(*c, **kw)
        got = (m[1], int(m[2]), int(m[3]), int(m[4]), m[5], int(m[6]), int(m[9]), int(m[10]), int(m[11]))
        assert got == want, (c, line, want)
        nseg, seg_F = int(m[7]), int(m[8])
        if m[5] != "sync_metric_argmax_kernel<96>" or not c[5]:
            assert nseg == 1, (c, line)                 # only the thirteen-wave form is cut, and only with its scratch
        if c[2] == 1:
            arg_of[c[0]] = m[5]
    if not kw.get("four"):      # at most 256 workgroups of 64 positions: the thirteen-wave form; 16686 and longer: round 3's four waves
        assert arg_of == {n: "sync_metric_argmax_kernel<96>" if n <= 16384 else "sync_metric_argmax4_kernel" for n in PL_FRAMES + (16384, 16385)}
        assert [arg_of[n] for n in PL_FRAMES] == ["sync_metric_argmax_kernel<96>"] * 4 + ["sync_metric_argmax4_kernel"] * 3
    else:
        assert set(arg_of.values()) == {"sync_metric_argmax4_kernel"}


def test_synchronizer_segments_are_the_segment_plan_under_every_cap(exe):
    """sync_choose's cut of a one-stream call = sync_segment_plan with the cap DVBS2HIP_SYNC_SEGMENTS gives (tests/test_sync_seg_plan.py holds that function to its rule)"""
    cases = [(n, F, 1, 16, 1, 1, 1, 0) for n in PL_FRAMES[:4] for F in FRAMES]
    for cap in (None,) + tuple(range(1, 9)):
        env = {} if cap is None else {"DVBS2HIP_SYNC_SEGMENTS": str(cap)}
        want = segment_plans(exe, [(c[0], c[1], 8 if cap is None else cap) for c in cases])
        got = [(int(m[7]), int(m[8])) for m in (SYNC.match(l) for l in ask(exe, "sync", cases, env))]
        assert got == want, cap
        assert (max(g[0] for g in got) > 1) == (cap != 1)


# ------------------------------------------------------------------------------------------------------------------------ L&R, the walk
@pytest.mark.parametrize("env", [{}, {"DVBS2HIP_LR": "unfused"}, {"DVBS2HIP_LR_TIMEOUT_US": "0"}, {"DVBS2HIP_LR_TIMEOUT_US": "250"}], ids=["default", "unfused", "timeout0", "timeout250"])
def test_lr_one_launch_or_three_and_the_rotation(exe, env):
    cases = [(S, n, ax, ay) for S in (1, 2, 8) for n in (3402, 3401, 8370, 33282, 2048, 2050) for ax, ay in ((16, 16), (8, 16), (16, 8))]
    for c, line in zip(cases, ask(exe, "lr", cases, env)):
        S, n, ax, ay = c
        m = LR.match(line)
        pair = n % 2 == 0 and ax >= 16 and ay >= 16
        one = S == 1 and pair and env.get("DVBS2HIP_LR") != "unfused"
        rot = "sff_rotate2_kernel<0>" if pair else "sff_rotate_kernel<0>"
        want = ("sff_lr_fused_kernel", 1, int(env.get("DVBS2HIP_LR_TIMEOUT_US", 1000000)), -(-(n // 2) // 1024), rot) if one else (rot, 3, 0, 0, rot)
        assert m and (m[1], int(m[2]), int(m[3]), int(m[4]), m[5]) == want, (c, line)


def test_walk_form_around_the_level_count(exe):
    lane, levels = "pls_walk_lane_kernel", "pls_walk_double_kernel"
    assert ask(exe, "walk", [(k,) for k in (0, 1, 4, 5, 6, 7, 20)]) == [lane] * 4 + [levels] * 3            # PLSW_LANE_LEVELS = 5
    assert ask(exe, "walk", [(1,), (20,)], {"DVBS2HIP_PLS_WALK_FORM": "levels"}) == [levels] * 2
    assert ask(exe, "walk", [(1,), (20,)], {"DVBS2HIP_PLS_WALK_FORM": "lane"}) == [lane] * 2


# ------------------------------------------------------------------------------------------------------------------------ the names are kernels
def test_every_name_a_chooser_returns_is_a_kernel_of_the_built_library(exe):
    """symbol names only, as tests/test_ldpc_dispatch.py compares its tables with the code objects"""
    from tools import kernel_regs
    built = {re.sub(r", 1024>$", ">", k["name"].replace("dvbs2::", "")) for k in kernel_regs.kernels() if k["file"] in ("k_front", "k_fir", "k_fir_mfma", "k_sync", "k_sync_mfma", "k_pls_walk")}
    names = set()
    for env in ({}, {"DVBS2HIP_FRONT_TWO_SWEEP": "1"}, {"DVBS2HIP_FRONT_SINGLE": "1"}):
        names |= {FRONT.match(l)[1].replace(" sliced", "") for l in ask(exe, "front", front_cases(), env)}
    for env in ({}, {"DVBS2HIP_FIR": "valu"}):
        names |= {FIR.match(l)[1] for l in ask(exe, "fir", fir_cases(), env)}
    names |= {FIR.match(l)[1] for l in ask(exe, "upfir", [(97, 2, 4096, 16, 16, 1), (99, 2, 4096, 16, 16, 1)])}
    for env in ({}, {"DVBS2HIP_SYNC": "valu"}, {"DVBS2HIP_SYNC_UNFUSED": "1"}, {"DVBS2HIP_SYNC_ARGMAX4": "1"}):
        for m in (SYNC.match(l) for l in ask(exe, "sync", sync_cases(), env)):
            names |= {m[1], m[5]}
    for m in (LR.match(l) for l in ask(exe, "lr", [(1, 3402, 16, 16), (2, 3402, 16, 16), (1, 3401, 16, 16)])):
        names |= {m[1], m[5]}
    names |= set(ask(exe, "walk", [(1,), (20,)]))
    assert len(names) >= 7 + 15 + 8 + 8 + 3 + 3 + 2 and names <= built, sorted(names - built)
    # ... and every instantiation of a chosen family is one some call reaches
    family = re.compile(r"^(front_reg2?_kernel|front_kernel|fir_ccr_kernel|fir_mfma_kernel|sync_corr(_m|_mfma|_mfma_streams)?_kernel|sff_rotate2?_kernel<0)")
    assert {b for b in built if family.match(b)} <= names, sorted({b for b in built if family.match(b)} - names)
