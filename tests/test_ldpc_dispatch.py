"""Which LDPC kernel a call runs on (CPU; tools/plan_probe.cpp `choice` and `insts` link the library's host code): ldpc_choose (dvbs2_amd/csrc/ldpc_dispatch.h) is the one place
that decides it, and what it says is held here against the built code objects and against what each kernel family can do.

The plans are the 253 of tests/test_plan_digest.cases(), each asked for a QC-schedule call of 1 frame and of one frame more than the device has CUs and for natural-order calls of
1, 4096, 8192 and 32768 frames; on top, the opt-in forms (DVBS2HIP_LDPC_LAT, DVBS2HIP_LDPC_ORDER, DVBS2HIP_CHAIN_UNFUSED, DVBS2HIP_CHAIN_SYN, DVBS2HIP_NAT_PARTS) and doctored plans.
"""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import test_plan_digest as D  # noqa: E402

N_CUS = 256
CALLS = ["qc:1", "qc:%d" % (N_CUS + 1), "natural:1", "natural:4096", "natural:8192", "natural:32768"]
STEERING = ("DVBS2HIP_LDPC_LAT", "DVBS2HIP_CHAIN_UNFUSED", "DVBS2HIP_CHAIN_SYN", "DVBS2HIP_LDPC_ORDER", "DVBS2HIP_NAT_PARTS")
LINE = re.compile(r"^choice (\S+): (\w+)(<.*?>) \| info (\d) bch (\d) order (\d) \| block (\d+) lds (\d+) per_cu (\d+) \| name '(.*)' \| error '(.*)'$")
# what a family's kernel can write (LdpcKParams::info_out, ::bch_flag / ::cwd_bch, ::order): k_ldpc_wg8.hip all three; k_ldpc_cu1.hip no BCH verification; nobody else anything
MAY = {"ldpc_wg8_kernel": (1, 1, 1), "ldpc_cu1_kernel": (1, 0, 1)}


def probe(exe, case, calls, env=None, doctor=()):
    """[(call, kernel, template arguments, info, bch, order, block, lds, per_cu, name, error)], or the plan's error string"""
    modcod, rule, small, lds, cenv, extra = case
    base = {k: v for k, v in os.environ.items() if not k.startswith("DVBS2HIP_LDPC_") and k not in STEERING and k != "DVBS2HIP_VERBOSE"}
    r = subprocess.run([exe, "choice", modcod, str(rule), str(small), str(lds), str(N_CUS)] + list(calls) + list(extra) + list(doctor), env=dict(base, **cenv, **(env or {})),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if r.stdout.startswith("plan: "):
        return r.stdout.strip()
    out = [LINE.match(l) for l in r.stdout.splitlines()]
    assert all(out) and len(out) == len(calls), r.stdout
    return [(m[1], m[2], m[3], int(m[4]), int(m[5]), int(m[6]), int(m[7]), int(m[8]), int(m[9]), m[10], m[11]) for m in out]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ldpc_dispatch") / "plan_probe")
    D.build_probe(path)
    return path


@pytest.fixture(scope="module")
def built():
    """the LDPC decoders among the kernel symbols of the built code objects"""
    from tools import kernel_regs
    names = {k["name"] for k in kernel_regs.kernels() if k["file"].startswith("k_ldpc")}
    return {n for n in names if re.match(r"ldpc_(layered_nms|wg8|cu1|lat|nat|nat_part|nat_ck|nat_spa)_kernel<", n)}


@pytest.fixture(scope="module")
def choices(exe):
    with ThreadPoolExecutor(max_workers=4) as pool:
        return dict(zip((D.key(c) for c in D.cases()), pool.map(lambda c: probe(exe, c, CALLS), D.cases())))


@pytest.fixture(scope="module")
def extras(exe):
    """the opt-in forms, which the 253 cases never reach: (what, rows)"""
    S, N = ("QPSK-S_8/9", 0, 1, D.LDS_DEFAULT, {}, []), ("QPSK-N_8/9", 0, 0, D.LDS_DEFAULT, {}, [])
    cu1 = ("QPSK-N_8/9", 3, 0, D.LDS_DEFAULT, {"DVBS2HIP_LDPC_FAST_MODE": "cu1"}, [])
    out = [("lat", probe(exe, c, ["qc:1", "qc:%d" % N_CUS], {"DVBS2HIP_LDPC_LAT": "1"})) for c in (S, ("QPSK-S_3/5", 0, 1, D.LDS_DEFAULT, {}, []), ("32APSK-S_3/4", 0, 1, D.LDS_DEFAULT, {}, []))]
    for c in (S, N, cu1):
        out.append(("order", probe(exe, c, ["qc:%d" % (2 * N_CUS), "qc:%d" % (4 * N_CUS)], {"DVBS2HIP_LDPC_ORDER": "1"})))
        out.append(("unfused", probe(exe, c, ["qc:1", "qc:4096"], {"DVBS2HIP_CHAIN_UNFUSED": "1"})))
        out.append(("syn0", probe(exe, c, ["qc:1", "qc:4096"], {"DVBS2HIP_CHAIN_SYN": "0"})))
    for parts in ("1", "4", "8", "88", "44", "82", "81", "48", "41"):
        out.append(("parts" + parts, probe(exe, S, ["natural:1", "natural:32768"], {"DVBS2HIP_NAT_PARTS": parts})))
    return out


def test_every_chosen_kernel_is_built_and_every_listed_one_too(exe, built, choices, extras):
    listed = set(subprocess.run([exe, "insts"], capture_output=True, text=True, check=True).stdout.split("\n")) - {""}
    assert listed == built, "the families' tables and the code objects differ: only listed %s, only built %s" % (sorted(listed - built), sorted(built - listed))
    assert sum(n.startswith("ldpc_wg8_kernel<") for n in listed) == 2 * 8 + 16 + 1      # 11 and 13 slots: image in LDS | global x four rules; 27 slots: modes 0, 1, 3, 4 x four rules, mode 5 min-sum only
    rows = [r for v in choices.values() if not isinstance(v, str) for r in v] + [r for _, v in extras for r in v]
    assert len(choices) == 253 and len(rows) >= 6 * 220
    for r in rows:
        assert r[10] or r[1] + r[2] in built, r
    assert {r[1] for r in rows if not r[10]} == {"ldpc_layered_nms_kernel", "ldpc_wg8_kernel", "ldpc_cu1_kernel", "ldpc_lat_kernel", "ldpc_nat_kernel", "ldpc_nat_part_kernel", "ldpc_nat_ck_kernel", "ldpc_nat_spa_kernel"}


def test_a_plan_without_the_fast_tables_has_no_natural_order_and_nothing_else_fails(choices):
    want = json.load(open(D.FIXTURE))
    for k, v in choices.items():
        err = re.match(r"digest: '(.*?)' fast ", want[k])[1]
        if err:      # (no plan, no handle: the recorded error strings, an address out of range among them)
            assert v == "plan: '%s'" % err, (k, v)
            continue
        fast = " fast 1 " in want[k]
        for r in v:
            assert bool(r[10]) == (r[0].startswith("natural") and not fast), (k, r)
            assert r[10] or (r[6] > 0 and r[6] % 64 == 0 and r[7] <= 160 * 1024 and r[8] in (0, 1, 2)), (k, r)
    assert sum(isinstance(v, str) for v in choices.values()) < 40


def test_a_choice_writes_only_what_its_family_can(choices, extras):
    rows = [r for v in choices.values() if not isinstance(v, str) for r in v] + [r for _, v in extras for r in v]
    for r in rows:
        may = MAY.get(r[1], (0, 0, 0))
        assert r[3] <= may[0] and r[4] <= may[1] and r[5] <= may[2], r
        assert r[4] <= r[3], r
    # ... and the fused chain is what a plain QC call gets: the throughput kernels write the output socket, k_ldpc_wg8.hip verifies
    for k, v in choices.items():
        for r in ([] if isinstance(v, str) else v[:2]):
            assert (r[3], r[4], r[5]) == {"ldpc_wg8_kernel": (1, 1, 0), "ldpc_cu1_kernel": (1, 0, 0)}.get(r[1], (0, 0, 0)), (k, r)
    ex = extras
    assert all(r[3] == 0 and r[4] == 0 for w, v in ex if w == "unfused" for r in v)
    assert all(r[3] == 1 and r[4] == 0 for w, v in ex if w == "syn0" for r in v)
    order = [v for w, v in ex if w == "order"]      # QPSK-S, QPSK-N (wg8: from 4 frames per CU), QPSK-N cu1 (from 2)
    assert [[r[5] for r in v] for v in order] == [[0, 1], [0, 1], [1, 1]] and order[2][0][1] == "ldpc_cu1_kernel"


def test_the_natural_order_form_follows_the_batch_and_the_override(choices, extras):
    v = choices[D.key(("QPSK-N_8/9", 0, 0, D.LDS_DEFAULT, {}, []))]
    assert [r[1] + r[2] for r in v[2:]] == ["ldpc_nat_ck_kernel<27, 8, 1>", "ldpc_nat_ck_kernel<27, 8, 2>", "ldpc_nat_ck_kernel<27, 4, 2>", "ldpc_nat_ck_kernel<27, 4, 2>"]
    assert all(r[9] == "ldpc_nat_kernel<27> / ldpc_nat_part_kernel<27,4|8> / ldpc_nat_ck_kernel<27,8|4,1|2|4> by batch size" for r in v[2:])
    got = {w: v[0][1] + v[0][2] for w, v in extras if w.startswith("parts")}
    assert got == {"parts1": "ldpc_nat_kernel<27>", "parts4": "ldpc_nat_part_kernel<27, 4, 12>", "parts8": "ldpc_nat_part_kernel<27, 8, 24>", "parts88": "ldpc_nat_ck_kernel<27, 8, 4>",
                   "parts44": "ldpc_nat_ck_kernel<27, 4, 2>", "parts82": "ldpc_nat_ck_kernel<27, 8, 2>", "parts81": "ldpc_nat_ck_kernel<27, 8, 1>", "parts48": "ldpc_nat_ck_kernel<27, 4, 4>",
                   "parts41": "ldpc_nat_ck_kernel<27, 4, 1>"}


def test_the_latency_kernel_only_where_its_preconditions_hold(exe):
    lat = {"DVBS2HIP_LDPC_LAT": "1"}
    for modcod, deg in (("QPSK-S_8/9", 27), ("QPSK-S_3/5", 11), ("32APSK-S_3/4", 13)):
        c = (modcod, 0, 1, D.LDS_DEFAULT, {}, [])
        one, full, over = probe(exe, c, ["qc:1", "qc:%d" % N_CUS, "qc:%d" % (N_CUS + 1)], lat)
        for r in (one, full):
            assert r[1] + r[2] == r[9] == "ldpc_lat_kernel<%d>" % deg and (r[3], r[4], r[5]) == (0, 0, 0) and r[6] == 768, r
        assert over[1] == "ldpc_wg8_kernel"
        assert probe(exe, c, ["qc:1"])[0][1] == "ldpc_wg8_kernel"                                    # not asked for
        # the junk row one row off, a slot count the kernel is not built for: chosen as wg8, named as wg8, the fused output kept
        r, = probe(exe, c, ["qc:1"], lat, ["--junk-row"])
        assert r[1] + r[2] == "ldpc_wg8_kernel<%d, 0, 0>" % deg and r[9] == "ldpc_wg8_kernel<%d,0>" % deg and (r[3], r[4]) == (1, 1) and not r[10], r
        r, = probe(exe, c, ["qc:1"], lat, ["--deg", "12"])
        assert r[1] == "ldpc_wg8_kernel" and r[3] == 1, r
    # sum-product, an image outside the LDS: not the LDS-only min-sum plan
    assert probe(exe, ("QPSK-S_8/9", 3, 1, D.LDS_DEFAULT, {}, []), ["qc:1"], lat)[0][1] == "ldpc_wg8_kernel"
    assert probe(exe, ("QPSK-S_8/9", 0, 1, D.LDS_DEFAULT, {"DVBS2HIP_LDPC_FAST_MODE": "global"}, []), ["qc:1"], lat)[0][1] == "ldpc_wg8_kernel"


def test_a_triple_without_an_instantiation_is_an_error_with_a_text(exe):
    N = ("QPSK-N_8/9", 0, 0, D.LDS_DEFAULT, {}, [])
    for doctor, text in ((["--rule", "3"], "ldpc_wg8_kernel<27,5,3>"),            # a sum-product plan in mode 5: k_ldpc_wg8.hip's own dispatch would run <27, 1, 3> on mode-5 tables
                         (["--mode", "2"], "ldpc_wg8_kernel<27,2,0>"), (["--deg", "12"], "ldpc_wg8_kernel<12,5,0>"), (["--mode", "3", "--deg", "13"], "ldpc_wg8_kernel<13,3,0>")):
        r, = probe(exe, N, ["qc:4096"], None, doctor)
        assert r[10] == "LDPC: the plan asks for %s, which is not built" % text, r
    for sched, text in (("natural:1", "ldpc_nat_ck_kernel<12,8,1>"), ("natural:32768", "ldpc_nat_ck_kernel<12,4,2>")):
        r, = probe(exe, N, [sched], None, ["--deg", "12"])
        assert r[10] == "LDPC: the plan asks for %s, which is not built" % text, r
    r, = probe(exe, ("QPSK-N_8/9", 3, 0, D.LDS_DEFAULT, {}, []), ["natural:1"], None, ["--deg", "12"])      # (the parent launched no decoder here and reported success)
    assert r[10] == "LDPC: the plan asks for ldpc_nat_spa_kernel<12,1>, which is not built", r
