"""The LDPC plan, byte for byte (CPU; tools/plan_probe.cpp `digest` links the library's host code): the planner is seeded and deterministic, so every table the LDPC
kernels read -- layer tables, per-lane address tables, row lists, swap masks, natural-order tables, the generic kernel's entries -- and every scalar that sizes their memory
is pinned by one line per case in tests/golden/ldpc_plan_digests.json, recorded from the plan as it stood before it was taken apart into stages.  A line that differs
means a table changed: `plan_probe digest ... --fields` at both commits names the field.

    python tests/test_plan_digest.py record        # rewrites the fixture (only for a change that is MEANT to alter a table)
    python tests/test_plan_digest.py against REV   # where the fixture comes from: the same cases with the plan builder of git revision REV -- its k_ldpc.hip compiled
                                                   # against this tree's headers and linked in front of the library's -- compared with the fixture
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ldpc_plan_digests.json")
CODES = ("QPSK-S_8/9", "QPSK-S_3/5", "32APSK-S_3/4", "QPSK-N_8/9")        # the four address tables
LDS_DEFAULT = 160 * 1024 - 512                                             # what dvbs2hip_create passes on gfx950
LDS_SMALL = 64 * 1024 - 512


def cases():
    """(modcod, spa_rule, small_batch, lds_limit, environment, extra arguments) of every pinned plan."""
    out = []
    for modcod in CODES:
        for rule in range(4):
            for small in (0, 1):
                for mode in (None, "lds", "global", "static", "park", "park4", "cu1"):
                    out.append((modcod, rule, small, LDS_DEFAULT, {"DVBS2HIP_LDPC_FAST_MODE": mode} if mode else {}, []))
    for modcod in CODES:
        for rule in (0, 3):
            out.append((modcod, rule, 0, LDS_SMALL, {}, []))
    for modcod in ("QPSK-N_8/9", "32APSK-S_3/4"):
        for rule in (0, 3):
            for env in ({"DVBS2HIP_LDPC_PATH": "generic"},
                        {"DVBS2HIP_LDPC_LOCK_DUPS": "0"},                                                                  # the retry-as-generic path
                        {"DVBS2HIP_LDPC_PATH": "generic", "DVBS2HIP_LDPC_C2V": "lds", "DVBS2HIP_LDPC_LDS_GROUPS": "20"},
                        {"DVBS2HIP_LDPC_PATH": "generic", "DVBS2HIP_LDPC_C2V": "global", "DVBS2HIP_LDPC_LDS_GROUPS": "20"},
                        {"DVBS2HIP_LDPC_SLOT_ALIGN": "4096", "DVBS2HIP_LDPC_SLOT_PAD": "256"}):
                out.append((modcod, rule, 0, LDS_DEFAULT, env, []))
    out.append(("QPSK-S_8/9", 0, 0, LDS_DEFAULT, {}, ["--bad-address"]))                                                  # an address >= M
    return out


def key(case):
    modcod, rule, small, lds, env, extra = case
    return " ".join([modcod, "spa_rule=%d" % rule, "small_batch=%d" % small, "lds=%d" % lds] + ["%s=%s" % (k.replace("DVBS2HIP_LDPC_", ""), v) for k, v in sorted(env.items())] + extra)


def build_probe(exe):
    from dvbs2_amd import build
    build.build_lib()
    lib = os.path.join(ROOT, "dvbs2_amd", "lib")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(ROOT, "dvbs2_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "plan_probe.cpp"), "-L", lib, "-ldvbs2hip", "-Wl,-rpath," + lib, "-o", exe], stderr=subprocess.DEVNULL)


def run_all(exe):
    base = {k: v for k, v in os.environ.items() if not k.startswith("DVBS2HIP_LDPC_") and k != "DVBS2HIP_VERBOSE"}

    def one(case):
        modcod, rule, small, lds, env, extra = case
        r = subprocess.run([exe, "digest", modcod, str(rule), str(small), str(lds)] + extra, env=dict(base, **env), capture_output=True, text=True)
        return key(case), (r.stdout.strip() if r.returncode == 0 else "exit %d: %s" % (r.returncode, r.stderr.strip()))
    with ThreadPoolExecutor(max_workers=4) as pool:
        return dict(pool.map(one, cases()))


@pytest.fixture(scope="module")
def digests(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_digest") / "plan_probe")
    build_probe(exe)
    return run_all(exe)


def test_every_plan_is_the_recorded_one(digests):
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(key(c) for c in cases()), "the fixture and the list of cases differ"
    assert len(want) == 4 * 4 * 2 * 7 + 4 * 2 + 2 * 2 * 5 + 1
    wrong = ["%s\n   recorded %s\n   built    %s" % (k, want[k], digests.get(k)) for k in sorted(want) if digests.get(k) != want[k]]
    assert not wrong, "%d of %d plans differ from the recorded ones:\n%s" % (len(wrong), len(want), "\n".join(wrong[:12]))


def test_the_cases_reach_every_image_mode_and_the_error_paths(digests):
    """The fixture is only worth what its cases cover: all six image modes, the generic kernel (forced, and by the retry), and an error string."""
    lines = list(digests.values())
    for mode in (0, 1, 3, 4, 5, 6):
        assert any(" fast 1 " in l and " fast_mode %d " % mode in l for l in lines), mode
    assert any(l.startswith("digest: '' fast 0 ") for l in lines)
    assert digests[key(("QPSK-N_8/9", 0, 0, LDS_DEFAULT, {"DVBS2HIP_LDPC_LOCK_DUPS": "0"}, []))].startswith("digest: '' fast 0 ")
    assert digests[key(cases()[-1])].startswith("digest: 'LDPC: address out of range' ")


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    sys.path.insert(0, ROOT)
    exe = os.path.join(ROOT, "tools", "bin", "plan_probe_digest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    build_probe(exe)
    got = run_all(exe)
    json.dump(got, open(FIXTURE, "w"), indent=0, sort_keys=True)
    print("%d cases -> %s" % (len(got), FIXTURE))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "against":
    import tempfile
    sys.path.insert(0, ROOT)
    from dvbs2_amd import build
    build.build_lib()
    csrc, lib = os.path.join(ROOT, "dvbs2_amd", "csrc"), os.path.join(ROOT, "dvbs2_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        src, obj, probe, exe = (os.path.join(td, n) for n in ("k_ldpc_rev.hip", "k_ldpc_rev.o", "probe.o", "plan_probe"))
        open(src, "w").write(subprocess.check_output(["git", "-C", ROOT, "show", sys.argv[2] + ":dvbs2_amd/csrc/k_ldpc.hip"], text=True))
        cc = ["/opt/rocm/bin/hipcc"]
        subprocess.check_call(cc + build.FLAGS + ["-I", csrc, "-c", src, "-o", obj], stderr=subprocess.DEVNULL)
        subprocess.check_call(cc + ["-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tools", "plan_probe.cpp"), "-o", probe], stderr=subprocess.DEVNULL)
        subprocess.check_call(cc + ["--offload-arch=" + build.ARCH, probe, obj, "-L", lib, "-ldvbs2hip", "-Wl,-rpath," + lib, "-o", exe], stderr=subprocess.DEVNULL)
        got = run_all(exe)
    want = json.load(open(FIXTURE))
    wrong = sorted(k for k in want if got.get(k) != want[k])
    print("plan builder of %s: %d of %d cases equal the fixture" % (sys.argv[2], len(want) - len(wrong), len(want)))
    for k in wrong[:12]:
        print(" ", k, "\n    recorded", want[k], "\n    built   ", got.get(k))
    sys.exit(1 if wrong else 0)
