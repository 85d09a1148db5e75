"""The LDPC kernel a handle reports (dvbs2hip_ldpc_kernel_name), handle by handle, against tests/golden/ldpc_kernel_names.json: the names as the library gave them when the
kernel of a call was still decided in seven places, before ldpc_dispatch.hip took the choice over.  bench.py holds the name against profiles/ldpc_pmc_traffic.json and the
decoder tests compare it literally, so it stays character for character.  Nothing is decoded: a handle is created, asked, destroyed.

    python tests/test_ldpc_names_gpu.py record [FILE]      # (on a GPU) rewrites the fixture; public API only, so it runs in a checkout of any commit that has this file copied in
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ldpc_kernel_names.json")
IMPLEMS = ("NMS", "MS", "SPA", "SPA_TANH", "SPA_EXACT")
SHORT = ("QPSK-S_8/9", "QPSK-S_3/5", "32APSK-S_3/4")
STEERING = ("DVBS2HIP_LDPC_FAST_MODE", "DVBS2HIP_LDPC_LAT", "DVBS2HIP_LDPC_PATH", "DVBS2HIP_LDPC_ORDER", "DVBS2HIP_NAT_PARTS", "DVBS2HIP_CHAIN_UNFUSED", "DVBS2HIP_CHAIN_SYN", "DVBS2HIP_LDS_LIMIT")


def blocks():
    """block -> [(modcod, implem, environment, max_frames, natural order)]"""
    return {
        "normal": [("QPSK-N_8/9", i, {"DVBS2HIP_LDPC_FAST_MODE": m} if m else {}, f, False)
                   for i in IMPLEMS for m in (None, "lds", "global", "static", "park", "park4", "cu1") for f in (6, 1024)],
        "short": [(c, i, {"DVBS2HIP_LDPC_FAST_MODE": m} if m else {}, 1024, False) for c in SHORT for i in IMPLEMS for m in (None, "lds", "global")],
        "latency": [(c, "NMS", {"DVBS2HIP_LDPC_LAT": "1"}, 5, False) for c in SHORT],
        "natural": [(c, i, {}, 1024, True) for c in SHORT + ("QPSK-N_8/9",) for i in ("NMS", "SPA", "SPA_TANH")],
    }


def key(spec):
    modcod, implem, env, max_frames, natural = spec
    return " ".join([modcod, implem, "max_frames=%d" % max_frames] + ["%s=%s" % (k.replace("DVBS2HIP_LDPC_", ""), v) for k, v in sorted(env.items())] + (["natural"] if natural else []))


def names(specs):
    """the name of every handle (or the text its creation fails with); the steering variables are those of the spec alone"""
    from dvbs2_amd import lib_binding as B
    from dvbs2_amd.receiver import Dvbs2Hip
    saved = {k: os.environ.pop(k) for k in STEERING if k in os.environ}
    out = {}
    try:
        for spec in specs:
            modcod, implem, env, max_frames, natural = spec
            os.environ.update(env)
            try:
                rx = Dvbs2Hip(modcod, max_frames=max_frames, n_ite=10, implem=implem)
                if natural:
                    rx.set_ldpc_schedule(B.SCHED_NATURAL)
                out[key(spec)] = rx.ldpc_kernel_name()
                rx.close()
            except B.Dvbs2HipError as e:
                out[key(spec)] = "error: %s" % e
            finally:
                for k in env:
                    del os.environ[k]
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("block", sorted(blocks()))
def test_every_handle_names_the_kernel_it_named_before(block):
    want = json.load(open(FIXTURE))
    specs = blocks()[block]
    assert sorted(want) == sorted(key(s) for b in blocks().values() for s in b), "the fixture and the list of handles differ"
    got = names(specs)
    wrong = ["%s: recorded %r, now %r" % (k, want[k], got[k]) for k in got if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)


def test_the_handles_reach_every_family_and_image_mode():
    """(CPU) the fixture is only worth what its handles cover"""
    want = json.load(open(FIXTURE))
    assert len(want) == 5 * 7 * 2 + 3 * 5 * 3 + 3 + 4 * 3
    for piece in ["ldpc_wg8_kernel<27,%d>" % m for m in (0, 1, 3, 4, 5)] + ["ldpc_wg8_kernel<27,4,3>", "ldpc_wg8_kernel<11,1,2>", "ldpc_wg8_kernel<13,0,1>", "ldpc_cu1_kernel<27>", "ldpc_cu1_kernel<27,3>",
                  "ldpc_cu1_kernel<27,1>", "ldpc_lat_kernel<27>", "ldpc_lat_kernel<11>", "ldpc_lat_kernel<13>", "ldpc_nat_spa_kernel<27,1>", "ldpc_nat_spa_kernel<11,2>", "ldpc_nat_kernel<13> / "]:
        assert any(v.startswith(piece) for v in want.values()), piece
    assert not any(v.startswith("error") for v in want.values())


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    import time
    sys.path.insert(0, ROOT)
    t0 = time.time()
    got = names([s for b in blocks().values() for s in b])
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    json.dump(got, open(path, "w"), indent=0, sort_keys=True)
    print("%d handles in %.1f s -> %s" % (len(got), time.time() - t0, path))
