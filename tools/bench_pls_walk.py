"""PLHEADER walk: device time of dvbs2hip_pls_walk_dev in its two forms -- one lane following the chain, and pointer doubling over the candidates -- against
dvbs2hip_pls_scan_dev on the same buffer (the one device call before the walk that yields headers at unknown places), in the same process on the same device buffers.
The form is chosen per call through DVBS2HIP_PLS_WALK_FORM (lane | levels), which the library reads at every call; "default" is the library's own choice.
The three walks' outputs are compared before anything is timed.  hipEvent times around the launches of each call (the library's own per-kernel timers, the PLS decoder at
the candidates included); REPS repetitions that alternate between the calls after a warm-up: median, min, max.
Buffers: 8 mixed short frames and a cut-off ninth; short frames of four MODCODs over and over to 2^23 symbols.  Noise-free, the library's own transmitter.
usage: python tools/bench_pls_walk.py [--out results/pls_walk/bench.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dvbs2_amd import lib_binding as B
from dvbs2_amd import params as P
from dvbs2_amd.receiver import Dvbs2Hip

REPS, WARM = 9, 3
MIX = ["QPSK-S_8/9", "32APSK-S_3/4", "16APSK-S_8/9", "8PSK-S_3/5"]
MAX_OUT = 4096


def frames():
    out = {}
    for i, name in enumerate(MIX):
        h = Dvbs2Hip(name, max_frames=2)
        out[name] = list(h.tx_bb(2, seed=300 + i)[1])
        h.close()
    return out


def measure(rx, x, table):
    """table: "caller" (params.VCM_FRAME_SYMBOLS on the device: the walk has to allow for a hop of 90 symbols) or "library" (LEN = NULL: the shortest frame is known)"""
    dev = torch.device("cuda", 0)
    n_sym = x.size // 2
    K = n_sym - 89
    xd = torch.from_numpy(x).to(dev)
    LEN = torch.from_numpy(P.VCM_FRAME_SYMBOLS).to(dev) if table == "caller" else None
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    outs = {k: dict(OFF=i32(MAX_OUT), VAL=i32(MAX_OUT), Q=torch.zeros(MAX_OUT, device=dev), SRC=torch.zeros(MAX_OUT, dtype=torch.int64, device=dev), IDX=i32(MAX_OUT), CNT=i32(256), RES=i32(4))
            for k in ("default", "lane", "levels")}
    scan = (i32(K), torch.zeros(K, device=dev), torch.zeros(K, device=dev))
    torch.cuda.synchronize()

    def walk(form):
        def call():
            if form == "default":
                os.environ.pop("DVBS2HIP_PLS_WALK_FORM", None)
            else:
                os.environ["DVBS2HIP_PLS_WALK_FORM"] = form
            o = outs[form]
            rx.pls_walk_dev(xd.data_ptr(), n_sym, 0, None if LEN is None else LEN.data_ptr(), None, MAX_OUT, *(o[k].data_ptr() for k in ("OFF", "VAL", "Q", "SRC", "IDX", "CNT", "RES")))
        return call

    calls = {"pls_scan_dev": lambda: rx.pls_scan_dev(xd.data_ptr(), n_sym, *(t.data_ptr() for t in scan))}
    calls.update({"pls_walk_dev " + f: walk(f) for f in outs})
    for _ in range(WARM):
        for fn in calls.values():
            fn()
    rx.synchronize()
    N = int(outs["lane"]["RES"][0])
    for k in ("OFF", "VAL", "Q", "SRC", "IDX", "CNT", "RES"):                        # the forms agree, bit for bit
        n = N if k not in ("CNT", "RES") else None
        assert torch.equal(outs["lane"][k][:n], outs["levels"][k][:n]) and torch.equal(outs["lane"][k][:n], outs["default"][k][:n]), k
    rx.timing_enable(True)
    ms = {k: [] for k in calls}
    for _ in range(REPS):
        for k, fn in calls.items():
            rx.timing_reset()
            fn()
            ms[k].append(rx.timing_get(B.K_MISC)[0])                                # (synchronizes)
    rx.timing_enable(False)
    os.environ.pop("DVBS2HIP_PLS_WALK_FORM", None)
    r = {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ms.items()}
    r["frames"], r["status"] = N, int(outs["lane"]["RES"][2])
    return r


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    f = frames()
    small = np.concatenate([f[n][0] for n in MIX] + [f[n][1] for n in MIX] + [f[MIX[0]][0][:4000]])
    cycle = np.concatenate([f[n][i] for i in range(2) for n in MIX])
    big = np.tile(cycle, -(-2 * (1 << 23) // cycle.size))[:2 << 23]
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=1)
    res = {}
    for name, x in (("8 short frames", small), ("2^23 symbols", big)):
        for table in ("caller", "library"):
            res["%s, n_sym=%d, %s's table" % (name, x.size // 2, table)] = r = measure(rx, x, table)
            for k, v in r.items():
                if isinstance(v, dict):
                    print("%-16s n_sym=%-8d %-8s %-22s median %.4f ms  (min %.4f, max %.4f)" % (name, x.size // 2, table, k, v["median_ms"], v["min_ms"], v["max_ms"]))
            print("%-16s frames %d, status %d" % (name, r["frames"], r["status"]))
    rx.close()
    line = json.dumps(dict(tool="bench_pls_walk", reps=REPS, warmup=WARM, max_out=MAX_OUT, device=torch.cuda.get_device_name(0), results=res))
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
