"""PLHEADER scan: device time of dvbs2hip_pls_scan_dev against dvbs2hip_pls_decode_located_dev over a table of all K = n_sym - 89 offsets of the same buffer -- the
existing decoder at a stride of one symbol, which is what the scan replaces (in two calls where K is above a handle's largest max_frames, their times added) -- and
of the whole dvbs2hip_pls_search_dev, in the same process on the same device buffers.
The two scans' outputs are compared bit for bit before anything is timed.  hipEvent times around the launches of each call (the library's own per-kernel timers); REPS
repetitions that alternate between the calls after a warm-up: median, min, max.  Buffers: frames of the library's own transmitter without noise, 2 frames + 90 symbols.
usage: python tools/bench_pls_search.py [--out results/pls_search/bench.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dvbs2_amd import lib_binding as B
from dvbs2_amd.receiver import Dvbs2Hip

REPS, WARM = 7, 3
BUFFERS = [("32APSK-S_3/4", 2 * 3402 + 90), ("QPSK-S_8/9", 2 * 8370 + 90), ("QPSK-N_8/9", 2 * 33282 + 90)]


def measure(modcod, n_sym):
    dev = torch.device("cuda", 0)
    K = n_sym - 89
    FMAX = min(K, 65534)                                                             # a handle's largest max_frames: the located decoder takes the K offsets in calls of at most this
    rx = Dvbs2Hip(modcod, max_frames=FMAX, n_ite=10)
    n, F = rx.pl_frame, 3
    zero = torch.zeros(F, dtype=torch.float32, device=dev)
    sent = torch.empty((F, rx.K_bch), dtype=torch.int32, device=dev)
    x = torch.empty((F, 2 * n), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rx.tx_bb_dev(None, 7, zero.data_ptr(), sent.data_ptr(), x.data_ptr(), F)        # PL frames of the library's own transmitter, no noise
    rx.synchronize()
    assert n_sym <= F * n
    out = {k: (torch.full((K,), -1, dtype=torch.int32, device=dev), torch.full((K,), -1.0, dtype=torch.float32, device=dev), torch.full((K,), -1.0, dtype=torch.float32, device=dev))
           for k in ("scan", "located")}
    SRC = torch.from_numpy(x.data_ptr() + 8 * np.arange(K, dtype=np.int64)).to(dev)
    RES = torch.zeros(4, dtype=torch.int32, device=dev); SCORE = torch.zeros(1, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    calls = {
        "pls_scan_dev": lambda: rx.pls_scan_dev(x.data_ptr(), n_sym, *(o.data_ptr() for o in out["scan"])),
        "pls_decode_located_dev": lambda: [rx.pls_decode_located_dev(SRC.data_ptr() + 8 * a, *(o.data_ptr() + 4 * a for o in out["located"]), min(FMAX, K - a)) for a in range(0, K, FMAX)],
        "pls_search_dev": lambda: rx.pls_search_dev(x.data_ptr(), n_sym, None, RES.data_ptr(), SCORE.data_ptr()),
    }
    for _ in range(WARM):
        for fn in calls.values():
            fn()
    rx.synchronize()
    for a, b in zip(out["scan"], out["located"]):
        assert torch.equal(a, b)                                                     # bit for bit: PLS, MET, ENE
    res = RES.cpu().numpy().tolist()
    assert res == [0, rx.pls_expected(), 3, 3], res                                  # headers at 0, n and 2 n: the last offset of the buffer is the third
    rx.timing_enable(True)
    ms = {k: [] for k in calls}
    for _ in range(REPS):
        for k, fn in calls.items():
            rx.timing_reset()
            fn()
            ms[k].append(rx.timing_get(B.K_MISC)[0])                                # (synchronizes)
    rx.timing_enable(False)
    rx.close()
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ms.items()}


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {}
    for modcod, n_sym in BUFFERS:
        res["%s n_sym=%d" % (modcod, n_sym)] = r = measure(modcod, n_sym)
        for k, v in r.items():
            print("%-14s n_sym=%-6d %-26s median %.4f ms  (min %.4f, max %.4f)" % (modcod, n_sym, k, v["median_ms"], v["min_ms"], v["max_ms"]))
    line = json.dumps(dict(tool="bench_pls_search", reps=REPS, warmup=WARM, device=torch.cuda.get_device_name(0), results=res))
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
