"""PLS decoder: device time of a call of dvbs2hip_pls_decode_dev and of dvbs2hip_pls_decode_located_dev, and for scale of dvbs2hip_sync_freq_phase_synchronize_dev
(the pilot-phase synchronizer: it reads and writes whole frames), on the same frames in the same device buffers of one process.  hipEvent times around the launches of
each call (the library's own per-kernel timers); REPS repetitions that alternate between the three calls after a warm-up: median, min, max.
usage: python tools/bench_pls.py [--out results/pls/bench.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dvbs2_amd import lib_binding as B
from dvbs2_amd.receiver import Dvbs2Hip

REPS, WARM = 7, 3
BATCHES = [("QPSK-S_8/9", 4096), ("QPSK-N_8/9", 1024)]


def measure(modcod, F):
    dev = torch.device("cuda", 0)
    rx = Dvbs2Hip(modcod, max_frames=F, n_ite=10)
    n = rx.pl_frame
    zero = torch.zeros(F, dtype=torch.float32, device=dev)
    sent = torch.empty((F, rx.K_bch), dtype=torch.int32, device=dev)
    x = torch.empty((F, 2 * n), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    PLS = torch.empty(F, dtype=torch.int32, device=dev)
    MET, ENE, FRQ, PHS = (torch.empty(F, dtype=torch.float32, device=dev) for _ in range(4))
    SRC = torch.from_numpy(x.data_ptr() + 8 * n * np.arange(F, dtype=np.int64)).to(dev)
    torch.cuda.synchronize()
    rx.tx_bb_dev(None, 7, zero.data_ptr(), sent.data_ptr(), x.data_ptr(), F)        # PL frames of the library's own transmitter, no noise
    rx.synchronize()
    calls = {
        "pls_decode_dev": lambda: rx.pls_decode_dev(x.data_ptr(), PLS.data_ptr(), MET.data_ptr(), ENE.data_ptr(), F),
        "pls_decode_located_dev": lambda: rx.pls_decode_located_dev(SRC.data_ptr(), PLS.data_ptr(), MET.data_ptr(), ENE.data_ptr(), F),
        "sync_freq_phase_synchronize_dev": lambda: rx._chk(rx.L.dvbs2hip_sync_freq_phase_synchronize_dev(rx.h, x.data_ptr(), FRQ.data_ptr(), PHS.data_ptr(), y.data_ptr(), F)),
    }
    for _ in range(WARM):
        for fn in calls.values():
            fn()
    rx.synchronize()
    assert bool((PLS == rx.pls_expected()).all())
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
    for modcod, F in BATCHES:
        res["%s F=%d" % (modcod, F)] = r = measure(modcod, F)
        for k, v in r.items():
            print("%-14s F=%-5d %-34s median %.4f ms  (min %.4f, max %.4f)" % (modcod, F, k, v["median_ms"], v["min_ms"], v["max_ms"]))
    line = json.dumps(dict(tool="bench_pls", reps=REPS, warmup=WARM, device=torch.cuda.get_device_name(0), results=res))
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
