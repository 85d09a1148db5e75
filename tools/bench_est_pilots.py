"""Pilot-aided noise estimator: device time of a call of dvbs2hip_estimate_pilots_dev (scrambled = 1, alpha = 0) and, on the same frames in the same run, of
dvbs2hip_estimate_dev (the M2M4 estimator, which reads every data symbol of the XFEC frames).  hipEvent times around the launches of each call (the library's own
per-kernel timers); REPS repetitions that alternate between the calls after a warm-up: median, min, max.  Writes bench.json and README.md into --out-dir.
usage: python tools/bench_est_pilots.py [--out-dir results/est_pilots]"""
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
    sig = torch.full((F,), 0.1, dtype=torch.float32, device=dev)
    sent = torch.empty((F, rx.K_bch), dtype=torch.int32, device=dev)
    x = torch.empty((F, 2 * n), dtype=torch.float32, device=dev)
    xf = torch.empty((F, 2 * rx.N_xfec), dtype=torch.float32, device=dev)
    out = torch.empty((2, 3, F), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rx.tx_bb_dev(None, 7, sig.data_ptr(), sent.data_ptr(), x.data_ptr(), F)         # PL frames of the library's own transmitter at sigma = 0.1 (Es/N0 = 17 dB)
    rx._chk(rx.L.dvbs2hip_pl_descramble_dev(rx.h, x.data_ptr(), x.data_ptr(), F))
    rx._chk(rx.L.dvbs2hip_remove_plh_dev(rx.h, x.data_ptr(), xf.data_ptr(), F))
    rx.synchronize()
    calls = {
        "estimate_pilots_dev": lambda: rx.estimate_pilots_dev(x.data_ptr(), 0, out[0, 0].data_ptr(), out[0, 1].data_ptr(), out[0, 2].data_ptr(), F),
        "estimate_dev": lambda: rx._chk(rx.L.dvbs2hip_estimate_dev(rx.h, xf.data_ptr(), out[1, 0].data_ptr(), out[1, 1].data_ptr(), out[1, 2].data_ptr(), F)),
    }
    for _ in range(WARM):
        for fn in calls.values():
            fn()
    rx.synchronize()
    s = out[0, 0].cpu().numpy()
    assert np.abs(s / 0.1 - 1).max() < 0.25, (s.min(), s.max())                      # (the frames are what the call is meant for)
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
    out_dir = sys.argv[sys.argv.index("--out-dir") + 1] if "--out-dir" in sys.argv else None
    res = {}
    for modcod, F in BATCHES:
        res["%s F=%d" % (modcod, F)] = r = measure(modcod, F)
        for k, v in r.items():
            print("%-14s F=%-5d %-22s median %.4f ms  (min %.4f, max %.4f)" % (modcod, F, k, v["median_ms"], v["min_ms"], v["max_ms"]))
    line = json.dumps(dict(tool="bench_est_pilots", reps=REPS, warmup=WARM, device=torch.cuda.get_device_name(0), results=res))
    print(line)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        open(os.path.join(out_dir, "bench.json"), "w").write(line + "\n")
        rows = ["| %s | `dvbs2hip_%s` | %.4f | %.4f .. %.4f |" % (b.replace(" F=", ", ") + " frames", k, v["median_ms"], v["min_ms"], v["max_ms"]) for b, r in res.items() for k, v in r.items()]
        open(os.path.join(out_dir, "README.md"), "w").write(
            "# Pilot-aided noise estimator: device time of a call\n\n"
            "`tools/bench_est_pilots.py` (`bench.json` beside this file; %s as the runtime reports it).  One process, one set of device buffers per batch: PL frames of the\n"
            "library's own transmitter at sigma = 0.1, PL-descrambled; the M2M4 call runs on their XFEC symbols.  hipEvent pairs of the handle around the launches of each call;\n"
            "after %d warm-up rounds, %d rounds that alternate between the two calls; median, min .. max in ms.\n\n"
            "| batch | call | median ms | min .. max ms |\n|---|---|---|---|\n%s\n\n"
            "The pilot-aided call fetches the 90 + 36 N_pilots known symbols of a frame (2.2 KB of a short QPSK frame, 7 KB of a normal one); the M2M4 call reads every data symbol\n"
            "(65 and 259 KB per frame).  No target was set for either.  Not measured: the host form, the averaging form (alpha > 0: a second, serial launch), a kernel-trace time.\n"
            % (torch.cuda.get_device_name(0), WARM, REPS, "\n".join(rows)))


if __name__ == "__main__":
    main()
