"""hipEvent ms per synchronize + extract of the timing synchronizer (Gardner, osf 2) at S = 1 .. 16384 streams of QPSK-S frames, the aggregate input rate, and the
single-thread C twin (tests/timing_twin.c) on the host beside it (64 frames per timed call, median of at least 5).  One JSON line per S, then a summary line.

Every stream gets the same matched-filter signal (a shaped, delayed, noisy QPSK stream made once on the host and tiled on the device); the loop's work does not
depend on the data.  Frames per stream: 8, fewer where S * 8 would pass the handle's 65534-frame limit.  Per S: one warm-up call, then `reps` timed calls, median.
usage: python tools/bench_timing.py [--reps 5] [--streams 1,64,1024,4096,16384] [--out results/...json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", default="1,64,1024,4096,16384")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import timing_ref as TR
    from dvbs2_amd import lib_binding as LB
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod("QPSK-S_8/9")
    N = 2 * mc.pl_frame
    base = TR.shaped_stream(8 * N, np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), 4.5, 0.05, np.random.default_rng(1)).reshape(8, 2 * N)
    # the host twin, one thread, one stream: 64 frames (1.07 M samples) per timed call, a warm-up call, then `reps` calls, median
    big = np.tile(base, (8, 1))
    tw = TR.Timing(mc.pl_frame)
    Y, B, _ = tw.synchronize(big)
    tw.extract(Y, B)
    cpu = []
    for _ in range(max(a.reps, 5)):
        tw.reset()
        t0 = time.perf_counter()
        Y, B, _ = tw.synchronize(big)
        tw.extract(Y, B)
        cpu.append(time.perf_counter() - t0)
    cpu_s = float(np.median(cpu))
    rows = []
    for S in [int(s) for s in a.streams.split(",")]:
        Fs = min(8, 65534 // S)
        F = S * Fs
        rx = Dvbs2Hip("QPSK-S_8/9", max_frames=F)
        rx.sync_timing_set_streams(S)
        dev = torch.device("cuda", 0)
        X = torch.from_numpy(base[:Fs]).to(dev).reshape(1, -1).repeat(S, 1).reshape(F, 2 * N).contiguous()
        Yd = torch.empty_like(X)
        Bd = torch.empty(X.shape, dtype=torch.int32, device=dev)
        MU = torch.empty(F, dtype=torch.float32, device=dev)
        Y2 = torch.empty((F, N), dtype=torch.float32, device=dev)
        UFW = torch.empty(F, dtype=torch.int32, device=dev)
        RDY = torch.empty(S, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            rx.sync_timing_synchronize_dev(X.data_ptr(), Yd.data_ptr(), Bd.data_ptr(), MU.data_ptr(), F)
            rx.sync_timing_extract_dev(Yd.data_ptr(), Bd.data_ptr(), Y2.data_ptr(), UFW.data_ptr(), RDY.data_ptr(), F)

        call()
        rx.synchronize()
        rx.L.dvbs2hip_timing_enable(rx.h, 1)
        ms = []
        for _ in range(a.reps):
            rx.L.dvbs2hip_timing_reset(rx.h)
            call()
            import ctypes as C
            tot, n = C.c_double(), C.c_int64()
            rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
            ms.append(tot.value)
        med = float(np.median(ms))
        samples = F * N
        row = dict(S=S, frames_per_stream=Fs, samples=samples, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                   Msamples_per_s=round(samples / med / 1e3, 2), ns_per_sample_per_stream=round(med * 1e6 / (Fs * N), 2),
                   ready_streams=int(RDY.sum().item()))
        print(json.dumps(row), flush=True)
        rows.append(row)
        rx.close()
        del X, Yd, Bd, MU, Y2, UFW, RDY
        torch.cuda.empty_cache()
    summ = dict(cpu_twin_one_thread_ms_64_frames_median=round(cpu_s * 1e3, 2), cpu_twin_ms_min=round(min(cpu) * 1e3, 2), cpu_twin_ms_max=round(max(cpu) * 1e3, 2),
                cpu_twin_reps=len(cpu), cpu_twin_Msamples_per_s=round(64 * N / cpu_s / 1e6, 2), cpu_twin_ns_per_sample=round(cpu_s * 1e9 / (64 * N), 2),
                gpu=torch.cuda.get_device_name(0))
    print(json.dumps(summ), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(dict(rows=rows, summary=summ), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
