"""hipEvent ms per step_mf synchronize + extract (the coarse-frequency loop, k_stepmf.hip) at S = 1 .. 16384 streams of QPSK-S frames, 8 frames per stream (fewer
where S * 8 would pass the handle's 65534-frame limit), the aggregate input rate, the single-thread C twin (tests/stepmf_twin.c) on the host beside it, and the wall
time of a full 150 / 150 / 200 acquisition at S = 1 through dvbs2_amd/acquire.py.  One JSON line per S, then the twin's and the acquisition's lines.

Every stream gets the same received signal (a shaped QPSK-S 8/9 stream with pilots, 0.05 cycles per sample off, delayed by 4.5, noisy, made once on the host and tiled on
the device); the loop's work does not depend on the data.  Per S: one warm-up call, then `reps` timed calls, median.
--kernel LANE | WAVE chooses the loop's form (dvbs2hip_sync_step_mf_set_kernel; k_stepmf_wave.hip is WAVE), for the timed calls and for the acquisition alike.
usage: python tools/bench_stepmf.py [--reps 5] [--streams 1,64,1024,4096,16384] [--kernel LANE] [--out results/coarse/bench_stepmf.json]"""
import argparse
import ctypes as C
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
    ap.add_argument("--kernel", choices=["LANE", "WAVE"], default="LANE")
    ap.add_argument("--no-acquisition", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import stepmf_ref as SR
    from dvbs2_amd import lib_binding as LB
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod("QPSK-S_8/9")
    N = 2 * mc.pl_frame
    base = SR.received_stream("QPSK-S_8/9", 8, 0.05, 8.0, seed=1, off=1234, D=4.5)
    # the host twin, one thread, one stream: 8 frames per timed call, a warm-up call, then `reps` calls, median
    cpu = []
    for i in range(max(a.reps, 5) + 1):
        sm = SR.StepMf(mc.pl_frame)
        t0 = time.perf_counter()
        _, _, _, Y, B = sm.synchronize(np.zeros(8, np.int32), base)
        sm.tm.extract(Y, B)
        if i:
            cpu.append(time.perf_counter() - t0)
    cpu_s = float(np.median(cpu))
    rows = []
    dev = torch.device("cuda", 0)
    for S in [int(s) for s in a.streams.split(",")]:
        Fs = min(8, 65534 // S)
        F = S * Fs
        rx = Dvbs2Hip("QPSK-S_8/9", max_frames=F)
        rx.sync_timing_set_streams(S)
        rx.sync_step_mf_set_kernel(a.kernel)
        X = torch.from_numpy(base[:Fs]).to(dev).reshape(1, -1).repeat(S, 1).reshape(F, 2 * N).contiguous()
        Yd = torch.empty_like(X)
        Bd = torch.empty(X.shape, dtype=torch.int32, device=dev)
        M = torch.empty(3 * F, dtype=torch.float32, device=dev)
        D = torch.zeros(F, dtype=torch.int32, device=dev)
        Y2 = torch.empty((F, N), dtype=torch.float32, device=dev)
        UFW = torch.empty(F, dtype=torch.int32, device=dev)
        RDY = torch.empty(S, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m = M.data_ptr()

        def call():
            rx.sync_step_mf_synchronize_dev(D.data_ptr(), X.data_ptr(), m, m + 4 * F, m + 8 * F, Yd.data_ptr(), Bd.data_ptr(), F)
            rx.sync_timing_extract_dev(Yd.data_ptr(), Bd.data_ptr(), Y2.data_ptr(), UFW.data_ptr(), RDY.data_ptr(), F)

        call()
        rx.synchronize()
        rx.L.dvbs2hip_timing_enable(rx.h, 1)
        ms = []
        for _ in range(a.reps):
            rx.L.dvbs2hip_timing_reset(rx.h)
            call()
            tot, n = C.c_double(), C.c_int64()
            rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
            ms.append(tot.value)
        med = float(np.median(ms))
        samples = F * N
        row = dict(kernel=a.kernel, S=S, frames_per_stream=Fs, samples=samples, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                   Msamples_per_s=round(samples / med / 1e3, 2), ns_per_sample_per_stream=round(med * 1e6 / (Fs * N), 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
        rx.close()
        del X, Yd, Bd, M, D, Y2, UFW, RDY
        torch.cuda.empty_cache()
    summ = dict(cpu_twin_one_thread_ms_8_frames_median=round(cpu_s * 1e3, 2), cpu_twin_ms_min=round(min(cpu) * 1e3, 2), cpu_twin_ms_max=round(max(cpu) * 1e3, 2),
                cpu_twin_reps=len(cpu), cpu_twin_Msamples_per_s=round(8 * N / cpu_s / 1e6, 2), cpu_twin_ns_per_sample=round(cpu_s * 1e9 / (8 * N), 2),
                gpu=torch.cuda.get_device_name(0))
    print(json.dumps(summ), flush=True)
    acq = None
    if not a.no_acquisition:
        # a full acquisition at the reference's 150 / 150 / 200 frames, one stream, one frame per call, host-socket forms (what rx.py --wl-phases does): wall time
        from dvbs2_amd.acquire import acquire
        stream = SR.received_stream("QPSK-S_8/9", 560, 0.05, 8.0, seed=2, off=1234, D=4.5)
        it = iter(stream)
        rx = Dvbs2Hip("QPSK-S_8/9", max_frames=1)
        t0 = time.perf_counter()
        res = acquire(rx, lambda: next(it)[None, :], n_frames=1, smf_kernel=a.kernel)
        wall = time.perf_counter() - t0
        rx.close()
        acq = dict(kernel=a.kernel, acquisition_wall_s=round(wall, 3), frames=res["frames"], flag=res["flag"], acquired=res["acquired"], freq=res["freq"],
                   what="acquire() at S = 1, F = 1, 150 / 150 / 200, host-socket calls, PCIe copies and the Python loop included")
        print(json.dumps(acq), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(dict(kernel=a.kernel, rows=rows, summary=summ, acquisition=acq), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
