"""hipEvent ms of dvbs2hip_sync_timing_synchronize_dev alone, FAST (a lane per stream) against ULTRA (a wave per stream: act on at two hold sizes, act off), in ONE process on
one device: S = 1, 64, 1024 streams of 8 QPSK-S frames each, one warm-up call per variant, then `reps` timed calls, median / min / max.  One JSON line per (S, variant), then
the ratios FAST / ULTRA per S with the spread of both.  Every stream gets the same matched-filter signal (a shaped, delayed, noisy QPSK stream made once on the host); ULTRA's
warm-up call runs with act off, as a receiver's learning frames do, before act is set.
usage: python tools/bench_timing_ultra.py [--reps 5] [--streams 1,64,1024] [--hold-sizes 101,1001] [--out results/timing_ultra/bench_timing_ultra.json]"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", default="1,64,1024")
    ap.add_argument("--hold-sizes", default="101,1001")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import timing_ref as TR
    from dvbs2_amd import lib_binding as LB
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    mc = P.get_modcod("QPSK-S_8/9")
    N, Fs = 2 * mc.pl_frame, 8
    base = TR.shaped_stream(Fs * N, np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), 4.5, 0.05, np.random.default_rng(1)).reshape(Fs, 2 * N)
    holds = [int(h) for h in a.hold_sizes.split(",")]
    variants = [("FAST", None, False)] + [("ULTRA", h, True) for h in holds] + [("ULTRA", holds[0], False)]
    dev = torch.device("cuda", 0)
    rows = []
    for S in [int(s) for s in a.streams.split(",")]:
        F = S * Fs
        X = torch.from_numpy(base).to(dev).reshape(1, -1).repeat(S, 1).reshape(F, 2 * N).contiguous()
        Yd = torch.empty_like(X)
        Bd = torch.empty(X.shape, dtype=torch.int32, device=dev)
        MU = torch.empty(F, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for stm_type, hold, act in variants:
            rx = Dvbs2Hip("QPSK-S_8/9", max_frames=F)
            rx.sync_timing_set_streams(S)
            if stm_type == "ULTRA":
                rx.sync_timing_set_type("ULTRA", hold)
            call = lambda: rx.sync_timing_synchronize_dev(X.data_ptr(), Yd.data_ptr(), Bd.data_ptr(), MU.data_ptr(), F)
            call()                                                      # warm-up: the learning frames (act off)
            rx.synchronize()
            rx.sync_timing_set_act(act)
            rx.L.dvbs2hip_timing_enable(rx.h, 1)
            ms = []
            for _ in range(a.reps):
                rx.L.dvbs2hip_timing_reset(rx.h)
                call()
                tot, n = C.c_double(), C.c_int64()
                rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
                ms.append(tot.value)
            med = float(np.median(ms))
            strobes = float(Bd[:, 0::2].float().mean().item())
            row = dict(S=S, stm_type=stm_type, hold_size=hold, act=bool(act), frames_per_stream=Fs, samples=F * N, ms_median=round(med, 4), ms_min=round(min(ms), 4),
                       ms_max=round(max(ms), 4), ms_all=[round(m, 4) for m in ms], ns_per_sample_per_stream=round(med * 1e6 / (Fs * N), 2),
                       Msamples_per_s=round(F * N / med / 1e3, 2), strobe_fraction=round(strobes, 4), mu_last=round(float(MU[-1].item()), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
            rx.close()
        del X, Yd, Bd, MU
        torch.cuda.empty_cache()
    ratios = []
    for S in sorted({r["S"] for r in rows}):
        fast = next(r for r in rows if r["S"] == S and r["stm_type"] == "FAST")
        for r in rows:
            if r["S"] == S and r["stm_type"] == "ULTRA":
                ratios.append(dict(S=S, hold_size=r["hold_size"], act=r["act"], fast_over_ultra_median=round(fast["ms_median"] / r["ms_median"], 3),
                                   fast_min_over_ultra_max=round(fast["ms_min"] / r["ms_max"], 3)))       # the ratio with the five samples' spread against ULTRA
    summ = dict(ratios=ratios, gpu=torch.cuda.get_device_name(0), reps=a.reps)
    print(json.dumps(summ), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(dict(rows=rows, summary=summ), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
