"""hipEvent ms of ONE S-stream call (dvbs2hip_set_streams) of the three block-wise tasks with a memory -- matched filter, frame synchronizer, L&R -- against the same work as
S calls on S single-stream handles that share one HIP stream (what the library offered before the entry), QPSK-S_8/9, F/S = 4 frames per stream, device forms.

Both forms run in the same process and alternate rep by rep; both are warmed up first; per form the median of `reps` (>= 5) with min and max.  The events are recorded on
the shared stream around the call(s), so the S-calls form includes the host's launch work where that is what the stream waits for.  Between reps every handle is
synchronized (outside the timed stretch: a single-stream L&R call in its one-launch form is looked at then, not inside the next timed call).  At S = 1 the two forms are a
handle that called set_streams(1) and one that never did.
usage: python tools/bench_streams.py [--reps 7] [--streams 1,8,64,512] [--commit TEXT] [--out results/streams/README.md]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

MODCOD, FS = "QPSK-S_8/9", 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", default="1,8,64,512")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    import torch
    from helpers import make_pl_frames, rot
    from oracle import oracle as O
    from dvbs2_amd.receiver import Dvbs2Hip
    O.build()
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    _, pl, _, _ = make_pl_frames(O, MODCOD, FS, 9.0, seed=3)
    n = pl.shape[1] // 2
    rng = np.random.default_rng(4)
    base = {"filter": rng.standard_normal((FS, 4 * n)).astype(np.float32),                    # two samples per symbol
            "frame sync": np.concatenate([np.zeros(2 * 321, np.float32), pl.reshape(-1)])[:FS * 2 * n].reshape(FS, 2 * n),
            "L&R": np.stack([rot(O, pl[f], 1e-4, 0.1 * f) for f in range(FS)])}
    Ss = [int(s) for s in a.streams.split(",")]
    singles = [Dvbs2Hip(MODCOD, max_frames=FS, stream=ts.cuda_stream) for _ in range(max(Ss))]
    rows = []
    for S in Ss:
        F = S * FS
        multi = Dvbs2Hip(MODCOD, max_frames=F, stream=ts.cuda_stream)
        multi.set_streams(S)
        for task in ("filter", "frame sync", "L&R"):
            per = base[task].shape[1]
            X = torch.from_numpy(base[task]).to(dev).reshape(1, -1).repeat(S, 1).reshape(F, per).contiguous()
            Y = torch.empty_like(X)
            DEL = torch.empty(F, dtype=torch.int32, device=dev)
            FLG = torch.empty(F, dtype=torch.int32, device=dev)
            TRI = torch.empty(2 * F, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()

            def call(h, f0, nf):
                x, y = X[f0:f0 + nf].data_ptr(), Y[f0:f0 + nf].data_ptr()
                if task == "filter":
                    h.filter_dev(x, y, per // 2, nf)
                elif task == "frame sync":
                    h.sync_frame_synchronize_dev(x, DEL[f0:].data_ptr(), FLG[f0:].data_ptr(), TRI[f0:].data_ptr(), y, nf)
                else:
                    h._chk(h.L.dvbs2hip_sync_lr_synchronize_dev(h.h, x, TRI[f0:].data_ptr(), TRI[F + f0:].data_ptr(), y, nf))

            def one_call():
                call(multi, 0, F)

            def s_calls():
                for s in range(S):
                    call(singles[s], s * FS, FS)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                fn()
                e1.record(ts)
                e1.synchronize()
                multi.synchronize()
                for s in range(S):
                    singles[s].synchronize()
                return e0.elapsed_time(e1)

            for fn in (one_call, s_calls, one_call, s_calls):
                timed(fn)
            ta, tb = [], []
            for _ in range(reps):
                ta.append(timed(one_call))
                tb.append(timed(s_calls))
            row = dict(task=task, S=S, frames=F, one_call_ms=[round(float(np.median(ta)), 4), round(min(ta), 4), round(max(ta), 4)],
                       s_calls_ms=[round(float(np.median(tb)), 4), round(min(tb), 4), round(max(tb), 4)], reps=reps)
            spread = row["s_calls_ms"][2] - row["s_calls_ms"][1]
            if S == 1:
                row["holds"] = bool(abs(row["one_call_ms"][0] - row["s_calls_ms"][0]) <= spread)
            else:
                row["holds"] = bool(row["one_call_ms"][0] <= row["s_calls_ms"][0] + spread)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del X, Y, DEL, FLG, TRI
        multi.close()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# Streams in the block-wise tasks: one S-stream call against S single-stream calls\n\n")
            f.write("`python tools/bench_streams.py --reps %d --streams %s`, %s, %s.\n\n" % (reps, a.streams, a.commit or "commit not given", torch.cuda.get_device_name(0)))
            f.write("%s, F/S = %d frames per stream, device forms, hipEvent ms on the one HIP stream all handles share: median (min .. max) of %d alternating reps after two "
                    "warm-up rounds of each form.  \"one call\": a handle after `dvbs2hip_set_streams(S)`.  \"S calls\": S single-stream handles, one call each.  At S = 1 "
                    "the two are a handle that called `set_streams(1)` and one that never did.\n\n" % (MODCOD, FS, reps))
            f.write("Condition at S >= 8: the one call's median is no longer than the S calls' median plus their own min-max spread.  Condition at S = 1: the two medians differ "
                    "by no more than the spread of the handle that never called the entry.\n\n")
            f.write("| task | S | frames | one call, ms | S calls, ms | S calls / one call | condition |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                o, c = r["one_call_ms"], r["s_calls_ms"]
                f.write("| %s | %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %s |\n"
                        % (r["task"], r["S"], r["frames"], o[0], o[1], o[2], c[0], c[1], c[2], c[0] / o[0], "holds" if r["holds"] else "FAILS"))
    for h in singles:
        h.close()


if __name__ == "__main__":
    main()
