"""hipEvent time of each of the seven TX tasks alone (the `_dev` entries dvbs2hip_bb_scramble_dev .. dvbs2hip_pl_scramble_dev, the handle's own event pair around every call), in ONE process
on one device: QPSK-S_8/9 and 32APSK-S_3/4 at 4096 frames, QPSK-N_8/9 at 1024.  Per MODCOD the chain runs once on a seeded random payload (warm-up of every kernel, and it fills the
sockets every task is then timed on); each task is timed `reps` times, `inner` calls per sample, median / min / max of the per-call time.  In the same run: the time the task's socket
bytes (input read once + output written once) would take at the rate of the library's streaming copy kernel (dvbs2hip_device_copy_bandwidth), and the fused dvbs2hip_tx_bb_dev at the same
batch.  There is no bar; the ratio to the copy-rate time says how far a task is from a pure streaming pass.
usage: python tools/bench_tx_tasks.py [--reps 5] [--inner 10] [--out-dir results/tx_tasks]      -> <out-dir>/bench.json, <out-dir>/README.md"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np

CONFIGS = [("QPSK-S_8/9", 4096), ("32APSK-S_3/4", 4096), ("QPSK-N_8/9", 1024)]
TASKS = ["bb_scramble", "bch_encode", "ldpc_encode", "interleave", "modulate", "framer_generate", "pl_scramble"]
# what a task that is not a pure streaming pass waits for (printed for the tasks whose ratio to the copy-rate time is above 2)
WAITS = {
    "bb_scramble": "4 bytes per lane in and out (the kernel dvbs2hip_bb_descramble uses, unchanged): the memory pipeline's request rate, not its bandwidth.",
    "bch_encode": "the parity launch: a dependent chain of LDS table look-ups, a byte of the message per step and 16 lanes per frame (tx_bch_remainder) -- latency of the division, "
                  "as in the fused TX's tx_bchpar_kernel; the pack-and-copy launch in front of it is a streaming pass.",
    "ldpc_encode": "one 6-wave workgroup per frame with three barriers: packing into LDS, the parity rows (funnel shifts out of LDS) and the output are phases that do not overlap inside a "
                   "workgroup, and the output phase takes one bit per LDS read; the loads of a frame are not in flight while its rows are formed.",
    "interleave": "the column/row gather: four 4-byte loads per lane at the stride of the column count, so a wave's load instruction touches `cols` times the cache lines of a contiguous one.",
    "modulate": "2 bps separate 4-byte loads per lane (a lane's bits are contiguous, its neighbours' are 8 bps bytes apart) and the constellation look-up in LDS.",
    "framer_generate": "(a streaming pass with an index map)",
    "pl_scramble": "(a streaming pass; the sequence is one byte per symbol on top)",
}


def task_bytes(rx, name):
    """socket bytes of one frame: (read, written)"""
    b, s = 4, 8
    return {"bb_scramble": (rx.K_bch * b, rx.K_bch * b), "bch_encode": (rx.K_bch * b, rx.K_ldpc * b), "ldpc_encode": (rx.K_ldpc * b, rx.N_ldpc * b),
            "interleave": (rx.N_ldpc * b, rx.N_ldpc * b), "modulate": (rx.N_ldpc * b, rx.N_xfec * s), "framer_generate": (rx.N_xfec * s, rx.pl_frame * s),
            "pl_scramble": (rx.pl_frame * s, rx.pl_frame * s)}[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "results", "tx_tasks"))
    a = ap.parse_args()
    import torch
    from dvbs2_amd import lib_binding as LB
    from dvbs2_amd.receiver import Dvbs2Hip
    from dvbs2_amd.tx import TxTasks
    if not torch.cuda.is_available():
        raise SystemExit("bench_tx_tasks.py needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)

    def timed(rx, call):
        """-> per-call ms samples: `reps` samples of `inner` calls each, after one warm-up call"""
        call(); rx.synchronize()
        out = []
        for _ in range(a.reps):
            rx.timing_reset()
            for _ in range(a.inner):
                call()
            tot, n = C.c_double(), C.c_int64()
            rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
            out.append(tot.value / a.inner)
        return out

    rows, fused_rows = [], []
    copy_GBps = None
    for modcod, F in CONFIGS:
        rx = Dvbs2Hip(modcod, max_frames=F)
        if copy_GBps is None:
            copy_GBps = rx.device_copy_GBps(1 << 28, 10)
        t = TxTasks(rx, F)
        info = torch.from_numpy(np.random.default_rng(7).integers(0, 2, (F, rx.K_bch)).astype(np.int32)).to(dev)
        sent = torch.empty_like(info)
        fused = torch.empty_like(t.pl)
        torch.cuda.synchronize()
        t.run_dev(info); rx.synchronize()                      # every socket now holds its stage's output
        rx.tx_bb_dev(info.data_ptr(), 0, None, sent.data_ptr(), fused.data_ptr(), F); rx.synchronize()
        assert torch.equal(fused, t.pl), "the seven tasks and the fused tx_bb differ"
        rx.timing_enable(True)
        socks = [info, t.scr, t.bch, t.cw, t.itl, t.sym, t.plf, t.pl]
        total = 0.0
        for k, name in enumerate(TASKS):
            fn = getattr(rx, name + "_dev")
            ms = timed(rx, lambda: fn(socks[k].data_ptr(), socks[k + 1].data_ptr(), F))
            rd, wr = task_bytes(rx, name)
            nbytes = (rd + wr) * F
            med = float(np.median(ms))
            copy_ms = nbytes / (copy_GBps * 1e9) * 1e3
            row = dict(modcod=modcod, frames=F, task=name, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), ms_all=[round(m, 4) for m in ms],
                       socket_MB=round(nbytes / 1e6, 1), copy_rate_ms=round(copy_ms, 4), ratio_to_copy=round(med / copy_ms, 2), GBps=round(nbytes / med / 1e6, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
            total += med
        ms = timed(rx, lambda: rx.tx_bb_dev(info.data_ptr(), 0, None, sent.data_ptr(), fused.data_ptr(), F))
        med = float(np.median(ms))
        fr = dict(modcod=modcod, frames=F, tx_bb_ms_median=round(med, 4), tx_bb_ms_min=round(min(ms), 4), tx_bb_ms_max=round(max(ms), 4), tasks_ms_sum_of_medians=round(total, 4),
                  tasks_over_tx_bb=round(total / med, 2))
        print(json.dumps(fr), flush=True)
        fused_rows.append(fr)
        rx.close()
        del t, info, sent, fused, socks
        torch.cuda.empty_cache()
    summ = dict(gpu=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, copy_GBps_read_plus_written=round(copy_GBps, 1))
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(dict(tasks=rows, fused=fused_rows, summary=summ), open(os.path.join(a.out_dir, "bench.json"), "w"), indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("# TX tasks at the task boundary: time of each `_dev` entry alone\n\n")
        f.write("Written by `tools/bench_tx_tasks.py` (%s; hipEvent pairs of the handle around every call, median of %d samples of %d calls after a warm-up, "
                "spread = min .. max of the samples).  `copy-rate ms` is the time the task's socket bytes (input read once, output written once) take at the %.0f GB/s "
                "(read + written) that `dvbs2hip_device_copy_bandwidth` measured in the same run; `ratio` = median / copy-rate ms.  There is no bar: nobody has measured "
                "these kernels before.\n\n" % (summ["gpu"], a.reps, a.inner, copy_GBps))
        f.write("| MODCOD | frames | task | median ms | min .. max ms | socket MB | copy-rate ms | ratio | GB/s |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %s | %.4f | %.4f .. %.4f | %.1f | %.4f | %.2f | %.0f |\n" % (r["modcod"], r["frames"], r["task"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                                          r["socket_MB"], r["copy_rate_ms"], r["ratio_to_copy"], r["GBps"]))
        f.write("\nThe seven tasks against the fused `dvbs2hip_tx_bb_dev` (no noise, the same payload, the same batch).  The tasks move 32 times the bits -- an int32 per bit where the "
                "fused kernels keep packed words between their stages -- so the sum is the slower; that is the price of the task boundary, not a defect.\n\n")
        f.write("| MODCOD | frames | tx_bb median ms | min .. max ms | seven tasks, sum of medians ms | tasks / tx_bb |\n|---|---|---|---|---|---|\n")
        for r in fused_rows:
            f.write("| %s | %d | %.4f | %.4f .. %.4f | %.4f | %.2f |\n" % (r["modcod"], r["frames"], r["tx_bb_ms_median"], r["tx_bb_ms_min"], r["tx_bb_ms_max"],
                                                                        r["tasks_ms_sum_of_medians"], r["tasks_over_tx_bb"]))
        over = sorted({r["task"] for r in rows if r["ratio_to_copy"] > 2}, key=TASKS.index)
        f.write("\n## Tasks above twice their copy-rate time, and what they wait for\n\n")
        for name in over:
            worst = max(r["ratio_to_copy"] for r in rows if r["task"] == name)
            f.write("- `%s` (up to %.2f): %s\n" % (name, worst, WAITS[name]))
        if not over:
            f.write("None.\n")


if __name__ == "__main__":
    main()
