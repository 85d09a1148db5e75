"""Time of the BBFRAME layer, in ONE process on one device, the candidates alternated sample by sample: QPSK-S_8/9 at 4096 frames, QPSK-N_8/9 at 1024.
 (a) device forms, hipEvent pairs of the handle around every call: dvbs2hip_bbframe_parse_dev (its three launches together) and dvbs2hip_bbframe_build_dev against
     dvbs2hip_bb_descramble_dev on the same frames -- the existing call that streams the same 4 K_bch bytes per frame in, and as many out.
 (b) host forms, host clock around calls that end in a synchronise: dvbs2hip_rx_bb against dvbs2hip_rx_bb_up on the same PL frames (pageable host memory): the difference
     is the device-to-host copy of 4 K_bch bytes per frame that rx_bb_up does not make.
Each sample is `inner` calls after a warm-up of every call; median / min / max over `reps` samples.  There is no bar.
usage: python tools/bench_bbframe.py [--reps 5] [--inner 10] [--out-dir results/bbframe]      -> <out-dir>/bench.json, <out-dir>/README.md"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np

CONFIGS = [("QPSK-S_8/9", 4096), ("QPSK-N_8/9", 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-inner", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "results", "bbframe"))
    a = ap.parse_args()
    import torch
    from dvbs2_amd import lib_binding as LB
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_bbframe.py needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    rows, host_rows = [], []
    for modcod, F in CONFIGS:
        rx = Dvbs2Hip(modcod, max_frames=F, n_ite=10, implem="NMS")
        mc = P.get_modcod(modcod)
        K, D = rx.K_bch, (rx.K_bch - 80) // 8
        stream = np.random.default_rng(7).integers(0, 256, F * D, dtype=np.uint8)
        d_stream = torch.from_numpy(stream).to(dev)
        bits, scr = torch.empty((F, K), dtype=torch.int32, device=dev), torch.empty((F, K), dtype=torch.int32, device=dev)
        cap = rx.bbframe_max_packets(F)
        UP, ST = torch.empty(cap * 188, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
        N, HDR = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty((F, 8), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        calls = {
            "bb_descramble_dev": lambda: rx._chk(rx.L.dvbs2hip_bb_descramble_dev(rx.h, C.c_void_p(bits.data_ptr()), C.c_void_p(scr.data_ptr()), F)),
            "bbframe_parse_dev": lambda: rx.bbframe_parse_dev(bits.data_ptr(), None, UP.data_ptr(), ST.data_ptr(), N.data_ptr(), HDR.data_ptr(), F),
            "bbframe_build_dev": lambda: rx.bbframe_build_dev(d_stream.data_ptr(), stream.size, bits.data_ptr(), F),
        }
        rx.bbframe_reset()
        for c in ("bbframe_build_dev", "bb_descramble_dev", "bbframe_parse_dev"):        # warm-up; `bits` now holds BBFRAMEs
            calls[c]()
        rx.synchronize()
        assert int(N.item()) == (F * D - 1) // 188 and not bool(ST[:int(N.item())].any()), "the parser does not return the packets the builder sent"
        rx.timing_enable(True)
        samples = {c: [] for c in calls}
        for _ in range(a.reps):
            for c in ("bb_descramble_dev", "bbframe_parse_dev", "bbframe_build_dev"):    # alternated: one sample of each per round (build last: it leaves `bits` a BBFRAME stream)
                rx.timing_reset()
                for _ in range(a.inner):
                    calls[c]()
                tot, n = C.c_double(), C.c_int64()
                rx._chk(rx.L.dvbs2hip_timing_get(rx.h, LB.K_MISC, C.byref(tot), C.byref(n)))
                samples[c].append(tot.value / a.inner)
        rx.timing_enable(False)
        for c, ms in samples.items():
            wr = {"bb_descramble_dev": 4 * K * F, "bbframe_parse_dev": cap * 189 + 32 * F, "bbframe_build_dev": 4 * K * F}[c]
            rd = {"bb_descramble_dev": 4 * K * F, "bbframe_parse_dev": 4 * K * F, "bbframe_build_dev": stream.size}[c]
            med = float(np.median(ms))
            row = dict(modcod=modcod, frames=F, call=c, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), ms_all=[round(m, 4) for m in ms],
                       MB_read=round(rd / 1e6, 1), MB_written=round(wr / 1e6, 1), GBps=round((rd + wr) / med / 1e6, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
        # (b) host forms on the same PL frames
        sigma = P.esn0_to_sigma(P.ebn0_to_esn0(8.0, mc.K_bch / mc.N_ldpc, mc.bps))
        _, pl = rx.tx_bb(F, info=bits.cpu().numpy(), seed=3, sigma=sigma)
        host = {"rx_bb": lambda: rx.rx_bb(pl, sigma=sigma), "rx_bb_up": lambda: rx.rx_bb_up(pl, sigma=sigma)}
        rx.bbframe_reset()
        info = host["rx_bb"]()[0]
        pk = host["rx_bb_up"]()[0]
        rx.bbframe_reset()
        assert np.array_equal(pk, rx.bbframe_parse(info)[0]), "rx_bb_up and bbframe_parse(rx_bb) differ"      # the two calls that are timed return the same packets
        be = int((info != bits.cpu().numpy()).sum())                                                          # (of the channel and the decoder, not of this layer)
        hs = {c: [] for c in host}
        for _ in range(a.reps):
            for c in host:
                t0 = time.perf_counter()
                for _ in range(a.host_inner):
                    host[c]()
                hs[c].append((time.perf_counter() - t0) * 1e3 / a.host_inner)
        for c, ms in hs.items():
            back = 4 * K * F + 2 * F if c == "rx_bb" else cap * 189 + 34 * F + 4
            row = dict(modcod=modcod, frames=F, call=c, ms_median=round(float(np.median(ms)), 2), ms_min=round(min(ms), 2), ms_max=round(max(ms), 2), MB_device_to_host=round(back / 1e6, 2),
                       packets=len(pk), bit_errors=be)
            print(json.dumps(row), flush=True)
            host_rows.append(row)
        rx.close()
        del bits, scr, UP, ST, HDR, d_stream, pl
        torch.cuda.empty_cache()
    summ = dict(gpu=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, host_inner=a.host_inner)
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(dict(device=rows, host=host_rows, summary=summ), open(os.path.join(a.out_dir, "bench.json"), "w"), indent=1)
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("# BBFRAME layer: time of the device and the host forms\n\n")
        f.write("Written by `python tools/bench_bbframe.py --reps %d --inner %d --host-inner %d` (%s), one process, the calls alternated sample by sample.\n\n" % (a.reps, a.inner, a.host_inner, summ["gpu"]))
        f.write("## (a) device forms\n\nhipEvent pairs of the handle around every call (`bbframe_parse_dev`: around its three launches together), median of %d samples of %d calls "
                "after a warm-up.  `bb_descramble_dev` is the comparison: it reads the same 4 K_bch bytes per frame and writes as many.\n\n" % (a.reps, a.inner))
        f.write("| MODCOD | frames | call | median ms | min .. max ms | MB read | MB written | GB/s |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %s | %.4f | %.4f .. %.4f | %.1f | %.1f | %.0f |\n" % (r["modcod"], r["frames"], r["call"], r["ms_median"], r["ms_min"], r["ms_max"], r["MB_read"], r["MB_written"], r["GBps"]))
        f.write("\n## (b) host forms\n\nHost clock around %d calls (each ends in a synchronise), pageable host memory, the same PL frames at Eb/N0 = 8 dB, NMS with 10 iterations.\n\n" % a.host_inner)
        f.write("`packets`: what one `rx_bb_up` call from reset returns, equal to `bbframe_parse` of `rx_bb`'s bits; `bit errors`: `rx_bb`'s bits against the sent ones (the channel's and the "
                "decoder's, counted so that the packet count can be read against them).\n\n")
        f.write("| MODCOD | frames | call | median ms | min .. max ms | MB device to host | packets | bit errors |\n|---|---|---|---|---|---|---|---|\n")
        for r in host_rows:
            f.write("| %s | %d | %s | %.2f | %.2f .. %.2f | %.2f | %d | %d |\n" % (r["modcod"], r["frames"], r["call"], r["ms_median"], r["ms_min"], r["ms_max"], r["MB_device_to_host"],
                                                                                 r["packets"], r["bit_errors"]))


if __name__ == "__main__":
    main()
