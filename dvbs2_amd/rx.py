"""`dvbs2_rx` work-alike: raw IQ file -> [--wl-phases: the waiting and learning phases on the head of the file, dvbs2_amd/acquire.py, which find the carrier offset with the
coarse frequency loop on the GPU (--wl-frames L1 L2 L3: frames of learning phases 1 to 3, default 150 150 200; --wl-wait-max: frames after which the waiting phase gives up,
default 2000); without it the offset is handed in by --coarse-freq] -> front gain stage (Multiplier_AGC, RX/main_sched.cpp:197)
-> coarse frequency shift (:198) -> matched filter (a5) -> symbol timing (--stm-type: extraction at a known phase, or FAST / ULTRA, the Gardner loop on the GPU, :202-204) -> gain stage
(main_sched.cpp:205) -> frame synchronizer (N4) -> pilot-aided phase synchronizer (N4, optional) -> fused RX chain (a7 .. a8) -> monitor against the source pattern -> sink.  It serves
files made by `dvbs2_amd.tx` / `dvbs2_amd.ch` (or by the reference's dvbs2_tx / dvbs2_ch without timing or frequency
offsets): README.md:151-169 of the reference.

  python -m dvbs2_amd.rx --src-type USER --src-path K_14232.src --rad-rx-file-path out_tx_noisy.bin -F 8 \
         --mod-cod QPSK-S_8/9 --dec-implem NMS --dec-ite 10 --snk-path /dev/null --rad-rx-no-loop
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import params as P
from .iqfile import ProcessingAborted, RadioUserBinary
from .srcfile import SinkUserBinary, load_src


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="dvbs2_rx", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mod-cod", default="QPSK-S_8/9")
    ap.add_argument("-F", "--src-fra", type=int, default=1, dest="n_frames_batch")
    ap.add_argument("--src-type", default="USER", choices=["USER", "NONE"], help="USER: count errors against the pattern file")
    ap.add_argument("--src-path", default="")
    ap.add_argument("--shp-osf", type=int, default=2, dest="osf")
    ap.add_argument("--rad-type", default="USER_BIN", choices=["USER_BIN"])
    ap.add_argument("--rad-rx-file-path", required=True)
    ap.add_argument("--rad-rx-no-loop", action="store_true")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--dec-implem", default="SPA", choices=["NMS", "MS", "SPA", "SPA_TANH", "SPA_EXACT"])    # the reference's defaults (DVBS2.cpp:135-138)
    ap.add_argument("--dec-ite", type=int, default=50)
    ap.add_argument("--dec-alpha", type=float, default=1.0)
    ap.add_argument("--dec-simd", default="", help="accepted and ignored (the GPU batches frames with -F)")
    wl = ap.add_mutually_exclusive_group()
    wl.add_argument("--no-wl-phases", action="store_true", help="accepted: the waiting / learning phases do not run unless --wl-phases asks for them")
    wl.add_argument("--wl-phases", action="store_true", help="run the reference's waiting and learning phases (main_sched.cpp:407-635) on the head of the file, then decode the rest; "
                                                             "needs --stm-type FAST, excludes --coarse-freq")
    ap.add_argument("--wl-frames", type=int, nargs=3, default=[150, 150, 200], metavar=("L1", "L2", "L3"), help="frames of learning phases 1, 2 and 3")
    ap.add_argument("--wl-wait-max", type=int, default=2000, help="frames after which the waiting phase gives up")
    ap.add_argument("--snk-path", default="", help="decoded payload of every frame, eight bits per byte (the reference's Sink_user_binary: a file sent with dvbs2_tx --src-type USER_BIN comes out as it went in)")
    ap.add_argument("--timing-offset", type=int, default=-1, help="sample index of the first symbol after the matched filter (default: two group delays)")
    ap.add_argument("--sync-fine", action="store_true", help="run the pilot-aided phase synchronizer before the chain")
    ap.add_argument("--coarse-freq", type=float, default=0.0, help="carrier offset of the received samples in cycles per sample: the coarse frequency synchronizer's task of the transmission "
                                                                   "phase (the frequency shift) with this as its loop's frozen estimate (--wl-phases runs the loop instead)")
    ap.add_argument("--stm-type", default="PERFECT", choices=["PERFECT", "FAST", "ULTRA"], help="symbol timing: PERFECT takes every osf-th sample from --timing-offset (the default here); "
                                                                                     "FAST runs the reference's Gardner loop (Synchronizer_Gardner_fast_osf2) on the GPU; "
                                                                                     "ULTRA its held form (Synchronizer_Gardner_ultra_osf2), a wave per stream")
    ap.add_argument("--stm-hold-size", type=int, default=101, help="ULTRA: samples per hold block; mu is held over all but the last four of them once the loop holds")
    ap.add_argument("--stm-learn-frames", type=int, default=None, help="ULTRA: frames the whole loop runs on every sample before it starts to hold (the reference's learning phases, "
                                                                       "then set_act(true), main_sched.cpp:655); default: the sum of --wl-frames")
    ap.add_argument("--stm-df", type=float, default=0.5 ** 0.5, help="damping factor of the Gardner loop filter")
    ap.add_argument("--stm-nbw", type=float, default=5e-5, help="normalized bandwidth of the Gardner loop filter")
    ap.add_argument("--stm-dg", type=float, default=2.0, help="detector gain of the Gardner loop filter")
    ap.add_argument("--no-agc", action="store_true", help="leave out the two gain stages of the reference's graph (front_agc on the samples, mult_agc on the symbols)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sim-stats", action="store_true", help="per-kernel-group device time at the end (the reference's --sim-stats)")
    return ap


def run(args, out=sys.stdout) -> dict:
    from .receiver import Dvbs2Hip
    mc = P.get_modcod(args.mod_cod)
    F, n, osf = args.n_frames_batch, mc.pl_frame, args.osf
    if not args.rad_rx_no_loop and not args.max_frames:
        raise ValueError("a looping input needs --max-frames")
    pattern = load_src(args.src_path, mc.K_bch) if args.src_type == "USER" and args.src_path else None
    rx = Dvbs2Hip(mc.name, max_frames=F, n_ite=args.dec_ite, alpha=args.dec_alpha, early_stop=True, implem=args.dec_implem, device=args.device)
    if args.sim_stats:
        rx.timing_enable(True)
    if args.coarse_freq:
        rx.sync_coarse_set_freq(args.coarse_freq)
    fast = args.stm_type == "FAST"
    wl = getattr(args, "wl_phases", False)
    if wl and args.coarse_freq:
        raise ValueError("--wl-phases finds the carrier offset itself: it excludes --coarse-freq")
    ultra = args.stm_type == "ULTRA"
    if wl and ultra:
        raise ValueError("--wl-phases steps FAST's detector inside the coarse-frequency loop: with --stm-type ULTRA it is not provided (use --stm-learn-frames)")
    if wl and not fast:
        raise ValueError("--wl-phases runs the Gardner loop: it needs --stm-type FAST")
    if fast or ultra:
        if osf != 2:
            raise ValueError("--stm-type %s is the Gardner loop at two samples per symbol (--shp-osf 2)" % args.stm_type)
        rx.sync_timing_set_params(args.stm_df, args.stm_nbw, args.stm_dg)
    learn = 0
    if ultra:
        rx.sync_timing_set_type("ULTRA", args.stm_hold_size)
        learn = sum(args.wl_frames) if args.stm_learn_frames is None else args.stm_learn_frames
        fast = True                                                                # the same two tasks from here on
    fed = 0                                                                        # frames the timing loop has taken
    rcv = RadioUserBinary(n * osf, input_filename=args.rad_rx_file_path, auto_reset=not args.rad_rx_no_loop, n_frames=F)
    snk = SinkUserBinary(args.snk_path, mc.K_bch) if args.snk_path else None
    off = args.timing_offset if args.timing_offset >= 0 else 2 * 20 * osf          # two group delays of grp_delay * osf samples
    tail = np.zeros((0, 2), np.float32)                                            # matched-filter samples not yet turned into symbols
    skip = off
    st = dict(frames=0, locked_frames=0, be=0, fe=0, delay=None)
    stable = 0                                                                     # frames since the synchronizer's delay last moved
    try:
        if wl:
            from .acquire import acquire
            l1, l2, l3 = args.wl_frames
            st["acquisition"] = acq = acquire(rx, rcv.receive, n_frames=F, osf=osf, learn1=l1, learn2=l2, learn3=l3, wait_max=args.wl_wait_max, agc=not args.no_agc)
            print("# waiting %d | learning %d + %d + %d frames | packet flag %s | coarse frequency %s" % (
                acq["frames"]["waiting"], acq["frames"]["learning1"], acq["frames"]["learning2"], acq["frames"]["learning3"], acq["flag"], acq["freq"]), file=out)
        while not args.max_frames or st["frames"] < args.max_frames:
            try:
                x = rcv.receive()
            except ProcessingAborted:
                break
            x = x.astype(np.float32, copy=False)
            if not args.no_agc:
                x = rx.agc(x, n_frames=F, output_energy=1.0 / osf)                  # front_agc: DVBS2.cpp:660-664
            if args.coarse_freq or wl:
                _, _, x = rx.sync_coarse_synchronize(x, n_frames=F)                  # sync_coarse_f: RX/main_sched.cpp:198-200
            if fast:
                # sync_timing: synchronize -> extract (RX/main_sched.cpp:202-204); a call that underflows holds its symbols for the next one
                if ultra and fed >= learn:
                    rx.sync_timing_set_act(True)                                     # the learning frames are over: the loop holds (calls are whole: the first one at or past N)
                y, b, _ = rx.sync_timing_synchronize(rx.filter(x, n_frames=F).reshape(F, -1))
                fed += F
                y2, _, rdy = rx.sync_timing_extract(y, b)
                if not rdy[0]:
                    continue
                sym, n_sym = y2.reshape(-1, 2), F * n
            else:
                mf = np.concatenate([tail, rx.filter(x, n_frames=F).reshape(-1, 2)])
                mf, skip = mf[skip:], 0                                            # perfect timing: every osf-th sample from `off`
                n_sym = (mf.shape[0] // osf // n) * n                              # whole frames of symbols
                if n_sym == 0:
                    tail = mf
                    continue
                sym, tail = mf[: n_sym * osf : osf], mf[n_sym * osf:]
            for b0 in range(0, n_sym // n, F):
                blk = np.ascontiguousarray(sym[b0 * n:(b0 + F) * n])
                Fb = blk.shape[0] // n
                if not args.no_agc:
                    blk = rx.agc(blk, n_frames=Fb, output_energy=1.0)                   # mult_agc: DVBS2.cpp:653-657
                delay, flags, tri, aligned = rx.sync_frame_synchronize(blk.reshape(Fb, 2 * n), with_flags=True)
                if args.sync_fine or wl:
                    # the reference's task order (src/mains/RX/main.cpp): PL descramble -> fine synchronizer -> remove PLH ->
                    # estimate -> demodulate + deinterleave -> LDPC -> BCH -> BB descramble, one C-ABI call per task
                    desc = rx.pl_descramble(aligned)
                    if wl:
                        _, _, desc = rx.sync_lr_synchronize(desc)                     # what the frozen coarse estimate leaves: L&R, as learning phase 3 has trained it (main_sched.cpp:208)
                    _, _, fixed = rx.sync_freq_phase_synchronize(desc)
                    xf = rx.remove_plh(fixed)
                    sig, _, _ = rx.estimate(xf)
                    vk, _ = rx.decode_siho(rx.demodulate(sig, xf, deinterleave=True))
                    bits = rx.bb_descramble(rx.decode_hiho(vk)[0])
                else:
                    bits, _, _ = rx.rx_bb(aligned)
                for f in range(Fb):
                    st["frames"] += 1
                    stable = stable + 1 if st["delay"] is not None and delay[f] == st["delay"] else 0
                    locked = stable >= 2                                           # the delay line has settled on this alignment
                    st["delay"] = int(delay[f])
                    if snk:
                        snk.send(bits[f])
                    if pattern is not None and locked:
                        e = min(int((bits[f] != p).sum()) for p in pattern)
                        st["locked_frames"] += 1; st["be"] += e; st["fe"] += e > 0
    finally:
        if args.sim_stats:
            from .sim import print_stats
            print_stats([rx], out)
        rx.close(); rcv.close()
        if snk:
            snk.close()
    st["ber"] = st["be"] / max(1, st["locked_frames"] * mc.K_bch)
    st["fer"] = st["fe"] / max(1, st["locked_frames"])
    print("# frames %(frames)d | in lock %(locked_frames)d | BE %(be)d | FE %(fe)d | BER %(ber).2e | FER %(fer).2e | delay %(delay)s" % st, file=out)
    return st


if __name__ == "__main__":
    run(build_parser().parse_args())
