"""`dvbs2_rx` work-alike: raw IQ file -> [--wl-phases: the waiting and learning phases on the head of the file, dvbs2_amd/acquire.py, which find the carrier offset with the
coarse frequency loop on the GPU (--wl-frames L1 L2 L3: frames of learning phases 1 to 3, default 150 150 200; --wl-wait-max: frames after which the waiting phase gives up,
default 2000); without it the offset is handed in by --coarse-freq] -> front gain stage (Multiplier_AGC, RX/main_sched.cpp:197)
-> coarse frequency shift (:198) -> matched filter (a5) -> symbol timing (--stm-type: extraction at a known phase, or FAST / ULTRA, the Gardner loop on the GPU, :202-204) -> gain stage
(main_sched.cpp:205) -> frame synchronizer (N4) -> pilot-aided phase synchronizer (N4, optional) -> fused RX chain (a7 .. a8) -> monitor against the source pattern -> sink.  It serves
files made by `dvbs2_amd.tx` / `dvbs2_amd.ch` (or by the reference's dvbs2_tx / dvbs2_ch without timing or frequency
offsets): README.md:151-169 of the reference.

  python -m dvbs2_amd.rx --src-type USER --src-path K_14232.src --rad-rx-file-path out_tx_noisy.bin -F 8 \
         --mod-cod QPSK-S_8/9 --dec-implem NMS --dec-ite 10 --snk-path /dev/null --rad-rx-no-loop

--mod-cod VCM (an extension): variable coding and modulation -- the MODCOD changes from frame to frame (dvbs2_tx --mod-cod-seq).  The symbols go to vcm.VcmReceiver, which
follows the PLHEADERs from frame to frame and decodes each frame as its header says; --snk-path gets every decoded frame's bits in stream order, one line sums up.  Pilots
on, no --wl-phases, --sync-fine, --snk-type TS, --src-type USER or --pls-check.

--mod-cod AUTO (an extension): the MODCOD is read from the PLHEADERs of the head of the file first (detect(): a probe handle, the same front tasks, dvbs2hip_pls_search), one
line says what was found, and the run goes on as with that MODCOD named.  Constant coding and modulation, pilots on, no --wl-phases.
"""
from __future__ import annotations

import argparse
import collections
import sys

import numpy as np

from . import params as P
from .iqfile import ProcessingAborted, RadioUserBinary
from .rx_sequence import LockTracker, RxSequence, add_timing_args
from .srcfile import SinkTS, SinkUserBinary, load_src


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="dvbs2_rx", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mod-cod", default="QPSK-S_8/9", help="a MODCOD of the table, or AUTO (an extension): read it from the PLHEADERs of the head of the file (constant coding and "
                                                            "modulation, pilots on; excludes --wl-phases), or VCM (an extension): follow the PLHEADERs from frame to frame and "
                                                            "decode every frame by its own MODCOD")
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
    ap.add_argument("--smf-kernel", choices=["LANE", "WAVE"], default=None, help="with --wl-phases: the form of the coarse-frequency loop (LANE: one lane per stream, the library's "
                                                                                 "default; WAVE: one wave per stream, the faster one here; the same results); default: not set")
    ap.add_argument("--snk-path", default="", help="decoded payload of every frame, eight bits per byte (the reference's Sink_user_binary: a file sent with dvbs2_tx --src-type USER_BIN comes out as it went in)")
    ap.add_argument("--snk-type", default="BITS", choices=["BITS", "TS"], help="BITS: --snk-path gets every frame's K_bch bits; TS (an extension): the frames are DVB-S2 BBFRAMEs (dvbs2_tx --src-type TS) "
                                                                               "and --snk-path gets the transport packets of the frames whose BBHEADER checks -- nothing before the lock, nothing of a broken frame")
    ap.add_argument("--timing-offset", type=int, default=-1, help="sample index of the first symbol after the matched filter (default: two group delays)")
    ap.add_argument("--sync-fine", action="store_true", help="run the pilot-aided phase synchronizer before the chain")
    ap.add_argument("--est-type", default="DVBS2", choices=["DVBS2", "PILOTS"], help="the noise estimator: DVBS2 is the reference's M2M4 (biased low on 16APSK and 32APSK: it takes every point to have "
                                                                                    "the same modulus), PILOTS the data-aided one on the frames' header and pilot symbols")
    ap.add_argument("--pls-check", action="store_true", help="decode the PLHEADER of every aligned frame (MODCOD, frame type, pilots) and count the frames in lock whose value is not "
                                                              "the one of --mod-cod; a stream of another MODCOD stops the run once 16 frames in lock have been seen and most of them differ")
    ap.add_argument("--coarse-freq", type=float, default=0.0, help="carrier offset of the received samples in cycles per sample: the coarse frequency synchronizer's task of the transmission "
                                                                   "phase (the frequency shift) with this as its loop's frozen estimate (--wl-phases runs the loop instead)")
    add_timing_args(ap, learn_default=None)
    ap.add_argument("--stm-df", type=float, default=0.5 ** 0.5, help="damping factor of the Gardner loop filter")
    ap.add_argument("--stm-nbw", type=float, default=5e-5, help="normalized bandwidth of the Gardner loop filter")
    ap.add_argument("--stm-dg", type=float, default=2.0, help="detector gain of the Gardner loop filter")
    ap.add_argument("--no-agc", action="store_true", help="leave out the two gain stages of the reference's graph (front_agc on the samples, mult_agc on the symbols)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sim-stats", action="store_true", help="per-kernel-group device time at the end (the reference's --sim-stats)")
    return ap


def _pls_text(v):
    """a decoded PLS value for a message: `QPSK-S_3/5 (PLS 23, pilots on)`, or the value alone when the table has no MODCOD for it"""
    name, pilots = P.pls_name(v)
    return "%s (PLS %d, pilots %s)" % (name, v, "on" if pilots else "off") if name else "PLS %d, pilots %s" % (v, "on" if pilots else "off")


AUTO_SYMBOLS = 2 * 33282 + 90      # --mod-cod AUTO searches at least this many symbols (or what the file holds): two frames of the longest MODCOD and a header


def detect(args, out=sys.stdout) -> dict:
    """--mod-cod AUTO: what the stream is and where its frames start, from the PLHEADERs of the head of the file.  A probe handle (any MODCOD: no task in front of the frame
    synchronizer depends on it) takes the samples through RxSequence.front and RxSequence.symbols as the run itself would, the symbols go through pls_search, and
    params.find_modcod accepts the result or not -> dict(modcod, value, pilots, offset, count, slots, score, symbols); ValueError when no chain of headers is found"""
    from .receiver import Dvbs2Hip
    if getattr(args, "wl_phases", False):
        raise ValueError("--mod-cod AUTO reads the PLHEADER coherently over its 90 symbols and takes the carrier offset the PLS decoder takes; the coarse-frequency loop of "
                         "--wl-phases needs the frame length before it can remove a larger one: name the MODCOD, or hand the offset in with --coarse-freq")
    if not args.rad_rx_no_loop and not args.max_frames:
        raise ValueError("a looping input needs --max-frames")
    mc = P.get_modcod("")
    F, n, osf = args.n_frames_batch, mc.pl_frame, args.osf
    rx = Dvbs2Hip(mc.name, max_frames=F, device=args.device)
    rcv = None
    try:
        if args.coarse_freq:
            rx.sync_coarse_set_freq(args.coarse_freq)
        learn = 0
        if args.stm_type in ("FAST", "ULTRA"):
            if osf != 2:
                raise ValueError("--stm-type %s is the Gardner loop at two samples per symbol (--shp-osf 2)" % args.stm_type)
            rx.sync_timing_set_params(args.stm_df, args.stm_nbw, args.stm_dg)
        if args.stm_type == "ULTRA":
            rx.sync_timing_set_type("ULTRA", args.stm_hold_size)
            learn = sum(args.wl_frames) if args.stm_learn_frames is None else args.stm_learn_frames
        rcv = RadioUserBinary(n * osf, input_filename=args.rad_rx_file_path, auto_reset=not args.rad_rx_no_loop, n_frames=F)
        seq = RxSequence(rx, F, osf, pl_frame=n, agc=not args.no_agc, coarse=bool(args.coarse_freq), timing=args.stm_type, learn_frames=learn,
                         timing_offset=args.timing_offset if args.timing_offset >= 0 else 2 * 20 * osf, fused=True)
        got, have = [], 0
        while have < AUTO_SYMBOLS:
            try:
                x = rcv.receive()
            except ProcessingAborted:
                break
            sym = seq.symbols(seq.front(x))
            if sym is not None:
                got.append(np.asarray(sym, np.float32).reshape(-1)); have += got[-1].size // 2
        if have < 90:
            raise ValueError("--mod-cod AUTO: the file holds %d symbols, a PLHEADER has 90" % have)
        res, score = rx.pls_search(np.concatenate(got))
    finally:
        rx.close()
        if rcv is not None:
            rcv.close()
    found = P.find_modcod(res, score)
    offset, value, count, slots = (int(v) for v in res)
    if found is None:
        best = "none" if offset < 0 else "%s at symbol %d, %d of %d headers, score %.2f" % (_pls_text(value), offset, count, slots, score)
        raise ValueError("--mod-cod AUTO: no chain of PLHEADERs in the first %d symbols (searched: the %d MODCODs of the table, pilots on, at least two headers one frame "
                         "apart explaining %.2f of their windows' energy each); best chain: %s" % (have, len(P.MODCODS), P.PLS_SEARCH_Q_MIN, best))
    print("# AUTO: %s | header at symbol %d | %d of %d headers | score %.2f" % (_pls_text(value), offset, count, slots, score), file=out)
    return dict(modcod=found[0].name, value=value, pilots=found[1], offset=offset, count=count, slots=slots, score=score, symbols=have)


def run_vcm(args, out=sys.stdout) -> dict:
    """--mod-cod VCM: the front tasks as detect() runs them -- a probe handle, RxSequence.front and RxSequence.symbols, then the gain stage on the symbols -- and every
    read's symbols into vcm.VcmReceiver, which walks the PLHEADER chain and decodes every frame with a handle of the MODCOD its header names.  At the end of a file that
    does not loop, the last read is filled up with noise of the file's own power and one read of noise follows: the matched filter and the timing task hold the
    stream's last symbols until more samples come.  -> dict(frames, per_modcod, skipped, losses, ldpc_down, bch_down)"""
    for flag, given, why in (
            ("--wl-phases", getattr(args, "wl_phases", False), "the coarse-frequency loop needs one frame length, and a VCM stream has several"),
            ("--sync-fine", args.sync_fine, "the pilot-aided phase synchronizer runs on the frame synchronizer's aligned frames of one MODCOD"),
            ("--snk-type TS", getattr(args, "snk_type", "BITS") == "TS", "a BBFRAME's DFL changes with the MODCOD, and the parser is built for one"),
            ("--src-type USER", args.src_type == "USER" and bool(args.src_path), "a pattern file holds frames of one K_bch"),
            ("--pls-check", getattr(args, "pls_check", False), "it counts the headers that differ from one expected MODCOD, and here every header is followed")):
        if given:
            raise ValueError("--mod-cod VCM excludes %s: %s." % (flag, why))
    if not args.rad_rx_no_loop and not args.max_frames:
        raise ValueError("a looping input needs --max-frames")
    from .vcm import VcmReceiver
    mc = P.get_modcod("")                                                          # the probe: no task in front of the walk depends on the MODCOD
    F, n, osf = args.n_frames_batch, mc.pl_frame, args.osf
    if args.stm_type in ("FAST", "ULTRA") and osf != 2:
        raise ValueError("--stm-type %s is the Gardner loop at two samples per symbol (--shp-osf 2)" % args.stm_type)
    vr = VcmReceiver(max_frames=F, n_ite=args.dec_ite, alpha=args.dec_alpha, implem=args.dec_implem, estimator=getattr(args, "est_type", "DVBS2"), device=args.device)
    rx, fh, snk = vr.base, None, None
    st = dict(frames=0)
    try:
        if args.sim_stats:
            rx.timing_enable(True)
        if args.coarse_freq:
            rx.sync_coarse_set_freq(args.coarse_freq)
        learn = 0
        if args.stm_type in ("FAST", "ULTRA"):
            rx.sync_timing_set_params(args.stm_df, args.stm_nbw, args.stm_dg)
        if args.stm_type == "ULTRA":
            rx.sync_timing_set_type("ULTRA", args.stm_hold_size)
            learn = sum(args.wl_frames) if args.stm_learn_frames is None else args.stm_learn_frames
        skip = args.timing_offset if args.timing_offset >= 0 else 2 * 20 * osf
        seq = RxSequence(rx, F, osf, pl_frame=n, agc=not args.no_agc, coarse=bool(args.coarse_freq), timing=args.stm_type, learn_frames=learn, timing_offset=skip, fused=True)
        fh = open(args.rad_rx_file_path, "rb")
        snk = open(args.snk_path, "wb") if args.snk_path else None
        blk = 2 * n * osf * F                                                      # floats of one read
        rng = np.random.default_rng(0)
        samples, pushed, total, reads_left = 0, 0, None, None                      # the file's samples taken; symbols pushed; the symbols the file gives, once its end is known
        while (not args.max_frames or st["frames"] < args.max_frames) and reads_left != 0:
            x = np.fromfile(fh, np.float32, blk) if reads_left is None else np.zeros(0, np.float32)
            if x.size < blk:
                if not args.rad_rx_no_loop:
                    if fh.tell() < 4 * blk:
                        raise ValueError("the file holds less than one read of %d complex samples" % (blk // 2))
                    fh.seek(0)
                    continue
                if reads_left is None:
                    samples += x.size // 2
                    total, reads_left = max(samples - (skip if args.stm_type == "PERFECT" else 0), 0) // osf, 2
                    power = float(np.mean(np.square(x, dtype=np.float64))) if x.size else 1.0 / (2 * osf)
                reads_left -= 1
                x = np.concatenate([x, (np.sqrt(power) * rng.standard_normal(blk - x.size)).astype(np.float32)])
            else:
                samples += blk // 2
            sym = seq.symbols(seq.front(x))
            if sym is None:
                continue
            if not args.no_agc:
                sym = rx.agc(sym, n_frames=len(sym), output_energy=1.0)
            sym = np.asarray(sym, np.float32).reshape(-1)
            n_new = sym.size // 2
            for _, _, _, bits, _, _ in vr.push(sym, None if total is None else min(max(total - pushed, 0), n_new)):
                st["frames"] += 1
                if snk:
                    snk.write(np.packbits((bits != 0).astype(np.uint8), bitorder="little").tobytes())      # SinkUserBinary's bytes, frames of any K_bch
            pushed += n_new
    finally:
        if args.sim_stats:
            from .sim import print_stats
            print_stats(list(vr.h.values()), out)
        vr.close()
        for f in (fh, snk):
            if f:
                f.close()
    st.update(per_modcod=dict(vr.stats["frames"]), skipped=vr.stats["skipped"], losses=vr.stats["losses"], ldpc_down=vr.stats["ldpc_down"], bch_down=vr.stats["bch_down"])
    print("# VCM: frames %d (%s) | skipped %d | losses of lock %d | LDPC flag down %d | BCH flag down %d" % (
        st["frames"], ", ".join("%s: %d" % kv for kv in st["per_modcod"].items()) or "none", st["skipped"], st["losses"], st["ldpc_down"], st["bch_down"]), file=out)
    return st


def run(args, out=sys.stdout) -> dict:
    if args.mod_cod == "VCM":
        return run_vcm(args, out)
    from .receiver import Dvbs2Hip
    auto = None
    if args.mod_cod == "AUTO":
        auto = detect(args, out)
        args = argparse.Namespace(**dict(vars(args), mod_cod=auto["modcod"]))        # from here on exactly as --mod-cod <that name>
    mc = P.get_modcod(args.mod_cod)
    F, n, osf = args.n_frames_batch, mc.pl_frame, args.osf
    if not args.rad_rx_no_loop and not args.max_frames:
        raise ValueError("a looping input needs --max-frames")
    pattern = load_src(args.src_path, mc.K_bch) if args.src_type == "USER" and args.src_path else None
    ts = getattr(args, "snk_type", "BITS") == "TS"
    if ts and pattern is not None:
        raise ValueError("--snk-type TS hands out packets, not bits: there is nothing to count against a pattern (--src-type NONE)")
    rx = Dvbs2Hip(mc.name, max_frames=F, n_ite=args.dec_ite, alpha=args.dec_alpha, early_stop=True, implem=args.dec_implem, device=args.device)
    if args.sim_stats:
        rx.timing_enable(True)
    if args.coarse_freq:
        rx.sync_coarse_set_freq(args.coarse_freq)
    fast = args.stm_type == "FAST"
    wl = getattr(args, "wl_phases", False)
    if wl and args.coarse_freq:
        raise ValueError("--wl-phases finds the carrier offset itself: it excludes --coarse-freq")
    smf_kernel = getattr(args, "smf_kernel", None)
    if smf_kernel is not None and not wl:
        raise ValueError("--smf-kernel chooses the kernel of the coarse-frequency loop, which only --wl-phases runs: give both or neither")
    ultra = args.stm_type == "ULTRA"
    pls_check = getattr(args, "pls_check", False)
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
    rcv = RadioUserBinary(n * osf, input_filename=args.rad_rx_file_path, auto_reset=not args.rad_rx_no_loop, n_frames=F)
    snk = (SinkTS(args.snk_path) if ts else SinkUserBinary(args.snk_path, mc.K_bch)) if args.snk_path else None
    # the task sequence (rx_sequence.py); --wl-phases: the frozen coarse estimate in front, and L&R as learning phase 3 has trained it, for what that estimate leaves
    seq = RxSequence(rx, F, osf, pl_frame=n, agc=not args.no_agc, coarse=bool(args.coarse_freq or wl), timing=args.stm_type, learn_frames=learn,
                     timing_offset=args.timing_offset if args.timing_offset >= 0 else 2 * 20 * osf,      # two group delays of grp_delay * osf samples
                     fine=bool(args.sync_fine or wl), lr=wl, pls_check=pls_check, estimator=getattr(args, "est_type", "DVBS2"), packets=ts)
    st = dict(frames=0, locked_frames=0, be=0, fe=0, delay=None)
    if auto is not None:
        st["auto"] = auto
    if ts:
        st.update(bbframes_dropped=0, packets=0, crc8_errors=0)
    if pls_check:
        st["pls_mismatches"] = 0
        pls_want, pls_locked, pls_seen = rx.pls_expected(), 0, collections.Counter()
    lock = LockTracker()
    try:
        if wl:
            from .acquire import acquire
            l1, l2, l3 = args.wl_frames
            st["acquisition"] = acq = acquire(rx, rcv.receive, n_frames=F, osf=osf, learn1=l1, learn2=l2, learn3=l3, wait_max=args.wl_wait_max, agc=not args.no_agc,
                                              **({} if smf_kernel is None else dict(smf_kernel=smf_kernel)))
            print("# waiting %d | learning %d + %d + %d frames | packet flag %s | coarse frequency %s" % (
                acq["frames"]["waiting"], acq["frames"]["learning1"], acq["frames"]["learning2"], acq["frames"]["learning3"], acq["flag"], acq["freq"]), file=out)
        while not args.max_frames or lock.frames < args.max_frames:
            try:
                x = rcv.receive()
            except ProcessingAborted:
                break
            sym = seq.symbols(seq.front(x))
            if sym is None:
                continue
            delay, flags, tri, aligned = seq.align(sym)
            bits = seq.decode(aligned)
            if ts:                                                                 # the batch's packets, its frames' statuses: counted here from what the one call returned
                packets, status, hdr = bits
                st["bbframes_dropped"] += int((hdr[:, 0] != 0).sum()); st["packets"] += len(packets); st["crc8_errors"] += int((status != 0).sum())
                if snk:
                    snk.send(packets)
            for f in range(len(sym)):
                locked = lock.update(delay[f]) >= 2                                # the delay line has settled on this alignment
                if pls_check and locked:
                    v = int(seq.pls[0][f])
                    pls_locked += 1; st["pls_mismatches"] += v != pls_want
                    pls_seen[v] += v != pls_want
                    if pls_locked >= 16 and 2 * st["pls_mismatches"] > pls_locked:
                        raise ValueError("stream carries %s; the receiver was built for %s (PLS %d)" % (_pls_text(pls_seen.most_common(1)[0][0]), mc.name, pls_want))
                if snk and not ts:
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
    st["frames"], st["delay"] = lock.frames, lock.delay
    st["ber"] = st["be"] / max(1, st["locked_frames"] * mc.K_bch)
    st["fer"] = st["fe"] / max(1, st["locked_frames"])
    print("# frames %(frames)d | in lock %(locked_frames)d | BE %(be)d | FE %(fe)d | BER %(ber).2e | FER %(fer).2e | delay %(delay)s" % st +
          (" | PLS mismatches %d" % st["pls_mismatches"] if pls_check else "") +
          (" | BBFRAMEs dropped %(bbframes_dropped)d | packets %(packets)d | CRC-8 errors %(crc8_errors)d" % st if ts else ""), file=out)
    return st


if __name__ == "__main__":
    run(build_parser().parse_args())
