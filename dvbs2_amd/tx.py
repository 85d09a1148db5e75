"""`dvbs2_tx` work-alike (rows N1 + N2 + N3): source -> BB scramble -> BCH -> LDPC -> interleave -> modulate -> frame ->
PL scramble -> shaping filter -> raw IQ file, every stage on the GPU (src/mains/TX/main.cpp of the reference; README.md:151-158).

  python -m dvbs2_amd.tx --rad-tx-file-path out_tx.bin -F 8 --src-type USER --src-path K_14232.src --mod-cod QPSK-S_8/9 --n-frames 64

`--mod-cod-seq NAME:COUNT[,NAME:COUNT...]` (an extension) sends variable coding and modulation instead: COUNT frames of each MODCOD in turn, the list over and over
(vcm.VcmTransmitter), -F frames per call through one shaping filter, and 40 zero symbols behind the last frame so that the file ends whole.

`--tx-tasks` makes the PL frames by the seven TX tasks of the C ABI, one call per task (TxTasks below), instead of the fused tx_bb: the same file.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import params as P
from .iqfile import RadioUserBinary
from .srcfile import SourceAZCW, SourceDone, SourceTS, SourceUser, SourceUserBinary


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="dvbs2_tx", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mod-cod", default="QPSK-S_8/9")
    ap.add_argument("--mod-cod-seq", default=None, metavar="NAME:COUNT[,NAME:COUNT...]", help="variable coding and modulation (an extension): COUNT frames of each MODCOD in turn, the list "
                    "over and over, in place of --mod-cod; every PLHEADER names its frame's MODCOD (the receiver's --mod-cod VCM); the payload source is RAND")
    ap.add_argument("-F", "--src-fra", type=int, default=1, dest="n_frames_batch")
    ap.add_argument("--src-type", default="RAND", choices=["RAND", "USER", "USER_BIN", "AZCW", "TS"],      # DVBS2.cpp:66
                    help="TS (an extension): --src-path is an MPEG transport stream, sent as DVB-S2 BBFRAMEs (BBHEADER, CRC-8 per packet; the receiver's --snk-type TS)")
    ap.add_argument("--src-path", default="")
    ap.add_argument("--src-no-loop", action="store_true", help="USER_BIN: send the file once (the last frame zero-padded) instead of over and over; TS: once, then one null packet (the last frame "
                    "short), the batch and one more padded with all-zero frames, which a BBFRAME parser drops")
    ap.add_argument("--shp-osf", type=int, default=2, dest="osf", choices=[2], help="samples per symbol (the GPU shaping filter is built for 2)")
    ap.add_argument("--rad-type", default="USER_BIN", choices=["USER_BIN"])
    ap.add_argument("--rad-tx-file-path", required=True)
    ap.add_argument("--n-frames", type=int, default=0, help="stop after this many frames")
    ap.add_argument("--tx-time-limit", type=float, default=0.0, help="stop after this many milliseconds")
    ap.add_argument("--sim-seed", type=int, default=0, dest="seed")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sim-stats", action="store_true", help="per-kernel-group device time at the end (the reference's --sim-stats)")
    ap.add_argument("--tx-tasks", action="store_true", help="make the PL frames by the seven TX tasks, one C-ABI call per task in the reference's order, instead of the fused tx_bb "
                    "(payload sources USER, USER_BIN, AZCW and TS; same frames)")
    return ap


class TxTasks:
    """The PL frames of a batch by the seven tasks of the reference's TX mains, each a `_dev` call on the handle's stream:
    BB scramble -> BCH encode -> LDPC encode -> interleave -> modulate -> frame -> PL scramble; the sockets in between stay on the device."""

    def __init__(self, rx, n_frames, device=0):
        import torch
        self.torch, self.rx, self.F = torch, rx, n_frames
        self.dev = torch.device("cuda", device)
        bits = lambda n: torch.empty((n_frames, n), dtype=torch.int32, device=self.dev)
        syms = lambda n: torch.empty((n_frames, 2 * n), dtype=torch.float32, device=self.dev)
        self.scr, self.bch, self.cw, self.itl = bits(rx.K_bch), bits(rx.K_ldpc), bits(rx.N_ldpc), bits(rx.N_ldpc)
        self.sym, self.plf, self.pl = syms(rx.N_xfec), syms(rx.pl_frame), syms(rx.pl_frame)

    def run_dev(self, info):
        """info: int32 device tensor [F, K_bch] -> the device tensor of the scrambled PL frames (valid once the handle's stream has got there)"""
        rx, F = self.rx, self.F
        rx.bb_scramble_dev(info.data_ptr(), self.scr.data_ptr(), F)
        rx.bch_encode_dev(self.scr.data_ptr(), self.bch.data_ptr(), F)
        rx.ldpc_encode_dev(self.bch.data_ptr(), self.cw.data_ptr(), F)
        rx.interleave_dev(self.cw.data_ptr(), self.itl.data_ptr(), F)
        rx.modulate_dev(self.itl.data_ptr(), self.sym.data_ptr(), F)
        rx.framer_generate_dev(self.sym.data_ptr(), self.plf.data_ptr(), F)
        rx.pl_scramble_dev(self.plf.data_ptr(), self.pl.data_ptr(), F)
        return self.pl

    def run(self, info):
        """info: int32 array [F, K_bch] -> f32 array [F, 2 * pl_frame]"""
        torch = self.torch
        d_info = torch.from_numpy(info.reshape(self.F, self.rx.K_bch)).to(self.dev)
        torch.cuda.current_stream(self.dev).synchronize()          # (the copy is asynchronous to the handle's stream)
        pl = self.run_dev(d_info)
        self.rx.synchronize()
        return pl.cpu().numpy()


def run_vcm(args, out=sys.stdout) -> int:
    """--mod-cod-seq: -F frames per call of vcm.VcmTransmitter, in schedule order through one shaping filter -> number of frames written"""
    from .vcm import VcmTransmitter, parse_schedule
    schedule = parse_schedule(args.mod_cod_seq)
    if args.src_type != "RAND":
        raise ValueError("--mod-cod-seq sends frames of several K_bch and fills them with tx_bb's random payloads: --src-type %s is not provided with it" % args.src_type)
    if args.tx_tasks:
        raise ValueError("--mod-cod-seq builds its frames with the fused tx_bb of one handle per MODCOD: --tx-tasks is not provided with it")
    if not args.n_frames and not args.tx_time_limit:
        raise ValueError("one of --n-frames / --tx-time-limit is needed to end the transmission")
    F = args.n_frames_batch
    tx = VcmTransmitter(schedule, device=args.device, seed=args.seed)
    snd = RadioUserBinary(1, output_filename=args.rad_tx_file_path)
    t0, frames, per = time.perf_counter(), 0, {}
    try:
        while (not args.n_frames or frames < args.n_frames) and (not args.tx_time_limit or (time.perf_counter() - t0) * 1e3 < args.tx_time_limit):
            n = min(F, args.n_frames - frames) if args.n_frames else F
            sent, x = tx.samples(n, osf=args.osf)
            snd.send(x)
            frames += n
            for name, _ in sent:
                per[name] = per.get(name, 0) + 1
        snd.send(tx.flush(osf=args.osf))                                            # the last frame's last symbols are still in the filter: a file ends whole
    finally:
        tx.close(); snd.close()
    print("(II) %d frames (%s) written in '%s'" % (frames, ", ".join("%s: %d" % kv for kv in per.items()), args.rad_tx_file_path), file=out)
    return frames


def run(args, out=sys.stdout) -> int:
    """-> number of frames written"""
    if getattr(args, "mod_cod_seq", None) is not None:
        return run_vcm(args, out)
    from .receiver import Dvbs2Hip
    mc = P.get_modcod(args.mod_cod)
    once = args.src_type in ("USER_BIN", "TS") and args.src_no_loop
    if not args.n_frames and not args.tx_time_limit and not once:
        raise ValueError("one of --n-frames / --tx-time-limit is needed to end the transmission")
    if args.src_type in ("USER", "USER_BIN", "TS") and not args.src_path:
        raise ValueError("--src-type %s needs --src-path" % args.src_type)
    if args.tx_tasks and args.src_type == "RAND":
        raise ValueError("--tx-tasks needs a payload source (USER, USER_BIN, AZCW or TS): the random source lives inside the fused tx_bb")
    F = args.n_frames_batch
    src = (SourceUser(args.src_path, mc.K_bch) if args.src_type == "USER" else SourceUserBinary(args.src_path, mc.K_bch, auto_reset=not args.src_no_loop) if args.src_type == "USER_BIN"
           else SourceAZCW(mc.K_bch) if args.src_type == "AZCW" else SourceTS(args.src_path, (mc.K_bch - 80) // 8, auto_reset=not args.src_no_loop) if args.src_type == "TS" else None)
    ts = args.src_type == "TS"
    rx = Dvbs2Hip(mc.name, max_frames=F, device=args.device)
    if args.sim_stats:
        rx.timing_enable(True)
    tasks = TxTasks(rx, F, args.device) if args.tx_tasks else None
    snd = RadioUserBinary(mc.pl_frame * args.osf, output_filename=args.rad_tx_file_path, n_frames=F)
    t0, frames, call = time.perf_counter(), 0, 0
    try:
        while (not args.n_frames or frames < args.n_frames) and (not args.tx_time_limit or (time.perf_counter() - t0) * 1e3 < args.tx_time_limit):
            try:
                info = src.generate(F) if src else None
            except SourceDone:
                break
            if ts:                                                          # the packet stream's next bytes -> BBFRAMEs on the GPU; frames the stream does not fill stay zero
                stream, n = info
                info = np.zeros((F, mc.K_bch), np.int32)
                if n:
                    info[:n] = rx.bbframe_build(stream, n)
            if tasks:
                pl = tasks.run(info)
            else:
                _, pl = rx.tx_bb(F, info=info, seed=(args.seed << 32) + call)
            snd.send(rx.shape_filter(pl, n_frames=F, osf=args.osf))        # the filter memory carries over from call to call
            frames += F
            call += 1
    finally:
        if args.sim_stats:
            from .sim import print_stats
            print_stats([rx], out)
        rx.close(); snd.close()
    print("(II) %d frames of %d complex samples written in '%s'" % (frames, mc.pl_frame * args.osf, args.rad_tx_file_path), file=out)
    return frames


if __name__ == "__main__":
    run(build_parser().parse_args())
