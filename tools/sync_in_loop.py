#!/usr/bin/env python3
"""FER of the chain with the IN-SCOPE synchronizers in the loop (frame synchronizer, Luise-Reggiannini fine frequency, pilot-aided phase), beside the
genie-timed loop of results/r06/filtered_loop.md -- what the block-wise synchronizers cost at the operating point, the reference's sample-serial loops (timing, coarse
frequency, AGC) being replaced by a genie.  GPU box:

    python tools/sync_in_loop.py --ebn0 3.7 3.8 --fe 400 --max-frames 200000 --json gpurun_out/sync_in_loop.json

One continuous stream per noise point, as a receiver sees it: the fixed payload conf/src/K_14232.src in every frame (what the reference's dvbs2_rx counts errors against,
RX/main.cpp: Source_user), an unknown frame start (--off symbols), a constant carrier phase and a residual frequency offset (--freq cycles per symbol: what a coarse loop
leaves behind) -> shaping filter -> AWGN at the sample rate -> matched filter -> every second sample (timing by genie) -> the tasks of the reference's RX graph in its order,
one C-ABI call per task: frame synchronizer -> PL descrambler -> L&R -> pilot-aided phase -> remove PLH -> estimate -> demodulate + de-interleave -> LDPC -> BCH -> BB
descrambler.  Variants: `frame` (frame synchronizer only, no rotation applied: its cost alone), `fine` (rotation applied; L&R + phase synchronizer correct it).
Filters, synchronizers and the delay line keep their state from call to call, so the stream is continuous across the calls.

--chn-max-delay D puts the reference channel's three delay tasks (dvbs2hip_channel_delay) behind the shaping filter, and --stm-type FAST replaces the genie by the
Gardner timing loop on the GPU (synchronize -> extract, RX/main_sched.cpp:202-204): a call whose extract underflows yields no frames, and the loop's learning frames
are the first --skip frames, which are not counted.

--chn-max-freq-shift f puts the channel's frequency shift (dvbs2hip_channel_freq_shift, f cycles per sample) behind the delay tasks, and --wl-phases runs the reference's
waiting and learning phases (dvbs2_amd/acquire.py: the coarse-frequency loop on the GPU, 150 / 150 / 200 frames) on the head of the stream before anything is counted; the
transmission phase then shifts by the frozen estimate (dvbs2hip_sync_coarse_synchronize) in front of the matched filter.  --wl-phases needs --stm-type FAST.
--smf-kernel {LANE,WAVE} chooses the loop's kernel for --wl-phases (dvbs2hip_sync_step_mf_set_kernel).
--stm-type ULTRA --stm-hold-size H is the held loop (dvbs2hip_sync_timing_set_type): the whole loop for --stm-learn-frames frames, then it holds."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dvbs2_amd.rx_sequence import LockTracker, RxSequence, add_timing_args      # noqa: E402

LEARN_FRAMES = 500                                                                 # --stm-learn-frames: the learning phases' 150 + 150 + 200


def run_point(Rx, P, mc, ebn0, variant, a):
    F, n, off = a.F, mc.pl_frame, a.off
    rx = Rx(mc.name, max_frames=F, n_ite=50, alpha=1.0, early_stop=True, implem="SPA")
    pattern = np.unpackbits(np.load(os.path.join(ROOT, "tests", "golden", "src_K_%d.npy" % (14232 if mc.K_bch == 14232 else 9552))))[:mc.K_bch].astype(np.int32)      # DVBS2.cpp:336-349
    _, pl = rx.tx_bb(1, info=pattern[None, :])
    frame = pl.reshape(n, 2).astype(np.float64)
    frame = frame[:, 0] + 1j * frame[:, 1]
    sigma = np.float32(P.esn0_to_sigma(P.ebn0_to_esn0(ebn0, mc.code_rate, mc.bps)))
    rot = variant == "fine"
    delay_D = getattr(a, "chn_max_delay", None)
    stm_type = getattr(a, "stm_type", "PERFECT")
    freq_shift = getattr(a, "chn_max_freq_shift", None)
    wl = getattr(a, "wl_phases", False)
    if wl and stm_type != "FAST":
        raise ValueError("--wl-phases needs --stm-type FAST")
    smf_kernel = getattr(a, "smf_kernel", None)
    if smf_kernel is not None and not wl:
        raise ValueError("--smf-kernel chooses the kernel of the coarse-frequency loop, which only --wl-phases runs: give both or neither")
    if stm_type == "ULTRA":
        rx.sync_timing_set_type("ULTRA", a.stm_hold_size)                              # the held loop: the whole loop for --stm-learn-frames frames, then set_act
    if delay_D is not None:
        rx.channel_set_delay(delay_D)
    if freq_shift is not None:
        rx.channel_set_freq_shift(freq_shift)
    # the receiver's tasks (dvbs2_amd/rx_sequence.py): timing by genie is its PERFECT at offset 0 -- the two filters delay the stream by 40 symbols, part of the unknown
    # frame start; --wl-phases: the shift by the loop's frozen estimate in front of the matched filter; `fine` runs L&R always
    seq = RxSequence(rx, F, 2, pl_frame=n, agc=a.agc, coarse=wl, timing=stm_type, timing_offset=0, learn_frames=getattr(a, "stm_learn_frames", LEARN_FRAMES),
                     fine=rot, lr=rot, sigma=sigma if a.est_perfect else None)
    st = dict(frames=0, counted=0, be=0, fe=0, delay=None, stable=0, moved=0)
    lock = LockTracker()
    t0 = time.time()
    idx = (np.arange(F * n) - off) % n
    calls = [0]

    def received():
        """the next F frames of the receiver's input, before its front gain stage"""
        k = calls[0]
        calls[0] += 1
        t = np.arange(F * n, dtype=np.float64) + float(k) * F * n                      # absolute symbol index of this call's stretch of the stream
        s = frame[idx]                                                                 # F n is a multiple of n: the same indices every call
        if rot:
            s = s * np.exp(1j * (a.phase + 2.0 * np.pi * a.freq * t))
        x = np.empty((F * n, 2), np.float32); x[:, 0] = s.real; x[:, 1] = s.imag
        up = rx.shape_filter(x, n_frames=F, osf=2)
        if delay_D is not None:
            up = rx.channel_delay(up.reshape(F, -1))                                    # chn_frm_del -> chn_int_del -> chn_frac_del (TX_RX/main.cpp:215-218)
        if freq_shift is not None:
            up = rx.channel_freq_shift(up.reshape(F, -1))                               # freq_shift (TX_RX/main.cpp:219)
        return rx.add_noise(sigma, up, seed=(a.seed << 20) + k, n_frames=F)

    if wl:
        from dvbs2_amd.acquire import acquire
        st["acquisition"] = acquire(rx, received, n_frames=F, agc=a.agc, **({} if smf_kernel is None else dict(smf_kernel=smf_kernel)))
        if not st["acquisition"]["acquired"]:
            raise RuntimeError("the waiting phase gave up: %r" % (st["acquisition"],))
    while st["fe"] < a.fe and st["counted"] < a.max_frames:
        sym = seq.symbols(seq.front(received()))
        if sym is None:
            continue                                                                    # underflow: the symbols wait in the carry buffer
        delay, flags, tri, aligned = seq.align(sym)
        err = (seq.decode(aligned) != pattern[None, :]).sum(axis=1)
        for f in range(F):
            lock.update(delay[f])
            if lock.frames > a.skip:                                                    # every frame after the acquisition counts, locked or not (a lost lock is a lost frame)
                st["counted"] += 1; st["be"] += int(err[f]); st["fe"] += int(err[f] > 0)
    rx.close()
    st.update(frames=lock.frames, delay=lock.delay, stable=lock.stable, moved=lock.moved, ebn0=ebn0, variant=variant, fer=st["fe"] / max(1, st["counted"]), ber=st["be"] / max(1, st["counted"] * mc.K_bch), seconds=time.time() - t0)
    return st


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mod-cod", default="QPSK-S_8/9")
    ap.add_argument("--ebn0", type=float, nargs="+", default=[3.7, 3.8])
    ap.add_argument("--variants", nargs="+", default=["frame", "fine"])
    ap.add_argument("-F", type=int, default=256)
    ap.add_argument("--fe", type=int, default=400)
    ap.add_argument("--max-frames", type=int, default=200000)
    ap.add_argument("--skip", type=int, default=16, help="frames of acquisition at the head of the stream that are not counted")
    ap.add_argument("--off", type=int, default=1234)
    ap.add_argument("--phase", type=float, default=0.7)
    ap.add_argument("--freq", type=float, default=2e-5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--est-perfect", action="store_true", help="the channel's sigma instead of the M2M4 estimate (the reference's 16APSK trace: --est-type PERFECT)")
    ap.add_argument("--agc", action="store_true", help="the reference's two gain stages in the loop (front_agc on the samples, mult_agc on the symbols)")
    ap.add_argument("--chn-max-delay", type=float, default=None, help="the reference channel's delay tasks with this D (>= 2) behind the shaping filter")
    add_timing_args(ap, learn_default=LEARN_FRAMES)
    ap.add_argument("--chn-max-freq-shift", type=float, default=None, help="the reference channel's frequency shift (cycles per sample) behind the delay tasks")
    ap.add_argument("--wl-phases", action="store_true", help="run the waiting and learning phases (the coarse-frequency loop on the GPU) before anything is counted")
    ap.add_argument("--smf-kernel", choices=["LANE", "WAVE"], default=None, help="with --wl-phases: the form of the coarse-frequency loop (LANE: one lane per stream; WAVE: one wave "
                                                                                 "per stream; the same results); default: not set")
    ap.add_argument("--json", default=None)
    return ap


def main():
    a = build_parser().parse_args()
    from dvbs2_amd.receiver import Dvbs2Hip
    from dvbs2_amd import params as P
    mc = P.get_modcod(a.mod_cod)
    rows = []
    for e in a.ebn0:
        for v in a.variants:
            r = run_point(Dvbs2Hip, P, mc, e, v, a)
            rows.append(r)
            print("%s %.2f dB %-5s: frames %d counted %d FE %d FER %.3e BER %.2e | delay %s, moved %d times after acquisition | %.0f s" % (
                mc.name, e, v, r["frames"], r["counted"], r["fe"], r["fer"], r["ber"], r["delay"], r["moved"], r["seconds"]), flush=True)
    if a.json:
        json.dump(dict(args=vars(a), rows=rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
