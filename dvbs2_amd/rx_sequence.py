"""The receiver's transmission-phase task sequence (the reference's src/mains/RX/main_sched.cpp:197-223) above the C ABI, written once: dvbs2_amd/rx.py, tools/sync_in_loop.py
and learning phase 3 of dvbs2_amd/acquire.py drive it, each with its own source, counting and stop rule.

  front       front gain stage (Multiplier_AGC, :197)
  symbols     coarse frequency shift (:198) -> matched filter (:199-201) -> symbol timing: Gardner synchronize -> extract (:202-204), or every osf-th sample at a known offset
  align       gain stage (:205) -> frame synchronizer (:206-209) [-> PLS decoder on the aligned frames' headers: pls_check, an extension]
  fine_sync   PL descrambler (:210) -> L&R (:211) -> pilot-aided phase synchronizer (:212)
  decode      fine_sync -> remove PLH -> estimate -> demodulate + deinterleave -> LDPC -> BCH -> BB descrambler (:213-220), one C-ABI call per task; or the fused chain
              (estimator="PILOTS", an extension: sigma from the frames' header and pilot symbols instead, ahead of remove PLH or of the fused chain)

The handle is a `Dvbs2Hip` or anything with the methods used here.  ULTRA's set_act(True) goes in front of the matched filter: the reference sets it once, ahead of the
whole sequence (main_sched.cpp:655), and it touches the timing task's state alone, so where it stands among the tasks before sync_timing_synchronize changes no result."""
import numpy as np


class RxSequence:
    """One per handle and stream.  agc: the two gain stages; coarse: the shift in front of the matched filter; timing: "PERFECT" (every osf-th matched-filter sample from
    timing_offset, needs pl_frame), "FAST" or "ULTRA" (the Gardner loop the handle has been set to; ULTRA holds once learn_frames frames have been fed); fine: the fine
    synchronizers and the chain task by task, lr: L&R among them; fused (None: unless fine): rx_bb, the fused chain; sigma: the channel's, None for the estimator's;
    pls_check: align() also reads the aligned frames' PLHEADERs and leaves (PLS, MET, ENE) of its last call in self.pls (off: the call sequence has no such task);
    estimator: "DVBS2" (M2M4, the reference's; the call sequence is as it was) or "PILOTS" (estimate_pilots: unbiased for 16APSK and 32APSK too), used when sigma is None;
    packets: decode() hands out the user packets of the frames' BBFRAMEs instead of their bits (rx_bb_up in place of rx_bb, or bbframe_parse behind bb_descramble)."""

    def __init__(self, rx, F, osf=2, pl_frame=None, agc=True, coarse=False, timing="PERFECT", timing_offset=0, learn_frames=0, fine=False, lr=False, sigma=None, fused=None, pls_check=False,
                 estimator="DVBS2", packets=False):
        if estimator not in ("DVBS2", "PILOTS"):
            raise ValueError("estimator is DVBS2 or PILOTS")
        if fused == fine:
            raise ValueError("the fused chain has no fine synchronizer in it, the tasks one by one start with them: fine or fused, not both or neither")
        self.rx, self.F, self.osf, self.n, self.agc, self.coarse, self.timing, self.learn_frames, self.fine, self.lr, self.sigma = rx, F, osf, pl_frame, agc, coarse, timing, learn_frames, fine, lr, sigma
        self.pls_check, self.pls, self.estimator, self.packets = pls_check, None, estimator, packets
        self.fed = 0                                                               # frames the timing loop has taken
        self.skip = timing_offset
        self.tail = np.zeros((0, 2), np.float32)                                   # PERFECT: matched-filter samples not yet turned into symbols

    def front(self, x):
        """front_agc: DVBS2.cpp:660-664"""
        x = np.asarray(x, np.float32).reshape(self.F, -1)
        return self.rx.agc(x, n_frames=self.F, output_energy=1.0 / self.osf).reshape(self.F, -1) if self.agc else x

    def symbols(self, x):
        """-> [frames, 2 pl_frame] symbols, or None when this call completed no frame (the samples wait: in the tail, or in the timing task's carry buffer)"""
        rx, F, osf, n = self.rx, self.F, self.osf, self.n
        if self.coarse:
            _, _, x = rx.sync_coarse_synchronize(x, n_frames=F)
        if self.timing == "PERFECT":
            mf, self.skip = np.concatenate([self.tail, rx.filter(x, n_frames=F).reshape(-1, 2)])[self.skip:], 0
            n_sym = mf.shape[0] // osf // n * n                                    # whole frames: at most F, a call brings F and the tail holds less than one
            self.tail = mf[n_sym * osf:]
            return np.ascontiguousarray(mf[:n_sym * osf:osf]).reshape(-1, 2 * n) if n_sym else None
        if self.timing == "ULTRA" and self.fed >= self.learn_frames:
            rx.sync_timing_set_act(True)                                           # the learning frames are over: the loop holds (calls are whole: from the first one at or past them)
        y, b, _ = rx.sync_timing_synchronize(rx.filter(x, n_frames=F).reshape(F, -1))
        self.fed += F
        y2, _, rdy = rx.sync_timing_extract(y, b)
        return y2.reshape(F, -1) if rdy[0] else None                               # an extract that underflows holds its symbols for the next call

    def align(self, sym):
        """-> (delay, flags, tri, aligned)"""
        if self.agc:
            sym = self.rx.agc(sym, n_frames=len(sym), output_energy=1.0).reshape(len(sym), -1)     # mult_agc: DVBS2.cpp:653-657
        out = self.rx.sync_frame_synchronize(sym, with_flags=True)
        if self.pls_check:
            self.pls = self.rx.pls_decode(out[3])
        return out

    def fine_sync(self, aligned):
        desc = self.rx.pl_descramble(aligned)
        if self.lr:
            _, _, desc = self.rx.sync_lr_synchronize(desc)
        return self.rx.sync_freq_phase_synchronize(desc)[2]

    def decode(self, aligned):
        """-> bits [frames, K_bch]; packets: (packets [n, UPLB], status [n], hdr [frames, 8]) instead, the BBFRAME parser behind the chain"""
        rx = self.rx
        pilots = self.estimator == "PILOTS" and self.sigma is None
        if not self.fine:
            sigma = rx.estimate_pilots(aligned, scrambled=True)[0] if pilots else self.sigma
            return rx.rx_bb_up(aligned, sigma=sigma)[:3] if self.packets else rx.rx_bb(aligned, sigma=sigma)[0]
        desc = self.fine_sync(aligned)
        xf = rx.remove_plh(desc)
        if pilots:
            sig = rx.estimate_pilots(desc, scrambled=False)[0]
        else:
            sig = rx.estimate(xf)[0] if self.sigma is None else np.full(len(aligned), self.sigma, np.float32)
        vk, _ = rx.decode_siho(rx.demodulate(sig, xf, deinterleave=True))
        bits = rx.bb_descramble(rx.decode_hiho(vk)[0])
        return rx.bbframe_parse(bits) if self.packets else bits


class LockTracker:
    """The frame synchronizer's delay, frame by frame (update(delay) -> stable): `stable` frames since it last moved, `moved` moves after the first 8 frames (the acquisition's own)."""

    def __init__(self):
        self.frames = self.stable = self.moved = 0
        self.delay = None

    def update(self, delay):
        self.frames += 1
        same = self.delay is not None and delay == self.delay
        self.stable = self.stable + 1 if same else 0
        self.moved += not same and self.frames > 8
        self.delay = int(delay)
        return self.stable


def add_timing_args(ap, learn_default):
    """--stm-type, --stm-hold-size, --stm-learn-frames; learn_default None: the sum of --wl-frames"""
    ap.add_argument("--stm-type", default="PERFECT", choices=["PERFECT", "FAST", "ULTRA"], help="symbol timing: PERFECT takes every osf-th sample from a known offset (the default here); "
                                                                                     "FAST runs the reference's Gardner loop (Synchronizer_Gardner_fast_osf2) on the GPU; "
                                                                                     "ULTRA its held form (Synchronizer_Gardner_ultra_osf2), a wave per stream")
    ap.add_argument("--stm-hold-size", type=int, default=101, help="ULTRA: samples per hold block; mu is held over all but the last four of them once the loop holds")
    ap.add_argument("--stm-learn-frames", type=int, default=learn_default, help="ULTRA: frames the whole loop runs on every sample before it starts to hold (the reference's learning phases, "
                                                                                "then set_act(true), main_sched.cpp:655); default: " +
                                                                                ("the sum of --wl-frames" if learn_default is None else "%(default)s, the learning phases' 150 + 150 + 200"))
