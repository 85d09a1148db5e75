"""Variable coding and modulation above the C ABI: a stream whose MODCOD changes from one PL frame to the next, made and received with one handle per MODCOD.

  VcmTransmitter   PL frames in the order of a cyclic schedule [(name, count), ...], each run by its MODCOD's tx_bb, the concatenation through one shaping filter
  VcmReceiver      symbols at one sample per symbol, in pieces of any size -> the decoded frames in stream order.  Acquisition once per lock on the host
                   (params.find_vcm_start on one pls_scan), then per push one dvbs2hip_pls_walk_dev -- every frame's start and value and a pointer table per value, on the
                   GPU -- one copy of its RES and CNT to the host, and per value the located estimator and the located fused chain of that MODCOD's handle, all handles on
                   the base handle's stream.

Out of scope: carrier or phase recovery across MODCODs, the frame synchronizer's delay line, BBFRAMEs and transport streams (DFL changes with the MODCOD), frames without
pilots, transmitting dummy frames (the receiver steps over those it meets).  Nothing here computes on the CPU but the bookkeeping."""
from __future__ import annotations

import numpy as np

from . import params as P

END, LOST, FULL = 0, 1, 2
ACQ_SYMBOLS = 2 * 33282 + 90       # acquisition looks at this many symbols at most: two frames of the longest MODCOD and a header (rx --mod-cod AUTO's window)


def parse_schedule(text: str):
    """`NAME:COUNT[,NAME:COUNT...]` -> [(name, count), ...]; ValueError with one sentence on anything else"""
    out = []
    for part in text.split(","):
        name, sep, count = part.rpartition(":")
        if not sep or not name or not count.strip().isdigit():
            raise ValueError("--mod-cod-seq takes NAME:COUNT[,NAME:COUNT...], for instance QPSK-S_3/5:3,16APSK-S_8/9:2 (got '%s')" % part)
        if int(count) < 1:
            raise ValueError("--mod-cod-seq: a COUNT has to be at least 1 (got '%s')" % part)
        out.append((P.get_modcod(name.strip()).name, int(count)))
    return out


class VcmTransmitter:
    """schedule: [(name, count), ...], repeated cyclically.  One handle per MODCOD; the first one's shaping filter serves the stream, its memory carried across calls."""

    def __init__(self, schedule, device: int = 0, seed: int = 0):
        from .receiver import Dvbs2Hip
        if not schedule:
            raise ValueError("the schedule is empty")
        self.schedule = [(P.get_modcod(n).name, int(c)) for n, c in schedule]
        if any(c < 1 for _, c in self.schedule):
            raise ValueError("a schedule entry's count has to be at least 1")
        self.h = {}
        for name, _ in self.schedule:
            if name not in self.h:
                self.h[name] = Dvbs2Hip(name, max_frames=max(c for n, c in self.schedule if n == name), device=device)
        self.shaper = self.h[self.schedule[0][0]]
        self.seed, self.calls = int(seed), 0                                       # tx_bb's random payloads: call c of the stream takes seed (seed << 32) + c
        self.entry, self.done = 0, 0                                               # the schedule entry the next frame belongs to, and the frames of it already sent

    def frames(self, n_frames: int):
        """the next n_frames PL frames -> (sent: [(name, bits int32[K_bch]), ...] in stream order, pl float32[2 * symbols], the frames back to back)"""
        sent, pl = [], []
        while len(sent) < n_frames:
            name, count = self.schedule[self.entry]
            n = min(count - self.done, n_frames - len(sent))
            bits, x = self.h[name].tx_bb(n, seed=(self.seed << 32) + self.calls)
            self.calls += 1
            sent += [(name, b) for b in bits]
            pl.append(x.reshape(-1))
            self.done += n
            if self.done == count:
                self.entry, self.done = (self.entry + 1) % len(self.schedule), 0
        return sent, np.concatenate(pl)

    def samples(self, n_frames: int, osf: int = 2):
        """-> (sent, the frames through the shaping filter: float32[2 * osf * symbols])"""
        sent, pl = self.frames(n_frames)
        return sent, self.shaper.shape_filter(pl, n_frames=1, osf=osf)

    def flush(self, osf: int = 2, grp_delay: int = 20):
        """the end of a transmission: 2 grp_delay zero symbols through the shaping filter, the samples that carry the last frame's last symbols through this filter's
        group delay and the receiver's matched filter's -> float32[2 * osf * 2 * grp_delay]"""
        return self.shaper.shape_filter(np.zeros(2 * 2 * grp_delay, np.float32), n_frames=1, osf=osf)

    def close(self):
        for h in self.h.values():
            h.close()
        self.h = {}


class VcmReceiver:
    """max_frames: frames per call of a MODCOD's decoder; estimator: "DVBS2" (M2M4 inside the fused chain) or "PILOTS" (estimate_pilots_located_dev in front of it).
    LEN: the walk's table, default params.VCM_FRAME_SYMBOLS; a value it knows and the library cannot decode (the dummy frame) is stepped over and counted.
    stats: frames per MODCOD name, skipped, losses of lock, frames whose LDPC or BCH flag is down."""

    def __init__(self, max_frames: int = 8, n_ite: int = 50, alpha: float = 1.0, implem: str = "NMS", early_stop: bool = True, estimator: str = "DVBS2", device: int = 0,
                 LEN=None, q_min: float = None, max_out: int = 4096):
        import torch
        from .receiver import Dvbs2Hip
        if estimator not in ("DVBS2", "PILOTS"):
            raise ValueError("estimator is DVBS2 or PILOTS")
        self.torch, self.dev = torch, torch.device("cuda", device)
        self.kw = dict(max_frames=int(max_frames), n_ite=n_ite, alpha=alpha, implem=implem, early_stop=early_stop, device=device)
        self.F, self.estimator, self.max_out = int(max_frames), estimator, int(max_out)
        self.LEN = np.ascontiguousarray(P.VCM_FRAME_SYMBOLS if LEN is None else LEN, np.int32)
        self.q_min = P.PLS_SEARCH_Q_MIN if q_min is None else float(q_min)
        ok = self.LEN[(self.LEN >= 90) & (self.LEN % 18 == 0)]
        if not ok.size:
            raise ValueError("LEN holds no frame length")
        self.min_len = int(ok.min())
        self.base = Dvbs2Hip("", **self.kw)                                        # owns the stream; serves its own MODCOD too
        self.h = {self.base.mc.name: self.base}
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_len = torch.from_numpy(self.LEN).to(self.dev)
        self.d_off, self.d_val, self.d_idx, self.d_cr = i32(self.max_out), i32(self.max_out), i32(self.max_out), i32(260)      # CNT and RES side by side: one copy
        self.d_q = torch.zeros(self.max_out, dtype=torch.float32, device=self.dev)
        self.d_src = torch.zeros(self.max_out, dtype=torch.int64, device=self.dev)
        self.d_sig = torch.zeros(self.F, dtype=torch.float32, device=self.dev)
        self.reset()                                                               # tail: the symbols carried; pos: the stream's symbol index of tail[0]

    def reset(self):
        """a new stream: nothing carried, not in lock, the counters at zero (the handles stay)"""
        self.tail, self.pos, self.locked = np.zeros(0, np.float32), 0, False
        self.stats = dict(frames={}, skipped=0, losses=0, ldpc_down=0, bch_down=0)

    def handle(self, name):
        """the MODCOD's handle, made on first use on the base handle's stream"""
        if name not in self.h:
            from .receiver import Dvbs2Hip
            self.h[name] = Dvbs2Hip(name, stream=self.base.stream, **self.kw)
        return self.h[name]

    def close(self):
        for h in self.h.values():
            if h is not self.base:
                h.close()
        self.base.close()
        self.h = {}

    def _acquire(self, buf, a0):
        """-> the symbol of a first header at or behind a0, None when the symbols from a0 show no chain"""
        n = min(len(buf) // 2 - a0, ACQ_SYMBOLS)
        k = P.find_vcm_start(*self.base.pls_scan(buf[2 * a0:2 * (a0 + n)]), self.LEN, self.q_min)
        return None if k is None else a0 + k

    def _decode(self, xd, n_sym, c):
        """one walk from symbol c of the device buffer and the decodes of its frames -> (frames in stream order, NEXT, STATUS)"""
        torch, base = self.torch, self.base
        max_out = min(self.max_out, (n_sym - c) // self.min_len + 1)                # no more frames fit; the walk sizes its jump table by max_out
        base.pls_walk_dev(xd.data_ptr(), n_sym, c, self.d_len.data_ptr(), self.q_min, max_out, self.d_off.data_ptr(), self.d_val.data_ptr(), self.d_q.data_ptr(),
                          self.d_src.data_ptr(), self.d_idx.data_ptr(), self.d_cr.data_ptr(), self.d_cr.data_ptr() + 4 * 256)
        base.synchronize()
        cr = self.d_cr.cpu().numpy()                                               # the one round trip ahead of the decodes
        CNT, (N, NEXT, STATUS, _) = cr[:256], (int(v) for v in cr[256:])
        first = np.concatenate([[0], np.cumsum(CNT)])
        out = {}
        for v in np.flatnonzero(CNT):
            name, pilots = P.pls_name(int(v))
            if name is None or not pilots or P.get_modcod(name).pl_frame != self.LEN[v]:      # (a caller's length that is not the decoder's frame: not its frame)
                self.stats["skipped"] += int(CNT[v])
                continue
            h, n = self.handle(name), int(CNT[v])
            info = torch.empty((n, h.K_bch), dtype=torch.int32, device=self.dev)
            cw = torch.zeros((2, n), dtype=torch.int8, device=self.dev)
            torch.cuda.synchronize(self.dev)                                       # (torch's allocations and fills are on its own stream)
            for a in range(0, n, self.F):
                f = min(self.F, n - a)
                src = self.d_src.data_ptr() + 8 * (int(first[v]) + a)
                sig = None
                if self.estimator == "PILOTS":
                    sig = self.d_sig.data_ptr()
                    h.estimate_pilots_located_dev(src, True, sig, None, None, f)
                h.rx_bb_located_dev(src, sig, info.data_ptr() + 4 * h.K_bch * a, cw.data_ptr() + a, cw.data_ptr() + n + a, f)
            out[int(v)] = (name, info, cw)
        base.synchronize()                                                         # every handle is on the base handle's stream
        OFF, IDX = self.d_off[:N].cpu().numpy(), self.d_idx[:N].cpu().numpy()
        place = np.empty(N, np.int64)
        place[IDX] = np.arange(N)                                                  # frame j stands at place[j] of the grouped tables
        host = {v: (name, info.cpu().numpy(), cw.cpu().numpy()) for v, (name, info, cw) in out.items()}
        val = np.repeat(np.arange(256), CNT)                                       # the value of every place
        frames = []
        for j in range(N):
            v = int(val[place[j]])
            if v not in host:
                continue
            name, info, cw = host[v]
            g = int(place[j] - first[v])
            frames.append((self.pos + int(OFF[j]), v, name, info[g], int(cw[0, g]), int(cw[1, g])))
            self.stats["frames"][name] = self.stats["frames"].get(name, 0) + 1
            self.stats["ldpc_down"] += int(not cw[0, g])
            self.stats["bch_down"] += int(not cw[1, g])
        return frames, NEXT, STATUS

    def push(self, symbols, n_valid: int = None):
        """symbols: float32[2 n], the stream's next n symbols -> [(offset, value, name, bits int32[K_bch], cwd_ldpc, cwd_bch), ...] of the frames this push completed, in
        stream order; offset counts the stream's symbols from the first one ever pushed.  n_valid: only that many of the n symbols are the stream's, the rest pads its end
        (what a matched filter needs to give up its last symbols): a header missed behind them is the end of the stream, not a loss of lock."""
        torch = self.torch
        new = np.asarray(symbols, np.float32).reshape(-1)
        buf = np.concatenate([self.tail, new])
        n_sym = buf.size // 2
        real = n_sym if n_valid is None else n_sym - (new.size // 2 - int(n_valid))
        if n_sym > (1 << 24):
            raise ValueError("a push and the carried tail hold %d symbols, the walk takes %d: push smaller pieces" % (n_sym, 1 << 24))
        frames, c, keep, xd = [], 0, 0, None
        while True:
            if not self.locked:
                if n_sym - keep < 90:
                    break
                c = self._acquire(buf, keep)
                if c is None:
                    if n_sym - keep < ACQ_SYMBOLS:
                        break                                                      # too little to say: wait for more
                    keep += int(self.LEN.max())                                    # no chain starts in here
                    continue
                self.locked = True
            if n_sym - c < 90:
                keep = c
                break
            if xd is None:
                xd = torch.from_numpy(buf).to(self.dev)
                torch.cuda.synchronize(self.dev)
            got, c, status = self._decode(xd, n_sym, c)
            frames += got
            keep = c
            if status == END:
                break
            if status == LOST:
                self.locked = False
                if c >= real:
                    keep = n_sym                                                   # the padding behind the stream's end
                    break
                self.stats["losses"] += 1
        self.tail = buf[2 * keep:].copy()
        self.pos += keep
        return frames
