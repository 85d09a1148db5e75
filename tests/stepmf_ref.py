"""CPU references for the coarse-frequency loop (test infrastructure): the C twin (tests/stepmf_twin.c, compiled on first use with the system compiler and -O2
-ffp-contract=off, loaded with ctypes) driven stream by stream like libdvbs2hip's S-stream calls and sharing the timing twin's state (tests/timing_ref.py), and a
pure-Python restatement in numpy float32 scalars, written module by module from the reference's sources, that pins the twin itself."""
import ctypes as C

import numpy as np

import timing_ref as TR
import twin_build

_lib = None


class SfcState(C.Structure):
    _fields_ = [("prev", C.c_float * 2), ("pprev", C.c_float * 2), ("lfs", C.c_float), ("ifs", C.c_float), ("dds", C.c_float), ("est", C.c_float),
                ("nu_k", C.c_int), ("n", C.c_int), ("curr_idx", C.c_int), ("last_delay", C.c_int)]


def lib():
    global _lib
    if _lib is None:
        L = twin_build.load("stepmf_twin.c")
        fp, vp, i, f = C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_float
        L.twin_pll_gains.argtypes = [i, f, f, fp, fp]
        L.twin_pilots.argtypes = [vp, i, vp, i]
        L.twin_stepmf.argtypes = [C.POINTER(TR.StmState), C.POINTER(SfcState), vp, vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, f, f, f, f, f]
        L.twin_nco_turn_worst.restype = C.c_double
        L.twin_nco_turn.argtypes = [i, fp, fp]
        L.twin_nco_index.argtypes = [i, i]
        L.twin_nco_index.restype = i
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pll_gains(pll_sps=1, damping=np.float32(0.5 ** 0.5), nbw=1e-4):
    pg, ig = C.c_float(), C.c_float()
    lib().twin_pll_gains(int(pll_sps), float(np.float32(damping)), float(np.float32(nbw)), C.byref(pg), C.byref(ig))
    return np.float32(pg.value), np.float32(ig.value)


def pl_sequence():
    from oracle import oracle as O
    return np.ascontiguousarray(O.pl_rand_seq(), np.uint8)


def pilots(n_p):
    seq = pl_sequence()
    P = np.zeros(2 * n_p, np.float32)
    lib().twin_pilots(_p(seq), seq.size, _p(P), n_p)
    return P


def taps81():
    from dvbs2_amd import params as P
    t = np.ascontiguousarray(P.rrc_taps(0.2, 2, 20), np.float32)
    assert t.size == 81 and np.array_equal(t, t[::-1])
    return t


class StepMf:
    """S streams of Synchronizer_step_mf_cc on the twin, frames stream-major; `timing` (a timing_ref.Timing) lends its per-stream loop state and carry buffers, so that
    its synchronize / extract carry on from the loop as libdvbs2hip's do."""

    def __init__(self, pl_frame, S=1, timing=None):
        self.pl, self.N, self.S = pl_frame, 2 * pl_frame, S
        self.tm = timing if timing is not None else TR.Timing(pl_frame, S)
        self.taps = taps81()
        self.n_p = 2 * pl_frame
        self.P = pilots(self.n_p)
        self.cf = [SfcState() for _ in range(S)]
        self.ring = [np.zeros(160, np.float32) for _ in range(S)]
        self.set_pll()
        self.reset_coarse()

    def set_pll(self, pll_sps=1, damping=np.float32(0.5 ** 0.5), nbw=1e-4):
        self.pg, self.ig = pll_gains(pll_sps, damping, nbw)

    def reset_coarse(self):
        for c in self.cf:
            ld = c.last_delay
            C.memset(C.byref(c), 0, C.sizeof(c))
            c.curr_idx, c.last_delay = self.pl - 1, ld

    def reset(self):
        """Synchronizer_step_mf_cc::reset: coarse, matched filter, timing"""
        self.reset_coarse()
        for r in self.ring:
            r[:] = 0
        self.tm.reset()

    def set_freq(self, estimated_freq):
        for c in self.cf:
            c.nu_k = int(np.floor(np.float32(-np.float32(estimated_freq)) * np.float32(1e6)))

    def synchronize(self, DEL, X):
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 2 * self.N)
        F = X.shape[0]
        Fs = F // self.S
        D = np.ascontiguousarray(DEL, np.int32).ravel()
        assert D.size == F
        Y, B = np.empty_like(X), np.empty(X.shape, np.int32)
        MU, FRQ, PHS = (np.empty(F, np.float32) for _ in range(3))
        for s in range(self.S):
            sl = slice(s * Fs, (s + 1) * Fs)
            x, y, b, mu, frq, phs, d = X[sl], Y[sl], B[sl], MU[sl], FRQ[sl], PHS[sl], D[sl]
            lib().twin_stepmf(C.byref(self.tm.st[s]), C.byref(self.cf[s]), _p(self.ring[s]), _p(self.taps), _p(self.P), self.n_p, _p(d), int(self.tm.head[s]) // 2,
                              _p(x), _p(y), _p(b), _p(mu), _p(frq), _p(phs), Fs, self.N, self.pl, float(self.tm.kp), float(self.tm.ki), float(self.pg), float(self.ig), 2.0)
        return MU, FRQ, PHS, Y, B


# ------------------------------------------------------------------ the pure-Python restatement: one object per module of the reference, numpy float32 scalars throughout
f32 = np.float32


def py_turn_cs(p):
    """dvbs2_amd/csrc/nco_turn.h in numpy float32 scalars"""
    octant, r = divmod(int(p), 125000)
    if octant & 1:
        r = 125000 - r
    x = f32(r) * f32(6.2831853071795865e-6)
    x2 = x * x
    ps = x2 * f32(2.7557319223985893e-6)
    ps = x2 * (ps - f32(1.9841269841269841e-4))
    ps = x2 * (ps + f32(8.3333333333333333e-3))
    ps = x2 * (ps - f32(1.6666666666666667e-1))
    ps = x * (ps + f32(1))
    pc = x2 * f32(2.4801587301587302e-5)
    pc = x2 * (pc - f32(1.3888888888888889e-3))
    pc = x2 * (pc + f32(4.1666666666666667e-2))
    pc = x2 * (pc - f32(0.5))
    pc = pc + f32(1)
    c, s = (ps, pc) if octant in (1, 2, 5, 6) else (pc, ps)
    return (-c if 2 <= octant <= 5 else c), (-s if octant >= 4 else s)


class PyMultiplierSine:
    """Multiplier_sine_ccc_naive: nu kept as the whole number of millionths that set_nu's floor leaves, n the sample counter; the phase is the exact turn fraction"""

    def __init__(self):
        self.k, self.n = 0, 0

    def set_nu(self, nu):
        self.k = int(np.floor(f32(nu) * f32(1e6)))

    def step(self, xr, xi):
        c, s = py_turn_cs((self.k % 1000000) * self.n % 1000000)
        self.n = 0 if self.n >= 999999 else self.n + 1
        return xr * c - xi * s, xr * s + xi * c


class PyMatchedFilter:
    """Filter_FIR_ccr_naive::step with the order of additions of stepmf_twin.c's header"""

    def __init__(self, taps):
        self.t = np.asarray(taps, np.float32)
        self.wr, self.wi = np.zeros(81, np.float32), np.zeros(81, np.float32)        # oldest first

    def step(self, zr, zi):
        out = []
        for w, z in ((self.wr, zr), (self.wi, zi)):
            w[:-1] = w[1:]
            w[80] = z
            prod = self.t[:40] * (w[:40] + w[80:40:-1])
            a = np.cumsum(prod.reshape(10, 4), axis=0, dtype=np.float32)[-1]          # a_j: the products i = j, j + 4, .. in increasing i, one float32 sum at a time
            out.append(((a[0] + a[1]) + (a[2] + a[3])) + self.t[40] * w[40])
        return out[0], out[1]


class PyGardnerStep:
    """Synchronizer_Gardner_fast_osf2::step (.hxx:8-87) with Filter_Farrow_ccr_naive"""

    def __init__(self, kp, ki):
        self.kp, self.ki = f32(kp), f32(ki)
        self.h = [(f32(0), f32(0))] * 3
        self.T0 = self.T1 = (f32(0), f32(0))
        self.mu = self.nco = self.lfp = self.lfo = f32(0)
        self.is_strobe = self.prev_is_strobe = 0
        self.last = (f32(0), f32(0))
        self.set_mu(self.mu)

    def set_mu(self, mu):
        hm = f32(0.5) * mu
        hms = hm * mu
        self.b = (hms - hm, f32(1) - hm - hms, mu + hm - hms)

    def step(self, xr, xi):
        b0, b1, b2 = self.b
        (h1r, h1i), (h2r, h2i), (h3r, h3i) = self.h
        yr = (h3r * b0 + h2r * b1) + (h1r * b2 + xr * b0)
        yi = (h3i * b0 + h2i * b1) + (h1i * b2 + xi * b0)
        self.h = [(xr, xi), self.h[0], self.h[1]]
        B = self.is_strobe
        if B == 1:
            self.last = (yr, yi)
        hist = self.is_strobe + 2 * self.prev_is_strobe               # TED_update
        e = f32(0)
        if hist == 1:
            e = self.T1[0] * (self.T0[0] - yr) + self.T1[1] * (self.T0[1] - yi)
            self.T0, self.T1 = (f32(0), f32(0)), (yr, yi)
        elif hist != 0:
            self.T0, self.T1 = self.T1, (yr, yi)
        vp = e * self.kp                                              # loop_filter
        vi = self.lfp + e * self.ki
        self.lfp = vi
        self.lfo = vp + vi
        W = self.lfo + f32(0.5)                                       # interpolation_control
        self.prev_is_strobe = self.is_strobe
        self.is_strobe = int(self.nco < W)
        if self.is_strobe:
            self.mu = self.nco / W
            self.set_mu(self.mu)
            self.nco = self.nco + f32(1)
        self.nco = self.nco - W
        return yr, yi, B, hist


class PyCoarse:
    """Synchronizer_freq_coarse_DVBS2_aib: step, update_phase, set_PLL_coeffs' gains handed in"""

    def __init__(self, pl_frame, P, pg, ig):
        self.length_max = pl_frame
        self.P = np.asarray(P, np.float32).reshape(-1, 2)
        self.pg, self.ig = f32(pg), f32(ig)
        self.mult = PyMultiplierSine()
        self.prev = self.pprev = (f32(0), f32(0))
        self.lfs = self.ifs = self.dds = self.est = f32(0)
        self.curr_idx = pl_frame - 1
        self.branches = [0, 0, 0]                                     # pilot window, the clearing at rem_pos 90, neither

    def update_phase(self, sr, si):
        ci = self.curr_idx
        rem = ci % 1476
        if 54 <= rem < 90 and ci >= 1530:
            p2r, p2i = self.P[(ci - 2) % self.length_max]
            pcr, pci = self.P[ci] if ci < len(self.P) else (f32(0), f32(0))
            ar, ai = sr * p2r - si * p2i, sr * p2i + si * p2r
            br, bi = self.pprev[0] * pcr - self.pprev[1] * pci, self.pprev[0] * pci + self.pprev[1] * pcr
            err = ai * br - ar * bi
            self.lfs = self.lfs + err * self.ig
            self.ifs = self.ifs + self.dds
            self.dds = err * self.pg + self.lfs
            self.est = self.ifs / f32(2)
            self.mult.set_nu(-self.est)
            self.pprev, self.prev = self.prev, (sr, si)
            self.branches[0] += 1
        elif rem == 90 and ci >= 1530:
            self.prev = self.pprev = (f32(0), f32(0))
            self.branches[1] += 1
        else:
            self.branches[2] += 1
        self.curr_idx = (ci + 1) % self.length_max


def py_stepmf(X, DEL, pl_frame, taps, P, kp, ki, pg, ig, n0=0, nu_k0=0, last_delay=0, carry_cplx=0):
    """Synchronizer_step_mf_cc::synchronize over len(DEL) frames of one stream from the reset state (with the counter at n0 and nu at nu_k0 millionths) ->
    dict(Y complex64, B, MU, FRQ, hist, nu_k per sample, the PyCoarse and PyGardnerStep objects)"""
    x = np.asarray(X, np.float32).reshape(-1, 2)
    N = 2 * pl_frame
    sfc, mf, stm = PyCoarse(pl_frame, P, pg, ig), PyMatchedFilter(taps), PyGardnerStep(kp, ki)
    sfc.mult.n, sfc.mult.k = n0, nu_k0
    N_out = 2 * N
    Y, B, H, K, MU, FRQ = [], [], [], [], [], []
    for f, d in enumerate(DEL):
        sfc.curr_idx = (N_out - int(d) + last_delay) % (N_out // 2)
        last_delay = carry_cplx
        for xr, xi in x[f * N:(f + 1) * N]:
            zr, zi = sfc.mult.step(xr, xi)
            mr, mi = mf.step(zr, zi)
            yr, yi, b, hist = stm.step(mr, mi)
            if b == 1:
                sfc.update_phase(*stm.last)
            Y.append(complex(yr, yi)); B.append(b); H.append(hist); K.append(sfc.mult.k)
        MU.append(stm.mu); FRQ.append(sfc.est)
    return dict(Y=np.array(Y, np.complex64), B=np.array(B, np.int32), hist=np.array(H), nu_k=np.array(K), MU=np.array(MU, np.float32), FRQ=np.array(FRQ, np.float32),
                sfc=sfc, stm=stm, last_delay=last_delay)


# ------------------------------------------------------------------ test signals
_frames_cache = {}


def pl_frames(modcod, n_distinct, seed):
    """n_distinct PL frames (complex128 symbols) from the oracle's TX chain, random payloads"""
    key = (modcod, n_distinct, seed)
    if key not in _frames_cache:
        from oracle import oracle as O
        from helpers import chain
        ch = chain(O, modcod)
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n_distinct):
            plf, _ = ch.tx(rng.integers(0, 2, ch.mc.K_bch).astype(np.int32))
            out.append(plf[0::2].astype(np.float64) + 1j * plf[1::2].astype(np.float64))
        _frames_cache[key] = np.array(out)
    return _frames_cache[key]


def received_stream(modcod, F, freq, ebn0_db, seed, off=0, D=None, n_distinct=4, phase=0.3):
    """F frames of a receiver's input, float32 [F, 4 pl_frame]: PL frames (cycled) from symbol offset `off` -> SRRC shaping at two samples per symbol -> the channel's
    delay D (optional) -> a carrier offset of `freq` cycles per SAMPLE -> AWGN at Eb/N0 -> front AGC to 1 / osf per frame"""
    from dvbs2_amd import params as P
    from oracle import oracle as O
    mc = P.get_modcod(modcod)
    fr = pl_frames(modcod, n_distinct, seed)
    n = mc.pl_frame
    rng = np.random.default_rng(seed + 1)
    sym = np.concatenate([fr[i % n_distinct] for i in range(F + 1)])[off: off + F * n]
    up = np.zeros(2 * F * n, complex)
    up[::2] = sym
    tx = np.convolve(up, P.rrc_taps(0.2, 2, 20).astype(np.float64))[: 2 * F * n]
    if D is not None:
        X = np.empty(2 * tx.size, np.float32)
        X[0::2], X[1::2] = tx.real, tx.imag
        z = TR.ChannelDelay(D)(X).astype(np.float64)
        tx = z[0::2] + 1j * z[1::2]
    t = np.arange(tx.size)
    tx = tx * np.exp(1j * (phase + 2 * np.pi * freq * t))
    sigma = P.esn0_to_sigma(P.ebn0_to_esn0(ebn0_db, mc.K_bch / mc.N_ldpc, mc.bps))
    rx = tx + sigma * (rng.standard_normal(tx.size) + 1j * rng.standard_normal(tx.size))
    out = np.empty((F, 4 * n), np.float32)
    flat = out.reshape(-1)
    flat[0::2], flat[1::2] = rx.real, rx.imag
    for f in range(F):
        out[f] = O.agc(out[f], 0.5)
    return out


# ------------------------------------------------------------------ a stand-in for the Dvbs2Hip handle on the twins and the oracle: what dvbs2_amd/acquire.py drives, no GPU
class TwinHandle:
    """one stream, one frame per call: step_mf on the twin, extract / timing on the timing twin, the gain stages, the frame synchronizer, the block-wise shift and
    filter, the PL descrambler and the fine synchronizers on the oracle.  State is shared as in libdvbs2hip: the timing loop's, the coarse frequency and sample counter, the
    matched filter's memory.  `log` records the calls in order."""

    def __init__(self, modcod):
        from dvbs2_amd import params as P
        from oracle import oracle as O
        self.O, self.mc = O, P.get_modcod(modcod)
        self.pl = self.mc.pl_frame
        self.sm = StepMf(self.pl)
        self.sf = O.SyncFrame(self.pl)
        self.lr = O.SyncLR(self.pl)
        self.log = []
        self.pll = None

    def agc(self, x, n_frames=1, output_energy=1.0):
        x = np.asarray(x, np.float32).reshape(n_frames, -1)
        return np.concatenate([self.O.agc(f, output_energy) for f in x])

    def sync_coarse_set_pll(self, pll_sps=1, damping=0.5 ** 0.5, nbw=1e-4):
        self.log.append(("set_pll", pll_sps, float(nbw)))
        self.pll = (pll_sps, float(nbw))
        self.sm.set_pll(pll_sps, np.float32(damping), nbw)

    def sync_step_mf_synchronize(self, DEL, X):
        self.log.append(("step_mf", int(np.asarray(DEL).ravel()[0])))
        return self.sm.synchronize(DEL, X)

    def sync_timing_extract(self, Y, B):
        return self.sm.tm.extract(Y, B)

    def sync_timing_synchronize(self, X):
        self.log.append(("timing",))
        return self.sm.tm.synchronize(X)

    def sync_frame_synchronize(self, sym, with_flags=False):
        d, y = self.sf.synchronize(np.asarray(sym, np.float32).ravel())
        self.log.append(("frame", d))
        return np.array([d], np.int32), np.array([int(self.sf.packet_flag)], np.int32), np.array([self.sf.metric], np.float32), y.reshape(1, -1)

    def sync_step_mf_reset(self):
        self.log.append(("reset_step_mf",))
        self.sm.reset()

    def sync_frame_reset(self):
        self.log.append(("reset_frame",))
        self.sf.reset()

    def sync_timing_reset(self):
        self.log.append(("reset_timing",))
        self.sm.tm.reset()

    def sync_coarse_synchronize(self, X, n_frames=1):
        c = self.sm.cf[0]
        self.log.append(("shift", c.nu_k))
        z, n = self.O.nco(X, np.float32(c.nu_k) / np.float32(1e6), float(c.n))
        c.n = int(n)
        return np.array([c.est], np.float32), np.zeros(1, np.float32), z

    def filter(self, X, n_frames=1):
        return self.O.fir(self.sm.taps, self.sm.ring[0], X)

    def pl_descramble(self, X):
        return self.O.pl_scramble(np.asarray(X, np.float32).ravel(), 90, False)

    def sync_lr_synchronize(self, X):
        self.log.append(("lr",))
        return self.lr.synchronize(X)

    def sync_freq_phase_synchronize(self, X):
        self.log.append(("fine",))
        return self.O.sync_freq_phase(X)

    def sync_coarse_get_freq(self):
        return np.array([c.est for c in self.sm.cf], np.float32), np.array([np.float32(c.nu_k) / np.float32(1e6) for c in self.sm.cf], np.float32)


# ------------------------------------------------------------------ a recording stand-in: what dvbs2_amd/rx.py, tools/sync_in_loop.py and dvbs2_amd/acquire.py call, no GPU
class RecordingHandle:
    """Every method the three callers use appends [name, scalar arguments, crc32 of each array argument] to `log` and returns arrays of the handle's shapes and dtypes
    whose contents are a function of that entry alone, so equal logs mean the same tasks in the same order on the same data with the same scalars.  The timing
    extract's RDY and the frame synchronizer's packet flag follow a script: `not_ready` holds the extract calls (counted from 0) that underflow, `flag_from` the
    frame-synchronizer call from which the flag is up; delays are 7 but at the calls in `delay_moves`.  Subclass to set the script; `made` keeps the instances."""
    not_ready, flag_from, delay_moves = (), 0, ()
    made = None

    def __init__(self, modcod="QPSK-S_8/9", max_frames=1, **kw):
        from dvbs2_amd import params as P
        self.mc = P.get_modcod(modcod)
        self.n = self.mc.pl_frame
        self.log = []
        self.n_extract = self.n_frame_sync = 0
        if self.made is not None:
            self.made.append(self)
        self._rec("init", [modcod, max_frames] + [[k, kw[k]] for k in sorted(kw)])

    def _rec(self, name, scalars=(), *arrays):
        import zlib
        e = [name, [v if isinstance(v, (str, list, bool, type(None))) else float(v) for v in scalars], [zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]]
        self.log.append(e)
        return zlib.crc32(repr(e).encode())

    @staticmethod
    def _fill(seed, shape, dtype=np.float32, k=0):
        h = (np.arange(int(np.prod(shape)), dtype=np.uint32) + np.uint32(seed)) * np.uint32(2654435761) + np.uint32(k)
        h ^= h >> np.uint32(15)
        return ((h & np.uint32(1)).astype(np.int32) if dtype == np.int32 else (h & np.uint32(0xFFFF)).astype(np.float32) / np.float32(32768) - np.float32(1)).reshape(shape)

    def _same(self, name, X, scalars=()):
        """a task whose output has its input's size (float32, flat as libdvbs2hip's wrappers give it)"""
        return self._fill(self._rec(name, scalars, X), np.asarray(X).size)

    # setters and resets: scalars only
    def timing_enable(self, on=True): self._rec("timing_enable", [on])
    def sync_coarse_set_freq(self, estimated_freq): self._rec("sync_coarse_set_freq", [estimated_freq])
    def sync_timing_set_params(self, damping=0.5 ** 0.5, nbw=5e-5, detector_gain=2.0): self._rec("sync_timing_set_params", [damping, nbw, detector_gain])
    def sync_timing_set_type(self, stm_type="FAST", hold_size=101): self._rec("sync_timing_set_type", [stm_type, hold_size])
    def sync_timing_set_act(self, act=True): self._rec("sync_timing_set_act", [act])
    def sync_coarse_set_pll(self, pll_sps=1, damping=0.5 ** 0.5, nbw=1e-4): self._rec("sync_coarse_set_pll", [pll_sps, damping, nbw])
    def channel_set_delay(self, D): self._rec("channel_set_delay", [D])
    def channel_set_freq_shift(self, freq_shift): self._rec("channel_set_freq_shift", [freq_shift])
    def sync_step_mf_reset(self): self._rec("sync_step_mf_reset")
    def sync_frame_reset(self): self._rec("sync_frame_reset")
    def sync_timing_reset(self): self._rec("sync_timing_reset")
    def close(self): self._rec("close")

    def sync_coarse_get_freq(self):
        s = self._rec("sync_coarse_get_freq")
        return self._fill(s, 1), self._fill(s, 1, k=1)

    # the receiver's tasks
    def agc(self, X_N, n_frames=1, output_energy=1.0): return self._same("agc", X_N, [n_frames, output_energy])
    def filter(self, X_N1, n_frames=1): return self._same("filter", X_N1, [n_frames])
    def pl_descramble(self, Y_N1): return self._same("pl_descramble", Y_N1).reshape(-1, 2 * self.n)

    def sync_coarse_synchronize(self, X_N1, n_frames=1):
        s = self._rec("sync_coarse_synchronize", [n_frames], X_N1)
        return self._fill(s, n_frames), self._fill(s, n_frames, k=1), self._fill(s, np.asarray(X_N1).size, k=2)

    def sync_timing_synchronize(self, X_N1):
        X = np.asarray(X_N1).reshape(-1, 4 * self.n)
        s = self._rec("sync_timing_synchronize", (), X)
        return self._fill(s, X.shape), self._fill(s, X.shape, np.int32, k=1), self._fill(s, X.shape[0], k=2)

    def sync_timing_extract(self, Y_N1, B_N1, out=None):
        F = np.asarray(Y_N1).reshape(-1, 4 * self.n).shape[0]
        s = self._rec("sync_timing_extract", (), Y_N1, B_N1)
        rdy = np.array([self.n_extract not in self.not_ready], np.int32)
        self.n_extract += 1
        return self._fill(s, (F, 2 * self.n)), np.zeros(F, np.int32), rdy

    def sync_step_mf_synchronize(self, DEL, X_N1):
        X = np.asarray(X_N1).reshape(-1, 4 * self.n)
        s, F = self._rec("sync_step_mf_synchronize", (), DEL, X), X.shape[0]
        return self._fill(s, F), self._fill(s, F, k=1), self._fill(s, F, k=2), self._fill(s, X.shape, k=3), self._fill(s, X.shape, np.int32, k=4)

    def sync_frame_synchronize(self, X_N1, with_flags=False):
        X = np.asarray(X_N1).reshape(-1, 2 * self.n)
        s, F = self._rec("sync_frame_synchronize", [with_flags], X), X.shape[0]
        delay = np.full(F, 7 + 3 * (self.n_frame_sync in self.delay_moves), np.int32)
        flags = np.full(F, int(self.n_frame_sync >= self.flag_from), np.int32)
        self.n_frame_sync += 1
        return delay, flags, self._fill(s, F), self._fill(s, X.shape, k=1)

    def _sff(self, name, X_N1):
        X = np.asarray(X_N1).reshape(-1, 2 * self.n)
        s = self._rec(name, (), X)
        return self._fill(s, X.shape[0]), self._fill(s, X.shape[0], k=1), self._fill(s, X.shape, k=2)

    def sync_lr_synchronize(self, X_N1): return self._sff("sync_lr_synchronize", X_N1)
    def sync_freq_phase_synchronize(self, X_N1): return self._sff("sync_freq_phase_synchronize", X_N1)

    def remove_plh(self, Y_N1):
        F = np.asarray(Y_N1).reshape(-1, 2 * self.n).shape[0]
        return self._fill(self._rec("remove_plh", (), Y_N1), (F, 2 * self.mc.N_ldpc // self.mc.bps))

    def estimate(self, X_N):
        s, F = self._rec("estimate", (), X_N), len(X_N)
        return self._fill(s, F), self._fill(s, F, k=1), self._fill(s, F, k=2)

    def demodulate(self, CP, Y_N1, deinterleave=False): return self._fill(self._rec("demodulate", [deinterleave], CP, Y_N1), (len(Y_N1), self.mc.N_ldpc))

    def decode_siho(self, Y_N, with_post=False, out=None):
        s = self._rec("decode_siho", [with_post], Y_N)
        return self._fill(s, (len(Y_N), self.mc.K_ldpc), np.int32), self._fill(s, len(Y_N), np.int32, k=1)

    def decode_hiho(self, Y_N):
        s = self._rec("decode_hiho", (), Y_N)
        return self._fill(s, (len(Y_N), self.mc.K_bch), np.int32), self._fill(s, len(Y_N), np.int32, k=1)

    def bb_descramble(self, Y_N1): return self._fill(self._rec("bb_descramble", (), Y_N1), np.asarray(Y_N1).shape, np.int32)

    def rx_bb(self, pl_frames, sigma=None, out=None):
        F = np.asarray(pl_frames).reshape(-1, 2 * self.n).shape[0]
        s = self._rec("rx_bb", [sigma], pl_frames)
        return self._fill(s, (F, self.mc.K_bch), np.int32), self._fill(s, F, np.int32, k=1), self._fill(s, F, np.int32, k=2)

    # the tool's transmitter and channel
    def tx_bb(self, n_frames, info=None, seed=0, sigma=None):
        s = self._rec("tx_bb", [n_frames, seed, sigma], info)
        return info, self._fill(s, (n_frames, 2 * self.n))

    def shape_filter(self, X_N1, n_frames=1, osf=2): return self._fill(self._rec("shape_filter", [n_frames, osf], X_N1), np.asarray(X_N1).size * osf)
    def channel_delay(self, X): return self._same("channel_delay", X)
    def channel_freq_shift(self, X): return self._same("channel_freq_shift", X)
    def add_noise(self, sigma, X_N, seed=0, n_frames=1): return self._same("add_noise", X_N, [sigma, seed, n_frames])
