"""CPU references for the held Gardner loop (`--stm-type ULTRA`; test infrastructure): the C twin (tests/timing_ultra_twin.c, compiled on first use with the system compiler and
-O2 -ffp-contract=off, loaded with ctypes) driven stream by stream like libdvbs2hip's S-stream calls, and a NumPy restatement written the way the GPU kernel works -- per hold
block a vectorised Farrow filter and vectorised detector errors, two in-order float32 accumulations, four control steps -- which proves that decomposition to be the serial
algorithm bit for bit.  Also the inputs the CPU and the GPU tests share, with the coverage condition they assert on the twin's trace."""
import ctypes as C

import numpy as np

import timing_ref as TR
import twin_build

_lib = None

StmState = TR.StmState          # the same layout: the library keeps one state per stream for both loops


def lib():
    global _lib
    if _lib is None:
        L = twin_build.load("timing_ultra_twin.c")
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        L.twin_ultra_gains.argtypes = [C.c_float, C.c_float, C.c_float, fp, fp]
        L.twin_ultra_synchronize.argtypes = [C.POINTER(StmState), vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, vp]
        _lib = L
    return _lib


_p = TR._p


def gains(damping=np.float32(0.5 ** 0.5), nbw=5e-5, dg=2.0):
    kp, ki = C.c_float(), C.c_float()
    lib().twin_ultra_gains(float(np.float32(damping)), float(nbw), float(dg), C.byref(kp), C.byref(ki))
    return np.float32(kp.value), np.float32(ki.value)


class UltraTiming(TR.Timing):
    """S streams of the held loop, frames stream-major; `act` as Synchronizer_timing::set_act.  extract is the FAST twin's (the task is the same one).
    `first_hist` collects, per synchronize call and stream, the strobe history at every hold block's first held sample."""

    def __init__(self, pl_frame, H, S=1, damping=np.float32(0.5 ** 0.5), nbw=5e-5, dg=2.0, act=False):
        TR.Timing.__init__(self, pl_frame, S, damping, nbw, dg)
        self.kp, self.ki = gains(damping, nbw, dg)
        self.H = int(H)
        self.act = bool(act)
        self.first_hist = []

    def reset(self):
        TR.Timing.reset(self)
        self.act = False                      # Synchronizer_timing::reset clears it
        self.first_hist = []

    def synchronize(self, X):
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 2 * self.N)
        F = X.shape[0]
        Fs = F // self.S
        Y, B, MU = np.empty_like(X), np.empty(X.shape, np.int32), np.empty(F, np.float32)
        nb = self.N // self.H if self.act else 0
        for s in range(self.S):
            sl = slice(s * Fs, (s + 1) * Fs)
            x, y, b, mu = X[sl], Y[sl], B[sl], MU[sl]
            fh = np.full(max(Fs * nb, 1), -1, np.int32)
            lib().twin_ultra_synchronize(C.byref(self.st[s]), _p(x), _p(y), _p(b), _p(mu), Fs, self.N, self.H, int(self.act), float(self.kp), float(self.ki), _p(fh))
            self.first_hist.append(fh[: Fs * nb])
        return Y, B, MU


# ------------------------------------------------------------------------------------------------------------------ the restatement, shaped like the kernel
_f = np.float32
_HALF = _f(0.5)


def _taps(mu):
    hm = _HALF * mu
    hms = hm * mu
    return hms - hm, _f(1) - hm - hms, mu + hm - hms


class PyState:
    """reset state of one stream, in numpy float32 scalars"""

    def __init__(self):
        z = _f(0)
        self.h = [(z, z)] * 3                # x[n-1], x[n-2], x[n-3]
        self.T0 = self.T1 = (z, z)
        self.mu = self.nco = self.lfp = self.lfo = z
        self.is_s = self.prev = 0


def _ted_shift(st, hist, y):
    if hist in (1, 2):
        st.T0, st.T1 = st.T1, y
    elif hist == 3:
        st.T0, st.T1 = (_f(0), _f(0)), y


def _control(st, xr, xi, kp, ki):
    """one control sample: Farrow step, B, detector, loop filter, interpolation control -> (yr, yi, b)"""
    b0, b1, b2 = _taps(st.mu)
    (h1r, h1i), (h2r, h2i), (h3r, h3i) = st.h
    yr = (h3r * b0 + h2r * b1) + (h1r * b2 + xr * b0)
    yi = (h3i * b0 + h2i * b1) + (h1i * b2 + xi * b0)
    st.h = [(xr, xi), st.h[0], st.h[1]]
    b = st.is_s
    hist = 2 * st.prev + st.is_s
    st.prev = st.is_s
    e = _f(0)
    if hist == 1:
        e = st.T1[0] * (st.T0[0] - yr) + st.T1[1] * (st.T0[1] - yi)
    _ted_shift(st, hist, (yr, yi))
    vi = st.lfp + e * ki
    st.lfp = vi
    st.lfo = e * kp + vi
    W = st.lfo + _HALF
    st.is_s = int(st.nco < W)
    if st.is_s:
        st.mu = st.nco / W
        st.nco = st.nco + _f(1)
    st.nco = st.nco - W
    return yr, yi, b


def _held_block(st, x, kp, ki, yo, bo):
    """the n = H - 4 held samples of a block, data-parallel where the kernel is: x complex64[n] -> yo, bo filled; the state moved past them"""
    n = x.size
    b0, b1, b2 = _taps(st.mu)
    cr = np.concatenate([np.array([st.h[2][0], st.h[1][0], st.h[0][0]], _f), x.real.astype(_f)])
    ci = np.concatenate([np.array([st.h[2][1], st.h[1][1], st.h[0][1]], _f), x.imag.astype(_f)])
    yr = (cr[0:n] * b0 + cr[1:n + 1] * b1) + (cr[2:n + 2] * b2 + cr[3:n + 3] * b0)
    yi = (ci[0:n] * b0 + ci[1:n + 1] * b1) + (ci[2:n + 2] * b2 + ci[3:n + 3] * b0)
    st.h = [(cr[n + 2], ci[n + 2]), (cr[n + 1], ci[n + 1]), (cr[n], ci[n])]
    is0 = st.is_s
    isj = (is0 + np.arange(n)) & 1                       # the strobe alternates from is_strobe
    yo.real[:], yo.imag[:], bo[:] = yr, yi, isj
    hist0 = 2 * st.prev + is0
    # the detector's error of every held sample as if it were a strobe with history 1: for j >= 2 the buffer holds y[j-2], y[j-1] ...
    e = np.zeros(n, _f)
    if n > 2:
        e[2:] = yr[1:n - 1] * (yr[0:n - 2] - yr[2:]) + yi[1:n - 1] * (yi[0:n - 2] - yi[2:])
    # ... samples 0 and 1 take the carried buffer, through whatever history sample 0 has
    e[0] = st.T1[0] * (st.T0[0] - yr[0]) + st.T1[1] * (st.T0[1] - yi[0])
    if n > 1:
        if hist0 == 2:
            a0, a1 = st.T1, (yr[0], yi[0])
        elif hist0 == 0:
            a0, a1 = st.T0, st.T1
        else:                                                # sample 1 is no strobe then: its error is not used
            a0, a1 = (_f(0), _f(0)), (_f(0), _f(0))
        e[1] = a1[0] * (a0[0] - yr[1]) + a1[1] * (a0[1] - yi[1])
    used = isj == 1                                          # history 1 = a strobe behind a sample that was none: every strobe from sample 1 on ...
    used[0] = hist0 == 1                                     # ... and sample 0 when the carried history says so
    # the two in-order float32 accumulations: the integrator over the strobes, the NCO's half steps
    lfp = st.lfp
    for j in np.flatnonzero(used):
        lfp = lfp + e[j] * ki
    e_last = e[n - 1] if used[n - 1] else _f(0)
    if not used[n - 1]:
        lfp = lfp + e_last * ki
    st.lfp = lfp
    st.lfo = e_last * kp + lfp
    nco = st.nco
    for j in range(n):
        nco = nco + (_f(1 - isj[j]) - _HALF)
    st.nco = nco
    # the detector's buffer behind the block
    _ted_shift(st, hist0, (yr[0], yi[0]))
    if n > 1:
        st.T0, st.T1 = st.T1, (yr[1], yi[1])
    if n > 2:
        st.T0, st.T1 = (yr[n - 2], yi[n - 2]), (yr[n - 1], yi[n - 1])
    st.prev = int(isj[n - 1])
    st.is_s = int(1 - isj[n - 1])


def py_synchronize(st, X, N, H, act, kp, ki):
    """frames of N complex samples (float32 re/im interleaved) of one stream from the state `st` -> Y like X, B int32 like X, MU float32 per frame"""
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 2 * N)
    F = X.shape[0]
    Y, B, MU = np.empty((F, N), np.complex64), np.empty((F, N), np.int32), np.empty(F, np.float32)
    nb = N // H if act else 0
    for f in range(F):
        x = X[f].view(np.complex64)
        for k in range(nb + 1):
            if k < nb:
                _held_block(st, x[k * H: k * H + H - 4], kp, ki, Y[f, k * H: k * H + H - 4], B[f, k * H: k * H + H - 4])
            for i in (range(k * H + H - 4, k * H + H) if k < nb else range(nb * H, N)):       # a block's four control samples; behind the last block the tail
                yr, yi, b = _control(st, _f(x[i].real), _f(x[i].imag), kp, ki)
                Y[f, i] = complex(yr, yi)
                B[f, i] = b
        MU[f] = st.mu
    return Y.view(np.float32).reshape(F, 2 * N), np.repeat(B, 2, axis=1), MU


# ------------------------------------------------------------------------------------------------------------------ the inputs both test files use
HOLD_SIZES = (5, 6, 68, 69, 101)
NOISY = dict(damping=np.float32(0.5 ** 0.5), nbw=2e-2, dg=2.0)       # the fast loop of test_twin_equals_the_restatement_through_stuffing_and_skipping


def noisy_frames(pl_frame, F, seed, noise=0.3, D=5.0):
    """F frames of the loop's input: QPSK shaped, delayed, noisy, matched-filtered"""
    qpsk = np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2)
    return TR.shaped_stream(F * 2 * pl_frame, qpsk, D, noise, np.random.default_rng(seed)).reshape(F, -1)


def coverage(traces):
    """traces: [(H, first_hist array)] of act-on runs -> (count of each history at a block's first held sample over all of them, the same over the runs with more than 64
    held samples per block)"""
    allc, wide = np.zeros(4, int), np.zeros(4, int)
    for H, fh in traces:
        c = np.bincount(np.asarray(fh, int), minlength=4)[:4]
        allc += c
        if H - 4 > 64:
            wide += c
    return allc, wide


def assert_coverage(traces):
    allc, wide = coverage(traces)
    assert (allc >= 3).all() and (wide >= 1).all(), (allc.tolist(), wide.tolist())
