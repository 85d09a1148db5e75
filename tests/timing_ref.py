"""CPU references for the timing synchronizer and the channel's delay tasks (test infrastructure): the C twin (tests/timing_twin.c, compiled on first use with
the system compiler and -O2 -ffp-contract=off, loaded with ctypes) driven stream by stream like libdvbs2hip's S-stream calls, and a pure-Python restatement of
the Gardner loop in numpy float32 scalars that pins the twin itself."""
import ctypes as C

import numpy as np

import twin_build

_lib = None


class StmState(C.Structure):
    _fields_ = [("h", C.c_float * 6), ("ted", C.c_float * 4), ("mu", C.c_float), ("nco", C.c_float), ("lf_prev_in", C.c_float), ("lf_output", C.c_float),
                ("last", C.c_float * 2), ("is_strobe", C.c_int), ("prev_is_strobe", C.c_int)]


def lib():
    global _lib
    if _lib is None:
        L = twin_build.load("timing_twin.c")
        fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_void_p
        L.twin_gains.argtypes = [C.c_float, C.c_float, C.c_float, fp, fp]
        L.twin_synchronize.argtypes = [C.POINTER(StmState), vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float]
        L.twin_extract.argtypes = [vp, C.POINTER(C.c_longlong), C.c_longlong, vp, vp, vp, vp, vp, C.c_int, C.c_int]
        L.twin_extract.restype = C.c_int
        L.twin_channel_taps.argtypes = [C.c_float, vp]
        L.twin_channel_taps.restype = C.c_longlong
        L.twin_channel_delay.argtypes = [vp, C.c_longlong, vp, vp, vp, C.c_longlong]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def gains(damping=np.float32(0.5 ** 0.5), nbw=5e-5, dg=2.0):
    kp, ki = C.c_float(), C.c_float()
    lib().twin_gains(float(np.float32(damping)), float(nbw), float(dg), C.byref(kp), C.byref(ki))
    return np.float32(kp.value), np.float32(ki.value)


class Timing:
    """S streams of the timing synchronizer, frames stream-major as libdvbs2hip lays them out (stream s = frames [s F/S, (s+1) F/S))."""

    def __init__(self, pl_frame, S=1, damping=np.float32(0.5 ** 0.5), nbw=5e-5, dg=2.0):
        self.N = 2 * pl_frame                     # complex samples per frame (osf = 2)
        self.S = S
        self.kp, self.ki = gains(damping, nbw, dg)
        self.reset()

    def reset(self):
        self.st = [StmState() for _ in range(self.S)]
        self.carry = [None] * self.S
        self.head = [0] * self.S
        self.uf = None

    def synchronize(self, X):
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 2 * self.N)
        F = X.shape[0]
        Fs = F // self.S
        Y, B, MU = np.empty_like(X), np.empty(X.shape, np.int32), np.empty(F, np.float32)
        for s in range(self.S):
            sl = slice(s * Fs, (s + 1) * Fs)
            x, y, b, mu = X[sl], Y[sl], B[sl], MU[sl]
            lib().twin_synchronize(C.byref(self.st[s]), _p(x), _p(y), _p(b), _p(mu), Fs, self.N, float(self.kp), float(self.ki))
        return Y, B, MU

    def extract(self, Y, B, out=None):
        Y = np.ascontiguousarray(Y, np.float32).reshape(-1, 2 * self.N)
        B = np.ascontiguousarray(B, np.int32).reshape(-1, 2 * self.N)
        F = Y.shape[0]
        Fs = F // self.S
        cap = 4 * Fs * self.N
        Y2 = np.zeros((F, self.N), np.float32) if out is None else out
        UFW, RDY = np.empty(F, np.int32), np.empty(self.S, np.int32)
        if self.uf is None or self.uf.size != F:
            self.uf = np.zeros(F, np.int32)
        for s in range(self.S):
            c = np.zeros(cap, np.float32)
            if self.carry[s] is not None:
                k = min(self.head[s], cap)
                c[:k] = self.carry[s][:k]
            self.carry[s] = c
            head = C.c_longlong(self.head[s])
            sl = slice(s * Fs, (s + 1) * Fs)
            y2, ufw, uf = Y2[sl], UFW[sl], self.uf[sl]
            RDY[s] = lib().twin_extract(_p(c), C.byref(head), cap, _p(uf), _p(Y[sl]), _p(B[sl]), _p(y2), _p(ufw), Fs, self.N)
            self.uf[sl] = uf
            self.head[s] = head.value
        return Y2, UFW, RDY


class ChannelDelay:
    def __init__(self, D):
        self.b = np.zeros(3, np.float32)
        self.H = lib().twin_channel_taps(float(np.float32(D)), _p(self.b))
        self.hist = np.zeros(2 * self.H, np.float32)

    def __call__(self, X):
        X = np.ascontiguousarray(X, np.float32)
        Y = np.empty_like(X)
        lib().twin_channel_delay(_p(self.hist), self.H, _p(self.b), _p(X), _p(Y), X.size // 2)
        return Y


def py_synchronize(x, kp, ki):
    """the Gardner loop restated in numpy float32 scalars, one complex sample at a time from the reset state -> (y complex64, b int, mu after the last sample,
    the strobe history of every sample)"""
    f = np.float32
    half = f(0.5)

    def taps(mu):
        hm = half * mu
        hms = hm * mu
        return hms - hm, f(1) - hm - hms, mu + hm - hms

    hist = [np.complex64(0)] * 3            # x[n-1], x[n-2], x[n-3]
    T0 = T1 = (f(0), f(0))
    mu = nco = lfp = lfo = f(0)
    is_s = prev = 0
    b0, b1, b2 = taps(mu)
    ys, bs, hs = [], [], []
    for v in np.asarray(x, np.complex64):
        xr, xi = f(v.real), f(v.imag)
        h1, h2, h3 = hist
        yr = (h3.real * b0 + h2.real * b1) + (h1.real * b2 + xr * b0)
        yi = (h3.imag * b0 + h2.imag * b1) + (h1.imag * b2 + xi * b0)
        hist = [np.complex64(complex(xr, xi)), h1, h2]
        h = is_s + 2 * prev
        if h == 1:
            e = T1[0] * (T0[0] - yr) + T1[1] * (T0[1] - yi)
            lfp = lfp + e * ki
            lfo = lfp + e * kp
            T0, T1 = T1, (yr, yi)
        elif h == 2:
            T0, T1 = T1, (yr, yi)
            lfo = lfp
        elif h == 3:
            T0, T1 = (f(0), f(0)), (yr, yi)
            lfo = lfp
        else:
            lfo = lfp
        W = lfo + half
        prev, is_s = is_s, int(nco < W)
        if is_s:
            mu = nco / W
            b0, b1, b2 = taps(mu)
            nco = nco + (f(1) - W)
        else:
            nco = nco - W
        ys.append(complex(yr, yi))
        bs.append(1 if h in (1, 3) else 0)
        hs.append(h)
    return np.array(ys, np.complex64), np.array(bs, np.int32), mu, np.array(hs, np.int32)


def shaped_stream(n_cplx, points, D, noise, rng):
    """random symbols of `points` -> SRRC shaping at two samples per symbol (0.2, 81 taps) -> the twin's channel delay D -> AWGN -> matched filter:
    n_cplx samples of a timing synchronizer's input, float32 re/im interleaved"""
    from dvbs2_amd import params as P
    taps = P.rrc_taps(0.2, 2, 20).astype(np.float64)
    sym = np.asarray(points)[rng.integers(0, len(points), (n_cplx + 1) // 2)]
    up = np.zeros(n_cplx, complex)
    up[::2] = sym[: up[::2].size]
    tx = np.convolve(up, taps)[:n_cplx]
    X = np.empty(2 * n_cplx, np.float32)
    X[0::2], X[1::2] = tx.real, tx.imag
    z = ChannelDelay(D)(X).astype(np.float64)
    z = z[0::2] + 1j * z[1::2] + noise * (rng.standard_normal(n_cplx) + 1j * rng.standard_normal(n_cplx))
    mf = np.convolve(z, taps)[:n_cplx]
    M = np.empty(2 * n_cplx, np.float32)
    M[0::2], M[1::2] = mf.real, mf.imag
    return M
