"""CPU reference for the one-wave-per-stream form of the coarse-frequency loop (test infrastructure): tests/stepmf_wave_twin.c, the loop of stepmf_twin.c in the kernel's
chunk / ahead / cut order, driven like stepmf_ref.StepMf and reporting the cuts of every call; and the cases the GPU tests run (tests/test_stepmf_wave_gpu.py), so that the
CPU test can say what their inputs exercise (tests/test_stepmf_wave_twin.py)."""
import ctypes as C

import numpy as np

import stepmf_ref as SR
import timing_ref as TR
import twin_build
from dvbs2_amd import params as P

MODCOD = "QPSK-S_8/9"
PL = P.get_modcod(MODCOD).pl_frame
N = 2 * PL                                                              # complex samples per frame: 16740 = 261 * 64 + 36
CHUNK = 64

# (S, frames per call, calls, device-pointer form, seed of the streams): the cases of tests/test_stepmf_wave_gpu.py.  The last one is 64 frames = 1 071 360 samples of one
# stream: the sample counter wraps at 1e6 in call 14.  Seeds are test_stepmf_gpu.py's 10 S + Fs; the cut list they give is asserted in test_stepmf_wave_twin.py.
CASES = [(1, 1, 20, False, 11), (1, 4, 5, True, 14), (3, 7, 3, True, 37), (65, 1, 20, False, 651), (1, 4, 16, False, 15)]
PLL = (1, np.float32(0.5 ** 0.5), 1e-3)                                 # a fast PLL: nu moves from the first pilot block on

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = twin_build.load("stepmf_wave_twin.c")
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.twin_stepmf_wave.argtypes = [C.POINTER(TR.StmState), C.POINTER(SR.SfcState), vp, vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, f, f, f, f, f, vp, i]
        L.twin_stepmf_wave.restype = i
        _lib = L
    return _lib


class StepMfWave(SR.StepMf):
    """stepmf_ref.StepMf on the chunked twin; `cuts` collects (call, stream, sample index in the call, position in its chunk) of every cut"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cuts, self.n_calls = [], 0

    def synchronize(self, DEL, X):
        X = np.ascontiguousarray(X, np.float32).reshape(-1, 2 * self.N)
        F = X.shape[0]
        Fs = F // self.S
        D = np.ascontiguousarray(DEL, np.int32).ravel()
        assert D.size == F
        Y, B = np.empty_like(X), np.empty(X.shape, np.int32)
        MU, FRQ, PHS = (np.empty(F, np.float32) for _ in range(3))
        room = Fs * self.N                                              # a cut per sample at the most
        cuts = np.empty(2 * room, np.int32)
        for s in range(self.S):
            sl = slice(s * Fs, (s + 1) * Fs)
            x, y, b, mu, frq, phs, d = X[sl], Y[sl], B[sl], MU[sl], FRQ[sl], PHS[sl], D[sl]
            k = lib().twin_stepmf_wave(C.byref(self.tm.st[s]), C.byref(self.cf[s]), SR._p(self.ring[s]), SR._p(self.taps), SR._p(self.P), self.n_p, SR._p(d),
                                       int(self.tm.head[s]) // 2, SR._p(x), SR._p(y), SR._p(b), SR._p(mu), SR._p(frq), SR._p(phs), Fs, self.N, self.pl,
                                       float(self.tm.kp), float(self.tm.ki), float(self.pg), float(self.ig), 2.0, SR._p(cuts), room)
            assert 0 <= k <= room
            self.cuts += [(self.n_calls, s, int(a), int(p)) for a, p in cuts[:2 * k].reshape(-1, 2)]
        self.n_calls += 1
        return MU, FRQ, PHS, Y, B


def case_inputs(S, Fs, calls, seed):
    """the streams of a case, [S, Fs * calls, 2 N]: test_stepmf_gpu.py's construction (four carrier offsets, ragged offsets), unchanged"""
    from test_stepmf_gpu import streams
    return streams(S, Fs * calls, seed=seed)


def call_inputs(xs, S, Fs, c):
    """call c of a case: (DEL[S Fs], X[S Fs, 2 N]), frames stream-major"""
    from test_stepmf_gpu import dels
    return dels(S, Fs, c), np.ascontiguousarray(xs[:, c * Fs:(c + 1) * Fs]).reshape(S * Fs, 2 * N)


def twins(S, cls=SR.StepMf):
    """(timing twin, loop twin of class `cls`) for S streams with the cases' PLL"""
    tm = TR.Timing(PL, S)
    sm = cls(PL, S, tm)
    sm.set_pll(*PLL)
    return tm, sm


def state_bits(sm):
    """everything the loop carries between calls, as bytes: the coarse state, the timing state, the matched filter's memory"""
    return b"".join(bytes(c) for c in sm.cf) + b"".join(bytes(s) for s in sm.tm.st) + b"".join(r.tobytes() for r in sm.ring)
