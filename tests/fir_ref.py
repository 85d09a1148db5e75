"""float64 references of the streaming filters and correlators, and a CPU model of the matrix-core kernels' operand split.

Plain numpy: nothing here needs a GPU or the oracle.  Streams are interleaved (re, im) float arrays as on the sockets; the taps are real,
so the two planes never mix.  The history conventions are the handle's (Dvbs2Hip.filter / shape_filter): the samples that came before the
call, oldest first -- T - 1 of them for the matched filter, (T - 1) // osf INPUT samples for the shaping filter (the oracle's upfir keeps
T - 1 samples of the zero-stuffed stream instead).

    fir64 / upfir64 / corr64     the operation itself, products and sums in float64
    split3, model_mfma           what k_fir_mfma.hip / k_sync_mfma.hip compute when every fp32 addition is taken as exact: each operand
                                 cut into three bf16 parts (round to nearest even, remainders formed in float32), a chosen set of
                                 (tap part, sample part) products, each exact, summed in float64.  With a product left out it shows how
                                 large the error of a kernel that loses that product would be -- the size a test's bar has to see.
"""
import numpy as np

# (tap part, sample part) in the kernels' order of accumulation, smallest first: b3 x1, b2 x2, b1 x3, b2 x1, b1 x2, b1 x1
ALL_SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


def _planes(v):
    """interleaved float array -> float64 [n, 2]"""
    v = np.asarray(v)
    assert v.ndim == 1 and v.size % 2 == 0
    return v.astype(np.float64).reshape(-1, 2)


def _ext(hist, x, H):
    h, x = _planes(hist), _planes(x)
    assert h.shape[0] == H, (h.shape, H)
    return np.concatenate([h, x]), x.shape[0]


def _band(taps, ext, H, n, with_abs):
    """y[i] = sum_k taps[k] ext[H + i - k] over both planes, k ascending; ext = history ++ stream"""
    y = np.zeros((n, 2))
    ya = np.zeros((n, 2)) if with_abs else None
    ae = np.abs(ext) if with_abs else None
    taps = [(k, float(b)) for k, b in enumerate(np.asarray(taps, dtype=np.float64)) if b != 0.0]
    CH = 1 << 15                                         # a block of outputs at a time: the loop over the taps stays in the cache
    tmp = np.empty((min(CH, n), 2))
    for i0 in range(0, n, CH):
        m = min(CH, n - i0)
        yo, t = y[i0:i0 + m], tmp[:m]
        for k, b in taps:
            np.multiply(ext[H - k + i0:H - k + i0 + m], b, out=t)
            yo += t
            if with_abs:
                np.multiply(ae[H - k + i0:H - k + i0 + m], abs(b), out=t)
                ya[i0:i0 + m] += t
    return y, ya


def fir64(taps, hist, x, with_abs=True):
    """y[n] = sum_k taps[k] x[n - k], x[<0] from hist (the T - 1 samples before the call).  -> (y64, yabs), interleaved float64;
    yabs[n] = sum_k |taps[k]| |x[n - k]| per plane (None if with_abs is False)"""
    T = len(taps)
    ext, n = _ext(hist, x, T - 1)
    y, ya = _band(taps, ext, T - 1, n, with_abs)
    return y.reshape(-1), (ya.reshape(-1) if with_abs else None)


def upfir64(taps, osf, hist_in, x, with_abs=True):
    """y[i osf + f] = sum_m taps[f + m osf] x[i - m], x[<0] from hist_in (the (T - 1) // osf input samples before the call)"""
    taps = np.asarray(taps, dtype=np.float64)
    T = taps.size
    Hin = (T - 1) // osf
    ext, n = _ext(hist_in, x, Hin)
    y = np.zeros((n, osf, 2))
    ya = np.zeros((n, osf, 2)) if with_abs else None
    for f in range(osf):
        br = taps[f::osf]
        assert br.size <= Hin + 1
        y[:, f], a = _band(br, ext, Hin, n, with_abs)
        if with_abs:
            ya[:, f] = a
    return y.reshape(-1), (ya.reshape(-1) if with_abs else None)


def corr64(x, taps, z_prev):
    """The frame synchronizer's correlation in complex128: d[i] = x[i - 1] conj(x[i]), cor[o] = sum_m taps[m] d[o - m].  x: interleaved
    samples of this call; z_prev: the 64 complex samples before it (a fresh synchronizer: 63 zeros, then reg_channel = 1)."""
    z_prev = np.asarray(z_prev, dtype=np.complex128)
    taps = np.asarray(taps, dtype=np.float64)
    assert z_prev.size == 64 and taps.size <= 64
    p = _planes(x)
    z = np.concatenate([z_prev, p[:, 0] + 1j * p[:, 1]])
    d = np.zeros(z.size, np.complex128)
    d[1:] = z[:-1] * np.conj(z[1:])                      # d[0] would need a 65th sample: no tap reaches it
    cor = np.zeros(p.shape[0], np.complex128)
    for m, b in enumerate(taps):
        cor += b * d[64 - m:z.size - m]
    return cor


def bf16_rne(v):
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def split3(v):
    """v = p1 + p2 + p3 with three bf16 parts, as fm_split / fir_mfma_afrag form them: every remainder a float32 subtraction"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    p1 = bf16_rne(v)
    r = v - p1
    p2 = bf16_rne(r)
    r = r - p2
    p3 = bf16_rne(r)
    return p1, p2, p3


def model_mfma(taps, x, products=ALL_SIX, hist=None, osf=1):
    """The split scheme with exact products and float64 sums: sum over (a, b) in products of FIR(tap part a, sample part b).  x, hist
    interleaved as for fir64 (osf = 1) or upfir64; hist None = zeros.  -> y interleaved float64"""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    H = (taps.size - 1) // osf
    if hist is None:
        hist = np.zeros(2 * H, np.float32)
    tp = [p.astype(np.float64) for p in split3(taps)]
    sx, sh = split3(x), split3(hist)
    y = None
    for a in range(3):
        sel = [b for (aa, b) in products if aa == a]
        if not sel:
            continue
        xs = sum(sx[b].astype(np.float64) for b in sel)          # sums of a sample's parts are exact in float64
        hs = sum(sh[b].astype(np.float64) for b in sel)
        ya = (fir64(tp[a], hs, xs, with_abs=False) if osf == 1 else upfir64(tp[a], osf, hs, xs, with_abs=False))[0]
        y = ya if y is None else y + ya
    return y if y is not None else np.zeros(np.asarray(x).size * osf)


def diff32(x, z_last):
    """the correlators' input as the kernels form it: d[i] = x[i - 1] conj(x[i]) in float32 (products and sums rounded one by one),
    interleaved; z_last = the complex sample before the call"""
    p = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    q = np.concatenate([np.array([[np.real(z_last), np.imag(z_last)]], np.float32), p[:-1]])
    d = np.empty_like(p)
    d[:, 0] = q[:, 0] * p[:, 0] + q[:, 1] * p[:, 1]
    d[:, 1] = q[:, 1] * p[:, 0] - q[:, 0] * p[:, 1]
    return d.reshape(-1)


class Err:
    def __init__(self, mx, rms):
        self.max, self.rms = float(mx), float(rms)

    def __repr__(self):
        return "max %.3e rms %.3e" % (self.max, self.rms)


def err_stats(y, y64):
    """max and rms of |y - y64| (complex arrays are taken as they are, real ones element by element)"""
    e = np.abs(np.asarray(y).astype(np.complex128 if np.iscomplexobj(y) or np.iscomplexobj(y64) else np.float64) - y64)
    return Err(e.max() if e.size else 0.0, np.sqrt(np.mean(e * e)) if e.size else 0.0)


def c_of(v):
    """interleaved floats -> complex128"""
    p = _planes(v)
    return p[:, 0] + 1j * p[:, 1]


def tail(stream, H):
    """the history a handle carries after `stream` (interleaved, from a reset handle): its last H samples, zeros before its start"""
    s = np.asarray(stream, dtype=np.float32).ravel()
    return np.concatenate([np.zeros(2 * H, np.float32), s])[s.size:].copy() if H else np.zeros(0, np.float32)


# ---------------------------------------------------------------- inputs shared by tests/test_fir_ref.py (the model) and tests/test_fir_fp64_gpu.py (the kernels)
N3 = 3 * 2048 + 5                                        # three tiles of the matrix-core kernel and a ragged tail
IMPULSE_AT = tuple(range(3, N3, 97))                     # 97 = 6 * 16 + 1: at least 96 apart, sixteen in a row take every block phase
IMPULSE_CUT = 3040                                       # a first call that ends 30 samples after the impulse at 3010 (a multiple of 16)


def impulse_stream():
    x = np.zeros((N3, 2), np.float32)
    x[list(IMPULSE_AT)] = 1.0
    return x.reshape(-1)


def impulse_response(taps, osf=1):
    """what a filter with `taps` answers to impulse_stream(): the taps, bit for bit, behind every impulse"""
    taps = np.asarray(taps, dtype=np.float32)
    y = np.zeros((N3 * osf, 2), np.float32)
    for p in IMPULSE_AT:
        seg = taps[:N3 * osf - p * osf]
        y[p * osf:p * osf + seg.size] = seg[:, None]
    return y.reshape(-1)


def random_taps(T):
    return np.random.default_rng(1000 + T).standard_normal(T).astype(np.float32)


def delta_taps(T, j, s):
    b = np.zeros(T, np.float32)
    b[j] = s
    return b


def delayed(x, j, s, osf=1):
    """the answer of delta_taps(T, j, s) to the interleaved stream x from a reset handle: s x[n - j]; at osf 2, branch j % 2 of input n - j // 2"""
    p = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    n = p.shape[0]
    y = np.zeros((n, osf, 2), np.float32)
    m = j // osf
    y[m:, j % osf] = np.float32(s) * p[:n - m]
    return y.reshape(-1)


def srrc(n_taps):
    """the two SRRC sets the suite filters with: 81 taps (roll-off 0.2, osf 2, 20 symbols) and 41 taps (0.35, osf 4, 5 symbols)"""
    from dvbs2_amd import params as P
    taps = {81: P.rrc_taps(0.2, 2, 20), 41: P.rrc_taps(0.35, 4, 5)}[n_taps]
    assert taps.size == n_taps
    return np.ascontiguousarray(taps, dtype=np.float32)


# unit-power Gaussian input against float64: name -> (taps, handle's osf, seed, calls of (samples per frame, frames))
RANDOM_FIR = {
    "srrc81": (lambda: srrc(81), 2, 5, ((6804, 3),) * 3),
    "srrc41": (lambda: srrc(41), 4, 6, ((7, 1), (1, 1), (33, 1), (2049, 1), (5, 1))),
    "rand2": (lambda: random_taps(2), 2, 102, ((2 * 2048 + 257, 1),)),
    "rand17": (lambda: random_taps(17), 2, 117, ((2 * 2048 + 257, 1),)),
    "rand49": (lambda: random_taps(49), 2, 149, ((2 * 2048 + 257, 1),)),
    "rand80": (lambda: random_taps(80), 2, 180, ((2 * 2048 + 257, 1),)),
}
RANDOM_UPFIR = {
    "srrc81": (lambda: srrc(81), 2, 15, ((3402, 2), (7, 1), (5000, 4))),
    "rand98": (lambda: random_taps(98), 2, 198, ((4101, 1),)),
}
LONG_N = 3073 * 2048 - 300                               # four tiles per workgroup of the matrix-core kernel, the last workgroup one ragged tile


def gauss_calls(seed, calls):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(F * 2 * n).astype(np.float32) for n, F in calls]


# ---------------------------------------------------------------- the correlators' inputs (tests/test_sync_gpu.py and the model in tests/test_fir_ref.py)
Z0 = np.concatenate([np.zeros(63), [1.0]]).astype(np.complex128)      # a fresh synchronizer's memory: nothing, then reg_channel = (1, 0)
SYNC_SHAPES = (("32APSK-S_3/4", 5), ("QPSK-S_8/9", 1))


def sync_stream(O, modcod, F):
    """-> (two calls of F noisy PL frames each, behind 4321 samples of noise: float32 [2, F, 2 n]; n)"""
    from helpers import make_pl_frames
    rng = np.random.default_rng(5)
    _, pl, _, _ = make_pl_frames(O, modcod, F, 5.0, seed=9)
    n = pl.shape[1] // 2
    s = np.concatenate([0.7 * rng.standard_normal(2 * 4321).astype(np.float32), pl.reshape(-1), pl.reshape(-1)])[:2 * F * 2 * n]
    return s.reshape(2, F, 2 * n), n


def unit_stream(n_total, seed=6):
    """samples from {1, j, -1, -j}: every differential sample is one of them too, exactly, and the correlations are whole numbers below 64"""
    k = np.random.default_rng(seed).integers(0, 4, n_total)
    x = np.zeros((n_total, 2), np.float32)
    x[:, 0] = np.array([1, 0, -1, 0], np.float32)[k]
    x[:, 1] = np.array([0, 1, 0, -1], np.float32)[k]
    return x.reshape(-1)


def oracle_corr(O, n, frames):
    """the oracle's two correlations of consecutive frames [F, 2 n] from a fresh synchronizer, its two tasks run frame by frame (synchronize2 is
    what moves reg_channel on) -> (cor_SOF, cor_PLSC) complex, [F n] each"""
    sf = O.SyncFrame(n)
    cs, cp = [], []
    for x in frames:
        c1, c2 = sf.synchronize1(x)
        sf.synchronize2(x, c1, c2)
        cs.append(c_of(c1)); cp.append(c_of(c2))
    return np.concatenate(cs), np.concatenate(cp)
