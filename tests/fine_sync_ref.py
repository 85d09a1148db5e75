"""float64 references of the two pilot-aided fine synchronizers (k_sync.hip: Synchronizer_Luise_Reggiannini_DVBS2_aib, "L&R", and
Synchronizer_freq_phase_DVBS2_aib), a CPU model of the index arithmetic of the four rotation forms, and the case table that
tests/test_fine_sync_ref.py (CPU) and tests/test_fine_sync_fp64_gpu.py (the kernels) share.

Plain numpy, written from the definitions.  Frames are interleaved (re, im) float arrays of n complex samples, PL-descrambled, as on the
sockets.  A pilot block is 36 symbols (1 + j) / sqrt 2 and starts at sample 1530 + 1476 p < n; z = x (1 - j) turns it onto the real axis.

    fp_estimate64     per-pilot phase of the 36-symbol sum in [0, 2 pi), unwrapped by whole turns where the step exceeds pi, least-squares
                      line over t = start + 18 -> (freq, phase) in cycles, and how far the input is from the estimator's two decisions
    lr_pilot64        sum_p sum_{m = 1..9} R_p(m) / (2 (18 - m)) over the first 18 symbols of every pilot block, complex double
    lr_estimates64    R <- alpha R + (1 - alpha) t over the frames, est = atan2(R) / (10 pi) per frame
    rotate64          y = x e^{-j theta} with theta formed in fp32 exactly as the kernels form it from the estimate THEY reported, cos / sin and
                      the product in float64: an estimate's error and a rotation's error stay apart
    model_rotate      the four rotation forms' index arithmetic (which k, which frame's estimate, for every sample), with hooks for the
                      mistakes of tests/test_fine_sync_ref.py; used only there
"""
import functools

import numpy as np

PILOT0, PILOT_STEP, PILOT_LEN = 1530, 1476, 36
TWO_PI = 2.0 * np.pi


def c_of(v):
    """interleaved floats -> complex128"""
    p = np.asarray(v).astype(np.float64).reshape(-1, 2)
    return p[:, 0] + 1j * p[:, 1]


def pilot_starts(n, first=PILOT0):
    return np.arange(first, n, PILOT_STEP)


def _pilots(x, first, length):
    """z = x (1 - j) of the first `length` samples of every pilot block: complex128 [P, length]"""
    c = c_of(x)
    ps = pilot_starts(c.size, first)
    assert ps.size >= 1, "a frame without a pilot block: the estimators divide by zero"
    return ps, np.stack([c[s:s + length] for s in ps]) * (1 - 1j)


# ---------------------------------------------------------------------------------------------------------------- freq_phase
def fp_estimate64(x, first=PILOT0, unwrap="both"):
    """-> (freq, phase) in cycles per sample / cycles, and a dict: `step_margin` = min_p | |phi_p - phi_{p-1}| - pi |, `seam_margin` = distance
    of phi_0 from 0 and from 2 pi (radians: how far the input is from the two decisions an ulp of atan2f could turn), `turns` = the whole
    turns taken out at every pilot (+1 after an upward step, -1 after a downward one).
    unwrap: "both" (the definition), "none" (left out), "floor" (the downward direction rounded with floor as well: see test_fine_sync_ref.py)"""
    ps, z = _pilots(x, first, PILOT_LEN)
    s = z.sum(axis=1)
    phi = np.arctan2(s.imag, s.real)
    phi = np.where(phi < 0, phi + TWO_PI, phi)
    d = np.diff(phi)
    up, down = np.floor(d / TWO_PI + 0.5), np.ceil(d / TWO_PI - 0.5)
    if unwrap == "floor":
        down = np.floor(d / TWO_PI - 0.5)
    turns = np.where(np.abs(d) > np.pi, np.where(d > 0, up, down), 0.0)
    if unwrap == "none":
        turns[:] = 0.0
    y = phi / TWO_PI - np.concatenate([[0.0], np.cumsum(turns)])
    t = ps + PILOT_LEN / 2.0
    P = ps.size
    ef = (P * np.sum(t * y) - np.sum(t) * np.sum(y)) / (P * np.sum(t * t) - np.sum(t) ** 2)
    ep = (np.sum(y) - ef * np.sum(t)) / P
    info = {"step_margin": float(np.min(np.abs(np.abs(d) - np.pi))) if P > 1 else np.inf,
            "seam_margin": float(min(phi[0], TWO_PI - phi[0])), "turns": turns, "P": P}
    return float(ef), float(ep), info


# ---------------------------------------------------------------------------------------------------------------- L&R
LR_LP, LR_LAGS = PILOT_LEN // 2, PILOT_LEN // 4


def lr_pilot64(x, first=PILOT0, lp=LR_LP):
    """the frame's term of the damped autocorrelation: sum_p sum_{m = 1..9} (sum_{k = m}^{lp - 1} z_k conj z_{k - m}) / (2 (lp - m))"""
    _, z = _pilots(x, first, lp)
    t = 0j
    for m in range(1, LR_LAGS + 1):
        t += np.sum(z[:, m:] * np.conj(z[:, :lp - m])) / (2 * (lp - m))
    return complex(t)


def lr_estimates64(frames, alpha, R0=0j, **hooks):
    """frames [F, 2 n] -> (est[F] in cycles per sample, the final R)"""
    R, est = complex(R0), []
    for x in frames:
        R = alpha * R + (1 - alpha) * lr_pilot64(x, **hooks)
        est.append(np.arctan2(R.imag, R.real) / ((LR_LAGS + 1) * np.pi))
    return np.array(est), R


# ---------------------------------------------------------------------------------------------------------------- the rotation
def _theta32(frq32, phs32, k, mode, fused=True, kmul=2):
    """the phase argument as the kernels form it (sff_rotate): float32 arrays in, per sample; -> (theta32, amb in radians)"""
    frq = np.asarray(frq32, np.float32).astype(np.float64)
    kf = np.asarray(k)
    if mode == 0:
        estpi = (frq * np.pi).astype(np.float32)                              # (float)((double)est * pi)
        two_k = (kmul * kf).astype(np.float32).astype(np.float64)             # (float)(2 k): exact below 2^24
        return (estpi.astype(np.float64) * two_k).astype(np.float32), np.zeros(kf.shape)      # a product of two floats is exact in double: one rounding
    phs = np.asarray(phs32, np.float32).astype(np.float64)
    prod = frq * kf.astype(np.float32).astype(np.float64)                     # 24 x 17 bits: exact in double
    if fused:
        c32 = (prod + phs).astype(np.float32)                                 # one rounding (exact in double: both terms are multiples of 2^-50 below 2^3)
    else:
        c32 = (prod.astype(np.float32).astype(np.float64) + phs).astype(np.float32)
    amb = TWO_PI * np.spacing(np.abs(c32)).astype(np.float64)
    return (TWO_PI * c32.astype(np.float64)).astype(np.float32), amb


def _turn(x, theta32):
    """x e^{-j theta}: cos, sin and the products in float64 -> complex128"""
    th = theta32.astype(np.float64)
    return c_of(x) * (np.cos(th) - 1j * np.sin(th))


def rotate64(x, frq32, phs32, mode, fused=True):
    """one frame by the estimate the device (or the oracle) reported.  mode 0 (L&R): theta32 = float32(float32(float64(est) pi) float32(2 k)).
    mode 1 (freq_phase): c32 = float32(ef float32(k) + ep), theta32 = float32(2 pi float64(c32)); a compiler may contract ef k + ep into one
    rounding (fused, the default; the oracle is built without contraction: fused=False rounds the product first).
    -> (y complex128 [n], amb[n]): amb = 2 pi spacing(|c32|), the width of that ambiguity in radians (0 in mode 0)"""
    n = np.asarray(x).size // 2
    th, amb = _theta32(np.float32(frq32), np.float32(phs32), np.arange(n), mode, fused)
    return _turn(x, th), amb


def rel_err(y, y64, x):
    """per sample |y - y64| / |x| (complex magnitudes; y interleaved floats, y64 complex)"""
    return np.abs(c_of(y) - y64) / np.abs(c_of(x))


# ---------------------------------------------------------------------------------------------------------------- the rotation forms' indices
SFF_RCH = 1024                                           # 16-byte pairs per workgroup of sff_lr_fused_kernel


def form_indices(form, n, F, second=1, chunk_base=0, first_from_previous=False):
    """which sample index k and which frame's estimate every sample of a call of F frames of n samples is rotated with:
        "pair"   sff_rotate2_kernel: lane g of n F / 2 takes the pair 2 g: f = 2 g / n, k = 2 g - f n, and k + 1
        "chunk"  sff_lr_fused_kernel: workgroup w = f cpf + c, cpf = ceil(n / 2 / 1024), pair q = 1024 c + lane + 256 u < n / 2: 2 q, 2 q + 1
        "flat"   sff_rotate_kernel: g of n F: f = g / n, k = g - f n
    hooks: `second` = what the pair forms add for the second sample (1), `chunk_base` = pairs added to a chunk's base in the phase index (0),
    `first_from_previous` = the flat form's frame number taken one sample late.  -> (k[F, n], f[F, n]) int64; every sample is visited once"""
    k = np.full(F * n, -1, np.int64)
    fr = np.full(F * n, -1, np.int64)
    if form == "flat":
        g = np.arange(F * n)
        f = g // n
        k[g], fr[g] = g - f * n, (np.maximum(g - 1, 0) // n if first_from_previous else f)
    elif form == "pair":
        assert n % 2 == 0
        g = np.arange(F * n // 2)
        f = (2 * g) // n
        k0 = 2 * g - f * n
        k[2 * g], k[2 * g + 1], fr[2 * g], fr[2 * g + 1] = k0, k0 + second, f, f
    elif form == "chunk":
        assert n % 2 == 0
        npf = n // 2
        cpf = (npf + SFF_RCH - 1) // SFF_RCH
        seen = 0
        for w in range(F * cpf):
            f = w // cpf
            c = w - f * cpf
            for u in range(4):
                q = c * SFF_RCH + np.arange(256) + u * 256
                q = q[q < npf]
                at = f * n + 2 * q
                assert np.all(k[at] == -1)
                k[at], k[at + 1], fr[at], fr[at + 1] = 2 * (q + chunk_base), 2 * (q + chunk_base) + second, f, f
                seen += 2 * q.size
        assert seen == F * n
    else:
        raise ValueError(form)
    assert np.all(fr >= 0)
    return k.reshape(F, n), fr.reshape(F, n)


def model_rotate(X, frq32, phs32, mode, form, sign=1.0, kmul=2, **index_hooks):
    """a call of F frames through one rotation form: the form's indices, then the rotation of rotate64 (fused phase argument) per sample.
    hooks: those of form_indices, `sign` (the estimate's sign in the rotation), `kmul` (mode 0's 2 k).  -> complex128 [F, n]"""
    X = np.asarray(X, np.float32)
    F, n = X.shape[0], X.shape[1] // 2
    k, fr = form_indices(form, n, F, **index_hooks)
    frq = np.float32(sign) * np.asarray(frq32, np.float32)[fr]
    phs = np.float32(sign) * np.asarray(phs32, np.float32)[fr]
    th, _ = _theta32(frq, phs, k, mode, True, kmul)
    return _turn(X.reshape(-1), th.reshape(-1)).reshape(F, n)


# ---------------------------------------------------------------------------------------------------------------- the case table
def modcods():
    from test_front_gpu import ALL
    assert len(ALL) == 9
    return list(ALL)


EBN0, SEED = 10.0, 9
FP_FREQS = (1e-4, -1e-4, 2.5e-4, -2.5e-4, 3.1e-4, -3.1e-4)
LR_FREQS = (1e-4, -1e-4, 3e-3, -3e-3, 0.04, -0.04)
PH = 0.13
PH_OF = {}                                               # modcod -> phase of a row whose input would otherwise break the 0.05 rad margin
MARGIN = 0.05                                            # rad: a condition on the inputs, asserted from fp_estimate64 before any comparison
FRQ_BAR, PHS_BAR = 1e-6, 1e-4                            # device against oracle, the bars tests/test_sync_gpu.py has always had


@functools.lru_cache(maxsize=None)
def _frames(O, modcod):
    from helpers import make_pl_frames
    _, pl, _, _ = make_pl_frames(O, modcod, len(FP_FREQS), EBN0, seed=SEED)
    return pl


@functools.lru_cache(maxsize=None)
def table_inputs(O, modcod, sync):
    """the six rows of a MODCOD as one batch: frame i of make_pl_frames(O, modcod, 6, 10 dB, seed 9), PL-descrambled, turned by the i-th
    frequency of the synchronizer's list from PH cycles.  sync "fp" | "lr" -> float32 [6, 2 n], read-only"""
    from helpers import rot
    pl = _frames(O, modcod)
    freqs = FP_FREQS if sync == "fp" else LR_FREQS
    x = np.stack([rot(O, pl[i], f, PH_OF.get(modcod, PH)) for i, f in enumerate(freqs)])
    x.setflags(write=False)
    return x


def assert_margins(x_fp):
    """the condition on a batch of freq_phase inputs; -> the rows' info dicts"""
    infos = [fp_estimate64(x)[2] for x in x_fp]
    for i, m in enumerate(infos):
        assert m["step_margin"] >= MARGIN and m["seam_margin"] >= MARGIN, (i, m)
    return infos


class Yardstick:
    """the oracle on the whole table against float64: E[mode] = max per-sample relative rotation error against rotate64 of ITS estimates
    (its own phase argument reproduced: mode 1 without contraction), fp_frq / fp_phs / lr_frq = max estimate error against float64; `rows`
    keeps every row's figures"""


@functools.lru_cache(maxsize=None)
def oracle_yardstick(O):
    Y = Yardstick()
    Y.E, Y.fp_frq, Y.fp_phs, Y.lr_frq, Y.rows = {0: 0.0, 1: 0.0}, 0.0, 0.0, 0.0, []
    for mc in modcods():
        xf, xl = table_inputs(O, mc, "fp"), table_inputs(O, mc, "lr")
        assert_margins(xf)
        n = xf.shape[1] // 2
        for i in range(len(FP_FREQS)):
            fo, po, Yo = O.sync_freq_phase(xf[i])
            f64, p64, _ = fp_estimate64(xf[i])
            r = dict(modcod=mc, sync="fp", f=FP_FREQS[i], frq_o=fo, phs_o=po, frq_err=abs(fo - f64), phs_err=abs(po - p64),
                     rot=float(np.max(rel_err(Yo, rotate64(xf[i], fo, po, 1, fused=False)[0], xf[i]))))
            Y.rows.append(r)
            lr = O.SyncLR(n, alpha=0.0)
            fo, _, Yo = lr.synchronize(xl[i])
            r = dict(modcod=mc, sync="lr", f=LR_FREQS[i], frq_o=fo, phs_o=0.0, frq_err=abs(fo - lr_estimates64(xl[i:i + 1], 0.0)[0][0]), phs_err=0.0,
                     rot=float(np.max(rel_err(Yo, rotate64(xl[i], fo, 0.0, 0)[0], xl[i]))))
            Y.rows.append(r)
    for r in Y.rows:
        m = 1 if r["sync"] == "fp" else 0
        Y.E[m] = max(Y.E[m], r["rot"])
        if m:
            Y.fp_frq, Y.fp_phs = max(Y.fp_frq, r["frq_err"]), max(Y.fp_phs, r["phs_err"])
        else:
            Y.lr_frq = max(Y.lr_frq, r["frq_err"])
    return Y


def oracle_row(Yd, modcod, sync, f):
    return next(r for r in Yd.rows if r["modcod"] == modcod and r["sync"] == sync and r["f"] == f)


def check_rows(sync, f_rows, X, FRQ, PHS, Y, E, frq64, frq_bar, frq_o, phs64=None, phs_bar=None, phs_o=None):
    """every bar of tests/test_fine_sync_fp64_gpu.py on a batch (the kernels' sockets, or the CPU model's answer in their place):
        rot      |Y_k - rotate64(x, FRQ, PHS)_k| <= (4 E + amb_k) |x_k|                 Y: interleaved float32 or complex [F, n]
                 (freq_phase: against rotate64 with one rounding of ef k + ep or with two, per sample whichever is nearer)
        frq64    |FRQ - float64| <= frq_bar (4 x the oracle's own error)        phs64 likewise (freq_phase only)
        frq_orc  |FRQ - oracle| <= 1e-6                                         phs_orc: 1e-4
    -> one dict per row: the figures, and `broken`, the names of the bars it misses"""
    mode = 1 if sync == "fp" else 0
    out = []
    for i, f in enumerate(f_rows):
        y = Y[i] if np.iscomplexobj(Y[i]) else c_of(Y[i])
        ph = PHS[i] if mode else 0.0
        y64, amb = rotate64(X[i], FRQ[i], ph, mode)
        err = np.abs(y - y64)
        bar = rotation_bar(E, amb, X[i], f)
        r = {"f": f}
        if mode:
            # ef k + ep is one rounding or two, as the compiler was told (the library is built without contraction, like the oracle): a sample
            # is held to the bar against either of the two, whichever it took.  amb alone does not make one reference do for both: where
            # the two c32 are neighbours, theta32 = float32(2 pi c32) moves by a whole ulp of ITS binade (up to 1.27 amb), and the product's
            # own rounding is in the product's binade (twice c32's spacing where ep takes the sum below a power of two)
            err2 = np.abs(y - rotate64(X[i], FRQ[i], ph, mode, fused=False)[0])
            r["rot_fused_over_bar"], r["rot_unfused_over_bar"] = float(np.max(err / bar)), float(np.max(err2 / bar))
            r["rot_fused"], r["rot_unfused"] = float(np.max(err / np.abs(c_of(X[i])))), float(np.max(err2 / np.abs(c_of(X[i]))))
            err = np.minimum(err, err2)
        r.update({"rot": float(np.max(err / np.abs(c_of(X[i])))), "rot_over_bar": float(np.max(err / bar)), "rot_bar": float(4 * E + np.max(amb)),
                  "frq_err": abs(float(FRQ[i]) - frq64[i]), "frq_orc": abs(float(FRQ[i]) - frq_o[i]), "broken": set()})
        checks = [("rot", bool(np.all(err <= bar))), ("frq64", r["frq_err"] <= frq_bar), ("frq_orc", r["frq_orc"] <= FRQ_BAR)]
        if mode:
            r["phs_err"], r["phs_orc"] = abs(float(PHS[i]) - phs64[i]), abs(float(PHS[i]) - phs_o[i])
            checks += [("phs64", r["phs_err"] <= phs_bar), ("phs_orc", r["phs_orc"] <= PHS_BAR)]
        r["broken"] = {name for name, ok in checks if not ok}          # (a NaN figure fails its comparison)
        out.append(r)
    return out


def table_refs(O, Yd, modcod, sync):
    """what check_rows needs for a batch of the table: (X, f_rows, keyword arguments)"""
    X = table_inputs(O, modcod, sync)
    if sync == "fp":
        f_rows, e64 = FP_FREQS, [fp_estimate64(x)[:2] for x in X]
        orc = [oracle_row(Yd, modcod, sync, f) for f in f_rows]
        return X, f_rows, dict(E=Yd.E[1], frq64=[e[0] for e in e64], frq_bar=4 * Yd.fp_frq, frq_o=[r["frq_o"] for r in orc],
                               phs64=[e[1] for e in e64], phs_bar=4 * Yd.fp_phs, phs_o=[r["phs_o"] for r in orc])
    f_rows = LR_FREQS
    orc = [oracle_row(Yd, modcod, sync, f) for f in f_rows]
    return X, f_rows, dict(E=Yd.E[0], frq64=[lr_estimates64(X[i:i + 1], 0.0)[0][0] for i in range(len(f_rows))], frq_bar=4 * Yd.lr_frq,
                           frq_o=[r["frq_o"] for r in orc])


def rotation_bar(E, amb, x, f_row):
    """|Y_k - rotate64_k| <= (4 E + amb_k) |x_k|: 4 for the device's sincosf and its contracted multiply-add against libm and the oracle's
    separate roundings.  The condition that makes the bar worth having is asserted here: everywhere below a quarter of what one sample's
    slip turns a sample by at the row's frequency, 2 pi |f| |x_k|."""
    rel = 4.0 * E + amb
    assert np.all(rel < 0.25 * TWO_PI * abs(f_row)), (E, float(np.max(amb)), f_row)
    return rel * np.abs(c_of(x))
