"""float64 twin of the receive chain's fused front end (k_front.hip: front_launch = PL descrambling, header / pilot removal, the M2M4 noise
estimate, the soft demapper and the de-interleaver in one launch), the bars its outputs are held to, and an fp32 model of the demapper's
arithmetic.  tests/test_front_ref.py (CPU) and tests/test_front_fp64_gpu.py (the kernels, through dvbs2hip_rx_front*) share all of it.

Plain numpy, written from the definitions; nothing here calls the oracle library.  dvbs2_amd.params gives the MODCOD rows (bits per symbol, the
interleaver's columns and order, the code rate), the constellation files and their fp32 normalisation, and the two SNR formulas.  It holds neither
the PL scrambling sequence nor an interleaver table, so both are built here: the sequence from ETSI EN 302 307 5.5.4 (n = 0), the table from
the column / row definition; tests/test_front_ref.py holds both to the oracle's bit for bit.

A PL frame is pl_frame complex symbols as interleaved (re, im) float32: 90 header symbols, then the n_sym payload symbols in slots of 90 with
36 pilots after every 16 slots.  Scrambling position i (from 0 at the first symbol behind the header) turns a symbol by R(i) quarter turns.

    xfec            the payload symbols, derotated: sign changes and swaps only, so exact in float32
    estimate64      M2M4 over the n_sym payload symbols -> (sigma, Eb/N0, Es/N0)
    llr64           L_b = logsumexp_{s: bit b of s = 0}(-|y - s|^2 / 2 sigma^2) - logsumexp_{s: bit b of s = 1}(...), bit b of s = (s >> b) & 1,
                    LLR b of symbol k at k bps + b
    deinterleave    LLR i of the interleaved order placed at itl_table[i] of the natural (code) order
    far_symbols     the symbols the kernel's general demapper hands to demap_symbol_far (docs/kernels.md): a bit's weaker subset sums to less than
                    2^-100 with every term taken relative to 2^120 at distance zero, i.e. log2 sum_s 2^(-k |y - s|^2) < -220, k = log2(e) / 2 sigma^2
    near32          the general demapper's near form with every fp32 rounding of its exponent arguments and of the frame's table reproduced
                    (exp2 / log2 rounded correctly to float32, where v_exp / v_log are good to one ulp): what the tight bar's margin is derived from, and what the far path exists to avoid
    judge           the bars of tests/test_front_fp64_gpu.py on one call's LLR and EST sockets
Hooks (keyword arguments, all off by default) put the mistakes of tests/test_front_ref.py into the index maps.
"""
import functools

import numpy as np

from dvbs2_amd import params as P

PL_M, PL_P, PL_GAP = P.PL_M, P.PL_P, 16 * P.PL_M
LOG2E = 1.4426950408889634
LLR_BAR = 1e-4                       # |L - L64| <= 1e-4 max(1, |L64|): BASELINE.json north_star
SIGMA_BAR, DB_BAR = 1e-4, 2e-3       # relative; dB (tests/test_front_gpu.py::test_front_stages_match_oracle)
# rms over a frame of the normalized LLR error against the oracle's own on the same frame and sigma.  Derived in results/front_fp64/README.md from model32:
# an exponent argument near 120 and a log2 near 120 have an fp32 ulp of 2^-17 = 7.6e-6, three such roundings enter every term and two every LLR, against
# the oracle's metrics of a few units.  With every operation rounded correctly the model needs up to 28.5x on the inputs of the tests (32APSK at the
# M2M4 estimate's sigma); v_exp_f32 and v_log_f32 are good to one ulp, twice a correct rounding's bound: 57x, and the next power of two.
TIGHT_MARGIN = 64.0


# ---------------------------------------------------------------------------------------------------------------- tables
@functools.lru_cache(maxsize=None)
def pl_seq():
    """R(i), i < 66420: x^18 = x^7 + 1 from 1, 0, ..; y^18 = y^10 + y^7 + y^5 + 1 from all ones; z(i) = x(i) + y(i); R(i) = 2 z(i + 131072) + z(i)"""
    n = (1 << 18) - 1
    x, y = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    x[0] = 1
    y[:18] = 1
    for i in range(n - 18):
        x[i + 18] = x[i + 7] ^ x[i]
        y[i + 18] = y[i + 10] ^ y[i + 7] ^ y[i + 5] ^ y[i]
    z = x ^ y
    i = np.arange(66420)
    seq = (2 * z[(i + 131072) % n] + z[i]).astype(np.uint8)
    seq.setflags(write=False)
    return seq


@functools.lru_cache(maxsize=None)
def constellation(mc):
    """float32 [2^bps, 2], unit mean energy, index = label"""
    c = P.normalise_constellation(P.load_constellation(mc.cstl_file))
    assert c.shape == (1 << mc.bps, 2)
    c.setflags(write=False)
    return c


def itl_table(mc, mirror=False):
    """natural position of interleaved LLR i: written column by column, read row by row; row i, column j of the read-out sits in column j (order
    0, TOP_LEFT) or cols - 1 - j (order 1) of the written block.  mirror: the other order"""
    N, cols = mc.N_ldpc, mc.itl_cols
    if cols <= 1:
        return np.arange(N)
    rows = N // cols
    i, j = np.divmod(np.arange(N), cols)
    top_left = (mc.itl_order == 0) != bool(mirror)
    return (j if top_left else cols - 1 - j) * rows + i


def payload_index(mc, pilot_slip=0):
    """index inside the PL frame of payload symbol k.  pilot_slip: added from the second pilot block on (clipped to the frame)"""
    k = np.arange(mc.N_xfec)
    b = np.minimum(k // PL_GAP, mc.N_pilots)
    return np.minimum(PL_M + k + PL_P * b + np.where(b >= 2, pilot_slip, 0), mc.pl_frame - 1)


# ---------------------------------------------------------------------------------------------------------------- the stages
def xfec(pl, mc, pilot_slip=0, seq_shift=0, swap_quadrants=False):
    """one PL frame float32[2 pl_frame] -> derotated payload symbols float32 [n_sym, 2].
    R = 0: (x, y)   1: (y, -x)   2: (-x, -y)   3: (-y, x).  hooks: pilot_slip (payload_index), seq_shift (the sequence read that many
    positions late), swap_quadrants (R = 1 and R = 3 exchanged)"""
    c = np.asarray(pl, np.float32).reshape(-1, 2)
    assert c.shape[0] == mc.pl_frame
    pi = payload_index(mc, pilot_slip)
    y = c[pi]
    R = pl_seq()[payload_index(mc) - PL_M + seq_shift].astype(np.int64)
    if swap_quadrants:
        R = np.where(R == 1, 3, np.where(R == 3, 1, R))
    re = np.choose(R, [y[:, 0], y[:, 1], -y[:, 0], -y[:, 1]])
    im = np.choose(R, [y[:, 1], -y[:, 0], -y[:, 1], y[:, 0]])
    return np.stack([re, im], axis=1).astype(np.float32)


def estimate64(x, mc, divisor=None):
    """M2M4 over the payload symbols x [n_sym, 2] -> (sigma, Eb/N0 dB, Es/N0 dB).  divisor: what the moment sums are divided by (n_sym)"""
    e = (np.asarray(x).astype(np.float64) ** 2).sum(axis=1)
    n = float(divisor if divisor else e.size)
    m2, m4 = e.sum() / n, (e * e).sum() / n
    se = np.sqrt(abs(2.0 * m2 * m2 - m4))
    ne = abs(m2 - se)
    esn0 = 10.0 * np.log10(se / ne)
    sigma = P.esn0_to_sigma(esn0)
    ebn0 = esn0 - (P.ebn0_to_esn0(0.0, mc.code_rate, mc.bps))
    return float(sigma), float(ebn0), float(esn0)


def _metrics(x, sigma, mc):
    """-|y - s|^2 / 2 sigma^2, float64 [n_sym, 2^bps]"""
    y = np.asarray(x).astype(np.float64)
    s = constellation(mc).astype(np.float64)
    d2 = (y[:, None, 0] - s[None, :, 0]) ** 2 + (y[:, None, 1] - s[None, :, 1]) ** 2
    return -d2 / (2.0 * float(sigma) ** 2)


def _lse(v):
    m = v.max(axis=1)
    return m + np.log(np.exp(v - m[:, None]).sum(axis=1))


def _subsets(mc):
    s = np.arange(1 << mc.bps)
    return [(np.flatnonzero((s >> b) & 1 == 0), np.flatnonzero((s >> b) & 1 == 1)) for b in range(mc.bps)]


def llr64(x, sigma, mc):
    """exact LLRs of the payload symbols for this sigma, float64 [n_sym, bps]"""
    met = _metrics(x, sigma, mc)
    return np.stack([_lse(met[:, s0]) - _lse(met[:, s1]) for s0, s1 in _subsets(mc)], axis=1)


def far_symbols(x, sigma, mc):
    """bool [n_sym]: the symbols on the general demapper's far path"""
    met = _metrics(x, sigma, mc)
    lo = np.min([np.minimum(_lse(met[:, s0]), _lse(met[:, s1])) for s0, s1 in _subsets(mc)], axis=0)
    return lo * LOG2E < -220.0


def deinterleave(L, mc, mirror=False, reverse_bits=False, swap_pairs=False, drop_last=False):
    """LLRs [n_sym, bps] -> natural order [N_ldpc].  hooks: mirror (itl_table), reverse_bits (LLR b of a symbol written where bps - 1 - b
    belongs), swap_pairs (symbols 2 j and 2 j + 1 exchanged), drop_last (the frame's last symbol left as NaN)"""
    L = np.array(L, dtype=np.float64)
    if reverse_bits:
        L = L[:, ::-1]
    if swap_pairs:
        L = L.reshape(-1, 2, mc.bps)[:, ::-1].reshape(-1, mc.bps)
    if drop_last:
        L[-1] = np.nan
    nat = np.empty(mc.N_ldpc)
    nat[itl_table(mc, mirror)] = L.reshape(-1)
    return nat


def front64(pl, mc, sigma):
    """one PL frame, this sigma -> natural-order LLRs float64 [N_ldpc]"""
    return deinterleave(llr64(xfec(pl, mc), sigma, mc), mc)


# ---------------------------------------------------------------------------------------------------------------- the demapper's fp32 arithmetic
def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def near32(x, sigma, mc):
    """the general demapper's near form (demap_symbols_s: 2^(u_s - ref) = exp2(yr A_s + (yi B_s + (120 - k |y|^2)) + D_s), subset sums, two log2
    per bit) with the fp32 roundings of the table (A, B, D, k)_s and of every exponent argument; products and sums of two floats are exact in
    double, so one cast is one fused rounding.  exp2 below 2^-126 gives zero, as the hardware's does.  -> LLRs float64 [n_sym, bps]; +-inf where a
    subset vanished, which is what the far path is there for"""
    y = np.asarray(x, np.float32).astype(np.float64)
    s = constellation(mc).astype(np.float64)
    s32 = float(np.float32(sigma))
    inv = _f32(1.0 / _f32(2.0 * _f32(s32 * s32)))
    k = _f32(inv * float(np.float32(LOG2E)))
    A, B = _f32(2.0 * k * s[:, 0]), _f32(2.0 * k * s[:, 1])
    D = _f32(-k * _f32(_f32(s[:, 0] * s[:, 0]) + _f32(s[:, 1] * s[:, 1])))
    q = _f32(y[:, 0] * y[:, 0] + _f32(y[:, 1] * y[:, 1]))
    c0 = _f32(-k * q + 120.0)
    e = _f32(_f32(y[:, :1] * A[None, :] + _f32(y[:, 1:] * B[None, :] + c0[:, None])) + D[None, :])
    t = np.where(e < -126.0, 0.0, _f32(np.exp2(e)))
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for s0, s1 in _subsets(mc):
            l0, l1 = _f32(np.log2(_f32(t[:, s0].sum(axis=1)))), _f32(np.log2(_f32(t[:, s1].sum(axis=1))))      # a log2 near 120: an ulp of 2^-17 again
            out.append(_f32(float(np.float32(np.log(2.0))) * _f32(l0 - l1)))
    return np.stack(out, axis=1)


def far32(x, sigma, mc):
    """the far form (demap_symbol_far: u_s = yr A_s + (yi B_s + D_s), every subset relative to its own maximum, L = ln 2 ((m0 - m1) + (log2 s0 -
    log2 s1))) with the same roundings reproduced -> LLRs float64 [n_sym, bps]"""
    y = np.asarray(x, np.float32).astype(np.float64)
    s = constellation(mc).astype(np.float64)
    s32 = float(np.float32(sigma))
    k = _f32(_f32(1.0 / _f32(2.0 * _f32(s32 * s32))) * float(np.float32(LOG2E)))
    A, B = _f32(2.0 * k * s[:, 0]), _f32(2.0 * k * s[:, 1])
    D = _f32(-k * _f32(_f32(s[:, 0] * s[:, 0]) + _f32(s[:, 1] * s[:, 1])))
    u = _f32(y[:, :1] * A[None, :] + _f32(y[:, 1:] * B[None, :] + D[None, :]))
    out = []
    for s0, s1 in _subsets(mc):
        m0, m1 = u[:, s0].max(axis=1), u[:, s1].max(axis=1)
        t0, t1 = _f32(np.exp2(_f32(u[:, s0] - m0[:, None]))).sum(axis=1), _f32(np.exp2(_f32(u[:, s1] - m1[:, None]))).sum(axis=1)
        out.append(_f32(float(np.float32(np.log(2.0))) * _f32(_f32(m0 - m1) + _f32(_f32(np.log2(_f32(t0))) - _f32(np.log2(_f32(t1)))))))
    return np.stack(out, axis=1)


def model32(x, sigma, mc):
    """what the general demapper's arithmetic gives: near32, far32 on the symbols of far_symbols"""
    L, far = near32(x, sigma, mc), far_symbols(x, sigma, mc)
    if far.any():
        L[far] = far32(np.asarray(x)[far], sigma, mc)
    return L


# ---------------------------------------------------------------------------------------------------------------- the bars
def norm_err(L, L64):
    """|L - L64| / max(1, |L64|); NaN where L is NaN"""
    L64 = np.asarray(L64, np.float64)
    return np.abs(np.asarray(L).astype(np.float64) - L64) / np.maximum(1.0, np.abs(L64))


def rms(e):
    return float(np.sqrt(np.mean(np.square(e))))


def judge(mc, pl, LLR, EST, sigma_in, oracle_rms, frames=None, margin=TIGHT_MARGIN):
    """the bars on one call: pl [F, 2 pl_frame], LLR [F, N_ldpc] and EST [F, 3] as the sockets hold them, sigma_in float32 [F] or None.
    oracle_rms(x, sigma32, L64) -> the oracle demapper's rms normalized error on payload symbols x at that sigma against L64 [n_sym, bps].
    Every frame of `frames` (all) is compared with the twin at the sigma EST reports for it:
        nan       nothing of the sockets' NaN fill is left (all frames)
        echo      sigma given: EST == (sigma_in[f], 0, 0) bit for bit (all frames)
        contract  |L - L64| <= 1e-4 max(1, |L64|) for every LLR
        tight     rms over the frame of the normalized error <= margin x the oracle's own on the same frame and sigma
        sigma     sigma estimated: within 1e-4 relative of estimate64             ebn0 / esn0: within 2e-3 dB
    -> one dict per frame judged: the figures, and `broken`, the names of the bars it misses"""
    pl, LLR, EST = np.asarray(pl), np.asarray(LLR), np.asarray(EST)
    F = LLR.shape[0]
    whole = set()
    if np.isnan(LLR).any() or np.isnan(EST).any():
        whole.add("nan")
    if sigma_in is not None:
        want = np.zeros((F, 3), np.float32)
        want[:, 0] = np.asarray(sigma_in, np.float32)
        if not np.array_equal(EST.view(np.uint32), want.view(np.uint32)):
            whole.add("echo")
    rows = []
    for f in (range(F) if frames is None else frames):
        x = xfec(pl[f], mc)
        sig = np.float32(EST[f, 0])
        r = {"frame": f, "sigma": float(sig), "broken": set(whole)}
        if not np.isfinite(sig) or sig <= 0:
            r["broken"].add("contract")
            rows.append(r)
            continue
        L64 = llr64(x, sig, mc)
        e = norm_err(LLR[f], deinterleave(L64, mc))
        r["max_e"], r["rms_e"], r["rms_oracle"] = float(np.nanmax(e)) if not np.isnan(e).all() else np.nan, rms(e), float(oracle_rms(x, sig, L64))
        checks = [("contract", bool(np.all(e <= LLR_BAR))), ("tight", r["rms_e"] <= margin * r["rms_oracle"])]
        if sigma_in is None:
            s64, eb64, es64 = estimate64(x, mc)
            r["sig_err"], r["eb_err"], r["es_err"] = abs(float(sig) - s64) / s64, abs(float(EST[f, 1]) - eb64), abs(float(EST[f, 2]) - es64)
            checks += [("sigma", r["sig_err"] <= SIGMA_BAR), ("ebn0", r["eb_err"] <= DB_BAR), ("esn0", r["es_err"] <= DB_BAR)]
        r["broken"] |= {name for name, ok in checks if not ok}          # (a NaN figure fails its comparison)
        rows.append(r)
    return rows


def broken(rows):
    out = set()
    for r in rows:
        out |= r["broken"]
    return out


# ---------------------------------------------------------------------------------------------------------------- the inputs both test files use
SEED, SIGMA_SCALE = 31, (0.9, 1.0, 1.25)
HIGH_SNR = dict(ebn0=30.0, seed=1, sigmas=(0.05, 0.1, 0.2), modcods=("8PSK-S_8/9", "8PSK-N_8/9", "16APSK-S_8/9", "32APSK-S_3/4"))      # case E


def modcods():
    from test_front_gpu import ALL
    assert len(ALL) == 9
    return list(ALL)


@functools.lru_cache(maxsize=None)
def frames(O, modcod, F=3, ebn0=None, seed=SEED):
    """make_pl_frames at test_front_gpu's EBN0 table (or ebn0) -> (info, pl, cw, sigma), read-only and shared"""
    from helpers import make_pl_frames
    from test_front_gpu import EBN0
    info, pl, cw, sigma = make_pl_frames(O, modcod, F, EBN0[modcod] if ebn0 is None else ebn0, seed=seed)
    for a in (info, pl, cw):
        a.setflags(write=False)
    return info, pl, cw, sigma


def sigmas(sigma, F):
    """a sigma per frame: the true one times 0.9, 1.0, 1.25, cycling"""
    return (float(sigma) * np.array([SIGMA_SCALE[f % 3] for f in range(F)])).astype(np.float32)


def oracle_rms_of(O, modcod):
    """judge's yardstick: the oracle's pairwise max* demapper on the same symbols and sigma"""
    from helpers import chain
    ch = chain(O, modcod)

    def fn(x, sigma32, L64):
        return rms(norm_err(O.demodulate(ch.cstl, ch.mc.bps, np.float32(sigma32), np.asarray(x, np.float32).ravel()).reshape(L64.shape), L64))
    return fn


def twin_call(mc, pl, sigma_in):
    """the sockets of a faultless device: the twin's own answer cast to float32 -> (LLR [F, N_ldpc], EST [F, 3])"""
    F = pl.shape[0]
    LLR, EST = np.empty((F, mc.N_ldpc), np.float32), np.zeros((F, 3), np.float32)
    for f in range(F):
        if sigma_in is None:
            EST[f] = estimate64(xfec(pl[f], mc), mc)
        else:
            EST[f, 0] = sigma_in[f]
        LLR[f] = front64(pl[f], mc, EST[f, 0])
    return LLR, EST
