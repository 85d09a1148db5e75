"""The pilot-aided noise estimator's float64 reference (NumPy only): include/dvbs2hip.h states the definition, dvbs2_amd/csrc/k_est_pilots.hip computes it in fp32.

Known position k of L = 90 + 36 N_pilots: the header at [0, 90), pilot block b = 1..N_pilots at [90 + 1440 b + 36 (b - 1), +36).  Known values: the PLHEADER of the
MODCOD's pls row with pairing bit 1, and (1 + j) / sqrt(2) on every pilot.  Everything is restated here from the standard (the PLS code, the PL scrambling sequence of
ETSI EN 302 307 5.5.4 with n = 0) and shares no code with the library; tests/test_est_pilots_cpu.py checks it against the oracle's framer and PL scrambler."""
import functools

import numpy as np

G = np.array([
    [1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1],
    [0, 1] * 16,
    [0, 0, 1, 1] * 8,
    [0, 0, 0, 0, 1, 1, 1, 1] * 4,
    ([0] * 8 + [1] * 8) * 2,
    [0] * 16 + [1] * 16,
    [1] * 32])
SCR = np.array([0, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 1,
                0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 0])
SOF = np.array([0, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0])


def n_pilots(n_xfec):
    return n_xfec // 1440


def positions(n_xfec):
    """-> int[L], where in the PL frame the known symbols are"""
    blocks = [90 + 1440 * b + 36 * (b - 1) + np.arange(36) for b in range(1, n_pilots(n_xfec) + 1)]
    return np.concatenate([np.arange(90)] + blocks)


def values(pls_bits, n_xfec):
    """-> complex128[L], what the framer puts there (before the PL scrambler)"""
    c = (np.asarray(pls_bits) @ G) % 2
    y = np.empty(64, int)
    y[0::2], y[1::2] = c, c ^ 1
    s = 1 - 2 * np.concatenate([SOF, y ^ SCR])
    base = np.where(np.arange(90) % 2 == 0, 1 + 1j, -1 + 1j) / np.sqrt(2)
    base[26:] *= 1j if pls_bits[0] else 1
    return np.concatenate([base * s, np.full(36 * n_pilots(n_xfec), (1 + 1j) / np.sqrt(2))])


@functools.lru_cache(None)
def pl_sequence():
    """R(i) of the PL scrambler, i = frame position - 90: the symbol is multiplied by exp(j pi/2 R)"""
    P = (1 << 18) - 1
    x, y = np.zeros(P, np.uint8), np.zeros(P, np.uint8)
    x[0] = 1
    y[:18] = 1
    for i in range(P - 18):
        x[i + 18] = x[i + 7] ^ x[i]
        y[i + 18] = y[i + 10] ^ y[i + 7] ^ y[i + 5] ^ y[i]
    z = x ^ y
    i = np.arange(66420)
    return 2 * z[(i + 131072) % P].astype(int) + z[i]


def known(frames, n_xfec, scrambled):
    """float32[F, 2 pl_frame] -> complex128[F, L], the received known symbols, the pilots PL-descrambled when the frames are scrambled (exact: a swap or a sign change)"""
    x = np.asarray(frames, np.float32).reshape(-1, 2 * (90 + n_xfec + 36 * n_pilots(n_xfec)))
    pos = positions(n_xfec)
    y = x[:, 2 * pos].astype(np.float64) + 1j * x[:, 2 * pos + 1].astype(np.float64)
    if scrambled:
        turn = np.array([1, -1j, -1, 1j])[pl_sequence()[pos[90:] - 90]]              # conj(exp(j pi/2 R))
        y[:, 90:] = y[:, 90:] * turn
    return y


def powers(frames, mc, scrambled):
    """-> (A, N) per frame: |c|^2 and the noise power per complex symbol, in the residual form"""
    y = known(frames, mc.N_xfec, scrambled)
    p = values(mc.pls, mc.N_xfec)
    L = len(p)
    c = (y * p.conj()).sum(1) / L
    N = (np.abs(y - c[:, None] * p) ** 2).sum(1) / (L - 1)
    return np.abs(c) ** 2, N


def finish(A, N, mc):
    """(A, N) -> (SIG, Eb_N0, Es_N0)"""
    A, N = np.asarray(A, np.float64), np.asarray(N, np.float64)
    L = 90 + 36 * n_pilots(mc.N_xfec)
    S = A - N / L
    with np.errstate(divide="ignore", invalid="ignore"):
        es = 10 * np.log10(S / N)
    es = np.where(S <= 0, -100.0, np.where((N == 0) | ~(es < 100.0), 100.0, es))
    return np.sqrt(1.0 / (2.0 * 10.0 ** (es / 10.0))), es - 10.0 * np.log10(mc.code_rate * mc.bps), es


def average(A, N, alpha, streams=1, state=None):
    """the recurrence per stream (stream s = frames [s F/S, (s+1) F/S)), in float64; state: None (after a reset) or what an earlier call returned -> (Abar, Nbar, state)"""
    A, N = np.asarray(A, np.float64).reshape(streams, -1), np.asarray(N, np.float64).reshape(streams, -1)
    Ab, Nb = np.empty_like(A), np.empty_like(N)
    state = [None] * streams if state is None else list(state)
    for s in range(streams):
        for f in range(A.shape[1]):
            state[s] = (A[s, f], N[s, f]) if state[s] is None else (alpha * state[s][0] + (1 - alpha) * A[s, f], alpha * state[s][1] + (1 - alpha) * N[s, f])
            Ab[s, f], Nb[s, f] = state[s]
    return Ab.ravel(), Nb.ravel(), state


def estimate(frames, mc, scrambled=True, alpha=0.0, streams=1, state=None):
    """-> (SIG, Eb_N0, Es_N0) float64 per frame [, state when alpha > 0]"""
    A, N = powers(frames, mc, scrambled)
    if alpha == 0.0:
        return finish(A, N, mc)
    Ab, Nb, state = average(A, N, alpha, streams, state)
    return finish(Ab, Nb, mc) + (state,)
