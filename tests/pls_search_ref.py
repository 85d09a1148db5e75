"""The PLHEADER search's twin, written from the definition in include/dvbs2hip.h and sharing nothing with dvbs2_amd/csrc/k_pls_search.hip.

  scan64    the float64 exhaustive search of tests/test_pls_cpu.py (the 256 headers, |r . conj(H)|, smallest value first) slid over every offset of a buffer
  chain     the chain rule on per-offset (PLS, MET, ENE) from anywhere, in the dtype asked for: float32 restates the device's arithmetic operation by operation (each
            rounded once, the sum serial from 0), float64 is the reference
  search64  the two together

and the buffers the CPU and the GPU tests share: three frames of a short-frame MODCOD through the oracle's transmitter, cut at a random symbol, at the MODCOD's lowest
trace Es/N0."""
import json
import os

import numpy as np

from test_pls_cpu import HEADERS, ml_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = ["QPSK-S_8/9", "QPSK-S_3/5", "8PSK-S_3/5", "8PSK-S_8/9", "16APSK-S_8/9", "32APSK-S_3/4"]      # every short-frame MODCOD of the table
TRACE = {"QPSK-S_3/5": "QPSK_3_5.txt", "QPSK-S_8/9": "QPSK_8_9.txt", "8PSK-S_3/5": "8PSK_3_5.txt", "8PSK-S_8/9": "8PSK_8_9.txt", "16APSK-S_8/9": "16APSK_8_9.txt"}
EBN0_32APSK = 7.8                                                                    # no trace: the point of tests/test_est_pilots_chain_gpu.py


def complex_of(x):
    """float32[2 n] -> complex128[n], the samples as float32 says them"""
    x = np.asarray(x, np.float32).reshape(-1, 2).astype(np.float64)
    return x[:, 0] + 1j * x[:, 1]


def scan64(x, chunk=4096):
    """x: float32[2 n_sym] or complex[n_sym] -> (PLS int32[K], MET float64[K], ENE float64[K]), K = n_sym - 89"""
    r = complex_of(x) if not np.iscomplexobj(x) else np.asarray(x, np.complex128)
    W = np.lib.stride_tricks.sliding_window_view(r, 90)
    K = len(W)
    PLS, MET, ENE = np.empty(K, np.int32), np.empty(K), np.empty(K)
    for a in range(0, K, chunk):
        w = W[a:a + chunk]
        V, m, _ = ml_decode(w)
        PLS[a:a + chunk], MET[a:a + chunk], ENE[a:a + chunk] = V, m, (np.abs(w) ** 2).sum(1)
    return PLS, MET, ENE


def quality(MET, ENE, dtype=np.float32):
    """q[k] = (MET MET) / (90 ENE), 0 where ENE = 0: three operations, each rounded once in dtype"""
    MET, ENE = np.asarray(MET, dtype), np.asarray(ENE, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (MET * MET) / (dtype(90) * ENE)
    return np.where(ENE == 0, dtype(0), q).astype(dtype)


def chain(PLS, MET, ENE, LEN, dtype=np.float32):
    """-> (RES = [OFFSET, VALUE, COUNT, SLOTS], SCORE as dtype)"""
    PLS, LEN = np.asarray(PLS), np.asarray(LEN)
    K = len(PLS)
    q = quality(MET, ENE, dtype)
    L = LEN[PLS].astype(np.int64)
    L[L < 90] = 0
    best = None
    for k in np.flatnonzero((L > 0) & (np.arange(K) < L)):
        slots = np.arange(k, K, L[k])
        C, count = dtype(0), 0
        for kj in slots:
            match = PLS[kj] == PLS[k]
            C = dtype(C + (q[kj] if match else dtype(0)))
            count += int(match)
        if best is None or C > best[1]:                                              # ascending k: among equal C the smallest stays
            best = ([int(k), int(PLS[k]), count, len(slots)], C)
    return (np.array(best[0], np.int32), best[1]) if best else (np.array([-1, 0, 0, 0], np.int32), dtype(0))


def search64(x, LEN):
    return chain(*scan64(x), LEN, dtype=np.float64)


def lowest_esn0(P, modcod):
    """the Es/N0 of the lowest Eb/N0 row of the MODCOD's trace in tests/golden/refs_tx_rx_bb.json; 32APSK-S_3/4 has none: 7.8 dB Eb/N0"""
    mc = P.get_modcod(modcod)
    if modcod not in TRACE:
        return P.ebn0_to_esn0(EBN0_32APSK, mc.code_rate, mc.bps)
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "refs_tx_rx_bb.json")))[TRACE[modcod]]["rows"]
    return min(rows, key=lambda r: r["ebn0"])["esn0"]


_buffers = {}


def short_frame_buffer(O, P, modcod):
    """three PL frames of the oracle's transmitter at lowest_esn0, from a random symbol of the first on -> dict(x float32[2 n_sym], offset, value, mc, esn0, and the
    float64 twin's scan and search on the library's table: scan, res, score); made once per MODCOD and not to be written to"""
    if modcod not in _buffers:
        from helpers import chain as oracle_chain
        ch = oracle_chain(O, modcod)
        mc = ch.mc
        rng = np.random.default_rng(1000 + SHORT.index(modcod))
        esn0 = lowest_esn0(P, modcod)
        sigma = P.esn0_to_sigma(esn0)
        pl = np.concatenate([ch.tx(rng.integers(0, 2, mc.K_bch).astype(np.int32))[0] for _ in range(3)]).astype(np.float32)
        pl = pl + (sigma * rng.standard_normal(pl.size)).astype(np.float32)
        cut = int(rng.integers(1, mc.pl_frame))
        x = np.ascontiguousarray(pl[2 * cut:])
        x.setflags(write=False)
        scan = scan64(x)
        res, score = chain(*scan, P.PLS_FRAME_SYMBOLS, dtype=np.float64)
        _buffers[modcod] = dict(x=x, offset=mc.pl_frame - cut, value=P.pls_value(mc), mc=mc, esn0=esn0, scan=scan, res=res, score=score)
    return _buffers[modcod]


def header_free_buffer(rng, n_sym, kind):
    """unit-power buffers without a PLHEADER: "noise" complex Gaussian, "qpsk" / "8psk" / "16apsk" data symbols of that constellation under noise at 6 dB"""
    if kind == "noise":
        return (rng.standard_normal((n_sym, 2)) * np.sqrt(0.5)).astype(np.float32).ravel()
    if kind == "qpsk":
        pts = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    elif kind == "8psk":
        pts = np.exp(1j * np.pi / 4 * np.arange(8))
    else:
        g = 3.15                                                                     # 16APSK, ring ratio of rate 2/3
        pts = np.concatenate([np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4))), g * np.exp(1j * (np.pi / 12 + np.pi / 6 * np.arange(12)))])
        pts = pts / np.sqrt((np.abs(pts) ** 2).mean())
    s = pts[rng.integers(0, len(pts), n_sym)] + np.sqrt(0.5 * 10 ** -0.6) * (rng.standard_normal(n_sym) + 1j * rng.standard_normal(n_sym))
    return np.stack([s.real, s.imag], 1).astype(np.float32).ravel()
