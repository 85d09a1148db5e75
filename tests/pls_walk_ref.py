"""The PLHEADER walk's twin, written from the definition in include/dvbs2hip.h and sharing nothing with dvbs2_amd/csrc/k_pls_walk.hip.

  walk       the six steps on per-candidate (PLS, q) given as a function of the offset: integers and comparisons only, so it is exact whatever produced q
  group      CNT, IDX from VAL: by value ascending, in stream order within a value
  walk_scan  the walk on the outputs of a scan, entry k = offset k (what dvbs2_amd.params.find_vcm_start sees), q in fp32 operation by operation
  header64   the float64 exhaustive decoder of tests/test_pls_cpu.py on the 90 symbols at one offset -> (V, q)
  dummy      a dummy PLFRAME: the header of value 0 and 36 slots of unit-modulus symbols
"""
import numpy as np

from pls_search_ref import complex_of, quality
from test_pls_cpu import HEADERS, ml_decode

END, LOST, FULL = 0, 1, 2


def clean_len(LEN):
    L = np.asarray(LEN, np.int64).copy()
    assert L.shape == (256,)
    L[(L < 90) | (L % 18 != 0)] = 0
    return L


def walk(header, n_sym, start, LEN, q_min, max_out):
    """header(c) -> (V, q) for an offset c with c + 90 <= n_sym.  -> (OFF, VAL, Q, RES = [N, NEXT, STATUS, 0])"""
    L = clean_len(LEN)
    c, OFF, VAL, Q = int(start), [], [], []
    while True:
        if c + 90 > n_sym:
            status = END
            break
        V, q = header(c)
        if L[V] == 0 or not q >= q_min:
            status = LOST
            break
        if c + L[V] > n_sym:
            status = END
            break
        if len(OFF) == max_out:
            status = FULL
            break
        OFF.append(c); VAL.append(int(V)); Q.append(q)
        c += int(L[V])
    return np.array(OFF, np.int32), np.array(VAL, np.int32), np.array(Q), np.array([len(OFF), c, status, 0], np.int32)


def group(VAL):
    """-> (CNT int32[256], IDX int32[N])"""
    VAL = np.asarray(VAL, np.int64)
    return np.bincount(VAL, minlength=256).astype(np.int32), np.argsort(VAL, kind="stable").astype(np.int32)


def walk_scan(PLS, MET, ENE, start, LEN, q_min, max_out):
    """the walk over a scan's outputs (K = n_sym - 89 entries, entry k the header at offset k); q as the device forms it"""
    q = quality(MET, ENE, np.float32)
    return walk(lambda c: (int(PLS[c]), q[c]), len(PLS) + 89, start, LEN, np.float32(q_min), max_out)


def walk_candidates(PLS, MET, ENE, n_sym, start, LEN, q_min, max_out):
    """the walk over the decoder's outputs at the candidates start + 18 i alone"""
    q = quality(MET, ENE, np.float32)

    def header(c):
        assert (c - start) % 18 == 0
        return int(PLS[(c - start) // 18]), q[(c - start) // 18]
    return walk(header, n_sym, start, LEN, np.float32(q_min), max_out)


def header64(x):
    """x: float32[2 n_sym] -> header(c) in float64"""
    r = complex_of(x)

    def header(c):
        w = r[c:c + 90]
        V, m, _ = ml_decode(w[None, :])
        e = float((np.abs(w) ** 2).sum())
        return int(V[0]), (float(m[0]) ** 2 / (90.0 * e) if e else 0.0)
    return header


def best_start(PLS, MET, ENE, LEN, q_min):
    """acquisition as dvbs2_amd.params.find_vcm_start defines it, by running the walk from every offset: the headers a walk accepts are its frames and, when it ends
    on a frame the buffer cuts off, that frame's header"""
    L = clean_len(LEN)
    q = quality(MET, ENE, np.float32)
    n_sym = len(PLS) + 89
    best, best_n = None, 1
    header = lambda c: (int(PLS[c]), q[c])
    for k in range(min(int(L.max()), len(PLS))):
        res = walk(header, n_sym, k, LEN, np.float32(q_min), 1 << 30)[3]
        n, c = int(res[0]), int(res[1])
        if res[2] == END and c + 90 <= n_sym and L[PLS[c]] and q[c] >= np.float32(q_min):
            n += 1
        if n > best_n:
            best, best_n = k, n
    return best


def dummy(rng):
    """float32[2 * 3330]: the PLHEADER of value 0 (no pilots) and 36 slots"""
    s = np.concatenate([HEADERS[0], np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, 36 * 90)))])
    return np.stack([s.real, s.imag], 1).astype(np.float32).ravel()
