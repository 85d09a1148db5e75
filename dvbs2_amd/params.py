"""MODCOD parameter table for the DVB-S2 RX inner path.

Restates ``factory::DVBS2::modcod_init`` (/root/reference src/common/Factory/DVBS2/DVBS2.cpp:287-356)
as plain data, extended with the normal-frame / 32APSK rows BASELINE.json's configs 2-5 need
(ETSI EN 302 307; not supported by the reference, whose N_ldpc is the constant 16200:
DVBS2.hpp:49).  Pure host logic: no GPU, no oracle.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

PL_M = 90    # slot length / PLHEADER length in symbols   (Framer.hxx:38-40)
PL_P = 36    # pilot block length in symbols

# BCH primitive polynomials, coefficient of x^i at index i
BCH_PRIM_SHORT = [1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]          # DVBS2.hpp:55, GF(2^14)
BCH_PRIM_NORMAL = [1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]   # ETSI 5.3.1, GF(2^16)


@dataclass(frozen=True)
class ModCod:
    name: str
    mod: str
    cod: str
    bps: int
    cstl_file: str
    N_ldpc: int
    K_ldpc: int           # = N_bch
    K_bch: int
    bch_m: int
    bch_t: int
    itl_cols: int         # 1 = no interleaver
    itl_order: int        # 0 TOP_LEFT, 1 TOP_RIGHT
    pls: tuple            # 7-entry vector of Framer.hxx:111-126
    in_reference: bool
    ldpc_table: str

    @property
    def N_bch(self) -> int:
        return self.K_ldpc

    @property
    def N_xfec(self) -> int:          # symbols
        return self.N_ldpc // self.bps

    @property
    def S(self) -> int:
        return self.N_xfec // PL_M

    @property
    def N_pilots(self) -> int:
        # the reference's formula (DVBS2.cpp:353); equals the standard's for every row here
        return self.N_xfec // (16 * PL_M)

    @property
    def pl_frame(self) -> int:        # symbols
        return PL_M * (self.S + 1) + self.N_pilots * PL_P

    @property
    def code_rate(self) -> float:     # R used for SNR conversion (TX_RX_BB/main.cpp:142)
        return self.K_bch / self.N_ldpc

    @property
    def bch_prim(self) -> List[int]:
        return BCH_PRIM_SHORT if self.bch_m == 14 else BCH_PRIM_NORMAL


def _mc(name, mod, cod, bps, cstl, N, Kl, Kb, m, t, cols, order, pls, ref, table):
    return ModCod(name, mod, cod, bps, cstl, N, Kl, Kb, m, t, cols, order, tuple(pls), ref, table)


MODCODS = {m.name: m for m in [
    # ---- the five MODCODs the reference accepts (DVBS2.cpp:287-356, Framer.hxx:111-126)
    _mc("QPSK-S_8/9",   "QPSK",   "8/9", 2, "4QAM_GRAY.mod", 16200, 14400, 14232, 14, 12, 1, 0, [0, 0, 1, 0, 1, 0, 1], True,  "N16200_8_9.txt"),
    _mc("QPSK-S_3/5",   "QPSK",   "3/5", 2, "4QAM_GRAY.mod", 16200,  9720,  9552, 14, 12, 1, 0, [0, 0, 0, 1, 0, 1, 1], True,  "N16200_3_5.txt"),
    _mc("8PSK-S_3/5",   "8PSK",   "3/5", 3, "8PSK.mod",      16200,  9720,  9552, 14, 12, 3, 1, [0, 0, 1, 1, 0, 0, 1], True,  "N16200_3_5.txt"),
    _mc("8PSK-S_8/9",   "8PSK",   "8/9", 3, "8PSK.mod",      16200, 14400, 14232, 14, 12, 3, 0, [0, 1, 0, 0, 0, 0, 1], True,  "N16200_8_9.txt"),
    _mc("16APSK-S_8/9", "16APSK", "8/9", 4, "16APSK.mod",    16200, 14400, 14232, 14, 12, 4, 0, [0, 1, 0, 1, 1, 0, 1], True,  "N16200_8_9.txt"),
    # ---- extensions required by BASELINE.json configs 2-5 (ETSI EN 302 307)
    _mc("QPSK-N_8/9",   "QPSK",   "8/9", 2, "4QAM_GRAY.mod", 64800, 57600, 57472, 16,  8, 1, 0, [0, 0, 1, 0, 1, 0, 0], False, "N64800_8_9.txt"),
    _mc("8PSK-N_8/9",   "8PSK",   "8/9", 3, "8PSK.mod",      64800, 57600, 57472, 16,  8, 3, 0, [0, 1, 0, 0, 0, 0, 0], False, "N64800_8_9.txt"),
    _mc("16APSK-N_8/9", "16APSK", "8/9", 4, "16APSK.mod",    64800, 57600, 57472, 16,  8, 4, 0, [0, 1, 0, 1, 1, 0, 0], False, "N64800_8_9.txt"),
    _mc("32APSK-S_3/4", "32APSK", "3/4", 5, "32APSK_3_4.mod", 16200, 11880, 11712, 14, 12, 5, 0, [0, 1, 1, 0, 0, 0, 1], False, "N16200_3_4.txt"),
]}


def get_modcod(name: str) -> ModCod:
    if name == "":
        name = "QPSK-S_8/9"        # DVBS2.cpp:290 default
    if name not in MODCODS:
        # same failure mode as DVBS2.cpp:319
        raise ValueError(name + " mod-cod scheme not supported.")
    return MODCODS[name]


def pls_value(mc: ModCod, pilots: bool = True) -> int:
    """What the PLS decoder returns for a frame of this MODCOD: b0 128 + b1 64 + .. + b6 2 + pilots, b0..b6 the `pls` row (QPSK-S_8/9 with pilots: 43)."""
    v = 0
    for b in mc.pls:
        v = v << 1 | (b & 1)
    return v << 1 | bool(pilots)


def pls_name(value: int):
    """-> (the MODCOD of the table whose `pls` row is value >> 1, or None; pilots), as dvbs2hip_pls_describe"""
    if not 0 <= value <= 255:
        raise ValueError("a PLS value has 8 bits ('value' = %d)." % value)
    for m in MODCODS.values():
        if pls_value(m, False) == value & ~1:
            return m.name, bool(value & 1)
    return None, bool(value & 1)


def pls_frame_symbols(value: int) -> int:
    """pl_frame of the MODCOD of the table whose PLS value, pilots on (the only frames the library builds), is `value`; 0 when there is none: dvbs2hip_pls_frame_symbols"""
    if 0 <= value <= 255 and value & 1:
        for m in MODCODS.values():
            if pls_value(m, True) == value:
                return m.pl_frame
    return 0


# the PLHEADER search's own length table (dvbs2hip_pls_search with LEN = NULL): PL frame symbols by PLS value
PLS_FRAME_SYMBOLS = np.array([pls_frame_symbols(v) for v in range(256)], dtype=np.int32)

# what find_modcod asks of a chain per slot: the geometric mean of the largest per-slot score of buffers without a header and the smallest of the true chain at the
# lowest operating point, both measured with the float64 twin (results/pls_search/README.md, tools/measure_pls_search_qmin.py)
PLS_SEARCH_Q_MIN = 0.2805          # sqrt(0.1431 x 0.5500)


def find_modcod(res, score: float, q_min: float = None):
    """What dvbs2hip_pls_search returned, RES = (OFFSET, VALUE, COUNT, SLOTS) and SCORE -> (ModCod, pilots, offset), or None when it is not to be believed: no start, a
    single header (COUNT < 2), a chain that explains less than q_min of its slots' energy (SCORE < q_min SLOTS), or a value the table has no MODCOD for"""
    q_min = PLS_SEARCH_Q_MIN if q_min is None else q_min
    offset, value, count, slots = (int(v) for v in res)
    if offset < 0 or count < 2 or not score >= q_min * slots:
        return None
    name, pilots = pls_name(value)
    return (MODCODS[name], pilots, offset) if name else None


# the PLHEADER walk's table for a VCM stream (dvbs2hip_pls_walk's LEN): the frames the library builds, and value 0, the dummy PLFRAME with pilots off -- a header and 36
# slots of 90 symbols -- which a receiver has to step over.  Value 1 (a dummy frame with the pilot bit set) and data frames without pilots are left out: the library
# neither builds nor decodes them, and a header that names one ends the walk as LOST
VCM_FRAME_SYMBOLS = PLS_FRAME_SYMBOLS.copy()
VCM_FRAME_SYMBOLS[0] = 90 + 36 * 90


def find_vcm_start(PLS, MET, ENE, LEN=None, q_min: float = None):
    """Acquisition of a VCM stream on the host, once per stream: (PLS, MET, ENE) of one pls_scan of the stream's head -> the offset k < max(LEN) whose walk (the walk of
    dvbs2hip_pls_walk from k over the scanned symbols, max_out unbounded) accepts the most headers -- every frame it counts, and the header of a last frame that the
    buffer cuts off -- the smallest k among equal counts; None when no walk accepts two."""
    LEN = VCM_FRAME_SYMBOLS if LEN is None else LEN
    q_min = PLS_SEARCH_Q_MIN if q_min is None else q_min
    PLS, MET, ENE = np.asarray(PLS, np.int64), np.asarray(MET, np.float32), np.asarray(ENE, np.float32)
    L = np.asarray(LEN, np.int64).copy()
    L[(L < 90) | (L % 18 != 0)] = 0
    K = PLS.size
    n_sym = K + 89
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(ENE == 0, np.float32(0), (MET * MET) / (np.float32(90) * ENE))
    hop = L[PLS & 255]
    ok = np.flatnonzero((hop > 0) & (q >= np.float32(q_min)))
    count = {}
    for k in ok[::-1]:                                      # a walk's count from its successor's: the chain goes forward only
        nxt = int(k + hop[k])
        count[int(k)] = 1 + (count.get(nxt, 0) if nxt <= n_sym else 0)
    best = None
    for k in ok:
        if k >= L.max():
            break
        if count[int(k)] >= 2 and (best is None or count[int(k)] > count[best]):
            best = int(k)
    return best


def load_ldpc_table(fname: str):
    """-> (row_ptr int32[n_rows+1], addr int32[n_addr]) from dvbs2_amd/data/ldpc/<fname>."""
    rows = []
    with open(os.path.join(_DATA, "ldpc", fname)) as fh:
        for line in fh:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            rows.append([int(x) for x in line.split()])
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    addr = np.array([a for r in rows for a in r], dtype=np.int32)
    return row_ptr, addr


def load_constellation(fname: str) -> np.ndarray:
    """Raw (un-normalised) points, float32 [n_pts, 2]; index = line order (conf/mod/*.mod)."""
    pts = []
    with open(os.path.join(_DATA, "mod", fname)) as fh:
        for line in fh:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            a, b = line.split()[:2]
            pts.append((float(a), float(b)))
    return np.array(pts, dtype=np.float32)


def normalise_constellation(pts: np.ndarray) -> np.ndarray:
    """Unit mean energy in fp32, as tools::Constellation_user does."""
    pts = np.asarray(pts, dtype=np.float32)
    es = np.float32(0)
    for p in pts:
        es = np.float32(es + np.float32(p[0] * p[0] + p[1] * p[1]))
    s = np.sqrt(np.float32(es / np.float32(len(pts))), dtype=np.float32)
    return (pts / s).astype(np.float32)


def ebn0_to_esn0(ebn0_db: float, rate: float, bps: int) -> float:
    return ebn0_db + 10.0 * math.log10(rate * bps)     # TX_RX_BB/main.cpp:142-146


def esn0_to_sigma(esn0_db: float) -> float:
    return math.sqrt(1.0 / (2.0 * 10.0 ** (esn0_db / 10.0)))


def rrc_taps(rolloff: float = 0.2, osf: int = 2, grp_delay: int = 20) -> np.ndarray:
    """fp32 restatement of Filter_RRC_ccr_naive::compute_rrc_coefs
    (src/common/Module/Filter/Filter_FIR/Filter_RRC/Filter_RRC_ccr_naive.cpp:13-48);
    defaults from Shaping_filter.hpp:24-28 -> 81 taps."""
    f = np.float32
    pi = f(3.1415926535897932384626433832795)
    ro = f(rolloff)
    c = grp_delay * osf
    taps = np.zeros(2 * c + 1, dtype=np.float32)
    eps = np.finfo(np.float32).eps
    taps[c] = f(1.0) - ro + f(4.0) * ro / pi
    en = f(taps[c] * taps[c])
    for i in range(1, c + 1):
        t = f(i) / f(osf)
        if abs(f(4.0) * ro * t - f(1.0)) <= eps or abs(f(4.0) * ro * t + f(1.0)) <= eps:
            v = ro / np.sqrt(f(2.0)) * ((f(1.0) + f(2.0) / pi) * np.sin(pi / (f(4.0) * ro)) +
                                         (f(1.0) - f(2.0) / pi) * np.cos(pi / (f(4.0) * ro)))
        else:
            den = pi * t * (f(1.0) - f(16.0) * ro * ro * t * t)
            num = np.sin(pi * t * (f(1.0) - ro)) + f(4.0) * ro * t * np.cos(pi * t * (f(1.0) + ro))
            v = num / den
        taps[c + i] = v
        taps[c - i] = v
        en = f(en + f(v * v + v * v))
    return (taps / np.sqrt(en)).astype(np.float32)
