"""The PLS decoder's float64 reference, and what can be said about the PLS code without a GPU.

The reference is everything above the tests: the 256 PLHEADERs the framer can build (Framer.hxx:97-196 of the reference project: seven bits times G, every coded bit
twice with the pairing bit, the 64-bit scrambler, pi/2-BPSK, times j for b0 = 1, behind the SOF) and an exhaustive search over |r . conj(H)|, smallest value first among
equal metrics.  It shares nothing with the decomposition of dvbs2_amd/csrc/k_pls.hip; tests/test_pls_gpu.py imports it from here."""
import numpy as np
import pytest

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


def header(bits7, pilots=1):
    """-> complex128[90]"""
    c = (np.asarray(bits7) @ G) % 2
    y = np.empty(64, int)
    y[0::2], y[1::2] = c, c ^ pilots
    s = 1 - 2 * np.concatenate([SOF, y ^ SCR])
    base = np.where(np.arange(90) % 2 == 0, 1 + 1j, -1 + 1j) / np.sqrt(2)
    base[26:] *= 1j if bits7[0] else 1
    return base * s


def value_bits(V):
    """V = b0 128 + .. + b6 2 + p -> ((b0 .. b6), p)"""
    return tuple((V >> (7 - k)) & 1 for k in range(7)), V & 1


HEADERS = np.array([header(*value_bits(V)) for V in range(256)])                    # row V


def ml_decode(r):
    """r complex128[F, 90] -> (V, metric, all 256 metrics); np.argmax takes the first of equal ones: the smallest V"""
    m = np.abs(r @ HEADERS.conj().T)
    V = m.argmax(1)
    return V, m[np.arange(len(r)), V], m


def test_reference_headers_are_what_the_framer_encodes(O, P):
    for mc in P.MODCODS.values():
        plh = O.plheader(mc.pls).reshape(90, 2)                                     # float32, the oracle's restatement of Framer::generate_plh
        h = HEADERS[P.pls_value(mc)]
        assert np.array_equal(h.real.astype(np.float32), plh[:, 0]) and np.array_equal(h.imag.astype(np.float32), plh[:, 1]), mc.name
    assert P.pls_value(P.get_modcod("QPSK-S_8/9")) == 43 and P.pls_value(P.get_modcod("QPSK-S_3/5")) == 23


def test_the_256_headers_are_distinct_and_38_of_90_apart():
    C = np.abs(HEADERS @ HEADERS.conj().T)
    assert np.allclose(np.diag(C), 90.0, atol=1e-9)
    np.fill_diagonal(C, 0.0)
    assert abs(C.max() - 38.0) < 1e-9                                                # the largest |cross-correlation| of two different headers
    assert len(np.unique(np.round(HEADERS * np.sqrt(2)), axis=0)) == 256
    V, met, _ = ml_decode(HEADERS * np.exp(0.7j))
    assert np.array_equal(V, np.arange(256)) and np.allclose(met, 90.0)


def test_pls_name_round_trips_the_table(P):
    for mc in P.MODCODS.values():
        for pil in (True, False):
            assert P.pls_name(P.pls_value(mc, pil)) == (mc.name, pil)
    used = {P.pls_value(mc, False) for mc in P.MODCODS.values()}
    free = next(v for v in range(0, 256, 2) if v not in used)
    assert P.pls_name(free) == (None, False) and P.pls_name(free + 1) == (None, True)
    assert P.pls_name(128 + 43) == (None, True)                                      # the extension bit set: no MODCOD of the table
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            P.pls_name(bad)
