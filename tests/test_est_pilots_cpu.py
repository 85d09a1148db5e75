"""The pilot-aided noise estimator without a GPU: its float64 reference (tests/est_pilots_ref.py) against the oracle's framer and PL scrambler, what it measures where
the reference project's M2M4 estimator cannot, the averaging, and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import est_pilots_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_WANT = {"QPSK-S_8/9": 270, "8PSK-S_3/5": 198, "16APSK-S_8/9": 162, "32APSK-S_3/4": 162, "QPSK-N_8/9": 882, "16APSK-N_8/9": 486}


def test_known_positions_and_values_are_the_framers(O, P):
    seq = R.pl_sequence()
    for mc in P.MODCODS.values():
        n = mc.N_xfec
        pos, val = R.positions(n), R.values(mc.pls, n)
        assert len(pos) == len(val) == 90 + 36 * R.n_pilots(n) and len(np.unique(pos)) == len(pos) and pos.max() < mc.pl_frame
        if mc.name in L_WANT:
            assert len(pos) == L_WANT[mc.name]
        # a frame whose data symbols are zero: what is left is the header and the pilots, where the reference says they are and with its values
        plh = O.plheader(mc.pls)
        plf = O.framer_generate(np.zeros(2 * n, np.float32), plh).reshape(-1, 2)
        there = np.zeros(mc.pl_frame, bool); there[pos] = True
        assert np.array_equal(there, (plf != 0).any(1)), mc.name
        assert np.array_equal(val.real.astype(np.float32), plf[pos, 0]) and np.array_equal(val.imag.astype(np.float32), plf[pos, 1]), mc.name
        assert np.array_equal(plf[:90].ravel(), plh)
        # the reference's descrambling of the pilots is the oracle's descrambler at those positions, bit for bit, and it undoes the scrambler
        x = np.random.default_rng(n).standard_normal((1, 2 * mc.pl_frame)).astype(np.float32)
        d = O.pl_scramble(x[0], 90, False).reshape(-1, 2)
        got = R.known(x, n, scrambled=True)[0]
        assert np.array_equal(got.real.astype(np.float32), d[pos, 0]) and np.array_equal(got.imag.astype(np.float32), d[pos, 1]), mc.name
        s = O.pl_scramble(plf.ravel(), 90, True)[None, :]
        back = R.known(s, n, scrambled=True)[0]
        assert np.array_equal(back.real.astype(np.float32), plf[pos, 0]) and np.array_equal(back.imag.astype(np.float32), plf[pos, 1])
    assert seq.shape == (66420,) and set(np.unique(seq)) == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def apsk16_at_14_db(O, P):
    """400 frames of 16APSK-S_8/9 at a true Es/N0 of 14 dB -> (mc, PL frames as the frame synchronizer delivers them, their XFEC symbols)"""
    from helpers import chain
    ch = chain(O, "16APSK-S_8/9")
    mc = ch.mc
    rng = np.random.default_rng(14)
    sigma = P.esn0_to_sigma(14.0)
    pl, xfec = np.empty((400, 2 * mc.pl_frame), np.float32), np.empty((400, 2 * mc.N_xfec), np.float32)
    for f in range(400):
        sym = O.modulate(ch.cstl, mc.bps, rng.integers(0, 2, mc.N_ldpc).astype(np.int32))
        clean = O.pl_scramble(O.framer_generate(sym, ch.plh), 90, True)
        pl[f] = clean + (sigma * rng.standard_normal(clean.size)).astype(np.float32)
        xfec[f] = O.framer_remove_plh(O.pl_scramble(pl[f], 90, False), mc.N_xfec)
    return mc, pl, xfec


def test_unbiased_where_m2m4_is_not(O, apsk16_at_14_db):
    mc, pl, xfec = apsk16_at_14_db
    sig, eb, es = R.estimate(pl, mc, scrambled=True)
    m2m4 = np.array([O.estimate(x, mc.code_rate, mc.bps)[2] for x in xfec])
    print("16APSK-S_8/9 at 14 dB: pilots %.3f +- %.3f (standard error %.3f), M2M4 %.3f +- %.3f" % (es.mean(), es.std(), es.std() / 20, m2m4.mean(), m2m4.std()))
    assert abs(es.mean() - 14.0) < 0.1
    assert m2m4.mean() < 9.0
    assert np.allclose(sig, np.sqrt(1 / (2 * 10 ** (es / 10)))) and np.allclose(eb, es - 10 * np.log10(mc.code_rate * mc.bps))
    # the same on frames that are already descrambled, and under a constant phase
    d = np.stack([O.pl_scramble(x, 90, False) for x in pl[:8]])
    assert np.array_equal(R.estimate(d, mc, scrambled=False)[2], es[:8])
    c = (pl[:8, 0::2] + 1j * pl[:8, 1::2]) * np.exp(0.3j)
    turned = np.empty_like(pl[:8]); turned[:, 0::2], turned[:, 1::2] = c.real, c.imag
    assert np.allclose(R.estimate(turned, mc, scrambled=True)[2], es[:8], atol=1e-4)


def test_averaging_halves_the_spread_and_carries_its_state(apsk16_at_14_db):
    mc, pl, _ = apsk16_at_14_db
    es0 = R.estimate(pl, mc)[2]
    _, _, es9, state = R.estimate(pl, mc, alpha=0.9)
    print("std of Es_N0 over frames 100..399: per frame %.3f, alpha 0.9 %.3f" % (es0[100:].std(), es9[100:].std()))
    assert es9[100:].std() < 0.5 * es0[100:].std()
    assert es9[0] == es0[0] and abs(es9[100:].mean() - 14.0) < 0.1
    a = R.estimate(pl[:5], mc, alpha=0.9)
    b = R.estimate(pl[5:12], mc, alpha=0.9, state=a[3])
    assert np.array_equal(np.concatenate([a[2], b[2]]), es9[:12])
    three = R.estimate(pl[:12], mc, alpha=0.9, streams=3)[2]                         # stream s = frames [4 s, 4 s + 4)
    assert np.array_equal(three, np.concatenate([R.estimate(pl[4 * s:4 * s + 4], mc, alpha=0.9)[2] for s in range(3)]))


def test_edge_cases_of_the_reference(P):
    mc = P.get_modcod("32APSK-S_3/4")
    x = np.zeros((2, 2 * mc.pl_frame), np.float32)
    pos, val = R.positions(mc.N_xfec), R.values(mc.pls, mc.N_xfec)
    x[0, 2 * pos], x[0, 2 * pos + 1] = val.real, val.imag                            # no noise; frame 1: nothing at all
    sig, eb, es = R.estimate(x, mc, scrambled=False)
    assert es[0] == 100.0 and es[1] == -100.0 and np.isfinite(sig).all() and sig[0] == np.sqrt(0.5e-10)


CTYPE = {"dvbs2hip_t *": C.c_void_p, "const float *": C.c_void_p, "float *": C.c_void_p, "const float *const *": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}


def test_binding_lists_every_new_symbol_with_the_headers_arguments():
    from dvbs2_amd import lib_binding as B
    from dvbs2_amd.receiver import Dvbs2Hip
    hdr = open(os.path.join(ROOT, "include", "dvbs2hip.h")).read()
    protos = dict(re.findall(r"^int (dvbs2hip_estimate_pilots\w*)\(([^)]*)\);", hdr, re.M))
    assert sorted(protos) == ["dvbs2hip_estimate_pilots", "dvbs2hip_estimate_pilots_dev", "dvbs2hip_estimate_pilots_located_dev", "dvbs2hip_estimate_pilots_reset",
                              "dvbs2hip_estimate_pilots_set_alpha"]
    for name, args in protos.items():
        types = [CTYPE[re.sub(r"\w+$", "", a.strip()).strip()] for a in args.split(",")]
        assert B.ABI[name] == (C.c_int, types), name
        assert callable(getattr(Dvbs2Hip, name[len("dvbs2hip_"):]))


def test_parsers_take_the_estimator_and_default_to_the_reference_one():
    from dvbs2_amd import rx, sim
    ap = rx.build_parser()
    assert ap.parse_args(["--rad-rx-file-path", "x.bin"]).est_type == "DVBS2"
    assert ap.parse_args(["--rad-rx-file-path", "x.bin", "--est-type", "PILOTS"]).est_type == "PILOTS"
    ap = sim.build_parser()
    assert ap.parse_args([]).est_type == "DVBS2" and ap.parse_args(["--est-type", "PILOTS"]).est_type == "PILOTS"


@pytest.mark.parametrize("fine", [False, True])
def test_the_sequence_takes_sigma_from_the_pilots_only_when_asked(fine):
    """no GPU: the calls RxSequence.decode makes -- DVBS2 (the default) as before, PILOTS one estimate_pilots call in place of estimate (task by task, on the descrambled
    frames) or in front of the fused chain (on the aligned frames)"""
    import stepmf_ref as SR
    from dvbs2_amd.rx_sequence import RxSequence

    class Spy(SR.RecordingHandle):
        def estimate_pilots(self, X_N1, scrambled=True):
            F = np.asarray(X_N1).reshape(-1, 2 * self.n).shape[0]
            self._rec("estimate_pilots", (bool(scrambled),), X_N1)
            return tuple(np.full(F, v, np.float32) for v in (0.15, 8.0, 14.0))

        def rx_bb(self, pl_frames, sigma=None, out=None):                            # (sigma may be an array here)
            return SR.RecordingHandle.rx_bb(self, pl_frames, sigma=None if sigma is None else float(np.asarray(sigma).ravel()[0]), out=out)

    logs = {}
    for est in ("DVBS2", "PILOTS"):
        h = Spy()
        seq = RxSequence(h, 2, pl_frame=h.n, fine=fine, fused=not fine, estimator=est)
        seq.decode(SR.RecordingHandle._fill(3, (2, 2 * h.n)))
        logs[est] = h.log
    names = {k: [e[0] for e in v] for k, v in logs.items()}
    assert "estimate_pilots" not in names["DVBS2"]
    assert names["PILOTS"].count("estimate_pilots") == 1
    call = next(e for e in logs["PILOTS"] if e[0] == "estimate_pilots")
    assert call[1] == [not fine]
    if fine:
        assert "estimate" in names["DVBS2"] and "estimate" not in names["PILOTS"]
        assert [n for n in names["PILOTS"] if n != "estimate_pilots"] == [n for n in names["DVBS2"] if n != "estimate"]
    else:
        assert [n for n in names["PILOTS"] if n != "estimate_pilots"] == names["DVBS2"] == ["init", "rx_bb"]
    with pytest.raises(ValueError):
        RxSequence(Spy(), 2, estimator="M2M4")
