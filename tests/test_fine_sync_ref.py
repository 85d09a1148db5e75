"""The test of the tests: tests/fine_sync_ref.py (float64 references of the two pilot-aided fine synchronizers, the model of the four rotation
forms' index arithmetic) against the C oracle on the whole case table, and the bars of tests/test_fine_sync_fp64_gpu.py against nine
mistakes a kernel could make, on the CPU.

The "device" of the mutation test is the reference itself with one mistake put in: its estimates are the float64 ones rounded to float32,
its rotated frames come from the form's indices and rotate64's arithmetic.  Without a mistake it meets every bar on every row; with any of
the nine it misses at least one (results/fine_sync_fp64/README.md has the table this test prints).

About "the unwrap with floor in both directions": floorf(d / 2 pi + 0.5) and ceilf(d / 2 pi - 0.5) are both round-to-nearest and differ at
exact ties only, so writing the upward expression in the downward branch is no mistake.  The mistake modelled is ceilf turned into floorf in
the downward branch, floorf(d / 2 pi - 0.5): one turn too many on every downward step.
"""
import numpy as np
import pytest

import fine_sync_ref as R


@pytest.fixture(scope="module")
def Yd(O):
    return R.oracle_yardstick(O)


def test_table_holds_its_conditions(O):
    """the 0.05 rad margin of every freq_phase row (asserted from float64, before anything is compared), and what the table has to contain:
    an upward and a downward unwrap, a frame with two pilot blocks, a frame whose n / 2 is no multiple of 1024"""
    up = down = 0
    Ps, ragged, worst = set(), [], (np.inf, np.inf)
    for mc in R.modcods():
        X = R.table_inputs(O, mc, "fp")
        infos = R.assert_margins(X)
        for m in infos:
            up += int(np.sum(m["turns"] > 0)); down += int(np.sum(m["turns"] < 0))
            worst = (min(worst[0], m["step_margin"]), min(worst[1], m["seam_margin"]))
        Ps.add(infos[0]["P"])
        n = X.shape[1] // 2
        assert n % 2 == 0 and R.table_inputs(O, mc, "lr").shape == X.shape
        if (n // 2) % 1024:
            ragged.append((mc, n // 2))
    print("margins: step %.3f rad, seam %.3f rad; unwraps up %d down %d; pilot blocks %s; ragged %s" % (worst + (up, down, sorted(Ps), ragged)))
    assert up >= 1 and down >= 1 and 2 in Ps and ragged
    assert ("8PSK-N_8/9", 11115) in ragged and Ps >= {2, 3, 11, 15}


def test_estimators_on_a_clean_tone():
    """the references from their definitions: pilots (1 + j) / sqrt 2 turned by a known line give that line back; the L&R term has the
    phase of ten lags' mean"""
    n = 8370
    k = np.arange(n)
    for f, ph in ((2e-4, 0.3), (-3e-4, 0.9), (0.0, 0.0001)):
        c = np.exp(2j * np.pi * (f * k + ph)) * (1 + 1j) / np.sqrt(2)
        x = np.stack([c.real, c.imag], 1).reshape(-1)
        ef, ep, info = R.fp_estimate64(x)
        # (a block's 36 samples are centred on start + 17.5, the definition's t is start + 18: half a sample of f in the phase)
        assert abs(ef - f) < 1e-12 and abs((ep - (ph - 0.5 * f) + 0.5) % 1 - 0.5) < 1e-9 and info["P"] == 5
    for f in (1e-4, -3e-3, 0.04, -0.09):
        c = np.exp(2j * np.pi * f * k) * (1 + 1j) / np.sqrt(2)
        x = np.stack([c.real, c.imag], 1).reshape(-1)
        est, Rl = R.lr_estimates64([x, x], 0.5)
        # every lag m contributes e^{j 2 pi f m} / 2 per pilot block (|z|^2 = 2, 18 - m terms, divided by 2 (18 - m))
        assert abs(R.lr_pilot64(x) - 5 * np.sum(np.exp(2j * np.pi * f * np.arange(1, 10)))) < 1e-9
        assert abs(Rl - 0.75 * R.lr_pilot64(x)) < 1e-9 and est[0] == pytest.approx(est[1], abs=1e-15)
        assert abs(est[0] - f * 5 / 10 * 2) < abs(f) * 0.02 + 1e-12      # the mean of lags 1..9 is lag 5: atan2 = 2 pi f 5, over 10 pi


def test_form_indices_visit_every_sample_once_with_its_own_index():
    for n, F in ((3402, 3), (22230, 2), (8370, 1), (7, 2)):
        want_k, want_f = np.tile(np.arange(n), (F, 1)), np.repeat(np.arange(F), n).reshape(F, n)
        for form in ("flat", "pair", "chunk") if n % 2 == 0 else ("flat",):
            k, f = R.form_indices(form, n, F)
            assert np.array_equal(k, want_k) and np.array_equal(f, want_f), (form, n, F)


def test_reference_against_the_oracle_on_the_whole_table(Yd):
    """the oracle's estimates within the existing GPU test's bars of float64 (FRQ 1e-6, PHS 1e-4), its rotated frames within fp32 arithmetic of
    rotate64 of its own estimates: cosf and sinf within an ulp (2^-23 each on values up to 1), two products and a sum rounded once each
    (2^-24 relative each) -- per component at most (|x_re| + |x_im|) (2^-23 + 2^-24) + 2^-24 |y|, as a complex magnitude below 4 x 2^-23 |x|"""
    for r in Yd.rows:
        assert r["frq_err"] <= R.FRQ_BAR and r["phs_err"] <= R.PHS_BAR and r["rot"] <= 4 * 2.0 ** -23, r
    for mc in R.modcods():
        for sync in ("fp", "lr"):
            rows = [r for r in Yd.rows if r["modcod"] == mc and r["sync"] == sync]
            print("oracle %-13s %s  rot %.2e  frq %.2e  phs %.2e" % (mc, sync, max(r["rot"] for r in rows), max(r["frq_err"] for r in rows), max(r["phs_err"] for r in rows)))
    print("oracle against float64: E_orc L&R %.3e freq_phase %.3e; freq_phase FRQ %.3e PHS %.3e; L&R FRQ %.3e" % (Yd.E[0], Yd.E[1], Yd.fp_frq, Yd.fp_phs, Yd.lr_frq))
    assert 2.0 ** -26 < Yd.E[0] and 2.0 ** -26 < Yd.E[1]             # a yardstick, not zero: fp32 arithmetic was measured
    assert 0 < Yd.fp_frq and 0 < Yd.fp_phs and 0 < Yd.lr_frq


def test_rotation_bar_takes_either_rounding_of_the_phase_argument(O, Yd):
    """freq_phase forms ef k + ep in fp32: one rounding where the compiler contracts it, two where it does not (the oracle, and the library as
    it is built).  The oracle's own frames show that amb_k does not let the one-rounding reference do for both -- on the long frames they are
    outside (4 E + amb_k) |x_k| of it, by up to 1.8 -- while against their own rounding they are inside E: check_rows holds every sample to
    the bar against either, and the oracle in the device's place meets every bar"""
    worst = {}
    for mc in R.modcods():
        X, f_rows, refs = R.table_refs(O, Yd, mc, "fp")
        got = [O.sync_freq_phase(x) for x in X]
        rows = R.check_rows("fp", f_rows, X, [g[0] for g in got], [g[1] for g in got], [g[2] for g in got], **refs)
        assert not any(r["broken"] for r in rows), (mc, rows)
        assert all(r["rot_unfused"] <= refs["E"] for r in rows)
        worst[mc] = max(r["rot_fused_over_bar"] for r in rows)
        print("oracle frames against the one-rounding reference: %-13s worst sample at %.2f of its bar" % (mc, worst[mc]))
    assert worst["QPSK-N_8/9"] > 1 and worst["8PSK-N_8/9"] > 1


def test_oracle_recurrence_against_float64(O):
    """the damped form, as the GPU test runs it: alpha 0.7 over the six frames, the six again, the six reversed; the oracle object stays within
    the existing FRQ bar of the float64 recurrence, and its final R within fp32 of the float64 one"""
    for mc in ("32APSK-S_3/4", "QPSK-N_8/9"):
        X = R.table_inputs(O, mc, "lr")
        seq = np.concatenate([X, X, X[::-1]])
        lr = O.SyncLR(X.shape[1] // 2, alpha=0.7)
        got = np.array([lr.synchronize(x)[0] for x in seq])
        est, Rl = R.lr_estimates64(seq, 0.7)
        print("oracle recurrence %-13s max |FRQ - float64| %.3e" % (mc, np.max(np.abs(got - est))))
        assert np.max(np.abs(got - est)) <= R.FRQ_BAR
        assert abs(complex(lr.R_l[0], lr.R_l[1]) - Rl) <= 1e-5 * abs(Rl)


# ---------------------------------------------------------------------------------------------------------------- which bar sees which mistake
# name -> (synchronizers, rotation forms, hooks of the estimator, hooks of model_rotate)
MUTATIONS = {
    "k + 1 for k on the second sample of a pair": (("fp", "lr"), ("pair", "chunk"), {}, {"second": 2}),
    "chunk base off by one pair": (("lr",), ("chunk",), {}, {"chunk_base": 1}),
    "k for 2 k in mode 0": (("lr",), ("pair", "chunk", "flat"), {}, {"kmul": 1}),
    "first sample with the previous frame's estimate": (("fp", "lr"), ("flat",), {}, {"first_from_previous": True}),
    "pilot start 1529": (("fp", "lr"), ("pair",), {"first": 1529}, {}),
    "17 for 18 samples of a pilot block (L&R)": (("lr",), ("pair",), {"lp": 17}, {}),
    "unwrap left out": (("fp",), ("pair",), {"unwrap": "none"}, {}),
    "unwrap with floor in both directions": (("fp",), ("pair",), {"unwrap": "floor"}, {}),
    "frequency's sign flipped": (("fp", "lr"), ("pair", "chunk", "flat"), {}, {"sign": -1.0}),
}
FORMS_OF = {"fp": ("pair", "flat"), "lr": ("pair", "chunk", "flat")}       # freq_phase has no chunked form


def _model_device(O, Yd, mc, sync, form, est_hooks, rot_hooks):
    X, f_rows, refs = R.table_refs(O, Yd, mc, sync)
    if sync == "fp":
        e = [R.fp_estimate64(x, **est_hooks)[:2] for x in X]
        FRQ, PHS = np.array([v[0] for v in e], np.float32), np.array([v[1] for v in e], np.float32)
    else:
        FRQ = np.array([R.lr_estimates64(X[i:i + 1], 0.0, **est_hooks)[0][0] for i in range(len(f_rows))], np.float32)
        PHS = np.zeros_like(FRQ)
    Y = R.model_rotate(X, FRQ, PHS, 1 if sync == "fp" else 0, form, **rot_hooks)
    return R.check_rows(sync, f_rows, X, FRQ, PHS, Y, **refs)


def test_every_mistake_is_seen_by_a_bar(O, Yd):
    for mc in R.modcods():                                # the model without a mistake meets every bar, in every form
        for sync in ("fp", "lr"):
            for form in FORMS_OF[sync]:
                for r in _model_device(O, Yd, mc, sync, form, {}, {}):
                    assert not r["broken"], (mc, sync, form, r)
    for name, (syncs, forms, est_hooks, rot_hooks) in MUTATIONS.items():
        seen = {}
        for mc in R.modcods():
            for sync in syncs:
                if sync == "fp" and est_hooks.get("lp"):
                    continue
                for form in forms:
                    if form not in FORMS_OF[sync]:
                        continue
                    hooks = {k: v for k, v in est_hooks.items() if not (sync == "lr" and k == "unwrap")}
                    for r in _model_device(O, Yd, mc, sync, form, hooks, rot_hooks):
                        for bar in r["broken"]:
                            seen.setdefault((sync, bar), []).append((mc, form, r["f"]))
        print("mutation: %s" % name)
        for (sync, bar), rows in sorted(seen.items()):
            total = len(R.FP_FREQS) * len(R.modcods()) * len([f for f in forms if f in FORMS_OF[sync]])
            print("    %-2s %-8s %3d of %3d rows, e.g. %s" % (sync, bar, len(rows), total, "; ".join("%s %s f=%g" % q for q in rows[:3])))
        assert seen, name
