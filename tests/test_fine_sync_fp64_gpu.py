"""The fine frequency / phase synchronizers of k_sync.hip against float64 (tests/fine_sync_ref.py), on the case table that
tests/test_fine_sync_ref.py checks on the CPU: all nine MODCODs, both signs of the frequency, L&R out to |f| = 0.04.

No bar here is a number taken from the kernels.  Each is formed when the test runs, from the float64 reference and the oracle's own fp32
error on the same inputs (fine_sync_ref.oracle_yardstick):

    rotation    |Y_k - rotate64(x, FRQ_dev, PHS_dev)_k| <= (4 E_orc + amb_k) |x_k| per sample: against the rotation by the estimate the device
                itself reported, its fp32 phase argument reproduced, so that a slip of one sample (2 pi |f| |x_k|, at least four times the bar:
                asserted) cannot hide behind an estimate's error.  freq_phase's ef k + ep is one fp32 rounding or two, as the compiler was
                told: a sample is held to this bar against either (fine_sync_ref.check_rows says why amb_k alone does not cover the other)
    estimates   |FRQ_dev - float64| <= 4 x the oracle's largest error over the table (PHS likewise), and within the 1e-6 / 1e-4 of the oracle
                that tests/test_sync_gpu.py has always asked for

Every test prints its figures (results/fine_sync_fp64/README.md keeps a run's)."""
import ctypes as C

import numpy as np
import pytest

import fine_sync_ref as R

pytestmark = pytest.mark.gpu
vp = C.c_void_p


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


@pytest.fixture(scope="module")
def Yd(O):
    return R.oracle_yardstick(O)


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint32) for a in arrays]


def _same_bits(a, b):
    return all(np.array_equal(u, v) for u, v in zip(_bits(*a), _bits(*b)))


def _hold(tag, mc, rows):
    """print a batch's figures, then assert that no row misses a bar"""
    for r in rows:
        print("fine_fp64 %-22s %-13s f=%-8g rot %.3e (bar %.3e, worst sample at %.2f of its bar) FRQ-f64 %.3e FRQ-orc %.3e%s"
              % (tag, mc, r["f"], r["rot"], r["rot_bar"], r["rot_over_bar"], r["frq_err"], r["frq_orc"],
                 " PHS-f64 %.3e PHS-orc %.3e | one rounding of ef k + ep: %.3e = %.2f of the bar, two: %.3e = %.2f"
                 % (r["phs_err"], r["phs_orc"], r["rot_fused"], r["rot_fused_over_bar"], r["rot_unfused"], r["rot_unfused_over_bar"]) if "phs_err" in r else ""))
    bad = [(r["f"], sorted(r["broken"])) for r in rows if r["broken"]]
    assert not bad, (tag, mc, bad)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from test_plan_digest import build_probe
    exe = str(tmp_path_factory.mktemp("fine_fp64") / "plan_probe")
    build_probe(exe)
    return exe


def _lr_form(monkeypatch, form, probe=None, n=0):
    """sets the knob of the asked form; with the probe, -> the kernel lr_choose (dvbs2_amd/csrc/rx_dispatch.h) names for a one-stream call on aligned sockets under
    it, which has to be the one launch / the pair rotation of the three"""
    if form == "unfused":
        monkeypatch.setenv("DVBS2HIP_LR", "unfused")
    else:
        monkeypatch.delenv("DVBS2HIP_LR", raising=False)
    if probe:
        from test_rx_dispatch import lr_form
        name = lr_form(probe, 1, n)
        assert name == ("sff_lr_fused_kernel" if form == "fused" else "sff_rotate2_kernel<0>"), (form, name)
        return name


@pytest.mark.parametrize("modcod", R.modcods())
def test_freq_phase_host_form_against_float64(O, Rx, Yd, modcod):
    """the six frequencies as one call of six frames: estimates and rotation against float64; the task has no state, so every frame alone
    gives the bits it gives in the batch"""
    X, f_rows, refs = R.table_refs(O, Yd, modcod, "fp")
    print("fine_fp64 bars: E_orc %.3e, FRQ %.3e, PHS %.3e" % (refs["E"], refs["frq_bar"], refs["phs_bar"]))
    rx = Rx(modcod, max_frames=len(f_rows))
    FRQ, PHS, Y = rx.sync_freq_phase_synchronize(X)
    _hold("freq_phase", modcod, R.check_rows("fp", f_rows, X, FRQ, PHS, Y, **refs))
    for i in range(len(f_rows)):
        one = rx.sync_freq_phase_synchronize(X[i:i + 1])
        assert _same_bits(one, (FRQ[i:i + 1], PHS[i:i + 1], Y[i:i + 1])), i
    rx.close()


@pytest.mark.parametrize("modcod", R.modcods())
def test_lr_both_forms_against_float64(O, Rx, Yd, monkeypatch, probe, modcod):
    """alpha 0: every frame's estimate is its own -- estimates against lr_estimates64, rotation against rotate64.  alpha 0.7 over the six
    frames, the six again, the six reversed: the recurrence against the float64 recurrence (which carries its own R), held to 4 x the error
    of the oracle object on the same sequence.  sff_lr_fused_kernel (default) and the three-kernel path give the same bits throughout."""
    X, f_rows, refs = R.table_refs(O, Yd, modcod, "lr")
    n, F = X.shape[1] // 2, len(f_rows)
    calls = [X, X, X[::-1].copy()]
    seq = np.concatenate(calls)
    est64, _ = R.lr_estimates64(seq, 0.7)
    lr = O.SyncLR(n, alpha=0.7)
    est_o = np.array([lr.synchronize(x)[0] for x in seq])
    seq_bar = 4 * float(np.max(np.abs(est_o - est64)))
    print("fine_fp64 bars: E_orc %.3e, FRQ alpha 0 %.3e, FRQ alpha 0.7 %.3e" % (refs["E"], refs["frq_bar"], seq_bar))
    out = {}
    for form in ("fused", "unfused"):
        print("fine_fp64 L&R %s: %s" % (form, _lr_form(monkeypatch, form, probe, n)))
        rx = Rx(modcod, max_frames=F)
        rx.sync_lr_set_alpha(0.0)
        FRQ, PHS, Y = rx.sync_lr_synchronize(X)
        assert not PHS.any()
        _hold("L&R %s alpha 0" % form, modcod, R.check_rows("lr", f_rows, X, FRQ, PHS, Y, **refs))
        rx.sync_lr_reset(); rx.sync_lr_set_alpha(0.7)
        got = [rx.sync_lr_synchronize(x) for x in calls]
        for c, (frq, phs, y) in enumerate(got):
            s = slice(c * F, (c + 1) * F)
            fr = f_rows if c < 2 else f_rows[::-1]
            _hold("L&R %s alpha 0.7 call %d" % (form, c), modcod,
                  R.check_rows("lr", fr, calls[c], frq, phs, y, E=refs["E"], frq64=est64[s], frq_bar=seq_bar, frq_o=est_o[s]))
        assert rx.sync_lr_timeouts() == 0
        out[form] = [(FRQ, PHS, Y)] + got
        rx.close()
    for a, b in zip(out["fused"], out["unfused"]):
        assert _same_bits(a, b)


def test_lr_repaired_call_against_float64(O, Rx, Yd, monkeypatch):
    """DVBS2HIP_LR_TIMEOUT_US=0: waiting workgroups give up at their first unsuccessful poll and the host rotates the call again (sff_lr_recover,
    through the launcher).  8PSK-N: 11115 pairs per frame, ten whole chunks and a ragged one."""
    modcod = "8PSK-N_8/9"
    X, f_rows, refs = R.table_refs(O, Yd, modcod, "lr")
    monkeypatch.delenv("DVBS2HIP_LR", raising=False)
    monkeypatch.setenv("DVBS2HIP_LR_TIMEOUT_US", "0")
    rx = Rx(modcod, max_frames=len(f_rows))
    rx.sync_lr_set_alpha(0.0)
    FRQ, PHS, Y = rx.sync_lr_synchronize(X)
    n_rep = rx.sync_lr_timeouts()
    print("fine_fp64 repaired call: %d repeats" % n_rep)
    _hold("L&R repaired", modcod, R.check_rows("lr", f_rows, X, FRQ, PHS, Y, **refs))
    assert n_rep != 0
    rx.close()


@pytest.mark.parametrize("modcod", ["QPSK-S_8/9", "8PSK-N_8/9"])
def test_freq_phase_on_8_byte_aligned_device_sockets(O, Rx, Yd, modcod):
    """sockets two floats into an allocation: sff_rotate_kernel (one sample per lane, flat index divided by n) instead of sff_rotate2_kernel
    -- the same bits, and both inside the float64 bars"""
    import torch
    from test_unaligned_gpu import _dev_pair
    X, f_rows, refs = R.table_refs(O, Yd, modcod, "fp")
    F = len(f_rows)
    out = []
    for shift in (0, 2):
        rx = Rx(modcod, max_frames=F)
        keep, d_x = _dev_pair(torch, np.array(X), shift)
        keep2, d_y = _dev_pair(torch, np.zeros_like(X), shift)
        assert (d_x.data_ptr() % 16 == 0) == (shift == 0) and (d_y.data_ptr() % 16 == 0) == (shift == 0)
        FRQ = torch.zeros(F, dtype=torch.float32, device="cuda"); PHS = torch.zeros_like(FRQ)
        torch.cuda.synchronize()
        rx._chk(rx.L.dvbs2hip_sync_freq_phase_synchronize_dev(rx.h, vp(d_x.data_ptr()), vp(FRQ.data_ptr()), vp(PHS.data_ptr()), vp(d_y.data_ptr()), F))
        rx.synchronize()
        out.append((FRQ.cpu().numpy(), PHS.cpu().numpy(), d_y.cpu().numpy().reshape(F, -1).copy()))
        _hold("freq_phase dev +%d B" % (4 * shift), modcod, R.check_rows("fp", f_rows, X, *out[-1], **refs))
        rx.close()
    assert _same_bits(out[0], out[1])


def test_lr_frame_that_is_not_a_number(O, Rx, monkeypatch):
    """an estimate that is not a number is published as the canonical NaN, never as the not-yet pattern the waiting workgroups of
    sff_lr_fused_kernel poll for (w0, w1): the frames from the bad one on come out as NaN, at once -- nothing waits, nothing is repeated --
    the frame before it is untouched, and a reset handle is clean again.  The bad sample carries the all-ones pattern itself."""
    modcod, F = "32APSK-S_3/4", 3
    clean = np.array(R.table_inputs(O, modcod, "lr")[:F])
    bad = clean.copy()
    bad.view(np.uint32)[1, 2 * (R.PILOT0 + 5)] = 0xFFFFFFFF
    assert np.isnan(bad[1]).sum() == 1 and not np.isnan(bad[[0, 2]]).any()
    out = {}
    for form in ("fused", "unfused"):
        _lr_form(monkeypatch, form)
        rx = Rx(modcod, max_frames=F)
        rx.sync_lr_set_alpha(0.5)
        ref = rx.sync_lr_synchronize(clean)
        assert not np.isnan(ref[0]).any() and not np.isnan(ref[2]).any()
        rx.sync_lr_reset()
        FRQ, PHS, Y = rx.sync_lr_synchronize(bad)
        assert _same_bits((FRQ[:1], Y[:1]), (ref[0][:1], ref[2][:1]))
        assert np.isnan(FRQ[1:]).all() and np.isnan(Y[1:]).all()
        assert rx.sync_lr_timeouts() == 0
        rx.sync_lr_reset()
        assert _same_bits(rx.sync_lr_synchronize(clean), ref)
        assert rx.sync_lr_timeouts() == 0
        out[form] = (ref, (FRQ, PHS, Y))
        rx.close()
    assert _same_bits(out["fused"][0], out["unfused"][0])
    for a, b in zip(out["fused"][1], out["unfused"][1]):
        assert np.array_equal(a, b, equal_nan=True)
