"""The fused front end (k_front.hip: front_launch, entered by every rx_bb* call) against its float64 twin, through the tap dvbs2hip_rx_front*.

Every kernel form is reached by its condition and named in the case's docstring; which form a call takes is decided on the host by front_choose
(dvbs2_amd/csrc/rx_dispatch.h) from the MODCOD, the frame count, two environment variables and the alignment of the PL and LLR sockets.  Each case asks
`plan_probe front` with its own facts and this process's knobs, requires the documented form and prints that name.  The bars are those of
tests/front_ref.py::judge, against the twin evaluated at the sigma the device itself reports in EST[:, 0], so the LLRs' scale and the estimate are
judged apart: no NaN of the sockets' fill left, EST = (sigma_in, 0, 0) bit for bit where sigma is given, |L - L64| <= 1e-4 max(1, |L64|) for every
LLR, the frame's rms normalized error within TIGHT_MARGIN of the oracle demapper's own on the same frame and sigma, and with the estimator sigma
within 1e-4 relative, Eb/N0 and Es/N0 within 2e-3 dB of the twin's M2M4.  tests/test_front_ref.py shows on the CPU that these bars reject eleven
mistakes such a kernel could make.  Measured figures per MODCOD and form: results/front_fp64/README.md (printed by every case before it asserts)."""
import numpy as np
import pytest

import front_ref as R
from helpers import chain

pytestmark = pytest.mark.gpu
GUARD = 64                       # floats of NaN in front of and behind each output socket, which have to stay


@pytest.fixture(scope="module")
def Rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    return Dvbs2Hip


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from test_plan_digest import build_probe
    exe = str(tmp_path_factory.mktemp("front_fp64") / "plan_probe")
    build_probe(exe)
    return exe


def _form(probe, modcod, F, want, **kw):
    """the form front_choose names for such a call, which has to be the documented one"""
    from test_rx_dispatch import front_form
    got = front_form(probe, modcod, F, **kw)
    assert got == want, (modcod, F, kw, got)
    return got


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tap(rx, pl, sigma, pl_off=0, llr_off=0, src=None):
    """dvbs2hip_rx_front_dev (src: dvbs2hip_rx_front_located_dev on that table) into NaN-filled sockets; pl_off / llr_off: floats the PL / LLR socket
    starts inside its 256-byte aligned allocation -> (LLR [F, N_ldpc], EST [F, 3])"""
    import torch
    F, N = (pl.shape[0] if src is None else src.numel()), rx.N_ldpc
    nan = float("nan")
    dl = torch.full((GUARD + llr_off + F * N + GUARD,), nan, dtype=torch.float32, device="cuda")
    de = torch.full((GUARD + 3 * F + GUARD,), nan, dtype=torch.float32, device="cuda")
    ds = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float32)).cuda() if sigma is not None else None
    lp, ep = dl.data_ptr() + 4 * (GUARD + llr_off), de.data_ptr() + 4 * GUARD
    if src is None:
        host = np.zeros(pl_off + pl.size, np.float32)
        host[pl_off:] = pl.ravel()
        dp = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        rx.rx_front_dev(dp.data_ptr() + 4 * pl_off, None if ds is None else ds.data_ptr(), lp, ep, F)
    else:
        torch.cuda.synchronize()
        rx.rx_front_located_dev(src.data_ptr(), None if ds is None else ds.data_ptr(), lp, ep, F)
    rx.synchronize()
    l, e = dl.cpu().numpy(), de.cpu().numpy()
    a, b = GUARD + llr_off, GUARD + llr_off + F * N
    assert np.isnan(l[:a]).all() and np.isnan(l[b:]).all() and np.isnan(e[:GUARD]).all() and np.isnan(e[GUARD + 3 * F:]).all(), "a write outside the sockets"
    return l[a:b].reshape(F, N).copy(), e[GUARD:GUARD + 3 * F].reshape(F, 3).copy()


def _judge(O, case, modcod, form, pl, LLR, EST, sigma, frames=None):
    """prints the figures, then asserts every bar"""
    mc = chain(O, modcod).mc
    rows = R.judge(mc, pl, LLR, EST, sigma, R.oracle_rms_of(O, modcod), frames)
    w = lambda k: max(r.get(k, 0.0) for r in rows)
    print("\nFRONT64 %s | %s | %s | %s | max_e %.3g rms_e %.3g oracle_rms %.3g ratio %.2f | sig %.3g eb %.3g es %.3g" % (
        case, modcod, form, "given" if sigma is not None else "estimated", w("max_e"), w("rms_e"), max(r.get("rms_oracle", 0.0) for r in rows),
        max((r.get("rms_e", 0.0) / r["rms_oracle"] for r in rows if r.get("rms_oracle")), default=0.0), w("sig_err"), w("eb_err"), w("es_err")))
    assert not R.broken(rows), (case, modcod, form, rows)
    return rows


def _both(O, case, modcod, form, rx, pl, sig, **kw):
    """a call with sigma given and one with the estimator, each under the bars -> the two (LLR, EST)"""
    out = []
    for s in (sig, None):
        LLR, EST = _tap(rx, pl, s, **kw)
        _judge(O, case, modcod, form, pl, LLR, EST, s)
        out.append((LLR, EST))
    return out


# ---------------------------------------------------------------------------------------------------------------- A
DOCUMENTED = {"QPSK-S_8/9": "front_reg2_kernel<4>", "QPSK-S_3/5": "front_reg2_kernel<4>", "QPSK-N_8/9": "front_reg2_kernel<16>",
                "8PSK-S_3/5": "front_reg_kernel<3, 8, false>", "8PSK-S_8/9": "front_reg_kernel<3, 8, false>", "8PSK-N_8/9": "front_reg_kernel<3, 22, false>",
                "16APSK-S_8/9": "front_kernel<4, true, true> sliced", "16APSK-N_8/9": "front_kernel<4, true, true> sliced", "32APSK-S_3/4": "front_kernel<5, true, true> sliced"}


@pytest.mark.parametrize("modcod", R.modcods())
def test_a_default_form_of_every_modcod(O, Rx, probe, modcod):
    """Three frames, 256-byte aligned sockets, no environment: QPSK takes front_reg2_kernel<4> (short) / <16> (normal: 16-byte aligned sockets, separable
    mapping, no interleaver), 8PSK front_reg_kernel<3, 8, false> (short: at most 8 symbols per lane) / <3, 22, false> (normal), 16APSK and 32APSK fall
    past the register-resident forms to the two-sweep front_kernel<4|5, true, true>, sliced over gridDim.y since 3 < 512 frames."""
    _, pl, _, sigma = R.frames(O, modcod)
    rx = Rx(modcod, max_frames=3)
    _both(O, "A", modcod, _form(probe, modcod, 3, DOCUMENTED[modcod]), rx, pl, R.sigmas(sigma, 3))
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("how", ["env_single", "pl_two_floats_in", "llr_two_floats_in"])
@pytest.mark.parametrize("modcod", ["QPSK-S_8/9", "QPSK-N_8/9"])
def test_b_qpsk_one_symbol_form_equals_the_pair_form(O, Rx, probe, monkeypatch, modcod, how):
    """front_reg_kernel<2, 8, true> (short) / <2, 32, true> (normal): the pair form is refused by DVBS2HIP_FRONT_SINGLE=1 (read at each call), by a PL socket
    two floats into its allocation, or by an LLR socket two floats in (either is then 8-byte aligned only).  With sigma given its LLRs equal the pair
    form's (front_reg2_kernel, the default) bit for bit; with the estimator the moments are summed in another order and only the bars apply."""
    _, pl, _, sigma = R.frames(O, modcod)
    sig = R.sigmas(sigma, 3)
    rx = Rx(modcod, max_frames=3)
    pair, _ = _tap(rx, pl, sig)
    if how == "env_single":
        monkeypatch.setenv("DVBS2HIP_FRONT_SINGLE", "1")
    kw = dict(pl_off=2) if how == "pl_two_floats_in" else dict(llr_off=2) if how == "llr_two_floats_in" else {}
    form = _form(probe, modcod, 3, "front_reg_kernel<2, %d, true>" % (8 if "-S" in modcod else 32), align_pl=8 if how == "pl_two_floats_in" else 16,
                 align_llr=8 if how == "llr_two_floats_in" else 16)
    (given, _), _ = _both(O, "B", modcod, "%s (%s)" % (form, how), rx, pl, sig, **kw)
    assert _same(given, pair)
    rx.close()


@pytest.mark.parametrize("modcod,form", [("QPSK-S_8/9", "front_reg_kernel<2, 8, false>"), ("QPSK-N_8/9", "front_kernel<2, true, true> sliced, general demapper")])
def test_b_qpsk_general_demapper(O, Rx, probe, monkeypatch, modcod, form):
    """DVBS2HIP_DEMAP_GENERAL=1 (read at create) leaves the mapping unmarked as separable: the short frame takes front_reg_kernel<2, 8, false> (log-sum-exp
    from the LDS table), the normal frame has no register-resident general form and falls to the two-sweep front_kernel<2, true, true>, sliced."""
    monkeypatch.setenv("DVBS2HIP_DEMAP_GENERAL", "1")
    _, pl, _, sigma = R.frames(O, modcod)
    rx = Rx(modcod, max_frames=3)
    _both(O, "B", modcod, _form(probe, modcod, 3, form.replace(", general demapper", ""), sep=0) + ", general demapper", rx, pl, R.sigmas(sigma, 3))
    rx.close()


@pytest.mark.parametrize("modcod", ["QPSK-S_8/9", "QPSK-N_8/9", "8PSK-S_3/5", "8PSK-S_8/9", "8PSK-N_8/9"])
def test_b_two_sweep_form_of_qpsk_and_8psk(O, Rx, probe, monkeypatch, modcod):
    """DVBS2HIP_FRONT_TWO_SWEEP=1 (read at each call) sends QPSK and 8PSK past the register-resident forms: front_kernel<2|3, true, true>, sliced (3 < 512 frames; 8PSK
    takes 1024 symbols per trip and slice, QPSK's linear form as well)."""
    monkeypatch.setenv("DVBS2HIP_FRONT_TWO_SWEEP", "1")
    _, pl, _, sigma = R.frames(O, modcod)
    rx = Rx(modcod, max_frames=3)
    form = _form(probe, modcod, 3, "front_kernel<%d, true, true> sliced" % chain(O, modcod).mc.bps)
    _both(O, "B", modcod, form + " (DVBS2HIP_FRONT_TWO_SWEEP)", rx, pl, R.sigmas(sigma, 3))
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("F", [1, 3, 300, 513])
@pytest.mark.parametrize("modcod", ["32APSK-S_3/4", "16APSK-S_8/9"])
def test_c_slicing_of_the_two_sweep_kernel(O, Rx, probe, modcod, F):
    """front_kernel<5|4, true, true>.  32APSK-S has 3240 symbols = 13 trips of 256 (the last with 168), 16APSK-S 4050 = 16 trips (the last with 210).
    F = 1: one frame, a slice per trip; F = 3: the same with three frames; F = 300: the cap of 1024 / 300 = 3 slices per frame (1280 / 1536 symbols
    each, the last shorter); F = 513: from 512 frames on unsliced, one workgroup walks the frame.  The frames are three distinct ones tiled with
    sigma cycling: every copy has to equal its first copy bit for bit, the first three are held to the twin."""
    _, pl3, _, sigma = R.frames(O, modcod)
    pl, sig = pl3[np.arange(F) % 3], R.sigmas(sigma, F)
    rx = Rx(modcod, max_frames=513)
    form = _form(probe, modcod, F, "front_kernel<%d, true, true>%s" % (chain(O, modcod).mc.bps, "" if F >= 512 else " sliced")) + (" unsliced" if F >= 512 else ", F = %d" % F)
    for s in (sig, None):
        LLR, EST = _tap(rx, pl, s)
        for f in range(3, F):
            assert _same(LLR[f], LLR[f % 3]) and _same(EST[f], EST[f % 3]), f
        _judge(O, "C", modcod, form, pl, LLR, EST, s, frames=range(min(F, 3)))
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- D
def test_d_located_form_equals_the_contiguous_call(O, Rx, probe):
    """The located variant of front_reg2_kernel<4> (QPSK-S), front_reg_kernel<3, 8, false> (8PSK-S) and the sliced front_kernel<5, true, true> (32APSK-S):
    frame f read at SRC[f].  The nine frames lie in one device stream in shuffled order with gaps of 1e30, every start at an odd complex-sample
    index, so 8-byte aligned only (the pair kernel reads a located frame through a buffer descriptor and keeps its form).  LLRs and EST equal the
    contiguous call's bit for bit, sigma given and estimated; a handle with set_streams(2) refuses the entry as rx_bb_located_dev does."""
    import torch
    modcods = ["QPSK-S_8/9", "8PSK-S_8/9", "32APSK-S_3/4"]
    rng = np.random.default_rng(7)
    inputs = {m: R.frames(O, m) for m in modcods}
    order = [(m, f) for m in modcods for f in range(3)]
    rng.shuffle(order)
    start, cur = {}, 1
    for m, f in order:
        start[m, f] = cur
        cur += inputs[m][1].shape[1] // 2 + 2 * int(rng.integers(0, 40)) + 2          # stays odd
    host = np.full(2 * cur, 1e30, np.float32)
    for (m, f), s in start.items():
        assert s % 2 == 1
        host[2 * s:2 * s + inputs[m][1].shape[1]] = inputs[m][1][f]
    stream = torch.from_numpy(host).cuda()
    assert stream.data_ptr() % 16 == 0
    for m in modcods:
        print("\nFRONT64 D | %s | %s, frames at 8-byte aligned starts" % (m, _form(probe, m, 3, DOCUMENTED[m], align_pl=8, located=True)))
        _, pl, _, sigma = inputs[m]
        sig = R.sigmas(sigma, 3)
        src = torch.tensor([stream.data_ptr() + 8 * start[m, f] for f in range(3)], dtype=torch.int64, device="cuda")
        rx = Rx(m, max_frames=3)
        for s in (sig, None):
            LLR, EST = _tap(rx, pl, s)
            LLRl, ESTl = _tap(rx, None, s, src=src)
            assert _same(LLRl, LLR) and _same(ESTl, EST), (m, s is None)
        rx.set_streams(2)
        dl, de = torch.zeros(3 * rx.N_ldpc, dtype=torch.float32, device="cuda"), torch.zeros(9, dtype=torch.float32, device="cuda")
        assert rx.L.dvbs2hip_rx_front_located_dev(rx.h, src.data_ptr(), None, dl.data_ptr(), de.data_ptr(), 2) == -4          # DVBS2HIP_EUNSUPPORTED
        rx.close()


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("modcod", R.HIGH_SNR["modcods"])
def test_e_high_llr_through_the_fused_entry(O, Rx, probe, modcod):
    """30 dB frames demapped with sigma 0.05, 0.1, 0.2: |LLR| up to several hundred.  front_reg_kernel<3, 8|22, false> (8PSK-S, 8PSK-N) and the sliced
    front_kernel<4|5, true, true> (16APSK-S, 32APSK-S), each through demap_symbols_s and, for the symbols whose weaker subset sums below 2^-100,
    demap_symbol_far.  The twin counts the symbols on either side of that threshold: both kinds are in the call.  Signs equal the sent code word."""
    mc = chain(O, modcod).mc
    H = R.HIGH_SNR
    _, pl, cw, _ = R.frames(O, modcod, 3, H["ebn0"], H["seed"])
    sig = np.array(H["sigmas"], np.float32)
    far = [int(R.far_symbols(R.xfec(pl[f], mc), sig[f], mc).sum()) for f in range(3)]
    print("\nFRONT64 E | %s | far-path symbols per frame %s of %d" % (modcod, far, mc.N_xfec))
    assert 0 < sum(far) < 3 * mc.N_xfec
    rx = Rx(modcod, max_frames=3)
    LLR, EST = _tap(rx, pl, sig)
    _judge(O, "E", modcod, _form(probe, modcod, 3, DOCUMENTED[modcod]) + ", far path", pl, LLR, EST, sig)
    assert np.array_equal((LLR < 0).astype(np.int32), cw)
    rx.close()


# ---------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("modcod,ebn0,given", [("QPSK-S_8/9", 3.9, False), ("16APSK-S_8/9", 7.4, True)])
def test_f_the_tap_shows_what_the_chain_consumes(O, Rx, modcod, ebn0, given):
    """24 frames near the waterfall, where a decoder's outcome hangs on its input: rx_bb once (front_reg2_kernel<4> with the estimator for QPSK-S, the sliced
    front_kernel<4, true, true> with sigma given for 16APSK-S, whose M2M4 estimate is biased), and separately the host form rx_front, then decode_siho,
    decode_hiho and bb_descramble on a handle with the same LDPC parameters.  Payload and both CWD flags equal frame for frame; some frames converge
    and some do not, so an LLR that differed would have shown."""
    F = 24
    info, pl, _, sigma = R.frames(O, modcod, F, ebn0, 61)
    s = np.full(F, sigma, np.float32) if given else None
    kw = dict(max_frames=F, n_ite=10, alpha=1.0, early_stop=True)
    rx = Rx(modcod, **kw)
    out, c0, c1 = rx.rx_bb(pl, sigma=s)
    rx.close()
    rx = Rx(modcod, **kw)
    LLR, EST = rx.rx_front(pl, sigma=s)
    V, cl = rx.decode_siho(LLR)
    W, cb = rx.decode_hiho(V)
    got = rx.bb_descramble(W)
    rx.close()
    print("\nFRONT64 F | %s | LDPC converged %d of %d, BCH code words %d, frames right %d" % (modcod, int((cl != 0).sum()), F, int((cb != 0).sum()), int((got == info).all(axis=1).sum())))
    assert np.array_equal(got, out) and np.array_equal(cl, c0) and np.array_equal(cb, c1)
    assert 0 < int((c0 != 0).sum()) < F
    ok = (out == info).all(axis=1)
    assert ok.any() and not ok.all()
