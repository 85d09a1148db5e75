"""dvbs2hip_pls_decode[_dev | _located_dev], dvbs2hip_pls_expected, dvbs2hip_pls_describe (dvbs2_amd/csrc/k_pls.hip, api_pls.hip) against the float64 maximum-likelihood
search of tests/test_pls_cpu.py.  The kernel adds in an order of its own, so nothing here is bit-exact with the reference; the bars on MET and ENE are first-order
rounding bounds: no input passes through more than 90 roundings on a serial path (about 16 on the kernel's trees) before the square root, u = 2^-24, and
256 u sum|r_k| has room for both."""
import ctypes as C

import numpy as np
import pytest

import test_pls_cpu as R
from dvbs2_amd.params import MODCODS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WAVES = 4                                                                            # frames per workgroup (PLS_WAVES of k_pls.hip)
SMALL = "32APSK-S_3/4"                                                               # the shortest PL frame of the table: 3402 symbols
EINVAL = -1


@pytest.fixture(scope="module")
def rx4096():
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(SMALL, max_frames=4096)
    yield rx
    rx.close()


def frames_of(hdr, n, rng=None):
    """complex[F, 90] headers -> float32[F, 2 n] PL frames (the payload: noise when rng is given, else zeros) and the headers as the float32 samples say them"""
    F = len(hdr)
    x = np.zeros((F, 2 * n), np.float32) if rng is None else rng.standard_normal((F, 2 * n)).astype(np.float32)
    x[:, 0:180:2], x[:, 1:180:2] = hdr.real, hdr.imag
    return x, x[:, 0:180:2].astype(np.float64) + 1j * x[:, 1:180:2].astype(np.float64)


def check_met_ene(r, MET, ENE, met64, what):
    """the bars of the module docstring, against float64 on the float32 samples"""
    ene64 = (np.abs(r) ** 2).sum(1)
    em, ee = np.abs(MET - met64), np.abs(ENE - ene64)
    bm, be = 256 * U * np.abs(r).sum(1), 128 * U * ene64
    print("%s: max |MET - float64| / bar = %.3f, max |ENE - float64| / bar = %.3f" % (what, (em / bm).max(), (ee / be).max()))
    assert (em <= bm).all() and (ee <= be).all()


def noisy(rng, F, esn0_db, nu=0.0):
    """F headers of uniformly drawn values and phases, Es = 1, at Es/N0, turning by nu cycles per symbol -> (values, complex[F, 90])"""
    idx = rng.integers(0, 256, F)
    sig = np.sqrt(10 ** (-esn0_db / 10) / 2)
    ph = np.exp(1j * (rng.uniform(0, 2 * np.pi, F)[:, None] + 2 * np.pi * nu * np.arange(90)[None, :]))
    return idx, R.HEADERS[idx] * ph + sig * (rng.standard_normal((F, 90)) + 1j * rng.standard_normal((F, 90)))


def test_every_code_word_at_three_amplitudes_and_four_phases(rx4096):
    amp = np.repeat([0.5, 1.0, 3.0], 256)
    V = np.tile(np.arange(256), 3)
    phase = 0.1 + ((V + np.repeat([0, 1, 2], 256)) % 4) * np.pi / 2                 # 0.1 + k pi/2, three of the four per value: none a multiple of pi/4
    x, r = frames_of(R.HEADERS[V] * (amp * np.exp(1j * phase))[:, None], rx4096.pl_frame)
    PLS, MET, ENE = rx4096.pls_decode(x)
    assert np.array_equal(PLS, V)
    sum_r = np.abs(r).sum(1)
    em, ee = np.abs(MET - 90 * amp), np.abs(ENE - 90 * amp ** 2)
    print("noiseless: max |MET - 90 a| / bar = %.3f, max |ENE - 90 a^2| / bar = %.3f" % ((em / (256 * U * sum_r)).max(), (ee / (128 * U * ENE)).max()))
    assert (em <= 256 * U * sum_r).all() and (ee <= 128 * U * ENE).all()


def test_equal_to_the_float64_ml_decoder_at_minus_6_db(rx4096):
    _, h = noisy(np.random.default_rng(20261), 4096, -6.0)
    x, r = frames_of(h, rx4096.pl_frame)
    V64, met64, m = R.ml_decode(r)
    srt = np.sort(m, 1)
    margin = (srt[:, -1] - srt[:, -2]) / srt[:, -1]
    clear = margin >= 1e-4
    print("-6 dB: smallest relative margin %.3g, %d frames under 1e-4" % (margin.min(), (~clear).sum()))
    assert (~clear).sum() <= 4
    PLS, MET, ENE = rx4096.pls_decode(x)
    assert np.array_equal(PLS[clear], V64[clear])
    check_met_ene(r, MET, ENE, met64, "-6 dB")


def test_no_error_where_a_receiver_works_minus_2_db(rx4096):
    idx, h = noisy(np.random.default_rng(20262), 4096, -2.0)
    x, r = frames_of(h, rx4096.pl_frame)
    assert np.array_equal(R.ml_decode(r)[0], idx)                                    # the float64 decoder first
    assert np.array_equal(rx4096.pls_decode(x)[0], idx)


def test_residual_carrier_of_1e_3_cycles_per_symbol_at_0_db(rx4096):
    idx, h = noisy(np.random.default_rng(20263), 4096, 0.0, nu=1e-3)                 # twice what L&R is documented to take
    x, r = frames_of(h, rx4096.pl_frame)
    assert np.array_equal(R.ml_decode(r)[0], idx)
    assert np.array_equal(rx4096.pls_decode(x)[0], idx)


@pytest.mark.parametrize("modcod", ["QPSK-S_8/9", SMALL, "QPSK-N_8/9"])             # pl_frame 8370, 3402, 33282
def test_frame_counts_around_a_workgroup_and_the_three_forms(modcod):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(modcod, max_frames=257)
    n = rx.pl_frame
    assert n == {"QPSK-S_8/9": 8370, SMALL: 3402, "QPSK-N_8/9": 33282}[modcod]
    rng = np.random.default_rng(n)
    idx, h = noisy(rng, 257, 3.0)
    x, r = frames_of(h, n, rng)                                                      # a payload that is not zero: a read past the header would show
    one = [rx.pls_decode(x[f]) for f in range(257)]                                  # one frame per call
    PLS1, MET1, ENE1 = (np.concatenate([o[k] for o in one]) for k in range(3))
    assert np.array_equal(PLS1, idx)
    check_met_ene(r, MET1, ENE1, R.ml_decode(r)[1], modcod)
    xd = torch.from_numpy(x).cuda()
    for F in (1, WAVES - 1, WAVES + 1, 257):
        PLS, MET, ENE = rx.pls_decode(x[:F])
        assert np.array_equal(PLS, PLS1[:F]) and np.array_equal(MET, MET1[:F]) and np.array_equal(ENE, ENE1[:F]), F
        # MET / ENE NULL, host form
        P0 = np.full(F, -1, np.int32)
        rx._chk(rx.L.dvbs2hip_pls_decode(rx.h, x[:F].ctypes.data_as(C.c_void_p), P0.ctypes.data_as(C.c_void_p), None, None, F))
        assert np.array_equal(P0, PLS1[:F])
        # device form, with and without MET / ENE
        Pd = torch.full((2, F), -1, dtype=torch.int32, device="cuda"); Md = torch.full((F,), -1.0, dtype=torch.float32, device="cuda"); Ed = Md.clone()
        torch.cuda.synchronize()
        rx.pls_decode_dev(xd.data_ptr(), Pd[0].data_ptr(), Md.data_ptr(), Ed.data_ptr(), F)
        rx.pls_decode_dev(xd.data_ptr(), Pd[1].data_ptr(), None, None, F)
        rx.synchronize()
        assert np.array_equal(Pd[0].cpu().numpy(), PLS1[:F]) and np.array_equal(Pd[1].cpu().numpy(), PLS1[:F])
        assert np.array_equal(Md.cpu().numpy(), MET1[:F]) and np.array_equal(Ed.cpu().numpy(), ENE1[:F])
    rx.close()


def test_located_form_on_8_byte_aligned_frames_in_shuffled_order(rx4096):
    import torch
    rx, n, F = rx4096, rx4096.pl_frame, 37
    rng = np.random.default_rng(5)
    idx, h = noisy(rng, F, 0.0)
    x, _ = frames_of(h, n, rng)
    # frame k of the buffer starts 2 k + 1 complex samples behind k (n + 16) complex samples: an odd complex offset, 8-byte aligned and not 16
    buf = torch.from_numpy(rng.standard_normal(2 * (F * (n + 16) + 2 * F + 1)).astype(np.float32)).cuda()
    assert buf.data_ptr() % 16 == 0
    order = rng.permutation(F)
    off = np.array([k * (n + 16) + 2 * k + 1 for k in range(F)])                     # complex samples; place k holds frame order[k]
    for k in range(F):
        buf[2 * off[k]:2 * (off[k] + n)] = torch.from_numpy(x[order[k]]).cuda()
    table = buf.data_ptr() + 8 * off[np.argsort(order)]                              # SRC[f]: where frame f is
    assert (table % 16 == 8).all()
    SRC = torch.from_numpy(table.astype(np.int64)).cuda()
    xd = torch.from_numpy(x).cuda()                                                  # the gathered copy
    out = []
    for form in ("plain", "located"):
        Pd = torch.full((F,), -1, dtype=torch.int32, device="cuda"); Md = torch.full((F,), -1.0, dtype=torch.float32, device="cuda"); Ed = Md.clone()
        torch.cuda.synchronize()
        if form == "plain":
            rx.pls_decode_dev(xd.data_ptr(), Pd.data_ptr(), Md.data_ptr(), Ed.data_ptr(), F)
        else:
            rx.pls_decode_located_dev(SRC.data_ptr(), Pd.data_ptr(), Md.data_ptr(), Ed.data_ptr(), F)
        rx.synchronize()
        out.append((Pd.cpu().numpy(), Md.cpu().numpy(), Ed.cpu().numpy()))
    assert np.array_equal(out[0][0], idx)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def describe(L, value):
    name, pil = C.create_string_buffer(32), C.c_int32(-1)
    rc = L.dvbs2hip_pls_describe(value, name, 32, C.byref(pil))
    return rc, name.value.decode(), pil.value


@pytest.mark.parametrize("modcod", list(MODCODS))
def test_through_the_librarys_own_framer(modcod):
    from dvbs2_amd import params as P
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(modcod, max_frames=2)
    sym = np.random.default_rng(1).standard_normal((2, 2 * rx.N_xfec)).astype(np.float32)
    pl = rx.framer_generate(sym)
    want = rx.pls_expected()
    assert want == P.pls_value(P.get_modcod(modcod))
    PLS, MET, ENE = rx.pls_decode(pl)
    assert (PLS == want).all() and np.allclose(MET, 90.0, atol=1e-3) and np.allclose(ENE, 90.0, atol=1e-3)
    assert (rx.pls_decode(rx.pl_scramble(pl))[0] == want).all()                     # the PL scrambler copies the header through
    assert describe(rx.L, want) == (0, modcod, 1) and describe(rx.L, want - 1) == (0, modcod, 0)
    assert P.pls_name(want) == (modcod, True)
    rx.close()


def test_errors_leave_the_handle_usable():
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip(SMALL, max_frames=3)
    x, _ = frames_of(R.HEADERS[[43, 23, 200]], rx.pl_frame)
    PLS = np.zeros(4, np.int32)
    xp, pp = x.ctypes.data_as(C.c_void_p), PLS.ctypes.data_as(C.c_void_p)
    for fn in (rx.L.dvbs2hip_pls_decode, rx.L.dvbs2hip_pls_decode_dev, rx.L.dvbs2hip_pls_decode_located_dev):
        assert fn(rx.h, xp, pp, None, None, 0) == EINVAL and b"n_frames" in rx.L.dvbs2hip_last_error(rx.h)
        assert fn(rx.h, xp, pp, None, None, 4) == EINVAL and b"max_frames" in rx.L.dvbs2hip_last_error(rx.h)
        assert fn(rx.h, xp, None, None, None, 3) == EINVAL and b"null" in rx.L.dvbs2hip_last_error(rx.h)
        assert fn(rx.h, None, pp, None, None, 3) == EINVAL
        assert fn(None, xp, pp, None, None, 3) == EINVAL
    assert describe(rx.L, 256)[0] == EINVAL and describe(rx.L, -1)[0] == EINVAL
    assert describe(rx.L, 2) == (0, "", 0) and describe(rx.L, 128 + 43) == (0, "", 1)      # no row of the table: the empty name, and no error
    assert rx.L.dvbs2hip_pls_expected(rx.h, None) == EINVAL
    assert np.array_equal(rx.pls_decode(x)[0], [43, 23, 200])
    rx.close()


def test_a_recorded_decode_replays_on_new_input():
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    F = 9
    rx = Dvbs2Hip(SMALL, max_frames=F)
    rng = np.random.default_rng(9)
    xd = torch.zeros((F, 2 * rx.pl_frame), dtype=torch.float32, device="cuda")
    Pd = torch.full((F,), -1, dtype=torch.int32, device="cuda"); Md = torch.full((F,), -1.0, dtype=torch.float32, device="cuda"); Ed = Md.clone()
    torch.cuda.synchronize()

    def once():
        rx.pls_decode_dev(xd.data_ptr(), Pd.data_ptr(), Md.data_ptr(), Ed.data_ptr(), F)

    once(); rx.synchronize()
    gid = rx.graph_capture(once)
    for _ in range(2):
        idx, h = noisy(rng, F, 0.0)
        xd.copy_(torch.from_numpy(frames_of(h, rx.pl_frame)[0])); torch.cuda.synchronize()
        once(); rx.synchronize()
        want = (Pd.clone(), Md.clone(), Ed.clone())
        Pd.fill_(-1); Md.fill_(-1.0); Ed.fill_(-1.0); torch.cuda.synchronize()
        rx.graph_launch(gid); rx.synchronize()
        assert torch.equal(Pd, want[0]) and torch.equal(Md, want[1]) and torch.equal(Ed, want[2])
        assert np.array_equal(Pd.cpu().numpy(), idx)
    rx.graph_destroy(gid)
    rx.close()
