"""dvbs2hip_pls_scan[_dev] and dvbs2hip_pls_search[_dev] (dvbs2_amd/csrc/k_pls_search.hip, api_pls_search.hip).

The scan is held to the existing decoder, bit for bit: dvbs2hip_pls_decode_located_dev over a table of all offsets of the same device buffer (that decoder is held to
float64 by tests/test_pls_gpu.py).  The search is held to the fp32 chain twin of tests/pls_search_ref.py on the device's own scan output, bit for bit, and to the float64
twin end to end at the project's bar, 1e-4 max(1, SCORE): both fp32 factors of q carry at most the decoder's 256 u relative error, q <= 1, and a chain here has two
slots."""
import ctypes as C

import numpy as np
import pytest

import pls_search_ref as R

pytestmark = pytest.mark.gpu

SMALL = "32APSK-S_3/4"                                                               # the shortest PL frame of the table: 3402 symbols
N = 3402
BIG = 2 * N + 90
SIZES = [90, 153, 154, 90 + 255, 90 + 256, BIG]                                      # one offset; 64 and 65 (a workgroup's offsets and one more); 256 and 257; two frames and a header
EINVAL = -1
LIMIT = 1 << 24                                                                      # DVBS2HIP_PLS_SCAN_MAX_SYM


@pytest.fixture(scope="module")
def rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    h = Dvbs2Hip(SMALL, max_frames=BIG - 89)
    yield h
    h.close()


@pytest.fixture(scope="module")
def buffers(rx):
    """BIG symbols each: noise, the noiseless output of the library's framer, the same at -2 dB"""
    rng = np.random.default_rng(2026)
    pl = rx.framer_generate(rng.standard_normal((3, 2 * rx.N_xfec)).astype(np.float32) * np.float32(np.sqrt(0.5))).reshape(-1)[:2 * BIG]
    sig = np.sqrt(10 ** 0.2 / 2)
    out = dict(noise=rng.standard_normal(2 * BIG).astype(np.float32), framer=np.ascontiguousarray(pl), minus2=(pl + sig * rng.standard_normal(2 * BIG)).astype(np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def outputs(K, pad=64):
    """PLS, MET, ENE with `pad` elements behind the K the call may write"""
    import torch
    return (torch.full((K + pad,), -7, dtype=torch.int32, device="cuda"), torch.full((K + pad,), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((K + pad,), -7.0, dtype=torch.float32, device="cuda"))


def located(rx, ptr, n_sym):
    """the existing decoder on a frame at every offset of the device buffer at ptr -> numpy (PLS, MET, ENE)"""
    import torch
    K = n_sym - 89
    SRC = torch.from_numpy(ptr + 8 * np.arange(K, dtype=np.int64)).cuda()
    o = outputs(K, 0)
    torch.cuda.synchronize()
    rx.pls_decode_located_dev(SRC.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), K)
    rx.synchronize()
    return tuple(t.cpu().numpy() for t in o)


def scan_dev(rx, ptr, n_sym, met=True, ene=True):
    import torch
    K = n_sym - 89
    o = outputs(K)
    torch.cuda.synchronize()
    rx.pls_scan_dev(ptr, n_sym, o[0].data_ptr(), o[1].data_ptr() if met else None, o[2].data_ptr() if ene else None)
    rx.synchronize()
    got = tuple(t.cpu().numpy() for t in o)
    for g in got:
        assert (g[K:] == -7).all()                                                   # nothing written past the K offsets
    return tuple(g[:K] for g in got)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def search_dev(rx, ptr, n_sym, LEN=None):
    import torch
    RES = torch.full((4,), -9, dtype=torch.int32, device="cuda"); SCORE = torch.full((1,), -9.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rx.pls_search_dev(ptr, n_sym, LEN, RES.data_ptr(), SCORE.data_ptr())
    rx.synchronize()
    return RES.cpu().numpy(), SCORE.cpu().numpy()[0]


@pytest.mark.parametrize("kind", ["noise", "framer", "minus2"])
def test_scan_equals_the_located_decoder_at_every_offset_bit_for_bit(rx, buffers, kind):
    xd = dev(buffers[kind])
    assert xd.data_ptr() % 16 == 0
    want = located(rx, xd.data_ptr(), BIG)
    if kind == "framer":
        assert want[0][0] == want[0][N] == want[0][2 * N] == rx.pls_expected()
    for n_sym in SIZES:
        got = scan_dev(rx, xd.data_ptr(), n_sym)
        assert same_bits(got, tuple(w[:n_sym - 89] for w in want)), (kind, n_sym)
    # X one complex sample past a 16-byte boundary: 8-byte aligned and no more
    for n_sym in (90, 154, BIG - 1):
        got = scan_dev(rx, xd.data_ptr() + 8, n_sym)
        assert same_bits(got, tuple(w[1:1 + n_sym - 89] for w in want)), (kind, n_sym, "odd sample")


def test_scan_without_met_and_ene_leaves_pls_unchanged(rx, buffers):
    xd = dev(buffers["minus2"])
    full = scan_dev(rx, xd.data_ptr(), BIG)
    for met, ene in ((False, False), (True, False), (False, True)):
        got = scan_dev(rx, xd.data_ptr(), BIG, met, ene)
        assert np.array_equal(got[0], full[0])
        assert same_bits(got[1:2], full[1:2]) if met else (got[1] == -7).all()
        assert same_bits(got[2:3], full[2:3]) if ene else (got[2] == -7).all()


def test_scan_of_2_to_the_20_symbols(rx):
    """the size the header promises at least: a sample of its offsets against the located decoder"""
    import torch
    n_sym = 1 << 20
    K = n_sym - 89
    rng = np.random.default_rng(20)
    xd = dev(rng.standard_normal(2 * n_sym).astype(np.float32))
    got = scan_dev(rx, xd.data_ptr(), n_sym)
    pick = np.unique(np.concatenate([np.arange(130), np.arange(K - 130, K), rng.integers(0, K, 4096)])).astype(np.int64)
    SRC = torch.from_numpy(xd.data_ptr() + 8 * pick).cuda()
    o = outputs(len(pick), 0)
    torch.cuda.synchronize()
    rx.pls_decode_located_dev(SRC.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), len(pick))
    rx.synchronize()
    assert same_bits(tuple(g[pick] for g in got), tuple(t.cpu().numpy() for t in o))


@pytest.mark.parametrize("kind", ["noise", "framer", "minus2"])
def test_search_equals_the_fp32_chain_twin_on_the_devices_own_scan(rx, P, buffers, kind):
    xd = dev(buffers[kind])
    for n_sym in (90, 154, N + 500, BIG):
        scan = scan_dev(rx, xd.data_ptr(), n_sym)
        want_res, want_score = R.chain(*scan, P.PLS_FRAME_SYMBOLS, np.float32)
        res, score = search_dev(rx, xd.data_ptr(), n_sym)
        assert np.array_equal(res, want_res), (kind, n_sym, res, want_res)
        assert np.float32(score).view(np.int32) == np.float32(want_score).view(np.int32), (kind, n_sym, score, want_score)
    if kind != "noise":
        assert res.tolist()[:2] == [0, rx.pls_expected()] and res.tolist()[2:] == [3, 3]
        assert P.find_modcod(res, score)[0].name == SMALL


@pytest.fixture(scope="module")
def errors():
    worst = dict(err=0.0)
    yield worst
    print("largest |SCORE - float64| / max(1, SCORE) over the short-frame buffers: %.3g" % worst["err"])


@pytest.mark.parametrize("modcod", R.SHORT)
def test_search_against_the_float64_twin_on_the_short_frame_buffers(rx, O, P, modcod, errors):
    b = R.short_frame_buffer(O, P, modcod)
    x = b["x"]
    xd = dev(x)
    res, score = search_dev(rx, xd.data_ptr(), len(x) // 2)
    err = abs(float(score) - float(b["score"])) / max(1.0, float(score))
    errors["err"] = max(errors["err"], err)
    print("%s: RES %s, SCORE %.6f, float64 %.6f, error / bar %.3g" % (modcod, res.tolist(), score, b["score"], err / 1e-4))
    assert res.tolist() == b["res"].tolist() == [b["offset"], b["value"], 2, 2]
    assert err <= 1e-4
    # the host forms equal the device forms
    hres, hscore = rx.pls_search(x)
    assert np.array_equal(hres, res) and np.float32(hscore) == np.float32(score)
    assert same_bits(rx.pls_scan(x), scan_dev(rx, xd.data_ptr(), len(x) // 2))
    found = P.find_modcod(hres, hscore)
    assert found[0].name == modcod and found[2] == b["offset"]


def test_a_callers_len_with_a_single_candidate(rx, O, P):
    b = R.short_frame_buffer(O, P, "8PSK-S_3/5")
    x, n_sym = b["x"], len(b["x"]) // 2
    xd = dev(x)
    scan = scan_dev(rx, xd.data_ptr(), n_sym)
    own = np.zeros(256, np.int32); own[b["value"]] = b["mc"].pl_frame                # the stream's own value alone: what the library's table finds
    other = np.zeros(256, np.int32); other[43] = 1000; other[b["value"]] = 89        # another value at a length of the caller's; the stream's own below 90: no candidate
    for LEN in (own, other):
        want_res, want_score = R.chain(*scan, LEN, np.float32)
        res, score = search_dev(rx, xd.data_ptr(), n_sym, dev(LEN).data_ptr())
        hres, hscore = rx.pls_search(x, LEN)
        assert np.array_equal(res, want_res) and np.array_equal(hres, want_res) and np.float32(score) == np.float32(hscore) == want_score
    assert res[1] in (43, 0)
    assert np.array_equal(search_dev(rx, xd.data_ptr(), n_sym, dev(own).data_ptr())[0], b["res"])
    res, score = search_dev(rx, xd.data_ptr(), n_sym, dev(np.zeros(256, np.int32)).data_ptr())
    assert res.tolist() == [-1, 0, 0, 0] and score == 0


def test_one_header_only_is_found_and_not_believed(rx, P):
    rng = np.random.default_rng(11)
    n_sym = N + 500
    x = rng.standard_normal(2 * n_sym).astype(np.float32) * np.float32(np.sqrt(0.5))
    h = R.HEADERS[rx.pls_expected()] * np.exp(0.3j)
    x[200:380:2], x[201:380:2] = h.real, h.imag                                      # a header at symbol 100; symbol 100 + 3402 is a slot, and holds noise
    res, score = rx.pls_search(x)
    want_res, want_score = R.chain(*rx.pls_scan(x), P.PLS_FRAME_SYMBOLS, np.float32)
    assert np.array_equal(res, want_res) and np.float32(score) == want_score
    assert res.tolist() == [100, rx.pls_expected(), 1, 2] and score > 0.99
    assert P.find_modcod(res, score) is None


def test_a_noise_only_buffer_is_rejected(rx, P, buffers):
    res, score = rx.pls_search(buffers["noise"])
    print("noise: RES %s, SCORE %.4f" % (res.tolist(), score))
    assert P.find_modcod(res, score) is None


def test_errors_leave_the_handle_usable(rx, buffers):
    x = buffers["framer"]
    xp = x.ctypes.data_as(C.c_void_p)
    out, res, sc = np.zeros(BIG, np.int32), np.zeros(4, np.int32), np.zeros(1, np.float32)
    op, rp, sp = (a.ctypes.data_as(C.c_void_p) for a in (out, res, sc))
    L = rx.L
    for n_sym in (89, 0, -1, LIMIT + 1):
        for fn in (L.dvbs2hip_pls_scan, L.dvbs2hip_pls_scan_dev):
            assert fn(rx.h, xp, n_sym, op, None, None) == EINVAL and b"n_sym" in L.dvbs2hip_last_error(rx.h)
        for fn in (L.dvbs2hip_pls_search, L.dvbs2hip_pls_search_dev):
            assert fn(rx.h, xp, n_sym, None, rp, sp) == EINVAL and b"n_sym" in L.dvbs2hip_last_error(rx.h)
    for fn in (L.dvbs2hip_pls_scan, L.dvbs2hip_pls_scan_dev):
        assert fn(rx.h, None, 90, op, None, None) == EINVAL and b"null" in L.dvbs2hip_last_error(rx.h)
        assert fn(rx.h, xp, 90, None, None, None) == EINVAL
        assert fn(None, xp, 90, op, None, None) == EINVAL
    for fn in (L.dvbs2hip_pls_search, L.dvbs2hip_pls_search_dev):
        assert fn(rx.h, xp, 90, None, None, sp) == EINVAL and b"null" in L.dvbs2hip_last_error(rx.h)
        assert fn(rx.h, xp, 90, None, rp, None) == EINVAL
        assert fn(None, xp, 90, None, rp, sp) == EINVAL
    assert L.dvbs2hip_pls_scan_dev(rx.h, C.c_void_p(xp.value + 4), 90, op, None, None) == EINVAL and b"aligned" in L.dvbs2hip_last_error(rx.h)
    res, score = rx.pls_search(x)
    assert res.tolist() == [0, rx.pls_expected(), 3, 3]


def test_a_recorded_search_replays_on_new_input(O, P):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip("QPSK-S_8/9", max_frames=1)                                        # the handle's MODCOD and max_frames do not enter
    bufs = [R.short_frame_buffer(O, P, m) for m in ("32APSK-S_3/4", "16APSK-S_8/9")]
    n_sym = min(len(b["x"]) // 2 for b in bufs)
    xd = torch.zeros(2 * n_sym, dtype=torch.float32, device="cuda")
    RES = torch.full((4,), -9, dtype=torch.int32, device="cuda"); SCORE = torch.full((1,), -9.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def once():
        rx.pls_search_dev(xd.data_ptr(), n_sym, None, RES.data_ptr(), SCORE.data_ptr())

    once(); rx.synchronize()                                                         # allocates the workspace and uploads the table
    assert RES.cpu().numpy().tolist() == [-1, 0, 0, 0] or RES.cpu().numpy()[0] >= 0
    gid = rx.graph_capture(once)
    for b in bufs:
        xd.copy_(torch.from_numpy(b["x"][:2 * n_sym].copy())); torch.cuda.synchronize()
        once(); rx.synchronize()
        want = (RES.clone(), SCORE.clone())
        RES.fill_(-9); SCORE.fill_(-9.0); torch.cuda.synchronize()
        rx.graph_launch(gid); rx.synchronize()
        assert torch.equal(RES, want[0]) and torch.equal(SCORE, want[1])
        assert RES.cpu().numpy().tolist()[:2] == [b["offset"], b["value"]]
    rx.graph_destroy(gid)
    rx.close()
