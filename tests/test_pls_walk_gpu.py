"""dvbs2hip_pls_walk[_dev] (dvbs2_amd/csrc/k_pls_walk.hip, api_pls_walk.hip) against the twin of tests/pls_walk_ref.py.

The buffer is the library's own transmitter's: 37 symbols of noise, then QPSK-S_8/9, 32APSK-S_3/4 twice, 16APSK-S_8/9, a dummy frame (the header of value 0 from the twin's
generator), 8PSK-S_3/5, one QPSK-N_8/9 (a hop of 33282 symbols), QPSK-S_3/5, and the first 2000 symbols of a ninth frame.  The walk is integers behind the PLS decoder, so
on the device's own decoder outputs at the candidates it has to equal the twin exactly, Q by bit pattern; end to end it is held to the float64 decoder at the search
test's bar for q, 1e-4.  The library resolves a chain of few levels with one lane and a longer one by pointer doubling (pls_walk_choose of rx_dispatch.h, PLSW_LANE_LEVELS = 5 levels, so
max_out 31 against 32 with a caller's table): MAX_OUT below takes every case through both."""
import ctypes as C

import numpy as np
import pytest

import pls_walk_ref as W

pytestmark = pytest.mark.gpu

LEAD = 37
ORDER = ["QPSK-S_8/9", "32APSK-S_3/4", "32APSK-S_3/4", "16APSK-S_8/9", None, "8PSK-S_3/5", "QPSK-N_8/9", "QPSK-S_3/5"]      # None: the dummy frame
NINTH = 2000
MAX_OUT = [8, 31, 32, 4096]                                                          # 4, 5 (one lane), 6 and 10 levels (pointer doubling)
EINVAL = -1
FMAX = 4096                                                                          # frames per call of the located decoder that makes the twin's input


@pytest.fixture(scope="module")
def rx():
    from dvbs2_amd.receiver import Dvbs2Hip
    h = Dvbs2Hip("QPSK-S_8/9", max_frames=FMAX)                                      # neither the MODCOD nor max_frames enters the walk
    yield h
    h.close()


@pytest.fixture(scope="module")
def stream(P):
    """dict(x float32[2 n_sym] not to be written to, off: the nine headers' symbols, val: the eight frames' values, n_sym)"""
    from dvbs2_amd.receiver import Dvbs2Hip
    rng = np.random.default_rng(77)
    made = {}
    for i, name in enumerate(sorted({m for m in ORDER if m})):
        h = Dvbs2Hip(name, max_frames=3)
        made[name] = list(h.tx_bb(3, seed=100 + i)[1])
        h.close()
    parts, off, val, c = [(rng.standard_normal(2 * LEAD) * np.sqrt(0.5)).astype(np.float32)], [], [], LEAD
    for name in ORDER:
        f = W.dummy(rng) if name is None else made[name].pop()
        parts.append(f); off.append(c); val.append(0 if name is None else P.pls_value(P.get_modcod(name)))
        c += f.size // 2
    off.append(c)
    parts.append(made["QPSK-S_8/9"].pop()[:2 * NINTH])
    x = np.concatenate(parts)
    x.setflags(write=False)
    assert x.size // 2 == c + NINTH and [b - a for a, b in zip(off, off[1:])] == [8370, 3402, 3402, 4212, 3330, 5598, 33282, 8370]
    return dict(x=x, off=off, val=val, n_sym=x.size // 2)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def walk_dev(rx, ptr, n_sym, start, LEN, q_min, max_out, pad=8):
    """-> dict of numpy outputs cut to N (SRC as byte offsets from X); nothing may be written past the max_out entries"""
    import torch
    n = min(max_out, 1 << 16)                                                        # (no buffer here holds that many frames)
    i32 = lambda k, v=-7: torch.full((k,), v, dtype=torch.int32, device="cuda")
    OFF, VAL, IDX, CNT, RES = i32(n + pad), i32(n + pad), i32(n + pad), i32(256 + pad), i32(4 + pad)
    Q = torch.full((n + pad,), -7.0, dtype=torch.float32, device="cuda")
    SRC = torch.full((n + pad,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rx.pls_walk_dev(ptr, n_sym, start, LEN, q_min, max_out, OFF.data_ptr(), VAL.data_ptr(), Q.data_ptr(), SRC.data_ptr(), IDX.data_ptr(), CNT.data_ptr(), RES.data_ptr())
    rx.synchronize()
    o = dict(OFF=OFF, VAL=VAL, Q=Q, SRC=SRC, IDX=IDX, CNT=CNT, RES=RES)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    N = int(o["RES"][0])
    assert 0 <= N <= n and o["RES"][3] == 0
    for k, size in (("OFF", n), ("VAL", n), ("Q", n), ("SRC", n), ("IDX", n), ("CNT", 256), ("RES", 4)):
        assert (o[k][size:] == -7).all(), k
        assert (o[k][N:size] == -7).all() or k in ("CNT", "RES"), k                  # (entries past N are undefined; this implementation leaves them alone)
    out = {k: (o[k][:N] if k not in ("CNT", "RES") else o[k][:256 if k == "CNT" else 4]) for k in o}
    out["SRC"] = out["SRC"] - ptr
    return out


def candidates(rx, ptr, n_sym, start):
    """the device's own decoder at start + 18 i, every i with a whole header in front of n_sym -> numpy (PLS, MET, ENE)"""
    import torch
    M = (n_sym - 90 - start) // 18 + 1 if start + 90 <= n_sym else 0
    SRC = torch.from_numpy(ptr + 8 * (start + 18 * np.arange(M, dtype=np.int64))).cuda()
    o = (torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(M, dtype=torch.float32, device="cuda"), torch.zeros(M, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    for a in range(0, M, FMAX):
        rx.pls_decode_located_dev(SRC.data_ptr() + 8 * a, o[0].data_ptr() + 4 * a, o[1].data_ptr() + 4 * a, o[2].data_ptr() + 4 * a, min(FMAX, M - a))
    rx.synchronize()
    return tuple(t.cpu().numpy() for t in o)


def check_against_twin(got, want, what):
    OFF, VAL, Q, RES = want
    CNT, IDX = W.group(VAL)
    assert got["RES"].tolist() == RES.tolist(), (what, got["RES"], RES)
    for k, w in (("OFF", OFF), ("VAL", VAL), ("CNT", CNT), ("IDX", IDX)):
        assert np.array_equal(got[k], w), (what, k)
    assert np.array_equal(got["Q"].view(np.int32), np.asarray(Q, np.float32).view(np.int32)), what
    assert np.array_equal(got["SRC"], 8 * OFF[IDX].astype(np.int64)), what


def twin_on_device_headers(rx, P, xd, n_sym, start, LEN, q_min, max_out):
    return W.walk_candidates(*candidates(rx, xd.data_ptr(), n_sym, start), n_sym, start, P.VCM_FRAME_SYMBOLS if LEN is None else LEN, q_min, max_out)


@pytest.mark.parametrize("max_out", MAX_OUT)
def test_the_walk_equals_the_twin_on_the_devices_own_headers(rx, P, stream, max_out):
    xd, n_sym = dev(stream["x"]), stream["n_sym"]
    LEN = dev(P.VCM_FRAME_SYMBOLS)
    got = walk_dev(rx, xd.data_ptr(), n_sym, LEAD, LEN.data_ptr(), P.PLS_SEARCH_Q_MIN, max_out)
    check_against_twin(got, twin_on_device_headers(rx, P, xd, n_sym, LEAD, None, P.PLS_SEARCH_Q_MIN, max_out), max_out)
    assert got["OFF"].tolist() == stream["off"][:8] and got["VAL"].tolist() == stream["val"]
    assert got["RES"].tolist() == [8, stream["off"][8], W.END, 0]                    # the ninth header was seen, its frame is cut off
    assert got["CNT"][0] == 1 and got["CNT"][P.pls_value(P.get_modcod("32APSK-S_3/4"))] == 2 and got["CNT"].sum() == 8
    assert (got["Q"] > 0.99).all()
    # X 8-byte aligned and no more, and a start that is one frame on
    od = dev(np.concatenate([np.zeros(2, np.float32), stream["x"]]))
    odd = walk_dev(rx, od.data_ptr() + 8, n_sym, stream["off"][1], LEN.data_ptr(), P.PLS_SEARCH_Q_MIN, max_out)
    assert odd["OFF"].tolist() == stream["off"][1:8] and np.array_equal(odd["SRC"], 8 * odd["OFF"][odd["IDX"]].astype(np.int64))


@pytest.fixture(scope="module")
def noisy(P, stream):
    """the buffer under noise at Es/N0 = 10 dB, and the float64 twin's walk on it"""
    rng = np.random.default_rng(78)
    x = (stream["x"] + P.esn0_to_sigma(10.0) * rng.standard_normal(stream["x"].size)).astype(np.float32)
    x.setflags(write=False)
    return x, W.walk(W.header64(x), stream["n_sym"], LEAD, P.VCM_FRAME_SYMBOLS, P.PLS_SEARCH_Q_MIN, 4096)


@pytest.mark.parametrize("max_out", [31, 4096])
def test_the_walk_against_the_float64_decoder_at_10_dB(rx, P, stream, noisy, max_out):
    x, (OFF, VAL, Q, RES) = noisy
    xd, LEN = dev(x), dev(P.VCM_FRAME_SYMBOLS)
    got = walk_dev(rx, xd.data_ptr(), stream["n_sym"], LEAD, LEN.data_ptr(), P.PLS_SEARCH_Q_MIN, max_out)
    err = np.abs(got["Q"].astype(np.float64) - Q).max()
    print("Es/N0 10 dB: smallest Q %.4f (q_min %.4f), largest |Q - float64| %.3g" % (got["Q"].min(), P.PLS_SEARCH_Q_MIN, err))
    assert np.array_equal(got["OFF"], OFF) and np.array_equal(got["VAL"], VAL) and got["RES"].tolist() == RES.tolist()
    assert got["OFF"].tolist() == stream["off"][:8]
    assert err <= 1e-4
    assert (got["Q"] > P.PLS_SEARCH_Q_MIN).all()


@pytest.mark.parametrize("max_out", MAX_OUT)
def test_stop_reasons(rx, P, stream, max_out):
    x, off, val, n_sym = stream["x"], stream["off"], stream["val"], stream["n_sym"]
    q_min = P.PLS_SEARCH_Q_MIN
    LEN = dev(P.VCM_FRAME_SYMBOLS)
    xd = dev(x)
    n = min(max_out, 8)
    # frame 4's header is noise: LOST there
    y = x.copy()
    y[2 * off[3]:2 * (off[3] + 90)] = (np.random.default_rng(79).standard_normal(180) * np.sqrt(0.5)).astype(np.float32)
    yd = dev(y)
    got = walk_dev(rx, yd.data_ptr(), n_sym, LEAD, LEN.data_ptr(), q_min, max_out)
    check_against_twin(got, twin_on_device_headers(rx, P, yd, n_sym, LEAD, None, q_min, max_out), "noise header")
    assert got["RES"].tolist() == [3, off[3], W.LOST, 0]
    # the table has no length for frame 2's value: LOST at frame 2
    own = P.VCM_FRAME_SYMBOLS.copy(); own[val[1]] = 0
    od = dev(own)
    got = walk_dev(rx, xd.data_ptr(), n_sym, LEAD, od.data_ptr(), q_min, max_out)
    check_against_twin(got, twin_on_device_headers(rx, P, xd, n_sym, LEAD, own, q_min, max_out), "LEN = 0")
    assert got["RES"].tolist() == [1, off[1], W.LOST, 0]
    # the library's own table knows no dummy frame: LOST at frame 5 (with fewer levels than a caller's table asks for: its shortest frame is known)
    got = walk_dev(rx, xd.data_ptr(), n_sym, LEAD, None, q_min, max_out)
    check_against_twin(got, twin_on_device_headers(rx, P, xd, n_sym, LEAD, P.PLS_FRAME_SYMBOLS, q_min, max_out), "LEN = NULL")
    assert got["RES"].tolist() == ([4, off[4], W.LOST, 0] if max_out >= 4 else [max_out, off[max_out], W.FULL, 0])
    # a length that is no multiple of 18, and one below 90, count as 0
    for bad in (3403, 72):
        own = P.VCM_FRAME_SYMBOLS.copy(); own[val[1]] = bad
        od = dev(own)
        assert walk_dev(rx, xd.data_ptr(), n_sym, LEAD, od.data_ptr(), q_min, max_out)["RES"].tolist() == [1, off[1], W.LOST, 0]
    # FULL
    got = walk_dev(rx, xd.data_ptr(), n_sym, LEAD, LEN.data_ptr(), q_min, 3)
    check_against_twin(got, twin_on_device_headers(rx, P, xd, n_sym, LEAD, None, q_min, 3), "max_out = 3")
    assert got["RES"].tolist() == [3, off[3], W.FULL, 0] and got["CNT"].sum() == 3
    # the buffer ends 10 symbols into frame 3's header: END, by step 1
    cut = off[2] + 10
    got = walk_dev(rx, xd.data_ptr(), cut, LEAD, LEN.data_ptr(), q_min, max_out)
    check_against_twin(got, twin_on_device_headers(rx, P, xd, cut, LEAD, None, q_min, max_out), "cut header")
    assert got["RES"].tolist() == [2, off[2], W.END, 0]
    # and exactly at the end of frame 2: NEXT = n_sym
    assert walk_dev(rx, xd.data_ptr(), off[2], LEAD, LEN.data_ptr(), q_min, max_out)["RES"].tolist() == [2, off[2], W.END, 0]
    # q_min above every header: LOST at once; start = n_sym and a start with 89 symbols behind it: END at once
    assert walk_dev(rx, xd.data_ptr(), n_sym, LEAD, LEN.data_ptr(), 1.5, max_out)["RES"].tolist() == [0, LEAD, W.LOST, 0]
    for start in (n_sym, n_sym - 89):
        got = walk_dev(rx, xd.data_ptr(), n_sym, start, LEN.data_ptr(), q_min, max_out)
        assert got["RES"].tolist() == [0, start, W.END, 0] and got["CNT"].sum() == 0
    assert n == len(walk_dev(rx, xd.data_ptr(), n_sym, LEAD, LEN.data_ptr(), q_min, n)["OFF"])


def test_the_host_form_equals_the_device_form(rx, P, stream):
    x, n_sym = stream["x"], stream["n_sym"]
    xd = dev(x)
    for LEN, max_out, start in ((P.VCM_FRAME_SYMBOLS, 4096, LEAD), (P.VCM_FRAME_SYMBOLS, 3, LEAD), (None, 31, LEAD), (P.VCM_FRAME_SYMBOLS, 31, stream["off"][2]), (None, 8, n_sym)):
        ld = None if LEN is None else dev(LEN)
        want = walk_dev(rx, xd.data_ptr(), n_sym, start, None if LEN is None else ld.data_ptr(), P.PLS_SEARCH_Q_MIN, max_out)
        OFF, VAL, Q, IDX, CNT, RES = rx.pls_walk(x, start, LEN=LEN, max_out=max_out)
        assert np.array_equal(RES, want["RES"]) and np.array_equal(CNT, want["CNT"])
        for g, k in ((OFF, "OFF"), (VAL, "VAL"), (IDX, "IDX")):
            assert np.array_equal(g, want[k]), k
        assert np.array_equal(Q.view(np.int32), want["Q"].view(np.int32))


def test_errors_leave_the_handle_usable(rx, P, stream):
    x, n_sym = stream["x"], stream["n_sym"]
    xp = x.ctypes.data_as(C.c_void_p)
    o = [np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(8, np.int32), np.zeros(256, np.int32), np.zeros(4, np.int32)]
    p = [a.ctypes.data_as(C.c_void_p) for a in o]
    L = rx.L
    q = C.c_float(0.3)
    host = lambda X, n, start, max_out, out=p: L.dvbs2hip_pls_walk(rx.h, X, n, start, None, q, max_out, *out)
    devf = lambda X, n, start, max_out, out=p: L.dvbs2hip_pls_walk_dev(rx.h, X, n, start, None, q, max_out, out[0], out[1], out[2], None, out[3], out[4], out[5])
    for fn in (host, devf):
        for n in (89, 0, -1, (1 << 24) + 1):
            assert fn(xp, n, 0, 8) == EINVAL and b"n_sym" in L.dvbs2hip_last_error(rx.h)
        for start in (-1, n_sym + 1):
            assert fn(xp, n_sym, start, 8) == EINVAL and b"start" in L.dvbs2hip_last_error(rx.h)
        for max_out in (0, -3):
            assert fn(xp, n_sym, 0, max_out) == EINVAL and b"max_out" in L.dvbs2hip_last_error(rx.h)
        assert fn(None, n_sym, 0, 8) == EINVAL and b"null" in L.dvbs2hip_last_error(rx.h)
        for k in range(6):
            assert fn(xp, n_sym, 0, 8, p[:k] + [None] + p[k + 1:]) == EINVAL and b"null" in L.dvbs2hip_last_error(rx.h)
    assert devf(C.c_void_p(xp.value + 4), n_sym, 0, 8) == EINVAL and b"aligned" in L.dvbs2hip_last_error(rx.h)
    assert L.dvbs2hip_pls_walk(None, xp, n_sym, 0, None, q, 8, *p) == EINVAL
    assert rx.pls_walk(x, LEAD, LEN=P.VCM_FRAME_SYMBOLS)[5].tolist() == [8, stream["off"][8], W.END, 0]


@pytest.mark.parametrize("max_out", [31, 4096])
def test_a_recorded_walk_replays_on_new_input(P, stream, max_out):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    rx = Dvbs2Hip("16APSK-S_8/9", max_frames=1)
    x, off, n_sym = stream["x"], stream["off"], stream["n_sym"]
    y = x.copy()
    y[2 * off[5]:2 * (off[5] + 90)] = 0                                              # the second input: frame 6's header is missing
    xd = torch.zeros(2 * n_sym, dtype=torch.float32, device="cuda")
    LEN = dev(P.VCM_FRAME_SYMBOLS)
    n = min(max_out, 64)
    t = dict(OFF=torch.zeros(n, dtype=torch.int32), VAL=torch.zeros(n, dtype=torch.int32), Q=torch.zeros(n), SRC=torch.zeros(n, dtype=torch.int64), IDX=torch.zeros(n, dtype=torch.int32),
             CNT=torch.zeros(256, dtype=torch.int32), RES=torch.zeros(4, dtype=torch.int32))
    t = {k: v.cuda() for k, v in t.items()}
    torch.cuda.synchronize()

    def once(start=LEAD):
        rx.pls_walk_dev(xd.data_ptr(), n_sym, start, LEN.data_ptr(), None, max_out, *(t[k].data_ptr() for k in ("OFF", "VAL", "Q", "SRC", "IDX", "CNT", "RES")))

    once(n_sym); rx.synchronize()                                                    # allocates the workspace: for this n_sym and max_out, whatever the start
    assert t["RES"].cpu().numpy().tolist() == [0, n_sym, W.END, 0]
    gid = rx.graph_capture(once)
    for inp, res in ((x, [8, off[8], W.END, 0]), (y, [5, off[5], W.LOST, 0])):
        xd.copy_(torch.from_numpy(np.array(inp))); torch.cuda.synchronize()
        once(); rx.synchronize()
        want = {k: v.clone() for k, v in t.items()}
        for v in t.values():
            v.fill_(-9)
        torch.cuda.synchronize()
        rx.graph_launch(gid); rx.synchronize()
        N = res[0]
        assert t["RES"].cpu().numpy().tolist() == res and torch.equal(t["CNT"], want["CNT"])
        for k in ("OFF", "VAL", "Q", "SRC", "IDX"):
            assert torch.equal(t[k][:N], want[k][:N]), k
    rx.graph_destroy(gid)
    rx.close()


def test_a_buffer_of_2_to_the_20_symbols(rx, P):
    """short frames over and over; the twin follows the chain with the float64 decoder at the headers it visits"""
    from dvbs2_amd.receiver import Dvbs2Hip
    n_sym = 1 << 20
    parts = []
    for i, name in enumerate(("QPSK-S_3/5", "32APSK-S_3/4", "16APSK-S_8/9", "8PSK-S_3/5")):
        h = Dvbs2Hip(name, max_frames=2)
        parts += list(h.tx_bb(2, seed=200 + i)[1])
        h.close()
    cycle = np.concatenate(parts)
    x = np.tile(cycle, -(-2 * n_sym // cycle.size))[:2 * n_sym]
    want = W.walk(W.header64(x), n_sym, 0, P.VCM_FRAME_SYMBOLS, P.PLS_SEARCH_Q_MIN, 4096)
    N = int(want[3][0])
    assert N > 190 and want[3][2] == W.END
    xd = dev(x)
    for LEN in (None, dev(P.VCM_FRAME_SYMBOLS)):                                     # 9 levels with the library's table, 13 with a caller's
        got = walk_dev(rx, xd.data_ptr(), n_sym, 0, None if LEN is None else LEN.data_ptr(), P.PLS_SEARCH_Q_MIN, 4096)
        assert got["RES"].tolist() == want[3].tolist()
        assert got["OFF"][-1] == want[0][-1] and np.array_equal(got["OFF"], want[0]) and np.array_equal(got["VAL"], want[1])
        CNT, IDX = W.group(want[1])
        assert np.array_equal(got["CNT"], CNT) and np.array_equal(got["IDX"], IDX)
    got = walk_dev(rx, xd.data_ptr(), n_sym, 0, None, P.PLS_SEARCH_Q_MIN, 100)  # FULL on a long chain
    assert got["RES"].tolist() == [100, int(want[0][100]), W.FULL, 0] and np.array_equal(got["OFF"], want[0][:100])
