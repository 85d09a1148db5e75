"""The transmitter's tasks at the task boundary (dvbs2hip_bb_scramble .. dvbs2hip_pl_scramble) against the oracle, stage by stage: each task alone on the oracle's
output of the stage before it, the seven chained on the device against the fused tx_bb, the encoders on impulses, device sockets that start off a 16-byte
boundary, and the error returns.  Bits compare as int32, symbols by value (the oracle's 8PSK / 32APSK frames hold negative zeros that a turn by swaps need not sign
the same way: the bar of test_tx_matches_oracle)."""
import ctypes

import numpy as np
import pytest

from helpers import chain
from test_tx_gpu import ALL

pytestmark = pytest.mark.gpu
F = 5
STAGES = ["bb_scramble", "bch_encode", "ldpc_encode", "interleave", "modulate", "framer_generate", "pl_scramble"]


def payloads(K):
    info = np.zeros((F, K), np.int32)
    info[1] = 1
    info[2, 0] = 1
    info[3, K - 1] = 1
    info[4] = np.random.default_rng(2024).integers(0, 2, K)
    return info


def oracle_stages(O, ch, info):
    """-> the eight sockets of the chain, [F, .] each: payload, then the output of every stage in STAGES' order"""
    mc = ch.mc
    scr = np.stack([O.bb_scramble(u) for u in info])
    bch = ch.bch.encode(scr)
    cw = ch.ldpc.encode(bch)
    itl = cw[:, ch.lut]
    sym = np.stack([O.modulate(ch.cstl, mc.bps, x) for x in itl])
    plf = np.stack([O.framer_generate(x, ch.plh) for x in sym])
    pl = np.stack([O.pl_scramble(x, 90, True) for x in plf])
    return [info, scr, bch, cw, itl, sym, plf, pl]


_ctx = {}


@pytest.fixture(scope="module")
def ctx(O):
    """modcod -> (handle with max_frames = 5, oracle chain, the oracle's sockets for the five payloads): made once per MODCOD, shared and left unchanged"""
    from dvbs2_amd.receiver import Dvbs2Hip

    def get(modcod):
        if modcod not in _ctx:
            ch = chain(O, modcod)
            ref = oracle_stages(O, ch, payloads(ch.mc.K_bch))
            for a in ref:
                a.setflags(write=False)
            _ctx[modcod] = (Dvbs2Hip(modcod, max_frames=F), ch, ref)
        return _ctx[modcod]
    yield get
    for rx, _, _ in _ctx.values():
        rx.close()
    _ctx.clear()


def same(got, ref):
    if ref.dtype == np.int32:
        return got.dtype == np.int32 and got.shape == ref.shape and np.array_equal(got, ref)
    return got.dtype == np.float32 and got.shape == ref.shape and not np.isnan(got).any() and np.array_equal(got, ref)


@pytest.mark.parametrize("modcod", ALL)
def test_each_task_alone_matches_its_oracle_stage(ctx, modcod):
    rx, ch, ref = ctx(modcod)
    for k, name in enumerate(STAGES):
        got = getattr(rx, name)(ref[k])
        assert same(got, ref[k + 1]), "%s: %d of %d elements differ" % (name, int((got != ref[k + 1]).sum()), got.size)
        one = getattr(rx, name)(ref[k][4:5])                       # F = 1 on the same handle
        assert same(one, ref[k + 1][4:5]), name


@pytest.mark.parametrize("modcod", ALL)
def test_chain_of_dev_tasks_equals_tx_bb_and_the_oracle(ctx, modcod):
    from dvbs2_amd.tx import TxTasks
    rx, ch, ref = ctx(modcod)
    info = np.array(ref[0])
    pl = TxTasks(rx, F).run(info)
    sent, fused = rx.tx_bb(F, info=info)
    assert np.array_equal(sent, info)
    assert same(pl, fused)
    for f in range(F):
        plo, _ = ch.tx(info[f])
        assert same(pl[f], plo), "frame %d differs at %d floats" % (f, int((pl[f] != plo).sum()))


# K_bch -> parity weights of the oracle's BCH and LDPC encoders for an impulse at bit 0 of their own input (pinned on the CPU in test_tx_tasks_cpu.py)
IMPULSE_W = {14232: (84, 1465), 9552: (71, 2526), 11712: (82, 2551), 57472: (66, 5861)}


@pytest.mark.parametrize("modcod", ALL)
def test_encoders_on_impulses(ctx, modcod):
    """The encoders are linear.  On the two impulse payloads of the fixture the parities are non-zero and the oracle's; an impulse fed to an encoder itself gives the
    oracle's parity, and the parity of (scrambled impulse) XOR (scrambled zeros) is the impulse's."""
    rx, ch, ref = ctx(modcod)
    mc = ch.mc
    bch, cw = rx.bch_encode(ref[1]), rx.ldpc_encode(ref[2])
    for f in (2, 3):
        assert bch[f, mc.K_bch:].any() and np.array_equal(bch[f, mc.K_bch:], ref[2][f, mc.K_bch:])
        assert cw[f, mc.K_ldpc:].any() and np.array_equal(cw[f, mc.K_ldpc:], ref[3][f, mc.K_ldpc:])
    u = np.zeros((2, mc.K_bch), np.int32); u[0, 0] = 1; u[1, -1] = 1
    v = np.zeros((2, mc.K_ldpc), np.int32); v[0, 0] = 1; v[1, -1] = 1
    gb, gl = rx.bch_encode(u), rx.ldpc_encode(v)
    assert np.array_equal(gb, ch.bch.encode(u)) and np.array_equal(gl, ch.ldpc.encode(v))
    assert gb[:, mc.K_bch:].any(axis=1).all() and gl[:, mc.K_ldpc:].any(axis=1).all()
    assert np.array_equal(bch[2, mc.K_bch:] ^ bch[0, mc.K_bch:], gb[0, mc.K_bch:]) and np.array_equal(bch[3, mc.K_bch:] ^ bch[0, mc.K_bch:], gb[1, mc.K_bch:])
    assert (int(gb[0, mc.K_bch:].sum()), int(gl[0, mc.K_ldpc:].sum())) == IMPULSE_W[mc.K_bch]


@pytest.mark.parametrize("modcod", ["QPSK-S_3/5", "32APSK-S_3/4"])
def test_unaligned_device_sockets(ctx, modcod):
    """both sockets of every _dev task one element (4 bytes for bits, 8 for a symbol) into a larger tensor: the same output as the aligned call, nothing written behind it"""
    import torch
    rx, ch, ref = ctx(modcod)
    dev = torch.device("cuda", 0)
    for k, name in enumerate(STAGES):
        x, want = ref[k], ref[k + 1]
        e_in = 1 if x.dtype == np.int32 else 2                    # scalars per element
        e_out = 1 if want.dtype == np.int32 else 2
        tdt = lambda a: torch.int32 if a.dtype == np.int32 else torch.float32
        big_in = torch.zeros(x.size + 2 * e_in, dtype=tdt(x), device=dev)
        big_in[e_in:e_in + x.size] = torch.from_numpy(np.array(x)).ravel().to(dev)
        guard = 77 if want.dtype == np.int32 else 77.0
        big_out = torch.full((want.size + 2 * e_out,), guard, dtype=tdt(want), device=dev)
        torch.cuda.synchronize()
        isz = big_in.element_size()
        getattr(rx, name + "_dev")(big_in.data_ptr() + e_in * isz, big_out.data_ptr() + e_out * isz, F)
        rx.synchronize()
        out = big_out.cpu().numpy()
        aligned = getattr(rx, name)(x)
        assert same(out[e_out:e_out + want.size].reshape(want.shape), aligned), name
        assert same(aligned, want), name
        assert (out[:e_out] == guard).all() and (out[e_out + want.size:] == guard).all(), name


def test_errors_leave_the_handle_usable(ctx):
    rx, ch, ref = ctx("QPSK-S_8/9")
    L = rx.L
    for k, name in enumerate(STAGES):
        x = np.ascontiguousarray(ref[k])
        out = np.empty_like(ref[k + 1])
        pi, po = x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
        for sfx in ("", "_dev"):
            fn = getattr(L, "dvbs2hip_" + name + sfx)
            assert fn(rx.h, pi, po, 0) == -1 and fn(rx.h, pi, po, F + 1) == -1, name + sfx
            assert fn(rx.h, None, po, F) == -1 and fn(rx.h, pi, None, F) == -1, name + sfx
            assert fn(None, pi, po, F) == -1, name + sfx
        assert same(getattr(rx, name)(ref[k]), ref[k + 1]), name
