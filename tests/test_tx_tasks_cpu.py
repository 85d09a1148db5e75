"""The TX tasks without a GPU: the binding and the command line know them, and the oracle's seven stages -- the references of test_tx_tasks_gpu.py -- compose to its
Chain.tx with the systematic parts where the C ABI says they are."""
import numpy as np
import pytest

from helpers import chain
from test_tx_gpu import ALL

TASKS = ["bb_scramble", "bch_encode", "ldpc_encode", "interleave", "modulate", "framer_generate", "pl_scramble"]


def test_binding_holds_the_fourteen_entries():
    from dvbs2_amd import lib_binding as B
    from dvbs2_amd.receiver import Dvbs2Hip
    for t in TASKS:
        for sfx in ("", "_dev"):
            assert "dvbs2hip_" + t + sfx in B.ABI
            assert callable(getattr(Dvbs2Hip, t + sfx))
    assert len([n for n in B.ABI if n[len("dvbs2hip_"):].replace("_dev", "") in TASKS]) == 14


def test_tx_parser_takes_tx_tasks_and_defaults_to_off():
    from dvbs2_amd import tx
    ap = tx.build_parser()
    assert ap.parse_args(["--rad-tx-file-path", "x.bin"]).tx_tasks is False
    assert ap.parse_args(["--rad-tx-file-path", "x.bin", "--tx-tasks"]).tx_tasks is True


def test_tx_tasks_refuse_the_random_source_before_any_device_work(tmp_path):
    from dvbs2_amd import tx
    with pytest.raises(ValueError, match="tx-tasks"):
        tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", str(tmp_path / "x.bin"), "--tx-tasks", "--src-type", "RAND", "--n-frames", "1"]))


# K_bch -> parity weights of the BCH and the LDPC encoder for an impulse at bit 0 of their own input
IMPULSE_W = {14232: (84, 1465), 9552: (71, 2526), 11712: (82, 2551), 57472: (66, 5861)}


@pytest.mark.parametrize("modcod", ALL)
def test_oracle_stages_compose_to_chain_tx(O, modcod):
    ch = chain(O, modcod)
    mc = ch.mc
    info = np.random.default_rng(5).integers(0, 2, mc.K_bch).astype(np.int32)
    scr = O.bb_scramble(info)
    bch = ch.bch.encode(scr)[0]
    cw = ch.ldpc.encode(bch)[0]
    sym = O.modulate(ch.cstl, mc.bps, cw[ch.lut])
    plf = O.framer_generate(sym, ch.plh)
    pl = O.pl_scramble(plf, 90, True)
    want, want_cw = ch.tx(info)
    assert pl.dtype == np.float32 and np.array_equal(pl.view(np.uint32), want.view(np.uint32)) and np.array_equal(cw, want_cw)
    assert bch.size == mc.K_ldpc and np.array_equal(bch[:mc.K_bch], scr) and cw.size == mc.N_ldpc and np.array_equal(cw[:mc.K_ldpc], bch)
    assert sym.size == 2 * mc.N_xfec and plf.size == 2 * mc.pl_frame and np.array_equal(plf[:180], ch.plh) and np.array_equal(pl[:180], ch.plh)
    assert np.array_equal(O.bb_scramble(scr), info)                      # the same XOR both ways
    if mc.itl_cols == 1:
        assert np.array_equal(cw[ch.lut], cw)
    u = np.zeros(mc.K_bch, np.int32); u[0] = 1
    v = np.zeros(mc.K_ldpc, np.int32); v[0] = 1
    assert (int(ch.bch.encode(u)[0, mc.K_bch:].sum()), int(ch.ldpc.encode(v)[0, mc.K_ldpc:].sum())) == IMPULSE_W[mc.K_bch]
