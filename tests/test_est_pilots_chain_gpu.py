"""Why the pilot-aided estimator exists, end to end: with the default decoder (SPA, 50 iterations, early stop) the 16APSK and 32APSK chains lose every frame when sigma
comes from the M2M4 estimator, which reads these constellations several dB low, and none when it comes from the frames' header and pilot symbols.  The control arms run the
existing path unchanged: they record the failure, they are not to be made to pass by touching the M2M4 estimator."""
import io

import numpy as np
import pytest

from helpers import make_pl_frames

pytestmark = pytest.mark.gpu

F = 48
CASES = [("16APSK-S_8/9", 8.0), ("32APSK-S_3/4", 7.8)]


@pytest.mark.parametrize("modcod,ebn0", CASES)
def test_sigma_from_the_pilots_decodes_what_m2m4_sigma_loses(O, modcod, ebn0):
    import torch
    from dvbs2_amd.receiver import Dvbs2Hip
    info, pl, _, sigma = make_pl_frames(O, modcod, F, ebn0, seed=5)
    rx = Dvbs2Hip(modcod, max_frames=F, n_ite=50, early_stop=True, implem="SPA")
    # pilots arm: the estimate goes from the task into the fused chain on the device
    x = torch.from_numpy(pl).cuda()
    sig = torch.zeros(F, dtype=torch.float32, device="cuda")
    bits = torch.zeros((F, rx.K_bch), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rx.estimate_pilots_dev(x.data_ptr(), 1, sig.data_ptr(), None, None, F)
    rx.rx_bb_dev(x.data_ptr(), sig.data_ptr(), bits.data_ptr(), None, None, F)
    rx.synchronize()
    s = sig.cpu().numpy()
    lost = int((bits.cpu().numpy() != info).any(1).sum())
    print("%s at %.1f dB: true sigma %.4f, pilots %.4f .. %.4f, frames lost %d of %d" % (modcod, ebn0, sigma, s.min(), s.max(), lost, F))
    assert np.abs(s / sigma - 1).max() < 0.2
    assert lost == 0
    # control arm: the existing path, sigma from the M2M4 estimator inside the chain
    got = rx.rx_bb(pl)[0]
    lost_m2m4 = int((got != info).any(1).sum())
    print("%s at %.1f dB: frames lost with the M2M4 estimate %d of %d" % (modcod, ebn0, lost_m2m4, F))
    assert lost_m2m4 >= F // 2
    # and with the channel's own sigma nothing is lost: the frames are decodable
    assert not (rx.rx_bb(pl, sigma=sigma)[0] != info).any()
    rx.close()


MODCOD = "16APSK-S_8/9"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """32 frames of 16APSK-S_8/9 through tx and the channel at Eb/N0 = 8 dB -> (pattern file, noisy IQ file, directory)"""
    from dvbs2_amd import ch, params as P, tx
    from dvbs2_amd.srcfile import save_src
    K = P.get_modcod(MODCOD).K_bch
    d = tmp_path_factory.mktemp("est_pilots")
    src, f_tx, f_noisy = (str(d / n) for n in ("pattern.src", "out_tx.bin", "out_tx_noisy.bin"))
    save_src(src, np.random.default_rng(3).integers(0, 2, K).astype(np.int32))
    log = io.StringIO()
    assert tx.run(tx.build_parser().parse_args(["--rad-tx-file-path", f_tx, "-F", "8", "--src-type", "USER", "--src-path", src, "--mod-cod", MODCOD, "--n-frames", "32"]), out=log) == 32
    assert ch.run(ch.build_parser().parse_args(["--rad-rx-file-path", f_tx, "--rad-tx-file-path", f_noisy, "--rad-rx-no-loop", "-F", "8", "--mod-cod", MODCOD, "-m", "8.0"]), out=log) == 32
    return src, f_noisy, d


def rx_run(f_noisy, src, extra):
    from dvbs2_amd import rx
    log = io.StringIO()
    st = rx.run(rx.build_parser().parse_args(["--rad-rx-file-path", f_noisy, "-F", "8", "--mod-cod", MODCOD, "--dec-implem", "SPA", "--src-type", "USER", "--src-path", src,
                                              "--rad-rx-no-loop"] + extra), out=log)
    return st, log.getvalue()


def test_rx_recovers_a_16apsk_file_with_est_type_pilots_and_not_without(files):
    src, f_noisy, _ = files
    st, printed = rx_run(f_noisy, src, ["--est-type", "PILOTS"])
    assert st["locked_frames"] >= 24 and st["be"] == 0 and st["fe"] == 0, printed
    st0, printed0 = rx_run(f_noisy, src, ["--est-type", "DVBS2"])
    assert st0["locked_frames"] == st["locked_frames"] and st0["fe"] >= st0["locked_frames"] // 2, printed0
    st1, printed1 = rx_run(f_noisy, src, [])                                         # the default is the reference's estimator
    assert st1 == st0 and printed1 == printed0
