"""q_min of params.find_modcod, measured on the CPU with the float64 twin of the PLHEADER search (tests/pls_search_ref.py):

  no header   the largest per-slot score SCORE / SLOTS the search finds in buffers that hold no PLHEADER: SEEDS noise-only buffers and SEEDS data-only ones (QPSK,
              8PSK and 16APSK symbols in turn, at 6 dB), 2 * 8370 + 90 symbols each, the library's own length table
  true chain  the smallest per-slot score of the true chain at the lowest operating point among the library's MODCODs -- QPSK-S_3/5 at the Es/N0 of the lowest Eb/N0 row
              of its trace in tests/golden/refs_tx_rx_bb.json -- over SEEDS buffers of the same length that start at a header: three slots, a slot whose header decodes
              to another value counting 0 as the definition has it (a window on a true header holds the header and noise, so only those windows are drawn)

q_min is the geometric mean of the two.
usage: python tools/measure_pls_search_qmin.py [--out results/pls_search/qmin.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import pls_search_ref as R
from dvbs2_amd import params as P

SEEDS = 20
N_SYM = 2 * 8370 + 90
KINDS = ["qpsk", "8psk", "16apsk"]


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    no_header = []
    for seed in range(SEEDS):
        for kind in ("noise", KINDS[seed % 3]):
            x = R.header_free_buffer(np.random.default_rng([seed, kind != "noise"]), N_SYM, kind)
            res, score = R.search64(x, P.PLS_FRAME_SYMBOLS)
            per_slot = float(score) / max(1, int(res[3]))
            no_header.append(dict(seed=seed, kind=kind, res=res.tolist(), score=float(score), per_slot=per_slot))
            print("no header   seed %2d %-6s RES %-24s per slot %.4f" % (seed, kind, res.tolist(), per_slot), flush=True)
    mc = P.get_modcod("QPSK-S_3/5")
    esn0 = R.lowest_esn0(P, mc.name)
    sigma, value = P.esn0_to_sigma(esn0), P.pls_value(mc)
    true_chain = []
    for seed in range(SEEDS):
        rng = np.random.default_rng([seed, 2])
        w = R.HEADERS[value][None, :] * np.exp(1j * rng.uniform(0, 2 * np.pi)) + sigma * (rng.standard_normal((3, 90)) + 1j * rng.standard_normal((3, 90)))
        w = w.astype(np.complex64).astype(np.complex128)
        V, met, _ = R.ml_decode(w)
        q = np.where(V == value, met ** 2 / (90 * (np.abs(w) ** 2).sum(1)), 0.0)
        true_chain.append(dict(seed=seed, decoded=V.tolist(), q=q.tolist(), per_slot=float(q.mean())))
        print("true chain  seed %2d decoded %s q %s per slot %.4f" % (seed, V.tolist(), np.round(q, 3).tolist(), q.mean()), flush=True)
    hi, lo = max(r["per_slot"] for r in no_header), min(r["per_slot"] for r in true_chain)
    q_min = float(np.sqrt(hi * lo))
    line = json.dumps(dict(tool="measure_pls_search_qmin", seeds=SEEDS, n_sym=N_SYM, esn0_db=esn0, modcod=mc.name, largest_without_header=hi, smallest_true_chain=lo, q_min=q_min,
                           no_header=no_header, true_chain=true_chain))
    print("largest per-slot score without a header %.4f | smallest of the true chain at %.2f dB %.4f | q_min = geometric mean = %.4f" % (hi, esn0, lo, q_min))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
