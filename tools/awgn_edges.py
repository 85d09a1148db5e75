#!/usr/bin/env python3
"""One-off: searches seeds whose noise reaches the edges of the Box-Muller map in the first 64 counters of frame 0, with the float64 twin
(tests/awgn_ref.py), and writes tests/golden/awgn_edge_seeds.json -- at least --hits entries per class and generator:

    A   radius word >= 2^32 - 128            u1 == 1.0f, the noise is exactly zero          2^-25 per word
    A2  radius word in [2^32 - 383, 2^32 - 129]   u1 = 1 - 2^-24, the largest float below 1   2^-24
    B   radius word < 200                    rad >= 5.81, the deep tail                     2^-24.4
    C   angle word >= 2^32 - 128             u2 == 1.0f, a whole revolution                 2^-25

for the channel's words x / y (stream 2) and the modulator's x / y and z / w (stream 1).  Seeds are scanned upwards from 0 and the first hits
kept, so the result does not depend on the number of processes.  No GPU; a few minutes of CPU.

    python tools/awgn_edges.py [--hits 4] [--procs 8]"""
import argparse
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import awgn_ref as R  # noqa: E402

PAIRS = 64
CHUNK = 1 << 15                     # seeds per task
# (stream, word inspected) per class kind: radius classes look at the radius word of the generator, C at its angle word
SLOTS = [(stream, rw, cls) for (stream, rw) in R.EDGE_GENERATORS for cls in R.EDGE_CLASSES]


def scan(c):
    seeds = np.arange(c * CHUNK, (c + 1) * CHUNK, dtype=np.uint64)[:, None]
    pair = np.arange(PAIRS, dtype=np.uint64)[None, :]
    found = []
    for stream in (2, 1):
        w = R.philox4x32_10((pair, 0, stream, 0), (seeds & R.M32, seeds >> np.uint64(32)))
        for (s, rw, cls) in SLOTS:
            if s != stream:
                continue
            word = rw + 1 if cls == "C" else rw
            for i, p in zip(*np.nonzero(R.edge_class(cls, w[word]))):
                found.append({"stream": stream, "seed": int(seeds[i, 0]), "frame": 0, "pair": int(p), "word": word, "class": cls, "r": int(w[word][i, p])})
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=4)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--max-chunks", type=int, default=1 << 10)
    ap.add_argument("-o", default=os.path.join(ROOT, "tests", "golden", "awgn_edge_seeds.json"))
    a = ap.parse_args()
    got = {(s, rw, cls): [] for (s, rw, cls) in SLOTS}
    with mp.Pool(a.procs) as pool:
        for c, found in enumerate(pool.imap(scan, range(a.max_chunks))):
            for e in sorted(found, key=lambda e: (e["seed"], e["pair"])):
                k = (e["stream"], e["word"] & 2, e["class"])
                if len(got[k]) < a.hits:
                    got[k].append(e)
            if all(len(v) >= a.hits for v in got.values()):
                break
            if c % 16 == 15:
                print("seeds below %d: %s" % ((c + 1) * CHUNK, " ".join(str(len(v)) for v in got.values())), flush=True)
    short = [k for k, v in got.items() if len(v) < a.hits]
    if short:
        sys.exit("not enough hits for %s: raise --max-chunks" % short)
    entries = [e for k in SLOTS for e in got[k]]
    with open(a.o, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(e) for e in entries) + "\n]\n")
    print("%d entries -> %s" % (len(entries), a.o))


if __name__ == "__main__":
    main()
