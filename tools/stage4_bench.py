"""Throughput of stage 4 on the device (sc_align_reads): reads/s and DP cell updates/s of the score pass (k_sw_score) and
of the traceback pass (k_sw_trace), on a synthetic set shaped like configs[2]: 100 seeds of 1 500 bp, reads of 150 bp
drawn from strains of the seeds (1 % substitutions) and from non-seed relatives (3 %, 8 % and 20 % divergent).

    python tools/stage4_bench.py [--reads N] [--repeat K]

One JSON line per repeat; the first call also pays for loading the code objects.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rambl_amd import capi  # noqa: E402


def mutate(rng, s, rate):
    b = bytearray(s)
    for i in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + int(rng.integers(1, 4))) % 4]
    return bytes(b)


def dataset(n_reads, n_seeds=100, glen=1500, rlen=150, seed=2):
    rng = np.random.default_rng(seed)
    seeds = [bytes(rng.choice(list(b"ACGT"), glen).astype(np.uint8)) for _ in range(n_seeds)]
    sources = [mutate(rng, s, 0.01) for s in seeds] + [mutate(rng, s, r) for s in seeds for r in (0.03, 0.08, 0.20)]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads, quals = [], []
    for _ in range(n_reads):
        src = sources[int(rng.integers(len(sources)))] if rng.random() < 0.5 else sources[int(rng.integers(n_seeds))]
        a = int(rng.integers(0, len(src) - rlen + 1))
        r = mutate(rng, src[a:a + rlen], 0.003)
        if rng.random() < 0.5:
            r = r.translate(comp)[::-1]
        reads.append(r)
        quals.append(bytes(rng.choice([63, 68, 71, 73], rlen).astype(np.uint8)))
    return seeds, reads, quals


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    seeds, reads, quals = dataset(a.reads)
    for k in range(a.repeat):
        t0 = time.perf_counter()
        res = capi.align_reads(seeds, reads, quals, a.device)
        wall = time.perf_counter() - t0
        st = res.stats
        print(json.dumps({
            "repeat": k, "reads": len(reads), "seeds": len(seeds), "aligned": int(st.n_traced),
            "score_ms": round(st.score_ms, 3), "score_reads_per_s": len(reads) / (st.score_ms / 1e3),
            "score_cells_per_s": st.score_cells / (st.score_ms / 1e3),
            "trace_ms": round(st.trace_ms, 3), "trace_reads_per_s": st.n_traced / max(st.trace_ms / 1e3, 1e-9),
            "trace_cells_per_s": st.trace_cells / max(st.trace_ms / 1e3, 1e-9),
            "upload_ms": round(st.upload_ms, 3), "call_ms": round(st.total_ms, 3), "wall_s": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
