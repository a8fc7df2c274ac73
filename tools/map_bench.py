"""The read mapper (sc_map_reads) on a synthetic database of related genes: phase times, pairs per read, the
share of reads whose AS equals the AS of sc_align_reads over all genes (on a subsample) and the share left unmapped, for the
defaults and for max_occ and max_cand at half and twice their defaults.

The database: families of genes that share conserved stretches, as a 16S database does.  A family has an ancestor made of
conserved blocks (common to every family) and variable blocks (the family's own); its members are the ancestor with 0.5 to
4 % substitutions.  The reads are 150 bases drawn from the genes at 0 to 5 % divergence, half of them reverse-complemented.

    python tools/map_bench.py [--families N] [--members M] [--reads N] [--sub N] [--out table.md]

One JSON line per setting, then the table in markdown (also written to --out).  The first call also pays for loading the
code objects; a warm-up call of a few reads goes before the timed ones.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rambl_amd import capi  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_seq(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def mutate(rng, s, rate):
    b = bytearray(s)
    for i in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + int(rng.integers(1, 4))) % 4]
    return bytes(b)


def dataset(n_families, n_members, n_reads, rlen=150, seed=18):
    rng = np.random.default_rng(seed)
    conserved = [rand_seq(rng, int(rng.integers(40, 120))) for _ in range(9)]
    genes = []
    for _ in range(n_families):
        ancestor = b"".join(mutate(rng, c, 0.01) + rand_seq(rng, int(rng.integers(60, 140))) for c in conserved)
        genes += [mutate(rng, ancestor, float(rng.uniform(0.005, 0.04))) for _ in range(n_members)]
    reads, quals, source = [], [], []
    for _ in range(n_reads):
        g = int(rng.integers(len(genes)))
        a = int(rng.integers(0, len(genes[g]) - rlen + 1))
        r = mutate(rng, genes[g][a:a + rlen], float(rng.uniform(0.0, 0.05)))
        if rng.random() < 0.5:
            r = r.translate(COMP)[::-1]
        reads.append(r)
        quals.append(bytes(rng.choice([63, 68, 71, 73], rlen).astype(np.uint8)))
        source.append(g)
    return genes, reads, quals, source


def main(argv=None):
    d = capi.MAP_DEFAULTS
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--families", type=int, default=250)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--sub", type=int, default=400, help="reads of the subsample that also go through sc_align_reads over all genes")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    genes, reads, quals, _ = dataset(a.families, a.members, a.reads)
    sub = min(a.sub, len(reads))
    t0 = time.perf_counter()
    full = capi.align_reads(genes, reads[:sub], quals[:sub], a.device)
    full_wall = time.perf_counter() - t0
    yard = {"setting": "sc_align_reads, all genes", "reads": sub, "genes": len(genes), "score_ms": round(full.stats.score_ms, 2),
            "trace_ms": round(full.stats.trace_ms, 2), "reads_per_s": round(sub / max(full.stats.total_ms / 1e3, 1e-9), 1),
            "wall_s": round(full_wall, 3)}
    print(json.dumps(yard), flush=True)
    rows = []
    with capi.MapIndex(genes, d["seed_k"], a.device) as ix:
        info = ix.info()
        ix.map_reads(reads[:8], quals[:8])
        settings = [("defaults", d["max_occ"], d["max_cand"])]
        settings += [("max_occ %d" % v, v, d["max_cand"]) for v in (d["max_occ"] // 2, d["max_occ"] * 2)]
        settings += [("max_cand %d" % v, d["max_occ"], v) for v in (d["max_cand"] // 2, d["max_cand"] * 2)]
        for name, max_occ, max_cand in settings:
            t0 = time.perf_counter()
            res = ix.map_reads(reads, quals, max_occ, max_cand, d["min_votes"])
            wall = time.perf_counter() - t0
            st = res.stats
            row = {"setting": name, "reads": len(reads), "genes": len(genes), "keys": info["n_keys"], "index_ms": round(info["index_ms"], 2),
                   "votes_ms": round(st.votes_ms, 2), "score_ms": round(st.score_ms, 2), "trace_ms": round(st.trace_ms, 2),
                   "call_ms": round(st.total_ms, 2), "reads_per_s": round(len(reads) / max(st.total_ms / 1e3, 1e-9), 1),
                   "pairs_per_read": round(st.n_pairs / len(reads), 2), "skipped_windows": round(st.n_skipped / max(st.n_windows, 1), 4),
                   "as_equal": round(float(np.mean(res.as_[:sub] == full.as_)), 4), "unmapped": round(float(np.mean(res.gene < 0)), 4),
                   "unmapped_all_genes": round(float(np.mean(full.seed < 0)), 4), "stretches": int(st.n_stretches), "wall_s": round(wall, 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    cols = ["setting", "votes_ms", "score_ms", "trace_ms", "call_ms", "reads_per_s", "pairs_per_read", "skipped_windows", "as_equal", "unmapped"]
    table = ["%d genes in %d families, %d keys (index %.1f ms), %d reads of 150 bases; the subsample of %d reads through sc_align_reads "
             "over all genes: %.1f reads/s, %.4f unmapped." % (len(genes), a.families, info["n_keys"], info["index_ms"], len(reads), sub,
                                                              yard["reads_per_s"], rows[0]["unmapped_all_genes"]), "",
             "| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    table += ["| " + " | ".join(str(r[c]) for c in cols) + " |" for r in rows]
    text = "\n".join(table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
