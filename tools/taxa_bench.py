"""Throughput of the genus assignment on the device (sc_taxa_train, sc_taxa_classify) on a synthetic
training set: 2 000 genera x 10 sequences x 1 500 bases (each genus a random ancestor, its sequences 3 % apart from it) and
1 000 queries of 1 500 bases (2 % apart from the ancestor of a random genus).

    python tools/taxa_bench.py [--genera G] [--per-genus N] [--length L] [--queries Q] [--repeat K] [--warmup W]

One JSON line per repeat after W unreported warm-up rounds (the first call also pays for loading the code objects); a round
trains a model and classifies the queries with it.  The times are the calls' own HIP-event statistics.  score_table_bytes is
what the score pass reads of the table, (W + 100 * D) * G * 4 per query with D = max(W / 8, 5), computed here from the
shapes; score_table_bytes_per_s divides it by score_ms (k_taxa_score and k_taxa_pick).  `agree` is the share of queries
assigned to the genus they were drawn from.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rambl_amd import capi  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _mutated(rng, anc, rate):
    out = anc.copy()
    hit = rng.random(len(anc)) < rate
    out[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    return BASES[out].tobytes()


def dataset(n_genera, per_genus, length, n_queries, seed=17):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, (n_genera, length), dtype=np.uint8)
    seqs, genus = [], []
    for g in range(n_genera):
        for _ in range(per_genus):
            seqs.append(_mutated(rng, anc[g], 0.03))
            genus.append(g)
    truth = rng.integers(0, n_genera, n_queries)
    queries = [_mutated(rng, anc[g], 0.02) for g in truth]
    return seqs, genus, queries, truth


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genera", type=int, default=2000)
    ap.add_argument("--per-genus", type=int, default=10)
    ap.add_argument("--length", type=int, default=1500)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    seqs, genus, queries, truth = dataset(a.genera, a.per_genus, a.length, a.queries)
    keys = list(range(1, len(queries) + 1))
    for k in range(-a.warmup, a.repeat):
        t0 = time.perf_counter()
        with capi.TaxaModel(seqs, genus, a.genera, a.device) as model:
            tr = model.stats
            best, winners, words, st = model.classify(queries, keys, seed=1)
        wall = time.perf_counter() - t0
        if k < 0:
            continue
        table_bytes = int(sum((int(w) + capi.TAXA_TRIALS * max(int(w) // 8, 5)) * a.genera * 4 for w in words if w))
        print(json.dumps({
            "repeat": k, "genera": a.genera, "train_seqs": len(seqs), "train_bases": sum(map(len, seqs)), "queries": len(queries),
            "query_words": int(words.sum()), "train_words": int(tr.n_words), "table_bytes": int(tr.table_bytes),
            "train_upload_ms": round(tr.upload_ms, 3), "words_ms": round(tr.words_ms, 3), "table_ms": round(tr.table_ms, 3),
            "train_call_ms": round(tr.total_ms, 3), "classify_upload_ms": round(st.upload_ms, 3), "score_ms": round(st.score_ms, 3),
            "classify_call_ms": round(st.total_ms, 3), "score_table_bytes": table_bytes,
            "score_table_bytes_per_s": table_bytes / (st.score_ms / 1e3), "queries_per_s": len(queries) / (st.score_ms / 1e3),
            "agree": float((best == truth).mean()), "wall_s": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
