"""Throughput of the gene profile's hits on the device (sc_profile_hits): DP cell updates/s, (segment, gene) pairs/s and
hits/s of the score pass (k_bl_score) and of the traceback pass (k_bl_trace), on the data set of tools/stage4_bench.py:
100 genes of 1 500 bp, segments of 150 bp drawn from strains of the genes (1 % substitutions) and from relatives (3 %, 8 %
and 20 % divergent).

    python tools/profile_bench.py [--reads N] [--repeat K] [--warmup W] [--seeded] [--related]

--seeded runs sc_profile_hits_seeded and adds seed_k, the pair count and its share of the full product,
index_ms and lookup_ms.  --related swaps the data set for one in which genes do share k-mers, as 16S genes do: the genes are
3-10 % divergent relatives of a few ancestors with conserved blocks kept exact (in the default set the genes are unrelated
random sequences, and a k-mer filter removes nearly every pair).

One JSON line per repeat after W unreported warm-up calls (the first call also pays for loading the code objects).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rambl_amd import capi  # noqa: E402
from stage4_bench import dataset  # noqa: E402


def related_dataset(n_reads, n_genes=100, glen=1500, n_ancestors=5, seed=7):
    """n_genes relatives of n_ancestors random ancestors: every base outside the conserved blocks (four of 60 bases per
    ancestor, shared by all ancestors) substituted at a rate drawn from 3-10 % per gene; n_reads segments of 150 bases from
    the genes, 1 % substitutions, either strand."""
    import random
    rng = random.Random(seed)
    comp = str.maketrans("ACGT", "TGCA")
    blocks = ["".join(rng.choice("ACGT") for _ in range(60)) for _ in range(4)]
    starts = [200, 550, 900, 1250]
    ancestors = []
    for _ in range(n_ancestors):
        a = ["".join(rng.choice("ACGT") for _ in range(glen))][0]
        for b, p in zip(blocks, starts):
            a = a[:p] + b + a[p + 60:]
        ancestors.append(a)
    genes = []
    for g in range(n_genes):
        a, rate = ancestors[g % n_ancestors], rng.uniform(0.03, 0.10)
        out = list(a)
        for p in range(glen):
            if not any(q <= p < q + 60 for q in starts) and rng.random() < rate:
                out[p] = rng.choice([c for c in "ACGT" if c != out[p]])
        genes.append("".join(out).encode())
    segs = []
    for _ in range(n_reads):
        g = genes[rng.randrange(n_genes)].decode()
        p = rng.randint(0, glen - 150)
        r = "".join(rng.choice([c for c in "ACGT" if c != x]) if rng.random() < 0.01 else x for x in g[p:p + 150])
        segs.append((r[::-1].translate(comp) if rng.random() < 0.5 else r).encode())
    return genes, segs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--identity", type=float, default=95.0)
    ap.add_argument("--evalue", type=float, default=1e-10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seeded", action="store_true", help="sc_profile_hits_seeded: score only the pairs that share a k-mer")
    ap.add_argument("--related", action="store_true", help="genes that share k-mers: relatives of a few ancestors with conserved blocks")
    a = ap.parse_args(argv)
    genes, segs = related_dataset(a.reads) if a.related else dataset(a.reads)[:2]
    for k in range(-a.warmup, a.repeat):
        t0 = time.perf_counter()
        res = capi.profile_hits(genes, segs, a.identity, a.evalue, device=a.device, **({"seeded": True} if a.seeded else {}))
        wall = time.perf_counter() - t0
        if k < 0:
            continue
        st = res.stats
        pairs = len(segs) * len(genes)
        extra = {}
        if a.seeded:
            extra = {"seed_k": int(st.seed_k), "gene_kmers": int(st.n_gene_kmers), "pairs": int(st.n_pairs),
                     "pair_share": st.n_pairs / pairs if st.seed_k else 1.0, "index_ms": round(st.index_ms, 3), "lookup_ms": round(st.lookup_ms, 3)}
        print(json.dumps({
            "repeat": k, "data": "related" if a.related else "default", "seeded": bool(a.seeded), **extra, "segments": len(segs), "genes": len(genes), "tiles": int(st.n_tiles), "candidates": int(st.n_candidates),
            "traced": int(st.n_traced), "hits": int(st.n_hits),
            "score_ms": round(st.score_ms, 3), "score_cells_per_s": st.score_cells / (st.score_ms / 1e3),
            "score_pairs_per_s": pairs / (st.score_ms / 1e3), "score_hits_per_s": st.n_hits / (st.score_ms / 1e3),
            "trace_ms": round(st.trace_ms, 3), "trace_cells_per_s": st.trace_cells / max(st.trace_ms / 1e3, 1e-9),
            "trace_pairs_per_s": st.n_traced / max(st.trace_ms / 1e3, 1e-9), "trace_hits_per_s": st.n_hits / max(st.trace_ms / 1e3, 1e-9),
            "upload_ms": round(st.upload_ms, 3), "call_ms": round(st.total_ms, 3), "wall_s": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
