"""Throughput of the gene profile's hits on the device (sc_profile_hits): DP cell updates/s, (segment, gene) pairs/s and
hits/s of the score pass (k_bl_score) and of the traceback pass (k_bl_trace), on the data set of tools/stage4_bench.py:
100 genes of 1 500 bp, segments of 150 bp drawn from strains of the genes (1 % substitutions) and from relatives (3 %, 8 %
and 20 % divergent).

    python tools/profile_bench.py [--reads N] [--repeat K] [--warmup W] [--seeded] [--related | --conserved] [--profile]

--seeded runs sc_profile_hits_seeded and adds seed_k, the pair count and its share of the full product,
index_ms and lookup_ms.  --related swaps the data set for one in which genes do share k-mers, as 16S genes do: the genes are
3-10 % divergent relatives of a few ancestors with conserved blocks kept exact (in the default set the genes are unrelated
random sequences, and a k-mer filter removes nearly every pair).

--conserved swaps it for 100 genes that share four exact 60-base blocks and differ everywhere else, so that most segments
hit most genes: the shape the counts mode is for.

--profile times the whole tool instead of the device call: profile.gene_profile from a FASTA and a SAM file to the table,
wall time with Python included, with and without --counts (add --seeded for both legs); one JSON line per leg and repeat,
and the two tables are compared byte for byte.

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


def conserved_dataset(n_reads, n_genes=100, glen=1500, seed=11):
    """n_genes unrelated random genes that share four exact blocks of 60 bases; n_reads segments of 150 bases from the genes,
    1 % substitutions, either strand.  A segment that holds a whole block (about one in two) has an exact common stretch of
    60 bases with every gene: a hit at the default thresholds."""
    import random
    rng = random.Random(seed)
    comp = str.maketrans("ACGT", "TGCA")
    blocks = ["".join(rng.choice("ACGT") for _ in range(60)) for _ in range(4)]
    genes = []
    for _ in range(n_genes):
        g = "".join(rng.choice("ACGT") for _ in range(glen))
        for b, p in zip(blocks, (200, 550, 900, 1250)):
            g = g[:p] + b + g[p + 60:]
        genes.append(g.encode())
    segs = []
    for _ in range(n_reads):
        g = genes[rng.randrange(n_genes)].decode()
        p = rng.randint(0, glen - 150)
        r = "".join(rng.choice([c for c in "ACGT" if c != x]) if rng.random() < 0.01 else x for x in g[p:p + 150])
        segs.append((r[::-1].translate(comp) if rng.random() < 0.5 else r).encode())
    return genes, segs


def profile_legs(a, genes, segs):
    """The whole gene_profile with and without the counts mode on the data set written as files."""
    import tempfile
    from rambl_amd import profile
    with tempfile.TemporaryDirectory() as d:
        fa, sam = os.path.join(d, "genes.fa"), os.path.join(d, "sample.sam")
        with open(fa, "w") as f:
            f.writelines(">gene%03d\n%s\n" % (k, g.decode()) for k, g in enumerate(genes))
        with open(sam, "w") as f:
            f.writelines("@SQ\tSN:gene%03d\tLN:%d\n" % (k, len(g)) for k, g in enumerate(genes))
            f.writelines("r%d\t0\tgene000\t1\t42\t%dM\t*\t0\t0\t%s\t%s\n" % (k, len(s), s.decode(), "I" * len(s)) for k, s in enumerate(segs))
        tables = {}
        for k in range(-a.warmup, a.repeat):
            for counts in (False, True):
                out = os.path.join(d, "counts" if counts else "hits")
                t0 = time.perf_counter()
                path, st = profile.gene_profile(fa, sam, "s", a.identity, a.evalue, out_dir=out, device=a.device, seeded=a.seeded, counts_only=counts)
                wall = time.perf_counter() - t0
                tables[counts] = open(path, "rb").read()
                if k < 0:
                    continue
                extra = {"rounds": int(st.n_rounds), "stretches": int(st.n_stretches), "reads_counted": int(st.n_reads_counted),
                         "select_ms": round(st.select_ms, 3), "count_ms": round(st.count_ms, 3)} if counts else {}
                if a.seeded:
                    extra.update({"seed_k": int(st.seed_k), "pairs": int(st.n_pairs), "index_ms": round(st.index_ms, 3), "lookup_ms": round(st.lookup_ms, 3)})
                print(json.dumps({
                    "repeat": k, "leg": "gene_profile", "counts": counts, "seeded": bool(a.seeded), "data": a.data, "segments": len(segs),
                    "genes": len(genes), "tiles": int(st.n_tiles), "candidates": int(st.n_candidates), "traced": int(st.n_traced),
                    "hits": int(st.n_hits), "hit_density": st.n_candidates / (len(segs) * len(genes)), **extra,
                    "upload_ms": round(st.upload_ms, 3), "score_ms": round(st.score_ms, 3), "trace_ms": round(st.trace_ms, 3),
                    "call_ms": round(st.total_ms, 3), "wall_s": round(wall, 3)}), flush=True)
        assert tables[True] == tables[False], "the counts mode wrote another table"


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
    ap.add_argument("--conserved", action="store_true", help="100 genes that share exact blocks: most segments hit most genes")
    ap.add_argument("--profile", action="store_true", help="time profile.gene_profile end to end, without and with the counts mode")
    a = ap.parse_args(argv)
    a.data = "conserved" if a.conserved else "related" if a.related else "default"
    genes, segs = conserved_dataset(a.reads) if a.conserved else related_dataset(a.reads) if a.related else dataset(a.reads)[:2]
    if a.profile:
        return profile_legs(a, genes, segs)
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
            "repeat": k, "data": a.data, "seeded": bool(a.seeded), **extra, "segments": len(segs), "genes": len(genes), "tiles": int(st.n_tiles), "candidates": int(st.n_candidates),
            "traced": int(st.n_traced), "hits": int(st.n_hits),
            "score_ms": round(st.score_ms, 3), "score_cells_per_s": st.score_cells / (st.score_ms / 1e3),
            "score_pairs_per_s": pairs / (st.score_ms / 1e3), "score_hits_per_s": st.n_hits / (st.score_ms / 1e3),
            "trace_ms": round(st.trace_ms, 3), "trace_cells_per_s": st.trace_cells / max(st.trace_ms / 1e3, 1e-9),
            "trace_pairs_per_s": st.n_traced / max(st.trace_ms / 1e3, 1e-9), "trace_hits_per_s": st.n_hits / max(st.trace_ms / 1e3, 1e-9),
            "upload_ms": round(st.upload_ms, 3), "call_ms": round(st.total_ms, 3), "wall_s": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
