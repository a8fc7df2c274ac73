"""Throughput of the gene profile's hits on the device (sc_profile_hits): DP cell updates/s, (segment, gene) pairs/s and
hits/s of the score pass (k_bl_score) and of the traceback pass (k_bl_trace), on the data set of tools/stage4_bench.py:
100 genes of 1 500 bp, segments of 150 bp drawn from strains of the genes (1 % substitutions) and from relatives (3 %, 8 %
and 20 % divergent).

    python tools/profile_bench.py [--reads N] [--repeat K] [--warmup W]

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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--identity", type=float, default=95.0)
    ap.add_argument("--evalue", type=float, default=1e-10)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    genes, segs, _ = dataset(a.reads)
    for k in range(-a.warmup, a.repeat):
        t0 = time.perf_counter()
        res = capi.profile_hits(genes, segs, a.identity, a.evalue, device=a.device)
        wall = time.perf_counter() - t0
        if k < 0:
            continue
        st = res.stats
        pairs = len(segs) * len(genes)
        print(json.dumps({
            "repeat": k, "segments": len(segs), "genes": len(genes), "tiles": int(st.n_tiles), "candidates": int(st.n_candidates),
            "traced": int(st.n_traced), "hits": int(st.n_hits),
            "score_ms": round(st.score_ms, 3), "score_cells_per_s": st.score_cells / (st.score_ms / 1e3),
            "score_pairs_per_s": pairs / (st.score_ms / 1e3), "score_hits_per_s": st.n_hits / (st.score_ms / 1e3),
            "trace_ms": round(st.trace_ms, 3), "trace_cells_per_s": st.trace_cells / max(st.trace_ms / 1e3, 1e-9),
            "trace_pairs_per_s": st.n_traced / max(st.trace_ms / 1e3, 1e-9), "trace_hits_per_s": st.n_hits / max(st.trace_ms / 1e3, 1e-9),
            "upload_ms": round(st.upload_ms, 3), "call_ms": round(st.total_ms, 3), "wall_s": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
