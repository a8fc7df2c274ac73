"""What a cohort call saves: 16 samples against the genes of tools/stage4_bench.py's data set (100 genes of
1 500 bp, segments of 150 bp from strains and relatives of the genes), profiled three ways in every repeat, one after the
other so that what else runs on the host hits them alike:

    loop    capi.profile_counts once per sample: the genes uploaded (and, seeded, indexed) and the arrays allocated 16 times
    fresh   one capi.ProfileIndex created, one counts() call with all samples, the index freed
    warm    the same call on an index that has served it before

    python tools/cohort_bench.py [--size small|full|both] [--samples 16] [--seeded] [--repeat K] [--warmup W]

small: about 500 segments per sample; full: 20 000, a sample's size in tools/profile_bench.py.  One JSON line per leg and repeat
after W unreported warm-up rounds: the wall time (a host clock around calls that end in a device synchronise) and the sums of
the calls' own statistics.  The three legs' rows are compared before anything is timed.
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

SIZES = {"small": 500, "full": 20000}
SUMMED = ("upload_ms", "index_ms", "lookup_ms", "score_ms", "select_ms", "trace_ms", "count_ms", "n_stretches", "n_rounds", "n_traced",
          "n_reads_counted")


def flat(samples):
    """The samples' segments back to back: every segment its own read, a sample per read."""
    segs = [s for smp in samples for s in smp]
    return segs, list(range(len(segs))), [k for k, smp in enumerate(samples) for _ in smp]


def summed(stats):
    out = {f: 0 for f in SUMMED}
    for st in stats:
        for f in SUMMED:
            out[f] += getattr(st, f)
    return {f: round(v, 3) if isinstance(v, float) else int(v) for f, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", choices=("small", "full", "both"), default="both")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--seeded", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    for size in (("small", "full") if a.size == "both" else (a.size,)):
        per = SIZES[size]
        genes, segs = dataset(per * a.samples)[:2]
        samples = [segs[k * per:(k + 1) * per] for k in range(a.samples)]
        call = flat(samples)
        kw = dict(device=a.device, seeded=a.seeded)

        def loop():
            t0 = time.perf_counter()
            res = [capi.profile_counts(genes, smp, list(range(len(smp))), **kw) for smp in samples]
            wall = time.perf_counter() - t0
            return wall, [(k,) + t for k, r in enumerate(res) for t in r.triples], [r.stats for r in res], None

        def fresh():
            t0 = time.perf_counter()
            with capi.ProfileIndex(genes, a.device) as ix:
                res = ix.counts(*call, a.samples, seeded=a.seeded)
            return time.perf_counter() - t0, res.rows, [res.stats], res.stats

        with capi.ProfileIndex(genes, a.device) as kept:
            def warm():
                t0 = time.perf_counter()
                res = kept.counts(*call, a.samples, seeded=a.seeded)
                return time.perf_counter() - t0, res.rows, [res.stats], res.stats

            legs = (("loop", loop), ("fresh", fresh), ("warm", warm))
            rows = {name: fn()[1] for name, fn in legs}
            assert rows["loop"] == rows["fresh"] == rows["warm"] and rows["loop"], "the legs disagree"
            for k in range(-a.warmup, a.repeat):
                for name, fn in legs:
                    wall, _, stats, cohort = fn()
                    if k < 0:
                        continue
                    extra = {} if cohort is None else {"n_allocs": int(cohort.n_allocs), "n_index_builds": int(cohort.n_index_builds)}
                    print(json.dumps({"repeat": k, "size": size, "leg": name, "seeded": bool(a.seeded), "samples": a.samples,
                                      "segments": len(call[0]), "genes": len(genes), "rows": len(rows[name]), "seed_k": int(stats[0].seed_k),
                                      "wall_ms": round(wall * 1e3, 3), "calls": len(stats), **summed(stats), **extra}), flush=True)


if __name__ == "__main__":
    main()
