"""Wall time of a whole pipeline run (rambl_amd/pipeline.py) by stage, on the synthetic world of the pipeline tests
(tests/pipeline_lib.py) at a chosen size.

    python tools/pipeline_bench.py                      the GPU test's world: 3 clades, 700 bp genes, 900 reads each
    python tools/pipeline_bench.py --configs2           the configs[2] shape: 100 clades, 1 500 bp genes with 3 strains,
                                                        2 000 to 10 000 reads each

One JSON line: the world's size, the seconds of every stage as the driver's -v lines report them, their sum, the exit
status and the number of records of the result.  The first stage also pays for loading the code objects.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pipeline_lib  # noqa: E402
from rambl_amd import pipeline  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs2", action="store_true", help="100 clades of the configs[2] shape")
    ap.add_argument("--clades", type=int, default=None)
    ap.add_argument("-c", "--cores", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    kw = dict(n_clades=100, glen=1500, n_strains=3, n_reads=(2000, 10000), first_gene_seed=100, n_sub=45, n_ins=2, n_del=2) if a.configs2 else {}
    if a.clades is not None:
        kw["n_clades"] = a.clades
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        w = pipeline_lib.make_world(os.path.join(d, "world"), **kw)
        t_world = time.perf_counter() - t0
        opts = pipeline.build_parser().parse_args([w["data_info"], "-c", str(a.cores), "--device", str(a.device), "-p", "bench", "-v"])
        data = pipeline.parse_data_info(w["data_info"])
        import logging
        logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
        status, times, _ = pipeline.run(opts, data, pipeline.check_data(data), cwd=d)
        result = open(os.path.join(d, "bench.fa")).read()
    print(json.dumps({"clades": len(w["clades"]), "genes": 2 * len(w["clades"]) + 3, "gene_length": len(w["genes"][0]["ref"]),
                      "alignments": sum(len(v) for f in w["files"] for v in f.values()), "sample_files": len(w["bams"]),
                      "world_s": round(t_world, 3), "stages_s": {k: round(v, 3) for k, v in times}, "total_s": round(sum(v for _, v in times), 3),
                      "status": status, "records": result.count(">")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
