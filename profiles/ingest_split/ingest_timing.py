"""Host-only timing of the native ingest: sc_aln_open on a SAM text, sc_aln_open on the BAM written from it, and one
sc_aln_load_reads over the whole gene, on the 60 000-read synthetic gene of
tests/test_host_side.py::test_bam_of_many_bgzf_members_decodes_like_the_sam.  No GPU.

    ingest_timing.py make DIR          write DIR/reads.sam, DIR/reads.bam, DIR/gene.fa
    ingest_timing.py time LABEL ROOT DIR     one JSON line under LABEL: seconds of the three calls (median of five calls each)
                                             with the library of the checkout ROOT
    ingest_timing.py headline LABEL ROOT     one JSON line: ms of the host ingest of one bench.py headline step
                                             (parse_cmd_line + load_regions on its 10 000-read gene), median of 20 calls

Each `time` is a process of its own (it loads ROOT's library); SC_INGEST_THREADS comes from the environment.
"""
import json
import os
import sys
import time


def main():
    mode = sys.argv[1]
    if mode == "make":
        here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        sys.path[:0] = [here, os.path.join(here, "tests")]
        import sc_testlib as T
        from rambl_amd import synth
        d = sys.argv[2]
        os.makedirs(d, exist_ok=True)
        gene = synth.make_gene(7, glen=1500, n_strains=3, n_reads=60000, name="g7")
        fa, sam = synth.write_dataset(d, [gene])
        os.replace(sam, os.path.join(d, "reads.sam"))
        os.replace(fa, os.path.join(d, "gene.fa"))
        T.write_bam(os.path.join(d, "reads.sam"), os.path.join(d, "reads.bam"))
        return
    if mode == "headline":
        import tempfile
        label, root = sys.argv[2], os.path.abspath(sys.argv[3])
        sys.path.insert(0, root)
        from rambl_amd import capi, cli, stage5, synth
        capi.lib()
        with tempfile.TemporaryDirectory() as d:
            fa, sam = synth.write_dataset(d, [synth.make_gene(21, glen=1500, n_strains=3, n_reads=10000, name="gene21")])
            argv = stage5.straincall_argv("gene21:1-1500", fa, sam)
            ts = []
            for _ in range(25):                  # the first five calls warm up
                t = time.perf_counter()
                cli.load_regions(cli.parse_cmd_line(argv))
                ts.append(1e3 * (time.perf_counter() - t))
        print(json.dumps({"build": label, "headline_ingest_ms": sorted(ts[5:])[10]}))
        return
    label, root, d = sys.argv[2], os.path.abspath(sys.argv[3]), sys.argv[4]
    sys.path.insert(0, root)
    from rambl_amd import capi
    seq = open(os.path.join(d, "gene.fa")).read().split("\n", 1)[1].replace("\n", "")
    capi.lib()                                   # the library is loaded before the clock starts
    out = {"build": label, "threads": os.environ.get("SC_INGEST_THREADS", "default")}

    def median_of_5(fn):
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return sorted(ts)[2], r
    out["open_sam_s"], a = median_of_5(lambda: capi.NativeAln(os.path.join(d, "reads.sam")))
    out["open_bam_s"], b = median_of_5(lambda: capi.NativeAln(os.path.join(d, "reads.bam")))
    assert a.records() == b.records() == 60000
    out["load_reads_s"], r = median_of_5(lambda: a.load_reads(seq, "g7", 1, 1500, 0, 70, 13, 800))
    out["n_reads"] = len(r.pos)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
