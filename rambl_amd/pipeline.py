"""The whole rambl pipeline from a data_info file, in one process on one MI355X GPU.

Mirror of scripts/rambl.py:205-287 (`rambl.py [-c cores] [-v] [-p prefix] data_info.txt`): the five stages and the length
filter, with rambl.py's argv, option mapping and file names, each stage a function call in this process
(stage1.depth_intervals, stage2.gene_abundance, stage3.find_seed_otus, stage4.recluster, stage5.strain_call +
stage5.seqtk_L) where the reference starts a script or a tool.  The driver adds nothing of its own to what a stage
computes: every file of the work directory equals what the stages' own command lines produce when chained by hand.

What differs from rambl.py: the process never changes its directory (the stages get paths, so relative paths of the
data_info file stay valid); the reads aligned to the seed genes are SAM text, to_seed_otus.all.sam, where the reference
has a BAM (stage4.py); `GeneTax` may be absent (the reference raises NameError then); a missing key or file is reported
before any GPU work; the alignment files of `BamFiles` are read once and serve stages 1 and 4; the exit status tells
whether the result is whole (0), a region failed or no seed gene was found (1), or the input was unusable (2).

--profile adds what the reference leaves to a script per sample: after the length filter the samples of `BamFiles` are
profiled against the assembled genes (cohort.cohort_profile) into <prefix>_profile/.  The alignment files
are read a second time for it: the profile needs SEQ of every mapped record, which stages 1 and 4 do not keep.
"""
import logging
import os
import random
import shutil
import sys
import time

from . import capi, stage1, stage2, stage3, stage4, stage5

KEYS = ("BamFiles", "GeneSeq", "GeneIndex", "GeneTree", "GeneTax", "GeneAlign")
OPTIONAL = ("GeneTax",)
STREAMS = 224                     # regions in flight on the GPU at most (stage5.main's default)
_NAME_CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


class DataInfoError(ValueError):
    pass


def parse_data_info(path):
    """rambl.py:52-79 -> {key: value}.  A line belongs to the key it starts with; the value is the text between the first
    `=` and the next, stripped; a key given twice keeps its last value; an absent key is ""."""
    data = dict.fromkeys(KEYS, "")
    with open(path) as f:
        for line in f:
            line = line.rstrip()
            for key in KEYS:
                if line.startswith(key):
                    parts = line.split("=")
                    if len(parts) < 2:
                        raise DataInfoError("%s: line %r has no '='" % (path, line))
                    data[key] = parts[1].strip()
                    break
    return data


def check_data(data, path="data_info"):
    """Every required key, and every file a stage will open, before any GPU work."""
    for key in KEYS:
        if not data[key]:
            if key in OPTIONAL:
                continue
            raise DataInfoError("%s: no %s" % (path, key))
        if not os.path.isfile(data[key]):
            raise DataInfoError("%s: %s = %s: no such file" % (path, key, data[key]))
    bams = stage4.read_bam_list(data["BamFiles"])
    if not bams:
        raise DataInfoError("%s: BamFiles = %s lists no file" % (path, data["BamFiles"]))
    for p in bams:
        if not os.path.isfile(p):
            raise DataInfoError("%s: %s listed in %s: no such file" % (path, p, data["BamFiles"]))
    return bams


def build_parser():
    """rambl.py:250-287, plus --device."""
    import argparse
    ap = argparse.ArgumentParser(prog="rambl", description="RAMBL: reference-based ribosome assembly -- full-length 16S rRNA genes "
                                 "of strains from metagenomics sequencing data, on one MI355X GPU",
                                 epilog="Example: rambl [options] data_info -v")
    ap.add_argument("data_info", help="data collection", metavar="DATA")
    ap.add_argument("-c", "--cores", help="number of computing cores [1]", default=1, type=int, dest="cores", metavar="INT")
    ap.add_argument("-D", "--max-depth", help="downsample data to the specified depth [800]", default=800, type=int,
                    dest="max_depth", metavar="INT")
    ap.add_argument("-q", "--map-qual", help="only include reads with mapping quality >= INT [0]", default=0, type=int,
                    dest="map_qual", metavar="INT")
    ap.add_argument("-i", "--max-ins", help="only include reads with insert length <= INT [13]", default=13, type=int,
                    dest="max_ins", metavar="INT")
    ap.add_argument("-l", "--read-len", help="only include reads with length >= INT [70]", default=70, type=int,
                    dest="read_len", metavar="INT")
    ap.add_argument("-t", "--tau", help="only include strains with abundance level >= FLT [0.02]", default=0.02, type=float,
                    dest="tau", metavar="FLT")
    ap.add_argument("-d", "--diff-rate", help="only include strains with difference rate >= FLT [0.02]", default=0.02, type=float,
                    dest="diff_rate", metavar="FLT")
    ap.add_argument("-g", "--gene-similarity", help="used in finding seed gene, merge genes with similarity >= FLT [0.9]",
                    default=0.9, type=float, dest="gene_sim", metavar="FLT")
    ap.add_argument("-K", "--clade-coverage", help="used in finding seed gene, the portion of clade covered by reads >= FLT [0.9]",
                    default=0.9, type=float, dest="clade_coverage", metavar="FLT")
    ap.add_argument("-A", "--clade-depth", help="used in finding seed gene, gene depth sum of a clade >= INT [1]", default=1,
                    type=int, dest="clade_depth", metavar="INT")
    ap.add_argument("-p", "--prefix", help="output filename prefix [16S_gene_assembly]", default="16S_gene_assembly",
                    dest="prefix", metavar="STR")
    ap.add_argument("-R", dest="keep", action="store_true", default=False, help="keep intermediate files")
    ap.add_argument("-v", dest="verbose", action="store_true", default=False, help="verbose output")
    ap.add_argument("--device", help="the GPU to run on [0]", default=0, type=int, dest="device", metavar="N")
    # (absent from the parsed options unless given: what rambl.py's own argv parses to stays what it was)
    ap.add_argument("--profile", dest="profile", action="store_true", default=argparse.SUPPRESS,
                    help="after the assembly, count the reads of every sample per assembled gene: <prefix>_profile/ with one table per "
                         "sample (named after its file) and the sample x gene matrix")
    ap.add_argument("--profile-seeded", dest="profile_seeded", action="store_true", default=argparse.SUPPRESS,
                    help="with --profile: score only the (segment, gene) pairs that share a k-mer (the same tables, less work)")
    return ap


def stage3_kwargs(opts, data):
    """rambl.py:122-143: -g is find_seed_otus.py's -s, -K its -c, -A its -d; -T when the data_info file names a taxonomy."""
    return dict(sim_thres=float(opts.gene_sim), gene_cover=float(opts.clade_coverage), depth_thres=float(opts.clade_depth),
                taxonomy=data["GeneTax"] or None)


def stage5_opts(opts):
    """The options rambl.py:181-187 hands to StrainCall (stage5.straincall_argv forms the argv, window 5000 included)."""
    return {k: getattr(opts, k) for k in stage5.RAMBL_DEFAULTS}


def make_work_dir(parent):
    """RAMBL_work_dir_<5 random characters> under `parent` (rambl.py:208-213; a name in use is never taken over)."""
    rng = random.SystemRandom()
    while True:
        d = os.path.join(parent, "RAMBL_work_dir_%s" % "".join(rng.sample(_NAME_CHARS, 5)))
        try:
            os.mkdir(d)
            return d
        except FileExistsError:
            continue


def profile_dir(result):
    """<prefix>_profile next to <prefix>.fa"""
    return os.path.splitext(result)[0] + "_profile"


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)


def run(opts, data, bams, cwd=None):
    """rambl_pipe (rambl.py:205-243) -> (exit status, [(stage, wall seconds)], work directory)."""
    cwd = cwd or os.getcwd()
    times = []

    def timed(what, fn):
        t0 = time.perf_counter()
        out = fn()
        times.append((what, time.perf_counter() - t0))
        if opts.verbose:
            logging.info("%s: %.3f s", what, times[-1][1])
        return out

    work = make_work_dir(cwd)
    result = os.path.join(cwd, "%s.fa" % opts.prefix)
    depth_file = os.path.join(work, "gene_depth.txt")
    abun_file = os.path.join(work, "gene_abundance.txt")
    seed_file = os.path.join(work, "seed_gene.txt")
    # host threads stay within -c and this process's share of the host (sc_host_plan), as under stage4.main / stage5.main
    old_threads = os.environ.get("SC_INGEST_THREADS")
    os.environ["SC_INGEST_THREADS"] = str(max(1, min(opts.cores, capi.host_plan(1)[2])))
    alns = []
    try:
        try:
            def depth():
                for p in bams:                  # each file is read here, once, for stages 1 and 4
                    alns.append(capi.NativeAln(p))
                iv, _ = stage1.depth_intervals(bams, data["GeneIndex"], device=opts.device, alns=alns)
                _write(depth_file, stage1.bed_text(iv))
            timed("profile sequencing depths", depth)
            timed("compute gene abundance",
                  lambda: _write(abun_file, "".join(ln + "\n" for ln in stage2.gene_abundance(depth_file, data["GeneIndex"]))))
            seeds = timed("find seed genes",
                          lambda: stage3.find_seed_otus(data["GeneTree"], abun_file, depth_file, data["GeneIndex"], data["GeneAlign"],
                                                        **stage3_kwargs(opts, data)))
            _write(seed_file, "".join(ln + "\n" for ln in seeds))
            if not seeds:
                sys.stderr.write("rambl: no seed gene: no clade reaches depth %s over %s of its length; %s is empty\n"
                                 % (opts.clade_depth, opts.clade_coverage, result))
                _write(result, "")
                return 1, times, work
            timed("map gene reads to seed genes",
                  lambda: stage4.recluster(data["GeneSeq"], seed_file, data["BamFiles"], out_dir=work, device=opts.device,
                                           verbose=opts.verbose, alns=alns))
        finally:
            for a in alns:                      # before stage 5's context is created
                a.close()
        fasta = os.path.join(work, "0_otu_dir", "seed_otus.fasta")
        streams = max(1, min(STREAMS, len(stage5.roi_list(fasta + ".fai"))))
        workers = max(1, min(opts.cores, capi.host_plan(streams)[2]))
        errors = []
        full = timed("strain-level assembly",
                     lambda: stage5.strain_call(fasta, os.path.join(work, "to_seed_otus.all.sam"), out_dir=work, prefix=opts.prefix,
                                                opts=stage5_opts(opts), device=opts.device, streams=streams, ingest_workers=workers,
                                                errors=errors))
        _write(result, stage5.seqtk_L(full, 400))               # rambl.py:236-238
        if getattr(opts, "profile", False):
            if os.path.getsize(result) == 0:
                logging.info("no assembled gene is left in %s: the samples are not profiled", result)
            else:
                from . import cohort
                timed("profile the samples",
                      lambda: cohort.cohort_profile(result, cohort.sample_names(bams), profile_dir(result), device=opts.device,
                                                    seeded=getattr(opts, "profile_seeded", False), verbose=opts.verbose))
        return (1 if errors else 0), times, work
    finally:
        if old_threads is None:
            os.environ.pop("SC_INGEST_THREADS", None)
        else:
            os.environ["SC_INGEST_THREADS"] = old_threads
        if not opts.keep:
            shutil.rmtree(work, ignore_errors=True)


def main(argv=None):
    """`python -m rambl_amd.pipeline DATA [options]` = `bin/rambl DATA [options]`: the argv of rambl.py."""
    t_start = time.time()
    ap = build_parser()
    opts = ap.parse_args(argv)
    if getattr(opts, "profile_seeded", False) and not getattr(opts, "profile", False):
        ap.error("--profile-seeded needs --profile")
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    try:
        data = parse_data_info(opts.data_info)
        bams = check_data(data, opts.data_info)
        if getattr(opts, "profile", False):                     # two samples of one name: known before any GPU work
            from . import cohort
            cohort.sample_names(bams)
        status, _, _ = run(opts, data, bams)
    except (ValueError, OSError, capi.StrainCallError) as e:
        sys.stderr.write("rambl: error: %s\n" % e)
        return 2
    if opts.verbose:
        logging.info("elapsed time is {} minutes".format(round((time.time() - t_start) / 60., 5)))
    return status


if __name__ == "__main__":
    sys.exit(main())
