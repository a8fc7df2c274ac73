"""Stage 4 of rambl.py (re-cluster the gene reads to the seed OTUs) on one MI355X GPU.

Mirror of scripts/recluster_data_to_seed_otus.py:198-277: the seed OTUs are cut out of the gene FASTA
(`samtools faidx`, :85-89), the reads the gene-database BAMs mapped are extracted (extract_reads.py:46-112), aligned
again to the seeds (`bowtie2 --sensitive-local`, :117-169), filtered like `samtools view -F1804` and sorted into
to_seed_otus.all (:40-55, :262-272).  bowtie2 and samtools are replaced by the exact optimum of bowtie2's --local
scoring with a fixed tie-break, computed by sc_align_reads (rambl_amd/csrc/sc_align.hip), and the
result is written as SAM text, which stage 5 (rambl_amd/stage5.py, bin/StrainCall) reads as it is.
"""
import math
import os

from . import capi, samio
from .samio import revcomp, sam_header  # noqa: F401  (names of this module)

MAPPER = "bowtie2"
MAP_ARGS = "--sensitive-local"


def threshold(n):
    """--score-min G,20,8: the least valid local score of a read of n bases."""
    return 20.0 + 8.0 * math.log(n)


def read_seed_list(path):
    """First column of every non-empty line (recluster_data_to_seed_otus.py:208-212)."""
    out = []
    with open(path) as f:
        for line in f:
            items = line.rstrip().split()
            if items:
                out.append(items[0])
    return out


def read_bam_list(path):
    """One path per line (:226-229)."""
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def extract_reads(records):
    """The reads of extract_reads.py:46-112 from (QNAME, FLAG, SEQ, QUAL) records in file-list order: records with 0x4 are
    skipped, 0x10 records are turned back into the read as sequenced, a QNAME with a 0x40 and a 0x80 record is a pair, any
    other QNAME a single read (its last record); the last record of a kind wins.  Returns [(QNAME, [(SEQ, QUAL), ...])]
    sorted by QNAME bytes, one tuple for a single read, two (mate 1, mate 2) for a pair."""
    pool = {}
    for q, flag, seq, qual in records:
        if flag & 0x4 or seq == b"*":                 # unmapped, or no bases to align
            continue
        if flag & 0x10:
            seq = revcomp(seq)
            qual = qual if qual == b"*" else qual[::-1]
        kind = 1 if flag & 0x40 else (2 if flag & 0x80 else 0)
        ent = pool.setdefault(q, {})
        ent[kind] = (seq, qual)
        ent["last"] = (seq, qual)
    out = []
    for q in sorted(pool):
        ent = pool[q]
        if 1 in ent and 2 in ent:
            out.append((q, [ent[1], ent[2]]))
        else:
            out.append((q, [ent["last"]]))
    return out


def write_seed_fasta(gene_fasta, seeds, path, width=60):
    """`samtools faidx GENE_FASTA seeds... > path` and `samtools faidx path`: the seed records in seed-list order with
    60-column lines, and the .fai (name, length, offset, line bases, line bytes)."""
    fa = samio.Fasta(gene_fasta)
    missing = [s for s in seeds if s not in fa.seqs]
    if missing:
        raise ValueError("seed OTU %s is not in %s" % (missing[0], gene_fasta))
    seqs = []
    with open(path, "w") as f, open(path + ".fai", "w") as fai:
        off = 0
        for s in seeds:
            seq = fa.seqs[s]
            head = ">%s\n" % s
            body = "".join(seq[k:k + width] + "\n" for k in range(0, len(seq), width))
            f.write(head + body)
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (s, len(seq), off + len(head), width, width + 1))
            off += len(head) + len(body)
            seqs.append(seq.encode())
    return seqs


def sam_records(reads, res, seed_names):
    """The SAM lines of the aligned reads in the contract's order: reads that do not align and pairs with a mate that does
    not align are dropped (-F1804), the rest sorted by (seed, POS, reverse) stably over QNAME order, mate 1 before mate 2.
    `res` holds one alignment per read entry of `reads` flattened (a pair's mates one after the other)."""
    return samio.sam_records(reads, res.seed, res.strand, res.pos, res.as_, res.xs, res.nm, res.cigar, seed_names,
                             keep_lone_mate=False, sort_by_strand=True)


def recluster(gene_fasta, seed_file, bam_file, out_dir=".", mapper=MAPPER, map_args=MAP_ARGS, device=0, verbose=False, alns=None):
    """recluster_data (:198-277).  Writes <out_dir>/0_otu_dir/seed_otus.fasta(.fai) and <out_dir>/to_seed_otus.all.sam;
    returns the SAM path and the sc_align_stats of the device call.  `alns`: the files of `bam_file` already opened
    (capi.NativeAln, in list order; the caller keeps and closes them) -- the whole-pipeline driver reads them once for
    stages 1 and 4."""
    if mapper != MAPPER or map_args != MAP_ARGS:
        raise ValueError("stage 4 computes bowtie2 %s alignments on the GPU; mapper %r with arguments %r is not available "
                         "(only -m %s -A %s)" % (MAP_ARGS, mapper, map_args, MAPPER, MAP_ARGS))
    seeds = read_seed_list(seed_file)
    otu_dir = os.path.join(out_dir, "0_otu_dir")
    os.makedirs(otu_dir, exist_ok=True)
    seed_seqs = write_seed_fasta(gene_fasta, seeds, os.path.join(otu_dir, "seed_otus.fasta"))

    def records():
        if alns is not None:
            for aln in alns:
                for r in aln.walk():
                    yield r
            return
        for path in read_bam_list(bam_file):
            aln = capi.NativeAln(path)
            try:
                for r in aln.walk():
                    yield r
            finally:
                aln.close()
    reads = extract_reads(records())
    flat_seq = [m[0] for _, mates in reads for m in mates]
    flat_qual = [m[1] for _, mates in reads for m in mates]
    res = capi.align_reads(seed_seqs, flat_seq, flat_qual, device)
    sam = os.path.join(out_dir, "to_seed_otus.all.sam")
    with open(sam, "w") as f:
        f.write(sam_header(seeds, seed_seqs))
        f.writelines(sam_records(reads, res, seeds))
    if verbose:
        import logging
        logging.info("stage 4: %d reads (%d aligned) onto %d seed OTUs, %s", len(flat_seq), int(res.stats.n_traced), len(seeds),
                     res.stats.as_dict())
    return sam, res.stats


def main(argv=None):
    """`python -m rambl_amd.stage4 GENE_FASTA SEED_OTUS BAM_FILES [-c N] [-v]`, the argv of recluster_data_to_seed_otus.py."""
    import argparse
    import logging
    ap = argparse.ArgumentParser(description="Re-cluster sequencing reads according to the given seed OTUs (on the GPU)")
    ap.add_argument("fasta", metavar="GENE_FASTA", help="gene reference genome file")
    ap.add_argument("otu", metavar="SEED_OTUS", help="a list of seed OTUs, one OTU one line")
    ap.add_argument("bams", metavar="BAM_FILES", help="a list of bam files, one file one line")
    ap.add_argument("-c", "--core", dest="cores", type=int, default=1, help="number of computing cores (default: 1)")
    ap.add_argument("-m", "--mapper", dest="mapper", default=MAPPER, help="mapping program (only bowtie2)")
    ap.add_argument("-A", "--map_args", dest="map_args", default=MAP_ARGS, help="mapping program arguments (only --sensitive-local)")
    ap.add_argument("-o", "--out-dir", dest="out_dir", default=".", help="where 0_otu_dir/ and to_seed_otus.all.sam go")
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("-v", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    if a.mapper != MAPPER or a.map_args != MAP_ARGS:
        ap.error("only -m %s -A %s is available: stage 4 computes those alignments on the GPU (got -m %s -A %s)"
                 % (MAPPER, MAP_ARGS, a.mapper, a.map_args))
    # the reader's inflate threads stay within -c and the rank's share of the host (sc_host_plan)
    os.environ["SC_INGEST_THREADS"] = str(max(1, min(a.cores, capi.host_plan(1)[2])))
    recluster(a.fasta, a.otu, a.bams, a.out_dir, a.mapper, a.map_args, a.device, a.verbose)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
