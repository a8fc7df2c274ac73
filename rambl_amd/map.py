"""A sample's FASTQ reads mapped to the gene database on one MI355X GPU: the input of the pipeline.

Mirror of scripts/get_sra_and_mapping.py:49-90, which runs `bowtie2 --local -x <gene database>` and `samtools view -F4 -bht`,
`sort` and `index` per sample.  bowtie2's seed heuristics are replaced by a candidate rule a plain program can restate and
the exact optimum of bowtie2's --local scoring over the candidates, computed by sc_map_reads
(rambl_amd/csrc/sc_map.hip).  The result is SAM text that sc_aln_open reads: stages 1 and 4, the gene profile and the cohort
take it where they took the BAM file.  Where this differs from bowtie2: a read that lies wholly in sequence many genes share
can end without a candidate and stays unmapped; mates are aligned independently (0x2 is never set); MAPQ is 0 when XS = AS
and 42 otherwise, as in stage 4.
"""
import gzip
import logging
import os
import sys

from . import capi, samio
from .samio import sam_header  # noqa: F401  (a name of this module)

MAX_READ = 512
MAX_GENE = 8192
MAX_GENES = (1 << 20) - 1


class InputError(Exception):
    """What ends the command with exit status 2 before the GPU is touched."""


def open_text(path):
    """A binary reader of `path`, through gzip when the file starts with gzip's magic bytes."""
    f = open(path, "rb")
    magic = f.read(2)
    f.seek(0)
    if magic == b"\x1f\x8b":
        return gzip.GzipFile(fileobj=f)
    return f


def qname_of(header):
    """QNAME of a FASTQ header line (without the '@'): up to the first blank, without a trailing /1 or /2."""
    fields = header.split(None, 1)
    name = fields[0] if fields else b""
    if name.endswith((b"/1", b"/2")):
        name = name[:-2]
    return name


def read_fastq(path):
    """[(QNAME, SEQ, QUAL)] of a FASTQ file, plain or gzip, records of four lines.  InputError when the file cannot be read
    as that."""
    out = []
    try:
        with open_text(path) as f:
            lines = f.read().split(b"\n")
    except (OSError, EOFError) as e:
        raise InputError("%s: %s" % (path, e))
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise InputError("%s: %d lines, no whole number of four-line records" % (path, len(lines)))
    for k in range(0, len(lines), 4):
        head, seq, plus, qual = (x.rstrip(b"\r") for x in lines[k:k + 4])
        if not head.startswith(b"@") or not plus.startswith(b"+") or len(seq) != len(qual):
            raise InputError("%s: record %d is no FASTQ record" % (path, k // 4 + 1))
        out.append((qname_of(head[1:]), seq, qual))
    return out


def read_genes(path):
    """(names, sequences as bytes) of the gene FASTA in file order."""
    try:
        fa = samio.Fasta(path)
    except OSError as e:
        raise InputError("%s: %s" % (path, e))
    if not fa.order:
        raise InputError("%s: no sequence" % path)
    if len(set(fa.order)) != len(fa.order):
        raise InputError("%s: a sequence name occurs twice" % path)
    if len(fa.order) > MAX_GENES:
        raise InputError("%s: more than %d sequences" % (path, MAX_GENES))
    seqs = [fa.seqs[n].encode() for n in fa.order]
    for n, s in zip(fa.order, seqs):
        if not 1 <= len(s) <= MAX_GENE:
            raise InputError("%s: %s has %d bases (1..%d supported)" % (path, n, len(s), MAX_GENE))
    return fa.order, seqs


def read_sample(r1, r2=None):
    """The reads of a sample as [(QNAME, [(SEQ, QUAL), ...])]: one entry per record of `r1`, with its mate of `r2` when
    there is a second file (the two must have equal record counts; QNAME is mate 1's)."""
    a = read_fastq(r1)
    if r2 is None:
        return [(q, [(s, ql)]) for q, s, ql in a]
    b = read_fastq(r2)
    if len(a) != len(b):
        raise InputError("%s has %d records, %s has %d" % (r1, len(a), r2, len(b)))
    return [(q, [(s, ql), (s2, ql2)]) for (q, s, ql), (_, s2, ql2) in zip(a, b)]


class Mapped:
    """Per read entry of the sample, flattened (a pair's mates one after the other): gene (-1: unmapped), strand, pos, cigar,
    as_, xs, nm."""

    def __init__(self, n):
        self.gene = [-1] * n
        self.strand, self.pos, self.as_, self.xs, self.nm = ([0] * n for _ in range(5))
        self.cigar = ["*"] * n


def map_sample(index, sample, max_occ, max_cand, min_votes, pair_room=0):
    """sc_map_reads over the reads of `sample` that the library takes (1..512 bases); returns (Mapped, the number of reads left
    out for their length, the ScMapStats)."""
    flat = [m for _, mates in sample for m in mates]
    take = [i for i, (s, _) in enumerate(flat) if 1 <= len(s) <= MAX_READ]
    res = index.map_reads([flat[i][0] for i in take], [flat[i][1] for i in take], max_occ, max_cand, min_votes, pair_room)
    out = Mapped(len(flat))
    for k, i in enumerate(take):
        out.gene[i], out.strand[i], out.pos[i] = int(res.gene[k]), int(res.strand[k]), int(res.pos[k])
        out.as_[i], out.xs[i], out.nm[i], out.cigar[i] = int(res.as_[k]), int(res.xs[k]), int(res.nm[k]), res.cigar[k]
    return out, len(flat) - len(take), res.stats


def sam_records(sample, res, names):
    """The SAM lines of the mapped reads (-F4), sorted by (gene index, POS) stably over input order, mate 1 before mate 2.  A
    mapped read whose mate did not map is kept, with 0x8, RNEXT * and PNEXT 0."""
    return samio.sam_records(sample, res.gene, res.strand, res.pos, res.as_, res.xs, res.nm, res.cigar, names,
                             keep_lone_mate=True, sort_by_strand=False)


def parse_args(argv):
    import argparse
    d = capi.MAP_DEFAULTS
    ap = argparse.ArgumentParser(prog="rambl-map", description="Map a sample's FASTQ reads to the gene database (on the GPU)")
    ap.add_argument("fasta", metavar="GENE_FASTA", help="gene reference genome file")
    ap.add_argument("-1", dest="r1", help="FASTQ file of mate 1 (plain or gzip)")
    ap.add_argument("-2", dest="r2", help="FASTQ file of mate 2")
    ap.add_argument("-U", dest="single", help="FASTQ file of unpaired reads")
    ap.add_argument("-o", dest="out", required=True, metavar="SAMPLE.sam", help="the SAM file to write")
    ap.add_argument("-k", dest="seed_k", type=int, default=d["seed_k"], help="k-mer length, 11..16 (default: %d)" % d["seed_k"])
    ap.add_argument("--max-occ", type=int, default=d["max_occ"], help="a k-mer with more entries in the index casts no vote (default: %d)" % d["max_occ"])
    ap.add_argument("--max-cand", type=int, default=d["max_cand"], help="candidate genes per read, 0: all (default: %d)" % d["max_cand"])
    ap.add_argument("--min-votes", type=int, default=d["min_votes"], help="least votes of a candidate (default: %d)" % d["min_votes"])
    ap.add_argument("-c", "--core", dest="cores", type=int, default=1, help="number of computing cores (default: 1)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-v", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)                           # argparse itself leaves with status 2
    if (a.single is None) == (a.r1 is None) or (a.r2 is not None and a.r1 is None):
        ap.error("give either -1 R1.fastq [-2 R2.fastq] or -U reads.fastq")
    if not 11 <= a.seed_k <= 16:
        ap.error("-k %d: 11..16 supported" % a.seed_k)
    if a.max_occ < 1 or a.max_cand < 0 or a.min_votes < 1 or a.cores < 1 or a.device < 0:
        ap.error("--max-occ, --min-votes and -c must be 1 or more, --max-cand and --device 0 or more")
    return a


def main(argv=None):
    """`rambl-map GENE_FASTA -1 R1.fastq [-2 R2.fastq] | -U reads.fastq -o SAMPLE.sam`; exit status 2 for an input error."""
    a = parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO if a.verbose else logging.WARNING)
    try:
        for p in (a.fasta, a.r1, a.r2, a.single):
            if p is not None and not os.path.isfile(p):
                raise InputError("%s: no such file" % p)
        names, genes = read_genes(a.fasta)
        sample = read_sample(a.single, None) if a.single is not None else read_sample(a.r1, a.r2)
    except InputError as e:
        sys.stderr.write("rambl-map: %s\n" % e)
        return 2
    with capi.MapIndex(genes, a.seed_k, a.device) as index:
        res, n_left_out, stats = map_sample(index, sample, a.max_occ, a.max_cand, a.min_votes)
    lines = sam_records(sample, res, names)
    with open(a.out, "w") as f:
        f.write(sam_header(names, genes))
        f.writelines(lines)
    n_reads = sum(len(m) for _, m in sample)
    if n_left_out:
        logging.warning("%d of %d reads are empty or longer than %d bases and stay unmapped", n_left_out, n_reads, MAX_READ)
    logging.info("%d reads, %d mapped onto %d genes, %s", n_reads, len(lines), len(genes), stats.as_dict())
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
