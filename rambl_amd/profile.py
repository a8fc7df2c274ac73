"""After the assembly: how much of each assembled gene is in one sample, on one MI355X GPU.

Mirror of scripts/per_sample_gene_profile_fast.py (copy-number correction from a fixrank file of taxa.py, off by default
as with `-n`): the reads the sample's
alignment file mapped are extracted (extract_mapped_reads.cpp:29-105), searched in the assembled genes
(`makeblastdb` / `blastn -reward 1 -penalty -2`, :80-117), the hits turned into a CSV (`bigBlastParser` + `sqlite3`,
:120-153), counted (blastout2abundance.cpp:70-196) and written as `<sample>_gene_count.tsv` (:324-336).  blastn and the
tools around it are replaced by the exact optimum of blastn's scoring with a fixed tie-break, computed by
sc_profile_hits (rambl_amd/csrc/sc_profile.hip); the counting rule is the reference's, on the host, one pass over the hits.
With --counts the rule runs on the device over each read's best hits only (sc_profile_counts).
--copy-correct divides every count by its gene's copy number (copy_number_correct, :223-246).
"""
import decimal
import math
import os
from fractions import Fraction

from . import capi

# Karlin-Altschul parameters of blastn's 1/-2 scoring with linear gaps, as NCBI tabulates them -- written down from memory
# and NOT checked against BLAST or its tables, which this project never had at hand.  Override them with --ka-lambda / --ka-k
# where the tables are.
KA_LAMBDA = 1.28
KA_K = 0.46
MIN_IDENTITY = 95.0               # -I of the script
MAX_EVALUE = 1e-10                # -e of the script
SCRIPT_DEFAULTS = {"word_size": 22, "reward": 1, "penalty": -2, "max_num_align": 30}


def extract_segments(records):
    """The query segments of extract_mapped_reads.cpp:29-105 from (QNAME, FLAG, SEQ, QUAL) records in file order: records
    with 0x4 or without SEQ are skipped; a QNAME ending in /1 or /2 loses the suffix; per name a 0x40 record sets the first
    segment, a 0x80 record the second, any other record the first, the last record of a kind winning; SEQ as stored (both
    strands are searched).  A name with both segments gives name/1 and name/2, any other name one segment under the name.
    Returns [(segment id, SEQ)] (bytes) ordered by name bytes, /1 before /2."""
    pool = {}
    for q, flag, seq, _ in records:
        if flag & 0x4 or seq == b"*" or not seq:
            continue
        if q[-2:] in (b"/1", b"/2"):
            q = q[:-2]
        ent = pool.setdefault(q, [None, None])
        ent[1 if (flag & 0x80 and not flag & 0x40) else 0] = seq
    out = []
    for q in sorted(pool):
        first, second = pool[q]
        if first is not None and second is not None:
            out.append((q + b"/1", first))
            out.append((q + b"/2", second))
        else:
            out.append((q, first if first is not None else second))
    return out


def format_evalue(e):
    """An E-value as the hit CSV holds it: six significant digits."""
    return "%.6g" % e


def hit_rows(hits, seg_ids, seg_lens, gene_names):
    """The ten columns the script's SQL selects (:142), one tuple of text per hit: segment id, gene, identity, align_len,
    query from, query to, hit from, hit to, E-value, segment length.  `hits`: capi.ProfileHits."""
    rows = []
    for k in range(len(hits)):
        s = int(hits.seg[k])
        rows.append((seg_ids[s], gene_names[int(hits.gene[k])], str(int(hits.identity[k])), str(int(hits.align_len[k])),
                     str(int(hits.qfrom[k])), str(int(hits.qto[k])), str(int(hits.hfrom[k])), str(int(hits.hto[k])),
                     format_evalue(float(hits.evalue[k])), str(int(seg_lens[s]))))
    return rows


def hits_csv(rows):
    """The rows as the CSV blastout2abundance reads (comma-separated, no header, no quoting: a name with a comma is not
    representable there either)."""
    return "".join(",".join(r) + "\n" for r in rows)


def parse_hits_csv(text):
    return [tuple(line.split(",")) for line in text.splitlines() if line]


def raw_abundance(rows, min_identity=MIN_IDENTITY, max_evalue=MAX_EVALUE):
    """blastout2abundance.cpp:70-196 on rows (segment id, gene, identity, align_len, qfrom, qto, hfrom, hto, evalue, segment
    length; text or numbers): a row with 100 * identity / align_len < min_identity or evalue > max_evalue is skipped, then a
    row whose (segment, gene) was seen before; a segment id ending in /1 .1 /2 .2 belongs to the read without the suffix (an
    id shorter than two characters, on which the reference throws, is its own read); per read the hits at the smallest
    E-value are kept (a strictly smaller one restarts the list, an equal one appends); the genes hit most often among them
    share the read, each getting times_hit / number_of_such_genes.  Returns [(gene, Fraction)] in byte order of the gene."""
    seen = set()
    reads = {}                                   # read -> [smallest E, [genes hit at it]]
    for row in rows:
        seg, gene = row[0], row[1]
        identity, align_len, evalue = float(row[2]), float(row[3]), float(row[8])
        if identity * 100 / align_len < min_identity or evalue > max_evalue:
            continue
        read = seg[:-2] if len(seg) >= 2 and seg[-2:] in ("/1", ".1", "/2", ".2") else seg
        if (seg, gene) in seen:
            continue
        seen.add((seg, gene))
        ent = reads.get(read)
        if ent is None or ent[0] > evalue:
            reads[read] = [evalue, [gene]]
        elif ent[0] == evalue:
            ent[1].append(gene)
    total = {}
    for _, genes in reads.values():
        times = {}
        for g in genes:
            times[g] = times.get(g, 0) + 1
        most = max(times.values())
        share = [g for g, n in times.items() if n == most]
        for g in share:
            total[g] = total.get(g, 0) + Fraction(most, len(share))
    return sorted(total.items(), key=lambda kv: kv[0].encode() if isinstance(kv[0], str) else kv[0])


def read_index(seg_ids):
    """The read of every segment by the counting rule's grouping: an id ending in /1 .1 /2 .2 belongs to the read without
    the suffix, an id shorter than two characters is its own read.  Returns (one read index per segment, number of reads);
    reads are numbered in order of first appearance."""
    reads, out = {}, []
    for seg in seg_ids:
        read = seg[:-2] if len(seg) >= 2 and seg[-2:] in ("/1", ".1", "/2", ".2") else seg
        out.append(reads.setdefault(read, len(reads)))
    return out, len(reads)


def counts_from_triples(triples, gene_names):
    """[(gene, Fraction)] in byte order of the gene, as raw_abundance returns it, from the (gene index, times_hit,
    number_of_such_genes, reads) of capi.profile_counts: every read behind a triple gives its gene times_hit /
    number_of_such_genes."""
    total = {}
    for gene, times, share, n in triples:
        g = gene_names[gene]
        total[g] = total.get(g, 0) + n * Fraction(times, share)
    return sorted(total.items(), key=lambda kv: kv[0].encode() if isinstance(kv[0], str) else kv[0])


def format_raw(counts):
    """What the reference's counter prints: `gene<TAB>count`, the count as `cout` prints a long double (6 significant digits)."""
    return "".join("%s\t%g\n" % (g, float(v)) for g, v in counts)


def _round_half_away(x, digits):
    """round(x, digits) of the interpreter the script was written for (Python 2): correctly rounded, halves away from zero."""
    q = decimal.Decimal(1).scaleb(-digits)
    return float(decimal.Decimal(x).quantize(q, rounding=decimal.ROUND_HALF_UP))


def format_table(sample, counts, relative=False):
    """`<sample>_gene_count.tsv` (:324-336): header `sample<TAB><sample>`, one line per gene in byte order; the value rounded
    to 3 decimals, or with `relative` divided by the column sum and rounded to 9, printed with repr (what pandas writes)."""
    vals = [(g, float(v)) for g, v in counts]
    if relative:
        s = math.fsum(v for _, v in vals)
        vals = [(g, _round_half_away(v / s, 9)) for g, v in vals]
    else:
        vals = [(g, _round_half_away(v, 3)) for g, v in vals]
    return "sample\t%s\n" % sample + "".join("%s\t%r\n" % (g, v) for g, v in vals)


def gene_profile(fasta, aln_path, sample, min_identity=MIN_IDENTITY, max_evalue=MAX_EVALUE, relative=False, ka_lambda=KA_LAMBDA,
                 ka_k=KA_K, out_dir=".", device=0, keep_hits=False, verbose=False, seeded=False, counts_only=False, copy_correct=None):
    """per_sample_gene_profile (:253-279) and the table of main (:324-336) for one sample.  Writes
    <out_dir>/<sample>_gene_count.tsv (and <sample>_hits.csv with `keep_hits`); returns the table path and the
    sc_profile_stats of the device call(s).  seeded: only the (segment, gene) pairs that share a k-mer are scored
    (sc_profile_hits_seeded): the same hits, the same files.  counts_only: the table comes from
    sc_profile_counts, which picks, traces and counts only each read's best hits on the device: the same
    table, no hit list (so no `keep_hits`); the statistics are sc_profile_count_stats.  copy_correct: None, or (fixrank path,
    copy-number table path, threshold): every count is divided by its gene's copy number before it is rounded
    (copy_number_correct, :223-246; the fixrank file comes from `rambl-taxa classify`)."""
    if counts_only and keep_hits:
        raise ValueError("there is no hit list in the counts mode")
    from . import samio

    correction = None
    if copy_correct is not None:                                # read before the device's work: a mistyped path fails at once
        from . import taxa
        with open(copy_correct[0]) as f:
            correction = (taxa.parse_fixrank(f.read()), taxa.load_copy_numbers(copy_correct[1]), copy_correct[2])

    def corrected(counts):
        return counts if correction is None else taxa.correct_counts(counts, *correction)

    fa = samio.Fasta(fasta)
    if not fa.order:
        raise ValueError("%s holds no gene" % fasta)
    genes = [fa.seqs[n].encode() for n in fa.order]
    aln = capi.NativeAln(aln_path)
    try:
        segments = extract_segments(aln.walk())
    finally:
        aln.close()
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, sample + "_gene_count.tsv")
    if counts_only:
        seg_read, n_reads = read_index([q.decode() for q, _ in segments])
        res = capi.profile_counts(genes, [s for _, s in segments], seg_read, min_identity, max_evalue, ka_lambda, ka_k, device, seeded=seeded)
        counts = corrected(counts_from_triples(res.triples, fa.order))
        with open(path, "w") as f:
            f.write(format_table(sample, counts, relative))
        if verbose:
            import logging
            st = res.stats
            logging.info("profile of %s (counts): %d segments of %d reads against %d genes, %d of %d candidates traced in %d rounds over %d "
                         "stretches, %d reads counted, %d genes counted, %s", sample, len(segments), n_reads, len(genes), st.n_traced,
                         st.n_candidates, st.n_rounds, st.n_stretches, st.n_reads_counted, len(counts), st.as_dict())
        return path, res.stats
    hits = capi.profile_hits(genes, [s for _, s in segments], min_identity, max_evalue, ka_lambda, ka_k, device, seeded=seeded)
    rows = hit_rows(hits, [q.decode() for q, _ in segments], [len(s) for _, s in segments], fa.order)
    counts = corrected(raw_abundance(rows, min_identity, max_evalue))
    if keep_hits:
        with open(os.path.join(out_dir, sample + "_hits.csv"), "w") as f:
            f.write(hits_csv(rows))
    with open(path, "w") as f:
        f.write(format_table(sample, counts, relative))
    if verbose:
        import logging
        logging.info("profile of %s: %d segments against %d genes, %d hits, %d genes counted, %s", sample, len(segments), len(genes),
                     len(rows), len(counts), hits.stats.as_dict())
        if seeded:
            full = len(segments) * len(genes)
            logging.info("seeded: seed_k %d%s, %d (segment, gene) pairs scored, %.4g %% of the full product of %d", hits.stats.seed_k,
                         "" if hits.stats.seed_k else " (ran unseeded)", hits.stats.n_tiles // 2, 100.0 * (hits.stats.n_tiles // 2) / max(full, 1), full)
    return path, hits.stats


def main(argv=None):
    """`python -m rambl_amd.profile GENE_SEQ SAMPLE_BAM SAMPLE_NAME [-c N] [-e E] [-I PCT] [-n] [-r] [-v]`, the argv of
    per_sample_gene_profile_fast.py."""
    import argparse
    import logging
    ap = argparse.ArgumentParser(description="Number of read hits per assembled gene for one sample (hits computed on the GPU)")
    ap.add_argument("fasta", metavar="GENE_SEQ", help="gene sequences")
    ap.add_argument("bam", metavar="SAMPLE_BAM", help="sample reads (SAM text or BAM)")
    ap.add_argument("sample", metavar="SAMPLE_NAME", help="sample name")
    ap.add_argument("-c", "--cores", dest="cores", type=int, default=1, help="CPU cores of the alignment-file reader [1]")
    ap.add_argument("-w", "--word-size", dest="word_size", type=int, default=22, help="only 22, and no word of that size is looked for: blastn's seeding loses hits. --seeded is the lossless counterpart")
    ap.add_argument("--seeded", dest="seeded", action="store_true",
                    help="score only the (segment, gene) pairs that share a k-mer, k chosen so that no hit is lost: the same output, less work")
    ap.add_argument("-R", "--reward", dest="reward", type=int, default=1, help="only 1")
    ap.add_argument("-P", "--penalty", dest="penalty", type=int, default=-2, help="only -2")
    ap.add_argument("-e", "--e-value", dest="e_value", type=float, default=MAX_EVALUE, help="e-value threshold [1e-10]")
    ap.add_argument("-A", "--max_num_alignments", dest="max_num_align", type=int, default=30, help="only 30: no cap is applied")
    ap.add_argument("-I", "--max_identity", dest="max_align_iden", type=float, default=MIN_IDENTITY, help="least alignment identity in percent [95]")
    ap.add_argument("-n", "--ignore-copy-correct", dest="ignore_copy_correct", action="store_true",
                    help="no copy number correction (the default; --copy-correct turns it on)")
    ap.add_argument("-C", "--rdp-classifier", dest="rdp_classifier", default=None, help="not available")
    ap.add_argument("-t", "--thresh", dest="thresh", type=float, default=None, help="not available")
    ap.add_argument("--copy-correct", dest="copy_correct", default=None, metavar="FIXRANK",
                    help="divide every gene's count by its copy number: the genes' fixrank file from `rambl-taxa classify` (needs --copy-number)")
    ap.add_argument("--copy-number", dest="copy_number", default=None, metavar="TSV", help="copy numbers per taxon: columns `name` and `mean` (rrnDB)")
    ap.add_argument("--copy-thresh", dest="copy_thresh", type=float, default=None, help="least bootstrap confidence of a rank that corrects [0.6]")
    ap.add_argument("-r", "--rel", dest="relative_abundance", action="store_true", help="output relative abundance")
    ap.add_argument("--ka-lambda", dest="ka_lambda", type=float, default=KA_LAMBDA, help="Karlin-Altschul lambda [%g]" % KA_LAMBDA)
    ap.add_argument("--ka-k", dest="ka_k", type=float, default=KA_K, help="Karlin-Altschul K [%g]" % KA_K)
    ap.add_argument("-o", "--out-dir", dest="out_dir", default=".", help="where <sample>_gene_count.tsv goes")
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("--keep-hits", dest="keep_hits", action="store_true", help="also write <sample>_hits.csv, the input of blastout2abundance")
    ap.add_argument("--counts", dest="counts", action="store_true",
                    help="choose, trace and count only each read's best hits on the GPU: the same table without the hit list (can be "
                         "combined with --seeded, not with --keep-hits)")
    ap.add_argument("-v", "--verbose", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    if a.rdp_classifier is not None or a.thresh is not None:
        ap.error("copy number correction (-C / -t) needs the RDP classifier and is not built: the tool behaves as the script does with -n")
    if (a.copy_correct is None) != (a.copy_number is None):
        ap.error("--copy-correct FIXRANK and --copy-number TSV go together")
    if a.copy_thresh is not None and a.copy_correct is None:
        ap.error("--copy-thresh needs --copy-correct")
    if a.copy_correct is not None and a.ignore_copy_correct:
        ap.error("--copy-correct cannot be combined with -n")
    if a.counts and a.keep_hits:
        ap.error("--counts cannot be combined with --keep-hits: there is no hit list in this mode")
    given = {"word_size": a.word_size, "reward": a.reward, "penalty": a.penalty, "max_num_align": a.max_num_align}
    if given != SCRIPT_DEFAULTS:
        ap.error("only -w 22 -R 1 -P -2 -A 30 is available: the hits are the exact optimum of that scoring, computed on the GPU "
                 "without word seeding or a cap on alignments (got -w %d -R %d -P %d -A %d)" % (a.word_size, a.reward, a.penalty, a.max_num_align))
    os.environ["SC_INGEST_THREADS"] = str(max(1, min(a.cores, capi.host_plan(1)[2])))
    gene_profile(a.fasta, a.bam, a.sample, a.max_align_iden, a.e_value, a.relative_abundance, a.ka_lambda, a.ka_k, a.out_dir, a.device,
                 a.keep_hits, a.verbose, a.seeded, a.counts,
                 None if a.copy_correct is None else (a.copy_correct, a.copy_number, 0.6 if a.copy_thresh is None else a.copy_thresh))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
