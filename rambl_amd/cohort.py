"""After the assembly: how much of each assembled gene is in every sample of a cohort, on one MI355X GPU.

What profile.py does for one sample with --counts, for all samples of a list against one gene index that stays on the device
(capi.ProfileIndex): the genes are uploaded once, the k-mer keys of the seeded mode are built once per seed
length, and the reads of several samples share the stretches of one device call.  Per sample the table is byte for byte what
`rambl-profile GENE_SEQ PATH NAME --counts` writes; beside the tables goes the sample x gene matrix.
"""
import os

from . import capi, profile

BATCH_SEGMENTS = 1 << 20          # segments of one device call.  A guess: what the right size is has not been measured.
MATRIX_NAME = "gene_count_matrix.tsv"


def default_name(path):
    """A sample without a name is called after its file: the base name without its last extension."""
    return os.path.splitext(os.path.basename(path))[0]


def sample_names(paths):
    """The default names of `paths`; ValueError when two are equal."""
    return _distinct([(p, default_name(p)) for p in paths])


def _distinct(samples):
    seen = {}
    for path, name in samples:
        if name in seen:
            raise ValueError("sample name %s is given twice (%s and %s)" % (name, seen[name], path))
        seen[name] = path
    return samples


def parse_samples(text):
    """[(path, name)] of a sample list: one sample per line, `PATH` or `PATH<TAB>NAME`; empty lines are skipped.  ValueError on
    a line with more fields or an empty one, a name given twice, or a file that is not there."""
    out = []
    for no, line in enumerate(text.splitlines(), 1):
        if not line.strip():
            continue
        fields = line.split("\t")
        if len(fields) > 2 or not all(f.strip() for f in fields):
            raise ValueError("line %d of the sample list: expected PATH or PATH<TAB>NAME, got %r" % (no, line))
        path = fields[0].strip()
        out.append((path, fields[1].strip() if len(fields) == 2 else default_name(path)))
    _distinct(out)
    for path, _ in out:
        if not os.path.isfile(path):
            raise ValueError("sample file %s does not exist" % path)
    return out


def batches(sized, cap):
    """Lists of whole items, in order, from (item, size) pairs: a batch closes when it is not empty and the next item would
    take it above `cap`, so an item larger than the cap goes alone."""
    batch, total = [], 0
    for item, size in sized:
        if batch and total + size > cap:
            yield batch
            batch, total = [], 0
        batch.append(item)
        total += size
    if batch:
        yield batch


def plan_batches(counts, cap):
    """[(first sample, end sample)] of the device calls for samples of `counts` segments."""
    return [(b[0], b[-1] + 1) for b in batches(enumerate(counts), cap)]


def table_cells(text):
    """{gene: the value as printed} of a <sample>_gene_count.tsv."""
    return dict(line.split("\t") for line in text.splitlines()[1:])


def matrix_text(gene_names, names, tables):
    """gene_count_matrix.tsv: the header `gene<TAB>NAME...` in the samples' order, one row per gene in byte order of the name,
    every cell as that sample's table prints it, 0.0 where the gene is not there.  tables: the tables' text, one per name."""
    cells = [table_cells(t) for t in tables]
    rows = ["gene\t" + "\t".join(names) + "\n" if names else "gene\n"]
    for g in sorted(gene_names, key=lambda n: n.encode()):
        rows.append("\t".join([g] + [c.get(g, "0.0") for c in cells]) + "\n")
    return "".join(rows)


def _segments(path):
    aln = capi.NativeAln(path)
    try:
        return profile.extract_segments(aln.walk())
    finally:
        aln.close()


def cohort_profile(fasta, samples, out_dir=".", min_identity=profile.MIN_IDENTITY, max_evalue=profile.MAX_EVALUE, relative=False,
                   ka_lambda=profile.KA_LAMBDA, ka_k=profile.KA_K, device=0, seeded=False, copy_correct=None, batch_segments=BATCH_SEGMENTS,
                   verbose=False):
    """samples: [(alignment file, name)].  Writes <out_dir>/<name>_gene_count.tsv per sample and <out_dir>/gene_count_matrix.tsv;
    returns (the matrix path, the ScProfileCohortStats of the device calls).  The samples go to the device in file order, in
    batches of whole samples of at most `batch_segments` segments; one index serves all of them.  copy_correct as
    profile.gene_profile takes it."""
    from . import samio
    correction = None
    if copy_correct is not None:                                # read before the device's work: a mistyped path fails at once
        from . import taxa
        with open(copy_correct[0]) as f:
            correction = (taxa.parse_fixrank(f.read()), taxa.load_copy_numbers(copy_correct[1]), copy_correct[2])
    fa = samio.Fasta(fasta)
    if not fa.order:
        raise ValueError("%s holds no gene" % fasta)
    _distinct(list(samples))
    genes = [fa.seqs[n].encode() for n in fa.order]
    os.makedirs(out_dir, exist_ok=True)
    tables, all_stats = [], []

    def loaded():
        for k, (path, _) in enumerate(samples):
            segments = _segments(path)
            yield (k, segments), len(segments)

    with capi.ProfileIndex(genes, device) as index:
        for batch in batches(loaded(), max(1, int(batch_segments))):
            segs, seg_read, read_sample = [], [], []
            for s, (_, segments) in enumerate(batch):           # a read name that occurs in two samples is two reads
                reads, n_reads = profile.read_index([q.decode() for q, _ in segments])
                segs += [x for _, x in segments]
                seg_read += [len(read_sample) + r for r in reads]
                read_sample += [s] * n_reads
            res = index.counts(segs, seg_read, read_sample, len(batch), min_identity, max_evalue, ka_lambda, ka_k, seeded=seeded)
            all_stats.append(res.stats)
            for s, (k, segments) in enumerate(batch):
                counts = profile.counts_from_triples(res.by_sample(s), fa.order)
                if correction is not None:
                    counts = taxa.correct_counts(counts, *correction)
                text = profile.format_table(samples[k][1], counts, relative)
                with open(os.path.join(out_dir, samples[k][1] + "_gene_count.tsv"), "w") as f:
                    f.write(text)
                tables.append(text)
            if verbose:
                import logging
                st = res.stats
                logging.info("cohort profile of %s: %d segments of %d reads against %d genes in %d stretches, %d reads counted, %d key "
                             "sets built, %d device allocations, %s", ", ".join(samples[k][1] for k, _ in batch), len(segs), len(read_sample),
                             len(genes), st.n_stretches, st.n_reads_counted, st.n_index_builds, st.n_allocs, st.as_dict())
    path = os.path.join(out_dir, MATRIX_NAME)
    with open(path, "w") as f:
        f.write(matrix_text(fa.order, [n for _, n in samples], tables))
    return path, all_stats


def main(argv=None):
    """`python -m rambl_amd.cohort GENE_SEQ SAMPLES [options]` = `bin/rambl-cohort`."""
    import argparse
    import logging
    ap = argparse.ArgumentParser(description="Number of read hits per assembled gene for every sample of a list: one table per sample "
                                             "and the sample x gene matrix (hits computed on the GPU against one resident gene index)")
    ap.add_argument("fasta", metavar="GENE_SEQ", help="gene sequences")
    ap.add_argument("samples", metavar="SAMPLES", help="one sample per line: PATH or PATH<TAB>NAME (SAM text or BAM; without a name "
                                                        "the sample is called after its file)")
    ap.add_argument("-o", "--out-dir", dest="out_dir", default=".", help="where the tables and %s go" % MATRIX_NAME)
    ap.add_argument("-c", "--cores", dest="cores", type=int, default=1, help="CPU cores of the alignment-file reader [1]")
    ap.add_argument("-e", "--e-value", dest="e_value", type=float, default=profile.MAX_EVALUE, help="e-value threshold [1e-10]")
    ap.add_argument("-I", "--max_identity", dest="max_align_iden", type=float, default=profile.MIN_IDENTITY,
                    help="least alignment identity in percent [95]")
    ap.add_argument("-r", "--rel", dest="relative_abundance", action="store_true", help="output relative abundance")
    ap.add_argument("--seeded", dest="seeded", action="store_true",
                    help="score only the (segment, gene) pairs that share a k-mer, k chosen so that no hit is lost: the same output, less work")
    ap.add_argument("--copy-correct", dest="copy_correct", default=None, metavar="FIXRANK",
                    help="divide every gene's count by its copy number: the genes' fixrank file from `rambl-taxa classify` (needs --copy-number)")
    ap.add_argument("--copy-number", dest="copy_number", default=None, metavar="TSV", help="copy numbers per taxon: columns `name` and `mean` (rrnDB)")
    ap.add_argument("--copy-thresh", dest="copy_thresh", type=float, default=None, help="least bootstrap confidence of a rank that corrects [0.6]")
    ap.add_argument("--ka-lambda", dest="ka_lambda", type=float, default=profile.KA_LAMBDA, help="Karlin-Altschul lambda [%g]" % profile.KA_LAMBDA)
    ap.add_argument("--ka-k", dest="ka_k", type=float, default=profile.KA_K, help="Karlin-Altschul K [%g]" % profile.KA_K)
    ap.add_argument("--batch-segments", dest="batch_segments", type=int, default=BATCH_SEGMENTS, metavar="N",
                    help="whole samples of at most N segments share a device call; a larger sample goes alone [%d]" % BATCH_SEGMENTS)
    ap.add_argument("--otu", dest="otu", default=None, metavar="PCT",
                    help="then cluster the genes into OTUs at this identity in percent, weighted by their matrix rows, and write what "
                         "`rambl-otu GENE_SEQ --id PCT --matrix %s` writes beside the matrix [off]" % MATRIX_NAME)
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("-v", "--verbose", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    if (a.copy_correct is None) != (a.copy_number is None):
        ap.error("--copy-correct FIXRANK and --copy-number TSV go together")
    if a.copy_thresh is not None and a.copy_correct is None:
        ap.error("--copy-thresh needs --copy-correct")
    if a.batch_segments < 1:
        ap.error("--batch-segments must be at least 1")
    if a.cores < 1:
        ap.error("-c must be at least 1")
    try:
        with open(a.samples) as f:
            samples = parse_samples(f.read())
        if not samples:
            raise ValueError("%s lists no sample" % a.samples)
        from . import samio
        if not samio.Fasta(a.fasta).order:
            raise ValueError("%s holds no gene" % a.fasta)
        if a.otu is not None:
            from . import otu
            diff = otu.diff_from_identity(a.otu)
            names, seqs, _ = otu.load_inputs(a.fasta)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    os.environ["SC_INGEST_THREADS"] = str(max(1, min(a.cores, capi.host_plan(1)[2])))
    path, _ = cohort_profile(a.fasta, samples, a.out_dir, a.max_align_iden, a.e_value, a.relative_abundance, a.ka_lambda, a.ka_k, a.device, a.seeded,
                             None if a.copy_correct is None else (a.copy_correct, a.copy_number, 0.6 if a.copy_thresh is None else a.copy_thresh),
                             a.batch_segments, a.verbose)
    if a.otu is not None:
        with open(path) as f:
            otu.cluster(names, seqs, diff, f.read(), a.out_dir, False, a.device, a.verbose)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
