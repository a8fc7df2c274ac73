"""After the assembly: the genus of every assembled gene, copy-number correction and the table of taxa per sample.

The reference's scripts/per_sample_gene_profile_fast.py:223-246 (copy_number_correct) and all of
scripts/per_sample_taxon_profile.py start with `java -jar classifier.jar -f fixrank`, the RDP classifier.  Here its stated
rule -- naive Bayes over 8-mers with 100 bootstrap trials -- is trained on a labelled set the user has (data_info's GeneSeq
and GeneTax) and run on the GPU by sc_taxa_train / sc_taxa_classify (rambl_amd/csrc/sc_taxa.hip); DESIGN.md §8.12 is the
contract, this project's own: parity with RDP's output is not claimed.  `classify` writes the genes' assignments in RDP's
fixrank layout, which the two parsers of the scripts (:197-221, :54-80) read; `table` is per_sample_taxon_profile.py:83-203
on an existing <sample>_gene_count.tsv; profile.py's --copy-correct is copy_number_correct on the same fixrank file.
"""
import csv
import logging
import os

from . import capi

RANKS = ("domain", "phylum", "class", "order", "family", "genus")
GREENGENES_PREFIXES = ("k__", "p__", "c__", "o__", "f__", "g__")
THRESH = 0.6                       # -t of both scripts
N_TRIALS = capi.TAXA_TRIALS


def fnv1a64(data):
    """FNV-1a, 64 bits, of bytes: the per-query key of the trials, so that a gene's row depends on its name and sequence only."""
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def parse_lineage(text):
    """The six names domain..genus of a taxonomy file's lineage, or None when a rank is missing or empty.  Two forms:
    GreenGenes (`k__A; p__B; c__C; o__D; f__E; g__F; s__G`: the prefixes stripped, s__ ignored) and six plain names
    separated by `;`."""
    fields = [f.strip() for f in text.strip().split(";")]
    if fields and fields[-1] == "":
        fields.pop()
    if fields and fields[0].startswith("k__"):
        if len(fields) < 6 or any(not f.startswith(p) for f, p in zip(fields, GREENGENES_PREFIXES)):
            return None
        names = tuple(f[3:].strip() for f in fields[:6])
    else:
        if len(fields) != 6:
            return None
        names = tuple(fields)
    return names if all(names) else None


def read_taxonomy(path):
    """{sequence id: lineage text} of an `id<TAB>lineage` file; the first line of an id wins."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line or "\t" not in line:
                continue
            k, v = line.split("\t", 1)
            out.setdefault(k.strip(), v)
    return out


def training_set(names, seqs, labels):
    """The labelled training set from FASTA names and sequences and {id: lineage text}.  A genus is its whole six-name path
    (equal names under different parents are different genera); genera are numbered in the order of their paths, so the
    numbering -- and with it every tie -- does not depend on the order of the files.  Returns (sequences, genus index per
    sequence, [path], drops) with drops = {"unlabelled": sequences without a label, "incomplete": sequences whose lineage
    lacks a rank, "no_sequence": labels without a sequence}."""
    kept, paths = [], []
    drops = {"unlabelled": 0, "incomplete": 0, "no_sequence": len(set(labels) - set(names))}
    for n, s in zip(names, seqs):
        if n not in labels:
            drops["unlabelled"] += 1
            continue
        path = parse_lineage(labels[n])
        if path is None:
            drops["incomplete"] += 1
            continue
        kept.append(s)
        paths.append(path)
    genera = sorted(set(paths))
    index = {p: i for i, p in enumerate(genera)}
    return kept, [index[p] for p in paths], genera, drops


def confidences(best, winners, genera):
    """Per rank the share of the trials whose winner has the assigned genus' ancestor there (the same path down to the
    rank)."""
    path = genera[best]
    return [sum(1 for w in winners if genera[w][:r + 1] == path[:r + 1]) / len(winners) for r in range(len(RANKS))]


def fixrank_line(gene, path=None, conf=None):
    """One line of RDP's fixrank layout: the gene, an empty field, then name, rank, confidence (%.2f) for the six ranks; an
    unclassified gene has the name and the empty field only."""
    if path is None:
        return "%s\t\n" % gene
    return "%s\t\t%s\n" % (gene, "\t".join("%s\t%s\t%.2f" % (n, r, c) for n, r, c in zip(path, RANKS, conf)))


def parse_fixrank(text):
    """[(gene, [(taxon, rank, confidence)])] in file order, read as both of the scripts' parsers read it: the fields after the
    gene up to a rank word are the taxon (joined by a space, double quotes removed, stripped), the field after the rank word is
    the confidence."""
    out = []
    for line in text.splitlines():
        fields = line.strip().split("\t")
        entries, level, terms = [], "", []
        for t in fields[1:]:
            if t in RANKS:
                level = t
            elif not level:
                terms.append(t)
            else:
                entries.append((" ".join(x.replace('"', "") for x in terms).strip(), level, float(t)))
                level, terms = "", []
        out.append((fields[0], entries))
    return out


def load_copy_numbers(path):
    """{taxon: mean copy number} of a tab-separated table with the columns `name` and `mean` (rrnDB's); the first row of a
    name wins (per_sample_gene_profile_fast.py:179-186)."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f, delimiter="\t"):
            out.setdefault(row["name"], float(row["mean"]))
    return out


def gene_copy_number(entries, copy_numbers, thresh=THRESH):
    """per_sample_gene_profile_fast.py:235-245 for one gene: of its ranks with confidence >= thresh, walked from domain to
    genus, the deepest whose taxon has a row in the table gives the copy number; none: 1.0."""
    copy = 1.0
    for rank in RANKS:
        for taxon, level, conf in entries:
            if level == rank and conf >= thresh and taxon in copy_numbers:
                copy = copy_numbers[taxon]
    return copy


def correct_counts(counts, fixrank, copy_numbers, thresh=THRESH):
    """copy_number_correct (:223-246): [(gene, float(count) / copy number)]; a gene the fixrank file does not hold keeps its
    count.  `fixrank`: parse_fixrank's list (a gene's first line wins, as the script's setdefault has it)."""
    lineage = {}
    for gene, entries in fixrank:
        lineage.setdefault(gene, entries)
    return [(g, float(v) / gene_copy_number(lineage.get(g, []), copy_numbers, thresh)) for g, v in counts]


def read_gene_counts(text):
    """{gene: count} of a <sample>_gene_count.tsv (per_sample_taxon_profile.py:173-179)."""
    out = {}
    for line in text.splitlines():
        if line.startswith("sample") or not line.strip():
            continue
        gene, count = line.strip().split()
        out[gene] = float(count)
    return out


def taxa_table(fixrank, gene_length, gene_count, copy_numbers, rank="genus", thresh=THRESH):
    """per_sample_taxon_profile.py:54-133 and :184-195 -> [(taxon, value)] in byte order of the taxon.  A taxon is taken from
    the genes whose confidence at `rank` is >= thresh; its count is the sum of their counts (genes the count table lacks give
    nothing), its length the longest of them, its copy number that of the taxon, else of its nearest ancestor with a row
    in the table (the lineage of the first line that names the taxon).  value = count / (copy * length), divided by the sum of
    all values + 1e-10, summed in the order of the output.  Where the script finds no copy number it divides by 0.0; here the
    taxon gets 1.0 and a log line."""
    if rank not in RANKS:
        raise ValueError("no rank %r (one of %s)" % (rank, ", ".join(RANKS)))
    taxa_genes, taxa_lineage = {}, {}
    for gene, entries in fixrank:
        lineage = {}
        for taxon, level, conf in entries:
            if level == rank and conf >= thresh:
                taxa_genes.setdefault(taxon, []).append(gene)
            lineage.setdefault(level, taxon)
        if rank in lineage:                                     # (the script throws on a gene without the rank: an unclassified gene)
            taxa_lineage.setdefault(lineage[rank], lineage)
    above = RANKS[:RANKS.index(rank)][::-1]
    values = {}
    for taxon, genes in taxa_genes.items():
        for g in genes:
            if g not in gene_length:
                raise ValueError("gene %s of the fixrank file is not among the gene sequences" % g)
        count = sum(gene_count[g] for g in genes if g in gene_count)
        length = max(gene_length[g] for g in genes)
        copy = copy_numbers.get(taxon)
        if copy is None:
            for high in above:
                t = taxa_lineage[taxon].get(high)
                if t in copy_numbers:
                    copy = copy_numbers[t]
                    break
        if copy is None:
            logging.info("no copy number for %s or an ancestor: 1.0 is used", taxon)
            copy = 1.0
        values[taxon] = count / (copy * length)
    order = sorted(values, key=lambda t: t.encode())
    z = sum(values[t] for t in order) + 1e-10
    return [(t, values[t] / z) for t in order]


def format_taxa_table(sample, rows):
    """<sample>_taxa_count.tsv: header `sample<TAB><sample>`, one line per taxon, the value printed with repr."""
    return "sample\t%s\n" % sample + "".join("%s\t%r\n" % (t, v) for t, v in rows)


def classify_genes(fasta, train_seq, train_tax, out_dir=".", seed=0, device=0, verbose=False):
    """Trains on (train_seq, train_tax), classifies the genes of `fasta` and writes <out_dir>/<basename of fasta without its
    extension>_fixrank.tsv.  Returns (path, training ScTaxaStats, classification ScTaxaStats)."""
    from . import samio
    tr = samio.Fasta(train_seq)
    seqs, genus, genera, drops = training_set(tr.order, [tr.seqs[n].encode() for n in tr.order], read_taxonomy(train_tax))
    logging.info("training set: %d sequences of %d genera; dropped: %d without a label, %d with an incomplete lineage; %d labels without a "
                 "sequence", len(seqs), len(genera), drops["unlabelled"], drops["incomplete"], drops["no_sequence"])
    if not seqs:
        raise ValueError("%s and %s give no labelled training sequence" % (train_seq, train_tax))
    fa = samio.Fasta(fasta)
    if not fa.order:
        raise ValueError("%s holds no gene" % fasta)
    with capi.TaxaModel(seqs, genus, len(genera), device) as model:
        best, winners, n_words, st = model.classify([fa.seqs[n].encode() for n in fa.order], [fnv1a64(n.encode()) for n in fa.order], seed, N_TRIALS)
        train_stats = model.stats
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, os.path.splitext(os.path.basename(fasta))[0] + "_fixrank.tsv")
    with open(path, "w") as f:
        for i, name in enumerate(fa.order):
            if n_words[i] == 0:
                f.write(fixrank_line(name))
            else:
                b = int(best[i])
                f.write(fixrank_line(name, genera[b], confidences(b, [int(w) for w in winners[i]], genera)))
    if verbose:
        logging.info("classified %d genes (%d without a word): train %s, classify %s", len(fa.order), int((n_words == 0).sum()),
                     train_stats.as_dict(), st.as_dict())
    return path, train_stats, st


def sample_taxa(fixrank_path, fasta, gene_count_path, sample, copy_number_path, rank="genus", thresh=THRESH, out_dir="."):
    """Writes <out_dir>/<sample>_taxa_count.tsv from a fixrank file, the gene sequences (for the lengths), the sample's gene
    count table and a copy-number table; returns the path."""
    from . import samio
    fa = samio.Fasta(fasta)
    with open(fixrank_path) as f:
        fixrank = parse_fixrank(f.read())
    with open(gene_count_path) as f:
        gene_count = read_gene_counts(f.read())
    rows = taxa_table(fixrank, {n: len(fa.seqs[n]) for n in fa.order}, gene_count, load_copy_numbers(copy_number_path), rank, thresh)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, sample + "_taxa_count.tsv")
    with open(path, "w") as f:
        f.write(format_taxa_table(sample, rows))
    return path


def main(argv=None):
    """`rambl-taxa classify GENE_SEQ --train-seq FASTA --train-tax TAX [-o DIR] [--seed N] [--device N] [-v]` and
    `rambl-taxa table FIXRANK GENE_SEQ GENE_COUNT_TSV SAMPLE --copy-number TSV [-L genus] [-t 0.6] [-o DIR]`."""
    import argparse
    ap = argparse.ArgumentParser(description="Genus of the assembled genes (classified on the GPU) and the table of taxa per sample")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("classify", help="write <GENE_SEQ>_fixrank.tsv: the genes' lineage and bootstrap confidence per rank")
    c.add_argument("fasta", metavar="GENE_SEQ", help="gene sequences")
    c.add_argument("--train-seq", required=True, metavar="FASTA", help="labelled training sequences (data_info's GeneSeq)")
    c.add_argument("--train-tax", required=True, metavar="TAX", help="their lineages, id<TAB>lineage (data_info's GeneTax)")
    c.add_argument("-o", "--out-dir", dest="out_dir", default=".")
    c.add_argument("--seed", type=int, default=0, help="seed of the bootstrap trials [0]")
    c.add_argument("-d", "--device", type=int, default=0)
    c.add_argument("-v", "--verbose", action="store_true")
    t = sub.add_parser("table", help="write <SAMPLE>_taxa_count.tsv from a fixrank file and <SAMPLE>_gene_count.tsv")
    t.add_argument("fixrank", metavar="FIXRANK")
    t.add_argument("fasta", metavar="GENE_SEQ")
    t.add_argument("gene_count", metavar="GENE_COUNT_TSV")
    t.add_argument("sample", metavar="SAMPLE")
    t.add_argument("--copy-number", required=True, metavar="TSV", help="copy numbers per taxon: columns `name` and `mean` (rrnDB)")
    t.add_argument("-L", "--tax-rank", dest="rank", default="genus", choices=RANKS, help="rank of the table [genus]")
    t.add_argument("-t", "--thresh", type=float, default=THRESH, help="least bootstrap confidence [0.6]")
    t.add_argument("-o", "--out-dir", dest="out_dir", default=".")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    if a.cmd == "classify":
        classify_genes(a.fasta, a.train_seq, a.train_tax, a.out_dir, a.seed, a.device, a.verbose)
    else:
        sample_taxa(a.fixrank, a.fasta, a.gene_count, a.sample, a.copy_number, a.rank, a.thresh, a.out_dir)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
