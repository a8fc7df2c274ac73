"""After the assembly: the assembled genes clustered into OTUs at an identity, on one MI355X GPU.

The device computes exact unit-cost edit distances of whole genes (capi: sc_gene_distances, sc_gene_pairs); the host walks the
genes by weight and makes greedy centroids from the qualifying pairs.  Every decision is an integer comparison: an identity
is the rational difference rate diff_num / diff_den, and a pair qualifies iff ed <= (max(len) * diff_num) // diff_den.
There are no free end gaps: a fragment of a gene is far from the gene.  At 100 % (diff_num 0) genes that hold a byte other than
A C G T never merge, not even exact copies: such a byte matches nothing, itself included.
"""
import ctypes as C
import fractions
import math
import os

from . import capi, profile

STAT_NAMES = ("upload_ms", "kernel_ms", "total_ms", "tiles", "pairs_scored", "pairs_skipped", "word_steps")      # the SC_PAIRS_STAT_* slots
MAX_LEN = 2048
OTUS_NAME, MAP_NAME, MATRIX_NAME, PAIRS_NAME = "otus.fa", "otu_map.tsv", "otu_count_matrix.tsv", "gene_pairs.tsv"


def widths():
    """sc_pairs_widths: the words per pattern the kernel is built for, ascending."""
    n = capi.lib().sc_pairs_widths(None, 0)
    out = (C.c_int * n)()
    capi.lib().sc_pairs_widths(out, n)
    return list(out)


def _stats(raw):
    return dict(zip(STAT_NAMES, raw))


def _genes(genes):
    return capi._pack_long([bytes(g) for g in genes])


def distances(genes, pairs, device=0, with_stats=False):
    """sc_gene_distances: [ed(genes[a], genes[b])] for the (a, b) of `pairs`; genes: a list of bytes of 1..2048 bases each;
    a == b is allowed.  with_stats: (the list, the call's statistics by STAT_NAMES)."""
    import numpy as np
    text, off = _genes(genes)
    a = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
    b = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
    out = np.zeros(max(len(a), 1), dtype=np.int32)
    raw = (C.c_double * len(STAT_NAMES))()
    rc = capi.lib().sc_gene_distances(int(device), text, capi._ptr(off), len(genes), capi._ptr(a), capi._ptr(b), len(a), capi._ptr(out), raw, len(raw))
    capi._check(rc, capi.lib().sc_pairs_error)
    got = out[:len(a)].tolist()
    return (got, _stats(raw)) if with_stats else got


def pairs_within(genes, diff_num, diff_den, device=0, cap=None, with_stats=False):
    """sc_gene_pairs: [(a, b, ed)] of every pair a < b with ed <= (max(len) * diff_num) // diff_den, sorted by (a, b).  The room
    for pairs starts at `cap` (default 65 536) and grows to what the library asks for."""
    import numpy as np
    text, off = _genes(genes)
    raw = (C.c_double * len(STAT_NAMES))()

    def attempt(cap):
        cols = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(3)]
        n = C.c_long()
        rc = capi.lib().sc_gene_pairs(int(device), text, capi._ptr(off), len(genes), int(diff_num), int(diff_den), *[capi._ptr(c) for c in cols],
                                      cap, C.byref(n), raw, len(raw))
        return rc, n.value, cols
    rc, k, cols = capi.with_room(1 << 16 if cap is None else int(cap), attempt)
    capi._check(rc, capi.lib().sc_pairs_error)
    got = list(zip(*(c[:k].tolist() for c in cols)))
    return (got, _stats(raw)) if with_stats else got


def diff_from_identity(text):
    """"99.5" -> (5, 1000), "97" -> (3, 100), "100" -> (0, 1): the difference rate 1 - identity / 100 of an identity in percent,
    exact, over the least denominator 100 * 10^k that holds it (in lowest terms where there is none: "295/3" -> (1, 60)).  The
    bound is the same whichever way the rate is written.  ValueError unless 0 < identity <= 100."""
    try:
        pct = fractions.Fraction(str(text).strip())
    except (ValueError, ZeroDivisionError):
        raise ValueError("identity %r is not a number" % (text,))
    if not 0 < pct <= 100:
        raise ValueError("identity %s is outside (0, 100]" % text)
    diff = 1 - pct / 100
    if diff.denominator >= 1 << 31:
        raise ValueError("identity %s has too many digits" % text)
    den = 100
    while diff and den < 1 << 31 and den % diff.denominator:
        den *= 10
    if not diff or den >= 1 << 31:
        return diff.numerator, diff.denominator
    return diff.numerator * (den // diff.denominator), den


def walk_order(names, lengths, weights):
    """The genes by (weight descending, length descending, name bytes ascending): the order the centroids are made in."""
    return sorted(range(len(names)), key=lambda g: (-weights[g], -lengths[g], names[g].encode()))


def greedy_otus(names, lengths, weights, pairs):
    """[(gene, centroid, ed)] by name, one entry per gene in input order.  pairs: the qualifying (a, b, ed) by index.  The genes
    are walked in walk_order; a gene joins the centroid made so far with which it qualifies and whose ed / max(len) is
    smallest (compared by cross-multiplication, ties to the centroid made first), and becomes a centroid (ed 0) when there
    is none."""
    near = [[] for _ in names]
    for a, b, d in pairs:
        near[a].append((b, d))
        near[b].append((a, d))
    rank = {}                                                   # centroid -> the order it was made in
    out = [None] * len(names)
    for g in walk_order(names, lengths, weights):
        best = None                                             # (ed, max length, rank, centroid)
        for c, d in near[g]:
            if c not in rank:
                continue
            cand = (d, max(lengths[g], lengths[c]), rank[c], c)
            if best is None or cand[0] * best[1] < best[0] * cand[1] or (cand[0] * best[1] == best[0] * cand[1] and cand[2] < best[2]):
                best = cand
        if best is None:
            rank[g] = len(rank)
            out[g] = (names[g], names[g], 0)
        else:
            out[g] = (names[g], names[best[3]], best[0])
    return out


def parse_matrix(text):
    """(header line, {gene: [cells as printed]}) of a gene_count_matrix.tsv; ValueError on a ragged or repeated row."""
    lines = text.splitlines()
    if not lines or lines[0].split("\t")[0] != "gene":
        raise ValueError("the matrix has no `gene` header line")
    n_cols, rows = len(lines[0].split("\t")), {}
    for no, line in enumerate(lines[1:], 2):
        f = line.split("\t")
        if len(f) != n_cols or f[0] in rows:
            raise ValueError("line %d of the matrix: %s" % (no, "gene %s is given twice" % f[0] if f[0] in rows else "expected %d fields" % n_cols))
        try:
            [float(x) for x in f[1:]]
        except ValueError:
            raise ValueError("line %d of the matrix holds a cell that is no number" % no)
        rows[f[0]] = f[1:]
    return lines[0], rows


def matrix_weights(matrix_text, names):
    """The weight of every gene of `names`: the sum of its matrix row (math.fsum: correctly rounded, whatever the order)."""
    _, rows = parse_matrix(matrix_text)
    return [math.fsum(float(x) for x in rows[n]) for n in names]


def otu_matrix_text(matrix_text, mapping):
    """otu_count_matrix.tsv: the matrix's header, then one row per centroid in byte order of the name; a cell is the sum of the
    member rows' cells, added in mapping order, printed as the per-sample tables print a count (3 decimals, repr)."""
    header, rows = parse_matrix(matrix_text)
    sums = {}
    for gene, centroid, _ in mapping:
        acc = sums.setdefault(centroid, [0.0] * (len(header.split("\t")) - 1))
        for k, x in enumerate(rows[gene]):
            acc[k] += float(x)
    return header + "\n" + "".join("%s\n" % "\t".join([c] + [repr(profile._round_half_away(v, 3)) for v in sums[c]])
                                   for c in sorted(sums, key=lambda n: n.encode()))


def otu_map_text(names, lengths, mapping):
    length = dict(zip(names, lengths))
    return "gene\totu\tedit_distance\tgene_length\totu_length\n" + "".join(
        "%s\t%s\t%d\t%d\t%d\n" % (g, c, d, length[g], length[c]) for g, c, d in mapping)


def otus_fasta_text(names, seqs, lengths, weights, mapping):
    """The centroids in the order they were made, one line of sequence each."""
    centroid = {c for _, c, _ in mapping}
    return "".join(">%s\n%s\n" % (names[g], seqs[g]) for g in walk_order(names, lengths, weights) if names[g] in centroid)


def pairs_text(names, pairs):
    return "a\tb\tedit_distance\n" + "".join("%s\t%s\t%d\n" % (names[a], names[b], d) for a, b, d in pairs)


def load_inputs(fasta, matrix=None):
    """(names, seqs, matrix text or None) of a gene FASTA and an optional gene_count_matrix.tsv; ValueError on a name given
    twice, an empty or too long gene, or a matrix whose genes are not those of the FASTA.  No device is touched."""
    from . import samio
    fa = samio.Fasta(fasta)
    if not fa.order:
        raise ValueError("%s holds no gene" % fasta)
    seen = set()
    for n in fa.order:
        if n in seen:
            raise ValueError("gene name %s is given twice in %s" % (n, fasta))
        seen.add(n)
        if not 1 <= len(fa.seqs[n]) <= MAX_LEN:
            raise ValueError("gene %s has %d bases (1..%d supported)" % (n, len(fa.seqs[n]), MAX_LEN))
    text = None
    if matrix is not None:
        with open(matrix) as f:
            text = f.read()
        _, rows = parse_matrix(text)
        if set(rows) != seen:
            odd = sorted(set(rows) ^ seen)
            raise ValueError("the genes of %s are not those of %s (%d differ, the first: %s)" % (matrix, fasta, len(odd), odd[0]))
    return list(fa.order), [fa.seqs[n] for n in fa.order], text


def cluster(names, seqs, diff, matrix_text=None, out_dir=".", keep_pairs=False, device=0, verbose=False):
    """Writes otus.fa, otu_map.tsv, with a matrix otu_count_matrix.tsv and with keep_pairs gene_pairs.tsv under out_dir; returns
    (the mapping, the statistics of the device call).  diff: (diff_num, diff_den)."""
    lengths = [len(s) for s in seqs]
    weights = matrix_weights(matrix_text, names) if matrix_text is not None else [0] * len(names)
    pairs, stats = pairs_within([s.encode() for s in seqs], diff[0], diff[1], device, with_stats=True)
    mapping = greedy_otus(names, lengths, weights, pairs)
    os.makedirs(out_dir, exist_ok=True)
    files = {OTUS_NAME: otus_fasta_text(names, seqs, lengths, weights, mapping), MAP_NAME: otu_map_text(names, lengths, mapping)}
    if matrix_text is not None:
        files[MATRIX_NAME] = otu_matrix_text(matrix_text, mapping)
    if keep_pairs:
        files[PAIRS_NAME] = pairs_text(names, pairs)
    for name, text in files.items():
        with open(os.path.join(out_dir, name), "w") as f:
            f.write(text)
    if verbose:
        import logging
        logging.info("%d genes at a difference rate of %d/%d: %d qualifying pairs, %d OTUs, %s", len(names), diff[0], diff[1], len(pairs),
                     len({c for _, c, _ in mapping}), stats)
    return mapping, stats


def main(argv=None):
    """`python -m rambl_amd.otu GENE_SEQ [options]` = `bin/rambl-otu`."""
    import argparse
    import logging
    ap = argparse.ArgumentParser(description="Cluster assembled genes into OTUs at an identity: greedy centroids over exact edit distances "
                                             "computed on the GPU")
    ap.add_argument("fasta", metavar="GENE_SEQ", help="gene sequences (1..%d bases each)" % MAX_LEN)
    ap.add_argument("--id", dest="identity", default="97", metavar="PCT", help="least identity in percent, in (0, 100] [97]")
    ap.add_argument("--matrix", dest="matrix", default=None, metavar="TSV",
                    help="a gene_count_matrix.tsv of the same genes: a gene's weight is the sum of its row, and otu_count_matrix.tsv is written")
    ap.add_argument("-o", "--out-dir", dest="out_dir", default=".", help="where the files go")
    ap.add_argument("--pairs", dest="pairs", action="store_true", help="also write %s: every qualifying pair" % PAIRS_NAME)
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("-v", "--verbose", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    try:
        diff = diff_from_identity(a.identity)
        names, seqs, matrix_text = load_inputs(a.fasta, a.matrix)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    cluster(names, seqs, diff, matrix_text, a.out_dir, a.pairs, a.device, a.verbose)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
