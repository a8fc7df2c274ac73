"""The contract of the genus assignment restated plainly -- Python sets and integers, numpy fp64 for the
table -- with the reference scripts' two fixrank parsers, and the named cases of tests/test_taxa_host.py and
tests/test_taxa_gpu.py.  Every named case carries a property check that its input reaches the edge it is named for.  Nothing
here imports the product."""
import math
import random

import numpy as np

K = 8
N_WORDS = 65536
CHUNK = 64                         # genera per workgroup of the device's score pass
RANKS = ["domain", "phylum", "class", "order", "family", "genus"]
MASK = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


# ---- words, training, table ---------------------------------------------------------------------------------------------

def word_list(seq):
    """The codes of the valid windows in order, repeats included."""
    out = []
    for i in range(len(seq) - K + 1):
        w = 0
        for ch in seq[i:i + K].upper():
            if ch not in CODE:
                break
            w = w * 4 + CODE[ch]
        else:
            out.append(w)
    return out


def train_counts(seqs, genus, G):
    """n[w], m[w][g], M[g], N."""
    n = np.zeros(N_WORDS, dtype=np.int64)
    m = np.zeros((N_WORDS, G), dtype=np.int64)
    M = np.zeros(G, dtype=np.int64)
    for s, g in zip(seqs, genus):
        M[g] += 1
        for w in set(word_list(s)):
            n[w] += 1
            m[w, g] += 1
    return n, m, M, len(seqs)


def table_real(n, m, M, N):
    """log2(P(w|g)) * 1024 in fp64, before rounding."""
    pw = (n.astype(np.float64) + 0.5) / (float(N) + 1.0)
    p = (m.astype(np.float64) + pw[:, None]) / (M.astype(np.float64) + 1.0)[None, :]
    return np.log2(p) * 1024.0


def half_margin(x):
    """The least distance of any cell from a half-integer."""
    return float(np.abs(x - np.floor(x) - 0.5).min())


def table(n, m, M, N):
    """q[w][g]; asserts the condition under which the device must agree exactly: no cell within 1e-6 of a half-integer."""
    x = table_real(n, m, M, N)
    assert half_margin(x) > 1e-6, "a cell lies within 1e-6 of a half-integer: change the case's counts"
    return np.rint(x).astype(np.int64)


# ---- scores, draws, winners ---------------------------------------------------------------------------------------------

def mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, key, t, j, W):
    z = mix(((seed ^ key) + (t * 65536 + j + 1) * 0x9E3779B97F4A7C15) & MASK)
    return ((z >> 32) * W) >> 32


def n_draws(W):
    return max(W // 8, 5)


def argmax_low(scores):
    best = 0
    for g in range(1, len(scores)):
        if scores[g] > scores[best]:
            best = g
    return best


def scores(q, words):
    return [int(v) for v in q[np.asarray(words, dtype=np.int64)].sum(axis=0)] if len(words) else [0] * q.shape[1]


def classify(q, query, key, seed=0, n_trials=100):
    """(assigned genus, [winner per trial], W); (-1, [-1] * n_trials, 0) for a query without a word."""
    words = word_list(query)
    W = len(words)
    if W == 0:
        return -1, [-1] * n_trials, 0
    best = argmax_low(scores(q, words))
    winners = []
    for t in range(n_trials):
        winners.append(argmax_low(scores(q, [words[draw(seed, key, t, j, W)] for j in range(n_draws(W))])))
    return best, winners, W


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & MASK
    return h


# ---- confidence, fixrank, the scripts' parsers and host rules -------------------------------------------------------------

def confidences(best, winners, genera):
    out = []
    for r in range(6):
        same = 0
        for w in winners:
            if tuple(genera[w][:r + 1]) == tuple(genera[best][:r + 1]):
                same += 1
        out.append(same / float(len(winners)))
    return out


def fixrank_text(names, results, genera):
    """The fixrank file of genes `names` with results [(best, winners, W)]."""
    lines = []
    for name, (best, winners, W) in zip(names, results):
        fields = [name, ""]
        if W:
            for r, c in enumerate(confidences(best, winners, genera)):
                fields += [genera[best][r], RANKS[r], "%.2f" % c]
        lines.append("\t".join(fields) + "\n")
    return "".join(lines)


def ref_parse_gene_lineage(text, thresh):
    """parse_rdp_result of per_sample_gene_profile_fast.py (:197-221): {gene: ['<rank index>__<taxon>' with score >= thresh]}."""
    prefix = dict((lv, "%d__" % i) for i, lv in enumerate(RANKS))
    gene_lineage = {}
    for line in text.splitlines(True):
        fields = line.strip().split("\t")
        gene = fields[0]
        taxon, level, score = "", "", 0
        lineage, terms = [], []
        for t in fields[1:]:
            if t in RANKS:
                level = t
            elif len(level) == 0:
                terms += [t]
            else:
                score = float(t)
                taxon = " ".join([x.replace('"', "") for x in terms]).strip()
                if score >= thresh:
                    lineage += [prefix[level] + taxon]
                taxon, level, score = "", "", 0
                terms = []
        gene_lineage.setdefault(gene, lineage)
    return gene_lineage


def ref_parse_taxa(text, taxon_rank, thresh):
    """parse_rdp_results of per_sample_taxon_profile.py (:54-80): ({taxon: [genes]}, {taxon: {rank: taxon}}).  The script
    throws on a line without `taxon_rank` (an unclassified gene); such a line is passed over here."""
    taxa_genes, taxa_lineage = {}, {}
    for line in text.splitlines(True):
        fields = line.strip().split("\t")
        gene = fields[0]
        taxon, level, score = "", "", 0
        lineage, terms = {}, []
        for t in fields[1:]:
            if t in RANKS:
                level = t
            elif len(level) == 0:
                terms += [t]
            else:
                score = float(t)
                taxon = " ".join([x.replace('"', "") for x in terms]).strip()
                if level == taxon_rank and score >= thresh:
                    taxa_genes.setdefault(taxon, []).append(gene)
                lineage.setdefault(level, taxon)
                taxon, level, score = "", "", 0
                terms = []
        if taxon_rank in lineage:
            taxa_lineage.setdefault(lineage[taxon_rank], lineage)
    return taxa_genes, taxa_lineage


def ref_copy_correct(gene_count, gene_lineage, taxon_copy_number):
    """copy_number_correct (:235-246) on {gene: count}: the sorted prefixed lineage is rank order; the last taxon with a row
    wins; none: 1.0."""
    out = {}
    for gene, count in gene_count.items():
        found = []
        for t in sorted(gene_lineage.get(gene, [])):
            t = t.split("__", 1)[1]
            if t in taxon_copy_number:
                found += [taxon_copy_number[t]]
        out[gene] = float(count) / (found[-1] if found else 1.0)
    return out


def ref_read_gene_counts(text):
    """per_sample_taxon_profile.py:173-179 on the text of a <sample>_gene_count.tsv."""
    gene_count = {}
    for line in text.splitlines(True):
        if line.startswith("sample"):
            continue
        gene, count = line.strip().split()
        gene_count[gene] = float(count)
    return gene_count


def ref_taxa_table(text, gene_length, gene_count, copy_numbers, rank, thresh):
    """per_sample_taxon_profile.py:83-133, :184-203 with the two stated differences: a taxon without a copy number gets 1.0,
    and the sum runs in the order of the output.  Returns the file's text after the header as [(taxon, value)]."""
    taxa_genes, taxa_lineage = ref_parse_taxa(text, rank, thresh)
    i = RANKS.index(rank)
    val = {}
    for taxon, genes in taxa_genes.items():
        count = sum([gene_count[g] for g in genes if g in gene_count])
        length = max([gene_length[g] for g in genes])
        copy = None
        if taxon in copy_numbers:
            copy = copy_numbers[taxon]
        else:
            for high in RANKS[:i][::-1]:
                if taxa_lineage[taxon][high] in copy_numbers:
                    copy = copy_numbers[taxa_lineage[taxon][high]]
                    break
        if copy is None:
            copy = 1.0
        val[taxon] = count / (copy * length)
    order = sorted(val, key=lambda t: t.encode())
    Z = sum([val[t] for t in order]) + 1e-10
    return [(t, val[t] / Z) for t in order]


# ---- named cases ----------------------------------------------------------------------------------------------------------

def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate):
    return "".join(rng.choice("ACGT") if rng.random() < rate else ch for ch in s)


def word_of(text):
    assert len(text) == K
    return word_list(text)[0]


class Model:
    """A training set with its restated counts and table."""

    def __init__(self, seqs, genus, G):
        self.seqs, self.genus, self.G = seqs, genus, G
        self.n, self.m, self.M, self.N = train_counts(seqs, genus, G)
        self.q = table(self.n, self.m, self.M, self.N)


def counts_case():
    """The training set of the count tests: 4 genera (genus 2 has one sequence, genus 3 none) and every word edge."""
    rng = random.Random(812)
    seqs = [
        ("ACGTACGTACGTACGT", 0),                   # ACGTACGT three times in one sequence
        ("GGACGTACGTCC", 0),                       # ... and in a second sequence of the genus
        ("TTACGTACGTAA", 1),                       # ... and in another genus
        ("NACGTACGGNTTGACCAAN", 1),                # N as the first base, inside a window, as the last base
        ("acguacguuugca", 0),                      # lower case and U
        ("ACGTACG", 1),                            # 7 bases: no word
        ("GGGGCCCC", 1),                           # 8 bases: one word
        ("", 1),                                   # empty
        ("AAAAAAAANTTTTTTTT", 2),                  # words 0 and 65 535: the bitset's first and last bit
        ("AAAAACTTNAAAAAGAA", 0),                  # words 31 and 32: both sides of a 32-bit bitset word
        (rand_seq(rng, 3000), 1),                  # more than 64 windows per lane stretch of one: every lane rolls a long stretch
    ]
    mo = Model([s for s, _ in seqs], [g for _, g in seqs], 4)
    w = word_of("ACGTACGT")
    assert word_list(seqs[0][0]).count(w) == 3 and mo.m[w, 0] == 3 and mo.m[w, 1] == 1 and mo.n[w] == 4   # seqs 0, 1, 4 (u = t) | 2
    assert word_list(seqs[3][0]) == word_list("ACGTACGG") + word_list("TTGACCAA")
    assert word_list(seqs[4][0]) == word_list("ACGTACGTTTGCA")
    assert word_list(seqs[5][0]) == [] and len(word_list(seqs[6][0])) == 1 and word_list(seqs[7][0]) == []
    assert word_list(seqs[8][0]) == [0, 65535] and mo.m[0, 2] == 1 and mo.m[65535, 2] == 1
    assert word_list(seqs[9][0]) == [31, 32] and 31 // 32 != 32 // 32
    assert len(word_list(seqs[10][0])) == 2993 > 64
    assert mo.M.tolist() == [4, 6, 1, 0]
    return mo


def second_trip_case():
    """5 sequences of 2 genera for grid_cap = 2: blocks 0 and 1 take a second (block 0 a third) sequence."""
    rng = random.Random(77)
    seqs = [rand_seq(rng, 90 + 7 * i) for i in range(5)]
    return Model(seqs, [0, 1, 0, 1, 1], 2)


def score_model(G, seed=5, twins=()):
    """G genera of 2 sequences each (240 bases, 3 % apart from the genus' ancestor); twins = [(a, b)]: genus b is trained on
    genus a's sequences, so their columns are equal."""
    rng = random.Random(seed * 1000 + G)
    anc = [rand_seq(rng, 240) for _ in range(G)]
    seqs, genus = [], []
    for g in range(G):
        src = dict((b, a) for a, b in twins).get(g, g)
        r2 = random.Random(seed * 7919 + src)
        for _ in range(2):
            seqs.append(mutate(r2, anc[src], 0.03))
            genus.append(g)
    mo = Model(seqs, genus, G)
    mo.anc = anc
    for a, b in twins:
        assert a < b and (mo.q[:, a] == mo.q[:, b]).all()
    return mo


def score_queries(mo, twins=()):
    """[(name, sequence)] against score_model(G): the length edges, the last genus, W = 0, and per pair of twins a query
    "tie<a>" drawn from the pair's ancestor: the pair ties at the top of its full score."""
    rng = random.Random(99 + mo.G)
    last = mo.anc[mo.G - 1]
    qs = [("w1", last[10:18]), ("w39", last[20:66]), ("w40", last[20:67]), ("w48", mo.anc[0][5:60]), ("w0_short", "ACGTACG"),
          ("w0_n", "ACGTNACGTNACGTNAC"), ("last_genus", mutate(rng, last, 0.01)), ("first_genus", mutate(rng, mo.anc[0], 0.01)),
          ("mid_n", mo.anc[mo.G // 2][:100] + "N" + mo.anc[mo.G // 2][100:200]), ("lower_u", mo.anc[1][:120].lower().replace("t", "u")),
          ("random", rand_seq(rng, 200)), ("other", mutate(rng, mo.anc[mo.G // 3], 0.05))]
    for a, b in twins:
        qs.append(("tie%d" % a, mutate(rng, mo.anc[a], 0.01)))
        sc = scores(mo.q, word_list(qs[-1][1]))
        assert sc[a] == sc[b] == max(sc) and argmax_low(sc) == a
    W = dict((n, len(word_list(s))) for n, s in qs)
    assert (W["w1"], W["w39"], W["w40"], W["w48"], W["w0_short"], W["w0_n"]) == (1, 39, 40, 48, 0, 0)
    assert (n_draws(1), n_draws(39), n_draws(40), n_draws(48)) == (5, 5, 5, 6)
    assert all(draw(3, 4, t, j, 1) == 0 for t in (0, 99) for j in range(5))
    return qs


# one pair in two chunks (the tie is settled by k_taxa_pick) and one inside a chunk (by the wavefront's reduction)
TWINS = [(3, 69), (5, 6)]
assert 3 // CHUNK != 69 // CHUNK and 5 // CHUNK == 6 // CHUNK


def bound_case():
    """A query of 8 192 bases whose every word has the table's largest-magnitude cell in every genus: training without T, the
    query all T."""
    rng = random.Random(404)
    seqs = [rand_seq(rng, 150, "ACG") for _ in range(6)]
    mo = Model(seqs, [0, 0, 1, 1, 2, 2], 3)
    query = "T" * 8192
    words = word_list(query)
    assert len(words) == 8185 and set(words) == {65535}
    assert (mo.q[65535] == mo.q.min(axis=0)).all() and (mo.q[65535] < 0).all()
    assert abs(int(mo.q.min())) <= 50 * 1024 and 8185 * abs(int(mo.q.min())) < 2 ** 31
    return mo, query


def lineages(n_genera):
    """n_genera six-name paths: two phyla, equal genus names under different families, a name with a space."""
    out = []
    for g in range(n_genera):
        out.append(("Bacteria", "Phylum%d" % (g % 2), "Class%d" % (g % 2), "Order%d" % (g % 2), "Family %d" % (g % 4), "Genus%d" % (g // 4)))
    assert len(set(out)) == n_genera
    return out


def cli_case():
    """A 40-sequence, 6-genus training set as FASTA and taxonomy text (GreenGenes form, with a sequence without a label, a
    label without a sequence and a lineage without a genus, all dropped), and genes to classify, one of them without a word.
    Returns (train_fasta, train_tax, gene_fasta, names, genera sorted, Model, gene names, gene seqs)."""
    rng = random.Random(2024)
    paths = lineages(6)
    genera = sorted(paths)
    anc = [rand_seq(rng, 300) for _ in range(6)]
    fasta, tax, seqs, genus = [], [], [], []
    for i in range(40):
        g = i % 6
        s = mutate(rng, anc[g], 0.04)
        fasta.append(">t%d some text\n%s\n%s\n" % (i, s[:170], s[170:]))
        tax.append("t%d\t%s; s__sp%d\n" % (i, "; ".join(p + n for p, n in zip(("k__", "p__", "c__", "o__", "f__", "g__"), paths[g])), i))
        seqs.append(s)
        genus.append(genera.index(paths[g]))
    fasta.append(">nolabel\n%s\n" % rand_seq(rng, 100))
    fasta.append(">nogenus\n%s\n" % rand_seq(rng, 100))
    tax.append("nogenus\tk__Bacteria; p__P; c__C; o__O; f__F; g__; s__\n")
    tax.append("noseq\tk__Bacteria; p__P; c__C; o__O; f__F; g__G; s__\n")
    assert len(seqs) == 40 and len(set(genus)) == 6
    gene_names = ["gene_%d" % i for i in range(7)] + ["gene_blank"]
    gene_seqs = [mutate(rng, anc[i % 6], 0.02)[10:250] for i in range(6)] + [rand_seq(rng, 150)] + ["N" * 30]
    genes = "".join(">%s\n%s\n" % (n, s) for n, s in zip(gene_names, gene_seqs))
    return "".join(fasta), "".join(tax), genes, genera, Model(seqs, genus, 6), gene_names, gene_seqs


def check_cases_on_the_cpu():
    """Builds every case (each asserts its own properties and the half-integer condition)."""
    counts_case()
    second_trip_case()
    for G in (CHUNK - 1, CHUNK, CHUNK + 1):
        score_queries(score_model(G))
    score_queries(score_model(70, twins=TWINS), twins=TWINS)
    bound_case()
    cli_case()
    return True


assert math.log2(0.5 / (2 ** 24 + 1) / (2 ** 24 + 1)) * 1024 > -50 * 1024      # the sum bound of the contract
