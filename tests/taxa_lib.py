"""The contract of the genus assignment restated plainly -- Python sets and integers, mpmath at 60 digits
for the table (numpy fp64 beside it) -- with the reference scripts' two fixrank parsers, and the named cases of
tests/test_taxa_host.py and tests/test_taxa_gpu.py.  Every named case carries a property check that its input reaches the
edge it is named for.  Nothing here imports the product."""
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


# The exact table.  A cell is decidable when a correct fp64 evaluation cannot round it to the other side: the device computes
#   pw = fl((n + 0.5) / (N + 1))      p = fl(fl(m + pw) / (M + 1))      x = fl(log2(p) * 1024)      q = llrint(x)
# where n + 0.5, N + 1 and M + 1 are exact.  To first order the error of x is at most the sum of
#   - three roundings in p (the two divisions and the sum): 3 * 2^-53 relative in p, that is 3 * 2^-53 / ln 2 absolute in
#     log2 p, times 1024;
#   - the device's fp64 log2, LOG2_ULPS ulps of log2 p: ulp(y) <= 2^-52 |y|, so times 1024 at most LOG2_ULPS * 2^-52 * |x|;
#   - half an ulp of x for the product: 2^-53 * |x| (the product by 1024 is in fact exact; the term is kept).
# |x| <= 50 * 1024 (contract, 3), so E <= 2.9e-11 everywhere.
LOG2_ULPS = 2.0


def table_error_bound(x):
    """E(x) of the comment above, for a cell value or an array of them.  LOG2_ULPS = 2 is an assumption, not a cited figure:
    ROCm ships no document and no header that states the accuracy of the device library's fp64 log2."""
    return 3.0 * 2.0 ** -53 / math.log(2.0) * 1024.0 + (LOG2_ULPS + 0.5) * 2.0 ** -52 * np.abs(x)


def table_exact(n, m, M, N):
    """(q[w][g], d[w][g]): the cell rounded from its exact value, and the exact value's distance from a half-integer.  mpmath
    at 60 digits, once per distinct (n[w], m[w][g], M[g]) -- a case has a few dozen."""
    import mpmath
    bm, bM = int(m.max()) + 1, int(M.max()) + 1
    key = ((n[:, None] * bm + m) * bM + M[None, :]).ravel()
    uniq, inv = np.unique(key, return_inverse=True)
    q_u, d_u = np.empty(len(uniq), dtype=np.int64), np.empty(len(uniq), dtype=np.float64)
    with mpmath.workdps(60):
        for i, k in enumerate(uniq.tolist()):
            nn, mm, Mg = k // (bM * bm), (k // bM) % bm, k % bM
            p = (mm + mpmath.mpf(2 * nn + 1) / (2 * (N + 1))) / (Mg + 1)
            x = mpmath.log(p, 2) * 1024
            lo = mpmath.floor(x)
            q_u[i] = int(lo) + (1 if x - lo > 0.5 else 0)
            d_u[i] = float(abs(x - lo - 0.5))
    return q_u[inv.ravel()].reshape(m.shape), d_u[inv.ravel()].reshape(m.shape)


def exact_checked(n, m, M, N):
    """table_exact with the cap: no cell within E of a half-integer (E at |q| + 1 >= |x|), from the reference alone."""
    q, d = table_exact(n, m, M, N)
    assert (d > table_error_bound(np.abs(q) + 1.0)).all(), "a cell lies within the fp64 error bound of a half-integer: change the case's counts"
    return q, d


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
    """A training set with its restated counts and table: q is the exact table, dist its cells' distances from a
    half-integer, every one beyond the fp64 error bound.  Unless `near_half`, no cell is within 1e-6 either and numpy's fp64
    table is asserted equal to the exact one."""

    def __init__(self, seqs, genus, G, near_half=False):
        self.seqs, self.genus, self.G = seqs, genus, G
        self.n, self.m, self.M, self.N = train_counts(seqs, genus, G)
        self.q, self.dist = exact_checked(self.n, self.m, self.M, self.N)
        if not near_half:
            assert (table(self.n, self.m, self.M, self.N) == self.q).all(), "numpy's fp64 table differs from the exact one"


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
    back = dict((b, a) for a, b in twins)
    for g in range(G):
        src = g
        while src in back:                              # chained twins (a, b), (b, c): c is trained on a's sequences too
            src = back[src]
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


# (N, M, n, m, rounds to): N sequences, M of genus 0, n holding the word, m of them in genus 0, the cell of (word, genus 0)
# lying between 100 E and 1e-7 of a half-integer.  Found by a search with numpy over N <= 320 under m <= n and
# n - m <= N - M (none exists for N <= 160); each confirmed with mpmath at 60 digits, and again by near_half_case().
NEAR_HALF = [(123, 86, 59, 54, -692),      # x = -691.500000027462: rounds down
             (199, 133, 134, 108, -309),   # x = -309.49999999028: rounds up
             (312, 234, 164, 128, -891)]   # x = -891.4999999988582: rounds up


def near_half_case():
    """One training set per NEAR_HALF tuple: N eight-base sequences of one word each, the special word m times in genus 0 and
    n - m times in genus 1, a filler word in the rest of either genus.  m = 128 is 128 workgroups adding to one cell."""
    special, fill0, fill1 = "ACGTTGCA", "GGATCCAA", "CTTAAGTC"
    out, sides = [], set()
    for N, M, n, m, q in NEAR_HALF:
        assert m <= n and n - m <= N - M and m <= M
        seqs = [special] * m + [fill0] * (M - m) + [special] * (n - m) + [fill1] * (N - M - (n - m))
        mo = Model(seqs, [0] * M + [1] * (N - M), 2, near_half=True)
        w = word_of(special)
        assert (mo.N, int(mo.M[0]), int(mo.n[w]), int(mo.m[w, 0])) == (N, M, n, m) and int(mo.q[w, 0]) == q
        d = float(mo.dist[w, 0])
        assert 100.0 * float(table_error_bound(abs(q) + 1.0)) < d < 1e-7
        x = float(table_real(mo.n, mo.m, mo.M, mo.N)[w, 0])
        sides.add(q > x)                                        # True: rounded up
        # every other cell (the fillers, the special word in genus 1, the absent words) is far from a half-integer
        others = mo.dist.copy()
        others[w, 0] = 1.0
        assert others.min() > 1e-6
        out.append(mo)
    assert sides == {True, False}
    return out


def lane_stretches(L):
    """k_taxa_words' split of a sequence of L bases: (nw, per, [(wa, wb) per lane]); a lane with wb <= wa is idle, a live lane
    reads bases wa .. wb + 6."""
    nw = L - K + 1
    per = (nw + 63) // 64
    return nw, per, [(lane * per, min(lane * per + per, nw)) for lane in range(64)]


def distinct_seq(rng, L, implant=None):
    """L random bases whose words are all different; implant = (position, 8 bases) is written over them first."""
    while True:
        s = rand_seq(rng, L)
        if implant:
            s = s[:implant[0]] + implant[1] + s[implant[0] + K:]
        if len(set(word_list(s))) == L - K + 1:
            return s


def with_n(base, pos):
    """base with an N at pos; asserts that exactly the windows holding pos are gone, and returns them."""
    nw = len(base) - K + 1
    gone = list(range(max(0, pos - K + 1), min(pos, nw - 1) + 1))
    s = base[:pos] + "N" + base[pos + 1:]
    assert word_list(s) == [w for i, w in enumerate(word_list(base)) if i not in gone]
    return s, gone


def seam_case():
    """The lane seams of k_taxa_words in one training set of 4 genera; every sequence but the homopolymer has only distinct
    words, so a lost or an invented window changes a count.  mo.names names the sequences in the order of the buffer."""
    rng = random.Random(1312)
    rows = []                                                   # (name, sequence, genus)
    # window counts: all lanes but one idle, one idle, none idle, two windows in some lanes and one in the next, ...
    for i, nw in enumerate((64 * 3 + 1, 1, 63, 64, 65, 127, 128, 129)):
        rows.append(("nw%d" % nw, distinct_seq(rng, nw + K - 1), i % 3))
    assert [r[0] for r in rows[:2]] == ["nw193", "nw1"]         # grid_cap 1: the shortest right behind the longest
    live = lambda L: [lane for lane, (wa, wb) in enumerate(lane_stretches(L)[2]) if wb > wa]
    assert live(1 + 7) == [0] and live(63 + 7) == list(range(63)) and live(64 + 7) == list(range(64))
    nw, per, st = lane_stretches(65 + 7)
    assert per == 2 and live(65 + 7) == list(range(33)) and st[31] == (62, 64) and st[32] == (64, 65)      # lane 32: a single window; 33..63 idle
    nw, per, st = lane_stretches(127 + 7)
    assert per == 2 and live(127 + 7) == list(range(64)) and st[63] == (126, 127)                          # the last lane is short
    assert lane_stretches(128 + 7)[1] == 2 and lane_stretches(128 + 7)[2][63] == (126, 128)
    nw, per, st = lane_stretches(129 + 7)
    assert per == 3 and live(129 + 7) == list(range(43)) and st[42] == (126, 129) and st[43][0] == 129     # 43 full lanes end at nw; 43..63 idle
    nw, per, st = lane_stretches(193 + 7)
    assert per == 4 and live(193 + 7) == list(range(49)) and st[48] == (192, 193)                          # lane 48: a single window
    # one N per sequence at a seam of lane 1, lane 32 and the last live lane (50: a short stretch, lanes 51..63 idle)
    L = 209
    nw, per, st = lane_stretches(L)
    assert (nw, per) == (202, 4) and live(L)[-1] == 50 and st[50] == (200, 202) and st[50][1] + 6 == L - 1
    for lane in (1, 32, 50):
        wa, wb = st[lane]
        for what, pos in (("wa", wa), ("wa-1", wa - 1), ("wa+7", wa + 7), ("wb+6", wb + 6)):
            s, gone = with_n(distinct_seq(rng, L), pos)
            own = [i for i in gone if wa <= i < wb]
            if what == "wa":                                    # the lane's first window and the 7 before it, of the lanes in front
                assert gone == list(range(max(0, wa - 7), wa + 1)) and own == [wa]
            elif what == "wa-1":                                # nothing of the lane: the last 8 windows of the lanes in front
                assert gone == list(range(max(0, wa - 8), wa)) and own == []
            elif what == "wa+7":                                # the lane's whole stretch: its first window's last base
                assert gone[0] == wa and own == list(range(wa, wb)) and gone[-1] == min(wa + 7, nw - 1)
            else:                                               # the last base the lane reads: of its own windows only the last
                assert gone[0] == wb - 1 and own == [wb - 1] and gone[-1] == min(wb + 6, nw - 1)
            rows.append(("n_lane%d_%s" % (lane, what), s, (lane + pos) % 3))
    # a word whose only occurrence is a lane's last window (it ends at the last base the lane reads) in one sequence, and the
    # next lane's first window in another; a third genus holds it too, so n = 3 and m = 1 in each
    X = "GATTACAG"
    wa, wb = lane_stretches(200)[2][5]
    assert (wa, wb) == (20, 24) and lane_stretches(200)[2][6][0] == 24
    for name, pos, g in (("straddle_last", wb - 1, 0), ("straddle_first", wb, 1)):
        s = distinct_seq(rng, 200, (pos, X))
        assert [i for i, w in enumerate(word_list(s)) if w == word_of(X)] == [pos]
        rows.append((name, s, g))
    rows.append(("straddle_other", "GG" + X + "CC", 2))
    # every lane sets the same bit
    rows.append(("homopolymer", "A" * 200, 3))
    # the last live lane ends at the sequence's end with another genus' bases behind it in the buffer, and at the buffer's end
    at = [r[0] for r in rows].index("nw128")
    rows.append(rows.pop(at))
    rows.append(("edge_last", distinct_seq(rng, 64 + K - 1), 3))
    mo = Model([r[1] for r in rows], [r[2] for r in rows], 4)
    mo.names = [r[0] for r in rows]
    for name in ("nw128", "edge_last"):
        i = mo.names.index(name)
        nw, per, st = lane_stretches(len(mo.seqs[i]))
        assert st[63][1] == nw and st[63][1] + 6 == len(mo.seqs[i]) - 1                 # lane 63 reads the very last base
    i = mo.names.index("nw128")
    assert mo.names[i + 1] == "edge_last" and mo.genus[i + 1] != mo.genus[i] and i + 2 == mo.N
    assert word_of(mo.seqs[i][-7:] + mo.seqs[i + 1][0]) not in word_list(mo.seqs[i])    # one base too far would add a word
    w = word_of(X)
    assert int(mo.n[w]) == 3 and mo.m[w].tolist() == [1, 1, 1, 0]
    i = mo.names.index("homopolymer")
    assert set(word_list(mo.seqs[i])) == {0} and len(word_list(mo.seqs[i])) == 193 and int(mo.m[0, 3]) == 1 and int(mo.n[0]) == 1
    for name, s in zip(mo.names, mo.seqs):
        assert name == "homopolymer" or len(set(word_list(s))) == len(word_list(s)) > 0
    return mo


SEAM_JUNK = "ACGTA"               # in front of the text of the offset call: valid bases, so an offset ignored would show


# The score kernel's shapes.  The call returns winners, not scores, so a word lost from a sum shows only where it decides:
# a "decisive" query is made of words that no training sequence holds -- every genus gets the same cell for them -- but one,
# held by a single genus c > 0.  With that word c wins, without it all genera tie and genus 0 does; a trial is won by c if one
# of its draws hits the word's position and by 0 otherwise.

def decisive_query(mo, rng, W, p, c, split=0):
    """A query of W words whose word p is held by genus c alone and whose other words by nobody; split > 0: an N after the
    first `split` words, which are then a run of their own.  Asserts what it claims from the reference scores."""
    assert 0 <= split <= p < W and c > 0
    absent = mo.n == 0
    own = [w for s, g in zip(mo.seqs, mo.genus) if g == c for w in word_list(s) if mo.n[w] == mo.m[w, c]]
    assert own

    def run(nwords, at, X):
        """nwords + 7 bases, every window absent from the training set but window `at`, which is X: depth first, a base at a
        time.  Some 60 % of the 65 536 words are absent from a 70-genus training set, so away from X one of the four bases
        nearly always fits and the search hardly backs up: about nwords + 7 steps.  The 7 windows on either side of X hold
        some of its bases; where none of the bases before X fits them the search would back up without end, so after
        200 000 steps (a hundred times the longest run) it gives up and the caller takes the genus' next word for X."""
        L, seq, choices, steps = nwords + K - 1, [], [], 0
        while len(seq) < L:
            i = len(seq)
            if len(choices) == i:
                opts = [CODE[X[i - at]]] if at is not None and at <= i < at + K else rng.sample(range(4), 4)
                choices.append(opts)
            steps += 1
            if steps > 200000:
                return None
            while choices[i]:
                b = choices[i].pop()
                if i < K - 1 or i - (K - 1) == at or absent[sum(v << (2 * (K - 1 - k)) for k, v in enumerate(seq[i - K + 1:] + [b]))]:
                    seq.append(b)
                    break
            else:
                choices.pop()
                if not seq:
                    return None
                seq.pop()
        return "".join("ACGT"[v] for v in seq)

    head = run(split, None, None) + "N" if split else ""
    for w in own:
        X = "".join("ACGT"[(w >> (2 * (K - 1 - k))) & 3] for k in range(K))
        tail = run(W - split, p - split, X)
        if tail is not None:
            break
    else:
        raise AssertionError("no decisive word of genus %d fits" % c)
    query = head + tail
    words = word_list(query)
    assert len(words) == W and words[p] == w and words.count(w) == 1
    assert argmax_low(scores(mo.q, words)) == c and len(set(scores(mo.q, words[:p] + words[p + 1:]))) == 1
    return query


SCORE_WAVES, STAGE = 4, 256        # k_taxa_score: wavefronts that split the full score by position; words staged per round
# W: (draws, per, the start of each wavefront's range clipped to W -- a start equal to W is a wavefront without a word)
LENGTHS = {2: (5, 1, [0, 1, 2, 2]), 3: (5, 1, [0, 1, 2, 3]), 4: (5, 1, [0, 1, 2, 3]), 5: (5, 2, [0, 2, 4, 5]), 7: (5, 2, [0, 2, 4, 6]),
           8: (5, 2, [0, 2, 4, 6]), 255: (31, 64, [0, 64, 128, 192]), 256: (32, 64, [0, 64, 128, 192]), 257: (32, 65, [0, 65, 130, 195]),
           1023: (127, 256, [0, 256, 512, 768]), 1024: (128, 256, [0, 256, 512, 768]), 1025: (128, 257, [0, 257, 514, 771])}


def wave_ranges(W):
    per = (W + SCORE_WAVES - 1) // SCORE_WAVES
    return per, [(min(v * per, W), min(v * per + per, W)) for v in range(SCORE_WAVES)]


def lengths_case(mo):
    """[(name, query)] against score_model(70, twins=TWINS) in the order of one call: per W of LENGTHS a query "c<W>" cut from
    ancestors and decisive queries "d<W>_<p>" with the deciding word last (a wavefront range cut short loses it) and, from
    255 on, first in the last wavefront's range; behind the 8 185 words of bound_case's query come the shortest lists."""
    rng = random.Random(4100 + mo.G)
    assert mo.G == 70
    for W, (D, per, starts) in LENGTHS.items():
        got_per, ranges = wave_ranges(W)
        assert n_draws(W) == D and got_per == per and [a for a, _ in ranges] == starts and ranges[3][1] == W
        assert all(b - a == per for a, b in ranges[:3] if b < W) and sum(b - a for a, b in ranges) == W
    assert wave_ranges(2) == (1, [(0, 1), (1, 2), (2, 2), (2, 2)])          # two wavefronts without a word
    assert wave_ranges(3) == (1, [(0, 1), (1, 2), (2, 3), (3, 3)])
    assert wave_ranges(5) == (2, [(0, 2), (2, 4), (4, 5), (5, 5)])          # a short range and an empty one
    assert wave_ranges(7) == (2, [(0, 2), (2, 4), (4, 6), (6, 7)])          # a short last range
    assert wave_ranges(257)[0] == 65 and wave_ranges(1025) == (257, [(0, 257), (257, 514), (514, 771), (771, 1025)])
    long_anc = "".join(mo.anc[10:16])
    qs = {"w0_short": "ACGTACG", "w0_n": "ACGTNACGTNACGTNAC", "long": "T" * 8192}
    c = 20
    for W in LENGTHS:
        qs["c%d" % W] = (mo.anc[mo.G - 2][10:] if W <= 8 else long_anc)[:W + K - 1]
        assert len(word_list(qs["c%d" % W])) == W
        spots = [W - 1] + ([wave_ranges(W)[1][3][0]] if W >= 255 else [])
        for p in spots:
            c += 1
            assert c not in (a for pair in TWINS for a in pair)
            qs["d%d_%d" % (W, p)] = decisive_query(mo, rng, W, p, c, split=400 if W == 1025 else 0)
    assert qs["d1025_1024"].count("N") == 1 and len(qs["d1025_1024"]) == 400 + 7 + 1 + 625 + 7
    assert {"d257_256", "d1025_1024", "d1024_768", "d1023_768"} <= set(qs) and 768 % STAGE == 0    # the first word of a staging round
    for W in (2, 3):                                                        # no word summed leaves genus 0 the winner: these two say otherwise
        assert argmax_low(scores(mo.q, word_list(qs["c%d" % W]))) == mo.G - 2
    big = [n for W in LENGTHS if W >= 255 for n in qs if n[1:].split("_")[0] == str(W)]
    small = [n for W in LENGTHS if W <= 8 for n in ("d%d_%d" % (W, W - 1), "c%d" % W)]
    order = ["w0_short"] + big + ["long", small[0], small[1], "w0_n"] + small[2:]
    assert sorted(order) == sorted(qs) and order[order.index("long") + 1] == "d2_1"
    return [(n, qs[n]) for n in order]


# G = 193: three full chunks and a fourth with one live lane, genus 192.  3 = 70 = 140 ties over chunks 0, 1 and 2, 5 = 190
# over chunks 0 and 2, 80 = 150 has its lower member in chunk 1, 130 = 131 lies inside chunk 2.
TWINS3 = [(3, 70), (70, 140), (5, 190), (80, 150), (130, 131)]
assert [g // CHUNK for g in (3, 70, 140, 5, 190, 80, 150, 130, 131, 193 // 2, 192)] == [0, 1, 2, 0, 2, 1, 2, 2, 2, 1, 3]


def genera_queries(mo, twins=()):
    """[(name, sequence)] for a score_model of any G >= 1: a query drawn from the first, the middle and the last genus'
    ancestor, a short and a random one, and per root of a set of twins a query "tie<a>" that the whole set ties on."""
    rng = random.Random(500 + mo.G)
    qs = [("first", mutate(rng, mo.anc[0], 0.01)), ("middle", mutate(rng, mo.anc[mo.G // 2], 0.01)), ("last", mutate(rng, mo.anc[mo.G - 1], 0.01)),
          ("short", mo.anc[mo.G - 1][30:40]), ("random", rand_seq(rng, 150)), ("w0", "ACGTNACG")]
    sc = dict((n, scores(mo.q, word_list(s))) for n, s in qs)
    assert argmax_low(sc["first"]) == 0 and argmax_low(sc["middle"]) == mo.G // 2 and argmax_low(sc["last"]) == mo.G - 1
    assert sc["first"].count(max(sc["first"])) == 1 or mo.G == 1
    sets = {}
    for a, b in twins:
        root = [r for r, s in sets.items() if a in s]
        sets.setdefault(root[0] if root else a, [a]).append(b)
    for a, members in sorted(sets.items()):
        qs.append(("tie%d" % a, mutate(rng, mo.anc[a], 0.01)))
        sc = scores(mo.q, word_list(qs[-1][1]))
        assert [g for g in range(mo.G) if sc[g] == max(sc)] == sorted(members) and argmax_low(sc) == a == min(members)
    return qs


_MODELS = {}


def shared_model(G, twins=()):
    """score_model(G, twins=twins), built once for all the tests that read it; none changes it."""
    k = (G, tuple(twins))
    if k not in _MODELS:
        _MODELS[k] = score_model(G, twins=twins)
    return _MODELS[k]


def forget_models():
    """Lets go of the shared models (m, q and dist are 65 536 x G each): called where the tests that read them end."""
    _MODELS.clear()


def max_trials_queries(mo):
    """The three queries of the 1 024-trial call: W = 1, 48 and the longest, 8 185 words cut from every ancestor in turn so
    that a trial's winner depends on its 1 023 draws."""
    qs = [("w1", mo.anc[mo.G - 1][10:18]), ("w48", mo.anc[0][5:60]), ("w8185", "".join(a[:118] for a in mo.anc)[:8192])]
    words = word_list(qs[2][1])
    assert [len(word_list(s)) for _, s in qs] == [1, 48, 8185] and len(qs[2][1]) == 8192 and n_draws(8185) == 1023
    assert 1023 * 65536 + 1022 + 1 < 2 ** 32 and len(set(words)) > 4000
    # the draws of two trials pick different genera: trial 0 and trial 1 023 are not won by the same one throughout
    sc = [argmax_low(scores(mo.q, [words[draw(1, 2, t, j, 8185)] for j in range(1023)])) for t in (0, 1, 2, 1023)]
    assert len(set(sc)) > 1
    return qs


# (name, the key of every query or None for the hash of its name, seed): seed ^ key is 0, its complement, and all ones
KEY_SEEDS = [("key_0", 0, 20240), ("key_max", MASK, 20240), ("seed_max", None, MASK), ("seed_is_key", 977, 977)]


def keys_case(mo, qs):
    """{setting: [(best, winners, W)]} of queries qs under KEY_SEEDS; the sum in draw() wraps, and the settings draw differently."""
    exp = {}
    for name, key, seed in KEY_SEEDS:
        exp[name] = [classify(mo.q, s, fnv1a64(n.encode()) if key is None else key, seed) for n, s in qs]
    assert ((MASK ^ 20240) + 0x9E3779B97F4A7C15) > MASK and (20240 + 101 * 65536 * 0x9E3779B97F4A7C15) > MASK      # the sum wraps
    win = [[r[1] for r in exp[name]] for name, _, _ in KEY_SEEDS]
    assert all(win[i] != win[j] for i in range(4) for j in range(i)), "two settings draw the same"
    assert len({tuple(r[0] for r in exp[name]) for name in exp}) == 1                   # the assignment has no draw in it
    return exp


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
    near_half_case()
    seam_case()
    twins = shared_model(70, TWINS)
    lengths_case(twins)
    max_trials_queries(twins)
    keys_case(twins, score_queries(twins, TWINS))
    for G in (1, 2, 2 * CHUNK, 2 * CHUNK + 1):
        genera_queries(shared_model(G))
    genera_queries(shared_model(3 * CHUNK + 1, TWINS3), TWINS3)
    forget_models()
    return True


assert math.log2(0.5 / (2 ** 24 + 1) / (2 ** 24 + 1)) * 1024 > -50 * 1024      # the sum bound of the contract
