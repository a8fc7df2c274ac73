"""The plain restatement of DESIGN.md §8.16 (gene against gene: exact edit distances, the pairs within an identity, greedy
OTUs, the OTU matrix) and the named edge cases the host and GPU tests of it share.  Written from the contract, not from
rambl_amd/otu.py or sc_pairs_core.hpp; numpy and the standard library only."""
import decimal
import functools
import math
import random

import numpy as np

MAX_LEN = 2048
GRID_TILES = 4096          # the blocks of a launch at most: more tiles go round the grid-stride loop


# ---- the contract, restated

def _codes(seq, other):
    """A C G T in either case as 0..3, every other byte as `other`."""
    table = np.full(256, other, dtype=np.int16)
    for k, c in enumerate(b"ACGT"):
        table[c] = table[c + 32] = k
    return table[np.frombuffer(bytes(seq), dtype=np.uint8)]


def _rows(pattern, text):
    """The rows D[i][0..len(text)] of the unit-cost table, i = 0..len(pattern), one at a time.  "Other" bytes get different
    codes on the two sides, so they match nothing."""
    ca, cb = _codes(pattern, 4), _codes(text, 5)
    idx = np.arange(len(cb) + 1, dtype=np.int64)
    row = idx.copy()
    yield row
    for i in range(1, len(ca) + 1):
        t = np.empty(len(cb) + 1, dtype=np.int64)
        t[0] = i
        np.minimum(row[:-1] + (cb != ca[i - 1]), row[1:] + 1, out=t[1:])          # substitution or match; deletion
        row = np.minimum.accumulate(t - idx) + idx                                # the insertion chain along the row
        yield row


@functools.lru_cache(maxsize=None)
def _distance(a, b):
    for row in _rows(a, b):
        pass
    return int(row[-1])


def edit_distance(a, b):
    """ed(a, b): whole sequences, substitution, insertion and deletion 1 each, no free end gaps.  The rows run over the
    shorter sequence (the distance is symmetric: a byte matches by the same rule from either side)."""
    a, b = bytes(a), bytes(b)
    assert 1 <= len(a) <= MAX_LEN and 1 <= len(b) <= MAX_LEN
    return _distance(a, b) if len(a) <= len(b) else _distance(b, a)


def literal_distance(a, b):
    """The same by a literal O(nm) double loop, for short sequences."""
    def code(x, other):
        return "ACGT".find(chr(x).upper()) if chr(x).upper() in "ACGT" else other
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (code(a[i - 1], -1) != code(b[j - 1], -2)), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[len(a)][len(b)]


def seam_differences(pattern, text):
    """The set of horizontal differences D[64k][j] - D[64k][j-1] over the block seams 64k (1 <= 64k < len(pattern)) and all j."""
    seen = set()
    for i, row in enumerate(_rows(bytes(pattern), bytes(text))):
        if i % 64 == 0 and 0 < i < len(pattern):
            seen |= set(np.diff(row).tolist())
    return seen


def substitution_distance(a, b):
    """Equal lengths: the positions that do not match."""
    assert len(a) == len(b)
    return int(np.count_nonzero(_codes(a, 4) != _codes(b, 5)))


def bound(len_a, len_b, diff_num, diff_den):
    return (max(len_a, len_b) * diff_num) // diff_den          # Python integers: no width to overflow


def candidates(lengths, diff_num, diff_den):
    """[(a, b)], a < b: the pairs the length prefilter leaves."""
    return [(a, b) for a in range(len(lengths)) for b in range(a + 1, len(lengths))
            if abs(lengths[a] - lengths[b]) <= bound(lengths[a], lengths[b], diff_num, diff_den)]


def pairs_within(genes, diff_num, diff_den):
    """[(a, b, ed)] of every pair a < b with ed(a, b) <= bound(a, b), sorted by (a, b)."""
    out = []
    for a, b in candidates([len(g) for g in genes], diff_num, diff_den):
        d = edit_distance(genes[a], genes[b])
        if d <= bound(len(genes[a]), len(genes[b]), diff_num, diff_den):
            out.append((a, b, d))
    return out


def walk_order(names, lengths, weights):
    """The genes by (weight descending, length descending, name bytes ascending)."""
    return sorted(range(len(names)), key=lambda g: (-weights[g], -lengths[g], names[g].encode()))


def greedy_otus(names, lengths, weights, pairs):
    """[(gene name, centroid name, ed)] in the genes' input order.  pairs: [(a, b, ed)], the qualifying pairs by index.  A gene
    joins the centroid it qualifies with whose ed / max(len) is smallest (cross-multiplied), the one made first on a tie; a
    centroid maps to itself with 0."""
    ed = {}
    for a, b, d in pairs:
        ed[(a, b)] = ed[(b, a)] = d
    centroids, out = [], {}
    for g in walk_order(names, lengths, weights):
        best = None
        for c in centroids:
            if (g, c) not in ed:
                continue
            d, L = ed[(g, c)], max(lengths[g], lengths[c])
            if best is None or d * best[2] < best[1] * L:          # d / L < best d / best L
                best = (c, d, L)
        if best is None:
            centroids.append(g)
            out[g] = (names[g], names[g], 0)
        else:
            out[g] = (names[g], names[best[0]], best[1])
    return [out[g] for g in range(len(names))]


def centroids_in_order(names, lengths, weights, mapping):
    """The centroid names in the order they were made."""
    is_centroid = {c for _, c, _ in mapping}
    return [names[g] for g in walk_order(names, lengths, weights) if names[g] in is_centroid]


def count_text(v):
    """A count as the per-sample tables print it: rounded to 3 decimals, halves away from zero, then repr."""
    return repr(float(decimal.Decimal(v).quantize(decimal.Decimal("0.001"), rounding=decimal.ROUND_HALF_UP)))


def matrix_rows(matrix_text):
    """(header line, {gene: [cells as float]}) of a gene_count_matrix.tsv."""
    lines = matrix_text.splitlines()
    return lines[0], {f[0]: [float(x) for x in f[1:]] for f in (ln.split("\t") for ln in lines[1:])}


def row_weights(matrix_text, names):
    _, rows = matrix_rows(matrix_text)
    return [math.fsum(rows[n]) for n in names]


def otu_matrix_text(matrix_text, mapping):
    """The header as it is; one row per centroid in byte order of the name, every cell the sum of the members' cells added in
    mapping order."""
    header, rows = matrix_rows(matrix_text)
    sums = {}
    for gene, centroid, _ in mapping:
        acc = sums.setdefault(centroid, [0.0] * (len(header.split("\t")) - 1))
        for k, v in enumerate(rows[gene]):
            acc[k] += v
    return header + "\n" + "".join("\t".join([c] + [count_text(v) for v in sums[c]]) + "\n" for c in sorted(sums, key=lambda n: n.encode()))


def otu_map_text(names, lengths, mapping):
    length = dict(zip(names, lengths))
    return "gene\totu\tedit_distance\tgene_length\totu_length\n" + "".join(
        "%s\t%s\t%d\t%d\t%d\n" % (g, c, d, length[g], length[c]) for g, c, d in mapping)


def otus_fasta_text(names, seqs, lengths, weights, mapping):
    seq = dict(zip(names, seqs))
    return "".join(">%s\n%s\n" % (c, seq[c]) for c in centroids_in_order(names, lengths, weights, mapping))


def pairs_text(names, pairs):
    return "a\tb\tedit_distance\n" + "".join("%s\t%s\t%d\n" % (names[a], names[b], d) for a, b, d in pairs)


# ---- sequences

def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other_base(rng, c):
    return rng.choice([x for x in b"ACGT" if x != c])


def substitute(rng, seq, positions):
    s = bytearray(seq)
    for p in positions:
        s[p] = other_base(rng, s[p])
    return bytes(s)


def mutate(rng, seq, n_edits, keep_length=False):
    """n_edits random substitutions, insertions and deletions (substitutions only with keep_length); never empty."""
    s = bytearray(seq)
    for _ in range(n_edits):
        op = 0 if keep_length else rng.randrange(3)
        p = rng.randrange(len(s))
        if op == 0:
            s[p] = other_base(rng, s[p])
        elif op == 1 and len(s) < MAX_LEN:
            s.insert(p, rng.choice(b"ACGT"))
        elif op == 2 and len(s) > 1:
            del s[p]
    return bytes(s)


def families(seed, n_families, per_family, length, n_edits):
    """(names, seqs): n_families random genes of about `length` bases with per_family - 1 near-copies each."""
    rng = random.Random(seed)
    names, seqs = [], []
    for f in range(n_families):
        root = rand_seq(rng, length + rng.randrange(-3, 4))
        for k in range(per_family):
            names.append("fam%02d_%d" % (f, k))
            seqs.append(root if k == 0 else mutate(rng, root, rng.randrange(1, n_edits + 1)))
    return names, seqs


# ---- named edges of the distance

class Edge:
    """genes: a list of sequences; pairs: (pattern index, text index) into it; prop(edge): asserts, by the restatement alone,
    that the input reaches its edge."""

    def __init__(self, name, genes, pairs, prop=None):
        self.name, self.genes, self.pairs, self.prop = name, list(genes), list(pairs), prop

    def expected(self):
        return [edit_distance(self.genes[a], self.genes[b]) for a, b in self.pairs]

    def check(self):
        for a, b in self.pairs:
            assert 0 <= a < len(self.genes) and 0 <= b < len(self.genes)
        for g in self.genes:
            assert 1 <= len(g) <= MAX_LEN, self.name
        if self.prop:
            self.prop(self)


def edge_lengths(widths):
    return sorted({1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048} | {64 * w + d for w in widths for d in (-1, 0, 1) if 64 * w + d <= MAX_LEN})


def _prop_distances(want):
    def prop(e):
        assert e.expected() == want(e), e.name
    return prop


def _prop_top_word(e):
    (a, b), = e.pairs
    assert len(e.genes[a]) == 65 and edit_distance(e.genes[a], e.genes[b]) != edit_distance(e.genes[a][:64], e.genes[b])


def _prop_seams(e):
    (a, b), = e.pairs
    assert seam_differences(e.genes[a], e.genes[b]) == {-1, 0, 1}


def _prop_shift(h):
    def prop(e):
        (a, b), = e.pairs
        assert len(e.genes[a]) == len(e.genes[b])
        d = edit_distance(e.genes[a], e.genes[b])
        assert d == 2 * h and d < substitution_distance(e.genes[a], e.genes[b]), (e.name, d)
    return prop


def _prop_wave(e):
    assert len(e.pairs) == 64 and len({a for a, _ in e.pairs}) == 1
    lens = [len(e.genes[b]) for _, b in e.pairs]
    assert min(lens) == 1 and max(lens) == MAX_LEN and len(set(lens)) == 64


def _prop_symmetric(e):
    assert {(b, a) for a, b in e.pairs} == set(e.pairs) and all(a != b for a, b in e.pairs)
    want = e.expected()
    assert all(want[k] == want[e.pairs.index((b, a))] for k, (a, b) in enumerate(e.pairs))


def _prop_grid(e):
    assert len({a for a, _ in e.pairs}) > GRID_TILES          # one tile per pattern at least


@functools.lru_cache(maxsize=None)
def distance_edges(widths):
    """The named edges of the distance for the instantiated W list `widths` (a tuple)."""
    rng = random.Random(8160)
    edges = []
    for n in edge_lengths(widths):
        x = rand_seq(rng, n)
        y = mutate(rng, x, 1 + n // 50)
        z = rand_seq(rng, max(1, min(MAX_LEN, n + rng.randrange(-2, 3))))
        edges.append(Edge("length %d, both ways" % n, [x, y, z], [(0, 1), (1, 0), (0, 2), (2, 0)]))
    lo, hi = rand_seq(rng, 1), rand_seq(rng, MAX_LEN)
    edges.append(Edge("1 against 2048 and back", [lo, hi], [(0, 1), (1, 0)],
                      _prop_distances(lambda e: [MAX_LEN - (lo.upper() in hi.upper())] * 2)))
    for n in (1, 64, 65, 1500, MAX_LEN):
        x = rand_seq(rng, n)
        edges.append(Edge("identical, %d bases" % n, [x, bytes(x)], [(0, 1)], _prop_distances(lambda e: [0])))
    for n, k in ((1, 1), (64, 65), (130, 7), (MAX_LEN, 1000)):
        edges.append(Edge("all A (%d) against all C (%d)" % (n, k), [b"A" * n, b"C" * k], [(0, 1), (1, 0)],
                          _prop_distances(lambda e, n=n, k=k: [max(n, k)] * 2)))
    edges.append(Edge("one-base pattern", [b"G", rand_seq(rng, 300) + b"G", b"ACTTCA"], [(0, 1), (0, 2), (0, 0)],
                      _prop_distances(lambda e: [300, 6, 0])))
    for n in (200, 64 * widths[0] + 9):
        x = rand_seq(rng, n)
        for p in (0, 63, 64, n - 1):
            variants = [substitute(rng, x, [p]), x[:p] + bytes([other_base(rng, x[p])]) + x[p:], x[:p] + x[p + 1:]]
            edges.append(Edge("one substitution, insertion, deletion at %d of %d" % (p, n), [x] + variants, [(0, 1), (0, 2), (0, 3)],
                              _prop_distances(lambda e: [1, 1, 1])))
    x = rand_seq(rng, 65)
    edges.append(Edge("65-base pattern: one valid bit in the top word", [x, substitute(rng, x, [10])], [(0, 1)], _prop_top_word))
    x = rand_seq(rng, 200)
    edges.append(Edge("carries between words: -1, 0 and +1 at a seam", [x, x[70:140] + rand_seq(rng, 40) + x[:60]], [(0, 1)], _prop_seams))
    for h in (1, 31, 32, 33):
        core = rand_seq(rng, 400)
        edges.append(Edge("shifted by %d" % h, [rand_seq(rng, h) + core, core + rand_seq(rng, h)], [(0, 1)], _prop_shift(h)))
    x = rand_seq(rng, 90)
    with_n = x[:40] + b"N" + x[41:]
    edges.append(Edge("N in both at the same place counts 1", [with_n, bytes(with_n)], [(0, 1), (0, 0)], _prop_distances(lambda e: [1, 1])))
    edges.append(Edge("lower case against upper case counts 0", [x, x.lower(), x.swapcase()], [(0, 1), (1, 2)], _prop_distances(lambda e: [0, 0])))
    edges.append(Edge("a whole sequence of N", [b"N" * 70, b"N" * 70, x, b"n" * 3], [(0, 1), (0, 2), (2, 0), (3, 3)],
                      _prop_distances(lambda e: [70, 90, 90, 3])))
    root = rand_seq(rng, MAX_LEN)
    lens = [1, MAX_LEN] + [1 + (k * (MAX_LEN - 1)) // 63 for k in range(1, 63)]
    texts = [mutate(rng, root[:n], n // 40, keep_length=True) for n in lens]
    edges.append(Edge("one wavefront, text lengths 1 to 2048", [root] + texts, [(0, 1 + k) for k in range(64)], _prop_wave))
    x, y = rand_seq(rng, 150), rand_seq(rng, 700)
    edges.append(Edge("(a, b) and (b, a) in one call", [x, y, mutate(rng, y, 9)], [(0, 1), (1, 0), (1, 2), (2, 1)], _prop_symmetric))
    edges.append(Edge("a == b", [x, with_n], [(0, 0), (1, 1)], _prop_distances(lambda e: [0, 1])))
    tiny = [rand_seq(rng, 1 + k % 3) for k in range(GRID_TILES + 5)]
    edges.append(Edge("more tiles than one grid trip", tiny, [(k, (7 * k + 1) % len(tiny)) for k in range(len(tiny))], _prop_grid))
    assert len({e.name for e in edges}) == len(edges)
    return edges


def flatten(edges):
    """(genes, pairs, expected) of several edges as one call: the edges' genes back to back, their pairs re-indexed."""
    genes, pairs, want = [], [], []
    for e in edges:
        pairs += [(a + len(genes), b + len(genes)) for a, b in e.pairs]
        genes += e.genes
        want += e.expected()
    return genes, pairs, want


# ---- named edges of the pair list

class ListEdge:
    """genes, the difference rate, and prop(edge) as above.  expected(): the restatement's list."""

    def __init__(self, name, genes, diff_num, diff_den, prop=None):
        self.name, self.genes, self.diff_num, self.diff_den, self.prop = name, list(genes), diff_num, diff_den, prop

    def expected(self):
        return pairs_within(self.genes, self.diff_num, self.diff_den)

    def check(self):
        if self.prop:
            self.prop(self)


def _prop_expected(pred):
    def prop(e):
        assert pred(e.expected()), e.name
    return prop


def _prop_first_pattern_candidates(k):
    def prop(e):
        lens = [len(g) for g in e.genes]
        first = min(range(len(lens)), key=lambda g: (lens[g], g))          # the pattern the length order puts first
        assert sum(1 for a, b in candidates(lens, e.diff_num, e.diff_den) if first in (a, b)) == k
        assert 0 < len(e.expected()) < len(lens) * (len(lens) - 1) // 2
    return prop


def _prop_length_gap(e):
    lens = [len(g) for g in e.genes]
    assert lens[1] - lens[0] == bound(lens[0], lens[1], e.diff_num, e.diff_den)
    assert lens[2] - lens[0] == bound(lens[0], lens[2], e.diff_num, e.diff_den) + 1
    assert (0, 1) in candidates(lens, e.diff_num, e.diff_den) and (0, 2) not in candidates(lens, e.diff_num, e.diff_den)
    assert [(a, b) for a, b, _ in e.expected()] == [(0, 1), (1, 2)]


def _prop_ed_at_bound(e):
    b = bound(len(e.genes[0]), len(e.genes[1]), e.diff_num, e.diff_den)
    assert edit_distance(e.genes[0], e.genes[1]) == b and edit_distance(e.genes[0], e.genes[2]) == b + 1
    assert (0, 1, b) in e.expected() and not [p for p in e.expected() if p[:2] == (0, 2)]


def _prop_dereplication(e):
    assert e.diff_num == 0 and e.expected() == [(0, 1, 0), (0, 4, 0), (1, 4, 0)]
    assert e.genes[2] == e.genes[3] and edit_distance(e.genes[2], e.genes[3]) == 1          # copies that hold an N never merge


def _prop_needs_64_bits(e):
    n = max(len(g) for g in e.genes)
    assert n * e.diff_num >= 1 << 32 and e.diff_num < 1 << 31 and e.diff_den < 1 << 31
    wrapped = ((n * e.diff_num) % (1 << 32)) // e.diff_den
    d = edit_distance(e.genes[0], e.genes[1])
    assert wrapped < d <= bound(n, n, e.diff_num, e.diff_den) and e.expected() == [(0, 1, d)]


@functools.lru_cache(maxsize=None)
def list_edges():
    rng = random.Random(8161)
    edges = [ListEdge("one gene", [rand_seq(rng, 50)], 3, 100, _prop_expected(lambda got: got == []))]
    x = rand_seq(rng, 120)
    edges.append(ListEdge("two genes", [substitute(rng, x, [5, 77]), x], 3, 100, _prop_expected(lambda got: got == [(0, 1, 2)])))
    for k in (63, 64, 65, 129):
        root = rand_seq(rng, 6)
        genes = [root] + [root if rng.random() < 0.2 else mutate(rng, root, rng.randrange(1, 4), keep_length=True) for _ in range(k)]
        edges.append(ListEdge("a pattern with %d candidates" % k, genes, 1, 3, _prop_first_pattern_candidates(k)))
    x = rand_seq(rng, 100)
    edges.append(ListEdge("length difference of exactly bound and bound + 1", [x, x[:50] + b"ACG" + x[50:], x[:50] + b"ACGT" + x[50:]], 3, 100,
                          _prop_length_gap))
    edges.append(ListEdge("ed == bound and ed == bound + 1", [x, substitute(rng, x, [3, 50, 99]), substitute(rng, x, [0, 20, 64, 98])], 3, 100,
                          _prop_ed_at_bound))
    with_n = x[:9] + b"N" + x[10:]
    edges.append(ListEdge("dereplication: exact copies, and copies that hold an N", [x, x.lower(), with_n, bytes(with_n), bytes(x), x[:-1]], 0, 1,
                          _prop_dereplication))
    x = rand_seq(rng, MAX_LEN)
    edges.append(ListEdge("max_len * diff_num needs 64 bits", [x, substitute(rng, x, rng.sample(range(MAX_LEN), 61)), rand_seq(rng, MAX_LEN)],
                          30_000_000, 1_000_000_000, _prop_needs_64_bits))
    names, seqs = families(8162, 5, 4, 300, 8)
    order = list(range(len(seqs)))
    rng.shuffle(order)
    edges.append(ListEdge("families of mixed lengths, shuffled", [seqs[k] for k in order], 3, 100, _prop_expected(lambda got: len(got) >= 5)))
    assert len({e.name for e in edges}) == len(edges)
    return edges
