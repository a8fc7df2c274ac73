"""Named edge cases of the seeded gene profile (rambl_amd/csrc/sc_profile_seed.hpp: k_seed_keys, k_seed_lookup and the pair-list
score pass).  The promise under test: with the k-mer filter in front, the hits are the unseeded ones.

A case is genes, segments, thresholds, the seed length K the call must run at, and a check.  The check proves on the CPU, with
tests/seed_lib.py and the plain restatement tests/native/blast_hits_check.cpp alone, that the input reaches the edge it is
named for: a generator that loses its edge fails in tests/test_seed_edges_host.py before the device comparison of
tests/test_seed_edges_gpu.py could pass for nothing.

The families, and what of the kernels each one reaches:
- ordinary_k11..16: six (-I, -e) settings on a subset of the parity data set, one per seed length: mismatching hits, indels,
  Ns, both strands.  K = 16 fills the 32-bit code, takes `mask`'s own branch and shifts the reverse-complement code by 30.
- exact_k11..16, poly_t_k11..16, clamp: -I 100 with -e at the E-value of k matched bases of a k-base segment, so K = k: a
  segment of K and of K - 1 bases, a gene's first and last window, the segment's last window, a reverse-only hit, a k-mer
  across two adjacent genes, an N on either side, the all-A (code 0) and all-T (all ones: at K = 16 the key next to NO_KEY)
  k-mer on either strand; the k = 17 thresholds, which are cut to K = 16, with shared runs of 17, 16 and 15 bases.
- tight_k11..16: hits whose longest common run with the gene is exactly k*, on both strands, and the neighbour one column
  shorter that must not pass.
- seam_k13/k16_per2/3/8/nw: one shared k-mer at one window of a long random segment, placed on every edge of a lane's stretch
  of windows (a lane owns per = ceil(nw / 64) windows and reads k - 1 bases past its last), on either strand, with nw = 1, 63,
  64 and 65, and an N right in front of the shared k-mer at a lane's start.
- genes_65535/65536/65537/65569: more genes than one pass of the lookup's bitset holds (65 536), with posting runs that end
  at, start at and cross the range boundary; 1.3 Mbases also take k_seed_keys through its second trip.
- keys_second_trip: 129 genes of 8 192 bases, the last gene wholly on k_seed_keys' second trip."""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import count_lib as CL
import profile_lib as PL
import seed_lib as S
import stage4_lib as L
from align_edge_lib import need
from test_profile_seed_gpu import _exact_thresholds, _only_shared

SEED_WORDS, KEY_BLOCKS = 2048, 4096     # sc_profile_seed.hpp
GENE_RANGE = SEED_WORDS * 32            # genes per pass of k_seed_lookup over a segment
KEYS_TRIP = KEY_BLOCKS * 256            # gene bases per trip of k_seed_keys
KA = (1.28, 0.46)
# K on genes[:6], segs[:150] of the parity data set (3 270 gene bases, segments of 60 to 512 bases), computed with seed_lib
ORDINARY = {11: (94.0, 1e-10), 12: (96.0, 1e-5), 13: (95.0, 1e-10), 14: (96.5, 1e-5), 15: (95.0, 1e-20), 16: (97.0, 1e-10)}
_SWAP = {"A": "C", "C": "A", "G": "T", "T": "G"}


def call_k(genes, segs, thresholds):
    """The seed length of the call by seed_lib: the least k* over the lengths that can pass -e at all."""
    n = sum(len(g) for g in genes)
    lens = {len(s) for s in segs if S.least_score2(len(s), n, *thresholds[1:]) is not None}
    return S.seed_length(lens, n, *thresholds)


def lookup_per(n, k):
    """(nw, per, lanes in use) of k_seed_lookup for a segment of n bases."""
    nw = n - k + 1
    per = (nw + 63) // 64
    return nw, per, -(-nw // per)


def parallel_hits(exe, genes, segs, thresholds, jobs=8):
    """profile_lib.run_hits_check, a segment per run and `jobs` runs at a time (a segment's hits depend on the genes only)."""
    with ThreadPoolExecutor(jobs) as pool:
        parts = list(pool.map(lambda s: PL.run_hits_check(exe, genes, [s], *thresholds), segs))
    return [(k,) + h[1:] for k, part in enumerate(parts) for h in part]


class SeedCase:
    """genes, segs (text), thresholds, k (the seed length the call must report), names (one per segment, may be None),
    prove(case, exe): the property that the input reaches its edge, and after(case, hits, pairs): what the device's hits and
    seed_lib's pairs must show on top of the comparison itself."""

    def __init__(self, name, genes, segs, thresholds, k, prove, after=None, names=None, split=False):
        self.name, self.genes, self.segs, self.thresholds, self.k = name, genes, segs, tuple(thresholds), k
        self.prove, self.after, self.names, self.split = prove, after, names, split
        self._hits = {}

    def key(self):
        return (self.genes, self.segs, self.thresholds, self.k)

    def hits(self, exe, min_identity=None):
        """The restatement's hits, computed once (at another -I when given)."""
        th = self.thresholds if min_identity is None else (min_identity,) + self.thresholds[1:]
        if th not in self._hits:
            if self.split:
                self._hits[th] = parallel_hits(exe, self.genes, self.segs, th)
            else:
                self._hits[th] = CL.hits_in_parts(exe, self.genes, self.segs, th)
        return self._hits[th]

    def pairs(self):
        if not hasattr(self, "_pairs"):
            self._pairs = S.sharing_pairs(self.genes, self.segs, self.k)
        return self._pairs

    def at(self, name):
        return self.names.index(name)

    def genes_of(self, name):
        return {g for s, g in self.pairs() if s == self.at(name)}

    def check(self, exe):
        need(call_k(self.genes, self.segs, self.thresholds) == self.k, "K = %d" % self.k)
        self.prove(self, exe)


# ---- 1. every seed length, ordinary thresholds

_PARITY = []


def parity_subset():
    if not _PARITY:
        genes, segs = PL.parity_dataset()
        _PARITY.append((genes[:6], segs[:150]))
    return _PARITY[0]


def ordinary_case(k):
    genes, segs = parity_subset()

    def prove(case, exe):
        hits = case.hits(exe)
        need(len(hits) >= 20, "20 hits or more (%d)" % len(hits))
        need(sum(1 for h in hits if h[4] != h[5]) >= 10, "10 inexact hits or more")
        need(min(sum(1 for h in hits if h[2] == s) for s in (0, 1)) >= 5, "5 hits or more on each strand")
        need(any(h[5] > h[7] - h[6] + 1 or h[5] > abs(h[9] - h[8]) + 1 for h in hits), "a hit with a gap")
    return SeedCase("ordinary_k%d" % k, genes, segs, ORDINARY[k] + KA, k, prove)


def count_case(k):
    """The ordinary setting of K = k as a count_lib.CountCase: reads of one, two and three segments."""
    genes, segs = parity_subset()
    ids = [("p%d/1" % (s // 5), "p%d/2" % (s // 5), "p%d.1" % (s // 5), "s%d" % s, "t%d.2" % s)[s % 5] for s in range(len(segs))]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(len(rows) >= 20 and len(full) >= 3, "hits on several genes")
        need(len(set(map(CL.read_of, case.ids))) < len(case.ids), "reads of several segments")
    return CL.CountCase("seed_edges_k%d" % k, genes, segs, ids, check, ORDINARY[k] + KA)


# ---- 1. every seed length, the exact recipe: -I 100 and -e at the E-value of k matched bases of a k-base segment

def _no_a_before(gene, p):
    """The gene with a C in front of position p where it had an A.  A reverse-complement code that lost its last base reads as
    A + the first k - 1 bases: it would still find a reverse-only k-mer that an A precedes in the gene."""
    return gene[:p - 1] + ("C" if gene[p - 1] == "A" else gene[p - 1]) + gene[p:]


def _poly_gene(rng, base, k, before, after):
    return L.rand_seq(rng, 25) + before + base * k + after + L.rand_seq(rng, 25)


def _expect(case, exe, pairs_of, hit_names, maybe=()):
    """Every named segment pairs with exactly these genes and exactly these segments hit (`maybe`: k shared bases inside a
    longer segment, where a flank that matches one base further can make a hit)."""
    for name, genes in pairs_of.items():
        need(case.genes_of(name) == set(genes), "%s pairs with %s (%s)" % (name, sorted(genes), sorted(case.genes_of(name))))
    need(set(pairs_of) == set(case.names), "every segment is named")
    need({case.names[h[0]] for h in case.hits(exe)} - set(maybe) == set(hit_names), "the hits are %s" % sorted(hit_names))


def exact_case(k):
    """The named seed edges of test_profile_seed_gpu.test_seed_edges at seed length k, and the all-A k-mer (code 0)."""
    rng = random.Random(4242 + k)
    genes = [L.rand_seq(rng, 80) for _ in range(4)]
    whole3 = genes[3]
    genes[3] = whole3[:40] + "N" + whole3[41:]                       # an N in the gene breaks the windows over column 40
    genes.append(_poly_gene(rng, "A", k, "C", "G"))
    genes[2] = _no_a_before(_no_a_before(genes[2], 10), 50)          # (before the two reverse-only k-mers)
    j = lambda n: L.rand_seq(rng, n)                                 # noqa: E731
    h = k // 2
    segs = {
        "exactly_k": genes[0][20:20 + k],
        "k_minus_1": genes[0][20:19 + k],
        "gene_first_window": genes[1][:k],
        "gene_last_window": genes[1][-k:],
        "gene_first_window_long": j(20) + genes[1][:k] + j(20),
        "gene_last_window_long": j(20) + genes[1][-k:] + j(20),
        "segment_last_window": j(29) + _SWAP[genes[2][29]] + genes[2][30:30 + k],
        "reverse_only": S.revcomp(genes[2][10:10 + k]),
        "reverse_only_long": S.revcomp(j(15) + genes[2][50:50 + k] + j(15)),
        "across_genes": genes[0][-h:] + genes[1][:k - h],
        "across_genes_long": j(20) + genes[1][-(k - h):] + genes[2][:h] + j(20),
        "n_in_gene": whole3[40 - h:40 - h + k],
        "n_in_segment": genes[0][40:40 + h] + "N" + genes[0][41 + h:40 + k],
        "n_in_segment_long": j(10) + genes[0][40:40 + h] + "N" + genes[0][41 + h:40 + k] + j(10),
        "poly_a": "A" * k,
        "poly_a_long": j(10) + "G" + "A" * k + "C" + j(10),
        "poly_a_reverse": "T" * k,
        "poly_a_reverse_long": S.revcomp(j(10) + "G" + "A" * k + "C" + j(10)),
    }

    def prove(case, exe):
        n = sum(len(g) for g in case.genes)
        need(S.least_score2(k - 1, n, *case.thresholds[1:]) is None, "a segment of K - 1 bases cannot pass")
        _expect(case, exe, {
            "exactly_k": [0], "k_minus_1": [], "gene_first_window": [1], "gene_last_window": [1], "gene_first_window_long": [1],
            "gene_last_window_long": [1], "segment_last_window": [2], "reverse_only": [2], "reverse_only_long": [2], "across_genes": [],
            "across_genes_long": [], "n_in_gene": [], "n_in_segment": [], "n_in_segment_long": [], "poly_a": [4], "poly_a_long": [4],
            "poly_a_reverse": [4], "poly_a_reverse_long": [4]},
            ("exactly_k", "gene_first_window", "gene_last_window", "reverse_only", "poly_a", "poly_a_reverse"),
            maybe=[n for n in segs if n.endswith("_long")])
        by = {case.names[x[0]]: x for x in case.hits(exe)}
        need(by["gene_first_window"][8:10] == (1, k) and by["gene_last_window"][8:10] == (81 - k, 80), "a gene's first and last window")
        need(by["reverse_only"][2] == 1 and by["poly_a_reverse"][2] == 1 and by["poly_a"][2] == 0, "the strands")
        need(_only_shared(segs["segment_last_window"], genes[2], k) == ({segs["segment_last_window"][-k:]}, set()), "the segment's last window only")
        need(_only_shared(segs["reverse_only"], genes[2], k) == (set(), {genes[2][10:10 + k]}), "the reverse strand only")
        need("A" not in (genes[2][9], genes[2][49]), "no A in front of the reverse-only k-mers")
        need(segs["across_genes"] in "".join(genes) and genes[1][-(k - h):] + genes[2][:h] in "".join(genes), "the k-mer exists across two genes")
        need(segs["n_in_gene"] in whole3 and "N" in segs["n_in_segment"], "an N in the gene and one in the segment")
        need(_only_shared(segs["poly_a_long"], genes[4], k) == ({"A" * k}, set()), "the all-A k-mer alone, forward")
        need(_only_shared(segs["poly_a_reverse_long"], genes[4], k) == (set(), {"A" * k}), "the all-A k-mer alone, reverse")
    return SeedCase("exact_k%d" % k, genes, list(segs.values()), _exact_thresholds(genes, k), k, prove, names=list(segs))


def poly_t_case(k):
    """The all-T k-mer, whose code is all ones, in one gene only; the segments hold it forward and as all-A on the reverse."""
    rng = random.Random(5151 + k)
    genes = [L.rand_seq(rng, 80) for _ in range(3)] + [_poly_gene(rng, "T", k, "C", "G")]
    j = lambda n: L.rand_seq(rng, n)                                 # noqa: E731
    segs = {
        "exactly_k": genes[0][20:20 + k],
        "poly_t": "T" * k,
        "poly_t_long": j(10) + "G" + "T" * k + "C" + j(10),
        "poly_t_last_window": j(30) + "G" + "T" * k,
        "poly_t_reverse": "A" * k,
        "poly_t_reverse_long": S.revcomp(j(10) + "G" + "T" * k + "C" + j(10)),
        "nearly": "T" * (k - 1) + "G",
    }

    def prove(case, exe):
        _expect(case, exe, {"exactly_k": [0], "poly_t": [3], "poly_t_long": [3], "poly_t_last_window": [3], "poly_t_reverse": [3],
                            "poly_t_reverse_long": [3], "nearly": [3]}, ("exactly_k", "poly_t", "poly_t_reverse", "nearly"),
                maybe=("poly_t_long", "poly_t_last_window", "poly_t_reverse_long"))
        need(("T" * k) in genes[3] and ("T" * (k + 1)) not in genes[3] and ("T" * (k - 1) + "G") in genes[3], "one run of exactly k Ts, then G")
        need(_only_shared(segs["poly_t_long"], genes[3], k) == ({"T" * k}, set()), "the all-T k-mer alone, forward")
        need(_only_shared(segs["poly_t_reverse_long"], genes[3], k) == (set(), {"T" * k}), "the all-T k-mer alone, reverse")
    return SeedCase("poly_t_k%d" % k, genes, list(segs.values()), _exact_thresholds(genes, k), k, prove, names=list(segs))


def clamp_case(seed=1717):
    """The k = 17 thresholds: the bound is 17, the call runs at K = 16."""
    rng = random.Random(seed)
    genes = [_no_a_before(L.rand_seq(rng, 80), 40) for _ in range(3)]
    j = lambda n: L.rand_seq(rng, n)                                 # noqa: E731
    cut = lambda g, a, n: g[a:a + n] + _SWAP[g[a + n]]               # noqa: E731  (n gene bases and a base that ends the run)
    segs = {
        "run_17": genes[0][10:27],
        "run_16": cut(genes[1], 10, 16),
        "run_15": cut(genes[2], 10, 15) + "A",
        "run_17_reverse": S.revcomp(genes[0][40:57]),
        "run_16_reverse": S.revcomp(cut(genes[1], 40, 16)),
        "run_15_reverse": S.revcomp(cut(genes[2], 40, 15) + "C"),
        "run_16_long": j(20) + _SWAP[genes[2][29]] + cut(genes[2], 30, 16) + j(20),
    }
    runs = {"run_17": (0, 17), "run_16": (1, 16), "run_15": (2, 15), "run_17_reverse": (0, 17), "run_16_reverse": (1, 16),
            "run_15_reverse": (2, 15), "run_16_long": (2, 16)}

    def prove(case, exe):
        n = sum(len(g) for g in case.genes)
        need(min(S.lossless_k(len(s), n, *case.thresholds) for s in case.segs) == 17, "the lossless bound is 17")
        for name, (g, run) in runs.items():
            s = segs[name]
            need(max(S.longest_common_run(s, genes[g]), S.longest_common_run(S.revcomp(s), genes[g])) == run, "%s: a run of %d" % (name, run))
        _expect(case, exe, {name: ([g] if run >= 16 else []) for name, (g, run) in runs.items()}, ("run_17", "run_17_reverse"))
    return SeedCase("clamp", genes, list(segs.values()), _exact_thresholds(genes, 17), 16, prove, names=list(segs))


# ---- 2. hits that reach the bound

def tight_shape(k, gene_bases):
    """(L, i, m) of the ordinary setting of K = k: a segment of L = i + m bases whose i identity columns and m mismatches are
    a hit at k*(L) = k = ceil(i / (m + 1)), and whose neighbour without the last column passes -e at its own length (with
    k*(L - 1) = k too, so the call has K = k) but fails -I."""
    I, e = ORDINARY[k]
    for n in range(20, 400):
        if S.lossless_k(n, gene_bases, I, e) != k or S.lossless_k(n - 1, gene_bases, I, e) != k:
            continue
        s2, s2n = S.least_score2(n, gene_bases, e), S.least_score2(n - 1, gene_bases, e)
        for m in range(1, n // 2):
            i = n - m
            if -(-i // (m + 1)) == k and 100.0 * i / (i + m) >= I and not 100.0 * (i - 1) / (i - 1 + m) >= I \
                    and 2 * i - 4 * m >= s2 and 2 * (i - 1) - 4 * m >= s2n:
                return n, i, m
    return None


def _broken(gene, a, i, m):
    """i + m bases of the gene from a with m substitutions between m + 1 runs of identity columns, the longest first and of
    ceil(i / (m + 1)) columns."""
    q, rem = divmod(i, m + 1)
    x = list(gene[a:a + i + m])
    p = 0
    for r in range(m):
        p += q + (1 if r < rem else 0)
        x[p] = _SWAP[x[p]]
        p += 1
    return "".join(x)


def tight_case(k, seed=77):
    rng = random.Random(seed + k)
    gene = _no_a_before(L.rand_seq(rng, 400), 200 if k == 16 else 250)
    if k == 16:                                                      # the 97 % setting's bound is 17: the exact recipe, a run of exactly 16
        th = _exact_thresholds([gene], 16)
        n, i, m = 16, 16, 0
        segs = [gene[100:116], gene[100:115], S.revcomp(gene[200:216]),
                L.rand_seq(rng, 20) + _SWAP[gene[299]] + gene[300:316] + _SWAP[gene[316]] + L.rand_seq(rng, 20)]
    else:
        th = ORDINARY[k] + KA
        n, i, m = tight_shape(k, len(gene))
        segs = [_broken(gene, 100, i, m), _broken(gene, 100, i, m)[:-1], S.revcomp(_broken(gene, 250, i, m))]

    def prove(case, exe):
        need([S.lossless_k(len(s), 400, *th) for s in segs[:3]] == ([16, None, 16] if k == 16 else [k, k, k]), "k* = %d at every length" % k)
        hits = case.hits(exe)
        by = {h[0]: h for h in hits}
        need(set(by) == {0, 2} and by[0][2] == 0 and by[2][2] == 1, "the tight segment and its reverse twin hit, the neighbour does not")
        need(all((by[s][4], by[s][5]) == (i, n) for s in (0, 2)), "%d identity columns of %d" % (i, n))
        need([S.longest_common_run(*S.hit_slices(h, case.genes, case.segs)) for h in hits] == [k, k], "the longest common run is k*")
        loose = {h[0] for h in case.hits(exe, 0.0)}
        if k == 16:
            need(loose == {0, 2} and S.longest_common_run(segs[3], gene) == 16 and case.pairs() == {(0, 0), (2, 0), (3, 0)},
                 "15 bases cannot pass -e; a long segment with a run of exactly 16 pairs")
        else:
            need(loose == {0, 1, 2}, "it is -I that drops the neighbour")

    def after(case, hits, pairs):
        assert {(0, 0), (2, 0)} <= pairs and [h[:2] for h in hits] == [(0, 0), (2, 0)]
    return SeedCase("tight_k%d" % k, [gene], segs, th, k, prove, after)


# ---- 3. lane seams of the lookup

def _planted(rng, genes, g, kmer, n, w, k, reverse=False, n_at=None):
    """A random segment of n bases that holds the gene's k-mer (its reverse complement when `reverse`) at window w, an N at
    base n_at when given, and shares no other k-mer with any gene on either strand."""
    want = (set(), {kmer}) if reverse else ({kmer}, set())
    for _ in range(1000):
        x = L.rand_seq(rng, n)
        x = x[:w] + (S.revcomp(kmer) if reverse else kmer) + x[w + k:]
        if n_at is not None:
            x = x[:n_at] + "N" + x[n_at + 1:]
        if all(_only_shared(x, gene, k) == (want if t == g else (set(), set())) for t, gene in enumerate(genes)):
            return x
    raise AssertionError("no segment with the k-mer at window %d alone" % w)


def seam_windows(n, k):
    """The windows on the edges of a middle lane's and of the last used lane's stretch, the segment's last window and
    window 0; and, for the middle lane, the bases wa - 1, wa and wa + k - 1 that get an N with the k-mer right behind."""
    nw, per, lanes = lookup_per(n, k)
    ws = {0, nw - 1}
    for lane in (lanes // 2, lanes - 1):
        wa, wb = lane * per, min(lane * per + per, nw)
        ws |= {wa - 1, wa, wb - 1, wb}
    wa = (lanes // 2) * per
    return sorted(w for w in ws if 0 <= w < nw), [b for b in (wa - 1, wa, wa + k - 1) if b >= 0 and b + 1 + k <= n]


def seam_case(k, what):
    """what: 2, 3 or 8 windows per lane (65, 129 and 513 - k windows), or "nw": 1, 63, 64 and 65 windows."""
    rng = random.Random(1000 * k + (what if what != "nw" else 0))
    genes = [L.rand_seq(rng, 120) for _ in range(3)]
    genes[1] = _no_a_before(genes[1], 50)
    kmer = genes[1][50:50 + k]
    lengths = [nw + k - 1 for nw in (1, 63, 64, 65)] if what == "nw" else [512 if what == 8 else 64 * (what - 1) + k]
    segs, where = [genes[0][5:5 + k]], [None]                       # (a k-base segment: with it the exact recipe gives K = k)
    for n in lengths:
        ws, ns = seam_windows(n, k)
        for reverse in (False, True):
            for w in ws:
                segs.append(_planted(rng, genes, 1, kmer, n, w, k, reverse))
                where.append((n, w, reverse, None))
            for b in ns:
                segs.append(_planted(rng, genes, 1, kmer, n, b + 1, k, reverse, n_at=b))
                where.append((n, b + 1, reverse, b))

    def prove(case, exe):
        pers = {lookup_per(n, k)[1] for n in lengths}
        need(pers == ({1, 2} if what == "nw" else {what}), "windows per lane: %s" % sorted(pers))
        need({lookup_per(n, k)[0] for n in lengths} == ({1, 63, 64, 65} if what == "nw" else {513 - k if what == 8 else 64 * (what - 1) + 1}), "nw")
        for s, at in enumerate(where):
            if at is None:
                continue
            n, w, reverse, n_at = at
            seg = case.segs[s]
            need(len(seg) == n and seg[w:w + k] == (S.revcomp(kmer) if reverse else kmer), "the k-mer is at window %d" % w)
            need(n_at is None or (seg[n_at] == "N" and n_at == w - 1), "the N is right in front of the k-mer")
            for g, gene in enumerate(case.genes):
                shared = _only_shared(seg, gene, k)
                need(shared == ((set(), set()) if g != 1 else (set(), {kmer}) if reverse else ({kmer}, set())), "segment %d shares one k-mer" % s)
        if what != "nw":
            nw, per, lanes = lookup_per(lengths[0], k)
            mid, last = (lanes // 2) * per, (lanes - 1) * per
            got = {at[1] for at in where if at and not at[2] and at[3] is None}
            need({0, mid - 1, mid, mid + per - 1, mid + per, last - 1, last, nw - 1} <= got, "every edge of a middle and of the last lane")
            need({at[3] for at in where if at and at[3] is not None} == {mid - 1, mid, mid + k - 1}, "an N before, at and k - 1 behind a lane's start")
        need(case.genes[1][49] != "A" and case.genes[1][50:50 + k] == kmer, "no A in front of the k-mer in its gene")
        need(case.pairs() == {(0, 0)} | {(s, 1) for s in range(1, len(case.segs))}, "every segment pairs with gene 1 alone")
        need([h[:2] for h in case.hits(exe)] == [(0, 0)] + [(s, 1) for s, at in enumerate(where) if at and at[0] == k],
             "k shared bases are no hit of a longer segment")
    return SeedCase("seam_k%d_%s" % (k, "nw" if what == "nw" else "per%d" % what), genes, segs, _exact_thresholds(genes, k), k, prove)


# ---- 4. gene ranges, and the second trip of k_seed_keys

def _random_genes(seed, n_genes, length):
    flat = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(seed).randint(0, 4, size=n_genes * length)].tobytes().decode()
    return [flat[g * length:(g + 1) * length] for g in range(n_genes)]


def range_case(n_genes):
    """Genes of 20 bases, the exact recipe at K = 16.  Genes 65 534 to 65 537 (to the last gene where there are fewer) begin with
    the same 20 bases: a posting run over the boundary of the lookup's gene ranges."""
    rng = random.Random(n_genes)
    genes = _random_genes(n_genes, n_genes, 20)
    last = n_genes - 1
    a, b = min(GENE_RANGE - 1, last), min(GENE_RANGE, last)
    common = L.rand_seq(rng, 20)
    run = list(range(GENE_RANGE - 2, min(GENE_RANGE + 1, last) + 1))
    for g in run:
        genes[g] = common + genes[g]
    j = lambda n: L.rand_seq(rng, n)                                 # noqa: E731
    segs = {
        "last_gene": j(8) + genes[last][-20:] + j(8),
        "last_of_first_range": j(8) + genes[a][-20:] + j(8),
        "first_of_second_range": j(8) + genes[b][-20:] + j(8),
        "across_ranges": j(8) + common + j(8),
        "nothing": j(36),
        "reverse_only": S.revcomp(j(8) + genes[b][-20:] + j(8)),
    }
    want = {"last_gene": [last], "last_of_first_range": [a], "first_of_second_range": [b], "across_ranges": run, "nothing": [], "reverse_only": [b]}

    def prove(case, exe):
        need(sum(len(g) for g in case.genes) > KEYS_TRIP, "more gene bases than one trip of k_seed_keys")
        need(run[0] == GENE_RANGE - 2 and run[-1] == min(GENE_RANGE + 1, last) and len(run) == min(4, n_genes - GENE_RANGE + 2), "the posting run")
        _expect(case, exe, want, [n for n in want if n != "nothing"])
        hits = {(case.names[h[0]], h[1], h[2]) for h in case.hits(exe)}
        need(hits == {(n, g, int(n == "reverse_only")) for n, gs in want.items() for g in gs}, "every pair is a hit, one of them reverse")

    def after(case, hits, pairs):
        assert {(h[0], h[1]) for h in hits} == pairs == {(case.at(n), g) for n, gs in want.items() for g in gs}
    return SeedCase("genes_%d" % n_genes, genes, list(segs.values()), _exact_thresholds(genes, 16), 16, prove, after, names=list(segs), split=True)


def keys_trip_case(seed=129):
    """129 genes of 8 192 bases at the defaults: the last gene begins where the first trip of k_seed_keys ends."""
    rng = random.Random(seed)
    genes = _random_genes(seed, 129, 8192)
    first, last = genes[0], genes[-1]
    mid = lambda s: s[:25] + _SWAP[s[25]] + s[26:]                   # noqa: E731
    segs = {"end_of_last": last[-50:], "start_of_first": first[:50], "end_of_last_reverse": S.revcomp(mid(last[-50:])),
            "start_of_first_inexact": mid(first[:50]), "start_of_last": last[:50], "end_of_gene_127": genes[127][-50:],
            "nothing": L.rand_seq(rng, 50)}
    want = {"end_of_last": 128, "start_of_first": 0, "end_of_last_reverse": 128, "start_of_first_inexact": 0, "start_of_last": 128,
            "end_of_gene_127": 127}

    def prove(case, exe):
        need(128 * 8192 == KEYS_TRIP and sum(len(g) for g in case.genes) == KEYS_TRIP + 8192, "the last gene is the second trip")
        hits = {(case.names[h[0]], h[1]) for h in case.hits(exe)}
        need(hits == set(want.items()), "the hits")
        need(all(want[n] in case.genes_of(n) for n in want), "and their pairs")

    def after(case, hits, pairs):
        assert {(case.names[h[0]], h[1]) for h in hits} == set(want.items())
    return SeedCase("keys_second_trip", genes, list(segs.values()), CL.DEFAULTS, 13, prove, after, names=list(segs), split=True)


KS = range(11, 17)
CASES = {}
for _k in KS:
    CASES["ordinary_k%d" % _k] = (ordinary_case, _k)
    CASES["exact_k%d" % _k] = (exact_case, _k)
    CASES["poly_t_k%d" % _k] = (poly_t_case, _k)
    CASES["tight_k%d" % _k] = (tight_case, _k)
CASES["clamp"] = (clamp_case,)
for _k in (13, 16):
    for _what in (2, 3, 8, "nw"):
        CASES["seam_k%d_%s" % (_k, "nw" if _what == "nw" else "per%d" % _what)] = (seam_case, _k, _what)
for _n in (65535, 65536, 65537, 65569):
    CASES["genes_%d" % _n] = (range_case, _n)
CASES["keys_second_trip"] = (keys_trip_case,)
_BUILT = {}


def build(name):
    return CASES[name][0](*CASES[name][1:])


def case(name):
    """A named case, built once."""
    if name not in _BUILT:
        _BUILT[name] = build(name)
    return _BUILT[name]
