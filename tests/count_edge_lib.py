"""Named edge cases of the counts mode of the gene profile (rambl_amd/csrc/sc_profile_counts.hpp: k_cnt_pick, group_at under
k_cnt_advance and k_cnt_count, k_cnt_resolve's walk over the round's new list parts, the rank table).

A case is a count_lib.CountCase: genes, segments, segment ids, thresholds and a check.  The check proves on the CPU, with the
plain restatement's hits (tests/native/blast_hits_check.cpp through count_lib.reference) and count_lib.lazy_rule alone, that the
input reaches the seam it is named for: a builder that loses its seam fails in tests/test_count_edges_host.py before the device
comparison of tests/test_count_edges_gpu.py could pass for nothing.  A check reads the seam from the case's name, not from the
builder's arguments, so a builder called with other numbers fails it.

The hits of a read lie on the device sorted by (rank of E6, segment, gene); E6 depends on the segment's length and the score
only, so the genes that hold the same piece of a segment are one group, in gene order.  The families:
- strand_tie_dirty / strand_tie_clean: one segment whose strands score the same, 94 of 100 columns against a clean 82; forward
  is the dirty one, and in the second case (the segment's reverse complement) the clean one.  k_cnt_pick's `<=` and `<`.
- seam_64_64, seam_63_65, seam_128_129, seam_end_64: a read whose first group (n1 genes, 94 %) fails -I and whose second (n2
  genes, clean) passes, so that group_at's trips of 64 records end on, one before and one behind a full trip, with another
  group or another read's records right behind.
- mates_64, mates_65, mates_129: a read of two mates that n genes hold both: the quadratic walk of k_cnt_count over a group of
  2 n + 2 records, a gene's two records n + 1 apart; a gene hit once in the group, and one whose other hit is in a later
  group; and a second read of two mates with one gene, whose first record fails -I at the E6 at which the second passes.
- five_segments: a read of five segments (ids a/1 a/2 a.1 a.2 a): three bits of `times`.
- all_buckets: a read with a failing first group and a passing second at every length at which the traceback bucket
  (L + 63) / 64 - 1 changes, with two plain reads of that length: every one of the eight lists gets records in round one and
  again in round two.
- rank_edges: the last column of the rank table (a clean 512-base segment, doubled score 1 024), the first ranked column of a
  length and the score below it, the shortest length that can pass and the length below it."""
import math
import random
from collections import Counter

import cohort_lib as HL
import count_lib as CL
import stage4_lib as L
from align_edge_lib import need

N_BUCKETS = 8                           # sc_profile_counts.hpp: MAX_ROWS / 64 traceback lists
BUCKET_LENGTHS = (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512)
_SWAP = {"A": "C", "C": "A", "G": "T", "T": "G"}


def bits_of(v):
    """sc_profile_counts.hpp's bits_of: the bits that hold 0..v."""
    return int(v).bit_length()


def bucket_of(length):
    return (length + 63) // 64 - 1


def evalue(length, gene_bases, score2, thresholds=CL.DEFAULTS):
    """E by the contract's expression (sc_profile_dp.hpp: evalue_of), in double."""
    return thresholds[3] * float(length) * float(gene_bases) * math.exp(-thresholds[2] * (0.5 * float(score2)))


def evalue6(length, gene_bases, score2, thresholds=CL.DEFAULTS):
    return float("%.6g" % evalue(length, gene_bases, score2, thresholds))


def min2(length, gene_bases, thresholds=CL.DEFAULTS):
    """sc_profile_dp.hpp's least_score2: the least doubled score of a segment of this length with E <= T; above 2 * length:
    the segment cannot pass."""
    s2 = 1
    while s2 <= 2 * length and not evalue(length, gene_bases, s2, thresholds) <= thresholds[1]:
        s2 += 1
    return s2


def unlike(rng, against, n):
    """n bases of which base i differs from against[i - 1], against[i] and against[i + 1]: laid beside a shared piece where
    `against` follows it on the other side, it extends the match neither straight on nor behind a gap of one base."""
    out = []
    for i in range(n):
        near = {against[j] for j in (i - 1, i, i + 1) if 0 <= j < len(against)}
        out.append(rng.choice([c for c in "ACGT" if c not in near]))
    return "".join(out)


def unlike_before(rng, against, n):
    """unlike() for the left side: n bases that end where the shared piece begins; `against` ends there on the other side."""
    return unlike(rng, against[::-1], n)[::-1]


def _rows_of(all_rows, seg):
    return [r for r in all_rows if r[0] == seg]


def _clean(r, n):
    return (int(r[2]), int(r[3])) == (n, n)


# ---- the strand tie

def strand_score2(seg, gene):
    """The best doubled local score of one strand of a segment against a gene (match 2, mismatch -4, a gap base -5), in plain
    Python: what the other strand of a pair scores, which the restatement's hits do not say."""
    prev, best = [0] * (len(gene) + 1), 0
    for a in seg:
        cur = [0] * (len(gene) + 1)
        for j, b in enumerate(gene, 1):
            cur[j] = max(0, prev[j - 1] + (2 if a == b and a in "ACGT" else -4), cur[j - 1] - 5, prev[j] - 5)
        best = max(best, max(cur))
        prev = cur
    return best


def strand_tie_case(name, mismatches=6, seed=61):
    clean = name.endswith("clean")
    for s in range(seed, seed + 20):                            # a seed whose two pieces do not extend each other by a base
        rng = random.Random(s)
        g = L.rand_seq(rng, 400)
        seg = CL.spread_mismatches(g[50:150], mismatches) + L.revcomp(g[250:332])
        if seg[100] != g[150] and L.revcomp(seg)[82] != g[332]:
            break
    segs = [L.revcomp(seg) if clean else seg, g[340:400]]
    want = (82, 82) if clean else (94, 100)

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        tie = [h for h in CL.loose_hits(case) if h[0] == 0]
        need(len(tie) == 1 and tie[0][2] == 0 and tie[0][3] == 164, "the restatement reports the forward strand at doubled score 164")
        need((tie[0][4], tie[0][5]) == want, "%d of %d columns on the forward strand" % want)
        other = strand_score2(L.revcomp(case.segs[0]), case.genes[0])
        need(other == 164, "the reverse strand scores 164 too (%d)" % other)
        need(bool(CL._hit(rows, "tie", "g00000")) == clean and failed["tie"] == (0 if clean else 1), "the tie read counts only when forward is clean")
        need(dict(full) == {"g00000": 2 if clean else 1} and looked == 2, "the plain read counts")
    return CL.CountCase(name, [g], segs, ["tie", "plain"], check)


# ---- group seams

def seam_sizes(name):
    """(n1, n2) a seam case is named for; seam_end_64: no failing group, 64 passing records."""
    return (0, 64) if name == "seam_end_64" else tuple(int(x) for x in name.split("_")[1:])


def seam_case(name, n1, n2, seed=63):
    """n1 genes hold X (100 bases), n2 others hold Y (60 bases); the read is X with six mismatches, two bases, Y; the genes'
    flanks next to X and Y are unlike what the read has there.  A plain read lies in the private flank of the first Y gene."""
    rng = random.Random(seed + 1000 * n1 + n2)
    x, y = L.rand_seq(rng, 100), L.rand_seq(rng, 60)
    read = (CL.spread_mismatches(x, 6) + L.rand_seq(rng, 2) if n1 else "") + y
    genes = [L.rand_seq(rng, rng.randint(50, 70)) + x + unlike(rng, read[100:], 30) for _ in range(n1)]
    genes += [L.rand_seq(rng, rng.randint(10, 30)) + unlike_before(rng, read[:-60], 30) + y + L.rand_seq(rng, rng.randint(80, 100)) for _ in range(n2)]
    segs = [read, genes[n1][-50:]]
    w1, w2 = seam_sizes(name)

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        groups = CL.groups_of(all_rows)["seam"]
        need([len(g) for g in groups] == ([w1, w2] if w1 else [w2]), "groups of %s records (%s)" % ((w1, w2), [len(g) for g in groups]))
        need(failed["seam"] == (1 if w1 else 0), "the first group fails -I, the second passes")
        if w1:
            need(all((int(r[2]), int(r[3])) == (94, 100) for r in groups[0]), "the first group: 94 of 100 columns")
        need(all(_clean(r, 60) for r in groups[-1]) and {r[1] for r in groups[-1]} == set(case.names[-w2:]), "the last group: the Y genes, clean")
        if name in ("seam_64_64", "seam_63_65", "seam_end_64"):
            need((w1 + w2) % 64 == 0 and len(_rows_of(all_rows, "plain")) == 1, "the next read's records start on a seam of 64")
        want = Counter({(g, 1, w2): 1 for g in case.names[-w2:]})
        want[(case.names[-w2], 1, 1)] += 1
        need(triples == want and looked == w1 + w2 + 1, "the read is shared by the %d Y genes, the plain read counts once" % w2)
    return CL.CountCase(name, genes, segs, ["seam", "plain"], check)


# ---- the quadratic walk

def mates_size(name):
    return int(name.split("_")[1])


def mates_case(name, n, seed=64):
    """Mates P and Q of 60 bases: n genes hold both, gene n holds P only, gene n + 1 holds P with four mismatches and a clean Q.
    Gene n + 2 is the variant's: read v is 100 bases of it with six mismatches (94 %: fails) and a clean 82 of it filled up to
    100 bases with bases unlike the gene's -- both at doubled score 164 and length 100, so at one E6."""
    rng = random.Random(seed + n)
    p, q = L.rand_seq(rng, 60), L.rand_seq(rng, 60)
    j = lambda a, b: L.rand_seq(rng, rng.randint(a, b))             # noqa: E731
    genes = [j(20, 40) + p + j(10, 30) + q + j(20, 40) for _ in range(n)]
    genes.append(j(60, 70) + p + L.rand_seq(rng, 70))
    genes.append(j(20, 40) + CL.spread_mismatches(p, 4) + j(10, 30) + q + j(20, 40))
    z = L.rand_seq(rng, 400)
    genes.append(z)
    segs = [p, q, CL.spread_mismatches(z[50:150], 6), z[250:332] + unlike(rng, z[332:], 18), z[160:240], genes[n][-50:]]
    ids = ["m/1", "m/2", "v/1", "v/2", "pz", "pn"]
    want = mates_size(name)

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        names = case.names
        groups = CL.groups_of(all_rows)
        kept = groups["m"][0]
        need(len(case.genes) == want + 3 and len(kept) == 2 * want + 2 and all(_clean(r, 60) for r in kept), "a kept group of 2 n + 2 clean records")
        need(want < 65 or len(kept) > 64, "the group is longer than a wavefront")
        need(want + 1 >= 64, "a gene's two records lie a trip of the walk apart")
        twice = {g for g, c in Counter(r[1] for r in kept).items() if c == 2}
        need(twice == set(names[:want]) and {r[1] for r in kept} - twice == {names[want], names[want + 1]}, "n genes hit twice, two hit once")
        later = CL._hit(all_rows, "m/1", names[want + 1])
        need(later and (int(later[2]), int(later[3])) == (56, 60) and later in groups["m"][1] and len(groups["m"]) == 2,
             "gene n + 1's hit on P lies in a later group")
        v1, v2 = CL._hit(all_rows, "v/1", names[-1]), CL._hit(all_rows, "v/2", names[-1])
        need(v1 and v2 and (int(v1[2]), int(v1[3])) == (94, 100) and _clean(v2, 82), "the variant: 94 of 100 and a clean 82")
        need(v1[8] == v2[8] and v1[9] == v2[9] == "100" and groups["v"][0] == [v1, v2] and failed["v"] == 0,
             "at one E6 in one group, the failing record first")
        want_triples = Counter({(g, 2, want): 1 for g in names[:want]})
        want_triples[(names[-1], 1, 1)] = 2
        want_triples[(names[want], 1, 1)] = 1
        need(triples == want_triples and looked == 2 * want + 2 + 2 + 2, "triples (gene, 2, n) for exactly n genes")
    return CL.CountCase(name, genes, segs, ids, check)


def five_segments_case(seed=65):
    rng = random.Random(seed)
    s = [L.rand_seq(rng, 60) for _ in range(5)]
    genes = ["".join(x + L.rand_seq(rng, 5) for x in s), "".join(x + L.rand_seq(rng, 5) for x in s[:4]), L.rand_seq(rng, 70) + s[4] + L.rand_seq(rng, 70)]
    ids = ["a/1", "a/2", "a.1", "a.2", "a"]

    def check(case, rows, all_rows, out):
        from rambl_amd import profile
        full, triples, looked, failed = out
        need(profile.read_index(case.ids) == ([0] * 5, 1), "one read of five segments")
        groups = CL.groups_of(all_rows)["a"]
        need(len(groups) == 1 and Counter(r[1] for r in groups[0]) == Counter({"g00000": 5, "g00001": 4, "g00002": 1}), "genes hit 5, 4 and 1 times")
        need(triples == Counter({("g00000", 5, 1): 1}), "the triple (gene 0, 5, 1)")
        need(bits_of(5) == 3 and bits_of(3) == 2, "times takes three bits where the other cases take two")
    return CL.CountCase("five_segments", genes, s, ids, check)


# ---- every traceback list in two rounds

def all_buckets_case(lengths=BUCKET_LENGTHS, seed=66):
    rng = random.Random(seed)
    g = [L.rand_seq(rng, 700), L.rand_seq(rng, 700)]
    bases = 1400
    segs, ids = [], []
    for k, n in enumerate(lengths):
        for b in range(max(27, n // 4), n):                     # the clean piece: the shortest that passes -e and scores below the dirty one
            a = n - 2 - b
            m = a // 20 + 1
            if evalue6(n, bases, 2 * b) <= 1e-10 and 2 * a - 6 * m > 2 * b:
                break
        p, q = 20 + k, 300 + k
        sep = "".join(next(c for c in "ACGT" if c not in avoid) for avoid in ((g[0][p + a], g[1][q - 2]), (g[0][p + a + 1], g[1][q - 1])))
        segs += [CL.spread_mismatches(g[0][p:p + a], m) + sep + g[1][q:q + b], g[0][k:k + n], g[1][700 - n - k:700 - k]]
        ids += ["adv%d" % n, "pa%d" % n, "pb%d" % n]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        groups = CL.groups_of(all_rows)
        rounds = [set(), set()]
        for read, gs in groups.items():
            need(len(gs) == (2 if read.startswith("adv") else 1) and all(len(x) == 1 for x in gs), "%s: one record per group" % read)
            need(failed[read] == (1 if read.startswith("adv") else 0), "%s: resolved in round %d" % (read, len(gs)))
            for r, x in enumerate(gs):
                rounds[r].add(bucket_of(int(x[0][9])))
        need(rounds[0] == rounds[1] == set(range(N_BUCKETS)), "every list has records in round one and again in round two")
        lens = sorted({len(s) for s in case.segs})
        need(all(n in lens for n in BUCKET_LENGTHS) and len(groups) == 3 * len(lens), "both sides of every change of (L + 63) / 64 - 1; every read hits")
        need(looked == 4 * len(lens) and dict(full) == {"g00000": len(lens), "g00001": 2 * len(lens)}, "the second group gives the read to gene 1")
    return CL.CountCase("all_buckets", g, segs, ids, check)


# ---- edges of the rank table

def rank_edges_case(seed=67, least_shift=0):
    rng = random.Random(seed)
    g = [L.rand_seq(rng, 600), L.rand_seq(rng, 600)]
    bases = 1200
    shortest = next(n for n in range(1, 513) if min2(n, bases) <= 2 * n)
    # a length whose least passing score is even (a clean run reaches it) and still passes as E6
    n = next(n for n in range(90, 140) if min2(n, bases) % 2 == 0 and evalue6(n, bases, min2(n, bases)) <= 1e-10)
    c = min2(n, bases) // 2 + least_shift
    junk = unlike(rng, g[1][100 + c:], n - c)
    segs = [g[0][40:552], g[1][100:100 + c] + junk, g[1][100:100 + c - 1] + _SWAP[g[1][100 + c - 1]] + junk,
            g[0][560:560 + shortest - 1], g[1][300:300 + shortest]]
    ids = ["full512", "least", "twin", "short", "shortest"]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        top = CL._hit(rows, "full512", "g00000")
        need(top and _clean(top, 512) and float(top[8]) == evalue6(512, bases, 1024), "a clean 512-base segment: doubled score 1 024")
        m2 = min2(n, bases)
        least = CL._hit(rows, "least", "g00001")
        need(least and _clean(least, m2 // 2) and m2 % 2 == 0 and float(least[8]) == evalue6(n, bases, m2) <= 1e-10 and len(case.segs[1]) == n,
             "a clean run of min2 / 2 bases in a segment of %d: the first ranked column of its length" % n)
        need(not evalue(n, bases, m2 - 1) <= 1e-10 and len(case.segs[2]) == n and not _rows_of(all_rows, "twin"), "one base less does not pass -e")
        need(not HL.can_pass(shortest - 1, bases) and len(case.segs[3]) == shortest - 1 and not _rows_of(all_rows, "short"),
             "a segment of %d bases cannot pass: no row even at -I 0" % (shortest - 1))
        last = CL._hit(rows, "shortest", "g00001")
        need(HL.can_pass(shortest, bases) and last and _clean(last, shortest) and float(last[8]) <= 1e-10, "%d bases matched throughout pass" % shortest)
        need(HL.plan_stretches([[len(s)] for s in case.segs], 2, bases, 1) == [(0, 1), (1, 2), (2, 3), (3, 5)], "the too-short read costs no tile")
        need(dict(full) == {"g00000": 1, "g00001": 2} and looked == 3, "three reads count")
    return CL.CountCase("rank_edges", g, segs, ids, check)


EDGES = {"strand_tie_dirty": lambda: strand_tie_case("strand_tie_dirty"), "strand_tie_clean": lambda: strand_tie_case("strand_tie_clean"),
         "seam_64_64": lambda: seam_case("seam_64_64", 64, 64), "seam_63_65": lambda: seam_case("seam_63_65", 63, 65),
         "seam_128_129": lambda: seam_case("seam_128_129", 128, 129), "seam_end_64": lambda: seam_case("seam_end_64", 0, 64),
         "mates_64": lambda: mates_case("mates_64", 64), "mates_65": lambda: mates_case("mates_65", 65),
         "mates_129": lambda: mates_case("mates_129", 129), "five_segments": five_segments_case, "all_buckets": all_buckets_case,
         "rank_edges": rank_edges_case}
_BUILT = {}


def case(name):
    """A named case, built once."""
    if name not in _BUILT:
        _BUILT[name] = EDGES[name]()
    return _BUILT[name]
