"""The counts mode of the gene profile (sc_profile_counts) restated on the hits of the plain restatement
(profile_lib.run_hits_check): the counting rule in two forms, and the named inputs of its edges.

full_rule is profile.raw_abundance on the rows of the hit path.  lazy_rule is what the device does: per read the pairs
grouped by E6 (the E-value as the hit CSV holds it), smallest first, stopping at the first group with a pair that passes
-I; it also says how many pairs it had to look at, which is what the mode saves."""
import math
import random
from collections import Counter
from fractions import Fraction

import profile_lib as PL
import stage4_lib as L
from align_edge_lib import need

COUNT_ROUNDS = 3                        # sc_profile_counts.hpp: rounds of one group per read before the rest is traced at once
REC_BLOCKS, READ_BLOCKS = 256, 8192     # sc_profile_counts.hpp: blocks of 256 threads, a record each / of one wavefront, a read each
DEFAULTS = (95.0, 1e-10, 1.28, 0.46)
SUFFIXES = ("/1", ".1", "/2", ".2")


def read_of(seg):
    return seg[:-2] if len(seg) >= 2 and seg[-2:] in SUFFIXES else seg


def full_rule(rows, min_identity=95.0, max_evalue=1e-10):
    """[(gene, Fraction)] in byte order of the gene: the hit path's own counting."""
    from rambl_amd import profile
    return profile.raw_abundance(rows, min_identity, max_evalue)


def lazy_rule(rows, min_identity=95.0, max_evalue=1e-10):
    """rows: every (segment, gene) pair with E <= T, whether it passes -I or not (ten columns as raw_abundance takes them).
    Returns ([(gene, Fraction)] as full_rule, Counter of (gene, times_hit, number_of_such_genes) triples, pairs looked at,
    {read: number of groups that failed before it was resolved or ran out})."""
    def passes(r):
        return not (float(r[2]) * 100 / float(r[3]) < min_identity)
    pairs = {}                                                  # (segment, gene): its first row that passes, else its first row
    for r in rows:
        if float(r[8]) > max_evalue:
            continue
        k = (r[0], r[1])
        if k not in pairs or (not passes(pairs[k]) and passes(r)):
            pairs[k] = r
    reads = {}
    for r in pairs.values():
        reads.setdefault(read_of(r[0]), {}).setdefault(float(r[8]), []).append(r)
    total, triples, looked, failed = {}, Counter(), 0, {}
    for read, groups in reads.items():
        failed[read] = 0
        for e6 in sorted(groups):
            looked += len(groups[e6])
            times = Counter(r[1] for r in groups[e6] if passes(r))
            if not times:
                failed[read] += 1
                continue
            most = max(times.values())
            share = [g for g, n in times.items() if n == most]
            for g in share:
                total[g] = total.get(g, 0) + Fraction(most, len(share))
                triples[(g, most, len(share))] += 1
            break
    return sorted(total.items(), key=lambda kv: kv[0].encode()), triples, looked, failed


def gene_names(n):
    return ["g%05d" % k for k in range(n)]


class CountCase:
    """genes, segs (text), ids (segment ids: they decide the reads), thresholds, and check(case, rows, all_rows, out): the
    property that the input still reaches its edge (rows: the hit path's; all_rows: at -I 0; out: lazy_rule's on all_rows,
    with full_rule's counts first)."""

    def __init__(self, name, genes, segs, ids, check, thresholds=DEFAULTS):
        self.name, self.genes, self.segs, self.ids, self.check, self.thresholds = name, genes, segs, ids, check, thresholds
        self.names = gene_names(len(genes))

    def n_bases(self):
        return sum(len(g) for g in self.genes)


_REFERENCE = {}
_LOOSE = {}


def hits_in_parts(exe, genes, segs, thresholds, jobs=8):
    """profile_lib.run_hits_check with the segments split over `jobs` runs at a time: a segment's hits depend on the genes
    only, so the parts' hits are the whole's."""
    from concurrent.futures import ThreadPoolExecutor
    step = max(16, -(-len(segs) // (4 * jobs)))
    starts = list(range(0, len(segs), step))
    with ThreadPoolExecutor(jobs) as pool:
        parts = list(pool.map(lambda a: PL.run_hits_check(exe, genes, segs[a:a + step], *thresholds), starts))
    return [(h[0] + a,) + h[1:] for a, part in zip(starts, parts) for h in part]


def reference(case, exe):
    """(rows of the hit path, rows at -I 0) of a case, computed once: the restatement's hits at -I 0, and those of them that
    pass -I by the contract's expression (the restatement applies the same one after the same strand pick)."""
    if case.name not in _REFERENCE:
        lens = [len(s) for s in case.segs]
        th = case.thresholds
        loose = hits_in_parts(exe, case.genes, case.segs, (0.0,) + tuple(th[1:]))
        hits = [h for h in loose if 100.0 * h[4] / h[5] >= th[0]]
        _LOOSE[case.name] = loose
        _REFERENCE[case.name] = (PL.rows_of(hits, case.ids, lens, case.names), PL.rows_of(loose, case.ids, lens, case.names))
    return _REFERENCE[case.name]


def loose_hits(case, exe=None):
    """The restatement's own hits of a case at -I 0 (profile_lib.run_hits_check's tuples: strand and doubled score, which the
    rows do not carry), kept by reference(); without exe: for a case's check, which runs after reference()."""
    if exe is not None:
        reference(case, exe)
    return _LOOSE[case.name]


def groups_of(all_rows, min_identity=95.0, max_evalue=1e-10):
    """{read: its rows at -I 0 with E6 <= T grouped by E6, smallest first}: the groups lazy_rule walks, in its order."""
    reads = {}
    for r in all_rows:
        if float(r[8]) <= max_evalue:
            reads.setdefault(read_of(r[0]), {}).setdefault(float(r[8]), []).append(r)
    return {read: [groups[e6] for e6 in sorted(groups)] for read, groups in reads.items()}


def check_rules(case, exe):
    """lazy_rule == full_rule on the case, then the case's own property.  Returns (counts, triples)."""
    rows, all_rows = reference(case, exe)
    I, T = case.thresholds[:2]
    full = full_rule(rows, I, T)
    lazy, triples, looked, failed = lazy_rule(all_rows, I, T)
    assert lazy == full, (case.name, lazy[:5], full[:5])
    if case.check:
        case.check(case, rows, all_rows, (full, triples, looked, failed))
    return full, triples


def device_counts(case, seeded=False, **kw):
    from rambl_amd import capi, profile
    seg_read, _ = profile.read_index(case.ids)
    return capi.profile_counts([g.encode() for g in case.genes], [s.encode() for s in case.segs], seg_read, *case.thresholds, seeded=seeded, **kw)


def compare_device(case, exe, seeded=False, **kw):
    """Device counts against full_rule (exact Fractions) and the triples against lazy_rule's."""
    from rambl_amd import profile
    full, triples = check_rules(case, exe)
    res = device_counts(case, seeded, **kw)
    print("%s%s: %d triples, %s" % (case.name, " seeded" if seeded else "", len(res), res.stats.as_dict()))
    got = Counter()
    for g, times, share, n in res.triples:
        got[(case.names[g], times, share)] += n
    assert [t[:3] for t in res.triples] == sorted(t[:3] for t in res.triples) and len(got) == len(res.triples)
    assert profile.counts_from_triples(res.triples, case.names) == full
    assert got == triples
    assert res.stats.n_reads_counted == sum(Fraction(n, share) for (_, _, share), n in triples.items())
    return res


def spread_mismatches(piece, k):
    """The piece with k evenly spread substitutions, none at an end."""
    x = list(piece)
    for i in range(k):
        p = (i + 1) * len(x) // (k + 1)
        x[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[x[p]]
    return "".join(x)


def _other(c):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[c]


def _hit(rows, seg, gene):
    got = [r for r in rows if r[0] == seg and r[1] == gene]
    return got[0] if got else None


def _pct(r):
    return 100.0 * int(r[2]) / int(r[3])


def parity_case():
    genes, segs = PL.parity_dataset()
    ids = []
    for k in range(len(segs)):
        kind = k % 5
        ids.append(("p%d/1" % (k // 5), "p%d/2" % (k // 5), "p%d.1" % (k // 5), "s%d" % k, "t%d.2" % k)[kind])

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(len(rows) > 200 and len(all_rows) > len(rows), "hits, and pairs that fail -I only")
        need(any(t[2] >= 2 for t in triples) and len(set(map(read_of, case.ids))) < len(case.ids), "a shared read, reads of several segments")
        need(any(n > 0 for n in failed.values()), "a read whose best group fails -I")
    return CountCase("parity", genes, segs, ids, check)


def parity_loose_case():
    c = parity_case()
    return CountCase("parity_loose", c.genes, c.segs, c.ids, None, (0.0, 10.0, 1.28, 0.46))


def mixture_cases():
    from rambl_amd import profile
    names, seqs, samples = PL.mixture_dataset()
    out = []
    for sample, lines, _ in samples:
        segments = profile.extract_segments(PL.sam_records(lines))
        c = CountCase("mixture_" + sample, seqs, [s.decode() for _, s in segments], [q.decode() for q, _ in segments], None)
        c.names = names
        out.append(c)
    return out


def advance_case(seed=51):
    rng = random.Random(seed)
    a, b = L.rand_seq(rng, 300), L.rand_seq(rng, 300)
    sep = "".join(next(c for c in "ACGT" if c not in avoid) for avoid in ((a[160], b[98]), (a[161], b[99])))      # extends neither piece
    segs = [spread_mismatches(a[60:160], 6) + sep + b[100:150], a[10:110], b[200:280]]
    ids = ["adv", "na", "nb"]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        top, second = _hit(all_rows, "adv", "g00000"), _hit(all_rows, "adv", "g00001")
        need(top and second and (int(top[2]), int(top[3])) == (94, 100) and _pct(top) < 95.0, "the best gene has 94 of 100 columns")
        need(float(top[8]) < float(second[8]) and (int(second[2]), int(second[3])) == (50, 50), "the second gene is a clean 50-base hit")
        need(failed["adv"] == 1 and dict(full)["g00001"] == 2, "the top group fails, the second gives the read to the second gene")
    return CountCase("advance", [a, b], segs, ids, check)


def exhausted_case(seed=52):
    rng = random.Random(seed)
    a, b = L.rand_seq(rng, 300), L.rand_seq(rng, 300)
    segs = [a[20:100], spread_mismatches(a[60:160], 6) + spread_mismatches(b[100:180], 5), b[30:130]]
    ids = ["n1", "gone", "n2"]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        mine = [r for r in all_rows if r[0] == "gone"]
        need(len(mine) == 2 and all(_pct(r) < 95.0 for r in mine) and failed["gone"] == 2, "both groups of the read fail -I")
        need(dict(full) == {"g00000": 1, "g00001": 1}, "the neighbours count")
    return CountCase("exhausted", [a, b], segs, ids, check)


def strand_trap_case(seed=99):
    rng = random.Random(seed)
    gene = L.rand_seq(rng, 400)
    x = list(gene[50:139])
    for p in range(12, 89, 13):
        x[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[x[p]]
    segs = ["".join(x) + L.revcomp(gene[200:240]), gene[300:360]]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        trap = _hit(all_rows, "trap", "g00000")
        need(trap and int(trap[6]) < int(trap[7]) and _pct(trap) < 95.0, "the forward strand wins and fails -I")
        need(not _hit(rows, "trap", "g00000") and dict(full) == {"g00000": 1}, "the pair gives nothing, the other read counts")
    return CountCase("strand_trap", [gene], segs, ["trap", "other"], check)


def mates_case(seed=54):
    rng = random.Random(seed)
    g = [L.rand_seq(rng, 300) for _ in range(3)]
    tail = _other(g[1][150]) + L.rand_seq(rng, 19)              # the flank does not extend the match
    segs = [g[0][20:120], g[0][150:250],                        # a: both mates on one gene
            g[0][30:130], g[1][30:130],                         # b: two genes, equal E6
            g[0][40:140], g[1][50:150] + tail,       # c: equal scores, 100 and 120 bases
            g[0][60:160], g[0][170:270], g[1][60:160],          # d: three segments
            g[2][10:110]]
    ids = ["a/1", "a/2", "b/1", "b/2", "c/1", "c/2", "d/1", "d/2", "d.1", "e"]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        c1, c2 = _hit(rows, "c/1", "g00000"), _hit(rows, "c/2", "g00001")
        need(c1 and c2 and (c1[2], c1[3], c2[2], c2[3]) == ("100",) * 4 and (c1[9], c2[9]) == ("100", "120"), "mates c: 100 columns each")
        need(float(c1[8]) < float(c2[8]), "equal scores, different lengths: no tie")
        need(triples == Counter({("g00000", 2, 1): 2, ("g00000", 1, 2): 1, ("g00001", 1, 2): 1, ("g00000", 1, 1): 1, ("g00002", 1, 1): 1}),
             "a and d give gene 0 two, b halves, c goes to gene 0")
    return CountCase("mates", g, segs, ids, check)


def e6_edge_case(at_e6, seed=55):
    """A clean hit whose E rounds up in six digits; T = E (the hit path emits the row, the counting rule drops it) or, with
    at_e6, T = E6 (it counts)."""
    from rambl_amd import capi
    rng = random.Random(seed)
    g = [L.rand_seq(rng, 300) for _ in range(2)]
    n = 600
    for length in range(60, 120):
        e = 0.46 * float(length) * float(n) * math.exp(-1.28 * (0.5 * float(2 * length)))
        e6 = capi.profile_evalue6(length, n, 2 * length)
        if e6 > e:
            break
    segs = [g[0][20:20 + length], g[1][10:150]]
    th = (95.0, e6 if at_e6 else e, 1.28, 0.46)

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        edge = _hit(rows, "edge", "g00000")
        need(e < e6 and edge and int(edge[2]) == length and float(edge[8]) == e6, "the hit path emits the hit, E <= T, and E6 > E")
        need(dict(full) == ({"g00000": 1, "g00001": 1} if at_e6 else {"g00001": 1}), "it counts only with T = E6")
    return CountCase("e6_edge_at_e6" if at_e6 else "e6_edge_at_e", g, segs, ["edge", "plain"], check, th)


def wide_tie_case(seed=56, n_genes=2049):
    rng = random.Random(seed)
    common, private = L.rand_seq(rng, 60), L.rand_seq(rng, 60)
    genes = [common] * n_genes
    genes[7] = common + private
    segs = [common, private]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(len(triples) == n_genes + 1 and all(t[2] == n_genes for t in triples if t[1:] != (1, 1)), "one read shared by all genes")
        d = dict(full)
        need(d["g00007"] == 1 + Fraction(1, n_genes) and d["g02048"] == Fraction(1, n_genes), "the second read is added exactly")
    return CountCase("wide_tie", genes, segs, ["wide", "one"], check)


def deep_groups_case(seed=57):
    rng = random.Random(seed)
    g = [L.rand_seq(rng, 300) for _ in range(6)]
    seg = (spread_mismatches(g[0][50:150], 6) + spread_mismatches(g[1][50:140], 6) + spread_mismatches(g[2][50:130], 5) +
           spread_mismatches(g[3][50:120], 4) + g[4][50:90])
    segs = [seg, g[5][100:200], spread_mismatches(g[0][150:250], 6) + spread_mismatches(g[1][150:240], 6) +
            spread_mismatches(g[2][150:230], 5) + spread_mismatches(g[3][150:220], 4)]
    ids = ["deep", "plain", "deep_gone"]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(failed["deep"] > COUNT_ROUNDS and dict(full).get("g00004") == 1, "more failing groups than rounds, then a passing one")
        need(failed["deep_gone"] > COUNT_ROUNDS and "deep_gone" not in {r[0] for r in rows}, "and a read that runs out in the tail")
    return CountCase("deep_groups", g, segs, ids, check)


def strides_case(seed=58):
    rng = random.Random(seed)
    a, b = L.rand_seq(rng, 60), L.rand_seq(rng, 60)
    genes = [a, b] * 8
    segs = []
    for k in range(READ_BLOCKS + 108):
        r = L.mutate(rng, (a, b)[k % 2][rng.randint(0, 20):][:40], 0.01)
        segs.append(L.revcomp(r) if k % 3 == 0 else r)
    ids = ["r%d" % k for k in range(len(segs))]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(len(segs) > READ_BLOCKS, "more reads than the per-read kernels have blocks")
        need(looked > REC_BLOCKS * 256 and looked > 8192 and len({len(s) for s in segs}) == 1,
             "more pairs in the first round, in one bucket, than the per-record kernels have threads and the trace kernel has blocks")
        late = {r[0] for r in rows[REC_BLOCKS * 256:]}
        need(len(late) > 50, "hits on the second trip")
    return CountCase("strides", genes, segs, ids, check)


def conserved_case(seed=59, n_genes=32, n_segs=400):
    rng = random.Random(seed)
    block = L.rand_seq(rng, 60)
    genes = [L.rand_seq(rng, 60) + block + L.rand_seq(rng, 60) for _ in range(n_genes)]
    segs = []
    for k in range(n_segs):
        g = genes[k % n_genes]
        segs.append(g[50:130] if k % 2 == 0 else g[rng.randint(0, 100):][:80])
        if k % 3 == 0:
            segs[-1] = L.revcomp(segs[-1])
    ids = ["c%d" % k for k in range(n_segs)]

    def check(case, rows, all_rows, out):
        full, triples, looked, failed = out
        need(len(all_rows) >= n_segs // 2 * n_genes, "the segments over the block hit every gene")
        need(5 * looked <= len(all_rows), "the lazy rule looks at no more than a fifth of the pairs the hit path traces")
    return CountCase("conserved", genes, segs, ids, check)


NAMED = {"advance": advance_case, "exhausted": exhausted_case, "strand_trap": strand_trap_case, "mates": mates_case,
         "e6_edge_at_e": lambda: e6_edge_case(False), "e6_edge_at_e6": lambda: e6_edge_case(True), "wide_tie": wide_tie_case,
         "deep_groups": deep_groups_case, "strides": strides_case, "conserved": conserved_case}
_CASES = {}


def case(name):
    """A named case, the parity sets or a mixture sample, built once."""
    if name not in _CASES:
        if name in NAMED:
            _CASES[name] = NAMED[name]()
        elif name == "parity":
            _CASES[name] = parity_case()
        elif name == "parity_loose":
            _CASES[name] = parity_loose_case()
        else:
            for c in mixture_cases():
                _CASES[c.name] = c
    return _CASES[name]


DATASETS = ("parity", "parity_loose", "mixture_sample0", "mixture_sample1", "mixture_sample2")
