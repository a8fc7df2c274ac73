"""A cohort against one resident gene index (sc_profile_index_counts): the named inputs of its edges, each
with a check that raises unless the input still reaches its edge, and what to expect of them from what exists -- per sample
the counting rule on the plain restatement's hits (count_lib.check_rules) and capi.profile_counts on the sample alone.

plan_stretches is restated here over Python ints so that a case can prove where its stretch boundaries fall."""
import math
import random
from collections import Counter

import count_lib as CL
import profile_lib as PL
import stage4_lib as L
from align_edge_lib import need

MAX_SAMPLES = 65536                     # sc_profile_counts.hpp
CL_ROOM = 1 << 23                       # sc_profile_counts.hpp: COUNT_ROOM, the default cand_room
SEAMS_ROOM = 18 * 300                   # the seams case: 300 segments of the mixture against its 9 genes


def can_pass(length, gene_bases, thresholds=CL.DEFAULTS):
    """A segment of this length passes -e with every base matched (raw score = length)."""
    _, max_evalue, ka_lambda, ka_k = thresholds
    return ka_k * float(length) * float(gene_bases) * math.exp(-ka_lambda * float(length)) <= max_evalue


def plan_stretches(read_lens, n_genes, gene_bases, room, thresholds=CL.DEFAULTS):
    """sc_profile_counts.hpp's plan, unseeded: read_lens[r] = the lengths of read r's segments; a read costs 2 * n_genes
    tiles per segment that can pass; whole reads in order, a stretch closes when it is not empty and the next read would
    exceed the room.  Returns [(first read, end read)]; a stretch without a tile is none."""
    out, first, tiles = [], 0, 0
    for r, lens in enumerate(read_lens):
        cost = sum(2 * n_genes for n in lens if can_pass(n, gene_bases, thresholds))
        if tiles > 0 and tiles + cost > room:
            out.append((first, r))
            first, tiles = r, 0
        tiles += cost
    if tiles > 0:
        out.append((first, len(read_lens)))
    return out


class Sample:
    """The segments of one sample: ids decide its reads (profile.read_index), segs are text."""

    def __init__(self, ids, segs):
        from rambl_amd import profile
        self.ids, self.segs = list(ids), list(segs)
        self.seg_read, self.n_reads = profile.read_index(self.ids)


class Cohort:
    """genes (text) with their names, the samples in order, and check(cohort, exe): the property that the input reaches its
    edge.  flat() is the call's input: the samples' segments back to back, reads numbered through, a sample per read."""

    def __init__(self, name, genes, names, samples, check=None, thresholds=CL.DEFAULTS):
        self.name, self.genes, self.names, self.samples, self.check, self.thresholds = name, genes, names, samples, check, thresholds

    def n_bases(self):
        return sum(len(g) for g in self.genes)

    def flat(self):
        segs, seg_read, read_sample = [], [], []
        for si, s in enumerate(self.samples):
            segs += [x.encode() for x in s.segs]
            seg_read += [len(read_sample) + r for r in s.seg_read]
            read_sample += [si] * s.n_reads
        return segs, seg_read, read_sample

    def read_lens(self):
        """Per read of the call the lengths of its segments."""
        segs, seg_read, read_sample = self.flat()
        out = [[] for _ in read_sample]
        for s, r in zip(segs, seg_read):
            out[r].append(len(s))
        return out

    def plan(self, room):
        return plan_stretches(self.read_lens(), len(self.genes), self.n_bases(), room, self.thresholds)

    def first_read(self):
        """The call's index of each sample's first read, and the number of reads at the end."""
        at = [0]
        for s in self.samples:
            at.append(at[-1] + s.n_reads)
        return at

    def as_case(self, si):
        """Sample si alone as a count_lib.CountCase (no check of its own)."""
        c = CL.CountCase("%s_%d" % (self.name, si), self.genes, self.samples[si].segs, self.samples[si].ids, None, self.thresholds)
        c.names = self.names
        return c


def device_counts(cohort, index=None, seeded=False, **kw):
    """One call with all samples, on `index` or on a fresh one."""
    from rambl_amd import capi
    segs, seg_read, read_sample = cohort.flat()
    if index is not None:
        return index.counts(segs, seg_read, read_sample, len(cohort.samples), *cohort.thresholds, seeded=seeded, **kw)
    with capi.ProfileIndex([g.encode() for g in cohort.genes]) as ix:
        return ix.counts(segs, seg_read, read_sample, len(cohort.samples), *cohort.thresholds, seeded=seeded, **kw)


_ALONE = {}


def alone(cohort, si, seeded=False):
    """capi.profile_counts on sample si alone, computed once per (cohort, sample, mode)."""
    key = (cohort.name, si, seeded)
    if key not in _ALONE:
        _ALONE[key] = CL.device_counts(cohort.as_case(si), seeded)
    return _ALONE[key]


def check_rows(res):
    """The rows are ascending and distinct."""
    keys = [r[:4] for r in res.rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(r[4] > 0 for r in res.rows)


def compare_alone(cohort, res, seeded=False):
    """Per sample the rows are capi.profile_counts' triples on the sample alone; the statistics that add up do."""
    check_rows(res)
    assert {r[0] for r in res.rows} <= set(range(len(cohort.samples)))
    counted = 0
    for si in range(len(cohort.samples)):
        one = alone(cohort, si, seeded)
        assert res.by_sample(si) == one.triples, (cohort.name, si, res.by_sample(si)[:5], one.triples[:5])
        counted += one.stats.n_reads_counted
    assert res.stats.n_reads_counted == counted and res.stats.n_samples == len(cohort.samples)


def compare_rule(res, si, names, triples):
    """The rows of sample si against lazy_rule's triples (a Counter over (gene name, times, share))."""
    got = Counter()
    for g, times, share, n in res.by_sample(si):
        got[(names[g], times, share)] += n
    assert got == triples, (si, sorted(got.items())[:5], sorted(triples.items())[:5])


def _mixture_samples():
    return [Sample(CL.case("mixture_sample%d" % k).ids, CL.case("mixture_sample%d" % k).segs) for k in range(3)]


def mixture():
    """The three samples of profile_lib.mixture_dataset() in one call."""
    c = CL.case("mixture_sample0")

    def check(cohort, exe):
        need(all(400 <= len(s.segs) <= 500 and s.n_reads < len(s.segs) for s in cohort.samples), "about 450 segments, mates among them")
        need(len(cohort.plan(CL_ROOM)) == 1, "one stretch holds the three samples")
    return Cohort("mixture", c.genes, c.names, _mixture_samples(), check)


def seams():
    """The mixture with a room that cuts inside samples and lets a stretch run over the end of a sample."""
    m = mixture()

    def check(cohort, exe):
        plan, at = cohort.plan(SEAMS_ROOM), cohort.first_read()
        inner = [a for a, _ in plan[1:]]
        need(any(at[s] < a < at[s + 1] for a in inner for s in range(len(cohort.samples))), "a boundary strictly inside a sample")
        need(any(a < at[s] < b for a, b in plan for s in range(1, len(cohort.samples))), "a stretch with the end of one sample and the start of the next")
        need(len(plan) >= 3, "several stretches")
    return Cohort("seams", m.genes, m.names, m.samples, check)


def same_names():
    """Samples 0 and 1 are the same SAM lines, read names included; sample 2 is another."""
    m = mixture()
    samples = [m.samples[0], Sample(m.samples[0].ids, m.samples[0].segs), m.samples[1]]

    def check(cohort, exe):
        need(set(cohort.samples[0].ids) & set(cohort.samples[1].ids), "a read name in both samples")
        _, triples = CL.check_rules(CL.case("mixture_sample0"), exe)
        need(len(triples) > 0, "so every triple of sample 0 occurs in sample 1 too")
    return Cohort("same_names", m.genes, m.names, samples, check)


def gaps(seed=77):
    """Five samples: a real one, one without reads, one of random reads that hit nothing, a real one, one without reads."""
    m = mixture()
    rng = random.Random(seed)
    noise = Sample(["noise%d" % k for k in range(40)], [L.rand_seq(rng, 150) for _ in range(40)])
    samples = [m.samples[0], Sample([], []), noise, m.samples[1], Sample([], [])]

    def check(cohort, exe):
        th = cohort.thresholds
        need(PL.run_hits_check(exe, cohort.genes, cohort.samples[2].segs, 0.0, *th[1:]) == [], "the restatement finds no hit for the random reads")
        need([s.n_reads > 0 for s in cohort.samples] == [True, False, True, True, False], "samples without reads in the middle and at the end")
    c = Cohort("gaps", m.genes, m.names, samples, check)
    c.expected = {0: "mixture_sample0", 3: "mixture_sample1"}
    return c


def ride_along(name):
    """A named case of count_lib as sample 1 with its own genes; mixture_sample0's reads ride along as sample 0."""
    case, rider = CL.case(name), CL.case("mixture_sample0")

    def check(cohort, exe):
        need(len(cohort.samples[0].segs) > 400 and cohort.samples[1].ids == case.ids, "the named case is sample 1, whole")
    return Cohort("ride_" + name, case.genes, case.names, [Sample(rider.ids, rider.segs), Sample(case.ids, case.segs)], check, case.thresholds)


def reuse_calls():
    """(cohort A, cohort B, k of A, k of B) for one index: A has 150-base segments, B exact pieces of the genes of a length
    whose seed length differs from A's."""
    from rambl_amd import capi
    a = mixture()
    bases = a.n_bases()
    k_a = capi.profile_seed_length([150], bases, *a.thresholds)
    length = next(n for n in range(28, 150) if capi.profile_seed_length([n], bases, *a.thresholds) not in (0, k_a))
    k_b = capi.profile_seed_length([length], bases, *a.thresholds)
    rng = random.Random(5)
    samples = []
    for si in range(2):
        segs = []
        for k in range(60):
            g = a.genes[rng.randrange(len(a.genes))]
            p = rng.randint(0, len(g) - length)
            segs.append(g[p:p + length])
        samples.append(Sample(["b%d_%d" % (si, k) for k in range(60)], segs))

    def check(cohort, exe):
        need({len(s) for smp in a.samples for s in smp.segs} == {150}, "call A has 150-base segments only")
        need(k_a >= 11 and k_b >= 11 and k_a != k_b, "both calls run seeded, with different k (%d, %d)" % (k_a, k_b))
    b = Cohort("reuse_b", a.genes, a.names, samples, check)
    return a, b, k_a, k_b


NAMED = {"mixture": mixture, "seams": seams, "same_names": same_names, "gaps": gaps}
_COHORTS = {}


def cohort(name):
    """A named cohort, built once."""
    if name not in _COHORTS:
        _COHORTS[name] = NAMED[name]() if name in NAMED else ride_along(name[len("ride_"):])
    return _COHORTS[name]
