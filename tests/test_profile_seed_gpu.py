"""GPU: the seeded gene profile (sc_profile_hits_seeded: k_seed_keys, k_seed_lookup, k_bl_score_pairs in
rambl_amd/csrc/sc_profile_seed.hpp and sc_profile_dp.hpp) against the unseeded call and the plain restatements: equal hits field by
field, and the pair list's size, cells and tiles against tests/seed_lib.py wherever the call was seeded."""
import math
import os
import random

import pytest

import align_edge_lib as E
import profile_lib as PL
import seed_lib as S
import stage4_lib as L

pytestmark = pytest.mark.gpu

DEFAULTS = (95.0, 1e-10, 1.28, 0.46)
LOOKUP_BLOCKS = 8192                                                  # sc_profile_seed.hpp: blocks of one wavefront, one segment each


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


def _run(genes, segs, thresholds, seeded, **kw):
    from rambl_amd import capi
    return capi.profile_hits([g.encode() for g in genes], [s.encode() for s in segs], *thresholds, seeded=seeded, **kw)


def both_modes(genes, segs, thresholds=DEFAULTS, exp=None, name="seeded"):
    """Seeded against unseeded (and the restatement's hits `exp` when given), then the seeded call's statistics against
    seed_lib.  Returns (hits, seeded result, the expected pairs or None when the call ran unseeded)."""
    plain, seeded = _run(genes, segs, thresholds, False), _run(genes, segs, thresholds, True)
    hits = PL.device_hits(plain)
    got = PL.device_hits(seeded)
    assert got == hits, "%s: %d hits seeded, %d unseeded, first differences %s" % (
        name, len(got), len(hits), [(a, b) for a, b in zip(got, hits) if a != b][:3])
    if exp is not None:
        assert hits == [PL.as_csv_fields(h) for h in exp]
    n = sum(len(g) for g in genes)
    possible = [k for k, s in enumerate(segs) if S.least_score2(len(s), n, thresholds[1], thresholds[2], thresholds[3]) is not None]
    k = S.seed_length([len(segs[p]) for p in possible], n, *thresholds)
    st = seeded.stats
    print("%s: seed_k %d, %d pairs of %d, %s" % (name, st.seed_k, st.n_pairs, len(possible) * len(genes), st.as_dict()))
    assert st.seed_k == k and st.n_hits == len(hits) and st.n_candidates <= plain.stats.n_candidates
    if k == 0:
        assert st.n_tiles == plain.stats.n_tiles and st.score_cells == plain.stats.score_cells and st.n_pairs == 0
        assert st.n_candidates == plain.stats.n_candidates
        return hits, seeded, None
    pairs = {(possible[s], g) for s, g in S.sharing_pairs(genes, [segs[p] for p in possible], k)}
    assert st.n_pairs == len(pairs) and st.n_tiles == 2 * len(pairs)
    assert st.score_cells == sum(2 * len(segs[s]) * len(genes[g]) for s, g in pairs)
    assert st.n_gene_kmers == sum(sum(1 for p in range(len(g) - k + 1) if set(g[p:p + k].upper()) <= set("ACGT")) for g in genes)
    assert {(h[0], h[1]) for h in hits} <= pairs
    return hits, seeded, pairs


@pytest.fixture(scope="module")
def parity(hits_check):
    genes, segs = PL.parity_dataset()
    return genes, segs, PL.run_hits_check(hits_check, genes, segs, *DEFAULTS)


def test_parity_dataset_seeded_equals_unseeded_equals_restatement(parity):
    genes, segs, exp = parity
    hits, res, pairs = both_modes(genes, segs, exp=exp, name="parity")
    assert res.stats.seed_k == 13 and len(hits) > 200
    assert {(len(segs[s]) + 63) // 64 for s, _ in pairs} == set(range(1, 9))                 # every bucket has pairs
    assert 0 < res.stats.n_tiles < 2 * len(segs) * len(genes)                                 # strictly below the full product
    assert res.stats.score_cells < 2 * sum(map(len, segs)) * sum(map(len, genes))


def test_identity_90_runs_unseeded(parity):
    genes, segs, _ = parity
    hits, res, pairs = both_modes(genes[:6], segs[:150], (90.0, 1e-10, 1.28, 0.46), name="I 90")
    assert pairs is None and res.stats.seed_k == 0 and res.stats.n_tiles == 2 * 150 * 6 and len(hits) > 20


def test_unseeded_run_reports_what_the_plain_entry_point_does(parity):
    """seed_k == 0: sc_profile_hits_seeded's counters are sc_profile_hits's on the same call, and what is the seeded mode's
    own stays 0."""
    from rambl_amd import capi
    genes, segs, _ = parity
    genes, segs, thresholds = genes[:6], segs[:150], (90.0, 1e-10, 1.28, 0.46)
    assert capi.profile_seed_length([len(s) for s in segs], sum(len(g) for g in genes), *thresholds) == 0     # no device needed
    plain, seeded = _run(genes, segs, thresholds, False).stats, _run(genes, segs, thresholds, True).stats
    print("plain %s\nseeded %s" % (plain.as_dict(), seeded.as_dict()))
    assert seeded.seed_k == 0 and plain.n_tiles == 2 * 150 * 6 and plain.n_hits > 20 and plain.trace_cells > 0
    for field in ("score_cells", "trace_cells", "n_tiles", "n_candidates", "n_traced", "n_hits"):
        assert getattr(seeded, field) == getattr(plain, field), field
    assert seeded.n_pairs == 0 and seeded.n_gene_kmers == 0 and seeded.index_ms == 0 and seeded.lookup_ms == 0


@pytest.mark.parametrize("name", sorted(E.PROFILE_CASES))
def test_named_case(name, hits_check):
    case = E.PROFILE_CASES[name]()
    rows = PL.run_hits_check(hits_check, case.genes, case.segs, *case.thresholds())
    both_modes(case.genes, case.segs, case.thresholds(), exp=rows, name=name)


def test_segment_order_does_not_matter(parity):
    genes, segs, _ = parity
    segs = segs[:200]
    first = PL.device_hits(_run(genes, segs, DEFAULTS, True))
    order = list(range(len(segs)))
    random.Random(5).shuffle(order)
    again = PL.device_hits(_run(genes, [segs[k] for k in order], DEFAULTS, True))
    assert len(first) > 50 and sorted(((order[h[0]],) + h[1:] for h in again), key=lambda h: h[:2]) == first


# ---- named seed edges.  At -I 100 a hit has no column but identity columns, so k*(L) = ceil(min2(L) / 2); with -e set to the
# E-value of 13 matched bases of a 13-base segment, min2(13) = 26 and a call that holds a 13-base segment has K = 13.

def _exact_thresholds(genes, k=13):
    n = sum(len(g) for g in genes)
    return (100.0, 0.46 * float(k) * float(n) * math.exp(-1.28 * (0.5 * float(2 * k))), 1.28, 0.46)


def _only_shared(seg, gene, k=13):
    """The k-mers the segment (forward, reverse complement) shares with the gene."""
    return S.kmers(seg, k) & S.kmers(gene, k), S.kmers(S.revcomp(seg), k) & S.kmers(gene, k)


def test_seed_edges(hits_check):
    rng = random.Random(4242)
    genes = [L.rand_seq(rng, 80) for _ in range(4)]
    whole3 = genes[3]
    genes[3] = whole3[:40] + "N" + whole3[41:]                       # an N in the gene breaks the windows over column 40
    th = _exact_thresholds(genes)
    j = lambda n: L.rand_seq(rng, n)                                 # noqa: E731
    segs = {
        "exactly_k": genes[0][20:33],
        "k_minus_1": genes[0][20:32],
        "gene_first_window": genes[1][:13],
        "gene_last_window": genes[1][-13:],
        "gene_first_window_long": j(20) + genes[1][:13] + j(20),
        "gene_last_window_long": j(20) + genes[1][-13:] + j(20),
        "segment_last_window": j(30) + genes[2][30:43],
        "reverse_only": S.revcomp(genes[2][10:23]),
        "reverse_only_long": S.revcomp(j(15) + genes[2][50:63] + j(15)),
        "across_genes": genes[0][-6:] + genes[1][:7],
        "across_genes_long": j(20) + genes[1][-7:] + genes[2][:6] + j(20),
        "n_in_gene": whole3[34:47],
        "n_in_segment": genes[0][40:46] + "N" + genes[0][47:53],
        "n_in_segment_long": j(10) + genes[0][40:46] + "N" + genes[0][47:53] + j(10),
    }
    names, texts = list(segs), list(segs.values())
    at = {n: k for k, n in enumerate(names)}
    exp = PL.run_hits_check(hits_check, genes, texts, *th)
    hits, res, pairs = both_modes(genes, texts, th, exp=exp, name="seed edges")
    assert res.stats.seed_k == 13
    by = {names[h[0]]: h for h in hits}
    # a segment of exactly K bases hits, one of K - 1 cannot pass and is in no bucket
    assert by["exactly_k"][1:3] == (0, 0) and by["exactly_k"][4:6] == (13, 13) and "k_minus_1" not in by
    assert (at["k_minus_1"], 0) not in pairs and S.least_score2(12, 320, th[1]) is None
    # the first and the last window of a gene
    assert by["gene_first_window"][8:10] == (1, 13) and by["gene_last_window"][8:10] == (68, 80)
    for n, kmer in (("gene_first_window_long", genes[1][:13]), ("gene_last_window_long", genes[1][-13:])):
        fw, rv = _only_shared(segs[n], genes[1])
        assert kmer in fw and len(fw) <= 2 and not rv and (at[n], 1) in pairs          # (a flank may match one base further)
    # the segment's last window
    assert _only_shared(segs["segment_last_window"], genes[2]) == ({segs["segment_last_window"][-13:]}, set())
    assert (at["segment_last_window"], 2) in pairs
    # the forward strand shares nothing, the reverse strand gives the hit
    assert _only_shared(segs["reverse_only"], genes[2]) == (set(), {genes[2][10:23]})
    assert by["reverse_only"][1:3] == (2, 1) and by["reverse_only"][8:10] == (23, 11)
    fw, rv = _only_shared(segs["reverse_only_long"], genes[2])
    assert not fw and genes[2][50:63] in rv and len(rv) <= 2 and (at["reverse_only_long"], 2) in pairs
    # a k-mer that exists only across the boundary of two adjacent genes gives no pair
    for n in ("across_genes", "across_genes_long"):
        assert not [p for p in pairs if p[0] == at[n]] and n not in by
    assert segs["across_genes"] in "".join(genes) and genes[1][-7:] + genes[2][:6] in "".join(genes)
    # an N in the gene, an N in the segment
    for n in ("n_in_gene", "n_in_segment", "n_in_segment_long"):
        assert not [p for p in pairs if p[0] == at[n]] and n not in by
    assert segs["n_in_gene"] in whole3
    assert res.stats.n_pairs == len(pairs) == 8


def test_strand_choice_trap(hits_check):
    """The forward optimum scores higher but fails -I 95 and shares no 13-mer (runs of 12 between mismatches); the reverse
    complement holds 40 exact gene bases, scores lower and would pass.  The pair is scored on both strands, the forward strand
    wins, the identity filter drops it: no hit in either mode.  Scored on the sharing strand alone it would be a hit."""
    rng = random.Random(99)
    gene = L.rand_seq(rng, 400)
    x = list(gene[50:139])                                           # the last run has 11 bases: a chance match after it makes 12
    for p in range(12, 89, 13):
        x[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[x[p]]
    seg = "".join(x) + S.revcomp(gene[200:240])
    other = gene[300:360]
    fw, rv = _only_shared(seg, gene)
    assert not fw and 28 <= len(rv) <= 36                            # (the flank may match a few bases further)
    exp = PL.run_hits_check(hits_check, [gene], [seg, other], *DEFAULTS)
    loose = PL.run_hits_check(hits_check, [gene], [seg, other], 0.0, *DEFAULTS[1:])
    assert [h[0] for h in exp] == [1]
    trap = [h for h in loose if h[0] == 0][0]
    assert trap[2] == 0 and trap[3] > 120 and 100.0 * trap[4] / trap[5] < 95.0                # forward, above the reverse's 2 * 40
    alone = PL.run_hits_check(hits_check, [gene], [S.revcomp(gene[200:240])], *DEFAULTS)
    assert len(alone) == 1 and alone[0][3] == 80                                             # what the reverse strand alone would give
    hits, res, pairs = both_modes([gene], [seg, other], exp=exp, name="strand trap")
    assert res.stats.seed_k == 13 and pairs == {(0, 0), (1, 0)} and res.stats.n_tiles == 4 and [h[0] for h in hits] == [1]


@pytest.mark.parametrize("n_genes", (31, 32, 33, 63, 64, 65, 2049))
def test_bitset_word_edges_and_a_long_posting_run(n_genes, hits_check):
    """One 13-mer is in every gene (a posting run of n_genes keys), the gene counts cross the bitset's word edges, and the last
    gene is hit."""
    rng = random.Random(n_genes)
    common = L.rand_seq(rng, 13)
    genes = []
    for _ in range(n_genes):
        a = rng.randint(0, 47)
        g = L.rand_seq(rng, 60)
        genes.append(g[:a] + common + g[a + 13:])
    segs = [genes[-1], L.rand_seq(rng, 20) + common + L.rand_seq(rng, 27), S.revcomp(genes[0]), L.rand_seq(rng, 60)]
    exp = PL.run_hits_check(hits_check, genes, segs, *DEFAULTS)
    hits, res, pairs = both_modes(genes, segs, exp=exp, name="%d genes" % n_genes)
    assert res.stats.seed_k == 13 and res.stats.n_pairs >= 3 * n_genes
    assert {g for s, g in pairs if s == 1} == set(range(n_genes))
    assert (0, n_genes - 1) in {(h[0], h[1]) for h in hits} and (2, 0) in {(h[0], h[1]) for h in hits}


def test_duplicate_genes(hits_check):
    rng = random.Random(12)
    g, h = L.rand_seq(rng, 200), L.rand_seq(rng, 150)
    genes = [g, g, h, g]
    segs = [g[30:110], S.revcomp(L.mutate(rng, g[100:190], 0.02)), h[20:100], L.rand_seq(rng, 80)]
    exp = PL.run_hits_check(hits_check, genes, segs, *DEFAULTS)
    hits, res, pairs = both_modes(genes, segs, exp=exp, name="duplicates")
    assert pairs == {(0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (1, 3), (2, 2)} and len(hits) == 7


def test_second_trip_of_the_lookup_and_of_the_pair_score_loop(hits_check):
    """More segments in one bucket than the lookup has blocks, and more pairs' tiles than the score kernel has wavefronts."""
    rng = random.Random(2)
    a, b = L.rand_seq(rng, 60), L.rand_seq(rng, 60)
    genes = [a, b] * 4
    segs = []
    for k in range(LOOKUP_BLOCKS + 200):
        r = L.mutate(rng, (a, b)[k % 2][rng.randint(0, 20):][:40], 0.01)
        segs.append(S.revcomp(r) if k % 3 == 0 else r)
    exp = PL.run_hits_check(hits_check, genes, segs, *DEFAULTS)
    hits, res, pairs = both_modes(genes, segs, exp=exp, name="second trips")
    assert res.stats.seed_k == 13 and len(segs) > LOOKUP_BLOCKS and res.stats.n_tiles > E.SCORE_BLOCKS * E.SCORE_WAVES
    late = {h[0] for h in hits if h[0] > LOOKUP_BLOCKS}
    assert len(late) > 150 and len(hits) > 4 * LOOKUP_BLOCKS * 0.9


def test_no_pair_shares_a_kmer():
    rng = random.Random(77)
    genes = [L.rand_seq(rng, 300) for _ in range(5)]
    segs = [L.rand_seq(rng, n) for n in (60, 100, 150, 200, 300)]
    assert not S.sharing_pairs(genes, segs, 13)
    hits, res, pairs = both_modes(genes, segs, name="no pair")
    st = res.stats
    assert pairs == set() and not hits and st.seed_k == 13
    assert (st.n_pairs, st.n_tiles, st.n_candidates, st.n_traced, st.score_cells, st.trace_cells) == (0, 0, 0, 0, 0, 0)


def test_command_line_seeded_writes_the_same_files(tmp_path):
    from rambl_amd import profile
    names, seqs, samples = PL.mixture_dataset()
    fa, sams = PL.write_mixture(tmp_path, names, seqs, samples)
    sample, sam = samples[0][0], sams[0]
    for flag, out in ((["--seeded"], "seeded"), ([], "plain")):
        assert profile.main([fa, sam, sample, "-n", "-v", "-o", os.path.join(str(tmp_path), out), "--keep-hits"] + flag) == 0
    for f in (sample + "_gene_count.tsv", sample + "_hits.csv"):
        a = open(os.path.join(str(tmp_path), "seeded", f), "rb").read()
        assert a == open(os.path.join(str(tmp_path), "plain", f), "rb").read() and a.count(b"\n") > 5
