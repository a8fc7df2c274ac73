"""CPU: the seed length of the seeded gene profile (sc_profile_seed_length) against the brute-force
restatement tests/seed_lib.py, and the lemma behind it on the restatement of the hit contract
(tests/native/blast_hits_check.cpp): every emitted hit's two slices have a common run of k*(L) bases or more."""
import pytest

import align_edge_lib as E
import profile_lib as PL
import seed_lib as S

GENE_BASES = (200, 3000, 150000, 1500000)


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@pytest.mark.parametrize("max_evalue", (1e-10, 1e-30, 10.0))
@pytest.mark.parametrize("min_identity", (0.0, 90.0, 95.0, 97.0, 100.0))
def test_seed_length_equals_brute_force(min_identity, max_evalue):
    from rambl_amd import capi
    none = 0
    for n in GENE_BASES:
        exp = [S.lossless_k(L, n, min_identity, max_evalue) for L in range(1, 513)]
        got = [capi.profile_seed_length([L], n, min_identity, max_evalue, lossless=True) for L in range(1, 513)]
        assert got == exp, [(L + 1, e, g) for L, (e, g) in enumerate(zip(exp, got)) if e != g][:5]
        none += exp.count(None)
        # the call's K: 0 below 11 and when nothing can pass, at most 16; the least over the lengths of the call
        for L in (1, 20, 40, 50, 150, 512):
            k = exp[L - 1]
            assert capi.profile_seed_length([L], n, min_identity, max_evalue) == (0 if k is None or k < 11 else min(k, 16))
        for lens in ([150, 512, 60], [3, 7], [512, 512, 33, 150], list(range(1, 513))):
            assert capi.profile_seed_length(lens, n, min_identity, max_evalue) == S.seed_length(lens, n, min_identity, max_evalue)
    assert none > 0 or max_evalue == 10.0                            # lengths that cannot pass are in the grid


def test_seed_length_at_the_defaults_and_by_identity():
    from rambl_amd import capi
    for n in GENE_BASES:
        ks = {capi.profile_seed_length([L], n, lossless=True) for L in range(50, 513)}
        assert ks == {13}
    assert {capi.profile_seed_length([L], 280000000, lossless=True) for L in range(60, 513)} == {14}
    table = {100: 31, 99: 31, 97: 17, 95: 13, 90: 8, 80: 4, 50: 3, 0: 3}
    assert {i: capi.profile_seed_length([150], 150000, float(i), lossless=True) for i in table} == table
    assert [capi.profile_seed_length([150], 150000, float(i)) for i in (100, 97, 95, 90)] == [16, 16, 13, 0]
    assert capi.profile_seed_length([], 1000) == 0 and capi.profile_seed_length([5, 9], 1000, lossless=True) is None
    with pytest.raises(capi.StrainCallError):
        capi.profile_seed_length([513], 1000)


def _assert_lemma(hits, genes, segs, thresholds, name):
    """Every hit's slices have a common run of k*(L) or more; returns k* per hit."""
    n = sum(len(g) for g in genes)
    k_of = {}
    out = []
    for h in hits:
        L = len(segs[h[0]])
        if L not in k_of:
            k_of[L] = S.lossless_k(L, n, *thresholds)
        a, b = S.hit_slices(h, genes, segs)
        assert k_of[L] is not None and S.has_common_run(a, b, k_of[L]), "%s: hit %s has a longest common run of %d, k* = %s" % (
            name, h, S.longest_common_run(a, b), k_of[L])
        out.append(k_of[L])
    return out


def test_lemma_on_the_parity_dataset(hits_check):
    genes, segs = PL.parity_dataset()
    for thresholds in ((95.0, 1e-10, 1.28, 0.46), (90.0, 1e-10, 1.28, 0.46)):
        hits = PL.run_hits_check(hits_check, genes, segs, *thresholds)
        assert len(hits) > 200
        _assert_lemma(hits, genes, segs, thresholds, "parity")


@pytest.mark.parametrize("name", sorted(E.PROFILE_CASES))
def test_lemma_on_the_named_cases(name, hits_check):
    case = E.PROFILE_CASES[name]()
    hits = PL.run_hits_check(hits_check, case.genes, case.segs, *case.thresholds())
    assert hits
    _assert_lemma(hits[::max(1, len(hits) // 400)] if name in ("score_stride", "trace_stride") else hits, case.genes, case.segs,
                  case.thresholds(), name)


def tight_family(seed=77):
    """Hits that reach the bound.  One gene of 400 random bases.  Segment 0: 40 gene bases with the bases after aligned
    columns 13 and 26 changed: i = 38, m = 2, identity exactly 95 %, doubled score 68, runs of 13, 13 and 12.  Segment 1: its
    one-base-shorter neighbour (39 columns, 37 / 39 < 95 %), which must not pass.  Segment 2: the same shape on the reverse
    strand.  Segment 3: mismatches after 13 and 27 of 41 (runs 13, 13, 13; 39 / 41 = 95.12 %).  Thresholds at the defaults: a
    segment of 40 bases passes -e 1e-10 from a doubled score of 50 on against 400 gene bases."""
    import random
    import stage4_lib as L
    rng = random.Random(seed)
    gene = L.rand_seq(rng, 400)

    def broken(a, n, at):
        r = list(gene[a:a + n])
        for p in at:
            r[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[r[p]]
        return "".join(r)
    segs = [broken(100, 40, (13, 27)), broken(100, 39, (13, 27)), L.revcomp(broken(200, 40, (13, 27))), broken(300, 41, (13, 27))]
    return [gene], segs, (95.0, 1e-10, 1.28, 0.46)


def test_tight_cases_reach_the_bound(hits_check):
    genes, segs, thresholds = tight_family()
    n = len(genes[0])
    assert [S.lossless_k(len(s), n, *thresholds) for s in segs] == [13, 13, 13, 13]
    hits = PL.run_hits_check(hits_check, genes, segs, *thresholds)
    by_seg = {h[0]: h for h in hits}
    assert set(by_seg) == {0, 2, 3}, hits                            # the one-base-shorter neighbour does not pass
    assert (by_seg[0][4], by_seg[0][5]) == (38, 40) and (by_seg[2][4], by_seg[2][5], by_seg[2][2]) == (38, 40, 1)
    assert _assert_lemma(hits, genes, segs, thresholds, "tight") == [13, 13, 13]
    assert [S.longest_common_run(*S.hit_slices(h, genes, segs)) for h in hits] == [13, 13, 13]      # the bound is reached
    # without the identity threshold the neighbour is a hit: it is the threshold that drops it
    loose = PL.run_hits_check(hits_check, genes, segs, 0.0, *thresholds[1:])
    assert {h[0] for h in loose} == {0, 1, 2, 3}
