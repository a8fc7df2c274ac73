"""CPU: every named case of tests/seed_edge_lib.py reaches the edge of the seeded gene profile it is named for, by
tests/seed_lib.py and the plain restatement (tests/native/blast_hits_check.cpp) alone, is deterministic, stays inside the
library's limits and runs at the seed length it claims -- by seed_lib and by the library's own sc_profile_seed_length."""
import pytest

import align_edge_lib as E
import count_lib as CL
import profile_lib as PL
import seed_edge_lib as SE
import seed_lib as S


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@pytest.mark.parametrize("name", sorted(SE.CASES))
def test_case_reaches_its_edge(name, hits_check):
    from rambl_amd import capi
    case = SE.case(name)
    if len(case.genes) < 1000:
        assert case.key() == SE.build(name).key()                                          # deterministic
    assert all(1 <= len(g) <= E.MAX_SEED for g in case.genes) and all(1 <= len(s) <= E.MAX_READ for s in case.segs)
    case.check(hits_check)
    n = sum(len(g) for g in case.genes)
    lens = [len(s) for s in case.segs if S.least_score2(len(s), n, *case.thresholds[1:]) is not None]
    assert capi.profile_seed_length(lens, n, *case.thresholds) == case.k


def test_the_families_cover_what_they_claim():
    ks = set(SE.KS)
    assert ks == set(range(S.SEED_MIN_K, S.SEED_MAX_K + 1)) == set(SE.ORDINARY)
    for family in ("ordinary", "exact", "poly_t", "tight"):
        assert {SE.case("%s_k%d" % (family, k)).k for k in ks} == ks
    assert SE.case("clamp").k == 16
    seams = ("per2", "per3", "per8", "nw")
    pers = {k: {SE.lookup_per(len(s), k)[1] for what in seams for s in SE.case("seam_k%d_%s" % (k, what)).segs} for k in (13, 16)}
    assert pers == {13: {1, 2, 3, 8}, 16: {1, 2, 3, 8}}
    assert [len(SE.case("genes_%d" % n).genes) for n in (65535, 65536, 65537, 65569)] == [65535, 65536, 65537, 65569]
    assert SE.GENE_RANGE == 65536 and SE.KEYS_TRIP == 1048576
    assert SE.lookup_per(77, 13) == (65, 2, 33) and SE.lookup_per(141, 13) == (129, 3, 43) and SE.lookup_per(512, 13) == (500, 8, 63)
    assert SE.lookup_per(13, 13) == (1, 1, 1) and SE.lookup_per(79, 16) == (64, 1, 64) and SE.lookup_per(80, 16) == (65, 2, 33)


@pytest.mark.parametrize("k", range(11, 16))
def test_tight_shape_is_on_the_grid(k):
    """The (L, i, m) a tight case is built from is feasible and attains k*(L), and _broken gives it runs of at most k* with
    the first of exactly k* (K = 16 is the exact recipe: i = L = 16, m = 0)."""
    I, e = SE.ORDINARY[k]
    n, i, m = SE.tight_shape(k, 400)
    s2 = S.least_score2(n, 400, e)
    assert i + m == n and 100.0 * i / n >= I and 2 * i - 4 * m >= s2 and -(-i // (m + 1)) == k == S.lossless_k(n, 400, I, e)
    x = SE._broken("ACGT" * 100, 3, i, m)
    runs = [len(r) for r in "".join("=" if a == b else "x" for a, b in zip(x, ("ACGT" * 100)[3:])).split("x")]
    assert len(x) == n and len(runs) == m + 1 and max(runs) == runs[0] == k and sum(runs) == i


@pytest.mark.parametrize("k", SE.KS)
def test_count_case_reaches_its_rule(k, hits_check):
    case = SE.count_case(k)
    assert SE.call_k(case.genes, case.segs, case.thresholds) == k
    CL.check_rules(case, hits_check)
