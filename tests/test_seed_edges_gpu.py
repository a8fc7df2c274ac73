"""GPU: the named edges of the seeded gene profile (tests/seed_edge_lib.py; k_seed_keys, k_seed_lookup and the pair-list score
pass of rambl_amd/csrc/sc_profile_seed.hpp) through the comparison of tests/test_profile_seed_gpu.py: seeded
hits = unseeded hits = the plain restatement's, field by field; seed_k, n_pairs, n_tiles, score_cells and n_gene_kmers as
tests/seed_lib.py gives them; every hit's pair among the expected pairs.  Every seed length from 11 to 16 and the clamp, by
ordinary thresholds and by the exact recipe, through the hit list, the counts and one resident index; hits that reach the
bound; the lane seams of the lookup at 1, 2, 3 and 8 windows per lane; 65 535 to 65 569 genes; more than 1 048 576 gene
bases.  Every case is compared with the restatement: none needed the shortcut of seeded against unseeded alone."""
import pytest

import cohort_lib as HL
import count_lib as CL
import profile_lib as PL
import seed_edge_lib as SE
from test_profile_seed_gpu import both_modes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@pytest.mark.parametrize("name", sorted(SE.CASES))
def test_named_case(name, hits_check):
    case = SE.case(name)
    hits, res, pairs = both_modes(case.genes, case.segs, case.thresholds, exp=case.hits(hits_check), name=name)
    assert res.stats.seed_k == case.k and pairs == case.pairs()
    if case.after:
        case.after(case, hits, pairs)


@pytest.mark.parametrize("k", SE.KS)
def test_counts_at_every_seed_length(k, hits_check):
    res = CL.compare_device(SE.count_case(k), hits_check, seeded=True)
    assert res.stats.seed_k == k and res.stats.n_pairs > 0 and res.stats.n_stretches == 1


def test_one_index_holds_every_seed_length():
    """Six seeded calls on one index, one per seed length: each builds its keys once, the index keeps all six, a seventh call
    at K = 13 builds nothing, and every call's rows are those of a call on a fresh index and of sc_profile_counts."""
    from rambl_amd import capi
    cohorts = {}
    for k in SE.KS:
        c = SE.count_case(k)
        cohorts[k] = HL.Cohort(c.name, c.genes, c.names, [HL.Sample(c.ids, c.segs)], None, c.thresholds)
    fresh = {k: HL.device_counts(c, seeded=True) for k, c in cohorts.items()}
    with capi.ProfileIndex([g.encode() for g in cohorts[11].genes]) as ix:
        for k in SE.KS:
            res = HL.device_counts(cohorts[k], ix, seeded=True)
            assert (res.stats.seed_k, res.stats.n_index_builds) == (k, 1) and res.rows == fresh[k].rows and len(res) >= 3
            assert res.by_sample(0) == CL.device_counts(SE.count_case(k), seeded=True).triples
            assert ix.info()["cached_k"] == list(range(11, k + 1))
        assert ix.info()["cached_k"] == [11, 12, 13, 14, 15, 16]
        again = HL.device_counts(cohorts[13], ix, seeded=True)
        assert (again.stats.seed_k, again.stats.n_index_builds) == (13, 0) and again.rows == fresh[13].rows
        assert ix.info()["cached_k"] == [11, 12, 13, 14, 15, 16]
