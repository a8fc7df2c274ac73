"""GPU: the named edge cases of tests/align_edge_lib.py through k_bl_score<1..8> / k_bl_trace<1..8>
(rambl_amd/csrc/sc_profile.hip, sc_profile_dp.hpp) against the plain restatement (tests/native/blast_hits_check.cpp): every field of every hit,
exactly, E through profile.format_evalue.  `every_bucket` launches every instantiation, `score_stride` and `trace_stride`
the second trip of the two grid-stride loops."""
import math
import random

import pytest

import align_edge_lib as E
import profile_lib as PL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


def _device(case, segs=None, genes=None, **kw):
    from rambl_amd import capi
    segs = case.segs if segs is None else segs
    genes = case.genes if genes is None else genes
    return capi.profile_hits([g.encode() for g in genes], [s.encode() for s in segs], *case.thresholds(), **kw)


def _possible(case, seg):
    """A segment that can pass -e with every base matched (the others are in no bucket and cost no cell)."""
    n = sum(len(g) for g in case.genes)
    return case.ka_k * len(seg) * n * math.exp(-case.ka_lambda * len(seg)) <= case.max_evalue


@pytest.mark.parametrize("name", sorted(E.PROFILE_CASES))
def test_case_equals_restatement(name, hits_check):
    case = E.PROFILE_CASES[name]()
    rows = E.run_profile_check(case, hits_check)
    exp, res = PL.compare_hits(hits_check, case.genes, case.segs, *case.thresholds(), name=name, exp=rows)
    assert res.stats.n_traced >= len(exp)
    cells = 2 * sum(len(s) for s in case.segs if _possible(case, s)) * sum(len(g) for g in case.genes)
    if name in ("every_bucket", "impossible_segments"):                  # lengths at which the segment's E is far from -e
        assert res.stats.score_cells == cells and res.stats.score_cells < 2 * sum(map(len, case.segs)) * sum(map(len, case.genes))
    elif name != "short_genes":
        assert res.stats.score_cells == cells == 2 * sum(map(len, case.segs)) * sum(map(len, case.genes))


def test_impossible_segments_alone_launch_nothing():
    case = E.pr_impossible_segments()
    res = _device(case, segs=case.alone)
    assert len(res) == 0 and res.stats.n_tiles == 0 and res.stats.n_candidates == 0 and res.stats.score_cells == 0


def test_a_hit_exactly_on_the_evalue_threshold(hits_check):
    case, hit, e = E.evalue_edge(hits_check)
    for t, there in ((e, True), (math.nextafter(e, 0.0), False)):
        exp, _ = PL.compare_hits(hits_check, case.genes, case.segs, 0.0, t, name="evalue_edge")
        assert (PL.as_csv_fields(hit) in exp) == there


def test_candidate_overflow_retries():
    """cap = 3 gives 1 030 candidate records; the parity data set passes more tiles than that at -I 0 -e 10, so the first
    answer is SC_ERR_CAPACITY with the number of passing tiles and the binding calls again."""
    from rambl_amd import capi
    genes, segs = PL.parity_dataset()
    g, s = [x.encode() for x in genes], [x.encode() for x in segs]
    a = capi.profile_hits(g, s, 0.0, 10.0)
    b = capi.profile_hits(g, s, 0.0, 10.0, cap=3)
    assert b.stats.n_candidates > 2 * 3 + 1024 and b.stats.n_candidates == a.stats.n_candidates
    assert len(PL.device_hits(a)) > 1000 and PL.device_hits(a) == PL.device_hits(b)


def test_segment_order_does_not_matter():
    case = E.pr_every_bucket()
    first = PL.device_hits(_device(case))
    order = list(range(len(case.segs)))
    random.Random(3).shuffle(order)
    again = PL.device_hits(_device(case, segs=[case.segs[k] for k in order]))
    back = sorted(((order[h[0]],) + h[1:] for h in again), key=lambda h: h[:2])
    assert len(first) > 200 and back == first


def test_buckets_do_not_disturb_each_other():
    case = E.pr_every_bucket()
    groups = [case.segs, E.pr_top_score().segs, E.pr_identity_edge().segs, E.pr_ties().segs]
    alone, at = [], 0
    for g in groups:
        alone += [(h[0] + at,) + h[1:] for h in PL.device_hits(_device(case, segs=g))]
        at += len(g)
    together = PL.device_hits(_device(case, segs=[s for g in groups for s in g]))
    # E = K m n e^(-lambda S) does not depend on the other segments: equal hits, field for field
    assert len(alone) > 200 and together == alone


def test_the_longest_segment_and_gene_are_accepted(hits_check):
    rng = random.Random(8)
    genes = [PL.L.rand_seq(rng, E.MAX_SEED)]
    segs = [genes[0][4000:4512], PL.L.revcomp(genes[0][E.MAX_SEED - 512:])]
    exp, _ = PL.compare_hits(hits_check, genes, segs, name="512 on 8192")
    assert [h[3] for h in exp] == [1024, 1024] and exp[1][8] == E.MAX_SEED
