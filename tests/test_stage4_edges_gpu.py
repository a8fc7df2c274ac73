"""GPU: the named edge cases of tests/align_edge_lib.py through k_sw_score<1..8> / k_sw_trace<1..8>
(rambl_amd/csrc/sc_align.hip) against the plain restatement (tests/native/sw_check.cpp): every field of every read, exactly.
`every_bucket` launches every instantiation, `score_stride` and `trace_stride` the second trip of the two grid-stride
loops."""
import random

import pytest

import align_edge_lib as E
import stage4_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sw_check(tmp_path_factory):
    return L.build_sw_check(tmp_path_factory.mktemp("sw_check"))


def _align(seeds, reads):
    from rambl_amd import capi
    return capi.align_reads([s.encode() for s in seeds], [r.encode() for r, _ in reads], [q.encode() for _, q in reads])


@pytest.mark.parametrize("name", sorted(E.STAGE4_CASES))
def test_case_equals_restatement(name, sw_check):
    case = E.STAGE4_CASES[name]()
    exp = L.run_sw_check(sw_check, case.seeds, case.reads)
    case.check(exp)
    got = _align(case.seeds, case.reads)
    L.compare_rows(case.reads, exp, L.device_rows(got), name)
    assert got.stats.n_traced == sum(e[2] >= 0 for e in exp)
    assert got.stats.score_cells == 2 * sum(len(r) for r, _ in case.reads) * sum(len(s) for s in case.seeds)
    # block b of a window is swept from the window's first column, and stage 4 counts every block of every window
    cells = 0
    for (r, _), e in zip(case.reads, exp):
        if e[2] >= 0:
            w = E.stage4_window(len(r), e[0], e[4], e[5])
            cells += (len(r) - E.clips(e[5])[1]) * sum(min(w["ncol"], E.TB_COLS * (b + 1)) for b in range(w["blocks"]))
    assert got.stats.trace_cells == cells


def test_read_order_does_not_matter():
    """The two atomicMax of a tile must not depend on which tile arrives first."""
    case = E.s4_every_bucket()
    first = L.device_rows(_align(case.seeds, case.reads))
    order = list(range(len(case.reads)))
    random.Random(3).shuffle(order)
    again = L.device_rows(_align(case.seeds, [case.reads[k] for k in order]))
    back = [None] * len(order)
    for at, k in enumerate(order):
        back[k] = again[at]
    L.compare_rows(case.reads, first, back, "every_bucket permuted")
    again = L.device_rows(_align(case.seeds[::-1], case.reads))                        # ... nor the seed order, up to the index
    n = len(case.seeds)
    flipped = [e[:2] + ((n - 1 - e[2]) if e[2] >= 0 else -1,) + e[3:] for e in again]
    L.compare_rows(case.reads, first, flipped, "every_bucket, seeds reversed")


def test_buckets_do_not_disturb_each_other():
    """Four cases in one call against one seed set, the seeds of all four: every read as in its own call."""
    cases = [E.s4_every_bucket(), E.s4_gbar_rows(), E.s4_top_score(), E.s4_most_operations()]
    seeds = [s for c in cases for s in c.seeds]
    groups = [c.reads for c in cases]
    alone = [L.device_rows(_align(seeds, g)) for g in groups]
    assert all(any(e[2] >= 0 for e in rows) for rows in alone)                         # every group has reads that align
    reads = [r for g in groups for r in g]
    together = L.device_rows(_align(seeds, reads))
    L.compare_rows(reads, [e for rows in alone for e in rows], together, "four cases in one call")
    # every_bucket alone has 23 lengths of 63 bases and more, four reads each, all copied from a seed with a few edits
    assert sum(e[2] >= 0 for rows in alone for e in rows) >= 92 and {E.bucket(len(r)) for r, _ in reads} == set(range(1, 9))


def test_the_longest_read_and_seed_are_accepted(sw_check):
    rng = random.Random(8)
    seeds = [L.rand_seq(rng, E.MAX_SEED)]
    reads = [(seeds[0][4000:4512], "*"), (L.revcomp(seeds[0][E.MAX_SEED - 512:]), "*")]
    exp = L.run_sw_check(sw_check, seeds, reads)
    assert [e[0] for e in exp] == [1024, 1024] and exp[1][4] + 511 == E.MAX_SEED
    L.compare_rows(reads, exp, L.device_rows(_align(seeds, reads)), "512 on 8192")
