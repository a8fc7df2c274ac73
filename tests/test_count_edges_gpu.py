"""GPU: the named edge cases of tests/count_edge_lib.py through the counts mode of the gene profile (sc_profile_counts: the
k_cnt_* kernels, reduce_triples and merge_rows in rambl_amd/csrc/sc_profile_counts.hpp): exact Fractions and
equal triples against the counting rule on the plain restatement's hits, unseeded and seeded, with the statistics that show
the device walked the seam; then every case one read per stretch, as the second sample of a cohort on one index, and with its
segments in reverse order.  Beside the cases: the capacity of the caller's arrays over many stretches, and the samples beside
the triples at the ends of their range."""
import ctypes as C

import numpy as np
import pytest

import cohort_lib as HL
import count_edge_lib as EL
import count_lib as CL
import profile_lib as PL
from rambl_amd.capi import ProfileIndex, profile_counts  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("seeded", (False, True), ids=("unseeded", "seeded"))
CASES = pytest.mark.parametrize("name", sorted(EL.EDGES))
_ALONE = {}


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


def alone(name, hits_check, seeded=False):
    """count_lib.compare_device on the case alone, once per (case, mode)."""
    if (name, seeded) not in _ALONE:
        _ALONE[(name, seeded)] = CL.compare_device(EL.case(name), hits_check, seeded)
    return _ALONE[(name, seeded)]


def read_lens(case):
    from rambl_amd import profile
    seg_read, n = profile.read_index(case.ids)
    out = [[] for _ in range(n)]
    for s, r in zip(case.segs, seg_read):
        out[r].append(len(s))
    return out


@MODES
@CASES
def test_edge_case(name, seeded, hits_check):
    case = EL.case(name)
    st = alone(name, hits_check, seeded).stats
    _, triples, looked, failed = CL.lazy_rule(CL.reference(case, hits_check)[1], *case.thresholds[:2])
    # a read visits its groups in order up to the first with a passing pair: the rounds are the most groups a read visits (no
    # case here reaches the at-once tail), the pairs traced those of the visited groups -- lazy_rule's `looked` -- and the
    # hits those of them that pass -I.  (Seeded, a pair that fails -I may share no k-mer and never be scored: fewer pairs
    # traced, never more; a pair that passes shares one.)
    rounds = passing = 0
    for read, gs in CL.groups_of(CL.reference(case, hits_check)[1], *case.thresholds[:2]).items():
        ok = [sum(1 for r in group if CL._pct(r) >= case.thresholds[0]) for group in gs]
        visited = next((k + 1 for k, n in enumerate(ok) if n), len(gs))
        assert visited == min(failed[read] + 1, len(gs))
        rounds, passing = max(rounds, visited), passing + ok[visited - 1]
    assert st.n_rounds == rounds <= CL.COUNT_ROUNDS and st.n_stretches == 1
    assert st.n_traced <= looked if seeded else st.n_traced == looked
    assert st.n_hits == passing
    if name.startswith("seam_"):
        n1, n2 = EL.seam_sizes(name)
        assert st.n_rounds == (2 if n1 else 1) and looked == n1 + n2 + 1 and st.n_reads_counted == 2
    if name == "all_buckets":
        assert st.n_rounds == 2 and looked == 4 * len(EL.BUCKET_LENGTHS) and st.n_reads_counted == 3 * len(EL.BUCKET_LENGTHS)
    if name.startswith("mates_"):
        assert st.n_reads_counted == 1 + 3                                  # the mates; the variant and two plain reads
    if name.startswith("strand_tie_"):
        assert st.n_reads_counted == sum(triples.values()) == (2 if name.endswith("clean") else 1)
    if name == "five_segments":
        assert st.n_reads_counted == 1
    if name == "rank_edges":
        assert st.n_reads_counted == 3


@MODES
@CASES
def test_one_read_per_stretch(name, seeded, hits_check):
    case = EL.case(name)
    whole = alone(name, hits_check, seeded)
    tiny = CL.device_counts(case, seeded, cand_room=1)
    plan = HL.plan_stretches(read_lens(case), len(case.genes), case.n_bases(), 1, case.thresholds)
    assert tiny.triples == whole.triples and tiny.stats.n_stretches == len(plan) == sum(1 for lens in read_lens(case) if any(HL.can_pass(n, case.n_bases(), case.thresholds) for n in lens))
    assert tiny.stats.n_traced == whole.stats.n_traced and tiny.stats.n_reads_counted == whole.stats.n_reads_counted


def plain_sample(case):
    """A few clean pieces of the case's genes, a read each."""
    genes = case.genes[:3]
    return HL.Sample(["r%d" % k for k in range(len(genes))], [g[10:70] for g in genes])


@MODES
@CASES
def test_rides_along_as_second_sample(name, seeded, hits_check):
    case = EL.case(name)
    whole = alone(name, hits_check, seeded)
    cohort = HL.Cohort("edge_ride_" + name, case.genes, case.names, [plain_sample(case), HL.Sample(case.ids, case.segs)], None, case.thresholds)
    res = HL.device_counts(cohort, seeded=seeded)
    HL.check_rows(res)
    assert res.by_sample(1) == whole.triples
    assert res.by_sample(0) == HL.alone(cohort, 0, seeded).triples and len(res.by_sample(0)) > 0
    assert res.stats.n_reads_counted == whole.stats.n_reads_counted + HL.alone(cohort, 0, seeded).stats.n_reads_counted


@MODES
@CASES
def test_reads_in_reverse_order(name, seeded, hits_check):
    from rambl_amd import profile
    case = EL.case(name)
    whole = alone(name, hits_check, seeded)
    order = list(range(len(case.segs)))[::-1]
    seg_read, _ = profile.read_index([case.ids[k] for k in order])
    res = profile_counts([g.encode() for g in case.genes], [case.segs[k].encode() for k in order], seg_read, *case.thresholds, seeded=seeded)
    assert seg_read[0] == 0 and res.triples == whole.triples
    assert res.stats.n_traced == whole.stats.n_traced and res.stats.n_rounds == whole.stats.n_rounds


# ---- capacity over stretches

SENTINEL = -7
_PARITY = {}


def _parity_whole():
    if not _PARITY:
        _PARITY["whole"] = CL.device_counts(CL.case("parity"))
    return _PARITY["whole"]


def _raw_counts(case, cap, cand_room, room):
    """sc_profile_counts itself with arrays of `room` elements, all SENTINEL -> (rc, *n_out, the arrays as rows, message)."""
    from rambl_amd import capi, profile
    gl = np.array([0] + [len(g) for g in case.genes], dtype=np.int64).cumsum()
    sl = np.array([0] + [len(s) for s in case.segs], dtype=np.int64).cumsum()
    reads = np.array(profile.read_index(case.ids)[0], dtype=np.int32)
    out = [np.full(room, SENTINEL, dtype=np.int32) for _ in range(3)] + [np.full(room, SENTINEL, dtype=np.int64)]
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    n = C.c_long()
    rc = capi.lib().sc_profile_counts(0, "".join(case.genes).encode(), gl.ctypes.data_as(lp), len(case.genes), "".join(case.segs).encode(),
                                      sl.ctypes.data_as(lp), len(case.segs), reads.ctypes.data_as(ip), int(reads.max()) + 1, *case.thresholds,
                                      0, cand_room, out[0].ctypes.data_as(ip), out[1].ctypes.data_as(ip), out[2].ctypes.data_as(ip),
                                      out[3].ctypes.data_as(lp), cap, C.byref(n), None)
    return rc, n.value, [tuple(int(a[k]) for a in out) for k in range(room)], capi.lib().sc_profile_error().decode()


@pytest.mark.parametrize("which", ("0", "1", "n-1", "n"))
def test_capacity_over_stretches(which):
    """One read per stretch, so that a row's reads come from many stretches: the first `cap` rows are the whole call's, their
    numbers of reads included, and nothing is written behind them."""
    case, whole = CL.case("parity"), _parity_whole()
    n = len(whole)
    cap = {"0": 0, "1": 1, "n-1": n - 1, "n": n}[which]
    assert n > 10 and max(t[3] for t in whole.triples) > 3 and whole.stats.n_stretches == 1
    rc, n_out, rows, msg = _raw_counts(case, cap, 1, cap + 3)
    assert n_out == n and rows[:cap] == whole.triples[:cap]
    assert rows[cap:] == [(SENTINEL,) * 4] * 3                           # the element at index cap and those behind it
    if cap < n:
        assert rc == -5 and "%d triples, room for %d" % (n, cap) in msg
    else:
        assert rc == 0


# ---- samples beside the triples

def test_samples_at_the_ends_of_their_range():
    """65 536 samples, reads in samples 0, 32 768 and 65 535: the sort by sample takes 17 bits; the rows' samples ascend and each
    sample's rows are the sample's alone."""
    case = CL.case("mates")
    genes, segs = [g.encode() for g in case.genes], [s.encode() for s in case.segs]
    seg_read = [0, 0, 1, 1, 2, 2, 3, 3, 3, 4]
    read_sample = [0, 0, 32768, 32768, 65535]
    assert EL.bits_of(HL.MAX_SAMPLES) == 17 and len(seg_read) == len(segs)
    with ProfileIndex(genes) as ix:
        res = ix.counts(segs, seg_read, read_sample, HL.MAX_SAMPLES)
        once = ix.counts(segs, seg_read, read_sample, HL.MAX_SAMPLES, cand_room=1)
    HL.check_rows(res)
    assert once.rows == res.rows and once.stats.n_stretches == 5 and res.stats.n_samples == HL.MAX_SAMPLES
    assert sorted({r[0] for r in res.rows}) == [0, 32768, 65535]
    for s in (0, 32768, 65535):
        mine = [k for k, r in enumerate(seg_read) if read_sample[r] == s]
        first = seg_read[mine[0]]
        one = profile_counts(genes, [segs[k] for k in mine], [seg_read[k] - first for k in mine])
        assert res.by_sample(s) == one.triples and len(one) > 0
