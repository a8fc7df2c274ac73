"""CPU: every named edge case of tests/depth_edge_lib.py is deterministic, valid input for sc_depth_scan_runs and reaches its
edge on the plain numpy reference alone; that reference and the oracle's merge_mean (oracle/depth_oracle.py, over a depth
list built by a plain loop over the runs) are two independent restatements that have to agree on every case."""
import os
import sys

import numpy as np
import pytest

import depth_edge_lib as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import depth_oracle  # noqa: E402  (test infrastructure)


def oracle_intervals(ref_len, run_ref, run_start, run_end, max_gap, refs=None):
    """merge_mean per reference, from depths counted cell by cell: [(ref, start, end, sum, n)]"""
    ref_len = [int(x) for x in ref_len]
    refs = list(range(len(ref_len))) if refs is None else list(refs)
    depth = {r: [0] * (ref_len[r] + 2) for r in refs}
    for r, s, e in zip(np.asarray(run_ref).tolist(), np.asarray(run_start).tolist(), np.asarray(run_end).tolist()):
        if r in depth:
            d = depth[r]
            for p in range(s, e + 1):
                d[p] += 1
    return [(r, s, e, sm, n) for r in refs for s, e, sm, n in depth_oracle.merge_mean(depth[r], ref_len[r], max_gap)]


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_case_reaches_its_edge(name):
    case = D.CASES[name]()
    assert case.name == name and case.key() == D.CASES[name]().key()                     # a function of its name alone
    assert 0 <= case.max_gap <= D.MAX_GAP_LIMIT and np.all(case.ref_len >= 0)
    assert case.run_ref.size == case.run_start.size == case.run_end.size
    if case.n_runs:
        assert np.all((case.run_ref >= 0) & (case.run_ref < case.n_refs))
        assert np.all((1 <= case.run_start) & (case.run_start <= case.run_end) & (case.run_end <= case.ref_len[case.run_ref]))
    out = case.reference()
    assert out == sorted(out) and len(set((r, s) for r, s, _, _, _ in out)) == len(out)
    case.check(out)


@pytest.mark.parametrize("name", sorted(set(D.CASES) - set(D.LARGE)))
def test_reference_equals_oracle(name):
    case = D.CASES[name]()
    assert case.reference() == oracle_intervals(case.ref_len, case.run_ref, case.run_start, case.run_end, case.max_gap)


@pytest.mark.parametrize("max_gap", [10, 0])
def test_reference_equals_oracle_on_a_thousandth_of_deep_sum(max_gap):
    full = D.deep_sum(max_gap)
    case = D.deep_sum(max_gap, n_runs=1100)
    assert full.n_runs - 1 == 1000 * (case.n_runs - 1) and full.max_gap == case.max_gap and np.array_equal(full.ref_len, case.ref_len)
    for a, b in ((full.run_ref, case.run_ref), (full.run_start, case.run_start), (full.run_end, case.run_end)):
        assert np.all(a[:-1] == a[0]) and np.all(b[:-1] == a[0]) and a[-1] == b[-1]      # the same runs, a thousand times as often
    out = case.reference()
    case.check(out)
    assert out == oracle_intervals(case.ref_len, case.run_ref, case.run_start, case.run_end, max_gap)
    assert [(r, s, e, 1000 * sm if r == 0 else sm, n) for r, s, e, sm, n in out] == full.reference()


@pytest.mark.parametrize("max_gap", [10, 0])
def test_reference_equals_oracle_on_a_fraction_of_deep_lane_sum(max_gap):
    full = D.deep_lane_sum(max_gap)
    case = D.deep_lane_sum(max_gap, n_runs=11)                                          # a 100 000th of the runs
    assert full.n_runs == 100_000 * case.n_runs and np.array_equal(full.ref_len, case.ref_len)
    for a, b in ((full.run_ref, case.run_ref), (full.run_start, case.run_start), (full.run_end, case.run_end)):
        assert np.all(a == a[0]) and np.all(b == a[0])
    out = case.reference()
    case.check(out)
    assert out == oracle_intervals(case.ref_len, case.run_ref, case.run_start, case.run_end, max_gap)
    assert [(r, s, e, 100_000 * sm, n) for r, s, e, sm, n in out] == full.reference()


def test_reference_equals_oracle_on_both_ends_of_grid_stride():
    case = D.CASES["grid_stride"]()
    n = case.n_refs
    keep = list(range(2000)) + list(range(n - 600, n))
    assert n - 600 < D.MAX_WAVES < n
    exp = oracle_intervals(case.ref_len, case.run_ref, case.run_start, case.run_end, case.max_gap, refs=keep)
    kept = set(keep)
    assert [row for row in case.reference() if row[0] in kept] == exp and len(exp) > 4000


def test_restated_geometry_matches_the_source():
    src = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_depth.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "straincall_hip.h")).read()
    assert "constexpr int TILE = %d;" % D.TILE in src and "constexpr int FIXED = %d;" % D.FIXED in src
    assert "std::min((n_refs + 3) / 4, 1 << 16)" in src and D.MAX_WAVES == 4 << 16
    assert "if (max_gap >= 3)" in src and "for (int q0 = 0; q0 < tl; q0 += 64 * PPL)" in src
    assert "#define SC_DEPTH_MAX_GAP ((1 << 30) - (1 << 24))" in hdr and D.MAX_GAP_LIMIT == (1 << 30) - (1 << 24)


def test_reference_on_a_hand_computed_case():
    # the 40-base gene of test_stage1.py as runs.  Sample 1: 3-7, 20-22 and 25-26 (23-24 deleted); sample 2: 6-9, 38-40.
    # Covered: 3-9 (depths 1 1 1 2 2 1 1), 20-22, 25-26, 38-40; gaps 10-19 (10 bases), 23-24, 27-37 (11 bases).
    runs = [(3, 7), (20, 22), (25, 26), (6, 9), (38, 40)]
    ref, start, end = [0] * len(runs), [s for s, _ in runs], [e for _, e in runs]
    assert D.reference([40], ref, start, end, 10) == [(0, 3, 26, 9 + 5, 7 + 5), (0, 38, 40, 3, 3)]
    assert D.reference([40], ref, start, end, 9) == [(0, 3, 9, 9, 7), (0, 20, 26, 5, 5), (0, 38, 40, 3, 3)]
    assert D.reference([40], ref, start, end, 0) == [(0, 3, 9, 9, 7), (0, 20, 22, 3, 3), (0, 25, 26, 2, 2), (0, 38, 40, 3, 3)]
    # the same gene behind an empty reference and in front of one that a run fills to its last cell
    assert D.reference([0, 40, 3], [1] * len(runs) + [2], start + [1], end + [3], 10) == \
        [(1, 3, 26, 14, 12), (1, 38, 40, 3, 3), (2, 1, 3, 3, 3)]
    assert D.reference([5], [], [], [], 10) == [] and D.reference([], [], [], [], 10) == []
    assert D.ppl(3) == 4 and D.ppl(2) == 1 and D.step(10) == 256 and D.step(0) == 64
