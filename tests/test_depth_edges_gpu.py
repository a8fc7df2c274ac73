"""GPU: the named edge cases of tests/depth_edge_lib.py through k_depth_fused<4> / k_depth_fused<1> (rambl_amd/csrc/sc_depth.hip)
against the plain numpy reference: every interval with its depth sum and covered positions, exactly (all five columns are
integers).  Every case runs with cap == its interval count; the capacity contract, the max_gap limit and the CIGAR walk of
sc_depth_scan have tests of their own."""
import os
import sys

import numpy as np
import pytest

import depth_edge_lib as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import depth_oracle  # noqa: E402  (test infrastructure)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_named_case(name):
    case = D.CASES[name]()
    exp = case.reference_arrays()
    case.check(list(zip(*(a.tolist() for a in exp))))
    got = D.scan_case(case, cap=len(exp[0]))                                   # cap == n
    print("%s: kernel_ms %.3f, %d runs, %d intervals" % (name, got.stats.kernel_ms, case.n_runs, len(exp[0])))
    assert got.rc == D.SC_OK and got.n == len(exp[0])
    assert D.first_difference(tuple(a[:got.n] for a in got.arrays), exp) is None
    assert got.stats.cells == int(case.ref_len.sum()) and got.stats.runs == case.n_runs
    assert (got.stats.kernel_ms > 0) == (case.n_refs > 0)


def test_capacity(tmp_path):
    from rambl_amd import stage1
    case = D.many_starts(0)
    exp = case.reference_arrays()
    n = len(exp[0])
    assert n > 5000                                                            # all but FIXED per reference in the shared list
    for cap in (n - 1, 1, 0):                                                  # one short; far below the shared list's count
        got = D.scan_case(case, cap=cap)
        assert (got.rc, got.n) == (D.SC_ERR_CAPACITY, n)
        assert all(np.all(a == -1) for a in got.arrays)                        # nothing is written when the call fails
    got = D.scan_case(case, cap=n)
    assert got.rc == D.SC_OK and D.first_difference(tuple(a[:got.n] for a in got.arrays), exp) is None
    # the same pattern as one-base reads on one reference: more intervals than depth_intervals' first capacity (1 024 for one
    # reference), so that its regrow loop runs
    ln = 3 * D.TILE
    records = [(0, "g", p, "1M") for p in range(1, ln + 1, 2)]
    path, fai = str(tmp_path / "s.sam"), str(tmp_path / "genes.fai")
    open(path, "w").write(D.sam_text([("g", ln)], records))
    open(fai, "w").write("g\t%d\t0\t60\t61\n" % ln)
    exp = depth_oracle.stage1([D.by_name(records)], [("g", ln)], max_gap=0)
    assert len(exp) == ln // 2 > 1024
    got, st = stage1.depth_intervals([path], fai, max_gap=0)
    assert got == [("g", s, e, sm, k) for _, s, e, sm, k in exp] and st["runs"] == len(records)


def test_extreme_max_gap():
    """The contract: max_gap up to SC_DEPTH_MAX_GAP = 2^30 - 2^24 works (everything of a reference merges), above it both
    entry points refuse with SC_ERR_ARG before anything is launched; so does a reference longer than 2^30 bases."""
    import ctypes as C
    from rambl_amd import capi, stage1
    case = D.gap_seams(10)
    covered = sorted(set(case.run_ref.tolist()))
    assert covered == [0, 1, 2]
    for g in (10 ** 9, D.MAX_GAP_LIMIT):
        exp = D.reference_arrays(case.ref_len, case.run_ref, case.run_start, case.run_end, g)
        assert exp[0].tolist() == covered                                      # one interval per covered reference
        got = D.scan_case(case, cap=len(covered), max_gap=g)
        assert got.rc == D.SC_OK and D.first_difference(tuple(a[:got.n] for a in got.arrays), exp) is None
    for g in (D.MAX_GAP_LIMIT + 1, 2 ** 31 - 1):
        got = D.scan_case(case, cap=16, max_gap=g)
        assert (got.rc, got.n, got.stats.kernel_ms) == (D.SC_ERR_ARG, -7, -1.0)   # neither *n_intervals nor the stats are touched
        assert all(np.all(a == -1) for a in got.arrays)
    got = D.scan_runs([5, 2 ** 30 + 1], [0], [1], [5], 10, cap=16)
    assert (got.rc, got.n, got.stats.kernel_ms) == (D.SC_ERR_ARG, -7, -1.0)
    # sc_depth_scan: the same limit, with no alignment file at all
    lib = capi.lib()
    names = (C.c_char_p * 1)(b"g")
    lens = (C.c_int * 1)(100)
    handles = (C.c_void_p * 1)()
    out = [(C.c_int * 4)() for _ in range(4)]
    sm = (C.c_long * 4)()
    for g, rc in ((D.MAX_GAP_LIMIT, D.SC_OK), (D.MAX_GAP_LIMIT + 1, D.SC_ERR_ARG), (2 ** 31 - 1, D.SC_ERR_ARG)):
        n = C.c_int(-7)
        st = stage1.DepthStats()
        st.kernel_ms = -1.0
        assert lib.sc_depth_scan(0, handles, 0, names, lens, 1, g, out[0], out[1], out[2], sm, out[3], 4, C.byref(n), C.byref(st)) == rc
        if rc == D.SC_OK:
            assert n.value == 0 and st.kernel_ms > 0
        else:
            assert (n.value, st.kernel_ms) == (-7, -1.0)


def test_cigar_walk_edges(tmp_path):
    """sc_depth_scan's CIGAR walk from SAM text against the oracle: reads at and past the reference end, operations that
    consume no reference, the flags samtools depth drops, a gene in two files, references on one side only."""
    from rambl_amd import stage1
    fai_refs = [("7", 100), ("9", 2100), ("12", 50), ("lonely", 40), ("filtered", 60)]
    counted_a = [
        (0, "7", 5, "10M"),
        (0, "7", 96, "10M"),              # an M operation straddling the reference end: 96-100 count
        (16, "7", 30, "3I4M2P4M"),        # a leading I and a P consume no reference: 30-37
        (0, "7", 50, "5H3S6M5H"),         # H and S: 50-55
        (0x800, "7", 70, "8M"),           # supplementary: counts
        (0, "9", 2040, "20M"),            # across the tile seam of a reference of two tiles
        (0, "9", 2090, "5M3D5M4N9M"),     # 2090-2094; 2098-2100 of the second M; the third lies past the end behind the N
    ]
    dropped_a = [
        (0, "7", 101, "10M"),             # POS beyond ref_len
        (0, "7", 60, "4M5000N6M"),        # its second M lies wholly past the reference end (the first, 60-63, counts)
        (0, "7", 20, "*"),                # no CIGAR
        (0x4, "7", 1, "100M"), (0x100, "7", 1, "100M"), (0x200, "7", 1, "100M"), (0x400, "7", 1, "100M"),      # each bit of 0x704
        (0x400, "filtered", 1, "60M"), (0x4, "filtered", 10, "5M"),                                           # a reference whose reads are all dropped
        (0, "stranger", 1, "30M"),        # a SAM reference that the .fai does not have
    ]
    file_b = [(0, "7", 8, "10M"), (0x800 | 16, "12", 50, "1M"), (0x100, "12", 1, "50M")]      # the same gene in a second file
    sam_refs = fai_refs[:3] + [("filtered", 60), ("stranger", 30)]                             # "lonely" is in no file
    texts = [D.sam_text(sam_refs, sorted(counted_a + dropped_a, key=lambda r: (r[1], r[2]))), D.sam_text(sam_refs, file_b)]
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("s%d.sam" % i)))
        open(paths[-1], "w").write(t)
    fai = str(tmp_path / "genes.fai")
    open(fai, "w").write("".join("%s\t%d\t0\t60\t61\n" % r for r in fai_refs))
    order = sorted(fai_refs, key=lambda r: (stage1._numeric_key(r[0]), r[0]))
    files = [D.by_name(counted_a + dropped_a), D.by_name(file_b)]
    exp = depth_oracle.stage1(files, order, max_gap=10)
    named = [(order[ri][0], s, e, sm, n) for ri, s, e, sm, n in exp]
    assert {r[0] for r in named} == {"7", "9", "12"} and ("7", 96, 100, 5, 5) in named and ("12", 50, 50, 1, 1) in named
    assert ("9", 2040, 2059, 20, 20) in named and ("9", 2090, 2100, 8, 8) in named
    # the dropped reads would have changed the result: each of them in turn with its flag cleared
    for k, rec in enumerate(dropped_a):
        if rec[0] & 0x704:
            unflagged = dropped_a[:k] + [(0,) + rec[1:]] + dropped_a[k + 1:]
            assert depth_oracle.stage1([D.by_name(counted_a + unflagged), files[1]], order, max_gap=10) != exp, rec
    without_supp = [r for r in counted_a if not r[0] & 0x800]
    assert depth_oracle.stage1([D.by_name(without_supp + dropped_a), files[1]], order, max_gap=10) != exp
    # the reads that hang over the end add nothing behind it, and 4M5000N6M adds its first M only
    assert sum(sm for name, _, _, sm, _ in named if name == "7") == 10 + 5 + 8 + 6 + 8 + 4 + 10
    got, st = stage1.depth_intervals(paths, fai, max_gap=10)
    assert got == named
    assert st["runs"] == 12 and st["cells"] == sum(l for _, l in fai_refs)
