"""CPU: every named case of tests/update_edge_lib.py reaches the edge of the level update it is named for, by its input alone;
the reference agrees with a second, literal per-cell restatement of the rules on the three smallest cases; the set of names
is complete; the constants the library restates are the kernels'."""
import os
import re

import numpy as np
import pytest

import update_edge_lib as UL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", UL.NAMES)
def test_case_reaches_its_edge(name):
    case = UL.case(name)
    again = UL.case(name)
    for k, v in case.__dict__.items():                                    # deterministic
        w = again.__dict__[k]
        if isinstance(v, np.ndarray):
            assert v.shape == w.shape and v.dtype == w.dtype and UL.same_bits(v.astype(np.float64), w.astype(np.float64)).size == 0, k
        else:
            assert v == w, k
    UL.reaches(case)
    ref = UL.reference(case)
    assert ref["ll"].shape == (UL.MAXS, case.n_reads) and ref["isnew"].shape == (case.Rn,)
    assert ref["isnew"].tolist() == [int(f) for f in UL.fresh_of(case)]
    assert ref["has"].tolist() == [1 if (case.has[r] or r in case.ent_rid) else 0 for r in range(case.n_reads)]
    # rows nobody names come back as they were, and so do the cells of a destination from 2 * ceil(n / 2) on
    before = UL.prior_matrix(case)
    named = set(case.slot) | {d for _, d in case.copies}
    for row in range(UL.MAXS):
        if row not in named:
            assert UL.same_bits(ref["ll"][row], before[row]).size == 0 and not ref["free"][row].any()
    n = min(case.copy_n, case.n_reads)
    assert ref["free"].sum() == (len(case.copies) if n % 2 == 1 and n < case.n_reads else 0)
    for src, dst in case.copies:
        assert UL.same_bits(ref["ll"][dst, :n], before[src, :n]).size == 0 or dst in case.slot


def test_the_names_are_complete():
    assert sorted(UL.NAMES) == sorted(UL.EDGES) and len(set(UL.NAMES)) == len(UL.NAMES)
    for family, least in (("plain_", 23), ("sym_", 7), ("item_", 3), ("dup_", 5), ("cop", 14), ("grid_", 9)):
        assert sum(1 for n in UL.NAMES if n.startswith(family)) >= least, family
    assert max(UL.case(n).S * UL.case(n).Rn for n in UL.NAMES) < 5000          # small: a fraction of a second each
    assert {UL.case(n).K for n in UL.NAMES if n.startswith("sym_")} == {6, 8, 16}
    assert {(UL.case(n).K, UL.case(n).code_N) for n in UL.NAMES if n.startswith("sym_") and UL.case(n).code_N >= 0} == {(8, 6), (8, 7), (16, 6), (16, 15)}
    assert sorted(len(UL.case(n).copies) for n in UL.NAMES if n.startswith("copies_")) == [0, 1, 2, 5]
    assert sorted(UL.case("dup_S%d" % s).S for s in (1, 2, 64, 128)) == [1, 2, 64, 128]


def smallest_three():
    return sorted(UL.NAMES, key=lambda n: (UL.case(n).S * UL.case(n).Rn, n))[:3]


@pytest.mark.parametrize("name", ["item_mix", "dup_multi", "copy_parent_child", "copyn_odd", "sym_K8_N7"] + smallest_three())
def test_reference_against_the_literal_restatement(name):
    """Cell by cell, every row of the matrix: the three smallest cases, and one of each family whose rules the smallest do not meet."""
    case = UL.case(name)
    ref = UL.reference(case)
    literal = np.zeros_like(ref["ll"])
    free = np.zeros(literal.shape, dtype=bool)
    for row in range(UL.MAXS):
        for col in range(case.n_reads):
            v = UL.literal_cell(case, row, col)
            free[row, col] = v is None
            literal[row, col] = 0.0 if v is None else v
    assert np.array_equal(free, ref["free"])
    assert UL.same_bits(ref["ll"], literal, free).size == 0


def test_the_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_level.hip")).read()
    dev = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_device.hpp")).read()
    assert re.search(r"LDS_TOTAL = 160 \* 1024 - 256;", src) and re.search(r"LDS_SMALL = 18 \* 1024;", src) and "LDS_BIG = LDS_TOTAL - LDS_SMALL" in src
    assert "return LDS_BIG / (int)sizeof(double)" in src and UL.TABLE_CAP == 18144 and UL.CAP_S == 70
    assert "constexpr int MAXS = 128;" in dev and "constexpr int KMAX = 16;" in dev
    assert "LV_COPIES_DONE = 1, LV_ITEMS_DONE = 2, LV_HAS_DONE = 4" in src and "LV_TICKED = 64" in src
    assert "constexpr int U = 16;" in src
    assert [UL.partition(t) for t in (1, 256, 257, 512, 513, 3013)] == [(1, 256), (1, 256), (1, 512), (1, 512), (2, 512), (6, 512)]
    # no trailing workgroup is empty below the cap of 1 024 workgroups
    assert all((UL.partition(t)[0] - 1) * UL.partition(t)[1] < t for t in list(range(1, 6000)) + [1024 * 512])
    b, per = UL.partition(1024 * 512 + 1)
    assert (b - 1) * per >= 1024 * 512 + 1


def test_expected_done_follows_the_launcher():
    plain, dup, multi, copies = (UL.case(n) for n in ("plain_S17_R33", "dup_S2", "item_mix", "copies_2"))
    assert UL.expected_done(plain, True) == UL.LV_ITEMS | UL.LV_HAS | UL.LV_TICKED and UL.expected_done(plain, False) == 0
    assert UL.expected_done(dup, True) == 0 and UL.expected_done(multi, True) == 0
    assert UL.expected_done(copies, True) == UL.LV_COPIES | UL.LV_ITEMS | UL.LV_HAS | UL.LV_TICKED and UL.expected_done(copies, False) == 0
