"""CPU: every named case of tests/hard_edge_lib.py reaches the edge of the hard update it is named for, by the reference
alone; the long-double reference agrees with decimal arithmetic at 50 digits and with the literal, un-shifted quotient; it
leaves the matrix of update_edge_lib.reference alone where no slot has a mate; the slot arithmetic of the grid's loops; the
constants the library restates are the kernels'."""
import decimal
import os

import numpy as np
import pytest

import hard_edge_lib as HL
import update_edge_lib as UL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not HL.LONG_DOUBLE_OK, reason="np.longdouble is not the 80-bit extended format")
L = np.longdouble
U_LONG = 2.0 ** -64                                           # unit roundoff of the long double


@pytest.fixture(scope="module")
def refs():
    cases = {n: HL.case(n) for n in HL.NAMES}
    return cases, {n: HL.reference(c) for n, c in cases.items()}


@pytest.mark.parametrize("name", HL.NAMES)
def test_case_reaches_its_edge(name, refs):
    cases, all_refs = refs
    c, ref = cases[name], all_refs[name]
    again = HL.reference(HL.case(name))                                   # deterministic
    for k in ("ll", "resp", "abund", "subst"):
        assert HL.same_bits(np.asarray(ref[k], dtype=np.float64), np.asarray(again[k], dtype=np.float64)).size == 0, k
    HL.reaches(c, ref)
    assert ref["resp"].shape == (c.S, c.Q) and ref["qrid"].shape == (c.Q,) and ref["subst"].shape == (c.S, c.K, c.K)
    # every finite column adds up to one, every abundance to Q
    p = ref["resp"]
    fin = ~np.isnan(p.astype(np.float64)).any(axis=0)
    assert np.all(np.abs(p[:, fin].sum(axis=0) - 1) < 1e-17 * c.S)
    if fin.all():
        assert abs(float(ref["abund"].sum()) - c.Q) < 1e-12 * c.Q
    # the rows nobody names keep the bits the update left
    named = set(c.u.slot)
    for row in range(HL.MAXS):
        if row not in named:
            assert HL.same_bits(ref["ll"][row], ref["before"]["ll"][row]).size == 0


def test_the_names_are_complete():
    assert sorted(HL.NAMES) == sorted(HL.EDGES) and len(set(HL.NAMES)) == len(HL.NAMES)
    cases = {n: HL.case(n) for n in HL.NAMES}
    shapes = {(c.S, c.Q) for c in cases.values() if c.K == 6}
    assert {(s, q) for s in (1, 3) for q in (1, 63, 64, 65, 128, 129)} <= shapes
    assert {(3, q) for q in (255, 256, 257, 511, 512, 513)} | {(5, 103)} <= shapes
    assert {(s, 70) for s in (2, 16, 17, 32, 33, 64, 65, 127, 128)} <= shapes
    assert {c.K for c in cases.values()} >= {6, 7, 8, 16} and cases["cap_K16"].S == HL.CAP_S
    assert all(c.u.e0 > 0 for c in cases.values())
    assert sum(1 for c in cases.values() if c.u.has_dups) >= 1 and sum(1 for c in cases.values() if c.u.any_multi) >= 2
    assert sorted(HL.EXACT) == sorted(n for n, c in cases.items() if c.exact) and len(HL.EXACT) == 10
    assert max(c.S * c.Q for c in cases.values()) <= 128 * 70                       # small: a fraction of a second each


def small_cases():
    return [n for n in HL.NAMES if HL.case(n).Q <= 70 and HL.case(n).S <= 5]


def _dec(v):
    return decimal.Decimal(float(v))


def _dec_long(v):
    """A long double as a Decimal: its 64-bit mantissa in two exact halves."""
    m, e = np.frexp(v)
    m = np.ldexp(m, 64)
    hi = np.floor(np.ldexp(m, -32))
    lo = m - np.ldexp(hi, 32)
    return (decimal.Decimal(int(float(hi))) * 2 ** 32 + decimal.Decimal(int(float(lo)))) * decimal.Decimal(2) ** (int(e) - 64)


@pytest.mark.parametrize("name", small_cases())
def test_reference_against_decimal_and_the_literal_quotient(name, refs):
    """The same bound as the device's, with the long double's unit roundoff in place of fp64's: x_s is the exact sum of the
    doubles in decimal, rounded twice in long double."""
    cases, all_refs = refs
    c, ref = cases[name], all_refs[name]
    tol = HL.tolerances(c, ref, u=U_LONG)
    _, qrid, quid, _ = HL.slots(c)
    rows = ref["ll"][c.u.slot]
    checked = literal = 0
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        ctx.Emin, ctx.Emax = -10 ** 6, 10 ** 6
        for q in range(c.Q):
            col = [[c.logpri[s], rows[s, qrid[q]]] + ([rows[s, quid[q]]] if quid[q] >= 0 else []) for s in range(c.S)]
            flat = [v for terms in col for v in terms]
            if any(np.isnan(v) for v in flat) or all(any(np.isneginf(v) for v in terms) for terms in col):
                assert np.isnan(ref["resp"][:, q].astype(np.float64)).all(), (name, q)
                continue
            ex = [decimal.Decimal(0) if any(np.isneginf(v) for v in terms) else sum(_dec(v) for v in terms).exp() for terms in col]
            z = sum(ex)
            for s in range(c.S):
                want, got = ex[s] / z, ref["resp"][s, q]
                if want == 0:
                    assert got == 0, (name, s, q)
                    continue
                err = abs(_dec_long(got) - want) / want
                assert float(err) <= tol["resp_rel"][q], (name, s, q, float(err), tol["resp_rel"][q])
                checked += 1
            # the literal quotient, where no exp(x) leaves the long double's normal range
            x = ref["x"][:, q]
            if float(x[np.isfinite(x)].min()) > -11000.0:              # (no NaN here, and a finite x: see above)
                e = np.exp(x)
                lit = e / e.sum()
                assert np.all(np.abs(lit - ref["resp"][:, q]) <= ref["resp"][:, q] * tol["resp_rel"][q] * 2), (name, q)
                literal += 1
    if not np.isnan(ref["resp"].astype(np.float64)).all():
        assert checked > 0 and literal > 0


def test_reference_leaves_the_update_alone_without_mates(refs):
    cases, all_refs = refs
    without = [n for n in HL.NAMES if (all_refs[n]["quid"] < 0).all()]
    assert len(without) >= 10
    for n in without:
        up = UL.reference(cases[n].u)
        assert HL.same_bits(all_refs[n]["ll"], up["ll"]).size == 0 and np.array_equal(all_refs[n]["has"], up["has"]) and np.array_equal(all_refs[n]["isnew"], up["isnew"]), n
    with_mates = [n for n in HL.NAMES if all_refs[n]["zeroed"]]
    assert len(with_mates) >= 20
    for n in with_mates:                                                       # and with them, only the zeroed cells and marks differ
        up, ref, c = UL.reference(cases[n].u), all_refs[n], cases[n]
        diff = {tuple(ix) for ix in HL.same_bits(ref["ll"], up["ll"]).tolist()}
        assert diff <= {(row, v) for row in c.u.slot for v in ref["zeroed"]}, n
        assert set(np.flatnonzero(ref["has"] != up["has"]).tolist()) == set(ref["zeroed"]), n


def test_slot_arithmetic_of_the_grid_and_the_lanes():
    src = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_level.hip")).read()
    assert "const int gq = grid_blocks(h.Q, 256, 2048);" in src and "for (int q = lane; q < Q; q += 64)" in src
    assert "LV_HARD_DONE = 8, LV_SLOTS_DONE = 16" in src and "__launch_bounds__(512) void k_level(" in src
    assert [HL.grid_blocks(q, 256, 2048) for q in (1, 255, 256, 257, 511, 512, 513, 2048 * 256, 2048 * 256 + 1)] == [1, 1, 1, 2, 2, 2, 3, 2048, 2048]
    # (workgroup, thread, trip) of the last slot: the first thread of a new workgroup at 257 and 513, the second trip of
    # the grid's first thread at 2048 * 256 + 1
    assert HL.last_slot(256) == (0, 255, 0) and HL.last_slot(257) == (1, 0, 0) and HL.last_slot(513) == (2, 0, 0)
    assert HL.last_slot(2048 * 256) == (2047, 255, 0) and HL.last_slot(2048 * 256 + 1) == (0, 0, 1)
    # inside the level's workgroup of 512 threads: slot 512 is thread 0's second
    assert HL.last_slot(512, per=512, most=1) == (0, 511, 0) and HL.last_slot(513, per=512, most=1) == (0, 0, 1)
    # strain_sums: lane (Q - 1) % 64 takes the last slot, in round ceil(Q / 64)
    assert [HL.wave_additions(q) for q in (1, 63, 64, 65, 128, 129)] == [7, 7, 7, 8, 8, 9]
    assert HL.TABLE_CAP == 18144 and HL.CAP_S == 70


def test_array_reference_of_the_grid_trip_is_the_reference(refs):
    """big_reference, which the case of 2048 * 256 + 1 slots is checked with, gives the bits of reference() and the bounds of
    tolerances() on the plain cases with finite columns; the big case has its last slot on the grid's second trip."""
    cases, all_refs = refs
    for n in ("blocks_Q257", "blocks_Q513", "odd_S5_Q103", "mates_absent", "strains_S17_Q70"):
        big, ref = HL.big_reference(cases[n]), all_refs[n]
        assert np.array_equal(big["resp"], ref["resp"]) and np.array_equal(big["resp_rel"], HL.tolerances(cases[n], ref)["resp_rel"]), n
        assert HL.same_bits(big["ll"], ref["ll"]).size == 0 and np.array_equal(big["has"], ref["has"]) and big["zeroed"] == ref["zeroed"], n
    c = HL.big_case()
    big = HL.big_reference(c)
    assert c.Q == HL.BIG_Q == 2048 * 256 + 1 and c.S == 2 and not c.u.has_dups and not c.u.any_multi
    assert HL.last_slot(c.Q) == (0, 0, 1) and big["quid"][-1] in big["zeroed"] and set(big["qcode"].tolist()) == set(range(6))
    r = big["resp"].astype(np.float64)                                       # the check passes the reference's own numbers
    sub = np.zeros((2, 6, 6))
    for s in range(2):
        for b in range(6):
            sub[s, c.u.strain_labels[s][0], b] = r[s, big["qcode"] == b].sum()
    assert max(HL.big_check(c, big, r, np.array([r[0].sum(), r[1].sum()]), sub)) < 0.1          # (pairwise sums: within the wavefront's bound)


def test_expected_done_follows_the_launcher():
    plain, dup, multi, copies = (HL.case(n) for n in ("lanes_S3_Q65", "dups", "multi", "mates_absent"))
    full = HL.LV_HARD | HL.LV_SLOTS | HL.LV_ITEMS | HL.LV_HAS | HL.LV_TICKED
    assert full == 94 and HL.expected_done(plain, True) == full and HL.expected_done(plain, False) == 0
    assert HL.expected_done(dup, True) == 0 and HL.expected_done(multi, True) == 0 and HL.expected_done(multi, False) == 0
    assert HL.expected_done(copies, True) == full | HL.LV_COPIES and HL.expected_done(copies, False) == 0
