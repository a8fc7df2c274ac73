"""CPU: the counts mode of the gene profile on the host -- the two forms of the counting rule
(tests/count_lib.py) against each other and against the reference counter's recorded output, the six-digit E-value of the
library against Python's own, the read grouping, the summing of triples, and every named case's property."""
import json
import math
import os
from fractions import Fraction

import pytest

import count_lib as CL
import profile_lib as PL
from rambl_amd.capi import profile_counts, profile_evalue6  # noqa: F401  (the feature: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "profile_counts")


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@pytest.mark.parametrize("name", CL.DATASETS + tuple(sorted(CL.NAMED)))
def test_lazy_rule_equals_full_rule_and_the_case_reaches_its_edge(name, hits_check):
    full, triples = CL.check_rules(CL.case(name), hits_check)
    assert full and sum(f for _, f in full) == sum(Fraction(m * n, s) for (_, m, s), n in triples.items())


@pytest.mark.parametrize("case", sorted(json.load(open(os.path.join(GOLD, "meta.json")))["cases"]))
def test_both_rules_reproduce_the_reference_counter(case):
    from rambl_amd import profile
    t = json.load(open(os.path.join(GOLD, "meta.json")))["cases"][case]
    rows = profile.parse_hits_csv(open(os.path.join(GOLD, case + ".csv")).read())
    want = open(os.path.join(GOLD, case + ".raw"), "rb").read()
    assert profile.format_raw(CL.full_rule(rows, float(t["-I"]), float(t["-E"]))).encode() == want
    lazy, triples, looked, _ = CL.lazy_rule(rows, float(t["-I"]), float(t["-E"]))
    assert profile.format_raw(lazy).encode() == want and 0 < looked <= len(rows)
    # the triples are the counts
    names = sorted({g for g, _, _ in triples})
    assert profile.counts_from_triples([(names.index(g), m, s, n) for (g, m, s), n in triples.items()], names) == lazy


@pytest.mark.parametrize("gene_bases", (600, 150000, 123456789))
def test_evalue6_is_the_six_digit_text_read_back(gene_bases):
    """Every (L, S2) with L in 1..512 and S2 up to 2 L: the library's E6 is float("%.6g" % E), E by the contract's expression."""
    bad = []
    for L in range(1, 513):
        for s2 in range(1, 2 * L + 1):
            e = 0.46 * float(L) * float(gene_bases) * math.exp(-1.28 * (0.5 * float(s2)))
            if profile_evalue6(L, gene_bases, s2) != float("%.6g" % e):
                bad.append((L, s2, e))
    assert not bad, bad[:5]
    assert profile_evalue6(150, 150000, 62, 1.0, 0.5) == float("%.6g" % (0.5 * 150.0 * 150000.0 * math.exp(-1.0 * (0.5 * 62.0))))


def test_read_index():
    from rambl_amd import profile
    ids = ["a/1", "a/2", "a.1", "b.2", "b", "c/3", "", "x", "/1", "/2", "a", "x/1", ".2"]
    reads, n = profile.read_index(ids)
    # a/1 a/2 a.1 and the bare a are one read of four segments; b.2 joins b; c/3 keeps its suffix; "" and "x" are their own
    # reads; "/1", "/2" and ".2" have two characters and lose both: they are the read "" as well
    assert reads == [0, 0, 0, 1, 1, 2, 3, 4, 3, 3, 0, 4, 3] and n == 5
    assert len({(r, CL.read_of(i)) for r, i in zip(reads, ids)}) == n
    assert profile.read_index([]) == ([], 0)


def test_counts_from_triples():
    from rambl_amd import profile
    names = ["Zeta", "alpha", "beta"]
    triples = [(0, 1, 1, 5), (0, 1, 3, 2), (1, 1, 3, 2), (2, 1, 3, 2), (1, 2, 1, 7), (2, 3, 2049, 1)]
    want = [("Zeta", 5 + Fraction(2, 3)), ("alpha", Fraction(2, 3) + 14), ("beta", Fraction(2, 3) + Fraction(3, 2049))]
    assert profile.counts_from_triples(triples, names) == want
    assert profile.counts_from_triples([], names) == []
    assert profile.counts_from_triples([(1, 1, 1, 1), (0, 1, 1, 1)], ["b", "B"]) == [("B", 1), ("b", 1)]        # byte order


def test_conserved_case_saves_four_fifths(hits_check):
    case = CL.case("conserved")
    rows, all_rows = CL.reference(case, hits_check)
    _, _, looked, _ = CL.lazy_rule(all_rows)
    assert 5 * looked <= len(all_rows) and looked >= len(case.segs)


def test_counts_and_keep_hits_exclude_each_other(capsys):
    from rambl_amd import profile
    with pytest.raises(SystemExit) as e:
        profile.main(["genes.fa", "sample.sam", "s", "--counts", "--keep-hits"])
    assert e.value.code == 2 and "no hit list" in capsys.readouterr().err
