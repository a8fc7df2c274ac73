"""CPU: the host side of the OTU clustering (rambl_amd/otu.py) against the plain restatement of
tests/pair_lib.py: the restatement itself against a literal double loop, the named edges' property checks, the clustering
rules on hand-made pair lists, the identity parser, the matrix sum, the file formats and the command's early errors.  No
device is touched."""
import os
import random

import pytest

import pair_lib as P
from rambl_amd import otu


def test_restatement_equals_the_literal_double_loop():
    rng = random.Random(8164)
    for _ in range(400):
        a = bytes(rng.choice(b"ACGTacgtNn-") for _ in range(rng.randrange(1, 14)))
        b = P.mutate(rng, a, rng.randrange(0, 4)) if rng.random() < 0.5 else bytes(rng.choice(b"ACGTN") for _ in range(rng.randrange(1, 14)))
        assert P.edit_distance(a, b) == P.literal_distance(a, b) == P.edit_distance(b, a), (a, b)
    a, b = P.rand_seq(rng, 70), P.rand_seq(rng, 90)
    assert P.edit_distance(a, b) == P.literal_distance(a, b)
    assert P.edit_distance(b"N", b"N") == 1 and P.edit_distance(b"a", b"A") == 0 and P.edit_distance(b"ACGT", b"AGT") == 1


def test_distance_edges_reach_their_edges():
    edges = P.distance_edges(tuple(otu.widths()))
    for e in edges:
        e.check()
    lengths = {len(g) for e in edges for g in e.genes}
    assert set(P.edge_lengths(otu.widths())) <= lengths and {1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048} <= lengths
    for w in otu.widths():
        assert {64 * w - 1, 64 * w} <= lengths and (64 * w + 1 in lengths or 64 * w == P.MAX_LEN)
    as_pattern = {len(e.genes[a]) for e in edges for a, _ in e.pairs}
    as_text = {len(e.genes[b]) for e in edges for _, b in e.pairs}
    assert set(P.edge_lengths(otu.widths())) <= as_pattern & as_text          # every length both ways


def test_list_edges_reach_their_edges():
    for e in P.list_edges():
        e.check()


def test_bound_is_integer_division_of_the_longer_length():
    assert P.bound(1500, 1400, 3, 100) == 45 and P.bound(1499, 1, 3, 100) == 44 and P.bound(199, 199, 5, 1000) == 0 and P.bound(200, 1, 5, 1000) == 1
    assert P.bound(2048, 7, 0, 1) == 0 and P.bound(2048, 2048, 1, 1) == 2048


def test_identity_text_becomes_an_exact_rate():
    assert otu.diff_from_identity("97") == (3, 100) and otu.diff_from_identity("99.5") == (5, 1000) and otu.diff_from_identity("100") == (0, 1)
    assert otu.diff_from_identity("99.9") == (1, 1000) and otu.diff_from_identity(" 98.70 ") == (13, 1000) and otu.diff_from_identity("0.1") == (999, 1000)
    assert otu.diff_from_identity("50") == (50, 100) and otu.diff_from_identity("295/3") == (1, 60) and otu.diff_from_identity("99.99999") == (1, 10000000)
    # 99.5 % is 5 / 1000 = 1 / 200: the same bound for every length, whichever way the rate is written
    assert all(P.bound(n, n, 5, 1000) == P.bound(n, n, 1, 200) for n in range(1, 2049))
    for bad in ("0", "-3", "100.0001", "101", "abc", "", "1/0", "99." + "9" * 12):
        with pytest.raises(ValueError):
            otu.diff_from_identity(bad)


def test_a_tie_goes_to_the_centroid_made_first():
    names, lengths, weights = ["c2", "c1", "g"], [100, 100, 100], [5, 9, 1]
    pairs = [(0, 2, 2), (1, 2, 2)]                              # c1 is heavier, so it is made first; g is as near to both
    for f in (otu.greedy_otus, P.greedy_otus):
        assert f(names, lengths, weights, pairs) == [("c2", "c2", 0), ("c1", "c1", 0), ("g", "c1", 2)]
    assert otu.greedy_otus(names, lengths, [9, 5, 1], pairs)[2] == ("g", "c2", 2)
    assert otu.greedy_otus(names, lengths, [9, 5, 1], pairs[::-1])[2] == ("g", "c2", 2)          # whatever the order of the list


def test_the_best_ratio_is_chosen_in_integers():
    # 1 / 3 against 333333333333333333 / 10^18: equal as doubles, the second smaller as rationals
    assert 1 / 3 == 333333333333333333 / 10 ** 18
    names, lengths, weights = ["first", "second", "g"], [3, 10 ** 18, 2], [3, 2, 1]
    pairs = [(0, 2, 1), (1, 2, 333333333333333333)]
    for f in (otu.greedy_otus, P.greedy_otus):
        assert f(names, lengths, weights, pairs)[2] == ("g", "second", 333333333333333333)
    # and with gene-sized numbers: 29 / 1450 = 0.02 against 30 / 1499
    names, lengths, weights = ["x", "y", "g"], [1450, 1499, 1400], [3, 2, 1]
    for f in (otu.greedy_otus, P.greedy_otus):
        assert f(names, lengths, weights, [(0, 2, 29), (1, 2, 30)])[2] == ("g", "x", 29)
        assert f(names, lengths, weights, [(0, 2, 30), (1, 2, 30)])[2] == ("g", "y", 30)          # 30 / 1499 < 30 / 1450


def test_the_walk_goes_by_weight_then_length_then_name():
    names, lengths = ["b", "a", "long", "heavy"], [10, 10, 12, 5]
    assert otu.walk_order(names, lengths, [0, 0, 0, 0]) == [2, 1, 0, 3] == P.walk_order(names, lengths, [0, 0, 0, 0])
    assert otu.walk_order(names, lengths, [0, 0, 0, 0.5]) == [3, 2, 1, 0]
    pairs = [(0, 1, 0), (0, 2, 1), (1, 2, 1), (2, 3, 1)]
    assert otu.greedy_otus(names, lengths, [0, 0, 0, 0], pairs) == [("b", "long", 1), ("a", "long", 1), ("long", "long", 0), ("heavy", "long", 1)]
    # a member is no centroid: heavy joins long's only through long, not through a member
    assert otu.greedy_otus(names, lengths, [0, 0, 0, 0], [(0, 1, 0), (0, 3, 1)]) == [("b", "a", 0), ("a", "a", 0), ("long", "long", 0), ("heavy", "heavy", 0)]
    assert otu.greedy_otus(names, lengths, [0, 0, 0, 7], pairs) == [("b", "a", 0), ("a", "a", 0), ("long", "heavy", 1), ("heavy", "heavy", 0)]


def test_dereplication_is_the_rate_zero():
    genes = P.list_edges()[8].genes
    assert P.list_edges()[8].name.startswith("dereplication")
    names = ["g%d" % k for k in range(len(genes))]
    lengths = [len(g) for g in genes]
    mapping = otu.greedy_otus(names, lengths, [0] * len(genes), P.pairs_within(genes, 0, 1))
    assert mapping == P.greedy_otus(names, lengths, [0] * len(genes), P.pairs_within(genes, 0, 1))
    assert [c for _, c, _ in mapping] == ["g0", "g0", "g2", "g3", "g0", "g5"]          # the copies with an N stay apart


def test_greedy_otus_equals_the_restatement_on_random_inputs():
    rng = random.Random(8165)
    for _ in range(200):
        n = rng.randrange(1, 14)
        names = ["n%d" % k for k in rng.sample(range(100), n)]
        lengths = [rng.randrange(90, 100) for _ in range(n)]
        weights = [rng.choice([0, 0, 1, 2.5, 7]) for _ in range(n)]
        pairs = [(a, b, rng.randrange(0, 4)) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.4]
        rng.shuffle(pairs)
        got = otu.greedy_otus(names, lengths, weights, pairs)
        assert got == P.greedy_otus(names, lengths, weights, pairs)
        assert [g for g, _, _ in got] == names and all(dict((g, c) for g, c, _ in got)[c] == c for _, c, _ in got)


MATRIX = "gene\ts1\ts2\nga\t0.0625\t2.0\ngb\t0.25\t0.0\ngc\t10.125\t0.5\ngd\t0.0\t0.0\n"


def test_the_matrix_sum_and_the_weights():
    mapping = [("gb", "gb", 0), ("ga", "gb", 1), ("gd", "gd", 0), ("gc", "gb", 2)]
    want = "gene\ts1\ts2\ngb\t10.438\t2.5\ngd\t0.0\t0.0\n"          # 0.25 + 0.0625 + 10.125 = 10.4375, a half in binary too: away from zero
    assert otu.otu_matrix_text(MATRIX, mapping) == want == P.otu_matrix_text(MATRIX, mapping)
    assert otu.matrix_weights(MATRIX, ["gd", "ga"]) == [0.0, 2.0625] == P.row_weights(MATRIX, ["gd", "ga"])
    assert otu.otu_matrix_text("gene\n" + "x\ny\n", [("x", "y", 1), ("y", "y", 0)]) == "gene\ny\n"          # a matrix of no sample
    for bad in ("", "name\ts1\nga\t1\n", "gene\ts1\nga\t1\t2\n", "gene\ts1\nga\t1\nga\t2\n", "gene\ts1\nga\tx\n"):
        with pytest.raises(ValueError):
            otu.parse_matrix(bad)


def test_the_file_formats():
    names, seqs = ["g1", "g0", "g2"], ["ACGTACGTAC", "ACGTACGTACG", "TTTT"]
    lengths, weights = [10, 11, 4], [0, 0, 0]
    mapping = otu.greedy_otus(names, lengths, weights, [(0, 1, 1)])
    assert mapping == [("g1", "g0", 1), ("g0", "g0", 0), ("g2", "g2", 0)]
    assert otu.otu_map_text(names, lengths, mapping) == "gene\totu\tedit_distance\tgene_length\totu_length\ng1\tg0\t1\t10\t11\ng0\tg0\t0\t11\t11\ng2\tg2\t0\t4\t4\n"
    assert otu.otus_fasta_text(names, seqs, lengths, weights, mapping) == ">g0\nACGTACGTACG\n>g2\nTTTT\n"
    assert otu.pairs_text(names, [(0, 1, 1)]) == "a\tb\tedit_distance\ng1\tg0\t1\n"
    assert otu.otu_map_text(names, lengths, mapping) == P.otu_map_text(names, lengths, mapping)
    assert otu.otus_fasta_text(names, seqs, lengths, weights, mapping) == P.otus_fasta_text(names, seqs, lengths, weights, mapping)
    assert otu.pairs_text(names, [(0, 1, 1)]) == P.pairs_text(names, [(0, 1, 1)])
    assert len(otu.STAT_NAMES) == 7


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_early_errors_of_rambl_otu(tmp_path, capsys, monkeypatch):
    """Each ends with a message and exit status 2 before any device work: the library is never asked for a pair."""
    from rambl_amd import capi, cohort
    monkeypatch.setattr(capi, "lib", lambda: pytest.fail("the device was reached"))
    good = _write(tmp_path / "g.fa", ">ga\nACGT\n>gb x\nACGA\n")
    twice = _write(tmp_path / "twice.fa", ">ga\nACGT\n>ga\nACGA\n")
    long_ = _write(tmp_path / "long.fa", ">ga\n" + "A" * 2049 + "\n")
    empty = _write(tmp_path / "empty.fa", ">ga\n>gb\nAC\n")
    none = _write(tmp_path / "none.fa", "")
    other = _write(tmp_path / "other.tsv", "gene\ts1\nga\t1.0\ngz\t2.0\n")
    fewer = _write(tmp_path / "fewer.tsv", "gene\ts1\nga\t1.0\n")
    cases = [([twice], "gene name ga is given twice"), ([good, "--matrix", other], "are not those of"), ([good, "--matrix", fewer], "are not those of"),
             ([good, "--id", "0"], "outside (0, 100]"), ([good, "--id", "100.5"], "outside (0, 100]"), ([good, "--id", "x"], "is not a number"),
             ([long_], "has 2049 bases"), ([empty], "has 0 bases"), ([none], "holds no gene"), ([good, "--matrix", str(tmp_path / "absent.tsv")], "absent.tsv")]
    for argv, message in cases:
        with pytest.raises(SystemExit) as e:
            otu.main(argv + ["-o", str(tmp_path / "out")])
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    assert not os.path.exists(tmp_path / "out")
    listing = _write(tmp_path / "samples.txt", _write(tmp_path / "s.sam", "@SQ\tSN:ga\tLN:4\n") + "\n")
    for argv, message in (([twice, listing, "--otu", "97"], "given twice"), ([good, listing, "--otu", "0"], "outside (0, 100]")):
        with pytest.raises(SystemExit) as e:
            cohort.main(argv + ["-o", str(tmp_path / "out")])
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    assert not os.path.exists(tmp_path / "out")
