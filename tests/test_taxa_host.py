"""CPU: the host side of the genus assignment (rambl_amd/taxa.py, sc_taxa_draw, profile.py's --copy-correct) against the plain
restatement in tests/taxa_lib.py and against values worked out by hand.  No device is touched."""
import os

import pytest

import taxa_lib as T


def test_every_named_case_reaches_its_edge():
    assert T.check_cases_on_the_cpu()


def test_exact_table_by_hand_and_its_error_bound():
    import numpy as np
    # N = 1: P_w = 0.25 for a word nobody holds, and with M = 0 the cell is log2(0.25) * 1024 = -2048 exactly, half a unit from
    # either half-integer (M = 1: -3072); the word one sequence holds has P_w = 0.75: log2(0.75) * 1024 = -424.99839926...
    # with m = 0, M = 0, and with n = m = M = 1 p = (1 + 0.75) / 2 = 0.875, log2(0.875) * 1024 = -197.26855981...
    n, m, M = np.array([0, 1]), np.array([[0, 0], [0, 1]]), np.array([0, 1])
    q, d = T.table_exact(n, m, M, 1)
    assert q.tolist() == [[-2048, -3072], [-425, -197]] and d[0, 0] == 0.5 and d[0, 1] == 0.5
    assert abs(d[1, 1] - (197.5 - 197.26855981301338)) < 1e-12 and abs(d[1, 0] - (0.5 - (425 - 424.99839926153606))) < 1e-12
    assert (T.table(n, m, M, 1) == q).all()
    # the bound: 4.9e-13 from the roundings of p, the rest grows with |x|; at the contract's largest cell it is under 3e-11
    assert 4.9e-13 < T.table_error_bound(0.0) < 5.0e-13 and 2.8e-11 < T.table_error_bound(50 * 1024) < 3e-11
    # the near-half-integer tuples keep their recorded distances, each 100 E away and nearer than 1e-7
    dist = [float(mo.dist[T.word_of("ACGTTGCA"), 0]) for mo in T.near_half_case()]
    for got, want in zip(dist, (2.7462e-8, 9.7189e-9, 1.1418e-9)):
        assert abs(got / want - 1.0) < 1e-3 and got > 100 * T.table_error_bound(900.0)
    # a cell inside the bound is refused: the cap is asserted from the reference alone
    near = T.table_exact
    try:
        T.table_exact = lambda *a: (np.array([[-692]]), np.array([[1e-13]]))
        with pytest.raises(AssertionError):
            T.exact_checked(n, m, M, 1)
    finally:
        T.table_exact = near


def test_draw_at_the_limits_equals_the_restatement():
    """The last draw of the last trial, and seed ^ key at 0, at all ones and one below: the 64-bit sum wraps."""
    from rambl_amd import capi
    for seed, key in ((0, 0), (T.MASK, 0), (0, T.MASK), (T.MASK, T.MASK), (T.MASK, 1), (977, 977)):
        for t, j in ((0, 0), (1, 0), (1023, 1022), (1023, 0), (512, 5)):
            for W in (1, 2, 48, 8185):
                got = capi.taxa_draw(seed, key, t, j, W)
                assert got == T.draw(seed, key, t, j, W) and 0 <= got < W
    assert 1023 * 65536 + 1022 + 1 < 2 ** 32


def test_draw_equals_the_restatement():
    from rambl_amd import capi
    for W in (1, 7, 8, 40, 8185):
        for t in (0, 99):
            for j in (0, T.n_draws(W) - 1):
                for seed, key in ((0, 0), (12345, T.fnv1a64(b"gene_7")), (T.MASK, T.MASK - 5)):
                    got = capi.taxa_draw(seed, key, t, j, W)
                    assert got == T.draw(seed, key, t, j, W) and 0 <= got < W
    assert capi.taxa_draw(1, 2, 0, 0, 0) == -1
    assert len({capi.taxa_draw(9, 9, t, j, 8185) for t in range(4) for j in range(50)}) > 150     # the draws are spread


def test_fnv_key():
    from rambl_amd import taxa
    assert taxa.fnv1a64(b"") == 0xCBF29CE484222325 and taxa.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    assert taxa.fnv1a64(b"gene_7") == T.fnv1a64(b"gene_7")


def test_both_lineage_forms():
    from rambl_amd import taxa
    six = ("Bacteria", "Firmicutes", "Clostridia", "Clostridiales", "Clostridiaceae", "Clostridium sensu stricto")
    gg = "k__Bacteria; p__Firmicutes; c__Clostridia; o__Clostridiales; f__Clostridiaceae; g__Clostridium sensu stricto; s__x"
    assert taxa.parse_lineage(gg) == six
    assert taxa.parse_lineage(gg.rsplit(";", 1)[0]) == six                   # without s__
    assert taxa.parse_lineage(";".join(six)) == six and taxa.parse_lineage("; ".join(six) + ";") == six
    assert taxa.parse_lineage(gg.replace("g__Clostridium sensu stricto", "g__")) is None
    assert taxa.parse_lineage(gg.replace("c__Clostridia;", "c__;")) is None  # a rank above the genus is empty
    assert taxa.parse_lineage("Bacteria;Firmicutes;;Clostridiales;Clostridiaceae;Clostridium") is None
    assert taxa.parse_lineage("Bacteria;Firmicutes") is None


def test_training_set_and_its_drops(tmp_path):
    from rambl_amd import samio, taxa
    train_fa, train_tax, _, genera, mo, _, _ = T.cli_case()
    fa, tx = tmp_path / "t.fa", tmp_path / "t.tax"
    fa.write_text(train_fa)
    tx.write_text(train_tax)
    f = samio.Fasta(str(fa))
    seqs, genus, got_genera, drops = taxa.training_set(f.order, [f.seqs[n].encode() for n in f.order], taxa.read_taxonomy(str(tx)))
    assert drops == {"unlabelled": 1, "incomplete": 1, "no_sequence": 1}
    assert [s.decode() for s in seqs] == mo.seqs and genus == mo.genus and got_genera == genera
    # equal genus names under different parents are different genera
    assert len({g[5] for g in genera}) < len(genera) == 6


def test_fixrank_round_trip_through_the_scripts_parsers():
    from rambl_amd import taxa
    genera = [("Bacteria", "P", "C", "O", "F", 'Genus "quoted" name'), ("Bacteria", "P", "C", "O", "F 2", "Clostridium sensu stricto")]
    results = [(0, [0] * 60 + [1] * 40, 50), (1, [1] * 100, 9), (-1, [-1] * 100, 0)]
    names = ["g0", "g1", "blank"]
    text = "".join(taxa.fixrank_line(n, genera[b], taxa.confidences(b, w, genera)) if W else taxa.fixrank_line(n) for n, (b, w, W) in zip(names, results))
    assert text == T.fixrank_text(names, results, genera)
    assert text.splitlines()[0] == 'g0\t\tBacteria\tdomain\t1.00\tP\tphylum\t1.00\tC\tclass\t1.00\tO\torder\t1.00\tF\tfamily\t0.60\tGenus "quoted" name\tgenus\t0.60'
    assert text.splitlines()[2] == "blank\t"
    # the gene profile's parser: prefixed names at or above the threshold; the quotes go, the space stays
    gl = T.ref_parse_gene_lineage(text, 0.6)
    assert gl["g0"] == ["0__Bacteria", "1__P", "2__C", "3__O", "4__F", "5__Genus quoted name"]
    assert gl["g1"][-1] == "5__Clostridium sensu stricto" and gl["blank"] == []
    assert T.ref_parse_gene_lineage(text, 0.61)["g0"] == ["0__Bacteria", "1__P", "2__C", "3__O"]
    # the taxon profile's parser
    tg, tl = T.ref_parse_taxa(text, "genus", 0.6)
    assert tg == {"Genus quoted name": ["g0"], "Clostridium sensu stricto": ["g1"]}
    assert tl["Clostridium sensu stricto"]["family"] == "F 2"
    # the product's parser reads what both read
    mine = dict(taxa.parse_fixrank(text))
    assert mine["blank"] == [] and [e[0] for e in mine["g0"]] == [t.split("__", 1)[1] for t in gl["g0"]]
    assert mine["g0"][4] == ("F", "family", 0.6)


COPY_TSV = "rank\tname\tmean\tn\nphylum\tP\t4.0\t3\nfamily\tF\t2.5\t9\nfamily\tF\t9.0\t1\ngenus\tNowhere\t7.0\t1\n"


def _copy_numbers(tmp_path):
    from rambl_amd import taxa
    p = tmp_path / "copy.tsv"
    p.write_text(COPY_TSV)
    return taxa.load_copy_numbers(str(p))


def test_copy_number_rule_by_hand(tmp_path):
    from rambl_amd import taxa
    cn = _copy_numbers(tmp_path)
    assert cn == {"P": 4.0, "F": 2.5, "Nowhere": 7.0}                        # the first duplicate name wins
    ent = [("Bacteria", "domain", 1.0), ("P", "phylum", 0.9), ("C", "class", 0.8), ("O", "order", 0.7), ("F", "family", 0.6), ("G", "genus", 0.3)]
    assert taxa.gene_copy_number(ent, cn, 0.6) == 2.5                        # the deepest rank with a row; 0.6 >= 0.6 passes
    assert taxa.gene_copy_number(ent, cn, 0.6000001) == 4.0                  # family now fails: the phylum's row
    assert taxa.gene_copy_number(ent, cn, 0.95) == 1.0                       # only the domain passes, and it has no row
    assert taxa.gene_copy_number([], cn, 0.6) == 1.0
    from fractions import Fraction
    text = T.fixrank_text(["a", "b"], [(0, [0] * 100, 5), (-1, [], 0)], [("Bacteria", "P", "C", "O", "F", "G")])
    counts = [("a", Fraction(10, 3)), ("b", Fraction(7)), ("c", Fraction(1, 2))]
    got = taxa.correct_counts(counts, taxa.parse_fixrank(text), cn, 0.6)
    assert got == [("a", float(Fraction(10, 3)) / 2.5), ("b", 7.0), ("c", 0.5)]
    assert dict(got) == T.ref_copy_correct(dict(counts), T.ref_parse_gene_lineage(text, 0.6), cn)


def test_taxon_table_by_hand(tmp_path):
    from rambl_amd import taxa
    cn = _copy_numbers(tmp_path)
    genera = [("Bacteria", "P", "C", "O", "F", "Zeta"), ("Bacteria", "P", "C", "O", "F9", "Alpha"), ("Archaea", "Q", "C", "O", "F8", "alpha"),
              ("Bacteria", "P", "C", "O", "F", "Weak")]
    res = [(0, [0] * 100, 9), (0, [0] * 100, 9), (1, [1] * 100, 9), (2, [2] * 100, 9), (3, [3] * 59 + [0] * 41, 9), (-1, [], 0)]
    names = ["z1", "z2", "a1", "x1", "w1", "blank"]
    text = T.fixrank_text(names, res, genera)
    length = {"z1": 1000, "z2": 1500, "a1": 800, "x1": 500, "w1": 100, "blank": 30}
    count = {"z1": 10.0, "z2": 5.5, "a1": 8.0, "x1": 3.0, "w1": 100.0}
    rows = taxa.taxa_table(taxa.parse_fixrank(text), length, count, cn, "genus", 0.6)
    # Zeta: family F's row (ancestor fallback: 2.5), the longest gene; Alpha: F9 has none, the phylum's 4.0; alpha: nothing
    # up to the domain: 1.0; Weak has 0.59 < 0.6 and is no taxon
    val = {"Zeta": 15.5 / (2.5 * 1500), "Alpha": 8.0 / (4.0 * 800), "alpha": 3.0 / (1.0 * 500)}
    order = ["Alpha", "Zeta", "alpha"]                                       # byte order: capitals first
    z = sum([val[t] for t in order]) + 1e-10
    assert rows == [(t, val[t] / z) for t in order]
    assert rows == T.ref_taxa_table(text, length, count, cn, "genus", 0.6)
    assert abs(sum(v for _, v in rows) - 1.0) < 1e-6 and sum(v for _, v in rows) < 1.0
    assert taxa.format_taxa_table("S1", rows) == "sample\tS1\n" + "".join("%s\t%r\n" % r for r in rows)
    # at the phylum rank a taxon with its own row takes it
    rows = taxa.taxa_table(taxa.parse_fixrank(text), length, count, cn, "phylum", 0.6)
    assert rows == T.ref_taxa_table(text, length, count, cn, "phylum", 0.6) and [t for t, _ in rows] == ["P", "Q"]
    # a gene missing from the count table gives nothing
    del count["z2"]
    assert taxa.taxa_table(taxa.parse_fixrank(text), length, count, cn, "genus", 0.6) == T.ref_taxa_table(text, length, count, cn, "genus", 0.6)


def test_table_command_line(tmp_path):
    from rambl_amd import taxa
    genera = [("Bacteria", "P", "C", "O", "F", "G1")]
    (tmp_path / "genes.fa").write_text(">a\n%s\n>b\n%s\n" % ("ACGT" * 50, "ACGT" * 70))
    (tmp_path / "fx.tsv").write_text(T.fixrank_text(["a", "b"], [(0, [0] * 100, 9), (0, [0] * 100, 9)], genera))
    (tmp_path / "S_gene_count.tsv").write_text("sample\tS\na\t2.0\nb\t1.5\n")
    (tmp_path / "copy.tsv").write_text(COPY_TSV)
    out = tmp_path / "out"
    assert taxa.main(["table", str(tmp_path / "fx.tsv"), str(tmp_path / "genes.fa"), str(tmp_path / "S_gene_count.tsv"), "S", "--copy-number",
                      str(tmp_path / "copy.tsv"), "-o", str(out)]) == 0
    v = 3.5 / (2.5 * 280)
    assert (out / "S_taxa_count.tsv").read_text() == "sample\tS\nG1\t%r\n" % (v / (v + 1e-10))


def test_profile_options(tmp_path, capsys):
    from fractions import Fraction
    from rambl_amd import profile, taxa
    for extra in (["-C", "x.jar"], ["-t", "0.5"]):
        with pytest.raises(SystemExit):
            profile.main(["g.fa", "s.sam", "s"] + extra)
        assert "copy number correction (-C / -t) needs the RDP classifier" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        profile.main(["g.fa", "s.sam", "s", "-n", "--copy-correct", "fx.tsv", "--copy-number", "c.tsv"])
    assert "--copy-correct cannot be combined with -n" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        profile.main(["g.fa", "s.sam", "s", "--copy-correct", "fx.tsv"])
    assert "go together" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        profile.main(["g.fa", "s.sam", "s", "--copy-thresh", "0.5"])
    assert "--copy-thresh needs --copy-correct" in capsys.readouterr().err
    # a corrected count goes through format_table as a float, rounded after the division
    cn = _copy_numbers(tmp_path)
    text = T.fixrank_text(["a"], [(0, [0] * 100, 5)], [("Bacteria", "P", "C", "O", "F", "G")])
    got = profile.format_table("S", taxa.correct_counts([("a", Fraction(10, 3)), ("b", Fraction(5, 2))], taxa.parse_fixrank(text), cn))
    assert got == "sample\tS\na\t1.333\nb\t2.5\n"
    assert profile.format_table("S", [("a", Fraction(10, 3))]) == "sample\tS\na\t3.333\n"


def test_golden_copy_number_excerpt():
    """The excerpt of the reference's table reads as the scripts read it."""
    from rambl_amd import taxa
    cn = taxa.load_copy_numbers(os.path.join(os.path.dirname(__file__), "golden", "taxa", "rrnDB_excerpt.tsv"))
    assert len(cn) >= 10 and all(v > 0 for v in cn.values()) and "Bacteria" in cn
