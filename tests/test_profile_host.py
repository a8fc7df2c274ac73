"""CPU: the host side of the per-sample gene profile (rambl_amd/profile.py) -- the counting rule against
the recorded output of the reference's own counter, the reads-in rule, the table format, the plain restatement of the hit
contract (tests/native/blast_hits_check.cpp) on alignments computed by hand, and the meaning of the end-to-end data set."""
import json
import math
import os

import pytest

import profile_lib as PL
import stage4_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "profile_counts")


def _cases():
    return sorted(json.load(open(os.path.join(GOLD, "meta.json")))["cases"])


@pytest.mark.parametrize("case", _cases())
def test_counting_rule_equals_the_reference_counter(case):
    from rambl_amd import profile
    t = json.load(open(os.path.join(GOLD, "meta.json")))["cases"][case]
    rows = profile.parse_hits_csv(open(os.path.join(GOLD, case + ".csv")).read())
    got = profile.format_raw(profile.raw_abundance(rows, float(t["-I"]), float(t["-E"])))
    assert got.encode() == open(os.path.join(GOLD, case + ".raw"), "rb").read()


def test_fixtures_cover_what_they_must():
    """Suffix styles, E-value spellings, failing rows, duplicates and gene order are all in the fixtures."""
    from rambl_amd import profile
    rows = [r for c in _cases() for r in profile.parse_hits_csv(open(os.path.join(GOLD, c + ".csv")).read())]
    ends = {r[0][-2:] for r in rows}
    assert {"/1", "/2", ".1", ".2"} <= ends
    assert {"1e-60", "0.0"} <= {r[8] for r in rows}
    assert any(float(r[2]) * 100 / float(r[3]) < 95 for r in rows) and any(float(r[8]) > 1e-10 for r in rows)
    pairs = [(r[0], r[1]) for r in rows]
    assert len(set(pairs)) < len(pairs)
    first_seen = list(dict.fromkeys(r[1] for r in profile.parse_hits_csv(open(os.path.join(GOLD, "case01.csv")).read())))
    assert first_seen != sorted(first_seen, key=str.encode)
    assert any(int(r[6]) > int(r[7]) for r in rows)


def test_counting_rule_by_hand():
    from rambl_amd import profile
    F = profile.Fraction

    def row(seg, gene, e="1e-60", identity=100, n=100):
        return (seg, gene, identity, n, 1, n, 1, n, e, n)
    # a pair both of whose mates tie on one gene gives it 2
    assert profile.raw_abundance([row("a/1", "g"), row("a/2", "g")]) == [("g", F(2))]
    # a failing row does not mark its (segment, gene) as seen: the passing row after it counts
    assert profile.raw_abundance([row("a", "g", identity=90), row("a", "g")]) == [("g", F(1))]
    # a segment id shorter than two characters (the reference throws) is its own read
    assert profile.raw_abundance([row("x", "g"), row("", "h")]) == [("g", F(1)), ("h", F(1))]
    # numbers and text are the same rows
    assert profile.raw_abundance([("a", "g", "100", "100", "1", "100", "1", "100", "1e-60", "100")]) == [("g", F(1))]
    assert profile.format_raw([("g", F(10, 3)), ("h", F(1, 7)), ("i", F(2000000))]) == "g\t3.33333\nh\t0.142857\ni\t2e+06\n"


def test_reads_in_rule():
    from rambl_amd import profile
    recs = [
        (b"pair", 0x41, b"AAAA", b"IIII"), (b"pair", 0x81 | 0x10, b"CCCC", b"IIII"),          # a pair; 0x10 leaves SEQ as stored
        (b"single", 0x10, b"GGTT", b"IIII"),                                                  # a single read, reverse strand
        (b"named/1", 0x41, b"ACAC", b"IIII"), (b"named/2", 0x81, b"TGTG", b"IIII"),           # /1 /2 names lose the suffix
        (b"gone", 0x4, b"TTTT", b"IIII"),                                                     # unmapped: skipped
        (b"twice", 0, b"AAAC", b"IIII"), (b"twice", 0, b"AAAG", b"IIII"),                     # the last record of a kind wins
        (b"noseq", 0, b"*", b"*"),                                                            # no SEQ: skipped
        (b"half", 0x81, b"CACA", b"IIII"),                                                    # only a second segment: one segment
        (b"mixed", 0x41, b"GAGA", b"IIII"), (b"mixed", 0, b"GAGG", b"IIII"),                  # flagless record sets the first
        (b"Upper", 0, b"TTAA", b"IIII"),
    ]
    assert profile.extract_segments(recs) == [
        (b"Upper", b"TTAA"), (b"half", b"CACA"), (b"mixed", b"GAGG"), (b"named/1", b"ACAC"), (b"named/2", b"TGTG"),
        (b"pair/1", b"AAAA"), (b"pair/2", b"CCCC"), (b"single", b"GGTT"), (b"twice", b"AAAG")]


def test_table_format():
    from rambl_amd import profile
    F = profile.Fraction
    counts = [("Zeta", F(1)), ("alpha", F(10, 3)), ("beta", F(1, 16)), ("gamma", F(12345))]
    assert profile.format_table("s1", counts) == "sample\ts1\nZeta\t1.0\nalpha\t3.333\nbeta\t0.063\ngamma\t12345.0\n"
    rel = profile.format_table("s1", [("a", F(1)), ("b", F(2))], relative=True)
    assert rel == "sample\ts1\na\t0.333333333\nb\t0.666666667\n"
    assert profile.format_table("empty", []) == "sample\tempty\n"


def test_hits_csv_round_trip():
    from rambl_amd import profile
    rows = [("r/1", "g", "149", "150", "1", "150", "300", "151", "3.21e-75", "150")]
    assert profile.hits_csv(rows) == "r/1,g,149,150,1,150,300,151,3.21e-75,150\n"
    assert profile.parse_hits_csv(profile.hits_csv(rows)) == rows
    assert profile.format_evalue(3.4287416591068102e-08) == "3.42874e-08" and profile.format_evalue(0.0) == "0"


def test_options_outside_the_contract_are_errors(capsys):
    from rambl_amd import profile
    for extra in (["-C", "classifier.jar"], ["-w", "11"], ["-P", "-3"], ["-A", "5"], ["-R", "2"], ["-t", "0.5"]):
        with pytest.raises(SystemExit) as e:
            profile.main(["genes.fa", "sample.sam", "s"] + extra)
        assert e.value.code == 2
    assert "copy number correction" in capsys.readouterr().err


G = "ACGTACGTTAGCCGATAGGCTTAACCGGATATCGCGATTACA"           # 42 bases


def _sub(s, i, c):
    return s[:i] + c + s[i + 1:]


# (name, gene, segment, expected (strand, doubled score, identity, align_len, qfrom, qto, hfrom, hto)); computed by hand
BY_HAND = [
    ("exact match", G, G[8:26], (0, 36, 18, 18, 1, 18, 9, 26)),
    ("reverse strand", G, L.revcomp(G[8:26]), (1, 36, 18, 18, 1, 18, 26, 9)),
    ("one mismatch", G, _sub(G[8:28], 10, "T"), (0, 34, 19, 20, 1, 20, 9, 28)),                       # 19 * 2 - 4
    ("a gene base missing from the segment", G, G[4:16] + G[17:30], (0, 45, 25, 26, 1, 25, 5, 30)),    # 25 * 2 - 5: 22.5
    ("a base more in the segment", G, G[4:16] + "T" + G[16:30], (0, 47, 26, 27, 1, 27, 5, 30)),        # 26 * 2 - 5: 23.5
    ("N in the segment", G, _sub(G[8:28], 10, "N"), (0, 34, 19, 20, 1, 20, 9, 28)),
    ("N in the gene", _sub(G, 18, "N"), G[8:28], (0, 34, 19, 20, 1, 20, 9, 28)),
    ("N against N is a mismatch", _sub(G, 18, "N"), _sub(G[8:28], 10, "N"), (0, 34, 19, 20, 1, 20, 9, 28)),
    ("overhang at the gene start", G, "CCCCC" + G[0:15], (0, 30, 15, 15, 6, 20, 1, 15)),
    ("overhang at the gene end", G, G[30:42] + "GGGGG", (0, 24, 12, 12, 1, 12, 31, 42)),
    ("overhang on the reverse strand", G, L.revcomp("CCCCC" + G[0:15]), (1, 30, 15, 15, 1, 15, 15, 1)),
    ("two places: the smaller end column", "GATTACAGGCTA" + "TTTTT" + "GATTACAGGCTA", "GATTACAGGCTA", (0, 24, 12, 12, 1, 12, 1, 12)),
    ("both strands: forward", "TTTT" + "GAATTCGAATTC" + "CCCC", "GAATTCGAATTC", (0, 24, 12, 12, 1, 12, 5, 16)),
    # crossing the mismatch (-4) to two more matches (+4) only ties: the smaller end column ends before it
    ("a tie ends early", G, G[8:18] + "T" + G[19:21], (0, 20, 10, 10, 1, 10, 9, 18)),
]


def test_restatement_on_alignments_by_hand(tmp_path):
    exe = PL.build_hits_check(tmp_path)
    assert G[18] == "G" and len(G) == 42 and len(BY_HAND) >= 12
    for name, gene, seg, exp in BY_HAND:
        got = PL.run_hits_check(exe, [gene], [seg], 0.0, 1e300)
        assert len(got) == 1, name
        assert got[0][:2] == (0, 0) and got[0][2:10] == exp, (name, got[0])
        e = 0.46 * len(seg) * len(gene) * math.exp(-1.28 * exp[1] / 2.0)
        assert float(got[0][10]) == pytest.approx(e, rel=1e-12), name
    # thresholds: 19 of 20 columns is exactly 95 %; the E-value of the exact match (raw score 18, m 18, n 42) is 3.4e-08
    one = BY_HAND[2]
    assert len(PL.run_hits_check(exe, [one[1]], [one[2]], 95.0, 1e300)) == 1
    assert len(PL.run_hits_check(exe, [one[1]], [one[2]], 95.1, 1e300)) == 0
    assert len(PL.run_hits_check(exe, [G], [G[8:26]], 0.0, 3.5e-8)) == 1 and len(PL.run_hits_check(exe, [G], [G[8:26]], 0.0, 3.4e-8)) == 0
    # n is the sum of all gene lengths, hits come in (segment, gene) order, a segment without a match gives no hit
    got = PL.run_hits_check(exe, [G, "TTTTTTTT", G], ["CCCCCC", G[8:26]], 0.0, 1e300)
    assert [h[:2] for h in got if h[3] >= 30] == [(1, 0), (1, 2)]
    assert float([h for h in got if h[:2] == (1, 0)][0][10]) == pytest.approx(0.46 * 18 * 92 * math.exp(-1.28 * 18), rel=1e-12)


def test_mixture_orders_the_strains_as_mixed(tmp_path):
    """The end-to-end data set means something: with the restatement chain, within each gene the strains' order by count is
    their order by mixed proportion (4 : 2 : 1), in every sample.  tests/test_profile_gpu.py relies on this."""
    exe = PL.build_hits_check(tmp_path)
    names, seqs, samples = PL.mixture_dataset()
    for sample, lines, mix in samples:
        _, counts = PL.expected_table(exe, names, seqs, sample, lines)
        for k in range(3):
            got = [float(counts.get("gene%d_strain%d" % (k, s), 0)) for s in range(3)]
            assert sorted(range(3), key=lambda s: got[s]) == sorted(range(3), key=lambda s: mix[k][s]), (sample, k, got, mix[k])
            assert min(got) > 0
