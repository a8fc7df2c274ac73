"""CPU: stage 4 (rambl_amd/stage4.py) -- the constants of the alignment contract pinned by hand-computed cases on the
plain restatement (tests/native/sw_check.cpp), read extraction, the SAM writer and its order, and that the written SAM
loads through the library's reader."""
import math
import os
import random

import numpy as np
import pytest

import stage4_lib as L
from rambl_amd import stage4


@pytest.fixture(scope="module")
def sw(tmp_path_factory):
    return L.build_sw_check(tmp_path_factory.mktemp("sw"))


SEED = L.rand_seq(random.Random(5), 120)


def one(sw, read, qual="*"):
    return L.run_sw_check(sw, [SEED], [(read, qual)])[0]


def test_exact_match_30(sw):
    r = one(sw, SEED[40:70])
    assert r[0] == 60 and r[5] == "30M" and r[4] == 41 and r[6] == 0 and r[3] == 0


def test_one_q40_mismatch_in_the_middle(sw):
    read = list(SEED[40:70])
    read[15] = "A" if read[15] != "A" else "C"
    r = one(sw, "".join(read), "I" * 30)
    assert r[0] == 52 and r[5] == "30M" and r[6] == 1


def test_mismatch_at_read_base_0_is_clipped(sw):
    read = list(SEED[40:70])
    read[0] = "A" if read[0] != "A" else "C"
    r = one(sw, "".join(read))
    assert r[0] == 58 and r[5] == "1S29M" and r[4] == 42


def test_low_quality_and_n_penalties(sw):
    read = list(SEED[40:70])
    read[15] = "A" if read[15] != "A" else "C"
    assert one(sw, "".join(read), "I" * 15 + "+" + "I" * 14)[0] == 60 - 2 - 3     # Q10: 2 + floor(4 * 10 / 40)
    read[15] = "N"
    assert one(sw, "".join(read))[0] == 60 - 2 - 1


def test_two_base_deletion_costs_11(sw):
    read = SEED[20:50] + SEED[52:82]
    r = one(sw, read)
    assert r[0] == 120 - 11 and r[6] == 2
    m, n = r[5].split("M2D")                           # where the repeat lets it slide, diagonal-first puts it leftmost
    assert int(m) + int(n[:-1]) == 60 and int(m) <= 30 and n.endswith("M")


def test_no_gap_within_4_of_a_read_end(sw):
    # the deletion after read base 2 would score 37 * 2 - 11 = 63; barred, the read clips instead: 3S35M = 70 - ... no gap
    read = SEED[10:13] + SEED[15:50]
    r = one(sw, read)
    assert "D" not in r[5] and "I" not in r[5]
    read = SEED[10:16] + SEED[18:50]                   # after read base 5: allowed
    r = one(sw, read)
    assert r[5] == "6M2D32M" and r[0] == 76 - 11


def test_threshold_at_30():
    assert abs(stage4.threshold(30) - 47.2) < 0.01
    assert stage4.threshold(30) == 20.0 + 8.0 * math.log(30)


def test_ties_lower_seed_forward_strand(sw):
    s2 = [SEED, SEED, L.revcomp(SEED)]
    r = L.run_sw_check(sw, s2, [(SEED[10:60], "*")])[0]
    assert r[2] == 0 and r[3] == 0 and r[1] == r[0]     # duplicated seed: XS = AS
    r = L.run_sw_check(sw, [L.revcomp(SEED), SEED], [(SEED[10:60], "*")])[0]
    assert r[2] == 0 and r[3] == 1                     # the reverse strand of seed 0 beats the forward strand of seed 1


def test_extraction():
    recs = [
        (b"r2", 0x1 | 0x40, b"AACC", b"ABCD"),
        (b"r2", 0x1 | 0x80 | 0x10, b"AACG", b"EFGH"),   # reverse: back to the read as sequenced
        (b"r1", 0x0, b"GGGT", b"IIII"),
        (b"r3", 0x1 | 0x40, b"TTTT", b"JJJJ"),          # orphan mate: a single read
        (b"r4", 0x4, b"CCCC", b"KKKK"),                  # unmapped: skipped
        (b"r1", 0x10, b"ACGT", b"LMNO"),                 # duplicated QNAME: the last record wins
        (b"r2", 0x1 | 0x40, b"CCCC", b"PQRS"),           # a later mate 1 replaces the first
    ]
    out = stage4.extract_reads(recs)
    assert [q for q, _ in out] == [b"r1", b"r2", b"r3"]
    assert out[0][1] == [(b"ACGT", b"ONML")]
    assert out[1][1] == [(b"CCCC", b"PQRS"), (b"CGTT", b"HGFE")]
    assert out[2][1] == [(b"TTTT", b"JJJJ")]


class _Res:
    def __init__(self, rows):
        cols = list(zip(*rows))
        self.as_, self.xs, self.seed, self.strand, self.pos, self.nm = (np.array(c) for c in cols[:6])
        self.cigar = list(cols[6])


def test_sam_writer_flags_order_and_drops():
    reads = [(b"a", [(b"ACGTA", b"IIIII"), (b"CCCCC", b"IIIII")]),       # pair, mate 2 unaligned: dropped
             (b"b", [(b"GGGGG", b"ABCDE")]),                              # single, reverse
             (b"c", [(b"TTTTT", b"IIIII"), (b"AAAAA", b"IIIII")]),        # pair on one seed
             (b"d", [(b"ACACA", b"IIIII")])]                              # single, same key as c's mate 1
    res = _Res([(10, -1, 0, 0, 5, 0, "5M"), (3, -1, -1, 0, 0, 0, "*"),
                (10, 10, 1, 1, 7, 1, "5M"),
                (10, 8, 0, 0, 3, 0, "5M"), (10, -1, 0, 1, 20, 0, "2S3M"),
                (10, -1, 0, 0, 3, 0, "5M")])
    lines = stage4.sam_records(reads, res, ["s0", "s1"])
    f = [ln.rstrip("\n").split("\t") for ln in lines]
    assert [x[0] for x in f] == ["c", "d", "c", "b"]                   # (seed, POS, reverse), stable in QNAME order
    c1, d, c2, b = f
    assert int(c1[1]) == 0x1 | 0x40 | 0x20 and c1[6] == "=" and c1[7] == "20" and c1[8] == "20"
    assert int(c2[1]) == 0x1 | 0x80 | 0x10 and c2[7] == "3" and c2[8] == "-20"
    assert int(b[1]) == 0x10 and b[9] == "CCCCC" and b[10] == "EDCBA" and b[4] == "0" and "XS:i:10" in b[11:]
    assert d[4] == "42" and not any(t.startswith("XS:i:") for t in d[11:]) and "NM:i:0" in d[11:]
    assert stage4.sam_header(["s0", "s1"], [b"AC", b"GGT"]) == "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:s0\tLN:2\n@SQ\tSN:s1\tLN:3\n"


def test_written_sam_loads_through_the_reader(tmp_path):
    from rambl_amd import samio
    reads = [(b"r%d" % k, [(b"ACGTACGTAC", b"IIIIIIIIII")]) for k in range(5)]
    res = _Res([(20, -1, k % 2, 0, 1 + k, 0, "10M") for k in range(5)])
    p = tmp_path / "x.sam"
    p.write_text(stage4.sam_header(["s0", "s1"], [b"A" * 40, b"C" * 40]) + "".join(stage4.sam_records(reads, res, ["s0", "s1"])))
    aln = samio.Alignments(str(p))
    assert aln.native.ref_stats("s0")[0] == 3 and aln.native.ref_stats("s1")[0] == 2
    walked = list(aln.native.walk())
    assert [w[0] for w in walked] == [b"r0", b"r2", b"r4", b"r1", b"r3"] and walked[0][3] == b"IIIIIIIIII"


def test_seed_fasta_and_fai(tmp_path):
    g = tmp_path / "genes.fa"
    g.write_text(">x desc\n" + "A" * 70 + "\n>y\n" + "C" * 130 + "\n>z\nGG\n")
    seqs = stage4.write_seed_fasta(str(g), ["z", "y"], str(tmp_path / "seed_otus.fasta"))
    assert seqs == [b"GG", b"C" * 130]
    assert (tmp_path / "seed_otus.fasta").read_text() == ">z\nGG\n>y\n" + "C" * 60 + "\n" + "C" * 60 + "\n" + "C" * 10 + "\n"
    assert (tmp_path / "seed_otus.fasta.fai").read_text() == "z\t2\t3\t60\t61\ny\t130\t9\t60\t61\n"


def test_other_mapper_is_an_error(tmp_path):
    with pytest.raises(SystemExit):
        stage4.main(["a", "b", "c", "-m", "bwa"])
    with pytest.raises(ValueError):
        stage4.recluster("a", "b", "c", map_args="--very-sensitive-local")
