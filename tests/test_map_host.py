"""CPU: the read mapper's contract on the restatement (map_lib), its named cases' property checks, the lemma of DESIGN.md
§8.18, and the host half of rambl_amd/map.py: FASTQ parsing, the SAM writer and the command line's errors.  No device call."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import sys

import pytest

import map_edge_lib as E
import map_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "straincall_hip.h")
NEW = ["sc_map_index_create", "sc_map_index_info", "sc_map_index_free", "sc_map_reads", "sc_map_candidates", "sc_map_limits", "sc_map_error"]


def _range_genes():
    from rambl_amd import capi
    return capi.map_limits()[0]


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in E.cases(_range_genes())}


CASE_NAMES = [c.name for c in E.cases(64)]          # the names do not depend on the range size


def test_limits_are_exported():
    from rambl_amd import capi
    rg, mv = capi.map_limits()
    assert rg >= 64 and rg % 64 == 0 and mv == 502 and (rg * 4) <= 64 * 1024


@pytest.mark.parametrize("name", CASE_NAMES)
def test_named_case_reaches_its_edge(cases, name):
    c = cases[name]
    assert all(1 <= len(g) <= 8192 for g in c.genes) and all(1 <= len(r) <= 512 for r in c.reads)
    c.check()


def longest_common_run(read, piece):
    """The longest run of equal bases of two sequences of equal length, position by position."""
    best = run = 0
    for a, b in zip(read, piece):
        run = run + 1 if a == b else 0
        best = max(best, run)
    return best


def test_lemma_substitutions_leave_a_shared_run():
    """A read of L bases with s substitutions and no indel shares a run of ceil((L - s) / (s + 1)) bases with its gene; at
    L = 150 and k = 16 that is s <= 8, and with max_occ unbounded the gene is then a candidate."""
    rng = random.Random(88)
    L = 150
    assert all(-(-(L - s) // (s + 1)) >= 16 for s in range(9)) and -(-(L - 9) // 10) < 16
    genes = [E.seq(rng, 400) for _ in range(6)]
    index = M.build_index(genes, 16)
    for trial in range(200):
        s = trial % 9
        g = rng.randrange(len(genes))
        a = rng.randrange(0, 400 - L)
        piece = genes[g][a:a + L]
        read = list(piece)
        if trial < 18 and s:                                      # the worst case: substitutions spread evenly
            where = [((i + 1) * (L - s)) // (s + 1) + i for i in range(s)]
        else:
            where = rng.sample(range(L), s)
        for i in where:
            read[i] = E.other(rng, read[i])
        read = "".join(read)
        assert longest_common_run(read, piece) >= -(-(L - s) // (s + 1))
        if trial % 2:
            read = M.revcomp(read)
        assert g in [x[0] for x in M.candidates(index, read, 16, 1 << 30, 0, 1)], (trial, s)


# ---------------------------------------------------------------------------------------------------- FASTQ

def _write_fastq(path, recs, gz=False):
    text = "".join("@%s\n%s\n+\n%s\n" % r for r in recs).encode()
    with open(path, "wb") as f:
        f.write(gzip.compress(text) if gz else text)


def test_fastq_plain_gzip_and_names(tmp_path):
    from rambl_amd import map as P
    recs = [("r1/1 extra words", "ACGT", "IIII"), ("r2/2", "GGCA", "II#I"), ("r3 1:N:0", "TTTT", "5555"), ("r4/3", "A", "I")]
    plain, packed = str(tmp_path / "a.fastq"), str(tmp_path / "a.fastq.gz")
    _write_fastq(plain, recs)
    _write_fastq(packed, recs, gz=True)
    want = [(b"r1", b"ACGT", b"IIII"), (b"r2", b"GGCA", b"II#I"), (b"r3", b"TTTT", b"5555"), (b"r4/3", b"A", b"I")]
    assert P.read_fastq(plain) == want and P.read_fastq(packed) == want
    assert [(q.encode(), s.encode(), ql.encode()) for q, s, ql in M.fastq_records(packed)] == want
    assert open(packed, "rb").read(2) == b"\x1f\x8b"
    empty = str(tmp_path / "e.fastq")
    open(empty, "w").close()
    assert P.read_fastq(empty) == []


def test_fastq_errors(tmp_path):
    from rambl_amd import map as P
    for k, text in enumerate(("@r\nACGT\n+\nIII\n", "@r\nACGT\n+\n", "r\nACGT\n+\nIIII\n", "@r\nACGT\n-\nIIII\n")):
        p = str(tmp_path / ("bad%d.fastq" % k))
        open(p, "w").write(text)
        with pytest.raises(P.InputError):
            P.read_fastq(p)
    a, b = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq")
    _write_fastq(a, [("x/1", "ACGT", "IIII"), ("y/1", "ACGT", "IIII")])
    _write_fastq(b, [("x/2", "ACGT", "IIII")])
    with pytest.raises(P.InputError):
        P.read_sample(a, b)
    assert P.read_sample(a) == [(b"x", [(b"ACGT", b"IIII")]), (b"y", [(b"ACGT", b"IIII")])]


class _FakeIndex:
    """Stands in for capi.MapIndex: records what it is given and maps every read to gene 0."""

    def map_reads(self, reads, quals, max_occ, max_cand, min_votes, pair_room):
        self.reads = reads
        n = len(reads)

        class R:
            gene, strand, pos, as_, xs, nm, cigar, stats = [0] * n, [0] * n, [1] * n, [50] * n, [-1] * n, [0] * n, ["%dM" % len(r) for r in reads], None
        return R


def test_empty_and_over_long_reads_stay_unmapped():
    from rambl_amd import map as P
    sample = [(b"a", [(b"ACGT" * 10, b"I" * 40), (b"", b"")]), (b"b", [(b"A" * 513, b"I" * 513), (b"C" * 512, b"I" * 512)])]
    fake = _FakeIndex()
    res, left_out, _ = P.map_sample(fake, sample, 1024, 16, 1)
    assert left_out == 2 and fake.reads == [b"ACGT" * 10, b"C" * 512]
    assert res.gene == [0, -1, -1, 0] and res.cigar == ["40M", "*", "*", "512M"]
    lines = P.sam_records(sample, res, ["g"])
    assert [int(x.split("\t")[1]) for x in lines] == [0x1 | 0x40 | 0x8, 0x1 | 0x80 | 0x8]


# ---------------------------------------------------------------------------------------------------- SAM

def _rows_to_mapped(rows):
    from rambl_amd import map as P
    res = P.Mapped(len(rows))
    for i, (as_, xs, gene, strand, pos, cigar, nm) in enumerate(rows):
        res.as_[i], res.xs[i], res.gene[i], res.strand[i], res.pos[i], res.cigar[i], res.nm[i] = as_, xs, gene, strand, pos, cigar, nm
    return res


def test_sam_flags_order_and_header():
    from rambl_amd import map as P
    names, genes = ["gB", "gA", "gC"], ["A" * 300, "C" * 200, "G" * 100]
    q = "I" * 9 + "#"
    sample = [("p1", [("ACGTACGTAC", q), ("TTGACCATGA", q)]),         # both on gene 1, mate 2 reverse and to the left
              ("p2", [("ACGTACGTAC", q), ("TTGACCATGA", q)]),         # mate 2 unmapped
              ("p3", [("ACGTACGTAC", q), ("TTGACCATGA", q)]),         # mates on different genes
              ("p4", [("ACGTACGTAC", q), ("TTGACCATGA", q)]),         # both unmapped
              ("p5", [("ACGTACGTAC", q), ("TTGACCATGA", q)])]         # same gene, same POS as p1's mate 2: input order decides
    rows = [(20, -1, 1, 0, 50, "10M", 0), (18, 18, 1, 1, 30, "4M1D6M", 1),
            (20, 12, 0, 1, 7, "2S8M", 0), M.NO_ROW,
            (20, -1, 2, 0, 5, "10M", 0), (16, -1, 0, 0, 9, "3M1I6M", 2),
            M.NO_ROW, (5, -1, -1, 0, 0, "*", 0),
            (20, -1, 1, 0, 30, "10M", 0), (20, -1, 1, 1, 30, "10M", 0)]
    as_bytes = [(n.encode(), [(s.encode(), ql.encode()) for s, ql in mates]) for n, mates in sample]
    got = P.sam_header(names, [g.encode() for g in genes]) + "".join(P.sam_records(as_bytes, _rows_to_mapped(rows), names))
    assert got == M.sam_text(names, genes, sample, rows)
    lines = got.splitlines()
    assert lines[:4] == ["@HD\tVN:1.0\tSO:coordinate", "@SQ\tSN:gB\tLN:300", "@SQ\tSN:gA\tLN:200", "@SQ\tSN:gC\tLN:100"]
    recs = [x.split("\t") for x in lines[4:]]
    assert [(r[0], int(r[1]), r[2], int(r[3])) for r in recs] == [
        ("p2", 0x1 | 0x40 | 0x10 | 0x8, "gB", 7), ("p3", 0x1 | 0x80, "gB", 9),
        ("p1", 0x1 | 0x80 | 0x10, "gA", 30), ("p5", 0x1 | 0x40 | 0x20, "gA", 30), ("p5", 0x1 | 0x80 | 0x10, "gA", 30), ("p1", 0x1 | 0x40 | 0x20, "gA", 50),
        ("p3", 0x1 | 0x40, "gC", 5)]
    assert not any(int(r[1]) & 0x2 for r in recs)
    by = {(r[0], int(r[1]) & 0xC0): r for r in recs}
    assert by[("p2", 0x40)][6:9] == ["*", "0", "0"] and by[("p3", 0x40)][6:9] == ["gB", "9", "0"]
    assert by[("p1", 0x40)][6:9] == ["=", "30", "-30"] and by[("p1", 0x80)][6:9] == ["=", "50", "30"]
    assert by[("p1", 0x80)][4] == "0" and by[("p1", 0x40)][4] == "42"              # MAPQ 0 when XS = AS
    assert by[("p1", 0x80)][9] == M.revcomp("TTGACCATGA") and by[("p1", 0x80)][10] == q[::-1]
    assert by[("p1", 0x80)][11:] == ["AS:i:18", "XS:i:18", "NM:i:1"] and by[("p1", 0x40)][11:] == ["AS:i:20", "NM:i:0"]


def test_shared_sam_writer_policies_differ_only_as_stated():
    """samio.sam_records under stage 4's policies (a pair with an unaligned mate dropped, the strand in the sort key) and the
    mapper's (the aligned mate kept with 0x8, sorted by reference and POS alone) on one input: the two texts differ in that
    pair and in the order of two records of one POS, and nowhere else; numpy arrays and lists give the same text."""
    import numpy as np
    from rambl_amd import samio
    names = ["gA", "gB"]
    reads = [(b"lone", [(b"ACGTACGTAC", b"IIIIIIIII#"), (b"TTGACCATGA", b"#IIIIIIIII")]),      # mate 2 unaligned
             (b"same", [(b"ACGTTGCAAC", b"ABCDEFGHIJ"), (b"GGATCCAATT", b"JIHGFEDCBA")]),      # one POS, mate 1 reverse, mate 2 forward
             (b"star", [(b"AACCGGTTAC", b"*")]),                                             # reverse, no qualities
             (b"last", [(b"ACGTACGTAC", b"IIIIIIIIII")])]
    cols = dict(ref=[0, -1, 1, 1, 0, 1], strand=[0, 0, 1, 0, 1, 0], pos=[40, 0, 20, 20, 7, 90], as_=[20, 0, 20, 18, 16, 20],
                xs=[-1, -1, 18, 18, -1, 20], nm=[0, 0, 0, 1, 2, 0])
    cigar = ["10M", "*", "10M", "4M1D6M", "2S8M", "10M"]

    def text(keep, by_strand, arrays):
        c = {k: np.array(v, dtype=np.int32) for k, v in cols.items()} if arrays else cols
        return samio.sam_records(reads, c["ref"], c["strand"], c["pos"], c["as_"], c["xs"], c["nm"], cigar, names, keep, by_strand)
    stage4, mapper = text(False, True, True), text(True, False, False)
    assert stage4 == text(False, True, False) and mapper == text(True, False, True)
    # the pair with the unaligned mate
    lone = [x for x in mapper if x.startswith("lone\t")]
    assert not any(x.startswith("lone\t") for x in stage4) and len(lone) == 1
    f = lone[0].split("\t")
    assert int(f[1]) == 0x1 | 0x40 | 0x8 and f[2:4] == ["gA", "40"] and f[6:9] == ["*", "0", "0"]
    # the two records of one POS: forward before reverse under stage 4's key, input order (mate 1, the reverse one) under the mapper's
    def flags(lines):
        return [int(x.split("\t")[1]) for x in lines if x.startswith("same\t")]
    assert flags(stage4) == [0x1 | 0x80 | 0x20, 0x1 | 0x40 | 0x10] and flags(mapper) == flags(stage4)[::-1]
    # every other line, and its place
    rest = [x for x in mapper if not x.startswith("lone\t")]
    a, b = (k for k, x in enumerate(rest) if x.startswith("same\t"))
    assert b == a + 1
    rest[a], rest[b] = rest[b], rest[a]
    assert rest == stage4 and [x.split("\t")[0] for x in stage4] == ["star", "same", "same", "last"]
    star = stage4[0].split("\t")
    assert int(star[1]) == 0x10 and star[9:11] == [M.revcomp("AACCGGTTAC"), "*"] and star[5] == "2S8M"
    same1 = stage4[2].split("\t")
    assert same1[4] == "42" and same1[6:9] == ["=", "20", "11"] and same1[10] == "JIHGFEDCBA" and same1[11:] == ["AS:i:20", "XS:i:18", "NM:i:0\n"]
    assert stage4[1].split("\t")[4] == "0" and stage4[1].split("\t")[8] == "-11"


# ---------------------------------------------------------------------------------------------------- command line

def test_command_line_errors_leave_with_2_and_touch_no_device(tmp_path, monkeypatch):
    from rambl_amd import capi
    from rambl_amd import map as P

    def no_device(*a, **kw):
        raise AssertionError("the library was called")
    monkeypatch.setattr(capi, "lib", no_device)
    fa, fq, bad = str(tmp_path / "g.fa"), str(tmp_path / "r.fastq"), str(tmp_path / "bad.fastq")
    open(fa, "w").write(">g1 x\nACGTACGTACGTACGTACGTAAA\n")
    _write_fastq(fq, [("r/1", "ACGTACGTACGTACGTACGT", "I" * 20)])
    open(bad, "w").write("@r\nACGT\n+\nII\n")
    out = str(tmp_path / "o.sam")
    long_fa = str(tmp_path / "long.fa")
    open(long_fa, "w").write(">g\n" + "A" * 8193 + "\n")

    def status(argv):
        try:
            return P.main(argv)
        except SystemExit as e:
            return e.code
    assert status([fa, "-1", str(tmp_path / "missing.fastq"), "-o", out]) == 2
    assert status([str(tmp_path / "missing.fa"), "-1", fq, "-o", out]) == 2
    assert status([fa, "-1", bad, "-o", out]) == 2
    assert status([long_fa, "-1", fq, "-o", out]) == 2
    assert status([fa, "-1", fq, "-2", bad, "-o", out]) == 2
    for extra in (["-k", "10"], ["-k", "17"], ["--max-occ", "0"], ["--max-cand", "-1"], ["--min-votes", "0"], ["-c", "0"], ["--device", "-1"]):
        assert status([fa, "-1", fq, "-o", out] + extra) == 2, extra
    assert status([fa, "-o", out]) == 2 and status([fa, "-1", fq, "-U", fq, "-o", out]) == 2 and status([fa, "-2", fq, "-o", out]) == 2
    assert status([fa, "-1", fq]) == 2
    assert not os.path.exists(out)


def test_bin_rambl_map_missing_file_is_status_2(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rambl-map"), str(tmp_path / "no.fa"), "-U", str(tmp_path / "no.fastq"),
                        "-o", str(tmp_path / "o.sam")], stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"no such file" in r.stderr


# ---------------------------------------------------------------------------------------------------- the C interface

def test_header_table_and_exports_agree_on_the_new_names():
    from rambl_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(sc_map_\w+)\s*\(", hdr)
    assert declared == NEW and [n for n in capi.EXPORTS if n.startswith("sc_map_")] == NEW
    lib = capi.lib()
    for n in NEW:
        getattr(lib, n)
    text = open(HEADER).read()
    for n in NEW[:1] + NEW[3:6]:
        at = text.index("int %s(" % n)
        assert "get_sra_and_mapping.py:49-90" in text[text.rindex("/*", 0, at):at], n
    assert capi.MapIndex._free == "sc_map_index_free" and issubclass(capi.MapIndex, capi.Handle)
    assert capi.MAP_DEFAULTS == dict(seed_k=16, max_occ=1024, max_cand=16, min_votes=1)


def test_map_stats_layout_matches_its_mirror(tmp_path):
    """sc_map_stats is declared as a tagged struct with its typedef beside it, so this file holds its layout against
    capi.ScMapStats member by member."""
    from rambl_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct sc_map_stats \{(.*?)\};", hdr, flags=re.S).group(1)
    members = [m for stmt in body.split(";") if stmt.strip() for m in [stmt.split()[-1]]]
    assert members == [f for f, _ in capi.ScMapStats._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "straincall_hip.h"', 'int main(void) {',
             '    printf("%zu\\n", sizeof(sc_map_stats));']
    lines += ['    printf("%%zu %%zu\\n", offsetof(sc_map_stats, %s), sizeof(((sc_map_stats*)0)->%s));' % (m, m) for m in members]
    lines += ['    return 0;', '}', '']
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-Wall", "-I", os.path.dirname(HEADER), "-o", exe, src])
    printed = [tuple(int(x) for x in line.split()) for line in subprocess.check_output([exe]).decode().splitlines()]
    assert printed[0] == (C.sizeof(capi.ScMapStats),)
    for m, got in zip(members, printed[1:]):
        f = getattr(capi.ScMapStats, m)
        assert (f.offset, f.size) == got, m
