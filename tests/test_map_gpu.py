"""GPU: the read mapper on the device (rambl_amd/csrc/sc_map.hip) against the plain restatement of its contract (map_lib,
tests/native/sw_check.cpp) on every named case, against sc_align_reads where every gene is a candidate, and bin/rambl-map
end to end."""
import os
import random
import subprocess
import sys

import pytest

import map_edge_lib as E
import map_lib as M
import stage4_lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    from rambl_amd import capi
    return E.cases(capi.map_limits()[0])


CASE_NAMES = [c.name for c in E.cases(64)]


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in _cases()}


@pytest.fixture(scope="module")
def sw_check(tmp_path_factory):
    return L.build_sw_check(tmp_path_factory.mktemp("sw"))


def _b(seqs):
    return [s.encode() for s in seqs]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_candidates_equal_the_restatement(cases, name):
    from rambl_amd import capi
    c = cases[name]
    c.check()
    with capi.MapIndex(_b(c.genes), c.k) as ix:
        off, gene, fw, rc = ix.candidates(_b(c.reads), c.max_occ, c.max_cand, c.min_votes, cap=4)          # the room grows from 4
        info = ix.info()
    want = M.flat_candidates(c.candidates())
    assert (off.tolist(), gene.tolist(), fw.tolist(), rc.tolist()) == want
    assert info["n_genes"] == len(c.genes) and info["seed_k"] == c.k and info["gene_bases"] == sum(len(g) for g in c.genes)
    assert info["n_keys"] == sum(len(v) for v in M.build_index(c.genes, c.k).values())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_reads_equal_sw_check_on_the_candidates(cases, sw_check, name):
    from rambl_amd import capi
    c = cases[name]
    rng = random.Random(len(name))
    reads = [(r, L.qual_string(rng, len(r), low=(i % 3 == 0)) if i % 5 else "*") for i, r in enumerate(c.reads)]
    exp = M.expected_rows(sw_check, c.genes, reads, c.candidates())
    with capi.MapIndex(_b(c.genes), c.k) as ix:
        got = ix.map_reads(_b(r for r, _ in reads), _b(q for _, q in reads), c.max_occ, c.max_cand, c.min_votes, c.pair_room)
    L.compare_rows(reads, exp, M.device_rows(got), c.name)
    assert got.n_cand.tolist() == [len(x) for x in c.candidates()]
    assert got.stats.n_pairs == sum(len(x) for x in c.candidates()) and got.stats.n_traced == sum(1 for e in exp if e[2] >= 0)
    if c.stretches is not None:
        assert got.stats.n_stretches == c.stretches
    if c.max_occ < E.BIG:
        assert got.stats.n_skipped > 0
    assert got.stats.n_windows == 2 * sum(1 for r in c.reads for w in M.windows(r, c.k) if w is not None)


def test_boundary_read_maps_with_sc_align_reads_only(cases):
    from rambl_amd import capi
    c = cases["valid_alignment_without_a_shared_kmer"]
    full = capi.align_reads(_b(c.genes), _b(c.reads))
    assert full.seed.tolist() == [0] and full.as_[0] == 2 * 140 - 6 * 10
    with capi.MapIndex(_b(c.genes), c.k) as ix:
        got = ix.map_reads(_b(c.reads))
    assert got.gene.tolist() == [-1] and got.as_.tolist() == [0] and got.xs.tolist() == [-1] and got.n_cand.tolist() == [0]


def anchored_set():
    """Every gene and every read holds one common anchor 16-mer, so with a large max_occ and max_cand = 0 every gene is a
    candidate of every read: the mapper then has to return what sc_align_reads returns.  Reads of both strands, R = 1..8."""
    rng = random.Random(77)
    anchor = E.seq(rng, 16)
    genes = []
    for i in range(9):
        body = E.seq(rng, rng.choice([300, 500, 700]))
        at = rng.randrange(20, len(body) - 40)
        genes.append(body[:at] + anchor + body[at + 16:])
    at = genes[2].index(anchor)
    close = L.mutate(rng, genes[2], 0.03)
    genes.append(close[:at] + anchor + close[at + 16:])                    # a close relative, the anchor kept
    genes.append(genes[4])                                                 # a duplicate: ties go to the lower index
    reads = []
    for n in (40, 100, 150, 200, 300, 350, 400, 500):                      # 1..8 rows per lane
        for rep in range(4):
            g = genes[rng.randrange(len(genes))]
            a = rng.randrange(0, len(g) - min(n, len(g)) + 1)
            r = L.mutate(rng, g[a:a + n], 0.03)
            if len(r) < n:
                r += E.seq(rng, n - len(r))
            if rep == 1:
                p = rng.randrange(10, n - 26)
                r = r[:p] + r[p + 2:] + "AC"                               # a deletion from the read
            if anchor not in r:
                p = rng.randrange(0, n - 16)
                r = r[:p] + anchor + r[p + 16:]
            if rep % 2:
                r = L.revcomp(r)
            reads.append((r, L.qual_string(rng, n) if rep != 3 else "*"))
    return genes, reads


@pytest.fixture(scope="module")
def anchored():
    return anchored_set()


def test_every_gene_a_candidate_equals_sc_align_reads(anchored):
    from rambl_amd import capi
    genes, reads = anchored
    cands = M.all_candidates(genes, [r for r, _ in reads], 16, E.BIG, 0, 1)
    assert all([g for g, _, _ in c] == list(range(len(genes))) for c in cands)
    assert sorted({(len(r) + 63) // 64 for r, _ in reads}) == list(range(1, 9))
    full = capi.align_reads(_b(genes), _b(r for r, _ in reads), _b(q for _, q in reads))
    with capi.MapIndex(_b(genes)) as ix:
        got = ix.map_reads(_b(r for r, _ in reads), _b(q for _, q in reads), max_occ=E.BIG, max_cand=0)
    for f in ("as_", "xs", "seed", "strand", "pos", "nm"):
        assert getattr(got, f).tolist() == getattr(full, f).tolist(), f
    assert got.cigar == full.cigar and got.n_cand.tolist() == [len(genes)] * len(reads)
    assert sum(1 for s in full.seed if s >= 0) >= 24 and {0, 1} <= set(full.strand.tolist()) and any("D" in c or "I" in c for c in full.cigar)


def test_read_order_and_repeated_calls_change_nothing(anchored):
    from rambl_amd import capi
    genes, reads = anchored
    seqs, quals = _b(r for r, _ in reads), _b(q for _, q in reads)
    with capi.MapIndex(_b(genes)) as ix:
        a = ix.map_reads(seqs, quals, max_cand=3)
        b = ix.map_reads(seqs[::-1], quals[::-1], max_cand=3)
        c = ix.map_reads(seqs, quals, max_cand=3, pair_room=7)
        small = ix.map_reads(seqs[:3], quals[:3], max_cand=3)
    assert M.device_rows(a) == M.device_rows(b)[::-1] == M.device_rows(c) and a.n_cand.tolist() == b.n_cand.tolist()[::-1] == c.n_cand.tolist()
    assert M.device_rows(small) == M.device_rows(a)[:3]
    assert c.stats.n_stretches > a.stats.n_stretches == 1 and a.n_cand.tolist() == [3] * len(reads)


def test_read_without_candidates_and_argument_errors():
    from rambl_amd import capi
    rng = random.Random(5)
    genes = [E.seq(rng, 200) for _ in range(3)]
    with capi.MapIndex(_b(genes)) as ix:
        got = ix.map_reads([E.seq(rng, 100).encode(), genes[1][20:120].encode(), b"ACGT"])
        assert M.device_rows(got)[0] == M.NO_ROW and M.device_rows(got)[2] == M.NO_ROW and got.gene.tolist() == [-1, 1, -1]
        assert ix.map_reads([]).cigar == []
        for bad in (dict(max_occ=0), dict(max_cand=-1), dict(min_votes=0)):
            with pytest.raises(capi.StrainCallError) as ei:
                ix.map_reads([b"ACGT" * 10], **bad)
            assert ei.value.code == capi.SC_ERR_ARG
        with pytest.raises(capi.StrainCallError) as ei:
            ix.map_reads([b"A" * 513])
        assert ei.value.code == capi.SC_ERR_UNSUPPORTED and "513" in str(ei.value)
    for genes_bad, k, code in (([b"A" * 8193], 16, capi.SC_ERR_UNSUPPORTED), ([b"ACGT" * 10], 10, capi.SC_ERR_ARG), ([b"ACGT" * 10], 17, capi.SC_ERR_ARG)):
        with pytest.raises(capi.StrainCallError) as ei:
            capi.MapIndex(genes_bad, k)
        assert ei.value.code == code


def paired_sample():
    """(gene names, genes, [(QNAME, [(seq, qual), (seq, qual)])]): pairs drawn from a family of related genes and from unrelated
    ones; some mates map nowhere, some pairs are turned round, one mate is too long to be mapped."""
    rng = random.Random(31)
    fam = E.seq(rng, 400)
    genes = [L.mutate(rng, fam, 0.05) for _ in range(4)] + [E.seq(rng, 350) for _ in range(3)]
    names = ["gene%d|x" % i for i in range(len(genes))]
    sample = []
    for i in range(40):
        g = genes[rng.randrange(len(genes))]
        a = rng.randrange(0, len(g) - 220)
        m1, m2 = L.mutate(rng, g[a:a + 100], 0.02), L.revcomp(L.mutate(rng, g[a + 120:a + 220], 0.02))
        if i % 7 == 3:
            m2 = E.seq(rng, 100)                                           # the mate maps nowhere
        if i % 11 == 5:
            m1, m2 = L.revcomp(m2), L.revcomp(m1)
        sample.append(("read%02d" % i, [(m1, L.qual_string(rng, 100)), (m2, L.qual_string(rng, 100, low=True))]))
    sample.append(("long", [("A" * 600, "I" * 600), (genes[0][10:110], "I" * 100)]))
    return names, genes, sample


def paired_rows(sw_check, genes, sample, max_cand):
    """The restatement's row per read entry of the sample, flattened; a read the mapper leaves out has no candidates."""
    flat = [m for _, mates in sample for m in mates]
    index = M.build_index(genes, 16)
    cands = [M.candidates(index, m[0], 16, 1024, max_cand, 1) if 1 <= len(m[0]) <= M.MAX_READ else [] for m in flat]
    return M.expected_rows(sw_check, genes, [m if 1 <= len(m[0]) <= M.MAX_READ else ("A", "I") for m in flat], cands)


def test_rambl_map_end_to_end(tmp_path, sw_check):
    """Paired FASTQ files through bin/rambl-map: the SAM opens with capi.NativeAln, is the restatement's byte for byte, and
    stage4.extract_reads pairs the mates again."""
    from rambl_amd import capi, stage4
    names, genes, sample = paired_sample()
    fa, r1, r2, out = (str(tmp_path / n) for n in ("genes.fa", "s_1.fastq.gz", "s_2.fastq", "s.sam"))
    open(fa, "w").write("".join(">%s some text\n%s\n%s\n" % (n, g[:70], g[70:]) for n, g in zip(names, genes)))
    import gzip
    open(r1, "wb").write(gzip.compress("".join("@%s/1 x\n%s\n+\n%s\n" % (q, m[0][0], m[0][1]) for q, m in sample).encode()))
    open(r2, "w").write("".join("@%s/2\n%s\n+\n%s\n" % (q, m[1][0], m[1][1]) for q, m in sample))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "bin", "rambl-map"), fa, "-1", r1, "-2", r2, "-o", out, "--max-cand", "3"])
    rows = paired_rows(sw_check, genes, sample, 3)
    want = M.sam_text(names, genes, sample, rows)
    assert open(out).read() == want
    mapped = [r for r in rows if r[2] >= 0]
    assert len(mapped) > 60 and any(r[3] for r in mapped) and rows[-2] == M.NO_ROW and rows[-1][2] == 0
    with capi.NativeAln(out) as aln:
        assert aln.records() == len(mapped)
        recs = list(aln.walk())
    again = dict(stage4.extract_reads(recs))
    both = [(q, mates) for (q, mates), k in zip(sample, range(0, len(rows), 2)) if rows[k][2] >= 0 and rows[k + 1][2] >= 0]
    assert len(both) > 20
    for q, mates in both:
        assert again[q.encode()] == [(s.encode(), ql.encode()) for s, ql in mates]
