"""GPU: gene against gene (rambl_amd/csrc/sc_pairs.hip).  Every named edge of tests/pair_lib.py through
sc_gene_distances and sc_gene_pairs against the plain restatement, exactly, the order of the list included; the limits and the
capacity answer; two calls alike; one run of bin/rambl-otu byte for byte; and rambl-cohort with and without --otu."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_lib as P
from rambl_amd import capi, otu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edges():
    found = P.distance_edges(tuple(otu.widths()))
    for e in found:
        e.check()
    return found


def test_every_distance_edge_in_one_call(edges):
    """All edges but the last as one call: tiles of every width class, full and ragged."""
    genes, pairs, want = P.flatten(edges[:-1])
    got, stats = otu.distances(genes, pairs, with_stats=True)
    print(stats)
    by_edge = iter(zip(got, want))
    for e in edges[:-1]:
        for (a, b), (g, w) in zip(e.pairs, by_edge):
            assert g == w, (e.name, len(e.genes[a]), len(e.genes[b]), g, w)
    assert stats["pairs_scored"] == len(pairs) and stats["tiles"] >= len({a for a, _ in pairs})
    assert stats["word_steps"] == sum(len(genes[b]) * ((len(genes[a]) + 63) // 64) for a, b in pairs)
    assert otu.distances(genes, pairs) == got          # two calls alike


@pytest.mark.parametrize("k", range(8))
def test_distance_edges_alone(edges, k):
    """The named edges an eighth at a time, each edge as its own call: an edge cannot lean on another's tile."""
    for e in edges[:-1][k::8]:
        assert otu.distances(e.genes, e.pairs) == e.expected(), e.name


def test_more_tiles_than_one_grid_trip(edges):
    e = edges[-1]
    assert e.name == "more tiles than one grid trip"
    got, stats = otu.distances(e.genes, e.pairs, with_stats=True)
    assert got == e.expected() and stats["tiles"] > P.GRID_TILES


def test_every_list_edge():
    for e in P.list_edges():
        e.check()
        got, stats = otu.pairs_within(e.genes, e.diff_num, e.diff_den, with_stats=True)
        assert got == e.expected(), e.name
        n = len(e.genes)
        lens = [len(g) for g in e.genes]
        assert stats["pairs_scored"] == len(P.candidates(lens, e.diff_num, e.diff_den)), e.name
        assert stats["pairs_scored"] + stats["pairs_skipped"] == n * (n - 1) // 2, e.name
        assert otu.pairs_within(e.genes, e.diff_num, e.diff_den) == got, e.name          # the same on every call


def _raw_pairs(genes, diff_num, diff_den, cap, n_stats=7):
    text, off = capi._pack_long(genes)
    cols = [np.full(max(cap, 1), -7, dtype=np.int32) for _ in range(3)]
    n, stats = C.c_long(-1), (C.c_double * 7)(*[-1.0] * 7)
    rc = capi.lib().sc_gene_pairs(0, text, capi._ptr(off), len(genes), diff_num, diff_den, *[capi._ptr(c) for c in cols], cap, C.byref(n), stats, n_stats)
    return rc, n.value, [tuple(int(c[k]) for c in cols) for k in range(max(0, min(cap, n.value)))], list(stats)


def test_capacity_is_answered_with_the_needed_count():
    e = P.list_edges()[4]                                       # 65 candidates
    want = e.expected()
    assert len(want) > 3
    rc, n, rows, stats = _raw_pairs(e.genes, e.diff_num, e.diff_den, len(want))
    assert rc == capi.SC_OK and n == len(want) and rows == want and min(stats) >= 0
    rc, n, _, _ = _raw_pairs(e.genes, e.diff_num, e.diff_den, len(want) - 1)
    assert rc == capi.SC_ERR_CAPACITY and n == len(want) and b"room for %d" % (len(want) - 1) in capi.lib().sc_pairs_error()
    rc, n, _, _ = _raw_pairs(e.genes, e.diff_num, e.diff_den, 0)
    assert rc == capi.SC_ERR_CAPACITY and n == len(want)
    assert otu.pairs_within(e.genes, e.diff_num, e.diff_den, cap=1) == want          # the binding grows the room
    rc, n, rows, stats = _raw_pairs(e.genes, e.diff_num, e.diff_den, len(want), n_stats=2)          # fewer slots: what fits
    assert rc == capi.SC_OK and rows == want and stats[0] >= 0 and stats[1] > 0 and stats[2:] == [-1.0] * 5


def test_limits_and_arguments():
    ok = [b"ACGT" * 512, b"ACGA"]
    assert otu.distances(ok, [(0, 1), (1, 0)]) == [P.edit_distance(*ok)] * 2
    for call in (lambda g: otu.distances(g, [(0, 1)]), lambda g: otu.pairs_within(g, 3, 100)):
        with pytest.raises(capi.StrainCallError) as e:
            call([b"ACGT", b"A" * 2049])
        assert e.value.code == capi.SC_ERR_UNSUPPORTED and "gene 1 has 2049 bases (1..2048 supported)" in str(e.value)
        with pytest.raises(capi.StrainCallError) as e:
            call([b"ACGT", b"", b"AC"])
        assert e.value.code == capi.SC_ERR_ARG and "gene 1 is empty" in str(e.value)
    with pytest.raises(capi.StrainCallError) as e:
        otu.distances(ok, [(0, 2)])
    assert e.value.code == capi.SC_ERR_ARG and "pair 0 names a gene outside 0..1" in str(e.value)
    for num, den in ((-1, 100), (3, 0), (101, 100)):
        with pytest.raises(capi.StrainCallError) as e:
            otu.pairs_within(ok, num, den)
        assert e.value.code == capi.SC_ERR_ARG
    assert otu.distances(ok, []) == [] and otu.pairs_within([], 3, 100) == [] and otu.pairs_within(ok[:1], 3, 100) == []
    assert otu.pairs_within([b"ACGTACGT", b"TTTTTTTT"], 1, 1) == [(0, 1, 6)]          # a rate of 1: everything qualifies


@pytest.fixture(scope="module")
def otu_files(tmp_path_factory):
    """About 40 synthetic genes in families with a small matrix, as files, and what the restatement writes for them at 97 %."""
    d = str(tmp_path_factory.mktemp("otu_files"))
    names, seqs = P.families(8166, 8, 5, 260, 7)
    seqs[3] = seqs[3][:100] + b"N" + seqs[3][101:]
    order = np.random.RandomState(8).permutation(len(names))
    names, seqs = [names[k] for k in order], [seqs[k].decode() for k in order]
    rng = np.random.RandomState(9)
    matrix = "gene\ts1\ts2\ts3\n" + "".join("%s\t%s\n" % (n, "\t".join(repr(float(v)) for v in rng.randint(0, 40, 3) / 8.0))
                                             for n in sorted(names, key=lambda n: n.encode()))
    fa, tsv = os.path.join(d, "genes.fa"), os.path.join(d, "gene_count_matrix.tsv")
    with open(fa, "w") as f:
        f.write("".join(">%s some description\n%s\n%s\n" % (n, s[:70], s[70:]) for n, s in zip(names, seqs)))
    with open(tsv, "w") as f:
        f.write(matrix)
    lengths = [len(s) for s in seqs]
    pairs = P.pairs_within([s.encode() for s in seqs], 3, 100)
    weights = P.row_weights(matrix, names)
    mapping = P.greedy_otus(names, lengths, weights, pairs)
    want = {otu.OTUS_NAME: P.otus_fasta_text(names, seqs, lengths, weights, mapping), otu.MAP_NAME: P.otu_map_text(names, lengths, mapping),
            otu.MATRIX_NAME: P.otu_matrix_text(matrix, mapping), otu.PAIRS_NAME: P.pairs_text(names, pairs)}
    plain = P.greedy_otus(names, lengths, [0] * len(names), pairs)
    return dict(d=d, fa=fa, tsv=tsv, want=want, n_otus=len({c for _, c, _ in mapping}), n=len(names),
                plain={otu.OTUS_NAME: P.otus_fasta_text(names, seqs, lengths, [0] * len(names), plain), otu.MAP_NAME: P.otu_map_text(names, lengths, plain)})


def _read_dir(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


def test_rambl_otu_end_to_end(otu_files):
    out = os.path.join(otu_files["d"], "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rambl-otu"), otu_files["fa"], "--matrix", otu_files["tsv"], "-o", out, "--pairs", "-v"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert _read_dir(out) == otu_files["want"]
    assert 8 <= otu_files["n_otus"] < otu_files["n"]            # the families merged, the input did not collapse
    plain = os.path.join(otu_files["d"], "plain")
    assert otu.main([otu_files["fa"], "--id", "97.0", "-o", plain]) == 0          # no matrix: every weight 0, two files
    assert _read_dir(plain) == otu_files["plain"]


def test_rambl_cohort_is_as_it_was_without_otu_and_adds_the_otu_files_with_it(tmp_path):
    import profile_lib as PL
    from rambl_amd import cohort, profile
    names, seqs, samples = PL.mixture_dataset()
    fa, sams = PL.write_mixture(tmp_path, names, seqs, samples)
    listing = str(tmp_path / "samples.txt")
    open(listing, "w").write("".join(s + "\n" for s in sams))
    assert cohort.main([fa, listing, "-o", str(tmp_path / "plain")]) == 0
    plain = _read_dir(str(tmp_path / "plain"))
    order = [s for s, _, _ in samples]
    assert sorted(plain) == sorted([cohort.MATRIX_NAME] + [s + "_gene_count.tsv" for s in order])          # what it writes today, and no more
    tables = []
    for sample, sam in zip(order, sams):
        profile.gene_profile(fa, sam, sample, out_dir=str(tmp_path / "single"), counts_only=True)
        tables.append(open(str(tmp_path / "single" / (sample + "_gene_count.tsv"))).read())
        assert plain[sample + "_gene_count.tsv"] == tables[-1]
    assert plain[cohort.MATRIX_NAME] == cohort.matrix_text(names, order, tables)
    assert cohort.main([fa, listing, "-o", str(tmp_path / "otu"), "--otu", "90"]) == 0
    with_otu = _read_dir(str(tmp_path / "otu"))
    assert {k: v for k, v in with_otu.items() if k in plain} == plain
    lengths, matrix = [len(s) for s in seqs], plain[cohort.MATRIX_NAME]
    weights = P.row_weights(matrix, names)
    mapping = P.greedy_otus(names, lengths, weights, P.pairs_within([s.encode() for s in seqs], 10, 100))
    assert {k: v for k, v in with_otu.items() if k not in plain} == {
        otu.OTUS_NAME: P.otus_fasta_text(names, seqs, lengths, weights, mapping), otu.MAP_NAME: P.otu_map_text(names, lengths, mapping),
        otu.MATRIX_NAME: P.otu_matrix_text(matrix, mapping)}
    assert len({c for _, c, _ in mapping}) < len(names)
