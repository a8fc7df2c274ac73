"""GPU: the genus assignment on the device (rambl_amd/csrc/sc_taxa.hip) against the plain restatement of DESIGN.md §8.12 in
tests/taxa_lib.py: counts and table cell for cell (exactly: every case keeps its cells off the half-integers), assigned
genus and trial winners, the limits, and the command lines byte for byte."""
import os

import numpy as np
import pytest

import taxa_lib as T

pytestmark = pytest.mark.gpu

SEED = 20240


def _train(mo, grid_cap=0, keep_counts=False):
    from rambl_amd import capi
    return capi.TaxaModel([s.encode() for s in mo.seqs], mo.genus, mo.G, grid_cap=grid_cap, keep_counts=keep_counts)


def _check_model(dev, mo):
    for g in range(mo.G):
        m, n = dev.counts(g)
        assert (n.astype(np.int64) == mo.n).all(), "n"
        assert (m.astype(np.int64) == mo.m[:, g]).all(), "m of genus %d" % g
        assert (dev.table(g).astype(np.int64) == mo.q[:, g]).all(), "q of genus %d" % g
    st = dev.stats
    assert st.n_seqs == mo.N and st.n_genera == mo.G and st.n_words == int(mo.n.sum()) and st.table_bytes == 65536 * mo.G * 4


@pytest.mark.parametrize("grid_cap", [0, 2])
def test_counts_and_table(grid_cap):
    mo = T.counts_case()
    with _train(mo, grid_cap, keep_counts=True) as dev:
        _check_model(dev, mo)


def test_counts_second_trip():
    mo = T.second_trip_case()
    assert mo.N == 5
    with _train(mo, 2, keep_counts=True) as dev:
        _check_model(dev, mo)


def test_counts_are_kept_on_request_only():
    """Without keep_counts the counts are gone (the table replaces them in place) and the table is the same."""
    from rambl_amd import capi
    mo = T.second_trip_case()
    with _train(mo) as dev:
        with pytest.raises(capi.StrainCallError) as ei:
            dev.counts(0)
        assert ei.value.code == -4 and "keep_counts" in str(ei.value)
        for g in range(mo.G):
            assert (dev.table(g).astype(np.int64) == mo.q[:, g]).all()


def _expected(mo, qs, seed, n_trials=100):
    return [T.classify(mo.q, s, T.fnv1a64(n.encode()), seed, n_trials) for n, s in qs]


def _classify(dev, qs, seed, n_trials=100, grid_cap=0):
    best, winners, words, st = dev.classify([s.encode() for _, s in qs], [T.fnv1a64(n.encode()) for n, _ in qs], seed, n_trials, grid_cap)
    assert st.n_seqs == len(qs) and st.n_words == int(words.sum())
    return [(int(best[i]), [int(w) for w in winners[i]], int(words[i])) for i in range(len(qs))]


@pytest.mark.parametrize("G", [T.CHUNK - 1, T.CHUNK, T.CHUNK + 1])
def test_winners_around_the_chunk_size(G):
    mo = T.score_model(G)
    qs = T.score_queries(mo)
    exp = _expected(mo, qs, SEED)
    names = [n for n, _ in qs]
    assert exp[names.index("last_genus")][0] == G - 1           # the last genus of the last chunk wins
    assert exp[names.index("w0_short")] == (-1, [-1] * 100, 0)
    with _train(mo) as dev:
        assert (dev.table(G - 1).astype(np.int64) == mo.q[:, G - 1]).all()
        assert _classify(dev, qs, SEED) == exp
        # grid_cap 2: 12 queries x the chunks and 12 x 101 slots are more than 2 blocks of either loop
        assert len(qs) * 101 > 2 * 256
        assert _classify(dev, qs, SEED, grid_cap=2) == exp


def test_ties_permutation_seeds_and_one_trial():
    mo = T.score_model(70, twins=T.TWINS)
    qs = T.score_queries(mo, T.TWINS)
    exp = _expected(mo, qs, SEED)
    for a, b in T.TWINS:                                        # a tie in the full score and in every trial, across chunks and inside one
        tie = exp[[n for n, _ in qs].index("tie%d" % a)]
        assert tie[0] == a and set(tie[1]) == {a}
    with _train(mo) as dev:
        assert _classify(dev, qs, SEED) == exp
        # the same queries permuted and split over two calls give the same rows
        perm = qs[::-1]
        got = _classify(dev, perm[:5], SEED) + _classify(dev, perm[5:], SEED)
        assert got[::-1] == exp
        # another seed: other draws somewhere, the same assignment
        other = _classify(dev, qs, SEED + 1)
        assert other == _expected(mo, qs, SEED + 1)
        assert [r[0] for r in other] == [r[0] for r in exp] and [r[1] for r in other] != [r[1] for r in exp]
        assert _classify(dev, qs, SEED, n_trials=1) == _expected(mo, qs, SEED, 1)


def test_longest_query_against_the_largest_cells():
    mo, query = T.bound_case()
    qs = [("long", query), ("long_too", query[:8191] + "A")]
    with _train(mo, keep_counts=True) as dev:
        _check_model(dev, mo)
        assert _classify(dev, qs, SEED) == _expected(mo, qs, SEED)


def test_limits():
    from rambl_amd import capi
    with pytest.raises(capi.StrainCallError) as ei:
        capi.TaxaModel([b"ACGTACGTAC"], [0], 16385)
    assert ei.value.code == -4 and "16385 genera" in str(ei.value)
    with pytest.raises(capi.StrainCallError) as ei:
        capi.TaxaModel([], [], 2)
    assert ei.value.code == -4 and "0 training sequences" in str(ei.value)
    for bad in (2, -1):
        with pytest.raises(capi.StrainCallError) as ei:
            capi.TaxaModel([b"ACGTACGTAC", b"ACGTACGTAC"], [0, bad], 2)
        assert ei.value.code == -4 and "has genus %d" % bad in str(ei.value)
    with capi.TaxaModel([b"ACGTACGTAC", b"GGGTACGTAC"], [0, 1], 2) as dev:
        with pytest.raises(capi.StrainCallError) as ei:
            dev.classify([b"ACGTACGTAC", b"A" * 8193], [1, 2])
        assert ei.value.code == -4 and "query 1 has 8193 bases" in str(ei.value)
        with pytest.raises(capi.StrainCallError) as ei:
            dev.classify([b"ACGTACGTAC"], [1], n_trials=0)
        assert ei.value.code == -4
        best, winners, words, _ = dev.classify([b"ACGTACGTAC"], [1])
        assert int(best[0]) == 0 and int(words[0]) == 3


def test_classify_command_line(tmp_path):
    from rambl_amd import taxa
    train_fa, train_tax, genes, genera, mo, gene_names, gene_seqs = T.cli_case()
    for name, text in (("train.fa", train_fa), ("train.tax", train_tax), ("genes.fasta", genes)):
        (tmp_path / name).write_text(text)
    out = tmp_path / "out"
    assert taxa.main(["classify", str(tmp_path / "genes.fasta"), "--train-seq", str(tmp_path / "train.fa"), "--train-tax", str(tmp_path / "train.tax"),
                      "-o", str(out), "--seed", "7"]) == 0
    exp = T.fixrank_text(gene_names, [T.classify(mo.q, s, T.fnv1a64(n.encode()), 7) for n, s in zip(gene_names, gene_seqs)], genera)
    assert (out / "genes_fixrank.tsv").read_text() == exp
    assert exp.splitlines()[-1] == "gene_blank\t" and exp.count("\tgenus\t") == 7


def test_copy_correction_and_taxon_table_on_a_sample(tmp_path):
    """The mixture's first sample: the nine assembled genes classified against themselves (one genus per gene, its three
    strains the training set), then `rambl-profile --copy-correct` and `rambl-taxa table`: the restatement's files, and the
    uncorrected file as it was."""
    import profile_lib as PL
    from rambl_amd import profile, taxa
    names, seqs, samples = PL.mixture_dataset()
    fa, sams = PL.write_mixture(tmp_path, names, seqs, samples)
    paths = [("Bacteria", "P%d" % (k % 2), "C", "O", "F%d" % k, "Genus %d" % k) for k in range(3)]
    (tmp_path / "train.tax").write_text("".join("%s\t%s\n" % (n, ";".join(paths[i // 3])) for i, n in enumerate(names)))
    (tmp_path / "copy.tsv").write_text("name\tmean\nGenus 0\t2.0\nF1\t3.0\nP0\t5.0\nGenus 0\t9.0\n")
    out = str(tmp_path / "out")
    assert taxa.main(["classify", fa, "--train-seq", fa, "--train-tax", str(tmp_path / "train.tax"), "-o", out]) == 0
    fixrank = os.path.join(out, "assembly_fixrank.tsv")
    genera = sorted(paths)                                      # genera are numbered in the order of their paths: Genus 2 (P0) before Genus 1 (P1)
    assert genera != paths
    mo = T.Model(seqs, [genera.index(paths[i // 3]) for i in range(9)], 3)
    text = T.fixrank_text(names, [T.classify(mo.q, s, T.fnv1a64(n.encode()), 0) for n, s in zip(names, seqs)], genera)
    assert open(fixrank).read() == text
    sample, lines, _ = samples[0]
    exe = PL.build_hits_check(tmp_path)
    plain, counts = PL.expected_table(exe, names, seqs, sample, lines)
    assert profile.main([fa, sams[0], sample, "-o", out]) == 0
    table = os.path.join(out, sample + "_gene_count.tsv")
    assert open(table).read() == plain
    # the taxon table from the uncorrected counts
    cn = {"Genus 0": 2.0, "F1": 3.0, "P0": 5.0}
    assert taxa.main(["table", fixrank, fa, table, sample, "--copy-number", str(tmp_path / "copy.tsv"), "-o", out]) == 0
    rows = T.ref_taxa_table(text, dict(zip(names, map(len, seqs))), T.ref_read_gene_counts(plain), cn, "genus", 0.6)
    assert [t for t, _ in rows] == ["Genus 0", "Genus 1", "Genus 2"]
    assert open(os.path.join(out, sample + "_taxa_count.tsv")).read() == "sample\t%s\n" % sample + "".join("%s\t%r\n" % r for r in rows)
    # the corrected gene table on every path: genus 0 by its own row, genus 1 by its family's, genus 2 by its phylum's
    corr = T.ref_copy_correct(counts, T.ref_parse_gene_lineage(text, 0.6), cn)
    assert sorted(counts) == sorted(names)
    assert [round(float(counts[n]) / corr[n], 9) for n in names] == [2.0] * 3 + [3.0] * 3 + [5.0] * 3
    exp = profile.format_table(sample, sorted(corr.items(), key=lambda kv: kv[0].encode()))
    for extra in ([], ["--seeded"], ["--counts"]):
        cdir = os.path.join(out, "corrected" + "".join(extra))
        assert profile.main([fa, sams[0], sample, "-o", cdir, "--copy-correct", fixrank, "--copy-number", str(tmp_path / "copy.tsv")] + extra) == 0
        assert open(os.path.join(cdir, sample + "_gene_count.tsv")).read() == exp
    assert open(table).read() == plain
