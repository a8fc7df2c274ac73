"""GPU: the genus assignment on the device (rambl_amd/csrc/sc_taxa.hip) against the plain restatement of DESIGN.md §8.12 in
tests/taxa_lib.py: counts and table cell for cell (exactly, against the table computed with mpmath: every case keeps its
cells beyond the fp64 error bound of a half-integer, and one case puts cells within 1e-7 of one), assigned genus and trial
winners, the limits, and the command lines byte for byte.  The named edge cases of the word, table and score kernels are
in taxa_lib with their property checks.

Not reached: the second batch of sc_taxa_classify (q0 > 0).  A batch holds PART_ROOM = 2^25 (query, chunk, slot) records, so
a second one needs some 16 384 genera, a 4 GiB table, while PART_ROOM is a constant of the library."""
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
        with pytest.raises(capi.StrainCallError) as ei:
            dev.classify([b"ACGTACGTAC"], [1], n_trials=1025)
        assert ei.value.code == -4 and "1025 trials (1..1024 supported)" in str(ei.value)
        with pytest.raises(capi.StrainCallError) as ei:
            dev.classify([b"ACGTACGTAC", b""], [1, 2])
        assert ei.value.code == -4 and "query 1 has 0 bases (1..8192 supported)" in str(ei.value)
        best, winners, words, _ = dev.classify([b"A" * 8192], [1])
        assert int(best[0]) in (0, 1) and int(words[0]) == 8185 and winners.shape == (1, 100)


# ---- named edge cases (taxa_lib holds them with their property checks) --------------------------------------------------------

_ONCE = {}


def _once(name, make):
    """A case or an expected result, built once for the tests that read it."""
    if name not in _ONCE:
        _ONCE[name] = make()
    return _ONCE[name]


@pytest.fixture(scope="module", autouse=True)
def _shared_cases_end_with_this_module():
    yield
    _ONCE.clear()
    T.forget_models()


@pytest.mark.parametrize("grid_cap", [0, 1])
def test_table_cells_next_to_a_half_integer(grid_cap):
    """Cells 1e-9 .. 3e-8 from a half-integer, one rounding down and two up, equal to the exact table; 128 workgroups (or one,
    128 times) add to one cell."""
    for mo in _once("near_half", T.near_half_case):
        with _train(mo, grid_cap, keep_counts=True) as dev:
            _check_model(dev, mo)


@pytest.mark.parametrize("grid_cap", [0, 1])
def test_word_kernel_lane_seams(grid_cap):
    """grid_cap 1: one workgroup takes every sequence in turn, the shortest right after the longest."""
    mo = _once("seam", T.seam_case)
    with _train(mo, grid_cap, keep_counts=True) as dev:
        _check_model(dev, mo)


def test_training_text_at_an_offset():
    """sc_taxa_train with seq_off[0] = 5 and 5 bases in front of the text gives the counts and the table of the call from 0."""
    import ctypes as C
    from rambl_amd import capi
    mo = _once("seam", T.seam_case)
    text = (T.SEAM_JUNK + "".join(mo.seqs)).encode()
    off = np.array([0] + [len(s) for s in mo.seqs], dtype=np.int64).cumsum() + len(T.SEAM_JUNK)
    assert off[0] == 5 and text[:off[1] - 5] != mo.seqs[0].encode() and text[off[0]:off[1]] == mo.seqs[0].encode()
    gi = np.ascontiguousarray(mo.genus, dtype=np.int32)
    dev = capi.TaxaModel.__new__(capi.TaxaModel)
    dev.n_genera, dev._h, dev.stats = mo.G, C.c_void_p(), capi.ScTaxaStats()
    rc = capi.lib().sc_taxa_train(0, text, off.ctypes.data_as(C.POINTER(C.c_long)), mo.N, gi.ctypes.data_as(C.POINTER(C.c_int)), mo.G, 0, 1,
                                  C.byref(dev._h), C.byref(dev.stats))
    assert rc == 0, capi.lib().sc_taxa_error().decode()
    with dev:
        _check_model(dev, mo)


@pytest.mark.parametrize("G", [1, 2, 2 * T.CHUNK, 2 * T.CHUNK + 1])
def test_winners_by_genera_count(G):
    """One and two live lanes in a chunk, exactly two chunks, a third with one live lane."""
    mo = T.shared_model(G)
    qs = T.genera_queries(mo)
    exp = _expected(mo, qs, SEED)
    names = [n for n, _ in qs]
    assert exp[names.index("last")][0] == G - 1 and exp[names.index("middle")][0] == G // 2 and exp[names.index("w0")] == (-1, [-1] * 100, 0)
    with _train(mo) as dev:
        for grid_cap in (0, 1):
            assert _classify(dev, qs, SEED, grid_cap=grid_cap) == exp, grid_cap


def test_ties_and_winners_over_four_chunks():
    G = 3 * T.CHUNK + 1
    mo = T.shared_model(G, T.TWINS3)
    qs = T.genera_queries(mo, T.TWINS3)
    exp = _expected(mo, qs, SEED)
    res = dict((n, r) for (n, _), r in zip(qs, exp))
    for a in (3, 5, 80, 130):                                   # chunks 0 = 1 = 2; 0 = 2; 1 = 2; inside chunk 2: the lowest genus, in every trial
        assert res["tie%d" % a][0] == a and set(res["tie%d" % a][1]) == {a}
    assert res["middle"][0] == G // 2 and (G // 2) // T.CHUNK == 1 and res["last"][0] == G - 1 == 192 and res["first"][0] == 0
    with _train(mo) as dev:
        for grid_cap in (0, 1):
            assert _classify(dev, qs, SEED, grid_cap=grid_cap) == exp, grid_cap


def test_query_lengths_in_one_call():
    """W = 2 .. 8 and around 256 and 1 024 words, the W = 0 queries and the longest query in one call; the decisive queries
    lose their winner with a single word."""
    mo = T.shared_model(70, T.TWINS)
    qs = _once("lengths", lambda: T.lengths_case(mo))
    exp = _once("lengths_exp", lambda: _expected(mo, qs, SEED))
    for (name, _), (best, winners, W) in zip(qs, exp):
        if name[0] == "d":
            assert W == int(name[1:].split("_")[0]) and best > 0 and best in winners and set(winners) <= {0, best}, name
    assert [r[2] for (n, _), r in zip(qs, exp) if n in ("w0_short", "long", "w0_n")] == [0, 8185, 0]
    # grid_cap 1: one workgroup makes every (query, chunk) trip, query after query within a chunk, so in both chunks the 2 words
    # of "d2_1" are staged right after the 8 185 of "long"
    n_chunks = (mo.G + T.CHUNK - 1) // T.CHUNK
    names = [n for n, _ in qs]
    assert n_chunks == 2 and n_chunks * len(qs) == 66 and names[names.index("long") + 1] == "d2_1"
    assert exp[names.index("long")][2] == 8185 and exp[names.index("d2_1")][2] == 2
    with _train(mo) as dev:
        for grid_cap in (0, 1):
            got = _classify(dev, qs, SEED, grid_cap=grid_cap)
            for (name, _), g, e in zip(qs, got, exp):
                assert g == e, (name, grid_cap)


def test_trial_counts_around_the_wavefronts():
    """2 .. 8 trials: wavefronts without a trial, and with one more than their neighbour."""
    mo = T.shared_model(70, T.TWINS)
    qs = T.score_queries(mo, T.TWINS)
    with _train(mo) as dev:
        for n_trials in (2, 3, 4, 5, 7, 8):
            exp = _expected(mo, qs, SEED, n_trials)
            assert all(len(r[1]) == n_trials for r in exp)
            for grid_cap in (0, 1):
                assert _classify(dev, qs, SEED, n_trials, grid_cap) == exp, (n_trials, grid_cap)


def test_most_trials_and_most_draws():
    """1 024 trials of 5, 6 and 1 023 draws: the largest t * 65536 + j + 1."""
    mo = T.shared_model(70, T.TWINS)
    qs = T.max_trials_queries(mo)
    exp = _expected(mo, qs, SEED, 1024)
    assert [r[2] for r in exp] == [1, 48, 8185] and len(set(exp[2][1])) > 1 and len(set(exp[2][1][-4:] + exp[1][1][-4:])) > 1
    with _train(mo) as dev:
        for grid_cap in (0, 1):
            got = _classify(dev, qs, SEED, 1024, grid_cap)
            for (name, _), g, e in zip(qs, got, exp):
                assert g == e, (name, grid_cap)


def test_keys_and_seeds_at_the_ends_of_64_bits():
    mo = T.shared_model(70, T.TWINS)
    qs = T.score_queries(mo, T.TWINS)
    exp = _once("keys", lambda: T.keys_case(mo, qs))
    with _train(mo) as dev:
        for name, key, seed in T.KEY_SEEDS:
            keys = [T.fnv1a64(n.encode()) if key is None else key for n, _ in qs]
            for grid_cap in (0, 1):
                best, winners, words, _ = dev.classify([s.encode() for _, s in qs], keys, seed, 100, grid_cap)
                got = [(int(best[i]), [int(w) for w in winners[i]], int(words[i])) for i in range(len(qs))]
                assert got == exp[name], (name, grid_cap)


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
