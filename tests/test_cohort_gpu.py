"""GPU: a cohort against one resident gene index (sc_profile_index_* in rambl_amd/csrc/sc_profile.hip, the sample beside the
triples in sc_profile_counts.hpp).  The contract: per sample the rows are sc_profile_counts' triples for that
sample alone -- checked against capi.profile_counts and against the counting rule on the plain restatement's hits
(tests/count_lib.py) on the named inputs of tests/cohort_lib.py -- then the index kept across calls, the limits, and the
rambl-cohort command."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cohort_lib as HL
import count_lib as CL
import profile_lib as PL
from rambl_amd.capi import ProfileIndex  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("seeded", (False, True), ids=("unseeded", "seeded"))


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


def run(cohort, hits_check, seeded=False, **kw):
    cohort.check(cohort, hits_check)
    res = HL.device_counts(cohort, seeded=seeded, **kw)
    print("%s%s: %d rows, %s" % (cohort.name, " seeded" if seeded else "", len(res), res.stats.as_dict()))
    return res


@MODES
def test_mixture(seeded, hits_check):
    cohort = HL.cohort("mixture")
    res = run(cohort, hits_check, seeded)
    HL.compare_alone(cohort, res, seeded)
    for si in range(3):
        _, triples = CL.check_rules(CL.case("mixture_sample%d" % si), hits_check)
        HL.compare_rule(res, si, cohort.names, triples)
    assert res.stats.n_stretches == 1                                    # one stretch holds three samples
    assert res.stats.n_reads_counted == sum(HL.alone(cohort, si, seeded).stats.n_reads_counted for si in range(3)) > 900


@MODES
def test_seams(seeded, hits_check):
    cohort = HL.cohort("seams")
    whole = HL.device_counts(cohort, seeded=seeded)
    res = run(cohort, hits_check, seeded, cand_room=HL.SEAMS_ROOM)
    HL.compare_alone(cohort, res, seeded)
    assert res.rows == whole.rows and whole.stats.n_stretches == 1
    assert res.stats.n_stretches == len(cohort.plan(HL.SEAMS_ROOM))       # (a seeded call plans by the same tiles)
    tiny = HL.device_counts(cohort, seeded=seeded, cand_room=1)          # one read per stretch
    assert tiny.rows == whole.rows and tiny.stats.n_stretches == len(cohort.plan(1)) == cohort.first_read()[-1]


def test_same_names(hits_check):
    cohort = HL.cohort("same_names")
    res = run(cohort, hits_check)
    HL.compare_alone(cohort, res)
    one = HL.alone(cohort, 0).triples
    assert res.by_sample(0) == res.by_sample(1) == one and len(one) > 3
    # nothing merged across the samples: every row of sample 0 is there a second time with the same reads behind it, and
    # the reads that count are those of the three samples
    assert sum(r[4] for r in res.rows if r[0] == 0) == sum(r[4] for r in res.rows if r[0] == 1) == sum(t[3] for t in one)
    assert res.stats.n_reads_counted == 2 * HL.alone(cohort, 0).stats.n_reads_counted + HL.alone(cohort, 2).stats.n_reads_counted


@MODES
def test_gaps(seeded, hits_check):
    cohort = HL.cohort("gaps")
    res = run(cohort, hits_check, seeded)
    assert sorted({r[0] for r in res.rows}) == [0, 3] and res.stats.n_samples == 5
    HL.check_rows(res)
    for si, name in cohort.expected.items():
        _, triples = CL.check_rules(CL.case(name), hits_check)
        HL.compare_rule(res, si, cohort.names, triples)
        assert res.by_sample(si) == HL.alone(cohort, si, seeded).triples
    with ProfileIndex([g.encode() for g in cohort.genes]) as ix:         # an all-empty call
        none = ix.counts([], [], [], 5, seeded=seeded)
        assert none.rows == [] and none.stats.n_stretches == 0


@pytest.mark.parametrize("name", ("mates", "wide_tie", "strides"))
def test_edges_ride_along(name, hits_check):
    cohort = HL.cohort("ride_" + name)
    case = CL.case(name)
    full, triples = CL.check_rules(case, hits_check)
    res = run(cohort, hits_check)
    HL.check_rows(res)
    from rambl_amd import profile
    assert profile.counts_from_triples(res.by_sample(1), case.names) == full
    HL.compare_rule(res, 1, case.names, triples)
    assert res.by_sample(0) == HL.alone(cohort, 0).triples
    if name == "wide_tie":
        assert len(res.by_sample(1)) == 2050


def test_index_reuse(hits_check):
    a, b, k_a, k_b = HL.reuse_calls()
    b.check(b, hits_check)
    genes = [g.encode() for g in a.genes]
    fresh_a, fresh_b = HL.device_counts(a, seeded=True), HL.device_counts(b, seeded=True)
    assert fresh_a.stats.n_index_builds == 1 and fresh_a.stats.n_allocs > 0 and len(fresh_b) > 0
    with ProfileIndex(genes) as ix:
        assert ix.info() == {"n_genes": len(genes), "gene_bases": a.n_bases(), "cached_k": []}
        plain = HL.device_counts(a, ix)                                  # an unseeded call builds nothing
        assert plain.stats.n_index_builds == 0 and plain.stats.seed_k == 0 and ix.info()["cached_k"] == []
        first = HL.device_counts(a, ix, seeded=True)
        second = HL.device_counts(b, ix, seeded=True)
        third = HL.device_counts(a, ix, seeded=True)
        print("index reuse: %s" % [(r.stats.seed_k, r.stats.n_index_builds, r.stats.n_allocs, r.stats.index_ms) for r in (first, second, third)])
        assert [r.stats.seed_k for r in (first, second, third)] == [k_a, k_b, k_a]
        assert [r.stats.n_index_builds for r in (first, second, third)] == [1, 1, 0]
        assert third.stats.n_allocs == 0
        assert ix.info()["cached_k"] == sorted((k_a, k_b))
        assert first.rows == third.rows == fresh_a.rows and second.rows == fresh_b.rows and plain.rows == fresh_a.rows
        assert third.stats.n_gene_kmers == first.stats.n_gene_kmers == fresh_a.stats.n_gene_kmers > 0
    with pytest.raises(ValueError):
        ix.info()                                                        # closed
    with ProfileIndex(genes) as again:
        assert HL.device_counts(a, again, seeded=True).rows == fresh_a.rows


def _raw_call(ix, segs, seg_read, read_sample, n_samples, cap):
    """sc_profile_index_counts itself -> (rc, n_out, rows written, message)."""
    from rambl_amd import capi
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    sl = np.array([0] + [len(s) for s in segs], dtype=np.int64).cumsum()
    reads, samples = np.array(seg_read, dtype=np.int32), np.array(read_sample, dtype=np.int32)
    out = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(4)] + [np.zeros(max(cap, 1), dtype=np.int64)]
    n = C.c_long()
    rc = capi.lib().sc_profile_index_counts(ix._h, b"".join(segs), sl.ctypes.data_as(lp), len(segs), reads.ctypes.data_as(ip), len(samples),
                                            samples.ctypes.data_as(ip), n_samples, 95.0, 1e-10, 1.28, 0.46, 0, 0, out[0].ctypes.data_as(ip),
                                            out[1].ctypes.data_as(ip), out[2].ctypes.data_as(ip), out[3].ctypes.data_as(ip),
                                            out[4].ctypes.data_as(lp), cap, C.byref(n), None)
    rows = [tuple(int(a[k]) for a in out) for k in range(min(n.value, cap))]
    return rc, n.value, rows, capi.lib().sc_profile_error().decode()


def test_limits_and_arguments():
    from rambl_amd import capi
    case = CL.case("mates")
    genes, segs = [g.encode() for g in case.genes], [s.encode() for s in case.segs]
    seg_read = [0, 0, 1, 1, 2, 2, 3, 3, 3, 4]
    with ProfileIndex(genes) as ix:
        good = ix.counts(segs, seg_read, [0, 0, 1, 1, 1], 2)
        assert len(good) > 2
        rc, n, rows, msg = _raw_call(ix, segs, seg_read, [0, 1, 1, 0, 1], 2, 64)
        assert rc == -3 and "read 3 belongs to sample 0 after sample 1" in msg
        rc, n, rows, msg = _raw_call(ix, segs, seg_read, [0, 0, 1, 1, 2], 2, 64)
        assert rc == -3 and "read 4 belongs to sample 2 of 2" in msg
        for n_samples in (0, HL.MAX_SAMPLES + 1):
            rc, n, rows, msg = _raw_call(ix, segs, seg_read, [0] * 5, n_samples, 64)
            assert rc == -3 and "%d samples (1..65536 supported)" % n_samples in msg
        assert _raw_call(ix, segs, seg_read, [0, 0, 1, 1, HL.MAX_SAMPLES - 1], HL.MAX_SAMPLES, 64)[0] == 0
        rc, n, rows, msg = _raw_call(ix, segs, seg_read, [0, 0, 1, 1, 1], 2, len(good) - 1)
        assert rc == -5 and n == len(good) and "room for %d" % (len(good) - 1) in msg and rows == good.rows[:-1]
        rc, n, rows, msg = _raw_call(ix, segs, seg_read, [0, 0, 1, 1, 1], 2, n)
        assert rc == 0 and rows == good.rows
        assert ix.counts(segs, seg_read, [0, 0, 1, 1, 1], 2, cap=1).rows == good.rows          # the binding grows the room
        with pytest.raises(capi.StrainCallError) as e:
            ix.counts(segs + [b"C" * 513], seg_read + [4], [0, 0, 1, 1, 1], 2)
        assert e.value.code == -4 and "sc_profile_index_counts: segment %d has 513 bases (1..512 supported)" % len(segs) in str(e.value)
        assert ix.counts(segs, seg_read, [0, 0, 1, 1, 1], 2).rows == good.rows                   # the index is as it was
    with pytest.raises(capi.StrainCallError) as e:
        ProfileIndex(genes + [b"A" * 8193])
    assert e.value.code == -4 and "sc_profile_index_create: gene %d has 8193 bases (1..8192 supported)" % len(genes) in str(e.value)


def _read(*path):
    return open(os.path.join(*path), "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory, hits_check):
    """The mixture written as files with a gene more that no read hits, one plain run of the command, and the chain
    restatement's tables (computed once, the three samples side by side)."""
    from concurrent.futures import ThreadPoolExecutor
    from rambl_amd import cohort
    d = str(tmp_path_factory.mktemp("cohort_files"))
    names, seqs, samples = PL.mixture_dataset()
    names, seqs = names + ["unhit"], seqs + [CL.L.rand_seq(random.Random(12), 500)]
    fa, sams = PL.write_mixture(d, names, seqs, samples)
    listing = os.path.join(d, "samples.txt")
    open(listing, "w").write("".join(s + "\n\n" for s in sams))        # empty lines are skipped
    assert cohort.main([fa, listing, "-o", os.path.join(d, "plain"), "-v"]) == 0
    with ThreadPoolExecutor(3) as pool:
        expected = list(pool.map(lambda s: PL.expected_table(hits_check, names, seqs, s[0], s[1])[0], samples))
    return dict(d=d, fa=fa, sams=sams, listing=listing, names=names, order=[s for s, _, _ in samples], expected=expected)


def test_rambl_cohort_tables_and_matrix(files):
    from rambl_amd import cohort, profile
    d, order = files["d"], files["order"]
    tables = {}
    for sample, sam, expected in zip(order, files["sams"], files["expected"]):
        got = _read(d, "plain", sample + "_gene_count.tsv")
        profile.gene_profile(files["fa"], sam, sample, out_dir=os.path.join(d, "single"), counts_only=True)
        assert got == _read(d, "single", sample + "_gene_count.tsv")
        assert got.decode() == expected and got.count(b"\n") > 5
        tables[sample] = dict(ln.split("\t") for ln in got.decode().splitlines()[1:])
    want = "gene\t" + "\t".join(order) + "\n" + "".join(
        "%s\t%s\n" % (g, "\t".join(tables[s].get(g, "0.0") for s in order)) for g in sorted(files["names"], key=lambda n: n.encode()))
    matrix = _read(d, "plain", cohort.MATRIX_NAME).decode()
    assert matrix == want and "unhit\t0.0\t0.0\t0.0\n" in matrix
    assert len(os.listdir(os.path.join(d, "plain"))) == 4


def test_rambl_cohort_same_bytes_in_batches_seeded_and_named(files):
    from rambl_amd import cohort
    d = files["d"]
    named = os.path.join(d, "named.txt")
    open(named, "w").write("".join("%s\t%s\n" % (sam, s) for sam, s in zip(files["sams"], files["order"])))
    for out, args in (("one", ["--batch-segments", "1"]), ("seeded", ["--seeded"]), ("named", [])):
        assert cohort.main([files["fa"], named if out == "named" else files["listing"], "-o", os.path.join(d, out)] + args) == 0
        assert sorted(os.listdir(os.path.join(d, out))) == sorted(os.listdir(os.path.join(d, "plain")))
        for f in os.listdir(os.path.join(d, "plain")):
            assert _read(d, out, f) == _read(d, "plain", f), (out, f)
    open(named, "w").write("%s\tleft\n%s\tright\n" % tuple(files["sams"][:2]))      # other names: other files, the same counts
    assert cohort.main([files["fa"], named, "-o", os.path.join(d, "renamed")]) == 0
    assert sorted(os.listdir(os.path.join(d, "renamed"))) == sorted([cohort.MATRIX_NAME, "left_gene_count.tsv", "right_gene_count.tsv"])
    assert _read(d, "renamed", "right_gene_count.tsv") == _read(d, "plain", files["order"][1] + "_gene_count.tsv").replace(
        files["order"][1].encode(), b"right", 1)


def test_rambl_cohort_relative_and_copy_corrected(files):
    from rambl_amd import cohort, profile
    d, fa, sams, order, listing = (files[k] for k in ("d", "fa", "sams", "order", "listing"))
    # -r: relative tables, as rambl-profile writes them
    assert cohort.main([fa, listing, "-o", os.path.join(d, "rel"), "-r"]) == 0
    profile.gene_profile(fa, sams[1], order[1], relative=True, out_dir=os.path.join(d, "single_rel"), counts_only=True)
    rel = _read(d, "rel", order[1] + "_gene_count.tsv")
    assert rel == _read(d, "single_rel", order[1] + "_gene_count.tsv") and rel != _read(d, "plain", order[1] + "_gene_count.tsv")
    # --copy-correct against rambl-profile --counts --copy-correct
    fixrank = os.path.join(d, "genes_fixrank.txt")
    genera = ("Odoribacter", "Solibacillus", "Thiobacillus")           # 4, 12 and 2 copies in the table
    open(fixrank, "w").write("".join("%s\t\tBacteria\tdomain\t1.0\t%s\tgenus\t%s\n" % (n, genera[k % 3], "0.9" if k % 4 else "0.3")
                                     for k, n in enumerate(files["names"][:-2])))
    table = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taxa", "rrnDB_excerpt.tsv")
    extra = ["--copy-correct", fixrank, "--copy-number", table]
    assert cohort.main([fa, listing, "-o", os.path.join(d, "cc")] + extra) == 0
    for sample, sam in zip(order, sams):
        assert profile.main([fa, sam, sample, "--counts", "-o", os.path.join(d, "single_cc")] + extra) == 0
        assert _read(d, "cc", sample + "_gene_count.tsv") == _read(d, "single_cc", sample + "_gene_count.tsv")
    assert _read(d, "cc", order[0] + "_gene_count.tsv") != _read(d, "plain", order[0] + "_gene_count.tsv")
