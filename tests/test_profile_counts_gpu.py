"""GPU: the counts mode of the gene profile (sc_profile_counts: k_cnt_* around k_bl_score / k_bl_trace in
rambl_amd/csrc/sc_profile_counts.hpp) against the counting rule on the plain restatement's hits
(tests/count_lib.py): exact Fractions and equal triples, unseeded and seeded, on the data sets and on every named edge."""
import os
import random

import pytest

import count_lib as CL
import profile_lib as PL
from rambl_amd.capi import profile_counts, profile_evalue6  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("seeded", (False, True), ids=("unseeded", "seeded"))


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@MODES
@pytest.mark.parametrize("name", CL.DATASETS)
def test_data_set(name, seeded, hits_check):
    res = CL.compare_device(CL.case(name), hits_check, seeded)
    assert res.stats.n_stretches == 1 and res.stats.n_traced <= res.stats.n_candidates


@MODES
@pytest.mark.parametrize("name", sorted(CL.NAMED))
def test_named_case(name, seeded, hits_check):
    res = CL.compare_device(CL.case(name), hits_check, seeded)
    st = res.stats
    # (seeded, a pair that fails -I may share no k-mer and never be scored: fewer pairs, never more)
    if name == "deep_groups":
        assert st.n_rounds == CL.COUNT_ROUNDS + 1                                     # the tail traces what is left at once
        assert st.n_traced <= 10 if seeded else st.n_traced == 10
    if name == "advance":
        assert st.n_rounds == 2 and (st.n_traced <= 4 if seeded else st.n_traced == 4)
    if name == "strides":
        assert st.n_traced > CL.REC_BLOCKS * 256 and st.n_reads_counted > CL.READ_BLOCKS
    if name == "wide_tie":
        assert len(res) == 2050 and st.n_reads_counted == 2


@MODES
def test_stretches(seeded, hits_check):
    case = CL.case("parity")
    whole = CL.device_counts(case, seeded)
    room = 2 * len(case.genes) * len(case.segs) // 4
    parts = CL.compare_device(case, hits_check, seeded, cand_room=room)
    assert parts.triples == whole.triples and parts.stats.n_stretches >= 3 and whole.stats.n_stretches == 1
    assert parts.stats.n_traced == whole.stats.n_traced and parts.stats.n_candidates == whole.stats.n_candidates
    if seeded:
        k = parts.stats.seed_k
        assert k == whole.stats.seed_k == 13 and parts.stats.n_pairs == whole.stats.n_pairs
        assert parts.stats.n_gene_kmers == whole.stats.n_gene_kmers == sum(
            sum(1 for p in range(len(g) - k + 1) if set(g[p:p + k]) <= set("ACGT")) for g in case.genes)
    # one read per stretch when the room holds no more
    tiny = CL.device_counts(case, seeded, cand_room=1)
    assert tiny.triples == whole.triples and tiny.stats.n_stretches > 100


@MODES
def test_one_score_pass_behind_every_entry_point(seeded):
    """The hit list's and the counts' entry points score the same tiles: equal statistics of the score pass on the same input,
    in one stretch and summed over three or more."""
    from rambl_amd import capi
    case = CL.case("parity")
    hits = capi.profile_hits([g.encode() for g in case.genes], [s.encode() for s in case.segs], *case.thresholds, seeded=seeded).stats
    fields = ("n_tiles", "n_candidates", "score_cells") + (("seed_k", "n_pairs", "n_gene_kmers") if seeded else ())
    expected = [getattr(hits, f) for f in fields]
    print("hits%s: %s" % (" seeded" if seeded else "", dict(zip(fields, expected))))
    assert hits.n_tiles > 0 and hits.n_candidates > 0 and (not seeded or hits.seed_k == 13)
    whole = CL.device_counts(case, seeded).stats
    parts = CL.device_counts(case, seeded, cand_room=2 * len(case.genes) * len(case.segs) // 4).stats
    assert whole.n_stretches == 1 and parts.n_stretches >= 3
    assert [getattr(whole, f) for f in fields] == expected
    assert [getattr(parts, f) for f in fields] == expected


def test_capacity_reaches_the_binding_and_grows(hits_check):
    from rambl_amd import capi, profile
    case = CL.case("mates")
    whole = CL.compare_device(case, hits_check)
    assert len(whole) > 1 and CL.device_counts(case, cap=1).triples == whole.triples
    # the library itself: SC_ERR_CAPACITY with the number that suffices
    import ctypes as C
    import numpy as np
    gl = np.array([0] + [len(g) for g in case.genes], dtype=np.int64).cumsum()
    sl = np.array([0] + [len(s) for s in case.segs], dtype=np.int64).cumsum()
    reads = np.array(profile.read_index(case.ids)[0], dtype=np.int32)
    out = [np.zeros(1, dtype=np.int32) for _ in range(3)] + [np.zeros(1, dtype=np.int64)]
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    n = C.c_long()
    rc = capi.lib().sc_profile_counts(0, "".join(case.genes).encode(), gl.ctypes.data_as(lp), len(case.genes), "".join(case.segs).encode(),
                                      sl.ctypes.data_as(lp), len(case.segs), reads.ctypes.data_as(ip), int(reads.max()) + 1, 95.0, 1e-10, 1.28,
                                      0.46, 0, 0, out[0].ctypes.data_as(ip), out[1].ctypes.data_as(ip), out[2].ctypes.data_as(ip),
                                      out[3].ctypes.data_as(lp), 1, C.byref(n), None)
    assert rc == -5 and n.value == len(whole) and "room for 1" in capi.lib().sc_profile_error().decode()
    assert (int(out[0][0]), int(out[1][0]), int(out[2][0]), int(out[3][0])) == whole.triples[0]


@MODES
def test_empties(seeded):
    from rambl_amd import capi
    rng = random.Random(3)
    genes = [CL.L.rand_seq(rng, 300).encode() for _ in range(3)]
    res = capi.profile_counts(genes, [CL.L.rand_seq(rng, n).encode() for n in (60, 150, 20)], [0, 0, 1], seeded=seeded)
    assert res.triples == [] and res.stats.n_traced == 0 and res.stats.n_reads_counted == 0
    res = capi.profile_counts(genes, [], [], seeded=seeded)
    assert res.triples == [] and res.stats.n_stretches == 0


@pytest.mark.parametrize("what,n", (("segment", 513), ("gene", 8193)))
def test_lengths_outside_the_limits(what, n):
    from rambl_amd import capi
    genes, segs = [b"ACGT" * 50], [b"ACGT" * 20, b"A" * 30]
    if what == "gene":
        genes.append(b"A" * n)
    else:
        segs.append(b"C" * n)
    with pytest.raises(capi.StrainCallError) as e:
        capi.profile_counts(genes, segs, list(range(len(segs))))
    assert e.value.code == -4 and "sc_profile_counts: %s %d has %d bases" % (what, len(genes if what == "gene" else segs) - 1, n) in str(e.value)


@MODES
def test_segment_order_does_not_matter(seeded):
    from rambl_amd import capi, profile
    case = CL.case("parity")
    genes, segs = [g.encode() for g in case.genes], [s.encode() for s in case.segs]
    reads, _ = profile.read_index(case.ids)
    first = capi.profile_counts(genes, segs, reads, seeded=seeded)
    order = list(range(len(segs)))
    random.Random(5).shuffle(order)
    again = capi.profile_counts(genes, [segs[k] for k in order], [reads[k] for k in order], seeded=seeded)
    assert len(first) > 10 and again.triples == first.triples and again.stats.n_traced == first.stats.n_traced


@MODES
def test_the_saving_is_real(seeded, hits_check):
    from rambl_amd import capi
    case = CL.case("conserved")
    res = CL.compare_device(case, hits_check, seeded)
    hits = capi.profile_hits([g.encode() for g in case.genes], [s.encode() for s in case.segs], seeded=seeded)
    print("conserved: counts traced %d, hits traced %d" % (res.stats.n_traced, hits.stats.n_traced))
    assert hits.stats.n_traced > 10 * len(case.segs) and 2 * res.stats.n_traced < hits.stats.n_traced


def test_command_line_counts_writes_the_same_table(tmp_path):
    from rambl_amd import profile
    names, seqs, samples = PL.mixture_dataset()
    fa, sams = PL.write_mixture(tmp_path, names, seqs, samples)
    for k, ((sample, _, _), sam) in enumerate(zip(samples, sams)):
        extra = ["-r"] if k == 1 else []
        runs = (([], "plain"), (["--counts"], "counts"), (["--counts", "--seeded", "-v"], "both"))
        for flags, out in runs:
            assert profile.main([fa, sam, sample, "-n", "-o", os.path.join(str(tmp_path), out)] + extra + flags) == 0
        want = open(os.path.join(str(tmp_path), "plain", sample + "_gene_count.tsv"), "rb").read()
        assert want.count(b"\n") > 5
        for _, out in runs[1:]:
            assert open(os.path.join(str(tmp_path), out, sample + "_gene_count.tsv"), "rb").read() == want
            assert not os.path.exists(os.path.join(str(tmp_path), out, sample + "_hits.csv"))
    with pytest.raises(SystemExit) as e:
        profile.main([fa, sams[0], "s", "--counts", "--keep-hits"])
    assert e.value.code == 2


def test_faults_come_in_order_and_leave_nothing_behind():
    """Which fault a call with several reports -- a missing argument before seg_read, seg_read before the genes' lengths, those
    before the segments' -- and that a call without a segment returns nothing with zeroed statistics: through the library
    itself, without an index and on one, and a good call on that index after the failed ones."""
    import ctypes as C
    import numpy as np
    from rambl_amd import capi
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    rng = random.Random(8)
    genes = [CL.L.rand_seq(rng, 40).encode() for _ in range(2)]
    segs = [genes[0][:30], genes[1][5:35], genes[1][10:40]]
    long_gene, long_seg = b"A" * 8193, b"C" * 513

    def call(ix, genes, segs, seg_read, with_gene=True):
        """sc_profile_counts, or sc_profile_index_counts on ix with every read in sample 0 of 1 -> (rc, rows, message, stats)."""
        offs = [np.array([0] + [len(s) for s in seqs], dtype=np.int64).cumsum() for seqs in (genes, segs)]
        reads, samples = np.array(seg_read, dtype=np.int32), np.zeros(2, dtype=np.int32)
        out = [np.zeros(8, dtype=np.int32) for _ in range(4)] + [np.zeros(8, dtype=np.int64)]
        n = C.c_long(-1)
        stats = capi.ScProfileCountStats() if ix is None else capi.ScProfileCohortStats()
        C.memset(C.byref(stats), 0xFF, C.sizeof(stats))
        head = (0, b"".join(genes), offs[0].ctypes.data_as(lp), len(genes)) if ix is None else (ix._h,)
        who = (reads.ctypes.data_as(ip), 2) + (() if ix is None else (samples.ctypes.data_as(ip), 1))
        rows = ([] if ix is None else [out[0].ctypes.data_as(ip)]) + [out[1].ctypes.data_as(ip) if with_gene else None] + \
               [out[2].ctypes.data_as(ip), out[3].ctypes.data_as(ip), out[4].ctypes.data_as(lp)]
        fn = capi.lib().sc_profile_counts if ix is None else capi.lib().sc_profile_index_counts
        rc = fn(*head, b"".join(segs), offs[1].ctypes.data_as(lp), len(segs), *who, 95.0, 1e-10, 1.28, 0.46, 0, 0, *rows, 8, C.byref(n), C.byref(stats))
        got = [tuple(int(a[k]) for a in out[1:]) for k in range(max(n.value, 0))]
        return rc, n.value, got, capi.lib().sc_profile_error().decode(), stats.as_dict()

    good = call(None, genes, segs, [0, 0, 1])
    assert good[0] == 0 and good[1] == len(good[2]) > 0 and good[4]["n_stretches"] == 1
    # without an index
    rc, n, rows, msg, stats = call(None, genes, [], [])
    assert rc == 0 and n == 0 and set(stats.values()) == {0}
    rc, n, rows, msg, stats = call(None, genes + [long_gene], segs + [long_seg], [0, 0, 1, 1])
    assert rc == -4 and "sc_profile_counts: gene 2 has 8193 bases (1..8192 supported)" in msg
    rc, n, rows, msg, stats = call(None, genes, [segs[0], long_seg, segs[2]], [0, 0, 5])
    assert rc == -3 and "segment 2 belongs to read 5 of 2" in msg
    rc, n, rows, msg, stats = call(None, genes + [long_gene], segs, [0, 0, 1], with_gene=False)
    assert rc == -3 and "sc_profile_counts: missing argument" in msg
    # on an index: its genes were checked when it was made
    with capi.ProfileIndex(genes) as ix:
        rc, n, rows, msg, stats = call(ix, (), [], [])
        assert rc == 0 and n == 0 and stats.pop("n_samples") == 1 and set(stats.values()) == {0}
        rc, n, rows, msg, stats = call(ix, (), [segs[0], long_seg, segs[2]], [0, 0, 5])
        assert rc == -3 and "segment 2 belongs to read 5 of 2" in msg
        rc, n, rows, msg, stats = call(ix, (), [segs[0], long_seg, segs[2]], [0, 0, 1], with_gene=False)
        assert rc == -3 and "sc_profile_index_counts: missing argument" in msg
        rc, n, rows, msg, stats = call(ix, (), [segs[0], long_seg, segs[2]], [0, 0, 1])
        assert rc == -4 and "sc_profile_index_counts: segment 1 has 513 bases (1..512 supported)" in msg
        rc, n, rows, msg, stats = call(ix, (), segs, [0, 0, 1])
        assert (rc, n, rows) == good[:3] and stats["n_stretches"] == 1
