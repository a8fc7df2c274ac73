"""CPU: the host side of the cohort profile (rambl_amd/cohort.py, the --profile options of rambl_amd/pipeline.py, the binding
of sc_profile_index_* in rambl_amd/capi.py) and the property checks of tests/cohort_lib.py that need no device."""
import ctypes
import os
import re

import pytest

import cohort_lib as HL
from rambl_amd import cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_list_names_defaults_and_empty_lines(tmp_path):
    a, b, c = (str(tmp_path / n) for n in ("a.sorted.bam", "b.sam", "c"))
    for p in (a, b, c):
        open(p, "w").close()
    text = "%s\n\n%s\tgut 7\n   \n%s\n" % (a, b, c)
    assert cohort.parse_samples(text) == [(a, "a.sorted"), (b, "gut 7"), (c, "c")]
    assert cohort.parse_samples("") == [] and cohort.parse_samples("\n\n") == []
    assert cohort.default_name("/x/y/s1.bam") == "s1" and cohort.default_name("s2") == "s2" and cohort.default_name("d.e/s.3.sam") == "s.3"


def test_sample_list_errors(tmp_path):
    a, b = str(tmp_path / "a.sam"), str(tmp_path / "other" / "a.bam")
    os.mkdir(str(tmp_path / "other"))
    for p in (a, b):
        open(p, "w").close()
    with pytest.raises(ValueError, match="sample name a is given twice"):
        cohort.parse_samples("%s\n%s\n" % (a, b))
    with pytest.raises(ValueError, match="sample name x is given twice"):
        cohort.parse_samples("%s\tx\n%s\tx\n" % (a, b))
    assert [n for _, n in cohort.parse_samples("%s\n%s\tb\n" % (a, b))] == ["a", "b"]
    with pytest.raises(ValueError, match="missing.sam does not exist"):
        cohort.parse_samples("%s\n%s\n" % (a, str(tmp_path / "missing.sam")))
    with pytest.raises(ValueError, match="line 2 of the sample list"):
        cohort.parse_samples("%s\n%s\tb\tc\n" % (a, b))
    with pytest.raises(ValueError, match="line 1 of the sample list"):
        cohort.parse_samples("%s\t\n" % a)
    with pytest.raises(ValueError, match="given twice"):
        cohort.sample_names(["/p/s.sam", "/q/s.bam"])
    assert cohort.sample_names(["/p/s.sam", "/q/t.bam"]) == [("/p/s.sam", "s"), ("/q/t.bam", "t")]


def test_batch_plan():
    plan = cohort.plan_batches
    assert plan([], 10) == []
    assert plan([7], 10) == [(0, 1)] and plan([70], 10) == [(0, 1)]
    assert plan([4, 6, 1, 9, 1], 10) == [(0, 2), (2, 4), (4, 5)]           # the cap itself still fits
    assert plan([4, 7, 1], 10) == [(0, 1), (1, 3)]
    assert plan([3, 30, 3, 3], 10) == [(0, 1), (1, 2), (2, 4)]             # a sample larger than the cap goes alone
    assert plan([0, 0, 5, 0], 1) == [(0, 2), (2, 3), (3, 4)]               # samples without a segment are samples all the same
    assert plan([0, 0, 5, 0], 5) == [(0, 4)]
    assert plan([5, 5, 5], 1) == [(0, 1), (1, 2), (2, 3)]
    assert list(cohort.batches([("a", 2), ("b", 2), ("c", 2)], 4)) == [["a", "b"], ["c"]]
    for counts in ([4, 6, 1, 9, 1], [3, 30, 3, 3], [1] * 7):              # whole samples, in order, none lost
        for cap in (1, 5, 10, 100):
            got = plan(counts, cap)
            assert [a for a, _ in got] == [0] + [b for _, b in got[:-1]] and got[-1][1] == len(counts)
            assert all(sum(counts[a:b]) <= cap or b - a == 1 for a, b in got)


def test_matrix_by_hand():
    from fractions import Fraction
    from rambl_amd import profile
    t0 = profile.format_table("s0", [("gA", Fraction(7, 3)), ("gC", 2)])
    t1 = profile.format_table("s1", [("gC", Fraction(1, 8)), ("gb", 10)])
    t2 = profile.format_table("s2", [])
    assert t2 == "sample\ts2\n"                                           # what a sample without any count gets
    assert cohort.table_cells(t0) == {"gA": "2.333", "gC": "2.0"}
    got = cohort.matrix_text(["gb", "gC", "gA", "gZ"], ["s0", "s1", "s2"], [t0, t1, t2])
    assert got == ("gene\ts0\ts1\ts2\n"
                   "gA\t2.333\t0.0\t0.0\n"
                   "gC\t2.0\t0.125\t0.0\n"
                   "gZ\t0.0\t0.0\t0.0\n"
                   "gb\t0.0\t10.0\t0.0\n")
    rel = profile.format_table("s0", [("gA", 1), ("gC", 2)], relative=True)
    assert cohort.matrix_text(["gA", "gC"], ["s0"], [rel]) == "gene\ts0\ngA\t0.333333333\ngC\t0.666666667\n"


def test_option_errors_of_rambl_cohort(tmp_path, capsys):
    fa, sam = str(tmp_path / "g.fa"), str(tmp_path / "s.sam")
    open(fa, "w").write(">g\nACGT\n")
    open(sam, "w").close()
    listing = str(tmp_path / "list.txt")
    open(listing, "w").write(sam + "\n")
    empty = str(tmp_path / "empty.fa")
    open(empty, "w").close()
    twice = str(tmp_path / "twice.txt")
    open(twice, "w").write("%s\n%s\n" % (sam, sam))
    gone = str(tmp_path / "gone.txt")
    open(gone, "w").write(str(tmp_path / "no.sam") + "\n")
    nothing = str(tmp_path / "nothing.txt")
    open(nothing, "w").write("\n")
    for argv, message in (([fa, listing, "--copy-correct", "fx.tsv"], "--copy-correct FIXRANK and --copy-number TSV go together"),
                          ([fa, listing, "--copy-thresh", "0.5"], "--copy-thresh needs --copy-correct"),
                          ([fa, listing, "--batch-segments", "0"], "--batch-segments must be at least 1"),
                          ([fa, listing, "-c", "0"], "-c must be at least 1"),
                          ([fa, twice], "sample name s is given twice"),
                          ([fa, gone], "no.sam does not exist"),
                          ([fa, nothing], "lists no sample"),
                          ([fa, str(tmp_path / "no_list.txt")], "no_list.txt"),
                          ([empty, listing], "holds no gene"),
                          ([fa], "SAMPLES")):
        with pytest.raises(SystemExit) as e:
            cohort.main(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    assert not any(n.endswith(".tsv") for n in os.listdir(str(tmp_path)))


def test_profile_seeded_needs_profile(tmp_path, capsys):
    from rambl_amd import pipeline
    with pytest.raises(SystemExit) as e:
        pipeline.main([str(tmp_path / "data_info.txt"), "--profile-seeded"])
    assert e.value.code == 2 and "--profile-seeded needs --profile" in capsys.readouterr().err
    opts = pipeline.build_parser().parse_args(["d.txt"])
    assert not hasattr(opts, "profile") and not hasattr(opts, "profile_seeded")          # rambl.py's argv parses to what it did
    opts = pipeline.build_parser().parse_args(["d.txt", "--profile", "--profile-seeded"])
    assert opts.profile is True and opts.profile_seeded is True
    assert pipeline.profile_dir("/w/16S_gene_assembly.fa") == "/w/16S_gene_assembly_profile" and pipeline.profile_dir("a.b.fa") == "a.b_profile"


def test_two_samples_of_one_name_stop_the_pipeline_early(tmp_path, capsys, monkeypatch):
    import pipeline_lib as P
    from rambl_amd import pipeline
    w = P.make_world(str(tmp_path / "world"), n_clades=1, n_reads=40, rel_reads=10)
    other = tmp_path / "elsewhere"
    other.mkdir()
    twin = str(other / "sample0.sam")
    open(twin, "w").write(open(w["bams"][0]).read())
    open(w["BamFiles"], "a").write(twin + "\n")
    monkeypatch.setattr(pipeline, "run", lambda *a, **k: pytest.fail("the pipeline ran"))
    assert pipeline.main([w["data_info"], "--profile"]) == 2
    assert "sample name sample0 is given twice" in capsys.readouterr().err


def test_index_entries_are_declared_exported_and_bound():
    """sc_profile_index_*: in the header, exported, bound with as many arguments as the header declares."""
    from rambl_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "straincall_hip.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name, ret, n_args in (("sc_profile_index_create", "int", 5), ("sc_profile_index_info", "int", 5),
                              ("sc_profile_index_counts", "int", 22), ("sc_profile_index_free", "void", 1)):
        decl = re.search(r"\b%s %s\s*\(([^)]*)\)" % (ret, name), hdr)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in capi.EXPORTS
        f = getattr(lib, name)
        assert len(f.argtypes) == n_args and f.restype is (ctypes.c_int if ret == "int" else None), name
    st = re.search(r"typedef struct sc_profile_cohort_stats \{(.*?)\} sc_profile_cohort_stats;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", st) == ["counts", "n_samples", "n_index_builds", "n_allocs"]
    own = [f for f, _ in capi.ScProfileCohortStats._fields_]
    assert own == [f for f, _ in capi.ScProfileCountStats._fields_] + ["n_samples", "n_index_builds", "n_allocs"]
    assert ctypes.sizeof(capi.ScProfileCohortStats) == ctypes.sizeof(capi.ScProfileCountStats) + 16
    for attr in ("counts", "info", "close", "__enter__", "__exit__"):
        assert hasattr(capi.ProfileIndex, attr)
    res = capi.ProfileCohortCounts([(0, 1, 1, 1, 5), (2, 0, 1, 2, 1), (2, 3, 1, 1, 4)], None)
    assert res.by_sample(2) == [(0, 1, 2, 1), (3, 1, 1, 4)] and res.by_sample(1) == [] and len(res) == 3


def test_restated_stretch_plan():
    plan = HL.plan_stretches
    assert HL.can_pass(150, 8100) and HL.can_pass(40, 960) and not HL.can_pass(10, 8100)
    # 3 genes: 6 tiles a segment.  Whole reads; a stretch closes when the next read would exceed the room
    reads = [[100], [100, 100], [100], [10], [100, 100, 100], [100]]
    assert plan(reads, 3, 900, 1 << 23) == [(0, 6)]
    assert plan(reads, 3, 900, 18) == [(0, 2), (2, 4), (4, 5), (5, 6)]     # read 3 has no tile and rides with read 2
    assert plan(reads, 3, 900, 1) == [(0, 1), (1, 2), (2, 3), (3, 5), (5, 6)]     # a full stretch closes in front of it: it opens the next
    assert plan(reads, 3, 900, 24) == [(0, 4), (4, 6)]
    assert plan([[10], [10]], 3, 900, 6) == [] and plan([], 3, 900, 6) == []


@pytest.mark.parametrize("name", ("seams", "gaps"))
def test_cases_reach_their_stretch_edges(name):
    """The checks of cases 2 and 4 that need no device: where the restated plan puts the stretch boundaries."""
    c = HL.cohort(name)
    at = c.first_read()
    assert at[-1] == sum(s.n_reads for s in c.samples) and len(c.flat()[2]) == at[-1]
    segs, seg_read, read_sample = c.flat()
    assert read_sample == sorted(read_sample) and max(seg_read) == at[-1] - 1 and len(segs) == len(seg_read)
    if name == "seams":
        plan = c.plan(HL.SEAMS_ROOM)
        assert len(plan) >= 3 and plan[0][0] == 0 and plan[-1][1] == at[-1]
        assert any(at[s] < a < at[s + 1] for a, _ in plan[1:] for s in range(3))
        assert any(a < at[s] < b for a, b in plan for s in (1, 2))
        assert len(c.plan(1)) == at[-1] and len(c.plan(HL.CL_ROOM)) == 1
    else:
        assert [s.n_reads > 0 for s in c.samples] == [True, False, True, True, False]
        assert sorted(set(read_sample)) == [0, 2, 3] and len(c.plan(HL.CL_ROOM)) == 1
        assert at[1] == at[2] and at[4] == at[5]
