"""GPU: the whole pipeline from a data_info file (rambl_amd/pipeline.py, bin/rambl) on the synthetic world of
tests/pipeline_lib.py -- three clades of a gene with two strains and a 3 %-divergent relative, a clade without reads, a
gene covered on a tenth of its length, the reads in two SAM files.  The driver's work directory against the stages' own
entry points chained by hand through files, the result against the C oracle and the true strains, the seed list, one
opening per alignment file, the -R rule, bin/rambl as a child process, and a run that finds no seed."""
import contextlib
import io
import os
import subprocess
import sys

import pytest

import pipeline_lib as P
import sc_testlib as T
from test_stage4_gpu import _edit

pytestmark = pytest.mark.gpu

ARGS = ["-p", "t", "-c", "4"]


def _files_under(d):
    out = {}
    for base, _, names in os.walk(d):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The world, and the condition it is built to meet, checked on the CPU: stage 3 on the stage-1 oracle's intervals finds
    exactly one seed in each of the three clades with reads (tests/test_pipeline_host.py checks the same without a GPU)."""
    from rambl_amd import pipeline, stage3
    d = tmp_path_factory.mktemp("world")
    w = P.make_world(str(d))
    depth, abun = P.cpu_files(w, str(d / "cpu"))
    kw = pipeline.stage3_kwargs(pipeline.build_parser().parse_args([w["data_info"]]), pipeline.parse_data_info(w["data_info"]))
    w["cpu_seed_lines"] = stage3.find_seed_otus(w["GeneTree"], abun, depth, w["GeneIndex"], w["GeneAlign"], **kw)
    assert sorted(P.clade_of(w, ln.split("\t")[0]) for ln in w["cpu_seed_lines"]) == [0, 1, 2]
    return w


@pytest.fixture(scope="module")
def kept(world, tmp_path_factory):
    """One run of the driver with -R, every capi.NativeAln construction counted by path."""
    from rambl_amd import capi, pipeline
    run_dir = str(tmp_path_factory.mktemp("run"))
    opened = []

    class Counted(capi.NativeAln):
        def __init__(self, path, only=None):
            opened.append(path)
            super().__init__(path, only)

    err = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(run_dir)
        mp.setattr(capi, "NativeAln", Counted)
        with contextlib.redirect_stderr(err):
            status = pipeline.main([world["data_info"], "-R"] + ARGS)
    (work,) = [x for x in os.listdir(run_dir) if x.startswith("RAMBL_work_dir_")]
    return dict(status=status, run_dir=run_dir, work=os.path.join(run_dir, work), opened=opened, err=err.getvalue(),
                result=open(os.path.join(run_dir, "t.fa")).read())


def test_work_directory_equals_the_stages_chained_by_hand(world, kept, tmp_path, capsys):
    """The driver adds nothing of its own: stage1.main's stdout -> gene_depth.txt, stage2.main, stage3.main, stage4.main -o,
    stage5.strain_call and seqtk_L in a second directory give the same files, byte for byte."""
    from rambl_amd import stage1, stage2, stage3, stage4, stage5
    assert kept["status"] == 0, kept["err"]
    d = str(tmp_path)
    w = world

    def stdout_of(main, argv, name):
        capsys.readouterr()
        assert main(argv) == 0
        open(os.path.join(d, name), "w").write(capsys.readouterr().out)
        return os.path.join(d, name)

    depth = stdout_of(stage1.main, [w["BamFiles"], w["GeneIndex"]], "gene_depth.txt")
    abun = stdout_of(stage2.main, [depth, w["GeneIndex"]], "gene_abundance.txt")
    seeds = stdout_of(stage3.main, ["-T", w["GeneTax"], "-s", "0.9", "-c", "0.9", "-d", "1", w["GeneTree"], abun, depth, w["GeneIndex"],
                                    w["GeneAlign"]], "seed_gene.txt")
    assert stage4.main([w["GeneSeq"], seeds, w["BamFiles"], "-o", d, "-c", "4"]) == 0
    full = stage5.strain_call(os.path.join(d, "0_otu_dir", "seed_otus.fasta"), os.path.join(d, "to_seed_otus.all.sam"), out_dir=d, prefix="t")
    got, exp = _files_under(kept["work"]), _files_under(d)
    assert sorted(got) == sorted(exp) == sorted(
        ["gene_depth.txt", "gene_abundance.txt", "seed_gene.txt", "0_otu_dir/seed_otus.fasta", "0_otu_dir/seed_otus.fasta.fai",
         "to_seed_otus.all.sam", "t.fa"] + ["3_straincall_results/%s.fa" % r for r in stage5.roi_list(os.path.join(d, "0_otu_dir", "seed_otus.fasta.fai"))])
    for name in sorted(exp):
        assert got[name] == exp[name], name
    assert kept["result"] == stage5.seqtk_L(full, 400) and len(kept["result"]) > 0
    # the device's stage 1 and the stage-1 oracle agree on this world, so the seed list is the one fixed on the CPU
    assert got["seed_gene.txt"].decode() == "".join(ln + "\n" for ln in w["cpu_seed_lines"])


def test_result_equals_the_oracle_and_holds_every_true_strain(world, kept, oracle_bin):
    """<prefix>.fa = the C oracle's per-region output on the driver's to_seed_otus.all.sam after the >= 400 filter, and every
    true strain of the three clades is within 1 % edits of a record (the bound of test_stage4_then_stage5_end_to_end)."""
    from rambl_amd import stage5, synth
    fa = os.path.join(kept["work"], "0_otu_dir", "seed_otus.fasta")
    sam = os.path.join(kept["work"], "to_seed_otus.all.sam")
    expected = ""
    for roi in stage5.roi_list(fa + ".fai"):
        out, _ = T.run_oracle(stage5.straincall_argv(roi, fa, sam), kept["work"])
        expected += out
    assert kept["result"] == stage5.seqtk_L(expected, 400)
    called = [s for s in kept["result"].split("\n") if s and not s.startswith(">")]
    worst = 0
    for g in world["genes"]:
        for edits in g["strains"]:
            strain = "".join(b for _, kind, b in synth._strain_columns(g["ref"], edits) if kind != "D")
            dist = min([x for x in (_edit(strain, c) for c in called) if x is not None], default=len(strain))
            worst = max(worst, dist)
            print("gene %s strain: %d edits of %d bases" % (g["name"], dist, len(strain)))
            assert dist <= len(strain) // 100, (g["name"], dist)
    print("worst strain edit distance", worst)


def test_seed_list_names_one_gene_of_each_clade_with_reads(world, kept):
    seeds = [ln.split("\t")[0] for ln in open(os.path.join(kept["work"], "seed_gene.txt")).read().splitlines()]
    assert len(seeds) == 3 and sorted(P.clade_of(world, s) for s in seeds) == [0, 1, 2]


def test_each_alignment_file_is_opened_once(world, kept):
    bams = [ln.strip() for ln in open(world["BamFiles"]) if ln.strip()]
    assert len(bams) == 2
    assert sorted(p for p in kept["opened"] if p in bams) == sorted(bams)
    # the only other file the library reads is stage 5's input
    assert [p for p in kept["opened"] if p not in bams] == [os.path.join(kept["work"], "to_seed_otus.all.sam")]


def test_without_R_the_work_directory_is_gone_and_bin_rambl_gives_the_same_bytes(world, kept, tmp_path, monkeypatch):
    from rambl_amd import pipeline
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    monkeypatch.chdir(a)
    assert pipeline.main([world["data_info"]] + ARGS) == 0
    assert os.listdir(str(a)) == ["t.fa"] and open(str(a / "t.fa")).read() == kept["result"]
    p = subprocess.run([sys.executable, os.path.join(P.ROOT, "bin", "rambl"), world["data_info"]] + ARGS, cwd=str(b), timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert os.listdir(str(b)) == ["t.fa"] and open(str(b / "t.fa")).read() == kept["result"]


def test_reads_below_the_clade_depth_give_no_seed(world, tmp_path, monkeypatch, capsys):
    from rambl_amd import pipeline, stage4, stage5
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(stage4, "recluster", lambda *a, **k: pytest.fail("stage 4 was called"))
    monkeypatch.setattr(stage5, "strain_call", lambda *a, **k: pytest.fail("stage 5 was called"))
    assert pipeline.main([world["data_info"], "-A", "100000"] + ARGS) == 1
    assert "no seed gene" in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == ["t.fa"] and open(str(tmp_path / "t.fa")).read() == ""
