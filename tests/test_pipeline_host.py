"""CPU: the whole-pipeline driver (rambl_amd/pipeline.py) without a GPU -- the data_info parser, rambl.py's argv table,
the option mapping into stages 3 and 5, the work directory and the -R rule with the stages replaced by stubs, and the
hand-over stage 1 -> 2 -> 3 on the synthetic world of the GPU test (tests/pipeline_lib.py), which also fixes the seed
list that test has to find."""
import os
import re

import pytest

import pipeline_lib as P
import seed_otus_oracle as O  # noqa: E402  (test infrastructure; pipeline_lib puts oracle/ on the path)
from rambl_amd import capi, pipeline, stage1, stage2, stage3, stage4, stage5


# ---------------------------------------------------------------------------------------------------- data_info

def test_parse_data_info_any_order_and_spaces(tmp_path):
    p = str(tmp_path / "data_info.txt")
    open(p, "w").write("# samples of the run\nGeneTree =  /db/gg.tree  \nBamFiles=/x/bams.txt\nGeneAlign\t=\t/db/gg.aln\n\n"
                       "GeneSeq = /db/gg.fa = ignored\nGeneTax= /db/gg.tax\nGeneIndex =/db/gg.fa.fai\nOther = 1\n")
    assert pipeline.parse_data_info(p) == {"BamFiles": "/x/bams.txt", "GeneSeq": "/db/gg.fa", "GeneIndex": "/db/gg.fa.fai",
                                           "GeneTree": "/db/gg.tree", "GeneTax": "/db/gg.tax", "GeneAlign": "/db/gg.aln"}
    open(p, "w").write("GeneSeq = a\nGeneSeq = b\nBamFiles\n")
    with pytest.raises(pipeline.DataInfoError, match="BamFiles"):
        pipeline.parse_data_info(p)


def _data(tmp_path, drop=(), missing=()):
    d = {}
    for k in pipeline.KEYS:
        if k in drop:
            continue
        d[k] = str(tmp_path / (k + ".file"))
        if k not in missing:
            open(d[k], "w").write(str(tmp_path / "s0.sam") + "\n" if k == "BamFiles" else "x\n")
        elif os.path.exists(d[k]):
            os.remove(d[k])
    open(str(tmp_path / "s0.sam"), "w").write("@SQ\tSN:g\tLN:10\n")
    p = str(tmp_path / "data_info.txt")
    open(p, "w").write("".join("%s = %s\n" % kv for kv in d.items()))
    return p


def test_gene_tax_is_optional_and_a_missing_key_or_file_is_an_error(tmp_path):
    p = _data(tmp_path, drop=("GeneTax",))
    data = pipeline.parse_data_info(p)
    assert data["GeneTax"] == "" and pipeline.check_data(data, p) == [str(tmp_path / "s0.sam")]
    assert pipeline.stage3_kwargs(pipeline.build_parser().parse_args([p]), data)["taxonomy"] is None
    for key in ("BamFiles", "GeneSeq", "GeneIndex", "GeneTree", "GeneAlign"):
        with pytest.raises(pipeline.DataInfoError, match=key):
            pipeline.check_data(pipeline.parse_data_info(_data(tmp_path, drop=(key,))))
    with pytest.raises(pipeline.DataInfoError, match="GeneTree"):
        pipeline.check_data(pipeline.parse_data_info(_data(tmp_path, missing=("GeneTree",))))
    p = _data(tmp_path)
    os.remove(str(tmp_path / "s0.sam"))
    with pytest.raises(pipeline.DataInfoError, match="s0.sam"):
        pipeline.check_data(pipeline.parse_data_info(p))


def test_unusable_input_ends_before_any_stage(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pipeline, "run", lambda *a, **k: pytest.fail("the pipeline started"))
    assert pipeline.main([_data(tmp_path, drop=("GeneIndex",))]) == 2
    assert "GeneIndex" in capsys.readouterr().err
    assert not [x for x in os.listdir(str(tmp_path)) if x.startswith("RAMBL_work_dir_")]


# ---------------------------------------------------------------------------------------------------- argv and mapping

def test_argv_table_of_rambl_py():
    ap = pipeline.build_parser()
    o = ap.parse_args(["data_info.txt"])
    assert vars(o) == dict(data_info="data_info.txt", cores=1, max_depth=800, map_qual=0, max_ins=13, read_len=70, tau=0.02,
                           diff_rate=0.02, gene_sim=0.9, clade_coverage=0.9, clade_depth=1, prefix="16S_gene_assembly",
                           keep=False, verbose=False, device=0)
    o = ap.parse_args("-c 8 -D 3000 -q 10 -i 5 -l 100 -t 0.05 -d 0.01 -g 0.97 -K 0.5 -A 25 -p out -R -v --device 3 d.txt".split())
    assert vars(o) == dict(data_info="d.txt", cores=8, max_depth=3000, map_qual=10, max_ins=5, read_len=100, tau=0.05,
                           diff_rate=0.01, gene_sim=0.97, clade_coverage=0.5, clade_depth=25, prefix="out", keep=True,
                           verbose=True, device=3)
    o = ap.parse_args("--cores 2 --max-depth 1 --map-qual 2 --max-ins 3 --read-len 4 --tau 0.5 --diff-rate 0.6 --gene-similarity 0.7 "
                      "--clade-coverage 0.8 --clade-depth 9 --prefix p d.txt".split())
    assert (o.cores, o.max_depth, o.map_qual, o.max_ins, o.read_len, o.tau, o.diff_rate, o.gene_sim, o.clade_coverage,
            o.clade_depth, o.prefix) == (2, 1, 2, 3, 4, 0.5, 0.6, 0.7, 0.8, 9, "p")


def test_option_mapping_into_stage3_and_stage5():
    ap = pipeline.build_parser()
    o = ap.parse_args("-D 3000 -q 10 -i 5 -l 100 -t 0.05 -d 0.01 -g 0.97 -K 0.5 -A 25 d.txt".split())
    data = dict.fromkeys(pipeline.KEYS, "x")
    # -g is find_seed_otus.py's -s, -K its -c (gene_cover) and -A its -d (depth_thres): rambl.py:138-139
    assert pipeline.stage3_kwargs(o, data) == dict(sim_thres=0.97, gene_cover=0.5, depth_thres=25.0, taxonomy="x")
    assert stage5.straincall_argv("g:1-700", "s.fasta", "a.sam", pipeline.stage5_opts(o)) == [
        "-r", "g:1-700", "-q", "10", "-D", "3000", "-I", "5", "-l", "100", "-t", "0.05", "-d", "0.01", "-w", "5000", "s.fasta", "a.sam"]
    # rambl.py's defaults are stage 5's: the driver holds no second copy of them
    assert pipeline.stage5_opts(ap.parse_args(["d.txt"])) == stage5.RAMBL_DEFAULTS
    assert stage5.straincall_argv("g:1-9", "f", "b", pipeline.stage5_opts(ap.parse_args(["d.txt"]))) == stage5.straincall_argv("g:1-9", "f", "b")


# ---------------------------------------------------------------------------------------------------- the driver on stubs

class _Stubs:
    """The five stages and the library calls of the driver, replaced: every stub records its call and writes what the
    stage would leave behind."""

    def __init__(self, monkeypatch, seeds=("g\t30.0\t1.0\t30.0\t1.0\t1\t",), fail_region=False):
        self.calls, self.open, self.closed_at_stage5 = [], [], None
        st = self

        class Aln:
            def __init__(self, path, only=None):
                self.path, self.is_open = path, True
                st.open.append(self)
                st.threads = os.environ.get("SC_INGEST_THREADS")

            def close(self):
                self.is_open = False

        def depth_intervals(paths, fai, max_gap=10, device=0, alns=None):
            st.calls.append(("stage1", dict(paths=paths, fai=fai, device=device, alns=alns)))
            return [("g", 1, 100, 3000, 100)], {}

        def gene_abundance(depth, index):
            st.calls.append(("stage2", dict(depth=open(depth).read(), index=index)))
            return ["g\t1\t100\t30.300000\t1.010000"]

        def find_seed_otus(tree, abun, mask, index, align=None, **kw):
            st.calls.append(("stage3", dict(tree=tree, abun=open(abun).read(), mask=mask, index=index, align=align, **kw)))
            return list(seeds)

        def recluster(fasta, seed_file, bams, out_dir=".", device=0, verbose=False, alns=None, **kw):
            st.calls.append(("stage4", dict(fasta=fasta, seeds=open(seed_file).read(), bams=bams, out_dir=out_dir, device=device,
                                            alns=alns, all_open=all(a.is_open for a in alns))))
            os.makedirs(os.path.join(out_dir, "0_otu_dir"))
            open(os.path.join(out_dir, "0_otu_dir", "seed_otus.fasta.fai"), "w").write("g\t100\t3\t60\t61\nh\t500\t9\t60\t61\n")
            open(os.path.join(out_dir, "to_seed_otus.all.sam"), "w").write("@HD\n")
            return os.path.join(out_dir, "to_seed_otus.all.sam"), None

        def strain_call(fasta, bam, out_dir=None, prefix="rambl", opts=None, device=0, streams=4, ingest_workers=4, errors=None, **kw):
            st.calls.append(("stage5", dict(fasta=fasta, bam=bam, out_dir=out_dir, prefix=prefix, opts=opts, device=device,
                                            streams=streams, ingest_workers=ingest_workers)))
            st.closed_at_stage5 = not any(a.is_open for a in st.open)
            if fail_region:
                errors.append(("h:1-500", "no read"))
            text = ">short\n" + "A" * 399 + "\n>long\n" + "C" * 400 + "\n"
            open(os.path.join(out_dir, "%s.fa" % prefix), "w").write(text)
            return text

        monkeypatch.setattr(capi, "NativeAln", Aln)
        monkeypatch.setattr(capi, "host_plan", lambda streams, *a: (3, 1, 6))
        monkeypatch.setattr(stage1, "depth_intervals", depth_intervals)
        monkeypatch.setattr(stage2, "gene_abundance", gene_abundance)
        monkeypatch.setattr(stage3, "find_seed_otus", find_seed_otus)
        monkeypatch.setattr(stage4, "recluster", recluster)
        monkeypatch.setattr(stage5, "strain_call", strain_call)


def _work_dirs(d):
    return [x for x in os.listdir(str(d)) if x.startswith("RAMBL_work_dir_")]


def test_driver_on_stubs_keeps_the_work_directory_with_R(tmp_path, monkeypatch):
    st = _Stubs(monkeypatch)
    info = _data(tmp_path)
    data = pipeline.parse_data_info(info)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    monkeypatch.chdir(run_dir)
    monkeypatch.setenv("SC_INGEST_THREADS", "31")
    assert pipeline.main([info, "-R", "-p", "t", "-c", "4", "-A", "7", "--device", "2"]) == 0
    assert os.environ["SC_INGEST_THREADS"] == "31" and st.threads == "4"        # -c 4 within the host's share of 6
    (work,) = _work_dirs(run_dir)
    assert re.fullmatch(r"RAMBL_work_dir_[0-9a-zA-Z]{5}", work) and len(set(work[-5:])) == 5
    work = str(run_dir / work)
    assert sorted(os.listdir(work)) == ["0_otu_dir", "gene_abundance.txt", "gene_depth.txt", "seed_gene.txt", "t.fa", "to_seed_otus.all.sam"]
    assert open(os.path.join(work, "gene_depth.txt")).read() == "g\t1\t101\t30\n"
    assert open(str(run_dir / "t.fa")).read() == ">long\n" + "C" * 400 + "\n"      # the length filter, outside the work directory
    assert os.getcwd() == str(run_dir)
    calls = dict(st.calls)
    assert [c[0] for c in st.calls] == ["stage1", "stage2", "stage3", "stage4", "stage5"]
    assert calls["stage1"]["paths"] == [str(tmp_path / "s0.sam")] and calls["stage1"]["fai"] == data["GeneIndex"]
    assert calls["stage1"]["alns"] is calls["stage4"]["alns"] and [a.path for a in st.open] == [str(tmp_path / "s0.sam")]
    assert calls["stage4"]["all_open"] and st.closed_at_stage5
    assert calls["stage2"] == dict(depth="g\t1\t101\t30\n", index=data["GeneIndex"])
    assert calls["stage3"] == dict(tree=data["GeneTree"], abun="g\t1\t100\t30.300000\t1.010000\n", mask=os.path.join(work, "gene_depth.txt"),
                                   index=data["GeneIndex"], align=data["GeneAlign"], sim_thres=0.9, gene_cover=0.9, depth_thres=7.0,
                                   taxonomy=data["GeneTax"])
    assert calls["stage4"]["fasta"] == data["GeneSeq"] and calls["stage4"]["bams"] == data["BamFiles"]
    assert calls["stage4"]["seeds"] == "g\t30.0\t1.0\t30.0\t1.0\t1\t\n" and calls["stage4"]["out_dir"] == work
    assert calls["stage5"] == dict(fasta=os.path.join(work, "0_otu_dir", "seed_otus.fasta"), bam=os.path.join(work, "to_seed_otus.all.sam"),
                                   out_dir=work, prefix="t", opts=stage5.RAMBL_DEFAULTS, device=2, streams=2, ingest_workers=4)
    assert {calls[s]["device"] for s in ("stage1", "stage4", "stage5")} == {2}


def test_driver_on_stubs_removes_the_work_directory_without_R(tmp_path, monkeypatch, capsys):
    st = _Stubs(monkeypatch, fail_region=True)
    info = _data(tmp_path)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    monkeypatch.chdir(run_dir)
    monkeypatch.delenv("SC_INGEST_THREADS", raising=False)
    assert pipeline.main([info, "-v", "-c", "64"]) == 1                          # a region failed
    assert "SC_INGEST_THREADS" not in os.environ and st.threads == "6"           # -c 64 on a share of 6 CPUs
    assert dict(st.calls)["stage5"]["ingest_workers"] == 6
    assert os.listdir(str(run_dir)) == ["16S_gene_assembly.fa"]


def test_driver_on_stubs_without_a_seed(tmp_path, monkeypatch, capsys):
    st = _Stubs(monkeypatch, seeds=())
    info = _data(tmp_path)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    monkeypatch.chdir(run_dir)
    assert pipeline.main([info, "-R", "-p", "t"]) == 1
    assert [c[0] for c in st.calls] == ["stage1", "stage2", "stage3"] and not any(a.is_open for a in st.open)
    assert "no seed gene" in capsys.readouterr().err and open(str(run_dir / "t.fa")).read() == ""
    (work,) = _work_dirs(run_dir)
    assert open(str(run_dir / work / "seed_gene.txt")).read() == ""


def test_a_failing_stage_leaves_no_work_directory(tmp_path, monkeypatch, capsys):
    _Stubs(monkeypatch)
    monkeypatch.setattr(stage3, "find_seed_otus", lambda *a, **k: (_ for _ in ()).throw(ValueError("no gene of the tree has any abundance")))
    monkeypatch.chdir(tmp_path)
    assert pipeline.main([_data(tmp_path)]) == 2
    assert "no gene of the tree" in capsys.readouterr().err and not _work_dirs(tmp_path)


# ---------------------------------------------------------------------------------------------------- hand-over 1 -> 2 -> 3

def test_handover_stage1_to_stage2_to_stage3_on_the_gpu_tests_world(tmp_path):
    """Intervals of the stage-1 oracle, printed by stage1.bed_text, through stage 2 into stage 3: the seed list of the
    literal restatement fed the same three files, and the condition the GPU test rests on: exactly one seed in each of the
    three clades with reads, none in the clade without reads, none for the gene covered on a tenth of its length."""
    w = P.make_world(str(tmp_path / "world"))
    depth, abun = P.cpu_files(w, str(tmp_path / "cpu"))
    kw = pipeline.stage3_kwargs(pipeline.build_parser().parse_args([w["data_info"]]), pipeline.parse_data_info(w["data_info"]))
    got = stage3.find_seed_otus(w["GeneTree"], abun, depth, w["GeneIndex"], w["GeneAlign"], **kw)
    assert got == O.find_seed_otus(w["GeneTree"], abun, depth, w["GeneIndex"], sim_thres=kw["sim_thres"], depth_thres=kw["depth_thres"],
                                   gene_cover_thres=kw["gene_cover"], taxonomy_file=kw["taxonomy"])
    seeds = [ln.split("\t")[0] for ln in got]
    assert sorted(P.clade_of(w, s) for s in seeds) == [0, 1, 2]
    rows = {ln.split("\t")[0]: ln.split("\t") for ln in open(abun).read().splitlines()}
    assert set(rows) == {g for c in w["clades"] for g in c} | {w["thin"]}                  # the quiet clade has no row at all
    assert float(rows[w["thin"]][3]) > 1 and float(rows[w["thin"]][4]) < 0.9                # abundant enough for -A 1, not covered for -K 0.9
    # with -A above every clade's depth there is no seed (the GPU test's last case)
    assert stage3.find_seed_otus(w["GeneTree"], abun, depth, w["GeneIndex"], **dict(kw, depth_thres=100000.0)) == []
