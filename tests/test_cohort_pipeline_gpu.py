"""GPU: `bin/rambl --profile` (rambl_amd/pipeline.py) on the synthetic world of tests/pipeline_lib.py: <prefix>_profile/ is what
rambl-cohort writes for <prefix>.fa and the files of BamFiles, and the flag changes nothing else."""
import os

import pytest

import pipeline_lib as P

pytestmark = pytest.mark.gpu

ARGS = ["-p", "t", "-c", "4"]


def _files_under(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_profile_flag_adds_the_cohort_tables_and_nothing_else(tmp_path, monkeypatch):
    from rambl_amd import cohort, pipeline
    w = P.make_world(str(tmp_path / "world"))
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    plain.mkdir()
    flagged.mkdir()
    monkeypatch.chdir(plain)
    assert pipeline.main([w["data_info"]] + ARGS) == 0
    assert os.listdir(str(plain)) == ["t.fa"]                            # no directory without the flag
    monkeypatch.chdir(flagged)
    opts = pipeline.build_parser().parse_args([w["data_info"], "--profile", "--profile-seeded"] + ARGS)
    data = pipeline.parse_data_info(w["data_info"])
    status, times, _ = pipeline.run(opts, data, pipeline.check_data(data, w["data_info"]))
    assert status == 0 and [t[0] for t in times][-2:] == ["strain-level assembly", "profile the samples"]
    assert sorted(os.listdir(str(flagged))) == ["t.fa", "t_profile"]
    result = open(str(flagged / "t.fa"), "rb").read()
    assert result == open(str(plain / "t.fa"), "rb").read() and result.count(b">") >= 3
    # the same files from the command on the same inputs, seeded or not
    listing = tmp_path / "samples.txt"
    listing.write_text("".join(b + "\n" for b in w["bams"]))
    assert cohort.main([str(flagged / "t.fa"), str(listing), "-o", str(tmp_path / "by_hand")]) == 0
    got = _files_under(str(flagged / "t_profile"))
    assert got == _files_under(str(tmp_path / "by_hand"))
    assert sorted(got) == [cohort.MATRIX_NAME, "sample0_gene_count.tsv", "sample1_gene_count.tsv"]
    matrix = got[cohort.MATRIX_NAME].decode().splitlines()
    assert matrix[0] == "gene\tsample0\tsample1" and len(matrix) == 1 + result.count(b">")
    assert any(float(c) > 0 for ln in matrix[1:] for c in ln.split("\t")[1:])
