"""GPU: the hits of the per-sample gene profile on the device (rambl_amd/csrc/sc_profile.hip, sc_profile_dp.hpp) against the plain restatement
of the contract (tests/native/blast_hits_check.cpp), its limits, and the profile of three mixed samples end to end."""
import os

import pytest

import profile_lib as PL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


def _gaps(h):
    """(gene bases the segment skips, segment bases the gene skips) of a hit."""
    return h[5] - (h[7] - h[6] + 1), h[5] - (abs(h[9] - h[8]) + 1)


def _compare(exe, genes, segs, min_identity, max_evalue):
    exp, res = PL.compare_hits(exe, genes, segs, min_identity, max_evalue)
    assert res.stats.score_cells > 0 and res.stats.n_tiles > 0
    return exp


def test_device_equals_restatement_at_the_defaults(hits_check):
    genes, segs = PL.parity_dataset()
    assert len(genes) >= 12 and len(segs) >= 500 and {(len(s) + 63) // 64 for s in segs} == set(range(1, 9))
    exp = _compare(hits_check, genes, segs, 95.0, 1e-10)
    assert len(exp) > 200 and {h[2] for h in exp} == {0, 1}
    assert any(_gaps(h)[0] > 0 for h in exp) and any(_gaps(h)[1] > 0 for h in exp)                  # gaps on either side
    on3 = {h[0]: h for h in exp if h[1] == 3}
    on12 = {h[0]: h for h in exp if h[1] == 12}
    assert on3 and set(on3) == set(on12) and all(on3[s][2:] == on12[s][2:] for s in on3)            # the duplicated gene ties


def test_device_equals_restatement_with_weak_hits(hits_check):
    genes, segs = PL.parity_dataset()
    exp = _compare(hits_check, genes, segs, 0.0, 10.0)
    assert len(exp) > 1000 and {h[2] for h in exp} == {0, 1}
    assert any(h[3] % 2 == 1 for h in exp) and any(_gaps(h)[0] > 0 for h in exp) and any(_gaps(h)[1] > 0 for h in exp)
    assert any(100.0 * h[4] / h[5] < 95 for h in exp)


def test_a_small_capacity_grows(hits_check):
    from rambl_amd import capi
    genes, segs = PL.parity_dataset()
    genes, segs = genes[:4], segs[:60]
    a = PL.device_hits(capi.profile_hits([g.encode() for g in genes], [s.encode() for s in segs], 0.0, 10.0))
    b = PL.device_hits(capi.profile_hits([g.encode() for g in genes], [s.encode() for s in segs], 0.0, 10.0, cap=3))
    assert len(a) > 3 and a == b


def test_too_long_segment_is_unsupported():
    from rambl_amd import capi
    with pytest.raises(capi.StrainCallError) as ei:
        capi.profile_hits([b"ACGT" * 50], [b"A" * 513])
    assert ei.value.code == -4 and "513" in str(ei.value)


def test_too_long_gene_is_unsupported():
    from rambl_amd import capi
    with pytest.raises(capi.StrainCallError) as ei:
        capi.profile_hits([b"ACGT" * 50, b"A" * 8193], [b"ACGT" * 30])
    assert ei.value.code == -4 and "8193" in str(ei.value)


def test_three_mixed_samples_end_to_end(tmp_path, hits_check):
    """Three genes of three strains as the assembly, three samples mixing the strains 4 : 2 : 1 in different orders, one SAM
    per sample through profile.main: the table equals the chain restatement hits -> raw_abundance byte for byte, and within
    each gene the strains' order by count is their order by proportion (checked on the CPU for this seed in
    tests/test_profile_host.py)."""
    from rambl_amd import profile
    names, seqs, samples = PL.mixture_dataset()
    fa, sams = PL.write_mixture(tmp_path, names, seqs, samples)
    out = os.path.join(str(tmp_path), "out")
    for (sample, lines, mix), sam in zip(samples, sams):
        relative = sample == "sample2"
        assert profile.main([fa, sam, sample, "-n", "-o", out, "--keep-hits"] + (["-r"] if relative else [])) == 0
        exp, counts = PL.expected_table(hits_check, names, seqs, sample, lines, relative)
        got = open(os.path.join(out, sample + "_gene_count.tsv")).read()
        assert got == exp
        assert got.startswith("sample\t%s\n" % sample) and got.count("\n") == 10
        kept = profile.parse_hits_csv(open(os.path.join(out, sample + "_hits.csv")).read())
        assert profile.raw_abundance(kept) == sorted(counts.items(), key=lambda kv: kv[0].encode())
        for k in range(3):
            c = [float(counts["gene%d_strain%d" % (k, s)]) for s in range(3)]
            assert sorted(range(3), key=lambda s: c[s]) == sorted(range(3), key=lambda s: mix[k][s])
