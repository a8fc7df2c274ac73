"""GPU: stage 4 on the device (rambl_amd/csrc/sc_align.hip) against the plain restatement of the contract
(tests/native/sw_check.cpp), its limits, and stage 4 feeding stage 5 end to end."""
import os
import random

import numpy as np
import pytest

import sc_testlib as T
import stage4_lib as L

pytestmark = pytest.mark.gpu


def _reads_for(rng, seeds):
    reads = []

    def take(s, n):
        a = rng.randint(-n // 4, max(len(s) - 3 * n // 4, -n // 4))            # overhangs either end of the seed
        frag = s[max(a, 0):max(a, 0) + n]
        if a < 0:
            frag = L.rand_seq(rng, -a) + frag
        if len(frag) < n:
            frag += L.rand_seq(rng, n - len(frag))
        return frag[:n]
    for k in range(500):
        si = rng.randrange(len(seeds))
        n = rng.choice([60, 100, 150, 150, 150, 200]) if k % 50 else rng.choice([250, 512])
        r = L.mutate(rng, take(seeds[si], n + 8), 0.02)
        kind = k % 10
        if kind == 1:                                              # indels near the --gbar limit
            p = rng.choice([3, 4, 5, 6, n - 7, n - 6, n - 5, n - 4])
            r = r[:p] + r[p + rng.randint(1, 3):] if rng.random() < 0.5 else r[:p] + L.rand_seq(rng, rng.randint(1, 3)) + r[p:]
        elif kind == 2:                                            # indels anywhere
            p = rng.randint(10, n - 10)
            r = r[:p] + r[p + rng.randint(1, 6):]
        elif kind == 3:
            r = "".join("N" if rng.random() < 0.03 else c for c in r)
        r = r[:n]
        if kind == 4:
            r = L.rand_seq(rng, n)                                 # aligns nowhere
        if rng.random() < 0.5:
            r = L.revcomp(r)
        q = L.qual_string(rng, len(r), low=(kind == 5)) if kind != 6 else "*"
        reads.append((r, q))
    return reads


def test_device_equals_restatement(tmp_path):
    from rambl_amd import capi
    rng = random.Random(404)
    seeds = [L.rand_seq(rng, rng.choice([120, 300, 450, 600])) for _ in range(11)]
    seeds[5] = seeds[5][:100] + "N" * 3 + seeds[5][103:]
    seeds.append(seeds[3])                                         # duplicated seed: ties go to index 3, MAPQ 0
    seeds[7] = L.mutate(rng, seeds[2], 0.03)                       # a close relative
    reads = _reads_for(rng, seeds)
    exe = L.build_sw_check(tmp_path)
    exp = L.run_sw_check(exe, seeds, reads)
    got = capi.align_reads([s.encode() for s in seeds], [r.encode() for r, _ in reads], [q.encode() for _, q in reads])
    L.compare_rows(reads, exp, L.device_rows(got))
    aligned = [e for e in exp if e[2] >= 0]
    assert len(aligned) > 350 and any(e[2] == 3 and e[1] == e[0] for e in aligned) and any(e[3] == 1 for e in aligned)
    assert any("I" in e[5] or "D" in e[5] for e in aligned) and any(e[5].startswith(tuple("123456789")) and "S" in e[5] for e in aligned)
    assert got.stats.score_cells > 0 and got.stats.n_traced == len(aligned)


def test_too_long_read_is_unsupported():
    from rambl_amd import capi
    with pytest.raises(capi.StrainCallError) as ei:
        capi.align_reads([b"ACGT" * 50], [b"A" * 513])
    assert ei.value.code == -4 and "513" in str(ei.value)


def _edit(a, b, band=60):
    """Banded Levenshtein distance (None when the lengths differ by more than the band)."""
    if abs(len(a) - len(b)) > band:
        return None
    INF = 1 << 30
    prev = {j: j for j in range(0, min(len(b), band) + 1)}
    for i in range(1, len(a) + 1):
        cur = {}
        for j in range(max(0, i - band), min(len(b), i + band) + 1):
            v = INF
            if j == 0:
                v = i
            else:
                v = min(v, prev.get(j - 1, INF) + (a[i - 1] != b[j - 1]), cur.get(j - 1, INF) + 1)
            v = min(v, prev.get(j, INF) + 1)
            cur[j] = v
        prev = cur
    return prev.get(len(b))


def test_stage4_then_stage5_end_to_end(tmp_path, oracle_bin):
    """A gene database of seeds plus 3 %-divergent relatives, its reads in one SAM; stage 4 re-aligns them to the seeds,
    stage 5 calls strains from that SAM on the GPU, the C oracle does the same from the same SAM: equal FASTA bytes, and
    every true strain of a seed within 1 % edits of a called strain."""
    from rambl_amd import stage4, stage5, synth
    d = str(tmp_path)
    rng = random.Random(7)
    genes = [synth.make_gene(500 + k, glen=700, n_strains=2, n_reads=900, rlen=150, err=0.003, n_sub=6, n_ins=1, n_del=1,
                             name="seed%d" % k) for k in range(3)]
    db = []
    lines = []
    for g in genes:
        db.append((g["name"], g["ref"]))
        lines += g["sam_lines"]
        rel = L.mutate(rng, g["ref"], 0.03)
        db.append((g["name"] + "_rel", rel))
        for k in range(150):
            a = rng.randint(0, len(rel) - 150)
            s = L.mutate(rng, rel[a:a + 150], 0.003)
            lines.append("%s_rel_r%d\t0\t%s_rel\t%d\t60\t150M\t*\t0\t0\t%s\t%s\n" % (g["name"], k, g["name"], a + 1, s, "I" * 150))
    with open(os.path.join(d, "genes.fa"), "w") as f:
        for n, s in db:
            f.write(">%s\n%s\n" % (n, s))
    with open(os.path.join(d, "genes.sam"), "w") as f:
        for n, s in db:
            f.write("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)))
        f.writelines(ln if ln.endswith("\n") else ln + "\n" for ln in lines)
    open(os.path.join(d, "seeds.txt"), "w").write("".join("%s\t1\n" % g["name"] for g in genes))
    open(os.path.join(d, "bams.txt"), "w").write(os.path.join(d, "genes.sam") + "\n")
    assert stage4.main([os.path.join(d, "genes.fa"), os.path.join(d, "seeds.txt"), os.path.join(d, "bams.txt"), "-o", d, "-c", "4"]) == 0
    sam = os.path.join(d, "to_seed_otus.all.sam")
    fa = os.path.join(d, "0_otu_dir", "seed_otus.fasta")
    n_rec = sum(1 for ln in open(sam) if not ln.startswith("@"))
    assert n_rec > 0.9 * (3 * 900 + 3 * 150)
    expected = ""
    for roi in stage5.roi_list(fa + ".fai"):
        out, _ = T.run_oracle(stage5.straincall_argv(roi, fa, sam), d)
        expected += out
    got = stage5.strain_call(fa, sam, out_dir=os.path.join(d, "work"), prefix="rambl", streams=3)
    assert got == expected
    called = [s for s in got.split("\n") if s and not s.startswith(">")]
    worst = 0
    for g in genes:
        for edits in g["strains"]:
            strain = "".join(b for _, kind, b in synth._strain_columns(g["ref"], edits) if kind != "D")
            dist = min(x for x in (_edit(strain, c) for c in called) if x is not None)
            worst = max(worst, dist)
            assert dist <= len(strain) // 100, (g["name"], dist)
    print("worst strain edit distance", worst)
