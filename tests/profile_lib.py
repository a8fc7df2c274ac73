"""Helpers of the gene-profile tests: the plain C++ restatement of the hit contract (tests/native/blast_hits_check.cpp), the
chain restatement hits -> rows -> counts -> table, and synthetic inputs."""
import os
import random
import subprocess

import stage4_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_hits_check(outdir):
    exe = os.path.join(str(outdir), "blast_hits_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "blast_hits_check.cpp")])
    return exe


def run_hits_check(exe, genes, segs, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46):
    """genes, segs: [str] -> [(segment, gene, strand, doubled score, identity, align_len, qfrom, qto, hfrom, hto, E text)]."""
    text = "G %d\n%s\nQ %d\n%s\n" % (len(genes), "\n".join(genes), len(segs), "\n".join(segs))
    out = subprocess.run([exe, repr(float(min_identity)), repr(float(max_evalue)), repr(float(ka_lambda)), repr(float(ka_k))],
                         input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    rows = []
    for line in out.splitlines():
        f = line.split()
        rows.append(tuple(int(x) for x in f[:10]) + (f[10],))
    return rows


def as_csv_fields(hit):
    """A restatement hit with its E-value as the hit CSV holds it."""
    from rambl_amd import profile
    return hit[:10] + (profile.format_evalue(float(hit[10])),)


def device_hits(res):
    """capi.ProfileHits in the restatement's form."""
    from rambl_amd import profile
    return [(int(res.seg[k]), int(res.gene[k]), int(res.strand[k]), int(round(2 * float(res.score[k]))), int(res.identity[k]),
             int(res.align_len[k]), int(res.qfrom[k]), int(res.qto[k]), int(res.hfrom[k]), int(res.hto[k]),
             profile.format_evalue(float(res.evalue[k]))) for k in range(len(res))]


def compare_hits(exe, genes, segs, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46, name="hits", cap=None, exp=None):
    """Every field of every hit, device against restatement (E as the hit CSV holds it), in (segment, gene) order; the first
    five differing records with their segment lengths.  Returns (expected hits, capi.ProfileHits)."""
    from rambl_amd import capi
    if exp is None:
        exp = run_hits_check(exe, genes, segs, min_identity, max_evalue, ka_lambda, ka_k)
    exp = [as_csv_fields(h) for h in exp]
    res = capi.profile_hits([g.encode() for g in genes], [s.encode() for s in segs], min_identity, max_evalue, ka_lambda, ka_k, cap=cap)
    got = device_hits(res)
    print("%s: thresholds -I %g -e %g: %d hits expected, %d from the device, %s" % (name, min_identity, max_evalue, len(exp), len(got), res.stats.as_dict()))
    assert got == sorted(got, key=lambda h: h[:2])
    bad = [(len(segs[e[0]]), e, g) for e, g in zip(exp, got) if e != g]
    assert len(got) == len(exp) and not bad, "%s: %d expected, %d got, %d differ, first differences: %s" % (name, len(exp), len(got), len(bad), bad[:5])
    assert res.stats.n_hits == len(exp)
    return exp, res


def rows_of(hits, seg_ids, seg_lens, gene_names):
    """The ten CSV columns (text) of restatement hits."""
    from rambl_amd import profile
    return [(seg_ids[h[0]], gene_names[h[1]], str(h[4]), str(h[5]), str(h[6]), str(h[7]), str(h[8]), str(h[9]),
             profile.format_evalue(float(h[10])), str(seg_lens[h[0]])) for h in hits]


def parity_dataset(seed=909):
    """>= 12 genes of 120-1 500 bases (a duplicate, a 3 % relative, one with Ns) and >= 500 segments of 60-512 bases in every
    bucket of rows per lane: mutated pieces that overhang gene ends, indels anywhere, Ns, random segments, either strand."""
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, n) for n in (120, 300, 450, 600, 800, 1000, 1200, 1500, 700, 900, 520, 640)]
    genes[5] = genes[5][:200] + "NNN" + genes[5][203:]
    genes[9] = L.mutate(rng, genes[4][:800] + L.rand_seq(rng, 100), 0.03)     # a close relative of gene 4
    genes.append(genes[3])                                                       # a duplicated gene: every hit ties
    lengths = [60, 64, 65, 100, 128, 150, 150, 192, 200, 250, 256, 300, 320, 384, 400, 448, 449, 500, 512]
    segs = []
    for k in range(540):
        n = lengths[k % len(lengths)]
        g = genes[rng.randrange(len(genes))]
        a = rng.randint(-n // 4, max(len(g) - 3 * n // 4, -n // 4))
        frag = g[max(a, 0):max(a, 0) + n + 8]
        if a < 0:
            frag = L.rand_seq(rng, -a) + frag
        if len(frag) < n + 8:
            frag += L.rand_seq(rng, n + 8 - len(frag))
        kind = k % 9
        s = L.mutate(rng, frag, 0.08 if kind == 5 else 0.02)
        if kind in (1, 2):                                                       # indels anywhere
            for _ in range(kind):
                p = rng.randint(5, n - 5)
                s = s[:p] + s[p + rng.randint(1, 4):] if rng.random() < 0.5 else s[:p] + L.rand_seq(rng, rng.randint(1, 4)) + s[p:]
        elif kind == 3:
            s = "".join("N" if rng.random() < 0.03 else c for c in s)
        elif kind == 4:
            s = L.rand_seq(rng, n)
        s = s[:n]
        if len(s) < n:
            s += L.rand_seq(rng, n - len(s))
        if rng.random() < 0.5:
            s = L.revcomp(s)
        segs.append(s)
    return genes, segs


def mixture_dataset(seed=31):
    """The end-to-end input: three genes of three strains each as the "assembly" (nine sequences), and three samples whose
    reads mix every gene's strains 4 : 2 : 1 in another order per sample.  Returns (names, sequences, samples) with
    samples = [(sample name, SAM lines, {gene index: (proportion of strain 0, 1, 2)})]."""
    from rambl_amd import synth
    rng = random.Random(seed)
    names, seqs = [], []
    for k in range(3):
        g = synth.make_gene(700 + k, glen=900, n_strains=3, n_reads=0, n_sub=36, n_ins=1, n_del=1, name="gene%d" % k)
        for s, edits in enumerate(g["strains"]):
            names.append("gene%d_strain%d" % (k, s))
            seqs.append("".join(b for _, kind, b in synth._strain_columns(g["ref"], edits) if kind != "D"))
    orders = [(4, 2, 1), (1, 4, 2), (2, 1, 4)]
    samples = []
    for si in range(3):
        lines = []
        mix = {}
        for k in range(3):
            w = orders[(si + k) % 3]
            mix[k] = w
            for s in range(3):
                src = seqs[3 * k + s]
                for r in range(16 * w[s]):
                    qn = "smp%d_g%d_s%d_%d" % (si, k, s, r)
                    paired = r % 3 == 0
                    a = rng.randint(0, len(src) - 320)
                    pieces = [(a, 0x41), (a + rng.randint(160, 170), 0x81)] if paired else [(a, 0)]
                    for p, flag in pieces:
                        read = L.mutate(rng, src[p:p + 150], 0.004)
                        if rng.random() < 0.5:
                            read, flag = L.revcomp(read), flag | 0x10       # SEQ as stored: on the reference strand of its mapping
                        lines.append("%s\t%d\t%s\t%d\t42\t150M\t*\t0\t0\t%s\t%s\n" % (qn, flag, names[3 * k + s], p + 1, read, "I" * 150))
        samples.append(("sample%d" % si, lines, mix))
    return names, seqs, samples


def write_mixture(outdir, names, seqs, samples):
    fa = os.path.join(str(outdir), "assembly.fa")
    with open(fa, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))
    sams = []
    for sample, lines, _ in samples:
        path = os.path.join(str(outdir), sample + ".sam")
        with open(path, "w") as f:
            for n, s in zip(names, seqs):
                f.write("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)))
            f.writelines(lines)
        sams.append(path)
    return fa, sams


def sam_records(lines):
    """(QNAME, FLAG, SEQ, QUAL) of SAM text lines, as capi.NativeAln.walk yields them."""
    out = []
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        out.append((f[0].encode(), int(f[1]), f[9].encode(), f[10].encode()))
    return out


def expected_table(exe, names, seqs, sample, lines, relative=False):
    """The chain restatement hits -> rows -> raw_abundance -> table for one sample, and the counts."""
    from rambl_amd import profile
    segments = profile.extract_segments(sam_records(lines))
    hits = run_hits_check(exe, seqs, [s.decode() for _, s in segments])
    rows = rows_of(hits, [q.decode() for q, _ in segments], [len(s) for _, s in segments], names)
    counts = profile.raw_abundance(rows)
    return profile.format_table(sample, counts, relative), dict(counts)
