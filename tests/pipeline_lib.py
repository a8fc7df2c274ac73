"""Helpers of the whole-pipeline tests: a synthetic world for rambl_amd.pipeline (gene database, phylogeny, taxonomy, the
reads of the samples split over SAM files, a data_info file), and the CPU route from that world to the seed list
(oracle/depth_oracle.py -> stage1.bed_text -> stage 2 -> stage 3) that fixes what the GPU run has to find."""
import os
import random
import sys

import stage4_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def make_world(d, n_clades=3, glen=700, n_strains=2, n_reads=900, rel_reads=150, n_files=2, seed=7, first_gene_seed=500,
               n_sub=6, n_ins=1, n_del=1):
    """Under `d`: `n_clades` clades, each a gene with the reads of `n_strains` strains (synth.make_gene) and a 3 %-divergent
    relative with `rel_reads` reads of its own; one clade of two genes without any read; one gene with 20 reads of 70 bases
    on the first tenth of its length.  Gene k of clade c is named 1000 + 10 c + k.  The tree puts a relative at 0.03 from its
    gene and every clade at 1.0 or more from the next.  `n_reads`: a number, or (low, high) for a draw per gene.
    -> dict(data_info, clades=[[gene, relative]], quiet=[names], thin=name, genes=[make_gene dicts], bams=[paths],
    files=[{reference: [(flag, pos, cigar)]}] (the records as oracle/depth_oracle.py takes them), plus the data_info keys)."""
    from rambl_amd import synth
    os.makedirs(d, exist_ok=True)
    rng = random.Random(seed)
    db, lines, genes, clades = [], [], [], []
    for c in range(n_clades):
        n = n_reads if isinstance(n_reads, int) else random.Random((first_gene_seed + c) * 7919 + 1).randint(*n_reads)
        g = synth.make_gene(first_gene_seed + c, glen=glen, n_strains=n_strains, n_reads=n, rlen=150, err=0.003, n_sub=n_sub,
                            n_ins=n_ins, n_del=n_del, name="%d" % (1000 + 10 * c))
        genes.append(g)
        rel_name = "%d" % (1000 + 10 * c + 1)
        rel = L.mutate(rng, g["ref"], 0.03)
        db += [(g["name"], g["ref"]), (rel_name, rel)]
        clades.append([g["name"], rel_name])
        lines += g["sam_lines"]
        for k in range(rel_reads):
            a = rng.randint(0, len(rel) - 150)
            s = L.mutate(rng, rel[a:a + 150], 0.003)
            lines.append("r%s_%d\t0\t%s\t%d\t60\t150M\t*\t0\t0\t%s\t%s" % (rel_name, k, rel_name, a + 1, s, "I" * 150))
    quiet = ["%d" % (1000 + 10 * n_clades + k) for k in range(2)]
    thin = "%d" % (1000 + 10 * (n_clades + 1))
    db += [(q, L.rand_seq(rng, glen)) for q in quiet] + [(thin, L.rand_seq(rng, glen))]
    for k in range(20):
        s = L.mutate(rng, db[-1][1][:70], 0.003)
        lines.append("r%s_%d\t0\t%s\t1\t60\t70M\t*\t0\t0\t%s\t%s" % (thin, k, thin, s, "I" * 70))

    w = dict(clades=clades, quiet=quiet, thin=thin, genes=genes, bams=[], files=[])
    p = {k: os.path.join(d, v) for k, v in (("GeneSeq", "genes.fa"), ("GeneIndex", "genes.fa.fai"), ("GeneTree", "genes.nwk"),
                                            ("GeneTax", "genes.tax"), ("GeneAlign", "genes.aln.fa"), ("BamFiles", "bams.txt"))}
    with open(p["GeneSeq"], "w") as f, open(p["GeneIndex"], "w") as fai, open(p["GeneAlign"], "w") as aln:
        off = 0
        for n, s in db:
            f.write(">%s\n%s\n" % (n, s))
            aln.write(">%s\n%s\n" % (n, s))
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (n, len(s), off + len(n) + 2, len(s), len(s) + 1))
            off += len(n) + 2 + len(s) + 1
    groups = ["(%s:0.01,%s:0.02):0.5" % tuple(c) for c in clades + [quiet]] + ["%s:0.6" % thin]
    open(p["GeneTree"], "w").write("(" + ",".join(groups) + ");\n")
    with open(p["GeneTax"], "w") as f:
        for ci, c in enumerate(clades + [quiet, [thin]]):
            for n in c:
                f.write("%s\tk__Bacteria; g__clade%d\n" % (n, ci))
    for i in range(n_files):                                   # the reads of the samples: every n_files-th record per file
        path = os.path.join(d, "sample%d.sam" % i)
        recs = {}
        with open(path, "w") as f:
            for n, s in db:
                f.write("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)))
            for ln in lines[i::n_files]:
                f.write(ln + "\n")
                fld = ln.split("\t")
                recs.setdefault(fld[2], []).append((int(fld[1]), int(fld[3]), fld[5]))
        w["bams"].append(path)
        w["files"].append(recs)
    open(p["BamFiles"], "w").write("".join(b + "\n" for b in w["bams"]))
    w["data_info"] = os.path.join(d, "data_info.txt")
    open(w["data_info"], "w").write("".join("%s = %s\n" % (k, p[k]) for k in ("GeneSeq", "BamFiles", "GeneTax", "GeneIndex", "GeneTree",
                                                                               "GeneAlign")))
    w.update(p)
    return w


def cpu_files(w, d):
    """Stages 1-2 of the world on the CPU: gene_depth.txt from the stage-1 oracle printed by stage1.bed_text, gene_abundance.txt
    from stage 2 -> (depth file, abundance file)."""
    import depth_oracle
    from rambl_amd import samio, stage1, stage2
    os.makedirs(d, exist_ok=True)
    refs = sorted(((n, int(l)) for n, l in samio.read_fai(w["GeneIndex"])), key=lambda r: (stage1._numeric_key(r[0]), r[0]))
    iv = depth_oracle.stage1(w["files"], refs, max_gap=10)
    depth, abun = os.path.join(d, "gene_depth.txt"), os.path.join(d, "gene_abundance.txt")
    open(depth, "w").write(stage1.bed_text([(refs[ri][0], s, e, sm, n) for ri, s, e, sm, n in iv]))
    open(abun, "w").write("".join(ln + "\n" for ln in stage2.gene_abundance(depth, w["GeneIndex"])))
    return depth, abun


def clade_of(w, gene):
    for ci, c in enumerate(w["clades"]):
        if gene in c:
            return ci
    return None
