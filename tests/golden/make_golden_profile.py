"""Rebuilds tests/golden/profile_counts: hit CSVs written here, each counted by the reference's own blastout2abundance.

    python tests/golden/make_golden_profile.py /path/to/reference

The reference's scripts/blastout2abundance.cpp is compiled into a temporary directory (neither the source nor the binary
is kept); caseNN.csv is its input, caseNN.raw its stdout, meta.json the source's sha256, the compiler line and each case's
thresholds.  tests/test_profile_host.py holds rambl_amd.profile.raw_abundance to the .raw bytes.

Rows: segment id, gene, identity, align_len, query from, query to, hit from, hit to, E-value, segment length.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "profile_counts")
COMPILE = ["g++", "-O2", "-std=c++11"]


def row(seg, gene, identity=150, align_len=150, e="1e-60", hfrom=1, hto=None, seg_len=150):
    hto = hfrom + align_len - 1 if hto is None else hto
    return "%s,%s,%d,%d,1,%d,%d,%d,%s,%d" % (seg, gene, identity, align_len, align_len, hfrom, hto, e, seg_len)


CASES = [
    # /1 /2 suffixes; mates that tie on one gene; mates on different genes at equal E; a three-way tie; an unpaired read;
    # E-values written as 1e-60 and 0.0
    dict(identity=95, evalue="1e-10", rows=[
        row("r1/1", "cA"), row("r1/2", "cA"),
        row("r2/1", "cA", e="0.0"), row("r2/2", "cB", e="0.0"),
        row("r3", "cA"), row("r3", "cB"), row("r3", "cC"),
        row("r4", "cB", e="0.0"),
        row("r5/1", "cC", e="1e-60"), row("r5/2", "cB", e="1e-60"), row("r5/2", "cC", e="1e-60"),
    ]),
    # .1 .2 suffixes; a later strictly better hit replaces the earlier ones; a row failing -I, one failing -E, a failing row
    # followed by a passing row of the same (segment, gene); a duplicate (segment, gene) row; genes whose byte order (Zeta <
    # alpha < beta) differs from their order of appearance; a reverse-strand hit (hit from > hit to)
    dict(identity=95, evalue="1e-10", rows=[
        row("s1.1", "beta", e="1e-20"), row("s1.1", "alpha", e="1e-40"), row("s1.2", "Zeta", e="1e-30"),
        row("s2", "beta", identity=90, align_len=100),                       # fails -I
        row("s3", "beta", e="1e-5"),                                         # fails -E
        row("s4", "alpha", identity=94, align_len=100), row("s4", "alpha", identity=96, align_len=100, e="1e-40"),
        row("s5", "Zeta", e="1e-50"), row("s5", "Zeta", e="1e-70"),           # duplicate: the second is dropped, E stays
        row("s5", "alpha", e="1e-60"),                                       # better than 1e-50: replaces Zeta
        row("s6.1", "beta", hfrom=400, hto=251), row("s6.2", "beta", e="0.0"),
        row("s7.1", "Zeta", identity=95, align_len=100, e="1e-10"),          # exactly on both thresholds: passes
    ]),
    # other thresholds; the mate with the worse E is dropped; one mate ties on two genes, the other hits one of them at the
    # same E: that gene is hit twice and takes the read whole
    dict(identity=90, evalue="1e-5", rows=[
        row("t1/1", "gA", e="1e-50"), row("t1/2", "gB", e="1e-30"),
        row("t2/1", "gA", e="1e-45"), row("t2/1", "gB", e="1e-45"), row("t2/2", "gA", e="1e-45"),
        row("t3", "gB", identity=90, align_len=100, e="1e-5"),
        row("t4", "gC", identity=89, align_len=100), row("t4", "gB", e="1e-4"),
        row("t5.1", "gC", e="2.5e-33"), row("t5.2", "gC", e="2.5e-33"), row("t5.2", "gA", e="2.5e-33"),
        row("t6", "gA"), row("t6", "gB"), row("t6", "gC"), row("t6", "gD"), row("t6", "gE"), row("t6", "gF"), row("t6", "gG"),
    ]),
]


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(argv[1], "scripts", "blastout2abundance.cpp")
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "blastout2abundance")
        subprocess.check_call(COMPILE + ["-o", exe, src])
        meta = {"source": "scripts/blastout2abundance.cpp", "sha256": hashlib.sha256(open(src, "rb").read()).hexdigest(),
                "compiler": " ".join(COMPILE + ["scripts/blastout2abundance.cpp"]), "cases": {}}
        for k, case in enumerate(CASES):
            name = "case%02d" % k
            csv = os.path.join(OUT, name + ".csv")
            with open(csv, "w") as f:
                f.write("".join(r + "\n" for r in case["rows"]))
            out = subprocess.run([exe, "-I", str(case["identity"]), "-E", case["evalue"], csv], stdout=subprocess.PIPE, check=True).stdout
            with open(os.path.join(OUT, name + ".raw"), "wb") as f:
                f.write(out)
            meta["cases"][name] = {"-I": case["identity"], "-E": case["evalue"]}
        with open(os.path.join(OUT, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
