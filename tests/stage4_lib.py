"""Helpers of the stage-4 tests: the plain C++ restatement of the alignment contract (tests/native/sw_check.cpp) and
synthetic inputs for it."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_sw_check(outdir):
    exe = os.path.join(str(outdir), "sw_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "sw_check.cpp")])
    return exe


def run_sw_check(exe, seeds, reads):
    """seeds: [str]; reads: [(seq, qual or '*')] -> [(AS, XS, seed, strand, pos, CIGAR, NM)]."""
    text = "S %d\n%s\nR %d\n%s\n" % (len(seeds), "\n".join(seeds), len(reads), "\n".join("%s %s" % r for r in reads))
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    rows = []
    for line in out.splitlines():
        f = line.split()
        rows.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], int(f[6])))
    return rows


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):
    out = list(s)
    for i in range(len(out)):
        if rng.random() < rate:
            out[i] = rng.choice([c for c in "ACGT" if c != out[i]])
    return "".join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def qual_string(rng, n, low=False):
    if low:
        return "".join(chr(33 + rng.randint(0, 40)) for _ in range(n))
    return "".join(chr(33 + rng.choice([30, 35, 38, 40, 41])) for _ in range(n))


def device_rows(got):
    """capi.AlignResult in the restatement's form."""
    return [(int(got.as_[i]), int(got.xs[i]), int(got.seed[i]), int(got.strand[i]) if got.seed[i] >= 0 else 0, int(got.pos[i]),
             got.cigar[i], int(got.nm[i])) for i in range(len(got.cigar))]


def compare_rows(reads, exp, got_rows, name="reads"):
    """Every field of every read, device against restatement; the first five differing records with their lengths."""
    bad = [(i, len(reads[i][0]), e, g) for i, (e, g) in enumerate(zip(exp, got_rows)) if g != e]
    assert len(got_rows) == len(exp) and not bad, "%s: %d of %d reads differ, first: %s" % (name, len(bad), len(exp), bad[:5])
