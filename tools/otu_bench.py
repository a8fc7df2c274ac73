#!/usr/bin/env python3
"""The gene-against-gene kernel on a synthetic assembly: N genes of about 1 500 bases in families of near-copies,
every pair within 97 % through sc_gene_pairs.  Prints one JSON line per N: kernel ms, pairs per second and word steps per second
of the device call, and -- with --host-pairs K -- the same block code on one CPU core (tests/native/pairs_check.cpp built with
-O3, no sanitizer) on the first K scored pairs, with the ratio of the two word-step rates.  Not a test, and bench.py does not
read it."""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASES = b"ACGT"


def synthetic_genes(n, seed=816, length=1500, family=16, n_sub=12, n_indel=3):
    """n genes: families of `family` near-copies of a random root (up to n_sub substitutions and n_indel one-base insertions or
    deletions each), in a seeded shuffle."""
    rng = random.Random(seed)
    genes = []
    while len(genes) < n:
        root = bytearray(rng.choice(BASES) for _ in range(length + rng.randrange(-20, 21)))
        for _ in range(min(family, n - len(genes))):
            s = bytearray(root)
            for _ in range(rng.randrange(n_sub + 1)):
                p = rng.randrange(len(s))
                s[p] = rng.choice([b for b in BASES if b != s[p]])
            for _ in range(rng.randrange(n_indel + 1)):
                p = rng.randrange(len(s))
                if rng.random() < 0.5:
                    s.insert(p, rng.choice(BASES))
                else:
                    del s[p]
            genes.append(bytes(s))
    rng.shuffle(genes)
    return genes


def host_rate(genes, k, diff):
    """The first k pairs the length prefilter leaves, through the host build of the block code: (pairs, word steps, ms)."""
    lens = [len(g) for g in genes]
    pairs = []
    for a in range(len(genes)):
        for b in range(a + 1, len(genes)):
            if abs(lens[a] - lens[b]) <= (max(lens[a], lens[b]) * diff[0]) // diff[1]:
                pairs.append((a, b) if lens[a] <= lens[b] else (b, a))          # the shorter gene is the pattern, as in the library
                if len(pairs) == k:
                    break
        if len(pairs) == k:
            break
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pairs_check")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "pairs_check.cpp")])
        out = subprocess.run([exe, "time"], input=b"".join(genes[a] + b" " + genes[b] + b"\n" for a, b in pairs), stdout=subprocess.PIPE,
                             check=True).stdout.decode().split()
    fields = dict(zip(out[::2], out[1::2]))
    return int(fields["pairs"]), int(fields["word_steps"]), float(fields["ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-n", dest="sizes", type=int, nargs="+", default=[1024, 4096], help="genes per run [1024 4096]")
    ap.add_argument("--id", dest="identity", default="97")
    ap.add_argument("--repeat", type=int, default=3, help="device calls per size; the fastest kernel time is reported [3]")
    ap.add_argument("--host-pairs", dest="host_pairs", type=int, default=0, help="also time this many pairs on one CPU core [0: off]")
    ap.add_argument("-d", "--device", type=int, default=0)
    a = ap.parse_args()
    from rambl_amd import otu
    diff = otu.diff_from_identity(a.identity)
    for n in a.sizes:
        genes = synthetic_genes(n)
        runs = []
        for _ in range(a.repeat):
            pairs, stats = otu.pairs_within(genes, diff[0], diff[1], a.device, cap=1 << 22, with_stats=True)
            runs.append(stats)
        best = min(runs, key=lambda s: s["kernel_ms"])
        row = {"n_genes": n, "identity": a.identity, "pairs_found": len(pairs), "kernel_ms_all": [round(s["kernel_ms"], 3) for s in runs]}
        row.update({k: (round(v, 3) if k.endswith("_ms") else int(v)) for k, v in best.items()})
        row["pairs_per_s"] = round(best["pairs_scored"] / (best["kernel_ms"] / 1e3), 1)
        row["word_steps_per_s"] = round(best["word_steps"] / (best["kernel_ms"] / 1e3), 1)
        if a.host_pairs:
            hp, hs, hms = host_rate(genes, a.host_pairs, diff)
            row.update({"host_pairs": hp, "host_word_steps": hs, "host_ms": round(hms, 3), "host_word_steps_per_s": round(hs / (hms / 1e3), 1)})
            row["device_over_one_core"] = round(row["word_steps_per_s"] / row["host_word_steps_per_s"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
