"""The seeded gene profile (sc_profile_hits_seeded) restated in plain Python: the lossless seed length by
brute force over (identity columns, other columns), the (segment, gene) pairs that share a k-mer with Python sets, and the
longest common run of two slices, which is what the bound is about."""
import math
import re

import numpy as np

MATCH2, OTHER2 = 2, 4                  # doubled: an identity column +2, any other column costs 4 or more
SEED_MIN_K, SEED_MAX_K = 11, 16
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def least_score2(L, gene_bases, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46):
    """min2(L): the least doubled score of a segment of L bases with E <= T, None when even 2 L does not pass."""
    for s2 in range(1, MATCH2 * L + 1):
        if ka_k * float(L) * float(gene_bases) * math.exp(-ka_lambda * (0.5 * float(s2))) <= max_evalue:
            return s2
    return None


_GRID = {}


def _grid(min_identity, n=512):
    """Over i = 1..n identity columns and m = 0..n // 2 other columns: ceil(i / (m + 1)) where the identity test passes (a
    large number elsewhere), and the doubled score bound 2 i - 4 m."""
    if min_identity not in _GRID:
        i = np.arange(1, n + 1, dtype=np.int64)[:, None]
        m = np.arange(0, n // 2 + 1, dtype=np.int64)[None, :]
        ok = 100.0 * i.astype(np.float64) / (i + m).astype(np.float64) >= float(min_identity)
        _GRID[min_identity] = (np.where(ok, -(-i // (m + 1)), 1 << 30), MATCH2 * i - OTHER2 * m)
    return _GRID[min_identity]


def lossless_k(L, gene_bases, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46):
    """k*(L): the minimum of ceil(i / (m + 1)) over every (i, m) with i <= L, 100.0 * i / (i + m) >= I and 2 i - 4 m >= min2(L),
    by trying them all (m > L / 2 cannot have a positive score); None when the segment cannot pass."""
    s2 = least_score2(L, gene_bases, max_evalue, ka_lambda, ka_k)
    if s2 is None:
        return None
    run, score = _grid(min_identity)
    best = int(np.where(score[:L] >= s2, run[:L], 1 << 30).min())
    return None if best == 1 << 30 else best


def seed_length(seg_lens, gene_bases, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46):
    """K_seed of a call: the least k*(L) over the lengths that can pass, cut to 16; 0 below 11 or when none can pass."""
    ks = [lossless_k(L, gene_bases, min_identity, max_evalue, ka_lambda, ka_k) for L in sorted(set(seg_lens))]
    ks = [k for k in ks if k is not None]
    if not ks or min(ks) < SEED_MIN_K:
        return 0
    return min(min(ks), SEED_MAX_K)


def revcomp(s):
    """Reverse complement; a base outside ACGT stays outside."""
    return "".join(_COMP.get(c, "N") for c in reversed(s.upper()))


def kmers(s, k):
    """The k-mers of s that hold ACGT only."""
    return {m.group()[p:p + k] for m in re.finditer("[ACGT]+", s.upper()) for p in range(len(m.group()) - k + 1)} if k > 0 else {""}


def sharing_pairs(genes, segs, k):
    """{(segment, gene)}: the segment or its reverse complement has a k-mer (ACGT only) that lies inside the gene."""
    of_gene = [kmers(g, k) for g in genes]
    pairs = set()
    for s, seg in enumerate(segs):
        mine = kmers(seg, k) | kmers(revcomp(seg), k)
        pairs.update((s, g) for g, theirs in enumerate(of_gene) if mine & theirs)
    return pairs


def longest_common_run(a, b):
    """The length of the longest common substring of a and b made of ACGT only: the largest k at which they share a k-mer
    (sharing one of k bases, they share one of k - 1), found by bisection."""
    lo, hi = 0, min(len(a), len(b))
    while lo < hi:
        k = (lo + hi + 1) // 2
        if kmers(a, k) & kmers(b, k):
            lo = k
        else:
            hi = k - 1
    return lo


def hit_slices(hit, genes, segs):
    """The two slices of a restatement hit on the hit's strand: the segment's qfrom..qto (reverse-complemented on strand 1)
    and the gene's hfrom..hto (given from > to on strand 1)."""
    seg, gene, strand, qfrom, qto, hfrom, hto = hit[0], hit[1], hit[2], hit[6], hit[7], hit[8], hit[9]
    q = segs[seg][qfrom - 1:qto]
    lo, hi = min(hfrom, hto), max(hfrom, hto)
    return (revcomp(q) if strand else q), genes[gene][lo - 1:hi]


def has_common_run(a, b, k):
    """longest_common_run(a, b) >= k, without the bisection."""
    return bool(kmers(a, k) & kmers(b, k))
