"""Named edge cases of the two alignment kernel families: stage 4 (rambl_amd/csrc/sc_align.hip, restated in
tests/native/sw_check.cpp) and the gene profile (rambl_amd/csrc/sc_profile.hip and sc_profile_dp.hpp, restated in tests/native/blast_hits_check.cpp).
Both run one sweep and one traceback window, rambl_amd/csrc/sc_wave_dp.hpp (sweep, trace_window, sweep_block); stage4_window
and profile_window below restate that window, the launch limits are that header's.

A case is a function of a seed.  It returns the inputs and a property check: a function of the restatement's output that
raises unless the input reaches the edge the case is named for -- a generator that silently loses its edge fails on the CPU
(tests/test_align_edges_host.py) before the device comparison (tests/test_stage4_edges_gpu.py,
tests/test_profile_edges_gpu.py) could pass for nothing.  Which instantiation runs what: a read or segment of L bases runs
k_sw_score<R> / k_sw_trace<R> / k_bl_score<R> / k_bl_trace<R> with R = ceil(L / 64); `every_bucket` holds an aligned read
(a hit) for every R = 1..8, `score_stride` makes the grid-stride loop of the score kernels iterate, `trace_stride` that of the
traceback kernels."""
import math
import random
import re

import profile_lib as PL
import stage4_lib as L

MAX_READ, MAX_SEED, TB_COLS, GBAR = 512, 8192, 128, 4
SCORE_BLOCKS, SCORE_WAVES, TRACE_BLOCKS = 16384, 4, 8192            # the launch limits of sc_wave_dp.hpp


class Stage4Case:
    def __init__(self, name, seeds, reads, check):
        self.name, self.seeds, self.reads, self.check = name, seeds, reads, check

    def key(self):
        return (self.seeds, self.reads)


class ProfileCase:
    def __init__(self, name, genes, segs, check, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46):
        self.name, self.genes, self.segs, self.check = name, genes, segs, check
        self.min_identity, self.max_evalue, self.ka_lambda, self.ka_k = min_identity, max_evalue, ka_lambda, ka_k

    def key(self):
        return (self.genes, self.segs, self.min_identity, self.max_evalue, self.ka_lambda, self.ka_k)

    def thresholds(self):
        return (self.min_identity, self.max_evalue, self.ka_lambda, self.ka_k)


def need(cond, what):
    if not cond:
        raise AssertionError("the case misses its edge: " + what)


def bucket(n):
    return (n + 63) // 64


def valid_score(n):
    """The least integer score of a valid alignment of a read of n bases (20 + 8 ln n, in double)."""
    return int(math.ceil(20.0 + 8.0 * math.log(float(n))))


def cigar_ops(cigar):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDS])", cigar)] if cigar != "*" else []


def ref_span(cigar):
    return sum(n for n, op in cigar_ops(cigar) if op in "MD")


def clips(cigar):
    ops = cigar_ops(cigar)
    return (ops[0][0] if ops and ops[0][1] == "S" else 0), (ops[-1][0] if len(ops) > 1 and ops[-1][1] == "S" else 0)


def gap_rows(cigar):
    """[(op, first read row, last read row)] of the gaps: an I over the rows it inserts, a D on the row before it (the row
    whose E cell opens it)."""
    out, row = [], 0
    for n, op in cigar_ops(cigar):
        if op == "I":
            out.append(("I", row, row + n - 1))
        elif op == "D":
            out.append(("D", row - 1, row - 1))
        if op in "MIS":
            row += n
    return out


def stage4_window(read_len, as_, pos, cigar):
    """The traceback window of k_sw_trace recomputed from a SAM row: the alignment ends at row i and 0-based
    column j; the window is rows 0..i and columns j0..j with j0 = max(0, j - (i + 1) - floor((2 (i + 1) - AS) / 3) + 1).
    Returns j0, the number of window columns, the number of 128-column blocks, the window column of the first aligned base
    and the gap runs [(op, first window column, last window column)] (an I run sits in the column of the base before it)."""
    nrows = read_len - clips(cigar)[1]
    jend = pos - 1 + ref_span(cigar) - 1
    nd = max(0, (2 * nrows - as_) // 3)
    j0 = max(0, jend - nrows - nd + 1)
    ncol = jend - j0 + 1
    col, runs = pos - 1 - j0, []
    for n, op in cigar_ops(cigar):
        if op == "M":
            col += n
        elif op == "D":
            runs.append(("D", col, col + n - 1))
            col += n
        elif op == "I":
            runs.append(("I", col - 1, col - 1))
    return {"j0": j0, "ncol": ncol, "blocks": (ncol - 1) // TB_COLS + 1, "start": pos - 1 - j0, "runs": runs}


def profile_window(seg_len, hit):
    """The traceback window of k_bl_trace recomputed from a hit of the restatement:
    j0 = max(0, j - (i + 1) - floor((2 (i + 1) - S2) / 5) + 1) with S2 the doubled score."""
    _, _, strand, s2, _, _, qfrom, qto, hfrom, hto, _ = hit
    iend = seg_len - qfrom if strand else qto - 1
    jend, jstart = (hfrom - 1, hto - 1) if strand else (hto - 1, hfrom - 1)
    nrows = iend + 1
    nd = max(0, (2 * nrows - s2) // 5)
    j0 = max(0, jend - nrows - nd + 1)
    ncol = jend - j0 + 1
    return {"j0": j0, "ncol": ncol, "blocks": (ncol - 1) // TB_COLS + 1, "start": jstart - j0}


def py_stage4_dp(read, qual, seed):
    """The stage-4 DP of one short read (forward strand) against one seed in plain Python, for the property checks that need
    a cell the SAM row does not show.  Returns (H, E, F) as lists of rows, row / column 0 outside the matrix."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    n, m, neg = len(read), len(seed), -10 ** 9
    q = [40] * n if qual == "*" else [max(0, ord(c) - 33) for c in qual]
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[neg] * (m + 1) for _ in range(n + 1)]
    F = [[neg] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        a = code.get(read[i - 1].upper(), -1)
        for j in range(1, m + 1):
            b = code.get(seed[j - 1].upper(), -1)
            if GBAR <= i - 1 < n - GBAR:
                E[i][j] = max(H[i][j - 1] - 8, E[i][j - 1] - 3 if E[i][j - 1] != neg else neg)
                F[i][j] = max(H[i - 1][j] - 8, F[i - 1][j] - 3 if F[i - 1][j] != neg else neg)
            s = -1 if a < 0 or b < 0 else 2 if a == b else -(2 + (4 * min(q[i - 1], 40)) // 40)
            H[i][j] = max(0, H[i - 1][j - 1] + s, E[i][j], F[i][j])
    return H, E, F


def f_tie_on_path(read, qual, seed, pos, cigar):
    """True when the traced alignment passes an F cell where extending and opening tie (F[i-1][j] - 3 == H[i-1][j] - 8): the
    contract extends there, so the insertion run grows instead of closing."""
    H, E, F = py_stage4_dp(read, qual, seed)
    row, col = clips(cigar)[0], pos - 1                              # the next read row / seed column, 0-based
    for n, op in cigar_ops(cigar)[1 if clips(cigar)[0] else 0:]:
        if op == "M":
            row, col = row + n, col + n
        elif op == "D":
            col += n
        elif op == "I":
            for i in range(row + 1, row + n):                        # 0-based rows of the run after its first base
                if F[i][col] - 3 == H[i][col] - 8 and F[i + 1][col] == F[i][col] - 3:
                    return True
            row += n
    return False


def _place(rng, src, a, n, strand, edit=None):
    """A read of n bases copied from src[a:], edited by `edit`, on either strand."""
    r = src[a:a + n]
    if edit:
        r = edit(r)
    return L.revcomp(r) if strand else r


# ------------------------------------------------------------------------------------------------------------ stage 4

def _bucket_lengths():
    return [1, 2, 7, 8, 9, 12] + [64 * k + d for k in range(1, 8) for d in (-1, 0, 1)] + [511, 512]


def s4_every_bucket(seed=11):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 560) for _ in range(3)]
    reads = []
    for n in _bucket_lengths():
        for v in range(4):
            src = seeds[rng.randrange(3)]
            a = rng.randint(0, len(src) - n - 2)
            r = src[a:a + n + 2]
            if n >= 40:                                              # two substitutions, then an indel in the interior
                for p in (n // 4, 3 * n // 4):
                    r = r[:p] + rng.choice([c for c in "ACGT" if c != r[p]]) + r[p + 1:]
            if n >= 24:
                p = n // 2
                r = r[:p] + rng.choice([c for c in "ACGT" if c != r[p]]) + r[p:] if v in (0, 3) else r[:p] + r[p + 1:]
            r = r[:n]
            if v in (1, 3):
                r = L.revcomp(r)
            reads.append((r, L.qual_string(rng, n, low=(v == 2)) if v in (0, 2) else "*"))

    def check(rows):
        for r in range(1, 9):
            mine = [e for (s, _), e in zip(reads, rows) if bucket(len(s)) == r and e[2] >= 0]
            need(any(e[3] == 0 for e in mine) and any(e[3] == 1 for e in mine), "an aligned read on either strand at R = %d" % r)
            need(any("I" in e[5] for e in mine) and any("D" in e[5] for e in mine), "a CIGAR with I and one with D at R = %d" % r)
        short = [e for (s, _), e in zip(reads, rows) if len(s) < 2 * GBAR + 1]
        need(len(short) == 16 and all(e[0] >= 0 for e in short), "AS of the reads below 9 bases")
    return Stage4Case("every_bucket", seeds, reads, check)


def s4_top_score(seed=12):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 600), L.rand_seq(rng, 512)]
    reads = [(_place(rng, seeds[0], 40, 512, 0), "*"), (_place(rng, seeds[0], 88, 512, 1), L.qual_string(rng, 512)),
             (_place(rng, seeds[1], 0, 512, 0), L.qual_string(rng, 512, low=True)), (_place(rng, seeds[1], 0, 512, 1), "*")]

    def check(rows):
        need(sum(e[0] == 2 * MAX_READ for e in rows) == 4, "AS == 1024 (the top of the key's score field)")
        need({e[3] for e in rows} == {0, 1}, "both strands")
    return Stage4Case("top_score", seeds, reads, check)


def s4_short_seeds(seed=13):
    rng = random.Random(seed)
    lens = [1, 2, 3, 5, 31, 63, 64, 65, 127, 128, 129]
    seeds = [L.rand_seq(rng, n) for n in lens]
    reads, owner = [], []
    for k, s in enumerate(seeds):
        for j, n in enumerate((100, 300, 512)):
            n = max(n, len(s) + 20)
            a = rng.randint(5, n - len(s) - 5)
            r = L.rand_seq(rng, a) + s + L.rand_seq(rng, n - a - len(s))
            reads.append((L.revcomp(r) if (k + j) % 2 else r, "*" if j else L.qual_string(rng, n)))
            owner.append(k)

    def check(rows):
        def whole(k):
            return any(o == k and e[2] == k and e[4] == 1 and ref_span(e[5]) == lens[k] and min(clips(e[5])) > 0
                       for o, e in zip(owner, rows))
        for k in (4, 5, 6, 7):
            need(whole(k), "a read clipped on both ends over the whole seed of %d bases" % lens[k])
        need(any(lens[o] < 5 and len(r[0]) == 512 for o, r in zip(owner, reads)), "a seed shorter than the wavefront's diagonal")
    return Stage4Case("short_seeds", seeds, reads, check)


def s4_long_seeds(seed=14):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, n) for n in (8192, 8191, 4097)]
    reads = []
    for k, s in enumerate(seeds):
        n = 512 if k == 0 else 100
        reads.append((_place(rng, s, len(s) - n, n, k % 2), "*"))                     # ends on the last base
        reads.append((_place(rng, s, 0, n, 1 - k % 2), L.qual_string(rng, n)))        # starts on the first
        reads.append((_place(rng, s, len(s) - 70, 60, 0), "*"))                       # ends 10 before the last
    reads.append((_place(rng, seeds[0], 8192 - 150, 150, 1), "*"))

    def check(rows):
        need(any(e[2] == 0 and e[4] + ref_span(e[5]) - 1 == MAX_SEED for e in rows), "an alignment ending on column 8192")
        need(any(e[2] == 1 and e[4] + ref_span(e[5]) - 1 == 8191 for e in rows), "an alignment ending on column 8191")
        need(any(e[2] >= 0 and e[4] == 1 for e in rows), "an alignment with POS == 1")
        need(any(e[2] == 0 and e[3] == 1 and e[4] + ref_span(e[5]) - 1 == MAX_SEED for e in rows), "... on the reverse strand")
    return Stage4Case("long_seeds", seeds, reads, check)


def _split_read(src, p, a, n, gap):
    """n bases of src from p with `gap` seed bases left out after the first a (gap > 0), or -gap foreign bases put in."""
    if gap >= 0:
        return src[p:p + a] + src[p + a + gap:p + n + gap]
    ins = "".join("ACGT"[(("ACGT".index(src[p + a]) + 1 + k) % 4)] for k in range(-gap))
    return src[p:p + a] + ins + src[p + a:p + n + gap]


def s4_window_bound(seed=15):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 900), L.rand_seq(rng, 300)]
    src = seeds[0]
    reads, meta = [], []

    def add(p, a, n, gap, strand=0):
        r = _split_read(src, p, a, n, gap)
        assert len(r) == n
        reads.append((L.revcomp(r) if strand else r, "*"))
        meta.append((p, a, n, gap))
    for gap in (1, 20, 60, 120, 160, 166, 167, 168, 169, 170):                        # 168 is the largest that joins at 512
        add(100, 256, 512, gap, gap % 2)
    for gap in (1, 30, 64, 65, 66, 67):                                               # (200 - 5) / 3 = 65
        add(3, 100, 200, gap)                                                         # near the seed start: the window clamps
        add(400, 100, 200, gap, 1)                                                    # deep inside
    for gap in (-1, -5, -20, -40, -60):
        add(150, 256, 512, gap)
        add(2, 150, 300, gap)
    for a in range(20, 20 + TB_COLS):                                                 # the cut at every offset of a block
        add(300, a, 200, 3)
        add(300, a, 200, -2)
        add(351, a, 200, 3)                                          # another context: equal neighbours move a gap to the left
    add(200, 100, 512, 50)                                                            # a D run over window columns 127 | 128
    add(200, 250, 512, 10)                                                            # ... and 255 | 256
    add(150, 250, 512, -2)                                                            # an I run on window column 256

    def check(rows):
        win = [stage4_window(len(r[0]), e[0], e[4], e[5]) if e[2] >= 0 else None for r, e in zip(reads, rows)]
        need(any(e[5] == "256M168D256M" for e in rows), "the largest deletion that joins at L = 512")
        need(all("D" not in e[5] for m, e in zip(meta, rows) if m[2] == 512 and m[3] > 168), "a larger one does not join")
        need(any(w and w["j0"] > 0 and w["start"] <= 1 and w["runs"] for w in win), "an alignment that starts <= 1 column after its window")
        need(all(w["start"] >= 1 for w in win if w and w["j0"] > 0 and w["runs"] and w["runs"][0][0] == "D"),
             "the 5 of a gap's cost leaves one column: no alignment with a deletion starts on its window's first column")
        need(any(w and w["j0"] == 0 and w["runs"] and w["start"] + 1 < w["ncol"] for w in win), "a window clamped at column 0")
        need(any(w and w["blocks"] >= 3 for w in win), "a window of three or more blocks")
        runs = [r for w in win if w for r in w["runs"]]
        for edge in (TB_COLS, 2 * TB_COLS):
            need(any(op == "D" and a <= edge - 1 and b >= edge for op, a, b in runs), "a D run over window columns %d | %d" % (edge - 1, edge))
            need(any(op == "I" and a == edge for op, a, b in runs), "an I run on window column %d" % edge)
        # equal neighbours let the traceback move a gap to the left, so a few offsets stay empty
        need(len({a % TB_COLS for op, a, b in runs if op == "D"}) >= TB_COLS - TB_COLS // 8, "a deletion at (nearly) every offset of a block")
    return Stage4Case("window_bound", seeds, reads, check)


def s4_gbar_rows(seed=16):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 300)]
    reads, n = [], 60
    for row in list(range(0, 7)) + list(range(n - 7, n)):
        for k, kind in enumerate(("del", "ins")):
            a = rng.randint(0, 200)
            r = seeds[0][a:a + n + 1]
            if kind == "del":                                        # the seed base after read row `row` is left out
                r = r[:row + 1] + r[row + 2:]
            else:                                                    # read row `row` is a base the seed does not have
                r = r[:row] + rng.choice([c for c in "ACGT" if c != r[row] and c != r[row - 1]]) + r[row:]
            r = r[:n]
            reads.append((L.revcomp(r) if (row + k) % 3 == 0 else r, "*"))
    for n2 in (9, 10):                                               # one and two rows where a gap may open; never valid
        for row in (3, 4, 5):
            r = seeds[0][50:50 + n2 + 1]
            reads.append((r[:row + 1] + r[row + 2:], "*"))

    def check(rows):
        gaps = [(len(r[0]), g) for r, e in zip(reads, rows) if e[2] >= 0 for g in gap_rows(e[5])]
        # a gap on row L - 5 is allowed but never chosen: the 4 rows after it score at most 8, what the gap costs, and the tie
        # goes to the smaller end column (the clipped alignment).  Row L - 6 is the last one where a gap pays.
        need(any(a == GBAR for n_, (op, a, b) in gaps) and any(b == n_ - GBAR - 2 for n_, (op, a, b) in gaps),
             "a gap on row 4 and one on row L - 6")
        need(any(e[5] == "56M4S" for e in rows) and any(e[5] == "4S56M" for e in rows), "a gap on a barred row turns into a clip")
        need(all(a >= GBAR and b < n_ - GBAR for n_, (op, a, b) in gaps), "no gap in a barred row")
        need({op for _, (op, a, b) in gaps} == {"I", "D"}, "both kinds of gap")
        need(all(e[2] < 0 for r, e in zip(reads, rows) if len(r[0]) <= 10), "reads of 9 and 10 bases stay unaligned")
    return Stage4Case("gbar_rows", seeds, reads, check)


def s4_ties(seed=17):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, rng.randint(20, 40)) for _ in range(2100)]
    seeds[3] = L.rand_seq(rng, 40)
    half = L.rand_seq(rng, 20)
    seeds[10] = half + L.revcomp(half)                               # its own reverse complement
    unit = "ACGGTCATTG"
    seeds[11] = unit * 6                                             # a tandem repeat longer than the read
    body = L.rand_seq(rng, 36)
    seeds[12] = body + "A" + "CGT" + "A"                             # one mismatch then three matches: + 0 at Q 40
    seeds[13] = "A" * 30                                             # homopolymers shorter than their reads
    seeds[14] = "C" * 31
    base = L.rand_seq(rng, 40)
    seeds[15] = base
    seeds[16] = base[:12] + "N" + base[13:26] + "".join("ACGT"[3 - "ACGT".index(c)] for c in base[26:])
    seeds[2050] = L.rand_seq(rng, 40)
    seeds.append(seeds[3])                                           # the duplicate: index 2100
    reads = [(seeds[3], "*"), (L.revcomp(seeds[3]), "*"), (seeds[10], "*"), (unit * 4, "*"),
             (body + "G" + "CGT", "*"),
             ("A" * 50, "*"), ("A" * 100, "*"), ("C" * 100, "*"), ("C" * 130, "*"), ("G" * 100, "*"),
             (base, "*"), (base[:36], "*"), (base[:30], "*"), (seeds[2050], "*"), (L.revcomp(seeds[2050]), "*")]

    def check(rows):
        need(rows[0][2] == 3 and rows[0][1] == rows[0][0] == 80 and rows[1][2] == 3 and rows[1][3] == 1, "the duplicate goes to the lower seed, XS == AS")
        need(rows[2][2] == 10 and rows[2][3] == 0 and rows[2][1] == rows[2][0], "the palindrome on the forward strand, XS == AS from the reverse")
        need(rows[3][2] == 11 and rows[3][4] == 1 and rows[3][5] == "40M", "the repeat at its smallest end column")
        need(rows[4][2] == 12 and rows[4][0] == 72 and rows[4][5] == "36M4S", "the earlier of two cells of equal score on one diagonal")
        need(rows[5][2] == 13 and rows[5][5] == "30M20S" and rows[6][5] == "30M70S", "the smallest end row, one row per lane and two")
        need(rows[7][2] == 14 and rows[7][5] == "31M69S" and rows[8][5] == "31M99S" and rows[8][3] == 0, "the smallest end row inside one lane's rows")
        need(rows[9][2] == 14 and rows[9][3] == 1 and rows[9][5] == "31M69S", "the same on the reverse strand")
        H = py_stage4_dp(base, "*", seeds[16])[0]
        second = max(max(r) for r in H)
        need(second == 49 == valid_score(40) - 1 and rows[10][2] == 15 and rows[10][1] == -1, "XS left out one below the least valid score")
        need(valid_score(36) == 49 and rows[11][2] == 15 and rows[11][1] == 49, "XS printed on the least valid score")
        need(valid_score(30) < 49 and rows[12][2] == 15 and rows[12][1] == 49, "XS printed above it")
        need(rows[13][2] == 2050 and rows[14][2] == 2050 and rows[14][3] == 1, "a seed index above 2^11")
    return Stage4Case("ties", seeds, reads, check)


def s4_alphabet_quality(seed=18):
    rng = random.Random(seed)
    s = L.rand_seq(rng, 300)
    s = s[:100] + "NNNNN" + s[105:200] + "R" + s[201:230] + "y" + s[231:]
    seeds = [s, L.rand_seq(rng, 200).lower()]
    reads = [(s[20:180].lower(), "*"), (s[60:160], "*"), (L.revcomp(s[60:160].replace("N", "A")), "*"),
             (seeds[1][10:170].upper(), "*"), (s[150:280], L.qual_string(rng, 130))]
    r = s[10:70]
    r = r[:30] + [c for c in "ACGT" if c != r[30]][0] + r[31:]
    for q in range(0, 51):
        reads.append((r, "I" * 30 + chr(33 + q) + "I" * 29))
    reads.append((r, "*"))
    reads.append((r[:20] + "NNN" + r[23:], "*"))
    reads.append((r[:20] + "KMS" + r[23:], "*"))

    def check(rows):
        need(all(e[2] >= 0 for e in rows), "every read aligns")
        need(rows[1][4] <= 100 - 60 + 1 + 60 and rows[1][4] + ref_span(rows[1][5]) - 1 >= 105 and "D" not in rows[1][5] and "I" not in rows[1][5],
             "a read aligned across the N run")
        as_q = [rows[5 + q][0] for q in range(51)]
        need(sorted(set(as_q), reverse=True) == [120 - 2 - 2 - k for k in range(5)], "the five mismatch penalties by quality")
        need(as_q[9] != as_q[10] and as_q[40] == as_q[50] == rows[56][0], "AS moves with the quality at the mismatch, Q > 40 and * as Q 40")
        need(rows[57][0] == rows[58][0] == 2 * 56 - 6 - 3, "N and the other IUPAC letters score -1")
    return Stage4Case("alphabet_quality", seeds, reads, check)


def s4_most_operations(seed=19):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 700), "CCACAAAACCACAAAACCACAAACAAAAAAAACCAAAACCACCAACACCACACCCCCACC"]
    reads = []
    for n in (512, 300, 450):
        out, p, k = "", 30, 0
        while len(out) < n:
            out += seeds[0][p:p + 6]
            p += 6
            if k % 2:
                p += 1                                               # a deleted seed base
            else:
                out += [c for c in "ACGT" if c != seeds[0][p] and c != out[-1]][0]
            k += 1
        reads.append((out[:n], "*"))
    reads.append((L.revcomp(reads[0][0]), "*"))
    # two low-complexity reads found by search: an insertion of two bases ties with a mismatch at low quality followed by an
    # insertion of one, so the F cell of the second inserted row can extend or open at the same score
    for r, q in (("AAAAAAACCCAAAAACCACCAACACCACACCC", "I0&0&&D0D:&ID0D:II&&&D&:I&::0I&I"),
                 ("AAAAAAACCACAAAACCACCAACACCACACCC", ":&II:D:000&0D0:D00DI&0:0I0II:DD0")):
        reads.append((r, q))
        reads.append((L.revcomp(r), q[::-1]))

    def check(rows):
        for (r, _), e in list(zip(reads, rows))[:4]:
            need(100 < len(cigar_ops(e[5])) <= len(r) // 2 + 4 or len(r) < 512, "more than 100 CIGAR operations inside the stride")
            need(len(cigar_ops(e[5])) * 4 > len(r) // 2 and len(cigar_ops(e[5])) <= len(r) // 2 + 4, "a dense CIGAR inside the stride")
        ties = [e[2] == 1 and e[3] == 0 and "2I" in e[5] and f_tie_on_path(r, q, seeds[1], e[4], e[5]) for (r, q), e in list(zip(reads, rows))[4::2]]
        need(len(ties) == 2 and all(ties), "an insertion run through an F cell where extending and opening tie")
        need(all(e[3] == 1 and "2I" in e[5] for e in rows[5::2]), "the same on the reverse strand")
    return Stage4Case("most_operations", seeds, reads, check)


def s4_score_stride(seed=20):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 80) for _ in range(30)]
    reads = []
    for k in range(1100):
        s = seeds[rng.randrange(30)]
        reads.append((_place(rng, s, rng.randint(0, 40), 40, k % 2, lambda r: L.mutate(rng, r, 0.02)), "*"))

    def check(rows):
        need(len(reads) * 2 * len(seeds) > SCORE_BLOCKS * SCORE_WAVES and len({bucket(len(r)) for r, _ in reads}) == 1,
             "more tiles in one bucket than the score kernel has wavefronts")
        first_late = SCORE_BLOCKS * SCORE_WAVES // (2 * len(seeds))
        need(sum(e[2] >= 0 for e in rows) > 1000 and all(e[2] >= 0 for e in rows[first_late + 1:]), "reads of the second trip align")
    return Stage4Case("score_stride", seeds, reads, check)


def s4_trace_stride(seed=21):
    rng = random.Random(seed)
    seeds = [L.rand_seq(rng, 60) for _ in range(4)]
    reads = []
    for k in range(8400):
        s = seeds[rng.randrange(4)]
        a = rng.randint(0, 20)
        if k % 7 == 0:
            r = s[a:a + 20] + s[a + 21:a + 41]                       # a deletion: the CIGAR writer starts over per read
        else:
            r = L.mutate(rng, s[a:a + 40], 0.02)
        reads.append((L.revcomp(r) if k % 2 else r, "*"))

    def check(rows):
        n = sum(e[2] >= 0 for e in rows)
        need(n > TRACE_BLOCKS and len({bucket(len(r)) for r, _ in reads}) == 1, "more aligned reads in one bucket than the trace kernel has blocks")
        late = [e for e in rows[TRACE_BLOCKS + 8:] if e[2] >= 0]
        need(any("D" in e[5] for e in late) and any(e[5] == "40M" for e in late), "CIGARs of both shapes on the second trip")
    return Stage4Case("trace_stride", seeds, reads, check)


STAGE4_CASES = {f.__name__[3:]: f for f in (s4_every_bucket, s4_top_score, s4_short_seeds, s4_long_seeds, s4_window_bound, s4_gbar_rows,
                                            s4_ties, s4_alphabet_quality, s4_most_operations, s4_score_stride, s4_trace_stride)}


# ------------------------------------------------------------------------------------------------------------ profile

def _hits_of(rows, seg):
    return [h for h in rows if h[0] == seg]


def pr_every_bucket(seed=31):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 560) for _ in range(3)]
    segs = []
    for n in _bucket_lengths():
        for v in range(4):
            src = genes[rng.randrange(3)]
            a = rng.randint(0, len(src) - n - 2)
            r = src[a:a + n + 2]
            if n >= 60:
                p = n // 2
                r = r[:p] + rng.choice([c for c in "ACGT" if c != r[p]]) + r[p:] if v in (0, 3) else r[:p] + r[p + 1:]
            r = r[:n]
            segs.append(L.revcomp(r) if v in (1, 3) else r)

    def check(rows):
        for r in range(1, 9):
            mine = [h for h in rows if bucket(len(segs[h[0]])) == r]
            need({h[2] for h in mine} == {0, 1}, "a hit on either strand at R = %d" % r)
            need(any(h[5] > h[7] - h[6] + 1 for h in mine) and any(h[5] > abs(h[9] - h[8]) + 1 for h in mine), "gaps on either side at R = %d" % r)
        need(any(len(segs[h[0]]) < 9 for h in rows), "hits of the shortest segments")
    return ProfileCase("every_bucket", genes, segs, check, min_identity=0.0, max_evalue=10.0)


def pr_top_score(seed=32):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 600), L.rand_seq(rng, 512)]
    segs = [genes[0][40:552], L.revcomp(genes[0][88:600]), genes[1], L.revcomp(genes[1])]

    def check(rows):
        need(sum(h[3] == 2 * MAX_READ for h in rows) == 4 and {h[2] for h in rows} == {0, 1}, "S2 == 1024 on both strands")
    return ProfileCase("top_score", genes, segs, check)


def pr_short_genes(seed=33):
    rng = random.Random(seed)
    lens = [1, 2, 3, 5, 31, 63, 64, 65, 127, 128, 129]
    genes = [L.rand_seq(rng, n) for n in lens]
    segs, owner = [], []
    for k, g in enumerate(genes):
        for j, n in enumerate((100, 300, 512)):
            n = max(n, len(g) + 20)
            a = rng.randint(5, n - len(g) - 5)
            r = L.rand_seq(rng, a) + g + L.rand_seq(rng, n - a - len(g))
            segs.append(L.revcomp(r) if (k + j) % 2 else r)
            owner.append(k)

    def check(rows):
        for k in range(len(lens)):
            need(any(owner[h[0]] == k and h[1] == k and {h[8], h[9]} == {1, lens[k]} and h[4] == lens[k] for h in rows),
                 "a hit over the whole gene of %d bases" % lens[k])
    return ProfileCase("short_genes", genes, segs, check, min_identity=0.0, max_evalue=1e9)


def pr_long_genes(seed=34):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, n) for n in (8192, 8191, 4097)]
    segs = []
    for k, g in enumerate(genes):
        n = 512 if k == 0 else 100
        segs += [g[len(g) - n:], L.revcomp(g[len(g) - n:]), g[:n], L.revcomp(g[:n])]

    def check(rows):
        need(any(h[1] == 0 and h[2] == 0 and h[9] == MAX_SEED for h in rows), "hto == 8192 on the forward strand")
        need(any(h[1] == 0 and h[2] == 1 and h[8] == MAX_SEED for h in rows), "hfrom == 8192 on the reverse strand")
        need(any(h[1] == 1 and max(h[8], h[9]) == 8191 for h in rows) and any(min(h[8], h[9]) == 1 for h in rows), "column 8191 and column 1")
    return ProfileCase("long_genes", genes, segs, check)


def pr_window_bound(seed=35):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 900), L.rand_seq(rng, 300)]
    src = genes[0]
    segs, meta = [], []

    def add(p, a, n, gap, strand=0):
        r = _split_read(src, p, a, n, gap)
        assert len(r) == n
        segs.append(L.revcomp(r) if strand else r)
        meta.append((p, a, n, gap))
    for gap in (1, 20, 60, 100, 101, 102, 103, 104):                 # 1024 - 5 * 101 > 512 + 2: 101 joins, 103 cannot
        add(100, 256, 512, gap, gap % 2)
    for gap in (1, 20, 38, 39, 40, 41):                              # 400 - 5 * 39 > 200
        add(3, 100, 200, gap)
        add(400, 100, 200, gap, 1)
    for gap in (-1, -5, -20, -40):
        add(150, 256, 512, gap)
        add(2, 150, 300, gap)
    for a in range(20, 20 + TB_COLS):
        add(300, a, 200, 3)
        add(300, a, 200, -2)
        add(351, a, 200, 3)                                          # another context: equal neighbours move a gap to the left
    add(200, 100, 512, 50)
    add(200, 250, 512, 10)

    def check(rows):
        best = {}
        for h in rows:
            if h[1] == 0:
                best[h[0]] = h
        win = {s: profile_window(len(segs[s]), h) for s, h in best.items()}
        joined = {s for s, h in best.items() if h[5] == meta[s][2] + max(meta[s][3], 0) and h[7] - h[6] + 1 == meta[s][2]}
        need(any(meta[s][2:] == (512, 101) for s in joined) and not any(meta[s][2] == 512 and meta[s][3] > 102 for s in joined),
             "the largest deletions that join at L = 512 (102 ties with one half and a chance match)")
        need(any(win[s]["j0"] > 0 and win[s]["start"] == 0 and meta[s][3] > 0 for s in joined), "an alignment that starts on its window's first column")
        need(any(win[s]["j0"] == 0 and win[s]["start"] > 0 for s in joined), "a window clamped at column 0")
        need(any(win[s]["blocks"] >= 3 for s in joined), "a window of three or more blocks")
        # an alignment that fills its window: the deletion after a rows covers window columns a .. a + gap - 1
        cols = [(meta[s][1], meta[s][1] + meta[s][3] - 1) for s in joined if meta[s][3] > 0 and win[s]["start"] == 0 and win[s]["j0"] > 0
                and best[s][2] == 0]
        for edge in (TB_COLS, 2 * TB_COLS):
            need(any(a <= edge - 1 and b >= edge for a, b in cols), "a gap run over window columns %d | %d" % (edge - 1, edge))
        need({a % TB_COLS for a, b in cols} == set(range(TB_COLS)), "a deletion at every offset of a block")
        need(sum(meta[s][3] < 0 for s in joined) > TB_COLS, "the insertion counterparts join")
    return ProfileCase("window_bound", genes, segs, check, min_identity=0.0, max_evalue=10.0)


def pr_ties(seed=36):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 200) for _ in range(6)]
    half = L.rand_seq(rng, 30)
    pal = half + L.revcomp(half)
    genes[1] = genes[1][:70] + pal + genes[1][130:]
    unit = "ACGGTCATTG"
    genes[2] = L.rand_seq(rng, 40) + unit * 8 + L.rand_seq(rng, 40)
    genes[4] = "A" * 30
    genes.append(genes[3])
    segs = [pal, genes[3][20:120], L.revcomp(genes[3][20:120]), unit * 4, L.revcomp(unit * 4), "A" * 100, "T" * 100,
            genes[1][60:140], L.revcomp(genes[1][60:140])]

    def check(rows):
        h = _hits_of(rows, 0)
        need(len(h) == 1 and h[0][1] == 1 and h[0][2] == 0 and (h[0][8], h[0][9]) == (71, 130), "the palindrome on the forward strand")
        for s, strand in ((1, 0), (2, 1)):
            h = {x[1]: x for x in _hits_of(rows, s)}
            need(set(h) == {3, 6} and h[3][2:] == h[6][2:] and h[3][2] == strand, "the duplicated gene ties")
        h = _hits_of(rows, 3)
        need(len(h) == 1 and h[0][2] == 0 and (h[0][8], h[0][9]) == (41, 80), "the repeat at its smallest end column")
        h = _hits_of(rows, 4)
        need(len(h) == 1 and h[0][2] == 1 and (h[0][8], h[0][9]) == (80, 41), "... and on the reverse strand")
        h = _hits_of(rows, 5)
        need(len(h) == 1 and h[0][1] == 4 and (h[0][6], h[0][7]) == (1, 30), "the smallest end row")
        h = _hits_of(rows, 6)
        need(len(h) == 1 and h[0][2] == 1 and (h[0][6], h[0][7]) == (71, 100), "... and on the reverse strand")
        need({x[2] for x in _hits_of(rows, 7)} == {0} and {x[2] for x in _hits_of(rows, 8)} == {1}, "a palindrome inside a longer segment follows its flanks")
    return ProfileCase("ties", genes, segs, check)


def pr_score_stride(seed=37):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 50) for _ in range(30)]
    segs = []
    for k in range(1100):
        g = genes[rng.randrange(30)]
        r = L.mutate(rng, g[rng.randint(0, 10):][:40], 0.02)
        segs.append(L.revcomp(r) if k % 2 else r)

    def check(rows):
        need(len(segs) * 2 * len(genes) > SCORE_BLOCKS * SCORE_WAVES and len({bucket(len(s)) for s in segs}) == 1,
             "more tiles in one bucket than the score kernel has wavefronts")
        first_late = SCORE_BLOCKS * SCORE_WAVES // (2 * len(genes))
        need(len(rows) > 1000 and {h[0] for h in rows} >= set(range(first_late + 1, len(segs))), "segments of the second trip hit")
    return ProfileCase("score_stride", genes, segs, check)


def pr_trace_stride(seed=38):
    rng = random.Random(seed)
    g = L.rand_seq(rng, 60)
    genes = [g, g, L.rand_seq(rng, 60), g, g]
    segs = []
    for k in range(2100):
        a = rng.randint(0, 20)
        r = g[a:a + 20] + g[a + 21:a + 41] if k % 7 == 0 else L.mutate(rng, g[a:a + 40], 0.01)
        segs.append(L.revcomp(r) if k % 2 else r)

    def check(rows):
        need(len(rows) > TRACE_BLOCKS and len({bucket(len(s)) for s in segs}) == 1, "more hits in one bucket than the trace kernel has blocks")
        late = rows[TRACE_BLOCKS + 8:]
        need(any(h[5] == 41 for h in late) and any(h[5] == 40 and h[4] == 40 for h in late) and {h[2] for h in late} == {0, 1},
             "hits of both shapes and strands on the second trip")
    return ProfileCase("trace_stride", genes, segs, check, min_identity=90.0)


def pr_identity_edge(seed=39):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 400)]
    g = genes[0]

    def with_mismatches(a, n, at):
        r = list(g[a:a + n])
        for p in at:
            r[p] = [c for c in "ACGT" if c != r[p]][0]
        return "".join(r)
    segs = [with_mismatches(10, 100, (15, 32, 50, 68, 85)),          # 95 / 100
            with_mismatches(150, 100, (12, 28, 44, 60, 76, 90)),     # 94 / 100
            with_mismatches(300, 20, (9,)),                          # 19 / 20 when the whole segment aligns
            with_mismatches(200, 80, (20, 40, 60, 70)),              # 76 / 80 = 95 %
            with_mismatches(200, 79, (20, 40, 60, 70)),              # 75 / 79 < 95 %
            L.revcomp(with_mismatches(10, 100, (15, 32, 50, 68, 85)))]
    case = ProfileCase("identity_edge", genes, segs, None, min_identity=95.0, max_evalue=10.0)

    def check(rows, all_rows):
        """rows at -I 95, all_rows at -I 0: the hits on the edge stay, the ones a column below leave."""
        kept = {h[0]: h for h in rows}
        every = {h[0]: h for h in all_rows}
        need(set(every) == set(range(6)), "every segment hits at -I 0")
        for s in (0, 3, 5):
            need(s in kept and 100 * kept[s][4] == 95 * kept[s][5], "segment %d sits on 100 ident == 95 alen" % s)
        for s in (1, 4):
            need(s not in kept and 0 < 95 * every[s][5] - 100 * every[s][4] <= 100, "segment %d is at most one identical column below" % s)
        need(19 * every[2][5] == 20 * every[2][4] or every[2][4] == every[2][5], "the 20-base segment")
    case.check = check
    return case


def pr_impossible_segments(seed=40):
    rng = random.Random(seed)
    genes = [L.rand_seq(rng, 300), L.rand_seq(rng, 500)]
    short = [genes[0][k:k + n] for k, n in ((5, 1), (9, 8), (30, 16), (60, 24), (100, 20))]
    passing = [genes[0][20:120], L.revcomp(genes[1][100:300]), genes[1][7:70]]
    segs = [short[0], passing[0], short[1], short[2], passing[1], short[3], passing[2], short[4]]

    def check(rows):
        n_total = sum(len(g) for g in genes)
        for s in short:                                              # no score of the segment reaches E <= 1e-10
            need(0.46 * len(s) * n_total * math.exp(-1.28 * len(s)) > 1e-10, "a segment of %d bases cannot pass" % len(s))
        need({h[0] for h in rows} == {1, 4, 6}, "the passing segments hit between the impossible ones")
    case = ProfileCase("impossible_segments", genes, segs, check)
    case.alone = short
    return case


def pr_other_ka(seed=41):
    genes, segs = PL.parity_dataset(seed)
    genes, segs = genes[:5], segs[:120]

    def check(rows, default_rows):
        need(len(rows) > 20 and len(rows) != len(default_rows), "the other (lambda, K) keeps another set of hits")
    return ProfileCase("other_ka", genes, segs, check, min_identity=90.0, max_evalue=1e-10, ka_lambda=0.625, ka_k=0.41)


PROFILE_CASES = {f.__name__[3:]: f for f in (pr_every_bucket, pr_top_score, pr_short_genes, pr_long_genes, pr_window_bound, pr_ties,
                                             pr_score_stride, pr_trace_stride, pr_identity_edge, pr_impossible_segments, pr_other_ka)}


def run_profile_check(case, exe, rows=None):
    """The restatement's hits of a profile case, its property check run on them (with the second run some checks need)."""
    if rows is None:
        rows = PL.run_hits_check(exe, case.genes, case.segs, *case.thresholds())
    if case.name == "identity_edge":
        case.check(rows, PL.run_hits_check(exe, case.genes, case.segs, 0.0, case.max_evalue, case.ka_lambda, case.ka_k))
    elif case.name == "other_ka":
        case.check(rows, PL.run_hits_check(exe, case.genes, case.segs, case.min_identity, case.max_evalue))
    else:
        case.check(rows)
    return rows


def evalue_edge(exe):
    """A hit of the identity_edge data and its E-value as the restatement prints it (%.17g: the double itself): with -e equal
    to it the hit stays (E <= T), with the next double below it leaves."""
    case = pr_identity_edge()
    rows = PL.run_hits_check(exe, case.genes, case.segs, 0.0, 10.0)
    hit = [h for h in rows if h[0] == 2][0]
    e = float(hit[10])
    need(0.0 < e < 10.0 and repr(e) == repr(float("%.17g" % e)), "an E-value that survives the text")
    return case, hit, e
