"""Named edge cases of the graph-stage kernels, rambl_amd/csrc/sc_graph_kernels.hip: the threading of the reads along the
backbone (k_thread_walk, k_thread_scan, k_thread_sort, k_thread_sort_big), the insertion MSA (k_msa<false/true>) and the edge
supports (k_edge_support).  The constants below restate the geometry of those kernels and of their launchers (launch_thread,
launch_msa, launch_edge_support); sc_graph_kernels.hip is their source.

A case is a function of nothing but its name.  It returns the inputs and a property check: a function of the plain reference's
output that raises unless the input reaches the edge the case is named for -- a generator that silently loses its edge fails
on the CPU (tests/test_graph_edges_host.py) before the device comparison (tests/test_graph_edges_gpu.py) could pass for
nothing.  The plain references, thread_reference() and edge_support_reference(), are loops over Python ints that know nothing
of lanes, words, stretches or chunks; which kernel has to rank a class, and in how many words, rounds or stretches, is
arithmetic on the reference's pools (ranked_by)."""
import random
import re

import numpy as np

from align_edge_lib import need

SORT_WORDS = 512                  # k_thread_sort: words of a wavefront's bitmap, 32 ids each
BIG_WORDS = 16384                 # k_thread_sort_big: words of a stretch at the default (SC_SORT_BIG_WORDS shortens it, never below 64)
BIG_BLOCKS = 512                  # workgroups of k_thread_sort_big: more wide classes take another round
MSA_CM = 1024                     # k_msa<false>: columns kept in LDS; launch_msa: cmax = total bases + 1 > MSA_CM goes to HBM
MSA_CHUNK = 64                    # DP columns per chunk (one per lane); a later row of 64 bases or more also goes to HBM
GRID_BLOCKS, GRID_WAVES = 2048, 4  # k_thread_walk, k_thread_sort, k_edge_support: at most 2 048 blocks of 4 wavefronts
SCAN_THREADS = 1024               # k_thread_scan: one block, ceil(ncls / 1024) classes per thread
INT_MAX = 0x7fffffff
SC_ERR_UNSUPPORTED = -4
CHILD_BIG_WORDS = 64              # the stretch the wide-sort cases also run with, in a child process: 2 048 ids


# ---- reads and the plain reference of the threading tables

class Reads:
    """A window's reads as Context.submit takes them."""

    def __init__(self, gene_seq, reads):
        self.gene_seq = gene_seq
        self.pos = [r[0] for r in reads]
        self.cigar = [r[1] for r in reads]
        self.seq = [r[2] for r in reads]
        self.copies = [1] * len(reads)
        self.mates = [[] for _ in reads]

    def __len__(self):
        return len(self.pos)


def parse_cigar(cigar):
    return [("M" if op in "=X" else op, int(n)) for n, op in re.findall(r"(\d+)([MID=X])", cigar)]


def symbols(reads):
    """Code -> byte: A C G T, then the other bytes of the reads in byte order (thread_device)."""
    other = sorted(set(b for s in reads.seq for b in s.encode("ascii")) - set(b"ACGT"))
    return b"ACGT" + bytes(other)


def thread_reference(gene, reads):
    """The class tables of the per-base M loop (PartialOrderGraph.cpp:129-177) as the header of the threading kernels defines
    them.  Class (i, c) = window position i, symbol code c, index i * 8 + c.
      count, first   reads with a base in the class, the smallest of them (INT_MAX: none)
      off, pool      the reads of every class back to back, ascending inside a class
      smin           the smallest read whose first operation is M and whose first base is in the class
      emin           the smallest read whose last operation is M and whose last base is in the class
      tmin[i * 64 + cp * 8 + c]   the smallest read with symbols cp, c on positions i - 1, i inside one M run or across two
                     adjacent M operations
    A read that runs past the window or its own bases, or a ninth symbol, raises ValueError."""
    glen = len(gene)
    sym = symbols(reads)
    if len(sym) > 8:
        raise ValueError("more than 8 distinct symbols in the reads")
    code = {b: k for k, b in enumerate(sym)}
    members = [[] for _ in range(glen * 8)]
    smin, emin, tmin = [INT_MAX] * (glen * 8), [INT_MAX] * (glen * 8), [INT_MAX] * (glen * 64)
    for rid in range(len(reads)):
        seq = reads.seq[rid].encode("ascii")
        ops = parse_cigar(reads.cigar[rid])
        i, j, prev = reads.pos[rid], 0, None
        for k, (op, ln) in enumerate(ops):
            if op == "M":
                if i + ln > glen or j + ln > len(seq):
                    raise ValueError("read %d runs outside the window or past its own bases" % rid)
                for t in range(ln):
                    c = code[seq[j + t]]
                    cls = (i + t) * 8 + c
                    members[cls].append(rid)
                    if t > 0 or prev == "M":
                        e = (i + t) * 64 + code[seq[j + t - 1]] * 8 + c
                        tmin[e] = min(tmin[e], rid)
                    elif k == 0:
                        smin[cls] = min(smin[cls], rid)
                    if k == len(ops) - 1 and t == ln - 1:
                        emin[cls] = min(emin[cls], rid)
                i += ln
                j += ln
            elif op == "I":
                j += ln
            else:
                i += ln
            prev = op
    count = [len(m) for m in members]
    off = [0]
    for n in count:
        off.append(off[-1] + n)
    for m in members:
        assert m == sorted(set(m))                            # a read has one base per window position
    return dict(sym=sym + bytes(8 - len(sym)), count=count, first=[m[0] if m else INT_MAX for m in members], off=off,
                pool=[r for m in members for r in m], smin=smin, emin=emin, tmin=tmin)


def members_of(ref, i, ch):
    cls = i * 8 + ref["sym"].index(ch.encode("ascii"))
    return ref["pool"][ref["off"][cls]:ref["off"][cls + 1]]


def ranked_by(ref, n_reads, big_words=BIG_WORDS):
    """Which kernel has to put each class of more than one read into read order: {class: ("bitmap", words, rounds of the
    64-word prefix loop) | ("big", stretches)}.  launch_thread starts k_thread_sort_big only for more than 16 384 reads; no
    class of fewer reads can be wide."""
    out = {}
    for cls in range(len(ref["count"])):
        ids = ref["pool"][ref["off"][cls]:ref["off"][cls + 1]]
        if len(ids) < 2:
            continue
        span = ids[-1] - ids[0]
        if span < SORT_WORDS * 32:
            words = (span >> 5) + 1
            out[cls] = ("bitmap", words, (words + 63) // 64)
        else:
            need(n_reads > SORT_WORDS * 32, "a wide class needs more than 16 384 reads")
            out[cls] = ("big", span // (big_words * 32) + 1)
    return out


# ---- threading cases

class ThreadCase:
    def __init__(self, name, reads, check, parity=False, error=None, wide=False):
        """check(ref, big_words); parity: ACGT reads, few enough for the -G dump of the oracle; error: the code the region has
        to fail with (no tables then); wide: a wide-sort case, run with short stretches too."""
        self.name, self.reads, self.check, self.parity, self.error, self.wide = name, reads, check, parity, error, wide

    def key(self):
        r = self.reads
        return (r.gene_seq, tuple(r.pos), tuple(r.cigar), tuple(r.seq))

    def reference(self):
        return thread_reference(self.reads.gene_seq, self.reads)


def _gene(name, n):
    rng = random.Random("graph_edge_lib:" + name)
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(ch, k=1):
    return "ACGT"[("ACGT".index(ch) + k) % 4]


def _digits(k, n):
    """k in n base-4 digits, as bases: a read's serial number, so that no two reads of a case are equal"""
    return "".join("ACGT"[(k >> (2 * (n - 1 - d))) & 3] for d in range(n))


def _copy(gene, pos, n):
    return (pos, "%dM" % n, gene[pos:pos + n])


def _ordered(reads):
    need(all(a[0] <= b[0] for a, b in zip(reads, reads[1:])), "reads in start order")
    need(len(set(reads)) == len(reads), "distinct reads")
    return reads


def _cover(gene):
    """a few reads that copy the gene, the last one up to its last cell, with one mismatch each"""
    glen = len(gene)
    reads = []
    for k, pos in enumerate(sorted(set([0, glen // 7, glen // 3, glen // 2, max(0, glen - 60), max(0, glen - 33)]))):
        seq = list(gene[pos:min(glen, pos + 70 + k)])
        seq[len(seq) // 2] = _other(seq[len(seq) // 2], 1 + k % 3)
        reads.append((pos, "%dM" % len(seq), "".join(seq)))
    return reads


def one_read():
    gene = _gene("one_read", 40)
    seq = gene[5:8] + _other(gene[8]) + gene[9:25]
    reads = Reads(gene, [(5, "20M", seq)])

    def check(ref, big_words=BIG_WORDS):
        need(sum(ref["count"]) == 20 and max(ref["count"]) == 1, "twenty classes of one read")
        need(not ranked_by(ref, 1, big_words), "no class needs ranking")
        need(sum(v == 0 for v in ref["smin"]) == 1 and sum(v == 0 for v in ref["emin"]) == 1, "one start, one end")
        need(sum(v == 0 for v in ref["tmin"]) == 19, "nineteen transitions")
    return ThreadCase("one_read", reads, check, parity=True)


RUN_LENGTHS = (63, 64, 65, 128, 129)


def run_seams():
    """M runs of 63, 64, 65, 128 and 129 bases: k_thread_walk takes 64 bases of a run per round (`t += 64`).  Every read has a
    mismatch on the bases 62..65 and 126..129 of its run that it has, so that the transitions over a seam are its own."""
    gene = _gene("run_seams", 200)
    reads = []
    for k, ln in enumerate(RUN_LENGTHS):
        pos = 3 * k
        seq = list(gene[pos:pos + ln])
        for t in (62, 63, 64, 65, 126, 127, 128):
            if t < ln:
                seq[t] = _other(seq[t], 1 + k % 3)
        reads.append((pos, "%dM" % ln, "".join(seq)))
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        need(tuple(parse_cigar(c)[0][1] for c in reads.cigar) == RUN_LENGTHS, "runs of 63, 64, 65, 128, 129")
        for rid, ln in enumerate(RUN_LENGTHS):
            for t in (63, 64, 127, 128):                         # last base of a round, first base of the next
                if t < ln:
                    i, s = reads.pos[rid] + t, reads.seq[rid]
                    e = i * 64 + ref["sym"].index(s[t - 1].encode()) * 8 + ref["sym"].index(s[t].encode())
                    need(ref["tmin"][e] <= rid, "transition over base %d of read %d" % (t, rid))
                    need(rid in members_of(ref, i, s[t]), "base %d of read %d" % (t, rid))
    return ThreadCase("run_seams", reads, check, parity=True)


def last_cell():
    gene = _gene("last_cell", 90)
    glen = len(gene)
    reads = [_copy(gene, 0, 50), (30, "60M", gene[30:89] + _other(gene[89])), _copy(gene, 60, 30), (89, "1M", _other(gene[89], 2))]
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        ends = [r for r in range(len(reads)) if reads.pos[r] + parse_cigar(reads.cigar[r])[0][1] == glen]
        need(ends == [1, 2, 3], "three reads end on the window's last cell")
        need(sorted(v for v in ref["emin"][(glen - 1) * 8:] if v != INT_MAX) == [1, 2, 3], "each in a class of its own")
        need(ref["smin"][(glen - 1) * 8 + ref["sym"].index(_other(gene[89], 2).encode())] == 3, "a read of one base starts there too")
    return ThreadCase("last_cell", reads, check, parity=True)


def adjacent_m():
    """A transition across two adjacent M operations (`t > 0 || prev_m`): the second operation's first base has a left
    neighbour and is no read start.  Reads 1 and 2 carry symbols on both sides of the seam that no other read has there."""
    gene = _gene("adjacent_m", 60)
    reads = [_copy(gene, 0, 40)]
    s = list(gene[10:30])
    s[7], s[8] = _other(s[7]), _other(s[8], 2)
    reads.append((10, "8M12M", "".join(s)))                      # seam between window positions 17 and 18
    s = list(gene[20:42])
    s[4], s[5], s[10] = _other(s[4], 2), _other(s[5]), _other(s[10], 3)
    reads.append((20, "5=1X5=11M", "".join(s)))                  # seams at 25, 26, 31: = and X are M
    reads.append(_copy(gene, 25, 30))
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        for rid, i in ((1, 18), (2, 25), (2, 26), (2, 31)):
            sq, p = reads.seq[rid], i - reads.pos[rid]
            bounds, at = set(), 0
            for _, ln in parse_cigar(reads.cigar[rid]):
                bounds.add(at)
                at += ln
            need(p in bounds and p > 0, "position %d opens an M operation of read %d" % (i, rid))
            cls = i * 8 + ref["sym"].index(sq[p].encode())
            e = i * 64 + ref["sym"].index(sq[p - 1].encode()) * 8 + ref["sym"].index(sq[p].encode())
            need(ref["tmin"][e] == rid, "the transition into position %d is read %d's" % (i, rid))
            need(ref["smin"][cls] == INT_MAX, "and no start")
            if i in (18, 25):
                need(members_of(ref, i, sq[p]) == [rid] and members_of(ref, i - 1, sq[p - 1]) == [rid], "no other read has these symbols")
    return ThreadCase("adjacent_m", reads, check, parity=True)


def indel_resets():
    """After an I or a D the next M base has no transition and is no start.  Each read lies in a zone of the gene that no
    other read touches, with mismatches around its indel, so that an entry it must not write stays absent.  sc_roi_submit
    accepts a read whose first or last operation is I; both are here (reads 2 and 3)."""
    gene = _gene("indel_resets", 120)

    def mis(pos, n):
        return "".join(_other(ch) for ch in gene[pos:pos + n])
    reads = [
        (0, "4M2I4M", mis(0, 4) + "GG" + mis(4, 4)),            # I in the middle: position 4 follows the insertion
        (20, "4M3D4M", mis(20, 4) + mis(27, 4)),                # D in the middle: position 27 follows the deletion
        (40, "2I6M", "TT" + mis(40, 6)),                        # first operation I: position 40 is no start
        (60, "6M2I", mis(60, 6) + "CC"),                        # last operation I: position 65 is no end
        (80, "3M1I2M1D3M", mis(80, 3) + "A" + mis(83, 2) + mis(86, 3)),
    ]
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        need(max(ref["count"]) == 1, "every class has one read")
        for i in (4, 27, 40, 83, 86):                            # first base after an I or D (or a leading I)
            need(sum(ref["count"][i * 8:i * 8 + 8]) == 1, "a base on position %d" % i)
            need(all(v == INT_MAX for v in ref["tmin"][i * 64:i * 64 + 64]), "no transition into position %d" % i)
            need(all(v == INT_MAX for v in ref["smin"][i * 8:i * 8 + 8]), "no start on position %d" % i)
        need([v for v in ref["smin"] if v != INT_MAX] == [0, 1, 3, 4], "reads 0, 1, 3, 4 start with M, read 2 does not")
        need([v for v in ref["emin"] if v != INT_MAX] == [0, 1, 2, 4], "reads 0, 1, 2, 4 end with M, read 3 does not")
        need(all(v == INT_MAX for v in ref["emin"][65 * 8:66 * 8]) and sum(ref["count"][65 * 8:66 * 8]) == 1, "position 65 is no end")
    return ThreadCase("indel_resets", reads, check, parity=True)


def _filler(k, n_reads, zone, nd):
    return (k * zone // n_reads, "%dM" % nd, _digits(k, nd))


def _marked(name, n_reads, classes, glen=300):
    """n_reads reads in start order; class j = (marker position p_j, 'T') holds exactly the reads classes[j].  The gene has 'A'
    on its last len(classes) positions, the markers.  Every read begins with its serial number in base-4 digits; the members
    of class j go on with a copy of the gene up to p_j and end there in 'T'; the others, fillers, end in front of the markers."""
    nd = 7 if n_reads <= 16384 else 8
    nm = len(classes)
    gene = _gene(name, glen - nm) + "A" * nm
    zone = glen - nm - nd
    owner = {}
    for j, ids in enumerate(classes):
        for rid in ids:
            need(rid not in owner and 0 <= rid < n_reads, "a read is in one marked class")
            owner[rid] = j
    reads = []
    for k in range(n_reads):
        pos, cigar, seq = _filler(k, n_reads, zone, nd)
        if k in owner:
            p = glen - nm + owner[k]
            seq = seq + gene[pos + nd:p] + "T"
            cigar = "%dM" % len(seq)
        reads.append((pos, cigar, seq))
    return Reads(gene, _ordered(reads)), [glen - nm + j for j in range(nm)]


def _marked_case(name, n_reads, classes, expect, glen=300, wide=False, extra=None):
    """expect(j, big_words) -> what ranked_by has to say of marked class j"""
    reads, marks = _marked(name, n_reads, classes, glen)

    def check(ref, big_words=BIG_WORDS):
        rk = ranked_by(ref, len(reads), big_words)
        for j, ids in enumerate(classes):
            need(members_of(ref, marks[j], "T") == sorted(ids), "marked class %d holds its reads" % j)
            need(rk[marks[j] * 8 + 3] == expect(j, big_words), "marked class %d: %r, not %r" % (j, rk[marks[j] * 8 + 3], expect(j, big_words)))
        if extra:
            extra(ref, rk, big_words)
    return ThreadCase(name, reads, check, wide=wide)


def walk_second_round():
    """8 200 short reads: launch_thread caps the grid at 2 048 blocks of 4 wavefronts, so the reads from 8 192 on are a
    wavefront's second (`r += nwaves`)."""
    n = 8200
    reads, _ = _marked("walk_second_round", n, [], glen=100)

    def check(ref, big_words=BIG_WORDS):
        need(n > GRID_BLOCKS * GRID_WAVES and (n + 3) // 4 > GRID_BLOCKS, "more reads than wavefronts")
        need(sum(1 for v in ref["pool"] if v >= GRID_BLOCKS * GRID_WAVES) == 7 * (n - GRID_BLOCKS * GRID_WAVES), "bases of second-round reads")
        need(sum(ref["count"]) == 7 * n, "seven bases each")
    return ThreadCase("walk_second_round", reads, check)


def _scan_case(glen):
    """ncls = glen * 8 classes over the 1 024 threads of k_thread_scan, ceil(ncls / 1024) each."""
    name = "scan_%d" % glen
    gene = _gene(name, glen)
    reads = Reads(gene, _ordered(_cover(gene)))

    def check(ref, big_words=BIG_WORDS):
        ncls = glen * 8
        per = (ncls + SCAN_THREADS - 1) // SCAN_THREADS
        need(len(ref["count"]) == ncls, "glen * 8 classes")
        if glen == 127:
            need(per == 1 and ncls < SCAN_THREADS, "fewer classes than threads")
        elif glen == 128:
            need(per == 1 and ncls == SCAN_THREADS, "a class per thread")
        else:
            need(per >= 2 and (SCAN_THREADS - 1) * per > ncls, "the trailing threads start past the last class")
        need(any(ref["count"][(glen - 1) * 8:]) and ref["off"][-1] == sum(ref["count"]) > 300, "reads up to the last class")
    return ThreadCase(name, reads, check, parity=True)


def eight_symbols():
    """Symbol codes 4 to 7: reads that carry eight distinct bytes.  Codes follow the byte order: K N R a."""
    gene = _gene("eight_symbols", 80)
    reads = [(0, "12M", "ACGTNRKaACGT"), (3, "10M", "aKRNTGCAaa"), (10, "4M2I6M", "NNaaRRKKACGT"), _copy(gene, 12, 40), (40, "8M", "KaNRKaNR"),
             (72, "8M", "ACGTaNRK")]
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        need(ref["sym"] == b"ACGTKNRa", "eight symbols, the last four in byte order")
        per_code = [sum(ref["count"][c::8]) for c in range(8)]
        need(min(per_code) >= 4, "bases of every code")
        need(any(v != INT_MAX for i in range(len(gene)) for v in ref["tmin"][i * 64 + 7 * 8 + 4:i * 64 + 7 * 8 + 8]), "transitions among codes 4..7")
        need(ref["emin"][79 * 8 + 4] == 5, "a read ends on the last cell in code 4")
    return ThreadCase("eight_symbols", reads, check)


def nine_symbols():
    base = eight_symbols().reads
    reads = Reads(base.gene_seq, list(zip(base.pos, base.cigar, base.seq))[:-1] + [(72, "8M", "ACGTaNRY")])

    def check(ref, big_words=BIG_WORDS):
        need(ref is None and len(symbols(reads)) == 9, "nine symbols: no tables")
    return ThreadCase("nine_symbols", reads, check, error=SC_ERR_UNSUPPORTED)


def word_seams():
    """Classes whose reads span 31, 32 and 33 ids: the last id in the first word of the bitmap, the first of the second."""
    classes = [[100, 105, 131], [200, 217, 231, 232], [300, 301, 332, 333], [400, 431, 432, 463, 464, 465]]
    spans = [31, 32, 33, 65]
    return _marked_case("word_seams", 600, classes, lambda j, bw: ("bitmap", (spans[j] >> 5) + 1, 1))


def prefix_second_round():
    """Spans 2 047, 2 048 and 2 049: 64 words are one round of the prefix loop of k_thread_sort, 65 need the carry `run +=`."""
    classes = [[10, 11, 1000, 2057], [20, 21, 2000, 2067, 2068], [30, 1030, 2078, 2079], [40, 41, 42, 2090 + 2047, 2090 + 4090]]
    spans = [2047, 2048, 2049, 6140]
    return _marked_case("prefix_second_round", 6200, classes, lambda j, bw: ("bitmap", (spans[j] >> 5) + 1, ((spans[j] >> 5) + 64) // 64))


def bitmap_last():
    """Span 16 383 with 16 384 reads: the widest class a wavefront's bitmap holds (512 words, eight rounds); launch_thread does
    not start k_thread_sort_big."""
    n = SORT_WORDS * 32
    classes = [[0, 1, 8191, 8192, n - 1], [20, 16000, 20 + 16351]]

    def extra(ref, rk, big_words):
        need(all(v[0] == "bitmap" for v in rk.values()), "no wide class")
    return _marked_case("bitmap_last", n, classes, lambda j, bw: ("bitmap", 512 - j, 8), extra=extra)


def bitmap_first_wide():
    """Span 16 384 with 16 385 reads: the first class that goes to k_thread_sort_big, next to one of span 16 382 that stays."""
    n = SORT_WORDS * 32 + 1
    classes = [[0, 5, 8192, n - 1], [1, 6, 9000, n - 2]]
    return _marked_case("bitmap_first_wide", n, classes,
                        lambda j, bw: ("big", (n - 1) // (bw * 32) + 1) if j == 0 else ("bitmap", 512, 8))


def bitmap_full():
    """Every id of a 16 384-id span in one class: every bit of the 512 words set."""
    n, p = SORT_WORDS * 32, 30
    gene = _gene("bitmap_full", 60)
    reads = []
    for k in range(n):
        pos = p - 7 + k * 8 // n
        d = _digits(k, 7)
        reads.append((pos, "8M", d[:p - pos] + "T" + d[p - pos:]))
    gene = gene[:p] + "A" + gene[p + 1:]
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        need(members_of(ref, p, "T") == list(range(n)), "all 16 384 reads in one class")
        rk = ranked_by(ref, n, big_words)
        need(rk[p * 8 + 3] == ("bitmap", 512, 8) and all(v[0] == "bitmap" for v in rk.values()), "the bitmap kernel, eight rounds")
    return ThreadCase("bitmap_full", reads, check)


def _wide_ids(lo, stretches, extra):
    """ids of a class from lo over `stretches` stretches of CHILD_BIG_WORDS * 32 ids: both ends of every stretch, and `extra`"""
    s = CHILD_BIG_WORDS * 32
    ids = set(extra)
    for k in range(stretches):
        ids |= {lo + k * s, lo + k * s + s - 1}
    return sorted(ids)


def stretch_exact():
    """A class whose largest id is the last id of its ninth stretch of 2 048."""
    s = CHILD_BIG_WORDS * 32
    ids = _wide_ids(5, 9, [6, 5 + s // 2, 5 + 3 * s + 31, 5 + 3 * s + 32])
    n = ids[-1] + 10

    def extra(ref, rk, big_words):
        need((ids[-1] - ids[0]) % s == s - 1 and ids[-1] - ids[0] >= SORT_WORDS * 32, "the largest id is a stretch's last")
    return _marked_case("stretch_exact", n, [ids], lambda j, bw: ("big", 9 if bw == CHILD_BIG_WORDS else 1), wide=True, extra=extra)


def stretch_plus_one():
    """One id more: the tenth stretch holds the class's largest id and nothing else."""
    s = CHILD_BIG_WORDS * 32
    ids = _wide_ids(5, 9, [7, 5 + 9 * s])
    n = ids[-1] + 10

    def extra(ref, rk, big_words):
        need((ids[-1] - ids[0]) % s == 0 and ids[-2] == ids[-1] - 1, "the largest id is a stretch's first")
    return _marked_case("stretch_plus_one", n, [ids], lambda j, bw: ("big", 10 if bw == CHILD_BIG_WORDS else 1), wide=True, extra=extra)


def empty_middle():
    """Ids in the first and the last of ten stretches only: the count of the reads ranked so far (s_base) has to pass eight
    stretches that hold nothing."""
    s = CHILD_BIG_WORDS * 32
    lo = 3
    ids = [lo, lo + 1, lo + 40, lo + s - 1] + [lo + 9 * s, lo + 9 * s + 33, lo + 9 * s + 700]
    n = ids[-1] + 10

    def extra(ref, rk, big_words):
        used = sorted(set((v - lo) // s for v in ids))
        need(used == [0, 9], "stretches 1 to 8 are empty")
    return _marked_case("empty_middle", n, [ids], lambda j, bw: ("big", 10 if bw == CHILD_BIG_WORDS else 1), wide=True, extra=extra)


def many_wide():
    """More wide classes than k_thread_sort_big has workgroups (`bi += gridDim.x`): reads 0 and 16 384 copy a gene of 600
    bases, the 16 383 between them are fillers on its first 40 bases."""
    n, glen, nd = SORT_WORDS * 32 + 1, 600, 7
    gene = _gene("many_wide", glen)
    reads = [_copy(gene, 0, glen)] + [_filler(k, n, 34, nd) for k in range(1, n - 1)] + [_copy(gene, 40, glen - 40)]
    reads = Reads(gene, _ordered(reads))

    def check(ref, big_words=BIG_WORDS):
        rk = ranked_by(ref, n, big_words)
        big = [c for c, v in rk.items() if v[0] == "big"]
        need(len(big) > BIG_BLOCKS, "more than 512 wide classes")
        need(all(rk[c] == ("big", 9 if big_words == CHILD_BIG_WORDS else 1) for c in big), "of nine stretches each")
    return ThreadCase("many_wide", reads, check, wide=True)


THREAD_CASES = {f.__name__: f for f in (one_read, run_seams, last_cell, adjacent_m, indel_resets, walk_second_round, eight_symbols, nine_symbols,
                                        word_seams, prefix_second_round, bitmap_last, bitmap_first_wide, bitmap_full,
                                        stretch_exact, stretch_plus_one, empty_middle, many_wide)}
for _g in (127, 128, 129, 5000):
    THREAD_CASES["scan_%d" % _g] = (lambda g: lambda: _scan_case(g))(_g)
WIDE_CASES = ("stretch_exact", "stretch_plus_one", "empty_middle", "many_wide")
PARITY_CASES = ("one_read", "run_seams", "last_cell", "adjacent_m", "indel_resets", "scan_127", "scan_128", "scan_129", "scan_5000")


def sam_dataset(case, outdir):
    """The case as FASTA + SAM (synth.write_dataset) and the command line that keeps every read."""
    from rambl_amd import synth
    r = case.reads
    name = case.name
    lines = ["\t".join(["r%05d" % k, "0", name, str(r.pos[k] + 1), "42", r.cigar[k], "*", "0", "0", r.seq[k], "I" * len(r.seq[k])])
             for k in range(len(r))]
    fa, sam = synth.write_dataset(outdir, [dict(name=name, ref=r.gene_seq, sam_lines=lines)])
    return ["-r", "%s:1-%d" % (name, len(r.gene_seq)), "-q", "0", "-D", "1000000", "-I", "13", "-l", "0", "-t", "0.02", "-d", "0.02",
            "-w", "100000", fa, sam]


# ---- MSA cases

class MsaCase:
    def __init__(self, name, seqs, check):
        self.name, self.seqs, self.check = name, seqs, check

    def key(self):
        return tuple(self.seqs)


def msa_kernel(seqs):
    """What launch_msa decides: "lds" or "hbm", and the chunks of 64 DP columns the longest later row takes."""
    cmax = sum(len(s) for s in seqs) + 1
    longest = max([len(s) for s in seqs[1:]] or [0])
    stride = (longest + 1 + 63) // 64 * 64
    return ("hbm" if cmax > MSA_CM or stride > 64 else "lds"), stride // 64


def _rows_hold(seqs, rows):
    need(len(rows) == len(seqs) and len(set(len(r) for r in rows)) == 1, "rows of one length")
    need(all(r.replace("-", "") == s.replace("-", "") for r, s in zip(rows, seqs)), "a row is its sequence with gaps")


def _noisy_rows(name, lens):
    rng = random.Random("graph_edge_lib:" + name)
    base = "".join(rng.choice("ACGT") for _ in range(max(lens) + 10))
    rows = []
    for k, n in enumerate(lens):
        if k % 5 == 4:
            rows.append("".join(rng.choice("ACGT") for _ in range(n)))           # an unrelated row: it opens columns
            continue
        out = []
        for ch in base:
            r = rng.random()
            if r < 0.05:
                continue
            out.append(rng.choice("ACGT") if r < 0.12 else ch)
            if rng.random() < 0.04:
                out.append(rng.choice("ACGT"))
        out = (out + list(base))[:n]
        rows.append("".join(out))
    return rows


_SEAM_LENS = [60] * 17 + [3]                                  # 1 023 bases


def lds_last():
    """1 023 bases in all: cmax = 1 024, the last input k_msa<false> (LDS) takes."""
    seqs = _noisy_rows("msa_seam", _SEAM_LENS)

    def check(rows):
        need(sum(len(s) for s in seqs) == MSA_CM - 1 and msa_kernel(seqs) == ("lds", 1), "1 023 bases, LDS")
        _rows_hold(seqs, rows)
    return MsaCase("lds_last", seqs, check)


def hbm_first():
    """The rows of lds_last with one base more on the last: cmax = 1 025, the first input that goes to k_msa<true> (HBM)."""
    seqs = _noisy_rows("msa_seam", _SEAM_LENS)
    seqs[-1] += "G"

    def check(rows):
        base = lds_last().seqs
        need(seqs[:-1] == base[:-1] and seqs[-1][:-1] == base[-1], "lds_last and one base")
        need(sum(len(s) for s in seqs) == MSA_CM and msa_kernel(seqs) == ("hbm", 1), "1 024 bases, HBM")
        _rows_hold(seqs, rows)
    return MsaCase("hbm_first", seqs, check)


def long_first_lds():
    """A first sequence of 500 bases with later ones of 40 and 3: only the later rows need DP columns, this stays in LDS."""
    seqs = _noisy_rows("long_first_lds", [500, 40, 3])

    def check(rows):
        need([len(s) for s in seqs] == [500, 40, 3] and msa_kernel(seqs) == ("lds", 1), "500, 40, 3 in LDS")
        _rows_hold(seqs, rows)
    return MsaCase("long_first_lds", seqs, check)


def all_equal():
    """Twelve equal rows: where candidates tie, the order of the comparisons (diagonal, insert, delete) decides."""
    seqs = ["ACGTTGCAAC"] * 12

    def check(rows):
        need(len(set(seqs)) == 1 and len(seqs) == 12, "equal rows")
        _rows_hold(seqs, rows)
        need(rows == seqs, "equal rows align without a gap")
    return MsaCase("all_equal", seqs, check)


def one_base_rows():
    seqs = ["A", "C", "A", "G", "T", "A", "a", "C"]

    def check(rows):
        need(all(len(s) == 1 for s in seqs) and len(set(seqs)) == 5, "rows of one base")
        _rows_hold(seqs, rows)
    return MsaCase("one_base_rows", seqs, check)


def two_rows():
    """n == 2 with a second row of 129 bases: three chunks of 64 DP columns, so k_msa<true> and its column hand-over between
    chunks (`more`)."""
    seqs = _noisy_rows("two_rows", [130, 129])

    def check(rows):
        need(len(seqs) == 2 and msa_kernel(seqs) == ("hbm", 3), "two rows, three chunks")
        _rows_hold(seqs, rows)
    return MsaCase("two_rows", seqs, check)


def plus_and_case():
    """The '+' class of dna_score_cls, lower case (equal to its upper case) and a byte outside the table (scores 0)."""
    seqs = ["AC+GtaN+CA", "ac+GTAn+c", "A+CGT+", "+GT+", "a+", "+"]

    def check(rows):
        need(all("+" in s for s in seqs) and any(c.islower() for s in seqs for c in s) and seqs[-1] == "+", "plus, lower case, N")
        need([len(s) for s in seqs] == sorted((len(s) for s in seqs), reverse=True), "longest first")
        _rows_hold(seqs, rows)
    return MsaCase("plus_and_case", seqs, check)


MSA_CASES = {f.__name__: f for f in (lds_last, hbm_first, long_first_lds, all_equal, one_base_rows, two_rows, plus_and_case)}


# ---- edge support

def edge_support_reference(pool_ptr, pool_rid, pool_cn, node_is_end, edge_src, edge_dst):
    """number_of_reads_cover_nodes (PartialOrderGraph.cpp:1218-1244) for every edge, in its quadratic form; node 0 is the
    source, node_is_end marks the node labelled "$"."""
    pool_ptr, pool_rid, pool_cn, node_is_end = ([int(x) for x in a] for a in (pool_ptr, pool_rid, pool_cn, node_is_end))
    out = []
    for u, v in zip((int(x) for x in edge_src), (int(x) for x in edge_dst)):
        n = 0
        if u == 0:
            for j in range(pool_ptr[v], pool_ptr[v + 1]):
                n += pool_cn[j]
        elif node_is_end[v]:
            for i in range(pool_ptr[u], pool_ptr[u + 1]):
                n += pool_cn[i]
        else:
            for i in range(pool_ptr[u], pool_ptr[u + 1]):
                for j in range(pool_ptr[v], pool_ptr[v + 1]):
                    if pool_rid[i] == pool_rid[j]:
                        n += pool_cn[j]
        out.append(n)
    return out


class EdgeCase:
    def __init__(self, name, pools, ends, edges, flags, check):
        """pools: per node a list of (rid, cn); ends: the nodes labelled "$"; edges: (u, v); flags: the values of `sorted`
        the case runs under."""
        self.name, self.flags, self.check = name, tuple(flags), check
        self.pool_ptr = np.cumsum([0] + [len(p) for p in pools]).astype(np.int32)
        self.pool_rid = np.array([r for p in pools for r, _ in p], dtype=np.int32)
        self.pool_cn = np.array([c for p in pools for _, c in p], dtype=np.int32)
        self.node_is_end = np.zeros(len(pools), dtype=np.uint8)
        self.node_is_end[list(ends)] = 1
        self.edge_src = np.array([u for u, _ in edges], dtype=np.int32)
        self.edge_dst = np.array([v for _, v in edges], dtype=np.int32)

    def arrays(self):
        return (self.pool_ptr, self.pool_rid, self.pool_cn, self.node_is_end, self.edge_src, self.edge_dst)

    def key(self):
        return tuple(a.tobytes() for a in self.arrays()) + (self.flags,)

    def reference(self):
        return edge_support_reference(*self.arrays())

    def pool(self, a):
        return self.pool_rid[self.pool_ptr[a]:self.pool_ptr[a + 1]].tolist()

    def pools_sorted(self):
        return all(self.pool(a) == sorted(self.pool(a)) for a in range(len(self.node_is_end)))


def source_and_end():
    """Edges out of the source count the target's pool, edges into "$" the origin's; source -> "$" is a source edge."""
    pools = [[], [(0, 2), (1, 1), (4, 3)], [(1, 5), (2, 1)], [(7, 9)], []]
    edges = [(0, 1), (0, 2), (1, 2), (1, 4), (2, 4), (0, 4), (3, 4), (0, 3), (1, 3), (4, 1)]
    c = None

    def check(sup):
        need(sup == [6, 6, 5, 6, 6, 0, 9, 9, 0, 0], "hand-computed supports")
        need(c.node_is_end.tolist() == [0, 0, 0, 0, 1], "node 4 is the end")
    c = EdgeCase("source_and_end", pools, [4], edges, [1], check)
    return c


def multiplicity():
    """The origin's pool holds read 5 twice and read 7 three times: the support counts the target's copy number once per
    entry of the origin (`lo2 - lo` in the sorted branch)."""
    pools = [[], [(3, 1), (5, 1), (5, 1), (7, 2), (7, 2), (7, 2), (9, 1)], [(5, 4), (7, 10), (8, 100)], [(7, 1), (7, 1)], []]
    edges = [(1, 2), (2, 1), (1, 3), (3, 1), (3, 2)]

    def check(sup):
        need(sup == [2 * 4 + 3 * 10, 2 * 1 + 3 * 2, 3 + 3, 2 * 3 * 2, 2 * 10], "hand-computed supports")
    return EdgeCase("multiplicity", pools, [4], edges, [1, 0], check)


def _long_pools():
    rng = random.Random("graph_edge_lib:long_pools")
    sizes = [0, 65, 0, 128, 129, 0, 64, 1, 0]

    def pool(n):
        ids = sorted(rng.choice(range(0, 400)) for _ in range(n))         # repeats are possible
        return [(r, rng.randint(1, 9)) for r in ids]
    pools = [pool(n) for n in sizes]
    full = [a for a, n in enumerate(sizes) if n]
    edges = [(u, v) for u in full for v in full if u != v] + [(1, 2), (2, 3), (5, 4), (4, 5), (0, 3), (0, 2), (4, 8), (5, 8), (2, 5)]
    return sizes, pools, edges


def long_pools():
    """Pools of 65, 128 and 129 entries (a wavefront's second and third round over the target's pool) next to empty ones."""
    sizes, pools, edges = _long_pools()
    c = None

    def check(sup):
        need(sorted(len(c.pool(a)) for a in range(len(sizes))) == sorted(sizes) and {65, 128, 129} <= set(sizes), "65, 128, 129 entries")
        need(sizes[2] == sizes[5] == 0 and (1, 2) in edges and (2, 3) in edges, "edges to and from empty pools")
        need(sup[edges.index((1, 2))] == 0 and sup[edges.index((2, 3))] == 0, "an empty pool supports nothing")
        need(min(sup[edges.index((u, v))] for u in (1, 3, 4) for v in (1, 3, 4) if u != v) > 0, "the long pools share reads")
        need(c.pools_sorted(), "pools in read order")
    c = EdgeCase("long_pools", pools, [8], edges, [1], check)
    return c


def unsorted():
    """The graph of long_pools with shuffled pools under sorted = 0: the linear count."""
    sizes, pools, edges = _long_pools()
    rng = random.Random("graph_edge_lib:unsorted")
    for p in pools:
        rng.shuffle(p)
    c = None

    def check(sup):
        need(not c.pools_sorted(), "shuffled pools")
        need(sup == long_pools().reference(), "the supports of long_pools: the order inside a pool does not matter")
    c = EdgeCase("unsorted", pools, [8], edges, [0], check)
    return c


def sorted_flag_equal():
    """Sorted pools under both values of the flag: the two branches of the kernel on one input."""
    sizes, pools, edges = _long_pools()
    c = None

    def check(sup):
        need(c.pools_sorted() and c.flags == (1, 0), "sorted pools, both flags")
    c = EdgeCase("sorted_flag_equal", pools, [8], edges, [1, 0], check)
    return c


def grid_round():
    """8 200 edges: launch_edge_support caps the grid at 2 048 blocks of 4 wavefronts, the edges from 8 192 on are a
    wavefront's second (`e += nwaves`)."""
    rng = random.Random("graph_edge_lib:grid_round")
    n_nodes, n_edges = 300, 8200
    pools = [[]] + [[(r, rng.randint(1, 5)) for r in sorted(rng.sample(range(6), 0 if a % 7 == 0 else rng.randint(4, 6)))] for a in range(1, n_nodes - 1)] + [[]]
    edges = [(rng.randrange(0, n_nodes - 1), rng.randrange(1, n_nodes)) for _ in range(n_edges)]

    def check(sup):
        need(len(sup) == n_edges > GRID_BLOCKS * GRID_WAVES, "more edges than wavefronts")
        need(sum(1 for s in sup[GRID_BLOCKS * GRID_WAVES:] if s) >= 4, "second-round edges with support")
    return EdgeCase("grid_round", pools, [n_nodes - 1], edges, [1], check)


EDGE_CASES = {f.__name__: f for f in (source_and_end, multiplicity, long_pools, unsorted, sorted_flag_equal, grid_round)}
