"""Files of a StrainCall run: the gene FASTA and its index, and the mapping file.

The reference shells out to samtools 0.1.19 four times per window
(/root/reference/StrainCall/StrainCall.cpp:167 faidx, :496 view, :696 mpileup,
:229/:256 faidx for the index) and parses the text.  Here the FASTA is read as the plain
text it is, and the mapping file (SAM text or BAM) is read once by the library
(rambl_amd/csrc/sc_ingest.cpp: BGZF + the BAM record layout of the SAM specification, or SAM
text) -- no subprocess, no temp files.  Parity at the samtools boundary itself stays unpinned
(SURVEY.md section 8(c)); the emulation of the tool's TEXT that the tests compare the reader
with is tests/py_ingest_mirror.py.

The SAM text the package writes itself (stage 4's re-clustered reads, the read mapper's sample) comes from sam_header and
sam_records below; the two callers differ in two policies that sam_records takes as arguments.
"""


def is_bam(path):
    with open(path, "rb") as f:
        return f.read(2) == b"\x1f\x8b"


def parse_region(reg):
    if ":" in reg:
        name, span = reg.rsplit(":", 1)
        a, b = span.split("-")
        return name, int(a), int(b)
    return reg, None, None


class Fasta:
    """Whole-file FASTA reader (seed-gene files are a few MB)."""

    def __init__(self, path):
        self.path = path
        self.seqs = {}
        self.order = []
        name = None
        chunks = None
        with open(path) as f:
            for line in f:
                line = line.rstrip("\r\n")
                if line.startswith(">"):
                    if name is not None:
                        self.seqs[name] = "".join(chunks)
                    name = line[1:].split()[0] if len(line) > 1 else ""
                    chunks = []
                    self.order.append(name)
                elif name is not None:
                    chunks.append(line)
        if name is not None:
            self.seqs[name] = "".join(chunks)

    def fetch(self, region):
        """Sequence text `samtools faidx fa region` would print (header removed)."""
        name, a, b = parse_region(region)
        if name not in self.seqs and region in self.seqs:
            name, a, b = region, None, None
        s = self.seqs.get(name, "")
        if a is not None:
            s = s[max(0, a - 1):b]
        return s


def read_fai(path):
    """[(name, length)] from <fasta>.fai: fields 1-2 (StrainCall.cpp:233-270)."""
    out = []
    with open(path) as f:
        for line in f:
            fld = line.split()
            if fld:
                out.append((fld[0], fld[1] if len(fld) > 1 else ""))
    return out


_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def revcomp(seq):
    return seq.translate(_COMP)[::-1]


def ref_len(cigar):
    """The reference bases a CIGAR text covers."""
    n, v = 0, 0
    for ch in cigar:
        if ch.isdigit():
            v = v * 10 + ord(ch) - 48
        else:
            if ch in "MD=XN":
                n += v
            v = 0
    return n


def sam_header(names, seqs):
    """@HD with SO:coordinate and one @SQ per reference, in the given order."""
    return "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs))


def sam_records(reads, ref, strand, pos, as_, xs, nm, cigar, names, keep_lone_mate, sort_by_strand):
    """The SAM lines of the aligned reads of `reads`, [(QNAME, [(SEQ, QUAL), ...])] with one or two mates per entry.  ref,
    strand, pos, as_, xs, nm and cigar hold one value per read entry of `reads` flattened (a pair's mates one after the
    other), as numpy arrays or lists: ref is the index into `names` (-1: unaligned, and no line), pos is 1-based, xs < 0
    means none.  MAPQ is 0 when XS = AS and 42 otherwise; a reverse read is written reverse-complemented.
    keep_lone_mate: an aligned read whose mate is unaligned is kept, with 0x8, RNEXT * and PNEXT 0 (False: the pair is dropped).
    sort_by_strand: the lines are sorted by (reference, POS, reverse) (False: by (reference, POS)), stably over the order
    of `reads`, mate 1 before mate 2."""
    ref, strand, pos = [int(v) for v in ref], [int(v) for v in strand], [int(v) for v in pos]
    recs = []
    k = 0
    for q, mates in reads:
        idx = list(range(k, k + len(mates)))
        k += len(mates)
        if not keep_lone_mate and any(ref[i] < 0 for i in idx):
            continue
        for m, i in enumerate(idx):
            if ref[i] < 0:
                continue
            seq, qual = mates[m]
            flag = 0x10 if strand[i] else 0
            rnext, pnext, tlen = "*", 0, 0
            if len(mates) == 2:
                o = idx[1 - m]
                flag |= 0x1 | (0x40 if m == 0 else 0x80)
                if ref[o] < 0:
                    flag |= 0x8
                else:
                    flag |= 0x20 if strand[o] else 0
                    pnext = pos[o]
                    rnext = "=" if ref[o] == ref[i] else names[ref[o]]
                    if ref[o] == ref[i]:
                        a0, a1 = pos[i], pos[i] + ref_len(cigar[i]) - 1
                        b0, b1 = pos[o], pos[o] + ref_len(cigar[o]) - 1
                        span = max(a1, b1) - min(a0, b0) + 1
                        tlen = span if (a0 < b0 or (a0 == b0 and m == 0)) else -span
            if strand[i]:
                seq, qual = revcomp(seq), qual[::-1]          # a quality of * stays *
            a, x = int(as_[i]), int(xs[i])
            tags = "AS:i:%d" % a + ("\tXS:i:%d" % x if x >= 0 else "") + "\tNM:i:%d" % int(nm[i])
            line = "%s\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (
                q.decode(), flag, names[ref[i]], pos[i], 0 if x == a else 42, cigar[i], rnext, pnext, tlen, seq.decode(), qual.decode(), tags)
            recs.append(((ref[i], pos[i], strand[i] if sort_by_strand else 0), line))
    recs.sort(key=lambda r: r[0])                     # stable: input order, mate 1 before mate 2, stays inside a key
    return [r[1] for r in recs]


class Alignments:
    """The mapping file (SAM text or BAM) of a StrainCall run, read and indexed once by the library (capi.NativeAln:
    sc_aln_*): what the reference gets from `samtools view` / `samtools mpileup` per window (StrainCall.cpp:496,696),
    without the subprocess and without the text.  A window's reads never become Python objects."""

    def __init__(self, path, only=None):
        """only: reference names whose records the reader keeps ([]: none, the per-reference statistics only;
        None: all) -- a rank of a multi-GPU run prices every region, then keeps its own shard."""
        from . import capi
        self.path = path
        self.native = capi.NativeAln(path, only)

    def pileup_flags(self, mq, region):
        """What window_adjust extracts from the pileup (StrainCall.cpp:702-736)."""
        name, a0, b0 = parse_region(region)
        return self.native.pileup_flags(mq, name, a0, b0)
