"""A plain Python restatement of the read mapper's contract: the index, the votes, max_occ, the candidate
rule, the FASTQ reader and the SAM writer.  Nothing here imports the product; the expected alignments come from
tests/native/sw_check.cpp, run per group of reads with the same candidate set on the candidates in ascending gene order."""
import gzip

import stage4_lib as L

MAX_READ = 512
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NO_ROW = (0, -1, -1, 0, 0, "*", 0)          # a read without candidates: AS 0, XS -1, gene -1


def revcomp(s):
    return "".join(COMP.get(c, "N") for c in reversed(s.upper()))


def windows(seq, k):
    """The k-mer of every window of seq, None where the window holds a base outside ACGT."""
    s = seq.upper()
    return [s[i:i + k] if set(s[i:i + k]) <= set("ACGT") else None for i in range(len(s) - k + 1)]


def build_index(genes, k):
    """{k-mer: [gene of every occurrence, ascending]}: the run of a k-mer in the sorted keys."""
    index = {}
    for g, seq in enumerate(genes):
        for w in windows(seq, k):
            if w is not None:
                index.setdefault(w, []).append(g)
    return index


def strand_votes(index, seq, k, max_occ):
    """{gene: windows of seq whose k-mer the gene holds}; a run of more than max_occ entries casts no vote."""
    v = {}
    for w in windows(seq, k):
        run = index.get(w, ()) if w is not None else ()
        if len(run) > max_occ:
            continue
        for g in set(run):
            v[g] = v.get(g, 0) + 1
    return v


def candidates(index, read, k, max_occ, max_cand, min_votes):
    """[(gene, forward votes, reverse votes)] of the read's candidates, ascending by gene."""
    fw, rc = strand_votes(index, read, k, max_occ), strand_votes(index, revcomp(read), k, max_occ)
    v = {g: max(fw.get(g, 0), rc.get(g, 0)) for g in set(fw) | set(rc)}
    keep = [g for g in v if v[g] >= min_votes]
    if max_cand > 0:
        keep = sorted(keep, key=lambda g: (-v[g], g))[:max_cand]
    return [(g, fw.get(g, 0), rc.get(g, 0)) for g in sorted(keep)]


def all_candidates(genes, reads, k, max_occ, max_cand, min_votes, index=None):
    index = build_index(genes, k) if index is None else index
    return [candidates(index, r, k, max_occ, max_cand, min_votes) for r in reads]


def flat_candidates(cands):
    """(cand_off, gene, forward, reverse) as sc_map_candidates returns them."""
    off, gene, fw, rc = [0], [], [], []
    for c in cands:
        for g, a, b in c:
            gene.append(g); fw.append(a); rc.append(b)
        off.append(len(gene))
    return off, gene, fw, rc


def expected_rows(exe, genes, reads, cands):
    """[(AS, XS, gene, strand, pos, CIGAR, NM)] per read of `reads` = [(seq, qual or '*')]: sw_check on the read's candidates
    in ascending gene order, the indices mapped back."""
    groups = {}
    for r, c in enumerate(cands):
        groups.setdefault(tuple(g for g, _, _ in c), []).append(r)
    rows = [NO_ROW] * len(reads)
    for gset, members in groups.items():
        if not gset:
            continue
        got = L.run_sw_check(exe, [genes[g] for g in gset], [reads[r] for r in members])
        for r, row in zip(members, got):
            rows[r] = row[:2] + (gset[row[2]] if row[2] >= 0 else -1,) + row[3:]
    return rows


def device_rows(res):
    """capi.MapResult in the restatement's form."""
    return L.device_rows(res)


# ---------------------------------------------------------------------------------------------------- FASTQ and SAM

def fastq_records(path):
    """[(QNAME, SEQ, QUAL)] (text): records of four lines, QNAME up to the first blank without a trailing /1 or /2."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines = raw.decode().split("\n")
    if lines[-1] == "":
        lines.pop()
    assert len(lines) % 4 == 0
    out = []
    for k in range(0, len(lines), 4):
        name = lines[k][1:].split()[0]
        if name[-2:] in ("/1", "/2"):
            name = name[:-2]
        out.append((name, lines[k + 1], lines[k + 3]))
    return out


def cigar_ref_len(cigar):
    n, v = 0, ""
    for ch in cigar:
        if ch.isdigit():
            v += ch
        else:
            n += int(v) if ch in "MD" else 0
            v = ""
    return n


def sam_text(names, genes, sample, rows):
    """The whole SAM file of a sample = [(QNAME, [(seq, qual), ...])] with one row of expected_rows per read entry, flattened:
    @HD, one @SQ per gene, the mapped reads sorted by (gene, POS) stably over input order."""
    head = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(g)) for n, g in zip(names, genes))
    recs, k = [], 0
    for q, mates in sample:
        mine = rows[k:k + len(mates)]
        k += len(mates)
        for m, (as_, xs, gene, strand, pos, cigar, nm) in enumerate(mine):
            if gene < 0:
                continue
            seq, qual = mates[m]
            flag = 16 if strand else 0
            rnext, pnext, tlen = "*", 0, 0
            if len(mates) == 2:
                o = mine[1 - m]
                flag += 1 + (64 if m == 0 else 128)
                if o[2] < 0:
                    flag += 8
                else:
                    flag += 32 if o[3] else 0
                    pnext = o[4]
                    rnext = "=" if o[2] == gene else names[o[2]]
                    if o[2] == gene:
                        lo = min(pos, o[4])
                        hi = max(pos + cigar_ref_len(cigar), o[4] + cigar_ref_len(o[5])) - 1
                        tlen = (hi - lo + 1) * (1 if (pos < o[4] or (pos == o[4] and m == 0)) else -1)
            if strand:
                seq, qual = revcomp(seq), qual[::-1]
            fields = [q, str(flag), names[gene], str(pos), "0" if xs == as_ else "42", cigar, rnext, str(pnext), str(tlen), seq, qual,
                      "AS:i:%d" % as_] + (["XS:i:%d" % xs] if xs >= 0 else []) + ["NM:i:%d" % nm]
            recs.append(((gene, pos), "\t".join(fields) + "\n"))
    recs.sort(key=lambda r: r[0])
    return head + "".join(r[1] for r in recs)
