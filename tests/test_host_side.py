"""CPU: host-side pieces of the product path against the oracle -- Python ingest
(rows a1-a4), the C++ graph builder (a5, a6, a9-a11; MSA callback = oracle), the
libstdc++ sort port, the mt19937 stream, the CLI surface."""
import ctypes
import io
import os
import random
import re
import subprocess

import numpy as np
import pytest

import sc_testlib as T
import py_ingest_mirror as mirror          # the Python restatement of the read path (test infrastructure)
from rambl_amd import cli, ingest

ROOT = T.ROOT


def _dump_reads(args, d):
    base = os.path.join(d, "dump")
    T.run_oracle(args, d, graph=True, dump_reads=base)
    out = []
    i = 0
    while os.path.exists("%s.%d" % (base, i)):
        out.append(open("%s.%d" % (base, i)).read().splitlines())
        i += 1
    return out, base


def test_ingest_sorts_on_several_threads_match_oracle(tmp_path, oracle_bin):
    """sc_aln_load_reads sorts a deep region's reads on the ingest threads (stretches sorted side by side, merged pairwise):
    the cases of test_ingest_matches_oracle again in a child process whose stretches are 50 reads long and whose merges
    therefore all run."""
    import subprocess
    import sys
    env = dict(os.environ, SC_INGEST_SORT_MIN="50", SC_INGEST_THREADS="5")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", os.path.abspath(__file__), "-k", "test_ingest_matches_oracle"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    assert b"12 passed" in p.stdout


@pytest.mark.parametrize("seed", list(range(0, 12)))
def test_ingest_matches_oracle(seed, tmp_path, oracle_bin):
    d = str(tmp_path)
    args = T.make_case(seed, d)
    dumps, _ = _dump_reads(args, d)
    pa = cli.parse_cmd_line(args)
    regs = cli.load_regions(pa)
    assert len(regs) == len(dumps)
    for (w, r), lines in zip(regs, dumps):
        assert lines[0].split("\t")[1:] == [w[0], str(w[1]), str(w[2])]
        assert lines[1].split("\t")[1] == r.gene_seq
        exp = [l.split("\t") for l in lines[2:]]
        assert len(exp) == len(r)
        for i, e in enumerate(exp):
            got = [str(r.pos[i]), r.cigar[i], r.seq[i], str(r.copies[i]), ",".join(map(str, r.mates[i]))]
            assert got == e[1:6]


@pytest.fixture(scope="session")
def graph_check_bin(oracle_bin, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native") / "graph_host_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "native", "graph_host_check.cpp"),
                           *[os.path.join(ROOT, "rambl_amd", "csrc", f) for f in ("sc_graph.cpp", "sc_flatten.cpp", "sc_std_sort.cpp")],
                           "-L" + os.path.join(ROOT, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lpthread"])
    return out


@pytest.mark.parametrize("seed", list(range(0, 16)))
def test_host_graph_matches_oracle(seed, tmp_path, oracle_bin, graph_check_bin):
    d = str(tmp_path)
    args = T.make_case(seed, d)
    base = os.path.join(d, "dump")
    exp_g, _ = T.run_oracle(args, d, graph=True, dump_reads=base)
    got = ""
    i = 0
    while os.path.exists("%s.%d" % (base, i)):
        lines = open("%s.%d" % (base, i)).read().splitlines()
        if len(lines) > 2:
            p = subprocess.run([graph_check_bin, "%s.%d" % (base, i)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr.decode()
            assert "unsupported ''" in p.stderr.decode()
            got += p.stdout.decode()
        i += 1
    assert got == exp_g


# seeds 0-15 of make_case (reads with I and D, no symbol beyond A C G T) and a hand-made dump of 20 reads with one
# insertion, one deletion up to "$" and the symbols N and R: the smallest shape at which the label merge order, K and
# code_N can go wrong
FLAT_CASES = list(range(0, 16)) + ["hand"]


def _flat_digests(case, d, graph_check_bin, threads, min_entries):
    """{field: digest} of every region of the case that has reads, from `graph_host_check --flat-digest`."""
    if case == "hand":
        paths = [os.path.join(ROOT, "tests", "golden", "flat_hand_dump.txt")]
    else:
        base = os.path.join(d, "dump")
        T.run_oracle(T.make_case(case, d), d, graph=True, dump_reads=base)
        paths = []
        i = 0
        while os.path.exists("%s.%d" % (base, i)):
            if len(open("%s.%d" % (base, i)).read().splitlines()) > 2:
                paths.append("%s.%d" % (base, i))
            i += 1
    p = subprocess.run([graph_check_bin, "--flat-digest", str(threads), str(min_entries)] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    regions = []
    for line in p.stdout.decode().splitlines():
        if line.startswith("== "):
            regions.append({})
        else:
            k, v = line.split()
            regions[-1][k] = v
    assert len(regions) == len(paths) and all(len(r) == 30 for r in regions)
    return regions


@pytest.fixture(scope="session")
def flat_digests_serial(oracle_bin, graph_check_bin, tmp_path_factory):
    """The one-thread digests of every case, computed once for the two tests below."""
    return {case: _flat_digests(case, str(tmp_path_factory.mktemp("flat")), graph_check_bin, 1, 1 << 22) for case in FLAT_CASES}


@pytest.mark.parametrize("case", FLAT_CASES)
def test_flatten_threaded_equals_serial(case, tmp_path, graph_check_bin, flat_digests_serial):
    """Every FlatGraph array and every PoGraph pool at 4 threads with the threshold at 0 (the class pools, the pool copy,
    the label scan and the level fill all on helper threads) equals the one-thread result."""
    assert _flat_digests(case, str(tmp_path), graph_check_bin, 4, 0) == flat_digests_serial[case]


@pytest.mark.parametrize("case", FLAT_CASES)
def test_flatten_serial_equals_recorded(case, flat_digests_serial):
    """The one-thread digests equal those recorded from sc_graph.cpp as it stood before flatten and thread_reads were
    split (tests/golden/flat_digests.json; recorded twice, every case deterministic)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "flat_digests.json")))
    assert flat_digests_serial[case] == want[str(case)]


def _sort_cases():
    """Key sets full of ties at the sizes around libstdc++'s thresholds (16: insertion sort; 2 log2 n: heap fallback)."""
    rng = random.Random(3)
    cases = []
    for _ in range(300):
        n = rng.choice([1, 2, 5, 16, 17, 18, 33, 80, 81, 200, 1000])
        cases.append([float(rng.randint(0, max(1, n // rng.choice([1, 2, 8])))) for _ in range(n)])
    return cases


def test_product_sort_port_matches_libstdcxx(graph_check_bin):
    """sc::std_sort_perm (sc_std_sort.cpp) and the real std::sort in one binary, on the key sets of the test below."""
    text = "\n".join("%d %s" % (len(k), " ".join(map(repr, k))) for k in _sort_cases())
    p = subprocess.run([graph_check_bin, "--sort-check"], input=text.encode(), stdout=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode()
    assert p.stdout.decode().strip() == "300 cases equal"


def test_sort_port_matches_libstdcxx(tmp_path, oracle_bin):
    """oracle's std::sort port vs the real libstdc++ std::sort on keys full of ties."""
    src = tmp_path / "s.cpp"
    src.write_text(r'''
#include <algorithm>
#include <cstdio>
#include <vector>
int main() { int n; while (scanf("%d", &n) == 1) { std::vector<double> k(n); for (auto& x : k) scanf("%lf", &x);
  std::vector<int> p(n); for (int i = 0; i < n; i++) p[i] = i;
  std::sort(p.begin(), p.end(), [&](int a, int b) { return k[a] > k[b]; });
  for (int i = 0; i < n; i++) printf("%d ", p[i]); printf("\n"); } }
''')
    exe = str(tmp_path / "s")
    subprocess.check_call(["g++", "-O1", "-o", exe, str(src)])
    lib = T.oracle_lib()
    rng = random.Random(3)
    text, cases = [], []
    for _ in range(300):
        n = rng.choice([1, 2, 5, 16, 17, 18, 33, 80, 81, 200, 1000])
        keys = [float(rng.randint(0, max(1, n // rng.choice([1, 2, 8])))) for _ in range(n)]
        cases.append(keys)
        text.append("%d %s" % (n, " ".join(map(repr, keys))))
    out = subprocess.run([exe], input="\n".join(text).encode(), stdout=subprocess.PIPE).stdout.decode().splitlines()
    for keys, line in zip(cases, out):
        n = len(keys)
        perm = (ctypes.c_int * n)()
        lib.oracle_sort_desc_perm((ctypes.c_double * n)(*keys), n, perm)
        assert list(perm) == [int(x) for x in line.split()]


def test_mt19937_canonical_stream(oracle_bin):
    lib = T.oracle_lib()
    n = 3000
    out = (ctypes.c_double * n)()
    lib.oracle_mt_canonical(1234, n, out)
    gen = mirror.MT19937(1234)
    assert [gen.canonical() for _ in range(n)] == list(out)
    # std::mt19937 known answer: the 10000th output of the default-seeded engine is 4123659995
    g = mirror.MT19937(5489)
    v = 0
    for _ in range(10000):
        v = g.next_u32()
    assert v == 4123659995


def test_cli_argv_forms():
    pa = cli.parse_cmd_line(["-r", "g:1-10", "--window", "77", "-overlap", "5", "-e", "0.5", "-q", "7", "-D", "9",
                             "-I", "3", "-l", "44", "-t", "0.25", "--diff-rate", "0.125", "-G", "--bogus", "a.fa", "b.bam", "c.bam"])
    assert (pa.roi, pa.window_size, pa.overlap_size, pa.mapping_qual, pa.max_depth, pa.max_ins, pa.read_len) == \
        ("g:1-10", 77, 5, 7, 9, 3, 44)
    assert float(pa.error_rate) == 0.5 and float(pa.tau) == 0.25 and float(pa.diff_rate) == 0.125
    assert pa.plot_graph and pa.gene_file == "a.fa" and pa.mapping_file == "c.bam"
    assert float(cli.parse_cmd_line(["-t", "0.02"]).tau) == float(np.float32(0.02))
    assert ingest.stoi("12abc") == 12
    with pytest.raises(ValueError):
        ingest.stoi("abc")
    assert ingest.gene_roi_end_pos("g:1-9") == 9
    with pytest.raises(ValueError):            # first '-' of the WHOLE roi (StrainCall.cpp:210-220): stoi("b:1-9") throws
        ingest.gene_roi_end_pos("a-b:1-9")


def test_cli_help_goes_to_stderr():
    out, err = io.StringIO(), io.StringIO()
    assert cli.main([], out=out, err=err) == 0
    assert out.getvalue() == "" and err.getvalue().startswith("StrainCall marker_gene read_mapping")
    out, err = io.StringIO(), io.StringIO()
    assert cli.main(["-h", "x.fa", "y.sam"], out=out, err=err) == 0
    assert "-G,--plot-graph    print graph" in err.getvalue()


def test_crop_and_cigar_helpers():
    assert mirror.parse_cigar("3S10M2I4D5=6X") == [("S", 3), ("M", 10), ("I", 2), ("D", 4), ("M", 5), ("M", 6)]
    cig = mirror.parse_cigar("10M")
    assert mirror.crop_read_within_window(5, 8, "ACGTACGTAC", "IIIIIIIIII", cig, 3, 12) == ("GTAC", "4M")
    assert mirror.crop_read_within_window(1, 100, "ACGTACGTAC", "IIIIIIIIII", cig, 3, 12) == ("ACGTACGTAC", "10M")
    assert mirror.max_insert_size("5M3I2M7I1M") == 7


@pytest.fixture(scope="module")
def ingest_check_bin(tmp_path_factory):
    """tests/native/ingest_check.cpp with the two ingest sources, plain g++ under the address and undefined-behaviour
    sanitizers: not the library, nothing loaded into Python."""
    out = str(tmp_path_factory.mktemp("native") / "ingest_check")
    csrc = os.path.join(ROOT, "rambl_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out, os.path.join(ROOT, "tests", "native", "ingest_check.cpp"), os.path.join(csrc, "sc_aln_file.cpp"),
                           os.path.join(csrc, "sc_ingest.cpp"), "-lz", "-lpthread"])
    return out


def _crop_named_cases():
    """(name, w0, w1, pos, cigar) at the smallest sizes.  The plain reads cover 10-19 (10M), 10-14 + 15-19 around an
    insertion (5M2I5M), 10-14 + 17-21 around a deletion at 15-16 (5M2D5M)."""
    plain = [
        ("window starts inside an M", 12, 30, 10, "10M"),
        ("window starts inside a D", 16, 30, 10, "5M2D5M"),
        ("window starts on the M/I boundary, insertion in front of w0", 15, 30, 10, "5M2I5M"),
        ("window starts on the last M base before the I", 14, 30, 10, "5M2I5M"),
        ("window starts on the M/D boundary", 15, 30, 10, "5M2D5M"),
        ("window starts on the first M base after the D", 17, 30, 10, "5M2D5M"),
        ("insertion immediately after w1", 5, 14, 10, "5M2I5M"),
        ("window ends on the first M base after the I", 5, 15, 10, "5M2I5M"),
        ("window ends on the M/D boundary", 5, 14, 10, "5M2D5M"),
        ("window ends inside the D", 5, 15, 10, "5M2D5M"),
        ("read ends exactly at w1", 5, 19, 10, "10M"),
        ("read ends one past w1", 5, 18, 10, "10M"),
        ("read starts exactly at w0", 10, 30, 10, "10M"),
        ("read starts one before w0", 11, 30, 10, "10M"),
        ("read wholly inside the window", 5, 30, 10, "10M"),
        ("read covers the whole window", 12, 15, 10, "10M"),
        ("w0 == w1 inside the read", 12, 12, 10, "10M"),
        ("w0 == w1 on the read's first base", 10, 10, 10, "10M"),
        ("w0 == w1 on the read's last base", 19, 19, 10, "10M"),
        ("w0 == w1 inside a D", 15, 15, 10, "5M2D5M"),
        ("N inside the window", 5, 30, 10, "4M3N4M"),
        ("N across the window start", 15, 30, 10, "4M3N4M"),
        ("N across the window end", 5, 15, 10, "4M3N4M"),
        ("= and X", 5, 30, 3, "3=1X2I1D2M"),
        ("= and X cut at both ends", 4, 7, 3, "3=1X2I1D2M"),
        ("zero-length operation first", 5, 30, 10, "0M10M"),
        ("zero-length operation first, cut in front", 12, 30, 10, "0M10M"),
        ("read wholly before the window", 30, 40, 10, "10M"),
        ("read wholly after the window", 30, 40, 50, "10M"),
        ("everything consumed by the front walk", 20, 30, 10, "10M"),
    ]
    cases = list(plain)
    cases += [(name + ", soft clips on both ends", w0, w1, pos, "3S" + cig + "4S") for name, w0, w1, pos, cig in plain]
    cases += [
        ("H outside the S", 12, 17, 10, "2H3S10M4S2H"),
        ("H outside the S, read inside the window", 5, 30, 10, "2H3S10M4S2H"),
        ("zero-length soft clip first", 12, 30, 10, "0S10M"),
        ("only S", 5, 30, 10, "5S"),
        ("only S and H", 5, 30, 10, "5S2H"),
        ("trailing S when the front walk consumed everything else", 20, 30, 10, "10M4S"),
        ("trailing S after an insertion the back walk removes", 5, 14, 10, "5M2I5M4S"),
    ]
    return cases


def _crop_random_cases(seed=7, n=2000):
    """CIGARs and positions of _random_sam's generator, each with a window that starts near the read's start."""
    import tempfile
    rng = random.Random(seed)
    with tempfile.TemporaryDirectory() as d:
        _random_sam(rng, os.path.join(d, "x.sam"), n=n)
        recs = [ln.split("\t") for ln in open(os.path.join(d, "x.sam")) if not ln.startswith("@")][:n]
    cases = []
    for k, f in enumerate(recs):
        w0 = max(1, int(f[3]) + rng.randint(-20, 30))
        cases.append(("random %d" % k, w0, w0 + rng.randint(0, 120), int(f[3]), f[5]))
    return cases


def _bam_error_files(d):
    """{file: the message sc_aln_open must give}: BGZF and BAM bytes broken by hand in one place each, and the intact file."""
    import struct
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 2) + b"g\x00" + struct.pack("<i", 50)

    def rec(l_seq, extra_block=0):
        body = struct.pack("<iiBBHHHiiii", 0, 4, 3, 30, 4680, 1, 0, l_seq, -1, -1, 0) + b"r1\x00" + struct.pack("<I", 4 << 4) + bytes([0x12, 0x48]) + bytes([30] * 4)
        return struct.pack("<i", len(body) + extra_block) + body

    good = _bgzf_block(head + rec(4))
    no_bc = good.replace(b"BC", b"XY", 1)
    big = good[:-4] + struct.pack("<I", 65537)
    crc = good[:-8] + struct.pack("<I", struct.unpack("<I", good[-8:-4])[0] ^ 1) + good[-4:]
    files = {
        "good.bam": (good, ""),
        "cut_in_data.bam": (good[:-10], "BGZF block without a BC field or truncated"),
        "cut_in_extra.bam": (good[:20], "truncated BGZF block"),
        "no_bc.bam": (no_bc, "BGZF block without a BC field or truncated"),
        "isize.bam": (big, "BGZF block claims more than 64 KiB of data"),
        "crc.bam": (crc, "corrupt BGZF block (inflate or CRC-32)"),
        "block_size.bam": (_bgzf_block(head + rec(4, extra_block=100)), "truncated BAM record"),
        "l_seq.bam": (_bgzf_block(head + rec(4000)), "corrupt BAM record"),
        "l_seq_negative.bam": (_bgzf_block(head + rec(-1)), "corrupt BAM record"),
    }
    for name, (blob, _) in files.items():
        open(os.path.join(d, name), "wb").write(blob)
    return {os.path.join(d, name): msg for name, (_, msg) in files.items()}


def test_ingest_native_check(ingest_check_bin, tmp_path):
    """The pure parts of the ingest (sc_cigar.hpp, stable_sort_mt and name_cmp of sc_ingest.hpp, the BGZF/BAM decoder of
    sc_aln_file.cpp) in a stand-alone program under the host sanitizers, which end the program at the first fault.
    (a) parse_cigar + crop_to_window on named edge cases and 2 000 random ones equal the Python mirror's
    crop_read_within_window: bases, CIGAR text, and a failure exactly where the mirror raises.  (b) stable_sort_mt equals
    std::stable_sort on keys full of ties around every nt * min_stretch; name_cmp orders as std::string does.  (c) every
    BGZF / BAM error path on hand-made bytes returns its message."""
    def run(args, text=b""):
        p = subprocess.run([ingest_check_bin] + args, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, (p.stdout.decode()[-2000:], p.stderr.decode()[-4000:])
        return p.stdout.decode().split("\n")[:-1]
    # (a)
    named, rand = _crop_named_cases(), _crop_random_cases()
    assert len({c[0] for c in named}) == len(named) and len(rand) == 2000
    rng = random.Random(11)
    seqs, want = [], []
    for name, w0, w1, pos, cig in named + rand:
        ops = mirror.parse_cigar(cig)
        seq = "".join(rng.choice("ACGT") for _ in range(sum(int(n) for n in re.findall(r"(\d+)[MIS=X]", cig))))
        seqs.append(seq)
        try:
            want.append(mirror.crop_read_within_window(w0, w1, seq, "I" * len(seq), ops, pos, mirror.read_align_end_pos(pos, ops)))
        except (IndexError, ValueError):
            want.append(None)
    n_fail_random = sum(w is None for w in want[len(named):])
    assert n_fail_random <= 200, n_fail_random
    fails = {c[0] for c, w in zip(named, want) if w is None}
    assert {"only S", "read wholly before the window", "read wholly after the window"} <= fails
    text = "".join("%d %d %d %s %d\n" % (w0, w1, pos, cig, len(seq)) for (_, w0, w1, pos, cig), seq in zip(named + rand, seqs))
    out = run(["crop"], text.encode())
    assert len(out) == len(want)
    for (name, w0, w1, pos, cig), seq, w, line in zip(named + rand, seqs, want, out):
        if w is None:
            assert line == "FAIL", (name, w0, w1, pos, cig, line)
            continue
        assert line != "FAIL", (name, w0, w1, pos, cig)
        lead, trail, got_cig = line.split(" ")
        bases, exp_cig = w
        cnt = len(seq) - int(lead) - int(trail)
        assert (seq[int(lead):] if cnt < 0 else seq[int(lead):int(lead) + cnt], got_cig) == (bases, exp_cig), (name, w0, w1, pos, cig, line)
    # (b)
    assert run(["order"])[-1] == "order ok"
    # (c)
    files = _bam_error_files(str(tmp_path))
    out = run(["open"] + list(files))
    assert len(out) == len(files)
    for (path, msg), line in zip(files.items(), out):
        rc, n, got = line.split(" ", 2)
        assert (rc == "0", got) == (msg == "", msg), (path, line)
        assert n == ("1" if msg == "" else "0"), (path, line)


@pytest.mark.parametrize("seed", [0, 1, 2, 5, 6, 13])
def test_pileup_flags_equal_pileup_text(seed, tmp_path):
    """The array-based pileup summary equals the summary of the emulated pileup text."""
    from rambl_amd import samio
    args = T.make_case(seed, str(tmp_path))
    aln = samio.Alignments(args[-1])
    text = mirror.SamText(args[-1])
    name = "g%d" % seed
    for region in ("%s:1-5000" % name, "%s:40-180" % name, "%s:200-260" % name):
        for mq in (0, 50):
            assert aln.pileup_flags(mq, region) == mirror.flags_from_pileup_text(text.mpileup(mq, region)) == text.pileup_flags(mq, region)


@pytest.mark.parametrize("seed", [2, 4])
def test_native_bam_reader_gives_the_same_regions(seed, tmp_path, monkeypatch):
    """BAM input read natively (no samtools in the image) yields the same ingest as the SAM text."""
    d = str(tmp_path)
    args = T.make_case(seed, d)
    bam = os.path.join(d, "reads.bam")
    T.write_bam(args[-1], bam)
    from rambl_amd import samio
    assert samio.is_bam(bam)
    a = cli.load_regions(cli.parse_cmd_line(args))
    b = cli.load_regions(cli.parse_cmd_line(args[:-1] + [bam]))
    assert len(a) == len(b)
    for (wa, ra), (wb, rb) in zip(a, b):
        assert wa == wb and ra.gene_seq == rb.gene_seq
        assert (ra.pos, ra.cigar, ra.seq, ra.copies, ra.mates) == (rb.pos, rb.cigar, rb.seq, rb.copies, rb.mates)


def _random_sam(rng, path, genes=("gA", "gB"), n=400, glen=400):
    """SAM records with every CIGAR shape the ingest has a rule for: soft / hard clips, insertions and deletions at
    and across window edges, = and X, N skips, reads hanging over both ends of a window, duplicates, mates by flag
    and by name, repeated names, filtered flags, low mapping qualities, short reads, N bases."""
    lines = ["@SQ\tSN:%s\tLN:%d" % (g, glen) for g in genes]
    recs = []
    for k in range(n):
        g = rng.choice(genes)
        pos = rng.randint(1, glen - 30)
        ops = []
        if rng.random() < 0.15:
            ops.append((rng.randint(1, 12), "H"))
        if rng.random() < 0.3:
            ops.append((rng.randint(1, 15), "S"))
        body = []
        for _ in range(rng.randint(1, 6)):
            body.append((rng.randint(1, 60), rng.choice("MMMM=X")))
            r = rng.random()
            if r < 0.25:
                body.append((rng.randint(1, 14), "I"))
            elif r < 0.5:
                body.append((rng.randint(1, 9), "D"))
            elif r < 0.55:
                body.append((rng.randint(1, 20), "N"))
        while body and body[-1][1] in "IDN":
            body.pop()
        ops += body
        if rng.random() < 0.3:
            ops.append((rng.randint(1, 15), "S"))
        if rng.random() < 0.1:
            ops.append((rng.randint(1, 12), "H"))
        qlen = sum(l for l, o in ops if o in "MIS=X")
        seq = "".join(rng.choice("ACGT") for _ in range(qlen))
        if rng.random() < 0.04:
            seq = seq[:3] + rng.choice("Nn") + seq[4:]
        flag = rng.choice([0, 0, 0, 16, 65, 129, 81, 161, 4, 256, 512, 1024, 2048, 99, 147])
        name = "r%d" % rng.randint(0, n // 2)
        if rng.random() < 0.1:
            name += rng.choice(["/1", "/2"])
        mapq = rng.choice([0, 1, 3, 9, 10, 12, 30, 42, 60])
        recs.append((g, pos, "\t".join([name, str(flag), g, str(pos), str(mapq), "".join("%d%s" % x for x in ops), "*", "0", "0", seq,
                                        "I" * len(seq)])))
        if rng.random() < 0.2:      # an exact duplicate under another name
            f = recs[-1][2].split("\t")
            f[0] = "d%d" % k
            recs.append((g, pos, "\t".join(f)))
    recs.sort(key=lambda r: (r[0], r[1]))
    with open(path, "w") as f:
        f.write("\n".join(lines + [r[2] for r in recs]) + "\n")


@pytest.mark.parametrize("seed", list(range(8)))
def test_native_ingest_equals_python_mirror(seed, tmp_path):
    """sc_aln_* (C++, the product's reader) against the Python mirror of StrainCall.cpp:480-736 on records with every
    CIGAR shape, over many windows and option values: reads, copies, mates, depth thinning, pileup flags."""
    from rambl_amd import capi, samio
    rng = random.Random(1000 + seed)
    sam = str(tmp_path / "x.sam")
    _random_sam(rng, sam)
    nat = capi.NativeAln(sam)
    py = mirror.SamText(sam)

    class PyAln:
        native = None
        view = staticmethod(lambda mq, region: py.view(mq, 1804, region))
    n_checked = 0
    for _ in range(40):
        g = rng.choice(["gA", "gB"])
        p0 = rng.randint(1, 300)
        p1 = rng.randint(p0 + 5, 400)
        mq = rng.choice([0, 3, 10])
        rl = rng.choice([0, 20, 70])
        max_ins = rng.choice([3, 10, 13])
        max_depth = rng.choice([2, 10, 800])
        roi = "%s:%d-%d" % (g, p0, p1)
        assert nat.pileup_flags(mq, g, p0, p1) == py.pileup_flags(mq, roi)
        try:
            exp = mirror.load_mapping_reads("", PyAln, mq, rl, max_ins, max_depth, roi)
        except (ValueError, IndexError):
            with pytest.raises(capi.StrainCallError):
                nat.load_reads("", g, p0, p1, mq, rl, max_ins, max_depth)
            continue
        got = nat.load_reads("", g, p0, p1, mq, rl, max_ins, max_depth)
        assert (got.pos, got.cigar, got.seq, got.copies, got.mates) == (exp.pos, exp.cigar, exp.seq, exp.copies, exp.mates), roi
        assert got.n_input == len(py.view(mq, 1804, roi))
        n_checked += len(exp)
    assert n_checked > 200


def test_add_ones_equals_the_literal_loop(tmp_path):
    """The urn update `a[c] += 1` per draw (NonparametricClustering.cpp:195) in O(log k): tests/native/add_ones_check.cpp
    compares sc_add_ones with the literal long double loop around every binade border and at random."""
    exe = str(tmp_path / "add_ones_check")
    subprocess.check_call(["g++", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "add_ones_check.cpp"),
                           "-L" + os.path.join(ROOT, "rambl_amd"), "-lstraincall_hip", "-Wl,-rpath," + os.path.join(ROOT, "rambl_amd")])
    p = subprocess.run([exe], stdout=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode()
    assert b" 0 differences" in p.stdout


def _bgzf_block(payload):
    """One BGZF block exactly as SAM specification section 4.1 lays it out (gzip member, FEXTRA with the BC subfield)."""
    import struct
    import zlib
    comp = zlib.compressobj(9, zlib.DEFLATED, -15)
    cdata = comp.compress(payload) + comp.flush()
    bsize = len(cdata) + 25                                   # total block size - 1
    return (b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<H", 2) +
            struct.pack("<H", bsize) + cdata + struct.pack("<I", zlib.crc32(payload) & 0xFFFFFFFF) + struct.pack("<I", len(payload)))


@pytest.mark.parametrize("threads", ["1", "5"])
def test_bam_of_many_bgzf_members_decodes_like_the_sam(threads, tmp_path, monkeypatch):
    """A BAM of a few hundred BGZF members (inflated side by side by SC_INGEST_THREADS host threads) gives the records of
    the SAM text it was written from, in the same order; a flipped bit in one member is reported, not decoded."""
    from rambl_amd import capi, synth
    monkeypatch.setenv("SC_INGEST_THREADS", threads)
    gene = synth.make_gene(7, glen=1500, n_strains=3, n_reads=60000, name="g7")
    fa, sam = synth.write_dataset(str(tmp_path), [gene])
    bam = str(tmp_path / "reads.bam")
    T.write_bam(sam, bam)
    assert os.path.getsize(bam) > 300000                 # ~230 members of 60 000 bytes before compression
    a, b = capi.NativeAln(sam), capi.NativeAln(bam)
    assert a.records() == b.records() == 60000
    seq = open(fa).read().split("\n", 1)[1].replace("\n", "")
    ra, rb = a.load_reads(seq, "g7", 1, 1500, 0, 70, 13, 800), b.load_reads(seq, "g7", 1, 1500, 0, 70, 13, 800)
    assert (ra.pos, ra.cigar, ra.seq, ra.copies, ra.mates) == (rb.pos, rb.cigar, rb.seq, rb.copies, rb.mates)
    raw = bytearray(open(bam, "rb").read())
    raw[len(raw) // 2] ^= 0x40
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(capi.StrainCallError):
        capi.NativeAln(bad)


def test_bam_decoder_on_hand_assembled_bytes(tmp_path):
    """The library's BGZF/BAM decoder (sc_aln_open) on bytes assembled field by field from the SAM specification (section
    4.2: block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen, read_name,
    cigar as oplen<<4|op, 4-bit packed seq over '=ACMGRSVTWYHKDBN', qual) -- not by any BAM writer of this repository:
    records that straddle BGZF block borders, an empty block in the middle, = and X and N and H and P operations, an odd
    l_seq, a 0xff quality string, an unmapped mate (flag 73) and a fully unmapped read (refID -1).  The expected SAM fields
    are written out by hand below; the Python reader (samio.bam_records, gzip module) must agree too."""
    import struct
    from rambl_amd import capi, samio

    def rec(ref_id, pos0, name, mapq, cigar_ops, flag, seq_nibbles, l_seq, qual, next_ref=-1, next_pos=-1, tlen=0):
        body = struct.pack("<iiBBHHHiiii", ref_id, pos0, len(name) + 1, mapq, 4680, len(cigar_ops), flag, l_seq, next_ref, next_pos, tlen)
        body += name + b"\x00" + b"".join(struct.pack("<I", c) for c in cigar_ops) + seq_nibbles + qual
        return struct.pack("<i", len(body)) + body

    hdr_text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:otuA\tLN:50\n@SQ\tSN:otuB\tLN:40\n"
    head = b"BAM\x01" + struct.pack("<i", len(hdr_text)) + hdr_text + struct.pack("<i", 2)
    head += struct.pack("<i", 5) + b"otuA\x00" + struct.pack("<i", 50) + struct.pack("<i", 5) + b"otuB\x00" + struct.pack("<i", 40)
    # r1: otuA pos 3, 2S 3= 1X 2I 1D 2M (7 aligned read bases + 2 clipped = 10 bases "TTACGTAACG"), flag 99, mate at otuA:30
    r1 = rec(0, 2, b"r1", 42, [2 << 4 | 4, 3 << 4 | 7, 1 << 4 | 8, 2 << 4 | 1, 1 << 4 | 2, 2 << 4 | 0], 99,
             bytes([0x88, 0x12, 0x48, 0x11, 0x24]), 10, bytes([40] * 10), 0, 29, 37)
    # r2: otuA pos 10, 5M 4N 3M with hard clips and a pad: 2H 5M 4N 1P 3M 3H; 8 bases "GGGGGCCC"; odd length next: see r3
    r2 = rec(0, 9, b"read/2", 0, [2 << 4 | 5, 5 << 4 | 0, 4 << 4 | 3, 1 << 4 | 6, 3 << 4 | 0, 3 << 4 | 5], 16,
             bytes([0x44, 0x44, 0x42, 0x22]), 8, bytes([0xff] * 8))
    # r3: otuB pos 1, 7M, 7 bases "ACGTNRY" (odd l_seq: the last low nibble is padding), mate unmapped (flag 73)
    r3 = rec(1, 0, b"r3", 255, [7 << 4 | 0], 73, bytes([0x12, 0x48, 0xF5, 0xA0]), 7, bytes(range(7)), 1, 0, 0)
    # r4: unmapped, no reference, no cigar, 4 bases "TTTT"
    r4 = rec(-1, -1, b"r4", 0, [], 77, bytes([0x88, 0x88]), 4, bytes([30] * 4))
    stream = head + r1 + r2 + r3 + r4
    # block borders inside the header, inside r1's cigar, inside r2's name; one empty block; EOF marker block
    cuts = [0, 17, len(head) + 44, len(head) + len(r1) + 40, len(stream)]
    blob = b""
    for a, b in zip(cuts, cuts[1:]):
        blob += _bgzf_block(stream[a:b])
        if a == 17:
            blob += _bgzf_block(b"")
    blob += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    path = str(tmp_path / "hand.bam")
    open(path, "wb").write(blob)

    expected = [
        ["r1", "99", "otuA", "3", "42", "2S3=1X2I1D2M", "=", "30", "37", "TTACGTAACG", "I" * 10],
        ["read/2", "16", "otuA", "10", "0", "2H5M4N1P3M3H", "*", "0", "0", "GGGGGCCC", "*"],
        ["r3", "73", "otuB", "1", "255", "7M", "=", "1", "0", "ACGTNRY", "!\"#$%&'"],
        ["r4", "77", "*", "0", "0", "*", "*", "0", "0", "TTTT", "????"],
    ]
    assert list(mirror.bam_records(path)) == expected
    aln = capi.NativeAln(path)
    assert aln.records() == 4
    assert aln.ref_stats("otuA") == (2, (3 + 1 + 1 + 2) + (5 + 4 + 3)) and aln.ref_stats("otuB") == (1, 7) and aln.ref_stats("*") == (1, 1)
    # view semantics on them: -F 1804 drops r4 (unmapped) and keeps r1 (99), r2 (16), r3 (73: mate unmapped is bit 8 = filtered)
    got = aln.load_reads("", "otuA", 1, 50, 0, 0, 13, 800)
    assert got.n_input == 2
    assert (got.pos, got.cigar, got.seq, got.copies) == ([2, 9], ["3M1M2I1D2M", "2H5M4N1P3M3H"], ["ACGTAACG", "GGGGGCCC"], [1, 1])
    assert got.mates == [[-1], [-1]]                         # r1 -> "r1/1" (flag 99 has 65 set? 99 = 1+2+32+64: yes), mate "r1/2" absent
    assert aln.load_reads("", "otuB", 1, 40, 0, 0, 13, 800).n_input == 0      # flag 73 & 1804 = 8: mate unmapped is filtered by -F 1804
    # pileup: r1 covers 3-9 (insertion marked on the base before it, 6; deleted base 7), r2 covers 10-21; its reference
    # skip 15-18 prints '<' (reverse strand), which window_adjust (StrainCall.cpp:712-735) does not read as a deletion
    assert aln.pileup_flags(0, "otuA", 1, 50) == {p: (p == 6, p == 7) for p in range(3, 22)}


def test_reference_skip_is_coverage_not_deletion(tmp_path):
    """CIGAR N (reference skip): mpileup prints '>' / '<' there, not '*'; window_adjust looks for '+', '-' and '*' only
    (StrainCall.cpp:712-735), so the skipped span counts as covered and carries no deletion mark -- in the native
    reader, in the Python mirror and in the pileup text of the stand-in alike."""
    from rambl_amd import capi, samio
    sam = tmp_path / "n.sam"
    sam.write_text("@SQ\tSN:g\tLN:60\n"
                   "a\t0\tg\t5\t30\t4M3N4M1D2M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n"
                   "b\t16\tg\t20\t30\t3M2N3M\t*\t0\t0\tACGTAC\tIIIIII\n")
    want = {p: (False, p in (15, 16)) for p in list(range(5, 19)) + list(range(20, 28))}     # 15: "-1N" on the base before; 16: '*'
    nat = capi.NativeAln(str(sam))
    assert nat.pileup_flags(0, "g", 1, 60) == want
    text = mirror.SamText(str(sam))
    assert text.pileup_flags(0, "g:1-60") == want
    lines = text.mpileup(0, "g:1-60")
    assert mirror.flags_from_pileup_text(lines) == want
    assert ">" in lines[4].split("\t")[4] and "<" in [ln for ln in lines if ln.split("\t")[1] == "23"][0].split("\t")[4]
