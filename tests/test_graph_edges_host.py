"""CPU: every named edge case of tests/graph_edge_lib.py is deterministic and reaches its edge on the plain references alone;
thread_reference agrees with the restatement loops of test_gpu_parity.py on seeded regions, edge_support_reference with the
supports the C oracle prints for the pools it dumps, every MSA case through the oracle equals the rows recorded from the
reference, and the ACGT threading cases are regions the oracle accepts with every read kept."""
import gzip
import json
import os
import subprocess

import pytest

import graph_edge_lib as G
import sc_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(case):
    try:
        return case.reference()
    except ValueError:
        return None


@pytest.mark.parametrize("name", sorted(G.THREAD_CASES))
def test_thread_case_reaches_its_edge(name):
    case = G.THREAD_CASES[name]()
    assert case.name == name and case.key() == G.THREAD_CASES[name]().key()                # a function of its name alone
    r = case.reads
    assert len(r) == len(r.cigar) == len(r.seq) == len(r.copies) == len(r.mates) >= 1
    assert r.pos == sorted(r.pos) and len(set(zip(r.pos, r.cigar, r.seq))) == len(r)         # start order, distinct
    assert all(0 <= p <= len(r.gene_seq) for p in r.pos) and set(r.gene_seq) <= set("ACGT")
    for cig, seq in zip(r.cigar, r.seq):
        ops = G.parse_cigar(cig)
        assert "".join("%d%s" % (n, op) for op, n in ops) == cig.replace("=", "M").replace("X", "M")
        assert sum(n for op, n in ops if op in "MI") == len(seq)
    ref = _reference(case)
    assert (ref is None) == (case.error is not None)
    assert case.wide == (name in G.WIDE_CASES) and case.parity == (name in G.PARITY_CASES)
    if case.parity:
        assert len(r) <= 300 and all(set(s) <= set("ACGT") for s in r.seq)
    case.check(ref, G.BIG_WORDS)
    if case.wide:
        case.check(ref, G.CHILD_BIG_WORDS)


def test_thread_reference_on_a_hand_computed_case():
    #            0123456789
    reads = G.Reads("ACGTACGTAC", [(0, "3M", "ACG"), (1, "2M1I2M", "CTNTA"), (2, "2M2D2M", "GTGN"), (8, "1M1M", "AC")])
    ref = G.thread_reference(reads.gene_seq, reads)
    assert ref["sym"] == b"ACGTN\0\0\0"
    A, C, Gc, Tc, N = range(5)

    def cls(i, c):
        return i * 8 + c
    exp_members = {cls(0, A): [0], cls(1, C): [0, 1], cls(2, Gc): [0, 2], cls(2, Tc): [1], cls(3, Tc): [1, 2], cls(4, A): [1],
                   cls(6, Gc): [2], cls(7, N): [2], cls(8, A): [3], cls(9, C): [3]}
    assert {c: ref["pool"][ref["off"][c]:ref["off"][c + 1]] for c in range(80) if ref["count"][c]} == exp_members
    assert [ref["first"][c] for c in sorted(exp_members)] == [m[0] for _, m in sorted(exp_members.items())]
    assert {c: v for c, v in enumerate(ref["smin"]) if v != G.INT_MAX} == {cls(0, A): 0, cls(1, C): 1, cls(2, Gc): 2, cls(8, A): 3}
    assert {c: v for c, v in enumerate(ref["emin"]) if v != G.INT_MAX} == {cls(2, Gc): 0, cls(4, A): 1, cls(7, N): 2, cls(9, C): 3}
    # read 1: C->T inside its first run, nothing into position 3 (after the I), T->A inside the second; read 2: nothing into
    # position 6 (after the D); read 3: A->C across two adjacent M operations
    assert {e: v for e, v in enumerate(ref["tmin"]) if v != G.INT_MAX} == {
        1 * 64 + A * 8 + C: 0, 2 * 64 + C * 8 + Gc: 0, 2 * 64 + C * 8 + Tc: 1, 4 * 64 + Tc * 8 + A: 1, 3 * 64 + Gc * 8 + Tc: 2,
        7 * 64 + Gc * 8 + N: 2, 9 * 64 + A * 8 + C: 3}
    with pytest.raises(ValueError):
        G.thread_reference("ACGT", G.Reads("ACGT", [(2, "3M", "GTA")]))


@pytest.mark.parametrize("seed", [1, 3, 7, 13])
def test_thread_reference_equals_the_restatement_of_the_parity_tests(seed, tmp_path):
    """count, first and pools against the loop of test_gpu_parity.test_thread_kernels_class_tables, restated here."""
    import py_ingest_mirror as mirror
    from rambl_amd import cli
    args = T.make_case(seed, str(tmp_path))
    seen = 0
    for window, reads in cli.load_regions(cli.parse_cmd_line(args)):
        if len(reads) == 0:
            continue
        ref = G.thread_reference(reads.gene_seq, reads)
        code = {ch: k for k, ch in enumerate(ref["sym"]) if ch}
        glen = len(reads.gene_seq)
        exp = {}
        for rid in range(len(reads)):
            i, j = reads.pos[rid], 0
            for op, ln in mirror.parse_cigar(reads.cigar[rid]):
                if op == "M":
                    for t in range(ln):
                        exp.setdefault((i + t) * 8 + code[ord(reads.seq[rid][j + t])], []).append(rid)
                    i += ln
                    j += ln
                elif op == "I":
                    j += ln
                elif op == "D":
                    i += ln
        assert len(ref["count"]) == glen * 8
        off = 0
        for cls in range(glen * 8):
            members = exp.get(cls, [])
            assert ref["count"][cls] == len(members) and ref["off"][cls] == off
            assert ref["pool"][off:off + len(members)] == members
            assert ref["first"][cls] == (members[0] if members else G.INT_MAX)
            off += len(members)
        assert off == len(ref["pool"])
        seen += 1
    assert seen


@pytest.mark.parametrize("name", sorted(G.PARITY_CASES))
def test_parity_case_is_a_region_the_oracle_accepts(name, tmp_path, oracle_bin):
    """The ACGT cases as FASTA + SAM: the product's ingest keeps every read as the case states it (positions relative to the
    window, = and X as M), and the oracle prints a graph for the region."""
    from rambl_amd import cli
    case = G.THREAD_CASES[name]()
    args = G.sam_dataset(case, str(tmp_path))
    (window, reads), = cli.load_regions(cli.parse_cmd_line(args))
    r = case.reads
    w0 = window[1] - 1
    assert reads.gene_seq == r.gene_seq[w0:window[2]]
    assert list(reads.pos) == [p - w0 for p in r.pos] and list(reads.seq) == r.seq and list(reads.copies) == r.copies
    assert list(reads.cigar) == [c.replace("=", "M").replace("X", "M") for c in r.cigar]
    dump, _ = T.run_oracle(args, str(tmp_path), graph=True)
    edges = [ln for ln in dump.splitlines() if not ln.startswith("#")]
    assert len(edges) >= 1 and dump.startswith("#\t0\t0\t^\t0\n")


def _recorded_msa():
    cases = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "msa_vectors.json.gz")).read())
    return {c["name"]: c for c in cases if "name" in c}


@pytest.mark.parametrize("name", sorted(G.MSA_CASES))
def test_msa_case_reaches_its_edge_and_the_oracle_equals_the_reference(name, oracle_bin):
    case = G.MSA_CASES[name]()
    assert case.name == name and case.key() == G.MSA_CASES[name]().key()
    rec = _recorded_msa()[name]
    assert rec["seqs"] == case.seqs and len(rec["rows"][0]) == rec["ncol"]
    rows = T.oracle_msa(case.seqs)
    case.check(rows)
    assert rows == rec["rows"]


def test_msa_vectors_hold_inputs_and_rows_only():
    cases = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "msa_vectors.json.gz")).read())
    assert sorted(c["name"] for c in cases if "name" in c) == sorted(G.MSA_CASES)
    for c in cases:
        assert set(c) <= {"seqs", "rows", "ncol", "name"}
        assert all(isinstance(s, str) for s in c["seqs"] + c["rows"]) and isinstance(c["ncol"], int)


@pytest.mark.parametrize("name", sorted(G.EDGE_CASES))
def test_edge_case_reaches_its_edge(name):
    case = G.EDGE_CASES[name]()
    assert case.name == name and case.key() == G.EDGE_CASES[name]().key()
    n_nodes = len(case.node_is_end)
    assert case.pool_ptr[0] == 0 and case.pool_ptr[-1] == len(case.pool_rid) == len(case.pool_cn)
    assert len(case.edge_src) == len(case.edge_dst) >= 1 and len(case.pool(0)) == 0
    assert ((0 <= case.edge_src) & (case.edge_src < n_nodes) & (0 <= case.edge_dst) & (case.edge_dst < n_nodes)).all()
    assert (case.pool_cn >= 1).all() and (case.pool_rid >= 0).all()
    assert set(case.flags) <= {0, 1} and (1 not in case.flags or case.pools_sorted())   # sorted = 1 only promises what holds
    case.check(case.reference())


def oracle_graph_and_pools(args, d):
    """The oracle's -G text and, through SC_ORACLE_DUMP_POOLS, the read pool of every node: one (nodes, pools) per region"""
    path = os.path.join(d, "pools.txt")
    env = dict(os.environ, PATH=T.TOOLS + os.pathsep + os.environ.get("PATH", ""), TMPDIR=d, SC_ORACLE_DUMP_POOLS=path)
    p = subprocess.run([T.ORACLE, "-G"] + list(args), cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    graphs = []
    for ln in open(path).read().splitlines():
        f = ln.split("\t")
        if f[0] == "graph":
            graphs.append([])
        else:
            assert int(f[0]) == len(graphs[-1])
            graphs[-1].append([tuple(int(x) for x in e.split(":")) for e in f[1].split()])
    return p.stdout.decode(), graphs


@pytest.mark.parametrize("seed", [1, 7, 9, 15])
def test_edge_support_reference_equals_the_oracle(seed, tmp_path, oracle_bin):
    """The seeds of test_gpu_parity.test_edge_support_kernel: CSR arrays from the oracle's own pools, supports from its -G text."""
    args = T.make_case(seed, str(tmp_path))
    dump, graphs = oracle_graph_and_pools(args, str(tmp_path))
    lines = dump.splitlines()
    at, n_edges = 0, 0
    for pools in graphs:
        nodes = [ln.split("\t") for ln in lines[at:at + len(pools)]]
        assert all(f[0] == "#" and int(f[1]) == k for k, f in enumerate(nodes))
        assert [int(f[4]) for f in nodes] == [sum(cn for _, cn in p) for p in pools]
        at += len(pools)
        edges = []
        while at < len(lines) and not lines[at].startswith("#"):
            edges.append(tuple(int(x) for x in lines[at].split("\t")))
            at += 1
        ptr = [0]
        for p in pools:
            ptr.append(ptr[-1] + len(p))
        sup = G.edge_support_reference(ptr, [r for p in pools for r, _ in p], [c for p in pools for _, c in p],
                                       [f[3] == "$" for f in nodes], [e[0] for e in edges], [e[1] for e in edges])
        assert sup == [e[2] for e in edges]
        n_edges += len(edges)
    assert at == len(lines) and n_edges > 50


def test_restated_geometry_matches_the_source():
    src = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_graph_kernels.hip")).read()
    assert "constexpr int SORT_WORDS = %d;" % G.SORT_WORDS in src and "constexpr int BIG_WORDS = %d;" % G.BIG_WORDS in src
    assert "constexpr int MSA_CM = %d;" % G.MSA_CM in src and "if (hi - lo < WORDS * 32)" in src
    assert "if (d.cmax > MSA_CM || d.mv_stride > 64)" in src and "for (int chunk = 0; chunk * 64 < nn; chunk++)" in src
    assert src.count("if (blocks > %d) blocks = %d;" % (G.GRID_BLOCKS, G.GRID_BLOCKS)) == 2 and "int waves_per_block = %d;" % G.GRID_WAVES in src
    assert "int blocks = (d.n_reads + 3) / 4;" in src and "if (sblocks > %d) sblocks = %d;" % (G.GRID_BLOCKS, G.GRID_BLOCKS) in src
    assert "k_thread_scan, dim3(1), dim3(%d)" % G.SCAN_THREADS in src and "const int per = (n + 1023) / 1024;" in src
    assert "k_thread_sort_big, dim3(%d), dim3(1024)" % G.BIG_BLOCKS in src and "if (d.n_reads > SORT_WORDS * 32)" in src
    assert "return w < %d ? %d :" % (G.CHILD_BIG_WORDS, G.CHILD_BIG_WORDS) in src
    hdr = open(os.path.join(ROOT, "include", "straincall_hip.h")).read()
    assert "#define SC_ERR_UNSUPPORTED (%d)" % G.SC_ERR_UNSUPPORTED in hdr
    region = open(os.path.join(ROOT, "rambl_amd", "csrc", "sc_region.cpp")).read()
    assert "const int cmax = (int)packed.size() + 1;" in region and "d.mv_stride = (int)((longest + 1 + 63) / 64) * 64;" in region
