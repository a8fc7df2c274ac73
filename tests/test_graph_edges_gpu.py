"""-m gpu: the graph-stage kernels (rambl_amd/csrc/sc_graph_kernels.hip) on the named edge cases of tests/graph_edge_lib.py.
Every comparison is exact: the six threading tables against thread_reference, the MSA rows against the oracle and the rows
recorded from the reference, the edge supports against edge_support_reference.  The property check of a case runs first, so
that a case that has lost its edge fails here too."""
import functools
import os
import subprocess
import sys

import pytest

import graph_edge_lib as G
import sc_testlib as T

pytestmark = pytest.mark.gpu

# the stretch of k_thread_sort_big in this process: the default, or what the parent of a child run set
BIG_WORDS = min(max(int(os.environ.get("SC_SORT_BIG_WORDS", G.BIG_WORDS)), 64), G.BIG_WORDS)


@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    with capi.Context(0, 1) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _thread_case(name):
    case = G.THREAD_CASES[name]()
    try:
        ref = case.reference()
    except ValueError:
        ref = None
    return case, ref


@pytest.mark.parametrize("name", sorted(G.THREAD_CASES))
def test_threading_tables(name, ctx):
    """count, first, pools, smin, emin, tmin and the symbol table of every threading and wide-sort case."""
    from rambl_amd import capi
    case, ref = _thread_case(name)
    case.check(ref, BIG_WORDS)
    params = capi.default_params(graph_only=True)
    h = ctx.submit(case.reads, params)
    if case.error is not None:
        with pytest.raises(capi.StrainCallError) as e:
            ctx.wait(h)
        assert e.value.code == case.error
        return
    ctx.wait(h, release=False)
    cnt, first, pool, sym = ctx.thread_tables(h)
    smin, emin, tmin = ctx.thread_edges(h)
    ctx.lib.sc_roi_release(ctx.h, h)
    assert sym == ref["sym"]
    assert cnt == ref["count"]
    assert first == ref["first"]
    assert pool == ref["pool"]
    assert smin == ref["smin"]
    assert emin == ref["emin"]
    assert tmin == ref["tmin"]


def test_wide_sort_cases_with_short_stretches():
    """The wide-sort cases again in a child process with SC_SORT_BIG_WORDS=64 (2 048 ids per stretch: nine or ten stretches
    per wide class); the property checks of the child count the stretches for that value."""
    env = dict(os.environ, SC_SORT_BIG_WORDS=str(G.CHILD_BIG_WORDS))
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "%s::test_threading_tables" % os.path.abspath(__file__),
                        "-k", " or ".join(G.WIDE_CASES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert "%d passed" % len(G.WIDE_CASES) in out, out[-3000:]


@pytest.mark.parametrize("name", sorted(G.PARITY_CASES))
def test_threading_case_graph_dump_equals_the_oracle(name, tmp_path, oracle_bin):
    """The ACGT cases as FASTA + SAM through the product's -G dump against the oracle's."""
    args = G.sam_dataset(G.THREAD_CASES[name](), str(tmp_path))
    exp, _ = T.run_oracle(args, str(tmp_path), graph=True)
    assert T.run_product(args, graph=True) == exp


@functools.lru_cache(maxsize=None)
def _recorded_msa():
    import gzip
    import json
    cases = json.loads(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msa_vectors.json.gz")).read())
    return {c["name"]: c for c in cases if "name" in c}


@pytest.mark.parametrize("name", sorted(G.MSA_CASES))
def test_msa_rows(name, ctx, oracle_bin):
    case = G.MSA_CASES[name]()
    exp = T.oracle_msa(case.seqs)
    case.check(exp)
    got = ctx.msa_align(case.seqs)
    assert got == exp
    rec = _recorded_msa()[name]
    assert rec["seqs"] == case.seqs and got == rec["rows"] and len(got[0]) == rec["ncol"]


@pytest.mark.parametrize("name", sorted(G.EDGE_CASES))
def test_edge_supports(name, ctx):
    case = G.EDGE_CASES[name]()
    exp = case.reference()
    case.check(exp)
    for flag in case.flags:
        assert ctx.edge_support_tables(*case.arrays(), flag) == exp, "sorted = %d" % flag


def test_edge_support_entry_checks_its_arguments(ctx):
    from rambl_amd import capi
    case = G.EDGE_CASES["unsorted"]()
    with pytest.raises(capi.StrainCallError) as e:                   # shuffled pools under sorted = 1: refused, not searched
        ctx.edge_support_tables(*case.arrays(), 1)
    assert e.value.code == -3
    ptr, rid, cn, end, src, dst = G.EDGE_CASES["source_and_end"]().arrays()
    with pytest.raises(capi.StrainCallError) as e:
        ctx.edge_support_tables(ptr, rid, cn, end, src, dst + 5, 1)      # an edge to a node that does not exist
    assert e.value.code == -3
