"""The commit section of the urn chain (rambl_amd/csrc/sc_sampler.hpp, urn_chain_q): an accepted draw adds one to its
strain's count in LDS and writes its strain as one byte to the region's draw log; the draws per (strain, read symbol)
are counted from that log after the chain (draw_log_counts).  One sampler level through the production kernel
(capi.Context.sample_level) against the oracle's draw loop, `kdraw` and `cnt` compared exactly, on the smallest shapes
at which the log, its indices or the count over it can go wrong: every draw of a wavefront on one strain, windows of
128 and of 64 draws, Q = 1 .. 129 (rows wrapped many times per window; Q no multiple of the window), totals of 1 ..
1 143 draws (below, at and above a window; across the refill of the staged uniforms), a slot without a single symbol,
a flagged slot, weight rows in LDS and in memory, a level run twice, and a region on resident level workers.

What these tests do not do through sample_level: the entry refuses a context with resident level workers
(tests/test_sampler_tiers.py pins that), so the workgroups that keep their idle wavefronts (urn_chain_shadow) are
reached by whole regions on a two-slot context instead, FASTA and per-level trace against the oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402
import test_sampler_tiers as ST  # noqa: E402

pytestmark = pytest.mark.gpu

KMAX = ST.KMAX
NO_SYMBOL = 0xFF                        # JobDev::qcode of a label that is no single symbol

# (Q, n_sweeps): totals 1, 127, 128, 129, 1025 with Q = 1; the same totals reached with Q = 3, 127, 129; and totals
# beyond 1024 (the staged uniforms are refilled from draw 512 on) with rows that wrap inside every window
SHAPES = [(1, 1), (1, 127), (1, 128), (1, 129), (1, 1025), (3, 43), (127, 1), (129, 1), (3, 342), (127, 9), (129, 8)]


@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    c = capi.Context(0, 1)
    yield c
    c.close()


def one_sided_level(Q, n_extra=8):
    """S = 2 and every read far on the side of strain 0: all draws of a pass commit to one count."""
    n_reads = Q + n_extra
    ll = np.empty((2, n_reads))
    ll[0, :] = -0.5
    ll[1, :] = -30.0
    return ST.Level([5000.0, 1.0], ll, np.ones(n_reads, dtype=np.uint8), list(range(Q)), [1] * Q,
                    [q % 5 for q in range(Q)], [], e0=7)


def test_every_draw_of_a_pass_on_one_strain(ctx):
    rng = np.random.default_rng(2)
    for Q, n in SHAPES:
        lv = one_sided_level(Q)
        U = rng.random(n * Q) * 0.9                        # (strain 1 holds < 1e-15 of the weight)
        r, choice = ST.check(ctx, lv, U, n, "S=2 one-sided Q=%d n=%d" % (Q, n))
        assert not choice.any() and r["kdraw"][0] == n * Q
        assert r["kind"] % 2 == 0                          # weight rows in LDS
        # The only boundary lies (1 - u) * T >= 500 above every target and moves down by at most u < 1 per earlier draw
        # (127 of them): every pass accepts its whole window, 16 draws per wavefront, all on one count
        assert r["n_pass"] == -(-n * Q // ST.window_of(2)), (Q, n, r["n_pass"])


@pytest.mark.parametrize("S", [17, 33, 128])
def test_windows_shapes_and_totals(ctx, S):
    """S = 17: eight wavefronts, S = 33 and 128: four; every (Q, n_sweeps) of SHAPES."""
    rng = np.random.default_rng(100 + S)
    for Q, n in SHAPES:
        lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=0.9, spread=2.0, e0=int(rng.integers(1, 30)))
        assert lv.Q == Q
        r, _ = ST.check(ctx, lv, rng.random(n * Q), n, "S=%d Q=%d n=%d" % (S, Q, n))
        assert r["kind"] % 2 == 0


@pytest.mark.parametrize("S", [5, 70])
def test_slot_without_symbol_and_flagged_slot(ctx, S):
    """Slot 2 has no single symbol: drawn, counted per strain, not per (strain, symbol).  Slot 4 is flagged (a NaN weight
    row): its draws come from the checked tiers on wavefront 0 and are logged and counted like the others."""
    rng = np.random.default_rng(500 + S)
    Q, n = 7, 40
    lv = ST.make_level(rng, S, Q, cn_max=1, has_frac=1.0, spread=2.0)
    lv.ll[:, 4] = -2000.0 - rng.random(S)
    lv = ST.Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    U = rng.random(n * Q)
    choice, kdraw, _ = ST.oracle_draws(lv, n, U)           # the draws do not depend on the symbols
    sym = np.array(lv.ent_sym, dtype=np.int32)
    sym[2] = NO_SYMBOL
    cnt = np.zeros((S, KMAX), dtype=np.int64)
    for t, c in enumerate(choice):
        if sym[t % Q] < KMAX:
            cnt[c, sym[t % Q]] += 1
    assert cnt.sum() == n * (Q - 1)
    r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, sym, lv.mates, n, U, e0=lv.e0)
    assert r["n_draws"] == n * Q and r["n_exact"] >= n
    assert np.array_equal(r["kdraw"].astype(np.int64), kdraw)
    assert np.array_equal(r["cnt"].astype(np.int64), cnt)


@pytest.mark.parametrize("S", [2, 33])
def test_rows_in_memory(ctx, S):
    """More draw slots than the weight rows have room for in LDS: the kernel variant that reads them from memory, whose
    vector-memory loads share a counter with the draw log's stores."""
    rng = np.random.default_rng(700 + S)
    stride = (S + 1 + 3) & ~3
    stride = stride if stride & 4 else stride + 4
    Q = 141056 // (4 * stride) + 9
    if S == 2:
        lv, n = one_sided_level(Q), 1
        U = rng.random(n * Q) * 0.9
    else:
        lv, n = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.2, has_frac=0.9, spread=2.0), 2
        U = rng.random(n * Q)
    r, _ = ST.check(ctx, lv, U, n, "S=%d Q=%d rows in memory" % (S, Q))
    assert r["kind"] % 2 == 1


def test_same_level_twice_with_other_uniforms(ctx):
    """The log is rewritten by every level: a second run with other uniforms, and a shorter third one, count their own
    draws.  (The test entry builds a private worker per call, so the three runs share a log only where the allocator
    hands the same block back; the log that really is rewritten level after level is the region's, below.)"""
    rng = np.random.default_rng(9)
    lv = ST.make_level(rng, 17, 50, cn_max=2, mate_frac=0.3, spread=0.5)
    seen = []
    for n in (20, 20, 3):
        U = rng.random(n * lv.Q)
        r, choice = ST.check(ctx, lv, U, n, "run %d" % len(seen))
        seen.append(r["cnt"].copy())
    assert not np.array_equal(seen[0], seen[1])


def test_region_on_resident_workers_with_two_slots(tmp_path, oracle_bin):
    """Resident level workers keep the wavefronts that do not run the chain (urn_chain_shadow) at its barriers, and the
    whole workgroup counts the log; a region rewrites one log level after level.  The region twice in flight on a two-slot
    context: FASTA and trace of both.  The counts per (strain, symbol) show here only through what they feed: a level's
    counts enter the strains' substitution models, which set the log-likelihoods and so the abundances of every later
    level, compared to 1e-9 in the trace.  (The entry that returns `cnt` itself refuses this kind of context.)"""
    from rambl_amd import capi, cli
    d = str(tmp_path)
    args = T.make_case(1, d)
    exp_fa, exp_tr = T.run_oracle(args, d, trace=True)
    pa = cli.parse_cmd_line(list(args))
    regions = [(w, r) for w, r in cli.load_regions(pa) if len(r)]
    params = capi.default_params(float(pa.error_rate), float(pa.tau), float(pa.diff_rate), want_trace=True)
    with capi.Context(0, 2) as c2:
        hs = [[(w, c2.submit(r, params)) for w, r in regions] for _ in range(2)]
        for handles in hs:
            res = [(w, c2.wait(h, want_trace=True)) for w, h in handles]
            assert "".join(cli.format_fasta(w, x, pa.tau) for w, x in res) == exp_fa
            T.compare_traces("".join(x.trace for _, x in res), exp_tr)
            assert sum(x.stats["draws"] for _, x in res) > 0
