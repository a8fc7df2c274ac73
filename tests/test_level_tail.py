"""The count over the draw log behind the urn chain (rambl_amd/csrc/sc_sampler.hpp, draw_log_counts): a lane takes one
draw slot and a stretch of at most STRETCH of its sweeps, issues every load of the stretch (three blocks of BLOCK loads,
blocks that no stretch of the level reaches skipped) and the slot's symbol beside them, and only then counts.  One sampler
level through the production kernel (capi.Context.sample_level), `kdraw` and `cnt` compared exactly against the oracle's
draw loop, on the smallest shapes at which the item arithmetic can go wrong and which tests/test_chain_commit.py does not
reach (it stops at Q = 129 with many sweeps, and at large Q with n <= 2): Q around and above both thread counts with
columns longer than one block and longer than one stretch.

* Threads that count: S = 3 and 17 run the chain on eight wavefronts (512 threads count), S = 33 on four (256).
* Q = 255, 256, 257, 511, 513 (around the thread counts, off every alignment) and 861 (odd, above both); Q = 100 for
  stretches that exist only to fill the lanes, the last of which lie behind the last sweep.
* n = 1, around BLOCK and 2 * BLOCK (7, 8, 9, 16, 17), around STRETCH (23, 24, 25), 46 and 47 (two stretches of 23 and of
  24), 48 and 49 (two stretches of 24; three of 17, 17 and 15).
* (861, 47, 33), which the issue names, cannot run: 40 467 draws are more than the 40 000 (MAX_DRAWS, the reference's draw
  budget) that the entry accepts and tests/test_sampler_tiers.py pins; a level of 861 slots has 46 sweeps in production
  too.  (861, 46, 33) and (513, 47, 33) stand for it.
* Every level has slots without a single symbol (0xFF) at q = 0, 1, 2, 3 and Q - 1: drawn, counted per strain, not per
  (strain, symbol).  A lane takes one slot, so there is no first or last slot of a lane's share beyond these.
* The entry sizes the draw log for exactly n * Q draws (sc_sample_level: job_dev(..., Q * n_sweeps)), so in EVERY case
  here the last load of the last stretch is the last byte of the log's capacity.
* The log must hold runs that end: no strain takes more than 70 % of a level's draws (asserted from the oracle's draws).

The resident path (every wavefront stays and counts, k_level_resident) cannot go through sample_level, which refuses
such a context: one small region twice in flight on a two-slot context, FASTA and trace against the oracle."""
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
STRETCH = 24                            # sc_sampler.hpp: LOG_STRETCH, sweeps a lane loads before it counts
BLOCK = 8                               # loads per block of a stretch

# (Q, n_sweeps, S): every Q, every n and every S at least once
CASES = [
    (255, 25, 3), (255, 7, 17), (255, 46, 33),
    (256, 24, 17), (256, 17, 33), (256, 1, 3),
    (257, 23, 33), (257, 16, 3), (257, 49, 17),
    (511, 9, 17), (511, 46, 3), (511, 25, 33),
    (513, 8, 3), (513, 47, 33), (513, 48, 17),
    (861, 1, 3), (861, 24, 3), (861, 25, 17), (861, 46, 33),
    (100, 7, 3), (100, 47, 33),
]
assert {c[1] for c in CASES} >= {1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, STRETCH - 1, STRETCH, STRETCH + 1, 46, 47}
assert all(q * n <= ST.MAX_DRAWS for q, n, _ in CASES)


@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    c = capi.Context(0, 1)
    yield c
    c.close()


def threads_counting(S):
    return 64 * (8 if ST.nb_of(S) <= 2 else 4)


def stretches(Q, n, S):
    """(G, per) as draw_log_counts forms them."""
    G = max(-(-n // STRETCH), min(threads_counting(S) // Q, n))
    return G, -(-n // G)


def level_and_counts(seed, Q, n, S):
    """A level whose log holds runs that end, with symbol-less slots at both edges; the oracle's counts for it."""
    rng = np.random.default_rng(seed)
    # equal prior weights well above one draw and rows within a factor e^0.5: no strain runs away with the urn
    lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=0.9, spread=0.5, a0=np.full(S, 40.0),
                       e0=int(rng.integers(1, 30)))
    assert lv.Q == Q
    U = rng.random(n * Q)
    choice, kdraw, _ = ST.oracle_draws(lv, n, U)           # the draws do not depend on the symbols
    assert kdraw.max() <= 0.7 * n * Q, "one strain holds %.2f of the draws" % (kdraw.max() / (n * Q))
    sym = np.array(lv.ent_sym, dtype=np.int32)
    blank = sorted({0, 1, 2, 3, Q - 1})
    sym[blank] = NO_SYMBOL
    cnt = np.zeros((S, KMAX), dtype=np.int64)
    slot_sym = np.tile(sym, n)
    keep = slot_sym < KMAX
    np.add.at(cnt, (choice[keep], slot_sym[keep]), 1)
    assert cnt.sum() == n * (Q - len(blank))
    return lv, U, sym, kdraw, cnt


def run(ctx, lv, U, sym, n):
    return ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, sym, lv.mates, n, U, e0=lv.e0)


def compare(r, Q, n, S, kdraw, cnt):
    label = "Q=%d n=%d S=%d" % (Q, n, S)
    assert r["n_draws"] == n * Q, label
    assert ST.nb_of(S) == (r["kind"] + 1) // 2, label
    assert np.array_equal(r["kdraw"].astype(np.int64), kdraw), label + ": draws per strain differ"
    got = r["cnt"].astype(np.int64)
    assert np.array_equal(got, cnt), "%s: draws per (strain, symbol) differ at %s" % (label, np.argwhere(got != cnt)[:8].tolist())


@pytest.mark.parametrize("Q,n,S", CASES)
def test_counts_of_a_level(ctx, Q, n, S):
    G, per = stretches(Q, n, S)
    assert 1 <= per <= STRETCH and G * per >= n
    lv, U, sym, kdraw, cnt = level_and_counts(1000 * Q + 10 * n + S, Q, n, S)
    compare(run(ctx, lv, U, sym, n), Q, n, S, kdraw, cnt)


def test_the_shapes_reach_every_path_of_the_count():
    """What CASES is there for, stated on the stretch arithmetic itself (no GPU work)."""
    seen = {(stretches(Q, n, S), Q > threads_counting(S)) for Q, n, S in CASES}
    pers = {p for (_, p), _ in seen}
    assert {1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, STRETCH - 1, STRETCH} <= pers          # one, two and three blocks of loads
    assert any(G > 1 and wide for (G, _), wide in seen)                     # stretches although Q is above the thread count
    assert any(G > -(-n // STRETCH) for Q, n, S in CASES for G, _ in [stretches(Q, n, S)])      # stretches that only fill lanes
    assert any(G * per - n >= per for Q, n, S in CASES for G, per in [stretches(Q, n, S)])      # a stretch wholly behind the last sweep
    assert any(0 < G * per - n < per for Q, n, S in CASES for G, per in [stretches(Q, n, S)])   # a last stretch shorter than the others
    assert any(threads_counting(S) == 256 for _, _, S in CASES) and any(threads_counting(S) == 512 for _, _, S in CASES)


def test_a_long_level_then_a_shorter_one(ctx):
    """Nothing of the first log may be counted in the second: 46 sweeps of 861 slots, then 3 sweeps, then 25 of 257 slots on
    the same context.  (The entry builds a private worker per call: the runs share a log where the allocator hands the
    block back; the log that is rewritten level after level for certain is the region's, below.)"""
    for Q, n, S in ((861, 46, 33), (861, 3, 33), (257, 25, 33)):
        lv, U, sym, kdraw, cnt = level_and_counts(77 + n, Q, n, S)
        compare(run(ctx, lv, U, sym, n), Q, n, S, kdraw, cnt)


def test_region_twice_in_flight_on_resident_workers(tmp_path, oracle_bin):
    """k_level_resident: the wavefronts that do not run the chain stay (urn_chain_shadow) and all 512 threads count the
    log, whatever NB.  The counts per (strain, symbol) enter the strains' substitution models and so every later level's
    abundances, compared to 1e-9 in the trace."""
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
