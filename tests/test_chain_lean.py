"""The pass loop of the urn chain after its serial path was thinned (rambl_amd/csrc/sc_sampler.hpp, urn_chain_q): every
pass, the last one too, ends with the same commit and leaves the loop behind it; the loop exists twice, for levels with
at least a window of draw slots (Q >= 16 * NW: the row offset wraps with one compare) and for those with fewer (it
divides); wavefront 0 keeps one threshold `unext` for the refill of the staged uniforms (prefetch at ulo + 256, swap at
ulo + 512).  None of it changes which draws a pass accepts.

One sampler level through the production kernel (capi.Context.sample_level) against the oracle's draw loop
(oracle_urn_draws), `kdraw`, `cnt` and the number of draws compared exactly (test_sampler_tiers.check), on the shapes at
which these three can go wrong:

* both loops in every kernel variant: S = 2 .. 113 (NB = 1 .. 8), Q = 1, 3, 16 * NW - 1, 16 * NW, 16 * NW + 1, two and
  five sweeps;
* the last pass: totals of 1 and of a window less one, exactly one and one more, with urn weights ~1e6 (every pass
  accepts its whole window, so the last pass is the one that holds the remainder), totals of 256 and 512 (the last pass
  is the one in which t reaches the refill's prefetch and its swap), and a level whose last -- or first --
  draw lies 1e-9 * T from a boundary, so that the checked tier runs in the pass that leaves -- or enters -- the loop;
* the refill: 2 600 draws (each half of the staged window swapped twice), once with whole-window advances and once with
  uniforms on boundaries at the draws around every threshold, so that t passes each threshold in steps of one and the
  checked tier runs in the very passes that prefetch and swap;
* weight rows in memory (the <NB, false> variants), the last draw on a boundary;
* a region on resident level workers with two slots (urn_chain_shadow takes part in the chain's barriers, which are
  where they were): FASTA and trace against the oracle.

All 40 000-draw budgets are kept (the largest level here has 8 825 draws) and every crafted draw is checked to take the
intended side in the oracle before the device is asked."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402
import test_sampler_tiers as ST  # noqa: E402

pytestmark = pytest.mark.gpu

ON_BOUNDARY = 1e-9                       # relative to T: between the fp64 scan's margin (1e-10) and the window's (>= 4.8e-6)
# the draws around the thresholds of the refill (prefetch at 256 + 512 k, swap at 512 + 512 k)
REFILL_DRAWS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1279, 1280)


@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    c = capi.Context(0, 1)
    yield c
    c.close()


def heavy_level(rng, S, Q):
    """Urn weights ~1e6: a boundary moves by at most one per earlier draw against T ~ 1e5 * S and more, so a uniform 1e-2
    * T from every boundary is accepted anywhere in a window."""
    return ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=1.0, spread=2.0, a0=rng.random(S) * 1e6 + 1e6)


def on_boundary_run(lv, total, rng, at):
    """Clear uniforms (1e-2 * T from every boundary) but for the draws in `at`, which lie ON_BOUNDARY from one, on
    alternating sides.  Returns U; every crafted draw took its intended side in the oracle."""
    at = sorted(at)
    U, crafted, ch = ST.crafted_run(lv, total, rng, lambda t: (ON_BOUNDARY, 1 if at.index(t) % 2 else -1) if t in at else None)
    assert [t for t, _, _ in crafted] == at, ("no room for a crafted uniform", at, crafted)
    n = total // lv.Q
    choice, _, _ = ST.oracle_draws(lv, n, U)
    assert np.array_equal(choice, ch)
    for t, _, want in crafted:
        assert choice[t] == want, t
    return U


def windows(total, S):
    return -(-total // ST.window_of(S))


@pytest.mark.parametrize("S", [2, 17, 33, 49, 65, 81, 97, 113])
def test_both_loops_in_every_variant(ctx, S):
    """Q below, at and above the window of the variant, Q = 1 and 3 (the row offset wraps many times inside a window),
    two and five sweeps."""
    W = ST.window_of(S)
    assert W == (128 if S <= 32 else 64)
    rng = np.random.default_rng(4000 + S)
    for Q in (1, 3, W - 1, W, W + 1):
        lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=0.9, spread=2.0, e0=int(rng.integers(1, 30)))
        assert lv.Q == Q
        for n in (2, 5):
            r, _ = ST.check(ctx, lv, rng.random(n * Q), n, "S=%d Q=%d n=%d" % (S, Q, n))
            assert r["kind"] == 2 * ST.nb_of(S)              # this S's variant, weight rows in LDS


@pytest.mark.parametrize("S", [2, 33])
def test_last_pass_holds_the_remainder(ctx, S):
    """Totals of 1, W - 1, W and W + 1 draws with whole windows accepted: the last pass commits 1, W - 1, W and 1 draws.
    Totals of 256 and 512: t arrives at the prefetch threshold and at the swap threshold of the staged uniforms exactly in
    the last pass, which then prefetches (from the stream's padding) or swaps like any other pass.
    Each total as one slot drawn `total` times (the dividing loop) and as `total` slots drawn once (the wrapping loop from
    W slots on)."""
    W = ST.window_of(S)
    rng = np.random.default_rng(4100 + S)
    # (256 and 512: the last pass is also the one in which t reaches the refill's prefetch and its swap)
    for total in (1, W - 1, W, W + 1, 256, 512):
        for Q in sorted({1, total}):
            lv = heavy_level(rng, S, Q)
            n = total // Q
            U, _, ch = ST.crafted_run(lv, total, rng, lambda t: None)
            r, choice = ST.check(ctx, lv, U, n, "S=%d total=%d Q=%d" % (S, total, Q))
            assert np.array_equal(choice, ch)
            assert r["n_pass"] == windows(total, S) and r["n_slow"] == 0, (S, total, Q, r["n_pass"], r["n_slow"])


@pytest.mark.parametrize("S,Q,n", [(2, 7, 30), (2, 150, 2), (33, 7, 30), (33, 150, 2)])
@pytest.mark.parametrize("which", ["last", "first"])
def test_checked_tier_in_the_pass_that_leaves_or_enters(ctx, S, Q, n, which):
    """The last draw of the level on a boundary: the pass that commits it is the one that runs the fp64 scan, and it
    leaves the loop behind that commit.  The same for the first draw, in the pass that enters the loop."""
    rng = np.random.default_rng(4200 + S + Q)
    lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=1.0, spread=1.0, a0=rng.random(S) * 3.0 + 50.0)
    total = n * Q
    U = on_boundary_run(lv, total, rng, [total - 1 if which == "last" else 0])
    r, _ = ST.check(ctx, lv, U, n, "S=%d Q=%d %s draw on a boundary" % (S, Q, which))
    assert r["n_slow"] >= 1


@pytest.mark.parametrize("S", [2, 33])
def test_refill_with_whole_window_advances(ctx, S):
    """2 600 draws, every pass a whole window: t reaches the thresholds in steps of 128 / 64, the prefetch and the swap
    fall into full passes, each half of the staged uniforms is swapped twice."""
    rng = np.random.default_rng(4300 + S)
    lv = heavy_level(rng, S, 100)
    n = 26
    U, _, ch = ST.crafted_run(lv, n * lv.Q, rng, lambda t: None)
    r, choice = ST.check(ctx, lv, U, n, "S=%d refill, whole windows" % S)
    assert np.array_equal(choice, ch)
    assert r["n_pass"] == windows(n * lv.Q, S) and r["n_slow"] == 0


@pytest.mark.parametrize("S", [2, 33])
def test_refill_with_draws_on_boundaries_at_the_thresholds(ctx, S):
    """The draws at t = 255, 256, 257, ... 1 280 lie on boundaries: each goes through the checked tier in a pass that
    advances by one, so t passes every threshold of the refill in steps of one."""
    rng = np.random.default_rng(4400 + S)
    lv = ST.make_level(rng, S, 100, cn_max=1, mate_frac=0.3, has_frac=1.0, spread=1.0, a0=rng.random(S) * 3.0 + 50.0)
    n = 26
    U = on_boundary_run(lv, n * lv.Q, rng, REFILL_DRAWS)
    r, _ = ST.check(ctx, lv, U, n, "S=%d refill, boundaries at the thresholds" % S)
    assert r["n_slow"] >= len(REFILL_DRAWS)


@pytest.mark.parametrize("S", [2, 33])
def test_rows_in_memory_last_draw_on_a_boundary(ctx, S):
    """More draw slots than the weight rows have room for in LDS (the <NB, false> variants, whose row loads the last
    pass issues like any other), the level's last draw on a boundary."""
    rng = np.random.default_rng(4500 + S)
    stride = (S + 1 + 3) & ~3
    stride = stride if stride & 4 else stride + 4
    Q = 141056 // (4 * stride) + 9
    n = 1 if S == 2 else 2
    assert n * Q <= ST.MAX_DRAWS
    lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.2, has_frac=0.9, spread=1.0, a0=rng.random(S) * 3.0 + 50.0)
    # a plain run, then the same level with its last draw on a boundary
    r, _ = ST.check(ctx, lv, rng.random(n * Q), n, "S=%d Q=%d rows in memory" % (S, Q))
    assert r["kind"] == 2 * ST.nb_of(S) - 1          # this S's variant, weight rows in memory
    # (only the last sweep is replayed in long double: the draws in front of it come from the oracle)
    U = rng.random(n * Q)
    choice, kdraw, _ = ST.oracle_draws(lv, n, U)
    w = ST.Walk(lv)
    w.a = w.a + np.bincount(choice[:-1], minlength=S).astype(ST.LD)
    c = ST.craft(w.cp((n * Q - 1) % Q), ON_BOUNDARY, -1, rng)
    assert c is not None
    U[-1] = c[0]
    choice, _, _ = ST.oracle_draws(lv, n, U)
    assert choice[-1] == c[1]
    r, _ = ST.check(ctx, lv, U, n, "S=%d Q=%d rows in memory, last draw on a boundary" % (S, Q))
    assert r["kind"] == 2 * ST.nb_of(S) - 1 and r["n_slow"] >= 1


def test_region_on_resident_workers_with_two_slots(tmp_path, oracle_bin):
    """Resident level workers keep the wavefronts that do not run the chain at its barriers (urn_chain_shadow), which
    is untouched: the chain still meets it at one barrier behind the staged uniforms, two per pass but one in the last,
    and one behind the loop.  A region twice in flight on a two-slot context, FASTA and trace of both."""
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
