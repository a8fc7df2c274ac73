"""The second barrier of a pass of the urn chain waits for the pass's commit and not for the reads issued behind it
(rambl_amd/csrc/sc_sampler.hpp, urn_chain_q: the atomic on s_kf goes first, the window's bookkeeping and the reads of the
next window follow it, lds_barrier_keep<N> leaves the N youngest of them in flight), and every scalar the loop reads is
pinned in front of it.  None of it changes which draws a pass accepts.

One sampler level through the production kernel (capi.Context.sample_level) against the oracle's draw loop
(oracle_urn_draws), `kdraw`, `cnt` and the number of draws compared exactly (test_sampler_tiers.check), on the shapes at
which a commit not yet visible behind the second barrier, or a miscounted wait, would change a draw:

* a light urn (a0 0.5 .. 3: after a few sweeps the counts are most of T, and one pass of commits that the next pass does
  not see moves the boundaries by whole windows), one strain with weights near 1 and the others 1e-3 .. 1, so that the
  accepted draws of a wavefront mostly add to one s_kf address, the slowest atomic there is; S = 2 .. 113 (NB = 1 .. 8),
  Q = window + 1 (the wrapping loop) and Q = 3 (the dividing loop), about 2 600 draws (each half of the staged uniforms
  swapped twice);
* a heavy urn (a0 ~ 1e6): every pass commits its whole window on every wavefront, 2 600 draws, the number of passes
  asserted;
* the refill's LDS writes between the atomic and the row reads: draws on boundaries at every threshold of the refill,
  so that t passes each in steps of one;
* weight rows in memory (the <NB, false> variants: the read of the uniform is the only LDS operation behind the commit)
  at NB = 1, 2 and 3, the last draw on a boundary;
* a region on resident level workers with two slots (k_level_resident, urn_chain_shadow at the same barriers): FASTA and
  trace against the oracle.

Such a test is a net: a read that goes stale behind a barrier is a matter of timing.  The argument itself stands where
lds_barrier_keep is called.  Every level stays below 10 000 draws; every crafted draw is checked to take its intended
side in the oracle before the device is asked."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402
import test_chain_lean as CL  # noqa: E402
import test_sampler_tiers as ST  # noqa: E402

pytestmark = pytest.mark.gpu

DRAWS = 2600                             # past 2 * 1024 + 512: each half of the staged uniforms is swapped in twice
ROWS_LDS_BYTES = 141056                  # what a level's weight rows may take in LDS (test_chain_lean)


@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    c = capi.Context(0, 1)
    yield c
    c.close()


def light_level(rng, S, Q):
    """Urn weights 0.5 .. 3 and no mates; strain `hot` has the largest weight for every read of the level (its row is
    within 0.01 of the best log-likelihood there is), the others lie 1e-3 .. 1 below it."""
    lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.0, has_frac=1.0, spread=6.9, a0=rng.random(S) * 2.5 + 0.5)
    assert lv.Q == Q
    hot = int(rng.integers(S))
    lv.ll[hot, :Q] = -0.5 + rng.random(Q) * 0.01
    return lv


def sweeps(Q):
    return -(-DRAWS // Q)


def light_case(S, Q):
    rng = np.random.default_rng(5000 + 7 * S + Q)
    lv = light_level(rng, S, Q)
    n = sweeps(Q)
    return lv, rng.random(n * Q), n


def heavy_case(S):
    rng = np.random.default_rng(5100 + S)
    lv = CL.heavy_level(rng, S, 100)
    n = sweeps(lv.Q)
    U, _, ch = ST.crafted_run(lv, n * lv.Q, rng, lambda t: None)
    return lv, U, n, ch


def refill_case(S):
    rng = np.random.default_rng(5200 + S)
    lv = light_level(rng, S, 100)
    n = sweeps(lv.Q)
    return lv, CL.on_boundary_run(lv, n * lv.Q, rng, CL.REFILL_DRAWS), n


def rows_in_memory_case(S):
    """More draw slots than the weight rows have room for in LDS; the last draw lies on a boundary (only that draw is
    replayed in long double: the counts in front of it come from the oracle)."""
    rng = np.random.default_rng(5300 + S)
    stride = (S + 1 + 3) & ~3
    stride = stride if stride & 4 else stride + 4
    Q = ROWS_LDS_BYTES // (4 * stride) + 9
    n = 1 if Q > 5000 else 2
    lv = light_level(rng, S, Q)
    U = rng.random(n * Q)
    choice, _, _ = ST.oracle_draws(lv, n, U)
    w = ST.Walk(lv)
    w.a = w.a + np.bincount(choice[:-1], minlength=S).astype(ST.LD)
    c = ST.craft(w.cp((n * Q - 1) % Q), CL.ON_BOUNDARY, -1, rng)
    assert c is not None
    U[-1] = c[0]
    choice, _, _ = ST.oracle_draws(lv, n, U)
    assert choice[-1] == c[1]
    return lv, U, n


@pytest.mark.parametrize("S", [2, 17, 33, 49, 65, 81, 97, 113])
def test_light_urn_in_every_variant(ctx, S):
    """The counts soon outweigh the urn's own weights and most commits of a wavefront fall on one address: a pass that
    read s_kf before every wavefront's commits of the pass before had landed would place its boundaries elsewhere."""
    for Q in (ST.window_of(S) + 1, 3):
        lv, U, n = light_case(S, Q)
        assert DRAWS <= n * Q < 10000
        r, choice = ST.check(ctx, lv, U, n, "light urn S=%d Q=%d n=%d" % (S, Q, n))
        assert r["kind"] == 2 * ST.nb_of(S)                  # this S's variant, weight rows in LDS
        # (the level is what it is meant to be: the oracle gives one strain more than half of the draws)
        assert 2 * np.bincount(choice, minlength=S).max() > n * Q


@pytest.mark.parametrize("S", [2, 33])
def test_heavy_urn_commits_whole_windows(ctx, S):
    """Every pass accepts its whole window on every wavefront: each of them commits 16 draws per pass, and the next pass
    needs all of them."""
    lv, U, n, ch = heavy_case(S)
    r, choice = ST.check(ctx, lv, U, n, "heavy urn S=%d" % S)
    assert np.array_equal(choice, ch)
    assert r["n_pass"] == CL.windows(n * lv.Q, S) and r["n_slow"] == 0, (S, r["n_pass"], r["n_slow"])


@pytest.mark.parametrize("S", [2, 33])
def test_refill_writes_between_the_commit_and_the_row_reads(ctx, S):
    """The draws at t = 255, 256, 257, ... 1 280 lie on boundaries: each goes through the checked tier in a pass that
    advances by one, so wavefront 0 prefetches and swaps the staged uniforms -- its LDS writes sit between its commit and
    its row reads -- in passes of one draw, whose commit the very next pass needs."""
    lv, U, n = refill_case(S)
    r, _ = ST.check(ctx, lv, U, n, "S=%d refill, boundaries at the thresholds" % S)
    assert r["n_slow"] >= len(CL.REFILL_DRAWS)


@pytest.mark.parametrize("S", [2, 17, 33])
def test_rows_in_memory(ctx, S):
    lv, U, n = rows_in_memory_case(S)
    assert n * lv.Q < 10000
    r, _ = ST.check(ctx, lv, U, n, "S=%d Q=%d rows in memory, last draw on a boundary" % (S, lv.Q))
    assert r["kind"] == 2 * ST.nb_of(S) - 1 and r["n_slow"] >= 1          # this S's variant, weight rows in memory


def test_region_on_resident_workers_with_two_slots(tmp_path, oracle_bin):
    """Resident level workers: the variants as functions of k_level_resident, the wavefronts that do not run the chain
    at its barriers (urn_chain_shadow, which reads the advance between them as before).  A region twice in flight on a
    two-slot context, FASTA and trace of both."""
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
