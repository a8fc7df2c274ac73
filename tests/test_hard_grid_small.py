"""A lone region's hard update (hard_clustering) on the grid at ordinary sizes: launch_level_grid sends a MODE_HARD level
with an update, no duplicates and no multi-symbol label to k_hard_mates / k_hard_resp / k_hard_sums once the level goes
wide, behind the grid's update and k_level_entries; the level's own kernel then only stages and stamps (LV_HARD_DONE).
The kernels take the strains' rows, symbols and log priors as kernel arguments and the slot's read id from qrid.

Whole small regions as a lone region, in child processes (SC_WIDE_MIN is read once per process): with SC_WIDE_MIN=0
every level that can go wide does, with a huge value none.  FASTA and per-level trace of both runs against the oracle's
and against each other (%.17g traces byte-identical: the grid runs the same functions in the same order), and the level
log's `done` column shows which path ran.

The cases, found in the level logs of sc_testlib.make_case(1..8) walked with SC_WIDE_MIN=0 (mode 0 = hard update):
* seed 2 (paired reads, one strain): 17 hard levels, all S = 1 with Q = 24 .. 51 (below 64: one partial wavefront of
  k_hard_resp); 11 on the grid, 6 with a multi-symbol label stay in their workgroup.  Its reads are pairs, and level 1 (the
  first on the grid) comes before any later read has been entered: the mates of its slots are seen for the first time
  there, which is what k_hard_mates (zero_unseen_mates) is for.
* seed 5 (insertions): S = 1 .. 5, among them S = 2 at Q = 16, and 32 multi-symbol levels between the grid ones.
* seed 7 (300-600 noisy reads, up to ten candidates): Q up to 436, among them 257 (one slot into the second workgroup of
  k_hard_resp), 277, 287, 291, 310, 318; S = 1, 3 .. 10.
No case of these families has a level with duplicates (`dups` is 0 throughout): a level that must stay in its workgroup
is shown by the multi-symbol ones."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402
from test_wide_level import _region_child, WIDE, NARROW, LV_ITEMS, LV_HAS, LV_HARD, LV_SLOTS, LV_TICKED  # noqa: E402

pytestmark = pytest.mark.gpu

MODE_HARD = 0
CASES = ["seed2", "seed5", "seed7"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, oracle_bin):
    """case -> (oracle FASTA, oracle trace, grid run, workgroup run), made once per case."""
    made = {}

    def get(case):
        if case not in made:
            d = str(tmp_path_factory.mktemp(case))
            args = T.make_case(int(case[4:]), d)
            exp_fa, exp_tr = T.run_oracle(args, d, trace=True)
            made[case] = (exp_fa, exp_tr, _region_child(args, os.path.join(d, "wide"), WIDE),
                          _region_child(args, os.path.join(d, "narrow"), NARROW))
        return made[case]
    return get


def hard_levels(log):
    return [r for r in log if int(r["mode"]) == MODE_HARD]


def must_stay(r):
    return int(r["multi"]) != 0 or int(r["dups"]) != 0


@pytest.mark.parametrize("case", CASES)
def test_hard_levels_on_the_grid_equal_the_workgroup_and_the_oracle(case, runs):
    exp_fa, exp_tr, (w_fa, w_trace, w_log), (n_fa, n_trace, n_log) = runs(case)
    assert n_fa == exp_fa and w_fa == exp_fa
    assert w_trace == n_trace and n_trace.count("\n") > 10
    T.compare_traces(w_trace, exp_tr)
    T.compare_traces(n_trace, exp_tr)
    assert len(w_log) == len(n_log) > 3
    # which path ran: no level of the second run had anything on the grid; in the first every hard level that may go
    # there went, behind the grid's update, its `has` marks and its draw slots, and no other level did
    assert all(int(r["done"]) == 0 for r in n_log)
    hard = hard_levels(w_log)
    assert hard and any(not must_stay(r) for r in hard)
    for r in w_log:
        d = int(r["done"])
        if int(r["mode"]) == MODE_HARD and not must_stay(r):
            assert d & LV_HARD, r
            assert d & (LV_ITEMS | LV_HAS | LV_SLOTS | LV_TICKED) == LV_ITEMS | LV_HAS | LV_SLOTS | LV_TICKED, r
        else:
            assert d & LV_HARD == 0, r
    assert [(r["mode"], r["S"], r["Q"]) for r in w_log] == [(r["mode"], r["S"], r["Q"]) for r in n_log]


def test_the_cases_hold_the_shapes_they_were_chosen_for(runs):
    on_grid = {}
    stayed = 0
    for case in CASES:
        _, _, (_, _, w_log), _ = runs(case)
        on_grid[case] = [(int(r["S"]), int(r["Q"])) for r in hard_levels(w_log) if int(r["done"]) & LV_HARD]
        stayed += sum(1 for r in hard_levels(w_log) if must_stay(r) and not int(r["done"]) & LV_HARD)
    assert stayed > 0                                                   # multi-symbol levels between the grid ones
    assert all(S == 1 and Q < 64 for S, Q in on_grid["seed2"]) and on_grid["seed2"]
    assert any(S == 2 for S, _ in on_grid["seed5"])
    assert any(256 < Q <= 264 for _, Q in on_grid["seed7"])             # just above one workgroup of k_hard_resp
    assert max(S for S, _ in on_grid["seed7"]) >= 7


def test_mates_seen_for_the_first_time_on_the_grid(runs):
    """seed 2 is the paired family: the mate of a slot's read starts further along the window, so at the first levels no
    mate has been entered into read_loglik yet and the hard update gives it a zero cell first (zero_unseen_mates, on the
    grid k_hard_mates, a kernel boundary in front of the responsibilities that mark it present).  Its trace against the
    oracle's is in the parametrised test; here: the case is paired and its first grid level comes first of all."""
    kw, _ = T.scenario(2)
    assert kw.get("paired")
    _, _, (_, _, w_log), _ = runs("seed2")
    first = next(i for i, r in enumerate(w_log) if int(r["done"]) & LV_HARD)
    assert first <= 1 and int(w_log[first]["S"]) == 1
