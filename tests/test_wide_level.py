"""A lone region's levels with their pieces on a grid (launch_level: k_level_copy, k_level_update, k_level_entries,
k_level_rows in front of the level's kernel) against the same levels inside their one workgroup.

SC_WIDE_MIN (tests only, read once per process) is the number of (strain, read) items above which a level of a context
that walks a single region goes wide: 0 sends every level that can, a huge value none.  Every run with the variable set
is a child process with its own time limit.

Whole regions: FASTA equal to the oracle's and to each other, %.17g traces byte-identical, and the level log shows that
the wide run really had pieces on the grid where the other had none.  One level through sc_sample_level: draws per
strain, per (strain, symbol) and the tier counts equal between the two and equal to oracle_urn_draws."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402
import test_sampler_tiers as ST  # noqa: E402  (helpers only)
from test_gpu_parity import _GRID_CHILD  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE, NARROW = "0", str(1 << 60)
LV_COPIES, LV_ITEMS, LV_HAS, LV_HARD, LV_SLOTS, LV_ROWS, LV_TICKED = 1, 2, 4, 8, 16, 32, 64
ROWS_BYTES = 141056                       # LDS share of the weight rows (CHAINW_ROWS_BYTES), as test_sampler_tiers has it


# ---------------------------------------------------------------------------------------------------------------------
# whole regions

def _region_child(args, prefix, wide_min):
    """-> (FASTA, trace, level log rows) of the region walked in a child with SC_WIDE_MIN=wide_min."""
    log = prefix + ".levels"
    env = dict(os.environ, SC_WIDE_MIN=wide_min, SC_LEVEL_LOG=log)
    env.pop("SC_GRID_MIN", None)
    p = subprocess.run([sys.executable, "-c", _GRID_CHILD, T.ROOT, "1", "1", prefix] + list(args), env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    rows = []
    for line in open(log + ".0"):
        f = line.split()
        rows.append({f[i]: f[i + 1] for i in range(0, f.index("ph"), 2)})
    return open(prefix + "0.fa").read(), open(prefix + "0.trace").read(), rows


@pytest.fixture(scope="module")
def region_runs(tmp_path_factory, oracle_bin):
    """case -> (expected FASTA, wide run, workgroup run), made once per case."""
    made = {}

    def get(case):
        if case not in made:
            d = str(tmp_path_factory.mktemp(case))
            if case == "tie525":
                args, _ = T.big_case(525, d)
                exp_fa = open(os.path.join(ROOT, "tests", "golden", "tie_case525", "expected.fa")).read()
            else:
                args = T.make_case(int(case[4:]), d)
                exp_fa, _ = T.run_oracle(args, d)
            made[case] = (exp_fa, _region_child(args, os.path.join(d, "wide"), WIDE),
                          _region_child(args, os.path.join(d, "narrow"), NARROW))
        return made[case]
    return get


# seed 2: paired reads (the `has` -> rows order, the mate cells); seed 5: insertions (levels that must stay in their
# workgroup between wide ones); seed 7: up to five strains; tie525: an outcome that rests on bitwise equal sums
@pytest.mark.parametrize("case", ["seed2", "seed5", "seed7", "tie525"])
def test_wide_region_equals_workgroup_region(case, region_runs):
    exp_fa, (w_fa, w_trace, w_log), (n_fa, n_trace, n_log) = region_runs(case)
    assert n_trace.count("\n") > 10
    assert n_fa == exp_fa
    assert w_fa == n_fa
    assert w_trace == n_trace
    assert len(w_log) == len(n_log) > 3
    assert all(int(r["done"]) == 0 for r in n_log)
    done = [int(r["done"]) & ~LV_TICKED for r in w_log]
    assert all((int(r["done"]) & LV_TICKED != 0) == (d != 0) for d, r in zip(done, w_log))      # level_wall from the first grid kernel
    # a sampler level with single-symbol labels has its update, marks, slots and rows on the grid, one without an update
    # (read_assign) its slots and rows; seed 2 never has more than one candidate: its levels are plain ones
    full = LV_ITEMS | LV_HAS | LV_SLOTS | LV_ROWS
    sampler = [(d, r) for d, r in zip(done, w_log) if float(r["chain_us"]) > 0]
    assert sampler or case == "seed2"
    for d, r in sampler:
        assert int(r["multi"]) or d & full == full or d == LV_SLOTS | LV_ROWS, r
    assert any(d & (LV_ITEMS | LV_HAS) == LV_ITEMS | LV_HAS for d in done), done
    for d, r in zip(done, w_log):
        if int(r["multi"]):
            assert d & LV_ITEMS == 0, r                                 # ... a level with a multi-symbol label keeps its update
        if d & LV_ITEMS:
            assert d & LV_HAS and (int(r["ncopy"]) == 0 or int(r["copyn"]) == 0 or d & LV_COPIES), r      # copies in front of the update
        if d & LV_ROWS:
            assert d & LV_SLOTS, r
    if case == "seed5":
        assert any(int(r["multi"]) for r in w_log)            # levels between the wide ones that stay in their workgroup


def test_wide_copies_with_odd_prefix_and_empty_first_level(region_runs):
    """The row copies of a wide level move min(copy_n, reads) cells as double2.  The level logs of seeds 5 and 7 show
    copies on the grid with an odd copy_n (7 and 60 levels).  The first level of every region has copy_n = 0 and no copy
    to make, and no later level can have copies with copy_n = 0: a copy comes from an extension behind a branching node,
    a node is in the graph because reads cover it, and those reads are entries of its level, which put copy_n of every
    later level above 0.  No seed can show that case, so k_level_copy has no special path for it (an empty loop).  The
    traces of these runs are compared above."""
    odd = 0
    for case in ("seed2", "seed5", "seed7"):
        _, (_, _, w_log), _ = region_runs(case)
        assert int(w_log[0]["copyn"]) == 0 and int(w_log[0]["ncopy"]) == 0
        for r in w_log:
            if int(r["ncopy"]) > 0:
                assert int(r["copyn"]) > 0, r
                assert int(r["done"]) & LV_COPIES or int(r["done"]) == 0, r
                odd += int(r["done"]) & LV_COPIES and int(r["copyn"]) % 2
    assert odd > 0


_CAP120_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from rambl_amd import capi, cli, synth
meta = json.load(open(sys.argv[2]))
gene = synth.make_gene(77, glen=600, n_strains=100, n_reads=30000, name="wide", n_sub=12, err=0.01)
fa, sam = synth.write_dataset(sys.argv[3], [gene])
pa = cli.parse_cmd_line(meta["argv"] + [fa, sam])
params = capi.default_params(float(pa.error_rate), float(pa.tau), float(pa.diff_rate), want_trace=True)
params.max_candidates = meta["max_candidates"]
with capi.Context(0, 1) as ctx:
    res = [(w, ctx.wait(ctx.submit(r, params), want_trace=True)) for w, r in cli.load_regions(pa)]
open(sys.argv[4] + ".fa", "w").write("".join(cli.format_fasta(w, r, pa.tau) for w, r in res))
open(sys.argv[4] + ".trace", "w").write("".join(r.trace for _, r in res))
"""


def test_wide_cap120(tmp_path):
    """tests/golden/wide_cap120 (up to 122 candidates at a level: every NB of k_level_rows in a walk; the fixture that
    found a copy made over an already updated parent row), every level wide against every level in its workgroup: the
    fixture's FASTA from both, %.17g traces byte-identical."""
    gold = os.path.join(ROOT, "tests", "golden", "wide_cap120")
    runs = []
    for tag, wide_min in (("wide", WIDE), ("narrow", NARROW)):
        d = tmp_path / tag
        d.mkdir()
        out = str(d / "out")
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        p = subprocess.run([sys.executable, "-c", _CAP120_CHILD, T.ROOT, os.path.join(gold, "meta.json"), str(d), out], env=env,
                           timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        runs.append((open(out + ".fa").read(), open(out + ".trace").read()))
    (w_fa, w_trace), (n_fa, n_trace) = runs
    assert n_fa == open(os.path.join(gold, "expected.fa")).read()
    assert w_fa == n_fa
    assert n_trace.count("\n") > 100
    assert w_trace == n_trace


# ---------------------------------------------------------------------------------------------------------------------
# one level

def w_stride(S):
    st = (S + 1 + 3) & ~3
    return st if st & 4 else st + 4


def _levels():
    """name -> (level, sweeps, uniforms): the smallest shapes at which the slots and rows on the grid, and the copy of
    the rows into LDS, can go wrong.  The same in the parent and in both children (seeded)."""
    out = {}

    def add(name, lv, n=None, seed=0):
        n = max(1, min(ST.MAX_DRAWS // lv.Q, 400 // lv.Q + 1)) if n is None else n
        out[name] = (lv, n, np.random.default_rng(seed + 99).random(n * lv.Q))

    # S: 16 | 17 and 32 | 33 and 48 | 65 change NB; above 32 strains the rows loop reads its cells twice
    for S in (2, 16, 17, 32, 33, 48, 65, 128):
        rng = np.random.default_rng(7000 + S)
        add("S%d" % S, ST.make_level(rng, S, 40, cn_max=2, mate_frac=0.5, has_frac=0.8, spread=4.0, e0=int(rng.integers(1, 30))), seed=S)
    # Q: one slot; 63 | 64 | 65 around a wavefront = a workgroup of k_level_rows; 600: a second round of the level's
    # workgroup; 8200: a second round of the grid of k_level_rows (128 wavefronts)
    for Q in (1, 63, 64, 65, 600, 8200):
        rng = np.random.default_rng(8000 + Q)
        S = 2 if Q == 8200 else 9
        add("Q%d" % Q, ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.5, has_frac=0.85, spread=2.0, e0=int(rng.integers(3, 40))),
            n=2 if Q >= 600 else None, seed=Q)
    # the largest Q whose rows (and the 16 floats behind them) fit the LDS, and the first that does not: both kinds of NB = 2
    S = 20
    q_fit = (ROWS_BYTES // 4 - 16) // w_stride(S)
    for name, Q in (("fits", q_fit), ("fits_not", q_fit + 1)):
        rng = np.random.default_rng(8500)
        add(name, ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.3, has_frac=0.9, spread=3.0), n=2, seed=5)
    # named slots: flagged rows (-650 at best; -inf throughout), a read without `has`, a copy number of 3 whose copies draw
    # with a mate that is present, a mate that is absent and no mate
    rng = np.random.default_rng(8600)
    S, n_ent, n_reads = 5, 12, 20
    ll = -rng.random((S, n_reads)) * 5.0 - 0.5
    ll[:, 0] = -650.0 - rng.random(S) * 30.0
    ll[2, 0] = -650.0
    ll[:, 1] = -np.inf
    has = np.ones(n_reads, dtype=np.uint8)
    has[2] = 0
    has[15] = 0
    cn = np.ones(n_ent, dtype=np.int64)
    cn[3] = 3
    mates = [[] for _ in range(n_reads)]
    mates[3] = [14, 15]                    # copy 2 has no mate, copy 1 draws with 15 (absent), copy 0 with 14 (present)
    mates[4] = [-1]
    mates[5] = [16]
    add("named", ST.Level(rng.random(S) * 10 + 0.5, ll, has, list(range(n_ent)), cn, rng.integers(0, 6, n_ent), mates, e0=5), n=30, seed=1)
    return out


def child_main(path):
    """What a child runs: every level through sc_sample_level, the results as JSON."""
    from rambl_amd import capi
    res = {}
    with capi.Context(0, 1) as ctx:
        for name, (lv, n, U) in _levels().items():
            r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, lv.mates, n, U, e0=lv.e0)
            res[name] = dict(kdraw=r["kdraw"].tolist(), cnt=r["cnt"].tolist(),
                             out=[int(r[k]) for k in ("n_draws", "n_slow", "n_exact", "n_pass")], kind=int(r["kind"]), done=int(r["done"]))
    json.dump(res, open(path, "w"))


@pytest.fixture(scope="module")
def level_runs(tmp_path_factory, oracle_bin):
    d = tmp_path_factory.mktemp("levels")
    runs = []
    for tag, wide_min in (("wide", WIDE), ("narrow", NARROW)):
        out = str(d / (tag + ".json"))
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_wide_level as W; W.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), out)
        p = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        runs.append(json.load(open(out)))
    return _levels(), runs[0], runs[1]


_NAMES = ["S2", "S16", "S17", "S32", "S33", "S48", "S65", "S128", "Q1", "Q63", "Q64", "Q65", "Q600", "Q8200", "fits", "fits_not", "named"]


@pytest.mark.parametrize("name", _NAMES)
def test_wide_level_equals_workgroup_level_and_oracle(name, level_runs):
    levels, wide, narrow = level_runs
    assert sorted(levels) == sorted(_NAMES)
    lv, n, U = levels[name]
    _, kdraw, cnt = ST.oracle_draws(lv, n, U)
    w, g = wide[name], narrow[name]
    assert w["out"][0] == g["out"][0] == n * lv.Q
    assert np.array_equal(np.array(g["kdraw"], dtype=np.int64), kdraw), name
    assert np.array_equal(np.array(g["cnt"], dtype=np.int64), cnt), name
    assert w["kdraw"] == g["kdraw"] and w["cnt"] == g["cnt"], name
    assert w["out"] == g["out"], (name, w["out"], g["out"])          # draws, fp64-scan draws, literal draws, passes
    assert w["kind"] == g["kind"]
    # the wide run had its draw slots and weight rows on the grid (a level without update: nothing else), the other nothing
    assert w["done"] == LV_SLOTS | LV_ROWS | LV_TICKED and g["done"] == 0, (name, w["done"], g["done"])
    if name == "fits":
        assert w["kind"] == 4                                         # NB = 2, rows in LDS: copied there from tabLf, all of them
    if name == "fits_not":
        assert w["kind"] == 3                                         # NB = 2, rows in HBM
    if name == "named":
        assert w["out"][2] >= 2 * n                                   # the two flagged slots draw in the literal tier
