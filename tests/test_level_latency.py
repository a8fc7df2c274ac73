"""The grid kernels in front of a lone region's level after their dependent reads were taken out: the strains' rows,
symbols and copy pairs arrive as kernel arguments (GridParams), k_level_rows gives a draw slot to a group of G = 8
neighbouring lanes (lane k owns the row's blocks of four strains k, k + 8, ...: strain s belongs to lane (s // 4) % 8)
and finds the slot's read id in JobDev::qrid.  The rows in tabLf must be bitwise what the one-lane walk of the level's
own workgroup writes, so every level here is drawn twice -- in a child with SC_WIDE_MIN=0 (on the grid) and in a child
with a huge value (in its workgroup) -- and the two must agree exactly with each other and with oracle_urn_draws:
draws per strain, per (strain, symbol), the tier counts (fp64 scan, literal) and the passes.  The uniforms of the
seam levels sit at 2 * eps and eps / 10 from the boundaries (test_sampler_tiers), where a weight one ulp off changes a
tier count.  Every case checks that its input reaches the seam it is named for.

sc_sample_level runs a level without an update (the read_assign shape).  What only a level with an update has -- the
symbols and log tables of k_level_update, the copies of k_level_copy, the marks between the update and the rows --
is reached by whole regions (seeds 2 and 7 of make_case, and a paired region without indels made here), wide against
narrow, with the level log showing which pieces ran on the grid and with how many copies.  The log names counts, not
values: the values of an update and of its copies (a label N, a symbol >= K, K = KMAX, which pairs a level copies) are
compared on single levels through sc_update_level (tests/test_update_edges_gpu.py).  Step 3 of the work (fewer launches)
was not built: k_level_entries is launched as before."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402,F401
import test_sampler_tiers as ST  # noqa: E402  (helpers only)
import test_wide_level as W  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu

G = 8                                   # lanes per draw slot in k_level_rows (ROWS_G)
STRAINS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 127, 128)
SLOTS = (1, 2, 15, 16, 17, 63, 64, 65, 129)
SLOT_STRAINS = (2, 17, 33)
FLAG_KINDS = ("below600", "nan1", "neginf", "lane_neginf")
FLAG_Q = 70
FLAG_AT = (0, 7, 63, FLAG_Q - 1)        # first; last of a wavefront of k_level_rows (8 slots); last of a wavefront of the
#                                         level's own workgroup (64 slots); last


def lane_of(s):
    return (s // 4) % G


def _crafted(lv, total, rng):
    """Uniforms a third of which sit 2 * eps or eps / 10 from a boundary, the others 1e-2 from every boundary."""
    S = lv.S

    def plan(t):
        if t % 3 != 1:
            return None
        return ST.delta_value("2eps" if (t // 3) % 2 else "eps/10", S), (1 if (t // 6) % 2 else -1)
    U, crafted, _ = ST.crafted_run(lv, total, rng, plan)
    assert len(crafted) >= total // 6, (S, total, len(crafted))
    return U


def _heavy_a0(rng, S):
    # a few strains carry most of the weight: room for uniforms 1e-2 from every boundary
    a0 = rng.random(S) * 3.0 + 0.5
    a0[rng.choice(S, min(S, 3), replace=False)] += 200.0
    return a0


def make_levels():
    """name -> (level, sweeps, uniforms).  Made once by the parent and handed to both children in a file."""
    out = {}
    for S in STRAINS:
        rng = np.random.default_rng(31000 + S)
        lv = ST.make_level(rng, S, 24, cn_max=2, mate_frac=0.4, has_frac=0.9, spread=1.0, a0=_heavy_a0(rng, S), e0=int(rng.integers(1, 30)))
        n = max(1, 120 // lv.Q)
        out["S%d" % S] = (lv, n, _crafted(lv, n * lv.Q, rng))
    for S in SLOT_STRAINS:
        for Q in SLOTS:
            rng = np.random.default_rng(32000 + 200 * S + Q)
            lv = ST.make_level(rng, S, Q, cn_max=1, mate_frac=0.4, has_frac=0.9, spread=1.0, a0=_heavy_a0(rng, S), e0=int(rng.integers(1, 30)))
            n = max(1, 130 // lv.Q)
            out["Q%d_S%d" % (Q, S)] = (lv, n, _crafted(lv, n * lv.Q, rng))
    # flagged slots and their neighbours, 40 strains: ten blocks and the padding, so lanes 0 .. 2 of a group own two
    # blocks and the others one
    S = 40
    for kind in FLAG_KINDS:
        rng = np.random.default_rng(33000 + FLAG_KINDS.index(kind))
        lv = ST.make_level(rng, S, FLAG_Q, cn_max=1, spread=3.0)
        lv.has[:] = 1
        for r in FLAG_AT:
            if kind == "below600":
                row = -650.0 - rng.random(S) * 30.0
            elif kind == "nan1":
                row = lv.ll[:, r].copy()
                row[int(rng.integers(S))] = np.nan
            elif kind == "neginf":
                row = np.full(S, -np.inf)
            else:
                row = lv.ll[:, r].copy()
                row[[s for s in range(S) if lane_of(s) == 2]] = -np.inf
            lv.ll[:, r] = row
        lv = ST.Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
        out["flag_" + kind] = (lv, 3, rng.random(3 * lv.Q))
    # where the maximum sits
    rng = np.random.default_rng(33100)
    lv = ST.make_level(rng, S, 33, cn_max=1, spread=3.0)
    lv.has[:] = 1
    last = [s for s in range(S) if lane_of(s) == G - 1]
    for r in range(33):
        lv.ll[last[r % len(last)], r] = 1.0 + rng.random()              # above every other cell of the slot
    lv = ST.Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    out["max_last_lane"] = (lv, 4, rng.random(4 * lv.Q))
    rng = np.random.default_rng(33200)
    lv = ST.make_level(rng, S, 33, cn_max=1, spread=3.0)
    lv.has[:] = 1
    for r in range(33):
        a, b = 4 * (r % 4), 16 + 4 * ((r + 1) % 4)                       # two strains of neighbouring lanes
        if r % 2 == 0:
            lv.ll[:, r] -= 800.0                                         # tied and flagged (every other slot)
        lv.ll[a, r] = lv.ll[b, r] = 0.25 if r % 2 else -700.0 + r       # above the rest
    lv = ST.Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    out["max_tied"] = (lv, 4, rng.random(4 * lv.Q))
    # one block of strains: lanes 1 .. 7 of every group hold no strain (S <= 4)
    rng = np.random.default_rng(33300)
    lv = ST.make_level(rng, 3, 21, cn_max=1, spread=3.0)
    lv.has[:] = 1
    lv.ll[:, 0] = -np.inf
    lv.ll[:, 20] = -650.0 - rng.random(3)
    lv.ll[1, 7] = np.nan
    lv = ST.Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    out["empty_share"] = (lv, 6, rng.random(6 * lv.Q))
    # mates: read present or not x mate present or not, a mate that is an entry of the same level
    rng = np.random.default_rng(33400)
    lv = ST.make_level(rng, 9, 40, cn_max=2, mate_frac=0.8, has_frac=0.5, spread=1.0, a0=_heavy_a0(rng, 9), e0=11)
    n = 3
    out["mates"] = (lv, n, _crafted(lv, n * lv.Q, rng))
    return out


def _names():
    return (["S%d" % S for S in STRAINS] + ["Q%d_S%d" % (Q, S) for S in SLOT_STRAINS for Q in SLOTS] +
            ["flag_" + k for k in FLAG_KINDS] + ["max_last_lane", "max_tied", "empty_share", "mates"])


def child_main(levels_path, out_path):
    """What a child runs: every level through sc_sample_level, the results as JSON."""
    from rambl_amd import capi
    levels = pickle.load(open(levels_path, "rb"))
    res = {}
    with capi.Context(0, 1) as ctx:
        for name, (lv, n, U) in levels.items():
            r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, lv.mates, n, U, e0=lv.e0)
            res[name] = dict(kdraw=r["kdraw"].tolist(), cnt=r["cnt"].tolist(),
                             out=[int(r[k]) for k in ("n_draws", "n_slow", "n_exact", "n_pass")], kind=int(r["kind"]), done=int(r["done"]))
    json.dump(res, open(out_path, "w"))


@pytest.fixture(scope="module")
def level_runs(tmp_path_factory, oracle_bin):
    d = tmp_path_factory.mktemp("latency_levels")
    levels = make_levels()
    path = str(d / "levels.pickle")
    pickle.dump(levels, open(path, "wb"))
    runs = []
    for tag, wide_min in (("wide", W.WIDE), ("narrow", W.NARROW)):
        out = str(d / (tag + ".json"))
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_level_latency as L; L.child_main(%r, %r)" % (
            ROOT, os.path.join(ROOT, "tests"), path, out)
        p = subprocess.run([sys.executable, "-c", code], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        runs.append(json.load(open(out)))
    return levels, runs[0], runs[1]


def _reaches_seam(name, lv, n, w):
    """Raises unless the level `name` is the input its name promises."""
    slot_max = np.full(lv.Q, -np.inf)
    has = lv.has != 0
    with np.errstate(all="ignore"):
        x = np.where(has[lv.rid][None, :], lv.ll[:, lv.rid], 0.0)
        hu = (lv.uid >= 0) & has[np.maximum(lv.uid, 0)]
        x = x + np.where(hu[None, :], lv.ll[:, np.maximum(lv.uid, 0)], 0.0)
        slot_max = np.fmax.reduce(x, axis=0)                  # fmax: passes over a NaN, as the kernels do
    flagged = ~(slot_max >= -600.0)
    if name.startswith("S"):
        S = int(name[1:])
        assert lv.S == S and (w["kind"] + 1) // 2 == ST.nb_of(S)
        assert lv.Q > 64 // G                                     # more than one wavefront of k_level_rows
    elif name.startswith("Q"):
        Q, S = (int(v[1:]) for v in name.split("_"))
        assert lv.Q == Q and lv.S == S
    elif name.startswith("flag_"):
        kind = name[5:]
        assert lv.Q == FLAG_Q and (FLAG_Q * G + 63) // 64 > 4 and FLAG_Q > 64       # several wavefronts on either path
        for q in FLAG_AT:
            col = x[:, q]
            if kind == "below600":
                assert flagged[q] and np.all(col < -600.0) and np.all(np.isfinite(col))
            elif kind == "nan1":
                assert np.isnan(col).sum() == 1 and not flagged[q]
            elif kind == "neginf":
                assert flagged[q] and np.all(np.isneginf(col))
            else:
                share = np.array([lane_of(s) == 2 for s in range(lv.S)])
                assert np.all(np.isneginf(col[share])) and np.all(np.isfinite(col[~share])) and not flagged[q]
        assert flagged.sum() == (len(FLAG_AT) if kind in ("below600", "neginf") else 0)
        assert w["out"][2] >= n * int(flagged.sum())              # flagged slots draw in the literal tier
    elif name == "max_last_lane":
        assert all(lane_of(int(np.argmax(x[:, q]))) == G - 1 for q in range(lv.Q))
    elif name == "max_tied":
        for q in range(lv.Q):
            top = np.nonzero(x[:, q] == slot_max[q])[0]
            assert len(top) == 2 and lane_of(int(top[0])) != lane_of(int(top[1])), (q, top)
        assert flagged.any() and not flagged.all()
    elif name == "empty_share":
        assert lv.S < G and flagged[0] and flagged[lv.Q - 1] and np.isnan(x[:, 7]).sum() == 1
    elif name == "mates":
        hr = has[lv.rid]
        assert {(bool(a), bool(b)) for a, b in zip(hr, hu)} == {(False, False), (False, True), (True, False), (True, True)}
        assert np.any((lv.uid >= 0) & np.isin(lv.uid, lv.rid))                         # a mate that is an entry of the same level
        assert np.any((lv.uid >= 0) & ~has[np.maximum(lv.uid, 0)])                    # a mate that is absent
    else:
        raise AssertionError("no seam check for " + name)


@pytest.mark.parametrize("name", _names())
def test_grid_level_equals_workgroup_level_and_oracle(name, level_runs):
    levels, wide, narrow = level_runs
    assert sorted(levels) == sorted(_names())
    lv, n, U = levels[name]
    _, kdraw, cnt = ST.oracle_draws(lv, n, U)
    w, g = wide[name], narrow[name]
    _reaches_seam(name, lv, n, w)
    assert w["out"][0] == g["out"][0] == n * lv.Q
    assert np.array_equal(np.array(g["kdraw"], dtype=np.int64), kdraw), name
    assert np.array_equal(np.array(g["cnt"], dtype=np.int64), cnt), name
    assert w["kdraw"] == g["kdraw"] and w["cnt"] == g["cnt"], name
    assert w["out"] == g["out"], (name, w["out"], g["out"])          # draws, fp64-scan draws, literal draws, passes
    assert w["kind"] == g["kind"]
    # a level without an update: its draw slots and weight rows on the grid, nothing else; the other run nothing
    assert w["done"] == W.LV_SLOTS | W.LV_ROWS | W.LV_TICKED and g["done"] == 0, (name, w["done"], g["done"])


def test_largest_row_index_travels_in_the_packed_argument(level_runs):
    """sc_sample_level puts strain s into row (37 s + 5) % 128: with 128 strains every row 0 .. 127 is named, the largest
    the region's builder can hand out (MAXS - 1), and the rows' order is not the strains'."""
    levels, wide, narrow = level_runs
    rows = sorted((37 * s + 5) % 128 for s in range(levels["S128"][0].S))
    assert rows == list(range(128))
    assert wide["S128"]["kdraw"] == narrow["S128"]["kdraw"]


# ---------------------------------------------------------------------------------------------------------------------
# whole regions: levels with an update (k_level_copy, k_level_update, k_level_entries in front of the rows)

@pytest.fixture(scope="module")
def region_runs(tmp_path_factory, oracle_bin):
    made = {}

    def get(seed):
        if seed not in made:
            d = str(tmp_path_factory.mktemp("latency_seed%d" % seed))
            args = T.make_case(seed, d)
            exp_fa, _ = T.run_oracle(args, d)
            made[seed] = (exp_fa, W._region_child(args, os.path.join(d, "wide"), W.WIDE),
                          W._region_child(args, os.path.join(d, "narrow"), W.NARROW))
        return made[seed]
    return get


def make_update_case(outdir):
    """A paired region of three strains without indels: every label is one symbol, so every level past the first has its
    update on the grid, its sampler levels carry mates, and the strains' substitutions and the reads' errors make
    branches with one copy, with several, and none."""
    from rambl_amd import synth
    gene = synth.make_gene(41, glen=320, n_strains=3, n_reads=400, rlen=100, err=0.005, n_sub=6, n_ins=0, n_del=0,
                           paired=True, name="u")
    fa, sam = synth.write_dataset(outdir, [gene])
    return ["-r", "u:1-%d" % len(gene["ref"])] + T.RAMBL_ARGS + [fa, sam]


@pytest.fixture(scope="module")
def update_runs(tmp_path_factory, oracle_bin):
    d = str(tmp_path_factory.mktemp("latency_update"))
    args = make_update_case(d)
    exp_fa, _ = T.run_oracle(args, d)
    return exp_fa, W._region_child(args, os.path.join(d, "wide"), W.WIDE), W._region_child(args, os.path.join(d, "narrow"), W.NARROW)


def test_copy_counts_and_mates_on_levels_with_an_update(update_runs):
    """k_level_copy's pairs and k_level_update's rows and symbols as kernel arguments, on levels with an update, through
    the normal walk (sc_sample_level runs none).  Reached, each with its check on the wide run's level log: levels with no
    copy, with one and with several, an odd copy_n among them, every one of them copied on the grid; sampler levels of a
    paired region with the update, the marks, the slots and the rows on the grid (every read of the region has a mate, so
    the rows of those levels read `has` of mates that the marks in front of them set or left).  The FASTA is the oracle's
    and the %.17g trace the narrow run's, byte for byte.

    What the entry points cannot express, and what therefore has no case here (a decision, not an oversight): which of the
    four (hr, hu) combinations a region's slots take -- the level log names counts only; the four combinations and the
    same-level mate are asserted on the single level `mates` above, which has no update.  (A strain label N, a symbol >= K,
    K = KMAX and which pairs a level copies are cases of tests/update_edge_lib.py, through sc_update_level.)"""
    exp_fa, (w_fa, w_trace, w_log), (n_fa, n_trace, n_log) = update_runs
    summary = [(int(r["S"]), int(r["ncopy"]), int(r["copyn"]), int(r["multi"]), int(r["done"]), float(r["chain_us"]) > 0) for r in w_log]
    print("S ncopy copyn multi done sampler:", summary)
    assert n_fa == exp_fa and w_fa == exp_fa
    assert n_trace.count("\n") > 10 and w_trace == n_trace
    assert len(w_log) == len(n_log) > 3 and all(int(r["done"]) == 0 for r in n_log)
    done = [int(r["done"]) & ~W.LV_TICKED for r in w_log]
    upd = [r for d, r in zip(done, w_log) if d & W.LV_ITEMS]
    assert len(upd) >= len(w_log) // 2 and max(int(r["S"]) for r in upd) >= 3            # several strains' rows and symbols
    copies = [r for d, r in zip(done, w_log) if d & W.LV_COPIES]
    assert all(d & W.LV_COPIES or d == 0 for d, r in zip(done, w_log) if int(r["ncopy"]) > 0)
    assert any(int(r["ncopy"]) == 0 and d & W.LV_ITEMS for d, r in zip(done, w_log))    # n_copy = 0 in front of an update
    assert any(int(r["ncopy"]) == 1 for r in copies) and any(int(r["ncopy"]) >= 2 for r in copies), [int(r["ncopy"]) for r in copies]
    assert any(int(r["copyn"]) % 2 for r in copies)
    full = W.LV_ITEMS | W.LV_HAS | W.LV_SLOTS | W.LV_ROWS
    assert sum(1 for d, r in zip(done, w_log) if d & full == full and float(r["chain_us"]) > 0) >= 3, done


# seed 2: paired reads (mates; the marks between the update and whoever reads them); seed 7: up to five strains (sampler
# levels with an update, copies with one source and an odd prefix)
@pytest.mark.parametrize("seed", [2, 7])
def test_whole_region_wide_against_narrow(seed, region_runs):
    exp_fa, (w_fa, w_trace, w_log), (n_fa, n_trace, n_log) = region_runs(seed)
    assert n_fa == exp_fa and w_fa == exp_fa
    assert n_trace.count("\n") > 10 and w_trace == n_trace
    assert len(w_log) == len(n_log) > 3 and all(int(r["done"]) == 0 for r in n_log)
    done = [int(r["done"]) & ~W.LV_TICKED for r in w_log]
    assert any(d & (W.LV_ITEMS | W.LV_HAS) == W.LV_ITEMS | W.LV_HAS for d in done), done      # the update's arguments
    if seed == 7:
        full = W.LV_ITEMS | W.LV_HAS | W.LV_SLOTS | W.LV_ROWS
        sampler = [(d, r) for d, r in zip(done, w_log) if float(r["chain_us"]) > 0]
        assert any(d & full == full for d, _ in sampler)                                        # update, marks, slots, rows
        assert any(d == W.LV_SLOTS | W.LV_ROWS for d, _ in sampler)                             # read_assign: no update
        copies = [r for d, r in zip(done, w_log) if d & W.LV_COPIES]
        assert copies and any(int(r["copyn"]) % 2 for r in copies)                              # the copy pairs, an odd prefix
