"""GPU: one level's hard update behind its update through the test entry sc_hard_level (the production launcher
launch_level: k_level's level_plain_body, and in front of it k_level_entries, k_hard_mates, k_hard_resp and k_hard_sums where
the level goes to the grid), on the named cases of tests/hard_edge_lib.py against the library's long-double reference: the
draw slots, the whole 128-row matrix, `has` and `isnew` bit for bit; the responsibilities, the abundances and the
substitution histogram within the bounds the library derives from the case (bit for bit on the exact cases, NaN for NaN).

Every case runs in two child processes -- SC_WIDE_MIN is read once per process -- one with SC_WIDE_MIN = 0 (every level the
grid can take goes there) and one with a huge value (everything inside the level's workgroup); the pieces each run reports
(LevelHdr::done) must be the ones launch_level_grid states, and the two runs must agree with each other bit for bit.

Worst error / bound measured on an MI355X (each test prints its own): responsibilities 0.237 (0.325 on the grid trip's
524 289 slots), sums against the device's own responsibilities 0.498, sums against the reference 0.189."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_edge_lib as HL  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HL.LONG_DOUBLE_OK, reason="np.longdouble is not the 80-bit extended format")]

WIDE, NARROW = "0", str(1 << 60)
DOUBLES, INTS = ("ll", "resp", "abund", "subst"), ("has", "isnew", "qrid", "quid", "qcode")


def child_main(cases_path, out_path):
    """What a child runs: every case through sc_hard_level, the results as JSON (doubles as their 64 bits)."""
    from rambl_amd import capi
    cases = pickle.load(open(cases_path, "rb"))
    res = {}
    with capi.Context(0, 1) as ctx:
        for name, case in cases.items():
            r = ctx.hard_level(**case.call_args())
            res[name] = dict({k: np.ascontiguousarray(r[k]).view(np.uint64).ravel().tolist() for k in DOUBLES},
                             **{k: r[k].tolist() for k in INTS}, done=int(r["done"]))
    json.dump(res, open(out_path, "w"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hard_edges")
    cases = {name: HL.case(name) for name in HL.NAMES}
    path = str(d / "cases.pickle")
    pickle.dump(cases, open(path, "wb"))
    out = []
    for tag, wide_min in (("wide", WIDE), ("narrow", NARROW)):
        res = str(d / (tag + ".json"))
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_hard_edges_gpu as G; G.child_main(%r, %r)" % (
            ROOT, os.path.join(ROOT, "tests"), path, res)
        p = subprocess.run([sys.executable, "-c", code], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        out.append(json.load(open(res)))
    return cases, {name: HL.reference(case) for name, case in cases.items()}, out[0], out[1]


def doubles(run, key, shape):
    return np.array(run[key], dtype=np.uint64).view(np.float64).reshape(shape)


@pytest.mark.parametrize("name", HL.NAMES)
def test_level_equals_the_reference_on_the_grid_and_in_the_workgroup(name, runs):
    cases, refs, wide, narrow = runs
    c, ref = cases[name], refs[name]
    HL.reaches(c, ref)
    tol = HL.tolerances(c, ref)
    S, K, Q, n_reads = c.S, c.K, c.Q, c.u.n_reads
    for tag, run in (("wide", wide[name]), ("narrow", narrow[name])):
        for key in ("qrid", "quid", "qcode"):
            assert run[key] == ref[key].tolist(), (name, tag, key)
        got = doubles(run, "ll", (HL.MAXS, n_reads))
        bad = HL.same_bits(got, ref["ll"], ref["free"])
        assert bad.size == 0, "%s, %s run: %d cells differ, the first (row, read) %s: %r for %r" % (
            name, tag, len(bad), bad[0].tolist(), got[tuple(bad[0])], ref["ll"][tuple(bad[0])])
        assert run["has"] == ref["has"].tolist(), (name, tag)
        assert run["isnew"] == ref["isnew"].tolist(), (name, tag)
        resp, abund, subst = doubles(run, "resp", (S, Q)), doubles(run, "abund", (S,)), doubles(run, "subst", (S, K, K))
        worst = (HL.check_resp(c, ref, tol, resp),) + HL.check_sums(c, ref, tol, resp, abund, subst)
        print("%s %s: worst error / bound: resp %.3f, sums against own resp %.3f, sums against the reference %.3f" % ((name, tag) + worst))
        if c.exact:
            for key, dev in (("resp", resp), ("abund", abund), ("subst", subst)):
                assert HL.same_bits(dev, ref[key].astype(np.float64)).size == 0, (name, tag, key)
            assert np.all(resp == 1.0 / S) and np.all(abund == Q / S)
            if S == 1:
                a = c.u.strain_labels[0][0]
                assert subst[0, a].tolist() == [float(sum(1 for v in ref["qcode"] if v == b)) for b in range(K)] and subst.sum() == Q
        if name == "twins":
            assert resp[1].tobytes() == resp[5].tobytes() and abund[1].tobytes() == abund[5].tobytes() and subst[1].tobytes() == subst[5].tobytes()
            assert resp[1].tobytes() != resp[0].tobytes()
    assert narrow[name]["done"] == HL.expected_done(c, False) == 0, (name, narrow[name]["done"])
    assert wide[name]["done"] == HL.expected_done(c, True), (name, wide[name]["done"], HL.expected_done(c, True))
    # the grid runs the same functions in the same order: every output of the two runs has the same bits
    for key in DOUBLES:
        w, g = np.array(wide[name][key], dtype=np.uint64), np.array(narrow[name][key], dtype=np.uint64)
        free = ref["free"].ravel() if key == "ll" else np.zeros(w.shape, dtype=bool)
        assert np.all((w == g) | free), (name, key, int(np.flatnonzero((w != g) & ~free)[0]))
    for key in INTS:
        assert wide[name][key] == narrow[name][key], (name, key)


def test_both_paths_were_taken(runs):
    cases, _, wide, narrow = runs
    on_grid = [n for n in HL.NAMES if wide[n]["done"] & HL.LV_HARD]
    stayed = [n for n in HL.NAMES if not wide[n]["done"] & HL.LV_HARD]
    assert sorted(stayed) == ["dups", "multi", "multi_end_strain"] and len(on_grid) == len(HL.NAMES) - 3 == 53
    assert all(wide[n]["done"] & HL.LV_SLOTS for n in on_grid) and any(wide[n]["done"] & HL.LV_COPIES for n in on_grid)
    assert all(wide[n]["done"] == 0 for n in stayed) and all(narrow[n]["done"] == 0 for n in HL.NAMES)
    assert all(cases[n].u.has_dups or cases[n].u.any_multi for n in stayed)


def big_child_main(case_path, out_path):
    from rambl_amd import capi
    case = pickle.load(open(case_path, "rb"))
    with capi.Context(0, 1) as ctx:
        r = ctx.hard_level(**case.call_args())
    np.savez(out_path, done=np.int64(r["done"]), **{k: r[k] for k in DOUBLES + INTS})      # (binary: a double keeps its 64 bits)


def test_second_trip_of_the_grid_loops(tmp_path):
    """Q = 2048 * 256 + 1 at S = 2: k_hard_mates' and k_hard_resp's grids of 2 048 workgroups go round a second time for the
    last slot.  Checked with array arithmetic (hard_edge_lib.big_reference: the same rules, the same bounds), wide against
    narrow bit for bit."""
    c = HL.big_case()
    assert c.Q == HL.BIG_Q and HL.last_slot(c.Q) == (0, 0, 1) and HL.grid_blocks(c.Q, 256, 2048) == 2048
    ref = HL.big_reference(c)
    assert ref["quid"][-1] >= 0 and len(ref["zeroed"]) > 100                                  # the last slot has a mate
    path = str(tmp_path / "case.pickle")
    pickle.dump(c, open(path, "wb"))
    out = {}
    for tag, wide_min in (("wide", WIDE), ("narrow", NARROW)):
        res = str(tmp_path / (tag + ".npz"))
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_hard_edges_gpu as G; G.big_child_main(%r, %r)" % (
            ROOT, os.path.join(ROOT, "tests"), path, res)
        p = subprocess.run([sys.executable, "-c", code], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        out[tag] = run = dict(np.load(res))
        for key in ("qrid", "quid", "qcode", "has", "isnew"):
            assert np.array_equal(run[key], ref[key]), (tag, key)
        assert HL.same_bits(run["ll"], ref["ll"], ref["free"]).size == 0, tag
        print("grid_trip %s: worst error / bound: resp %.3f, sums against own resp %.3f, sums against the reference %.3f" % (
            (tag,) + HL.big_check(c, ref, run["resp"], run["abund"], run["subst"])))
    assert int(out["wide"]["done"]) == HL.expected_done(c, True) and int(out["narrow"]["done"]) == 0
    for key in DOUBLES + INTS:
        assert out["wide"][key].tobytes() == out["narrow"][key].tobytes(), key


def test_hard_level_rejects_what_it_cannot_run():
    from rambl_amd import capi
    okc = HL.case("mates_absent")
    ok = okc.call_args()
    multi = HL.case("multi").call_args()
    n_reads = len(ok["has"])

    def mates_with(r, ids):
        return [ids if k == r else list(m) for k, m in enumerate(ok["mates"])]
    big = HL.case("cap_K16")
    over = HL.build("over", big.S + 1, HL.copy_numbers(5), K=HL.KMAX)                            # a table over capacity
    assert over.S * 256 > HL.TABLE_CAP >= big.S * 256
    bad = [
        dict(ok, mates=mates_with(2, [n_reads])), dict(ok, mates=mates_with(0, [7, -2])),        # a mate id out of range
        dict(ok, ent_cn=[0] + ok["ent_cn"][1:]), dict(ok, ent_cn=ok["ent_cn"][:-1] + [-1]),      # a copy number below one
        dict(multi, ent_labels=[(6,)] + multi["ent_labels"][1:]),                                # a code >= K in a one-symbol label of a multi-symbol level
        dict(multi, ent_labels=[(0xFF,)] + multi["ent_labels"][1:]),
        dict(multi, ent_labels=multi["ent_labels"][:1] + [(1, 6)] + multi["ent_labels"][2:]),    # ... and in a longer one
        dict(ok, logpri=[np.nan] + ok["logpri"].tolist()[1:]), dict(ok, logpri=[np.inf] + ok["logpri"].tolist()[1:]),
        dict(ok, ent_rid=[-1] + ok["ent_rid"][1:]), dict(ok, slot=[HL.MAXS] + ok["slot"][1:]),   # what sc_update_level rejects
        over.call_args(),
    ]
    with capi.Context(0, 1) as ctx:
        for args in bad:
            with pytest.raises(capi.StrainCallError) as e:
                ctx.hard_level(**args)
            assert e.value.code == capi.SC_ERR_ARG
        r = ctx.hard_level(**ok)                                                                 # and the context still runs a level
        ref = HL.reference(okc)
        assert HL.same_bits(r["ll"], ref["ll"], ref["free"]).size == 0 and r["quid"].tolist() == ref["quid"].tolist()
        HL.check_resp(okc, ref, HL.tolerances(okc, ref), r["resp"])
    with capi.Context(0, 2) as c2:                                                               # a context of two streams
        with pytest.raises(capi.StrainCallError) as e:
            c2.hard_level(**ok)
        assert e.value.code == capi.SC_ERR_ARG
