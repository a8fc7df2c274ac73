"""GPU: one level's row copies and read log-likelihood update through the test entry sc_update_level (the production
launcher launch_level: k_level's phase_copies / phase_update / mark_present, and in front of it k_level_copy,
k_level_update and k_level_entries where the level goes to the grid), on the named cases of tests/update_edge_lib.py,
against the library's exact reference: the whole 128-row matrix, `has` and `isnew` bit for bit (a NaN for a NaN).

Every case runs in two child processes -- SC_WIDE_MIN is read once per process -- one with SC_WIDE_MIN = 0 (every level the
grid can take goes there) and one with a huge value (everything inside the level's workgroup); the pieces each run reports
(LevelHdr::done) must be the ones launch_level_grid states, and the two runs must agree with each other."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import update_edge_lib as UL  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE, NARROW = "0", str(1 << 60)


def child_main(cases_path, out_path):
    """What a child runs: every case through sc_update_level, the results as JSON (doubles as their 64 bits)."""
    from rambl_amd import capi
    cases = pickle.load(open(cases_path, "rb"))
    res = {}
    with capi.Context(0, 1) as ctx:
        for name, case in cases.items():
            r = ctx.update_level(**case.call_args())
            res[name] = dict(ll=r["ll"].view(np.uint64).ravel().tolist(), has=r["has"].tolist(), isnew=r["isnew"].tolist(), done=int(r["done"]))
    json.dump(res, open(out_path, "w"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("update_edges")
    cases = {name: UL.case(name) for name in UL.NAMES}
    path = str(d / "cases.pickle")
    pickle.dump(cases, open(path, "wb"))
    out = []
    for tag, wide_min in (("wide", WIDE), ("narrow", NARROW)):
        res = str(d / (tag + ".json"))
        env = dict(os.environ, SC_WIDE_MIN=wide_min)
        env.pop("SC_GRID_MIN", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_update_edges_gpu as G; G.child_main(%r, %r)" % (
            ROOT, os.path.join(ROOT, "tests"), path, res)
        p = subprocess.run([sys.executable, "-c", code], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        out.append(json.load(open(res)))
    return cases, {name: UL.reference(case) for name, case in cases.items()}, out[0], out[1]


def _matrix(run, case):
    return np.array(run["ll"], dtype=np.uint64).view(np.float64).reshape(UL.MAXS, case.n_reads)


@pytest.mark.parametrize("name", UL.NAMES)
def test_level_equals_the_reference_on_the_grid_and_in_the_workgroup(name, runs):
    cases, refs, wide, narrow = runs
    case, ref = cases[name], refs[name]
    UL.reaches(case)
    for tag, run in (("wide", wide[name]), ("narrow", narrow[name])):
        got = _matrix(run, case)
        bad = UL.same_bits(got, ref["ll"], ref["free"])
        assert bad.size == 0, "%s, %s run: %d cells differ, the first (row, read) %s: %r for %r" % (
            name, tag, len(bad), bad[0].tolist(), got[tuple(bad[0])], ref["ll"][tuple(bad[0])])
        assert run["has"] == ref["has"].tolist(), (name, tag)
        assert run["isnew"] == ref["isnew"].tolist(), (name, tag)
    assert narrow[name]["done"] == UL.expected_done(case, False) == 0, (name, narrow[name]["done"])
    assert wide[name]["done"] == UL.expected_done(case, True), (name, wide[name]["done"], UL.expected_done(case, True))
    w, g = _matrix(wide[name], case), _matrix(narrow[name], case)
    assert UL.same_bits(w, g, ref["free"]).size == 0 and wide[name]["has"] == narrow[name]["has"] and wide[name]["isnew"] == narrow[name]["isnew"]


def test_both_paths_were_taken(runs):
    cases, _, wide, narrow = runs
    on_grid = [n for n in UL.NAMES if wide[n]["done"] & UL.LV_ITEMS]
    assert len(on_grid) >= 40 and any(wide[n]["done"] & UL.LV_COPIES for n in UL.NAMES)
    assert all(wide[n]["done"] == 0 for n in UL.NAMES if cases[n].has_dups or cases[n].any_multi)
    assert sum(1 for n in UL.NAMES if cases[n].has_dups) >= 5 and sum(1 for n in UL.NAMES if cases[n].any_multi) >= 4


def test_update_level_rejects_what_it_cannot_run():
    from rambl_amd import capi
    ok = UL.case("copyn_odd").call_args()

    def broken(**change):
        return dict(ok, **change)
    multi = UL.case("item_six_noN").call_args()
    bad = [
        broken(ent_rid=ok["ent_rid"][:-1] + [len(ok["has"])]),                                   # a row id out of range
        broken(ent_rid=[-1] + ok["ent_rid"][1:]),
        broken(slot=[ok["slot"][1]] + ok["slot"][1:]),                                           # a shared slot
        broken(slot=[UL.MAXS] + ok["slot"][1:]),
        dict(multi, ent_labels=[(1, 8)] + multi["ent_labels"][1:]),                              # a code >= K in a multi-symbol label
        dict(multi, strain_labels=multi["strain_labels"][:2] + [(6, 9)]),
        dict(multi, ent_labels=multi["ent_labels"][:2] + [(9,)] + multi["ent_labels"][3:]),      # ... in a single one that a long strain label walks
        broken(copies=[ok["copies"][0], (ok["slot"][2], ok["copies"][0][1])]),                   # two copies into one row
        broken(copies=[ok["copies"][0], (ok["copies"][0][1], 1)]),                               # a destination that is a source
        broken(copies=[(UL.MAXS, 1)]),
        broken(K=5, lpt=ok["lpt"][:, :5, :5]), broken(code_N=3), broken(code_N=ok["K"]), broken(copy_n=-1), broken(e0=-1),
    ]
    big = UL.case("plain_cap_K16")
    over = UL.build("over", big.S + 1, 3, K=UL.KMAX)                                             # a table over capacity
    assert over.S * 256 > UL.TABLE_CAP >= big.S * 256
    bad.append(over.call_args())
    with capi.Context(0, 1) as ctx:
        for args in bad:
            with pytest.raises(capi.StrainCallError) as e:
                ctx.update_level(**args)
            assert e.value.code == capi.SC_ERR_ARG
        r = ctx.update_level(**ok)                                                               # and the context still runs a level
        ref = UL.reference(UL.case("copyn_odd"))
        assert UL.same_bits(r["ll"], ref["ll"], ref["free"]).size == 0
    with capi.Context(0, 2) as c2:                                                               # a context of two streams
        with pytest.raises(capi.StrainCallError) as e:
            c2.update_level(**ok)
        assert e.value.code == capi.SC_ERR_ARG
