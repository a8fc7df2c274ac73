"""The shape of a context (rambl_amd/csrc/sc_plan.hpp: plan_context) and the uniform stream, checked without a GPU.

Every expected row was derived by hand from sc_ctx_create as it stood before the plan was split out of it (commit
9ee573f, rambl_amd/csrc/sc_api.cpp; the line numbers below are that file's), on a GPU of 256 CUs:

  :1843-1844  stream_count clamped to 1..512
  :1852       resident = SC_RESIDENT != 0 when set, else stream_count > 1
  :1857-1859  cap = SC_RESIDENT_SLOTS or CUs - 32, clamped to 1..CUs; mailboxes = min(stream_count, cap) when resident
  :1863-1867  resident with several mailboxes: workers = min(max(stream_count, mailboxes + SC_SETUP_WORKERS), 512)
  :1880-1884  launch streams = SC_LAUNCH_STREAMS or 11, clamped to 1..30, 1 when resident, at most the workers;
              set-up streams = 4 from 8 workers on, 2 from 2 on, else 1
  :389-397    sc_host_plan: executors = CPUs / ranks - 1 clamped to 1..min(workers, 32); a server when workers > 1
  :1896-1898  watch = resident and workers > 1: one executor more (the server's CPU), at most min(workers, 32);
              SC_EXEC_THREADS >= 1 replaces the count (at most the workers)
  :1903-1906  arenas = max(executors + 1, 2) when staging (SC_PINNED_STAGING != 0 when set, else workers > 1), else 0;
              set-up places = max(1, (executors + 1) / 2), or max(1, SC_SETUP_LIMIT)
  :1948-1951  set-up threads = executors / 2 from 2 executors on, or SC_EXEC_LONG clamped to 0..executors - 1;
              without SC_SETUP_LIMIT and with set-up threads: set-up places = 2 * set-up threads
  :1954-1958  a server thread when not watching and workers > 1
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("resident", "res_slots", "workers", "launch_streams", "setup_streams", "exec_threads", "long_threads", "watch", "server",
        "arena_limit", "setup_limit")
# (stream_count, CPUs, ranks on the host, options) -> the values of KEYS
ROWS = [
    # one region: a launch per level from the worker itself, nothing shared
    ((1, 16, 1, ()), (0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1)),
    # 224: 15 executors + the server's CPU = 16, 8 of them for set-ups, 2 * 8 set-up places, 16 + 1 arenas
    ((224, 16, 1, ()), (1, 224, 224, 1, 4, 16, 8, 1, 0, 17, 16)),
    # above the CUs - 32 cap: 224 mailboxes, the workers asked for; 600 is clamped to 512
    ((256, 16, 1, ()), (1, 224, 256, 1, 4, 16, 8, 1, 0, 17, 16)),
    ((600, 16, 1, ()), (1, 224, 512, 1, 4, 16, 8, 1, 0, 17, 16)),
    # a launch per level: 11 streams and a server, 15 executors (7 for set-ups: 14 places), 16 arenas
    ((224, 16, 1, ("SC_RESIDENT=0",)), (0, 224, 224, 11, 4, 15, 7, 0, 1, 16, 14)),
    ((224, 16, 1, ("SC_RESIDENT_SLOTS=8", "SC_SETUP_WORKERS=4")), (1, 8, 224, 1, 4, 16, 8, 1, 0, 17, 16)),
    # 8 mailboxes + 4 workers for set-ups: 12 workers, so 12 executors at most (6 + 6), 13 arenas
    ((8, 16, 1, ("SC_RESIDENT_SLOTS=8", "SC_SETUP_WORKERS=4")), (1, 8, 12, 1, 4, 12, 6, 1, 0, 13, 12)),
    # SC_SETUP_LIMIT survives the set-up threads' override
    ((224, 16, 1, ("SC_SETUP_LIMIT=3",)), (1, 224, 224, 1, 4, 16, 8, 1, 0, 17, 3)),
    ((224, 16, 1, ("SC_EXEC_THREADS=2",)), (1, 224, 224, 1, 4, 2, 1, 1, 0, 3, 2)),
    # no set-up threads: the places stay (16 + 1) / 2
    ((224, 16, 1, ("SC_EXEC_LONG=0",)), (1, 224, 224, 1, 4, 16, 0, 1, 0, 17, 8)),
    ((224, 16, 1, ("SC_PINNED_STAGING=0",)), (1, 224, 224, 1, 4, 16, 8, 1, 0, 0, 16)),
    # 99 launch streams: 30 where levels are launched, still 1 where they are not
    ((224, 16, 1, ("SC_RESIDENT=0", "SC_LAUNCH_STREAMS=99")), (0, 224, 224, 30, 4, 15, 7, 0, 1, 16, 14)),
    ((224, 16, 1, ("SC_LAUNCH_STREAMS=99",)), (1, 224, 224, 1, 4, 16, 8, 1, 0, 17, 16)),
    # eight ranks on 16 CPUs: 2 CPUs each -- one executor and the server's CPU, which a resident context gives an executor
    ((224, 16, 8, ()), (1, 224, 224, 1, 4, 2, 1, 1, 0, 3, 2)),
    ((224, 16, 8, ("SC_RESIDENT=0",)), (0, 224, 224, 11, 4, 1, 0, 0, 1, 2, 1)),
    # a resident context of one region (SC_RESIDENT=1): one mailbox, nobody watches
    ((1, 16, 1, ("SC_RESIDENT=1",)), (1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1)),
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    # sc_plan.hpp alone, plain g++: no ROCm include path
    path = str(tmp_path_factory.mktemp("ctx_plan") / "ctx_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", path, os.path.join(ROOT, "tests", "native", "ctx_plan_check.cpp")])
    return path


def test_plan_rows(exe):
    # the options travel as arguments; the environment's SC_* must not reach the plan
    env = dict(os.environ, SC_RESIDENT="0", SC_EXEC_THREADS="3", SC_SETUP_LIMIT="1")
    args = ["%d:256:%g:%d" % (s, c, w) + "".join(":" + o for o in opts) for (s, c, w, opts), _ in ROWS]
    out = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().splitlines()
    assert len(out) == len(ROWS)
    for ((s, c, w, opts), want), line in zip(ROWS, out):
        rec = json.loads(line)
        assert tuple(rec[k] for k in KEYS) == want, (s, c, w, opts, rec)


def test_plan_agrees_with_sc_host_plan(exe):
    """The context's executors and server are sc_host_plan's: the same two threads' worth of CPUs, whichever of them
    watches the stamps (tests/test_stage5.py::test_eight_ranks_fit_sixteen_cpus pins sc_host_plan itself)."""
    from rambl_amd import capi
    for streams in (1, 16, 128, 224, 512):
        for cpus, world in ((16, 8), (16, 1), (256, 8), (2, 8)):
            for opts in ("", ":SC_RESIDENT=0"):
                arg = "%d:256:%d:%d%s" % (streams, cpus, world, opts)
                rec = json.loads(subprocess.run([exe, arg], stdout=subprocess.PIPE, check=True, timeout=60).stdout)
                ex, srv, ing = capi.host_plan(rec["workers"], world, float(cpus))
                assert rec["host_plan"] == [ex, srv, ing], (arg, rec)
                if rec["watch"]:       # :1897, the server's CPU is an executor's
                    assert (rec["exec_threads"], rec["server"]) == (min(ex + srv, rec["workers"], 32), 0), (arg, rec)
                else:
                    assert (rec["exec_threads"], rec["server"]) == (ex, srv), (arg, rec)
    rec = json.loads(subprocess.run([exe, "256:256:16:8"], stdout=subprocess.PIPE, check=True, timeout=60).stdout)
    assert rec["host_plan"] == [1, 1, 2] and (rec["exec_threads"], rec["server"]) == (2, 0)


def test_uniform_stream_is_mt19937(exe):
    """uniform_stream(1234, n) == std::mt19937(1234) through std::generate_canonical<double, 53>, value for value."""
    rec = json.loads(subprocess.run([exe], stdout=subprocess.PIPE, check=True, timeout=60).stdout)
    assert rec == {"uniform_ok": True}
