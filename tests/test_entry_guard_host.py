"""CPU: the guard every entry point of the library returns through (rambl_amd/csrc/sc_error.hpp: sc::guarded, sc::LastError) in a
stand-alone program under the host sanitizers.  The program includes that header alone, so the header's freedom from HIP and
from the public header is under test as well.  Not the library, nothing loaded into Python."""
import os
import subprocess

import pytest

from rambl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What a body that throws becomes (the boundary on the C++ side): the code, and the text of sc_*_error()
THROWN = {
    "sc": (capi.SC_ERR_CAPACITY, "x"),
    "hip": (capi.SC_ERR_HIP, "sc_x: a HIP call failed: hipMalloc(&p, n): out of memory"),
    "bad_alloc": (capi.SC_ERR_INTERNAL, "sc_x: std::bad_alloc"),
    "length": (capi.SC_ERR_INTERNAL, "sc_x: y"),
    "int": (capi.SC_ERR_INTERNAL, "sc_x: unknown exception"),
}
# What a body that returns leaves behind: its own code, the text as it left it
RETURNED = {
    "pass": (0, "left by the body"),
    "code": (capi.SC_ERR_CAPACITY, "sc_x: 7 hits, room for 3"),
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native") / "entry_guard_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-pthread", "-o", out, os.path.join(ROOT, "tests", "native", "entry_guard_check.cpp")])
    p = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, (p.stdout.decode()[-2000:], p.stderr.decode()[-4000:])
    lines = [line.split("\t") for line in p.stdout.decode().split("\n")[:-1]]
    assert all(len(f) == 3 for f in lines) and len({f[0] for f in lines}) == len(lines), lines
    return {name: (int(rc), text) for name, rc, text in lines}


def test_every_case_ran(cases):
    kinds = list(RETURNED) + list(THROWN)
    assert sorted(cases) == sorted(kinds + ["null " + k for k in kinds] + ["thread 0", "thread 1", "main after threads", "clear then pass"])


def test_a_body_that_returns_passes_through(cases):
    for kind, want in RETURNED.items():
        assert cases[kind] == want, kind


def test_every_thrown_kind_gives_the_code_and_text_of_the_table(cases):
    for kind, want in THROWN.items():
        assert cases[kind] == want, kind


def test_a_null_slot_gives_the_same_codes(cases):
    for kind in list(RETURNED) + list(THROWN):
        want = (RETURNED.get(kind) or THROWN[kind])[0]
        assert cases["null " + kind] == (want, "-"), kind


def test_two_threads_read_back_their_own_message(cases):
    assert cases["thread 0"] == (capi.SC_ERR_CAPACITY, "message of thread 0")
    assert cases["thread 1"] == (capi.SC_ERR_CAPACITY - 1, "message of thread 1")
    assert cases["main after threads"] == (0, "")          # and the thread that started them has none


def test_clear_then_a_successful_body_leaves_no_text(cases):
    assert cases["clear then pass"] == (0, "")
