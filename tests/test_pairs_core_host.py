"""CPU: the word arithmetic of the gene-against-gene kernel (rambl_amd/csrc/sc_pairs_core.hpp: codes, match masks, the block
step, the column of W steps) in a stand-alone program under the host sanitizers, at every instantiated W, on every named edge
of tests/pair_lib.py, against the plain restatement.  Not the library, nothing loaded into Python."""
import os
import random
import subprocess

import pytest

import pair_lib as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pairs_check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native") / "pairs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out, os.path.join(ROOT, "tests", "native", "pairs_check.cpp")])
    return out


def run(exe, args, text=b""):
    p = subprocess.run([exe] + args, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-2000:], p.stderr.decode()[-4000:])
    return p.stdout.decode().split("\n")[:-1]


def widths_of(exe):
    return tuple(int(x) for x in run(exe, ["widths"])[0].split())


def test_the_width_list_is_the_librarys(pairs_check_bin):
    from rambl_amd import otu
    widths = widths_of(pairs_check_bin)
    assert list(widths) == otu.widths() and list(widths) == sorted(set(widths)) and 64 * widths[-1] == P.MAX_LEN == otu.MAX_LEN


def test_every_named_edge_at_every_width(pairs_check_bin):
    widths = widths_of(pairs_check_bin)
    edges = P.distance_edges(widths)
    genes, pairs, want = P.flatten(edges)
    lines = run(pairs_check_bin, [], b"".join(genes[a] + b" " + genes[b] + b"\n" for a, b in pairs))
    assert len(lines) == len(pairs) > P.GRID_TILES
    seen = set()
    for (a, b), line, d in zip(pairs, lines, want):
        fits = [64 * w >= len(genes[a]) for w in widths]
        assert line.split() == [str(d) if f else "-" for f in fits], (len(genes[a]), len(genes[b]), line, d)
        seen.add(fits.index(True))
    assert seen == set(range(len(widths)))          # every W was some pattern's least


def test_random_pairs_with_other_bytes(pairs_check_bin):
    """Short and long random pairs over an alphabet with N, lower case and a byte above 127."""
    widths = widths_of(pairs_check_bin)
    rng = random.Random(8163)
    cases = []
    for k in range(120):
        n, m = (rng.randrange(1, 200), rng.randrange(1, 200)) if k < 100 else (rng.randrange(1, P.MAX_LEN + 1), rng.randrange(1, P.MAX_LEN + 1))
        a = bytes(rng.choice(b"ACGTacgtN-\xe9") for _ in range(n))
        cases.append((a, P.mutate(rng, a, rng.randrange(0, 12)) if k % 2 else bytes(rng.choice(b"ACGTacgtNR") for _ in range(m))))
    lines = run(pairs_check_bin, [], b"".join(a + b" " + b + b"\n" for a, b in cases))
    for (a, b), line in zip(cases, lines):
        d = P.edit_distance(a, b)
        assert line.split() == [str(d) if 64 * w >= len(a) else "-" for w in widths], (a[:40], b[:40])


def test_lengths_outside_the_limits_stop_the_program(pairs_check_bin):
    p = subprocess.run([pairs_check_bin], input=b"A " + b"C" * (P.MAX_LEN + 1) + b"\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"outside 1..2048" in p.stderr
