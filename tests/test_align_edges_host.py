"""CPU: every named edge case of tests/align_edge_lib.py reaches its edge with the plain restatements alone
(tests/native/sw_check.cpp, tests/native/blast_hits_check.cpp), is deterministic for its seed and stays inside the library's
limits; the helpers that recompute the traceback windows agree with DESIGN.md §8.7 / §8.9 on hand-made examples."""
import pytest

import align_edge_lib as E
import profile_lib as PL
import stage4_lib as L


@pytest.fixture(scope="module")
def sw_check(tmp_path_factory):
    return L.build_sw_check(tmp_path_factory.mktemp("sw_check"))


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    return PL.build_hits_check(tmp_path_factory.mktemp("hits_check"))


@pytest.mark.parametrize("name", sorted(E.STAGE4_CASES))
def test_stage4_case_reaches_its_edge(name, sw_check):
    case = E.STAGE4_CASES[name]()
    assert case.key() == E.STAGE4_CASES[name]().key()                                   # deterministic for its seed
    assert all(1 <= len(s) <= E.MAX_SEED for s in case.seeds) and all(1 <= len(r) <= E.MAX_READ for r, _ in case.reads)
    assert all(q == "*" or len(q) == len(r) for r, q in case.reads)
    case.check(L.run_sw_check(sw_check, case.seeds, case.reads))


@pytest.mark.parametrize("name", sorted(E.PROFILE_CASES))
def test_profile_case_reaches_its_edge(name, hits_check):
    case = E.PROFILE_CASES[name]()
    assert case.key() == E.PROFILE_CASES[name]().key()
    assert all(1 <= len(g) <= E.MAX_SEED for g in case.genes) and all(1 <= len(s) <= E.MAX_READ for s in case.segs)
    E.run_profile_check(case, hits_check)


def test_evalue_edge_flips_on_the_restatement(hits_check):
    case, hit, e = E.evalue_edge(hits_check)
    at = PL.run_hits_check(hits_check, case.genes, case.segs, 0.0, e)
    below = PL.run_hits_check(hits_check, case.genes, case.segs, 0.0, E.math.nextafter(e, 0.0))
    assert hit in at and hit not in below and len(at) == len(below) + 1


def test_window_helpers_on_hand_made_examples():
    # stage 4, DESIGN §8.7: a read of 100 bases, 10S40M5D45M5S at POS 201 with AS = 2 * 85 - (5 + 3 * 5) = 150.  The alignment
    # ends at row 94 and 0-based column 200 + 90 - 1 = 289; floor((2 * 95 - 150) / 3) = 13; j0 = 289 - 95 - 13 + 1 = 182.
    w = E.stage4_window(100, 150, 201, "10S40M5D45M5S")
    assert w == {"j0": 182, "ncol": 108, "blocks": 1, "start": 18, "runs": [("D", 58, 62)]}
    w = E.stage4_window(300, 2 * 298 - 11, 5, "150M2I148M")              # j = 4 + 298 - 1 = 301, floor(15 / 3) = 5: clamped at 0
    assert w == {"j0": 0, "ncol": 302, "blocks": 3, "start": 4, "runs": [("I", 153, 153)]}
    assert E.gap_rows("10S40M5D45M5S") == [("D", 49, 49)] and E.gap_rows("150M2I148M") == [("I", 150, 151)]
    # profile, DESIGN §8.9: 100 bases forward on gene columns 51..155 with five skipped gene bases, S2 = 200 - 25 = 175:
    # floor((200 - 175) / 5) = 5, j0 = 154 - 100 - 5 + 1 = 50: the alignment starts on the window's first column
    assert E.profile_window(100, (0, 0, 0, 175, 100, 105, 1, 100, 51, 155, "0")) == {"j0": 50, "ncol": 105, "blocks": 1, "start": 0}
    # reverse strand, segment bases 11..100 on gene columns 300 down to 211: rows 0..89, j = 299, S2 = 180, j0 = 299 - 90 + 1
    assert E.profile_window(100, (0, 0, 1, 180, 90, 90, 11, 100, 300, 211, "0")) == {"j0": 210, "ncol": 90, "blocks": 1, "start": 0}
    assert E.valid_score(40) == 50 and E.valid_score(36) == 49 and E.bucket(64) == 1 and E.bucket(65) == 2 and E.bucket(512) == 8
