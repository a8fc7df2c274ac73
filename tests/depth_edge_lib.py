"""Named edge cases of the stage-1 depth kernel, k_depth_fused<PPL> in rambl_amd/csrc/sc_depth.hip: one wavefront per reference,
the difference array of a reference in an LDS tile of TILE cells (a longer reference tile by tile, the runs of a tile found
by binary search in its start-sorted runs inside a window of max_run cells, max_run the longest run of the whole call), the
tile scanned in steps of 64 * PPL cells (PPL cells per lane), the first FIXED intervals of a reference in slots of its own and
the rest in one shared list, a grid of at most MAX_WAVES wavefronts that stride over the references.  The constants below
restate that geometry; sc_depth.hip is their source.

A case is a function of nothing but its name.  It returns the inputs (reference lengths, 1-based inclusive runs, max_gap) and a
property check: a function of the plain reference's output that raises unless the input reaches the edge the case is named
for -- a generator that silently loses its edge fails on the CPU (tests/test_depth_edges_host.py) before the device comparison
(tests/test_depth_edges_gpu.py) could pass for nothing.  The plain reference, reference(), is numpy in int64 over the
concatenated cells of all references and knows nothing of tiles, steps or lanes."""
import numpy as np

from align_edge_lib import need

TILE = 2048                       # cells of a wavefront's LDS tile
FIXED = 2                         # intervals of a reference that have output slots of their own
MAX_WAVES = 65536 * 4             # the grid: at most 65 536 workgroups of four wavefronts
MAX_GAP_LIMIT = (1 << 30) - (1 << 24)      # the largest max_gap the entry points accept (include/straincall_hip.h)
SC_OK, SC_ERR_ARG, SC_ERR_CAPACITY = 0, -3, -5

GAPS = (3, 10, 0, 2)              # two max_gap values for each instantiation: PPL = 4 (max_gap >= 3) and PPL = 1


def ppl(max_gap):
    return 4 if max_gap >= 3 else 1


def step(max_gap):
    return 64 * ppl(max_gap)


# ---- the plain reference

def reference_arrays(ref_len, run_ref, run_start, run_end, max_gap):
    """Five int64 arrays (ref, start, end, sum, n), sorted by (ref, start); start and end 1-based inclusive."""
    ref_len = np.asarray(ref_len, dtype=np.int64)
    run_ref, run_start, run_end = (np.asarray(a, dtype=np.int64) for a in (run_ref, run_start, run_end))
    off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(ref_len, dtype=np.int64)])
    cells = int(off[-1])
    # difference array over the concatenated cells: a run that ends on a reference's last cell takes its -1 on the next
    # reference's first cell, where the depth it ends has to be gone
    diff = (np.bincount(off[run_ref] + run_start - 1, minlength=cells + 1).astype(np.int64)
            - np.bincount(off[run_ref] + run_end, minlength=cells + 1).astype(np.int64))
    depth = np.cumsum(diff, dtype=np.int64)[:cells]
    covered = depth > 0
    pos = np.flatnonzero(covered).astype(np.int64)
    if pos.size == 0:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(5))
    ref = np.searchsorted(off, pos, side="right").astype(np.int64) - 1          # a reference of no cells owns no position
    p = pos - off[ref] + 1
    brk = np.ones(pos.size, dtype=bool)
    brk[1:] = (ref[1:] != ref[:-1]) | (pos[1:] - pos[:-1] - 1 > max_gap)
    first = np.flatnonzero(brk)
    last = np.concatenate([first[1:], [pos.size]]) - 1
    sums = np.add.reduceat(depth[pos], first)
    counts = np.add.reduceat(np.ones(pos.size, dtype=np.int64), first)
    return ref[first], p[first], p[last], sums.astype(np.int64), counts.astype(np.int64)


def reference(ref_len, run_ref, run_start, run_end, max_gap):
    """-> [(ref, start, end, sum, n)]"""
    return list(zip(*(a.tolist() for a in reference_arrays(ref_len, run_ref, run_start, run_end, max_gap))))


# ---- cases

class DepthCase:
    def __init__(self, name, ref_len, runs, max_gap, check):
        """runs: (ref, start, end) int arrays of equal length, or a list of such triples; 1-based inclusive."""
        self.name, self.max_gap, self.check = name, max_gap, check
        self.ref_len = np.asarray(ref_len, dtype=np.int32).reshape(-1)
        if isinstance(runs, list):
            runs = tuple(np.asarray([r[k] for r in runs], dtype=np.int32) for k in range(3))
        self.run_ref, self.run_start, self.run_end = (np.asarray(a, dtype=np.int32).reshape(-1) for a in runs)

    @property
    def n_refs(self):
        return int(self.ref_len.size)

    @property
    def n_runs(self):
        return int(self.run_ref.size)

    def key(self):
        return (self.max_gap, self.ref_len.tobytes(), self.run_ref.tobytes(), self.run_start.tobytes(), self.run_end.tobytes())

    def reference_arrays(self):
        return reference_arrays(self.ref_len, self.run_ref, self.run_start, self.run_end, self.max_gap)

    def reference(self):
        return reference(self.ref_len, self.run_ref, self.run_start, self.run_end, self.max_gap)


def per_ref(out, n_refs):
    """The reference's output split by reference: [[(start, end, sum, n)]]."""
    by = [[] for _ in range(n_refs)]
    for r, s, e, sm, n in out:
        by[r].append((s, e, sm, n))
    return by


def _cells(ref, positions):
    """one-base runs on the 0-based cells `positions` of reference `ref`"""
    return [(ref, p + 1, p + 1) for p in positions]


def gap_seams(max_gap):
    """Pairs of one-base runs `max_gap` (merge) and `max_gap + 1` (split) uncovered cells apart whose two cells lie on opposite
    sides of a seam of the kernel: two lanes of one step, two steps of one tile, two tiles.  Reference 0 (three tiles) holds
    a merging and a splitting pair for each kind; references 1 and 2 have coverage in tiles 0 and 2 only, 2 048 and 2 049
    uncovered cells apart: the whole of tile 1 is empty, and with max_gap = 2048 reference 1 still is one interval.  With
    max_gap = 2048 no pair fits a step or reference 0, which stays empty."""
    g, st, P = max_gap, step(max_gap), ppl(max_gap)
    pairs = []                                   # (kind, merges, x, y), 0-based cells of reference 0
    if g + 3 < st // 4:
        for kind, merge_at, split_at in (("lane", st // 8, st // 2), ("step", st, 3 * st), ("tile", TILE, 2 * TILE)):
            for merges, b in ((True, merge_at), (False, split_at)):
                x = b - 1 - g // 2
                pairs.append((kind, merges, x, x + g + (1 if merges else 2)))
    runs = _cells(0, sorted(c for _, _, x, y in pairs for c in (x, y)))
    runs += _cells(1, [TILE - 1, 2 * TILE]) + _cells(2, [TILE - 2, 2 * TILE])
    side = {"lane": lambda c: c // P, "step": lambda c: c // st, "tile": lambda c: c // TILE}
    inside = {"lane": lambda c: c // st, "step": lambda c: c // TILE, "tile": lambda c: 0}

    def check(out):
        by = per_ref(out, 3)
        for kind, merges, x, y in pairs:
            need(side[kind](x) != side[kind](y) and inside[kind](x) == inside[kind](y), "%s seam between %d and %d" % (kind, x, y))
            if merges:
                need((x + 1, y + 1, 2, 2) in by[0], "%s seam: %d and %d merge" % (kind, x, y))
            else:
                need((x + 1, x + 1, 1, 1) in by[0] and (y + 1, y + 1, 1, 1) in by[0], "%s seam: %d and %d split" % (kind, x, y))
        need(len(by[0]) == 3 * len(pairs) // 2, "the pairs of reference 0 do not disturb each other")
        need(len(pairs) == (0 if g >= TILE else 6), "a merging and a splitting pair at every kind of seam")
        need(by[1] == ([(TILE, 2 * TILE + 1, 2, 2)] if g >= TILE else [(TILE, TILE, 1, 1), (2 * TILE + 1, 2 * TILE + 1, 1, 1)]),
             "tile 1 of reference 1 is empty: one interval iff max_gap >= 2048")
        need(by[2] == [(TILE - 1, TILE - 1, 1, 1), (2 * TILE + 1, 2 * TILE + 1, 1, 1)], "2 049 uncovered cells split")
    return DepthCase("gap_seams[%d]" % g, [3 * TILE] * 3, runs, g, check)


def many_starts(max_gap):
    """Every (max_gap + 2)-th cell covered, so that every covered cell starts an interval: with max_gap = 0 alternating cells
    (32 starts per step of 64), with max_gap = 3 every fifth cell (51 or 52 per step of 256).  References of 2 048, 2 049 and
    three times 2 048 cells; all but FIXED of a reference's intervals go to the shared list."""
    g, st = max_gap, step(max_gap)
    need(g in (0, 3), "many_starts is defined for max_gap 0 and 3")
    lens = [TILE, TILE + 1, 3 * TILE]
    runs = [r for k, ln in enumerate(lens) for r in _cells(k, range(0, ln, g + 2))]

    def check(out):
        by = per_ref(out, len(lens))
        for k, ln in enumerate(lens):
            need(by[k] == [(p + 1, p + 1, 1, 1) for p in range(0, ln, g + 2)], "every covered cell is an interval of its own")
            per_step = np.bincount(np.array([s - 1 for s, _, _, _ in by[k]]) // st)
            need(per_step.max() >= 30 and per_step[:ln // st].min() >= 30, "30 and more interval starts in every whole step")
        need(by[1][-1][0] == TILE + 1 if g == 0 else by[1][-1][0] == TILE - 2, "the last cell of the 2 049-cell reference")
        need(max(len(b) for b in by) - FIXED >= 1000, "the shared list takes 1 000 and more intervals from one wavefront")
        if g == 0:
            need(len(by[0]) - FIXED >= 1000, "... from the one-tile reference already")
    return DepthCase("many_starts[%d]" % g, lens, runs, g, check)


def fixed_slots(max_gap):
    """References with 0, 1, 2, 3 and then 3, 2, 1, 0 intervals: either side of the FIXED = 2 slots of a reference."""
    g = max_gap
    counts = [0, 1, 2, 3, 3, 2, 1, 0]
    runs = [(k, 2 + j * (g + 4), 4 + j * (g + 4)) for k, c in enumerate(counts) for j in range(c)]

    def check(out):
        need([len(b) for b in per_ref(out, len(counts))] == counts, "0 1 2 3 3 2 1 0 intervals")
        need(FIXED == 2, "the counts straddle FIXED")
    return DepthCase("fixed_slots[%d]" % g, [3 * (g + 4) + 5] * len(counts), runs, g, check)


def _long_runs_inputs():
    T = TILE
    ref_len = [6200, 3 * T, 3 * T]
    # the runs the tiles' seams ask for, 1-based: ending on a tile's last cell, starting on a tile's first, exactly tile 1,
    # ending on tile 1's first cell
    seams = [(T - 48, T), (2 * T - 96, 2 * T), (T + 1, T + 52), (2 * T + 1, 2 * T + 104), (T + 1, 2 * T), (T - 8, T + 1)]
    runs = [(0, 1, 6000)] + [(0, s, e) for s, e in seams] + [(0, 30, 90), (0, 3000, 3000), (0, 5990, 6100), (0, 6200, 6200)]
    # reference 1: the depth of 1500..4500 is carried through tile 1, in which no run starts
    runs += [(1, 1500, 4500), (1, 100, 150), (1, 1990, T), (1, 2 * T + 1, 2 * T + 4), (1, 5000, 5050), (1, 6100, 3 * T)]
    runs += [(2, s, e) for s, e in seams] + [(2, 10, 20), (2, 25, 25), (2, 6000, 6010)]
    return ref_len, runs


def _long_runs_check(case_runs):
    T = TILE

    def check(out):
        by = per_ref(out, 3)
        rr, rs, re = case_runs
        need(any((s - 1) // T + 2 <= (e - 1) // T for s, e in zip(rs, re)), "a run over a whole tile it neither starts nor ends in")
        need(any(e % T == 0 for e in re) and any(s % T == 1 and s > 1 for s in rs), "a run ending on a tile's last cell, one starting on a first")
        need(any(s == T + 1 and e == 2 * T for s, e in zip(rs, re)) and any(e == T + 1 for e in re), "exactly tile 1; ending on its first cell")
        need(max(e - s + 1 for s, e in zip(rs, re)) >= 2 * T, "max_run is above c0 for tiles 1 and 2: lo_key = 0")
        tile1 = [(r, s) for r, s in zip(rr, rs) if r == 1 and T < s <= 2 * T]
        need(not tile1 and any(s <= T + 1 and e >= 2 * T and sm > n for s, e, sm, n in by[1]), "tile 1 of reference 1: depth carried, no run start")
        need(by[0][0][0] == 1 and by[0][0][1] >= 6000 and by[0][0][2] > by[0][0][3] >= 6000, "reference 0 is covered from 1 to 6000 and deeper than 1")
        need(by[0][-1][1] == 6200 and by[1][-1][1] == 3 * T, "runs reach the ends of references 0 and 1")
    return check


def long_runs(max_gap):
    """Runs longer than a tile, and runs that begin and end exactly on the cells next to a tile's seam."""
    ref_len, runs = _long_runs_inputs()
    case = DepthCase("long_runs[%d]" % max_gap, ref_len, runs, max_gap, None)
    case.check = _long_runs_check((case.run_ref.tolist(), case.run_start.tolist(), case.run_end.tolist()))
    return case


def unsorted_input(max_gap):
    """The inputs of long_runs with the runs of the three references interleaved and those of each reference by descending
    start: the bucketing by reference and the start order inside a long reference are the library's work."""
    base = long_runs(max_gap)
    rank = np.zeros(base.n_runs, dtype=np.int64)
    for r in range(base.n_refs):
        at = np.flatnonzero(base.run_ref == r)
        rank[at[np.argsort(-base.run_start[at].astype(np.int64), kind="stable")]] = np.arange(at.size)
    order = np.lexsort((base.run_ref, rank))
    runs = (base.run_ref[order], base.run_start[order], base.run_end[order])

    def check(out):
        rr, rs = runs[0].tolist(), runs[1].tolist()
        need(any(a > b for a, b in zip(rr, rr[1:])), "the references are interleaved")
        for r in range(base.n_refs):
            mine = [s for q, s in zip(rr, rs) if q == r]
            need(len(mine) > 2 and all(a >= b for a, b in zip(mine, mine[1:])) and mine[0] > mine[-1], "descending starts")
        need(out == base.reference(), "the same intervals as long_runs")
        base.check(out)
    return DepthCase("unsorted_input[%d]" % max_gap, base.ref_len, runs, max_gap, check)


RUN_TO_THE_END_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]


def run_to_the_end(max_gap):
    """Every length either side of a lane's four cells, a step and a tile: once covered by one run, once at its last cell only."""
    lens = [ln for ln in RUN_TO_THE_END_LENGTHS for _ in range(2)]
    runs = [(k, 1 if k % 2 == 0 else ln, ln) for k, ln in enumerate(lens)]

    def check(out):
        by = per_ref(out, len(lens))
        for k, ln in enumerate(lens):
            need(by[k] == [(1 if k % 2 == 0 else ln, ln, ln if k % 2 == 0 else 1, ln if k % 2 == 0 else 1)], "one interval that ends at ref_len")
    return DepthCase("run_to_the_end[%d]" % max_gap, lens, runs, max_gap, check)


def search_window(max_gap):
    """The low edge of a tile's run window, c0 - max_run with max_run = 300 the longest run of the call.  Reference 0 (5 000
    cells) has a run of max_run cells from 0-based 2048 - max_run, which ends on cell 2047 and must not touch tile 1, and one
    from 2048 - max_run + 1, which must touch its first cell; the same pair in front of tile 2, the first of them 200 times
    with lengths 1..200 (equal starts at the window's low edge, inside tile 1).  Reference 1 is short and holds a run of 300
    cells of its own.  Reference 2 (5 000 cells) has no run longer than 100, so its windows are three times wider than its
    runs need: max_run is the call's, not the reference's.
    (Two runs of max_run cells in a reference whose longest run is shorter than max_run cannot be; references 0 and 2 share
    the two demands.)"""
    T, M = TILE, 300
    runs = [(0, T - M + 1, T), (0, T - M + 2, T + 1)]                                   # 1-based: 0-based start + 1
    runs += [(0, 2 * T - M + 1, 2 * T - M + k) for k in range(1, 201)]
    runs += [(0, 2 * T - M + 1, 2 * T), (0, 2 * T - M + 2, 2 * T + 1), (0, 40, 60), (0, 4990, 5000)]
    runs += [(1, 1, M)]
    runs += [(2, T - 100 + 1, T), (2, T - 100 + 2, T + 1), (2, T - M + 1, T - M + 30), (2, 2 * T - 49, 2 * T + 50), (2, 2 * T + 400, 2 * T + 410)]

    def check(out):
        by = per_ref(out, 3)
        longest = [max(e - s + 1 for r, s, e in runs if r == k) for k in range(3)]
        need(longest == [M, M, 100] and 300 < T, "max_run = 300, also in the short reference; reference 2's longest run is 100")
        for c0 in (T, 2 * T):
            need((0, c0 - M + 1, c0) in runs and (0, c0 - M + 2, c0 + 1) in runs, "the pair at the window's low edge of tile %d" % (c0 // T))
            depth_at_seam = [sum(1 for r, s, e in runs if r == 0 and s <= p <= e) for p in (c0, c0 + 1, c0 + 2)]
            need(depth_at_seam == [2, 1, 0], "depth 2 on the tile's last cell, 1 on the next tile's first, 0 behind it")
            if max_gap < 100:
                need(any(e == c0 + 1 for s, e, _, _ in by[0]), "an interval of reference 0 ends on the first cell of tile %d" % (c0 // T))
        need(sum(1 for r, s, e in runs if r == 0 and s == 2 * T - M + 1) == 201, "200 and one runs with the same start")
        need(any(e == T + 1 for s, e, _, _ in by[2]) or max_gap >= 100, "reference 2: a run touches tile 1's first cell")
    return DepthCase("search_window[%d]" % max_gap, [5000, M, 5000], runs, max_gap, check)


def stale_tile(max_gap):
    """A full tile of depth 50, then a last tile of 37 cells with two covered cells: what tile 0 left in LDS behind cell 37
    must not be scanned, and the depth in front of tile 1 is 0."""
    T = TILE
    runs = [(0, 1, T)] * 50 + [(0, T + 1, T + 1), (0, T + 37, T + 37)]

    def check(out):
        need(max_gap < 35, "the two cells of tile 1 are 35 uncovered cells apart")
        need(out == [(0, 1, T + 1, 50 * T + 1, T + 1), (0, T + 37, T + 37, 1, 1)], "depth 50 over tile 0, depth 1 on cells 2049 and 2085")
    return DepthCase("stale_tile[%d]" % max_gap, [T + 37], runs, max_gap, check)


def grid_stride():
    """MAX_WAVES + 512 references of 1 to 8 cells: wavefronts 0..511 take a second reference.  The first MAX_WAVES have three
    one-base intervals (cells 1, 3, 5) where five cells fit, else one run over all their cells; of the last 512 every second
    has one run on its first cell -- behind a reference of three intervals -- and the others none."""
    n = MAX_WAVES + 512
    idx = np.arange(n)
    ref_len = np.array([1, 5, 2, 6, 3, 7, 4, 8], dtype=np.int32)[idx % 8]
    head = idx < MAX_WAVES
    three = np.flatnonzero(head & (ref_len >= 5))
    full = np.flatnonzero(head & (ref_len < 5))
    one = np.flatnonzero(~head & (idx % 2 == 1))
    run_ref = np.concatenate([np.repeat(three, 3), full, one])
    run_start = np.concatenate([np.tile([1, 3, 5], three.size), np.ones(full.size, dtype=np.int64), np.ones(one.size, dtype=np.int64)])
    run_end = np.concatenate([np.tile([1, 3, 5], three.size), ref_len[full], np.ones(one.size, dtype=np.int64)])
    order = np.argsort(run_ref, kind="stable")

    def check(out):
        need(n > MAX_WAVES, "more references than wavefronts")
        refs = np.array([o[0] for o in out], dtype=np.int64)
        count = np.bincount(refs, minlength=n)
        need(set(count[:MAX_WAVES].tolist()) == {1, 3} and set(count[MAX_WAVES:].tolist()) == {0, 1}, "1 or 3, then 0 or 1 intervals")
        need(bool(np.all(count[:512] != count[MAX_WAVES:])), "a wavefront's second reference has another interval count than its first")
        need(bool(np.all(count[:512][count[MAX_WAVES:] == 1] == 3)), "the one-cell references follow three intervals ending on cell 5")
    return DepthCase("grid_stride", ref_len, (run_ref[order], run_start[order], run_end[order]), 0, check)


def deep_sum(max_gap, n_runs=1_100_000):
    """One reference of 2 000 cells under 1 100 000 identical runs: the depth of a cell is above 2^20 and the interval's
    sum above 2^31.  (`n_runs` is for the CPU test, which compares a thousandth of it with the oracle.)"""
    run_ref = np.concatenate([np.zeros(n_runs, dtype=np.int32), [1]])
    run_start = np.concatenate([np.ones(n_runs, dtype=np.int32), [7]])
    run_end = np.concatenate([np.full(n_runs, 2000, dtype=np.int32), [9]])

    def check(out):
        need(out == [(0, 1, 2000, 2000 * n_runs, 2000), (1, 7, 9, 3, 3)], "one interval per reference")
        if n_runs == 1_100_000:
            need(out[0][3] > 2 ** 31 and out[0][3] // out[0][4] > 2 ** 20, "a sum above 2^31 from depths above 2^20")
    return DepthCase("deep_sum[%d]" % max_gap, [2000, 50], (run_ref, run_start, run_end), max_gap, check)


def deep_lane_sum(max_gap, n_runs=1_100_000):
    """The same depth over 64 tiles.  In deep_sum the interval's sum passes 2^31 only where the lanes' parts are added up;
    a lane keeps the sum of its own cells while an interval stays open, 32 cells of every tile for either PPL, and here that
    part alone passes 2^31: 64 * 32 cells under 1 100 000 runs.  Tiles times runs is what the kernel has to walk, and 2^31 / 32
    is its least value; 64 tiles keep the runs of deep_sum.  (`n_runs` is for the CPU test, as in deep_sum.)"""
    tiles = 64
    ln = tiles * TILE
    runs = (np.zeros(n_runs, dtype=np.int32), np.ones(n_runs, dtype=np.int32), np.full(n_runs, ln, dtype=np.int32))

    def check(out):
        need(out == [(0, 1, ln, ln * n_runs, ln)], "one interval")
        need(TILE % step(max_gap) == 0 and ln // 64 == 32 * tiles, "every lane scans 32 cells of every tile")
        if n_runs == 1_100_000:
            need(ln // 64 * n_runs > 2 ** 31 and tiles * n_runs < 1.05 * 2 ** 31 / 32, "a lane's part above 2^31, at little more than the least cost")
    return DepthCase("deep_lane_sum[%d]" % max_gap, [ln], runs, max_gap, check)


def empties_no_refs():
    def check(out):
        need(out == [], "no reference, no interval")
    return DepthCase("empties_no_refs", [], [], 10, check)


def empties_no_runs():
    def check(out):
        need(out == [], "no run, no interval")
    return DepthCase("empties_no_runs", [100, 2049, 1], [], 10, check)


def empties_zero_length():
    """References of no cells in front of, between and behind covered ones."""
    lens = [0, 30, 0, 0, 2049, 0]
    runs = [(1, 30, 30), (1, 1, 2), (4, 2049, 2049), (4, 2040, 2045)]

    def check(out):
        need(out == [(1, 1, 2, 2, 2), (1, 30, 30, 1, 1), (4, 2040, 2049, 7, 7)] and lens.count(0) == 4, "the empty references are skipped")
    return DepthCase("empties_zero_length", lens, runs, 10, check)


def _cases():
    out = {}
    for g in GAPS:
        for f in (gap_seams, fixed_slots, long_runs, run_to_the_end, search_window, unsorted_input, stale_tile):
            out["%s[%d]" % (f.__name__, g)] = (lambda f=f, g=g: f(g))
    out["gap_seams[2048]"] = lambda: gap_seams(2048)
    out["many_starts[0]"] = lambda: many_starts(0)
    out["many_starts[3]"] = lambda: many_starts(3)
    out["deep_sum[10]"] = lambda: deep_sum(10)
    out["deep_sum[0]"] = lambda: deep_sum(0)
    out["deep_lane_sum[10]"] = lambda: deep_lane_sum(10)
    out["deep_lane_sum[0]"] = lambda: deep_lane_sum(0)
    for f in (grid_stride, empties_no_refs, empties_no_runs, empties_zero_length):
        out[f.__name__] = f
    return out


CASES = _cases()
LARGE = ("grid_stride", "deep_sum[10]", "deep_sum[0]", "deep_lane_sum[10]", "deep_lane_sum[0]")           # too large for the oracle's Python loops


# ---- the device call (ctypes)

class ScanResult:
    def __init__(self, rc, n, arrays, stats):
        self.rc, self.n, self.arrays, self.stats = rc, n, arrays, stats

    def rows(self):
        return list(zip(*(a[:self.n].tolist() for a in self.arrays)))


def scan_runs(ref_len, run_ref, run_start, run_end, max_gap, cap, n_before=-7):
    """sc_depth_scan_runs on device 0 with output arrays of `cap` entries: ScanResult(rc, *n_intervals, the five columns as
    int64 arrays of cap entries, the sc_depth_stats).  *n_intervals holds `n_before` and stats.kernel_ms -1 before the call."""
    import ctypes as C
    from rambl_amd import capi, stage1
    lib = capi.lib()
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)

    def padded(a):                                 # never a null pointer, whatever the length
        a = np.asarray(a, dtype=np.int32).reshape(-1)
        return np.ascontiguousarray(a) if a.size else np.zeros(1, dtype=np.int32)
    n_refs, n_runs = int(np.asarray(ref_len).size), int(np.asarray(run_ref).size)
    ins = [padded(a) for a in (ref_len, run_ref, run_start, run_end)]
    iv = [np.full(max(cap, 1), -1, dtype=np.int32) for _ in range(3)]
    sm = np.full(max(cap, 1), -1, dtype=np.int64)
    cn = np.full(max(cap, 1), -1, dtype=np.int32)
    n = C.c_int(n_before)
    st = stage1.DepthStats()
    st.kernel_ms = -1.0
    rc = lib.sc_depth_scan_runs(0, ins[0].ctypes.data_as(ip), n_refs, ins[1].ctypes.data_as(ip), ins[2].ctypes.data_as(ip),
                                ins[3].ctypes.data_as(ip), n_runs, max_gap, iv[0].ctypes.data_as(ip), iv[1].ctypes.data_as(ip),
                                iv[2].ctypes.data_as(ip), sm.ctypes.data_as(lp), cn.ctypes.data_as(ip), cap, C.byref(n), C.byref(st))
    arrays = (iv[0].astype(np.int64), iv[1].astype(np.int64), iv[2].astype(np.int64), sm, cn.astype(np.int64))
    return ScanResult(rc, n.value, arrays, st)


def scan_case(case, cap, max_gap=None):
    return scan_runs(case.ref_len, case.run_ref, case.run_start, case.run_end, case.max_gap if max_gap is None else max_gap, cap)


def first_difference(got, exp):
    """None when the five columns agree, else a message with the first row that differs."""
    if len(got[0]) != len(exp[0]):
        k = min(len(got[0]), len(exp[0]))
    else:
        bad = np.zeros(len(exp[0]), dtype=bool)
        for a, b in zip(got, exp):
            bad |= np.asarray(a) != np.asarray(b)
        if not bad.any():
            return None
        k = int(np.flatnonzero(bad)[0])
    row = lambda cols, i: tuple(int(c[i]) for c in cols) if i < len(cols[0]) else None
    for i in range(k):
        if row(got, i) != row(exp, i):
            k = i
            break
    return "%d intervals, expected %d; row %d: got %s, expected %s" % (len(got[0]), len(exp[0]), k, row(got, k), row(exp, k))


# ---- SAM text for the CIGAR walk of sc_depth_scan

def sam_text(refs, records):
    """refs: [(name, length)] of the header; records: [(flag, name, pos, cigar)] -> SAM text (eleven fields, SEQ and QUAL '*')."""
    lines = ["@SQ\tSN:%s\tLN:%d" % r for r in refs]
    lines += ["r%d\t%d\t%s\t%d\t30\t%s\t*\t0\t0\t*\t*" % (k, flag, name, pos, cigar) for k, (flag, name, pos, cigar) in enumerate(records)]
    return "\n".join(lines) + "\n"


def by_name(records):
    """the oracle's view of a file: {name: [(flag, pos, cigar)]}"""
    out = {}
    for flag, name, pos, cigar in records:
        out.setdefault(name, []).append((flag, pos, cigar))
    return out
