"""Named edge cases of one level's row copies and read log-likelihood update (rambl_amd/csrc/sc_level.hip: phase_copies /
k_level_copy, phase_update / k_level_update, mark_present / k_level_entries), for the test entry sc_update_level
(capi.Context.update_level), with an exact reference.

A case is one level on hand-made inputs: S strains in rows (37 s + 5) % 128 of the 128-row matrix, each with a node label
and an arbitrary [K][K] table of doubles; the level's entries (read id, label, `first`) at entry index e0 (1..30, other
levels' entries in front); unsorted, sparse read ids; a mixed `has`; random rows before the level with a few -inf and NaN
cells; row copies.  reference(case) restates, in numpy fp64, what the reference program does
(NonparametricClustering.cpp:343-391, Strain.cpp:73-95, as oracle/o_cluster.h spells it) -- not what the kernels do:

* the copies first: dst[0:n] = src[0:n] of the rows before the level, n = min(copy_n, n_reads);
* then the entries in order, per strain.  fresh = first and not has_before[rid] (a later occurrence of a read in the level
  has first = 0: the first occurrence entered the read), isnew = fresh;
  - a single strain symbol a against a single read symbol b: lp[a][b], with a := b when a is N; NaN when a or b is no
    symbol of the level (>= K);
  - a single strain symbol against a longer read label: -inf for a < 6 that is not N (log 0 - log comp), else NaN (-inf - -inf);
  - a longer strain label: the in-order sum of lp over the aligned suffix, walked backwards, when isnew, over the aligned
    prefix, walked forwards, otherwise; an N in the strain's label becomes the read's symbol;
  - cell = val if fresh else cell + val;
* has[rid] = 1 for every entry, after the level.

A cell is one table value or an in-order sum of table values, written or added to the old cell: every result is exact, and
the device must return it bit for bit (a NaN as a NaN).  The one cell of a copy's destination between n and 2 * ceil(n / 2)
is not asserted: the kernels copy pairs of cells, and "cells past copy_n hold nothing yet".

Each case has a check, reaches(case), on the input alone: a builder that loses the edge its name promises fails on the CPU
(tests/test_update_edges_host.py) before the device comparison (tests/test_update_edges_gpu.py) could pass for nothing.

One edge of the grid's partition has no case: a trailing workgroup of k_level_update with lo >= hi.  The launch takes
b = ceil(items / 512) workgroups (at most 1 024) and gives each per = 256 * ceil(ceil(items / b) / 256) items; for b >= 2,
items / b lies in (256, 512], so per = 512 and (b - 1) * 512 < items: every workgroup has items until the cap of 1 024
workgroups binds, at 1 024 * 512 + 1 items."""
import zlib

import numpy as np

MAXS, KMAX = 128, 16
TABLE_CAP = (160 * 1024 - 256 - 18 * 1024) // 8      # level_table_capacity(): LDS_BIG doubles (sc_level.hip)
LV_COPIES, LV_ITEMS, LV_HAS, LV_TICKED = 1, 2, 4, 64
U = 16                                                # strains per item of the plain path


def slot_of(s):
    return (37 * s + 5) % MAXS


def need(cond, what):
    if not cond:
        raise AssertionError(what)


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def S(self):
        return len(self.slot)

    @property
    def Rn(self):
        return len(self.ent_rid)

    @property
    def has_dups(self):                               # as LevelWalk::run derives them
        return any(not f for f in self.ent_first)

    @property
    def any_multi(self):
        return any(len(x) != 1 for x in self.ent_labels) or any(len(x) != 1 for x in self.strain_labels)

    def call_args(self):
        return dict(slot=self.slot, strain_labels=self.strain_labels, K=self.K, code_N=self.code_N, lpt=self.lpt, ll=self.ll, has=self.has,
                    ent_rid=self.ent_rid, ent_labels=self.ent_labels, ent_first=self.ent_first, copies=self.copies, copy_n=self.copy_n, e0=self.e0)


def build(name, S, Rn, K=6, code_N=-1, strain_labels=None, ent_labels=None, rid=None, first=None, n_reads=None, has=None,
          copies=(), copy_n=0, clean=False):
    """The case `name`: whatever is not given is drawn from the name's own random stream."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if n_reads is None:
        n_reads = 2 * (max(rid) + 1 if rid is not None else Rn) + 3
    if rid is None:
        rid = rng.choice(n_reads, Rn, replace=False).tolist()            # unsorted, sparse
    if first is None:
        first = [1] * Rn
    if has is None:
        has = (rng.random(n_reads) < 0.5).astype(np.uint8)
    if strain_labels is None:
        strain_labels = [(int(rng.integers(K)),) for _ in range(S)]
    if ent_labels is None:
        ent_labels = [(int(rng.integers(K)),) for _ in range(Rn)]
    lpt = rng.standard_normal((S, K, K)) * 5.0 - 3.0
    ll = rng.standard_normal((S, n_reads)) * 10.0 - 20.0
    if not clean:
        mark = rng.random((S, n_reads))
        ll[mark < 0.04] = -np.inf
        ll[mark > 0.95] = np.nan
    return Case(name=name, K=K, code_N=code_N, slot=[slot_of(s) for s in range(S)], strain_labels=[tuple(x) for x in strain_labels],
                lpt=lpt, n_reads=n_reads, ll=ll, has=np.asarray(has, dtype=np.uint8), e0=1 + int(rng.integers(30)), ent_rid=[int(r) for r in rid],
                ent_labels=[tuple(x) for x in ent_labels], ent_first=[int(f) for f in first], copies=[tuple(c) for c in copies], copy_n=copy_n)


# ---- the reference

def value(case, s, r, isnew):
    """What the level adds for strain s and entry r."""
    sb, rb, lp, K, N = case.strain_labels[s], case.ent_labels[r], case.lpt[s], case.K, case.code_N
    if len(sb) == 1:
        a = sb[0]
        if len(rb) == 1:
            b = rb[0]
            if a == N:
                a = b
            return lp[a][b] if a < K and b < K else np.nan
        return -np.inf if a < 6 and a != N else np.nan
    val = np.float64(0.0)
    if isnew:
        ii, jj = len(sb), len(rb)
        while ii > 0 and jj > 0:
            ii, jj = ii - 1, jj - 1
            a, b = sb[ii], rb[jj]
            if a == N:
                a = b
            val = val + lp[a][b]
    else:
        ii = jj = 0
        while ii < len(sb) and jj < len(rb):
            a, b = sb[ii], rb[jj]
            ii, jj = ii + 1, jj + 1
            if a == N:
                a = b
            val = val + lp[a][b]
    return val


def prior_matrix(case):
    m = np.zeros((MAXS, case.n_reads))
    for s, row in enumerate(case.slot):
        m[row] = case.ll[s]
    return m


def reference(case):
    """dict(ll[128][n_reads], has, isnew, free: the cells that are not asserted)."""
    before = prior_matrix(case)
    m = before.copy()
    free = np.zeros(m.shape, dtype=bool)
    n = min(case.copy_n, case.n_reads)
    for src, dst in case.copies:
        m[dst, 0:n] = before[src, 0:n]
        free[dst, n:2 * ((n + 1) // 2)] = True
    isnew = np.zeros(case.Rn, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for s, row in enumerate(case.slot):
            for r, rid in enumerate(case.ent_rid):
                fresh = bool(case.ent_first[r]) and not case.has[rid]
                isnew[r] = 1 if fresh else 0
                val = value(case, s, r, fresh)
                m[row, rid] = val if fresh else m[row, rid] + val
    has = case.has.copy()
    has[case.ent_rid] = 1
    return dict(ll=m, has=has, isnew=isnew, free=free)


def literal_cell(case, row, col):
    """One cell of the matrix after the level, from the rules alone: where the cell comes from, then every entry of the
    level that names its read, in order.  None: not asserted."""
    n = min(case.copy_n, case.n_reads)
    own = {r: s for s, r in enumerate(case.slot)}
    start = case.ll[own[row]][col] if row in own else 0.0
    for src, dst in case.copies:
        if dst == row and col < n:
            start = case.ll[own[src]][col] if src in own else 0.0
        elif dst == row and n % 2 == 1 and col == n:
            return None
    if row not in own:
        return start
    s, cell = own[row], start
    with np.errstate(all="ignore"):
        for r, rid in enumerate(case.ent_rid):
            if rid != col:
                continue
            sb, rb = case.strain_labels[s], case.ent_labels[r]
            new = bool(case.ent_first[r]) and not case.has[col]
            swap = lambda a, b: b if a == case.code_N else a          # noqa: E731
            if len(sb) == 1 and len(rb) == 1:
                a, b = swap(sb[0], rb[0]), rb[0]
                val = case.lpt[s, a, b] if max(a, b) < case.K else np.nan
            elif len(sb) == 1:
                val = -np.inf if sb[0] in (0, 1, 2, 3, 4, 5) and sb[0] != case.code_N else np.nan
            else:
                pairs = list(zip(sb[::-1], rb[::-1])) if new else list(zip(sb, rb))
                val = np.float64(0.0)
                for a, b in pairs:
                    val = val + case.lpt[s, swap(a, b), b]
            cell = val if new else cell + val
    return cell


def same_bits(got, want, free=None):
    """Indices where `got` differs from `want`: a NaN for a NaN, every other cell bit for bit."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint64) == want.view(np.uint64))
    if free is not None:
        ok = ok | free
    return np.argwhere(~ok)


def expected_done(case, wide):
    """The LV_* bits launch_level returns for the case in a run with SC_WIDE_MIN = 0 (wide) or huge."""
    on_grid = wide and not case.has_dups and not case.any_multi and case.S * case.Rn > 0
    done = (LV_ITEMS | LV_HAS if on_grid else 0) | (LV_COPIES if on_grid and case.copies else 0)
    return done | (LV_TICKED if done else 0)


# ---- what the checks share

def fresh_of(case):
    return [bool(f) and not case.has[r] for f, r in zip(case.ent_first, case.ent_rid)]


def occurrences(case):
    out = {}
    for r, rid in enumerate(case.ent_rid):
        out.setdefault(rid, []).append(r)
    return out


def base_checks(case):
    """What every case is: inside the entry's limits, rows in their slots, foreign entries in front, sparse unsorted ids, first
    = 0 exactly on a later occurrence."""
    need(1 <= case.S <= MAXS and case.Rn >= 1 and 6 <= case.K <= KMAX, "limits")
    need(case.code_N == -1 or 6 <= case.code_N < case.K, "code_N")
    need(case.S * case.K * case.K <= TABLE_CAP, "the tables fit")
    need(case.slot == [slot_of(s) for s in range(case.S)] and len(set(case.slot)) == case.S, "slots")
    need(1 <= case.e0 <= 30, "e0")
    need(all(0 <= r < case.n_reads for r in case.ent_rid), "read ids")
    if case.Rn > 2:
        need(case.ent_rid != sorted(case.ent_rid) and case.n_reads > len(set(case.ent_rid)), "unsorted and sparse read ids")
    for rid, occ in occurrences(case).items():
        need([case.ent_first[r] for r in occ] == [1] + [0] * (len(occ) - 1), "first = 0 exactly on a later occurrence")
    multi_strain = any(len(x) > 1 for x in case.strain_labels)
    for x in case.strain_labels:
        need(len(x) >= 1 and all(c < 256 for c in x) and (len(x) == 1 or all(c < case.K or c == case.code_N for c in x)), "strain label")
    for x in case.ent_labels:
        need(len(x) >= 1 and all(c < 256 for c in x) and ((len(x) == 1 and not multi_strain) or all(c < case.K for c in x)), "entry label")
    srcs, dsts = [c[0] for c in case.copies], [c[1] for c in case.copies]
    need(len(set(dsts)) == len(dsts) and not set(dsts) & set(srcs) and all(0 <= v < MAXS for v in srcs + dsts), "copies are independent")


def _plain(case):
    need(not case.has_dups and not case.any_multi, "the plain path")


# ---- the cases

EDGES = {}


def edge(name, check):
    def deco(fn):
        EDGES[name] = (fn, check)
        return fn
    return deco


def case(name):
    c = EDGES[name][0]()
    need(c.name == name, "the case carries its name")
    return c


def reaches(c):
    base_checks(c)
    EDGES[c.name][1](c)


def _add_plain(S, Rn, K=6, name=None):
    name = name or "plain_S%d_R%d" % (S, Rn)

    def check(c):
        _plain(c)
        need((c.S, c.Rn, c.K) == (S, Rn, K), "shape")
        if name.startswith("plain_S%d_R" % S):
            need(int(name.split("_R")[1]) == c.Rn and int(name.split("_")[1][1:]) == c.S, "the name's shape")
        if c.Rn > 2:
            fr = fresh_of(c)
            need(any(fr) and not all(fr), "fresh and not fresh reads")
    EDGES[name] = (lambda: build(name, S, Rn, K=K), check)


for _S in (1, 15, 16, 17, 32, 33):
    for _Rn in (1, 2, 33):
        _add_plain(_S, _Rn)


def _second_trip(S, Rn):
    name = "plain_S%d_R%d" % (S, Rn)
    _add_plain(S, Rn)
    fn, chk = EDGES[name]

    def check(c):
        chk(c)
        items = c.Rn * ((c.S + U - 1) // U)
        need(512 < items <= 514, "the items of the plain path just across one round of 512 threads")
    EDGES[name] = (fn, check)


_second_trip(1, 513)
_second_trip(17, 257)
_add_plain(128, 5, K=6, name="plain_S128_K6")
_add_plain(128, 5, K=8, name="plain_S128_K8")
CAP_S = TABLE_CAP // (KMAX * KMAX)


@edge("plain_cap_K16", lambda c: (_plain(c), need(c.K == KMAX and c.S == CAP_S and (c.S + 1) * 256 > TABLE_CAP >= c.S * 256, "the largest table that fits")))
def _cap():
    return build("plain_cap_K16", CAP_S, 3, K=KMAX)


def _add_symbols(K, code_N):
    name = "sym_K%d_N%s" % (K, "none" if code_N < 0 else str(code_N))
    strain_codes = [0, 3, 5, 6, K - 1, K, 200] + ([code_N] if code_N >= 0 else [])
    read_codes = list(range(K)) + [K, 255]

    def make():
        rng = np.random.default_rng(K * 100 + code_N + 7)
        ents = read_codes + read_codes                            # every read symbol on a fresh read and on one that is not
        rid = rng.permutation(3 * len(ents))[:len(ents)].tolist()
        has = np.zeros(3 * len(ents) + 3, dtype=np.uint8)
        has[rid[len(read_codes):]] = 1
        has[[r for r in range(len(has)) if r not in rid][::2]] = 1
        c = build(name, len(strain_codes), len(ents), K=K, code_N=code_N, strain_labels=[(a,) for a in strain_codes],
                  ent_labels=[(b,) for b in ents], rid=rid, has=has, n_reads=len(has))
        for s in range(c.S):                                      # a finite cell under the read symbols >= K that are added to
            for r in range(len(read_codes), len(ents)):
                if ents[r] >= K:
                    c.ll[s, rid[r]] = -7.5 - s
        return c

    def check(c):
        _plain(c)
        need(c.K == K and c.code_N == code_N, "alphabet")
        fr = fresh_of(c)
        sl, el = [x[0] for x in c.strain_labels], [x[0] for x in c.ent_labels]
        for b in el:
            need(sum(1 for r in range(c.Rn) if el[r] == b and fr[r]) == 1 and sum(1 for r in range(c.Rn) if el[r] == b and not fr[r]) == 1,
                 "every read symbol once fresh, once not")
        need(set(range(K)) <= set(el) and K in el and 255 in el, "every symbol of the level as a read symbol, and two that are none")
        need(K in sl and 200 in sl and K != code_N, "a strain symbol >= K that is not N")
        for s in range(c.S):
            for r in range(c.Rn):
                if el[r] >= K and not fr[r]:
                    need(np.isfinite(c.ll[s, c.ent_rid[r]]), "a NaN is added to a finite cell")
                if el[r] >= K or (sl[s] >= K and sl[s] != code_N):
                    need(np.isnan(value(c, s, r, fr[r])), "a symbol outside the alphabet gives NaN")
        if code_N >= 0:
            need(code_N in sl and code_N in el, "a strain label N and a read label N")
            s = sl.index(code_N)
            need(all(value(c, s, r, True) == c.lpt[s, el[r], el[r]] for r in range(c.Rn) if el[r] < K), "the diagonal")
            need(any(c.lpt[s, el[r], el[r]] != c.lpt[s, code_N, el[r]] for r in range(c.Rn) if el[r] < K), "the diagonal is not row N")
        else:
            need(6 in sl and 6 in el, "code 6 in use as an ordinary symbol")
            if K > 6:
                s = sl.index(6)
                need(all(value(c, s, r, True) == c.lpt[s, 6, el[r]] for r in range(c.Rn) if el[r] < K), "row 6, not the diagonal")
    EDGES[name] = (make, check)


for _K, _N in ((6, -1), (8, -1), (16, -1), (8, 6), (8, 7), (16, 6), (16, 15)):
    _add_symbols(_K, _N)


def _check_item(c):
    need(c.any_multi and not c.has_dups, "the item path")


@edge("item_513", lambda c: (_check_item(c), need(c.S * c.Rn == 513, "513 items")))
def _item_513():
    K = 8
    rng = np.random.default_rng(513)
    sl = [tuple(rng.integers(K, size=1 + int(rng.integers(3))).tolist()) for _ in range(9)]
    sl[4] = (2, 1, 3)
    el = [tuple(rng.integers(K, size=1 + int(rng.integers(4))).tolist()) for _ in range(57)]
    return build("item_513", 9, 57, K=K, strain_labels=sl, ent_labels=el)


ITEM_STRAINS = [(0,), (4,), (5,), (7,), (2,), (1, 2), (3, 0, 1), (2, 7, 4, 1), (7, 7)]      # 7: N
ITEM_READS = [(3,), (7,), (1, 2), (0, 1, 3), (5, 4), (2, 3, 4, 1, 0), (6,), (1, 6, 2), (3, 5, 0, 2)]


def _directions_differ(c, s, r):
    with np.errstate(all="ignore"):
        return value(c, s, r, True) != value(c, s, r, False)


def _check_item_mix(c):
    _check_item(c)
    need(c.K == 8 and c.code_N == 7, "alphabet")
    fr = fresh_of(c)
    pairs = [(s, r) for s in range(c.S) for r in range(c.Rn)]
    ls, lr = [len(x) for x in c.strain_labels], [len(x) for x in c.ent_labels]
    need(any(ls[s] == 1 and lr[r] == 1 for s, r in pairs), "ls = 1 against lr = 1 inside a multi-symbol level")
    for a in (0, 4, 5, 7):
        need(any(c.strain_labels[s] == (a,) and lr[r] > 1 for s, r in pairs), "ls = 1 against lr > 1 for a = %d" % a)
    for rel in (lambda x, y: x < y, lambda x, y: x == y, lambda x, y: x > y):
        for new in (True, False):
            need(any(ls[s] > 1 and lr[r] > 1 and rel(ls[s], lr[r]) and fr[r] == new and _directions_differ(c, s, r) for s, r in pairs),
                 "ls > 1 below, at and above lr, new and old, the two directions with different sums")
    need(any(ls[s] > 1 and lr[r] == 1 for s, r in pairs), "a long strain label against a single read symbol")
    need(any(ls[s] > 2 and 7 in c.strain_labels[s][1:-1] for s in range(c.S)), "N inside a long strain label")
    need(any(np.isneginf(c.ll[s, c.ent_rid[r]]) and not fr[r] and np.isfinite(value(c, s, r, False)) for s, r in pairs), "a prior cell of -inf that is added to")


@edge("item_mix", _check_item_mix)
def _item_mix():
    reads = ITEM_READS + ITEM_READS
    n = len(reads)
    rid = [(7 * r + 3) % (2 * n + 1) for r in range(n)]
    has = np.zeros(2 * n + 4, dtype=np.uint8)
    has[rid[len(ITEM_READS):]] = 1                           # every label on a read that is new and on one that is not
    has[2 * n + 2] = 1
    c = build("item_mix", len(ITEM_STRAINS), n, K=8, code_N=7, strain_labels=ITEM_STRAINS, ent_labels=reads, rid=rid, has=has, n_reads=len(has))
    c.ll[6, rid[len(ITEM_READS) + 3]] = -np.inf
    # labels of equal length meet the same pairs in either direction: (2, N, 4, 1) against (3, 5, 0, 2) adds four cells whose
    # sum depends on the order (1.0 forwards, 0.0 backwards)
    c.lpt[7, 2, 3], c.lpt[7, 5, 5], c.lpt[7, 4, 0], c.lpt[7, 1, 2] = 1e16, 1.0, -1e16, 1.0
    return c


def _check_item_six(c):
    _check_item(c)
    need(c.code_N == -1 and c.K == 8, "N absent")
    need(any(c.strain_labels[s] == (6,) and len(c.ent_labels[r]) > 1 and np.isnan(value(c, s, r, True)) for s in range(c.S) for r in range(c.Rn)),
         "a = 6 against lr > 1 with N absent")
    need(any(c.strain_labels[s] == (5,) and len(c.ent_labels[r]) > 1 and np.isneginf(value(c, s, r, True)) for s in range(c.S) for r in range(c.Rn)),
         "a = 5 beside it")


@edge("item_six_noN", _check_item_six)
def _item_six():
    return build("item_six_noN", 3, 5, K=8, strain_labels=[(6,), (5,), (6, 2)], ent_labels=[(1, 2), (6,), (3,), (6, 6, 1), (0,)])


def _add_dup(S, multi=False):
    name = "dup_multi" if multi else "dup_S%d" % S
    # entries: read A at r = 0 and r = Rn - 1 (fresh first); B three times (not fresh first); C twice, neighbours; D, E once
    order = ["A", "B", "C", "C", "D", "B", "E", "B", "A"]
    ids = dict(A=9, B=2, C=14, D=0, E=11)

    def make():
        rid = [ids[x] for x in order]
        first = [1 if order.index(x) == r else 0 for r, x in enumerate(order)]
        has = np.zeros(17, dtype=np.uint8)
        has[[ids["B"], ids["D"], 5, 16]] = 1
        if multi:
            sl = [(1, 2, 3), (4,), (0, 7), (7, 5, 2, 1)][:S]
            el = [(3, 1), (2,), (1, 2, 3, 4), (0, 5), (6,), (4, 4, 1), (2, 2), (5, 3, 0, 1, 2), (1, 2, 3)]
            return build(name, S, len(order), K=8, code_N=7, strain_labels=sl, ent_labels=el, rid=rid, first=first, has=has, n_reads=17)
        return build(name, S, len(order), K=6, rid=rid, first=first, has=has, n_reads=17)

    def check(c):
        need(c.has_dups and c.S == S and c.any_multi == multi, "the duplicate path")
        occ = occurrences(c)
        need(sorted(len(v) for v in occ.values()) == [1, 1, 2, 2, 3], "a read twice and three times")
        fr = fresh_of(c)
        firsts = [v[0] for v in occ.values() if len(v) > 1]
        need(any(fr[r] for r in firsts) and any(not fr[r] for r in firsts), "a first occurrence that is fresh, and one that is not")
        need(all(not fr[r] for v in occ.values() for r in v[1:]), "a later occurrence always adds")
        need(c.ent_rid[0] == c.ent_rid[c.Rn - 1], "occurrences at r = 0 and r = Rn - 1")
        if multi:
            ls, lr = [len(x) for x in c.strain_labels], [len(x) for x in c.ent_labels]
            need(any(ls[s] > 1 and fr[v[0]] and lr[v[0]] != ls[s] and lr[v[1]] != ls[s] and _directions_differ(c, s, v[0]) and _directions_differ(c, s, v[1])
                     for s in range(c.S) for v in occ.values() if len(v) > 1),
                 "a first occurrence walked backwards and a second forwards, where the direction changes the sum")
    EDGES[name] = (make, check)


for _S in (1, 2, 64, 128):
    _add_dup(_S)
_add_dup(4, multi=True)


def _copy_case(name, S, Rn, copies, copy_n, n_reads, **kw):
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    rid = kw.pop("rid", None) or rng.choice(n_reads, Rn, replace=False).tolist()
    return build(name, S, Rn, rid=rid, n_reads=n_reads, copies=copies, copy_n=copy_n, **kw)


FREE_ROWS = [r for r in range(MAXS) if r not in [slot_of(s) for s in range(40)]]


def _add_copies(k):
    name = "copies_%d" % k
    # sources: strains of the level and one row that is nobody's; destinations: free rows and one strain of the level
    pairs = [(slot_of(0), FREE_ROWS[3]), (slot_of(2), slot_of(4)), (FREE_ROWS[7], FREE_ROWS[8]), (slot_of(0), FREE_ROWS[20]), (slot_of(3), FREE_ROWS[1])][:k]

    def check(c):
        _plain(c)
        need(len(c.copies) == k and 0 < c.copy_n < c.n_reads, "the number of copies")
    EDGES[name] = (lambda: _copy_case(name, 6, 7, pairs, 12, 19), check)


for _k in (0, 1, 2, 5):
    _add_copies(_k)


def _check_parent_child(c):
    _plain(c)
    need((c.S, c.Rn) == (3, 5) and len(c.copies) == 1, "3 x 5 cells")
    src, dst = c.copies[0]
    need(src in c.slot and dst in c.slot, "parent and child are strains of the level")
    p, ch = c.slot.index(src), c.slot.index(dst)
    need(c.copy_n >= c.n_reads and c.n_reads % 2 == 0, "the whole row is copied")
    fr = fresh_of(c)
    need(any(not f for f in fr), "a read that is added to")
    with np.errstate(all="ignore"):
        need(any(not fr[r] and np.isfinite(c.ll[p, rid]) and c.ll[p, rid] + value(c, p, r, False) + value(c, ch, r, False) != c.ll[p, rid] + value(c, ch, r, False)
                 for r, rid in enumerate(c.ent_rid)), "the parent's updated row would give the child another cell")


@edge("copy_parent_child", _check_parent_child)
def _parent_child():
    has = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.uint8)
    return _copy_case("copy_parent_child", 3, 5, [(slot_of(0), slot_of(1))], 8, 8, rid=[6, 2, 0, 5, 3], has=has, clean=True,
                      strain_labels=[(0,), (1,), (2,)])


COPYN = dict(copyn_0=0, copyn_1=1, copyn_odd=7, copyn_even=10, copyn_all=13, copyn_over=40)


def _add_copyn(name, n):
    def check(c):
        _plain(c)
        need(c.n_reads == 13 and c.copy_n == n and len(c.copies) == 2, "copy_n")
        need(dict(copyn_0=n == 0, copyn_1=n == 1, copyn_odd=n % 2 == 1 and 1 < n < 13, copyn_even=n % 2 == 0 and 0 < n < 13, copyn_all=n == 13,
                  copyn_over=n > 13)[name], "copy_n as named")
        need(any(d in c.slot for _, d in c.copies) and any(d not in c.slot for _, d in c.copies), "a destination that is a strain, and one that is not")
    EDGES[name] = (lambda: _copy_case(name, 4, 6, [(slot_of(1), slot_of(3)), (slot_of(0), FREE_ROWS[5])], n, 13), check)


for _name, _n in COPYN.items():
    _add_copyn(_name, _n)


def _add_copy_mod(m):
    name = "copy_mod%d" % m
    n_reads = {0: 12, 1: 13, 3: 15}[m]
    dst = slot_of(0) - 1

    def check(c):
        _plain(c)
        need(c.n_reads % 4 == m and c.copy_n == c.n_reads, "n_reads mod 4, the whole row copied")
        need(c.copies[0][1] + 1 in c.slot and c.copies[0][1] not in c.slot, "the slot behind the destination holds a live strain")
        s = c.slot.index(c.copies[0][1] + 1)
        need(0 in c.ent_rid and c.has[0] and np.isfinite(c.ll[s, 0]), "whose first cell is added to")
    EDGES[name] = (lambda: _copy_case(name, 3, 5, [(slot_of(1), dst)], n_reads, n_reads, rid=[7, 0, 11, 4, 2],
                                      has=np.array(([1, 0, 1, 1] * 4)[:n_reads], dtype=np.uint8), clean=True), check)


for _m in (0, 1, 3):
    _add_copy_mod(_m)


def partition(total):
    """k_level_update's split of `total` items: (workgroups, items per workgroup)."""
    b = min(max((total + 511) // 512, 1), 1024)
    return b, ((total + b - 1) // b + 255) // 256 * 256


def _add_grid(S, Rn, name=None):
    name = name or "grid_%d" % (S * Rn)

    def check(c):
        _plain(c)
        need((c.S, c.Rn) == (S, Rn), "shape")
        if name.startswith("grid_") and name[5:].isdigit():
            need(c.S * c.Rn == int(name[5:]), "items")
        b, per = partition(c.S * c.Rn)
        if name == "grid_3013":
            crossing = [w for w in range(b) if (w * per) // c.Rn < (min((w + 1) * per, c.S * c.Rn) - 1) // c.Rn]
            need(b >= 4 and len(crossing) >= 4, "several workgroups that each cross a strain boundary")
        if name == "grid_S128_R1":
            need(b == 1 and c.S == MAXS, "one workgroup stages every strain")
    EDGES[name] = (lambda: build(name, S, Rn, K=8, code_N=6), check)


for _S, _Rn in ((1, 1), (15, 17), (16, 16), (1, 257), (7, 73), (32, 16), (27, 19), (23, 131)):
    _add_grid(_S, _Rn)
_add_grid(128, 1, name="grid_S128_R1")

NAMES = (["plain_S%d_R%d" % (s, r) for s in (1, 15, 16, 17, 32, 33) for r in (1, 2, 33)] + ["plain_S1_R513", "plain_S17_R257", "plain_S128_K6", "plain_S128_K8",
         "plain_cap_K16"] + ["sym_K6_Nnone", "sym_K8_Nnone", "sym_K16_Nnone", "sym_K8_N6", "sym_K8_N7", "sym_K16_N6", "sym_K16_N15"] +
         ["item_513", "item_mix", "item_six_noN"] + ["dup_S1", "dup_S2", "dup_S64", "dup_S128", "dup_multi"] +
         ["copies_0", "copies_1", "copies_2", "copies_5", "copy_parent_child"] + list(COPYN) + ["copy_mod0", "copy_mod1", "copy_mod3"] +
         ["grid_1", "grid_255", "grid_256", "grid_257", "grid_511", "grid_512", "grid_513", "grid_3013", "grid_S128_R1"])
