"""The Polya-urn sampler draw by draw: one sampler level through the production kernel (k_level_sample, via the test
entry sc_sample_level) on chosen inputs and CHOSEN UNIFORMS, compared with the oracle's draw loop (oracle_urn_draws,
the loop of np_bayes_clustering in long double) for exact equality of the draws per strain and per (strain, symbol).

The kernel decides a draw in one of three tiers (rambl_amd/csrc/sc_sampler.hpp, urn_chain_q): a speculative fp32
window with one-sided margins, an fp64 scan with a 1e-10 * T margin (slow_draw) and the literal evaluation of the
reference's formula (exact_draw).  A wrong margin, lane or row index shows only when a uniform lands in the sliver it
gets wrong, which seeded data practically never does.  So the uniforms here are placed at known distances from the
boundaries of the sequential chain: `Walk` replays the oracle's arithmetic in numpy long double (the same x87 format),
and every crafted draw is checked to take the intended side in the oracle before the device is asked.

Distances delta are relative to the total weight T: 1e-2, 2 * EPSW, EPSW / 10, 1e-7, 1e-9, 1e-11, on both sides,
EPSW = (16 * NB + 16) * 1.5e-7 the window margin of the kernel variant (NB = ceil(S / 16)).  The inputs are shared
fp64, the device's fp64 and the reference's long double differ by ~1e-13: 1e-11 is the finest class asserted."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sc_testlib as T  # noqa: E402

LD = np.longdouble
KMAX = 16
MAX_DRAWS = 40000
DELTAS_ASSERTED = ("1e-2", "2eps", "eps/10", "1e-7", "1e-9", "1e-11")


def nb_of(S):
    return min(max((S + 15) // 16, 1), 8)


def epsw(S):
    return (16 * nb_of(S) + 16) * 1.5e-7


def delta_value(name, S):
    return {"1e-2": 1e-2, "2eps": 2 * epsw(S), "eps/10": epsw(S) / 10, "1e-7": 1e-7, "1e-9": 1e-9, "1e-11": 1e-11}[name]


def window_of(S):
    return 16 * (8 if nb_of(S) <= 2 else 4)


# ---------------------------------------------------------------------------------------------------------------------
# a level and the two ways of drawing it

class Level:
    """S strains, n_reads reads (rows ll[s][r], presence has[r]), the level's entries (read, copy number, symbol) in
    order; mates[r] lists the mate ids of read r (copy k of the read draws with mate mates[r][k])."""

    def __init__(self, a0, ll, has, ent_rid, ent_cn, ent_sym, mates, e0=7):
        self.a0 = np.asarray(a0, dtype=np.float64)
        self.ll = np.ascontiguousarray(ll, dtype=np.float64)
        self.S, self.n_reads = self.ll.shape
        self.has = np.asarray(has, dtype=np.uint8)
        self.ent_rid, self.ent_cn, self.ent_sym = list(ent_rid), list(ent_cn), list(ent_sym)
        self.mates = [list(m) for m in mates] + [[] for _ in range(self.n_reads - len(mates))]
        self.e0 = e0
        rid, uid, sym = [], [], []
        for r, cn, sy in zip(self.ent_rid, self.ent_cn, self.ent_sym):      # copies cn .. 1 (phase_slots, :161-167)
            for i in range(cn):
                k = cn - 1 - i
                rid.append(r)
                uid.append(self.mates[r][k] if k < len(self.mates[r]) else -1)
                sym.append(sy)
        self.rid = np.array(rid, dtype=np.int32)
        self.uid = np.array(uid, dtype=np.int32)
        self.sym = np.array(sym, dtype=np.int32)
        self.Q = len(rid)


def oracle_draws(lv, n_sweeps, U):
    lib = T.oracle_lib()
    P = ctypes.POINTER
    lib.oracle_urn_draws.argtypes = [ctypes.c_int, P(ctypes.c_double), ctypes.c_int, P(ctypes.c_double), P(ctypes.c_ubyte),
                                     ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int), P(ctypes.c_int), ctypes.c_int,
                                     ctypes.c_int, P(ctypes.c_double), P(ctypes.c_int), P(ctypes.c_long), P(ctypes.c_long)]
    total = n_sweeps * lv.Q
    U = np.ascontiguousarray(U[:total], dtype=np.float64)
    choice = np.zeros(total, dtype=np.int32)
    kdraw = np.zeros(lv.S, dtype=np.int64)
    cnt = np.zeros((lv.S, KMAX), dtype=np.int64)

    def p(x, t):
        return x.ctypes.data_as(P(t))
    rc = lib.oracle_urn_draws(lv.S, p(lv.a0, ctypes.c_double), lv.n_reads, p(lv.ll, ctypes.c_double), p(lv.has, ctypes.c_ubyte),
                              lv.Q, p(lv.rid, ctypes.c_int), p(lv.uid, ctypes.c_int), p(lv.sym, ctypes.c_int), KMAX,
                              n_sweeps, p(U, ctypes.c_double), p(choice, ctypes.c_int), p(kdraw, ctypes.c_long),
                              p(cnt, ctypes.c_long))
    assert rc == 0
    return choice, kdraw, cnt


class Walk:
    """The sequential chain of the oracle replayed in numpy long double (x87, as the oracle and the reference): the
    cumulative probabilities cp[] every draw compares its uniform with, exactly as the reference forms them."""

    def __init__(self, lv):
        self.lv = lv
        with np.errstate(all="ignore"):
            ll = lv.ll.astype(LD)
            has = lv.has != 0
            self.xr = np.where(has[lv.rid][:, None], ll[:, lv.rid].T, LD(0))                 # [Q][S]
            hu = (lv.uid >= 0) & has[np.maximum(lv.uid, 0)]
            self.hu = hu
            self.xu = ll[:, np.maximum(lv.uid, 0)].T
        self.a = lv.a0.astype(LD)

    def cp(self, q, a=None):
        a = self.a if a is None else a
        with np.errstate(all="ignore"):
            p = a / np.cumsum(a)[-1]
            y = np.log(p) + self.xr[q]
            if self.hu[q]:
                y = y + self.xu[q]
            w = np.exp(y).astype(np.float64)
            prob = w / np.cumsum(w)[-1]
            cp = np.cumsum(prob)
        cp[-1] = 1.0
        return cp

    @staticmethod
    def lower_bound(cp, u):
        lo, n = 0, len(cp)
        while n > 0:
            half = n >> 1
            mid = lo + half
            if cp[mid] < u:
                lo, n = mid + 1, n - half - 1
            else:
                n = half
        return lo

    def run(self, total, choose):
        """choose(t, q, cp, walk) -> u.  Returns (U, choices)."""
        U = np.zeros(total)
        ch = np.zeros(total, dtype=np.int32)
        for t in range(total):
            q = t % self.lv.Q
            cp = self.cp(q)
            u = choose(t, q, cp, self)
            U[t] = u
            c = self.lower_bound(cp, u)
            ch[t] = c
            self.a[c] += 1
        return U, ch


def craft(cp, delta, side, rng, clean=True):
    """A uniform at distance delta below (side -1: draws strain j) or above (side +1: draws strain j + 1) a boundary
    cp[j], j < S - 1, where the strain drawn has room (weight >= 2 delta when `clean`, so that no other boundary is
    nearer).  Returns (u, intended strain) or None."""
    S = len(cp)
    lo = np.concatenate([[0.0], cp[:-1]])
    width = cp - lo                                   # probability of strain s as the chain sees it
    need = 2 * delta if clean else 0.0
    if side < 0:
        js = [j for j in range(S - 1) if width[j] > max(need, 0.0) and cp[j] - delta > lo[j]]
    else:
        js = [j for j in range(S - 1) if width[j + 1] > max(need, 0.0) and cp[j] + delta <= 1.0]
    if not js:
        return None
    j = js[rng.integers(len(js))]
    u = cp[j] - delta if side < 0 else cp[j] + delta
    want = j if side < 0 else j + 1
    return float(u), want


def clear_uniform(cp, delta, rng):
    """A uniform at least delta (relative) from every boundary cp[0..S-2]."""
    b = np.concatenate([[-1.0], np.sort(cp[:-1]), [2.0]])
    lo = np.maximum(b[:-1] + delta, 0.0)
    hi = np.minimum(b[1:] - delta, 1.0 - 2.0 ** -53)
    ok = np.nonzero(hi > lo)[0]
    assert len(ok), "no room for a clear uniform"
    i = ok[rng.integers(len(ok))]
    return float(lo[i] + (hi[i] - lo[i]) * rng.random())


# ---------------------------------------------------------------------------------------------------------------------
# level generators

def make_level(rng, S, n_ent, cn_max=1, mate_frac=0.0, has_frac=1.0, spread=6.0, e0=7, n_extra=None, a0=None,
               symbols=6):
    """Reads 0..n_ent-1 in the level (one entry each), n_extra more reads that only mates and the entries in front of
    e0 name: distinct rows throughout."""
    n_extra = max(e0, 8) if n_extra is None else n_extra
    n_reads = n_ent + n_extra
    ll = -rng.random((S, n_reads)) * spread - 0.5
    ll[:, n_ent:] -= rng.random((S, n_extra)) * 20.0                 # rows of reads outside the level look nothing alike
    has = (rng.random(n_reads) < has_frac).astype(np.uint8)
    cn = rng.integers(1, cn_max + 1, n_ent)
    mates = []
    for r in range(n_reads):
        m = []
        if r < n_ent and rng.random() < mate_frac:
            for _ in range(int(rng.integers(1, cn[r] + 1))):
                m.append(int(rng.integers(-1, n_reads)))
        mates.append(m)
    if a0 is None:
        a0 = rng.random(S) * 20.0 + 0.5
    return Level(a0, ll, has, list(range(n_ent)), cn, rng.integers(0, symbols, n_ent), mates, e0=e0)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the oracle entry against the oracle's own level and against the long double replay

def test_oracle_urn_draws_is_the_oracles_own_level(oracle_bin):
    rng = np.random.default_rng(5)
    lib = T.oracle_lib()
    P = ctypes.POINTER
    lib.oracle_np_bayes_level.argtypes = [ctypes.c_int, P(ctypes.c_double), ctypes.c_int, P(ctypes.c_double), P(ctypes.c_ubyte),
                                          ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int), P(ctypes.c_int), P(ctypes.c_int),
                                          P(ctypes.c_int), ctypes.c_int, P(ctypes.c_double)]
    for S, n_ent, cn_max, mf in ((2, 30, 1, 0.0), (5, 40, 3, 0.6), (17, 25, 2, 0.8), (40, 60, 1, 0.3)):
        lv = make_level(rng, S, n_ent, cn_max=cn_max, mate_frac=mf, has_frac=0.9)
        n = min(6, MAX_DRAWS // lv.Q)
        U = np.zeros(n * lv.Q)
        lib.oracle_mt_canonical(1234, len(U), U.ctypes.data_as(P(ctypes.c_double)))
        choice, kdraw, cnt = oracle_draws(lv, n, U)
        # the level through np_bayes_clustering itself, with its own mt19937(1234)
        mate_off = np.zeros(lv.n_reads + 1, dtype=np.int32)
        mate_off[1:] = np.cumsum([len(m) for m in lv.mates])
        mate_idx = np.array([x for m in lv.mates for x in m] or [0], dtype=np.int32)
        e = [np.array(x, dtype=np.int32) for x in (lv.ent_rid, lv.ent_cn, lv.ent_sym)]
        ab = np.zeros(S)
        rc = lib.oracle_np_bayes_level(S, lv.a0.ctypes.data_as(P(ctypes.c_double)), lv.n_reads, lv.ll.ctypes.data_as(P(ctypes.c_double)),
                                       lv.has.ctypes.data_as(P(ctypes.c_ubyte)), len(e[0]), *[x.ctypes.data_as(P(ctypes.c_int)) for x in e],
                                       mate_off.ctypes.data_as(P(ctypes.c_int)), mate_idx.ctypes.data_as(P(ctypes.c_int)), n,
                                       ab.ctypes.data_as(P(ctypes.c_double)))
        assert rc == 0
        a = lv.a0.astype(LD) + kdraw.astype(LD)
        want = (a / np.cumsum(a)[-1] * LD(lv.Q)).astype(np.float64)
        assert np.array_equal(ab, want), (S, ab, want)
        # and the long double replay draws what the oracle draws
        U2, ch2 = Walk(lv).run(n * lv.Q, lambda t, q, cp, w: U[t])
        assert np.array_equal(ch2, choice)
        assert np.array_equal(np.bincount(choice, minlength=S), kdraw)
        assert np.array_equal(cnt.sum(axis=1), kdraw)


# ---------------------------------------------------------------------------------------------------------------------
# GPU

@pytest.fixture(scope="module")
def ctx():
    from rambl_amd import capi
    c = capi.Context(0, 1)
    yield c
    c.close()


def check(ctx, lv, U, n_sweeps, label=""):
    """Device against oracle on the same inputs and uniforms: every count equal, every draw made."""
    total = n_sweeps * lv.Q
    choice, kdraw, cnt = oracle_draws(lv, n_sweeps, U)
    r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, lv.mates, n_sweeps, U[:total], e0=lv.e0)
    assert r["n_draws"] == total, label
    assert np.array_equal(r["kdraw"].astype(np.int64), kdraw), "%s: draws per strain differ\n dev %s\n ref %s" % (
        label, r["kdraw"].tolist(), kdraw.tolist())
    assert np.array_equal(r["cnt"].astype(np.int64), cnt), "%s: draws per (strain, symbol) differ" % label
    return r, choice


def crafted_run(lv, total, rng, plan):
    """plan(t) -> None (a clear uniform, 1e-2 from every boundary) or (delta, side).  Returns U, the crafted draws
    [(t, delta, intended strain)] and the replay's choices."""
    crafted = []

    def choose(t, q, cp, w):
        p = plan(t)
        if p is not None:
            delta, side = p
            c = craft(cp, delta, side, rng)
            if c is not None:
                crafted.append((t, delta, c[1]))
                return c[0]
        return clear_uniform(cp, 1e-2, rng)
    U, ch = Walk(lv).run(total, choose)
    return U, crafted, ch


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 3, 15, 16, 17, 32, 33, 63, 64, 65, 96, 127, 128])
def test_boundary_distances(ctx, S):
    """Uniforms at every asserted distance on both sides of a boundary: exact equality, and each tier runs where the
    distance says it must."""
    rng = np.random.default_rng(1000 + S)
    n_ent = {2: 40, 3: 40, 15: 30, 16: 30, 17: 30, 32: 24, 33: 24}.get(S, 16)
    # a few strains carry most of the weight: room for uniforms 1e-2 from every boundary
    a0 = rng.random(S) * 3.0 + 0.5
    a0[rng.choice(S, min(S, 3), replace=False)] += 200.0
    lv = make_level(rng, S, n_ent, cn_max=2, mate_frac=0.4, has_frac=0.9, spread=1.0, a0=a0)
    n = max(1, 240 // lv.Q)
    total = n * lv.Q
    # clear draws only: the fp64 scan never runs
    U, crafted, ch = crafted_run(lv, total, rng, lambda t: (1e-2, 1 if t % 2 else -1))
    r, choice = check(ctx, lv, U, n, "S=%d clear" % S)
    assert np.array_equal(choice, ch)
    assert r["n_slow"] == 0 and r["n_exact"] == 0, (S, r)
    for name in DELTAS_ASSERTED[1:]:
        d = delta_value(name, S)
        U, crafted, ch = crafted_run(lv, total, rng, lambda t: (d, 1 if (t // 3) % 2 else -1) if t % 3 == 1 else None)
        assert len(crafted) >= total // 4, (S, name, len(crafted))
        r, choice = check(ctx, lv, U, n, "S=%d delta=%s" % (S, name))
        assert np.array_equal(choice, ch), "S=%d delta=%s: the replay and the oracle disagree" % (S, name)
        for t, _, want in crafted:
            assert choice[t] == want, (S, name, t)
        m = len(crafted)
        if d <= epsw(S) / 10 * (1 + 1e-9):
            assert r["n_slow"] >= m, "S=%d delta=%s: %d crafted draws, %d through the fp64 scan" % (S, name, m, r["n_slow"])
        if d <= 1e-11:
            assert r["n_exact"] >= m, "S=%d delta=%s: %d crafted draws, %d through the literal tier" % (S, name, m, r["n_exact"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 24, 40, 70])
def test_exact_boundary_and_few_ulp_reported(ctx, S, capsys):
    """delta = 0 and a few ulp: reported, not asserted (the device's fp64 exp/log and the reference's long double may
    round one ulp apart there)."""
    rng = np.random.default_rng(77 + S)
    lv = make_level(rng, S, 20, cn_max=1, spread=2.0)
    n = max(1, 200 // lv.Q)
    out = []
    for name, d in (("0", 0.0), ("2ulp", 4.4e-16), ("16ulp", 3.6e-15)):
        U, crafted, ch = crafted_run(lv, n * lv.Q, rng, lambda t: (d, 1 if t % 4 == 1 else -1) if t % 2 else None)
        choice, kdraw, cnt = oracle_draws(lv, n, U)
        r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, lv.mates, n, U, e0=lv.e0)
        same = np.array_equal(r["kdraw"].astype(np.int64), kdraw) and np.array_equal(r["cnt"].astype(np.int64), cnt)
        out.append("%s:%s(exact %d)" % (name, "equal" if same else "DIFFERS", r["n_exact"]))
    with capsys.disabled():
        print("\n  S=%d at the boundary: %s" % (S, " ".join(out)))


def window_adversarial(lv, total, rng, NW):
    """Each uniform lies between boundary j under the counts 1..16*NW-1 draws earlier and boundary j now: a decision
    taken with the counts in front of a window that started there differs from the sequential one."""
    W = 16 * NW
    hist = []
    n_adv = [0]

    def choose(t, q, cp, w):
        hist.append(w.a.copy())
        if len(hist) > W:
            hist.pop(0)
        if t == 0:
            return float(rng.random())
        d = int(rng.integers(1, min(t, W - 1) + 1))
        old = w.cp(q, hist[-1 - d])
        diff = np.abs(old[:-1] - cp[:-1])
        js = np.nonzero(diff > 1e-9)[0]
        if len(js) == 0:
            return float(rng.random())
        j = js[rng.integers(len(js))]
        n_adv[0] += 1
        return float((old[j] + cp[j]) / 2)
    U, ch = Walk(lv).run(total, choose)
    return U, ch, n_adv[0]


@pytest.mark.gpu
@pytest.mark.parametrize("S,NW", [(2, 8), (9, 8), (32, 8), (33, 4), (64, 4), (100, 4)])
def test_window_adversarial(ctx, S, NW):
    assert window_of(S) == 16 * NW
    rng = np.random.default_rng(300 + S)
    lv = make_level(rng, S, 50, cn_max=2, mate_frac=0.3, spread=1.5, a0=rng.random(S) * 2 + 0.2)
    n = max(1, 1500 // lv.Q)
    total = n * lv.Q
    U, ch, n_adv = window_adversarial(lv, total, rng, NW)
    assert n_adv > total // 2
    r, choice = check(ctx, lv, U, n, "S=%d window-adversarial" % S)
    assert np.array_equal(choice, ch)
    assert r["n_pass"] > total / (16 * NW), (S, r["n_pass"], total)


@pytest.mark.gpu
@pytest.mark.parametrize("top", [-650.0, -700.0, -720.0, -740.0, -760.0, -800.0, -np.inf])
@pytest.mark.parametrize("S", [4, 70])
def test_flagged_slots(ctx, S, top):
    """Slots whose best log-likelihood lies in the underflow range of the reference's exp (or is -inf) go to the
    literal tier, every draw of them."""
    rng = np.random.default_rng(int(abs(top) if np.isfinite(top) else 999) + S)
    lv = make_level(rng, S, 30, cn_max=2, mate_frac=0.3, spread=3.0)
    flagged = rng.random(lv.n_reads) < 0.4
    flagged[:3] = True
    for r in np.nonzero(flagged)[0]:
        if np.isfinite(top):
            row = top - rng.random(S) * 40.0
            row[rng.integers(S)] = top
        else:
            row = np.full(S, -np.inf)
        # the row of the read; its mate (if any) adds nothing that would lift it
        lv.ll[:, r] = row
    lv.has[:] = 1
    lv2 = Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [[] for _ in range(lv.n_reads)], e0=lv.e0)
    n = max(1, 600 // lv2.Q)
    U = rng.random(n * lv2.Q)
    r, choice = check(ctx, lv2, U, n, "S=%d top=%r" % (S, top))
    n_flag = int(flagged[lv2.rid].sum()) * n
    assert r["n_exact"] >= n_flag, (r["n_exact"], n_flag)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 20, 80])
def test_underflow_mixtures(ctx, S):
    """Only some candidates above -745: the reference's double weights of the others are 0 or denormal.  All
    candidates at -inf: the reference's 0/0 draws strain 0."""
    rng = np.random.default_rng(40 + S)
    lv = make_level(rng, S, 40, cn_max=1, spread=3.0)
    lv.has[:] = 1
    for r in range(40):
        kind = r % 4
        if kind == 0:
            row = -740.0 - rng.random(S) * 20.0                        # straddles -745
        elif kind == 1:
            row = np.where(rng.random(S) < 0.3, -700.0 - rng.random(S) * 8, -760.0 - rng.random(S) * 50)
        elif kind == 2:
            row = np.full(S, -np.inf)
            row[rng.integers(S)] = -730.0
        else:
            row = np.full(S, -np.inf)
        lv.ll[:, r] = row
    lv = Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    n = max(1, 800 // lv.Q)
    U = rng.random(n * lv.Q)
    r, choice = check(ctx, lv, U, n, "S=%d mixtures" % S)
    assert np.all(choice[np.arange(n * lv.Q) % lv.Q % 4 == 3] == 0)     # 0/0: strain 0
    assert r["n_exact"] >= n * lv.Q


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 7, 33, 90])
def test_extreme_uniforms_and_zero_weights(ctx, S):
    """u = 0, 2^-60, 1 - 2^-25, 1 - 2^-53 (the last two round to 1.0f in the fp32 copy), on rows with leading and
    trailing zero-weight candidates (with u near 1 discrete_distribution can draw a trailing zero-weight candidate:
    cp[S-1] = 1.0), exact ties, urn weights over 1e-3 .. 1e7."""
    rng = np.random.default_rng(900 + S)
    lv = make_level(rng, S, 24, cn_max=2, spread=2.0, a0=10.0 ** rng.uniform(-3, 7, S))
    lv.has[:] = 1
    for r in range(24):
        k = r % 6
        if k == 0:
            lv.ll[: S // 2 + 1, r] = -np.inf                           # leading zero weights
        elif k == 1:
            lv.ll[S // 2:, r] = -np.inf                                # trailing zero weights
        elif k == 2:
            lv.ll[:, r] = -3.0                                         # a tie across every candidate
        elif k == 3:
            lv.ll[:, r] = -3.0 - rng.uniform(85, 110, S)               # exp_weight: fp32 denormals or 0
            lv.ll[rng.integers(S), r] = -3.0
        elif k == 4:
            lv.ll[:, r] = -2000.0                                      # far below everything: flagged
    lv = Level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    ext = [0.0, 2.0 ** -60, 1.0 - 2.0 ** -25, 1.0 - 2.0 ** -53]
    n = max(1, 400 // lv.Q)
    # u = 1 - 2^-53 against a last boundary within a few ulp of 1 (trailing zero weights, or a last weight of 1e-40) is
    # a distance of a few ulp: the reference's own rounding of its sums decides it, reported below, not asserted here
    w = Walk(lv)
    U = np.zeros(n * lv.Q)
    for t in range(n * lv.Q):
        cp = w.cp(t % lv.Q)
        u = ext[t % 4] if t % 3 else rng.random()
        if u == ext[3] and cp[-2] > 1.0 - 1e-11:
            u = ext[2]
        U[t] = u
        w.a[w.lower_bound(cp, u)] += 1
    assert np.sum(U == ext[3]) > 0
    check(ctx, lv, U, n, "S=%d extremes" % S)
    # the same with every 1 - 2^-53 where the replay put it: reported
    U1 = np.array([ext[t % 4] if t % 3 else U[t] for t in range(n * lv.Q)])
    _, kdraw, cnt = oracle_draws(lv, n, U1)
    r = ctx.sample_level(lv.a0, lv.ll, lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, lv.mates, n, U1, e0=lv.e0)
    same = np.array_equal(r["kdraw"].astype(np.int64), kdraw) and np.array_equal(r["cnt"].astype(np.int64), cnt)
    print("\n  S=%d u = 1 - 2^-53 on last boundaries within a few ulp of 1: %s" % (S, "equal" if same else "DIFFERS"))
    # equal urn weights and equal rows: ties decided by position alone
    lv2 = Level(np.full(S, 5.0), np.full((S, lv.n_reads), -1.5), lv.has, lv.ent_rid, lv.ent_cn, lv.ent_sym, [], e0=lv.e0)
    U2, crafted, ch = crafted_run(lv2, n * lv2.Q, rng, lambda t: (1e-11, 1 if t % 2 else -1))
    r, choice = check(ctx, lv2, U2, n, "S=%d ties" % S)
    assert np.array_equal(choice, ch)
    assert r["n_exact"] >= len(crafted) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("u_last,want", [(1.0 - 1.25 * 2.0 ** -24, 0), (1.0 - 2.0 ** -25, 1), (1.0 - 3e-7, 0)])
def test_window_margin_with_a_small_total_weight(ctx, u_last, want):
    """Draws of u = 1e-9 (margin ~0 in the window) in front of a u close to 1, with the urn's total weight T = 0.1: the
    boundary below the target moves up by 1 - u per earlier draw, which the pass knows only as 1 - (fp32 u), and eps * T
    is far below the difference.  1 - 1.25 * 2^-24 reads 1 - 2^-24: the window used to accept strain 1 at draw 100,
    where the sequential chain, 100 draws of strain 0 later, draws strain 0.  (1 - 2^-25 reads 1.0f; 1 - 3e-7 is
    a control.)"""
    ll = np.array([[0.0], [np.log(1e-3)]])
    lv = Level([0.1, 7e-3], ll, [1], [0], [1], [2], [], e0=3)
    n = 200
    U = np.full(n, 1e-9)
    U[100] = u_last
    U[150] = u_last
    choice, kdraw, cnt = oracle_draws(lv, n, U)
    assert choice[100] == want
    check(ctx, lv, U, n, "u=%r" % u_last)


@pytest.mark.gpu
def test_every_kernel_variant_against_the_oracle(ctx):
    """NB = 1..8 with the weight rows in LDS and in HBM: the 16 kinds of the sampler kernel, each once, plus totals
    that refill the uniform window and are not a multiple of it, copy numbers > 1, mates, reads absent."""
    rng = np.random.default_rng(16)
    seen = set()
    for S in (2, 20, 40, 60, 70, 90, 110, 128):
        stride = (S + 1 + 3) & ~3
        stride = stride if stride & 4 else stride + 4
        q_hbm = 141056 // (4 * stride) + 8                             # rows beyond the LDS share of the rows
        for n_ent, cn_max in ((50, 3), (q_hbm, 1)):                    # ~100 draw slots in LDS; q_hbm slots in HBM
            lv = make_level(rng, S, n_ent, cn_max=cn_max, mate_frac=0.5, has_frac=0.8, spread=4.0, e0=int(rng.integers(1, 50)))
            n = max(1, min(MAX_DRAWS // lv.Q, 2600 // lv.Q + 1))
            U = rng.random(n * lv.Q)
            r, _ = check(ctx, lv, U, n, "S=%d Q=%d" % (S, lv.Q))
            seen.add(r["kind"])
    assert seen == set(range(1, 17)), sorted(seen)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Q", [(3, 1), (33, 7), (17, 64), (65, 100), (128, 7), (6, 3001)])
def test_shapes_and_window_refills(ctx, S, Q):
    """Q in {1, 7, 64, 100} and a total above 2048 that is no multiple of the window; e0 > 0 with distinct rows in
    front; crafted near-boundary draws through the checked tiers on every shape."""
    rng = np.random.default_rng(S * 1000 + Q)
    lv = make_level(rng, S, Q, cn_max=1, mate_frac=0.5, has_frac=0.85, spread=2.0, e0=int(rng.integers(3, 40)))
    n = 2500 // lv.Q + 1
    if n * lv.Q % window_of(S) == 0:
        n += 1
    total = n * lv.Q
    assert 2048 < total <= MAX_DRAWS and total % window_of(S) != 0
    d = epsw(S) / 10
    U, crafted, ch = crafted_run(lv, total, rng, lambda t: (d, 1 if t % 2 else -1) if t % 7 == 3 else None)
    r, choice = check(ctx, lv, U, n, "S=%d Q=%d" % (S, Q))
    assert np.array_equal(choice, ch)
    assert r["n_slow"] >= len(crafted) > 0


@pytest.mark.gpu
def test_sample_level_rejects_what_it_cannot_run(ctx):
    from rambl_amd import capi
    rng = np.random.default_rng(2)
    lv = make_level(rng, 4, 10)
    bad = [
        dict(a0=np.ones(1), ll=lv.ll[:1]),                                       # S = 1
        dict(a0=np.ones(129), ll=np.zeros((129, lv.n_reads))),                   # S = 129
        dict(ent_sym=[KMAX] * 10),                                               # symbol >= KMAX
        dict(n_sweeps=MAX_DRAWS // lv.Q + 1),                                    # too many draws
    ]
    for b in bad:
        args = dict(a0=lv.a0, ll=lv.ll, has=lv.has, ent_rid=lv.ent_rid, ent_cn=lv.ent_cn, ent_sym=lv.ent_sym, mates=lv.mates,
                    n_sweeps=1, U=np.full(MAX_DRAWS, 0.5), e0=lv.e0)
        args.update(b)
        with pytest.raises(capi.StrainCallError) as e:
            ctx.sample_level(**args)
        assert e.value.code == -3
    # a context of several regions in flight (resident level workers) does not take it
    ok = dict(a0=lv.a0, ll=lv.ll, has=lv.has, ent_rid=lv.ent_rid, ent_cn=lv.ent_cn, ent_sym=lv.ent_sym, mates=lv.mates,
              n_sweeps=1, U=np.full(lv.Q, 0.5), e0=lv.e0)
    ctx.sample_level(**ok)
    with capi.Context(0, 2) as c2:
        with pytest.raises(capi.StrainCallError) as e:
            c2.sample_level(**ok)
        assert e.value.code == -3
