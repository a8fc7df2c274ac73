"""Named edge cases of one level's hard update (rambl_amd/csrc/sc_level.hip: level_plain_body behind phase_update, and its
grid twin k_hard_mates / k_hard_resp / k_hard_sums; phase_slots, zero_unseen_mates, normalise_column, strain_sums), for the
test entry sc_hard_level (capi.Context.hard_level), with a long-double reference.

A case is an update case of tests/update_edge_lib.py (the level in front of the hard update: strains in rows
(37 s + 5) % 128, labels, tables, entries at e0 > 0, `has`, copies) and what the hard update adds: the strains' log priors,
the entries' copy numbers, the reads' mate lists.  reference(case) restates what the reference program does
(hard_clustering, Strain::logprob(int), Strain::update_model) on the matrix update_edge_lib.reference leaves:

* slots: entry r with copy number cn yields cn slots, copy k = cn - 1 ... 0; the slot's mate is mates[rid][k] where the
  list is that long, else none; its code is the label's symbol, 0xFF for a longer label;
* a mate that is not in `has` behind the update gets a +0.0 cell in the rows of the level's strains (logprob(uid) inserts
  it), and is present from then on; every other cell keeps its bits;
* per slot, in np.longdouble (the reference's DoubleL): x_s = logpri_s + ll_s[rid] (+ ll_s[uid]), p_s = exp(x_s) / sum_s
  exp(x_s), formed with the maximum taken out (the same quotient); a NaN in the column makes the column NaN, and so does a
  column of -inf (0 / 0);
* abundance_s = sum_q p_s; the histogram: a level of one-symbol labels adds p_s to [a][b], a the strain's symbol, b the
  slot's, for a, b < K; a level with a longer label walks the two labels backwards from their ends when the entry's read
  is new to the level, forwards from their starts otherwise, over min(len) steps, and a one-symbol read label counts only
  against a one-symbol strain label.

The bounds of tolerances() are derived from the case (see there); the exact cases need none.  reaches(case) asserts by the
reference alone that a case reaches the edge it is named for."""
import math
import zlib

import numpy as np

import update_edge_lib as UL

L = np.longdouble
LONG_DOUBLE_OK = np.finfo(np.longdouble).nmant == 63          # x87 extended: the tests skip otherwise
MAXS, KMAX, TABLE_CAP, CAP_S = UL.MAXS, UL.KMAX, UL.TABLE_CAP, UL.CAP_S
LV_COPIES, LV_ITEMS, LV_HAS, LV_HARD, LV_SLOTS, LV_TICKED = 1, 2, 4, 8, 16, 64
U64 = 2.0 ** -53                                              # unit roundoff of fp64
TINY, TINY_DEV = 2.0 ** -1000, 2.0 ** -999
need, slot_of, same_bits = UL.need, UL.slot_of, UL.same_bits


class HardCase:
    """u: the update case in front; logpri[S]; ent_cn[Rn]; mates: per read a list of mate ids; exact: every responsibility
    is 1 / S exactly."""

    def __init__(self, u, logpri, ent_cn, mates, exact=False):
        self.u, self.name, self.logpri, self.ent_cn, self.mates, self.exact = u, u.name, np.asarray(logpri, dtype=np.float64), [int(c) for c in ent_cn], mates, exact

    @property
    def S(self):
        return self.u.S

    @property
    def K(self):
        return self.u.K

    @property
    def Q(self):
        return sum(self.ent_cn)

    def call_args(self):
        return dict(self.u.call_args(), logpri=self.logpri, ent_cn=self.ent_cn, mates=self.mates)


def copy_numbers(Q, rng=None):
    """Copy numbers 1, 2, 3, 1, ... (or drawn) that add up to Q."""
    out = []
    while sum(out) < Q:
        c = (len(out) % 3) + 1 if rng is None else int(rng.integers(1, 4))
        out.append(min(c, Q - sum(out)))
    return out


def build(name, S, cns, mates=None, logpri=None, exact=False, mate_rate=0.5, **kw):
    """The case `name` on update_edge_lib.build(name, S, len(cns), clean = True, ...); mates and priors that are not given
    are drawn from the name's own stream (mates of any read, present or not, -1 among them, lists of 0 .. cn + 1 ids)."""
    kw.setdefault("clean", True)
    u = UL.build(name, S, len(cns), **kw)
    rng = np.random.default_rng(zlib.crc32((name + "/hard").encode()))
    if logpri is None:
        w = rng.random(S) + 0.05
        logpri = np.log(w / w.sum())
    if mates is None:
        mates = [[] for _ in range(u.n_reads)]
        for rid, cn in zip(u.ent_rid, cns):
            if rng.random() < mate_rate:
                mates[rid] = [int(rng.integers(-1, u.n_reads)) for _ in range(int(rng.integers(0, cn + 2)))]
    return HardCase(u, logpri, cns, mates, exact)


# ---- the reference

def slots(c):
    """(qent, qrid, quid, qcode) of the level's draw slots."""
    qent, qrid, quid, qcode = [], [], [], []
    for r, (rid, cn) in enumerate(zip(c.u.ent_rid, c.ent_cn)):
        ml = c.mates[rid] if rid < len(c.mates) else []
        lab = c.u.ent_labels[r]
        for k in range(cn - 1, -1, -1):
            qent.append(r)
            qrid.append(rid)
            quid.append(ml[k] if k < len(ml) else -1)
            qcode.append(lab[0] if len(lab) == 1 else 0xFF)
    return np.array(qent), np.array(qrid, dtype=np.int32), np.array(quid, dtype=np.int32), np.array(qcode, dtype=np.uint8)


def columns(c, m):
    """x[S][Q] in long double out of the matrix m behind the zeroing."""
    _, qrid, quid, _ = slots(c)
    rows = m[c.u.slot].astype(L)
    with np.errstate(all="ignore"):
        x = c.logpri.astype(L)[:, None] + rows[:, qrid]
        mate = quid >= 0
        x[:, mate] = x[:, mate] + rows[:, quid[mate]]
    return x


def responsibilities(x):
    """p[S][Q] = exp(x) / sum_s exp(x), the maximum taken out, the sum over the strains in order; long double."""
    S, Q = x.shape
    p = np.full((S, Q), np.nan, dtype=L)
    with np.errstate(all="ignore"):
        for q in range(Q):
            col = x[:, q]
            if np.isnan(col).any() or np.all(np.isneginf(col)):
                continue                                          # a NaN anywhere, or 0 / 0
            e = np.exp(col - col.max())
            z = L(0)
            for v in e:
                z = z + v
            p[:, q] = e / z
    return p


def contributions(c, isnew):
    """Per slot q and strain s the histogram cells (a, b) the slot adds p_s to, in the order of the walk."""
    qent, _, _, qcode = slots(c)
    u, K = c.u, c.K
    out = [[[] for _ in range(c.Q)] for _ in range(c.S)]
    for s, sb in enumerate(u.strain_labels):
        for q in range(c.Q):
            rb = u.ent_labels[qent[q]]
            if not u.any_multi or len(rb) == 1:
                pairs = [(sb[0], rb[0])] if len(sb) == 1 else []      # (a strain's label of several symbols is no key of one)
            elif isnew[qent[q]]:
                pairs = list(zip(sb[::-1], rb[::-1]))
            else:
                pairs = list(zip(sb, rb))
            out[s][q] = [(a, b) for a, b in pairs if a < K and b < K]
    return out


def reference(c):
    """dict(ll, has, isnew, free as update_edge_lib.reference, behind the hard update; qrid, quid, qcode; x, resp[S][Q],
    abund[S], subst[S][K][K] in long double; nadd[S][K][K]: additions into each cell; zeroed: the mates entered)."""
    up = UL.reference(c.u)
    m, has = up["ll"].copy(), up["has"].copy()
    qent, qrid, quid, qcode = slots(c)
    zeroed = sorted({int(v) for v in quid if v >= 0 and not has[v]})
    for v in zeroed:
        m[c.u.slot, v] = 0.0
    has[[int(v) for v in quid if v >= 0]] = 1
    x = columns(c, m)
    p = responsibilities(x)
    S, K, Q = c.S, c.K, c.Q
    abund = np.zeros(S, dtype=L)
    subst = np.zeros((S, K, K), dtype=L)
    nadd = np.zeros((S, K, K), dtype=np.int64)
    con = contributions(c, up["isnew"])
    for s in range(S):
        for q in range(Q):
            abund[s] = abund[s] + p[s, q]
            for a, b in con[s][q]:
                subst[s, a, b] = subst[s, a, b] + p[s, q]
                nadd[s, a, b] += 1
    return dict(ll=m, has=has, isnew=up["isnew"], free=up["free"], qent=qent, qrid=qrid, quid=quid, qcode=qcode, x=x, resp=p, abund=abund,
                subst=subst, nadd=nadd, con=con, zeroed=zeroed, before=up)


# ---- the bounds

def gamma(n, u=U64):
    """n roundings of relative size u on a sum of terms >= 0."""
    return n * u / (1.0 - n * u)


def wave_additions(Q):
    """strain_sums: ceil(Q / 64) additions per lane, then the 6 levels of the tree."""
    return (Q + 63) // 64 + 6


def tolerances(c, ref, u=U64):
    """resp_rel[Q]: the relative bound on a responsibility of slot q.  With A_q = max_s (|logpri_s + ll_r| + |x_s| + |x_s - m|)
    over the strains with a finite x_s (three roundings in front of exp(): of the first sum, of the second, of the
    difference; a strain at -inf has p = 0 exactly), the bound is (2 A_q + S + 8) 2u: those roundings for the term and for the
    dominant term of the sum, one ulp of exp() on each, S - 1 additions and the division.  sum_rel: the relative bound of a
    sum of the device's own responsibilities, gamma(additions): ceil(Q / 64) + 6 on a wavefront (strain_sums), the number of
    additions into the cell on the sequential walk of a level with a longer label."""
    x = ref["x"]
    _, qrid, _, _ = slots(c)
    rows = ref["ll"][c.u.slot].astype(L)
    rel = np.zeros(c.Q)
    with np.errstate(all="ignore"):
        first = np.abs(c.logpri.astype(L)[:, None] + rows[:, qrid])
        for q in range(c.Q):
            fin = np.isfinite(x[:, q])
            if not fin.any() or np.isnan(x[:, q]).any():
                continue
            mx = x[fin, q].max()
            A = float((first[fin, q] + np.abs(x[fin, q]) + np.abs(x[fin, q] - mx)).max())
            rel[q] = (2.0 * A + c.S + 8.0) * 2.0 * u
    seq = c.u.any_multi
    return dict(resp_rel=rel, sequential=seq, wave=gamma(wave_additions(c.Q)))


def check_resp(c, ref, tol, resp):
    """The device's responsibilities against the reference's: the worst error / bound (NaN for NaN, tiny for tiny)."""
    p, worst = ref["resp"], 0.0
    for q in range(c.Q):
        for s in range(c.S):
            want, got = p[s, q], float(resp[s, q])
            if np.isnan(want):
                need(math.isnan(got), "%s: resp[%d][%d] is %r where the reference has NaN" % (c.name, s, q, got))
            elif want < TINY:
                need(0.0 <= got < TINY_DEV, "%s: resp[%d][%d] is %r where the reference has %r" % (c.name, s, q, got, want))
            else:
                ratio = float(abs(L(got) - want) / want) / tol["resp_rel"][q]
                worst = max(worst, ratio)
                need(ratio <= 1.0, "%s: resp[%d][%d] = %r for %r: error / bound = %.3f" % (c.name, s, q, got, float(want), ratio))
    return worst


def cell_terms(c, ref, s, a=None, b=None):
    """The slots whose p_s goes into the abundance (a is None) or into cell [a][b], once per addition."""
    if a is None:
        return list(range(c.Q))
    return [q for q in range(c.Q) for ab in ref["con"][s][q] if ab == (a, b)]


def check_sums(c, ref, tol, resp, abund, subst):
    """The device's sums against its own responsibilities (math.fsum) and against the reference's sums, at the sum of the
    two bounds.  Returns the worst error / bound of either kind.  A cell nothing is added to is +0.0."""
    worst_own = worst_ref = 0.0
    cells = [(s, None, None) for s in range(c.S)] + [(s, a, b) for s in range(c.S) for a in range(c.K) for b in range(c.K)]
    for s, a, b in cells:
        got = float(abund[s]) if a is None else float(subst[s, a, b])
        want = ref["abund"][s] if a is None else ref["subst"][s, a, b]
        qs = cell_terms(c, ref, s, a, b)
        what = "%s: %s of strain %d" % (c.name, "abundance" if a is None else "cell [%d][%d]" % (a, b), s)
        if not qs:
            need(np.float64(got).view(np.uint64) == 0, what + " is %r, not +0.0" % got)
            continue
        own = [float(resp[s, q]) for q in qs]
        if np.isnan(want):
            need(math.isnan(got) and any(math.isnan(v) for v in own), what + " is %r where the reference has NaN" % got)
            continue
        need(not math.isnan(got), what + " is NaN")
        n = len(qs) if tol["sequential"] else wave_additions(c.Q)
        g = gamma(n)
        total = math.fsum(own)
        if total > 0.0 or got != 0.0:
            # (g * total is 0 for a sum of denormals: their additions are exact, and the sum must be)
            ratio = 0.0 if got == total else (abs(got - total) / (g * total) if g * total > 0.0 else math.inf)
            worst_own = max(worst_own, ratio)
            need(ratio <= 1.0, what + " = %r, its own responsibilities add up to %r: error / bound = %.3f" % (got, total, ratio))
        # against the reference: every term within its own bound (a tiny one within 2^-999), then the additions
        slack = sum(float(ref["resp"][s, q]) * tol["resp_rel"][q] if ref["resp"][s, q] >= TINY else TINY_DEV for q in qs)
        bound = slack + g * (float(want) + slack)
        if bound > 0.0:
            ratio = float(abs(L(got) - want)) / bound
            worst_ref = max(worst_ref, ratio)
            need(ratio <= 1.0, what + " = %r for %r: error / bound = %.3f" % (got, float(want), ratio))
        else:
            need(got == 0.0, what + " = %r for 0" % got)
    return worst_own, worst_ref


def expected_done(c, wide):
    """The LV_* bits launch_level returns for the case in a run with SC_WIDE_MIN = 0 (wide) or huge."""
    if not wide or c.u.has_dups or c.u.any_multi:
        return 0
    return LV_HARD | LV_SLOTS | LV_ITEMS | LV_HAS | LV_TICKED | (LV_COPIES if c.u.copies else 0)


def grid_blocks(n, per, most):
    return min(max((n + per - 1) // per, 1), most)


def last_slot(Q, per=256, most=2048):
    """Where the grid-stride loops of k_hard_mates / k_hard_resp meet slot Q - 1: (workgroup, thread, trip)."""
    threads = grid_blocks(Q, per, most) * per
    return ((Q - 1) % threads) // per, ((Q - 1) % threads) % per, (Q - 1) // threads


# ---- the cases

EDGES = {}
NAMES = []


def add(name, make, check):
    EDGES[name] = (make, check)
    NAMES.append(name)


def case(name):
    c = EDGES[name][0]()
    need(c.name == name, "the case carries its name")
    return c


def base_checks(c):
    UL.base_checks(c.u)
    need(len(c.ent_cn) == c.u.Rn and all(cn >= 1 for cn in c.ent_cn) and c.Q >= 1, "copy numbers")
    need(c.logpri.shape == (c.S,) and not np.isnan(c.logpri).any() and not np.isposinf(c.logpri).any(), "log priors")
    need(len(c.mates) == c.u.n_reads and all(-1 <= v < c.u.n_reads for ml in c.mates for v in ml), "mates")
    need(c.u.e0 > 0, "entries of other levels in front")


def reaches(c, ref=None):
    ref = ref or reference(c)
    base_checks(c)
    EDGES[c.name][1](c, ref)
    if c.exact:
        need(np.all(ref["resp"] == L(1) / L(c.S)) and float(L(1) / L(c.S)) * c.S == 1.0, "every responsibility is 1 / S, exactly")


def _plain(c):
    need(not c.u.has_dups and not c.u.any_multi, "one-symbol labels, no duplicates: the level the grid can take")


def _finite(ref):
    need(np.isfinite(ref["resp"].astype(np.float64)).all(), "finite columns")


def _equalise(c):
    """Every strain gets the first one's inputs: the same label, table, row and prior."""
    u = c.u
    u.strain_labels = [u.strain_labels[0]] * u.S
    u.lpt[:] = u.lpt[0]
    u.ll[:] = u.ll[0]
    c.logpri[:] = -math.log(u.S)
    c.exact = True
    return c


def _add_shape(name, S, Q, K=6, equal=False, fam_check=None):
    def make():
        c = build(name, S, copy_numbers(Q), K=K)
        return _equalise(c) if (equal or S == 1) else c

    def check(c, ref):
        _plain(c)
        need((c.S, c.Q, c.K) == (S, Q, K), "shape")
        need(set(c.ent_cn) <= {1, 2, 3} and (Q < 6 or set(c.ent_cn) == {1, 2, 3}), "copy numbers 1, 2 and 3")
        if Q >= 63:
            need((ref["quid"] >= 0).any() and (ref["quid"] < 0).any() and len(ref["zeroed"]) > 0, "slots with and without a mate, a mate not seen before")
        if not c.exact:
            _finite(ref)
            need(len({float(v) for v in ref["resp"][:, 0]}) == S or S > 8, "distinct responsibilities")
        if fam_check:
            fam_check(c, ref)
    add(name, make, check)


for _S in (1, 3):
    for _Q in (1, 63, 64, 65, 128, 129):                      # the lanes of strain_sums
        _add_shape("lanes_S%d_Q%d" % (_S, _Q), _S, _Q,
                   fam_check=lambda c, ref: need(c.Q in (1, 63, 64, 65, 128, 129) and wave_additions(c.Q) == {1: 7, 63: 7, 64: 7, 65: 8, 128: 8, 129: 9}[c.Q], "lanes"))
for _Q in (255, 256, 257, 511, 512, 513):                     # k_hard_resp's workgroups of 256, the level's 512 threads
    _add_shape("blocks_Q%d" % _Q, 3, _Q,
               fam_check=lambda c, ref: need(last_slot(c.Q) == {255: (0, 254, 0), 256: (0, 255, 0), 257: (1, 0, 0), 511: (1, 254, 0), 512: (1, 255, 0), 513: (2, 0, 0)}[c.Q], "blocks"))
_add_shape("odd_S5_Q103", 5, 103, fam_check=lambda c, ref: need((c.S * c.Q) % 512 != 0 and c.Q % 64 != 0 and 512 % c.Q != 0, "nothing aligned"))
for _S in (2, 16, 17, 32, 33, 64, 65, 127, 128):
    _add_shape("strains_S%d_Q70" % _S, _S, 70)
for _S in (2, 4, 64, 128):
    _add_shape("equal_S%d" % _S, _S, 70, equal=True)
_add_shape("K7_S3", 3, 70, K=7)
_add_shape("cap_K16", CAP_S, 70, K=KMAX, fam_check=lambda c, ref: need((c.S + 1) * 256 > TABLE_CAP >= c.S * 256, "the largest table that fits"))


def _symbols(name, K, code_N, strain_codes, read_codes, check):
    def make():
        cns = copy_numbers(2 * len(read_codes) + 3)[:len(read_codes)]
        return build(name, len(strain_codes), cns, K=K, code_N=code_N, strain_labels=[(a,) for a in strain_codes], ent_labels=[(b,) for b in read_codes])

    def chk(c, ref):
        _plain(c)
        if 0xFF not in strain_codes:
            _finite(ref)
        check(c, ref)
    add(name, make, chk)


def _chk_all_codes(c, ref):
    need(set(ref["qcode"].tolist()) == set(range(c.K)) and c.u.code_N in ref["qcode"], "every code 0 .. K - 1 on a slot, N among them")
    s = c.u.strain_labels.index((c.u.code_N,))
    need(all(ref["nadd"][s, c.u.code_N, b] > 0 for b in range(c.K)) and ref["nadd"][s].sum() == ref["nadd"][s, c.u.code_N].sum(), "a strain whose label is N counts in row N")


_symbols("sym_all_codes", 8, 7, [0, 3, 7, 5, 6], list(range(8)) + [7, 2, 0], _chk_all_codes)
_symbols("sym_missing", 6, -1, [0, 1, 4], [0, 1, 2, 3, 5, 5, 0, 2],
         lambda c, ref: need(4 not in ref["qcode"] and (ref["nadd"][:, :, 4] == 0).all() and c.u.strain_labels[2] == (4,), "a code no slot carries, and a strain that carries it"))
_symbols("sym_one", 6, -1, [2, 0, 2, 5], [2] * 40,
         lambda c, ref: need(set(ref["qcode"].tolist()) == {2} and c.Q > 64, "every slot carries one symbol, more slots than lanes"))
_symbols("sym_end_strain", 6, -1, [1, 0xFF, 3], [0, 1, 2, 3, 4, 5, 1],
         lambda c, ref: need(ref["nadd"][1].sum() == 0 and ref["nadd"][0].sum() == c.Q and np.isnan(ref["resp"].astype(np.float64)).all(),
                             "a strain on '$' (0xFF) counts in no cell; its log-likelihoods are log 0 - log 0, so every column is NaN"))


def _mates_lengths():
    # per copy number 1, 2, 3 a list of 0, 1, cn and cn + 1 mates: twelve entries, every mate another read, present before
    cns = [cn for cn in (1, 2, 3) for _ in range(4)]
    lens = [n for cn in (1, 2, 3) for n in (0, 1, cn, cn + 1)]
    n_reads = 48
    rng = np.random.default_rng(77)
    rid = rng.permutation(12).tolist()
    has = np.zeros(n_reads, dtype=np.uint8)
    has[12:] = 1
    has[rid[::2]] = 1
    mates = [[] for _ in range(n_reads)]
    nxt = 12
    for r, n in zip(rid, lens):
        mates[r] = list(range(nxt, nxt + n))
        nxt += n
    mates[rid[7]][1] = -1                                     # cn = 2, three mates: the second is none
    return build("mates_lengths", 3, cns, mates=mates, rid=rid, has=has, n_reads=n_reads)


def _chk_mates_lengths(c, ref):
    _plain(c)
    _finite(ref)
    for r, (rid, cn) in enumerate(zip(c.u.ent_rid, c.ent_cn)):
        got = [int(v) for q, v in enumerate(ref["quid"]) if ref["qent"][q] == r]
        want = [(c.mates[rid][k] if k < len(c.mates[rid]) else -1) for k in range(cn - 1, -1, -1)]
        need(got == want, "copy k = cn - 1 ... 0")
        if len(c.mates[rid]) >= 2 and cn >= 2:
            need(got != got[::-1], "the order of the copies shows")
    need({(cn, n) for cn in (1, 2, 3) for n in (0, 1, cn, cn + 1)} == {(cn, len(c.mates[rid])) for rid, cn in zip(c.u.ent_rid, c.ent_cn)}, "lists of 0, 1, cn and cn + 1 mates")
    need(any(-1 in c.mates[rid] and c.mates[rid][-1] != -1 for rid in c.u.ent_rid), "a -1 inside a list")
    need(not ref["zeroed"], "every mate was present")
    vals = ref["ll"][c.u.slot[0]][[v for v in ref["quid"] if v >= 0]]
    need(len(set(vals.tolist())) == len(vals), "every mate with its own log-likelihood")


add("mates_lengths", _mates_lengths, _chk_mates_lengths)

OUTSIDE = UL.FREE_ROWS[3]


def _mates_absent():
    # reads 0..5 are the level's (3 and 4 new to it); 6: present before; 7, 8: absent; the row of strain 0 is copied whole
    # into a row outside the level in front of the update
    n_reads = 12
    has = np.array([1, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
    mates = [[] for _ in range(n_reads)]
    mates[2], mates[0], mates[5], mates[1], mates[3] = [7], [7, 8], [4], [6], [-1, 8]
    return build("mates_absent", 4, [1, 2, 1, 1, 2, 1], mates=mates, rid=[2, 0, 5, 1, 3, 4], has=has, n_reads=n_reads,
                 copies=[(slot_of(0), OUTSIDE)], copy_n=n_reads)


def _chk_mates_absent(c, ref):
    _plain(c)
    _finite(ref)
    need(ref["zeroed"] == [7, 8], "two mates not seen before")
    need(sum(1 for v in ref["quid"] if v == 7) == 2 and len({ref["qent"][q] for q, v in enumerate(ref["quid"]) if v == 7}) == 2, "one of them under two slots of two entries")
    before = ref["before"]["ll"]
    for v in (7, 8):
        need(all(before[row, v] != 0.0 for row in c.u.slot) and before[OUTSIDE, v] != 0.0, "garbage in the mate's cells, inside and outside the level")
        need(all(np.float64(ref["ll"][row, v]).view(np.uint64) == 0 for row in c.u.slot), "+0.0 in the level's rows")
        need(np.float64(ref["ll"][OUTSIDE, v]).view(np.uint64) == np.float64(before[OUTSIDE, v]).view(np.uint64), "the row outside keeps its bits")
    need(OUTSIDE not in c.u.slot and c.u.copy_n >= c.u.n_reads, "a row outside the level")
    need(4 in ref["quid"] and not c.u.has[4] and 4 in c.u.ent_rid and ref["ll"][c.u.slot[0], 4] != 0.0, "a mate the level's update enters is not zeroed")
    need(6 in ref["quid"] and c.u.has[6] and 6 not in c.u.ent_rid, "a mate present before the level")
    need(ref["has"][[4, 6, 7, 8]].all() and not ref["has"][10], "the mates are present behind the level")


add("mates_absent", _mates_absent, _chk_mates_absent)


def _copy_child():
    has = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.uint8)
    mates = [[] for _ in range(8)]
    mates[6], mates[0] = [7, 5], [5]
    return build("copy_child", 3, [2, 1, 3, 1, 1], mates=mates, rid=[6, 2, 0, 5, 3], has=has, n_reads=8, strain_labels=[(0,), (1,), (2,)],
                 copies=[(slot_of(0), slot_of(1))], copy_n=8)


def _chk_copy_child(c, ref):
    _plain(c)
    _finite(ref)
    src, dst = c.u.copies[0]
    need(src in c.u.slot and dst in c.u.slot, "parent and child are strains of the level")
    need(same_bits(ref["ll"][dst], UL.prior_matrix(c.u)[dst]).size > 0, "the child's row is the parent's, updated")
    need(ref["zeroed"] == [7] and ref["resp"][1, 0] != ref["resp"][0, 0], "a mate not seen before; parent and child differ")


add("copy_child", _copy_child, _chk_copy_child)


# numbers: S strains, a handful of slots, x stated cell by cell.  Every read of the level was present (the update adds a
# table of zeros: the cell stays), no mates unless stated.
def _numbers(name, xs, logpri=None, cns=(1, 2, 1), twin=None):
    xs = np.asarray(xs, dtype=np.float64)                      # [S][Rn]
    S, Rn = xs.shape
    rid = [4, 1, 6, 0, 3][:Rn]
    n_reads = 9
    has = np.ones(n_reads, dtype=np.uint8)
    c = build(name, S, list(cns)[:Rn], mates=[[] for _ in range(n_reads)], logpri=np.zeros(S) if logpri is None else logpri, rid=rid, has=has, n_reads=n_reads,
              strain_labels=[(s % 6,) for s in range(S)])
    c.u.lpt[:] = 0.0
    for r in range(Rn):
        c.u.ll[:, rid[r]] = xs[:, r] - c.logpri if np.isfinite(c.logpri).all() else xs[:, r]
    return c


def _x_of(ref):
    return ref["x"].astype(np.float64)


def _add_close():
    def make():
        rng = np.random.default_rng(5)
        return _numbers("num_close", -37.0 + rng.random((4, 3)) * 1e-3, logpri=np.log([0.25, 0.25, 0.25, 0.25]))

    def check(c, ref):
        x = _x_of(ref)
        need((x.max(axis=0) - x.min(axis=0)).max() < 1e-3 and len(set(x[:, 0].tolist())) == c.S, "every x within 1e-3 of the others, none equal")
    add("num_close", make, check)


_add_close()


def _add_ahead(d):
    name = "num_ahead_%d" % d

    def make():
        xs = np.full((4, 3), -12.5 - d)
        xs[2, :] = -12.5
        xs[0, 1] -= 0.25
        xs[3, 2] -= 1.0
        return _numbers(name, xs)

    def check(c, ref):
        x = _x_of(ref)
        need(np.all(x[2] - np.delete(x, 2, axis=0).max(axis=0) == d), "one strain ahead by %d" % d)
        small = ref["resp"][0, 0]                              # (long double: e^-1500 is an ordinary number there)
        need({50: small >= TINY, 700: 0 < small < TINY, 745: 0 < small < TINY and math.exp(-745.0) > 0.0, 746: math.exp(-746.0) == 0.0 and small > 0,
              1500: math.exp(-1500.0) == 0.0 and small > 0}[d], "the range of exp(-%d) in fp64" % d)
    add(name, make, check)


for _d in (50, 700, 745, 746, 1500):
    _add_ahead(_d)


def _deep():
    rng = np.random.default_rng(11)
    xs = -800.0 - rng.random((5, 3)) * 700.0
    xs[1, 0], xs[4, 0] = -800.5, -1499.5
    xs[:, 1] = -1100.0 - rng.random(5) * 3.0
    return _numbers("num_deep", xs, logpri=np.log([0.4, 0.3, 0.15, 0.1, 0.05]))


add("num_deep", _deep, lambda c, ref: (_finite(ref), need(_x_of(ref).max() < -800 and _x_of(ref).min() > -1500.5 and np.all(np.exp(_x_of(ref)) == 0.0), "every exp(x) is 0 in fp64"),
                                         need((ref["resp"][:, 1] >= TINY).all() and float(ref["abund"].sum()) > 3.99, "and the responsibilities are ordinary numbers")))


def _pri_inf(name, which):
    def make():
        rng = np.random.default_rng(13)
        lp = np.log([0.5, 0.25, 0.125, 0.125])
        lp[which] = -np.inf
        return _numbers(name, -20.0 - rng.random((4, 3)) * 4.0, logpri=lp)

    def check(c, ref):
        need(np.isneginf(c.logpri[which]).all() and np.isneginf(_x_of(ref)[which]).all(), "log 0")
        if len(which) < c.S:
            need(np.all(ref["resp"][which] == 0) and np.isfinite(ref["resp"].astype(np.float64)).all() and np.all(ref["abund"][which] == 0), "p = 0 exactly, the others finite")
        else:
            need(np.isnan(ref["resp"].astype(np.float64)).all() and np.isnan(ref["abund"].astype(np.float64)).all(), "0 / 0")
    add(name, make, check)


_pri_inf("num_pri_inf_some", [1, 3])
_pri_inf("num_pri_inf_all", [0, 1, 2, 3])


def _special_cell(name, value, check):
    def make():
        rng = np.random.default_rng(17)
        xs = -15.0 - rng.random((4, 3)) * 6.0
        xs[2, 1] = value
        c = _numbers(name, xs, logpri=np.log([0.1, 0.2, 0.3, 0.4]))
        c.u.ent_labels = [(0,), (3,), (5,)]
        return c
    add(name, make, check)


_special_cell("num_cell_inf", -np.inf, lambda c, ref: need(np.all(ref["resp"][2, 1:3] == 0) and np.isfinite(ref["resp"].astype(np.float64)).all() and float(ref["resp"][2, 0]) > 0,
                                                           "a -inf cell: p = 0 on its two slots alone"))


def _chk_nan(c, ref):
    p, sub = ref["resp"].astype(np.float64), ref["subst"].astype(np.float64)
    need(np.isnan(p[:, 1:3]).all() and np.isfinite(p[:, 0]).all() and np.isfinite(p[:, 3]).all(), "the slots of one entry are NaN in every strain")
    need(np.isnan(ref["abund"].astype(np.float64)).all(), "every abundance is NaN")
    for s in range(c.S):
        a = c.u.strain_labels[s][0]
        need(np.isnan(sub[s, a, 3]) and np.isfinite(sub[s, a, 0]) and sub[s, a, 0] > 0 and np.isfinite(sub[s, a, 5]) and sub[s, a, 5] > 0, "only the cells of that slot's symbol are NaN")


_special_cell("num_nan", np.nan, _chk_nan)


def _twins():
    c = build("twins", 6, copy_numbers(70))
    u = c.u
    u.strain_labels[5] = u.strain_labels[1]
    u.lpt[5], u.ll[5], c.logpri[5] = u.lpt[1], u.ll[1], c.logpri[1]
    return c


add("twins", _twins, lambda c, ref: (_plain(c), _finite(ref), need(abs(c.u.slot[5] - c.u.slot[1]) > 16 and np.all(ref["resp"][1] == ref["resp"][5]) and
                                                                   len({float(v) for v in ref["resp"][:, 0]}) == 5, "two strains with identical inputs in distant rows")))


def _dups():
    order = ["A", "B", "C", "C", "D", "B", "E", "B", "A"]
    ids = dict(A=9, B=2, C=14, D=0, E=11)
    rid = [ids[x] for x in order]
    first = [1 if order.index(x) == r else 0 for r, x in enumerate(order)]
    has = np.zeros(17, dtype=np.uint8)
    has[[ids["B"], ids["D"], 5, 16]] = 1
    mates = [[] for _ in range(17)]
    mates[9], mates[2], mates[14] = [5, 3], [16, -1, 7], [9]
    return build("dups", 4, [2, 3, 1, 2, 1, 1, 2, 3, 1], mates=mates, rid=rid, first=first, has=has, n_reads=17)


def _chk_dups(c, ref):
    need(c.u.has_dups and not c.u.any_multi, "duplicates, one-symbol labels")
    occ = UL.occurrences(c.u)
    need(sorted(len(v) for v in occ.values()) == [1, 1, 2, 2, 3], "a read twice and three times")
    for rid, rs in occ.items():
        for r in rs:
            need(sum(1 for q in ref["qent"] if q == r) == c.ent_cn[r], "every occurrence has its own slots")
    need(len({c.ent_cn[r] for r in occ[2]}) > 1 and ref["zeroed"] == [3, 7], "occurrences with different copy numbers; mates not seen before")
    _finite(ref)


add("dups", _dups, _chk_dups)

MULTI_STRAINS = [(1,), (2, 1, 3), (4,), (0, 5, 2)]
MULTI_READS = [(3,), (1, 2), (0, 1, 3, 2), (5,), (2, 3), (4, 0, 5, 1)]


def _multi(name, strains):
    def make():
        reads = MULTI_READS + MULTI_READS
        n = len(reads)
        rid = [(7 * r + 3) % (2 * n + 1) for r in range(n)]
        has = np.zeros(2 * n + 4, dtype=np.uint8)
        has[rid[len(MULTI_READS):]] = 1                       # every label on a read that is new to the level and on one that is not
        has[2 * n + 2] = 1
        mates = [[] for _ in range(len(has))]
        mates[rid[1]], mates[rid[8]] = [2 * n + 2], [2 * n + 3, -1]
        return build(name, len(strains), copy_numbers(2 * n + 1)[:n], K=6, strain_labels=strains, ent_labels=reads, mates=mates, rid=rid, has=has, n_reads=len(has))
    return make


def _chk_multi(c, ref):
    need(c.u.any_multi and not c.u.has_dups, "a level with longer labels")
    _finite(ref)
    u = c.u
    need({len(x) for x in u.strain_labels} == {1, 3} and {len(x) for x in u.ent_labels} == {1, 2, 4}, "strain labels of 1 and 3 symbols, entry labels of 1, 2 and 4")
    for new in (0, 1):
        for n in (1, 2, 4):
            need(any(len(u.ent_labels[r]) == n and ref["isnew"][r] == new for r in range(u.Rn)), "every length on a read that is new and on one that is not")
    for s, sb in enumerate(u.strain_labels):
        for r, rb in enumerate(u.ent_labels):
            if len(sb) > 1 and len(rb) > 1:
                need(list(zip(sb[::-1], rb[::-1])) != list(zip(sb, rb))[::-1], "the backward and the forward walk meet different pairs")
    s3 = [s for s, sb in enumerate(u.strain_labels) if len(sb) == 3][0]
    q1 = [q for q in range(c.Q) if len(u.ent_labels[ref["qent"][q]]) == 1]
    need(q1 and all(ref["con"][s3][q] == [] for q in q1), "a one-symbol read against a three-symbol strain counts nowhere")
    need(ref["nadd"].max() >= 2 and ref["zeroed"] == [2 * len(MULTI_READS) * 2 + 3], "cells with several additions; a mate not seen before")


add("multi", _multi("multi", MULTI_STRAINS), _chk_multi)


def _chk_multi_end(c, ref):
    need(c.u.any_multi and (0xFF,) in c.u.strain_labels, "a strain on '$' (0xFF) in a level with longer labels")
    s = c.u.strain_labels.index((0xFF,))
    need(ref["nadd"][s].sum() == 0 and ref["nadd"][0].sum() > 0 and ref["nadd"][2].sum() > 0, "it counts in no cell; its neighbours do")
    need(np.isnan(ref["resp"].astype(np.float64)).all(), "its log-likelihoods are log 0 - log 0: every column is NaN")
    need(any(len(c.u.ent_labels[r]) == 1 for r in range(c.u.Rn)) and any(len(c.u.ent_labels[r]) > 1 for r in range(c.u.Rn)), "against one-symbol and longer read labels")


add("multi_end_strain", _multi("multi_end_strain", [(1,), (0xFF,), (2, 1, 3)]), _chk_multi_end)

EXACT = [n for n in NAMES if n.startswith("equal_") or n.startswith("lanes_S1_")]


# ---- the second trip of the grid's loops: one case of 2048 * 256 + 1 slots, checked with array arithmetic

BIG_Q = 2048 * 256 + 1


def big_case():
    """S = 2, 4 096 entries of 128 copies and one of 1, every one another read: a level of one-symbol labels without
    duplicates, so the grid takes it."""
    c = build("grid_trip", 2, [128] * 4096 + [1], mate_rate=0.3)
    absent = [r for r in range(c.u.n_reads) if not c.u.has[r] and r not in set(c.u.ent_rid)]
    c.mates[c.u.ent_rid[-1]] = [absent[-1]]                    # the last slot, the one of the second trip, has a mate not seen before
    return c


def big_reference(c):
    """reference() for a level of one-symbol labels whose columns are finite, array by array: the same rules."""
    need(not c.u.any_multi and not c.u.has_dups, "one-symbol labels, no duplicates")
    up = UL.reference(c.u)
    m, has = up["ll"].copy(), up["has"].copy()
    qent, qrid, quid, qcode = slots(c)
    zeroed = sorted({int(v) for v in quid if v >= 0 and not has[v]})
    m[np.ix_(c.u.slot, zeroed)] = 0.0
    has[quid[quid >= 0]] = 1
    x = columns(c, m)
    need(np.isfinite(x.astype(np.float64)).all(), "finite columns")
    e = np.exp(x - x.max(axis=0))
    z = e[0].copy()
    for s in range(1, c.S):
        z = z + e[s]
    p = e / z
    first = np.abs(c.logpri.astype(L)[:, None] + m[c.u.slot].astype(L)[:, qrid])
    A = (first + np.abs(x) + np.abs(x - x.max(axis=0))).max(axis=0).astype(np.float64)
    return dict(ll=m, has=has, isnew=up["isnew"], free=up["free"], qrid=qrid, quid=quid, qcode=qcode, x=x, resp=p, zeroed=zeroed,
                resp_rel=(2.0 * A + c.S + 8.0) * 2.0 * U64)


def big_check(c, ref, resp, abund, subst):
    """check_resp and check_sums for big_reference; returns the three worst error / bound."""
    p, rel = ref["resp"], ref["resp_rel"]
    tiny = p < TINY
    need(np.all((resp[tiny] >= 0) & (resp[tiny] < TINY_DEV)), "tiny for tiny")
    ratio = np.where(tiny, 0, np.abs(resp.astype(L) - p) / np.where(tiny, 1, p) / rel[None, :]).astype(np.float64)
    need(ratio.max() <= 1.0, "%s: a responsibility at error / bound = %.3f" % (c.name, ratio.max()))
    g = gamma(wave_additions(c.Q))
    worst_own = worst_ref = 0.0
    slack_q = np.where(tiny, TINY_DEV, p.astype(np.float64) * rel[None, :])
    for s in range(c.S):
        a = c.u.strain_labels[s][0]
        for b in [None] + list(range(c.K)):
            sel = np.ones(c.Q, dtype=bool) if b is None else ref["qcode"] == b
            got = float(abund[s]) if b is None else float(subst[s, a, b])
            if not sel.any():
                need(np.float64(got).view(np.uint64) == 0, "+0.0 where nothing is added")
                continue
            total = math.fsum(resp[s, sel].tolist())
            worst_own = max(worst_own, abs(got - total) / (g * total))
            want, slack = float(p[s, sel].sum()), float(slack_q[s, sel].sum())
            worst_ref = max(worst_ref, abs(got - want) / (slack + g * (want + slack)))
        rest = subst[s].copy()
        rest[a] = 0.0
        need(not rest.view(np.uint64).any(), "+0.0 outside the strain's row")
    need(worst_own <= 1.0 and worst_ref <= 1.0, "%s: a sum at error / bound = %.3f (own), %.3f (reference)" % (c.name, worst_own, worst_ref))
    return float(ratio.max()), worst_own, worst_ref
