"""Named edge cases of the read mapper.  A case is a tiny database, a few reads and the options of a call;
its `prop` is a check on the restatement's candidates (map_lib) that fails when the input no longer reaches its edge.
cases(range_genes) builds them all; range_genes is what sc_map_limits reports, so the seams are the kernel's own."""
import random

import map_lib as M

BIG = 1 << 20           # a max_occ no run of these databases reaches
VOTE_GRID = 2048        # VOTE_BLOCKS of sc_map.hip: the grid-stride case needs more reads than that


class Case:
    def __init__(self, name, genes, reads, prop, k=16, max_occ=BIG, max_cand=0, min_votes=1, pair_room=0, stretches=None):
        self.name, self.genes, self.reads, self.prop = name, genes, reads, prop
        self.k, self.max_occ, self.max_cand, self.min_votes, self.pair_room, self.stretches = k, max_occ, max_cand, min_votes, pair_room, stretches
        self._cands = None

    def candidates(self):
        """The restatement's candidates per read, computed once."""
        if self._cands is None:
            self._cands = M.all_candidates(self.genes, self.reads, self.k, self.max_occ, self.max_cand, self.min_votes)
        return self._cands

    def check(self):
        self.prop(self, self.candidates())

    def __repr__(self):
        return self.name


def seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


def hold(rng, read, a, n, left=12, right=12):
    """A gene that holds read[a:a + n] between random flanks; the flank bases next to the piece differ from the read's, so no
    shared k-mer reaches beyond the piece."""
    lf, rt = seq(rng, left), seq(rng, right)
    if a > 0 and left:
        lf = lf[:-1] + other(rng, read[a - 1])
    if a + n < len(read) and right:
        rt = other(rng, read[a + n]) + rt[1:]
    return lf + read[a:a + n] + rt


def around(rng, piece, left=10, right=10, nb="C"):
    """piece between random flanks, the base `nb` on either side of it.  A gene's piece has C there, a read's A or T (whose
    complement is no C either), so a window of the read that reaches beyond the piece matches the gene on neither strand."""
    return seq(rng, left - 1) + nb + piece + nb + seq(rng, right - 1)


def in_read(rng, piece, left=8, right=8):
    return around(rng, piece, left, right, "T" if piece[0] == "A" else "A")


def cases(range_genes):
    rng = random.Random(1818)
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- window count and alphabet
    g = seq(rng, 100)

    def p_lengths(c, cands):
        assert [len(r) for r in c.reads] == [15, 16, 17]
        assert cands[0] == [] and cands[1] == [(0, 1, 0)] and cands[2] == [(0, 2, 0)]
    add("read_k_minus_1_k_k_plus_1", [g, seq(rng, 60)], [g[10:25], g[10:26], g[10:27]], p_lengths)

    for nw in (64, 65, 128, 129):
        read = seq(rng, nw + 15)
        per = (nw + 63) // 64
        lane = 5
        last_lane = (nw - 1) // per
        ws = sorted({0, lane * per, min(lane * per + per, nw) - 1, last_lane * per, nw - 1})
        genes = [hold(rng, read, w, 16) for w in ws]

        def p_windows(c, cands, ws=ws, nw=nw):
            assert len(M.windows(c.reads[0], 16)) == nw
            assert cands[0] == [(i, 1, 0) for i in range(len(ws))], cands[0]          # one window each, and no neighbour of it
            index = M.build_index(c.genes, 16)
            for i, w in enumerate(ws):
                assert index[c.reads[0][w:w + 16]] == [i]
        add("windows_%d_first_and_last_of_a_lane" % nw, genes, [read], p_windows)

    g = seq(rng, 80)
    one = g[20:36]
    n_reads = [one[:o] + "N" + one[o + 1:] for o in range(16)] + [one, g[10:25] + "N" + g[26:41], g[8:31] + "N" + g[32:55]]

    def p_read_n(c, cands):
        assert all(cands[o] == [] for o in range(16)) and cands[16] == [(0, 1, 0)]
        assert len(c.reads[17]) == 31 and cands[17] == []                              # the N lies in every window
        assert len(c.reads[18]) == 47 and cands[18] == [(0, 16, 0)]                    # windows 0..7 and 24..31
    add("n_in_the_read_at_every_offset", [g, seq(rng, 50)], n_reads, p_read_n)

    g = seq(rng, 90)
    gn = g[:30] + "N" + g[31:]

    def p_gene_n(c, cands):
        nw = len(c.reads[0]) - 15
        assert cands[0] == [(0, nw - 16, 0)] and nw - 16 > 0 and "N" in c.genes[0] and "N" not in c.reads[0]
    add("n_in_a_gene", [gn, seq(rng, 50)], [g[10:70]], p_gene_n)

    for k in (16, 11):
        ga, gt = around(rng, "A" * (k + 4)), around(rng, "T" * (k + 2))
        reads = [in_read(rng, "A" * k, 6, 6), in_read(rng, "T" * k, 6, 6)]

        def p_poly(c, cands, k=k):
            index = M.build_index(c.genes, k)
            assert len(index["A" * k]) == 5 and len(index["T" * k]) == 3 and max(index) == "T" * k and min(index) == "A" * k
            assert cands[0] == [(0, 1, 0), (1, 0, 1)] and cands[1] == [(0, 0, 1), (1, 1, 0)], cands
        add("all_a_and_all_t_kmer_k%d" % k, [ga, gt, seq(rng, 40)], reads, p_poly, k=k)

    # ---- strands
    g = seq(rng, 100)

    def p_reverse(c, cands):
        assert cands[0] == [(0, 0, 45)]
    add("reverse_strand_votes_only", [g, seq(rng, 70)], [M.revcomp(g[10:70])], p_reverse)

    pal = "ACGTACGTACGTACGT"

    def p_pal(c, cands):
        assert M.revcomp(pal) == pal and cands[0] == [(0, 1, 1)]
    add("palindromic_kmer_votes_on_both_strands", [around(rng, pal), seq(rng, 60)], [in_read(rng, pal)], p_pal)

    # ---- counting
    p = seq(rng, 16)

    def p_twice_gene(c, cands, p=p):
        assert M.build_index(c.genes, 16)[p] == [0, 0] and cands[0] == [(0, 1, 0)]
    add("kmer_twice_in_one_gene", [around(rng, p) + around(rng, p), seq(rng, 60)], [in_read(rng, p)], p_twice_gene)

    def p_twice_read(c, cands, p=p):
        assert M.windows(c.reads[0], 16).count(p) == 2 and cands[0] == [(0, 2, 0)]
    add("kmer_in_two_windows_of_the_read", [around(rng, p), seq(rng, 60)], [in_read(rng, p) + in_read(rng, p)], p_twice_read)

    # ---- max_occ
    p, q, r = seq(rng, 16), seq(rng, 16), seq(rng, 16)
    genes = [around(rng, p) + around(rng, q), around(rng, p) + around(rng, q), around(rng, q) + around(rng, p), around(rng, q),
             around(rng, r) + around(rng, r) + around(rng, r) + around(rng, r), seq(rng, 50)]

    def p_max_occ(c, cands, p=p, q=q, r=r):
        index = M.build_index(c.genes, 16)
        assert c.max_occ == 3 and len(index[p]) == 3 and len(index[q]) == 4 and index[r] == [4, 4, 4, 4]
        assert cands[0] == [(0, 1, 0), (1, 1, 0), (2, 1, 0)] and cands[1] == [] and cands[2] == []
        assert M.all_candidates(c.genes, c.reads, 16, 4, 0, 1)[1:] == [[(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)], [(4, 1, 0)]]
    add("max_occ_runs_at_and_above", genes, [in_read(rng, x) for x in (p, q, r)], p_max_occ, max_occ=3)

    # ---- counters at their top
    for k, top in ((16, 497), (11, 502)):
        while True:                                                        # at k = 11 a chance hit on the other strand is likely enough to matter
            g, filler = seq(rng, 600), seq(rng, 80)
            read = g[40:552]
            if M.all_candidates([g, filler], [read], k, BIG, 0, 1) == [[(0, top, 0)]]:
                break

        def p_top(c, cands, top=top):
            assert len(c.reads[0]) == 512 and cands[0] == [(0, top, 0), (1, top, top)], cands[0]
        add("counter_top_k%d_and_both_halves" % k, [g, read + M.revcomp(read), filler], [read], p_top, k=k)

    # ---- gene ranges: voting genes on both sides of every seam
    R = range_genes
    for label, n in (("r_minus_1", R - 1), ("r", R), ("r_plus_1", R + 1), ("2r_plus_1", 2 * R + 1)):
        read = seq(rng, 120)
        voters = sorted({i for i in (0, R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, n - 1) if 0 <= i < n})
        genes = [seq(rng, 40) for _ in range(n)]
        want = []
        for j, i in enumerate(voters):
            m = 16 + 2 * j                                                 # 1 + 2 j votes
            genes[i] = hold(rng, read, 5 + 3 * j, m)
            want.append((i, m - 15, 0))

        def p_ranges(c, cands, want=want, n=n):
            assert len(c.genes) == n and cands[0] == want and cands[1] == [(g, b, a) for g, a, b in want], (cands[0], want)
        add("gene_ranges_%s_genes" % label, genes, [read, M.revcomp(read)], p_ranges)

    # ---- the cut
    read = seq(rng, 150)
    genes = [seq(rng, 60) for _ in range(12)]
    voters = {2: 20, 4: 18, 7: 25, 9: 17, 11: 30}                          # gene -> piece length: 5, 3, 10, 2, 15 votes
    for i, m in voters.items():
        genes[i] = hold(rng, read, 3 * i, m)
    by_votes = [11, 7, 2, 4, 9]
    for mc in (1, 4, 5, 6):
        def p_cut(c, cands, mc=mc):
            assert [g for g, _, _ in cands[0]] == sorted(by_votes[:mc]) and len(voters) == 5
        add("max_cand_%d_of_5_voting_genes" % mc, genes, [read], p_cut, max_cand=mc)

    def tie_case(name, n, ties, top, max_cand, keep):
        read = seq(rng, 100)
        genes = [seq(rng, 40) for _ in range(n)]
        for i in ties:
            genes[i] = hold(rng, read, 30, 19)                             # 4 votes each
        genes[top] = hold(rng, read, 60, 25)                               # 10 votes

        def p_ties(c, cands):
            full = M.all_candidates(c.genes, c.reads, 16, BIG, 0, 1)[0]
            assert full == sorted([(i, 4, 0) for i in ties] + [(top, 10, 0)])
            assert [g for g, _, _ in cands[0]] == keep, cands[0]
        add(name, genes, [read], p_ties, max_cand=max_cand)
    tie_case("ties_at_the_cut_inside_one_group", 200, [3, 7, 20], 150, 3, [3, 7, 150])
    tie_case("ties_at_the_cut_across_groups", 200, [3, 70, 130, 190], 150, 3, [3, 70, 150])
    tie_case("ties_at_the_cut_across_groups_last_kept_late", 200, [3, 70, 130, 190], 5, 4, [3, 5, 70, 130])
    tie_case("ties_at_the_cut_across_a_range_seam", R + 10, [R - 1, R, R + 5], 5, 3, [5, R - 1, R])
    tie_case("ties_at_the_cut_stop_before_a_range_seam", R + 10, [R - 1, R, R + 5], 5, 2, [5, R - 1])

    read = seq(rng, 80)
    genes = [hold(rng, read, 20, 19), seq(rng, 50)]
    for mv in (4, 5):
        def p_min_votes(c, cands, mv=mv):
            assert cands[0] == ([(0, 4, 0)] if mv == 4 else [])
        add("min_votes_%s" % ("at_the_vote" if mv == 4 else "one_above"), genes, [read], p_min_votes, min_votes=mv)

    # ---- grid stride and stretches
    genes = [seq(rng, 40) for _ in range(3)]
    reads = [genes[i % 3][(i // 3) % 25:(i // 3) % 25 + 16] for i in range(2 * VOTE_GRID + 3)]

    def p_grid(c, cands):
        assert len(c.reads) > 2 * VOTE_GRID and all(len(r) == 16 for r in c.reads)
        assert all(x == [(i % 3, 1, 0)] for i, x in enumerate(cands))
    add("more_reads_than_the_vote_grid", genes, reads, p_grid)

    p, q = seq(rng, 40), seq(rng, 40)
    genes = [around(rng, p) + around(rng, q), around(rng, q) + around(rng, p)] + [around(rng, q) for _ in range(4)]
    reads = [in_read(rng, p, 30, 30) for _ in range(4)] + [in_read(rng, q, 30, 30)]

    def p_stretches(c, cands):
        assert [len(x) for x in cands] == [2, 2, 2, 2, 6] and c.pair_room == 4 and len({len(r) for r in c.reads}) == 1
    add("pair_room_forces_three_stretches", genes, reads, p_stretches, pair_room=4, stretches=3)

    # ---- the contract's boundary: a valid alignment without a shared k-mer
    g = seq(rng, 200)
    read = list(g[20:170])
    for i in range(7, 150, 15):
        read[i] = other(rng, read[i])

    def p_boundary(c, cands):
        assert cands == [[]] and len(c.reads[0]) == 150
        assert 2 * 140 - 6 * 10 >= 20 + 8 * 5.02                          # ten Q40 mismatches still leave a valid score
    add("valid_alignment_without_a_shared_kmer", [g, seq(rng, 100)], ["".join(read)], p_boundary)
    return out
