// The per-sample gene profile on the device: every read segment of a sample against every assembled gene on both strands,
// the exact optimum of blastn's 1/-2 scoring with linear gaps and a fixed tie-break (DESIGN.md §8.9 is the contract) -- what
// scripts/per_sample_gene_profile_fast.py:80-153 runs makeblastdb, blastn, bigBlastParser and sqlite3 for.  The sweep, the
// traceback window and its block loop are sc_wave_dp.hpp; this file holds what is the profile's own:
//   * BlCell: the linear-gap cell, only H per cell: max(0, diagonal + s, left - 5, up - 5) in doubled scores (+2 / -4 / -5).
//   * k_bl_score: a tile whose best doubled score reaches the segment's least passing score (E <= T, computed by the host
//     in double) appends one record (segment, gene, strand, best cell) to a bounded buffer: one vector atomicAdd per
//     emitted tile.
//   * k_bl_trace: one wavefront per (segment, gene) hit; the walk through the 2-bit directions gives start cell, identity,
//     alignment length.
#include <cmath>
#include <cstring>

#include "sc_wave_dp.hpp"

namespace {

using namespace wave_dp;

constexpr int MATCH2 = 2;               // doubled: match +1
constexpr int MISMATCH2 = -4;           // mismatch -2 (a base outside ACGT on either side is a mismatch)
constexpr int GAP2 = 5;                 // a gap of n bases -2.5 n

// A tile's best cell: doubled score [63:32], then cell_bits.  Larger is better.
__host__ __device__ inline unsigned long long make_key(int score2, int col, int row) { return ((unsigned long long)score2 << 32) | cell_bits(col, row); }
__host__ __device__ inline int key_score2(unsigned long long key) { return (int)(key >> 32); }

struct Cand {
    int seg, gene2;                     // gene2 = gene * 2 + strand
    unsigned long long key;
};

struct BlCell {
    static constexpr int MATCH = MATCH2, SKIP = GAP2, BITS = 2;
    // A segment row: its base code with the strand applied (0..3 = ACGT, 4 = other, also beyond the last row).
    struct RowData { int rb; };
    static __device__ __forceinline__ RowData load_row(const uint8_t* sg, int L, int strand, int nrows, int i) {
        if (i >= nrows) return RowData{4};
        const int c = sg[strand ? L - 1 - i : i];
        return RowData{strand && c < 4 ? 3 - c : c};
    }
    struct Row {};                      // H is all the state there is
    struct Carry {};
    struct Out { int h; Row row; Carry carry; unsigned dir; };
    static __device__ __forceinline__ Row row0() { return Row{}; }
    static __device__ __forceinline__ Carry carry0() { return Carry{}; }
    static __device__ __forceinline__ Carry down(Carry c) { return c; }
    static __device__ __forceinline__ int column(int) { return 0; }
    // dir: 0 diagonal from a zero cell (the alignment starts here), 1 diagonal, 2 left (a gap in the segment), 3 up (a gap in
    // the gene) -- in that order of preference
    static __device__ __forceinline__ Out cell(RowData r, int gc, int, int hd, int hp, int hu, Row row, Carry c) {
        const int d = hd + (gc == r.rb ? MATCH2 : MISMATCH2);
        const int l = hp - GAP2, u = hu - GAP2;
        const int h = max(max(d, 0), max(l, u));
        return Out{h, row, c, h == d ? (hd > 0 ? 1u : 0u) : (h == l ? 2u : 3u)};
    }
};

template <int R>
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_bl_score(const uint8_t* genes, const long* gene_off, int n_genes, const uint8_t* sg,
                                                               const long* seg_off, const int* sids, const int* min2, long n_tiles,
                                                               Cand* cand, unsigned cap, unsigned* n_cand) {
    const int lane = threadIdx.x & 63;
    for (long w = first_tile(); w < n_tiles; w += tile_stride()) {
        const Tile t = tile_of(w, n_genes, sids);
        const int seg = t.item, gene = t.ref2 >> 1, strand = t.ref2 & 1;
        const long r0 = seg_off[seg];
        const int L = (int)(seg_off[seg + 1] - r0);
        const long g0 = gene_off[gene];
        const int ncols = (int)(gene_off[gene + 1] - g0);
        Rows<R, BlCell> rw;
        rw.load(sg + r0, L, strand, L, lane);
        unsigned keys[R];
        sweep<R, false, BlCell>(genes + g0, ncols, rw, (L + R - 1) / R, lane, keys, nullptr, 0, -1);
        const BestCell b = best_cell<R>(keys, L, lane);
        if (lane == 0 && b.score >= min2[seg]) {
            const unsigned slot = atomicAdd(n_cand, 1u);
            if (slot < cap) { cand[slot].seg = seg; cand[slot].gene2 = t.ref2; cand[slot].key = make_key(b.score, b.col, b.row); }
        }
    }
}

// One hit per workgroup of one wavefront.  out[t*4 + 0..3] = 0-based start column on the gene, start row, identity (columns
// with equal ACGT bases), alignment length (columns); -1 in [0] when the walk failed.
template <int R>
__global__ __launch_bounds__(64) void k_bl_trace(const uint8_t* genes, const long* gene_off, const uint8_t* sg, const long* seg_off,
                                                 const Cand* hits, int n_trace, int* out) {
    __shared__ unsigned bits[TB_COLS * 64];
    const int lane = threadIdx.x;
    for (int t = blockIdx.x; t < n_trace; t += gridDim.x) {
        const int seg = hits[t].seg, gene = hits[t].gene2 >> 1, strand = hits[t].gene2 & 1;
        const unsigned long long key = hits[t].key;
        const int iend = key_row(key);
        const long r0 = seg_off[seg];
        const int L = (int)(seg_off[seg + 1] - r0);
        const uint8_t* gq = genes + gene_off[gene];
        const int nrows = iend + 1;
        const Window w = trace_window<BlCell>(key_score2(key), key_col(key), nrows);
        const int j0 = w.j0;
        Rows<R, BlCell> rw;
        rw.load(sg + r0, L, strand, nrows, lane);
        int i = iend, jw = w.ncol - 1, ident = 0, alen = 0, bad = 0, done = 0;
        const int nl = (nrows + R - 1) / R;
        for (int b = last_block(w.ncol); b >= 0; b--) {
            const int colA = sweep_block<R, BlCell>(gq + j0, w.ncol, b, rw, nl, lane, bits);
            if (lane == 0) {
                while (!done && jw >= colA) {
                    if (i < 0) { bad = 1; break; }
                    const unsigned c = dir_at<R, BlCell>(bits, jw - colA, i);
                    alen++;
                    if (c <= 1) {
                        int rb = sg[r0 + (strand ? L - 1 - i : i)];
                        if (strand && rb < 4) rb = 3 - rb;
                        if (rb == (int)gq[j0 + jw]) ident++;
                        if (c == 0) done = 1; else { i--; jw--; }
                    } else if (c == 2) {
                        jw--;
                    } else {
                        i--;
                    }
                }
            }
            if (walk_over(done, bad)) break;
        }
        if (lane == 0) {
            if (!done || bad || i < 0 || jw < 0) {
                out[t * 4 + 0] = -1;
            } else {
                out[t * 4 + 0] = j0 + jw; out[t * 4 + 1] = i; out[t * 4 + 2] = ident; out[t * 4 + 3] = alen;
            }
        }
    }
}

thread_local LastError tl_error;

// E = K m n e^(-lambda S) of a raw score S = score2 / 2, in double -- the one expression of the contract.
double evalue_of(double ka_k, double ka_lambda, int m, long n, int score2) {
    return ka_k * (double)m * (double)n * std::exp(-ka_lambda * (0.5 * (double)score2));
}

}  // namespace

extern "C" {

const char* sc_profile_error(void) { return tl_error.text.c_str(); }

int sc_profile_hits(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                    int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg, int* hit_gene,
                    int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                    double* evalue, long cap, long* n_hits, sc_profile_stats* stats) try {
    tl_error.text.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_hits) *n_hits = 0;
    if (!gene_text || !gene_off || n_genes < 1 || n_segs < 0 || (n_segs > 0 && (!seg_text || !seg_off)) || !hit_seg || !hit_gene ||
        !hit_strand || !hit_score || !identity || !align_len || !qfrom || !qto || !hfrom || !hto || !evalue || cap < 0 || !n_hits)
        return tl_error.fail(SC_ERR_ARG, "sc_profile_hits: missing argument");
    if (!(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0))
        return tl_error.fail(SC_ERR_ARG, "sc_profile_hits: lambda and K must be positive, the E-value threshold not negative");
    Packed gn, sg;
    std::string why;
    if (!gn.rebase(gene_off, n_genes, MAX_COLS, "sc_profile_hits", "gene", why) ||
        (n_segs > 0 && !sg.rebase(seg_off, n_segs, MAX_ROWS, "sc_profile_hits", "segment", why)))
        return tl_error.fail(SC_ERR_UNSUPPORTED, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return tl_error.fail(SC_ERR_NO_DEVICE, "no HIP device");
    if (hipSetDevice(device) != hipSuccess) return tl_error.fail(SC_ERR_HIP, "hipSetDevice failed");
    if (n_segs == 0) return SC_OK;
    const double t0 = sc::now_ms();
    // ---- host packing: gene and segment codes; per segment length the least doubled score with E <= T; segments bucketed by
    // rows per lane (a segment that cannot pass even with every base matched is in no bucket)
    gn.pack(gene_text + gene_off[0], [](long, int c) { return c < 0 ? REF_OTHER : c; });
    sg.pack(seg_text + seg_off[0], [](long, int c) { return c < 0 ? 4 : c; });
    const long gene_bytes = gn.bytes();
    int min2_of_len[MAX_ROWS + 1] = {};                         // 0: not computed yet (a hit has a positive score)
    std::vector<int> min2((size_t)n_segs);
    Buckets by_r;
    for (int r = 0; r < n_segs; r++) {
        const int L = (int)sg.len(r);
        int& s2 = min2_of_len[L];
        if (s2 == 0)
            for (s2 = 1; s2 <= MATCH2 * L && !(evalue_of(ka_k, ka_lambda, L, gene_bytes, s2) <= max_evalue);) s2++;
        min2[(size_t)r] = s2;
        if (s2 <= MATCH2 * L) by_r.add(r, L);
    }
    const std::vector<int> sids = by_r.order();
    const long n_tiles = (long)sids.size() * 2L * n_genes;
    if (n_tiles > 0x7FFFFFFFL)
        return tl_error.fail(SC_ERR_UNSUPPORTED, "sc_profile_hits: " + std::to_string(n_tiles) + " (segment, gene, strand) tiles in one call (at most "
                                                     "2147483647: pass the segments in several calls)");
    // every passing tile is a candidate; a (segment, gene) pair gives at most two, so 2 * cap + 1024 records hold them unless
    // the caller's cap is too small as well
    const long cand_cap = std::min<long>(n_tiles, std::min<long>(2 * cap + 1024, 0x7FFFFFFFL));
    // ---- device: the score pass
    sc::DevMem<uint8_t> d_gq(gn.codes.size()), d_sq(sg.codes.size());
    sc::DevMem<long> d_go(gn.off.size()), d_so(sg.off.size());
    sc::DevMem<int> d_sids(sids.size()), d_min2(min2.size());
    sc::DevMem<Cand> d_cand((size_t)cand_cap);
    sc::DevMem<unsigned> d_ncand(1);
    sc::TimedStream st;
    st.mark("upload");
    st.h2d(d_gq, gn.codes); st.h2d(d_go, gn.off); st.h2d(d_sq, sg.codes); st.h2d(d_so, sg.off); st.h2d(d_sids, sids); st.h2d(d_min2, min2);
    st.zero(d_ncand.p, sizeof(unsigned));
    st.mark("score");
    by_r.each([&](auto r, long at, const std::vector<int>& ids) {
        const long nt = (long)ids.size() * 2L * n_genes;
        hipLaunchKernelGGL(k_bl_score<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d_gq.p, d_go.p, n_genes, d_sq.p, d_so.p,
                           d_sids.p + at, d_min2.p, nt, d_cand.p, (unsigned)cand_cap, d_ncand.p);
        st.launched();
        if (stats) for (int id : ids) stats->score_cells += 2L * sg.len(id) * gene_bytes;
    });
    st.mark("scored");
    unsigned n_cand = 0;
    st.d2h(&n_cand, d_ncand.p, sizeof(unsigned));
    st.sync();
    if (stats) { stats->n_tiles = n_tiles; stats->n_candidates = (long)n_cand; }
    int rc = SC_OK;
    if ((long)n_cand > cand_cap) {
        *n_hits = (long)n_cand;                                  // an upper bound of the hits: a cap of this size suffices
        rc = tl_error.fail(SC_ERR_CAPACITY, "sc_profile_hits: " + std::to_string(n_cand) + " tiles pass the E-value threshold, room for " +
                                                std::to_string(cap) + " hits");
    } else {
        std::vector<Cand> cand(n_cand);
        if (n_cand) HIPCHK(hipMemcpy(cand.data(), d_cand.p, (size_t)n_cand * sizeof(Cand), hipMemcpyDeviceToHost));
        // ---- per (segment, gene) the better strand (ties: forward), in (segment, gene) order; the traceback of those, bucketed
        // by rows per lane again
        std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.seg != b.seg ? a.seg < b.seg : a.gene2 < b.gene2; });
        std::vector<Cand> pick;
        for (size_t k = 0; k < cand.size(); k++) {
            if (!pick.empty() && pick.back().seg == cand[k].seg && (pick.back().gene2 >> 1) == (cand[k].gene2 >> 1)) {
                if (key_score2(cand[k].key) > key_score2(pick.back().key)) pick.back() = cand[k];      // reverse only when strictly better
            } else {
                pick.push_back(cand[k]);
            }
        }
        Buckets tr_r;
        for (size_t k = 0; k < pick.size(); k++) tr_r.add((int)k, sg.len(pick[k].seg));
        const std::vector<int> order = tr_r.order();
        const int n_tr = (int)order.size();
        std::vector<Cand> tlist((size_t)n_tr);
        for (int t = 0; t < n_tr; t++) tlist[(size_t)t] = pick[(size_t)order[(size_t)t]];
        std::vector<int> tout((size_t)n_tr * 4);
        sc::DevMem<Cand> d_hits((size_t)n_tr);
        sc::DevMem<int> d_out(tout.size());
        st.h2d(d_hits, tlist);
        st.mark("trace");
        tr_r.each([&](auto r, long at, const std::vector<int>& ids) {
            hipLaunchKernelGGL(k_bl_trace<decltype(r)::value>, trace_grid((int)ids.size()), dim3(64), 0, st, d_gq.p, d_go.p, d_sq.p, d_so.p,
                               d_hits.p + at, (int)ids.size(), d_out.p + 4 * at);
            st.launched();
        });
        st.mark("traced");
        st.d2h(tout, d_out);
        st.sync();
        // ---- the hits that pass, back in (segment, gene) order
        std::vector<int> slot_of((size_t)n_tr);
        for (int t = 0; t < n_tr; t++) slot_of[(size_t)order[(size_t)t]] = t;
        long n_out = 0;
        for (int k = 0; k < n_tr; k++) {
            const int t = slot_of[(size_t)k];
            const Cand& c = pick[(size_t)k];
            const int* o = &tout[(size_t)t * 4];
            if (o[0] < 0) {
                rc = tl_error.fail(SC_ERR_INTERNAL, "sc_profile_hits: traceback of segment " + std::to_string(c.seg) + " on gene " +
                                                        std::to_string(c.gene2 >> 1) + " failed");
                break;
            }
            const int L = (int)sg.len(c.seg);
            const int S2 = key_score2(c.key), jend = key_col(c.key), iend = key_row(c.key);
            const int strand = c.gene2 & 1, j0 = o[0], i0 = o[1];
            if (stats) {
                const Window w = trace_window<BlCell>(S2, jend, iend + 1);
                stats->trace_cells += window_cells(w, iend + 1, j0 - w.j0);
            }
            const double e = evalue_of(ka_k, ka_lambda, L, gene_bytes, S2);
            if (!(100.0 * (double)o[2] / (double)o[3] >= min_identity_pct) || !(e <= max_evalue)) continue;
            if (n_out < cap) {
                hit_seg[n_out] = c.seg; hit_gene[n_out] = c.gene2 >> 1; hit_strand[n_out] = strand;
                hit_score[n_out] = 0.5 * (double)S2; identity[n_out] = o[2]; align_len[n_out] = o[3];
                qfrom[n_out] = strand ? L - iend : i0 + 1;
                qto[n_out] = strand ? L - i0 : iend + 1;
                hfrom[n_out] = strand ? jend + 1 : j0 + 1;
                hto[n_out] = strand ? j0 + 1 : jend + 1;
                evalue[n_out] = e;
            }
            n_out++;
        }
        if (rc == SC_OK) {
            *n_hits = n_out;
            if (n_out > cap) rc = tl_error.fail(SC_ERR_CAPACITY, "sc_profile_hits: " + std::to_string(n_out) + " hits, room for " + std::to_string(cap));
        }
        if (stats && (rc == SC_OK || rc == SC_ERR_CAPACITY)) {
            read_phase_ms(st, stats);
            stats->n_traced = n_tr;
            stats->n_hits = n_out;
        }
    }
    if (stats) stats->total_ms = sc::now_ms() - t0;
    return rc;
} catch (const sc::HipError&) {
    return tl_error.fail(SC_ERR_HIP, "sc_profile_hits: a HIP call failed");
}

}  // extern "C"
