// The alignment of the gene profile (sc_profile.hip; DESIGN.md §8.9 is the contract): the exact optimum of blastn's 1/-2
// scoring with linear gaps and a fixed tie-break.  The sweep, the traceback window and its block loop are sc_wave_dp.hpp;
// here is what is the profile's own:
//   * BlCell: the linear-gap cell, only H per cell: max(0, diagonal + s, left - 5, up - 5) in doubled scores (+2 / -4 / -5).
//   * k_bl_score: a tile whose best doubled score reaches the segment's least passing score (E <= T, computed by the host
//     in double) appends one record (segment, gene, strand, best cell) to a bounded buffer: one vector atomicAdd per
//     emitted tile.  k_bl_score_pairs is the same kernel over a list of (segment, gene) pairs.
//   * k_bl_trace: one wavefront per (segment, gene) hit; the walk through the 2-bit directions gives start cell, identity,
//     alignment length.
//   * evalue_of, least_score2: E and the least passing score of a segment length, the host's half of the same contract.
#pragma once
#include <cmath>

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

// One kernel for both tile sources of sc_wave_dp.hpp (AllTiles, and PairTiles for the seeded mode): k_bl_score<R> is the full
// product, k_bl_score_pairs<R> the pair list.  The tile's body stays in the
// kernel: as a function of (segment, gene, strand), and as a function holding the whole loop, it cost a register per lane at
// R = 2..7 (the note at tile_of in sc_wave_dp.hpp says the same of its own case).
template <int R, class Tiles>
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_bl_score_of(const uint8_t* genes, const long* gene_off, const uint8_t* sg, const long* seg_off,
                                                                  Tiles tiles, const int* min2, long n_tiles, Cand* cand, unsigned cap,
                                                                  unsigned* n_cand) {
    const int lane = threadIdx.x & 63;
    for (long w = first_tile(); w < n_tiles; w += tile_stride()) {
        const Tile t = tiles.at(w);
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
template <int R> constexpr auto k_bl_score = k_bl_score_of<R, AllTiles>;
template <int R> constexpr auto k_bl_score_pairs = k_bl_score_of<R, PairTiles>;

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

// E = K m n e^(-lambda S) of a raw score S = score2 / 2, in double -- the one expression of the contract.
double evalue_of(double ka_k, double ka_lambda, int m, long n, int score2) {
    return ka_k * (double)m * (double)n * std::exp(-ka_lambda * (0.5 * (double)score2));
}

// The least doubled score of a segment of L bases with E <= T; above MATCH2 * L: the segment cannot pass.
int least_score2(double ka_k, double ka_lambda, int L, long n, double max_evalue) {
    int s2 = 1;
    while (s2 <= MATCH2 * L && !(evalue_of(ka_k, ka_lambda, L, n, s2) <= max_evalue)) s2++;
    return s2;
}

}  // namespace
