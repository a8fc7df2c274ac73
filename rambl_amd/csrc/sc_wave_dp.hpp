// The wavefront DP that stage 4 (sc_align.hip) and the gene profile (sc_profile.hip) share: a local alignment of up to 512
// rows (a read, a segment) against a reference of up to 8 192 columns (a seed, a gene) by one wavefront.
//   * Score pass: one wavefront per (row item, reference, strand) tile.  Lane l owns rows [l*R, l*R + R), R = ceil(L / 64),
//     and the reference is swept column by column as a systolic array: at step t lane l computes column t - l; the state of
//     its last row and the reference base move one lane down per step by DPP (wave_shr:1), so a cell never goes through LDS.
//     Per row the lane keeps max(H << 13 | 8191 - column); best_cell() turns that into the tile's best cell.
//   * Traceback pass: one wavefront per alignment recomputes only the window that can hold it (trace_window), in blocks of
//     TB_COLS columns whose direction bits live in LDS; lane 0 walks back through a block, and the block before it is
//     recomputed from the window start when the walk leaves it (sweep_block, walk_over).
// A family is a policy struct `Cell`; nothing here branches on it at run time:
//     MATCH, SKIP   the score of a matching row and the least cost of a skipped reference base (the window's bound)
//     BITS          direction bits per cell
//     RowData       what a lane knows of one row; load_row(rows, L, strand, nrows, i) makes it (i >= nrows: a row that never
//                   matches)
//     Row, Carry    the DP state of a row besides H / what a lane hands to the next one besides H of its last row, with
//                   row0(), carry0() and down(carry): the carry moved one lane down
//     column(rc)    per-column prologue, handed to every cell of the column
//     cell(data, rc, col, hd, hp, hu, row, carry) -> Out{h, row, carry, dir}: H of the cell from H of the diagonal, left
//                   and upper neighbour, the new state and the direction bits
// Everything goes to and from the policy by value, one row at a time, and the sweep keeps the H chain itself.  A cell
// that indexed the lane's arrays (cell(rows, k, ...)) compiled to another schedule of the same instructions: a register
// more at R = 2 and 3 and a stage-4 score pass 1.6 % slower.
// Integer DP in int32; scores stay below 2^11.  No scratch: every per-row array is unrolled into registers.
// The host half below is what the two entry points share around the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/straincall_hip.h"
#include "sc_host.hpp"

namespace wave_dp {

constexpr int MAX_ROWS = 512;           // the row field of a key has 9 bits,
constexpr int MAX_COLS = 8192;          // the column field 13
constexpr int TB_COLS = 128;            // columns of direction words in LDS per block: 128 * 64 lanes * 4 B = 32 KiB
constexpr int REF_OTHER = 5;            // reference code of a base outside ACGT (a row's is 4: the two never match)
// launch geometry: score tiles by 4 wavefronts per block in a grid-stride loop, one traceback per block of one wavefront
constexpr int SCORE_WAVES = 4, SCORE_BLOCKS = 16384, TRACE_BLOCKS = 8192;

// one lane down: lane l receives lane l - 1's value, lane 0 receives `first`
__device__ __forceinline__ int shr1(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false); }

// Both families' keys end in 8191 - end column [31:19], 511 - end row [18:10]: of equal scores the smaller column, then the
// smaller row is the larger key.
__host__ __device__ inline unsigned long long cell_bits(int col, int row) {
    return ((unsigned long long)(8191 - col) << 19) | ((unsigned long long)(511 - row) << 10);
}
__host__ __device__ inline int key_col(unsigned long long key) { return 8191 - (int)((key >> 19) & 8191); }
__host__ __device__ inline int key_row(unsigned long long key) { return 511 - (int)((key >> 10) & 511); }

// The traceback window of an alignment of score S that ends at (row nrows - 1, column jend): rows 0..nrows - 1 and columns
// j0..jend.  The alignment skips at most (MATCH * nrows - S) / SKIP reference bases, so it starts at j0 or later.
struct Window { int j0, ncol; };
template <class Cell> __host__ __device__ inline Window trace_window(int S, int jend, int nrows) {
    const int nd = (Cell::MATCH * nrows - S) / Cell::SKIP;
    int j0 = jend - nrows - (nd > 0 ? nd : 0) + 1;
    if (j0 < 0) j0 = 0;
    return Window{j0, jend - j0 + 1};
}
// The cells the block loop sweeps over a window when the walk ends in window column `last`: block b costs the columns from
// the window start to the block's end.  The two families report different numbers on purpose: stage 4 counts every block
// of the window (last = 0), the profile only the blocks its walk reached (last = the alignment's first column).
__host__ __device__ inline long window_cells(Window w, int nrows, int last) {
    long cols = 0;
    for (int b = (w.ncol - 1) / TB_COLS; b >= last / TB_COLS; b--) cols += w.ncol < (b + 1) * TB_COLS ? w.ncol : (b + 1) * TB_COLS;
    return cols * nrows;
}

// The rows of one lane: rows [lane * R, lane * R + R).
template <int R, class Cell> struct Rows {
    typename Cell::RowData d[R];
    __device__ __forceinline__ void load(const uint8_t* rows, int L, int strand, int nrows, int lane) {
#pragma unroll
        for (int k = 0; k < R; k++) d[k] = Cell::load_row(rows, L, strand, nrows, lane * R + k);
    }
};

// The systolic sweep over reference columns [0, ncols) of `ref` (codes).  SCORE: keys[k] = max over the columns of
// (H << 13 | 8191 - column) per row.  TRACE: the direction bits of every cell of columns [colA, colB] go to
// bits[(column - colA) * 64 + lane], bits [BITS * k, BITS * (k + 1)) of the word for row lane*R + k.
template <int R, bool TRACE, class Cell>
__device__ __forceinline__ void sweep(const uint8_t* ref, int ncols, const Rows<R, Cell>& rw, int nl, int lane, unsigned* keys,
                                      unsigned* bits, int colA, int colB) {
    int H[R];
    typename Cell::Row row[R];
#pragma unroll
    for (int k = 0; k < R; k++) { H[k] = 0; row[k] = Cell::row0(); if (!TRACE) keys[k] = 0; }
    typename Cell::Carry out = Cell::carry0();
    int hout = 0, hdiag = 0, rc = REF_OTHER, refbuf = REF_OTHER;
    const int steps = ncols + nl - 1;
    for (int t = 0; t < steps; t++) {
        if ((t & 63) == 0) { const int c = t + lane; refbuf = c < ncols ? (int)ref[c] : REF_OTHER; }
        const int fresh = __builtin_amdgcn_readlane(refbuf, t & 63);
        const int hup = shr1(0, hout);
        const typename Cell::Carry up = Cell::down(out);
        rc = shr1(fresh, rc);
        const int j = t - lane;
        if (j >= 0 && j < ncols && lane < nl) {
            const auto col = Cell::column(rc);
            int hd = hdiag, hu = hup;
            typename Cell::Carry c = up;
            unsigned word = 0;
            const unsigned cj = 8191u - (unsigned)j;
#pragma unroll
            for (int k = 0; k < R; k++) {
                const int hp = H[k];
                const typename Cell::Out o = Cell::cell(rw.d[k], rc, col, hd, hp, hu, row[k], c);
                const int h = o.h;
                c = o.carry;
                if (TRACE) word |= o.dir << (Cell::BITS * k);
                else keys[k] = max(keys[k], ((unsigned)h << 13) | cj);
                row[k] = o.row; H[k] = h; hd = hp; hu = h;
            }
            hout = hu; out = c;
            if (TRACE && j >= colA && j <= colB) bits[(j - colA) * 64 + lane] = word;
        }
        hdiag = hup;
    }
}

// The direction bits of (window column colA + dcol, row i) after a TRACE sweep.
template <int R, class Cell> __device__ __forceinline__ unsigned dir_at(const unsigned* bits, int dcol, int i) {
    return (bits[dcol * 64 + i / R] >> (Cell::BITS * (i % R))) & ((1u << Cell::BITS) - 1u);
}

// The best cell of a tile from the row keys of a SCORE sweep, the same in every lane: the largest score, then the smaller
// end column, then the smaller end row.  score == 0: no cell is positive.
struct BestCell { int score, col, row; };
template <int R> __device__ __forceinline__ BestCell best_cell(const unsigned* keys, int L, int lane) {
    unsigned lb = 0;
    int lrow = 0;
#pragma unroll
    for (int k = 0; k < R; k++)
        if (lane * R + k < L && keys[k] > lb) { lb = keys[k]; lrow = lane * R + k; }
    unsigned long long key = lb ? ((unsigned long long)(lb >> 13) << 32) | cell_bits(8191 - (int)(lb & 8191u), lrow) : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long x = __shfl_xor(key, o);
        key = x > key ? x : key;
    }
    return BestCell{(int)(key >> 32), key_col(key), key_row(key)};
}

// The tiles of a wavefront in a score kernel of SCORE_WAVES wavefronts per block: `for (long w = first_tile(); w < n_tiles;
// w += tile_stride())`, w = (item index * n_refs + reference) * 2 + strand.  The rest of a tile stays in the kernel: moved
// into a function of this header, inlined or not, it cost a register per lane at R = 2..7.
__device__ __forceinline__ long first_tile() { return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6))); }
__device__ __forceinline__ long tile_stride() { return (long)gridDim.x * SCORE_WAVES; }
struct Tile { int item, ref2; };        // ref2 = reference * 2 + strand
__device__ __forceinline__ Tile tile_of(long w, int n_refs, const int* ids) {
    const long ix = w / (2L * n_refs);
    return Tile{ids[ix], (int)(w - ix * 2L * n_refs)};
}

// Where a score kernel's tiles come from.  AllTiles: every bucket item against every reference on both strands (tile_of).
// PairTiles: tile w is pair w >> 1 on strand w & 1, so a pair is always scored on both strands (the better strand is picked
// before any filter; one strand alone could turn "no hit" into a hit).  `seg` is the row item of a pair, whatever the family
// calls it.
struct Pair { int seg, gene; };
struct AllTiles {
    int n_genes; const int* sids;
    __device__ __forceinline__ Tile at(long w) const { return tile_of(w, n_genes, sids); }
};
struct PairTiles {
    const Pair* pairs;
    __device__ __forceinline__ Tile at(long w) const { const Pair p = pairs[w >> 1]; return Tile{p.seg, p.gene * 2 + (int)(w & 1)}; }
};

// The block loop of a traceback by one wavefront, the window's last block first:
//     for (int b = last_block(ncol); b >= 0; b--) {
//         const int colA = sweep_block<R, Cell>(ref, ncol, b, rw, nl, lane, bits);
//         if (lane == 0) { ... walk while the column is colA or later; set done or bad ... }
//         if (walk_over(done, bad)) break;
//     }
// sweep_block sweeps block b from the window start `ref` into `bits` (LDS, TB_COLS * 64 words) and returns its first
// column; walk_over gives every lane lane 0's done | bad.  The walk is written in the kernel's own loop and not handed
// over as a lambda: through a closure its loop came out with more branches, and the profile's traceback pass 5 % slower.
__device__ __forceinline__ int last_block(int ncol) { return (ncol - 1) / TB_COLS; }
template <int R, class Cell>
__device__ __forceinline__ int sweep_block(const uint8_t* ref, int ncol, int b, const Rows<R, Cell>& rw, int nl, int lane, unsigned* bits) {
    const int colA = b * TB_COLS, colB = min(colA + TB_COLS, ncol) - 1;
    sweep<R, true, Cell>(ref, colB + 1, rw, nl, lane, nullptr, bits, colA, colB);
    __syncthreads();
    return colA;
}
__device__ __forceinline__ bool walk_over(int& done, int bad) {
    done = __shfl(done | bad, 0);
    __syncthreads();
    return done;
}

// ------------------------------------------------------------------------------------------------------------ host

inline dim3 score_grid(long n_tiles) { return dim3((unsigned)std::min<long>((n_tiles + SCORE_WAVES - 1) / SCORE_WAVES, SCORE_BLOCKS)); }
inline dim3 trace_grid(int n) { return dim3((unsigned)std::min(n, TRACE_BLOCKS)); }

// f(std::integral_constant<int, R>) for the instantiation of R rows per lane
template <class F> void dispatch_by_rows(int R, F&& f) {
    switch (R) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
    }
}

// Items bucketed by rows per lane, R = ceil(length / 64), in the order they were added.
struct Buckets {
    std::vector<int> by_r[MAX_ROWS / 64];
    void add(int id, long len) { by_r[(len + 63) / 64 - 1].push_back(id); }
    std::vector<int> order() const {
        std::vector<int> ids;
        for (auto& v : by_r) ids.insert(ids.end(), v.begin(), v.end());
        return ids;
    }
    // f(R as an integral_constant, where the bucket starts in order(), its items) for every bucket that has any
    template <class F> void each(F&& f) const {
        long at = 0;
        for (int k = 0; k < MAX_ROWS / 64; k++) {
            if (by_r[k].empty()) continue;
            dispatch_by_rows(k + 1, [&](auto r) { f(r, at, by_r[k]); });
            at += (long)by_r[k].size();
        }
    }
};

inline int code_of(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

// The sequences of one side of a call, off[n + 1] into a text: rebase() checks every length and moves the offsets to start
// at 0, pack() turns the text into one code byte per base.
struct Packed {
    std::vector<long> off;
    std::vector<uint8_t> codes;
    long bytes() const { return off.back(); }
    long len(int k) const { return off[(size_t)k + 1] - off[(size_t)k]; }
    // false with `why` set ("<fn>: <noun> 3 has 9000 bases (1..8192 supported)") when a length is not in 1..max_len
    bool rebase(const long* from, int n, int max_len, const char* fn, const char* noun, std::string& why) {
        off.resize((size_t)n + 1);
        for (int k = 0; k <= n; k++) off[(size_t)k] = from[k] - from[0];
        for (int k = 0; k < n; k++)
            if (len(k) < 1 || len(k) > max_len) {
                why = std::string(fn) + ": " + noun + " " + std::to_string(k) + " has " + std::to_string(len(k)) + " bases (1.." +
                      std::to_string(max_len) + " supported)";
                return false;
            }
        return true;
    }
    // codes[k] = code(k, code_of(text[k])) over the text from the first sequence on
    template <class F> void pack(const char* text, F code) {
        codes.resize((size_t)bytes());
        for (long k = 0; k < bytes(); k++) codes[(size_t)k] = (uint8_t)code(k, code_of(text[k]));
    }
};

// upload_ms, score_ms and trace_ms of a family's statistics from the marks both entry points set
template <class Stats> void read_phase_ms(const sc::TimedStream& st, Stats* stats) {
    stats->upload_ms = st.ms("upload", "score");
    stats->score_ms = st.ms("score", "scored");
    stats->trace_ms = st.ms("trace", "traced");
}

}  // namespace wave_dp
