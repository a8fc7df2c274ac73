// The alignment of stage 4 (sc_align.hip) and of the read mapper (sc_map.hip): the exact optimum of bowtie2's --local scoring
// with a fixed tie-break (DESIGN.md §8.7 is the contract).  The sweep, the traceback window and its block loop are
// sc_wave_dp.hpp; here is what the two share beyond it:
//   * SwCell: the affine-gap cell (H, E and F; quality-dependent mismatch penalties; no gap in the --gbar rows).
//   * k_sw_score_of: the tile's best cell becomes one 64-bit key (score, then the tie-break of the contract: lower seed, forward
//     strand, smaller end column, smaller end row); per read one vector atomicMax keeps the best key and a second one the
//     best of the keys it displaced or beat, which is the best of every other (seed, strand): XS.  k_sw_score<R> takes the
//     full product of reads and seeds, k_sw_score_pairs<R> a list of (read, seed) pairs.
//   * k_sw_trace: one wavefront per aligned read; the walk through the direction nibbles gives POS, CIGAR, NM.
#pragma once
#include <cmath>
#include <cstring>

#include "sc_wave_dp.hpp"

namespace {

using namespace wave_dp;

constexpr int MAX_SEEDS = (1 << 20) - 1;        // the seed field of a key has 20 bits
constexpr int GBAR = 4;                 // --gbar 4
constexpr int GAP_OPEN = 8;             // --rdg 5,3 / --rfg 5,3: 5 + 3n for a gap of n
constexpr int GAP_EXT = 3;
constexpr int BARRED = 1 << 20;         // open / extend cost of a row where no gap may be
constexpr int NEG = -(1 << 20);         // E and F before any gap

// The key of a tile's best cell: score [63:53], 0xFFFFF - seed [52:33], forward [32], then cell_bits.  Larger is better.
__host__ __device__ inline unsigned long long make_key(int score, int seed, int strand, int col, int row) {
    return ((unsigned long long)score << 53) | ((unsigned long long)(0xFFFFF - seed) << 33) | ((unsigned long long)(1 - strand) << 32) |
           cell_bits(col, row);
}
__host__ __device__ inline int key_score(unsigned long long key) { return (int)(key >> 53); }
__host__ __device__ inline int key_seed(unsigned long long key) { return 0xFFFFF - (int)((key >> 33) & 0xFFFFF); }
__host__ __device__ inline int key_strand(unsigned long long key) { return 1 - (int)((key >> 32) & 1); }

struct SwCell {
    static constexpr int MATCH = 2, SKIP = GAP_EXT, BITS = 4;
    // A read row: base code with the strand applied, mismatch penalty (negative) and the gap costs of the row (--gbar).
    // rd[i] = code | penalty << 4 (code 0..3 = ACGT, 4 = other; penalty = 1 for other, else 2 + floor(min(Q,40) / 10)).
    struct RowData { int rb, pen, go, ge; };
    static __device__ __forceinline__ RowData load_row(const uint8_t* rd, int L, int strand, int nrows, int i) {
        RowData r{4, -1, BARRED, BARRED};
        if (i < nrows) {
            const int b = rd[strand ? L - 1 - i : i];
            int c = b & 15;
            if (strand && c < 4) c = 3 - c;
            r.rb = c;
            r.pen = -(b >> 4);
            if (i >= GBAR && i < L - GBAR) { r.go = GAP_OPEN; r.ge = GAP_EXT; }
        }
        return r;
    }
    struct Row { int E; };
    struct Carry { int f; };            // F of the lane's last row
    struct Out { int h; Row row; Carry carry; unsigned dir; };
    static __device__ __forceinline__ Row row0() { return Row{NEG}; }
    static __device__ __forceinline__ Carry carry0() { return Carry{NEG}; }
    static __device__ __forceinline__ Carry down(Carry c) { return Carry{shr1(NEG, c.f)}; }
    // a seed base outside ACGT scores -1 against anything
    static __device__ __forceinline__ int column(int rc) { return rc > 3 ? -1 : -64; }
    // dir bits 0-1: how H was reached -- 0 diagonal from a zero cell (the alignment starts here), 1 diagonal, 2 E (D), 3 F (I)
    //               (diagonal before D before I);
    //     bit 2: E extends E of the column before (extension preferred on a tie); bit 3: F extends F of the row above.
    static __device__ __forceinline__ Out cell(RowData r, int rc, int nv, int hd, int hp, int hu, Row row, Carry c) {
        const int eo = row.E - GAP_EXT, eg = hp - r.go;
        const int e = max(eo, eg);
        const int fo = c.f - r.ge, fg = hu - r.go;
        const int f = max(fo, fg);
        const int s = max(rc == r.rb ? 2 : r.pen, nv);
        const int d = hd + s;
        const int h = max(max(d, 0), max(e, f));
        return Out{h, Row{e}, Carry{f}, (h == d ? (hd > 0 ? 1u : 0u) : (h == e ? 2u : 3u)) | (eo >= eg ? 4u : 0u) | (fo >= fg ? 8u : 0u)};
    }
};

// One kernel for both tile sources of sc_wave_dp.hpp.  The tile's body stays in the kernel (the note at tile_of says why).
template <int R, class Tiles>
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_sw_score_of(const uint8_t* seeds, const long* seed_off, const uint8_t* rd,
                                                                  const long* rd_off, Tiles tiles, long n_tiles,
                                                                  unsigned long long* best, unsigned long long* second) {
    const int lane = threadIdx.x & 63;
    for (long w = first_tile(); w < n_tiles; w += tile_stride()) {
        const Tile t = tiles.at(w);
        const int read = t.item, seed = t.ref2 >> 1, strand = t.ref2 & 1;
        const long r0 = rd_off[read];
        const int L = (int)(rd_off[read + 1] - r0);
        const long s0 = seed_off[seed];
        const int ncols = (int)(seed_off[seed + 1] - s0);
        Rows<R, SwCell> rw;
        rw.load(rd + r0, L, strand, L, lane);
        unsigned keys[R];
        sweep<R, false, SwCell>(seeds + s0, ncols, rw, (L + R - 1) / R, lane, keys, nullptr, 0, -1);
        const BestCell b = best_cell<R>(keys, L, lane);
        if (lane == 0) {
            const unsigned long long key = b.score ? make_key(b.score, seed, strand, b.col, b.row) : 0ull;
            const unsigned long long old = atomicMax(best + read, key);
            atomicMax(second + read, old < key ? old : key);
        }
    }
}
template <int R> constexpr auto k_sw_score = k_sw_score_of<R, AllTiles>;
template <int R> constexpr auto k_sw_score_pairs = k_sw_score_of<R, PairTiles>;

// One aligned read per workgroup of one wavefront.  out[t*4 + 0..3] = 0-based start column on the seed, start row, NM,
// CIGAR operations (BAM codes, length << 4 | op, in read order at cig[t * stride]); -1 in [0] when the walk failed.
template <int R>
__global__ __launch_bounds__(64) void k_sw_trace(const uint8_t* seeds, const long* seed_off, const uint8_t* rd, const long* rd_off,
                                                 const int* tids, int n_trace, const unsigned long long* best, int* out, unsigned* cig,
                                                 int stride) {
    __shared__ unsigned bits[TB_COLS * 64];
    const int lane = threadIdx.x;
    for (int t = blockIdx.x; t < n_trace; t += gridDim.x) {
        const int read = tids[t];
        const unsigned long long key = best[read];
        const int strand = key_strand(key), iend = key_row(key);
        const long r0 = rd_off[read];
        const int L = (int)(rd_off[read + 1] - r0);
        const uint8_t* sq = seeds + seed_off[key_seed(key)];
        const int nrows = iend + 1;
        const Window w = trace_window<SwCell>(key_score(key), key_col(key), nrows);
        const int j0 = w.j0;
        Rows<R, SwCell> rw;
        rw.load(rd + r0, L, strand, nrows, lane);
        unsigned* oc = cig + (long)t * stride;
        int st = 0, i = iend, jw = w.ncol - 1, nm = 0, nops = 0, cur_op = -1, cur_len = 0, bad = 0, done = 0;
        auto push = [&](int op, int n) {
            if (op == cur_op) { cur_len += n; return; }
            if (cur_op >= 0) { if (nops < stride) oc[nops] = ((unsigned)cur_len << 4) | (unsigned)cur_op; else bad = 1; nops++; }
            cur_op = op; cur_len = n;
        };
        if (lane == 0 && L - 1 - iend > 0) push(4, L - 1 - iend);
        const int nl = (nrows + R - 1) / R;
        for (int b = last_block(w.ncol); b >= 0; b--) {
            const int colA = sweep_block<R, SwCell>(sq + j0, w.ncol, b, rw, nl, lane, bits);
            if (lane == 0) {
                while (!done && !bad && jw >= colA) {
                    if (i < 0) { bad = 1; break; }
                    const unsigned nib = dir_at<R, SwCell>(bits, jw - colA, i);
                    if (st == 0) {
                        const unsigned c = nib & 3u;
                        if (c <= 1) {
                            push(0, 1);
                            int rb = rd[r0 + (strand ? L - 1 - i : i)] & 15;
                            if (strand && rb < 4) rb = 3 - rb;
                            if (rb > 3 || rb != (int)sq[j0 + jw]) nm++;
                            if (c == 0) done = 1; else { i--; jw--; }
                        } else {
                            st = c == 2 ? 1 : 2;
                        }
                    } else if (st == 1) {
                        push(2, 1); nm++; jw--; st = (nib & 4u) ? 1 : 0;
                    } else {
                        push(1, 1); nm++; i--; st = (nib & 8u) ? 2 : 0;
                    }
                }
            }
            if (walk_over(done, bad)) break;
        }
        if (lane == 0) {
            if (!done || i < 0 || jw < 0) bad = 1;
            if (i > 0) push(4, i);
            push(-1, 0);                                 // flush
            if (bad || nops > stride) {
                out[t * 4 + 0] = -1;
            } else {
                for (int a = 0, z = nops - 1; a < z; a++, z--) { const unsigned x = oc[a]; oc[a] = oc[z]; oc[z] = x; }
                out[t * 4 + 0] = j0 + jw; out[t * 4 + 1] = i; out[t * 4 + 2] = nm; out[t * 4 + 3] = nops;
            }
        }
    }
}

// The read rows both entry points pack: code | penalty << 4 per base (SwCell::load_row reads it).
inline uint8_t read_row_byte(int code, const char* qual, long k) {
    int q = qual ? (int)(unsigned char)qual[k] - 33 : 40;
    q = std::min(std::max(q, 0), 40);
    const int pen = code < 0 ? 1 : 2 + q / 10;
    return (uint8_t)((code < 0 ? 4 : code) | (pen << 4));
}

// The second half of both entry points, from the score pass's keys (on the host and in d_best) on: as and xs of every read,
// the traceback of the reads whose best score is valid (>= 20 + 8 ln(length), in double) between the marks "trace" and
// "traced" of `st`, and seed, strand, pos, nm and the CIGAR of those; every other read gets seed -1.  *trace_cells (may be
// null) grows by the cells swept.  Returns the number of reads traced, or -1 - r when the walk of read r failed.  The stream
// is synchronised.
inline int trace_aligned(sc::TimedStream& st, const uint8_t* d_sq, const long* d_so, const uint8_t* d_rq, const long* d_ro,
                         const unsigned long long* d_best, const Packed& rd, const std::vector<unsigned long long>& best,
                         const std::vector<unsigned long long>& second, int* as, int* xs, int* seed, int* strand, int* pos, int* nm,
                         unsigned* cigar, int cigar_stride, int* n_cigar, long* trace_cells) {
    const int n_reads = (int)best.size();
    Buckets tr_r;
    for (int r = 0; r < n_reads; r++) {
        const double thr = 20.0 + 8.0 * std::log((double)rd.len(r));
        const int S = key_score(best[(size_t)r]), X = key_score(second[(size_t)r]);
        as[r] = S;
        xs[r] = (double)X >= thr ? X : -1;
        seed[r] = -1; strand[r] = 0; pos[r] = 0; nm[r] = 0; n_cigar[r] = 0;
        if ((double)S >= thr) tr_r.add(r, rd.len(r));
    }
    const std::vector<int> tids = tr_r.order();
    const int n_tr = (int)tids.size();
    std::vector<int> tout((size_t)n_tr * 4);
    std::vector<unsigned> tcig((size_t)n_tr * (size_t)cigar_stride);
    sc::DevMem<int> d_tids((size_t)n_tr), d_out(tout.size());
    sc::DevMem<unsigned> d_cig(tcig.size());
    st.h2d(d_tids, tids);
    st.mark("trace");
    tr_r.each([&](auto r, long at, const std::vector<int>& ids) {
        hipLaunchKernelGGL(k_sw_trace<decltype(r)::value>, trace_grid((int)ids.size()), dim3(64), 0, st, d_sq, d_so, d_rq, d_ro, d_tids.p + at,
                           (int)ids.size(), d_best, d_out.p + 4 * at, d_cig.p + at * cigar_stride, cigar_stride);
        st.launched();
    });
    st.mark("traced");
    st.d2h(tout, d_out); st.d2h(tcig, d_cig);
    st.sync();
    for (int t = 0; t < n_tr; t++) {
        const int r = tids[(size_t)t];
        const unsigned long long key = best[(size_t)r];
        if (tout[(size_t)t * 4] < 0) return -1 - r;
        seed[r] = key_seed(key);
        strand[r] = key_strand(key);
        pos[r] = tout[(size_t)t * 4] + 1;
        nm[r] = tout[(size_t)t * 4 + 2];
        n_cigar[r] = tout[(size_t)t * 4 + 3];
        std::memcpy(cigar + (long)r * cigar_stride, tcig.data() + (size_t)t * cigar_stride, sizeof(unsigned) * (size_t)n_cigar[r]);
        if (trace_cells) {
            const int nrows = key_row(key) + 1;
            *trace_cells += window_cells(trace_window<SwCell>(key_score(key), key_col(key), nrows), nrows, 0);
        }
    }
    return n_tr;
}

}  // namespace
