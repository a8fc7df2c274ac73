// Stage 4 of rambl.py on the device: every gene read aligned to every seed OTU on both strands, the exact optimum of
// bowtie2's --local scoring (DESIGN.md §8.7 is the contract) -- what scripts/recluster_data_to_seed_otus.py:198-277
// runs bowtie2 --sensitive-local for.  The sweep, the traceback window and its block loop are sc_wave_dp.hpp; this file
// holds what is stage 4's own:
//   * SwCell: the affine-gap cell (H, E and F; quality-dependent mismatch penalties; no gap in the --gbar rows).
//   * k_sw_score: the tile's best cell becomes one 64-bit key (score, then the tie-break of the contract: lower seed, forward
//     strand, smaller end column, smaller end row); per read one vector atomicMax keeps the best key and a second one the
//     best of the keys it displaced or beat, which is the best of every other (seed, strand): XS.
//   * k_sw_trace: one wavefront per aligned read; the walk through the direction nibbles gives POS, CIGAR, NM.
#include <cmath>
#include <cstring>

#include "sc_wave_dp.hpp"

namespace {

using namespace wave_dp;

constexpr int MAX_SEEDS = (1 << 20) - 1;
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

template <int R>
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_sw_score(const uint8_t* seeds, const long* seed_off, int n_seeds, const uint8_t* rd,
                                                               const long* rd_off, const int* rids, long n_tiles,
                                                               unsigned long long* best, unsigned long long* second) {
    const int lane = threadIdx.x & 63;
    for (long w = first_tile(); w < n_tiles; w += tile_stride()) {
        const Tile t = tile_of(w, n_seeds, rids);
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

thread_local sc::LastError tl_error;

}  // namespace

extern "C" {

const char* sc_align_error(void) { return tl_error.text.c_str(); }

int sc_align_reads(int device, const char* seed_text, const long* seed_off, int n_seeds, const char* read_text, const char* qual_text,
                   const long* read_off, int n_reads, int* as, int* xs, int* seed, int* strand, int* pos, int* nm, unsigned* cigar,
                   int cigar_stride, int* n_cigar, sc_align_stats* stats) {
    tl_error.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    return sc::guarded(&tl_error, "sc_align_reads", [&] {
        if (!seed_text || !seed_off || n_seeds < 1 || n_reads < 0 || (n_reads > 0 && (!read_text || !read_off)) || !as || !xs || !seed ||
            !strand || !pos || !nm || !cigar || cigar_stride < 1 || !n_cigar)
            return tl_error.fail(SC_ERR_ARG, "sc_align_reads: missing argument");
        if (n_seeds > MAX_SEEDS) return tl_error.fail(SC_ERR_UNSUPPORTED, "sc_align_reads: more than 1048575 seeds");
        Packed sd, rd;
        std::string why;
        if (!sd.rebase(seed_off, n_seeds, MAX_COLS, "sc_align_reads", "seed", why) ||
            (n_reads > 0 && !rd.rebase(read_off, n_reads, MAX_ROWS, "sc_align_reads", "read", why)))
            return tl_error.fail(SC_ERR_UNSUPPORTED, why);
        long max_len = 0;
        for (int r = 0; r < n_reads; r++) max_len = std::max(max_len, rd.len(r));
        if (cigar_stride < max_len / 2 + 4) return tl_error.fail(SC_ERR_CAPACITY, "sc_align_reads: cigar_stride below max read length / 2 + 4");
        sc::select_device(device);
        if (n_reads == 0) return SC_OK;
        const double t0 = sc::now_ms();
        // ---- host packing: seed codes, read code | penalty << 4, reads bucketed by rows per lane
        sd.pack(seed_text + seed_off[0], [](long, int c) { return c < 0 ? REF_OTHER : c; });
        rd.pack(read_text + read_off[0], [&](long k, int c) {
            int q = qual_text ? (int)(unsigned char)qual_text[read_off[0] + k] - 33 : 40;
            q = std::min(std::max(q, 0), 40);
            const int pen = c < 0 ? 1 : 2 + q / 10;
            return (c < 0 ? 4 : c) | (pen << 4);
        });
        Buckets by_r;
        for (int r = 0; r < n_reads; r++) by_r.add(r, rd.len(r));
        const std::vector<int> rids = by_r.order();
        // ---- device: the score pass
        sc::DevMem<uint8_t> d_sq(sd.codes.size()), d_rq(rd.codes.size());
        sc::DevMem<long> d_so(sd.off.size()), d_ro(rd.off.size());
        sc::DevMem<int> d_rids(rids.size());
        sc::DevMem<unsigned long long> d_best((size_t)n_reads), d_second((size_t)n_reads);
        sc::TimedStream st;
        st.mark("upload");
        st.h2d(d_sq, sd.codes); st.h2d(d_so, sd.off); st.h2d(d_rq, rd.codes); st.h2d(d_ro, rd.off); st.h2d(d_rids, rids);
        st.zero(d_best.p, (size_t)n_reads * 8);
        st.zero(d_second.p, (size_t)n_reads * 8);
        st.mark("score");
        by_r.each([&](auto r, long at, const std::vector<int>& ids) {
            const long n_tiles = (long)ids.size() * 2L * n_seeds;
            hipLaunchKernelGGL(k_sw_score<decltype(r)::value>, score_grid(n_tiles), dim3(64 * SCORE_WAVES), 0, st, d_sq.p, d_so.p, n_seeds, d_rq.p,
                               d_ro.p, d_rids.p + at, n_tiles, d_best.p, d_second.p);
            st.launched();
            if (stats) for (int id : ids) stats->score_cells += 2L * rd.len(id) * sd.bytes();
        });
        st.mark("scored");
        std::vector<unsigned long long> best((size_t)n_reads), second((size_t)n_reads);
        st.d2h(best, d_best); st.d2h(second, d_second);
        st.sync();
        // ---- which reads align; the traceback of those, bucketed by rows per lane again
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
            hipLaunchKernelGGL(k_sw_trace<decltype(r)::value>, trace_grid((int)ids.size()), dim3(64), 0, st, d_sq.p, d_so.p, d_rq.p, d_ro.p,
                               d_tids.p + at, (int)ids.size(), d_best.p, d_out.p + 4 * at, d_cig.p + at * cigar_stride, cigar_stride);
            st.launched();
        });
        st.mark("traced");
        st.d2h(tout, d_out); st.d2h(tcig, d_cig);
        st.sync();
        int rc = SC_OK;
        for (int t = 0; t < n_tr; t++) {
            const int r = tids[(size_t)t];
            const unsigned long long key = best[(size_t)r];
            if (tout[(size_t)t * 4] < 0) { rc = tl_error.fail(SC_ERR_INTERNAL, "sc_align_reads: traceback of read " + std::to_string(r) + " failed"); break; }
            seed[r] = key_seed(key);
            strand[r] = key_strand(key);
            pos[r] = tout[(size_t)t * 4] + 1;
            nm[r] = tout[(size_t)t * 4 + 2];
            n_cigar[r] = tout[(size_t)t * 4 + 3];
            std::memcpy(cigar + (long)r * cigar_stride, tcig.data() + (size_t)t * cigar_stride, sizeof(unsigned) * (size_t)n_cigar[r]);
            if (stats) {
                const int nrows = key_row(key) + 1;
                stats->trace_cells += window_cells(trace_window<SwCell>(key_score(key), key_col(key), nrows), nrows, 0);
            }
        }
        if (stats && rc == SC_OK) {
            read_phase_ms(st, stats);
            stats->n_traced = n_tr;
        }
        if (stats) stats->total_ms = sc::now_ms() - t0;
        return rc;
    });
}

}  // extern "C"
