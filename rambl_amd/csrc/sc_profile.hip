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
//   * the seeded mode (sc_profile_hits_seeded): k_seed_keys and a radix sort index the genes' k-mers,
//     k_seed_lookup lists the (segment, gene) pairs that share one on either strand, and k_bl_score_pairs scores those pairs
//     only.  k is the host's bound seed_length(): no hit that passes both thresholds is without a common k-mer, so the hits
//     are the unseeded ones.
//   * the counts mode (sc_profile_counts): after the same score pass the strand pick, the order of a read's
//     pairs by their six-digit E-value, rounds of k_bl_trace over each unresolved read's best group only, and the counting
//     rule all stay on the device (k_cnt_*, rocprim sorts); the distinct (gene, times, share) triples come back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include <rocprim/rocprim.hpp>

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

// Where a score kernel's tiles come from.  AllTiles: every bucket segment against every gene on both strands (tile_of).
// PairTiles, the seeded mode: tile w is pair w >> 1 on strand w & 1, so a pair is always scored on both strands (the better
// strand is picked before the filters; one strand alone could turn "no hit" into a hit).
struct Pair { int seg, gene; };
struct AllTiles {
    int n_genes; const int* sids;
    __device__ __forceinline__ Tile at(long w) const { return tile_of(w, n_genes, sids); }
};
struct PairTiles {
    const Pair* pairs;
    __device__ __forceinline__ Tile at(long w) const { const Pair p = pairs[w >> 1]; return Tile{p.seg, p.gene * 2 + (int)(w & 1)}; }
};

// One kernel for both: k_bl_score<R> is the full product, k_bl_score_pairs<R> the pair list.  The tile's body stays in the
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

// ---------------------------------------------------------------------------------------- the seeded mode

constexpr int SEED_MAX_K = 16;          // a k-mer is 2 bits per base in 32 bits; a longer bound is cut to 16, still lossless
// Below this bound the call runs unseeded.  A guess: a 150-base segment shares a 10-mer with a large share of unrelated
// 1 500-base genes, so the filter saves little there.  Where the break-even lies has not been measured.
constexpr int SEED_MIN_K = 11;
constexpr int SEED_WORDS = 2048;        // the lookup's LDS bitset: 65 536 genes per pass over a segment (8 KiB)
constexpr int KEY_BLOCKS = 4096, LOOKUP_BLOCKS = 8192;
constexpr unsigned long long NO_KEY = ~0ull;    // a window that is no k-mer; sorts behind every key (a gene index has 31 bits)

// keys[p] = (code of the k bases from p) << 32 | gene for every window of the packed genes that lies inside one gene and
// holds ACGT only, NO_KEY for every other p; *n_valid counts the former.  Each thread reads its k bases itself: the index
// is built once per call and the reads hit the cache, so no rolling code is kept.
__global__ __launch_bounds__(256) void k_seed_keys(const uint8_t* genes, const long* gene_off, int n_genes, long n_bases, int k,
                                                   unsigned long long* keys, unsigned long long* n_valid) {
    for (long p0 = (long)blockIdx.x * 256; p0 < n_bases; p0 += (long)gridDim.x * 256) {
        const long p = p0 + threadIdx.x;
        unsigned long long key = NO_KEY;
        if (p < n_bases) {
            int lo = 0, hi = n_genes;                           // the gene of p: gene_off[lo] <= p < gene_off[lo + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (gene_off[mid] <= p) lo = mid; else hi = mid;
            }
            if (p + k <= gene_off[lo + 1]) {
                unsigned code = 0;
                bool ok = true;
                for (int j = 0; j < k; j++) {
                    const unsigned c = genes[p + j];
                    ok = ok && c < 4u;
                    code = (code << 2) | (c & 3u);
                }
                if (ok) key = ((unsigned long long)code << 32) | (unsigned)lo;
            }
            keys[p] = key;
        }
        const unsigned long long m = __ballot(key != NO_KEY);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_valid, (unsigned long long)__popcll(m));
    }
}

// One wavefront per bucket segment: the genes that share a k-mer with the segment or with its reverse complement.  A lane
// takes a stretch of the segment's windows and rolls both codes along it; per window it finds the k-mer's run in the sorted
// keys by binary search and sets the bit of every gene of the run in the wavefront's LDS bitset (both strands set the same
// bit: the pair is the unit).  The bitset is then read a word per lane; a prefix sum of the popcounts places each lane's
// genes.  FILL = false counts: cnt[s] pairs and glen[s] = the summed length of their genes.  FILL = true writes the pairs
// from pair_off[s] on, genes ascending.  More than 65 536 genes: the segment is gone over once per gene range.
template <bool FILL>
__global__ __launch_bounds__(64) void k_seed_lookup(const unsigned long long* keys, long n_keys, const long* gene_off, int n_genes,
                                                    const uint8_t* sg, const long* seg_off, const int* sids, int n_ids, int k, unsigned* cnt,
                                                    long* glen, const long* pair_off, Pair* pairs) {
    __shared__ unsigned bits[SEED_WORDS];
    const int lane = threadIdx.x;
    const unsigned mask = k == 16 ? ~0u : (1u << (2 * k)) - 1u;
    for (int s = blockIdx.x; s < n_ids; s += gridDim.x) {
        const int seg = sids[s];
        const long r0 = seg_off[seg];
        const int L = (int)(seg_off[seg + 1] - r0);
        const int nw = L - k + 1;                               // windows; none when the segment is shorter than k
        const int per = (nw + 63) / 64;
        const int wa = lane * per, wb = min(wa + per, nw);
        unsigned total = 0;
        long gl = 0;
        for (int g0 = 0; g0 < n_genes; g0 += SEED_WORDS * 32) {
            const int ng = min(n_genes - g0, SEED_WORDS * 32), nwords = (ng + 31) >> 5;
            for (int w = lane; w < nwords; w += 64) bits[w] = 0;
            __syncthreads();
            unsigned fw = 0, rc = 0;
            int run = 0;                                        // ACGT bases in a row up to here
            for (int i = wa, end = wb > wa ? wb + k - 1 : wa; i < end; i++) {
                const unsigned c = sg[r0 + i];
                if (c >= 4u) { run = 0; continue; }
                fw = ((fw << 2) | c) & mask;
                rc = (rc >> 2) | ((3u - c) << (2 * (k - 1)));
                if (++run < k) continue;
#pragma unroll
                for (int strand = 0; strand < 2; strand++) {
                    const unsigned code = strand ? rc : fw;
                    const unsigned long long first = ((unsigned long long)code << 32) | (unsigned)g0;
                    long lo = 0, hi = n_keys;
                    while (lo < hi) {
                        const long mid = (lo + hi) >> 1;
                        if (keys[mid] < first) lo = mid + 1; else hi = mid;
                    }
                    for (; lo < n_keys; lo++) {
                        const unsigned long long key = keys[lo];
                        const int g = (int)(unsigned)key - g0;
                        if ((unsigned)(key >> 32) != code || g >= ng) break;
                        atomicOr(&bits[g >> 5], 1u << (g & 31));
                    }
                }
            }
            __syncthreads();
            for (int w0 = 0; w0 < nwords; w0 += 64) {
                const int w = w0 + lane;
                unsigned word = w < nwords ? bits[w] : 0u;
                const int pc = __popc(word);
                int upto = pc;                                  // inclusive prefix sum over the lanes
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int x = __shfl_up(upto, o);
                    if (lane >= o) upto += x;
                }
                long dst = FILL ? pair_off[s] + total + (upto - pc) : 0;
                while (word) {
                    const int g = g0 + w * 32 + __ffs(word) - 1;
                    word &= word - 1u;
                    if (FILL) { pairs[dst].seg = seg; pairs[dst].gene = g; dst++; }
                    else gl += gene_off[g + 1] - gene_off[g];
                }
                total += (unsigned)__shfl(upto, 63);
            }
            __syncthreads();
        }
        if (!FILL) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) gl += __shfl_xor(gl, o);
            if (lane == 0) { cnt[s] = total; glen[s] = gl; }
        }
    }
}

// ---------------------------------------------------------------------------------------- the counts mode

constexpr int COUNT_ROUNDS = 3;         // rounds that trace one E6 group per unresolved read; then the rest at once.  A guess.
constexpr long COUNT_ROOM = 1L << 23;   // candidate records on the device at a time unless the caller says otherwise
constexpr int REC_BLOCKS = 256, READ_BLOCKS = 8192;     // grids: 256 threads a record each / one wavefront a read each
constexpr int N_BUCKETS = MAX_ROWS / 64;
constexpr unsigned NO_RANK = ~0u;       // in the rank table: E6 of this (length, score) is above the threshold
constexpr int RANK_COLS = MATCH2 * MAX_ROWS + 1;        // doubled scores 0..1024
// what the kernels count, one array of 64-bit words
enum { C_VALID = 0, C_TRIPLES, C_READS, C_HITS, C_CELLS, C_BAD, C_HIST, C_FILL = C_HIST + N_BUCKETS, C_WORDS = C_FILL + N_BUCKETS };
// a record's state: not traced yet, chosen for this round's traceback, traced and passing -I, traced and failing it
enum : unsigned char { S_NEW = 0, S_CHOSEN, S_PASS, S_FAIL };

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }
// One atomicAdd per wavefront for the lanes with `on`; every such lane gets its own slot.  Called by all lanes.
__device__ __forceinline__ unsigned long long wave_slots(unsigned long long* counter, bool on, int lane) {
    const unsigned long long m = __ballot(on);
    if (!m) return 0;
    const int lead = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    return __shfl(base, lead) + (unsigned long long)lanes_below(m, lane);
}

// key[c] = segment << 32 | gene2 and val[c] = the tile's best cell for the sort that brings the strands of a pair together
__global__ __launch_bounds__(256) void k_cnt_keys(const Cand* cand, long n, unsigned long long* key, unsigned long long* val) {
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long)gridDim.x * 256) {
        key[c] = ((unsigned long long)(unsigned)cand[c].seg << 32) | (unsigned)cand[c].gene2;
        val[c] = cand[c].key;
    }
}

// The strand pick on the sorted tiles: a tile is its pair's hit unless the other strand is there and better (reverse: or
// equal).  A hit gets key2 = read of the stretch << 32 | rank of its E6, NO_KEY when E6 is above the threshold; a tile that
// is no hit gets NO_KEY too.  Counted: the hits, and how many of them fall to each traceback bucket.
__global__ __launch_bounds__(256) void k_cnt_pick(const unsigned long long* key, const unsigned long long* val, long n, const long* seg_off,
                                                  const int* seg_read, int read0, const int* len_slot, const unsigned* rank,
                                                  unsigned long long* key2, Cand* hit, unsigned long long* ctr) {
    const int lane = threadIdx.x & 63;
    for (long c0 = (long)blockIdx.x * 256; c0 < n; c0 += (long)gridDim.x * 256) {
        const long c = c0 + threadIdx.x;
        unsigned long long k2 = NO_KEY;
        int bucket = -1;
        if (c < n) {
            const unsigned long long k = key[c], v = val[c];
            const int seg = (int)(k >> 32), gene2 = (int)(unsigned)k, s2 = key_score2(v);
            bool wins = true;
            if (!(gene2 & 1)) { if (c + 1 < n && key[c + 1] == k + 1) wins = key_score2(val[c + 1]) <= s2; }
            else if (c > 0 && key[c - 1] == k - 1) wins = key_score2(val[c - 1]) < s2;
            const int L = (int)(seg_off[seg + 1] - seg_off[seg]);
            const unsigned r = rank[(long)len_slot[L] * RANK_COLS + s2];
            if (wins && r != NO_RANK) {
                k2 = ((unsigned long long)(unsigned)(seg_read[seg] - read0) << 32) | r;
                bucket = (L + 63) / 64 - 1;
            }
            key2[c] = k2;
            hit[c].seg = seg; hit[c].gene2 = gene2; hit[c].key = v;
        }
        const unsigned long long m = __ballot(bucket >= 0);
        if (lane == 0 && m) atomicAdd(&ctr[C_VALID], (unsigned long long)__popcll(m));
        for (int b = 0; b < N_BUCKETS; b++) {
            const unsigned long long mb = __ballot(bucket == b);
            if (lane == 0 && mb) atomicAdd(&ctr[C_HIST + b], (unsigned long long)__popcll(mb));
        }
    }
}

// first[r], last[r] + 1: the records of read r in the hits sorted by key2 (first stays -1 for a read without any)
__global__ __launch_bounds__(256) void k_cnt_bounds(const unsigned long long* key2, long n, int* first, int* end) {
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        const unsigned r = (unsigned)(key2[j] >> 32);
        if (j == 0 || (unsigned)(key2[j - 1] >> 32) != r) first[r] = (int)j;
        if (j == n - 1 || (unsigned)(key2[j + 1] >> 32) != r) end[r] = (int)(j + 1);
    }
}

// A round's choice: of every unresolved read the untraced records of the group at its cursor (all: from its cursor on) go to
// the traceback list of their bucket, list[slot] with from[slot] = the record; bucket b's part of the list starts at
// part[b] and has ctr[C_FILL + b] records so far.
__global__ __launch_bounds__(256) void k_cnt_choose(const unsigned long long* key2, const Cand* hit, long n, const long* seg_off, const int* cursor,
                                                    const unsigned char* resolved, int all, unsigned char* state, Cand* list, int* from,
                                                    const long* part, unsigned long long* ctr) {
    const int lane = threadIdx.x & 63;
    for (long j0 = (long)blockIdx.x * 256; j0 < n; j0 += (long)gridDim.x * 256) {
        const long j = j0 + threadIdx.x;
        int bucket = -1;
        Cand h{};
        if (j < n && state[j] == S_NEW) {
            const unsigned r = (unsigned)(key2[j] >> 32);
            const int at = cursor[r];
            if (!resolved[r] && j >= at && (all || key2[j] == key2[at])) {
                h = hit[j];
                bucket = (int)((seg_off[h.seg + 1] - seg_off[h.seg] + 63) / 64) - 1;
            }
        }
        for (int b = 0; b < N_BUCKETS; b++) {
            const bool mine = bucket == b;
            const long slot = part[b] + (long)wave_slots(&ctr[C_FILL + b], mine, lane);
            if (mine) { list[slot] = h; from[slot] = (int)j; state[j] = S_CHOSEN; }
        }
    }
}

// The round's new part of every bucket's list, [begin[b], end[b]) in list slots
struct Fresh { long begin[N_BUCKETS], end[N_BUCKETS]; };

// -I on what a round's tracebacks gave: state = S_PASS or S_FAIL per record; a failed walk raises ctr[C_BAD].  Counted: the
// passing pairs and the cells the walks swept (window_cells, as sc_profile_hits reports them).
__global__ __launch_bounds__(256) void k_cnt_resolve(Fresh fresh, long n_fresh, const Cand* list, const int* from, const int* out,
                                                     double min_identity_pct, unsigned char* state, unsigned long long* ctr) {
    const int lane = threadIdx.x & 63;
    for (long x0 = (long)blockIdx.x * 256; x0 < n_fresh; x0 += (long)gridDim.x * 256) {
        long x = x0 + threadIdx.x, cells = 0;
        bool pass = false;
        if (x < n_fresh) {
            int b = 0;
            while (x >= fresh.end[b] - fresh.begin[b]) { x -= fresh.end[b] - fresh.begin[b]; b++; }
            const long t = fresh.begin[b] + x;
            const int* o = out + t * 4;
            if (o[0] < 0) {
                atomicOr(&ctr[C_BAD], 1ull);
            } else {
                const unsigned long long key = list[t].key;
                const Window w = trace_window<BlCell>(key_score2(key), key_col(key), key_row(key) + 1);
                cells = window_cells(w, key_row(key) + 1, o[0] - w.j0);
                pass = 100.0 * (double)o[2] / (double)o[3] >= min_identity_pct;
            }
            state[from[t]] = pass ? S_PASS : S_FAIL;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cells += __shfl_xor(cells, o);
        const unsigned long long m = __ballot(pass);
        if (lane == 0 && cells) atomicAdd(&ctr[C_CELLS], (unsigned long long)cells);
        if (lane == 0 && m) atomicAdd(&ctr[C_HITS], (unsigned long long)__popcll(m));
    }
}

// The group of equal key2 that starts at record c of a read whose records end at e: its end, and whether it holds a passing
// and an untraced record.  The same in every lane.
struct Group { int end; bool pass, fresh; };
__device__ __forceinline__ Group group_at(const unsigned long long* key2, const unsigned char* state, int c, int e, int lane) {
    const unsigned long long key = key2[c];
    Group g{c, false, false};
    for (int base = c; base < e; base += 64) {
        const int j = base + lane;
        const bool in = j < e && key2[j] == key;
        const unsigned char s = in ? state[j] : (unsigned char)S_FAIL;
        const unsigned long long m = __ballot(in);
        g.pass = g.pass || __ballot(in && s == S_PASS) != 0;
        g.fresh = g.fresh || __ballot(in && s == S_NEW) != 0;
        g.end = base + __popcll(m);                             // the records are sorted: the group's lanes are the first ones
        if (m != ~0ull) break;
    }
    return g;
}

// One wavefront per unresolved read: from its cursor on, a group with a passing pair resolves the read with that group (1), a
// group not traced yet is where the read waits, a group without a passing pair is left behind; no group left: the read
// counts nowhere (2).
__global__ __launch_bounds__(64) void k_cnt_advance(const unsigned long long* key2, const unsigned char* state, int n_reads, int* cursor,
                                                    const int* end, unsigned char* resolved) {
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        if (resolved[r]) continue;
        int c = cursor[r];
        const int e = c < 0 ? c : end[r];
        unsigned char res = 0;
        while (c >= 0 && c < e) {
            const Group g = group_at(key2, state, c, e, lane);
            if (g.fresh) break;
            if (g.pass) { res = 1; break; }
            c = g.end;
        }
        if (c < 0 || c >= e) res = 2;
        if (lane == 0) { cursor[r] = c; resolved[r] = res; }
    }
}

// One wavefront per resolved read: among the passing pairs of its group (sorted by segment, then gene) the genes hit most
// often; one triple gene << (gene_bits + times_bits) | times << gene_bits | number of such genes per such gene goes to
// triple[].  times[] is a word of room per record: a lane reads back only what it wrote itself.
__global__ __launch_bounds__(64) void k_cnt_count(const unsigned long long* key2, const unsigned char* state, const Cand* hit, int n_reads,
                                                  const int* cursor, const int* end, const unsigned char* resolved, int gene_bits,
                                                  int times_bits, int* times, unsigned long long* triple, unsigned long long* ctr) {
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        if (resolved[r] != 1) continue;
        const int c = cursor[r];
        const int g = group_at(key2, state, c, end[r], lane).end;
        const bool one_segment = hit[c].seg == hit[g - 1].seg;  // then no gene is there twice
        int most = 0;
        for (int j = c + lane; j < g; j += 64) {
            int t = 0;
            if (state[j] == S_PASS) {
                t = 1;
                if (!one_segment) {
                    const int gene = hit[j].gene2 >> 1;
                    for (int i = c; i < g && t; i++) {
                        if (i == j || state[i] != S_PASS || (hit[i].gene2 >> 1) != gene) continue;
                        t = i < j ? 0 : t + 1;                  // counted at the gene's first record only
                    }
                }
            }
            times[j] = t;
            most = max(most, t);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) most = max(most, __shfl_xor(most, o));
        int share = 0;
        for (int j0 = c; j0 < g; j0 += 64) share += __popcll(__ballot(j0 + lane < g && times[j0 + lane] == most));
        unsigned long long base = 0;
        if (lane == 0) { base = atomicAdd(&ctr[C_TRIPLES], (unsigned long long)share); atomicAdd(&ctr[C_READS], 1ull); }
        base = __shfl(base, 0);
        for (int j0 = c; j0 < g; j0 += 64) {
            const int j = j0 + lane;
            const bool mine = j < g && times[j] == most;
            const unsigned long long m = __ballot(mine);
            if (mine)
                triple[base + lanes_below(m, lane)] = ((unsigned long long)(hit[j].gene2 >> 1) << (gene_bits + times_bits)) |
                                                      ((unsigned long long)most << gene_bits) | (unsigned long long)share;
            base += __popcll(m);
        }
    }
}

thread_local LastError tl_error;

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

// k*(L) of DESIGN.md §8.10: every hit of a segment of L bases that passes both thresholds shares an exact k*-mer with its
// gene on the hit's strand.  A hit with i identity columns and m others has i <= L, 2 i - 4 m >= min2 (a column that is no
// identity column costs 4 doubled points or more) and passes the identity test below, the final filter's own expression;
// its identity columns fall into at most m + 1 diagonal runs, so one has ceil(i / (m + 1)) columns.  Both conditions get
// harder with m and the run shorter, so per i only the largest feasible m counts.  0: no (i, m) is feasible.
int lossless_k(int L, int min2, double min_identity_pct) {
    int best = 0;
    for (int i = (min2 + 1) / 2; i <= L; i++) {
        int m = (2 * i - min2) / 4;
        if (min_identity_pct > 0.0) m = (int)std::min<double>(m, std::floor((double)i * (100.0 - min_identity_pct) / min_identity_pct) + 2.0);
        while (m >= 0 && !(100.0 * (double)i / (double)(i + m) >= min_identity_pct)) m--;
        if (m < 0) continue;
        const int run = (i + m) / (m + 1);
        if (best == 0 || run < best) best = run;
    }
    return best;
}

// The seed length of a call: the least k*(L) over the segment lengths present that can pass at all, at most SEED_MAX_K; 0
// when it is below SEED_MIN_K (or no length can pass): the call runs unseeded.  *lossless: the bound before the clamps.
int seed_length(const bool* has_len, long gene_bases, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* lossless) {
    int best = 0;
    for (int L = 1; L <= MAX_ROWS; L++) {
        if (!has_len[L]) continue;
        const int s2 = least_score2(ka_k, ka_lambda, L, gene_bases, max_evalue);
        if (s2 > MATCH2 * L) continue;
        const int k = lossless_k(L, s2, min_identity_pct);
        if (k > 0 && (best == 0 || k < best)) best = k;
    }
    if (lossless) *lossless = best;
    return best < SEED_MIN_K ? 0 : std::min(best, SEED_MAX_K);
}

// What the seeded entry point reports besides sc_profile_stats.
struct SeedInfo { int seed_k = 0; long n_gene_kmers = 0, n_pairs = 0; double index_ms = 0, lookup_ms = 0; };

// The genes' k-mers sorted by (code, gene), enqueued on `st` by the constructor; n_keys holds their number once the stream
// was synchronised.
struct SeedIndex {
    sc::DevMem<unsigned long long> keys, sorted, count;
    sc::DevMem<uint8_t> tmp;
    unsigned long long n_keys = 0;
    SeedIndex(sc::TimedStream& st, const uint8_t* genes, const long* gene_off, int n_genes, long gene_bytes, int k)
        : keys((size_t)gene_bytes), sorted((size_t)gene_bytes), count(1), tmp(0) {
        st.zero(count.p, sizeof(unsigned long long));
        hipLaunchKernelGGL(k_seed_keys, dim3((unsigned)std::min<long>((gene_bytes + 255) / 256, KEY_BLOCKS)), dim3(256), 0, st, genes, gene_off,
                           n_genes, gene_bytes, k, keys.p, count.p);
        st.launched();
        size_t tmp_bytes = 0;
        HIPCHK(rocprim::radix_sort_keys(nullptr, tmp_bytes, keys.p, sorted.p, (size_t)gene_bytes, 0, 64, st));
        { sc::DevMem<uint8_t> room(tmp_bytes); std::swap(room.p, tmp.p); }
        HIPCHK(rocprim::radix_sort_keys(tmp.p, tmp_bytes, keys.p, sorted.p, (size_t)gene_bytes, 0, 64, st));
        st.d2h(&n_keys, count.p, sizeof n_keys);
    }
};

// The (segment, gene) pairs of the bucketed segments `sids` (d_sids on the device) that share a k-mer of the index: counted
// per segment, scanned on the host into pair_off[sids.size() + 1], and -- unless their tiles are more than one call takes --
// filled into `pairs` in bucket order, genes ascending.  *score_cells (may be null) grows by 2 * segment length * gene length
// per pair.  Returns the number of pairs; the stream is synchronised.
long seed_pairs(sc::TimedStream& st, const SeedIndex& index, const long* d_go, int n_genes, const uint8_t* d_sq, const long* d_so,
                const Packed& sg, const Buckets& by_r, const std::vector<int>& sids, const int* d_sids, int seed_k, std::vector<long>& pair_off,
                sc::DevMem<Pair>& pairs, long* score_cells) {
    sc::DevMem<unsigned> d_cnt(sids.size());
    sc::DevMem<long> d_glen(sids.size()), d_poff(pair_off.size());
    const auto lookup = [&](auto fill) {
        by_r.each([&](auto, long at, const std::vector<int>& ids) {
            hipLaunchKernelGGL(k_seed_lookup<decltype(fill)::value>, dim3((unsigned)std::min<size_t>(ids.size(), LOOKUP_BLOCKS)), dim3(64), 0, st,
                               index.sorted.p, (long)index.n_keys, d_go, n_genes, d_sq, d_so, d_sids + at, (int)ids.size(), seed_k,
                               d_cnt.p + at, d_glen.p + at, d_poff.p + at, pairs.p);
            st.launched();
        });
    };
    lookup(std::false_type{});
    std::vector<unsigned> cnt(sids.size());
    std::vector<long> glen(sids.size());
    st.d2h(cnt, d_cnt); st.d2h(glen, d_glen);
    st.sync();
    for (size_t k = 0; k < sids.size(); k++) {
        pair_off[k + 1] = pair_off[k] + cnt[k];
        if (score_cells) *score_cells += 2L * sg.len(sids[k]) * glen[k];
    }
    const long n_pairs = pair_off.back();
    if (2L * n_pairs > 0x7FFFFFFFL || n_pairs == 0) return n_pairs;
    { sc::DevMem<Pair> room((size_t)n_pairs); std::swap(room.p, pairs.p); }
    st.h2d(d_poff, pair_off);
    lookup(std::true_type{});
    st.sync();                                                  // the counters go with this scope
    return n_pairs;
}

// The body of sc_profile_hits (seed == nullptr) and of sc_profile_hits_seeded; `fn` names the entry point in messages.
int profile_hits(const std::string& fn, int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text,
                 const long* seg_off, int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg,
                 int* hit_gene, int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                 double* evalue, long cap, long* n_hits, sc_profile_stats* stats, SeedInfo* seed) try {
    tl_error.text.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_hits) *n_hits = 0;
    if (!gene_text || !gene_off || n_genes < 1 || n_segs < 0 || (n_segs > 0 && (!seg_text || !seg_off)) || !hit_seg || !hit_gene ||
        !hit_strand || !hit_score || !identity || !align_len || !qfrom || !qto || !hfrom || !hto || !evalue || cap < 0 || !n_hits)
        return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
    if (!(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0))
        return tl_error.fail(SC_ERR_ARG, fn + ": lambda and K must be positive, the E-value threshold not negative");
    Packed gn, sg;
    std::string why;
    if (!gn.rebase(gene_off, n_genes, MAX_COLS, fn.c_str(), "gene", why) ||
        (n_segs > 0 && !sg.rebase(seg_off, n_segs, MAX_ROWS, fn.c_str(), "segment", why)))
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
        if (s2 == 0) s2 = least_score2(ka_k, ka_lambda, L, gene_bytes, max_evalue);
        min2[(size_t)r] = s2;
        if (s2 <= MATCH2 * L) by_r.add(r, L);
    }
    const std::vector<int> sids = by_r.order();
    // the seeded mode's k, from the lengths of the segments in a bucket: 0 runs the full product
    int seed_k = 0;
    if (seed) {
        bool has_len[MAX_ROWS + 1] = {};
        for (int id : sids) has_len[sg.len(id)] = true;
        seed_k = seed->seed_k = seed_length(has_len, gene_bytes, min_identity_pct, max_evalue, ka_lambda, ka_k, nullptr);
    }
    const auto too_many = [&](long n_tiles) {
        return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_tiles) + " (segment, gene, strand) tiles in one call (at most "
                                                     "2147483647: pass the segments in several calls)");
    };
    long n_tiles = (long)sids.size() * 2L * n_genes;
    if (!seed_k && n_tiles > 0x7FFFFFFFL) return too_many(n_tiles);
    sc::DevMem<uint8_t> d_gq(gn.codes.size()), d_sq(sg.codes.size());
    sc::DevMem<long> d_go(gn.off.size()), d_so(sg.off.size());
    sc::DevMem<int> d_sids(sids.size()), d_min2(min2.size());
    sc::DevMem<unsigned> d_ncand(1);
    sc::TimedStream st;
    st.mark("upload");
    st.h2d(d_gq, gn.codes); st.h2d(d_go, gn.off); st.h2d(d_sq, sg.codes); st.h2d(d_so, sg.off); st.h2d(d_sids, sids); st.h2d(d_min2, min2);
    st.zero(d_ncand.p, sizeof(unsigned));
    // ---- device, seeded only: the genes' k-mers sorted by (code, gene); per bucket segment the genes that share one, counted,
    // scanned on the host (the pair list's size has to come back anyway) and filled in bucket order, genes ascending
    std::vector<long> pair_off(sids.size() + 1, 0);
    sc::DevMem<Pair> d_pairs(0);
    if (seed_k && !sids.empty()) {
        st.mark("index");
        SeedIndex index(st, d_gq.p, d_go.p, n_genes, gene_bytes, seed_k);
        st.mark("lookup");
        st.sync();
        seed->n_gene_kmers = (long)index.n_keys;
        seed->n_pairs = seed_pairs(st, index, d_go.p, n_genes, d_sq.p, d_so.p, sg, by_r, sids, d_sids.p, seed_k, pair_off, d_pairs,
                                   stats ? &stats->score_cells : nullptr);
        n_tiles = 2L * seed->n_pairs;
        if (n_tiles > 0x7FFFFFFFL) return too_many(n_tiles);
    }
    // every passing tile is a candidate; a (segment, gene) pair gives at most two, so 2 * cap + 1024 records hold them unless
    // the caller's cap is too small as well
    const long cand_cap = std::min<long>(n_tiles, std::min<long>(2 * cap + 1024, 0x7FFFFFFFL));
    sc::DevMem<Cand> d_cand((size_t)cand_cap);
    // ---- device: the score pass
    st.mark("score");
    by_r.each([&](auto r, long at, const std::vector<int>& ids) {
        if (seed_k) {
            const long nt = 2L * (pair_off[(size_t)at + ids.size()] - pair_off[(size_t)at]);
            if (nt == 0) return;
            hipLaunchKernelGGL(k_bl_score_pairs<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d_gq.p, d_go.p, d_sq.p, d_so.p,
                               PairTiles{d_pairs.p + pair_off[(size_t)at]}, d_min2.p, nt, d_cand.p, (unsigned)cand_cap, d_ncand.p);
            st.launched();
            return;
        }
        const long nt = (long)ids.size() * 2L * n_genes;
        hipLaunchKernelGGL(k_bl_score<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d_gq.p, d_go.p, d_sq.p, d_so.p,
                           AllTiles{n_genes, d_sids.p + at}, d_min2.p, nt, d_cand.p, (unsigned)cand_cap, d_ncand.p);
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
        rc = tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(n_cand) + " tiles pass the E-value threshold, room for " +
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
                rc = tl_error.fail(SC_ERR_INTERNAL, fn + ": traceback of segment " + std::to_string(c.seg) + " on gene " +
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
            if (n_out > cap) rc = tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(n_out) + " hits, room for " + std::to_string(cap));
        }
        if (stats && (rc == SC_OK || rc == SC_ERR_CAPACITY)) {
            read_phase_ms(st, stats);
            if (seed_k && !sids.empty()) {                      // "upload" .. "score" holds the index and the lookup here
                stats->upload_ms = st.ms("upload", "index");
                seed->index_ms = st.ms("index", "lookup");
                seed->lookup_ms = st.ms("lookup", "score");
            }
            stats->n_traced = n_tr;
            stats->n_hits = n_out;
        }
    }
    if (stats) stats->total_ms = sc::now_ms() - t0;
    return rc;
} catch (const sc::HipError&) {
    return tl_error.fail(SC_ERR_HIP, fn + ": a HIP call failed");
}

// E6: an E-value as the hit CSV holds it, six significant digits, read back.
double evalue6_of(double e) {
    char text[40];
    std::snprintf(text, sizeof text, "%.6g", e);
    return std::strtod(text, nullptr);
}

int bits_of(long v) { int b = 0; while (v >> b) b++; return b; }

// The body of sc_profile_counts.
int profile_counts(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off, int n_segs,
                   const int* seg_read, int n_reads, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int seeded,
                   long cand_room, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap, long* n_out,
                   sc_profile_count_stats* stats) try {
    const std::string fn = "sc_profile_counts";
    tl_error.text.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_out) *n_out = 0;
    if (!gene_text || !gene_off || n_genes < 1 || n_segs < 0 || n_reads < 0 || (n_segs > 0 && (!seg_text || !seg_off || !seg_read)) || !out_gene ||
        !out_times || !out_share || !out_reads || cap < 0 || cand_room < 0 || !n_out)
        return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
    if (!(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0))
        return tl_error.fail(SC_ERR_ARG, fn + ": lambda and K must be positive, the E-value threshold not negative");
    for (int r = 0; r < n_segs; r++)
        if (seg_read[r] < 0 || seg_read[r] >= n_reads)
            return tl_error.fail(SC_ERR_ARG, fn + ": segment " + std::to_string(r) + " belongs to read " + std::to_string(seg_read[r]) + " of " +
                                                 std::to_string(n_reads));
    Packed gn, sg;
    std::string why;
    if (!gn.rebase(gene_off, n_genes, MAX_COLS, fn.c_str(), "gene", why) ||
        (n_segs > 0 && !sg.rebase(seg_off, n_segs, MAX_ROWS, fn.c_str(), "segment", why)))
        return tl_error.fail(SC_ERR_UNSUPPORTED, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return tl_error.fail(SC_ERR_NO_DEVICE, "no HIP device");
    if (hipSetDevice(device) != hipSuccess) return tl_error.fail(SC_ERR_HIP, "hipSetDevice failed");
    if (n_segs == 0) return SC_OK;
    const double t0 = sc::now_ms();
    // ---- host, once per call: the codes; per segment length the least passing score and, per doubled score from there on, the
    // dense rank of E6 among all (length, score) of the call -- E and E6 by the expressions of the contract, E6 <= T or no rank
    gn.pack(gene_text + gene_off[0], [](long, int c) { return c < 0 ? REF_OTHER : c; });
    sg.pack(seg_text + seg_off[0], [](long, int c) { return c < 0 ? 4 : c; });
    const long gene_bytes = gn.bytes();
    int min2_of_len[MAX_ROWS + 1] = {};
    bool has_len[MAX_ROWS + 1] = {};                            // of the segments that can pass
    std::vector<int> min2((size_t)n_segs);
    std::vector<int> read_segs((size_t)n_reads + 1, 0);         // read r: segments by_read[read_segs[r] .. read_segs[r + 1])
    for (int r = 0; r < n_segs; r++) {
        const int L = (int)sg.len(r);
        int& s2 = min2_of_len[L];
        if (s2 == 0) s2 = least_score2(ka_k, ka_lambda, L, gene_bytes, max_evalue);
        min2[(size_t)r] = s2;
        if (s2 <= MATCH2 * L) has_len[L] = true;
        read_segs[(size_t)seg_read[r] + 1]++;
    }
    int most_segs = 0;
    for (int r = 0; r < n_reads; r++) { most_segs = std::max(most_segs, read_segs[(size_t)r + 1]); read_segs[(size_t)r + 1] += read_segs[(size_t)r]; }
    std::vector<int> by_read((size_t)n_segs);
    {
        std::vector<int> at(read_segs.begin(), read_segs.end() - 1);
        for (int r = 0; r < n_segs; r++) by_read[(size_t)at[(size_t)seg_read[r]]++] = r;
    }
    const int gene_bits = bits_of(n_genes), times_bits = bits_of(most_segs);
    if (2 * gene_bits + times_bits > 64)
        return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_genes) + " genes and " + std::to_string(most_segs) +
                                                     " segments in one read do not fit a 64-bit triple");
    std::vector<int> len_slot(MAX_ROWS + 1, 0);
    std::vector<unsigned> rank;
    {
        std::vector<double> e6s;
        int n_lens = 0;
        for (int L = 1; L <= MAX_ROWS; L++) {
            if (!has_len[L]) continue;
            len_slot[(size_t)L] = n_lens++;
            for (int s2 = min2_of_len[L]; s2 <= MATCH2 * L; s2++) {
                const double e6 = evalue6_of(evalue_of(ka_k, ka_lambda, L, gene_bytes, s2));
                if (e6 <= max_evalue) e6s.push_back(e6);
            }
        }
        std::sort(e6s.begin(), e6s.end());
        e6s.erase(std::unique(e6s.begin(), e6s.end()), e6s.end());
        rank.assign((size_t)std::max(n_lens, 1) * RANK_COLS, NO_RANK);
        for (int L = 1; L <= MAX_ROWS; L++) {
            if (!has_len[L]) continue;
            for (int s2 = min2_of_len[L]; s2 <= MATCH2 * L; s2++) {
                const double e6 = evalue6_of(evalue_of(ka_k, ka_lambda, L, gene_bytes, s2));
                if (e6 <= max_evalue)
                    rank[(size_t)len_slot[(size_t)L] * RANK_COLS + s2] = (unsigned)(std::lower_bound(e6s.begin(), e6s.end(), e6) - e6s.begin());
            }
        }
    }
    const int seed_k = seeded ? seed_length(has_len, gene_bytes, min_identity_pct, max_evalue, ka_lambda, ka_k, nullptr) : 0;
    if (stats) stats->seed_k = seed_k;
    // ---- the stretches: whole reads in read order while their segments' tiles fit the candidate room
    const long room_asked = cand_room > 0 ? cand_room : COUNT_ROOM;
    struct Stretch { int read0, read1; long tiles; };
    std::vector<Stretch> stretches;
    long room = 0;
    {
        Stretch cur{0, 0, 0};
        for (int r = 0; r < n_reads; r++) {
            long tiles = 0;
            for (int k = read_segs[(size_t)r]; k < read_segs[(size_t)r + 1]; k++)
                if (min2[(size_t)by_read[(size_t)k]] <= MATCH2 * sg.len(by_read[(size_t)k])) tiles += 2L * n_genes;
            if (cur.tiles > 0 && cur.tiles + tiles > room_asked) { stretches.push_back(cur); cur = Stretch{r, r, 0}; }
            cur.read1 = r + 1; cur.tiles += tiles;
            room = std::max(room, cur.tiles);
        }
        if (cur.tiles > 0) stretches.push_back(cur);
    }
    if (room > 0x7FFFFFFFL)
        return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(room) + " (segment, gene, strand) tiles in one read (at most 2147483647)");
    double ms[7] = {};                                          // upload, index, lookup, score, select, trace, count
    std::vector<std::pair<unsigned long long, long>> total;     // (triple, reads), merged over the stretches
    int rc = SC_OK;
    if (!stretches.empty()) {
        sc::DevMem<uint8_t> d_gq(gn.codes.size()), d_sq(sg.codes.size());
        sc::DevMem<long> d_go(gn.off.size()), d_so(sg.off.size()), d_part(N_BUCKETS);
        sc::DevMem<int> d_min2(min2.size()), d_read(n_segs), d_slot(len_slot.size());
        sc::DevMem<unsigned> d_rank(rank.size()), d_ncand(1);
        sc::DevMem<unsigned long long> d_ctr(C_WORDS);
        sc::DevMem<Cand> d_cand((size_t)room);
        std::unique_ptr<SeedIndex> index;
        {
            sc::TimedStream st;
            st.mark("upload");
            st.h2d(d_gq, gn.codes); st.h2d(d_go, gn.off); st.h2d(d_sq, sg.codes); st.h2d(d_so, sg.off); st.h2d(d_min2, min2);
            st.h2d(d_read.p, seg_read, (size_t)n_segs * sizeof(int)); st.h2d(d_slot, len_slot); st.h2d(d_rank, rank);
            st.mark("index");
            if (seed_k) index.reset(new SeedIndex(st, d_gq.p, d_go.p, n_genes, gene_bytes, seed_k));
            st.mark("indexed");
            st.sync();
            ms[0] += st.ms("upload", "index"); ms[1] += st.ms("index", "indexed");
            if (stats && seed_k) stats->n_gene_kmers = (long)index->n_keys;
        }
        // per-stretch arrays, grown to the largest stretch
        sc::DevBuf b_sids, b_k1, b_k1s, b_v1, b_v1s, b_k2, b_k2s, b_hit, b_hits, b_tmp, b_state, b_list, b_from, b_out, b_times, b_trip, b_trips,
            b_runs, b_first, b_end, b_res;
        for (const Stretch& s : stretches) {
            sc::TimedStream st;
            Buckets by_r;
            for (int k = read_segs[(size_t)s.read0]; k < read_segs[(size_t)s.read1]; k++) {
                const int id = by_read[(size_t)k];
                if (min2[(size_t)id] <= MATCH2 * sg.len(id)) by_r.add(id, sg.len(id));
            }
            const std::vector<int> sids = by_r.order();
            const int nr = s.read1 - s.read0;
            int* d_sids = (int*)b_sids.ensure(sids.size() * sizeof(int) + 16);
            st.mark("upload");
            st.h2d(d_sids, sids.data(), sids.size() * sizeof(int));
            st.zero(d_ncand.p, sizeof(unsigned));
            st.zero(d_ctr.p, C_WORDS * sizeof(unsigned long long));
            st.mark("lookup");
            std::vector<long> pair_off(sids.size() + 1, 0);
            sc::DevMem<Pair> d_pairs(0);
            long n_tiles = (long)sids.size() * 2L * n_genes;
            if (seed_k) {
                const long n_pairs = seed_pairs(st, *index, d_go.p, n_genes, d_sq.p, d_so.p, sg, by_r, sids, d_sids, seed_k, pair_off, d_pairs,
                                                stats ? &stats->score_cells : nullptr);
                n_tiles = 2L * n_pairs;
                if (stats) stats->n_pairs += n_pairs;
            }
            // ---- the score pass: k_bl_score / k_bl_score_pairs as in sc_profile_hits
            st.mark("score");
            by_r.each([&](auto r, long at, const std::vector<int>& ids) {
                if (seed_k) {
                    const long nt = 2L * (pair_off[(size_t)at + ids.size()] - pair_off[(size_t)at]);
                    if (nt == 0) return;
                    hipLaunchKernelGGL(k_bl_score_pairs<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d_gq.p, d_go.p, d_sq.p,
                                       d_so.p, PairTiles{d_pairs.p + pair_off[(size_t)at]}, d_min2.p, nt, d_cand.p, (unsigned)room, d_ncand.p);
                    st.launched();
                    return;
                }
                const long nt = (long)ids.size() * 2L * n_genes;
                hipLaunchKernelGGL(k_bl_score<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d_gq.p, d_go.p, d_sq.p, d_so.p,
                                   AllTiles{n_genes, d_sids + at}, d_min2.p, nt, d_cand.p, (unsigned)room, d_ncand.p);
                st.launched();
                if (stats) for (int id : ids) stats->score_cells += 2L * sg.len(id) * gene_bytes;
            });
            st.mark("select");
            unsigned n_cand = 0;
            st.d2h(&n_cand, d_ncand.p, sizeof(unsigned));
            st.sync();
            if ((long)n_cand > room) return tl_error.fail(SC_ERR_INTERNAL, fn + ": more candidates than tiles");
            if (stats) { stats->n_tiles += n_tiles; stats->n_candidates += (long)n_cand; stats->n_stretches++; }
            // ---- the strand pick: the tiles sorted by (segment, gene, strand), then the hits by (read, rank of E6); both sorts are
            // stable and the first one's keys are unique, so the order is the same whatever order the score pass wrote in
            const size_t nc = n_cand;
            const auto rec_grid = [](long n) { return dim3((unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, REC_BLOCKS))); };
            auto* k1 = (unsigned long long*)b_k1.ensure(nc * 8); auto* k1s = (unsigned long long*)b_k1s.ensure(nc * 8);
            auto* v1 = (unsigned long long*)b_v1.ensure(nc * 8); auto* v1s = (unsigned long long*)b_v1s.ensure(nc * 8);
            auto* k2 = (unsigned long long*)b_k2.ensure(nc * 8); auto* k2s = (unsigned long long*)b_k2s.ensure(nc * 8);
            auto* hit = (Cand*)b_hit.ensure(nc * sizeof(Cand)); auto* hits = (Cand*)b_hits.ensure(nc * sizeof(Cand));
            int* first = (int*)b_first.ensure((size_t)nr * sizeof(int)); int* end = (int*)b_end.ensure((size_t)nr * sizeof(int));
            auto* resolved = (unsigned char*)b_res.ensure((size_t)nr);
            unsigned long long ctr[C_WORDS] = {};
            if (nc) {
                hipLaunchKernelGGL(k_cnt_keys, rec_grid((long)nc), dim3(256), 0, st, d_cand.p, (long)nc, k1, v1);
                st.launched();
                size_t t1 = 0, t2 = 0;
                HIPCHK(rocprim::radix_sort_pairs(nullptr, t1, k1, k1s, v1, v1s, nc, 0, 64, st));
                HIPCHK(rocprim::radix_sort_pairs(nullptr, t2, k2, k2s, hit, hits, nc, 0, 64, st));
                void* tmp = b_tmp.ensure(std::max(t1, t2));
                HIPCHK(rocprim::radix_sort_pairs(tmp, t1, k1, k1s, v1, v1s, nc, 0, 64, st));
                hipLaunchKernelGGL(k_cnt_pick, rec_grid((long)nc), dim3(256), 0, st, k1s, v1s, (long)nc, d_so.p, d_read.p, s.read0, d_slot.p, d_rank.p,
                                   k2, hit, d_ctr.p);
                st.launched();
                HIPCHK(rocprim::radix_sort_pairs(tmp, t2, k2, k2s, hit, hits, nc, 0, 64, st));
                st.d2h(ctr, d_ctr.p, sizeof ctr);
                st.sync();
            }
            const long nv = (long)ctr[C_VALID];                 // the hits: the first nv records of k2s / hits
            long part[N_BUCKETS], filled[N_BUCKETS] = {};
            for (int b = 0, at = 0; b < N_BUCKETS; b++) { part[b] = at; at += (int)ctr[C_HIST + b]; }
            auto* state = (unsigned char*)b_state.ensure((size_t)nv);
            Cand* list = (Cand*)b_list.ensure((size_t)nv * sizeof(Cand));
            int* from = (int*)b_from.ensure((size_t)nv * sizeof(int));
            int* out = (int*)b_out.ensure((size_t)nv * 4 * sizeof(int));
            int* times = (int*)b_times.ensure((size_t)nv * sizeof(int));
            st.mark("trace");
            if (nv) {
                st.h2d(d_part.p, part, sizeof part);
                st.zero(state, (size_t)nv);
                st.zero(resolved, (size_t)nr);
                HIPCHK(hipMemsetAsync(first, 0xFF, (size_t)nr * sizeof(int), st));
                hipLaunchKernelGGL(k_cnt_bounds, rec_grid(nv), dim3(256), 0, st, k2s, nv, first, end);
                st.launched();
                // ---- the rounds: choose, trace, apply -I, move the reads; one readback (the lists' fill) per round
                const dim3 read_grid((unsigned)std::min(nr, READ_BLOCKS));
                for (int round = 0;; round++) {
                    hipLaunchKernelGGL(k_cnt_choose, rec_grid(nv), dim3(256), 0, st, k2s, hits, nv, d_so.p, first, resolved,
                                       round >= COUNT_ROUNDS ? 1 : 0, state, list, from, d_part.p, d_ctr.p);
                    st.launched();
                    st.d2h(ctr, d_ctr.p, sizeof ctr);
                    st.sync();
                    Fresh fresh;
                    long n_fresh = 0;
                    for (int b = 0; b < N_BUCKETS; b++) {
                        fresh.begin[b] = part[b] + filled[b];
                        filled[b] = (long)ctr[C_FILL + b];
                        fresh.end[b] = part[b] + filled[b];
                        n_fresh += fresh.end[b] - fresh.begin[b];
                    }
                    if (n_fresh == 0) break;                    // no unresolved read has a group left
                    for (int b = 0; b < N_BUCKETS; b++) {
                        const int n = (int)(fresh.end[b] - fresh.begin[b]);
                        if (n == 0) continue;
                        dispatch_by_rows(b + 1, [&](auto r) {
                            hipLaunchKernelGGL(k_bl_trace<decltype(r)::value>, trace_grid(n), dim3(64), 0, st, d_gq.p, d_go.p, d_sq.p, d_so.p,
                                               list + fresh.begin[b], n, out + 4 * fresh.begin[b]);
                        });
                        st.launched();
                    }
                    hipLaunchKernelGGL(k_cnt_resolve, rec_grid(n_fresh), dim3(256), 0, st, fresh, n_fresh, list, from, out, min_identity_pct, state,
                                       d_ctr.p);
                    st.launched();
                    hipLaunchKernelGGL(k_cnt_advance, read_grid, dim3(64), 0, st, k2s, state, nr, first, end, resolved);
                    st.launched();
                    if (stats) { stats->n_rounds++; stats->n_traced += n_fresh; }
                }
            }
            // ---- the triples of the resolved reads, sorted and reduced to distinct ones with their number of reads
            st.mark("count");
            std::vector<unsigned long long> trip;
            std::vector<unsigned> reads;
            if (nv) {
                auto* trips_in = (unsigned long long*)b_trip.ensure((size_t)nv * 8);
                auto* trips = (unsigned long long*)b_trips.ensure((size_t)nv * 8);
                hipLaunchKernelGGL(k_cnt_count, dim3((unsigned)std::min(nr, READ_BLOCKS)), dim3(64), 0, st, k2s, state, hits, nr, first, end, resolved,
                                   gene_bits, times_bits, times, trips_in, d_ctr.p);
                st.launched();
                st.d2h(ctr, d_ctr.p, sizeof ctr);
                st.sync();
                const size_t nt = (size_t)ctr[C_TRIPLES];
                if (ctr[C_BAD]) return tl_error.fail(SC_ERR_INTERNAL, fn + ": a traceback failed");
                if (nt) {
                    // distinct triples (k2 is free by now), their run lengths (as unsigned in `from`), their number
                    unsigned long long* uniq = k2;
                    unsigned* runs = (unsigned*)from;
                    unsigned* n_runs = (unsigned*)b_runs.ensure(sizeof(unsigned));
                    size_t t1 = 0, t2 = 0;
                    HIPCHK(rocprim::radix_sort_keys(nullptr, t1, trips_in, trips, nt, 0, 2 * gene_bits + times_bits, st));
                    HIPCHK(rocprim::run_length_encode(nullptr, t2, trips, (unsigned)nt, uniq, runs, n_runs, st));
                    void* tmp = b_tmp.ensure(std::max(t1, t2));
                    HIPCHK(rocprim::radix_sort_keys(tmp, t1, trips_in, trips, nt, 0, 2 * gene_bits + times_bits, st));
                    HIPCHK(rocprim::run_length_encode(tmp, t2, trips, (unsigned)nt, uniq, runs, n_runs, st));
                    unsigned n_uniq = 0;
                    st.d2h(&n_uniq, n_runs, sizeof n_uniq);
                    st.sync();
                    trip.resize(n_uniq); reads.resize(n_uniq);
                    st.d2h(trip.data(), uniq, (size_t)n_uniq * 8); st.d2h(reads.data(), runs, (size_t)n_uniq * sizeof(unsigned));
                }
            }
            st.mark("counted");
            st.sync();
            for (size_t k = 0; k < trip.size(); k++) total.emplace_back(trip[k], (long)reads[k]);
            ms[0] += st.ms("upload", "lookup"); ms[2] += st.ms("lookup", "score"); ms[3] += st.ms("score", "select");
            ms[4] += st.ms("select", "trace"); ms[5] += st.ms("trace", "count"); ms[6] += st.ms("count", "counted");
            if (stats) { stats->n_reads_counted += (long)ctr[C_READS]; stats->n_hits += (long)ctr[C_HITS]; stats->trace_cells += (long)ctr[C_CELLS]; }
        }
    }
    // ---- the stretches' triples merged (a read is in one stretch, so the numbers of reads add), ascending
    std::sort(total.begin(), total.end());
    long n = 0;
    for (size_t k = 0; k < total.size(); k++) {
        if (k > 0 && total[k].first == total[k - 1].first) { if (n <= cap) out_reads[n - 1] += total[k].second; continue; }
        if (n < cap) {
            out_gene[n] = (int)(total[k].first >> (gene_bits + times_bits));
            out_times[n] = (int)((total[k].first >> gene_bits) & ((1ull << times_bits) - 1ull));
            out_share[n] = (int)(total[k].first & ((1ull << gene_bits) - 1ull));
            out_reads[n] = total[k].second;
        }
        n++;
    }
    *n_out = n;
    if (n > cap) rc = tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(n) + " triples, room for " + std::to_string(cap));
    if (stats) {
        stats->upload_ms = ms[0]; stats->index_ms = ms[1]; stats->lookup_ms = ms[2]; stats->score_ms = ms[3]; stats->select_ms = ms[4];
        stats->trace_ms = ms[5]; stats->count_ms = ms[6];
        stats->total_ms = sc::now_ms() - t0;
    }
    return rc;
} catch (const sc::HipError&) {
    return tl_error.fail(SC_ERR_HIP, "sc_profile_counts: a HIP call failed");
}

}  // namespace

extern "C" {

const char* sc_profile_error(void) { return tl_error.text.c_str(); }

int sc_profile_hits(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                    int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg, int* hit_gene,
                    int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                    double* evalue, long cap, long* n_hits, sc_profile_stats* stats) {
    return profile_hits("sc_profile_hits", device, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct, max_evalue,
                        ka_lambda, ka_k, hit_seg, hit_gene, hit_strand, hit_score, identity, align_len, qfrom, qto, hfrom, hto, evalue, cap,
                        n_hits, stats, nullptr);
}

int sc_profile_hits_seeded(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                           int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg,
                           int* hit_gene, int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto,
                           int* hfrom, int* hto, double* evalue, long cap, long* n_hits, sc_profile_seed_stats* stats) {
    sc_profile_stats base;
    SeedInfo seed;
    if (stats) std::memset(stats, 0, sizeof *stats);
    const int rc = profile_hits("sc_profile_hits_seeded", device, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct,
                                max_evalue, ka_lambda, ka_k, hit_seg, hit_gene, hit_strand, hit_score, identity, align_len, qfrom, qto, hfrom,
                                hto, evalue, cap, n_hits, &base, &seed);
    if (stats) {
        stats->upload_ms = base.upload_ms; stats->score_ms = base.score_ms; stats->trace_ms = base.trace_ms; stats->total_ms = base.total_ms;
        stats->score_cells = base.score_cells; stats->trace_cells = base.trace_cells; stats->n_tiles = base.n_tiles;
        stats->n_candidates = base.n_candidates; stats->n_traced = base.n_traced; stats->n_hits = base.n_hits;
        stats->seed_k = seed.seed_k; stats->n_gene_kmers = seed.n_gene_kmers; stats->n_pairs = seed.n_pairs;
        stats->index_ms = seed.index_ms; stats->lookup_ms = seed.lookup_ms;
    }
    return rc;
}

int sc_profile_seed_length(const int* seg_len, int n_segs, long gene_bases, double min_identity_pct, double max_evalue, double ka_lambda,
                           double ka_k, int* lossless_k) {
    if (lossless_k) *lossless_k = 0;
    if (n_segs < 0 || (n_segs > 0 && !seg_len) || gene_bases < 1 || !(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0)) return SC_ERR_ARG;
    bool has_len[MAX_ROWS + 1] = {};
    for (int r = 0; r < n_segs; r++) {
        if (seg_len[r] < 1 || seg_len[r] > MAX_ROWS) return SC_ERR_UNSUPPORTED;
        has_len[seg_len[r]] = true;
    }
    return seed_length(has_len, gene_bases, min_identity_pct, max_evalue, ka_lambda, ka_k, lossless_k);
}

int sc_profile_counts(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                      int n_segs, const int* seg_read, int n_reads, double min_identity_pct, double max_evalue, double ka_lambda,
                      double ka_k, int seeded, long cand_room, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap,
                      long* n_out, sc_profile_count_stats* stats) {
    return profile_counts(device, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, seg_read, n_reads, min_identity_pct, max_evalue,
                          ka_lambda, ka_k, seeded, cand_room, out_gene, out_times, out_share, out_reads, cap, n_out, stats);
}

double sc_profile_evalue6(int L, long gene_bases, int score2, double ka_lambda, double ka_k) {
    return evalue6_of(evalue_of(ka_k, ka_lambda, L, gene_bases, score2));
}

}  // extern "C"
