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
#include <cmath>
#include <cstring>

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
        sc::DevMem<unsigned long long> d_keys((size_t)gene_bytes), d_sorted((size_t)gene_bytes), d_nkeys(1);
        st.zero(d_nkeys.p, sizeof(unsigned long long));
        hipLaunchKernelGGL(k_seed_keys, dim3((unsigned)std::min<long>((gene_bytes + 255) / 256, KEY_BLOCKS)), dim3(256), 0, st, d_gq.p, d_go.p,
                           n_genes, gene_bytes, seed_k, d_keys.p, d_nkeys.p);
        st.launched();
        size_t tmp_bytes = 0;
        HIPCHK(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys.p, d_sorted.p, (size_t)gene_bytes, 0, 64, st));
        sc::DevMem<uint8_t> d_tmp(tmp_bytes);
        HIPCHK(rocprim::radix_sort_keys(d_tmp.p, tmp_bytes, d_keys.p, d_sorted.p, (size_t)gene_bytes, 0, 64, st));
        unsigned long long n_keys = 0;
        st.d2h(&n_keys, d_nkeys.p, sizeof n_keys);
        st.mark("lookup");
        st.sync();
        seed->n_gene_kmers = (long)n_keys;
        sc::DevMem<unsigned> d_cnt(sids.size());
        sc::DevMem<long> d_glen(sids.size()), d_poff(pair_off.size());
        const auto lookup = [&](auto fill) {
            by_r.each([&](auto, long at, const std::vector<int>& ids) {
                hipLaunchKernelGGL(k_seed_lookup<decltype(fill)::value>, dim3((unsigned)std::min<size_t>(ids.size(), LOOKUP_BLOCKS)), dim3(64), 0, st,
                                   d_sorted.p, (long)n_keys, d_go.p, n_genes, d_sq.p, d_so.p, d_sids.p + at, (int)ids.size(), seed_k,
                                   d_cnt.p + at, d_glen.p + at, d_poff.p + at, d_pairs.p);
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
            if (stats) stats->score_cells += 2L * sg.len(sids[k]) * glen[k];
        }
        seed->n_pairs = pair_off.back();
        n_tiles = 2L * seed->n_pairs;
        if (n_tiles > 0x7FFFFFFFL) return too_many(n_tiles);
        if (seed->n_pairs > 0) {
            { sc::DevMem<Pair> room((size_t)seed->n_pairs); std::swap(room.p, d_pairs.p); }
            st.h2d(d_poff, pair_off);
            lookup(std::true_type{});
            st.sync();                                          // the index goes with this scope
        }
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

}  // extern "C"
