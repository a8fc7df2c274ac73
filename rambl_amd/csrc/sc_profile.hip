// The per-sample gene profile on the device: every read segment of a sample against every assembled gene on both strands,
// the exact optimum of blastn's 1/-2 scoring with linear gaps and a fixed tie-break (DESIGN.md §8.9 is the contract) -- what
// scripts/per_sample_gene_profile_fast.py:80-153 runs makeblastdb, blastn, bigBlastParser and sqlite3 for.  Two kernels:
//   * k_bl_score: one wavefront per (segment, gene, strand) tile, the systolic sweep of k_sw_score (sc_align.hip) with a
//     linear-gap cell: only H per cell, max(0, diagonal + s, left - 5, up - 5) in doubled scores (+2 / -4 / -5).  Lane l
//     owns segment rows [l*R, l*R + R); H of its last row and the gene base move one lane down per step by DPP
//     (wave_shr:1).  A tile whose best doubled score reaches the segment's least passing score (E <= T, computed by the
//     host in double) appends one record (segment, gene, strand, best cell) to a bounded buffer: one vector atomicAdd per
//     emitted tile.
//   * k_bl_trace: one wavefront per (segment, gene) hit.  It recomputes the window that can hold an alignment of that
//     score ending at the chosen cell, in blocks of TB_COLS columns whose 2-bit directions live in LDS, and one lane walks
//     back through them: start cell, identity, alignment length.
// Integer DP in int32; doubled scores stay below 2^11.  No scratch: every per-row array is unrolled into registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/straincall_hip.h"

namespace {

constexpr int MAX_SEG = 512;
constexpr int MAX_GENE = 8192;
constexpr int MATCH2 = 2;               // doubled: match +1
constexpr int MISMATCH2 = -4;           // mismatch -2 (a base outside ACGT on either side is a mismatch)
constexpr int GAP2 = 5;                 // a gap of n bases -2.5 n
constexpr int TB_COLS = 128;            // columns of direction words in LDS per block: 128 * 64 lanes * 4 B = 32 KiB
constexpr int GENE_OTHER = 5;           // gene code of a base outside ACGT (a segment's is 4: the two never match)

// one lane down: lane l receives lane l - 1's value, lane 0 receives `first`
__device__ __forceinline__ int shr1(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false); }

// A tile's best cell: doubled score [63:32], 8191 - end column [31:19], 511 - end row [18:10].  Larger is better.
__device__ __forceinline__ unsigned long long make_key(int score2, int col, int row) {
    return ((unsigned long long)score2 << 32) | ((unsigned long long)(8191 - col) << 19) | ((unsigned long long)(511 - row) << 10);
}

struct Cand {
    int seg, gene2;                     // gene2 = gene * 2 + strand
    unsigned long long key;
};

// The rows of one lane: segment base codes with the strand applied (0..3 = ACGT, 4 = other, also beyond the last row).
template <int R> struct Rows {
    int rb[R];
    __device__ __forceinline__ void load(const uint8_t* sg, int L, int strand, int nrows, int lane) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            const int i = lane * R + k;
            rb[k] = 4;
            if (i < nrows) {
                int c = sg[strand ? L - 1 - i : i];
                if (strand && c < 4) c = 3 - c;
                rb[k] = c;
            }
        }
    }
};

// The systolic sweep over gene columns [0, ncols) of `gq` (codes).  SCORE: keys[k] = max over the columns of
// (H << 13 | 8191 - column) per row.  TRACE: the direction of every cell of columns [colA, colB] goes to
// bits[(column - colA) * 64 + lane], bits 2k..2k+1 of the word for row lane*R + k: 0 diagonal from a zero cell (the alignment
// starts here), 1 diagonal, 2 left (a gap in the segment), 3 up (a gap in the gene) -- in that order of preference.
template <int R, bool TRACE>
__device__ __forceinline__ void sweep(const uint8_t* gq, int ncols, const Rows<R>& rw, int nl, int lane, unsigned* keys,
                                      unsigned* bits, int colA, int colB) {
    int H[R];
#pragma unroll
    for (int k = 0; k < R; k++) { H[k] = 0; if (!TRACE) keys[k] = 0; }
    int hout = 0, hdiag = 0, gc = GENE_OTHER, genebuf = GENE_OTHER;
    const int steps = ncols + nl - 1;
    for (int t = 0; t < steps; t++) {
        if ((t & 63) == 0) { const int c = t + lane; genebuf = c < ncols ? (int)gq[c] : GENE_OTHER; }
        const int fresh = __builtin_amdgcn_readlane(genebuf, t & 63);
        const int hup = shr1(0, hout);
        gc = shr1(fresh, gc);
        const int j = t - lane;
        if (j >= 0 && j < ncols && lane < nl) {
            int hd = hdiag, hu = hup;
            unsigned word = 0;
            const unsigned cj = 8191u - (unsigned)j;
#pragma unroll
            for (int k = 0; k < R; k++) {
                const int hl = H[k];
                const int d = hd + (gc == rw.rb[k] ? MATCH2 : MISMATCH2);
                const int l = hl - GAP2, u = hu - GAP2;
                const int h = max(max(d, 0), max(l, u));
                if (TRACE) {
                    const unsigned src = h == d ? (hd > 0 ? 1u : 0u) : (h == l ? 2u : 3u);
                    word |= src << (2 * k);
                } else {
                    keys[k] = max(keys[k], ((unsigned)h << 13) | cj);
                }
                H[k] = h; hd = hl; hu = h;
            }
            hout = hu;
            if (TRACE && j >= colA && j <= colB) bits[(j - colA) * 64 + lane] = word;
        }
        hdiag = hup;
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_bl_score(const uint8_t* genes, const long* gene_off, int n_genes, const uint8_t* sg,
                                                  const long* seg_off, const int* sids, const int* min2, long n_tiles, Cand* cand,
                                                  unsigned cap, unsigned* n_cand) {
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (blockDim.x >> 6);
    for (long w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6))); w < n_tiles; w += nw) {
        const long six = w / (2L * n_genes);
        const int rem = (int)(w - six * 2L * n_genes), gene = rem >> 1, strand = rem & 1;
        const int seg = sids[six];
        const long r0 = seg_off[seg];
        const int L = (int)(seg_off[seg + 1] - r0);
        const long g0 = gene_off[gene];
        const int ncols = (int)(gene_off[gene + 1] - g0);
        Rows<R> rw;
        rw.load(sg + r0, L, strand, L, lane);
        unsigned keys[R];
        sweep<R, false>(genes + g0, ncols, rw, (L + R - 1) / R, lane, keys, nullptr, 0, -1);
        unsigned lb = 0;
        int lrow = 0;
#pragma unroll
        for (int k = 0; k < R; k++)
            if (lane * R + k < L && keys[k] > lb) { lb = keys[k]; lrow = lane * R + k; }
        unsigned long long key = lb ? make_key((int)(lb >> 13), 8191 - (int)(lb & 8191u), lrow) : 0ull;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long x = __shfl_xor(key, o);
            key = x > key ? x : key;
        }
        if (lane == 0 && (int)(key >> 32) >= min2[seg]) {
            const unsigned slot = atomicAdd(n_cand, 1u);
            if (slot < cap) { cand[slot].seg = seg; cand[slot].gene2 = rem; cand[slot].key = key; }
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
        const int S2 = (int)(key >> 32);
        const int jend = 8191 - (int)((key >> 19) & 8191), iend = 511 - (int)((key >> 10) & 511);
        const long r0 = seg_off[seg];
        const int L = (int)(seg_off[seg + 1] - r0);
        const uint8_t* gq = genes + gene_off[gene];
        const int nrows = iend + 1;
        // an alignment of doubled score S2 ending at row iend skips at most (2 * nrows - S2) / 5 gene bases
        const int nd = max(0, (MATCH2 * nrows - S2) / GAP2);
        const int j0 = max(0, jend - nrows - nd + 1), ncol = jend - j0 + 1;
        Rows<R> rw;
        rw.load(sg + r0, L, strand, nrows, lane);
        const int nl = (nrows + R - 1) / R;
        int i = iend, jw = ncol - 1, ident = 0, alen = 0, bad = 0, done = 0;
        for (int b = (ncol - 1) / TB_COLS; b >= 0; b--) {
            const int colA = b * TB_COLS, colB = min(colA + TB_COLS, ncol) - 1;
            sweep<R, true>(gq + j0, colB + 1, rw, nl, lane, nullptr, bits, colA, colB);
            __syncthreads();
            if (lane == 0) {
                while (!done && jw >= colA) {
                    if (i < 0) { bad = 1; break; }
                    const unsigned c = (bits[(jw - colA) * 64 + i / R] >> (2 * (i % R))) & 3u;
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
            done = __shfl(done | bad, 0);
            __syncthreads();
            if (done) break;
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

thread_local std::string tl_error;
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int fail(int rc, const std::string& msg) { tl_error = msg; return rc; }

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 16)) == hipSuccess; }
};

template <int R>
void launch_score(hipStream_t st, const uint8_t* genes, const long* gene_off, int n_genes, const uint8_t* sg, const long* seg_off,
                  const int* sids, const int* min2, long n_tiles, Cand* cand, unsigned cap, unsigned* n_cand) {
    const long blocks = std::min<long>((n_tiles + 3) / 4, 16384);
    hipLaunchKernelGGL(k_bl_score<R>, dim3((unsigned)blocks), dim3(256), 0, st, genes, gene_off, n_genes, sg, seg_off, sids, min2,
                       n_tiles, cand, cap, n_cand);
}
template <int R>
void launch_trace(hipStream_t st, const uint8_t* genes, const long* gene_off, const uint8_t* sg, const long* seg_off, const Cand* hits,
                  int n, int* out) {
    const int blocks = std::min(n, 8192);
    hipLaunchKernelGGL(k_bl_trace<R>, dim3((unsigned)blocks), dim3(64), 0, st, genes, gene_off, sg, seg_off, hits, n, out);
}
typedef void (*ScoreFn)(hipStream_t, const uint8_t*, const long*, int, const uint8_t*, const long*, const int*, const int*, long, Cand*,
                        unsigned, unsigned*);
typedef void (*TraceFn)(hipStream_t, const uint8_t*, const long*, const uint8_t*, const long*, const Cand*, int, int*);
const ScoreFn SCORE[8] = {launch_score<1>, launch_score<2>, launch_score<3>, launch_score<4>,
                          launch_score<5>, launch_score<6>, launch_score<7>, launch_score<8>};
const TraceFn TRACE[8] = {launch_trace<1>, launch_trace<2>, launch_trace<3>, launch_trace<4>,
                          launch_trace<5>, launch_trace<6>, launch_trace<7>, launch_trace<8>};

int code_of(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

// E = K m n e^(-lambda S) of a raw score S = score2 / 2, in double -- the one expression of the contract.
double evalue_of(double ka_k, double ka_lambda, int m, long n, int score2) {
    return ka_k * (double)m * (double)n * std::exp(-ka_lambda * (0.5 * (double)score2));
}

}  // namespace

extern "C" {

const char* sc_profile_error(void) { return tl_error.c_str(); }

int sc_profile_hits(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                    int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg, int* hit_gene,
                    int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                    double* evalue, long cap, long* n_hits, sc_profile_stats* stats) {
    tl_error.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_hits) *n_hits = 0;
    if (!gene_text || !gene_off || n_genes < 1 || n_segs < 0 || (n_segs > 0 && (!seg_text || !seg_off)) || !hit_seg || !hit_gene ||
        !hit_strand || !hit_score || !identity || !align_len || !qfrom || !qto || !hfrom || !hto || !evalue || cap < 0 || !n_hits)
        return fail(SC_ERR_ARG, "sc_profile_hits: missing argument");
    if (!(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0))
        return fail(SC_ERR_ARG, "sc_profile_hits: lambda and K must be positive, the E-value threshold not negative");
    for (int g = 0; g < n_genes; g++) {
        const long n = gene_off[g + 1] - gene_off[g];
        if (n < 1 || n > MAX_GENE)
            return fail(SC_ERR_UNSUPPORTED, "sc_profile_hits: gene " + std::to_string(g) + " has " + std::to_string(n) + " bases (1.." +
                                                std::to_string(MAX_GENE) + " supported)");
    }
    for (int r = 0; r < n_segs; r++) {
        const long n = seg_off[r + 1] - seg_off[r];
        if (n < 1 || n > MAX_SEG)
            return fail(SC_ERR_UNSUPPORTED, "sc_profile_hits: segment " + std::to_string(r) + " has " + std::to_string(n) + " bases (1.." +
                                                std::to_string(MAX_SEG) + " supported)");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SC_ERR_NO_DEVICE, "no HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(SC_ERR_HIP, "hipSetDevice failed");
    if (n_segs == 0) return SC_OK;
    const double t0 = wall_ms();
    // ---- host packing: gene and segment codes; per segment length the least doubled score with E <= T; segments bucketed by
    // rows per lane (a segment that cannot pass even with every base matched is in no bucket)
    const long gene_bytes = gene_off[n_genes] - gene_off[0];
    std::vector<uint8_t> gq((size_t)gene_bytes);
    std::vector<long> go((size_t)n_genes + 1);
    for (int g = 0; g <= n_genes; g++) go[(size_t)g] = gene_off[g] - gene_off[0];
    for (long k = 0; k < gene_bytes; k++) { const int c = code_of(gene_text[gene_off[0] + k]); gq[(size_t)k] = (uint8_t)(c < 0 ? GENE_OTHER : c); }
    const long seg_bytes = seg_off[n_segs] - seg_off[0];
    std::vector<uint8_t> sq((size_t)seg_bytes);
    std::vector<long> so((size_t)n_segs + 1);
    for (int r = 0; r <= n_segs; r++) so[(size_t)r] = seg_off[r] - seg_off[0];
    for (long k = 0; k < seg_bytes; k++) { const int c = code_of(seg_text[seg_off[0] + k]); sq[(size_t)k] = (uint8_t)(c < 0 ? 4 : c); }
    int min2_of_len[MAX_SEG + 1] = {};                          // 0: not computed yet (a hit has a positive score)
    std::vector<int> min2((size_t)n_segs);
    std::vector<int> by_r[8];
    for (int r = 0; r < n_segs; r++) {
        const int L = (int)(so[(size_t)r + 1] - so[(size_t)r]);
        int& s2 = min2_of_len[L];
        if (s2 == 0)
            for (s2 = 1; s2 <= MATCH2 * L && !(evalue_of(ka_k, ka_lambda, L, gene_bytes, s2) <= max_evalue);) s2++;
        min2[(size_t)r] = s2;
        if (s2 <= MATCH2 * L) by_r[(L + 63) / 64 - 1].push_back(r);
    }
    std::vector<int> sids;
    for (auto& v : by_r) sids.insert(sids.end(), v.begin(), v.end());
    long n_tiles = 0;
    for (auto& v : by_r) n_tiles += (long)v.size() * 2L * n_genes;
    if (n_tiles > 0x7FFFFFFFL)
        return fail(SC_ERR_UNSUPPORTED, "sc_profile_hits: " + std::to_string(n_tiles) + " (segment, gene, strand) tiles in one call (at most "
                                            "2147483647: pass the segments in several calls)");
    // every passing tile is a candidate; a (segment, gene) pair gives at most two, so 2 * cap + 1024 records hold them unless
    // the caller's cap is too small as well
    const long cand_cap = std::min<long>(n_tiles, std::min<long>(2 * cap + 1024, 0x7FFFFFFFL));
    // ---- device
    DevBuf d_gq, d_go, d_sq, d_so, d_sids, d_min2, d_cand, d_ncand;
    if (!d_gq.alloc(gq.size()) || !d_go.alloc(go.size() * sizeof(long)) || !d_sq.alloc(sq.size()) || !d_so.alloc(so.size() * sizeof(long)) ||
        !d_sids.alloc(sids.size() * sizeof(int)) || !d_min2.alloc(min2.size() * sizeof(int)) || !d_cand.alloc((size_t)cand_cap * sizeof(Cand)) ||
        !d_ncand.alloc(sizeof(unsigned)))
        return fail(SC_ERR_HIP, "hipMalloc failed");
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {};
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(SC_ERR_HIP, "hipStreamCreate failed");
    int rc = SC_OK;
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = SC_ERR_HIP;
    unsigned n_cand = 0;
    std::vector<Cand> cand;
    if (rc == SC_OK) {
        bool ok = hipEventRecord(ev[0], st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_gq.p, gq.data(), gq.size(), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_go.p, go.data(), go.size() * sizeof(long), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_sq.p, sq.data(), sq.size(), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_so.p, so.data(), so.size() * sizeof(long), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && (sids.empty() || hipMemcpyAsync(d_sids.p, sids.data(), sids.size() * sizeof(int), hipMemcpyHostToDevice, st) == hipSuccess);
        ok = ok && hipMemcpyAsync(d_min2.p, min2.data(), min2.size() * sizeof(int), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemsetAsync(d_ncand.p, 0, sizeof(unsigned), st) == hipSuccess;
        ok = ok && hipEventRecord(ev[1], st) == hipSuccess;
        long at = 0;
        for (int k = 0; k < 8 && ok; k++) {
            if (by_r[k].empty()) continue;
            const long nt = (long)by_r[k].size() * 2L * n_genes;
            SCORE[k](st, (const uint8_t*)d_gq.p, (const long*)d_go.p, n_genes, (const uint8_t*)d_sq.p, (const long*)d_so.p,
                     (const int*)d_sids.p + at, (const int*)d_min2.p, nt, (Cand*)d_cand.p, (unsigned)cand_cap, (unsigned*)d_ncand.p);
            ok = hipGetLastError() == hipSuccess;
            at += (long)by_r[k].size();
            if (stats) for (int r : by_r[k]) stats->score_cells += 2L * (so[(size_t)r + 1] - so[(size_t)r]) * gene_bytes;
        }
        ok = ok && hipEventRecord(ev[2], st) == hipSuccess;
        ok = ok && hipMemcpyAsync(&n_cand, d_ncand.p, sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (ok && (long)n_cand > cand_cap) {
            *n_hits = (long)n_cand;                              // an upper bound of the hits: a cap of this size suffices
            rc = fail(SC_ERR_CAPACITY, "sc_profile_hits: " + std::to_string(n_cand) + " tiles pass the E-value threshold, room for " +
                                           std::to_string(cap) + " hits");
        } else if (ok) {
            cand.resize(n_cand);
            ok = n_cand == 0 || hipMemcpy(cand.data(), d_cand.p, (size_t)n_cand * sizeof(Cand), hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (!ok) rc = SC_ERR_HIP;
        if (stats) { stats->n_tiles = n_tiles; stats->n_candidates = (long)n_cand; }
    }
    if (rc == SC_OK) {
        // ---- per (segment, gene) the better strand (ties: forward), in (segment, gene) order; the traceback of those, bucketed
        // by rows per lane again
        std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.seg != b.seg ? a.seg < b.seg : a.gene2 < b.gene2; });
        std::vector<Cand> pick;
        for (size_t k = 0; k < cand.size(); k++) {
            if (!pick.empty() && pick.back().seg == cand[k].seg && (pick.back().gene2 >> 1) == (cand[k].gene2 >> 1)) {
                if ((cand[k].key >> 32) > (pick.back().key >> 32)) pick.back() = cand[k];      // reverse only when strictly better
            } else {
                pick.push_back(cand[k]);
            }
        }
        std::vector<int> tr_r[8];
        for (size_t k = 0; k < pick.size(); k++) {
            const int L = (int)(so[(size_t)pick[k].seg + 1] - so[(size_t)pick[k].seg]);
            tr_r[(L + 63) / 64 - 1].push_back((int)k);
        }
        std::vector<int> order;
        for (auto& v : tr_r) order.insert(order.end(), v.begin(), v.end());
        const int n_tr = (int)order.size();
        std::vector<Cand> tlist((size_t)n_tr);
        for (int t = 0; t < n_tr; t++) tlist[(size_t)t] = pick[(size_t)order[(size_t)t]];
        std::vector<int> tout((size_t)n_tr * 4);
        DevBuf d_hits, d_out;
        bool ok = d_hits.alloc((size_t)n_tr * sizeof(Cand)) && d_out.alloc((size_t)n_tr * 16);
        ok = ok && (n_tr == 0 || hipMemcpyAsync(d_hits.p, tlist.data(), (size_t)n_tr * sizeof(Cand), hipMemcpyHostToDevice, st) == hipSuccess);
        ok = ok && hipEventRecord(ev[3], st) == hipSuccess;
        int at = 0;
        for (int k = 0; k < 8 && ok; k++) {
            if (tr_r[k].empty()) continue;
            TRACE[k](st, (const uint8_t*)d_gq.p, (const long*)d_go.p, (const uint8_t*)d_sq.p, (const long*)d_so.p, (const Cand*)d_hits.p + at,
                     (int)tr_r[k].size(), (int*)d_out.p + 4L * at);
            ok = hipGetLastError() == hipSuccess;
            at += (int)tr_r[k].size();
        }
        ok = ok && hipEventRecord(ev[4], st) == hipSuccess;
        ok = ok && (n_tr == 0 || hipMemcpyAsync(tout.data(), d_out.p, (size_t)n_tr * 16, hipMemcpyDeviceToHost, st) == hipSuccess);
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) rc = fail(SC_ERR_HIP, "sc_profile_hits: a HIP call failed");
        // ---- the hits that pass, back in (segment, gene) order
        std::vector<int> slot_of((size_t)n_tr);
        for (int t = 0; t < n_tr; t++) slot_of[(size_t)order[(size_t)t]] = t;
        long n_out = 0;
        for (int k = 0; k < n_tr && rc == SC_OK; k++) {
            const int t = slot_of[(size_t)k];
            const Cand& c = pick[(size_t)k];
            const int* o = &tout[(size_t)t * 4];
            if (o[0] < 0) {
                rc = fail(SC_ERR_INTERNAL, "sc_profile_hits: traceback of segment " + std::to_string(c.seg) + " on gene " +
                                               std::to_string(c.gene2 >> 1) + " failed");
                break;
            }
            const int L = (int)(so[(size_t)c.seg + 1] - so[(size_t)c.seg]);
            const int S2 = (int)(c.key >> 32), jend = 8191 - (int)((c.key >> 19) & 8191), iend = 511 - (int)((c.key >> 10) & 511);
            const int strand = c.gene2 & 1, j0 = o[0], i0 = o[1];
            if (stats) {
                const int nrows = iend + 1, w0 = std::max(0, jend - nrows - std::max(0, (MATCH2 * nrows - S2) / GAP2) + 1);
                const long nb = (jend - w0) / TB_COLS + 1, ncol = jend - w0 + 1;
                long swept = 0;
                for (long b = nb - 1; b >= 0 && b * TB_COLS + TB_COLS > j0 - w0; b--) swept += std::min(ncol, (b + 1) * TB_COLS);
                stats->trace_cells += swept * nrows;
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
            if (n_out > cap) rc = fail(SC_ERR_CAPACITY, "sc_profile_hits: " + std::to_string(n_out) + " hits, room for " + std::to_string(cap));
        }
        if (stats && (rc == SC_OK || rc == SC_ERR_CAPACITY)) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) stats->upload_ms = ms;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) stats->score_ms = ms;
            if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) stats->trace_ms = ms;
            stats->n_traced = n_tr;
            stats->n_hits = n_out;
        }
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(st);
    if (stats) stats->total_ms = wall_ms() - t0;
    if (rc == SC_ERR_HIP && tl_error.empty()) tl_error = "sc_profile_hits: a HIP call failed";
    return rc;
}

}  // extern "C"
