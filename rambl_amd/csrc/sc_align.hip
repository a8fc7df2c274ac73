// Stage 4 of rambl.py on the device: every gene read aligned to every seed OTU on both strands, the exact optimum of
// bowtie2's --local scoring (DESIGN.md §8.7 is the contract) -- what scripts/recluster_data_to_seed_otus.py:198-277
// runs bowtie2 --sensitive-local for.  Two kernels:
//   * k_sw_score: one wavefront per (read, seed, strand) tile.  Lane l owns read rows [l*R, l*R + R) (R = ceil(L / 64)) and
//     the seed is swept column by column as a systolic array: at step t lane l computes column t - l, H and F of its last row
//     and the seed base move one lane down per step by DPP (wave_shr:1), so a cell never goes through LDS.  The tile's best
//     cell becomes one 64-bit key (score, then the tie-break of the contract: lower seed, forward strand, smaller end column,
//     smaller end row); per read one vector atomicMax keeps the best key and a second one the best of the keys it displaced
//     or beat, which is the best of every other (seed, strand): XS.
//   * k_sw_trace: one wavefront per aligned read.  It recomputes only the window that can hold an alignment of the best
//     score ending at the chosen cell (rows 0..end row, columns back as far as the score allows deletions), in blocks of
//     TB_COLS columns whose direction nibbles live in LDS, and one lane walks back through them: POS, CIGAR, NM.
// Integer DP in int32; scores stay below 2^11.  No scratch: every per-row array is unrolled into registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/straincall_hip.h"

namespace {

constexpr int MAX_READ = 512;
constexpr int MAX_SEED = 8192;
constexpr int MAX_SEEDS = (1 << 20) - 1;
constexpr int GBAR = 4;                 // --gbar 4
constexpr int GAP_OPEN = 8;             // --rdg 5,3 / --rfg 5,3: 5 + 3n for a gap of n
constexpr int GAP_EXT = 3;
constexpr int BARRED = 1 << 20;         // open / extend cost of a row where no gap may be
constexpr int NEG = -(1 << 20);         // E and F before any gap
constexpr int TB_COLS = 128;            // columns of direction nibbles in LDS per block: 128 * 64 lanes * 4 B = 32 KiB
constexpr int SEED_OTHER = 5;           // seed code of a base outside ACGT (a read's is 4: the two never match)

// one lane down: lane l receives lane l - 1's value, lane 0 receives `first`
__device__ __forceinline__ int shr1(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false); }

// The key of a tile's best cell: score [63:53], 0xFFFFF - seed [52:33], forward [32], 8191 - end column [31:19],
// 511 - end row [18:10].  Larger is better.
__device__ __forceinline__ unsigned long long make_key(int score, int seed, int strand, int col, int row) {
    return ((unsigned long long)score << 53) | ((unsigned long long)(0xFFFFF - seed) << 33) | ((unsigned long long)(1 - strand) << 32) |
           ((unsigned long long)(8191 - col) << 19) | ((unsigned long long)(511 - row) << 10);
}

// The rows of one lane: read base codes (strand applied), mismatch penalties and the gap costs of the rows (--gbar).
// rd[i] = code | penalty << 4 (code 0..3 = ACGT, 4 = other; penalty = 1 for other, else 2 + floor(min(Q,40) / 10)).
template <int R> struct Rows {
    int rb[R], pen[R], go[R], ge[R];
    __device__ __forceinline__ void load(const uint8_t* rd, int L, int strand, int nrows, int lane) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            const int i = lane * R + k;
            rb[k] = 4; pen[k] = -1; go[k] = BARRED; ge[k] = BARRED;
            if (i < nrows) {
                const int b = rd[strand ? L - 1 - i : i];
                int c = b & 15;
                if (strand && c < 4) c = 3 - c;
                rb[k] = c;
                pen[k] = -(b >> 4);
                if (i >= GBAR && i < L - GBAR) { go[k] = GAP_OPEN; ge[k] = GAP_EXT; }
            }
        }
    }
};

// The systolic sweep over seed columns [0, ncols) of `sq` (codes).  SCORE: keys[k] = max over the columns of
// (H << 13 | 8191 - column) per row.  TRACE: the direction nibble of every cell of columns [colA, colB] goes to
// bits[(column - colA) * 64 + lane], nibble k of the word for row lane*R + k:
//   bits 0-1: how H was reached -- 0 diagonal from a zero cell (the alignment starts here), 1 diagonal, 2 E (D), 3 F (I)
//             (diagonal before D before I);
//   bit 2: E extends E of the column before (extension preferred on a tie); bit 3: F extends F of the row above.
template <int R, bool TRACE>
__device__ __forceinline__ void sweep(const uint8_t* sq, int ncols, const Rows<R>& rw, int nl, int lane, unsigned* keys,
                                      unsigned* bits, int colA, int colB) {
    int H[R], E[R];
#pragma unroll
    for (int k = 0; k < R; k++) { H[k] = 0; E[k] = NEG; if (!TRACE) keys[k] = 0; }
    int hout = 0, fout = NEG, hdiag = 0, rc = SEED_OTHER, refbuf = SEED_OTHER;
    const int steps = ncols + nl - 1;
    for (int t = 0; t < steps; t++) {
        if ((t & 63) == 0) { const int c = t + lane; refbuf = c < ncols ? (int)sq[c] : SEED_OTHER; }
        const int fresh = __builtin_amdgcn_readlane(refbuf, t & 63);
        const int hup = shr1(0, hout), fup = shr1(NEG, fout);
        rc = shr1(fresh, rc);
        const int j = t - lane;
        if (j >= 0 && j < ncols && lane < nl) {
            const int nv = rc > 3 ? -1 : -64;          // a seed base outside ACGT scores -1 against anything
            int hd = hdiag, f = fup, hu = hup;
            unsigned word = 0;
            const unsigned cj = 8191u - (unsigned)j;
#pragma unroll
            for (int k = 0; k < R; k++) {
                const int hp = H[k];
                const int eo = E[k] - GAP_EXT, eg = hp - rw.go[k];
                const int e = max(eo, eg);
                const int fo = f - rw.ge[k], fg = hu - rw.go[k];
                f = max(fo, fg);
                const int s = max(rc == rw.rb[k] ? 2 : rw.pen[k], nv);
                const int d = hd + s;
                const int h = max(max(d, 0), max(e, f));
                if (TRACE) {
                    const unsigned src = h == d ? (hd > 0 ? 1u : 0u) : (h == e ? 2u : 3u);
                    word |= (src | (eo >= eg ? 4u : 0u) | (fo >= fg ? 8u : 0u)) << (4 * k);
                } else {
                    keys[k] = max(keys[k], ((unsigned)h << 13) | cj);
                }
                E[k] = e; H[k] = h; hd = hp; hu = h;
            }
            hout = hu; fout = f;
            if (TRACE && j >= colA && j <= colB) bits[(j - colA) * 64 + lane] = word;
        }
        hdiag = hup;
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_sw_score(const uint8_t* seeds, const long* seed_off, int n_seeds, const uint8_t* rd,
                                                  const long* rd_off, const int* rids, long n_tiles, unsigned long long* best,
                                                  unsigned long long* second) {
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (blockDim.x >> 6);
    for (long w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6))); w < n_tiles; w += nw) {
        const long rix = w / (2L * n_seeds);
        const int rem = (int)(w - rix * 2L * n_seeds), seed = rem >> 1, strand = rem & 1;
        const int read = rids[rix];
        const long r0 = rd_off[read];
        const int L = (int)(rd_off[read + 1] - r0);
        const long s0 = seed_off[seed];
        const int ncols = (int)(seed_off[seed + 1] - s0);
        Rows<R> rw;
        rw.load(rd + r0, L, strand, L, lane);
        unsigned keys[R];
        sweep<R, false>(seeds + s0, ncols, rw, (L + R - 1) / R, lane, keys, nullptr, 0, -1);
        unsigned lb = 0;
        int lrow = 0;
#pragma unroll
        for (int k = 0; k < R; k++)
            if (lane * R + k < L && keys[k] > lb) { lb = keys[k]; lrow = lane * R + k; }
        unsigned long long key = lb ? make_key((int)(lb >> 13), seed, strand, 8191 - (int)(lb & 8191u), lrow) : 0ull;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long x = __shfl_xor(key, o);
            key = x > key ? x : key;
        }
        if (lane == 0) {
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
        const int S = (int)(key >> 53), seed = 0xFFFFF - (int)((key >> 33) & 0xFFFFF), strand = 1 - (int)((key >> 32) & 1);
        const int jend = 8191 - (int)((key >> 19) & 8191), iend = 511 - (int)((key >> 10) & 511);
        const long r0 = rd_off[read];
        const int L = (int)(rd_off[read + 1] - r0);
        const uint8_t* sq = seeds + seed_off[seed];
        const int nrows = iend + 1;
        // an alignment of score S ending at row iend has at most (2 * nrows - S) / 3 deleted seed bases
        const int nd = max(0, (2 * nrows - S) / 3);
        const int j0 = max(0, jend - nrows - nd + 1), ncol = jend - j0 + 1;
        Rows<R> rw;
        rw.load(rd + r0, L, strand, nrows, lane);
        const int nl = (nrows + R - 1) / R;
        unsigned* oc = cig + (long)t * stride;
        int st = 0, i = iend, jw = ncol - 1, nm = 0, nops = 0, cur_op = -1, cur_len = 0, bad = 0, done = 0;
        auto push = [&](int op, int n) {
            if (op == cur_op) { cur_len += n; return; }
            if (cur_op >= 0) { if (nops < stride) oc[nops] = ((unsigned)cur_len << 4) | (unsigned)cur_op; else bad = 1; nops++; }
            cur_op = op; cur_len = n;
        };
        if (lane == 0 && L - 1 - iend > 0) push(4, L - 1 - iend);
        for (int b = (ncol - 1) / TB_COLS; b >= 0; b--) {
            const int colA = b * TB_COLS, colB = min(colA + TB_COLS, ncol) - 1;
            sweep<R, true>(sq + j0, colB + 1, rw, nl, lane, nullptr, bits, colA, colB);
            __syncthreads();
            if (lane == 0) {
                while (!done && !bad && jw >= colA) {
                    if (i < 0) { bad = 1; break; }
                    const unsigned nib = (bits[(jw - colA) * 64 + i / R] >> (4 * (i % R))) & 15u;
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
            done = __shfl(done | bad, 0);
            __syncthreads();
            if (done) break;
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

thread_local std::string tl_error;
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int fail(int rc, const std::string& msg) { tl_error = msg; return rc; }

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 16)) == hipSuccess; }
};

template <int R>
void launch_score(hipStream_t st, const uint8_t* seeds, const long* seed_off, int n_seeds, const uint8_t* rd, const long* rd_off,
                  const int* rids, long n_tiles, unsigned long long* best, unsigned long long* second) {
    const long blocks = std::min<long>((n_tiles + 3) / 4, 16384);
    hipLaunchKernelGGL(k_sw_score<R>, dim3((unsigned)blocks), dim3(256), 0, st, seeds, seed_off, n_seeds, rd, rd_off, rids, n_tiles,
                       best, second);
}
template <int R>
void launch_trace(hipStream_t st, const uint8_t* seeds, const long* seed_off, const uint8_t* rd, const long* rd_off, const int* tids,
                  int n, const unsigned long long* best, int* out, unsigned* cig, int stride) {
    const int blocks = std::min(n, 8192);
    hipLaunchKernelGGL(k_sw_trace<R>, dim3((unsigned)blocks), dim3(64), 0, st, seeds, seed_off, rd, rd_off, tids, n, best, out, cig, stride);
}
typedef void (*ScoreFn)(hipStream_t, const uint8_t*, const long*, int, const uint8_t*, const long*, const int*, long,
                        unsigned long long*, unsigned long long*);
typedef void (*TraceFn)(hipStream_t, const uint8_t*, const long*, const uint8_t*, const long*, const int*, int,
                        const unsigned long long*, int*, unsigned*, int);
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

}  // namespace

extern "C" {

const char* sc_align_error(void) { return tl_error.c_str(); }

int sc_align_reads(int device, const char* seed_text, const long* seed_off, int n_seeds, const char* read_text, const char* qual_text,
                   const long* read_off, int n_reads, int* as, int* xs, int* seed, int* strand, int* pos, int* nm, unsigned* cigar,
                   int cigar_stride, int* n_cigar, sc_align_stats* stats) {
    tl_error.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!seed_text || !seed_off || n_seeds < 1 || n_reads < 0 || (n_reads > 0 && (!read_text || !read_off)) || !as || !xs || !seed ||
        !strand || !pos || !nm || !cigar || cigar_stride < 1 || !n_cigar)
        return fail(SC_ERR_ARG, "sc_align_reads: missing argument");
    if (n_seeds > MAX_SEEDS) return fail(SC_ERR_UNSUPPORTED, "sc_align_reads: more than 1048575 seeds");
    for (int s = 0; s < n_seeds; s++) {
        const long n = seed_off[s + 1] - seed_off[s];
        if (n < 1 || n > MAX_SEED)
            return fail(SC_ERR_UNSUPPORTED, "sc_align_reads: seed " + std::to_string(s) + " has " + std::to_string(n) + " bases (1.." +
                                                std::to_string(MAX_SEED) + " supported)");
    }
    int max_len = 0;
    for (int r = 0; r < n_reads; r++) {
        const long n = read_off[r + 1] - read_off[r];
        if (n < 1 || n > MAX_READ)
            return fail(SC_ERR_UNSUPPORTED, "sc_align_reads: read " + std::to_string(r) + " has " + std::to_string(n) + " bases (1.." +
                                                std::to_string(MAX_READ) + " supported)");
        max_len = std::max(max_len, (int)n);
    }
    if (cigar_stride < max_len / 2 + 4) return fail(SC_ERR_CAPACITY, "sc_align_reads: cigar_stride below max read length / 2 + 4");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SC_ERR_NO_DEVICE, "no HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(SC_ERR_HIP, "hipSetDevice failed");
    if (n_reads == 0) return SC_OK;
    const double t0 = wall_ms();
    // ---- host packing: seed codes, read code | penalty << 4, reads bucketed by rows per lane
    const long seed_bytes = seed_off[n_seeds] - seed_off[0];
    std::vector<uint8_t> sq((size_t)seed_bytes);
    std::vector<long> so((size_t)n_seeds + 1);
    for (int s = 0; s <= n_seeds; s++) so[(size_t)s] = seed_off[s] - seed_off[0];
    for (long k = 0; k < seed_bytes; k++) { const int c = code_of(seed_text[seed_off[0] + k]); sq[(size_t)k] = (uint8_t)(c < 0 ? SEED_OTHER : c); }
    const long read_bytes = read_off[n_reads] - read_off[0];
    std::vector<uint8_t> rq((size_t)read_bytes);
    std::vector<long> ro((size_t)n_reads + 1);
    for (int r = 0; r <= n_reads; r++) ro[(size_t)r] = read_off[r] - read_off[0];
    for (long k = 0; k < read_bytes; k++) {
        const int c = code_of(read_text[read_off[0] + k]);
        int q = qual_text ? (int)(unsigned char)qual_text[read_off[0] + k] - 33 : 40;
        q = std::min(std::max(q, 0), 40);
        const int pen = c < 0 ? 1 : 2 + q / 10;
        rq[(size_t)k] = (uint8_t)((c < 0 ? 4 : c) | (pen << 4));
    }
    std::vector<int> by_r[8];
    for (int r = 0; r < n_reads; r++) by_r[(ro[(size_t)r + 1] - ro[(size_t)r] + 63) / 64 - 1].push_back(r);
    std::vector<int> rids;
    for (auto& v : by_r) rids.insert(rids.end(), v.begin(), v.end());
    // ---- device
    DevBuf d_sq, d_so, d_rq, d_ro, d_rids, d_best, d_second;
    if (!d_sq.alloc(sq.size()) || !d_so.alloc(so.size() * sizeof(long)) || !d_rq.alloc(rq.size()) || !d_ro.alloc(ro.size() * sizeof(long)) ||
        !d_rids.alloc(rids.size() * sizeof(int)) || !d_best.alloc((size_t)n_reads * 8) || !d_second.alloc((size_t)n_reads * 8))
        return fail(SC_ERR_HIP, "hipMalloc failed");
    hipStream_t st = nullptr;
    hipEvent_t ev[6] = {};
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(SC_ERR_HIP, "hipStreamCreate failed");
    int rc = SC_OK;
    for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = SC_ERR_HIP;
    std::vector<unsigned long long> best((size_t)n_reads), second((size_t)n_reads);
    std::vector<int> tids, tout;
    std::vector<unsigned> tcig;
    if (rc == SC_OK) {
        bool ok = hipEventRecord(ev[0], st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_sq.p, sq.data(), sq.size(), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_so.p, so.data(), so.size() * sizeof(long), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_rq.p, rq.data(), rq.size(), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_ro.p, ro.data(), ro.size() * sizeof(long), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(d_rids.p, rids.data(), rids.size() * sizeof(int), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipMemsetAsync(d_best.p, 0, (size_t)n_reads * 8, st) == hipSuccess;
        ok = ok && hipMemsetAsync(d_second.p, 0, (size_t)n_reads * 8, st) == hipSuccess;
        ok = ok && hipEventRecord(ev[1], st) == hipSuccess;
        long at = 0;
        for (int k = 0; k < 8 && ok; k++) {
            if (by_r[k].empty()) continue;
            const long n_tiles = (long)by_r[k].size() * 2L * n_seeds;
            SCORE[k](st, (const uint8_t*)d_sq.p, (const long*)d_so.p, n_seeds, (const uint8_t*)d_rq.p, (const long*)d_ro.p,
                     (const int*)d_rids.p + at, n_tiles, (unsigned long long*)d_best.p, (unsigned long long*)d_second.p);
            ok = hipGetLastError() == hipSuccess;
            at += (long)by_r[k].size();
            if (stats) for (int r : by_r[k]) stats->score_cells += 2L * (ro[(size_t)r + 1] - ro[(size_t)r]) * seed_bytes;
        }
        ok = ok && hipEventRecord(ev[2], st) == hipSuccess;
        ok = ok && hipMemcpyAsync(best.data(), d_best.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(second.data(), d_second.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) rc = SC_ERR_HIP;
    }
    if (rc == SC_OK) {
        // ---- which reads align; the traceback of those, bucketed by rows per lane again
        std::vector<int> tr_r[8];
        for (int r = 0; r < n_reads; r++) {
            const int L = (int)(ro[(size_t)r + 1] - ro[(size_t)r]);
            const double thr = 20.0 + 8.0 * std::log((double)L);
            const int S = (int)(best[(size_t)r] >> 53), X = (int)(second[(size_t)r] >> 53);
            as[r] = S;
            xs[r] = (double)X >= thr ? X : -1;
            seed[r] = -1; strand[r] = 0; pos[r] = 0; nm[r] = 0; n_cigar[r] = 0;
            if ((double)S >= thr) tr_r[(L + 63) / 64 - 1].push_back(r);
        }
        for (auto& v : tr_r) tids.insert(tids.end(), v.begin(), v.end());
        const int n_tr = (int)tids.size();
        tout.resize((size_t)n_tr * 4);
        tcig.resize((size_t)n_tr * (size_t)cigar_stride);
        DevBuf d_tids, d_out, d_cig;
        bool ok = d_tids.alloc((size_t)n_tr * 4) && d_out.alloc((size_t)n_tr * 16) && d_cig.alloc(tcig.size() * 4);
        ok = ok && hipMemcpyAsync(d_tids.p, tids.data(), (size_t)n_tr * 4, hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && hipEventRecord(ev[3], st) == hipSuccess;
        int at = 0;
        for (int k = 0; k < 8 && ok; k++) {
            if (tr_r[k].empty()) continue;
            TRACE[k](st, (const uint8_t*)d_sq.p, (const long*)d_so.p, (const uint8_t*)d_rq.p, (const long*)d_ro.p, (const int*)d_tids.p + at,
                     (int)tr_r[k].size(), (const unsigned long long*)d_best.p, (int*)d_out.p + 4L * at, (unsigned*)d_cig.p + (long)at * cigar_stride,
                     cigar_stride);
            ok = hipGetLastError() == hipSuccess;
            at += (int)tr_r[k].size();
        }
        ok = ok && hipEventRecord(ev[4], st) == hipSuccess;
        ok = ok && hipMemcpyAsync(tout.data(), d_out.p, (size_t)n_tr * 16, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(tcig.data(), d_cig.p, tcig.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipEventRecord(ev[5], st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) rc = fail(SC_ERR_HIP, "sc_align_reads: a HIP call failed");
        for (int t = 0; t < n_tr && rc == SC_OK; t++) {
            const int r = tids[(size_t)t];
            const unsigned long long key = best[(size_t)r];
            if (tout[(size_t)t * 4] < 0) { rc = fail(SC_ERR_INTERNAL, "sc_align_reads: traceback of read " + std::to_string(r) + " failed"); break; }
            seed[r] = 0xFFFFF - (int)((key >> 33) & 0xFFFFF);
            strand[r] = 1 - (int)((key >> 32) & 1);
            pos[r] = tout[(size_t)t * 4] + 1;
            nm[r] = tout[(size_t)t * 4 + 2];
            n_cigar[r] = tout[(size_t)t * 4 + 3];
            std::memcpy(cigar + (long)r * cigar_stride, tcig.data() + (size_t)t * cigar_stride, sizeof(unsigned) * (size_t)n_cigar[r]);
            if (stats) {
                const int S = (int)(key >> 53), nrows = 512 - (int)((key >> 10) & 511);
                const int jend = 8191 - (int)((key >> 19) & 8191), j0 = std::max(0, jend - nrows - std::max(0, (2 * nrows - S) / 3) + 1);
                const long nb = (jend - j0) / TB_COLS + 1, ncol = jend - j0 + 1;
                long swept = 0;
                for (long b = 0; b < nb; b++) swept += std::min(ncol, (b + 1) * TB_COLS);
                stats->trace_cells += swept * nrows;
            }
        }
        if (stats && rc == SC_OK) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) stats->upload_ms = ms;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) stats->score_ms = ms;
            if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) stats->trace_ms = ms;
            stats->n_traced = n_tr;
        }
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(st);
    if (stats) stats->total_ms = wall_ms() - t0;
    if (rc == SC_ERR_HIP && tl_error.empty()) tl_error = "sc_align_reads: a HIP call failed";
    return rc;
}

}  // extern "C"
