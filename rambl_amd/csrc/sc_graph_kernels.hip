// HIP kernels of the graph stage for gfx950 (MI355X, CDNA4, wave64).
//
//   k_thread_*       threading of the reads along the backbone                 (row a5)
//   k_msa            progressive sum-of-pairs MSA of insertion strings          (a7, a8)
//   k_edge_support   number_of_reads_cover_nodes for every edge                (a16)
//
// Integer loops bound by latency or HBM: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "sc_device.hpp"

namespace sc {

// --------------------------------------------------------------------------
// a16: support of edge e = (u -> v): PartialOrderGraph.cpp:1218-1244.
// One wavefront per edge; pools are rid-sorted (checked on the host, `sorted`),
// so the multiplicity of a read in u's pool comes from two binary searches.
__global__ __launch_bounds__(256) void k_edge_support(const int* __restrict__ out_ptr, const int* __restrict__ out_node,
                                                      const int* __restrict__ pool_ptr, const int* __restrict__ pool_rid,
                                                      const int* __restrict__ pool_cn, const uint8_t* __restrict__ node_is_end,
                                                      const int* __restrict__ edge_src, int n_edges, int sorted,
                                                      int* __restrict__ support) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int e = wave; e < n_edges; e += nwaves) {
        const int u = edge_src[e], v = out_node[e];
        const int ub = pool_ptr[u], ue = pool_ptr[u + 1], vb = pool_ptr[v], ve = pool_ptr[v + 1];
        long acc = 0;
        if (u == 0) {
            for (int j = vb + lane; j < ve; j += 64) acc += pool_cn[j];
        } else if (node_is_end[v]) {
            for (int i = ub + lane; i < ue; i += 64) acc += pool_cn[i];
        } else {
            for (int j = vb + lane; j < ve; j += 64) {
                const int rid = pool_rid[j];
                int mult = 0;
                if (sorted) {
                    int lo = ub, hi = ue;                 // lower_bound
                    while (lo < hi) { int mid = (lo + hi) >> 1; if (pool_rid[mid] < rid) lo = mid + 1; else hi = mid; }
                    int lo2 = lo, hi2 = ue;               // upper_bound
                    while (lo2 < hi2) { int mid = (lo2 + hi2) >> 1; if (pool_rid[mid] <= rid) lo2 = mid + 1; else hi2 = mid; }
                    mult = lo2 - lo;
                } else {
                    for (int i = ub; i < ue; i++) mult += (pool_rid[i] == rid);
                }
                acc += (long)mult * pool_cn[j];
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) support[e] = (int)acc;
    }
    (void)out_ptr;
}

// --------------------------------------------------------------------------
// a7/a8: progressive sum-of-pairs MSA, MultipleSequenceAlignmentSP.cpp:10-301,
// scored with SimpleDnaScore (SimpleDnaScore.cpp:15-42, Score.hpp:35).
//
// The per-row gap memory PP of the reference is uniform over the rows of a cell
// everywhere except in column j = 0 (its writers never advance the row iterator,
// :208-217/:235-245), so the three sum-of-pairs candidates of a cell reduce to
// dot products of the column's character counts with the score table.  The DP of
// one progressive step runs on one wavefront: lane j owns DP column j and the
// (i-1,j-1)/(i,j-1) dependencies arrive from lane j-1 through a lane shift, one
// anti-diagonal per iteration.  All values are small integers (exact in int32).
__device__ __forceinline__ int cls_of(char c) {
    switch (c) {
        case 'A': return 0; case 'a': return 1; case 'C': return 2; case 'c': return 3;
        case 'G': return 4; case 'g': return 5; case 'T': return 6; case 't': return 7;
        case '+': return 8; case '-': return 9; default: return 10;
    }
}
__device__ __forceinline__ int dna_score_cls(int x, int y) {
    if (x > 9 || y > 9) return 0;                 // std::map operator[] on a missing key
    if (x == y) return 3;
    if (x < 8 && y < 8 && (x >> 1) == (y >> 1)) return 3;
    if ((x == 8 && y == 9) || (x == 9 && y == 8)) return 3;
    if (x == 8 || y == 8) return -6;              // gap_open + gap_extend
    if (x == 9 || y == 9) return -2;              // gap_extend
    return -5;
}


constexpr int MSA_CM = 1024;                       // widest alignment (columns) kept in LDS
constexpr size_t MSA_LDS = 2 * MSA_CM * 10 * sizeof(unsigned short) + 2 * MSA_CM + (MSA_CM + 1) * 64 + 2 * (MSA_CM + 64) * sizeof(int);

// WIDE: the alignment may grow past MSA_CM columns (hundreds of distinct insertion strings at one site:
// the reference's scoring tends to open new columns); the same state then lives in HBM scratch sized for
// the sum of the sequence lengths instead of LDS.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_msa(MsaDev d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char m_raw[];
    const int CM = WIDE ? d.cmax : MSA_CM;                                        // capacity in columns
    unsigned short* s_cnt = WIDE ? reinterpret_cast<unsigned short*>(d.counts)    // [2][CM][10] class counts per column
                                 : reinterpret_cast<unsigned short*>(m_raw);
    char* s_c0 = reinterpret_cast<char*>(s_cnt + 2 * (size_t)CM * 10);            // [2][CM] row-0 character per column
    unsigned char* s_mv = WIDE ? d.moves : reinterpret_cast<unsigned char*>(s_c0 + 2 * CM);    // [(CM+1)][64] traceback moves
    int* s_trace = WIDE ? d.trace : reinterpret_cast<int*>(s_mv + (CM + 1) * 64);              // [2*(CM+64)]
    __shared__ int s_ncol, s_newn, s_err;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int n = d.n;
    int cur = 0;
    if (tid == 0) { s_ncol = d.seq_off[1] - d.seq_off[0]; s_err = (s_ncol > CM ? 2 : 0) | (n > 65535 ? 8 : 0); }
    __syncthreads();
    if (!s_err) {   // first sequence: one column per character
        const int l0 = s_ncol;
        for (int c = tid; c < l0; c += nt) {
            const char ch = d.seqs[d.seq_off[0] + c];
            d.cols[0][(long)c * n + 0] = ch;
            for (int k = 0; k < 10; k++) s_cnt[c * 10 + k] = 0;
            const int cl = cls_of(ch);
            if (cl < 10) s_cnt[c * 10 + cl] = 1;
            s_c0[c] = ch;
        }
    }
    __syncthreads();
    for (int t = 1; t < n && !s_err; t++) {
        const int s = t;                                  // rows already aligned
        const int ncol = s_ncol;
        const int m = ncol + 1;
        const char* seq = d.seqs + d.seq_off[t];
        const int len = d.seq_off[t + 1] - d.seq_off[t];
        const int nn = len + 1;
        const int mvs = WIDE ? d.mv_stride : 64;          // DP columns the traceback table holds per row
        if (nn > mvs || ncol + len > CM || ncol + len > d.cmax) {
            if (tid == 0) s_err = (nn > mvs ? 1 : 0) | (ncol + len > CM ? 2 : 0) | (ncol + len > d.cmax ? 4 : 0);
            __syncthreads();
            break;
        }
        const char* colc = d.cols[cur];
        const unsigned short* cntc = s_cnt + (size_t)cur * CM * 10;
        const char* c0c = s_c0 + (size_t)cur * CM;
        // ---- forward, wave 0: lane l = DP column j = 64 * chunk + l, time step tau handles row i = tau - l.  A sequence of
        // more than 63 bases takes several chunks of 64 columns, one after the other; the last column of a chunk leaves its
        // cells in `edge` (row by row), where lane 0 of the next chunk finds its left and diagonal neighbours
        if (tid < 64)
        for (int chunk = 0; chunk * 64 < nn; chunk++) {
            const int j = chunk * 64 + lane;
            const bool more = (chunk + 1) * 64 < nn;          // another chunk follows: record the last column
            int* edge = WIDE ? d.edge : nullptr;              // [2][m]: score, state of the cells (i, 64 * chunk - 1)
            const int b = (j >= 1 && j < nn) ? cls_of(seq[j - 1]) : 10;
            int scb[9];
#pragma unroll
            for (int c = 0; c < 9; c++) scb[c] = dna_score_cls(c, b);
            const int sb_minus = dna_score_cls(9, b), sb_plus = dna_score_cls(8, b);
            int sc_up = 0;          // SC[i-1][j]
            int st_up = 0;          // state of cell (i-1, j): 0 mat, 1 ins, 2 del
            // row 0: SC[0][j] = s*(-6) + (j-1)*s*(-2), state ins for j >= 1, mat at j = 0
            if (j >= 1) { sc_up = s * (-6) + (j - 1) * s * (-2); st_up = 1; }
            int sc_left_prev = 0, st_left_prev = 0;   // cell (i-1, j-1) as delivered last step
            if (chunk > 0 && lane == 0) { sc_left_prev = s * (-6) + (j - 2) * s * (-2); st_left_prev = 1; }     // cell (0, j-1)
            const int width = (nn - chunk * 64 < 64) ? nn - chunk * 64 : 64;      // DP columns of this chunk
            for (int tau = 1; tau < m + width - 1; tau++) {
                const int i = tau - lane;
                // values of cell (i, j-1) computed by lane l-1 in the previous step (lane 0 of a later chunk: by the chunk before)
                int sc_l = __shfl_up(sc_up, 1);            // lane l-1's current (i, j-1) sits in its sc_up
                int st_l = __shfl_up(st_up, 1);
                if (WIDE && chunk > 0 && lane == 0 && i < m) { sc_l = edge[i]; st_l = edge[d.cmax + 1 + i]; }
                int sc_new = sc_up, st_new = st_up;
                if (i >= 1 && i < m && j < nn) {
                    const unsigned short* cnt = cntc + (i - 1) * 10;
                    if (j == 0) {
                        int sp = 0;
                        const int y = (i == 1) ? 8 : 9;
#pragma unroll
                        for (int c = 0; c < 10; c++) sp += (int)cnt[c] * dna_score_cls(c, y);
                        sc_new = sc_up + sp;
                        st_new = 3;                       // per-row state, never ins and never uniform-del
                    } else {
                        const int nd = cnt[9];
                        const char c0 = c0c[i - 1];
                        int r1 = 0, r3 = 0;
                        const int y3 = (st_up == 2) ? 9 : 8;
#pragma unroll
                        for (int c = 0; c < 9; c++) {
                            const int k = cnt[c];
                            r1 += k * scb[c];             // diagonal: cell (i-1, j-1)
                            r3 += k * dna_score_cls(c, y3);   // delete: cell (i-1, j)
                        }
                        r1 += nd * (st_left_prev == 1 ? sb_minus : sb_plus) + sc_left_prev;
                        r3 += nd * 3 + sc_up;             // score('-','-')
                        const int r2 = s * (st_l == 1 ? sb_minus : sb_plus) + sc_l;   // insert: cell (i, j-1)
                        unsigned char mv;
                        if (r1 >= r2 && r1 >= r3) { sc_new = r1; st_new = (c0 == '-') ? 1 : 0; mv = 0; }
                        else if (r2 >= r1 && r2 >= r3) { sc_new = r2; st_new = 1; mv = 1; }
                        else { sc_new = r3; st_new = (c0 == '-') ? 0 : 2; mv = 2; }
                        s_mv[(size_t)i * mvs + j] = mv;
                    }
                    if (WIDE && more && lane == 63) { edge[i] = sc_new; edge[d.cmax + 1 + i] = st_new; }     // read 63 steps ago by this chunk's lane 0
                }
                // what lane j-1 held BEFORE this step is cell (i-1, j-1) for the next step
                sc_left_prev = sc_l; st_left_prev = st_l;
                if (i >= 1 && i < m && j < nn) { sc_up = sc_new; st_up = st_new; }
            }
        }
        __syncthreads();
        // ---- traceback, MultipleSequenceAlignmentSP.cpp:252-301 (thread 0)
        if (tid == 0) {
            int x = m - 1, y = nn - 1, cnt = 0;
            int r1 = ncol - 1, r2 = len - 1;
            while (!(x == 0 && y == 0)) {
                int mv;
                if (x == 0) mv = 1; else if (y == 0) mv = 2; else mv = s_mv[(size_t)x * mvs + y];
                if (mv == 0) { s_trace[2 * cnt] = r1; s_trace[2 * cnt + 1] = r2; --r1; --r2; --x; --y; }
                else if (mv == 1) { s_trace[2 * cnt] = -1; s_trace[2 * cnt + 1] = r2; --r2; --y; }
                else { s_trace[2 * cnt] = r1; s_trace[2 * cnt + 1] = -1; --r1; --x; }
                cnt++;
            }
            s_newn = cnt;
        }
        __syncthreads();
        // ---- rebuild columns (reversed traceback order); counts follow incrementally
        const int newn = s_newn;
        char* coln = d.cols[cur ^ 1];
        unsigned short* cntn = s_cnt + (size_t)(cur ^ 1) * CM * 10;
        char* c0n = s_c0 + (size_t)(cur ^ 1) * CM;
        for (long idx = tid; idx < (long)newn * (s + 1); idx += nt) {
            const int c = (int)(idx / (s + 1)), k = (int)(idx % (s + 1));
            const int src = s_trace[2 * (newn - 1 - c)], sj = s_trace[2 * (newn - 1 - c) + 1];
            char ch;
            if (k < s) ch = (src >= 0) ? colc[(long)src * n + k] : '-';
            else ch = (sj >= 0) ? seq[sj] : '-';
            coln[(long)c * n + k] = ch;
        }
        for (int c = tid; c < newn; c += nt) {
            const int src = s_trace[2 * (newn - 1 - c)], sj = s_trace[2 * (newn - 1 - c) + 1];
            const int cl = cls_of((sj >= 0) ? seq[sj] : '-');
            for (int k = 0; k < 10; k++) {
                int v = (src >= 0) ? (int)cntc[src * 10 + k] : (k == 9 ? s : 0);
                if (k == cl) v += 1;
                cntn[c * 10 + k] = (unsigned short)v;
            }
            c0n[c] = (src >= 0) ? c0c[src] : '-';
        }
        if (tid == 0) s_ncol = newn;
        cur ^= 1;
        __syncthreads();
    }
    if (tid == 0) { *d.ncol_out = s_ncol; *d.err_out = s_err | (cur << 8); }
}

// --------------------------------------------------------------------------
// a5: threading of the reads along the backbone (PartialOrderGraph.cpp:94-255,
// the per-base M loop :129-177).  A read base aligned to reference position i
// with symbol c lands in node class (i, c): the backbone node if c is the
// reference base, else the "mis" sibling for that symbol.  The kernels bucket all
// M-aligned bases of a packed read batch into those classes:
//   k_thread_count  one wavefront per read: class sizes, first read of every class
//                   (it creates the sibling), first read of every class-to-class
//                   transition / read start / read end (it adds the edge)
//   k_thread_scan   exclusive scan of the class sizes
//   k_thread_fill   read ids into the class pools
//   k_thread_sort   each pool into read order (the order the reference appends in)
// The host stitches nodes and edges from these tables in first-touch order and
// only walks the reads that contain insertions or deletions (sc_graph.cpp).

template <bool FILL>
__global__ __launch_bounds__(256) void k_thread_walk(ThreadDev d) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = wave; r < d.n_reads; r += nwaves) {
        const int c0 = d.cig_off[r], c1 = d.cig_off[r + 1];
        const int s0 = d.seq_off[r], slen = d.seq_off[r + 1] - s0;
        int i = d.pos[r], j = 0;
        bool prev_m = false;
        for (int k = c0; k < c1; k++) {
            const char op = d.cig_op[k];
            const int len = d.cig_len[k];
            if (op == 'M') {
                if (i + len > d.glen || j + len > slen) { if (lane == 0) atomicOr(d.err, 1); break; }
                for (int t = lane; t < len; t += 64) {
                    const int c = d.lut[(unsigned char)d.seq[s0 + j + t]];
                    const int cls = (i + t) * 8 + c;
                    if (!FILL) {
                        atomicAdd(&d.count[cls], 1);
                        atomicMin(&d.minrid[cls], r);
                        if (t > 0 || prev_m) {
                            const int cp = d.lut[(unsigned char)d.seq[s0 + j + t - 1]];
                            atomicMin(&d.tmin[(i + t) * 64 + cp * 8 + c], r);
                        } else if (k == c0) {
                            atomicMin(&d.smin[cls], r);
                        }
                        if (t == len - 1 && k == c1 - 1) atomicMin(&d.emin[cls], r);
                    } else {
                        const int p = atomicAdd(&d.cursor[cls], 1);
                        d.pool[d.off[cls] + p] = r;
                    }
                }
                i += len; j += len; prev_m = true;
            } else if (op == 'I') { j += len; prev_m = false; }
            else if (op == 'D') { i += len; prev_m = false; }
            else { if (lane == 0) atomicOr(d.err, 2); break; }
        }
    }
}

__global__ __launch_bounds__(1024) void k_thread_scan(const int* __restrict__ count, int* __restrict__ off, int n) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = tid * per, e = min(n, b + per);
    int sum = 0;
    for (int k = b; k < e; k++) sum += count[k];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int k = 0; k < 1024; k++) { const int v = part[k]; part[k] = acc; acc += v; } off[n] = acc; }
    __syncthreads();
    int acc = part[tid];
    for (int k = b; k < e; k++) { off[k] = acc; acc += count[k]; }
}

// every pool into ascending read order (ids are distinct inside a class).  Reads are sorted by
// start position, so the reads of one class span a short id range: a bitmap of that range in LDS
// gives every read its rank with two popcounts.  A class whose reads span more ids than a wavefront's
// bitmap holds (deep coverage: 59 000 reads over every position of configs[3]) goes on the list of
// k_thread_sort_big, which gives it a whole workgroup and a bitmap of half a million ids.  (Until round 3 such a class was
// ranked by comparing every read with every other: 9.3 s of the 19 s of the unthinned configs[3] region.)
constexpr int SORT_WORDS = 512;
__global__ __launch_bounds__(256) void k_thread_sort(const int* __restrict__ off, const int* __restrict__ in, int* __restrict__ out, int ncls,
                                                     int* __restrict__ big) {
    constexpr int WORDS = SORT_WORDS;                // 16 384 ids per wavefront
    __shared__ unsigned bits[4][WORDS];
    __shared__ int wpre[4][WORDS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int c = wave; c < ncls; c += nwaves) {
        const int b = off[c], n = off[c + 1] - b;
        if (n <= 0) continue;
        if (n == 1) { if (lane == 0) out[b] = in[b]; continue; }
        int lo = 0x7fffffff, hi = -1;
        for (int x = lane; x < n; x += 64) { const int v = in[b + x]; lo = min(lo, v); hi = max(hi, v); }
        for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
        if (hi - lo < WORDS * 32) {
            const int nw = ((hi - lo) >> 5) + 1;
            for (int k = lane; k < nw; k += 64) bits[w][k] = 0u;
            __builtin_amdgcn_wave_barrier();
            for (int x = lane; x < n; x += 64) { const int v = in[b + x] - lo; atomicOr(&bits[w][v >> 5], 1u << (v & 31)); }
            __builtin_amdgcn_wave_barrier();
            // exclusive prefix of the word popcounts (nw <= 512: eight words per lane)
            int run = 0;
            for (int k0 = 0; k0 < nw; k0 += 64) {
                const int k = k0 + lane;
                const int pc = (k < nw) ? __popc(bits[w][k]) : 0;
                int incl = pc;
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
                if (k < nw) wpre[w][k] = run + incl - pc;
                run += __shfl(incl, 63);
            }
            __builtin_amdgcn_wave_barrier();
            for (int x = lane; x < n; x += 64) {
                const int rid = in[b + x], v = rid - lo;
                const int rank = wpre[w][v >> 5] + __popc(bits[w][v >> 5] & ((1u << (v & 31)) - 1u));
                out[b + rank] = rid;
            }
            __builtin_amdgcn_wave_barrier();
        } else if (lane == 0) {
            big[1 + atomicAdd(&big[0], 1)] = c;
        }
    }
}

// The wide classes: one workgroup per class and pass over [lo, hi] in stretches of BIG_WORDS * 32 ids -- bits of the
// stretch's reads, exclusive prefix of the word popcounts (sixteen words per thread, then a scan over the threads), every
// read of the stretch to its rank.  Linear in the pool for the ranges that occur (one stretch up to 524 288 ids).
constexpr int BIG_WORDS = 16384;
__global__ __launch_bounds__(1024) void k_thread_sort_big(const int* __restrict__ off, const int* __restrict__ in, int* __restrict__ out,
                                                          const int* __restrict__ big, int words) {
    extern __shared__ unsigned s_big_raw[];
    unsigned* bits = s_big_raw;                                  // [BIG_WORDS]
    int* wpre = reinterpret_cast<int*>(s_big_raw + BIG_WORDS);   // [BIG_WORDS]
    __shared__ int s_part[1024];
    __shared__ int s_lo, s_hi, s_base;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nbig = big[0];
    for (int bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
        const int c = big[1 + bi];
        const int b = off[c], n = off[c + 1] - b;
        if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; s_base = 0; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1;
        for (int x = tid; x < n; x += nt) { const int v = in[b + x]; lo = min(lo, v); hi = max(hi, v); }
        for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
        if ((tid & 63) == 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
        __syncthreads();
        lo = s_lo; hi = s_hi;
        const long span = (long)words * 32;                      // ids per stretch (words <= BIG_WORDS; smaller only in tests)
        for (long c0 = lo; c0 <= hi; c0 += span) {
            const long c1 = c0 + span;                           // this stretch: ids [c0, c1)
            const int nw = (int)(((c1 <= hi ? c1 - 1 : (long)hi) - c0) >> 5) + 1;
            const int base = s_base;                             // reads of the class in the stretches before this one (written after the last barrier of a stretch, read before its first)
            for (int k = tid; k < nw; k += nt) bits[k] = 0u;
            __syncthreads();
            for (int x = tid; x < n; x += nt) {
                const long v = (long)in[b + x] - c0;
                if (v >= 0 && v < span) atomicOr(&bits[v >> 5], 1u << (v & 31));
            }
            __syncthreads();
            // exclusive prefix of the word popcounts: a thread's sixteen words, then the threads
            constexpr int PER = BIG_WORDS / 1024;
            int mine = 0;
#pragma unroll
            for (int j = 0; j < PER; j++) { const int k = tid * PER + j; if (k < nw) mine += __popc(bits[k]); }
            s_part[tid] = mine;
            __syncthreads();
            if (tid < 64) {
                // 1024 partial sums: sixteen per lane of the first wavefront, then across the lanes
                int loc[16], tot = 0;
#pragma unroll
                for (int j = 0; j < 16; j++) { loc[j] = tot; tot += s_part[tid * 16 + j]; }
                int incl = tot;
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (tid >= o) incl += t; }
                const int excl = incl - tot;
#pragma unroll
                for (int j = 0; j < 16; j++) s_part[tid * 16 + j] = excl + loc[j];
            }
            __syncthreads();
            {
                int run = s_part[tid];
#pragma unroll
                for (int j = 0; j < PER; j++) { const int k = tid * PER + j; if (k < nw) { wpre[k] = run; run += __popc(bits[k]); } }
            }
            __syncthreads();
            for (int x = tid; x < n; x += nt) {
                const int rid = in[b + x];
                const long v = (long)rid - c0;
                if (v >= 0 && v < span) out[b + base + wpre[v >> 5] + __popc(bits[v >> 5] & ((1u << (v & 31)) - 1u))] = rid;
            }
            if (tid == nt - 1) { const int k = nw - 1; s_base = base + wpre[k] + __popc(bits[k]); }
            __syncthreads();
        }
    }
}

// host-callable launchers (declared in sc_ctx.hpp; called from sc_sched.cpp, sc_region.cpp, sc_walk.cpp, sc_api.cpp)
void launch_edge_support(hipStream_t st, const int* out_ptr, const int* out_node, const int* pool_ptr, const int* pool_rid,
                         const int* pool_cn, const uint8_t* node_is_end, const int* edge_src, int n_edges, int sorted,
                         int* support) {
    if (n_edges <= 0) return;
    int waves_per_block = 4;
    int blocks = (n_edges + waves_per_block - 1) / waves_per_block;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_edge_support, dim3(blocks), dim3(256), 0, st, out_ptr, out_node, pool_ptr, pool_rid, pool_cn,
                       node_is_end, edge_src, n_edges, sorted, support);
}
int init_graph_kernels() {
    int rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(k_msa<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MSA_LDS);
    rc |= (int)hipFuncSetAttribute(reinterpret_cast<const void*>(k_thread_sort_big), hipFuncAttributeMaxDynamicSharedMemorySize, BIG_WORDS * 8);
    return rc;
}
void launch_msa(hipStream_t st, const MsaDev& d) {
    if (d.cmax > MSA_CM || d.mv_stride > 64) hipLaunchKernelGGL(k_msa<true>, dim3(1), dim3(256), 0, st, d);      // state in HBM scratch
    else hipLaunchKernelGGL(k_msa<false>, dim3(1), dim3(256), MSA_LDS, st, d);
}
// a5 in four launches; `pool_sorted` receives the class pools in read order.
void launch_thread(hipStream_t st, const ThreadDev& d, int* pool_sorted) {
    const int ncls = d.glen * 8;
    int blocks = (d.n_reads + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((k_thread_walk<false>), dim3(blocks), dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_thread_scan, dim3(1), dim3(1024), 0, st, d.count, d.off, ncls);
    hipLaunchKernelGGL((k_thread_walk<true>), dim3(blocks), dim3(256), 0, st, d);
    int sblocks = (ncls + 3) / 4;
    if (sblocks > 2048) sblocks = 2048;
    hipLaunchKernelGGL(k_thread_sort, dim3(sblocks), dim3(256), 0, st, d.off, d.pool, pool_sorted, ncls, d.big);
    // (no class of a region with fewer reads than a wavefront's bitmap has ids can be wide)
    static const int big_words = [] {                          // SC_SORT_BIG_WORDS: a short stretch, so that a test reaches the second one
        const char* e = getenv("SC_SORT_BIG_WORDS");
        const int w = e ? atoi(e) : BIG_WORDS;
        return w < 64 ? 64 : (w > BIG_WORDS ? BIG_WORDS : w);
    }();
    if (d.n_reads > SORT_WORDS * 32)
        hipLaunchKernelGGL(k_thread_sort_big, dim3(512), dim3(1024), BIG_WORDS * 8, st, d.off, d.pool, pool_sorted, d.big, big_words);
}


}  // namespace sc
