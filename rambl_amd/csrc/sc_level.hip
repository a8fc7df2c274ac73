// HIP kernels of one level of the strain walk for gfx950 (MI355X, CDNA4, wave64).
//
//   k_level_sample   one sampler level in one launch: rows of new strains, read
//                    log-likelihood update (a13), draw slots and weight rows, and
//                    the Polya-urn chain (a14, np_bayes_clustering; also a18,
//                    read_assign; sc_sampler.hpp)
//   k_level          one level without the sampler: the update (a13) and the soft
//                    update (a15, hard_clustering)
//   k_level_any / k_level_resident   a batch of levels of any kind / the resident level workers
//   k_level_copy/update/entries/rows, k_hard_*   the pieces of a level on a grid, in front of its workgroup: of a very
//                    large level, or of any level of a context that walks a single region (launch_level)
//
// These are integer / fp32 / fp64 loops bound by latency or HBM: no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "sc_device.hpp"
#include "sc_sampler.hpp"

namespace sc {

constexpr int LDS_TOTAL = 160 * 1024 - 256;   // dynamic part; the rest covers small static __shared__ variables
constexpr int LDS_SMALL = 18 * 1024;           // per-strain scalars (LevelLds)
constexpr int LDS_BIG = LDS_TOTAL - LDS_SMALL;
static_assert(LDS_SMALL >= (int)(sizeof(double) * 2 * MAXS + sizeof(StrainParam) * MAXS + sizeof(unsigned) * MAXS * KMAX + sizeof(int) * 6 * MAXS + 64), "LDS_SMALL");
static_assert(LDS_BIG >= (int)(sizeof(double) * MAXS * 64), "LDS_BIG");    // every level with <= 8 symbols stages its log tables in LDS

// --------------------------------------------------------------------------
// The pieces of one level of the walk (NonparametricClustering.cpp:284-458) that every mode shares.  They
// run inside the level's single workgroup (k_level_sample / k_level); for levels with hundreds of thousands
// of (strain, read) items, or in a context whose only region leaves the other CUs idle, the host runs them on a grid
// in front (k_level_copy, k_level_update, k_level_entries, k_level_rows) and says so in LevelHdr::done.
// LV_TICKED: the first of them has left its tick in JobBlock::t0 (the level's kernel follows on the same stream).
enum { LV_COPIES_DONE = 1, LV_ITEMS_DONE = 2, LV_HAS_DONE = 4, LV_HARD_DONE = 8, LV_SLOTS_DONE = 16, LV_ROWS_DONE = 32, LV_TICKED = 64 };
// The region's arrays as the batched level kernels see them: a block of device memory that does not change while the
// region is walked, read through the constant address space -- scalar loads the compiler may repeat at will, exactly
// like kernel arguments (which hold only a pointer to it: LevelItem).
typedef const __attribute__((address_space(4))) JobDev KJob;

// The per-strain parameters of the level, straight from host-mapped memory into LDS: 16-byte loads over PCIe,
// every thread a few, one round trip.
__device__ __forceinline__ void stage_params(const LevelHdr& h, const LevelParams* __restrict__ P, StrainParam* s_sp, int* s_copy,
                                             double* s_lpt, bool want_lpt, int K2, int tid, int nt) {
    const i4v* src_sp = reinterpret_cast<const i4v*>(P->sp);
    i4v* dst_sp = reinterpret_cast<i4v*>(s_sp);
    for (int i = tid; i < h.S * 2; i += nt) dst_sp[i] = src_sp[i];
    for (int i = tid; i < h.n_copy; i += nt) { s_copy[i] = P->copy_src[i]; s_copy[MAXS + i] = P->copy_dst[i]; }
    if (want_lpt) {
        const double2* s = reinterpret_cast<const double2*>(P->lpt);
        double2* d = reinterpret_cast<double2*>(s_lpt);
        for (int i = tid; i < (h.S * K2 + 1) / 2; i += nt) d[i] = s[i];
    }
}

// phase 0 inside the workgroup
template <class JD>
__device__ __forceinline__ void phase_copies(const JD& job, const LevelHdr& h, const int* s_copy, int tid, int nt) {
    const long stride = job.ll_stride;
    for (int c = 0; c < ((h.done & LV_COPIES_DONE) ? 0 : h.n_copy); c++) {
        const double2* src = reinterpret_cast<const double2*>(job.ll + (long)s_copy[c] * stride);
        double2* dst = reinterpret_cast<double2*>(job.ll + (long)s_copy[MAXS + c] * stride);
        const int n2 = ((h.copy_n < job.n_reads ? h.copy_n : job.n_reads) + 1) >> 1;      // cells past copy_n hold nothing yet
        int i = tid;
        for (; i + 3 * nt < n2; i += 4 * nt) {        // four independent 16-byte loads in flight per thread
            const double2 v0 = src[i], v1 = src[i + nt], v2 = src[i + 2 * nt], v3 = src[i + 3 * nt];
            dst[i] = v0; dst[i + nt] = v1; dst[i + 2 * nt] = v2; dst[i + 3 * nt] = v3;
        }
        for (; i < n2; i += nt) dst[i] = src[i];
    }
    // the copies are independent (a destination is a free row, a source a surviving parent's row): one barrier for all
    __syncthreads();
}

// The loops below that the grid kernels share take a first index and a step: tid, nt inside the level's workgroup, the
// global index and the size of the grid in k_level_entries / k_level_rows / k_hard_*.

// the level's reads are present in read_loglik from here on
template <class JD>
__device__ __forceinline__ void mark_present(const JD& job, const LevelHdr& h, int first, int step) {
    const int e0 = h.e0, Rn = h.e1 - h.e0;
    for (int r = first; r < Rn; r += step) job.has[job.ent_rid[e0 + r]] = 1;
}

// phase 1: read log-likelihood update, NonparametricClustering.cpp:343-391, then the reads of the level are
// present in read_loglik (`has`).  s_lpt: the strains' log tables in LDS.
template <class JD>
__device__ __forceinline__ void phase_update(const JD& job, const LevelHdr& h, const StrainParam* s_sp, const int* s_lab,
                                             const double* s_lpt, int tid, int nt) {
    const int S = h.S, K = job.K, K2 = K * K, e0 = h.e0, Rn = h.e1 - h.e0;
    const long stride = job.ll_stride;
    const bool plain_labels = !h.has_dups && !h.any_multi && !(h.done & LV_ITEMS_DONE);
    if (!plain_labels && !(h.done & LV_ITEMS_DONE)) {           // (k_level_update has written isnew with its items)
        // (the walk over multi-symbol labels below and in the soft update reads this; the usual level finds it on the way)
        for (int r = tid; r < Rn; r += nt) {
            const int e = e0 + r;
            job.isnew[r] = (job.ent_first[e] && !job.has[job.ent_rid[e]]) ? 1 : 0;
        }
        __syncthreads();
    }
    const int codeN = job.code_N;
    auto item = [&](int s, int r) {
        const int e = e0 + r;
        const int rid = job.ent_rid[e];
        const uint8_t* sb = job.labels + s_sp[s].lab_off;
        const uint8_t* rb = job.labels + job.ent_lab_off[e];
        const int ls = s_sp[s].lab_len, lr = job.ent_lab_len[e];
        const double* lp = s_lpt + s * K2;
        double val;
        if (ls == 1) {
            int a = sb[0], b = rb[0];
            if (lr == 1) {
                if (a == codeN) a = b;
                val = (a < K && b < K) ? lp[a * K + b] : __longlong_as_double(0x7ff8000000000000ll);
            } else {
                // logprob(sb, "multi"): sub_count[(sb, rb)] is created as 0 (std::map operator[]), so the
                // result is log 0 - log comp(sb) = -inf for a symbol of the alphabet; for N (sb becomes rb)
                // or a symbol outside the alphabet comp is created as 0 too: -inf - -inf
                val = (a < 6 && a != codeN) ? -INFINITY : __longlong_as_double(0x7ff8000000000000ll);
            }
        } else {
            val = 0.0;
            if (job.isnew[r]) {
                int ii = ls, jj = lr;
                while (ii > 0 && jj > 0) {
                    int a = sb[--ii], b = rb[--jj];
                    if (a == codeN) a = b;
                    val += lp[a * K + b];
                }
            } else {
                int ii = 0, jj = 0;
                while (ii < ls && jj < lr) {
                    int a = sb[ii++], b = rb[jj++];
                    if (a == codeN) a = b;
                    val += lp[a * K + b];
                }
            }
        }
        double* cell = job.ll + (long)s_sp[s].slot * stride + rid;
        const bool fresh = job.ent_first[e] && !job.has[rid];
        *cell = fresh ? val : (*cell + val);            // Strain::update_read_loglik, Strain.cpp:85-95
    };
    if (h.done & LV_ITEMS_DONE) {
        // k_level_update has applied the items
    } else if (!h.has_dups && !h.any_multi) {
        // single-symbol labels everywhere (the usual level): a thread takes a read of the level and walks the strains
        // eight at a time, so eight independent row cells are in flight per thread and neighbouring threads (reads
        // sorted by position: neighbouring ids) touch neighbouring cells of each row
        // An item is (sixteen strains, read): sixteen independent row cells in flight per thread, the items of a chunk of
        // strains on neighbouring threads (so that a level of 600 reads x 30 strains is three rounds of the workgroup, not
        // two rounds of reads x four chunks one after the other).
        constexpr int U = 16;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        const int nch = (S + U - 1) / U;
        const int items = Rn * nch;
        for (int idx = tid; idx < items; idx += nt) {
            const int ch = idx / Rn, r = idx - ch * Rn;
            const int e = e0 + r;
            const int rid = job.ent_rid[e];
            const int b = job.labels[job.ent_lab_off[e]];
            const bool fresh = job.ent_first[e] && !job.has[rid];
            if (ch == 0) job.isnew[r] = fresh ? 1 : 0;
            const int s0 = ch * U;
            long off[U];                                        // (no early exit from the unrolled loops: the arrays stay in registers)
            double old[U];
#pragma unroll
            for (int k = 0; k < U; k++) {
                const int sx = (s0 + k < S) ? s0 + k : S - 1;
                off[k] = (long)s_sp[sx].slot * stride + rid;
                old[k] = fresh ? 0.0 : job.ll[off[k]];
            }
#pragma unroll
            for (int k = 0; k < U; k++) {
                const int sx = s0 + k;
                if (sx < S) {
                    int a = s_lab[sx];
                    if (a == codeN) a = b;
                    const double val = (a < K && b < K) ? s_lpt[sx * K2 + a * K + b] : qnan;
                    job.ll[off[k]] = fresh ? val : (old[k] + val);       // Strain::update_read_loglik, Strain.cpp:85-95
                }
            }
        }
    } else if (!h.has_dups) {
        const long total = (long)S * Rn;
        for (long idx = tid; idx < total; idx += nt) item((int)(idx / Rn), (int)(idx % Rn));
    } else {
        if (tid < S) for (int r = 0; r < Rn; r++) item(tid, r);
    }
    if (h.done & LV_HAS_DONE) { __syncthreads(); return; }      // (k_level_entries, behind the grid's update; the barrier is the phase's)
    __syncthreads();
    mark_present(job, h, tid, nt);
    __syncthreads();
}

// phase 2: draw slots q = (entry, copy); the reference walks copies from cn down to 1 (:161-167)
template <bool BARRIER = true, class JD>
__device__ __forceinline__ void phase_slots(const JD& job, const LevelHdr& h, int tid, int nt) {
    const int e0 = h.e0, Rn = h.e1 - h.e0;
    for (int r = tid; r < Rn; r += nt) {
        const int e = e0 + r;
        const int rid = job.ent_rid[e], cn = job.ent_cn[e];
        const int qb = job.ent_qoff[e];
        const int mb = job.mate_ptr[rid], mn = job.mate_ptr[rid + 1] - mb;
        const uint8_t code = (job.ent_lab_len[e] == 1) ? job.labels[job.ent_lab_off[e]] : (uint8_t)0xFF;
        for (int i = 0; i < cn; i++) {
            const int k = cn - 1 - i;
            const int uid = (k < mn) ? job.mate_idx[mb + k] : -1;
            job.qent[qb + i] = r;
            job.qrid[qb + i] = rid;
            job.quid[qb + i] = uid;
            job.qcode[qb + i] = code;
        }
    }
    if (BARRIER) __syncthreads();
}

// every result of the level is in host memory before the stamp
__device__ __forceinline__ void finish_level(const LevelHdr& h, LevelResult* __restrict__ R, unsigned long long wall0, int tid) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        R->level_wall = wall_clock64() - wall0;
        R->xcc = (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 0xF);      // HW_REG_XCC_ID[3:0]
        __hip_atomic_store(&R->seq, h.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// --------------------------------------------------------------------------
// The pieces of hard_clustering (NonparametricClustering.cpp:17-125) that the level's workgroup (level_plain_body) and
// the grid (k_hard_*) both run.

// logprob(uid) inserts a zero log-likelihood for a mate not seen yet (Strain.cpp:147-150).  slot_of(s): the strain's row,
// out of LDS.
template <class JD, class SL>
__device__ __forceinline__ void zero_unseen_mates(const JD& job, const LevelHdr& h, SL slot_of, int first, int step) {
    const long stride = job.ll_stride;
    for (int q = first; q < h.Q; q += step) {
        const int uid = job.quid[q];
        if (uid >= 0 && !job.has[uid])
            for (int s = 0; s < h.S; s++) job.ll[(long)slot_of(s) * stride + uid] = 0.0;
    }
}

// One draw slot's column of tabA, x_s at col[s * cs] with maximum m, becomes p_s = exp(x_s - m) / sum_s exp(x_s - m), the
// sum taken over the strains in order.
__device__ __forceinline__ void normalise_column(double* col, long cs, int S, double m) {
    double norm = 0;
    for (int s = 0; s < S; s++) norm += exp(col[(long)s * cs] - m);
    for (int s = 0; s < S; s++) {
        double* cell = col + (long)s * cs;
        *cell = exp(*cell - m) / norm;
    }
}

// One strain's sums of responsibilities on one wavefront: lane j adds the slots j, j + 64, ... (in slot order), per read
// symbol (acc[b]) and over all of them (acc[KMAX]), then the 64 partial sums are joined by a tree of fixed shape; the sums
// are lane 0's.  The reference adds them one after the other in long double; any fixed order of fp64 additions is as close
// to that as another (1e-13 relative, the tests allow 1e-9), and two candidates with equal inputs still get bitwise equal
// sums, which is what their ties rest on.
__device__ __forceinline__ void strain_sums(const double* prow, const uint8_t* qcode, int Q, int lane, double (&acc)[KMAX + 1]) {
#pragma unroll
    for (int b = 0; b <= KMAX; b++) acc[b] = 0.0;
    for (int q = lane; q < Q; q += 64) {
        const double p = prow[q];
        const int code = qcode[q];
        acc[KMAX] += p;
#pragma unroll
        for (int b = 0; b < KMAX; b++) acc[b] += (code == b) ? p : 0.0;
    }
#pragma unroll
    for (int b = 0; b <= KMAX; b++) {
        double v = acc[b];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        acc[b] = v;
    }
}

// phase 3: what the sampler draws from.  Per draw slot q the fp32 weight row L[q][s] = exp(x_s - max_s x_s),
// x_s = ll(read) + ll(mate) in fp64, zeros behind it up to the stride, and 16 zeros behind the last row.  A slot whose
// log-likelihoods lie in the underflow range of the reference's exp() gets a NaN row, which sends its draws to the
// checked tiers.  put4(index, four floats) stores them: into LDS or tabLf inside the workgroup, into tabLf on the grid
// (k_level_rows).  s_slot: the strains' rows, in LDS.
//
// A lane takes a draw slot q and walks the strains: the 64 slots of a wavefront are neighbouring reads (slots follow
// the level's entries, entries the read ids), so one load instruction -- one strain's row at 64 nearby read ids --
// touches a dozen cache lines instead of 64.  (A lane used to take eight strains of one slot: every 8-byte cell came
// with its own 128-byte line from the L2, 3.3 MB per level of 860 read copies x 30 strains at the 64 bytes a clock a
// compute unit gets -- 25 us, the longest part of a level outside the chain.)  Up to 32 strains the cells stay in
// registers between the maximum and the exponentials; beyond, they are read a second time (from the L1 / L2).
// The rules of a row, stated once for the one-lane walk below and the lanes of a group in k_level_rows:
// the cell x_s of a draw slot (the read's and its mate's log-likelihood, each only when present in read_loglik), ...
struct SlotCells {
    const double* ll; long lstride; int rid, uid; bool hr, hu;
    __device__ __forceinline__ double operator()(int row) const {
        const double* r = ll + (long)row * lstride;
        double v = hr ? r[rid] : 0.0;
        if (hu) v += r[uid];
        return v;
    }
};
template <class JD>
__device__ __forceinline__ SlotCells slot_cells(const JD& job, const LevelHdr& h, int rid, int uid) {
    const bool hr = h.do_update ? true : job.has[rid] != 0;      // the update has just entered the level's reads
    const bool hu = uid >= 0 && job.has[uid] != 0;
    return SlotCells{job.ll, job.ll_stride, rid, uid, hr, hu};
}
// ... the slot whose maximum m lies in the underflow range of the reference's exp() (also NaN / -inf), ...
__device__ __forceinline__ bool row_flagged(double m) { return !(m >= -600.0); }
// ... four neighbouring floats of its row from strain s0 on, out of the cells x[0..3]: weights (NaN when flagged) of the
// strains below S, zeros behind them, ...
__device__ __forceinline__ f4v row_block(const double* x, int s0, int S, double m, bool flag) {
    const float qnanf = __int_as_float(0x7fc00000);
    f4v w;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float wk = s0 + k < S ? (flag ? qnanf : exp_weight(x[k] - m)) : 0.0f;
        if (k == 0) w.x = wk; else if (k == 1) w.y = wk; else if (k == 2) w.z = wk; else w.w = wk;
    }
    return w;
}
// ... and the 16 zeros at `end`, behind the last row: the chain reads whole 16-strain blocks, what follows stays finite.
template <class PUT>
__device__ __forceinline__ void row_tail(PUT put4, long end, int first, int step) {
    for (int i = first; i < 4; i += step) put4(end + 4 * i, f4v{0.0f, 0.0f, 0.0f, 0.0f});
}

template <int NB, class JD, class PUT>
__device__ __forceinline__ void weight_rows(const JD& job, const LevelHdr& h, const int* s_slot, PUT put4, int first, int step) {
    constexpr int SR = (NB <= 2) ? 16 * NB : 16;           // cells held per lane
    const int S = h.S, Q = h.Q, e0 = h.e0;
    const int stride = chain_w_stride(S);
    for (int q = first; q < Q; q += step) {
        const SlotCells cells = slot_cells(job, h, job.ent_rid[e0 + job.qent[q]], job.quid[q]);
        const long Lf = (long)q * stride;
        auto cell = [&](int sx) __attribute__((always_inline)) -> double { return cells(s_slot[sx]); };
        double m = -INFINITY;
        double x[SR];
        if (NB <= 2) {
#pragma unroll
            for (int i = 0; i < SR; i++) { x[i] = -INFINITY; if (i < S) { x[i] = cell(i); m = fmax(m, x[i]); } }
        } else {
            for (int s0 = 0; s0 < S; s0 += SR) {
#pragma unroll
                for (int i = 0; i < SR; i++) if (s0 + i < S) m = fmax(m, cell(s0 + i));
            }
        }
        const bool flag = row_flagged(m);
        // the row: S weights, zeros up to the stride (a multiple of four floats)
        for (int s0 = 0; s0 < stride; s0 += SR) {
            if (NB > 2) {
#pragma unroll
                for (int i = 0; i < SR; i++) x[i] = (s0 + i < S) ? cell(s0 + i) : -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < SR; i += 4)
                if (s0 + i < stride) put4(Lf + s0 + i, row_block(x + i, s0 + i, S, m, flag));
        }
        if (q == Q - 1) row_tail(put4, Lf + stride, 0, 1);
    }
}

// LDS of the level kernels: per-strain scalars first, then one big region that holds the strains' log tables
// during the update and the sampler's uniforms + weight rows (or the soft update's histogram) afterwards.
struct LevelLds {
    double* s_a; double* s_p; unsigned* s_cnt; int* s_slot; unsigned* s_kf; float* s_a0f; int* s_x; int* s_copy; int* s_lab;
    StrainParam* s_sp; unsigned char* s_big;
};
__device__ __forceinline__ LevelLds level_lds(unsigned char* raw) {
    LevelLds l;
    l.s_a = reinterpret_cast<double*>(raw);                        // [MAXS]
    l.s_p = l.s_a + MAXS;                                          // [MAXS]
    l.s_sp = reinterpret_cast<StrainParam*>(l.s_p + MAXS);         // [MAXS]
    l.s_cnt = reinterpret_cast<unsigned*>(l.s_sp + MAXS);          // [KMAX*MAXS], log_cnt_index
    l.s_slot = reinterpret_cast<int*>(l.s_cnt + MAXS * KMAX);      // [MAXS]
    l.s_kf = reinterpret_cast<unsigned*>(l.s_slot + MAXS);         // [MAXS] draws per strain so far
    l.s_a0f = reinterpret_cast<float*>(l.s_kf + MAXS);             // [MAXS] fp32 copy of the starting weights
    l.s_copy = reinterpret_cast<int*>(l.s_a0f + MAXS);             // [2*MAXS]
    l.s_lab = l.s_copy + 2 * MAXS;                                 // [MAXS] first symbol of the strain's node label
    l.s_x = l.s_lab + MAXS;                                        // [8] first failing position per wave
    l.s_big = raw + LDS_SMALL;
    return l;
}

// --------------------------------------------------------------------------
// a13 + a14 / a18: one sampler level in ONE launch -- np_bayes_clustering
// (NonparametricClustering.cpp:128-244) on the level's reads, and read_assign
// (:776-836) on the pseudo-level of all reads.  One workgroup: the per-strain
// parameters arrive from host-mapped memory, new strains get their rows, the
// level's read log-likelihoods are updated (a13), the draw slots and the fp32
// weight rows L[q][s] = exp(ll - max_s ll) are built straight into LDS (HBM when
// they do not fit), then four or eight wavefronts run the urn chain
// (urn_chain_q) and the results go to host-mapped memory, stamped.
// NB = ceil(S / 16): every lane of a quad owns 4 * NB consecutive strains.
constexpr int CHAINW_ROWS_BYTES = LDS_BIG - UWIN * 4;
constexpr int CHAIN_THREADS = 512;   // eight wavefronts build the level
// the level's scalars out of an item, whatever address space the item is read through (field by field: a struct in the
// constant address space has no copy constructor)
template <class IT>
__device__ __forceinline__ LevelHdr load_hdr(const IT& it) {
    LevelHdr h;
    h.mode = it.h.mode; h.S = it.h.S; h.e0 = it.h.e0; h.e1 = it.h.e1; h.has_dups = it.h.has_dups; h.any_multi = it.h.any_multi;
    h.Q = it.h.Q; h.n_sweeps = it.h.n_sweeps; h.n_copy = it.h.n_copy; h.do_update = it.h.do_update; h.done = it.h.done;
    h.copy_n = it.h.copy_n; h.seq = it.h.seq;
    return h;
}
// What both bodies begin with: the level's scalars out of the item, the per-strain parameters into LDS (the log tables
// into the big region where the body's own update will read them), the result block reset, the first tick.
// The level began with its first kernel: a grid kernel in front on the same stream has left its tick behind the region's
// JobDev.  (Not so for the grid kernels of a context with several regions: a host round trip and the hand-over to the
// level server or a resident worker lie between them and this kernel, which is no time the GPU spent on the level.)
template <class IT>
__device__ __forceinline__ unsigned long long level_wall0(const IT& it) {
    return (it.h.done & LV_TICKED) ? reinterpret_cast<const JobBlock*>(it.job)->t0 : wall_clock64();
}
template <class IT>
__device__ __forceinline__ LevelHdr begin_level(const IT& it, const LevelLds& l, unsigned long long wall0, int tid, int nt) {
    const LevelHdr h = load_hdr(it);
    KJob& job = *(KJob*)it.job;
    LevelResult* __restrict__ R = it.R;
    const bool upd = h.do_update && h.e1 > h.e0;
    stage_params(h, it.P, l.s_sp, l.s_copy, reinterpret_cast<double*>(l.s_big), upd && !(h.done & LV_ITEMS_DONE), job.K * job.K, tid, nt);
    if (tid == 0) { R->error = 0; R->n_draws = 0; R->n_exact = 0; R->n_slow = 0; R->n_pass = 0; R->chain_cycles = 0; R->chain_wall = 0; }
    __syncthreads();
    if (tid == 0) R->phase_ticks[0] = (unsigned)(wall_clock64() - wall0);
    return h;
}
template <int NB, bool ROWS_LDS, bool STAY, class IT>
__device__ __forceinline__ void level_sample_body(const IT& it, unsigned char* s_raw) {
    const unsigned long long wall0 = level_wall0(it);
    KJob& job = *(KJob*)it.job;
    LevelResult* __restrict__ R = it.R;
    const LevelLds l = level_lds(s_raw);
    float* s_uwin = reinterpret_cast<float*>(l.s_big);           // [UWIN]
    float* s_rows = s_uwin + UWIN;
    const int tid = threadIdx.x;
    int nt = blockDim.x;
    const LevelHdr h = begin_level(it, l, wall0, tid, nt);
    const int S = h.S, Q = h.Q, Rn = h.e1 - h.e0;
    const int stride = chain_w_stride(S);
    const bool upd = h.do_update && Rn > 0;
    for (int i = tid; i < MAXS * KMAX; i += nt) l.s_cnt[i] = 0;
    if (tid < MAXS) {
        l.s_slot[tid] = tid < S ? l.s_sp[tid].slot : 0;
        l.s_kf[tid] = 0u;
        l.s_a0f[tid] = tid < S ? (float)l.s_sp[tid].a0 : 0.0f;
        l.s_lab[tid] = tid < S ? (int)job.labels[l.s_sp[tid].lab_off] : 0;
    }
    phase_copies(job, h, l.s_copy, tid, nt);
    if (tid == 0) R->phase_ticks[1] = (unsigned)(wall_clock64() - wall0);
    // the draw slots depend on the level's entries alone: their loads and stores go out in front of the update's, and
    // the update's closing barriers cover them (phase_ticks[3] - [2] is therefore ~0 on a level with an update)
    const bool slots = !(h.done & LV_SLOTS_DONE);            // (else k_level_entries has written them)
    if (upd) {
        if (slots) phase_slots<false>(job, h, tid, nt);
        phase_update(job, h, l.s_sp, l.s_lab, reinterpret_cast<const double*>(l.s_big), tid, nt);
    }
    if (tid == 0) R->phase_ticks[2] = (unsigned)(wall_clock64() - wall0);
    if (!upd && slots) phase_slots(job, h, tid, nt);
    if (tid == 0) R->phase_ticks[3] = (unsigned)(wall_clock64() - wall0);

    if (!(h.done & LV_ROWS_DONE)) {
        SC_GLOBAL float* rows_g = (SC_GLOBAL float*)job.tabLf;
        weight_rows<NB>(job, h, l.s_slot, [&](long idx, f4v v) __attribute__((always_inline)) {
            if (ROWS_LDS) *(f4v*)(s_rows + idx) = v; else *(SC_GLOBAL f4v*)(rows_g + idx) = v;
        }, tid, nt);
    } else if (ROWS_LDS) {
        // k_level_rows has built them in tabLf: Q rows and the 16 zeros behind the last, 16 bytes a load
        const f4v* src = reinterpret_cast<const f4v*>(job.tabLf);
        f4v* dst = reinterpret_cast<f4v*>(s_rows);
        const int n4 = (Q * stride + 16) >> 2;
        for (int i = tid; i < n4; i += nt) dst[i] = src[i];
    }
    __syncthreads();
    if (tid == 0) R->phase_ticks[4] = (unsigned)(wall_clock64() - wall0);
    constexpr int NW = chain_nw(NB);
    if (tid >= 64 * NW) {
        if (!STAY) return;                                 // a finished wavefront no longer counts at the barriers below
        urn_chain_shadow<NW>(h, l.s_x);                    // ... one that has to stay takes part in them
    } else {
        auto chain = [&](auto wide_q) __attribute__((always_inline)) {
            urn_chain_q<NB, ROWS_LDS, NW, decltype(wide_q)::value>(job, h, l.s_sp, R, l.s_slot, l.s_a, l.s_p, l.s_kf, l.s_a0f, l.s_x, s_uwin, s_rows, stride, tid);
        };
        if (Q >= 16 * NW) chain(std::true_type{}); else chain(std::false_type{});     // (uniform: one of two instances of the same pass loop)
    }
    if (!STAY) nt = 64 * NW;
    draw_log_counts(job, h, l.s_cnt, tid, nt);               // (behind the chain's closing barrier, by every wavefront still here)
    __syncthreads();
    if (tid == 0) R->phase_ticks[5] = (unsigned)(wall_clock64() - wall0);      // the count's end: what follows is stores, fence and stamp
    for (int i = tid; i < S * KMAX; i += nt) R->cnt[i] = l.s_cnt[log_cnt_index(i / KMAX, i % KMAX)];
    finish_level(h, R, wall0, tid);
}

// --------------------------------------------------------------------------
// a13 + a15: one level without the sampler in one launch -- the read log-likelihood update, and for MODE_HARD
// the soft update hard_clustering (NonparametricClustering.cpp:17-125).  Single workgroup.
template <class IT>
__device__ __forceinline__ void level_plain_body(const IT& it, unsigned char* s_raw) {
    const unsigned long long wall0 = level_wall0(it);
    KJob& job = *(KJob*)it.job;
    LevelResult* __restrict__ R = it.R;
    const LevelLds l = level_lds(s_raw);
    double* s_tab = reinterpret_cast<double*>(l.s_big);          //   [S][K][K] log tables, later the substitution histogram
    const int tid = threadIdx.x, nt = blockDim.x;
    const LevelHdr h = begin_level(it, l, wall0, tid, nt);
    const int S = h.S, K = job.K, K2 = K * K, e0 = h.e0, Rn = h.e1 - h.e0;
    const long stride = job.ll_stride;
    const bool upd = h.do_update && Rn > 0;
    if (tid < S) l.s_lab[tid] = (int)job.labels[l.s_sp[tid].lab_off];
    phase_copies(job, h, l.s_copy, tid, nt);
    if (tid == 0) R->phase_ticks[1] = (unsigned)(wall_clock64() - wall0);
    if (upd) phase_update(job, h, l.s_sp, l.s_lab, s_tab, tid, nt);
    if (tid == 0) R->phase_ticks[2] = (unsigned)(wall_clock64() - wall0);
    if (Rn <= 0 || S <= 0 || h.mode != MODE_HARD || (h.done & LV_HARD_DONE)) { finish_level(h, R, wall0, tid); return; }
    phase_slots(job, h, tid, nt);
    if (tid == 0) R->phase_ticks[3] = (unsigned)(wall_clock64() - wall0);

    // hard_clustering, NonparametricClustering.cpp:17-125
    const int Q = h.Q;
    zero_unseen_mates(job, h, [&](int s) { return l.s_sp[s].slot; }, tid, nt);
    __syncthreads();
    for (int q = tid; q < Q; q += nt) { const int uid = job.quid[q]; if (uid >= 0) job.has[uid] = 1; }
    __syncthreads();
    // x[s][q] = log prior + ll(read) + ll(mate): one (strain, slot) pair per thread and step, so the scattered
    // row reads of a slot's strains are all in flight together
    for (long idx = tid; idx < (long)S * Q; idx += nt) {
        const int s = (int)(idx / Q), q = (int)(idx % Q);
        const int rid = job.qrid[q], uid = job.quid[q];         // (qrid: ent_rid of the slot's entry, one dependent load less)
        const double* row = job.ll + (long)l.s_sp[s].slot * stride;
        double x = l.s_sp[s].logpri + row[rid];
        if (uid >= 0) x += row[uid];
        job.tabA[(long)s * job.qcap + q] = x;
    }
    __syncthreads();
    for (int q = tid; q < Q; q += nt) {
        // p_s = exp(x_s) / sum_s exp(x_s) (:186-192).  The reference forms it in long double, where
        // exp(-800) is an ordinary number (a read laid against a long collapsed node it does not match
        // reaches such log-likelihoods for every strain); in fp64 the same quotient needs the maximum
        // taken out first.  A NaN x_s still makes every p NaN, as in the reference.
        double* col = job.tabA + q;
        double m = -INFINITY;
        for (int s = 0; s < S; s++) m = fmax(m, col[(long)s * job.qcap]);
        normalise_column(col, job.qcap, S, m);
    }
    for (int i = tid; i < S * K2; i += nt) s_tab[i] = 0.0;
    __syncthreads();
    if (tid == 0) R->phase_ticks[4] = (unsigned)(wall_clock64() - wall0);
    if (!h.any_multi) {
        // one wavefront per strain (strain_sums)
        const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
        for (int s = wv; s < S; s += nw) {
            double acc[KMAX + 1];
            strain_sums(job.tabA + (long)s * job.qcap, job.qcode, Q, lane, acc);
            if (lane == 0) {
                R->abund[s] = acc[KMAX];
                const int a = l.s_lab[s];
                if (a < K)
                    for (int b = 0; b < K; b++) s_tab[s * K2 + a * K + b] = acc[b];
            }
        }
    } else {
        if (tid < S) {
            const int s = tid;
            const double* prow = job.tabA + (long)s * job.qcap;
            double* hist = s_tab + s * K2;
            const uint8_t* sb = job.labels + l.s_sp[s].lab_off;
            const int ls = l.s_sp[s].lab_len;
            double acc = 0;
            // a strain on "^" or "$" carries the code 0xFF, which is no row of the histogram (the one-wavefront path and
            // k_hard_sums drop it the same way; the host reads the rows below K alone)
            auto add = [&](int a, int b, double p) __attribute__((always_inline)) { if (a < K && b < K) hist[a * K + b] += p; };
            for (int q = 0; q < Q; q++) {
                const double p = prow[q];
                acc += p;
                const int r = job.qent[q], e = e0 + r;
                const uint8_t* rb = job.labels + job.ent_lab_off[e];
                const int lr = job.ent_lab_len[e];
                if (lr == 1) {
                    if (ls == 1) add(sb[0], rb[0], p);
                } else if (job.isnew[r]) {
                    int i = ls, j = lr;
                    while (i > 0 && j > 0) { const int a = sb[--i], b = rb[--j]; add(a, b, p); }
                } else {
                    int i = 0, j = 0;
                    while (i < ls && j < lr) { const int a = sb[i++], b = rb[j++]; add(a, b, p); }
                }
            }
            R->abund[s] = acc;
        }
    }
    __syncthreads();
    for (int i = tid; i < S * K2; i += nt) R->subst[i] = s_tab[i];
    finish_level(h, R, wall0, tid);
}

// One kernel per kind of level (a single region in flight launches its levels directly) ...
template <int NB, bool ROWS_LDS>
__global__ __launch_bounds__(CHAIN_THREADS) void k_level_sample(LevelBatch batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    level_sample_body<NB, ROWS_LDS, false>(batch.it[blockIdx.x], s_raw);
}
__global__ __launch_bounds__(512) void k_level(LevelBatch batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    level_plain_body(batch.it[blockIdx.x], s_raw);
}
// ... and one kernel for a batch of levels of ANY kind (many regions in flight: with one kind per launch, and a
// stream held until its batch is done, the five or so kinds that wait at any time take turns for the free streams;
// tools/launch_policy_sim.py).  Workgroup b looks at the kind of its item and calls the variant: the variants are
// functions of their own (`noinline`: each keeps its own register allocation -- merged into one body they spilled
// 56 scalars into the sampler's pass loop), reading the item through the constant address space like kernel arguments.
typedef const __attribute__((address_space(4))) LevelItem KItem;
template <int NB, bool ROWS_LDS>
__device__ __noinline__ void level_sample_call(const LevelItem* it) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    level_sample_body<NB, ROWS_LDS, true>(*it, s_raw);      // every wavefront stays to the end (shared with the resident workgroups)
}
__device__ __noinline__ void level_plain_call(const LevelItem* it) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    level_plain_body(*it, s_raw);
}
__device__ __forceinline__ void level_dispatch(const LevelItem* it) {
    const int kind = item_kind(it->kind);
    if (!kind_has_sampler(kind)) { level_plain_call(it); return; }
    with_sampler_variant(kind, [&](auto nb, auto rows_lds) { level_sample_call<decltype(nb)::value, decltype(rows_lds)::value>(it); });
}
__global__ __launch_bounds__(CHAIN_THREADS) void k_level_any(LevelBatch batch) {
    __shared__ LevelItem s_item;                                                  // the variants read their item through a generic pointer
    KItem* it = (KItem*)__builtin_amdgcn_kernarg_segment_ptr() + blockIdx.x;      // batch is the only argument
    if (threadIdx.x < sizeof(LevelItem) / 4) reinterpret_cast<unsigned*>(&s_item)[threadIdx.x] = reinterpret_cast<const __attribute__((address_space(4))) unsigned*>(it)[threadIdx.x];
    __syncthreads();
    level_dispatch(&s_item);
    (void)batch;
}

// Resident level workers: workgroup b serves slot b of the context (see Mailbox in sc_device.hpp).  Wavefront 0 polls
// the slot's mailbox over PCIe (a relaxed system-scope load, then a nap that grows to ~3 us), the other wavefronts wait
// at the workgroup barrier.  A new level: one system-scope acquire (the arrays of a new region arrive by DMA while this
// workgroup stays on its CU: its L1 must not serve lines of the region before) and a scalar-cache invalidate (the
// region's JobDev block is read through the constant address space), then the item goes to LDS and the variant it names
// runs exactly as it does behind k_level_any.  Every wavefront reaches the exit: `stop`, or a heartbeat that stands still.
__global__ __launch_bounds__(CHAIN_THREADS) void k_level_resident(ResidentArgs a) {
    __shared__ __attribute__((aligned(16))) LevelItem s_item;
    __shared__ int s_cmd;
    Mailbox* mb = a.mail + blockIdx.x;
    const int tid = threadIdx.x;
    unsigned last = 0, served = 0;
    if (tid == 0) {
        last = __hip_atomic_load(&mb->ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    for (;;) {
        if (tid == 0) {
            int cmd = 0;
            unsigned naps = 0;
            unsigned long long t_hb = wall_clock64();
            unsigned hb0 = __hip_atomic_load(&a.ctl->heartbeat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            for (;;) {
                const unsigned sq = __hip_atomic_load(&mb->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (sq != last) { cmd = 1; break; }
                if ((naps & 15u) == 15u) {
                    if (__hip_atomic_load(&a.ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
                    const unsigned hb = __hip_atomic_load(&a.ctl->heartbeat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    const unsigned long long now = wall_clock64();
                    if (hb != hb0) { hb0 = hb; t_hb = now; }
                    else if (now - t_hb > a.idle_ticks) break;           // nobody is there any more
                }
                naps++;
                if (naps < 32) __builtin_amdgcn_s_sleep(4);
                else if (naps < 256) __builtin_amdgcn_s_sleep(32);
                else __builtin_amdgcn_s_sleep(127);
            }
            if (cmd) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                __builtin_amdgcn_s_dcache_inv();
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                const volatile u4v* src = reinterpret_cast<const volatile u4v*>(&mb->item);      // five 16-byte reads over PCIe
                u4v* dst = reinterpret_cast<u4v*>(&s_item);
                static_assert(sizeof(LevelItem) == 80 && alignof(Mailbox) >= 8, "mailbox item");
#pragma unroll
                for (int i = 0; i < 5; i++) dst[i] = src[i];
                last = s_item.h.seq;
                served++;
                // an item that does not name one worker's pair of blocks was not written by the library: leave rather than follow its pointers
                const long ip = s_item.P - a.P_base, ir = s_item.R - a.R_base;
                if (ip < 0 || ip >= a.n_blocks || ir != ip || a.P_base + ip != s_item.P || s_item.job == nullptr) cmd = 2;
            }
            s_cmd = cmd;
        }
        __syncthreads();
        if (s_cmd != 1) break;
        level_dispatch(&s_item);
        __syncthreads();                                   // the level is stamped; s_item and s_cmd may be rewritten
    }
    if (tid == 0) {
        __hip_atomic_store(&mb->levels, served, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->state, s_cmd == 2 ? 3u : 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// --------------------------------------------------------------------------
// The pieces of a level on a grid.  Each is a kernel of its own, launched in stream order in front of the level's
// kernel: a kernel boundary is the only synchronisation between them.  They find the region through the pointer to
// its JobDev, as the level kernels do.  The strains' rows and label symbols and the copy pairs are kernel arguments
// (GridParams), the log priors of a hard update too (HardPriors); the log tables lie behind P: a device copy (a very large
// level of a context with several regions, launched from the set-up stream) or the host-mapped block itself
// (launch_level), of which a workgroup of k_level_update then reads only what its own items need.  k_hard_* read nothing
// behind P: seven launches stand in front of a plain level of a lone region, and none of them waits for PCIe.  The first kernel of a level leaves its tick in JobBlock::t0.
__device__ __forceinline__ void grid_tick(unsigned long long* t0) {
    if (t0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *t0 = wall_clock64();
}

// grid, phase 0: rows of strains created by the last extension (Strain copy, Strain.cpp:73-83); copies are
// independent (a destination row is a free row, a source row a surviving parent's).  As in phase_copies, cells past
// copy_n hold nothing yet.
__global__ __launch_bounds__(256) void k_level_copy(const JobDev* jp, LevelHdr h, GridParams g, unsigned long long* t0) {
    grid_tick(t0);
    KJob& job = *(KJob*)jp;
    const int c = blockIdx.y;
    const double2* src = reinterpret_cast<const double2*>(job.ll + (long)g.copy_src[c] * job.ll_stride);
    double2* dst = reinterpret_cast<double2*>(job.ll + (long)g.copy_dst[c] * job.ll_stride);
    const int n2 = ((h.copy_n < job.n_reads ? h.copy_n : job.n_reads) + 1) >> 1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// grid, phase 1, single-symbol labels: ll[s][rid] (+)= log P(read symbol | strain symbol), NonparametricClustering.cpp:343-391.
// Item idx is (strain idx / Rn, entry idx % Rn); a workgroup takes a run of consecutive items and stages the rows, labels
// and table rows of the strains of that run alone.  The strains' rows and symbols are kernel arguments (g), so the table
// rows behind P (over PCIe for a lone region) are one round trip: no address waits for a value from there.
__global__ __launch_bounds__(256) void k_level_update(const JobDev* jp, LevelHdr h, GridParams g, const LevelParams* __restrict__ P, unsigned long long* t0) {
    __shared__ double s_row[MAXS * KMAX];       // lpt[s][label of s][b]
    __shared__ double s_diag[MAXS * KMAX];      // lpt[s][b][b]  (an N in the strain label matches the read symbol)
    __shared__ int s_slot[MAXS], s_lab[MAXS];
    grid_tick(t0);
    KJob& job = *(KJob*)jp;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int S = h.S, K = job.K, e0 = h.e0, Rn = h.e1 - h.e0, codeN = job.code_N;
    const long total = (long)S * Rn;
    const long per = ((total + gridDim.x - 1) / gridDim.x + nt - 1) / nt * nt;
    const long lo = (long)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
    if (lo >= hi) return;                                   // (the whole workgroup)
    const int sa = (int)(lo / Rn), sb = (int)((hi - 1) / Rn);
    for (int s = sa + tid; s <= sb; s += nt) { s_slot[s] = g.slot[s]; s_lab[s] = g.lab[s]; }
    __syncthreads();                                        // s_lab is the one source of a strain's symbol from here on
    for (int i = sa * KMAX + tid; i < (sb + 1) * KMAX; i += nt) {
        const int sx = i / KMAX, b = i % KMAX, a = s_lab[sx];
        const double* lp = P->lpt + (long)sx * K * K;                  // compact [K][K] table of the strain
        s_row[i] = (a < K && b < K) ? lp[a * K + b] : 0.0;
        s_diag[i] = (b < K) ? lp[b * K + b] : 0.0;
    }
    __syncthreads();
    const long stride = job.ll_stride;
    for (long idx = lo + tid; idx < hi; idx += nt) {
        const int sx = (int)(idx / Rn), e = e0 + (int)(idx % Rn);
        const int rid = job.ent_rid[e];
        const int b = job.labels[job.ent_lab_off[e]];
        const bool fresh = job.ent_first[e] && !job.has[rid];
        if (sx == 0) job.isnew[e - e0] = fresh ? 1 : 0;
        int a = s_lab[sx];
        const bool wild = (a == codeN);
        if (wild) a = b;
        const double val = (a < K && b < K) ? (wild ? s_diag[sx * KMAX + b] : s_row[sx * KMAX + b]) : __longlong_as_double(0x7ff8000000000000ll);
        double* cell = job.ll + (long)s_slot[sx] * stride + rid;
        *cell = fresh ? val : (*cell + val);               // Strain::update_read_loglik, Strain.cpp:85-95
    }
}

// grid, per entry of the level.  Behind phase 1 the level's reads are present in read_loglik from here on (what the
// level's own workgroup does with 512 threads -- 117 rounds of two dependent loads on a level of 60 000 entries); the
// entry's draw slots (phase_slots), for the sampler's weight rows or the hard update.  Either or both.
__global__ __launch_bounds__(256) void k_level_entries(const JobDev* jp, LevelHdr h, int has, int slots, unsigned long long* t0) {
    grid_tick(t0);
    KJob& job = *(KJob*)jp;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (has) mark_present(job, h, first, step);
    if (slots) phase_slots<false>(job, h, first, step);
}

// grid, phase 3: the sampler's weight rows into tabLf, bitwise what weight_rows writes, whichever variant of the level's
// kernel follows: one that keeps its rows in LDS copies them from there.  A wavefront per workgroup; a group of ROWS_G
// neighbouring lanes takes one draw slot.  Lane k of the group owns the row's blocks of four floats k, k + ROWS_G, ... (the
// cells of four neighbouring strains each, one 16-byte store; the group's stores of a round are 16 * ROWS_G neighbouring bytes).
// Neighbouring groups are neighbouring reads, so a load instruction is ROWS_G strains' rows at 64 / ROWS_G nearby read ids: whichever
// strains a lane owns, a wavefront touches the same lines of the same S rows, so the layout is chosen by the stores.  The
// cells stay in registers between the maximum and the exponentials for every NB (4 * (NB + 1) at most).  The group joins its
// maxima with fmax, which is exact, associative and passes over a NaN on either side: m and the flag are the one-lane
// walk's, and an empty share (S < 4 * ROWS_G) contributes -inf.  The slot's read id comes from qrid (phase_slots), the
// strains' rows from the kernel arguments: nothing here waits for a read over PCIe.
constexpr int ROWS_G = 8;      // measured against 4: profiles/level_latency
template <int NB>
__global__ __launch_bounds__(64) void k_level_rows(const JobDev* jp, LevelHdr h, GridParams g, unsigned long long* t0) {
    constexpr int NBLK = (4 * NB + 1 + ROWS_G - 1) / ROWS_G;      // blocks of a lane: the stride is at most 16 * NB + 4 floats
    static_assert(64 % ROWS_G == 0 && ROWS_G <= 8, "a group lies inside a wavefront");
    grid_tick(t0);
    KJob& job = *(KJob*)jp;
    const int S = h.S, Q = h.Q;
    const int stride = chain_w_stride(S), nblk = stride >> 2;
    const int k = threadIdx.x % ROWS_G;
    SC_GLOBAL float* rows_g = (SC_GLOBAL float*)job.tabLf;
    auto put4 = [&](long idx, f4v v) __attribute__((always_inline)) { *(SC_GLOBAL f4v*)(rows_g + idx) = v; };
    // (every lane of a wavefront goes round as often as its first group: the shuffles below are the whole wavefront's)
    const int per_wave = 64 / ROWS_G;
    for (int q0 = blockIdx.x * per_wave; q0 < Q; q0 += gridDim.x * per_wave) {
        const int q = q0 + threadIdx.x / ROWS_G;
        const bool live = q < Q;
        double x[NBLK][4];
        double m = -INFINITY;
        if (live) {
            const SlotCells cells = slot_cells(job, h, job.qrid[q], job.quid[q]);
#pragma unroll
            for (int j = 0; j < NBLK; j++) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int sx = 4 * (k + ROWS_G * j) + i;
                    x[j][i] = -INFINITY;
                    if (sx < S) { x[j][i] = cells(g.slot[sx]); m = fmax(m, x[j][i]); }
                }
            }
        }
#pragma unroll
        for (int o = 1; o < ROWS_G; o <<= 1) m = fmax(m, __shfl_xor(m, o));
        if (!live) continue;
        const bool flag = row_flagged(m);
        const long Lf = (long)q * stride;
#pragma unroll
        for (int j = 0; j < NBLK; j++) {
            const int blk = k + ROWS_G * j;
            if (blk < nblk) put4(Lf + 4 * blk, row_block(x[j], 4 * blk, S, m, flag));
        }
        if (q == Q - 1) row_tail(put4, Lf + stride, k, ROWS_G);
    }
}

// hard_clustering (NonparametricClustering.cpp:17-125) of a level with millions of (strain, draw slot) pairs on a grid --
// the unthinned configs[3] region has 103 such levels of 26 strains x 110 000 slots, 9-13 ms each inside ONE workgroup.
// The pieces are the functions level_plain_body runs, called with the grid's index and size: the draw slots (phase_slots,
// k_level_entries); a zero log-likelihood for a mate not seen yet (zero_unseen_mates); per slot the responsibilities
// (normalise_column; each side fills x and finds its maximum its own way: the workgroup spreads (strain, slot) pairs over
// its threads, a thread of the grid walks its slot's strains); per strain ONE wavefront that adds its responsibilities
// (strain_sums): bit-identical results, 100 CUs instead of one.
__global__ __launch_bounds__(256) void k_hard_mates(const JobDev* jp, LevelHdr h, GridParams g) {
    __shared__ int s_slot[MAXS];
    KJob& job = *(KJob*)jp;
    for (int s = threadIdx.x; s < h.S; s += blockDim.x) s_slot[s] = g.slot[s];
    __syncthreads();
    zero_unseen_mates(job, h, [&](int s) { return s_slot[s]; }, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
__global__ __launch_bounds__(256) void k_hard_resp(const JobDev* jp, LevelHdr h, GridParams g, HardPriors pri) {
    __shared__ int s_slot[MAXS];
    __shared__ double s_logpri[MAXS];
    KJob& job = *(KJob*)jp;
    const int S = h.S;
    for (int s = threadIdx.x; s < S; s += blockDim.x) { s_slot[s] = g.slot[s]; s_logpri[s] = pri.logpri[s]; }
    __syncthreads();
    const long stride = job.ll_stride;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < h.Q; q += gridDim.x * blockDim.x) {
        const int rid = job.qrid[q], uid = job.quid[q];      // (qrid: ent_rid of the slot's entry, written with the slot)
        if (uid >= 0) job.has[uid] = 1;                      // (every check of k_hard_mates is behind us: a kernel boundary)
        double* col = job.tabA + q;
        double m = -INFINITY;
        for (int s = 0; s < S; s++) {
            const double* row = job.ll + (long)s_slot[s] * stride;
            double x = s_logpri[s] + row[rid];
            if (uid >= 0) x += row[uid];
            col[(long)s * job.qcap] = x;
            m = fmax(m, x);
        }
        normalise_column(col, job.qcap, S, m);
    }
}
// one wavefront per strain (= per workgroup of 64); the strain's symbol is its label's only one (no multi-symbol label
// reaches the grid)
__global__ __launch_bounds__(64) void k_hard_sums(const JobDev* jp, LevelHdr h, GridParams g, LevelResult* __restrict__ R) {
    KJob& job = *(KJob*)jp;
    const int s = blockIdx.x, lane = threadIdx.x, K = job.K, K2 = K * K, Q = h.Q;
    double acc[KMAX + 1];
    strain_sums(job.tabA + (long)s * job.qcap, job.qcode, Q, lane, acc);
    const int a = (int)g.lab[s];
    // the strain's [K][K] block of the substitution histogram: zero except the row of its own symbol (every cell written
    // once, by the lane that owns it; the sums live in lane 0)
    double row[KMAX];
#pragma unroll
    for (int b = 0; b < KMAX; b++) row[b] = __shfl(acc[b], 0);
    for (int i = lane; i < K2; i += 64) {
        double v = 0.0;
#pragma unroll
        for (int b = 0; b < KMAX; b++) if (a < K && b < K && i == a * K + b) v = row[b];
        R->subst[(long)s * K2 + i] = v;
    }
    if (lane == 0) R->abund[s] = acc[KMAX];
}

// every level kernel may ask for the whole dynamic part: the log tables / histogram of S strains over K symbols (S * K * K
// doubles), or the sampler's uniforms and weight rows
static int allow_lds(const void* kernel) { return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL); }
int init_level_kernels() {
    int rc = allow_lds(reinterpret_cast<const void*>(k_level));
    rc |= allow_lds(reinterpret_cast<const void*>(k_level_any));
    rc |= allow_lds(reinterpret_cast<const void*>(k_level_resident));
    for (int kind = 1; kind <= N_SAMPLER_KINDS; kind++)
        with_sampler_variant(kind, [&](auto nb, auto rows_lds) { rc |= allow_lds(reinterpret_cast<const void*>(&k_level_sample<decltype(nb)::value, decltype(rows_lds)::value>)); });
    return rc;
}
// doubles of LDS a level can spend on the strains' log tables / the soft update's histogram: S * K * K must fit
int level_table_capacity() { return LDS_BIG / (int)sizeof(double); }
// A level of ordinary size is ONE launch (launch_level_batch).  When a level has so many (strain, read) items or such
// long rows that a single workgroup would crawl (unthinned deep coverage), its row copies, single-symbol update and hard
// update run on a grid first, in any context.  In a context that walks a single region every other CU is idle anyway:
// there a level above `wide_min` items runs its copies, update, `has` marks, draw slots and weight rows on a grid.
// launch_level_grid returns the LV_* bits to pass on in LevelHdr::done.
constexpr long GRID_ITEMS = 1L << 17;          // (strain, read) items of a level
constexpr long GRID_COPY_WORDS = 1L << 19;     // doubles copied for new strains
constexpr long GRID_HARD = 1L << 18;           // (strain, draw slot) pairs of a hard update
constexpr long WIDE_ITEMS = 1L << 12;          // (strain, read) items of a level of a lone region (profiles/wide_level)
// SC_GRID_MIN: tests only, read once; replaces all three (0: every level the grid can take goes there, however small)
static long grid_min(long dflt) {
    static const long forced = [] { const char* e = getenv("SC_GRID_MIN"); return e ? atol(e) : -1L; }();
    return forced >= 0 ? forced : dflt;
}
// SC_WIDE_MIN: tests only, read once; replaces WIDE_ITEMS (0: every level of a lone region that can go wide does)
static long wide_min() {
    static const long forced = [] { const char* e = getenv("SC_WIDE_MIN"); return e ? atol(e) : -1L; }();
    return forced >= 0 ? forced : WIDE_ITEMS;
}
static bool hard_on_grid(const LevelHdr& h) {
    // (behind the grid's update only: the pieces of a level keep their order; a context with several regions)
    return h.mode == MODE_HARD && h.do_update && (long)h.S * (h.e1 - h.e0) > grid_min(GRID_ITEMS) && !h.has_dups && !h.any_multi &&
           (long)h.S * h.Q > grid_min(GRID_HARD) && h.e1 > h.e0;
}
bool level_wants_grid(int n_reads, const LevelHdr& h) {
    const long items = (long)h.S * (h.e1 - h.e0);
    return (h.do_update && items > grid_min(GRID_ITEMS) && !h.has_dups && !h.any_multi) || (long)h.n_copy * n_reads > grid_min(GRID_COPY_WORDS);
}
static int grid_blocks(long n, int per, int most) {
    const long g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > most ? most : g));
}
// The grid kernels of a level on `st`, in the order the level's workgroup keeps; g: the strains' rows and symbols and
// the copy pairs, out of the host's own copy of the parameters; P: the level's parameters as the kernels read them (the
// log tables); pri: the log priors of a hard update.  `lone`: the level of a context that walks a single region.
// The arguments of k_level_update and of k_hard_resp, the longest lists among the grid kernels, as the kernel-argument
// segment lays them out: each at its natural alignment, as the members of a struct; behind them up to 256 bytes of
// implicit arguments.
struct GridUpdateArgs { const JobDev* job; LevelHdr h; GridParams g; const LevelParams* P; unsigned long long* t0; };
struct GridHardArgs { const JobDev* job; LevelHdr h; GridParams g; HardPriors pri; };
static_assert(sizeof(GridUpdateArgs) + 256 <= 4096 && sizeof(GridHardArgs) + 256 <= 4096, "kernel-argument segment of the grid kernels");
int launch_level_grid(hipStream_t st, const JobDev* job, int n_reads, const LevelHdr& h, int kind, const GridParams& g, const HardPriors& pri,
                      const LevelParams* P, LevelResult* R, bool lone) {
    const int S = h.S, Rn = h.e1 - h.e0;
    const long items = (long)S * Rn;
    const bool upd = h.do_update && Rn > 0;
    const bool wide = lone && items > wide_min() && Rn > 0 && S > 0;
    const bool update_on_grid = upd && !h.has_dups && !h.any_multi && (items > grid_min(GRID_ITEMS) || wide);
    // the weight rows read what the update writes and the `has` marks behind it: behind the grid's update, or on a level
    // without one (read_assign)
    const bool rows_on_grid = wide && kind_has_sampler(kind) && h.Q > 0 && (update_on_grid || !upd);
    // the hard update behind the grid's update: a very large one in any context, and in a lone region's every one whose
    // level went wide (255 CUs stand idle while one workgroup walks its (strain, slot) pairs: profiles/level_tail)
    const bool hard = update_on_grid && (hard_on_grid(h) || (wide && h.mode == MODE_HARD && h.Q > 0));
    int done = 0;
    unsigned long long* t0 = lone ? &reinterpret_cast<JobBlock*>(const_cast<JobDev*>(job))->t0 : nullptr;      // for the level's first kernel
    // The rows of the level's new candidates come first, whoever makes them: a candidate's row must be its parent's row of
    // BEFORE this level's update.  (Until round 3 the update could go to the grid while a few small copies stayed with the
    // level's own kernel, which then copied the parent's already updated row over the child's: the child was scored with its
    // parent's symbol at this level.  Levels of more than 131 072 (candidate, read) items with fewer than 2^19 / reads new
    // candidates -- tests/golden/wide_cap120 found it at 121 candidates x 1 085 reads.)
    if (h.n_copy > 0 && ((long)h.n_copy * n_reads > grid_min(GRID_COPY_WORDS) || update_on_grid || rows_on_grid)) {
        const int n = h.copy_n < n_reads ? h.copy_n : n_reads;
        hipLaunchKernelGGL(k_level_copy, dim3(grid_blocks((n + 1) >> 1, 1024, 256), h.n_copy), dim3(256), 0, st, job, h, g, t0);
        t0 = nullptr;
        done |= LV_COPIES_DONE;
    }
    if (update_on_grid) {
        hipLaunchKernelGGL(k_level_update, dim3(grid_blocks(items, 512, 1024)), dim3(256), 0, st, job, h, g, P, t0);
        t0 = nullptr;
        done |= LV_ITEMS_DONE | LV_HAS_DONE;
    }
    // the `has` marks behind the update, and the draw slots of whoever reads them on a grid
    const bool slots = rows_on_grid || hard;
    if (update_on_grid || slots) {
        hipLaunchKernelGGL(k_level_entries, dim3(grid_blocks(Rn, 256, 1024)), dim3(256), 0, st, job, h, update_on_grid ? 1 : 0, slots ? 1 : 0, t0);
        t0 = nullptr;
        if (slots) done |= LV_SLOTS_DONE;
    }
    if (rows_on_grid) {
        with_sampler_variant(kind, [&](auto nb, auto) {
            // every slot's group of lanes exists up to 4 096 wavefronts; beyond (Q <= MAX_DRAWS: 5 000), the kernel's loop goes round
            hipLaunchKernelGGL((k_level_rows<decltype(nb)::value>), dim3(grid_blocks(h.Q, 64 / ROWS_G, 4096)), dim3(64), 0, st, job, h, g, t0);
        });
        done |= LV_ROWS_DONE;
    }
    if (hard) {
        const int gq = grid_blocks(h.Q, 256, 2048);
        hipLaunchKernelGGL(k_hard_mates, dim3(gq), dim3(256), 0, st, job, h, g);
        hipLaunchKernelGGL(k_hard_resp, dim3(gq), dim3(256), 0, st, job, h, g, pri);
        hipLaunchKernelGGL(k_hard_sums, dim3(S), dim3(64), 0, st, job, h, g, R);
        done |= LV_HARD_DONE;
    }
    return done ? (done | (lone ? LV_TICKED : 0)) : 0;
}
// One launch = the current level of `n` regions whose levels need the same kernel (workgroup b = batch.it[b]).
// The kind (sc_device.hpp) names that kernel: NB = ceil(S / 16) register blocks, weight rows in LDS where they fit.
int level_kind(const LevelHdr& h) {
    const int S = h.S, Q = h.Q, Rn = h.e1 - h.e0;
    const bool chain = h.mode == MODE_SAMPLE && h.n_sweeps > 0 && S > 1 && Rn > 0;
    if (!chain) return 0;
    const bool wl = ((long)Q * chain_w_stride(S) + 16) * 4 <= (long)CHAINW_ROWS_BYTES;
    int nb = (S + 15) / 16;
    nb = nb < 1 ? 1 : (nb > 8 ? 8 : nb);
    return sampler_kind(nb, wl);
}
// LDS a level needs, in KB: the per-strain scalars, then whichever is larger of the strains' log tables (S * K * K
// doubles, staged for the update; the soft update's histogram has the same shape) and the sampler's uniforms + weight
// rows.  A launch asks for the largest need among its items instead of the whole CU's LDS, so that two (small sampler
// levels) to four (levels without sampler) workgroups share a CU once more levels are in flight than the GPU has CUs.
int level_lds_kb(const LevelHdr& h, int K) {
    const int kind = level_kind(h);
    const long S = h.S, Rn = h.e1 - h.e0;
    long big = 0;
    if ((h.do_update && Rn > 0) || h.mode == MODE_HARD) big = (long)sizeof(double) * S * K * K;
    if (kind_has_sampler(kind)) {
        long rows = (long)UWIN * 4;
        if (kind_rows_lds(kind)) rows += ((long)h.Q * chain_w_stride(h.S) + 16) * 4;
        if (rows > big) big = rows;
    }
    long need = LDS_SMALL + big + 64;
    if (need > LDS_TOTAL) need = LDS_TOTAL;
    return (int)((need + 1023) / 1024);
}
static size_t batch_lds(const LevelBatch& b, int n) {
    int kb = 0;
    for (int i = 0; i < n; i++) { const int k = item_lds_kb(b.it[i].kind); kb = k > kb ? k : kb; }
    size_t bytes = (size_t)kb * 1024;
    if (kb == 0 || bytes > (size_t)LDS_TOTAL) bytes = LDS_TOTAL;
    return bytes;
}
// every item carries its kind and its LDS need (pack_kind)
void launch_level_any(hipStream_t st, const LevelBatch& b, int n) {
    hipLaunchKernelGGL(k_level_any, dim3(n), dim3(CHAIN_THREADS), batch_lds(b, n), st, b);
}
void launch_level_batch(hipStream_t st, int kind, const LevelBatch& b, int n) {
    const size_t lds = batch_lds(b, n);
    if (!kind_has_sampler(kind)) {
        hipLaunchKernelGGL(k_level, dim3(n), dim3(512), lds, st, b);
        return;
    }
    with_sampler_variant(kind, [&](auto nb, auto rows_lds) {
        hipLaunchKernelGGL((k_level_sample<decltype(nb)::value, decltype(rows_lds)::value>), dim3(n), dim3(CHAIN_THREADS), lds, st, b);
    });
}
// One level of a context that launches its own levels (a single region: Worker::complete_level, sc_sample_level): the
// pieces that go on a grid, then the level's kernel, all on `st` in stream order.  Returns the level's LV_* bits.
int launch_level(hipStream_t st, const LevelItem& it, const GridParams& g, const HardPriors& pri, int n_reads) {
    LevelBatch batch;
    batch.it[0] = it;
    LevelItem& b = batch.it[0];
    b.h.done |= launch_level_grid(st, b.job, n_reads, b.h, item_kind(b.kind), g, pri, b.P, b.R, true);
    launch_level_batch(st, item_kind(b.kind), batch, 1);
    return b.h.done;
}
// one grid of `slots` resident workgroups, each with the whole LDS of its CU (every variant must fit)
void launch_resident(hipStream_t st, const ResidentArgs& a, int slots) {
    hipLaunchKernelGGL(k_level_resident, dim3(slots), dim3(CHAIN_THREADS), LDS_TOTAL, st, a);
}
}  // namespace sc
#ifdef SC_CHAIN_PROF
extern "C" int sc_debug_chain_prof(unsigned long long* out) {       // experiment builds only
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sc::g_chain_prof), sizeof(unsigned long long) * 12);
}
#endif
