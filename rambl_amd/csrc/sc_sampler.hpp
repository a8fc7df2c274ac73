// The Polya-urn chain of a sampler level (a14, np_bayes_clustering; also a18, read_assign): device code only, included by
// sc_level.hip, whose level_sample_body builds what the chain draws from and calls it.
//
// The sampler is one dependent chain per region; four or eight wavefronts speculate
// over a window of draws and prove every accepted decision equal to the
// sequential one, near-ties go to an fp64 scan and then to a literal evaluation of
// the reference's formula, so every draw equals the reference's draw.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "sc_device.hpp"

namespace sc {

#define SC_GLOBAL __attribute__((address_space(1)))
#define SC_LDS __attribute__((address_space(3)))

// --------------------------------------------------------------------------
// wave64 helpers
template <int CTRL, int ROW_MASK, int BANK_MASK, bool BOUND>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, BANK_MASK, BOUND);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, BANK_MASK, BOUND);
    return __hiloint2double(hi, lo);
}
// inclusive prefix sum over the 64 lanes, in lane order
__device__ __forceinline__ double wave_scan_incl(double v) {
    v += dpp_f64<0x111, 0xF, 0xF, true>(v);   // row_shr:1
    v += dpp_f64<0x112, 0xF, 0xF, true>(v);   // row_shr:2
    v += dpp_f64<0x114, 0xF, 0xF, true>(v);   // row_shr:4
    v += dpp_f64<0x118, 0xF, 0xF, true>(v);   // row_shr:8
    v += dpp_f64<0x142, 0xA, 0xF, false>(v);  // row_bcast:15 -> rows 1,3
    v += dpp_f64<0x143, 0xC, 0xF, false>(v);  // row_bcast:31 -> rows 2,3
    return v;
}
__device__ __forceinline__ double wave_shr1(double v) {   // lane i gets lane i-1, lane 0 gets 0
    return dpp_f64<0x138, 0xF, 0xF, true>(v);             // wave_shr:1
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// --------------------------------------------------------------------------
// Literal fp64 evaluation of one categorical draw, exactly as the reference
// forms it (NonparametricClustering.cpp:171-194 with libstdc++'s
// discrete_distribution): executed by lane 0 of the sampling wave for the rare
// draw whose uniform lies within the safety margin of a boundary.
struct SlowArgs {          // the few JobDev fields the rare tiers need, passed by value
    const int* qent; const int* quid; const int* ent_rid; const double* ll; long ll_stride; const uint8_t* has;
};
__device__ int exact_draw(const SlowArgs job, const int* s_slot, const volatile double* s_a,
                          volatile double* s_p, int S, int rid, int uid, double u) {
    double Z = 0;
    for (int s = 0; s < S; s++) Z += s_a[s];
    for (int s = 0; s < S; s++) {
        double p = s_a[s] / Z;
        const double* row = job.ll + (long)s_slot[s] * job.ll_stride;
        p = log(p) + (job.has[rid] ? row[rid] : 0.0);
        if (uid >= 0 && job.has[uid]) p += row[uid];
        s_p[s] = exp(p);
    }
    if (S < 2) return 0;
    double sum = 0;
    for (int s = 0; s < S; s++) sum += s_p[s];
    double acc = 0;
    for (int s = 0; s < S; s++) {
        double pr = s_p[s] / sum;
        acc = (s == 0) ? pr : acc + pr;
        s_p[s] = acc;
    }
    s_p[S - 1] = 1.0;
    int lo = 0, len = S;     // std::lower_bound
    while (len > 0) {
        int half = len >> 1, mid = lo + half;
        if (s_p[mid] < u) { lo = mid + 1; len = len - half - 1; }
        else len = half;
    }
    return lo;
}

constexpr double DRAW_EPS64 = 1e-10;  // margin (relative to the total weight) of the fp64 scan tier

// Tier 2 and 3 of one draw: fp64 weights and scan with a 1e-10 margin; if the
// uniform is still within the margin of a boundary (or the slot's log-likelihoods
// lie in the underflow range of the reference's exp), the literal evaluation.
// The slot's log-likelihoods are re-read from the rows (the table kept only their
// fp32 weights).  Wave-uniform call.
template <int NPL>
__device__ __noinline__ int slow_draw(const SlowArgs job, const int* s_slot, volatile double* s_a, volatile double* s_p,
                                      double a0, double a1, int S, int q, int e0, double u, int lane) {
    const double a[2] = {a0, a1};
    const int rid = job.ent_rid[e0 + job.qent[q]], uid = job.quid[q];
    const bool hr = job.has[rid] != 0, hu = uid >= 0 && job.has[uid] != 0;
    double x[NPL], m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPL; i++) {
        const int s = lane * NPL + i;
        x[i] = -INFINITY;
        if (s < S) {
            const double* row = job.ll + (long)s_slot[s] * job.ll_stride;
            double v = hr ? row[rid] : 0.0;
            if (hu) v += row[uid];
            x[i] = v;
            m = fmax(m, v);
        }
    }
    for (int d = 1; d < 64; d <<= 1) m = fmax(m, __shfl_xor(m, d));
    const bool flag = !(m >= -600.0);                     // underflow range of the reference's exp(); also NaN / -inf
    double w[NPL], pair = 0;
#pragma unroll
    for (int i = 0; i < NPL; i++) {
        const int s = lane * NPL + i;
        // fp64 weight a_s * exp(loglik - max)
        w[i] = (s < S) ? a[i] * exp(x[i] - m) : 0.0;
        pair += w[i];
    }
    const double incl = wave_scan_incl(pair);
    const double T = readlane_f64(incl, 63);
    const double tgt = u * T;
    const double lo = tgt - DRAW_EPS64 * T, hi = tgt + DRAW_EPS64 * T;
    bool ok = (T > 0.0) && (T < 1.0e300) && !flag;
    int c;
    if (NPL == 1) {
        const unsigned long long mlo = __ballot(incl >= lo), mhi = __ballot(incl >= hi);
        ok = ok && (mlo == mhi) && (mlo != 0ull);
        c = ok ? (int)__builtin_ctzll(mlo) : 0;
    } else {
        const double E = wave_shr1(incl);
        const double c0 = E + w[0], c1 = E + pair;
        const unsigned long long m0lo = __ballot(c0 >= lo), m0hi = __ballot(c0 >= hi);
        const unsigned long long m1lo = __ballot(c1 >= lo), m1hi = __ballot(c1 >= hi);
        ok = ok && (m0lo == m0hi) && (m1lo == m1hi) && (m1lo != 0ull);
        const int l1 = ok ? (int)__builtin_ctzll(m1lo) : 0;
        c = 2 * l1 + (((m0lo >> l1) & 1ull) ? 0 : 1);
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < NPL; i++) { int s = lane * NPL + i; if (s < S) s_a[s] = a[i]; }
        __builtin_amdgcn_wave_barrier();
        int cc = 0;
        if (lane == 0) cc = exact_draw(job, s_slot, s_a, s_p, S, rid, uid, u);
        c = __builtin_amdgcn_readfirstlane(cc);
        __builtin_amdgcn_wave_barrier();
        c |= 0x100;                                    // tell the caller the literal tier ran
    }
    return c;
}

// --------------------------------------------------------------------------
// Wide urn chain: a sliding window of 64 draws over the four wavefronts of the
// workgroup (one per SIMD), four lanes per draw (128 draws on eight wavefronts
// while a lane owns at most 8 strains).
//
// Draw t+p of a pass (p = 0..63) belongs to the quad of lanes 4*(p%16)..+3 of
// wave p/16; lane k of the quad walks its quarter of the strains in order with
// the counts as they are in front of draw t (uniform over the draws), one FMA
// per strain: cum_s = sum_{s'<=s} (a0_s' + k_s') * L[q][s'].  The quarters are
// joined inside the quad by DPP (totals -> offsets and T, then the number of
// boundaries below u*T and the distances to the nearest boundary on either side).
//
// Why a speculative decision is final.  Let d_s = cum_s - u*T.  Each of the p
// draws in front of draw t+p adds one to one count c_j, which adds L[c_j] <= 1
// to T and to every cum_s with s >= c_j: d_s moves by L[c_j]*([c_j <= s] - u),
// i.e. up by at most (1-u) and down by at most u per earlier draw.  So a boundary
// below the target (d_s < 0) stays below it if -d_s > (1-u)*p and one at or above
// it (d_s >= 0) stays there if d_s > u*p -- whatever the earlier draws of the
// window turn out to be.  The test adds eps*T on both sides for the fp32 error of
// the chains and sums (< (2*S + 9) * 2^-24 relative to T).  Each pass accepts the
// draws in front of the first one that fails the test (one LDS integer atomic per
// accepted draw, on its strain's count, and one byte -- the strain -- stored to
// the region's draw log in device memory, which no pass reads and no barrier
// waits for: the draws per (strain, read symbol) are counted from the log after
// the chain, draw_log_counts; the waves exchange the position through LDS) and
// the window moves on to that draw, which then has p = 0 and margin eps*T only.  A draw that
// fails at p = 0 is within the fp32 error bound of a boundary (or its row is NaN:
// flagged slot): wave 0 sends it through the fp64 scan and, if needed, the literal
// evaluation.
//
// Weight rows are row-major [Q][stride] fp32, stride = 4 * odd.
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fma_rn(float a, float b, float c) {       // three-address FMA (no v_fmac + copy)
    float d;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ f2v pk_sub(f2v a, f2v b) {
    f2v d;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// min over the raw bits as unsigned integers: among floats, the smallest non-negative one (a negative float has
// the sign bit set and compares above every non-negative float)
__device__ __forceinline__ unsigned min3_u32(unsigned m, unsigned x, unsigned y) {
    unsigned d;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(x), "v"(y));
    return d;
}
template <int QP> __device__ __forceinline__ float quad_f32(float v) {     // quad_perm DPP
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), QP, 0xF, 0xF, true));
}
template <int QP> __device__ __forceinline__ int quad_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, QP, 0xF, 0xF, true);
}
// LDS-only workgroup barrier: does not wait for outstanding global loads / stores
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// The same barrier, entered while the wavefront's N youngest LDS operations may still be in flight.  LDS operations of
// one wavefront retire in the order they were issued, so once at most N are outstanding every LDS operation in front of
// the N youngest has retired.  The caller has to know that at least N LDS operations follow, in the instruction stream,
// the one the other wavefronts need; if more follow, the wait is merely stricter.  A scalar load shares the counter and
// returns out of order with LDS: one outstanding here takes a place among the N and makes the wait stricter, never
// weaker (the LDS operations outstanding are still the youngest, and there are still at most N of them).
template <int N> __device__ __forceinline__ void lds_barrier_keep() {
    static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
    asm volatile("s_waitcnt lgkmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// A scalar a loop reads, as the compiler sees it from here on: a value in scalar registers of unknown origin.  Whatever
// loaded it has been waited for in front of this point, and the load can neither be repeated inside the loop nor be
// moved to its head (profiles/level_latency, profiles/level_tail: a scalar load pending at the head of the pass loop
// shares lgkmcnt with the loop's LDS reads and turns their staged waits into one wait for all).  64 bits go as two halves.
// (readfirstlane: a resident workgroup reads its item out of LDS, so the compiler holds these uniform values in vector
// registers there; on a value that is in scalar registers already it folds away.)
template <class T> __device__ __forceinline__ T pin_scalar(T x) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two scalar registers");
    if constexpr (sizeof(T) == 4) {
        unsigned v = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, x));
        asm volatile("" : "+s"(v));
        return __builtin_bit_cast(T, v);
    } else {
        const unsigned long long w = __builtin_bit_cast(unsigned long long, x);
        unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)w), hi = __builtin_amdgcn_readfirstlane((unsigned)(w >> 32));
        asm volatile("" : "+s"(lo), "+s"(hi));
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    }
}

constexpr int UWIN = 1024;     // uniforms staged in LDS (fp32), refilled in halves
#ifdef SC_CHAIN_PROF
// experiment builds only (make EXTRA=-DSC_CHAIN_PROF): where a pass of the chain spends its cycles, summed over every pass
// of wave 0: [0] counts read + chains, [1] test + s_x write, [2] first barrier + advance, [3] commit section: bookkeeping
// (ro, upos, uniform refill), [4] second barrier, [5] passes, and the rest of the commit section: [6] issue_loads, [7] the
// s_kf commit, [8] the draw-log store.  The three stamps inside the commit section first wait for the LDS operations in
// front of them (CHAIN_STAMP_W): what is asynchronous in the product build -- the next rows' LDS reads, the atomic -- is
// charged to its own part here, so the parts add up to more than the section costs when they overlap.  The last pass of a
// level runs the commit section and its stamps like any other and leaves in front of the second barrier and its stamp.
// (The product build issues the commit first and lets the bookkeeping and the reads run inside its latency: this build,
// which waits at [7], cannot show that overlap.)
__device__ unsigned long long g_chain_prof[12];
#define CHAIN_STAMP(k) do { if (wv == 0) { const unsigned t_ = (unsigned)clock64(); prof[k] += t_ - tprev; tprev = t_; } } while (0)
#define CHAIN_STAMP_W(k) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); CHAIN_STAMP(k); } while (0)
#else
#define CHAIN_STAMP(k) do {} while (0)
#define CHAIN_STAMP_W(k) do {} while (0)
#endif

// WIDE_Q: the level has at least a window of draw slots (Q >= 16 * NW), so a pass moves a lane's row at most once past the
// last one.  The caller decides it once per level (the pass loop holds neither the test nor the other way's code).
template <int NQ, bool ROWS_LDS, int NW, bool WIDE_Q, class JD>
__device__ __forceinline__ void urn_chain_q(const JD& job, const LevelHdr& h, const StrainParam* s_sp, LevelResult* __restrict__ R,
                                            const int* s_slot, volatile double* s_a, volatile double* s_p, unsigned* s_kf,
                                            const float* s_a0f, int* s_x, float* s_uwin, const float* rows_lds, int stride, int tid) {
    constexpr int SPL = 4 * NQ, SP = 16 * NQ;               // strains per lane, capacity
    constexpr int NPLC = SP > 64 ? 2 : 1;                  // strains per lane in the checked tier
    constexpr float EPSW = (float)(SP + 16) * 1.5e-7f;     // (2*S + 9) * 2^-24 for the chains and sums + 3 * 2^-24 for the weights (exp_weight)
    // (the wavefront's index as a scalar: what only wavefront 0 does -- the uniforms, the checked tiers -- then costs the
    // others a scalar branch instead of a walk through masked-off vector code)
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), k = lane & 3, pos = wv * 16 + (lane >> 2);
    // Every scalar the pass loop reads is pinned here (pin_scalar), the rare tiers' too: no scalar load is pending at the
    // head of the loop or issued inside it, so lgkmcnt counts this wavefront's LDS operations alone there.
    const int S = pin_scalar(h.S), Q = pin_scalar(h.Q), n = pin_scalar(h.n_sweeps), e0 = pin_scalar(h.e0);
    stride = pin_scalar(stride);
    const int Sm1 = S - 1;
    const int total = n * Q;
    const SlowArgs sa{pin_scalar(job.qent), pin_scalar(job.quid), pin_scalar(job.ent_rid), pin_scalar(job.ll), pin_scalar(job.ll_stride), pin_scalar(job.has)};
    const SC_GLOBAL double* Ustream = pin_scalar((const SC_GLOBAL double*)job.U);
    const SC_GLOBAL float* Uf = pin_scalar((const SC_GLOBAL float*)job.Uf);
    const SC_GLOBAL float* rows_g = pin_scalar((const SC_GLOBAL float*)job.tabLf);
    SC_GLOBAL unsigned char* dlog = pin_scalar((SC_GLOBAL unsigned char*)job.dlog);
    auto ld4 = [&](int idx) __attribute__((always_inline)) -> f4v {
        return ROWS_LDS ? *(const f4v*)(rows_lds + idx) : *(const SC_GLOBAL f4v*)(rows_g + idx);
    };
    auto ld1 = [&](int idx) __attribute__((always_inline)) -> float { return ROWS_LDS ? rows_lds[idx] : rows_g[idx]; };

    const int cbase = k * SPL;                              // first strain of this lane's quarter
    const float m0 = k > 0 ? 1.0f : 0.0f, m1 = k > 1 ? 1.0f : 0.0f;
    const float posf = (float)pos + 1.0e-37f;
    double a0m[NPLC];                                       // wave 0, checked tier: strains across the lanes
#pragma unroll
    for (int i = 0; i < NPLC; i++) { const int s = lane * NPLC + i; a0m[i] = (s < S) ? s_sp[s].a0 : 0.0; }
    f4v a0q[NQ];
#pragma unroll
    for (int g = 0; g < NQ; g++) a0q[g] = *(const f4v*)(s_a0f + cbase + 4 * g);
    unsigned n_exact = 0, n_slow = 0, n_pass = 0;           // (a level has at most MAX_DRAWS draws: 32 bits, widened in LevelResult)
    const unsigned long long clk0 = clock64(), wall0 = wall_clock64();

    // uniforms: draws [ulo, ulo + UWIN) live in s_uwin[p & (UWIN-1)]; wave 0 refills.  unext is the next t at which it
    // has anything to do: ulo + UWIN / 4 (prefetch the next half window into ux0 / ux1) and ulo + UWIN / 2 (swap it in)
    // in turn, every quarter of a window.  The other wavefronts never get there, so a pass asks one question, not who
    // and which.
    int ulo = 0;
    int unext = wv == 0 ? UWIN / 4 : INT_MAX;
    f4v ux0 = 0.0f, ux1 = 0.0f;
    if (wv == 0) {
#pragma unroll
        for (int j = 0; j < UWIN / 256; j++) *(f4v*)(s_uwin + 256 * j + 4 * lane) = *(const SC_GLOBAL f4v*)(Uf + 256 * j + 4 * lane);
    }
    __syncthreads();

    int t = 0;
    int ro = (pos % Q) * stride;                            // row offset (floats) of this lane's draw
    const int wrap = Q * stride;
    int upos = pos;                                        // (t + pos) & (UWIN - 1)
    f4v L[NQ];
    float uf = 0.0f, llast = 0.0f;
    auto issue_loads = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NQ; g++) L[g] = ld4(ro + cbase + 4 * g);
        llast = ld1(ro + Sm1);
        uf = s_uwin[upos];
    };
    if (total > 0) issue_loads();
#ifdef SC_CHAIN_PROF
    unsigned prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = (unsigned)clock64();     // (32 bits hold a level's cycles: scalar registers are short in this loop)
#endif
    // Every pass ends with the same commit, the last one too, and the loop is left behind that commit and in front of
    // the pass's second barrier -- where the last pass has always left it.  The barriers of the chain are therefore what
    // urn_chain_shadow takes part in: one behind the staged uniforms, two per pass but one in the last, one behind the loop.
#pragma unroll 1
    while (total > 0) {
        asm volatile("" ::: "memory");                      // s_kf below must be re-read
        n_pass++;
        // this lane's quarter: cumulative weights with the counts in front of draw t
        float loc[SPL];
        float run = 0.0f;
        u4v kq[NQ];
#pragma unroll
        for (int g = 0; g < NQ; g++) kq[g] = *(const u4v*)(s_kf + cbase + 4 * g);
        const unsigned klast = s_kf[Sm1];                       // (read with the others: one LDS round trip, not two)
        const float a0last = s_a0f[Sm1];
#pragma unroll
        for (int g = 0; g < NQ; g++) {
            const u4v kk = kq[g];
            const f4v av = a0q[g] + f4v{(float)kk.x, (float)kk.y, (float)kk.z, (float)kk.w};
            loc[4 * g + 0] = run = (g == 0) ? av.x * L[g].x : fma_rn(av.x, L[g].x, run);
            loc[4 * g + 1] = run = fma_rn(av.y, L[g].y, run);
            loc[4 * g + 2] = run = fma_rn(av.z, L[g].z, run);
            loc[4 * g + 3] = run = fma_rn(av.w, L[g].w, run);
        }
        const float alast = a0last + (float)klast;
        CHAIN_STAMP(0);
        // quad: offset of this quarter and the total weight (bitwise the same in the four lanes)
        const float i1 = fmaf(quad_f32<0x90>(run), m0, run);       // + previous lane of the quad   ([0,0,1,2])
        const float i2 = fmaf(quad_f32<0x40>(i1), m1, i1);         // + two lanes back              ([0,0,0,1])
        const float off = i2 - run;
        const float T = quad_f32<0xFF>(i2);
        // position of u*T among the boundaries and the distance to the nearest one on either side
        const float tgt = uf * T;
        const float tb = tgt - off;
        const f2v tb2 = {tb, tb};
        unsigned w = 0;
        unsigned up = 0x7f800000u, dn = 0x7f800000u;        // +inf: nearest boundary at / above and below the target
#pragma unroll
        for (int j = 0; j < SPL; j += 2) {
            const f2v lc = {loc[j], loc[j + 1]};
            const f2v d = pk_sub(lc, tb2);                   // cum - target
            const f2v e = pk_sub(tb2, lc);                   // target - cum
            w = __builtin_amdgcn_alignbit(w, __float_as_uint(d.x), 31);   // (w << 1) | sign(d)
            w = __builtin_amdgcn_alignbit(w, __float_as_uint(d.y), 31);
            up = min3_u32(up, __float_as_uint(d.x), __float_as_uint(d.y));
            dn = min3_u32(dn, __float_as_uint(e.x), __float_as_uint(e.y));
        }
        // Strains >= S-1 and the padding all sit at cum = T >= u*T: they are no boundaries.  They never count (a
        // padding entry can round to a tiny negative difference: the count is clamped, and that draw fails the
        // test below), and their distance T - u*T must not fail a draw whose target lies above the last real
        // boundary cum_{S-2}: alt = u*T - cum_{S-2} is then positive and IS the distance to the nearest real
        // boundary; once it clears the lower margin there is nothing above the target to test.
        const float alt = tgt - (T - alast * llast);
        const float epsT = EPSW * T;
        // a boundary at / above the target moves down by <= u per earlier draw, one below it up by <= 1 - u.  The pass
        // knows u only as its fp32 copy uf (|u - uf| <= 2^-25: 1 - uf can lie below 1 - u, uf below u) and forms the
        // limits in fp32: 2^-22 per earlier draw covers both.  (That slack is absolute, per draw of weight <= 1, so
        // eps * T does not cover it once T is small: 100 draws of u = 1e-9 in front of a u = 1 - 1.25 * 2^-24, which
        // reads 1 - 2^-24, at T = 0.1 -- tests/test_sampler_tiers.py)
        const float lim_up = fmaf(uf + 0x1p-22f, posf, epsT);
        const float lim_dn = fmaf((1.0f + 0x1p-22f) - uf, posf, epsT);
        // NaN (flagged slot) and T == 0 fail the test
        // (a ballot per compare and the masks joined as scalars: no branch around the second and third compare -- behind
        // which the compiler had moved the LDS read of klast -- and no 0 / 1 per lane to take the ballot from; every lane
        // of the wavefront is active here)
        const unsigned long long ok_dn = __builtin_amdgcn_ballot_w64(__uint_as_float(dn) >= lim_dn);
        const unsigned long long ok_up = __builtin_amdgcn_ballot_w64(__uint_as_float(up) >= lim_up);
        const unsigned long long ok_alt = __builtin_amdgcn_ballot_w64(alt >= lim_dn);
        const unsigned long long F = ~(ok_dn & (ok_up | ok_alt));
        const int fpos = F ? 16 * wv + ((int)__builtin_ctzll(F) >> 2) : 16 * NW;
        if (lane == 0) s_x[wv] = fpos;
        int c = __popc(w);
        c += quad_i32<0xB1>(c);
        c += quad_i32<0x4E>(c);
        c = min(c, Sm1);
        CHAIN_STAMP(1);
        lds_barrier();
        const int rem = total - t;
        int adv = 16 * NW;
#pragma unroll
        for (int j = 0; j < NW / 4; j++) {
            const i4v xf = *(const i4v*)(s_x + 4 * j);
            adv = min(adv, min(min(xf.x, xf.y), min(xf.z, xf.w)));
        }
        adv = adv < rem ? adv : rem;
        CHAIN_STAMP(2);
        if (adv == 0) {
            // draw t itself: fp64 scan with the exact counts, then the literal tier (wave 0)
            if (wv == 0) {
                const double u = Ustream[t];
                double ad[NPLC];
#pragma unroll
                for (int i = 0; i < NPLC; i++) { const int s = lane * NPLC + i; ad[i] = a0m[i] + (double)((s < S) ? s_kf[s] : 0u); }
                const int qi = __builtin_amdgcn_readfirstlane(ro) / stride;
                const int cc = slow_draw<NPLC>(sa, s_slot, s_a, s_p, ad[0], NPLC > 1 ? ad[NPLC - 1] : 0.0, S, qi, e0, u, lane);
                n_slow++;
                n_exact += (cc >> 8) & 1;
                c = cc & 0xFF;
            }
            adv = 1;
        }
        const bool acc = (pos < adv) && (k == 0);
        const unsigned lg = (unsigned)(t + pos);                 // acc: t + pos < total <= JobDev::dlog_cap (the log: base + 32 bits)
        t += adv;
        // The commit goes first: it is what the other wavefronts wait for at the second barrier, and everything else of
        // this section -- the window's bookkeeping, the reads of the next window -- runs inside its latency, not in
        // front of it.  Nothing below may be moved in front of it by the compiler (the reads would then be older than
        // the atomic and the barrier's count would cover less than it says).  (profiles/chain_waits: worth 0.26 cycles
        // per draw with the loop's scalars pinned, nothing without -- the two were measured apart.)
        if (acc) __hip_atomic_fetch_add(&s_kf[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
        CHAIN_STAMP_W(7);
        // The row and the uniform of this lane's draw in the next window.  The last pass (t == total) moves them like any
        // other and loads what nobody uses, from inside the rows and the staged uniforms: ro stays below wrap (WIDE_Q:
        // ro < wrap and adv * stride <= 16 * NW * stride <= wrap, so r1 < 2 * wrap and the smaller of r1, r1 - wrap is
        // < wrap; else a row index mod Q), the lane reads ro .. ro + SP - 1 <= the 16 zeros behind the last row, and upos
        // is masked to the window.  A refill in the last pass reads uniforms below total + 1280, inside the stream's
        // padding of 2048, and stores them to the half of s_uwin no draw of this level reads any more.
        if (WIDE_Q) {
            const unsigned r1 = (unsigned)(ro + adv * stride);
            const unsigned r2 = r1 - (unsigned)wrap;         // wraps to a huge value while r1 < wrap
            ro = (int)(r1 < r2 ? r1 : r2);
        } else {
            ro = ((ro / stride + adv) % Q) * stride;
        }
        upos = (upos + adv) & (UWIN - 1);
        // uniforms: prefetch the next half window, swap it in when the window has moved past the old one.  (A pass moves
        // t by at most 128 and the two are 256 apart, so they take turns.  Two tests in a row, not if / else: around an
        // else the compiler loads into other registers and copies them to ux0 / ux1 behind a wait for the load, in the
        // pass that issued it, and waits for the draw log's store of the pass before in front of every pass's row reads.)
        if (t >= unext) {                                    // wavefront 0 alone
            if (unext & (UWIN / 4)) {
                ux0 = *(const SC_GLOBAL f4v*)(Uf + ulo + UWIN + 4 * lane);
                ux1 = *(const SC_GLOBAL f4v*)(Uf + ulo + UWIN + 256 + 4 * lane);
            }
            if (t >= ulo + UWIN / 2) {
                *(f4v*)(s_uwin + ((ulo & (UWIN - 1)) + 4 * lane)) = ux0;
                *(f4v*)(s_uwin + ((ulo & (UWIN - 1)) + 256 + 4 * lane)) = ux1;
                ulo += UWIN / 2;
            }
            unext += UWIN / 4;
        }
        CHAIN_STAMP(3);
        issue_loads();                                       // behind the commit: the youngest of them may cross the barrier below
        CHAIN_STAMP_W(6);
        // the draw's strain goes to the region's draw log: a vector-memory byte store, which the barrier below (LDS counter
        // only) does not wait for.  The draws per (strain, read symbol) are counted from the log after the chain
        // (draw_log_counts): no pass reads them.
        if (acc) dlog[lg] = (unsigned char)c;
        CHAIN_STAMP_W(8);
        if (t >= total) break;                               // (in front of the barrier: urn_chain_shadow leaves here too)
        // Every wavefront's commits are in s_kf behind this barrier, which waits for the commit and not for the reads
        // issued behind it (lds_barrier_keep).  Behind the atomic this wavefront has issued, in this order: the refill's
        // two LDS writes (wavefront 0, some passes), then issue_loads() -- with the rows in LDS the NQ 16-byte reads of
        // L[g], which the compiler can neither merge nor leave out, and the reads of llast and uf; with the rows in memory
        // the read of uf alone, the rows being global loads that no LDS barrier ever waited for.  So at least NQ (or
        // one) LDS operations are younger than the atomic, and once at most that many are outstanding the atomic has
        // retired; llast and uf, counted or not, only make the wait stricter, and so do the refill's writes.  Those
        // need not be waited for here at all: they fill the half of s_uwin that no draw reads before the window has
        // moved on by a quarter of UWIN, several passes on, and wavefront 0 passes the next pass's first barrier --
        // lgkmcnt(0) -- before anyone gets there.  The reads left in flight are this wavefront's own; the compiler waits
        // for them where the next pass uses them.  The pass that leaves the loop leaves in front of this barrier, and the
        // closing __syncthreads() drains whatever it left.
        lds_barrier_keep<ROWS_LDS ? NQ : 1>();
        CHAIN_STAMP(4);
    }
#ifdef SC_CHAIN_PROF
    if (tid == 0) { for (int i = 0; i < 9; i++) if (i != 5) atomicAdd(&g_chain_prof[i], (unsigned long long)prof[i]); atomicAdd(&g_chain_prof[5], (unsigned long long)n_pass); }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the draw log's stores have left this wavefront ...
    __syncthreads();                                         // ... every wavefront's (draw_log_counts reads them)
    if (wv == 0) {
#pragma unroll
        for (int i = 0; i < NPLC; i++) {
            const int s = lane * NPLC + i;
            if (s < S) { R->abund[s] = a0m[i] + (double)s_kf[s]; R->kdraw[s] = s_kf[s]; }
        }
        if (lane == 0) {
            R->n_draws = (unsigned long long)total; R->n_exact = n_exact; R->n_slow = n_slow; R->n_pass = n_pass;
            R->chain_cycles = clock64() - clk0; R->chain_wall = wall_clock64() - wall0;
        }
    }
}

// The draws per (strain, read symbol) -- the substitution counts of :198-206 -- out of the draw log, after the chain's
// closing barrier, by every wavefront of the workgroup that is still there.  Draw t is the draw of slot t % Q, whose read
// symbol is job.qcode[slot]; a symbol >= KMAX (no single symbol) is not counted.  A lane takes one slot and a stretch of
// at most LOG_STRETCH of its sweeps and counts runs of one strain in a register: where a read prefers one strain sweep
// after sweep, a lane adds to s_cnt once per run, not once per draw.
//
// Where the time goes (profiles/level_tail): not into the loads -- a lane issues every load of its stretch, and the slot's
// symbol beside them, before it uses the first, one round trip to the L2 per round of the loop, and that alone moved the
// count by 0.5 us of 11.7 -- but into the LDS adds.  A level of 30 candidates that differ in one symbol each gives a read
// nearly the same weight for all of them: runs are one or two draws long, a level has tens of thousands of adds, and the
// slots of one level carry almost all the same symbol.  With counts laid out [strain][symbol] every add of a wavefront
// then falls on the two banks (strain * 16 + symbol) mod 32 leaves, one LDS cycle per distinct address.  s_cnt is therefore
// [symbol][strain] (log_cnt_index): the bank is the strain's, adds to different strains go side by side, and only lanes
// that add to the very same strain take turns.  The level's body writes LevelResult::cnt from it in the result's order.
//
// A stretch shorter than the loaded blocks of eight (the slot's last stretch, or a stretch that is no multiple of eight)
// loads its own last sweep again in place of the sweeps it does not have -- inside the log.  Those copies lengthen the
// stretch's last run, by a number the lane knows and takes off again, so no step of the walk asks whether it exists.
// Blocks of eight that no stretch of the level reaches are skipped by the whole workgroup.  The log is rewritten every
// level, also by a workgroup that stays on its CU (resident workers): the chain's wavefronts have drained their stores in
// front of the barrier, and a device-scope acquire here keeps the L1 from serving a line of an earlier level.
constexpr int LOG_STRETCH = 24;                              // sweeps a lane holds in registers (three blocks of eight loads)
__device__ __forceinline__ int log_cnt_index(int strain, int sym) { return sym * MAXS + strain; }     // s_cnt: [KMAX][MAXS]
template <class JD>
__device__ __forceinline__ void draw_log_counts(const JD& job, const LevelHdr& h, unsigned* s_cnt, int tid, int nt) {
    const int Q = h.Q, n = h.n_sweeps;
    if (Q <= 0 || n <= 0) return;                           // (no draws: uniform over the workgroup, like the chain's own loop)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const SC_GLOBAL unsigned char* dlog = (const SC_GLOBAL unsigned char*)job.dlog;
    const SC_GLOBAL unsigned char* qcode = (const SC_GLOBAL unsigned char*)job.qcode;
    // stretches of sweeps per slot: as many as a stretch needs to fit the registers, more while lanes would be idle
    const int G = max((n + LOG_STRETCH - 1) / LOG_STRETCH, min(nt / Q, n));
    const int per = (n + G - 1) / G;                        // 1 .. LOG_STRETCH, uniform
    const int loaded = (per + 7) & ~7;                      // sweeps a lane loads and walks: whole blocks
    for (int idx = tid; idx < Q * G; idx += nt) {           // (Q * G <= Q * n <= JobDev::dlog_cap)
        const int q = idx % Q, j0 = (idx / Q) * per;
        const int len = min(per, n - j0);                   // sweeps [j0, j0 + len) of slot q
        if (len <= 0) continue;                             // (G * per can pass n by more than a stretch)
        const unsigned at = (unsigned)(j0 * Q + q), last = (unsigned)(len - 1);
        int c[LOG_STRETCH];
#pragma unroll
        for (int b = 0; b < LOG_STRETCH; b += 8) {
            if (b < per) {
#pragma unroll
                for (int i = b; i < b + 8; i++) c[i] = dlog[at + min((unsigned)i, last) * (unsigned)Q];     // byte < n * Q
            } else {
#pragma unroll
                for (int i = b; i < b + 8; i++) c[i] = 0;
            }
        }
        const int sym = qcode[q];
        if (sym >= KMAX) continue;
        unsigned* const mine = s_cnt + log_cnt_index(0, sym);
        int cur = c[0] & (MAXS - 1);                        // (a strain index: s_cnt has MAXS of them per symbol)
        unsigned run = 0;
#pragma unroll
        for (int b = 0; b < LOG_STRETCH; b += 8) {
            if (b >= per) break;                            // (uniform)
#pragma unroll
            for (int i = b; i < b + 8; i++) {
                const int ci = c[i] & (MAXS - 1);
                if (ci != cur) {
                    __hip_atomic_fetch_add(&mine[cur], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    cur = ci; run = 0;
                }
                run++;
            }
        }
        run -= (unsigned)(loaded - len);                    // the copies of the last sweep: all in the last run, which has >= 1 beside them
        __hip_atomic_fetch_add(&mine[cur], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// What the wavefronts that do NOT run the chain do meanwhile, where they may not simply end (a resident workgroup, and
// the variants behind k_level_any that it shares): an s_barrier counts every live wavefront of the workgroup, so they
// take part in exactly the barriers of urn_chain_q -- the one after the uniforms are staged, the two of every pass (the
// advance of the pass is read from s_x between them, as the chain's wavefronts read it), the one after the loop.
template <int NW>
__device__ __forceinline__ void urn_chain_shadow(const LevelHdr& h, const int* s_x) {
    const int total = h.n_sweeps * h.Q;
    __syncthreads();
    int t = 0;
#pragma unroll 1
    while (t < total) {
        lds_barrier();
        int adv = 16 * NW;
#pragma unroll
        for (int j = 0; j < NW / 4; j++) {
            const i4v xf = *(const volatile i4v*)(s_x + 4 * j);
            adv = min(adv, min(min(xf.x, xf.y), min(xf.z, xf.w)));
        }
        const int rem = total - t;
        adv = adv < rem ? adv : rem;
        if (adv == 0) adv = 1;
        t += adv;
        if (t >= total) break;
        lds_barrier();
    }
    __syncthreads();
}

// exp(y), y <= 0, as an fp32 sampler weight: y = k ln2 + r in fp64 (exact to 2^-60), exp(r) by the fp32 hardware
// exponential, scaled by 2^k.  Relative error < 3 * 2^-24 (fp32 rounding of r: 0.35 * 2^-25; of r * log2 e: 0.5 * 2^-24;
// v_exp_f32: 1 ulp; the final rounding), which the window margin EPSW budgets for; a NaN stays a NaN (it sends the
// draw to the checked tiers), anything below 2^-149 is 0 as in the rounded exact value.
__device__ __forceinline__ float exp_weight(double y) {
    if (y < -104.0) return 0.0f;                              // below the last fp32 denormal (and -inf: log 0)
    const double k = rint(y * 1.4426950408889634);
    double r = fma(k, -0.693147180559945286, y);
    r = fma(k, -2.3190468138462996e-17, r);
    const float e = __builtin_amdgcn_exp2f((float)r * 1.44269504f);
    const double kc = fmax(k, -300.0);                        // ldexpf's int: far below the last denormal is still 0
    return (y == y) ? ldexpf(e, (int)kc) : __int_as_float(0x7fc00000);
}

__host__ __device__ inline int chain_w_stride(int S) {
    const int s4 = (S + 1 + 3) & ~3;                          // S weights + one zero (the row layout the kernel kinds' LDS limits were set with)
    return (s4 & 4) ? s4 : s4 + 4;                            // 4 * odd: conflict-free 16-byte row reads
}

// wavefronts that run the chain = window of 16 * NW draws: all eight while a lane's share of the strains is
// small (the pass is latency-bound and a wider window accepts more draws), four otherwise (the others leave)
constexpr int chain_nw(int nb) { return nb <= 2 ? 8 : 4; }

}  // namespace sc
