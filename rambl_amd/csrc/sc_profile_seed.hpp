// The seeded mode of the gene profile (sc_profile_hits_seeded and sc_profile_counts with `seeded`):
// k_seed_keys and a radix sort index the genes' k-mers, k_seed_lookup lists the (segment, gene) pairs that share one on
// either strand, and the score pass runs k_bl_score_pairs over those pairs only.  k is the host's bound seed_length(): no
// hit that passes both thresholds is without a common k-mer, so the hits are the unseeded ones.
#pragma once
#include <rocprim/rocprim.hpp>

#include "sc_profile_dp.hpp"

namespace {

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
inline int seed_length(const bool* has_len, long gene_bases, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* lossless) {
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
    // Once the stream was synchronised only `sorted` is read: an index that is kept lets the unsorted keys and the sort's
    // temporary go.
    void trim() {
        { sc::DevMem<unsigned long long> none(0); std::swap(none.p, keys.p); }
        { sc::DevMem<uint8_t> none(0); std::swap(none.p, tmp.p); }
    }
};

// What seed_pairs sets aside on the device, kept by its owner from one score pass to the next: the per-segment counts and
// offsets and the pair list.
struct SeedScratch {
    sc::DevArr<unsigned> cnt;
    sc::DevArr<long> glen, poff;
    sc::DevArr<Pair> pairs;
};

// The (segment, gene) pairs of the bucketed segments `sids` (d_sids on the device) that share a k-mer of the index: counted
// per segment, scanned on the host into pair_off[sids.size() + 1], and -- unless their tiles are more than one call takes --
// filled into sx.pairs in bucket order, genes ascending.  *score_cells (may be null) grows by 2 * segment length * gene length
// per pair.  Returns the number of pairs; the stream is synchronised.
inline long seed_pairs(sc::TimedStream& st, const SeedIndex& index, const long* d_go, int n_genes, const uint8_t* d_sq, const long* d_so,
                const Packed& sg, const Buckets& by_r, const std::vector<int>& sids, const int* d_sids, int seed_k, std::vector<long>& pair_off,
                SeedScratch& sx, long* score_cells) {
    unsigned* d_cnt = sx.cnt.ensure(sids.size() + 1);
    long* d_glen = sx.glen.ensure(sids.size() + 1);
    long* d_poff = sx.poff.ensure(pair_off.size());
    Pair* d_pairs = sx.pairs.get();
    const auto lookup = [&](auto fill) {
        by_r.each([&](auto, long at, const std::vector<int>& ids) {
            hipLaunchKernelGGL(k_seed_lookup<decltype(fill)::value>, dim3((unsigned)std::min<size_t>(ids.size(), LOOKUP_BLOCKS)), dim3(64), 0, st,
                               index.sorted.p, (long)index.n_keys, d_go, n_genes, d_sq, d_so, d_sids + at, (int)ids.size(), seed_k,
                               d_cnt + at, d_glen + at, d_poff + at, d_pairs);
            st.launched();
        });
    };
    lookup(std::false_type{});
    std::vector<unsigned> cnt(sids.size());
    std::vector<long> glen(sids.size());
    st.d2h(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned)); st.d2h(glen.data(), d_glen, glen.size() * sizeof(long));
    st.sync();
    for (size_t k = 0; k < sids.size(); k++) {
        pair_off[k + 1] = pair_off[k] + cnt[k];
        if (score_cells) *score_cells += 2L * sg.len(sids[k]) * glen[k];
    }
    const long n_pairs = pair_off.back();
    if (2L * n_pairs > 0x7FFFFFFFL || n_pairs == 0) return n_pairs;
    d_pairs = sx.pairs.ensure((size_t)n_pairs);
    st.h2d(d_poff, pair_off.data(), pair_off.size() * sizeof(long));
    lookup(std::true_type{});
    st.sync();                                                  // pair_off goes with the caller's scope
    return n_pairs;
}

}  // namespace
