// A sample's reads mapped to the gene database on the device (DESIGN.md §8.18 is the contract) -- what
// scripts/get_sra_and_mapping.py:49-90 runs bowtie2 --local and samtools view -F4 for.  The index is the gene profile's
// (k_seed_keys and SeedIndex of sc_profile_seed.hpp), the alignment stage 4's (sc_sw.hpp); this file holds what lies between:
//   * k_map_votes: one wavefront per read counts, per gene, the read's windows whose k-mer the gene holds, on either strand,
//     and keeps the genes the candidate rule keeps.  FILL = false counts them, FILL = true writes the (read, gene) pairs.
//   * the entry points: the reads go through the counting pass at once and through the filling pass and k_sw_score_pairs in
//     stretches whose pairs fit the room; k_sw_trace runs once over the reads that mapped.
#include <cstring>
#include <memory>

#include "sc_profile_seed.hpp"
#include "sc_sw.hpp"

namespace {

constexpr int MAP_RANGE = 8192;         // genes one pass over a read counts: a 32-bit word each, 32 KiB of LDS
constexpr int MAP_MAX_VOTES = 502;      // the windows of a 512-base read at k = 11; a half of the word holds 65 535
constexpr int MAP_HIST = 512;           // histogram bins: a vote count is its own bin
constexpr int VOTE_BLOCKS = 2048;       // workgroups of one wavefront; 42 KiB of LDS each lets three share a CU
constexpr long DEFAULT_PAIR_ROOM = 1L << 22, MAX_PAIR_ROOM = 1L << 30;
static_assert(MAP_MAX_VOTES == MAX_ROWS - SEED_MIN_K + 1 && MAP_MAX_VOTES < MAP_HIST, "a vote count is a histogram bin");

// The cut of a read: every gene with more than t votes is a candidate, and of the genes with t votes the first `keep` in gene
// order.  Without a cut (max_cand == 0, or no more genes than max_cand) t = min_votes - 1 and keep = 0.
struct Cut { int t, keep; };
enum { TALLY_WINDOWS, TALLY_SKIPPED, TALLY_CELLS, N_TALLY };
constexpr const char *VOTES = "votes", *SCORE = "score";      // the spans of a call's stream that sc_map_stats sums

// One wavefront per read of `rids`.  A lane takes a stretch of the read's windows and rolls both codes along it (the pattern
// of k_seed_lookup); the genes are gone over in ranges of MAP_RANGE, and per range the lane walks every window's run of the
// sorted keys as far as the range goes, adding to vote[gene - g0]: forward votes in the low half of the word, reverse votes
// in the high half.  The entries of a run are sorted by gene, so leaving out an entry equal to the one before it counts a
// window once per gene.  In the first range the run is found by binary search, and a run of more than max_occ entries is
// dropped (cursor -1); cursor[strand][window] then holds where the next range goes on.
// FILL = false: hist[v] counts the genes of every range with v = max(forward, reverse) >= min_votes votes; from it come cnt[s],
// the read's number of candidates, and cut[s].  tally[TALLY_WINDOWS / TALLY_SKIPPED] grow by the windows looked up and by
// those dropped.
// FILL = true: the candidates go to pairs[pair_off[s] - pair_base ...] in ascending gene order (votes[] beside them, the vote
// word, when it is not null): a lane per gene, 64 genes at a time; the genes with exactly t votes seen so far are carried
// across the groups and the ranges.  tally[TALLY_CELLS] grows by 2 * read length * gene length per pair.
template <bool FILL>
__global__ __launch_bounds__(64) void k_map_votes(const unsigned long long* keys, long n_keys, const long* gene_off, int n_genes,
                                                  const uint8_t* rd, const long* rd_off, const int* rids, int n_ids, int k, int max_occ,
                                                  int max_cand, int min_votes, unsigned* cnt, Cut* cut, unsigned long long* tally,
                                                  const long* pair_off, long pair_base, Pair* pairs, unsigned* votes) {
    __shared__ unsigned vote[MAP_RANGE];
    __shared__ long cursor[2][MAX_ROWS];
    __shared__ unsigned hist[MAP_HIST];
    const int lane = threadIdx.x;
    const unsigned mask = k == 16 ? ~0u : (1u << (2 * k)) - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long n_win = 0, n_skip = 0;
    for (int s = blockIdx.x; s < n_ids; s += gridDim.x) {
        const int read = rids[s];
        const long r0 = rd_off[read];
        const int L = (int)(rd_off[read + 1] - r0);
        const int nw = L - k + 1;                               // windows; none when the read is shorter than k
        const int per = nw > 0 ? (nw + 63) / 64 : 0;
        const int wa = lane * per, wb = min(wa + per, nw);
        const int t = FILL ? cut[s].t : 0, keep = FILL ? cut[s].keep : 0;
        const unsigned room = FILL ? cnt[s] : 0u;
        unsigned total = 0;
        int eq_seen = 0;
        long gl = 0;
        if (!FILL) for (int v = lane; v < MAP_HIST; v += 64) hist[v] = 0;
        for (int g0 = 0; g0 < n_genes; g0 += MAP_RANGE) {
            const int ng = min(n_genes - g0, MAP_RANGE);
            for (int g = lane; g < ng; g += 64) vote[g] = 0;
            __syncthreads();
            unsigned fw = 0, rc = 0;
            int run = 0;                                        // ACGT bases in a row up to here
            for (int i = wa, end = wb > wa ? wb + k - 1 : wa; i < end; i++) {
                const unsigned c = rd[r0 + i] & 15u;
                if (c >= 4u) { run = 0; continue; }
                fw = ((fw << 2) | c) & mask;
                rc = (rc >> 2) | ((3u - c) << (2 * (k - 1)));
                if (++run < k) continue;
                const int w = i - k + 1;                        // wa <= w < wb: the lane's own cursors
#pragma unroll
                for (int strand = 0; strand < 2; strand++) {
                    const unsigned code = strand ? rc : fw;
                    long at;
                    if (g0 == 0) {
                        const unsigned long long first = (unsigned long long)code << 32;
                        long lo = 0, hi = n_keys;
                        while (lo < hi) {
                            const long mid = (lo + hi) >> 1;
                            if (keys[mid] < first) lo = mid + 1; else hi = mid;
                        }
                        at = lo;
                        n_win++;
                        if (at + max_occ < n_keys && (unsigned)(keys[at + max_occ] >> 32) == code) { at = -1; n_skip++; }
                    } else {
                        at = cursor[strand][w];
                    }
                    if (at >= 0) {
                        int prev = -1;
                        for (; at < n_keys; at++) {
                            const unsigned long long key = keys[at];
                            const int g = (int)(unsigned)key - g0;
                            if ((unsigned)(key >> 32) != code || (unsigned)g >= (unsigned)ng) break;      // g < 0 cannot be: the range before ended there
                            if (g != prev) atomicAdd(&vote[g], strand ? 0x10000u : 1u);
                            prev = g;
                        }
                    }
                    cursor[strand][w] = at;
                }
            }
            __syncthreads();
            if (!FILL) {
                for (int g = lane; g < ng; g += 64) {
                    const unsigned x = vote[g];
                    const int v = (int)max(x & 0xFFFFu, x >> 16);
                    if (v >= min_votes) atomicAdd(&hist[min(v, MAP_HIST - 1)], 1u);
                }
            } else {
                for (int b = 0; b < ng; b += 64) {
                    const int g = b + lane;
                    const unsigned x = g < ng ? vote[g] : 0u;
                    const int v = (int)max(x & 0xFFFFu, x >> 16);
                    const bool eq = g < ng && v == t;
                    const unsigned long long em = __ballot(eq);
                    const bool kept = g < ng && v >= min_votes && (v > t || (eq && eq_seen + __popcll(em & below) < keep));
                    const unsigned long long km = __ballot(kept);
                    const unsigned slot = total + (unsigned)__popcll(km & below);
                    if (kept && slot < room) {
                        const long dst = pair_off[s] - pair_base + slot;
                        pairs[dst].seg = read; pairs[dst].gene = g0 + g;
                        if (votes) votes[dst] = x;
                        gl += gene_off[g0 + g + 1] - gene_off[g0 + g];
                    }
                    total += (unsigned)__popcll(km);
                    eq_seen += __popcll(em);
                }
            }
            __syncthreads();
        }
        if (!FILL) {
            unsigned mine = 0;                                  // the genes in the lane's eight bins
            for (int v = lane * (MAP_HIST / 64); v < (lane + 1) * (MAP_HIST / 64); v++) mine += hist[v];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
            if (lane == 0) {
                Cut c{min_votes - 1, 0};
                unsigned n = mine;
                if (max_cand > 0 && n > (unsigned)max_cand) {
                    unsigned above = 0;
                    for (int v = MAP_HIST - 1; v >= 0; v--) {
                        if (above + hist[v] > (unsigned)max_cand) { c.t = v; c.keep = max_cand - (int)above; break; }
                        above += hist[v];
                    }
                    n = (unsigned)max_cand;
                }
                cnt[s] = n; cut[s] = c;
            }
        } else {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) gl += __shfl_xor(gl, o);
            if (lane == 0 && gl) atomicAdd(tally + TALLY_CELLS, (unsigned long long)(2L * L * gl));
        }
        __syncthreads();
    }
    if (!FILL) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { n_win += __shfl_xor(n_win, o); n_skip += __shfl_xor(n_skip, o); }
        if (lane == 0) {
            if (n_win) atomicAdd(tally + TALLY_WINDOWS, n_win);
            if (n_skip) atomicAdd(tally + TALLY_SKIPPED, n_skip);
        }
    }
}

thread_local sc::LastError tl_error;

}  // namespace

// The handle of sc_map_index_create: the genes and their sorted keys on one device, and the arrays the calls work in, kept
// and grown from call to call.  One call at a time.
struct sc_map_index {
    int device, seed_k;
    Packed gn;
    sc::DevMem<uint8_t> d_gq;
    sc::DevMem<long> d_go;
    std::unique_ptr<SeedIndex> seeds;
    double index_ms = 0;
    sc::DevArr<uint8_t> rq;
    sc::DevArr<long> ro, poff;
    sc::DevArr<int> rids;
    sc::DevArr<unsigned> cnt, votes;
    sc::DevArr<Cut> cut;
    sc::DevArr<Pair> pairs;
    sc::DevArr<unsigned long long> best, second, tally;
    sc_map_index(int dev, int k, Packed&& genes) : device(dev), seed_k(k), gn(std::move(genes)), d_gq(gn.codes.size()), d_go(gn.off.size()) {
        sc::TimedStream st;
        st.h2d(d_gq, gn.codes); st.h2d(d_go, gn.off);
        st.mark("index");
        seeds.reset(new SeedIndex(st, d_gq.p, d_go.p, (int)gn.off.size() - 1, gn.bytes(), k));
        st.mark("indexed");
        st.sync();
        index_ms = st.ms("index", "indexed");
        seeds->trim();
        std::vector<uint8_t>().swap(gn.codes);                  // the lengths stay, the bases live on the device
    }
    int n_genes() const { return (int)gn.off.size() - 1; }
};

namespace {

// What sc_map_reads and sc_map_candidates share up to the cuts: the arguments checked, the reads packed, uploaded and taken
// through the counting pass in the order `ids`.
struct Front {
    Packed rd;
    std::vector<int> ids;
    std::vector<long> poff;                                     // pair offsets in the order of ids, [n + 1]
    uint8_t* d_rq = nullptr;
    long* d_ro = nullptr;
    int* d_ids = nullptr;
    unsigned* d_cnt = nullptr;
    Cut* d_cut = nullptr;
    unsigned long long* d_tally = nullptr;
};

int check_rule(const std::string& fn, const sc_map_index* ix, const char* read_text, const long* read_off, int n_reads, int max_occ, int max_cand,
               int min_votes, Packed& rd) {
    if (!ix || n_reads < 0 || (n_reads > 0 && (!read_text || !read_off))) return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
    if (max_occ < 1 || max_cand < 0 || min_votes < 1)
        return tl_error.fail(SC_ERR_ARG, fn + ": max_occ and min_votes must be 1 or more, max_cand 0 or more");
    std::string why;
    if (n_reads > 0 && !rd.rebase(read_off, n_reads, MAX_ROWS, fn.c_str(), "read", why)) return tl_error.fail(SC_ERR_UNSUPPORTED, why);
    return SC_OK;
}

template <bool FILL>
void launch_votes(sc::TimedStream& st, sc_map_index& ix, const Front& f, long at, int n, int max_occ, int max_cand, int min_votes, long pair_base,
                  Pair* d_pairs, unsigned* d_votes) {
    hipLaunchKernelGGL(k_map_votes<FILL>, dim3((unsigned)std::min(n, VOTE_BLOCKS)), dim3(64), 0, st, ix.seeds->sorted.p, (long)ix.seeds->n_keys,
                       ix.d_go.p, ix.n_genes(), f.d_rq, f.d_ro, f.d_ids + at, n, ix.seed_k, max_occ, max_cand, min_votes, f.d_cnt + at, f.d_cut + at,
                       f.d_tally, ix.poff.get() + at, pair_base, d_pairs, d_votes);
    st.launched();
}

// Packs and uploads the reads (rd rebased, ids set) and runs the counting pass; poff is then the scan of the counts and lies
// on the device too.  n_cand (may be null): the count of every read, by read.  The stream is synchronised.
void count_candidates(sc::TimedStream& st, sc_map_index& ix, Front& f, const char* read_text, const char* qual_text, int max_occ,
                      int max_cand, int min_votes, int* n_cand) {
    const size_t n = f.ids.size();
    f.rd.pack(read_text, [&](long k, int c) { return read_row_byte(c, qual_text, k); });
    f.d_rq = ix.rq.ensure(f.rd.codes.size());
    f.d_ro = ix.ro.ensure(n + 1);
    f.d_ids = ix.rids.ensure(n);
    f.d_cnt = ix.cnt.ensure(n);
    f.d_cut = ix.cut.ensure(n);
    f.d_tally = ix.tally.ensure(N_TALLY);
    long* d_poff = ix.poff.ensure(n + 1);
    st.h2d(f.d_rq, f.rd.codes.data(), f.rd.codes.size());
    st.h2d(f.d_ro, f.rd.off.data(), (n + 1) * sizeof(long));
    st.h2d(f.d_ids, f.ids.data(), n * sizeof(int));
    st.zero(f.d_tally, N_TALLY * sizeof(unsigned long long));
    st.span(VOTES, [&] { launch_votes<false>(st, ix, f, 0, (int)n, max_occ, max_cand, min_votes, 0, nullptr, nullptr); });
    std::vector<unsigned> cnt(n);
    st.d2h(cnt.data(), f.d_cnt, n * sizeof(unsigned));
    st.sync();
    f.poff.assign(n + 1, 0);
    for (size_t s = 0; s < n; s++) {
        f.poff[s + 1] = f.poff[s] + cnt[s];
        if (n_cand) n_cand[f.ids[s]] = (int)cnt[s];
    }
    st.h2d(d_poff, f.poff.data(), (n + 1) * sizeof(long));
}

}  // namespace

extern "C" {

const char* sc_map_error(void) { return tl_error.text.c_str(); }

int sc_map_limits(int* range_genes, int* max_votes) {
    if (range_genes) *range_genes = MAP_RANGE;
    if (max_votes) *max_votes = MAP_MAX_VOTES;
    return SC_OK;
}

int sc_map_index_create(int device, const char* gene_text, const long* gene_off, int n_genes, int seed_k, sc_map_index** out) {
    tl_error.clear();
    if (out) *out = nullptr;
    return sc::guarded(&tl_error, "sc_map_index_create", [&] {
        const std::string fn = "sc_map_index_create";
        if (!out || !gene_text || !gene_off || n_genes < 1) return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        if (seed_k < SEED_MIN_K || seed_k > SEED_MAX_K) return tl_error.fail(SC_ERR_ARG, fn + ": seed_k " + std::to_string(seed_k) + " (11..16 supported)");
        if (n_genes > MAX_SEEDS) return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": more than 1048575 genes");
        Packed gn;
        std::string why;
        if (!gn.rebase(gene_off, n_genes, MAX_COLS, fn.c_str(), "gene", why)) return tl_error.fail(SC_ERR_UNSUPPORTED, why);
        sc::select_device(device);
        gn.pack(gene_text + gene_off[0], [](long, int c) { return c < 0 ? REF_OTHER : c; });
        *out = new sc_map_index(device, seed_k, std::move(gn));
        return SC_OK;
    });
}

int sc_map_index_info(const sc_map_index* index, int* n_genes, long* gene_bases, int* seed_k, long* n_keys, double* index_ms) {
    return sc::guarded(&tl_error, "sc_map_index_info", [&] {
        if (!index) return tl_error.fail(SC_ERR_ARG, "sc_map_index_info: missing argument");
        if (n_genes) *n_genes = index->n_genes();
        if (gene_bases) *gene_bases = index->gn.bytes();
        if (seed_k) *seed_k = index->seed_k;
        if (n_keys) *n_keys = (long)index->seeds->n_keys;
        if (index_ms) *index_ms = index->index_ms;
        return SC_OK;
    });
}

void sc_map_index_free(sc_map_index* index) {
    if (!index) return;
    (void)hipSetDevice(index->device);
    delete index;
}

int sc_map_candidates(sc_map_index* index, const char* read_text, const long* read_off, int n_reads, int max_occ, int max_cand,
                      int min_votes, long* cand_off, int* cand_gene, int* cand_fw, int* cand_rc, long cap, long* n_cand) {
    tl_error.clear();
    if (n_cand) *n_cand = 0;
    return sc::guarded(&tl_error, "sc_map_candidates", [&] {
        const std::string fn = "sc_map_candidates";
        Front f;
        const int bad = check_rule(fn, index, read_text, read_off, n_reads, max_occ, max_cand, min_votes, f.rd);
        if (bad != SC_OK) return bad;
        if (!cand_off || !n_cand || cap < 0 || (cap > 0 && (!cand_gene || !cand_fw || !cand_rc))) return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        sc::select_device(index->device);
        cand_off[0] = 0;
        if (n_reads == 0) return SC_OK;
        sc_map_index& ix = *index;
        for (int r = 0; r < n_reads; r++) f.ids.push_back(r);
        sc::TimedStream st;
        count_candidates(st, ix, f, read_text + read_off[0], nullptr, max_occ, max_cand, min_votes, nullptr);
        const long total = f.poff.back();
        *n_cand = total;
        std::copy(f.poff.begin(), f.poff.end(), cand_off);
        if (total > cap) { st.sync(); return tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(total) + " candidates"); }
        if (total == 0) { st.sync(); return SC_OK; }
        Pair* d_pairs = ix.pairs.ensure((size_t)total);
        unsigned* d_votes = ix.votes.ensure((size_t)total);
        launch_votes<true>(st, ix, f, 0, n_reads, max_occ, max_cand, min_votes, 0, d_pairs, d_votes);
        std::vector<Pair> pairs((size_t)total);
        std::vector<unsigned> votes((size_t)total);
        st.d2h(pairs.data(), d_pairs, pairs.size() * sizeof(Pair));
        st.d2h(votes.data(), d_votes, votes.size() * sizeof(unsigned));
        st.sync();
        for (long p = 0; p < total; p++) {
            cand_gene[p] = pairs[(size_t)p].gene;
            cand_fw[p] = (int)(votes[(size_t)p] & 0xFFFFu);
            cand_rc[p] = (int)(votes[(size_t)p] >> 16);
        }
        return SC_OK;
    });
}

int sc_map_reads(sc_map_index* index, const char* read_text, const char* qual_text, const long* read_off, int n_reads, int max_occ,
                 int max_cand, int min_votes, long pair_room, int* as, int* xs, int* gene, int* strand, int* pos, int* nm,
                 unsigned* cigar, int cigar_stride, int* n_cigar, int* n_cand, sc_map_stats* stats) {
    tl_error.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    return sc::guarded(&tl_error, "sc_map_reads", [&] {
        const std::string fn = "sc_map_reads";
        Front f;
        const int bad = check_rule(fn, index, read_text, read_off, n_reads, max_occ, max_cand, min_votes, f.rd);
        if (bad != SC_OK) return bad;
        if (!as || !xs || !gene || !strand || !pos || !nm || !cigar || cigar_stride < 1 || !n_cigar || !n_cand || pair_room < 0)
            return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        long max_len = 0;
        for (int r = 0; r < n_reads; r++) max_len = std::max(max_len, f.rd.len(r));
        if (cigar_stride < max_len / 2 + 4) return tl_error.fail(SC_ERR_CAPACITY, fn + ": cigar_stride below max read length / 2 + 4");
        sc::select_device(index->device);
        if (n_reads == 0) return SC_OK;
        const double t0 = sc::now_ms();
        sc_map_index& ix = *index;
        const long room = pair_room > 0 ? std::min(pair_room, MAX_PAIR_ROOM) : DEFAULT_PAIR_ROOM;
        // ---- the reads bucketed by rows per lane, so that a stretch's pairs lie bucket by bucket; the counting pass
        Buckets by_r;
        for (int r = 0; r < n_reads; r++) by_r.add(r, f.rd.len(r));
        f.ids = by_r.order();
        sc::TimedStream st;
        count_candidates(st, ix, f, read_text + read_off[0], qual_text ? qual_text + read_off[0] : nullptr, max_occ, max_cand, min_votes,
                         n_cand);
        unsigned long long* d_best = ix.best.ensure((size_t)n_reads);
        unsigned long long* d_second = ix.second.ensure((size_t)n_reads);
        st.zero(d_best, (size_t)n_reads * 8);
        st.zero(d_second, (size_t)n_reads * 8);
        // ---- the stretches: whole reads while their pairs fit the room, a read that needs more alone
        std::vector<long> cuts{0};
        long most = 0;
        for (long a = 0; a < n_reads;) {
            long b = a + 1;
            while (b < n_reads && f.poff[(size_t)b + 1] - f.poff[(size_t)a] <= room) b++;
            most = std::max(most, f.poff[(size_t)b] - f.poff[(size_t)a]);
            cuts.push_back(b);
            a = b;
        }
        Pair* d_pairs = ix.pairs.ensure((size_t)std::max(most, 1L));
        for (size_t c = 0; c + 1 < cuts.size(); c++) {
            const long a = cuts[c], b = cuts[c + 1], base = f.poff[(size_t)a];
            if (f.poff[(size_t)b] == base) continue;
            st.span(VOTES, [&] { launch_votes<true>(st, ix, f, a, (int)(b - a), max_occ, max_cand, min_votes, base, d_pairs, nullptr); });
            st.span(SCORE, [&] {
                by_r.each([&](auto r, long at, const std::vector<int>& ids) {
                    const long lo = std::max(a, at), hi = std::min(b, at + (long)ids.size());
                    if (lo >= hi) return;
                    const long n_tiles = 2L * (f.poff[(size_t)hi] - f.poff[(size_t)lo]);
                    if (n_tiles == 0) return;
                    hipLaunchKernelGGL(k_sw_score_pairs<decltype(r)::value>, score_grid(n_tiles), dim3(64 * SCORE_WAVES), 0, st, ix.d_gq.p, ix.d_go.p,
                                       f.d_rq, f.d_ro, PairTiles{d_pairs + (f.poff[(size_t)lo] - base)}, n_tiles, d_best, d_second);
                    st.launched();
                });
            });
        }
        std::vector<unsigned long long> best((size_t)n_reads), second((size_t)n_reads), tally(N_TALLY);
        st.d2h(best.data(), d_best, best.size() * 8); st.d2h(second.data(), d_second, second.size() * 8);
        st.d2h(tally.data(), f.d_tally, tally.size() * 8);
        st.sync();
        // ---- which reads map; the traceback of those
        const int n_tr = trace_aligned(st, ix.d_gq.p, ix.d_go.p, f.d_rq, f.d_ro, d_best, f.rd, best, second, as, xs, gene, strand, pos, nm, cigar,
                                       cigar_stride, n_cigar, stats ? &stats->trace_cells : nullptr);
        int rc = SC_OK;
        if (n_tr < 0) rc = tl_error.fail(SC_ERR_INTERNAL, fn + ": traceback of read " + std::to_string(-1 - n_tr) + " failed");
        if (stats && rc == SC_OK) {
            stats->index_ms = ix.index_ms;
            stats->votes_ms = st.span_ms(VOTES);
            stats->score_ms = st.span_ms(SCORE);
            stats->trace_ms = st.ms("trace", "traced");
            stats->n_keys = (long)ix.seeds->n_keys;
            stats->n_windows = (long)tally[TALLY_WINDOWS];
            stats->n_skipped = (long)tally[TALLY_SKIPPED];
            stats->n_pairs = f.poff.back();
            stats->score_cells = (long)tally[TALLY_CELLS];
            stats->n_traced = n_tr;
            stats->n_stretches = (long)cuts.size() - 1;
        }
        if (stats) stats->total_ms = sc::now_ms() - t0;
        return rc;
    });
}

}  // extern "C"
