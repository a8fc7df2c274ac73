// Gene against gene on the device (DESIGN.md §8.16 is the contract): the exact unit-cost edit distance of whole sequences by
// the Myers / Hyyrö block bit-vector recurrence, one lane per pair.  The word arithmetic is sc_pairs_core.hpp's.
//   k_pairs<W>   one wavefront per tile: a pattern gene of at most 64 W bases, its match masks in LDS, and up to 64 text genes,
//                one per lane, each streamed a dword (eight codes) at a time.  Writes every distance (sc_gene_distances) or
//                appends the pairs within the bound to a list (sc_gene_pairs).
#include <climits>
#include <numeric>

#include "../../include/straincall_hip.h"
#include "sc_host.hpp"
#include "sc_pairs_core.hpp"

namespace {

using namespace sc_pairs;

constexpr int TILE_LANES = 64;
constexpr int PAIRS_BLOCKS = 4096;                 // blocks of a launch at most: more tiles go round the grid-stride loop

thread_local sc::LastError tl_error;

// A tile: the pattern gene and `count` (1..64) texts.  With a text list the texts are text_of[first .. first + count), without
// one they are the genes first .. first + count - 1 themselves.
struct Tile { int pattern, first, count; };

// What a launch reads and writes.  Genes are packed codes: gene g holds len[g] codes from dword dw_off[g] of `codes`.
struct PairArgs {
    const uint32_t* codes;
    const long* dw_off;
    const int* len;
    const Tile* tiles;
    int n_tiles;
    const int* text_of;          // null: a tile's texts are consecutive genes
    int* dist;                   // distances mode: dist[first + lane]
    long diff_num, diff_den;     // list mode (diff_den > 0): keep the pairs with ed <= bound
    int* out_a; int* out_b; int* out_d;
    unsigned long long* n_out;   // pairs within the bound, whether or not they found room
    long room;
};

template <int W>
__global__ __launch_bounds__(TILE_LANES) void k_pairs(PairArgs a) {
    __shared__ uint64_t peq[N_CODES * W];
    const int lane = threadIdx.x;
    for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const Tile tile = a.tiles[t];
        const int m = a.len[tile.pattern];
        const uint32_t* pat = a.codes + a.dw_off[tile.pattern];
        const long pat_dw = packed_dwords(m);
        const int last_word = (m - 1) / 64, last_bit = (m - 1) % 64;
        __syncthreads();                                        // the last trip's lanes are done with the masks
        for (int i = lane; i < N_CODES * W; i += TILE_LANES) {
            const int c = i / W, w = i - c * W;
            peq[i] = (c < 4 && w <= last_word) ? match_word(pat, pat_dw, w, (unsigned)c) : 0;
        }
        __syncthreads();
        if (lane < tile.count) {
            const int slot = tile.first + lane;
            const int g = a.text_of ? a.text_of[slot] : slot;
            const int n = a.len[g];
            const uint32_t* text = a.codes + a.dw_off[g];
            uint64_t pv[W], mv[W];
#pragma unroll
            for (int w = 0; w < W; w++) { pv[w] = ~(uint64_t)0; mv[w] = 0; }
            int score = m;
            for (int j0 = 0; j0 < n; j0 += CODES_PER_DWORD) {
                uint32_t x = text[j0 / CODES_PER_DWORD];
                const int cols = min(CODES_PER_DWORD, n - j0);
#pragma unroll 1
                for (int k = 0; k < cols; k++, x >>= 4) {
                    const uint64_t* row = peq + (x & 15u) * W;          // codes are 0..4 by construction (pack_codes)
                    score += column_step<W>(row, pv, mv, last_word, last_bit);
                }
            }
            if (a.diff_den > 0) {
                if ((long)score <= pair_bound(m, n, a.diff_num, a.diff_den)) {
                    const unsigned long long at = atomicAdd(a.n_out, 1ull);
                    if ((long)at < a.room) { a.out_a[at] = tile.pattern; a.out_b[at] = g; a.out_d[at] = score; }
                }
            } else {
                a.dist[slot] = score;
            }
        }
    }
}

template <int W> void launch(const PairArgs& a, hipStream_t st) {
    if (a.n_tiles == 0) return;
    hipLaunchKernelGGL(k_pairs<W>, dim3((unsigned)std::min(a.n_tiles, PAIRS_BLOCKS)), dim3(TILE_LANES), 0, st, a);
}
using Launch = void (*)(const PairArgs&, hipStream_t);
constexpr Launch LAUNCH[N_WIDTHS] = {launch<WIDTHS[0]>, launch<WIDTHS[1]>, launch<WIDTHS[2]>, launch<WIDTHS[3]>};

// The genes of a call as the kernel reads them; `order` lists the genes in the order they are packed.
struct Packed {
    std::vector<uint32_t> codes;
    std::vector<long> dw_off;
    std::vector<int> len;
};

// Checks the lengths (message in tl_error) and packs gene order[k] as gene k.  Returns SC_OK or the error.
int pack_genes(const std::string& fn, const char* gene_text, const long* gene_off, int n_genes, const std::vector<int>& order, Packed& out) {
    for (int g = 0; g < n_genes; g++) {
        const long len = gene_off[g + 1] - gene_off[g];
        if (len < 1) return tl_error.fail(SC_ERR_ARG, fn + ": gene " + std::to_string(g) + " is empty");
        if (len > MAX_LEN)
            return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": gene " + std::to_string(g) + " has " + std::to_string(len) + " bases (1.." + std::to_string(MAX_LEN) +
                                                         " supported)");
    }
    out.dw_off.assign((size_t)n_genes + 1, 0);
    out.len.resize((size_t)n_genes);
    for (int k = 0; k < n_genes; k++) {
        out.len[(size_t)k] = (int)(gene_off[order[(size_t)k] + 1] - gene_off[order[(size_t)k]]);
        out.dw_off[(size_t)k + 1] = out.dw_off[(size_t)k] + packed_dwords(out.len[(size_t)k]);
    }
    out.codes.resize((size_t)out.dw_off.back());
    for (int k = 0; k < n_genes; k++) pack_codes(gene_text + gene_off[order[(size_t)k]], out.len[(size_t)k], out.codes.data() + out.dw_off[(size_t)k]);
    return SC_OK;
}

struct Stat { double v[SC_PAIRS_N_STATS] = {}; };

// The tiles of every width class, class after class; class_first[k] .. class_first[k + 1] are class k's.
struct Tiles {
    std::vector<Tile> list;
    int class_first[N_WIDTHS + 1] = {};
};

// The genes and tiles of a call on the device: uploaded once, launched class after class.
struct Device {
    sc::DevMem<uint32_t> codes;
    sc::DevMem<long> dw_off;
    sc::DevMem<int> len;
    sc::DevMem<Tile> tiles;
    Device(const Packed& p, const Tiles& t) : codes(p.codes.size()), dw_off(p.dw_off.size()), len(p.len.size()), tiles(t.list.size()) {}
    void upload(sc::TimedStream& st, const Packed& p, const Tiles& t) {
        st.h2d(codes, p.codes); st.h2d(dw_off, p.dw_off); st.h2d(len, p.len); st.h2d(tiles, t.list);
    }
    void run(sc::TimedStream& st, const Tiles& t, PairArgs a) {
        a.codes = codes.p; a.dw_off = dw_off.p; a.len = len.p;
        for (int k = 0; k < N_WIDTHS; k++) {
            a.tiles = tiles.p + t.class_first[k];
            a.n_tiles = t.class_first[k + 1] - t.class_first[k];
            LAUNCH[k](a, st);
            st.launched();
        }
    }
};

void hand_stats(const Stat& all, double* stats, int n_stats) {
    for (int k = 0; stats && k < n_stats && k < SC_PAIRS_N_STATS; k++) stats[k] = all.v[k];
}

}  // namespace

extern "C" {

const char* sc_pairs_error(void) { return tl_error.text.c_str(); }

int sc_pairs_widths(int* widths, int cap) {
    for (int k = 0; widths && k < cap && k < N_WIDTHS; k++) widths[k] = WIDTHS[k];
    return N_WIDTHS;
}

int sc_gene_distances(int device, const char* gene_text, const long* gene_off, int n_genes, const int* pair_a, const int* pair_b, long n_pairs,
                      int* dist_out, double* stats_out, int n_stats) {
    Stat stats;
    tl_error.clear();
    const int rc = sc::guarded(&tl_error, "sc_gene_distances", [&] {
        const std::string fn = "sc_gene_distances";
        if (n_genes < 0 || n_pairs < 0 || (n_genes > 0 && (!gene_text || !gene_off)) || (n_pairs > 0 && (!pair_a || !pair_b || !dist_out)))
            return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        if (n_pairs > INT_MAX - TILE_LANES) return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_pairs) + " pairs in one call");
        const double t0 = sc::now_ms();
        std::vector<int> order((size_t)n_genes);
        std::iota(order.begin(), order.end(), 0);
        Packed packed;
        if (int rc = pack_genes(fn, gene_text, gene_off, n_genes, order, packed)) return rc;
        for (long p = 0; p < n_pairs; p++)
            if (pair_a[p] < 0 || pair_a[p] >= n_genes || pair_b[p] < 0 || pair_b[p] >= n_genes)
                return tl_error.fail(SC_ERR_ARG, fn + ": pair " + std::to_string(p) + " names a gene outside 0.." + std::to_string(n_genes - 1));
        if (n_pairs == 0) return SC_OK;
        // the pairs grouped by (width class of the pattern, pattern), in the caller's order inside a group
        std::vector<int> by_tile((size_t)n_pairs);
        std::iota(by_tile.begin(), by_tile.end(), 0);
        auto cls = [&](int p) { return width_class(packed.len[(size_t)pair_a[p]]); };
        std::stable_sort(by_tile.begin(), by_tile.end(), [&](int x, int y) {
            return cls(x) != cls(y) ? cls(x) < cls(y) : pair_a[x] < pair_a[y];
        });
        Tiles tiles;
        std::vector<int> text_of((size_t)n_pairs);
        long word_steps = 0;
        for (long s = 0; s < n_pairs; s++) {
            const int p = by_tile[(size_t)s], pat = pair_a[p];
            text_of[(size_t)s] = pair_b[p];
            word_steps += (long)packed.len[(size_t)pair_b[p]] * ((packed.len[(size_t)pat] + 63) / 64);
            if (tiles.list.empty() || tiles.list.back().pattern != pat || tiles.list.back().count == TILE_LANES) {
                tiles.list.push_back(Tile{pat, (int)s, 0});
                tiles.class_first[cls(p) + 1]++;
            }
            tiles.list.back().count++;
        }
        for (int k = 0; k < N_WIDTHS; k++) tiles.class_first[k + 1] += tiles.class_first[k];
        sc::select_device(device);
        Device dev(packed, tiles);
        sc::DevMem<int> d_text_of(text_of.size()), d_dist((size_t)n_pairs);
        std::vector<int> dist((size_t)n_pairs);
        sc::TimedStream st;
        st.mark("upload");
        dev.upload(st, packed, tiles);
        st.h2d(d_text_of, text_of);
        st.mark("score");
        PairArgs a = {};
        a.text_of = d_text_of.p; a.dist = d_dist.p;
        dev.run(st, tiles, a);
        st.mark("scored");
        st.d2h(dist, d_dist);
        st.sync();
        for (long s = 0; s < n_pairs; s++) dist_out[by_tile[(size_t)s]] = dist[(size_t)s];
        stats.v[SC_PAIRS_STAT_UPLOAD_MS] = st.ms("upload", "score"); stats.v[SC_PAIRS_STAT_KERNEL_MS] = st.ms("score", "scored");
        stats.v[SC_PAIRS_STAT_TILES] = (double)tiles.list.size(); stats.v[SC_PAIRS_STAT_PAIRS_SCORED] = (double)n_pairs;
        stats.v[SC_PAIRS_STAT_WORD_STEPS] = (double)word_steps;
        stats.v[SC_PAIRS_STAT_TOTAL_MS] = sc::now_ms() - t0;
        return SC_OK;
    });
    hand_stats(stats, stats_out, n_stats);
    return rc;
}

int sc_gene_pairs(int device, const char* gene_text, const long* gene_off, int n_genes, int diff_num, int diff_den, int* pair_a, int* pair_b,
                  int* pair_dist, long cap, long* n_pairs, double* stats_out, int n_stats) {
    Stat stats;
    tl_error.clear();
    const int rc = sc::guarded(&tl_error, "sc_gene_pairs", [&] {
        const std::string fn = "sc_gene_pairs";
        if (!n_pairs || n_genes < 0 || cap < 0 || (n_genes > 0 && (!gene_text || !gene_off)) || (cap > 0 && (!pair_a || !pair_b || !pair_dist)))
            return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        *n_pairs = 0;
        if (diff_den < 1 || diff_num < 0 || diff_num > diff_den)
            return tl_error.fail(SC_ERR_ARG, fn + ": the difference rate " + std::to_string(diff_num) + " / " + std::to_string(diff_den) + " is outside 0..1");
        const double t0 = sc::now_ms();
        // by (length, index): a pattern's candidates, the longer genes within the length bound, are then one range behind it
        std::vector<int> order((size_t)n_genes);
        std::iota(order.begin(), order.end(), 0);
        {
            std::vector<long> len((size_t)n_genes);
            for (int g = 0; g < n_genes; g++) len[(size_t)g] = gene_off[g + 1] - gene_off[g];
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len[(size_t)x] < len[(size_t)y]; });
        }
        Packed packed;
        if (int rc = pack_genes(fn, gene_text, gene_off, n_genes, order, packed)) return rc;
        // len - bound(len) does not fall as len grows (diff_num <= diff_den), so the end of the range moves forward only
        Tiles tiles;
        long n_cand = 0, word_steps = 0;
        std::vector<long> len_sum((size_t)n_genes + 1, 0);
        for (int g = 0; g < n_genes; g++) len_sum[(size_t)g + 1] = len_sum[(size_t)g] + packed.len[(size_t)g];
        std::vector<Tile> per_class[N_WIDTHS];
        for (int i = 0, end = 0; i < n_genes; i++) {
            const long li = packed.len[(size_t)i];
            end = std::max(end, i + 1);
            while (end < n_genes && packed.len[(size_t)end] - li <= pair_bound(li, packed.len[(size_t)end], diff_num, diff_den)) end++;
            n_cand += end - (i + 1);
            word_steps += (len_sum[(size_t)end] - len_sum[(size_t)i + 1]) * ((li + 63) / 64);
            for (int f = i + 1; f < end; f += TILE_LANES) per_class[width_class(li)].push_back(Tile{i, f, std::min(TILE_LANES, end - f)});
        }
        for (int k = 0; k < N_WIDTHS; k++) {
            tiles.list.insert(tiles.list.end(), per_class[k].begin(), per_class[k].end());
            tiles.class_first[k + 1] = (int)tiles.list.size();
        }
        const long all_pairs = (long)n_genes * (n_genes - 1) / 2;
        stats.v[SC_PAIRS_STAT_TILES] = (double)tiles.list.size(); stats.v[SC_PAIRS_STAT_PAIRS_SCORED] = (double)n_cand;
        stats.v[SC_PAIRS_STAT_PAIRS_SKIPPED] = (double)(all_pairs - n_cand); stats.v[SC_PAIRS_STAT_WORD_STEPS] = (double)word_steps;
        if (n_cand == 0) { stats.v[SC_PAIRS_STAT_TOTAL_MS] = sc::now_ms() - t0; return SC_OK; }
        sc::select_device(device);
        Device dev(packed, tiles);
        sc::DevMem<unsigned long long> d_n(1);
        sc::TimedStream st;
        st.mark("upload");
        dev.upload(st, packed, tiles);
        st.mark("score");
        // the list is compacted on the device into the room the caller has: a pair that finds none is still counted, and the call
        // then answers with the count alone
        const long room = std::min(n_cand, cap);
        sc::DevMem<int> d_a((size_t)room), d_b((size_t)room), d_d((size_t)room);
        st.zero(d_n.p, sizeof(unsigned long long));
        PairArgs a = {};
        a.diff_num = diff_num; a.diff_den = diff_den; a.out_a = d_a.p; a.out_b = d_b.p; a.out_d = d_d.p; a.n_out = d_n.p; a.room = room;
        dev.run(st, tiles, a);
        st.mark("scored");
        unsigned long long n_found = 0;
        st.d2h(&n_found, d_n.p, sizeof n_found);
        st.sync();
        const long found = (long)n_found, kept = std::min(found, room);
        std::vector<int> a_s((size_t)kept), b_s((size_t)kept), d_s((size_t)kept);
        st.d2h(a_s.data(), d_a.p, (size_t)kept * sizeof(int)); st.d2h(b_s.data(), d_b.p, (size_t)kept * sizeof(int));
        st.d2h(d_s.data(), d_d.p, (size_t)kept * sizeof(int));
        st.sync();
        stats.v[SC_PAIRS_STAT_UPLOAD_MS] = st.ms("upload", "score"); stats.v[SC_PAIRS_STAT_KERNEL_MS] = st.ms("score", "scored");
        *n_pairs = found;
        if (found > cap) {
            stats.v[SC_PAIRS_STAT_TOTAL_MS] = sc::now_ms() - t0;
            return tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(found) + " pairs, room for " + std::to_string(cap));
        }
        // back to the caller's indices, a < b, sorted by (a, b): the order the lanes appended in does not show
        struct Rec { int a, b, d; };
        std::vector<Rec> recs((size_t)found);
        for (long k = 0; k < found; k++) {
            const int x = order[(size_t)a_s[(size_t)k]], y = order[(size_t)b_s[(size_t)k]];
            recs[(size_t)k] = Rec{std::min(x, y), std::max(x, y), d_s[(size_t)k]};
        }
        std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
        for (long k = 0; k < found; k++) { pair_a[k] = recs[(size_t)k].a; pair_b[k] = recs[(size_t)k].b; pair_dist[k] = recs[(size_t)k].d; }
        stats.v[SC_PAIRS_STAT_TOTAL_MS] = sc::now_ms() - t0;
        return SC_OK;
    });
    hand_stats(stats, stats_out, n_stats);
    return rc;
}

}  // extern "C"
