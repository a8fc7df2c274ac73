// The counts mode of the gene profile (sc_profile_counts): after the score pass of sc_profile.hip the strand
// pick, the order of a read's pairs by their six-digit E-value, rounds of k_bl_trace over each unresolved read's best group
// only, and the counting rule all stay on the device (k_cnt_*, rocprim sorts); the distinct (gene, times, share) triples come
// back.  Included by sc_profile.hip below its front end (ProfileInput) and score pass (ScorePass), which the body here uses.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "sc_profile_seed.hpp"

namespace {

constexpr int COUNT_ROUNDS = 3;         // rounds that trace one E6 group per unresolved read; then the rest at once.  A guess.
constexpr long COUNT_ROOM = 1L << 23;   // candidate records on the device at a time unless the caller says otherwise
constexpr int REC_BLOCKS = 256, READ_BLOCKS = 8192;     // grids: 256 threads a record each / one wavefront a read each
constexpr int N_BUCKETS = MAX_ROWS / 64;
constexpr int MAX_SAMPLES = 65536;      // of one call on an index
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
// triple[].  times[] is a word of room per record: a lane reads back only what it wrote itself.  With read_sample (the sample
// of every read of the call; read r of the stretch is read0 + r there) the read's sample goes to triple_sample[] beside each
// of its triples.
__global__ __launch_bounds__(64) void k_cnt_count(const unsigned long long* key2, const unsigned char* state, const Cand* hit, int n_reads,
                                                  const int* cursor, const int* end, const unsigned char* resolved, int gene_bits,
                                                  int times_bits, int* times, unsigned long long* triple, unsigned long long* ctr,
                                                  const int* read_sample, int read0, int* triple_sample) {
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
        const int sample = read_sample ? read_sample[read0 + r] : 0;
        for (int j0 = c; j0 < g; j0 += 64) {
            const int j = j0 + lane;
            const bool mine = j < g && times[j] == most;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                const unsigned long long at = base + lanes_below(m, lane);
                triple[at] = ((unsigned long long)(hit[j].gene2 >> 1) << (gene_bits + times_bits)) | ((unsigned long long)most << gene_bits) |
                             (unsigned long long)share;
                if (read_sample) triple_sample[at] = sample;
            }
            base += __popcll(m);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host

// E6: an E-value as the hit CSV holds it, six significant digits, read back.
double evalue6_of(double e) {
    char text[40];
    std::snprintf(text, sizeof text, "%.6g", e);
    return std::strtod(text, nullptr);
}

int bits_of(long v) { int b = 0; while (v >> b) b++; return b; }

// Per segment length that can pass (len_slot[L]: its row) and per doubled score from the least passing one on, the dense rank
// of E6 among all (length, score) of the call -- E and E6 by the expressions of the contract, E6 <= T or no rank.
struct RankTable { std::vector<int> len_slot; std::vector<unsigned> rank; };
RankTable rank_table(const ProfileInput& in) {
    RankTable t{std::vector<int>(MAX_ROWS + 1, 0), {}};
    std::vector<double> e6s;                                    // of every (L, s2) the table holds, in the order of the loop below
    int n_lens = 0;
    for (int L = 1; L <= MAX_ROWS; L++) {
        if (!in.has_len[L]) continue;
        t.len_slot[(size_t)L] = n_lens++;
        for (int s2 = in.min2_of_len[L]; s2 <= MATCH2 * L; s2++) e6s.push_back(evalue6_of(evalue_of(in.ka_k, in.ka_lambda, L, in.gene_bytes, s2)));
    }
    std::vector<double> distinct;
    for (double e6 : e6s) if (e6 <= in.max_evalue) distinct.push_back(e6);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    t.rank.assign((size_t)std::max(n_lens, 1) * RANK_COLS, NO_RANK);
    size_t k = 0;
    for (int L = 1; L <= MAX_ROWS; L++) {
        if (!in.has_len[L]) continue;
        for (int s2 = in.min2_of_len[L]; s2 <= MATCH2 * L; s2++) {
            const double e6 = e6s[k++];
            if (e6 <= in.max_evalue)
                t.rank[(size_t)t.len_slot[(size_t)L] * RANK_COLS + s2] = (unsigned)(std::lower_bound(distinct.begin(), distinct.end(), e6) - distinct.begin());
        }
    }
    return t;
}

// The segments by read: read r has segments by_read[read_segs[r] .. read_segs[r + 1]), in the order given.
struct ReadSegs {
    std::vector<int> read_segs, by_read;
    int most_segs = 0;                                          // in one read
    ReadSegs(const int* seg_read, int n_segs, int n_reads) : read_segs((size_t)n_reads + 1, 0), by_read((size_t)n_segs) {
        for (int r = 0; r < n_segs; r++) read_segs[(size_t)seg_read[r] + 1]++;
        for (int r = 0; r < n_reads; r++) { most_segs = std::max(most_segs, read_segs[(size_t)r + 1]); read_segs[(size_t)r + 1] += read_segs[(size_t)r]; }
        std::vector<int> at(read_segs.begin(), read_segs.end() - 1);
        for (int r = 0; r < n_segs; r++) by_read[(size_t)at[(size_t)seg_read[r]]++] = r;
    }
    // the passable segments of reads [read0, read1), bucketed
    Buckets buckets(const ProfileInput& in, int read0, int read1) const {
        Buckets by_r;
        for (int k = read_segs[(size_t)read0]; k < read_segs[(size_t)read1]; k++)
            if (in.can_pass(by_read[(size_t)k])) by_r.add(by_read[(size_t)k], in.sg.len(by_read[(size_t)k]));
        return by_r;
    }
};

// The stretches: whole reads in read order while their segments' tiles fit the candidate room asked for.  room: the most
// tiles of one stretch (a read alone gets what it needs).
struct Stretch { int read0, read1; long tiles; };
struct StretchPlan { std::vector<Stretch> stretches; long room = 0; };
StretchPlan plan_stretches(const ProfileInput& in, const ReadSegs& rs, int n_reads, long room_asked) {
    StretchPlan plan;
    Stretch cur{0, 0, 0};
    for (int r = 0; r < n_reads; r++) {
        long tiles = 0;
        for (int k = rs.read_segs[(size_t)r]; k < rs.read_segs[(size_t)r + 1]; k++)
            if (in.can_pass(rs.by_read[(size_t)k])) tiles += 2L * in.n_genes;
        if (cur.tiles > 0 && cur.tiles + tiles > room_asked) { plan.stretches.push_back(cur); cur = Stretch{r, r, 0}; }
        cur.read1 = r + 1; cur.tiles += tiles;
        plan.room = std::max(plan.room, cur.tiles);
    }
    if (cur.tiles > 0) plan.stretches.push_back(cur);
    return plan;
}

// What a counts call keeps on the device besides its input, set aside once per call -- or, for a call on an index, taken from
// the index's CountArena, which grows when a call needs more and is kept otherwise; upload() enqueues the copies.
struct CountArena {
    sc::DevArr<int> read, slot, sample;
    sc::DevArr<unsigned> rank, ncand;
    sc::DevArr<unsigned long long> ctr;
    sc::DevArr<long> part;
    sc::DevArr<Cand> cand;
};
struct CountTables {
    template <class T> using Ref = ProfileInput::Ref<T>;
    Ref<int> read, slot;                                        // seg_read[], len_slot[]
    Ref<int> sample;                                            // read_sample[]; null for a call that has no samples
    Ref<unsigned> rank, ncand;
    Ref<unsigned long long> ctr;                                // C_WORDS counters, zeroed per stretch
    Ref<long> part;
    Ref<Cand> cand;                                             // the candidate room
    struct Own {
        sc::DevMem<int> read, slot;
        sc::DevMem<unsigned> rank, ncand;
        sc::DevMem<unsigned long long> ctr;
        sc::DevMem<long> part;
        sc::DevMem<Cand> cand;
        Own(int n_segs, const RankTable& t, long room)
            : read((size_t)n_segs), slot(t.len_slot.size()), rank(t.rank.size()), ncand(1), ctr(C_WORDS), part(N_BUCKETS), cand((size_t)room) {}
    };
    std::unique_ptr<Own> own;
    CountTables(int n_segs, const RankTable& t, long room) : own(new Own(n_segs, t, room)) {
        read.p = own->read.p; slot.p = own->slot.p; rank.p = own->rank.p; ncand.p = own->ncand.p; ctr.p = own->ctr.p; part.p = own->part.p;
        cand.p = own->cand.p;
    }
    CountTables(CountArena& a, int n_segs, int n_reads, const RankTable& t, long room) {
        read.p = a.read.ensure((size_t)n_segs); slot.p = a.slot.ensure(t.len_slot.size()); sample.p = a.sample.ensure((size_t)n_reads);
        rank.p = a.rank.ensure(t.rank.size()); ncand.p = a.ncand.ensure(1); ctr.p = a.ctr.ensure(C_WORDS); part.p = a.part.ensure(N_BUCKETS);
        cand.p = a.cand.ensure((size_t)room);
    }
    void upload(sc::TimedStream& st, const int* seg_read, int n_segs, const RankTable& t, const int* read_sample, int n_reads) {
        st.h2d(read.p, seg_read, (size_t)n_segs * sizeof(int)); st.h2d(slot.p, t.len_slot.data(), t.len_slot.size() * sizeof(int));
        st.h2d(rank.p, t.rank.data(), t.rank.size() * sizeof(unsigned));
        if (sample.p) st.h2d(sample.p, read_sample, (size_t)n_reads * sizeof(int));
    }
};

// The per-stretch arrays, grown to the largest stretch: per candidate record (k1 .. hits), per hit (state .. trips), per read
// of the stretch (first .. resolved).
struct CountBufs {
    sc::DevArr<int> sids;
    sc::DevArr<unsigned long long> k1, k1s, v1, v1s;            // (segment, gene2) and best cell of a tile, as written and sorted
    sc::DevArr<unsigned long long> k2, k2s;                     // key2 as picked and sorted.  Reused: k2 holds the distinct triples in the end
    sc::DevArr<Cand> hit, hits;                                 // the records that go with k2 / k2s
    sc::DevArr<uint8_t> tmp;                                    // rocprim's
    sc::DevArr<unsigned char> state;
    sc::DevArr<Cand> list;                                      // the traceback lists, bucket after bucket
    sc::DevArr<int> from;                                       // list slot -> record.  Reused: as unsigned, the triples' run lengths in the end
    sc::DevArr<int> out, times;
    sc::DevArr<unsigned long long> trip, trips;                 // the reads' triples as written and sorted
    sc::DevArr<unsigned> n_runs;
    sc::DevArr<int> first, end;                                 // a read's records in k2s / hits; first is its cursor
    sc::DevArr<unsigned char> resolved;
    sc::DevArr<int> tsamp, tsamps, usamp;                       // a call with samples: the triples' samples as written, sorted, distinct
    SeedScratch sx;                                             // the seeded score pass's
};

// One stretch on its way through the stages: what the host knows of it.
struct StretchRun {
    const Stretch& s;
    int nr;                                                     // reads
    long nv = 0;                                                // hits: the first nv records of k2s / hits
    long part[N_BUCKETS] = {};                                  // where bucket b's traceback list starts
    unsigned long long ctr[C_WORDS] = {};                       // the device's counters as last read back
    explicit StretchRun(const Stretch& of) : s(of), nr(of.read1 - of.read0) {}
};

inline dim3 rec_grid(long n) { return dim3((unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, REC_BLOCKS))); }

// The strand pick: the nc candidate tiles sorted by (segment, gene, strand), then the hits by (read, rank of E6); both sorts are
// stable and the first one's keys are unique, so the order is the same whatever order the score pass wrote in.  Sets run.nv
// and run.part (the histogram of the hits over the traceback buckets, as offsets).
void select_hits(sc::TimedStream& st, const ProfileInput& in, const CountTables& tb, CountBufs& b, size_t nc, StretchRun& run) {
    auto* k1 = b.k1.ensure(nc); auto* k1s = b.k1s.ensure(nc); auto* v1 = b.v1.ensure(nc); auto* v1s = b.v1s.ensure(nc);
    auto* k2 = b.k2.ensure(nc); auto* k2s = b.k2s.ensure(nc);
    Cand* hit = b.hit.ensure(nc); Cand* hits = b.hits.ensure(nc);
    if (nc) {
        hipLaunchKernelGGL(k_cnt_keys, rec_grid((long)nc), dim3(256), 0, st, tb.cand.p, (long)nc, k1, v1);
        st.launched();
        size_t t1 = 0, t2 = 0;
        HIPCHK(rocprim::radix_sort_pairs(nullptr, t1, k1, k1s, v1, v1s, nc, 0, 64, st));
        HIPCHK(rocprim::radix_sort_pairs(nullptr, t2, k2, k2s, hit, hits, nc, 0, 64, st));
        void* tmp = b.tmp.ensure(std::max(t1, t2));
        HIPCHK(rocprim::radix_sort_pairs(tmp, t1, k1, k1s, v1, v1s, nc, 0, 64, st));
        hipLaunchKernelGGL(k_cnt_pick, rec_grid((long)nc), dim3(256), 0, st, k1s, v1s, (long)nc, in.dev->so.p, tb.read.p, run.s.read0, tb.slot.p,
                           tb.rank.p, k2, hit, tb.ctr.p);
        st.launched();
        HIPCHK(rocprim::radix_sort_pairs(tmp, t2, k2, k2s, hit, hits, nc, 0, 64, st));
        st.d2h(run.ctr, tb.ctr.p, sizeof run.ctr);
        st.sync();
    }
    run.nv = (long)run.ctr[C_VALID];
    for (int k = 0, at = 0; k < N_BUCKETS; k++) { run.part[k] = at; at += (int)run.ctr[C_HIST + k]; }
}

// The rounds over the hits of a stretch: choose, trace, apply -I, move the reads; one readback (the lists' fill) per round.
// A round traces one E6 group per unresolved read, from round COUNT_ROUNDS on all that is left.  Sets the "trace" mark.
void trace_rounds(sc::TimedStream& st, const ProfileInput& in, const CountTables& tb, CountBufs& b, StretchRun& run, sc_profile_count_stats& stats) {
    const long nv = run.nv;
    const int nr = run.nr;
    int* first = b.first.ensure((size_t)nr); int* end = b.end.ensure((size_t)nr);
    auto* resolved = b.resolved.ensure((size_t)nr);
    auto* state = b.state.ensure((size_t)nv);
    Cand* list = b.list.ensure((size_t)nv);
    int* from = b.from.ensure((size_t)nv);
    int* out = b.out.ensure((size_t)nv * 4);
    b.times.ensure((size_t)nv);
    const unsigned long long* k2s = b.k2s.get();
    const ProfileInput::Dev& d = *in.dev;
    st.mark("trace");
    if (!nv) return;
    long filled[N_BUCKETS] = {};
    st.h2d(tb.part.p, run.part, sizeof run.part);
    st.zero(state, (size_t)nv);
    st.zero(resolved, (size_t)nr);
    HIPCHK(hipMemsetAsync(first, 0xFF, (size_t)nr * sizeof(int), st));
    hipLaunchKernelGGL(k_cnt_bounds, rec_grid(nv), dim3(256), 0, st, k2s, nv, first, end);
    st.launched();
    const dim3 read_grid((unsigned)std::min(nr, READ_BLOCKS));
    for (int round = 0;; round++) {
        hipLaunchKernelGGL(k_cnt_choose, rec_grid(nv), dim3(256), 0, st, k2s, b.hits.get(), nv, d.so.p, first, resolved,
                           round >= COUNT_ROUNDS ? 1 : 0, state, list, from, tb.part.p, tb.ctr.p);
        st.launched();
        st.d2h(run.ctr, tb.ctr.p, sizeof run.ctr);
        st.sync();
        Fresh fresh;
        long n_fresh = 0;
        for (int k = 0; k < N_BUCKETS; k++) {
            fresh.begin[k] = run.part[k] + filled[k];
            filled[k] = (long)run.ctr[C_FILL + k];
            fresh.end[k] = run.part[k] + filled[k];
            n_fresh += fresh.end[k] - fresh.begin[k];
        }
        if (n_fresh == 0) break;                                // no unresolved read has a group left
        for (int k = 0; k < N_BUCKETS; k++) {
            const int n = (int)(fresh.end[k] - fresh.begin[k]);
            if (n == 0) continue;
            dispatch_by_rows(k + 1, [&](auto r) {
                hipLaunchKernelGGL(k_bl_trace<decltype(r)::value>, trace_grid(n), dim3(64), 0, st, d.gq.p, d.go.p, d.sq.p, d.so.p,
                                   list + fresh.begin[k], n, out + 4 * fresh.begin[k]);
            });
            st.launched();
        }
        hipLaunchKernelGGL(k_cnt_resolve, rec_grid(n_fresh), dim3(256), 0, st, fresh, n_fresh, list, from, out, in.min_identity_pct, state, tb.ctr.p);
        st.launched();
        hipLaunchKernelGGL(k_cnt_advance, read_grid, dim3(64), 0, st, k2s, state, nr, first, end, resolved);
        st.launched();
        stats.n_rounds++; stats.n_traced += n_fresh;
    }
}

// One distinct row of a stretch: the triple, its sample (0 in a call without samples) and the reads behind it.
struct Row {
    int sample; unsigned long long triple; long reads;
    bool same(const Row& o) const { return sample == o.sample && triple == o.triple; }
    bool operator<(const Row& o) const { return sample != o.sample ? sample < o.sample : triple < o.triple; }
};

// The triples of the resolved reads, sorted and reduced to distinct ones with their number of reads, appended to `rows`; the
// stream is synchronised.  With samples (sample_bits > 0) the sample of each triple rides beside it: a stable sort by triple,
// then a stable sort by sample, then runs of equal (sample, triple).  A traceback that failed in some round shows here:
// SC_ERR_INTERNAL.
void reduce_triples(sc::TimedStream& st, const ProfileInput& in, const CountTables& tb, CountBufs& b, int gene_bits, int times_bits, int sample_bits,
                    StretchRun& run, std::vector<Row>& rows) {
    if (!run.nv) return;
    auto* trips_in = b.trip.ensure((size_t)run.nv);
    auto* trips = b.trips.ensure((size_t)run.nv);
    const bool by_sample = tb.sample.p != nullptr;
    int* samp_in = by_sample ? b.tsamp.ensure((size_t)run.nv) : nullptr;
    int* samps = by_sample ? b.tsamps.ensure((size_t)run.nv) : nullptr;
    int* usamp = by_sample ? b.usamp.ensure((size_t)run.nv) : nullptr;
    hipLaunchKernelGGL(k_cnt_count, dim3((unsigned)std::min(run.nr, READ_BLOCKS)), dim3(64), 0, st, b.k2s.get(), b.state.get(), b.hits.get(), run.nr,
                       b.first.get(), b.end.get(), b.resolved.get(), gene_bits, times_bits, b.times.get(), trips_in, tb.ctr.p, tb.sample.p,
                       run.s.read0, samp_in);
    st.launched();
    st.d2h(run.ctr, tb.ctr.p, sizeof run.ctr);
    st.sync();
    const size_t nt = (size_t)run.ctr[C_TRIPLES];
    if (run.ctr[C_BAD]) throw sc::ScError(SC_ERR_INTERNAL, in.fn + ": a traceback failed");
    if (!nt) return;
    unsigned long long* uniq = b.k2.get();                      // the reuses named at CountBufs: both arrays are free by now and
    unsigned* runs = (unsigned*)b.from.get();                   // hold nv >= nt elements of the size needed
    unsigned* n_runs = b.n_runs.ensure(1);
    const int triple_bits = 2 * gene_bits + times_bits;
    size_t t1 = 0, t2 = 0, t3 = 0;
    if (!by_sample) {
        HIPCHK(rocprim::radix_sort_keys(nullptr, t1, trips_in, trips, nt, 0, triple_bits, st));
        HIPCHK(rocprim::run_length_encode(nullptr, t2, trips, (unsigned)nt, uniq, runs, n_runs, st));
        void* tmp = b.tmp.ensure(std::max(t1, t2));
        HIPCHK(rocprim::radix_sort_keys(tmp, t1, trips_in, trips, nt, 0, triple_bits, st));
        HIPCHK(rocprim::run_length_encode(tmp, t2, trips, (unsigned)nt, uniq, runs, n_runs, st));
    } else {
        // (trips_in, samp_in) -> by triple -> (trips, samps) -> by sample, stable -> (trips_in, samp_in) again
        unsigned* ks_in = (unsigned*)samp_in; unsigned* ks = (unsigned*)samps;
        const auto pairs_in = rocprim::make_zip_iterator(rocprim::make_tuple(samp_in, trips_in));
        const auto pairs_out = rocprim::make_zip_iterator(rocprim::make_tuple(usamp, uniq));
        HIPCHK(rocprim::radix_sort_pairs(nullptr, t1, trips_in, trips, samp_in, samps, nt, 0, triple_bits, st));
        HIPCHK(rocprim::radix_sort_pairs(nullptr, t2, ks, ks_in, trips, trips_in, nt, 0, sample_bits, st));
        HIPCHK(rocprim::run_length_encode(nullptr, t3, pairs_in, (unsigned)nt, pairs_out, runs, n_runs, st));
        void* tmp = b.tmp.ensure(std::max(t1, std::max(t2, t3)));
        HIPCHK(rocprim::radix_sort_pairs(tmp, t1, trips_in, trips, samp_in, samps, nt, 0, triple_bits, st));
        HIPCHK(rocprim::radix_sort_pairs(tmp, t2, ks, ks_in, trips, trips_in, nt, 0, sample_bits, st));
        HIPCHK(rocprim::run_length_encode(tmp, t3, pairs_in, (unsigned)nt, pairs_out, runs, n_runs, st));
    }
    unsigned n_uniq = 0;
    st.d2h(&n_uniq, n_runs, sizeof n_uniq);
    st.sync();
    std::vector<unsigned long long> trip(n_uniq);
    std::vector<unsigned> reads(n_uniq);
    std::vector<int> samp(by_sample ? n_uniq : 0);
    st.d2h(trip.data(), uniq, (size_t)n_uniq * 8); st.d2h(reads.data(), runs, (size_t)n_uniq * sizeof(unsigned));
    st.d2h(samp.data(), usamp, samp.size() * sizeof(int));
    st.sync();
    for (unsigned k = 0; k < n_uniq; k++) rows.push_back(Row{by_sample ? samp[k] : 0, trip[k], (long)reads[k]});
}

// The caller's arrays for the rows; sample may be null (a call without samples)
struct RowsOut { int *sample, *gene, *times, *share; long* reads; long cap; };

// The stretches' rows merged into the caller's arrays, ascending: a read is in one stretch, so the numbers of reads of equal
// rows add.  Returns the number of distinct rows, which may be more than the `cap` that were written.
long merge_rows(std::vector<Row>& total, int gene_bits, int times_bits, const RowsOut& out) {
    std::sort(total.begin(), total.end());
    long n = 0;
    for (size_t k = 0; k < total.size(); k++) {
        if (k > 0 && total[k].same(total[k - 1])) { if (n <= out.cap) out.reads[n - 1] += total[k].reads; continue; }
        if (n < out.cap) {
            if (out.sample) out.sample[n] = total[k].sample;
            out.gene[n] = (int)(total[k].triple >> (gene_bits + times_bits));
            out.times[n] = (int)((total[k].triple >> gene_bits) & ((1ull << times_bits) - 1ull));
            out.share[n] = (int)(total[k].triple & ((1ull << gene_bits) - 1ull));
            out.reads[n] = total[k].reads;
        }
        n++;
    }
    return n;
}

// What an index (sc_profile_index) keeps from call to call; a call without one passes none of it.
struct Resident {
    int device;
    ResidentGenes genes;
    std::unique_ptr<SeedIndex> seeds[SEED_MAX_K - SEED_MIN_K + 1];      // per seed length a call has needed so far
    SegArena segs;
    CountArena tables;
    CountBufs bufs;
    Resident(int device_, Packed&& packed) : device(device_), genes(std::move(packed)) {}
};
// The samples of a call on an index: read_sample[n_reads], non-decreasing, in 0..n_samples-1
struct Samples { const int* of_read; int n; };

// The body of sc_profile_counts and sc_profile_index_counts, under their guard: the front end; once per call the rank table,
// the stretch plan, the uploads and the index (`res`: the genes are resident, the index of this k is built only when none is cached, and every
// array comes from res; *n_index_builds counts the builds); then per stretch the score pass and the stages above; the merge.
int profile_counts(const char* fn_name, int device, Resident* res, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text,
                   const long* seg_off, int n_segs, const int* seg_read, int n_reads, Samples samples, double min_identity_pct, double max_evalue,
                   double ka_lambda, double ka_k, int seeded, long cand_room, const RowsOut& out, long* n_out, sc_profile_count_stats* stats_out,
                   int* n_index_builds) {
    ProfileInput in(fn_name, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct, max_evalue, ka_lambda, ka_k);
    if (res) in.resident = &res->genes;
    const std::string& fn = in.fn;
    sc_profile_count_stats unasked;
    sc_profile_count_stats& stats = stats_out ? *stats_out : unasked;
    std::memset(&stats, 0, sizeof stats);
    if (n_out) *n_out = 0;
    if (const int rc = in.check(n_reads >= 0 && (n_segs <= 0 || seg_read) && (!res || out.sample) && out.gene && out.times && out.share &&
                                out.reads && out.cap >= 0 && cand_room >= 0 && n_out && (!res || n_reads == 0 || samples.of_read)))
        return rc;
    for (int r = 0; r < n_segs; r++)
        if (seg_read[r] < 0 || seg_read[r] >= n_reads)
            return tl_error.fail(SC_ERR_ARG, fn + ": segment " + std::to_string(r) + " belongs to read " + std::to_string(seg_read[r]) + " of " +
                                                 std::to_string(n_reads));
    if (res) {
        if (samples.n < 1 || samples.n > MAX_SAMPLES)
            return tl_error.fail(SC_ERR_ARG, fn + ": " + std::to_string(samples.n) + " samples (1.." + std::to_string(MAX_SAMPLES) + " supported)");
        for (int r = 0; r < n_reads; r++) {
            const int s = samples.of_read[r];
            if (s < 0 || s >= samples.n)
                return tl_error.fail(SC_ERR_ARG, fn + ": read " + std::to_string(r) + " belongs to sample " + std::to_string(s) + " of " +
                                                     std::to_string(samples.n));
            if (r > 0 && s < samples.of_read[r - 1])
                return tl_error.fail(SC_ERR_ARG, fn + ": read " + std::to_string(r) + " belongs to sample " + std::to_string(s) + " after sample " +
                                                     std::to_string(samples.of_read[r - 1]) + ": the samples come one after the other");
        }
    }
    if (const int rc = in.prepare(device, seeded != 0); rc != SC_OK || n_segs == 0) return rc;
    const ReadSegs rs(seg_read, n_segs, n_reads);
    const int gene_bits = bits_of(n_genes), times_bits = bits_of(rs.most_segs), sample_bits = res ? bits_of(samples.n) : 0;
    if (2 * gene_bits + times_bits > 64)
        return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_genes) + " genes and " + std::to_string(rs.most_segs) +
                                                     " segments in one read do not fit a 64-bit triple");
    const RankTable table = rank_table(in);
    stats.seed_k = in.seed_k;
    const StretchPlan plan = plan_stretches(in, rs, n_reads, cand_room > 0 ? cand_room : COUNT_ROOM);
    const long room = plan.room;
    if (room > 0x7FFFFFFFL)
        return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(room) + " (segment, gene, strand) tiles in one read (at most 2147483647)");
    std::vector<Row> total;                                     // the rows of every stretch
    if (!plan.stretches.empty()) {
        std::unique_ptr<CountTables> own_tb(res ? new CountTables(res->tables, n_segs, n_reads, table, room) : new CountTables(n_segs, table, room));
        CountTables& tb = *own_tb;
        std::unique_ptr<SeedIndex> own_index;
        const SeedIndex* index = nullptr;
        {
            sc::TimedStream st;
            if (res) in.upload(st, res->segs); else in.upload(st);
            tb.upload(st, seg_read, n_segs, table, samples.of_read, n_reads);
            st.mark("index");
            std::unique_ptr<SeedIndex>* cached = res && in.seed_k ? &res->seeds[in.seed_k - SEED_MIN_K] : nullptr;
            if (in.seed_k && !(cached && *cached)) {
                own_index.reset(new SeedIndex(st, in.dev->gq.p, in.dev->go.p, n_genes, in.gene_bytes, in.seed_k));
                if (n_index_builds) ++*n_index_builds;
            }
            st.mark("indexed");
            st.sync();
            if (cached && own_index) { own_index->trim(); *cached = std::move(own_index); }     // kept only once it is complete
            index = cached ? cached->get() : own_index.get();
            stats.upload_ms += st.ms("upload", "index"); stats.index_ms += st.ms("index", "indexed");
            if (index) stats.n_gene_kmers = (long)index->n_keys;
        }
        CountBufs own_bufs;
        CountBufs& bufs = res ? res->bufs : own_bufs;
        for (const Stretch& s : plan.stretches) {
            sc::TimedStream st;
            const Buckets by_r = rs.buckets(in, s.read0, s.read1);
            const std::vector<int> sids = by_r.order();
            int* d_sids = bufs.sids.ensure(sids.size() + 4);    // never empty
            st.mark("upload");
            st.h2d(d_sids, sids.data(), sids.size() * sizeof(int));
            st.zero(tb.ncand.p, sizeof(unsigned));
            st.zero(tb.ctr.p, C_WORDS * sizeof(unsigned long long));
            st.mark("lookup");
            const ScorePass pass(st, in, by_r, sids, d_sids, index, bufs.sx, CandBuf{tb.cand.p, room, tb.ncand.p}, &stats.score_cells);
            st.mark("select");
            unsigned n_cand = 0;
            st.d2h(&n_cand, tb.ncand.p, sizeof(unsigned));
            st.sync();
            if ((long)n_cand > room) return tl_error.fail(SC_ERR_INTERNAL, fn + ": more candidates than tiles");
            stats.n_pairs += pass.n_pairs; stats.n_tiles += pass.n_tiles; stats.n_candidates += (long)n_cand; stats.n_stretches++;
            StretchRun run(s);
            select_hits(st, in, tb, bufs, n_cand, run);
            trace_rounds(st, in, tb, bufs, run, stats);
            st.mark("count");
            reduce_triples(st, in, tb, bufs, gene_bits, times_bits, sample_bits, run, total);
            st.mark("counted");
            st.sync();
            stats.upload_ms += st.ms("upload", "lookup"); stats.lookup_ms += st.ms("lookup", "score"); stats.score_ms += st.ms("score", "select");
            stats.select_ms += st.ms("select", "trace"); stats.trace_ms += st.ms("trace", "count"); stats.count_ms += st.ms("count", "counted");
            stats.n_reads_counted += (long)run.ctr[C_READS]; stats.n_hits += (long)run.ctr[C_HITS]; stats.trace_cells += (long)run.ctr[C_CELLS];
        }
    }
    int rc = SC_OK;
    const long n = *n_out = merge_rows(total, gene_bits, times_bits, out);
    if (n > out.cap) rc = tl_error.fail(SC_ERR_CAPACITY, fn + ": " + std::to_string(n) + " triples, room for " + std::to_string(out.cap));
    stats.total_ms = sc::now_ms() - in.t0;
    return rc;
}

}  // namespace
