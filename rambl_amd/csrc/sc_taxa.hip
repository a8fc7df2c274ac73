// Genus assignment of gene sequences on the device (DESIGN.md §8.12 is the contract): naive Bayes over 8-mers with bootstrap
// trials -- the rule of the RDP classifier that scripts/per_sample_gene_profile_fast.py:223-246 (copy_number_correct) and
// scripts/per_sample_taxon_profile.py:47-52 (rdp_classify) start with `java -jar`.  Parity with RDP's own output is not
// claimed: its training set and Java's random stream were never at hand.
//   k_taxa_words   training: one wavefront per sequence, its distinct words counted into m[w * G + g] and n[w]
//   k_taxa_table   one thread per cell: m becomes q = llrint(log2(P(w|g)) * 1024) in place
//   k_taxa_score   one workgroup per (query, chunk of 64 genera): the full score and every trial, best (score, genus) each
//   k_taxa_pick    the chunks reduced to the assigned genus and the trial winners per query
//   k_taxa_column  a genus' column of the table or of the kept counts, for the read-backs
#include <climits>
#include <cmath>
#include <memory>

#include "../../include/straincall_hip.h"
#include "sc_host.hpp"

namespace {

constexpr int TAXA_K = 8;
constexpr int N_WORDS = 1 << (2 * TAXA_K);          // 65 536
constexpr int BITSET_WORDS = N_WORDS / 32;          // the wavefront's LDS bitset: 8 KiB
constexpr int MAX_GENERA = 16384, MAX_TRAIN = 1 << 24, MAX_TRAIN_LEN = 1 << 24, MAX_QUERY = 8192, MAX_TRIALS = 1024;
constexpr long MAX_TRAIN_BASES = 1L << 32;           // of one training set: 4 GiB of codes on the host and on the device
constexpr int CHUNK = 64;                           // genera per workgroup of the score pass: one per lane
constexpr int SCORE_WAVES = 4;                      // its wavefronts share the query's words and split the trials
constexpr int WORDS_BLOCKS = 8192, CELL_BLOCKS = 4096, SCORE_BLOCKS = 8192, PICK_BLOCKS = 1024;
constexpr long PART_ROOM = 1L << 25;                // (score, genus) records of the chunks held at a time: 256 MiB
constexpr uint8_t NO_BASE = 4;

thread_local sc::LastError tl_error;

inline uint8_t taxa_code(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return NO_BASE;
    }
}

// The word-list position of draw j of trial t: the same expression on the host (sc_taxa_draw) and in k_taxa_score.
__host__ __device__ inline unsigned draw_pos(unsigned long long seed, unsigned long long key, unsigned t, unsigned j, unsigned W) {
    unsigned long long z = (seed ^ key) + (unsigned long long)(t * 65536u + j + 1u) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(((z >> 32) * (unsigned long long)W) >> 32);
}

// One wavefront per training sequence.  A lane takes a stretch of the sequence's windows and rolls the code along it; every
// word sets its bit in the wavefront's LDS bitset, so a word counts once per sequence however often it occurs.  The bitset is
// then walked a word per lane: each set bit adds 1 to m[w * G + g] and to n[w] (integer atomics: the counts are exact
// whatever the order), and the lane clears its word for the next sequence.
__global__ __launch_bounds__(64) void k_taxa_words(const uint8_t* codes, const long* seq_off, const int* seq_genus, int n_seqs, int G, unsigned* m,
                                                   unsigned* n) {
    __shared__ unsigned bits[BITSET_WORDS];
    const int lane = threadIdx.x;
    for (int w = lane; w < BITSET_WORDS; w += 64) bits[w] = 0;
    for (int s = blockIdx.x; s < n_seqs; s += gridDim.x) {
        const int g = seq_genus[s];
        const long r0 = seq_off[s];
        const int L = (int)(seq_off[s + 1] - r0);
        const int nw = L - TAXA_K + 1;                          // windows; none when the sequence is shorter than 8
        const int per = (nw + 63) / 64;
        const int wa = lane * per, wb = min(wa + per, nw);
        __syncthreads();                                        // the bitset is clear
        unsigned fw = 0;
        int run = 0;                                            // ACGTU bases in a row up to here
        for (int i = wa, end = wb > wa ? wb + TAXA_K - 1 : wa; i < end; i++) {
            const unsigned c = codes[r0 + i];
            if (c >= 4u) { run = 0; continue; }
            fw = ((fw << 2) | c) & (unsigned)(N_WORDS - 1);
            if (++run >= TAXA_K) atomicOr(&bits[fw >> 5], 1u << (fw & 31u));
        }
        __syncthreads();
        for (int w = lane; w < BITSET_WORDS; w += 64) {
            unsigned word = bits[w];
            if (!word) continue;
            bits[w] = 0;
            while (word) {
                const unsigned code = (unsigned)w * 32u + (unsigned)(__ffs(word) - 1);
                word &= word - 1u;
                atomicAdd(&m[(size_t)code * (size_t)G + (size_t)g], 1u);
                atomicAdd(&n[code], 1u);
            }
        }
    }
}

// One thread per cell, in place: the cell's count m becomes q.  Every operation but log2 is a single correctly rounded fp64
// operation; log2's last bit matters only where log2(P) * 1024 is within an ulp of a half-integer.
__global__ __launch_bounds__(256) void k_taxa_table(int* table, const unsigned* n, const int* genus_seqs, int G, int n_seqs) {
    const size_t cells = (size_t)N_WORDS * (size_t)G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
        const size_t w = i / (size_t)G;
        const int g = (int)(i - w * (size_t)G);
        const double pw = ((double)n[w] + 0.5) / ((double)n_seqs + 1.0);
        const double p = ((double)(unsigned)table[i] + pw) / ((double)genus_seqs[g] + 1.0);
        table[i] = (int)llrint(log2(p) * 1024.0);
    }
}

// (the kept counts are uint32 in the same layout: the copy moves 32 bits either way)
__global__ __launch_bounds__(256) void k_taxa_column(const int* table, int G, int genus, int* out) {
    for (int w = blockIdx.x * 256 + threadIdx.x; w < N_WORDS; w += gridDim.x * 256) out[w] = table[(size_t)w * (size_t)G + (size_t)genus];
}

struct Best { int score, genus; };

// The largest score of the wavefront's lanes, the lowest genus among equals; every lane returns it.
__device__ inline Best wave_best(int score, int genus) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int os = __shfl_xor(score, o), og = __shfl_xor(genus, o);
        if (os > score || (os == score && og < genus)) { score = os; genus = og; }
    }
    return Best{score, genus};
}

// One workgroup per (query, chunk), chunk-major so that the workgroups in flight read the same 64 columns of the table.  The
// query's word list is staged in LDS; lane l of every wavefront owns genus chunk * 64 + l, and a word's 64 cells are one
// 256-byte read.  The full score is split over the four wavefronts by position and summed through LDS; the trials go round
// the wavefronts, each computing the trial's positions identically in every lane.  part[((chunk * nq + query) * slots +
// slot] is the chunk's best (score, genus), slot 0 the full score and 1 + t trial t.  A query without a word writes nothing.
__global__ __launch_bounds__(64 * SCORE_WAVES) void k_taxa_score(const int* table, int G, int n_chunks, const uint16_t* words, const long* word_off,
                                                                 const unsigned long long* key, int q0, int nq, unsigned long long seed,
                                                                 int n_trials, Best* part) {
    __shared__ uint16_t code[MAX_QUERY];
    __shared__ int partial[SCORE_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long total = (long)nq * n_chunks;
    const int slots = 1 + n_trials;
    for (long b = blockIdx.x; b < total; b += gridDim.x) {
        const int chunk = (int)(b / nq), qi = (int)(b - (long)chunk * nq);
        const long w0 = word_off[q0 + qi];
        const int W = (int)(word_off[q0 + qi + 1] - w0);
        if (W == 0) continue;                                   // the whole workgroup
        __syncthreads();                                        // the last trip's readers are done with the LDS
        for (int i = threadIdx.x; i < W; i += 64 * SCORE_WAVES) code[i] = words[w0 + i];
        __syncthreads();
        const int g = chunk * CHUNK + lane;
        const bool live = g < G;
        const int* col = table + (live ? g : 0);
        Best* out = part + (size_t)b * (size_t)slots;
        // |q| <= 50 * 1024 per word and a query has at most 8 185 words, so |sum| <= 419 072 000: every sum fits an int
        int sum = 0;
        const int per = (W + SCORE_WAVES - 1) / SCORE_WAVES;
        if (live) {
#pragma unroll 8
            for (int i = wave * per, end = min(i + per, W); i < end; i++) sum += col[(size_t)code[i] * (size_t)G];
        }
        partial[wave][lane] = sum;
        __syncthreads();
        if (wave == 0) {
            sum = 0;
#pragma unroll
            for (int v = 0; v < SCORE_WAVES; v++) sum += partial[v][lane];
            const Best best = wave_best(live ? sum : INT_MIN, g);
            if (lane == 0) out[0] = best;
        }
        const unsigned long long k = key[q0 + qi];
        const int D = max(W / 8, 5);
        for (int t = wave; t < n_trials; t += SCORE_WAVES) {
            sum = 0;                                            // at most 1 023 draws: the bound above holds
#pragma unroll 8
            for (int j = 0; j < D; j++) {
                const unsigned pos = draw_pos(seed, k, (unsigned)t, (unsigned)j, (unsigned)W);
                if (live) sum += col[(size_t)code[pos] * (size_t)G];
            }
            const Best best = wave_best(live ? sum : INT_MIN, g);
            if (lane == 0) out[1 + t] = best;
        }
    }
}

// One thread per (query, slot): the chunks in ascending order, a later one wins only with a larger score, so the lowest genus
// wins a tie.  A query without a word gets -1 everywhere.
__global__ __launch_bounds__(256) void k_taxa_pick(const Best* part, int n_chunks, const long* word_off, int q0, int nq, int n_trials, int* best_genus,
                                                   int* trial_winner) {
    const int slots = 1 + n_trials;
    const long total = (long)nq * slots;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int qi = (int)(i / slots), slot = (int)(i - (long)qi * slots);
        const int query = q0 + qi;
        int score = INT_MIN, genus = -1;
        if (word_off[query + 1] > word_off[query])
            for (int c = 0; c < n_chunks; c++) {
                const Best b = part[((size_t)c * (size_t)nq + (size_t)qi) * (size_t)slots + (size_t)slot];
                if (b.score > score) { score = b.score; genus = b.genus; }
            }
        if (slot == 0) best_genus[query] = genus;
        else trial_winner[(size_t)query * (size_t)n_trials + (size_t)(slot - 1)] = genus;
    }
}

unsigned grid_of(long units, int own_cap, int grid_cap) {
    return (unsigned)std::max<long>(1, std::min<long>(units, grid_cap > 0 ? grid_cap : own_cap));
}

}  // namespace

// A trained model on one device: the table and n; with keep_counts a copy of m as it stood before it became the table.
struct sc_taxa_model {
    int device, G;
    sc::DevMem<int> table;
    sc::DevMem<unsigned> n;
    std::unique_ptr<sc::DevMem<unsigned>> m;
    sc_taxa_model(int device_, int G_, bool keep_counts) : device(device_), G(G_), table((size_t)N_WORDS * (size_t)G_), n(N_WORDS) {
        if (keep_counts) m.reset(new sc::DevMem<unsigned>((size_t)N_WORDS * (size_t)G_));
    }
};

extern "C" {

const char* sc_taxa_error(void) { return tl_error.text.c_str(); }

int sc_taxa_train(int device, const char* seq_text, const long* seq_off, int n_seqs, const int* seq_genus, int n_genera, int grid_cap,
                  int keep_counts, sc_taxa_model** model, sc_taxa_stats* stats_out) {
    sc_taxa_stats unasked;
    sc_taxa_stats& stats = stats_out ? *stats_out : unasked;
    stats = {};
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_taxa_train", [&] {
        const std::string fn = "sc_taxa_train";
        if (!model || n_seqs < 0 || grid_cap < 0 || (n_seqs > 0 && (!seq_text || !seq_off || !seq_genus))) return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        *model = nullptr;
        if (n_genera < 1 || n_genera > MAX_GENERA)
            return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_genera) + " genera (1.." + std::to_string(MAX_GENERA) + " supported)");
        if (n_seqs < 1 || n_seqs > MAX_TRAIN)
            return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_seqs) + " training sequences (1.." + std::to_string(MAX_TRAIN) + " supported)");
        const double t0 = sc::now_ms();
        if (seq_off[n_seqs] - seq_off[0] > MAX_TRAIN_BASES)
            return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(seq_off[n_seqs] - seq_off[0]) + " training bases in all (at most " +
                                                         std::to_string(MAX_TRAIN_BASES) + " supported)");
        std::vector<long> off((size_t)n_seqs + 1);
        std::vector<int> genus(seq_genus, seq_genus + n_seqs), genus_seqs((size_t)n_genera, 0);
        for (int s = 0; s <= n_seqs; s++) off[(size_t)s] = seq_off[s] - seq_off[0];
        for (int s = 0; s < n_seqs; s++) {
            const long len = off[(size_t)s + 1] - off[(size_t)s];
            if (len < 0 || len > MAX_TRAIN_LEN)
                return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": training sequence " + std::to_string(s) + " has " + std::to_string(len) + " bases (0.." +
                                                             std::to_string(MAX_TRAIN_LEN) + " supported)");
            if (genus[(size_t)s] < 0 || genus[(size_t)s] >= n_genera)
                return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": training sequence " + std::to_string(s) + " has genus " + std::to_string(genus[(size_t)s]) +
                                                             " (0.." + std::to_string(n_genera - 1) + " supported)");
            genus_seqs[(size_t)genus[(size_t)s]]++;
        }
        std::vector<uint8_t> codes((size_t)off.back());
        for (size_t k = 0; k < codes.size(); k++) codes[k] = taxa_code(seq_text[seq_off[0] + (long)k]);
        sc::select_device(device);
        std::unique_ptr<sc_taxa_model> mo(new sc_taxa_model(device, n_genera, keep_counts != 0));
        sc::DevMem<uint8_t> d_codes(codes.size());
        sc::DevMem<long> d_off(off.size());
        sc::DevMem<int> d_genus(genus.size()), d_genus_seqs((size_t)n_genera);
        const size_t table_bytes = (size_t)N_WORDS * (size_t)n_genera * sizeof(int);
        sc::TimedStream st;
        st.mark("upload");
        st.h2d(d_codes, codes); st.h2d(d_off, off); st.h2d(d_genus, genus); st.h2d(d_genus_seqs, genus_seqs);
        st.zero(mo->table.p, table_bytes);
        st.zero(mo->n.p, N_WORDS * sizeof(unsigned));
        st.mark("words");
        hipLaunchKernelGGL(k_taxa_words, dim3(grid_of(n_seqs, WORDS_BLOCKS, grid_cap)), dim3(64), 0, st, d_codes.p, d_off.p, d_genus.p, n_seqs, n_genera,
                           (unsigned*)mo->table.p, mo->n.p);
        st.launched();
        if (mo->m) HIPCHK(hipMemcpyAsync(mo->m->p, mo->table.p, table_bytes, hipMemcpyDeviceToDevice, st));
        st.mark("table");
        hipLaunchKernelGGL(k_taxa_table, dim3(grid_of(((long)N_WORDS * n_genera + 255) / 256, CELL_BLOCKS, grid_cap)), dim3(256), 0, st, mo->table.p, mo->n.p,
                           d_genus_seqs.p, n_genera, n_seqs);
        st.launched();
        st.mark("done");
        std::vector<unsigned> n_host(N_WORDS);
        st.d2h(n_host, mo->n);
        st.sync();
        stats.upload_ms = st.ms("upload", "words"); stats.words_ms = st.ms("words", "table"); stats.table_ms = st.ms("table", "done");
        stats.n_seqs = n_seqs; stats.n_genera = n_genera; stats.table_bytes = (long)table_bytes;
        for (unsigned v : n_host) stats.n_words += v;
        stats.total_ms = sc::now_ms() - t0;
        *model = mo.release();
        return SC_OK;
    });
}

int sc_taxa_classify(const sc_taxa_model* mo, const char* query_text, const long* query_off, int n_queries, const unsigned long long* query_key,
                     unsigned long long seed, int n_trials, int grid_cap, int* best_genus, int* trial_winner, int* n_words,
                     sc_taxa_stats* stats_out) {
    sc_taxa_stats unasked;
    sc_taxa_stats& stats = stats_out ? *stats_out : unasked;
    stats = {};
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_taxa_classify", [&] {
        const std::string fn = "sc_taxa_classify";
        if (!mo || n_queries < 0 || grid_cap < 0 || (n_queries > 0 && (!query_text || !query_off || !query_key || !best_genus || !trial_winner || !n_words)))
            return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        if (n_trials < 1 || n_trials > MAX_TRIALS)
            return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": " + std::to_string(n_trials) + " trials (1.." + std::to_string(MAX_TRIALS) + " supported)");
        for (int r = 0; r < n_queries; r++) {
            const long len = query_off[r + 1] - query_off[r];
            if (len < 1 || len > MAX_QUERY)
                return tl_error.fail(SC_ERR_UNSUPPORTED, fn + ": query " + std::to_string(r) + " has " + std::to_string(len) + " bases (1.." + std::to_string(MAX_QUERY) +
                                                             " supported)");
        }
        if (n_queries == 0) return SC_OK;
        const double t0 = sc::now_ms();
        // the word lists: every window of ACGTU bases, in order
        std::vector<uint16_t> words;
        std::vector<long> word_off((size_t)n_queries + 1, 0);
        words.reserve((size_t)(query_off[n_queries] - query_off[0]));
        for (int r = 0; r < n_queries; r++) {
            unsigned fw = 0;
            int run = 0;
            for (long i = query_off[r]; i < query_off[r + 1]; i++) {
                const uint8_t c = taxa_code(query_text[i]);
                if (c == NO_BASE) { run = 0; continue; }
                fw = ((fw << 2) | c) & (unsigned)(N_WORDS - 1);
                if (++run >= TAXA_K) words.push_back((uint16_t)fw);
            }
            word_off[(size_t)r + 1] = (long)words.size();
            n_words[r] = (int)(word_off[(size_t)r + 1] - word_off[(size_t)r]);
        }
        sc::select_device(mo->device);
        const int n_chunks = (mo->G + CHUNK - 1) / CHUNK, slots = 1 + n_trials;
        const int batch = (int)std::max<long>(1, std::min<long>(n_queries, PART_ROOM / ((long)n_chunks * slots)));   // queries whose records are held at a time
        sc::DevMem<uint16_t> d_words(words.size());
        sc::DevMem<long> d_word_off(word_off.size());
        sc::DevMem<unsigned long long> d_key((size_t)n_queries);
        sc::DevMem<int> d_best((size_t)n_queries), d_winner((size_t)n_queries * (size_t)n_trials);
        sc::DevMem<Best> d_part((size_t)batch * (size_t)n_chunks * (size_t)slots);
        sc::TimedStream st;
        st.mark("upload");
        st.h2d(d_words, words); st.h2d(d_word_off, word_off);
        st.h2d(d_key.p, query_key, (size_t)n_queries * sizeof(unsigned long long));
        st.mark("score");
        for (int q0 = 0; q0 < n_queries; q0 += batch) {
            const int nq = std::min(batch, n_queries - q0);
            hipLaunchKernelGGL(k_taxa_score, dim3(grid_of((long)nq * n_chunks, SCORE_BLOCKS, grid_cap)), dim3(64 * SCORE_WAVES), 0, st, mo->table.p, mo->G,
                               n_chunks, d_words.p, d_word_off.p, d_key.p, q0, nq, seed, n_trials, d_part.p);
            st.launched();
            hipLaunchKernelGGL(k_taxa_pick, dim3(grid_of(((long)nq * slots + 255) / 256, PICK_BLOCKS, grid_cap)), dim3(256), 0, st, d_part.p, n_chunks,
                               d_word_off.p, q0, nq, n_trials, d_best.p, d_winner.p);
            st.launched();
        }
        st.mark("scored");
        st.d2h(best_genus, d_best.p, (size_t)n_queries * sizeof(int));
        st.d2h(trial_winner, d_winner.p, (size_t)n_queries * (size_t)n_trials * sizeof(int));
        st.sync();
        stats.upload_ms = st.ms("upload", "score"); stats.score_ms = st.ms("score", "scored");
        stats.n_seqs = n_queries; stats.n_words = (long)words.size(); stats.n_genera = mo->G;
        stats.table_bytes = (long)((size_t)N_WORDS * (size_t)mo->G * sizeof(int));
        stats.total_ms = sc::now_ms() - t0;
        return SC_OK;
    });
}

int sc_taxa_model_counts(const sc_taxa_model* mo, int genus, unsigned* m_out, unsigned* n_out) {
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_taxa_model_counts", [&] {
        if (!mo || !m_out || !n_out || genus < 0 || genus >= mo->G) return tl_error.fail(SC_ERR_ARG, "sc_taxa_model_counts: missing argument or no such genus");
        if (!mo->m) return tl_error.fail(SC_ERR_UNSUPPORTED, "sc_taxa_model_counts: the counts became the table in place; train with keep_counts to read them back");
        sc::select_device(mo->device);
        sc::DevMem<unsigned> d_m(N_WORDS);
        sc::TimedStream st;
        hipLaunchKernelGGL(k_taxa_column, dim3(N_WORDS / 256), dim3(256), 0, st, (const int*)mo->m->p, mo->G, genus, (int*)d_m.p);
        st.launched();
        st.d2h(m_out, d_m.p, N_WORDS * sizeof(unsigned));
        st.d2h(n_out, mo->n.p, N_WORDS * sizeof(unsigned));
        st.sync();
        return SC_OK;
    });
}

int sc_taxa_model_table(const sc_taxa_model* mo, int genus, int* q_out) {
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_taxa_model_table", [&] {
        if (!mo || !q_out || genus < 0 || genus >= mo->G) return tl_error.fail(SC_ERR_ARG, "sc_taxa_model_table: missing argument or no such genus");
        sc::select_device(mo->device);
        sc::DevMem<int> d_q(N_WORDS);
        sc::TimedStream st;
        hipLaunchKernelGGL(k_taxa_column, dim3(N_WORDS / 256), dim3(256), 0, st, mo->table.p, mo->G, genus, d_q.p);
        st.launched();
        st.d2h(q_out, d_q.p, N_WORDS * sizeof(int));
        st.sync();
        return SC_OK;
    });
}

void sc_taxa_free(sc_taxa_model* model) {
    if (!model) return;
    (void)hipSetDevice(model->device);
    delete model;
}

long sc_taxa_draw(unsigned long long seed, unsigned long long key, int trial, int draw, int W) {
    if (W < 1 || trial < 0 || draw < 0) return -1;
    return (long)draw_pos(seed, key, (unsigned)trial, (unsigned)draw, (unsigned)W);
}

}  // extern "C"
