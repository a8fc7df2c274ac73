// The level walk of one region, the reference's NonparametricClustering.cpp:262-582.  It keeps only the scalar
// bookkeeping of the candidate strains on the host, in long double as the reference has it (substitution models, abundances,
// pruning / extension decisions); the per-read work of a level -- rows of new candidates, log-likelihood update, soft update or
// Polya-urn sampler -- is ONE kernel launch (k_level / k_level_sample), its parameters read from host-mapped memory,
// its results and a completion stamp written back to it; the per-strain read log-likelihood rows never leave HBM.
#include <cmath>

#include "sc_ctx.hpp"

namespace sc {

// Host bookkeeping of one candidate (Strain, PartialOrderGraph.hpp:362-402).  The substitution model is the bulky
// part and lives in a pool: a candidate that survives a level keeps its model where it is (no copy when the candidate
// lists are filtered, sorted or extended), only the second and later children of a parent get a copy.
struct Model {
    // The tables are [ks][ks] with ks = the symbols of the region (6 for a gene of A C G T and its reads): a region in flight
    // comes back to its models once per level, after a few hundred other regions have used the core's caches, so what a
    // level touches is kept small and contiguous (rows of 16 entries spread the 36 live ones over four times the lines).
    int ks = KMAX;
    ld sub[KK];                       // sub_count over the symbol table, stride ks
    ld comp[6]; ld Z;
    ld lsub[KK];                      // logl(sub), valid where `stale` is clear
    double lpc[KK];                   // log sub(a,b) - log comp(a) as the device reads it; rows in `dirty` are stale
    uint16_t stale[KMAX];             // per row: entries whose count changed since lsub was formed
    unsigned dirty;
    Model() = default;
    Model(const Model& o) { *this = o; }
    Model& operator=(const Model& o) {            // the live [ks][ks] part only
        ks = o.ks; Z = o.Z; dirty = o.dirty;
        const size_t n = (size_t)ks * ks;
        std::memcpy(sub, o.sub, sizeof(ld) * n); std::memcpy(lsub, o.lsub, sizeof(ld) * n); std::memcpy(lpc, o.lpc, sizeof(double) * n);
        std::memcpy(comp, o.comp, sizeof comp); std::memcpy(stale, o.stale, sizeof stale);
        return *this;
    }
};
struct HStrain {
    ld abundance;
    int model;                        // index into the model pool
    int slot;                         // row of the device read_loglik matrix
    int tail;                         // path arena index
    int node;                         // last node of the path
    uint64_t hash; int seqlen;        // rolling hash / length of strain_seq()
};
struct PathRec { int node, parent; };

// ... and the same for the rows of `rows` only: a row whose counts did not change keeps its sum (the same additions in the
// same order give the same long double), and a level changes one row of a candidate -- its model is cold in the caches
// by the time the region comes back to it, so the lines it touches count
static void recount_rows(Model& s, unsigned rows) {
    rows &= 0x3Fu;
    if (!rows) return;
    for (int i = 0; i < 6; i++) {
        if (!(rows & (1u << i))) continue;
        s.comp[i] = 0;
        for (int j = 0; j < 6; j++) s.comp[i] += s.sub[i * s.ks + j];
    }
    s.Z = 0;
    for (int i = 0; i < 6; i++) s.Z += s.comp[i];
}
static void recount(Model& s) {                                           // Strain.cpp:115-124
    s.Z = 0;
    for (int i = 0; i < 6; i++) {
        s.comp[i] = 0;
        for (int j = 0; j < 6; j++) s.comp[i] += s.sub[i * s.ks + j];
        s.Z += s.comp[i];
    }
}
}  // namespace sc
// The reference adds 1 to a candidate's weight once per draw, in x87 long double (NonparametricClustering.cpp:195): k
// separate roundings, not one.  Inside a binade every a + j is exact (1 is a multiple of the unit in the last place
// while a < 2^64), so the only additions that round are the ones that cross into the next binade: the same k additions
// in O(log k) steps, bit for bit (tests/native/add_ones_check.cpp compares it with the literal loop).
extern "C" long double sc_add_ones(long double a, unsigned long k) {
    if (!std::isfinite((double)a) && !(a == a && a - a == 0)) return a + (long double)k;       // inf / NaN stay what they are
    while (k > 0) {
        if (!(a >= 1)) { a += 1; k--; continue; }            // below 1 (or negative): the literal addition, at most a few times
        {
            // the usual case without a call into libm (this runs once per candidate and level): all k additions stay below
            // the next power of two -- read off the x87 representation (sign + 15-bit exponent above a 64-bit mantissa)
            union { long double v; struct { uint64_t mant; uint16_t se; } b; } top;
            top.v = a;
            top.b.se = (uint16_t)((top.b.se & 0x7fffu) + 1u);      // 2^e for a in [2^(e-1), 2^e)
            top.b.mant = 0x8000000000000000ull;
            // (a < 2^64: an ulp of at most 1, so the difference and the sum are exact)
            if ((top.b.se & 0x7fffu) <= 16383u + 64u && top.v - a > (long double)k) return a + (long double)k;
        }
        int e;
        (void)frexpl(a, &e);                                 // a in [2^(e-1), 2^e)
        const long double top = ldexpl(1.0L, e);
        const long double room = top - a;                    // exact (Sterbenz)
        if (!(room >= 1) && !(room > 0)) { a += 1; k--; continue; }
        const long double jr = ceill(room) - 1;              // additions that stay below the next power of two
        if (jr >= (long double)k) return a + (long double)k;
        const unsigned long j = (unsigned long)jr;
        a += (long double)j; k -= j;                         // exact
        a += 1; k--;                                         // the crossing one rounds like the reference's
    }
    return a;
}
namespace sc {
static uint64_t hash_extend(uint64_t h, const std::string& lab) {
    for (unsigned char c : lab) { h ^= c; h *= 1099511628211ull; }
    return h;
}
static void fmt_g17(std::string& out, double v) {
    char b[64];
    snprintf(b, sizeof b, "%.17g", v);
    out += b;
}

// The level walk of one region: streaming_clustering (NonparametricClustering.cpp:262-582), then read_assign
// (:776-836).  It keeps the candidates' bookkeeping on the host and hands each level to the GPU on the worker's slot.
// Its buffers are reused from level to level: no allocation per level.
struct LevelWalk {
    Worker& w;
    Job& job;
    const FlatGraph& f;
    const JobDev& jd;                 // the region's device block, and its copy on the device
    const JobDev* jd_dev;
    const std::vector<int>& level_hi; // per level: the prefix of read ids a read_loglik row can hold (Worker::cluster)
    const int final_e0;               // the pseudo level of read_assign: one entry per read from here on
    const long total_copies;
    MailHold& mail;
    const sc_params& pa;
    const ld e, tau, diff;            // float widened, StrainCall.cpp:58-154
    const int K, n_reads;
    const bool want_trace;
    const LevelResult* const Rh;      // the slot's results, host-mapped

    std::vector<Model> models;                                           // pool; free entries in free_models
    std::vector<int> free_models, free_slots;                            // (free_slots: read_loglik rows no candidate holds)
    std::vector<PathRec> arena;
    std::vector<HStrain> level_strains, final_strains;
    std::vector<std::pair<int, int>> pending_copies;                     // (src slot, dst slot) for the next launch
    bool branching = false;
    int cur_level = 0;
    struct Cand { int parent; int node; ld abundance; };
    std::vector<Cand> cands;                                             // buffers of the walk, reused from level to level
    std::vector<int> first_child;
    std::vector<HStrain> kept_buf, sub_strains;
    int la_cache[MAXS];                                                  // the candidates' symbols, for the update after the level
    // where the host's time between two levels goes (sc_stats.host_us): [0] parameters of the level (log tables, the
    // host-mapped block), [1] results of the level into the candidates' models, pruning, [2] extension of the candidates
    double host_acc[3] = {0, 0, 0};
    double t_mark, t_last_done;
    FILE* level_log;                                                     // SC_LEVEL_LOG: diagnostics only

    LevelWalk(Worker& w, Job& job, const FlatGraph& f, const JobDev& jd, const JobDev* jd_dev, const std::vector<int>& level_hi,
              int final_e0, long total_copies, MailHold& mail)
        : w(w), job(job), f(f), jd(jd), jd_dev(jd_dev), level_hi(level_hi), final_e0(final_e0), total_copies(total_copies),
          mail(mail), pa(job.params), e((ld)pa.error_rate), tau((ld)pa.tau), diff((ld)pa.diff_rate), K(f.K),
          n_reads((int)job.reads.size()), want_trace(pa.want_trace != 0), Rh(w.Rh) {
        w.ev_used = 0;
        for (int i = MAXS - 1; i >= 0; i--) free_slots.push_back(i);
        {   // level_strains.push_back(Strain(100,e)), NonparametricClustering.cpp:281; Strain.cpp:41-71
            HStrain s{};
            s.model = model_new();
            Model& m = models[(size_t)s.model];
            m.ks = K;
            for (int i = 0; i < K * K; i++) m.sub[i] = 0;
            for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) m.sub[i * K + j] = (i == j) ? 100 * (1 - e) : 100 * e;
            recount(m);
            constexpr unsigned all_symbols = (1u << KMAX) - 1u;
            m.dirty = all_symbols;
            for (int a = 0; a < KMAX; a++) m.stale[a] = (uint16_t)all_symbols;
            s.abundance = 0; s.slot = free_slots.back(); free_slots.pop_back();
            s.tail = -1; s.node = -1; s.hash = 1469598103934665603ull; s.seqlen = 0;
            level_strains.push_back(s);
        }
        t_mark = t_last_done = now_ms();
        const Options& opt = w.ctx->plan.opt;
        level_log = opt.level_log ? fopen((opt.level_log_path + "." + std::to_string(w.slot)).c_str(), "a") : nullptr;
    }
    ~LevelWalk() { if (level_log) fclose(level_log); }
    // the levels in order (:284-334): their nodes, the update of the candidates (sampler once they branch), extension
    void run() {
        for (int level = 0; level < f.n_levels; level++) {
            visit_nodes(level);
            const int e0 = f.level_ent_ptr[level], e1 = f.level_ent_ptr[level + 1];
            const int Rn = e1 - e0;
            cur_level = level;
            if (Rn > 0 && !level_strains.empty()) {
                const int S = (int)level_strains.size();
                if (S > MAXS) throw ScError(SC_ERR_CAPACITY, "more than 128 candidate strains at one level");
                if ((long)S * K * K > (long)level_table_capacity())
                    throw ScError(SC_ERR_UNSUPPORTED, std::to_string(S) + " candidate strains over " + std::to_string(K) +
                                  " distinct symbols: their log tables do not fit the level kernel's LDS");
                bool has_dups = false, any_multi = false;
                for (int x = e0; x < e1; x++) { if (!f.ent_first[x]) has_dups = true; if (f.ent_lab_len[x] != 1) any_multi = true; }
                for (auto& s : level_strains) if (f.node_lab_len[s.node] != 1) any_multi = true;
                const int Q = f.level_read_count[level];
                if (branching) np_bayes_clustering(e0, e1, Q, has_dups, any_multi);
                else hard_clustering(e0, e1, Q, has_dups, any_multi);
            }
            trace_dump("after clustering", level, level_strains);
            lap(1);
            extend();
            lap(2);
        }
        read_assign();
        report();
    }
    // The nodes popped at this level: the root starts the first candidate's path; an end node runs read_reassign (only its
    // sort has an effect, :672-702) and merge_strains (:645-670).
    void visit_nodes(int level) {
        const int n0 = f.level_node_ptr[level], n1 = f.level_node_ptr[level + 1];
        for (int x = n0; x < n1; x++) {
            trace_dump("before clustering", level, level_strains);
            const int u = f.level_nodes[x];
            if (u == 0) {
                if (level_strains.empty()) throw ScError(SC_ERR_INTERNAL, "no strain at the root");
                HStrain& s = level_strains[0];
                arena.push_back({0, s.tail});
                s.tail = (int)arena.size() - 1; s.node = 0;
                s.hash = hash_extend(s.hash, f.node_label_str[0]); s.seqlen += (int)f.node_label_str[0].size();
                s.abundance = 1;
            } else if (f.node_is_end[u]) {
                // Every candidate pruned before the end of the gene: the reference runs into undefined behaviour here
                // (merged(1, strains[0]) of an empty vector, :650) and in practice prints nothing and exits 0; so does
                // this path (no contig for the region).
                if (level_strains.empty()) { final_strains.clear(); continue; }
                // sorted twice, as the reference does (read_reassign, then merge_strains): std_sort_perm is not stable
                sort_strains(level_strains);
                sort_strains(level_strains);
                std::vector<std::string> seqs;
                for (auto& s : level_strains) seqs.push_back(path_seq(s, false));
                std::vector<int> merged{0};
                for (int i = 1; i < (int)level_strains.size(); i++) {
                    size_t j;
                    for (j = 0; j < merged.size(); j++)
                        if (seq_identity(seqs[i], seqs[merged[j]]) > 1 - diff) {
                            level_strains[merged[j]].abundance += level_strains[i].abundance;
                            break;
                        }
                    if (j == merged.size()) merged.push_back(i);
                }
                std::vector<HStrain> kept;
                std::vector<char> keep(level_strains.size(), 0);
                for (int j : merged) { kept.push_back(level_strains[j]); keep[j] = 1; }
                for (size_t i = 0; i < level_strains.size(); i++) if (!keep[i]) drop(level_strains[i]);
                level_strains.swap(kept);
                final_strains = level_strains;
            }
        }
    }
    // One level on the GPU: its parameters into the slot's host-mapped block, the level handed over and waited for
    // (Worker::complete_level), its figures counted into job.stats.
    void run_level(int mode, int e0, int e1, int Q, int n_sweeps, bool do_update, const std::vector<HStrain>& sv,
                              bool has_dups, bool any_multi) {
        LevelParams& P = *w.Ph;
        const int S = (int)sv.size();
        LevelHdr H{};
        H.mode = mode; H.S = S; H.e0 = e0; H.e1 = e1; H.has_dups = has_dups; H.any_multi = any_multi; H.Q = Q;
        H.n_sweeps = n_sweeps; H.do_update = do_update ? 1 : 0;
        H.n_copy = (int)pending_copies.size();
        H.copy_n = do_update ? level_hi[(size_t)cur_level] : n_reads;
        GridParams& G = w.gp;                          // the same rows, symbols and copy pairs, for the grid kernels' arguments
        for (int c = 0; c < H.n_copy; c++) {
            P.copy_src[c] = pending_copies[c].first; P.copy_dst[c] = pending_copies[c].second;
            if ((unsigned)P.copy_src[c] >= (unsigned)MAXS || (unsigned)P.copy_dst[c] >= (unsigned)MAXS)
                throw ScError(SC_ERR_INTERNAL, "a row copy names a row outside the read_loglik matrix");
            G.copy_src[c] = (uint8_t)P.copy_src[c]; G.copy_dst[c] = (uint8_t)P.copy_dst[c];
        }
        pending_copies.clear();
        {   // every candidate owns its row of the read log-likelihood matrix
            uint64_t seen[2] = {0, 0};
            for (int s = 0; s < S; s++) {
                const int r = sv[s].slot;
                if (r < 0 || r >= MAXS || (seen[r >> 6] >> (r & 63)) & 1) throw ScError(SC_ERR_INTERNAL, "two candidates share a read_loglik row");
                seen[r >> 6] |= 1ull << (r & 63);
            }
        }
        // The region comes back to cold caches (hundreds of other regions have used this core since its last level): what the
        // loops below touch per candidate -- its node's label, its model's header and log table -- is asked for up front, all
        // candidates at once, instead of one miss after the other.
        for (int s = 0; s < S; s++) {
            const int nd = sv[s].node;
            if (nd >= 0) { __builtin_prefetch(&f.node_lab_off[(size_t)nd]); __builtin_prefetch(&f.node_lab_len[(size_t)nd]); }
            if (do_update) {
                const Model& hm = models[(size_t)sv[s].model];
                __builtin_prefetch(&hm.dirty); __builtin_prefetch(&hm.stale[0]);
                for (int o = 0; o < K * K; o += 8) __builtin_prefetch(&hm.lpc[o]);
            }
        }
        ld za = 0;
        for (int s = 0; s < S; s++) za += sv[s].abundance;                 // normalize(), :10-15
        for (int s = 0; s < S; s++) {
            StrainParam& sp = P.sp[s];
            sp.slot = sv[s].slot;
            sp.lab_off = sv[s].node >= 0 ? f.node_lab_off[sv[s].node] : 0;
            sp.lab_len = sv[s].node >= 0 ? f.node_lab_len[sv[s].node] : 0;
            la_cache[s] = (sp.lab_len == 1) ? (int)f.labels[(size_t)sp.lab_off] : -1;       // the candidate's symbol, for the update after the level
            sp.pad = 0;
            G.slot[s] = (uint8_t)sp.slot;                 // (0 .. MAXS - 1: checked above)
            G.lab[s] = sp.lab_len >= 1 ? f.labels[(size_t)sp.lab_off] : (uint8_t)0;
            sp.a0 = (double)sv[s].abundance;
            sp.logpri = (mode == MODE_HARD) ? (double)logl(sv[s].abundance / za) : 0.0;      // the sampler takes a0 itself
            w.hp.logpri[s] = sp.logpri;
            if (!do_update) continue;
            // log table of the strain: only the rows its counts changed in since the last level are redone, and in
            // them only the logarithms of the counts that changed
            Model& hm = models[(size_t)sv[s].model];
            for (int a = 0; a < K; a++) {
                if (!(hm.dirty & (1u << a))) continue;
                const ld lc = logl(a < 6 ? hm.comp[a] : (ld)0);                             // log comp_count[a], Strain.cpp:132-135
                for (int b = 0; b < K; b++) {
                    if (hm.stale[a] & (1u << b)) hm.lsub[a * K + b] = logl(hm.sub[a * K + b]);
                    hm.lpc[a * K + b] = (double)(hm.lsub[a * K + b] - lc);
                }
                hm.stale[a] = 0;
            }
            hm.dirty = 0;
            double* dst = P.lpt + (size_t)s * K * K;                                          // compact [K][K]
            std::memcpy(dst, hm.lpc, sizeof(double) * (size_t)K * K);
        }
        const bool chain = (mode == MODE_SAMPLE) && S > 1 && n_sweeps > 0;
        if (mode == MODE_SAMPLE && (long)n_sweeps * Q > jd.dlog_cap) throw ScError(SC_ERR_INTERNAL, "a level draws more than the region's draw log holds");
        const bool timed = chain && pa.want_timing && !w.grid;      // (no launch to bracket with events when the workers are resident)
        const bool lone = !w.grid && w.ctx->workers.size() == 1;      // launches its levels itself, grid kernels included (launch_level)
        if (!lone && level_wants_grid(jd.n_reads, H)) {
            // a very large level: row copies / the single-symbol update on a grid, from a device copy of the parameters
            const size_t bytes = offsetof(LevelParams, lpt) + sizeof(double) * (size_t)S * K * K;
            HIPCHK(hipMemcpyAsync(w.Pd, w.Ph, bytes, hipMemcpyHostToDevice, w.st));
            H.done = launch_level_grid(w.st, jd_dev, jd.n_reads, H, level_kind(H), w.gp, w.hp, w.Pd, w.Rd, false);
            w.sync_stream();                             // the level's kernel runs on another stream
        }
        const int ms = w.mslot.load(std::memory_order_relaxed);
        H.seq = ms >= 0 ? ++w.grid->mail_seq[(size_t)ms] : ++w.seq;     // (a mailbox keeps its own count: regions take turns on it)
        if (timed) {
            // a fresh pair of events per sampler launch; their times are read after the walk, not between levels
            if (w.ev_used + 2 > w.ev_pool.size()) {
                hipEvent_t a = nullptr, b = nullptr;
                HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
                w.ev_pool.push_back(a); w.ev_pool.push_back(b);
            }
            w.ev0 = w.ev_pool[w.ev_used]; w.ev1 = w.ev_pool[w.ev_used + 1];
            w.ev_used += 2;
        }
        const double t_launched = level_log ? now_ms() : 0.0;
        lap(0);
        const LevelItem it = w.level_item(jd_dev, H, K);
        w.complete_level(it, jd.n_reads, timed);
        t_mark = now_ms();                                   // (the wait for the level is not host work)
        sc_stats& stats = job.stats;
        stats.level_launches++;
        if (chain) {
            stats.sampler_launches++; stats.sampler_read_copies += Q;
            stats.draws += (long)Rh->n_draws; stats.exact_draws += (long)Rh->n_exact; stats.slow_draws += (long)Rh->n_slow;
            stats.sampler_strains += S; stats.chain_passes += (long)Rh->n_pass;
            stats.chain_cycles += (long)Rh->chain_cycles; stats.chain_wall_ticks += (long)Rh->chain_wall;
        }
        stats.level_kernel_ticks += (long)Rh->level_wall;
        if (chain) stats.sampler_level_ticks += (long)Rh->level_wall;
        if (level_log) {
            const double t_done = now_ms();
            fprintf(level_log, "h %d mode %d S %d Q %d n %d level_us %.1f chain_us %.1f cyc %llu passes %llu slow %llu xcc %d ncopy %d copyn %d multi %d dups %d done %d "
                    "ph %.1f %.1f %.1f %.1f %.1f %.1f host_us %.1f wait_us %.1f pend_us %.1f batch %d\n", job.handle, mode, S, Q,
                    n_sweeps, Rh->level_wall * 0.01, chain ? Rh->chain_wall * 0.01 : 0.0, chain ? (unsigned long long)Rh->chain_cycles : 0ull,
                    chain ? (unsigned long long)Rh->n_pass : 0ull, chain ? (unsigned long long)Rh->n_slow : 0ull, Rh->xcc, H.n_copy, H.copy_n, (int)any_multi, (int)has_dups, w.level_done,
                    Rh->phase_ticks[0] * 0.01, Rh->phase_ticks[1] * 0.01, Rh->phase_ticks[2] * 0.01, Rh->phase_ticks[3] * 0.01, Rh->phase_ticks[4] * 0.01,
                    chain ? Rh->phase_ticks[5] * 0.01 : 0.0,         // (the end of the count over the draw log: sampler levels only)
                    1e3 * (t_launched - t_last_done), 1e3 * (t_done - t_launched), 1e3 * (w.t_batch_launched - t_launched), w.batch_n);
            t_last_done = t_done;
        }
        stats.xcd_levels[Rh->xcc & 7]++;
        stats.kind_levels[std::min(std::max(item_kind(it.kind), 0), N_SAMPLER_KINDS)]++;
    }
    // np_bayes_clustering, :128-244 (+ pruning :404-454)
    void np_bayes_clustering(int e0, int e1, int Q, bool has_dups, bool any_multi) {
        const int S = (int)level_strains.size();
        const int n = level_sweeps(pa, Q);
        int last[MAXS];
        for (int s = 0; s < S; s++) {
            last[s] = s;
            for (int t = S - 1; t > s; t--)
                if (level_strains[t].hash == level_strains[s].hash && level_strains[t].seqlen == level_strains[s].seqlen) { last[s] = t; break; }
        }
        ld prior[MAXS], post[MAXS], a[MAXS];
        for (int s = 0; s < S; s++) prior[s] = level_strains[last[s]].abundance;
        run_level(MODE_SAMPLE, e0, e1, Q, n, true, level_strains, has_dups, any_multi);
        ld (*cnt)[KMAX] = reinterpret_cast<ld (*)[KMAX]>(w.cnt_scratch.data());     // (not thread_local: the fiber changes threads)
        for (int s = 0; s < S; s++) {                      // (cold caches: see run_level)
            const Model& m_ = models[(size_t)level_strains[s].model];
            __builtin_prefetch(&Rh->cnt[s * KMAX]);
            if ((s & 15) == 0) __builtin_prefetch(&Rh->kdraw[s]);
            __builtin_prefetch(&m_.comp[0]); __builtin_prefetch(&m_.comp[4]); __builtin_prefetch(&m_.stale[0]);
            const int la = la_cache[s];
            if (la >= 0 && la < K) { __builtin_prefetch(&m_.sub[la * K]); __builtin_prefetch(&m_.sub[la * K + 4]); }
        }
        for (int s = 0; s < S; s++) for (int b = 0; b < K; b++) cnt[s][b] = 0;
        if (S == 1 || n <= 0) {
            // a single weight consumes no random numbers (libstdc++ discrete_distribution)
            a[0] = level_strains[0].abundance;
            for (int s = 1; s < S; s++) a[s] = level_strains[s].abundance;
            if (n > 0) {
                const long tot = (long)n * Q;
                a[0] = sc_add_ones(a[0], (unsigned long)tot);
                for (int x = e0; x < e1; x++)
                    if (f.ent_lab_len[x] == 1) cnt[0][f.labels[f.ent_lab_off[x]]] += (ld)n * f.ent_cn[x];
            }
        } else {
            for (int s = 0; s < S; s++) {
                a[s] = sc_add_ones(level_strains[s].abundance, Rh->kdraw[s]);     // a[c] += 1 per draw, :195 (one rounding per draw)
                for (int b = 0; b < K; b++) cnt[s][b] = (ld)Rh->cnt[s * KMAX + b];
            }
        }
        ld z = 0;
        for (int s = 0; s < S; s++) z += a[s];
        for (int s = 0; s < S; s++) a[s] /= z;
        for (int s = 0; s < S; s++) a[s] *= Q;
        for (int s = 0; s < S; s++) {
            HStrain& st_ = level_strains[s];
            Model& m_ = models[(size_t)st_.model];
            st_.abundance += a[s];                                   // update_model, Strain.cpp:106-125
            unsigned changed = 0;
            {
                const int la = la_cache[s];                          // the symbol of the candidate's node (single-symbol labels only)
                if (la >= 0 && la < K) {
                    for (int b = 0; b < K; b++)
                        if (cnt[s][b] > 0) { m_.sub[la * K + b] += cnt[s][b] / n; m_.stale[la] |= (uint16_t)(1u << b); }
                    m_.dirty |= 1u << la;
                    changed = 1u << la;
                }
            }
            recount_rows(m_, changed);
        }
        for (int s = 0; s < S; s++) post[s] = level_strains[last[s]].abundance;
        ld A_delta_max = 0;
        for (int s = 0; s < S; s++) { ld d = post[s] - prior[s]; if (A_delta_max < d) A_delta_max = d; }
        ld Z = 0;
        for (int s = 0; s < S; s++) Z += a[s];
        const ld Zt = Z * tau;
        std::vector<HStrain>& kept = kept_buf;               // (the walk's own: no allocation per level)
        kept.clear();
        for (int s = 0; s < S; s++) {
            const ld d = post[s] - prior[s];
            if (a[s] < Zt || d < 0.01 * A_delta_max) drop(level_strains[s]);
            else kept.push_back(level_strains[s]);
        }
        level_strains.swap(kept);
    }
    // hard_clustering, :17-125
    void hard_clustering(int e0, int e1, int Q, bool has_dups, bool any_multi) {
        const int S = (int)level_strains.size();
        run_level(MODE_HARD, e0, e1, Q, 0, true, level_strains, has_dups, any_multi);
        for (int s = 0; s < S; s++) {                      // (cold caches: see run_level)
            const Model& m_ = models[(size_t)level_strains[s].model];
            for (int o = 0; o < K * K; o += 8) __builtin_prefetch(&Rh->subst[(size_t)s * K * K + o]);
            for (int o = 0; o < K * K; o += 4) __builtin_prefetch(&m_.sub[o]);
            __builtin_prefetch(&m_.comp[0]); __builtin_prefetch(&m_.comp[4]); __builtin_prefetch(&m_.stale[0]);
            if ((s & 7) == 0) __builtin_prefetch(&Rh->abund[s]);
        }
        for (int s = 0; s < S; s++) {
            HStrain& st_ = level_strains[s];
            Model& m_ = models[(size_t)st_.model];
            st_.abundance += (ld)Rh->abund[s];
            const double* sub_d = Rh->subst + (size_t)s * K * K;      // compact [K][K]
            unsigned changed = 0;
            for (int a = 0; a < K; a++)
                for (int b = 0; b < K; b++) {
                    const double d = sub_d[a * K + b];
                    if (d != 0.0) {                                   // (x + 0.0 == x for every x the counts can hold: they are never -0)
                        m_.sub[a * K + b] += (ld)d;
                        m_.dirty |= 1u << a; m_.stale[a] |= (uint16_t)(1u << b); changed |= 1u << a;
                    }
                }
            recount_rows(m_, changed);
        }
    }
    // candidate extension, :473-551
    void extend() {
        branching = false;
        cands.clear();
        for (const HStrain& s : level_strains) __builtin_prefetch(&f.out_ptr[(size_t)s.node]);
        for (const HStrain& s : level_strains) {
            const int ob = f.out_ptr[(size_t)s.node];
            __builtin_prefetch(&f.out_node[(size_t)ob]); __builtin_prefetch(&f.out_support[(size_t)ob]);
        }
        for (int si = 0; si < (int)level_strains.size(); si++) {
            const HStrain& s = level_strains[si];
            const int v = s.node;
            const int ob = f.out_ptr[v], oe = f.out_ptr[v + 1];
            ld oz = 0, moc = 0;
            for (int x = ob; x < oe; x++) { const ld oc0 = f.out_support[x]; oz += oc0; if (moc < oc0) moc = oc0; }
            int dd = 0;
            for (int x = ob; x < oe; x++) {
                const int o = f.out_node[x];
                const ld oc = f.out_support[x];
                if (!f.node_is_end[o] && oz > 0) {
                    if (oc <= 1. && oc < moc) { dd += 1; continue; }
                    ld ab;
                    if (oc > 0) ab = s.abundance * oc / oz;
                    else ab = oz * std::min(0.01, (double)tau);
                    cands.push_back({si, o, ab});
                } else {
                    cands.push_back({si, o, s.abundance});
                }
            }
            if (oe - ob > 1 + dd) branching = true;
        }
        if ((int)cands.size() > pa.max_candidates) {                          // :532-551, Qx :246-254
            std::vector<ld> ssa;
            for (auto& c : cands) ssa.push_back(c.abundance);
            std::sort(ssa.begin(), ssa.end(), [](ld x, ld y) { return x > y; });
            const ld Zt0 = (pa.max_candidates >= (int)ssa.size()) ? ssa.back() : ssa[pa.max_candidates];
            std::vector<Cand> kept;
            for (auto& c : cands) if (!(c.abundance < Zt0)) kept.push_back(c);
            cands.swap(kept);
        }
        if ((int)cands.size() > MAXS) throw ScError(SC_ERR_CAPACITY, "more than 128 candidate strains at one level");
        // materialise: the first surviving child of a parent inherits its row, the others copy it
        first_child.assign(level_strains.size(), -1);
        for (int c = 0; c < (int)cands.size(); c++) if (first_child[cands[c].parent] < 0) first_child[cands[c].parent] = c;
        for (size_t p = 0; p < level_strains.size(); p++) if (first_child[p] < 0) drop(level_strains[p]);
        sub_strains.clear();
        for (int c = 0; c < (int)cands.size(); c++) {
            const HStrain& par = level_strains[cands[c].parent];
            HStrain ns = par;
            if (first_child[cands[c].parent] == c) { ns.slot = par.slot; ns.model = par.model; }
            else {
                if (free_slots.empty()) throw ScError(SC_ERR_CAPACITY, "out of read_loglik rows");
                ns.slot = free_slots.back(); free_slots.pop_back();
                pending_copies.push_back({par.slot, ns.slot});
                ns.model = model_new();                                  // (may move the pool: take the source by index)
                models[(size_t)ns.model] = models[(size_t)par.model];
            }
            arena.push_back({cands[c].node, par.tail});
            ns.tail = (int)arena.size() - 1; ns.node = cands[c].node;
            ns.hash = hash_extend(par.hash, f.node_label_str[cands[c].node]);
            ns.seqlen = par.seqlen + (int)f.node_label_str[cands[c].node].size();
            ns.abundance = cands[c].abundance;
            sub_strains.push_back(ns);
        }
        level_strains.swap(sub_strains);
        sub_strains.clear();
    }
    // read_assign, :776-836, then the final sort, StrainCall.cpp:1027
    void read_assign() {
        std::vector<HStrain>& fs = final_strains;
        const int S = (int)fs.size();
        if (S == 0) return;
        const int Q = (int)total_copies;
        const int n = level_sweeps(pa, Q);
        std::vector<ld> a(S);
        if (S == 1 || n <= 0) {
            for (int s = 0; s < S; s++) a[s] = fs[s].abundance;
            if (n > 0) a[0] = sc_add_ones(a[0], (unsigned long)((long)n * Q));
        } else {
            pending_copies.clear();
            run_level(MODE_SAMPLE, final_e0, final_e0 + n_reads, Q, n, false, fs, false, true);
            for (int s = 0; s < S; s++) {
                a[s] = sc_add_ones(fs[s].abundance, Rh->kdraw[s]);                   // :823, one rounding per draw
            }
        }
        // The last level is done: the mailbox goes to the next region.  What is left of this one -- its sequences, and giving
        // back what the walk has allocated (the graph, the candidates' models: milliseconds of free()) -- is a long stretch, and
        // those belong on the pool's set-up threads: on a continuation thread it would hold up ~100 levels of other regions.
        mail.drop();
        if (w.ctx->gate.split_exec && FiberPool::in_fiber()) FiberPool::yield();
        ld z = 0;
        for (int s = 0; s < S; s++) z += a[s];
        for (int s = 0; s < S; s++) fs[s].abundance = a[s] / z;
        sort_strains(fs);
        for (auto& s : fs) {
            job.seqs.push_back(path_seq(s, true));
            job.abund.push_back((double)s.abundance);
        }
    }
    // The walk's figures into job.stats (the counters of every level are there already); the event pairs of the timed levels
    // are read now, after the walk.
    void report() {
        for (size_t k = 0; k + 1 < w.ev_used; k += 2) {
            float ms = 0;
            HIPCHK(hipEventSynchronize(w.ev_pool[k + 1]));
            HIPCHK(hipEventElapsedTime(&ms, w.ev_pool[k], w.ev_pool[k + 1]));
            job.stats.sampler_kernel_ms += ms;
        }
        w.ev_used = 0;
        for (int k = 0; k < 3; k++) job.stats.host_us[k] = 1e3 * host_acc[k];
        for (int k = 0; k < 2; k++) { job.stats.wake_us[k] = 1e3 * w.wake_acc[k]; w.wake_acc[k] = 0; }
    }

    int model_new() {
        if (!free_models.empty()) { const int m = free_models.back(); free_models.pop_back(); return m; }
        models.emplace_back();
        return (int)models.size() - 1;
    }
    void drop(const HStrain& s) { free_slots.push_back(s.slot); free_models.push_back(s.model); }
    void lap(int k) { const double t = now_ms(); host_acc[k] += t - t_mark; t_mark = t; }
    // the labels along the strain's path, root first: all of them (strain_seq), or without ^ $ - = (Strain::plain_seq,
    // Strain.cpp:211-223)
    std::string path_seq(const HStrain& s, bool plain) const {
        std::vector<int> rev;
        for (int t = s.tail; t >= 0; t = arena[t].parent) rev.push_back(arena[t].node);
        std::string q;
        for (auto it = rev.rbegin(); it != rev.rend(); ++it) {
            const std::string& pl = f.node_label_str[*it];
            if (!plain || (pl != "^" && pl != "$" && pl != "-" && pl != "=")) q += pl;
        }
        return q;
    }
    void trace_dump(const char* when, int level, const std::vector<HStrain>& sv) {
        if (!want_trace || sv.empty()) return;
        std::string& tr = job.trace;
        tr += "------------------------------\n"; tr += when; tr += "\nlevel: "; tr += std::to_string(level); tr += "\n";
        for (const auto& s : sv) { tr += path_seq(s, false); tr += "\t"; fmt_g17(tr, (double)s.abundance); tr += "\n"; }
    }
    static void sort_strains(std::vector<HStrain>& sv) {                 // std::sort, abundance descending
        std::vector<int> perm(sv.size());
        for (size_t i = 0; i < sv.size(); i++) perm[i] = (int)i;
        std_sort_perm(perm, [&](int a, int b) { return sv[a].abundance > sv[b].abundance; });
        std::vector<HStrain> t;
        t.reserve(sv.size());
        for (int i : perm) t.push_back(sv[i]);
        sv.swap(t);
    }
    static ld seq_identity(const std::string& a, const std::string& b) {  // NonparametricClustering.cpp:584-612
        int iden = 0, len = 0;
        for (size_t i = 0; i < a.size(); ++i) {
            const char x = a[i], y = i < b.size() ? b[i] : 0;
            if (x == '-' && y == '-') continue;
            else if (x == '=' && y == '=') continue;
            else if (x == '=' && y == '-') continue;
            else if (x == '-' && y == '=') continue;
            else if (x == '^' && y == '^') continue;
            else if (x == y) iden += 1;
            len += 1;
        }
        return (ld)((iden + 0.0) / len);
    }
};

void walk_levels(Worker& w, Job& job, const FlatGraph& f, const JobDev& jd, const JobDev* jd_dev, const std::vector<int>& level_hi,
                 int final_e0, long total_copies, MailHold& mail) {
    LevelWalk(w, job, f, jd, jd_dev, level_hi, final_e0, total_copies, mail).run();
}

}  // namespace sc
