// The per-sample gene profile on the device: every read segment of a sample against every assembled gene on both strands
// (DESIGN.md §8.9 is the contract) -- what scripts/per_sample_gene_profile_fast.py:80-153 runs makeblastdb, blastn,
// bigBlastParser and sqlite3 for.  One translation unit in four parts:
//   * sc_profile_dp.hpp      the cell, the score and traceback kernels, E-values
//   * sc_profile_seed.hpp    the seeded mode: the genes' k-mer index, the pair list, the seed length
//   * sc_profile_counts.hpp  the counts mode: the strand pick, the rounds and the counting rule on the device
//   * this file              what every entry point shares -- the front end (ProfileInput: checks, packing, least passing
//                            scores, seed length, device copies) and the score pass (ScorePass: the pair list when seeded, then
//                            k_bl_score / k_bl_score_pairs per bucket into a candidate buffer) -- then the body of
//                            sc_profile_hits and sc_profile_hits_seeded and the C entry points, those of the index that keeps
//                            the genes on the device from call to call among them (sc_profile_index_*).
#include <cstring>
#include <memory>

#include "sc_profile_seed.hpp"

namespace {

thread_local sc::LastError tl_error;

// The genes of an index that outlives its calls (sc_profile_index): packed on the host and copied to the device once.
struct ResidentGenes {
    Packed gn;
    sc::DevMem<uint8_t> gq;
    sc::DevMem<long> go;
    explicit ResidentGenes(Packed&& packed) : gn(std::move(packed)), gq(gn.codes), go(gn.off) {}
};
// Where a call on such an index puts its segments: arrays that grow when a call needs more and are kept otherwise.
struct SegArena {
    sc::DevArr<uint8_t> sq;
    sc::DevArr<long> so;
    sc::DevArr<int> min2;
};

// The front end of a call: the arguments every entry point takes, checked (check), packed on the host with what the score
// pass needs per segment (prepare), and copied to the device (upload).  `fn` names the entry point in messages.
struct ProfileInput {
    const std::string fn;
    const char* const gene_text; const long* const gene_off; const int n_genes;
    const char* const seg_text; const long* const seg_off; const int n_segs;
    const double min_identity_pct, max_evalue, ka_lambda, ka_k;
    Packed gn, sg;
    long gene_bytes = 0;
    double t0 = 0;                                              // when the host's work began
    int min2_of_len[MAX_ROWS + 1] = {};                         // per segment length the least doubled score with E <= T; 0: no such segment
    bool has_len[MAX_ROWS + 1] = {};                            // the lengths of the segments that can pass
    std::vector<int> min2;                                      // min2_of_len per segment
    int seed_k = 0;                                             // the seeded mode's k; 0 runs the full product
    template <class T> struct Ref { T* p = nullptr; };
    struct Dev {
        Ref<uint8_t> gq, sq;                                    // codes of the genes, of the segments
        Ref<long> go, so;                                       // their offsets
        Ref<int> min2;
    };
    struct Own {                                                // the arrays of a call that keeps nothing
        sc::DevMem<uint8_t> gq, sq;
        sc::DevMem<long> go, so;
        sc::DevMem<int> min2;
        explicit Own(const ProfileInput& in)
            : gq(in.gn.codes.size()), sq(in.sg.codes.size()), go(in.gn.off.size()), so(in.sg.off.size()), min2(in.min2.size()) {}
    };
    std::unique_ptr<Dev> dev;
    std::unique_ptr<Own> owned;
    const ResidentGenes* resident = nullptr;                    // set: the genes are these, gene_text and gene_off are not read

    ProfileInput(const char* fn_, const char* gene_text_, const long* gene_off_, int n_genes_, const char* seg_text_, const long* seg_off_,
                 int n_segs_, double min_identity_pct_, double max_evalue_, double ka_lambda_, double ka_k_)
        : fn(fn_), gene_text(gene_text_), gene_off(gene_off_), n_genes(n_genes_), seg_text(seg_text_), seg_off(seg_off_), n_segs(n_segs_),
          min_identity_pct(min_identity_pct_), max_evalue(max_evalue_), ka_lambda(ka_lambda_), ka_k(ka_k_) {}

    static void pack_genes(Packed& g, const char* text) { g.pack(text, [](long, int c) { return c < 0 ? REF_OTHER : c; }); }

    // SC_ERR_ARG unless the sequences are there, the caller's own arguments are (`own`), and the thresholds make sense
    int check(bool own) const {
        if (!own || (!resident && (!gene_text || !gene_off)) || n_genes < 1 || n_segs < 0 || (n_segs > 0 && (!seg_text || !seg_off)))
            return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        if (!(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0))
            return tl_error.fail(SC_ERR_ARG, fn + ": lambda and K must be positive, the E-value threshold not negative");
        return SC_OK;
    }

    // The lengths checked (SC_ERR_UNSUPPORTED), the device selected (sc::select_device throws); then, unless there is no
    // segment, the host packing: gene and segment codes, per segment the least passing score (a segment that cannot pass even
    // with every base matched is scored nowhere), and with `seeded` the seed length from the lengths that can pass.  Resident
    // genes were checked and packed when their index was created.
    int prepare(int device, bool seeded) {
        std::string why;
        if ((!resident && !gn.rebase(gene_off, n_genes, MAX_COLS, fn.c_str(), "gene", why)) ||
            (n_segs > 0 && !sg.rebase(seg_off, n_segs, MAX_ROWS, fn.c_str(), "segment", why)))
            return tl_error.fail(SC_ERR_UNSUPPORTED, why);
        sc::select_device(device);
        if (n_segs == 0) return SC_OK;
        t0 = sc::now_ms();
        if (!resident) pack_genes(gn, gene_text + gene_off[0]);
        sg.pack(seg_text + seg_off[0], [](long, int c) { return c < 0 ? 4 : c; });
        gene_bytes = resident ? resident->gn.bytes() : gn.bytes();
        min2.resize((size_t)n_segs);
        for (int r = 0; r < n_segs; r++) {
            const int L = (int)sg.len(r);
            int& s2 = min2_of_len[L];
            if (s2 == 0) s2 = least_score2(ka_k, ka_lambda, L, gene_bytes, max_evalue);     // a hit has a positive score
            min2[(size_t)r] = s2;
            if (can_pass(r)) has_len[L] = true;
        }
        if (seeded) seed_k = seed_length(has_len, gene_bytes, min_identity_pct, max_evalue, ka_lambda, ka_k, nullptr);
        return SC_OK;
    }
    bool can_pass(int seg) const { return min2[(size_t)seg] <= MATCH2 * sg.len(seg); }

    // The device copies, enqueued behind the mark "upload"
    void upload(sc::TimedStream& st) {
        owned.reset(new Own(*this));
        dev.reset(new Dev{{owned->gq.p}, {owned->sq.p}, {owned->go.p}, {owned->so.p}, {owned->min2.p}});
        st.mark("upload");
        st.h2d(owned->gq, gn.codes); st.h2d(owned->go, gn.off);
        upload_segments(st);
    }
    // The same for a call on resident genes: only the segments travel, into `arena`
    void upload(sc::TimedStream& st, SegArena& arena) {
        dev.reset(new Dev{{resident->gq.p}, {arena.sq.ensure(sg.codes.size() + 1)}, {resident->go.p}, {arena.so.ensure(sg.off.size())},
                          {arena.min2.ensure(min2.size() + 1)}});
        st.mark("upload");
        upload_segments(st);
    }
    void upload_segments(sc::TimedStream& st) {
        st.h2d(dev->sq.p, sg.codes.data(), sg.codes.size()); st.h2d(dev->so.p, sg.off.data(), sg.off.size() * sizeof(long));
        st.h2d(dev->min2.p, min2.data(), min2.size() * sizeof(int));
    }
};

// Where a score pass puts its candidates: room for `cap` records and their counter, zeroed by the caller.
struct CandBuf { Cand* p; long cap; unsigned* n; };

// The score pass over bucketed segments (`sids` = by_r.order(), d_sids on the device), enqueued on `st` by the constructor:
// every passing tile appends a candidate.  With an index the (segment, gene) pairs that share a k-mer are listed first
// (seed_pairs: the stream is synchronised) and only their tiles are scored; without, the full product.  The mark "score" is
// set in front of the kernels.  *score_cells grows by the cells of the tiles.  The pair list lives in `sx`.
struct ScorePass {
    long n_tiles = 0, n_pairs = 0;
    ScorePass(sc::TimedStream& st, const ProfileInput& in, const Buckets& by_r, const std::vector<int>& sids, const int* d_sids,
              const SeedIndex* index, SeedScratch& sx, CandBuf cand, long* score_cells) {
        const ProfileInput::Dev& d = *in.dev;
        const int n_genes = in.n_genes;
        std::vector<long> pair_off(sids.size() + 1, 0);
        n_tiles = (long)sids.size() * 2L * n_genes;
        if (index) {
            n_pairs = seed_pairs(st, *index, d.go.p, n_genes, d.sq.p, d.so.p, in.sg, by_r, sids, d_sids, in.seed_k, pair_off, sx, score_cells);
            n_tiles = 2L * n_pairs;
        }
        if (n_tiles > 0x7FFFFFFFL)
            throw sc::ScError(SC_ERR_UNSUPPORTED, in.fn + ": " + std::to_string(n_tiles) + " (segment, gene, strand) tiles in one call (at most "
                                                      "2147483647: pass the segments in several calls)");
        st.mark("score");
        by_r.each([&](auto r, long at, const std::vector<int>& ids) {
            if (index) {
                const long nt = 2L * (pair_off[(size_t)at + ids.size()] - pair_off[(size_t)at]);
                if (nt == 0) return;
                hipLaunchKernelGGL(k_bl_score_pairs<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d.gq.p, d.go.p, d.sq.p, d.so.p,
                                   PairTiles{sx.pairs.get() + pair_off[(size_t)at]}, d.min2.p, nt, cand.p, (unsigned)cand.cap, cand.n);
                st.launched();
                return;
            }
            const long nt = (long)ids.size() * 2L * n_genes;
            hipLaunchKernelGGL(k_bl_score<decltype(r)::value>, score_grid(nt), dim3(64 * SCORE_WAVES), 0, st, d.gq.p, d.go.p, d.sq.p, d.so.p,
                               AllTiles{n_genes, d_sids + at}, d.min2.p, nt, cand.p, (unsigned)cand.cap, cand.n);
            st.launched();
            for (int id : ids) *score_cells += 2L * in.sg.len(id) * in.gene_bytes;
        });
    }
};

}  // namespace

#include "sc_profile_counts.hpp"        // the counts mode is built on ProfileInput and ScorePass above

namespace {

// The caller's arrays of an entry point that returns hits
struct HitsOut {
    int *seg, *gene, *strand;
    double* score;
    int *identity, *align_len, *qfrom, *qto, *hfrom, *hto;
    double* evalue;
    long cap;
    bool complete() const { return seg && gene && strand && score && identity && align_len && qfrom && qto && hfrom && hto && evalue && cap >= 0; }
};

// Per (segment, gene) the better strand of the candidate tiles (ties: forward), in (segment, gene) order
std::vector<Cand> pick_strands(std::vector<Cand> cand) {
    std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.seg != b.seg ? a.seg < b.seg : a.gene2 < b.gene2; });
    std::vector<Cand> pick;
    for (size_t k = 0; k < cand.size(); k++) {
        if (!pick.empty() && pick.back().seg == cand[k].seg && (pick.back().gene2 >> 1) == (cand[k].gene2 >> 1)) {
            if (key_score2(cand[k].key) > key_score2(pick.back().key)) pick.back() = cand[k];          // reverse only when strictly better
        } else {
            pick.push_back(cand[k]);
        }
    }
    return pick;
}

// The traceback of the picked tiles, bucketed by rows per lane again, between the marks "trace" and "traced"; the stream is
// synchronised.  out[4 * slot_of[k] ..] is what k_bl_trace wrote for pick[k].
struct Traced { std::vector<int> slot_of, out; };
Traced trace_hits(sc::TimedStream& st, const ProfileInput& in, const std::vector<Cand>& pick) {
    Buckets tr_r;
    for (size_t k = 0; k < pick.size(); k++) tr_r.add((int)k, in.sg.len(pick[k].seg));
    const std::vector<int> order = tr_r.order();
    const int n_tr = (int)order.size();
    std::vector<Cand> tlist((size_t)n_tr);
    for (int t = 0; t < n_tr; t++) tlist[(size_t)t] = pick[(size_t)order[(size_t)t]];
    Traced tr{std::vector<int>((size_t)n_tr), std::vector<int>((size_t)n_tr * 4)};
    sc::DevMem<Cand> d_hits((size_t)n_tr);
    sc::DevMem<int> d_out(tr.out.size());
    const ProfileInput::Dev& d = *in.dev;
    st.h2d(d_hits, tlist);
    st.mark("trace");
    tr_r.each([&](auto r, long at, const std::vector<int>& ids) {
        hipLaunchKernelGGL(k_bl_trace<decltype(r)::value>, trace_grid((int)ids.size()), dim3(64), 0, st, d.gq.p, d.go.p, d.sq.p, d.so.p,
                           d_hits.p + at, (int)ids.size(), d_out.p + 4 * at);
        st.launched();
    });
    st.mark("traced");
    st.d2h(tr.out, d_out);
    st.sync();
    for (int t = 0; t < n_tr; t++) tr.slot_of[(size_t)order[(size_t)t]] = t;
    return tr;
}

// The traced pairs that pass both thresholds go to the caller's arrays in (segment, gene) order; *n_hits is their number
// (SC_ERR_CAPACITY when that is more than out.cap).  A failed walk: SC_ERR_INTERNAL.
int emit_hits(const ProfileInput& in, const std::vector<Cand>& pick, const Traced& tr, const HitsOut& out, long* n_hits,
              sc_profile_seed_stats& stats) {
    long n_out = 0;
    for (size_t k = 0; k < pick.size(); k++) {
        const Cand& c = pick[k];
        const int* o = &tr.out[(size_t)tr.slot_of[k] * 4];
        if (o[0] < 0)
            return tl_error.fail(SC_ERR_INTERNAL, in.fn + ": traceback of segment " + std::to_string(c.seg) + " on gene " +
                                                      std::to_string(c.gene2 >> 1) + " failed");
        const int L = (int)in.sg.len(c.seg);
        const int S2 = key_score2(c.key), jend = key_col(c.key), iend = key_row(c.key);
        const int strand = c.gene2 & 1, j0 = o[0], i0 = o[1];
        const Window w = trace_window<BlCell>(S2, jend, iend + 1);
        stats.trace_cells += window_cells(w, iend + 1, j0 - w.j0);
        const double e = evalue_of(in.ka_k, in.ka_lambda, L, in.gene_bytes, S2);
        if (!(100.0 * (double)o[2] / (double)o[3] >= in.min_identity_pct) || !(e <= in.max_evalue)) continue;
        if (n_out < out.cap) {
            out.seg[n_out] = c.seg; out.gene[n_out] = c.gene2 >> 1; out.strand[n_out] = strand;
            out.score[n_out] = 0.5 * (double)S2; out.identity[n_out] = o[2]; out.align_len[n_out] = o[3];
            out.qfrom[n_out] = strand ? L - iend : i0 + 1;
            out.qto[n_out] = strand ? L - i0 : iend + 1;
            out.hfrom[n_out] = strand ? jend + 1 : j0 + 1;
            out.hto[n_out] = strand ? j0 + 1 : jend + 1;
            out.evalue[n_out] = e;
        }
        n_out++;
    }
    *n_hits = n_out;
    if (n_out > out.cap) return tl_error.fail(SC_ERR_CAPACITY, in.fn + ": " + std::to_string(n_out) + " hits, room for " + std::to_string(out.cap));
    return SC_OK;
}

// The body of sc_profile_hits and, with `seeded`, of sc_profile_hits_seeded, under the guard; `fn` names the entry point in
// messages.  `stats` is the superset both report from.
int profile_hits(const char* fn, int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                 int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, bool seeded, const HitsOut& out,
                 long* n_hits, sc_profile_seed_stats& stats) {
    ProfileInput in(fn, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct, max_evalue, ka_lambda, ka_k);
    if (n_hits) *n_hits = 0;
    if (const int rc = in.check(out.complete() && n_hits)) return rc;
    if (const int rc = in.prepare(device, seeded); rc != SC_OK || n_segs == 0) return rc;
    stats.seed_k = in.seed_k;
    // the segments that can pass, bucketed by rows per lane
    Buckets by_r;
    for (int r = 0; r < n_segs; r++) if (in.can_pass(r)) by_r.add(r, in.sg.len(r));
    const std::vector<int> sids = by_r.order();
    // every passing tile is a candidate; a (segment, gene) pair gives at most two, so 2 * cap + 1024 records hold them unless
    // the caller's cap is too small as well
    const long cand_cap = std::min<long>((long)sids.size() * 2L * n_genes, std::min<long>(2 * out.cap + 1024, 0x7FFFFFFFL));
    sc::DevMem<int> d_sids(sids.size());
    sc::DevMem<unsigned> d_ncand(1);
    sc::DevMem<Cand> d_cand((size_t)cand_cap);
    sc::TimedStream st;
    in.upload(st);
    st.h2d(d_sids, sids);
    st.zero(d_ncand.p, sizeof(unsigned));
    // ---- seeded only: the genes' k-mers sorted by (code, gene); the score pass lists the pairs from them
    std::unique_ptr<SeedIndex> index;
    if (in.seed_k && !sids.empty()) {
        st.mark("index");
        index.reset(new SeedIndex(st, in.dev->gq.p, in.dev->go.p, n_genes, in.gene_bytes, in.seed_k));
        st.mark("lookup");
        st.sync();
        stats.n_gene_kmers = (long)index->n_keys;
    }
    SeedScratch sx;
    const ScorePass pass(st, in, by_r, sids, d_sids.p, index.get(), sx, CandBuf{d_cand.p, cand_cap, d_ncand.p}, &stats.score_cells);
    st.mark("scored");
    unsigned n_cand = 0;
    st.d2h(&n_cand, d_ncand.p, sizeof(unsigned));
    st.sync();
    stats.n_pairs = pass.n_pairs; stats.n_tiles = pass.n_tiles; stats.n_candidates = (long)n_cand;
    int rc = SC_OK;
    if ((long)n_cand > cand_cap) {
        *n_hits = (long)n_cand;                                  // an upper bound of the hits: a cap of this size suffices
        rc = tl_error.fail(SC_ERR_CAPACITY, in.fn + ": " + std::to_string(n_cand) + " tiles pass the E-value threshold, room for " +
                                                std::to_string(out.cap) + " hits");
    } else {
        std::vector<Cand> cand(n_cand);
        if (n_cand) HIPCHK(hipMemcpy(cand.data(), d_cand.p, (size_t)n_cand * sizeof(Cand), hipMemcpyDeviceToHost));
        const std::vector<Cand> pick = pick_strands(std::move(cand));
        const Traced tr = trace_hits(st, in, pick);
        rc = emit_hits(in, pick, tr, out, n_hits, stats);
        if (rc == SC_OK || rc == SC_ERR_CAPACITY) {
            stats.upload_ms = st.ms("upload", index ? "index" : "score");   // with an index "upload" .. "score" holds it and the lookup
            if (index) { stats.index_ms = st.ms("index", "lookup"); stats.lookup_ms = st.ms("lookup", "score"); }
            stats.score_ms = st.ms("score", "scored");
            stats.trace_ms = st.ms("trace", "traced");
            stats.n_traced = (long)pick.size();
            stats.n_hits = *n_hits;
        }
    }
    stats.total_ms = sc::now_ms() - in.t0;
    return rc;
}

}  // namespace

// The handle of sc_profile_index_create: what the calls on it share.  One call at a time.
struct sc_profile_index {
    Resident res;
    sc_profile_index(int device, Packed&& genes) : res(device, std::move(genes)) {}
};

extern "C" {

const char* sc_profile_error(void) { return tl_error.text.c_str(); }

int sc_profile_hits(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                    int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg, int* hit_gene,
                    int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                    double* evalue, long cap, long* n_hits, sc_profile_stats* stats) {
    sc_profile_seed_stats all = {};
    tl_error.clear();
    const int rc = sc::guarded(&tl_error, "sc_profile_hits", [&] {
        return profile_hits("sc_profile_hits", device, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct, max_evalue, ka_lambda,
                            ka_k, false, HitsOut{hit_seg, hit_gene, hit_strand, hit_score, identity, align_len, qfrom, qto, hfrom, hto, evalue, cap},
                            n_hits, all);
    });
    if (stats)
        *stats = sc_profile_stats{all.upload_ms, all.score_ms, all.trace_ms, all.total_ms, all.score_cells,
                                  all.trace_cells, all.n_tiles, all.n_candidates, all.n_traced, all.n_hits};
    return rc;
}

int sc_profile_hits_seeded(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                           int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg,
                           int* hit_gene, int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto,
                           int* hfrom, int* hto, double* evalue, long cap, long* n_hits, sc_profile_seed_stats* stats) {
    sc_profile_seed_stats unasked;
    sc_profile_seed_stats& all = stats ? *stats : unasked;
    all = {};
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_profile_hits_seeded", [&] {
        return profile_hits("sc_profile_hits_seeded", device, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, min_identity_pct, max_evalue,
                            ka_lambda, ka_k, true, HitsOut{hit_seg, hit_gene, hit_strand, hit_score, identity, align_len, qfrom, qto, hfrom, hto, evalue, cap},
                            n_hits, all);
    });
}

int sc_profile_seed_length(const int* seg_len, int n_segs, long gene_bases, double min_identity_pct, double max_evalue, double ka_lambda,
                           double ka_k, int* lossless_k) {
    if (lossless_k) *lossless_k = 0;
    if (n_segs < 0 || (n_segs > 0 && !seg_len) || gene_bases < 1 || !(ka_lambda > 0.0) || !(ka_k > 0.0) || !(max_evalue >= 0.0)) return SC_ERR_ARG;
    bool has_len[MAX_ROWS + 1] = {};
    for (int r = 0; r < n_segs; r++) {
        if (seg_len[r] < 1 || seg_len[r] > MAX_ROWS) return SC_ERR_UNSUPPORTED;
        has_len[seg_len[r]] = true;
    }
    return seed_length(has_len, gene_bases, min_identity_pct, max_evalue, ka_lambda, ka_k, lossless_k);
}

int sc_profile_counts(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                      int n_segs, const int* seg_read, int n_reads, double min_identity_pct, double max_evalue, double ka_lambda,
                      double ka_k, int seeded, long cand_room, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap,
                      long* n_out, sc_profile_count_stats* stats) {
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_profile_counts", [&] {
        return profile_counts("sc_profile_counts", device, nullptr, gene_text, gene_off, n_genes, seg_text, seg_off, n_segs, seg_read, n_reads,
                              Samples{nullptr, 0}, min_identity_pct, max_evalue, ka_lambda, ka_k, seeded, cand_room,
                              RowsOut{nullptr, out_gene, out_times, out_share, out_reads, cap}, n_out, stats, nullptr);
    });
}

int sc_profile_index_create(int device, const char* gene_text, const long* gene_off, int n_genes, sc_profile_index** out) {
    tl_error.clear();
    if (out) *out = nullptr;
    return sc::guarded(&tl_error, "sc_profile_index_create", [&] {
        const std::string fn = "sc_profile_index_create";
        if (!out || !gene_text || !gene_off || n_genes < 1) return tl_error.fail(SC_ERR_ARG, fn + ": missing argument");
        Packed gn;
        std::string why;
        if (!gn.rebase(gene_off, n_genes, MAX_COLS, fn.c_str(), "gene", why)) return tl_error.fail(SC_ERR_UNSUPPORTED, why);
        sc::select_device(device);
        ProfileInput::pack_genes(gn, gene_text + gene_off[0]);
        *out = new sc_profile_index(device, std::move(gn));
        return SC_OK;
    });
}

int sc_profile_index_info(const sc_profile_index* index, int* n_genes, long* gene_bases, int* n_cached_k, int* cached_k) {
    return sc::guarded(&tl_error, "sc_profile_index_info", [&] {
        if (!index) return tl_error.fail(SC_ERR_ARG, "sc_profile_index_info: missing argument");
        const Packed& gn = index->res.genes.gn;
        if (n_genes) *n_genes = (int)gn.off.size() - 1;
        if (gene_bases) *gene_bases = gn.bytes();
        int n = 0;
        for (int k = SEED_MIN_K; k <= SEED_MAX_K; k++) {
            if (!index->res.seeds[k - SEED_MIN_K]) continue;
            if (cached_k) cached_k[n] = k;
            n++;
        }
        if (n_cached_k) *n_cached_k = n;
        return SC_OK;
    });
}

int sc_profile_index_counts(sc_profile_index* index, const char* seg_text, const long* seg_off, int n_segs, const int* seg_read, int n_reads,
                            const int* read_sample, int n_samples, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k,
                            int seeded, long cand_room, int* out_sample, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap,
                            long* n_out, sc_profile_cohort_stats* stats) {
    sc_profile_cohort_stats unasked;
    sc_profile_cohort_stats& all = stats ? *stats : unasked;
    std::memset(&all, 0, sizeof all);
    tl_error.clear();
    const long allocs_before = sc::device_allocs;
    const int rc = sc::guarded(&tl_error, "sc_profile_index_counts", [&] {
        if (!index) return tl_error.fail(SC_ERR_ARG, "sc_profile_index_counts: missing argument");
        Resident& res = index->res;
        return profile_counts("sc_profile_index_counts", res.device, &res, nullptr, nullptr, (int)res.genes.gn.off.size() - 1, seg_text, seg_off, n_segs,
                              seg_read, n_reads, Samples{read_sample, n_samples}, min_identity_pct, max_evalue, ka_lambda, ka_k, seeded, cand_room,
                              RowsOut{out_sample, out_gene, out_times, out_share, out_reads, cap}, n_out, &all.counts, &all.n_index_builds);
    });
    if (index) { all.n_samples = n_samples; all.n_allocs = sc::device_allocs - allocs_before; }
    return rc;
}

void sc_profile_index_free(sc_profile_index* index) {
    if (!index) return;
    (void)hipSetDevice(index->res.device);
    delete index;
}

double sc_profile_evalue6(int L, long gene_bases, int score2, double ka_lambda, double ka_k) {
    return evalue6_of(evalue_of(ka_k, ka_lambda, L, gene_bases, score2));
}

}  // extern "C"
