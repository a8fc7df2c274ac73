// A region's set-up on its worker: the partial order graph (sc_graph.cpp; the per-base threading of the reads and the
// insertion MSA run on the device: k_thread_*, k_msa), flattened level-major (sc_flatten.cpp), uploaded once, every edge
// support computed on the device (k_edge_support).  Then the level walk (sc_walk.cpp).
#include "sc_ctx.hpp"
#include "sc_phase_timer.hpp"

namespace sc {

// a7 on the device.  Returns the number of columns.
int Worker::msa_device(const std::vector<std::string>& seqs, std::vector<std::string>& rows) {
    const int n = (int)seqs.size();
    std::vector<int> off(n + 1, 0);
    std::string packed;
    for (int i = 0; i < n; i++) { packed += seqs[i]; off[i + 1] = (int)packed.size(); }
    const int cmax = (int)packed.size() + 1;
    size_t longest = 0;                                   // (the first sequence only seeds the columns: any length)
    for (int i = 1; i < n; i++) longest = std::max(longest, seqs[i].size());
    MsaDev d;
    char* dseq = (char*)m_seqs.ensure(packed.size() + 1);
    int* doff = (int*)m_off.ensure(sizeof(int) * (n + 1));
    stage->h2d(dseq, packed.data(), packed.size(), st);               // page-locked staging while other regions are in flight
    stage->h2d(doff, off.data(), sizeof(int) * (n + 1), st);
    d.seqs = dseq; d.seq_off = doff; d.n = n; d.cmax = cmax;
    d.cols[0] = (char*)m_cols0.ensure((size_t)cmax * n);
    d.cols[1] = (char*)m_cols1.ensure((size_t)cmax * n);
    d.counts = (int*)m_counts.ensure(sizeof(int) * 11 * (size_t)cmax);
    d.mv_stride = (int)((longest + 1 + 63) / 64) * 64;
    d.moves = (uint8_t*)m_moves.ensure((size_t)(cmax + 1) * (size_t)d.mv_stride);
    d.edge = (int*)m_edge.ensure(sizeof(int) * 2 * (size_t)(cmax + 1));
    d.trace = (int*)m_trace.ensure(sizeof(int) * 2 * (size_t)(cmax + 64));
    int* dout = (int*)m_out.ensure(sizeof(int) * 2);
    d.ncol_out = dout; d.err_out = dout + 1;
    launch_msa(st, d);
    int out[2];
    stage->d2h(out, dout, sizeof(out), st);
    sync_stream();
    stage->land();
    if (out[1] & 0xFF) {
        size_t longest = 0;
        for (auto& q : seqs) longest = std::max(longest, q.size());
        throw ScError(SC_ERR_UNSUPPORTED, "MSA kernel capacity exceeded (" + std::string((out[1] & 1) ? "a sequence longer than 63; " : "") +
                      std::string((out[1] & 2) ? "more than 1024 columns; " : "") + std::string((out[1] & 4) ? "column buffer; " : "") +
                      std::string((out[1] & 8) ? "more than 65535 sequences; " : "") + std::to_string(n) + " sequences, longest " +
                      std::to_string(longest) + ", columns so far " + std::to_string(out[0]) + ")");
    }
    const int ncol = out[0], cur = out[1] >> 8;
    std::vector<char> cols((size_t)ncol * n);
    if (ncol > 0) {
        stage->d2h(cols.data(), d.cols[cur], (size_t)ncol * n, st);
        sync_stream();
        stage->land();
    }
    rows.assign(n, std::string((size_t)ncol, '-'));
    for (int c = 0; c < ncol; c++)
        for (int k = 0; k < n; k++) rows[k][c] = cols[(size_t)c * n + k];
    return ncol;
}


// a5 on the device: packs the read batch, runs k_thread_* and returns the class tables.
void Worker::thread_device(const std::string& G, const std::vector<AlignedRead>& R, const std::vector<std::vector<CigarOp>>& cig,
                           ThreadTables& T) {
    const int glen = (int)G.size(), n = (int)R.size();
    PhaseTimer tp("      thread_device ", 12);                    // an experiment build waits for the stream at every phase
    auto dphase = [&](const char* name) { if (PhaseTimer::on) { HIPCHK(hipStreamSynchronize(st)); tp.phase(name); } };
    // symbol table of the READS: A C G T first, then every other byte that occurs in a read, in byte order.  A base of the
    // gene that no read carries (an IUPAC code of a 16S reference) keeps the code 0xFF: no read base equals it, so every
    // read base aligned there lands in a sibling class, as `G[i]==r[j]` decides in the reference (PartialOrderGraph.cpp:133)
    bool present[256] = {false};
    for (const auto& r : R) for (unsigned char c : r.seq) present[c] = true;
    std::memset(T.lut, 0xFF, sizeof T.lut);
    T.sym.clear();
    for (char c : {'A', 'C', 'G', 'T'}) { T.lut[(unsigned char)c] = (uint8_t)T.sym.size(); T.sym.push_back(c); }
    for (int c = 0; c < 256; c++)
        if (present[c] && T.lut[c] == 0xFF) {
            if (T.sym.size() >= 8) throw ScError(SC_ERR_UNSUPPORTED, "more than 8 distinct symbols in the reads");
            T.lut[c] = (uint8_t)T.sym.size(); T.sym.push_back((char)c);
        }
    std::vector<int> pos(n), seq_off(n + 1, 0), cig_off(n + 1, 0), cig_len;
    std::string seq, cig_op;
    long m_bases = 0;
    for (int r = 0; r < n; r++) {
        pos[r] = R[r].pos;
        seq += R[r].seq; seq_off[r + 1] = (int)seq.size();
        for (const CigarOp& c : cig[r]) { cig_op.push_back(c.op); cig_len.push_back(c.len); if (c.op == 'M') m_bases += c.len; }
        cig_off[r + 1] = (int)cig_op.size();
    }
    dphase("pack");
    const int ncls = glen * 8;
    ThreadDev d{};
    d.glen = glen; d.n_reads = n;
    char* dref = (char*)t_ref.ensure((size_t)glen + 1);
    stage->h2d(dref, G.data(), (size_t)glen, st);
    d.ref = dref;
    d.pos = upload(*stage, t_pos, pos, st);
    d.seq_off = upload(*stage, t_seqoff, seq_off, st);
    char* dseq = (char*)t_seq.ensure(seq.size() + 1);
    stage->h2d(dseq, seq.data(), seq.size(), st);
    d.seq = dseq;
    d.cig_off = upload(*stage, t_cigoff, cig_off, st);
    char* dop = (char*)t_cigop.ensure(cig_op.size() + 1);
    stage->h2d(dop, cig_op.data(), cig_op.size(), st);
    d.cig_op = dop;
    d.cig_len = upload(*stage, t_ciglen, cig_len, st);
    uint8_t* dlut = (uint8_t*)t_lut.ensure(256);
    stage->h2d(dlut, T.lut, 256, st);
    d.lut = dlut;
    // tables: count | minrid | smin | emin (ncls each) | tmin (8*ncls) | off (ncls+1) | cursor (ncls) | err | big (1 + ncls)
    const size_t words = (size_t)ncls * 4 + (size_t)ncls * 8 + (size_t)ncls + 1 + (size_t)ncls + 1 + 1 + (size_t)ncls;
    int* tabs = (int*)t_tabs.ensure(sizeof(int) * words);
    d.count = tabs; d.minrid = tabs + ncls; d.smin = tabs + 2 * (size_t)ncls; d.emin = tabs + 3 * (size_t)ncls;
    d.tmin = tabs + 4 * (size_t)ncls; d.off = tabs + 12 * (size_t)ncls; d.cursor = d.off + ncls + 1; d.err = d.cursor + ncls; d.big = d.err + 1;
    HIPCHK(hipMemsetAsync(d.count, 0, sizeof(int) * (size_t)ncls, st));
    HIPCHK(hipMemsetAsync(d.minrid, 0x7f, sizeof(int) * (size_t)ncls * 11, st));          // minrid, smin, emin, tmin = 0x7f7f7f7f
    HIPCHK(hipMemsetAsync(d.off, 0, sizeof(int) * ((size_t)ncls * 2 + 3), st));           // off, cursor, err, the count of big classes
    d.pool = (int*)t_pool.ensure(sizeof(int) * (size_t)std::max<long>(m_bases, 1));
    int* pool_sorted = (int*)t_pool2.ensure(sizeof(int) * (size_t)std::max<long>(m_bases, 1));
    dphase("uploads");
    launch_thread(st, d, pool_sorted);
    dphase("kernels");
    T.count.resize(ncls); T.minrid.resize(ncls); T.smin.resize(ncls); T.emin.resize(ncls);
    T.tmin.resize((size_t)ncls * 8); T.off.resize((size_t)ncls + 1); T.pool.resize((size_t)m_bases);
    int err = 0;
    stage->d2h(T.count.data(), d.count, sizeof(int) * (size_t)ncls, st);
    stage->d2h(T.minrid.data(), d.minrid, sizeof(int) * (size_t)ncls, st);
    stage->d2h(T.smin.data(), d.smin, sizeof(int) * (size_t)ncls, st);
    stage->d2h(T.emin.data(), d.emin, sizeof(int) * (size_t)ncls, st);
    stage->d2h(T.tmin.data(), d.tmin, sizeof(int) * (size_t)ncls * 8, st);
    stage->d2h(T.off.data(), d.off, sizeof(int) * ((size_t)ncls + 1), st);
    stage->d2h(T.pool.data(), pool_sorted, sizeof(int) * (size_t)std::max<long>(m_bases, 0), st);
    stage->d2h(&err, d.err, sizeof(int), st);
    const double t_sync0 = now_ms();
    sync_stream();
    stage->land();
    if (ctx->plan.opt.sync_log) fprintf(stderr, "sync thread_device %.3f ms\n", now_ms() - t_sync0);
    dphase("downloads");
    if (err) throw ScError(SC_ERR_ARG, "a read runs outside the window or past its own bases");
    const int INF = 0x7fffffff;
    auto fix = [&](std::vector<int>& v) { for (int& x : v) if (x == 0x7f7f7f7f) x = INF; };
    fix(T.minrid); fix(T.smin); fix(T.emin); fix(T.tmin);
}

// The region's device block without what the caller sets itself (ll, has, U, Uf): the level-major entries of `f`, their
// copy-number prefixes `ent_qoff` and the mates uploaded through `ar`, the level kernels' scratch sized for `qcap` draw
// slots and `max_entries` entries at one level, the sampler's draw log for `max_draws` draws (the largest n_sweeps * Q of
// the region's levels).
JobDev Worker::job_dev(PinnedArena& ar, const FlatGraph& f, const std::vector<int>& ent_qoff, const std::vector<int>& mate_off,
                       const std::vector<int>& mate_idx, int n_reads, long qcap, int max_entries, long max_draws) {
    JobDev jd{};
    jd.ent_rid = upload(ar, b_ent_rid, f.ent_rid, st);
    jd.ent_cn = upload(ar, b_ent_cn, f.ent_cn, st);
    jd.ent_lab_off = upload(ar, b_ent_lab_off, f.ent_lab_off, st);
    jd.ent_lab_len = upload(ar, b_ent_lab_len, f.ent_lab_len, st);
    jd.ent_first = upload(ar, b_ent_first, f.ent_first, st);
    jd.ent_qoff = upload(ar, b_ent_qoff, ent_qoff, st);
    jd.labels = upload(ar, b_labels, f.labels, st);
    jd.mate_ptr = upload(ar, b_mate_ptr, mate_off, st);
    jd.mate_idx = upload(ar, b_mate_idx, mate_idx, st);
    jd.n_reads = n_reads; jd.K = f.K; jd.code_N = f.code_N;
    jd.ll_stride = ((long)n_reads + 3) & ~3L;
    jd.isnew = (uint8_t*)b_isnew.ensure((size_t)max_entries + 8);
    jd.qcap = qcap;
    jd.tabA = (double*)b_tabA.ensure(sizeof(double) * (size_t)qcap * MAXS);
    jd.tabLf = (float*)b_tabLf.ensure(sizeof(float) * (size_t)(std::min<long>(qcap, MAX_DRAWS) + 4) * 136);
    jd.qcode = (uint8_t*)b_qcode.ensure((size_t)qcap + 8);
    jd.qent = (int*)b_qent.ensure(sizeof(int) * (size_t)qcap);
    jd.quid = (int*)b_quid.ensure(sizeof(int) * (size_t)qcap);
    jd.qrid = (int*)b_qrid.ensure(sizeof(int) * (size_t)qcap);
    jd.dlog_cap = std::max<long>(max_draws, 1);
    jd.dlog = (uint8_t*)b_dlog.ensure((size_t)jd.dlog_cap + 8);
    return jd;
}

void Worker::cluster(Job& job, const PoGraph& g, FlatGraph& f) {
    const int n_reads = (int)job.reads.size();
    const double t_cluster0 = now_ms();

    // ---- pseudo level holding every read once, for read_assign (NonparametricClustering.cpp:776-836)
    const int final_e0 = (int)f.ent_rid.size();
    long total_copies = 0;
    {
        int qo = 0;
        for (int i = 0; i < n_reads; i++) {
            f.ent_rid.push_back(i); f.ent_cn.push_back(job.reads[i].cn); f.ent_lab_off.push_back(0);
            f.ent_lab_len.push_back(0); f.ent_first.push_back(1);
            qo += job.reads[i].cn;
        }
        total_copies = qo;
    }
    // prefix of copy numbers inside each level
    std::vector<int>& ent_qoff = ent_qoff_buf;                           // (the slot's: reused from region to region)
    ent_qoff.assign(f.ent_rid.size(), 0);
    int max_level_entries = n_reads, max_level_q = 0;
    for (int l = 0; l < f.n_levels; l++) {
        int qo = 0;
        for (int x = f.level_ent_ptr[l]; x < f.level_ent_ptr[l + 1]; x++) { ent_qoff[x] = qo; qo += f.ent_cn[x]; }
        max_level_entries = std::max(max_level_entries, f.level_ent_ptr[l + 1] - f.level_ent_ptr[l]);
        max_level_q = std::max(max_level_q, qo);
    }
    { int qo = 0; for (int i = 0; i < n_reads; i++) { ent_qoff[final_e0 + i] = qo; qo += job.reads[i].cn; } }
    const long qcap = std::max<long>(std::max<long>(max_level_q, total_copies), 1);
    // draws of the longest chain: n_sweeps * Q as np_bayes_clustering and read_assign form it (sc_walk.cpp), over the levels
    // and the pseudo-level
    auto level_draws = [&](long Q) { return (long)level_sweeps(job.params, Q) * Q; };
    long max_draws = level_draws(total_copies);
    for (int l = 0; l < f.n_levels; l++) max_draws = std::max(max_draws, level_draws(f.level_read_count[(size_t)l]));
    // cells of a read_loglik row that can hold a value when level l starts: the reads of the levels before it and their
    // mates (the soft update enters a mate the first time it is asked for, Strain.cpp:147-150) -- a prefix of the read ids
    std::vector<int> level_hi((size_t)f.n_levels + 1, 0);
    for (int l = 0; l < f.n_levels; l++) {
        int hi = level_hi[(size_t)l];
        for (int x = f.level_ent_ptr[l]; x < f.level_ent_ptr[l + 1]; x++) {
            const int rid = f.ent_rid[x];
            hi = std::max(hi, rid + 1);
            for (int k = job.mate_off[(size_t)rid]; k < job.mate_off[(size_t)rid + 1]; k++) hi = std::max(hi, job.mate_idx[(size_t)k] + 1);
        }
        level_hi[(size_t)l + 1] = hi;
    }

    // ---- upload the static arrays; the rows start empty, the uniforms are the context's
    JobDev jd = job_dev(*stage, f, ent_qoff, job.mate_off, job.mate_idx, n_reads, qcap, max_level_entries, max_draws);
    jd.ll = (double*)b_ll.ensure(sizeof(double) * (size_t)jd.ll_stride * MAXS);
    jd.has = (uint8_t*)b_has.ensure((size_t)n_reads + 8);
    HIPCHK(hipMemsetAsync(jd.has, 0, (size_t)n_reads + 8, st));
    jd.U = ctx->U.d.p;
    jd.Uf = ctx->U.f.p;
    // the batched level kernels find the region through a pointer: the block travels once, with the uploads
    const JobDev* jd_dev = (const JobDev*)b_jobdev.ensure(sizeof(JobBlock));
    stage->h2d((void*)jd_dev, &jd, sizeof jd, st);

    // ---- a16: every edge support on the device
    {
        std::vector<int> esrc(f.out_node.size());
        for (int a = 0; a < f.n_nodes; a++) for (int x = f.out_ptr[a]; x < f.out_ptr[a + 1]; x++) esrc[x] = a;
        int* d_out_ptr = upload(*stage, b_out_ptr, f.out_ptr, st);
        int* d_out_node = upload(*stage, b_out_node, f.out_node, st);
        int* d_pool_ptr = upload(*stage, b_pool_ptr, f.pool_ptr, st);
        int* d_pool_rid = upload(*stage, b_pool_rid, f.pool_rid, st);
        int* d_pool_cn = upload(*stage, b_pool_cn, f.pool_cn, st);
        uint8_t* d_isend = upload(*stage, b_isend, f.node_is_end, st);
        int* d_esrc = upload(*stage, b_esrc, esrc, st);
        int* d_sup = (int*)b_support.ensure(sizeof(int) * std::max<size_t>(esrc.size(), 1));
        launch_edge_support(st, d_out_ptr, d_out_node, d_pool_ptr, d_pool_rid, d_pool_cn, d_isend, d_esrc, (int)esrc.size(),
                            f.pools_sorted ? 1 : 0, d_sup);
        if (!esrc.empty())
            stage->d2h(f.out_support.data(), d_sup, sizeof(int) * esrc.size(), st);
        const double t_sync0 = now_ms();
        sync_stream();
        stage->land();
        if (stage != &passthrough) ctx->arenas.release(stage);      // every transfer of the set-up is done
        stage = &passthrough;
        if (ctx->plan.opt.sync_log) fprintf(stderr, "sync uploads+edge_support %.3f ms (since cluster start %.3f)\n", now_ms() - t_sync0, now_ms() - t_cluster0);
        job.edge_support = f.out_support;
    }

    // ---- level walk: from here on the region's host work is a few microseconds per level
    if (setup_held) { ctx->gate.leave(); setup_held = false; }
    job.stats.setup_ms = now_ms() - t_cluster0;
    MailHold mail_hold{this};          // the mailbox the region walks on (resident workers)
    if (grid) {
        const double t_m0 = now_ms();
        mslot.store(grid->acquire_mailbox(this), std::memory_order_release);
        job.stats.mailbox_ms = now_ms() - t_m0;
        __atomic_store_n(&Rh->seq, 0u, __ATOMIC_RELEASE);       // (stamps are the mailbox's from here on: never 0)
    }
    walk_levels(*this, job, f, jd, jd_dev, level_hi, final_e0, total_copies, mail_hold);
}

void Worker::process(Job& job) {
    const double t0 = now_ms();
    // page-locked staging for the set-up of this region; cluster() hands it back once the last copy has landed
    struct Lease {
        Worker* w;
        ~Lease() { if (w->stage && w->stage != &w->passthrough) w->ctx->arenas.release(w->stage); w->stage = nullptr; }
    } lease{this};
    struct Setup {                     // one of the context's set-up places, held until the level walk starts (cluster())
        Worker* w;
        ~Setup() { if (w->setup_held) { w->ctx->gate.leave(); w->setup_held = false; } }
    } setup{this};
    job.stats.queue_ms = t0 - job.t_submit;
    if (ctx->gate.split_exec) FiberPool::yield();           // the set-up belongs on one of the pool's set-up threads
    ctx->gate.enter(this);
    setup_held = true;
    job.stats.place_ms = now_ms() - t0;
    stage = ctx->arenas.lease(&passthrough);
    MsaFn msa = [this](const std::vector<std::string>& seqs, std::vector<std::string>& rows) { return msa_device(seqs, rows); };
    ThreadFn thr = [this, &job](const std::string& G, const std::vector<AlignedRead>& R, const std::vector<std::vector<CigarOp>>& cg,
                          ThreadTables& T) {
        thread_device(G, R, cg, T);
        if (job.params.graph_only || job.params.want_graph) {      // kept for sc_roi_thread_tables / sc_roi_thread_edges
            job.thr_count = T.count; job.thr_first = T.minrid; job.thr_pool = T.pool; job.thr_sym.assign(T.sym.begin(), T.sym.end());
            job.thr_smin = T.smin; job.thr_emin = T.emin; job.thr_tmin = T.tmin;                 // for sc_roi_thread_edges
        }
    };
    // a context with one region in flight gives the region's bulk copies (class pools, flattening: 88 M entries on the
    // unthinned configs[3] region) the rank's other CPUs; with many in flight those already run other regions
    sc::set_graph_threads(ctx->workers.size() == 1 ? std::min(8, std::max(1, (int)(sc::cpu_budget_host() / sc::local_world_size()))) : 1);
    PoGraph g(job.ref, job.reads, msa, thr);
    job.stats.msa_calls = g.msa_calls;
    if (job.params.graph_only || job.params.want_graph) job.graph_dump = g.dump();      // -G text, PartialOrderGraph.cpp:318-337
    FlatGraph& f = flat;               // (the slot's arrays, reused from region to region)
    f.reset();
    flatten(g, (int)job.reads.size(), f);
    job.stats.n_nodes = f.n_nodes; job.stats.n_levels = f.n_levels; job.stats.n_unique_reads = (int)job.reads.size();
    long copies = 0;
    for (auto& r : job.reads) copies += r.cn;
    job.stats.n_read_copies = copies;
    const double t1 = now_ms();
    job.stats.graph_ms = t1 - t0;
    if (!job.params.graph_only) {
        if (!f.unsupported.empty()) throw ScError(SC_ERR_UNSUPPORTED, f.unsupported);
        cluster(job, g, f);
    }
    job.stats.cluster_ms = now_ms() - t1;
}

}  // namespace sc
