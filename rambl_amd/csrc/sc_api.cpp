// The C ABI of libstraincall_hip.so.  See include/straincall_hip.h.
//
// Per region (a worker's fiber): its set-up (sc_region.cpp), then the level walk (sc_walk.cpp); the context, its workers
// and how their levels reach the GPU are in sc_ctx.hpp / sc_sched.cpp, the shape of a context in sc_plan.hpp.
#include <malloc.h>

#include <cmath>

#include "sc_ctx.hpp"

using namespace sc;
// What the one-level test entries (sc_sample_level, sc_update_level, sc_hard_level) share: a region that is nothing but one level.  Its
// entries lie at [e0, e0 + n_ent) of the region's arrays; entries [0, e0) belong to other levels: they name other reads (the
// last ones, backwards), so that an entry index that misses e0 reads the wrong row.  The vectors live as long as the stub:
// the copies of a private worker pass through, so their sources stay until the stream is synchronised.
struct LevelStub {
    FlatGraph f;
    std::vector<int> qoff, mptr, midx;
    std::vector<double> rows;
    std::vector<uint8_t> hv;
    JobDev jd{};
    // every entry with copy number 1, its one-symbol label at labels[e] (code 0) and `first` set; labels holds n_labels
    // codes (> e0).  The caller then states its own entries, [e0, e0 + n_ent).
    void entries(int e0, int n_ent, int n_reads, size_t n_labels) {
        const size_t E = (size_t)e0 + (size_t)n_ent;
        f.ent_rid.resize(E); f.ent_cn.assign(E, 1); f.ent_lab_off.resize(E); f.ent_lab_len.assign(E, 1); f.ent_first.assign(E, 1);
        f.labels.assign(n_labels, 0);
        qoff.assign(E, 0);
        for (size_t e = 0; e < E; e++) {
            f.ent_rid[e] = n_reads - 1 - (int)e % n_reads;
            f.ent_lab_off[e] = (int)e;
        }
        mptr.assign((size_t)n_reads + 1, 0);
        midx.clear();
    }
    // the region's device block (Worker::job_dev), the rows ll[s * n_reads + r] of the S strains in rows slot[s] of a
    // matrix of zeros, `has` padded as the region set-up pads it; the caller adds what it needs (U, Uf) and publishes
    JobDev& upload(Worker& w, int n_reads, long qcap, int n_ent, long max_draws, int S, const int* slot, const double* ll, const unsigned char* has) {
        jd = w.job_dev(w.passthrough, f, qoff, mptr, midx, n_reads, qcap, n_ent, max_draws);
        rows.assign((size_t)jd.ll_stride * MAXS, 0.0);
        for (int s = 0; s < S; s++) std::memcpy(&rows[(size_t)slot[s] * jd.ll_stride], ll + (size_t)s * n_reads, sizeof(double) * n_reads);
        jd.ll = sc::upload(w.passthrough, w.b_ll, rows, w.st);
        hv.assign(has, has + n_reads);
        hv.resize((size_t)n_reads + 8, 0);
        jd.has = sc::upload(w.passthrough, w.b_has, hv, w.st);
        return jd;
    }
    const JobDev* publish(Worker& w) {
        const JobDev* jd_dev = (const JobDev*)w.b_jobdev.ensure(sizeof(JobBlock));
        HIPCHK(hipMemcpyAsync((void*)jd_dev, &jd, sizeof jd, hipMemcpyHostToDevice, w.st));
        return jd_dev;
    }
};

struct sc_ctx { Ctx c; sc_ctx(int device, const CtxPlan& plan) : c(device, plan) {} };

// sc::guarded for an entry on a context: the message goes to sc_last_error(), under the context's mutex.
template <class F> static int ctx_guarded(Ctx* ctx, const char* fn, F&& body) noexcept {
    LastError err;
    const int rc = guarded(&err, fn, body);
    if (!err.text.empty()) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->last_error.swap(err.text); }
    return rc;
}

// One level on hand-made inputs, as sc_update_level and sc_hard_level state it (include/straincall_hip.h): the arguments
// both take ...
struct OneLevel {
    int S; const int *slot, *lab_off, *lab_len; int K, code_N; const double* lpt;
    int n_reads; const double* ll; const unsigned char *has, *labels; int n_labels, n_ent, e0;
    const int *ent_rid, *ent_lab_off, *ent_lab_len; const unsigned char* ent_first;
    int n_copy; const int *copy_src, *copy_dst; int copy_n;
    double* ll_out; unsigned char *has_out, *isnew_out; int* done_out;
};
// ... and what the hard update adds: the strains' log priors, the entries' copy numbers, the mates (CSR over the reads), and
// its results.
struct HardLevel {
    const double* logpri; const int *ent_cn, *mate_off, *mate_idx;
    double *abund, *subst, *resp; int *qrid, *quid; unsigned char* qcode;
};
// The checks, the stub region, the level's parameters, the launch through launch_level and the copies back, for both
// entries.  hard = nullptr: the update alone (the level's kernel returns behind it); else MODE_HARD behind the update, as
// LevelWalk::hard_clustering runs it.
static int one_level(sc_ctx* h, const char* fn, const OneLevel& a, const HardLevel* hard) {
    if (!h || !a.slot || !a.lab_off || !a.lab_len || !a.lpt || !a.ll || !a.has || !a.labels || !a.ent_rid || !a.ent_lab_off || !a.ent_lab_len ||
        !a.ent_first || !a.ll_out || !a.has_out || !a.isnew_out || !a.done_out)
        return SC_ERR_ARG;
    if (hard && (!hard->logpri || !hard->ent_cn || !hard->mate_off || !hard->abund || !hard->subst || !hard->resp || !hard->qrid || !hard->quid ||
                 !hard->qcode))
        return SC_ERR_ARG;
    Ctx* ctx = &h->c;
    if (ctx->resident || ctx->workers.size() != 1) return SC_ERR_ARG;      // as sc_sample_level
    const int S = a.S, K = a.K, code_N = a.code_N, n_reads = a.n_reads, n_ent = a.n_ent, e0 = a.e0, n_labels = a.n_labels, n_copy = a.n_copy;
    if (S < 1 || S > MAXS || K < 6 || K > KMAX || !(code_N == -1 || (code_N >= 6 && code_N < K)) || n_reads < 1 ||
        n_reads > (1 << 16) || n_ent < 1 || n_ent > (1 << 16) || e0 < 0 || e0 > (1 << 20) || n_labels < 1 || n_labels > (1 << 24) || n_copy < 0 || n_copy > MAXS || a.copy_n < 0)
        return SC_ERR_ARG;
    if ((long)S * K * K > (long)level_table_capacity()) return SC_ERR_ARG;
    if (n_copy > 0 && (!a.copy_src || !a.copy_dst)) return SC_ERR_ARG;
    // Everything a kernel indexes with.  A label lies inside `labels`.  The update: a label of a single symbol may hold any
    // code (its single-symbol paths check a < K && b < K themselves); the walks over a multi-symbol label index the strain's
    // table unchecked, so every code they meet is below K (an N of the strain's label becomes the read's symbol first): the
    // codes of every multi-symbol label, and of every entry's label once a strain's label has more than one symbol.  The hard
    // update of a level with any multi-symbol label walks every entry's label against every strain's: there every entry's
    // codes are below K, whatever the strains' labels are.  (A strain's single symbol stays free: "^" and "$" carry 0xFF in
    // production, and both updates test it.)
    auto label_ok = [&](int off, int len, bool strain, bool walked) {
        if (len < 1 || off < 0 || (long)off + len > (long)n_labels) return false;
        if (len == 1 && !walked) return true;
        for (int i = 0; i < len; i++) {
            const int c = a.labels[off + i];
            if (!(c < K || (strain && c == code_N))) return false;
        }
        return true;
    };
    bool multi_strain = false;
    uint64_t taken[2] = {0, 0}, dst_rows[2] = {0, 0}, src_rows[2] = {0, 0};
    auto bit = [](const uint64_t* m, int r) { return (m[r >> 6] >> (r & 63)) & 1; };
    auto set = [](uint64_t* m, int r) { m[r >> 6] |= 1ull << (r & 63); };
    for (int s = 0; s < S; s++) {
        if (a.slot[s] < 0 || a.slot[s] >= MAXS || bit(taken, a.slot[s])) return SC_ERR_ARG;
        set(taken, a.slot[s]);
        if (!label_ok(a.lab_off[s], a.lab_len[s], true, a.lab_len[s] > 1)) return SC_ERR_ARG;
        if (a.lab_len[s] > 1) multi_strain = true;
        if (hard && !(hard->logpri[s] < INFINITY)) return SC_ERR_ARG;      // (-inf is log 0; NaN and +inf are no log of a share)
    }
    bool has_dups = false, any_multi = multi_strain;
    for (int r = 0; r < n_ent; r++) {
        if (!a.ent_first[r]) has_dups = true;                 // as LevelWalk::run derives them from the level's entries
        if (a.ent_lab_len[r] != 1) any_multi = true;
    }
    long Q = 0;
    for (int r = 0; r < n_ent; r++) {
        if (a.ent_rid[r] < 0 || a.ent_rid[r] >= n_reads || !label_ok(a.ent_lab_off[r], a.ent_lab_len[r], false, hard ? any_multi : multi_strain)) return SC_ERR_ARG;
        if (hard && hard->ent_cn[r] < 1) return SC_ERR_ARG;
        Q += hard ? hard->ent_cn[r] : 1;
    }
    if (Q < 1 || Q > (1L << 20)) return SC_ERR_ARG;          // (tabA holds MAXS * Q doubles)
    int nm = 0;
    if (hard) {
        if (hard->mate_off[0] != 0) return SC_ERR_ARG;
        for (int r = 0; r < n_reads; r++) if (hard->mate_off[r + 1] < hard->mate_off[r]) return SC_ERR_ARG;
        nm = hard->mate_off[n_reads];
        if (nm > 0 && !hard->mate_idx) return SC_ERR_ARG;
        for (int i = 0; i < nm; i++) if (hard->mate_idx[i] < -1 || hard->mate_idx[i] >= n_reads) return SC_ERR_ARG;
    }
    // the copies are independent: a destination is no other pair's destination and nobody's source
    for (int c = 0; c < n_copy; c++) {
        if (a.copy_src[c] < 0 || a.copy_src[c] >= MAXS || a.copy_dst[c] < 0 || a.copy_dst[c] >= MAXS || bit(dst_rows, a.copy_dst[c])) return SC_ERR_ARG;
        set(dst_rows, a.copy_dst[c]); set(src_rows, a.copy_src[c]);
    }
    if ((dst_rows[0] & src_rows[0]) || (dst_rows[1] & src_rows[1])) return SC_ERR_ARG;
    return ctx_guarded(ctx, fn, [&] {
        Worker w;                                      // a private worker: own stream, own parameter / result blocks
        w.init_private(ctx);
        const int E = e0 + n_ent;
        LevelStub stub;
        FlatGraph& f = stub.f;
        f.K = K; f.code_N = code_N;
        stub.entries(e0, n_ent, n_reads, (size_t)e0 + (size_t)n_labels);      // the caller's labels behind those of the entries in front
        std::memcpy(f.labels.data() + e0, a.labels, (size_t)n_labels);
        for (int r = 0, q = 0; r < n_ent; r++) {
            const size_t e = (size_t)(e0 + r);
            f.ent_rid[e] = a.ent_rid[r]; f.ent_lab_off[e] = e0 + a.ent_lab_off[r]; f.ent_lab_len[e] = a.ent_lab_len[r];
            f.ent_first[e] = a.ent_first[r] ? 1 : 0;
            f.ent_cn[e] = hard ? hard->ent_cn[r] : 1;
            stub.qoff[e] = q; q += f.ent_cn[e];
        }
        if (hard) {
            stub.mptr.assign(hard->mate_off, hard->mate_off + n_reads + 1);
            if (nm > 0) stub.midx.assign(hard->mate_idx, hard->mate_idx + nm);
        }
        const hipStream_t st = w.st;
        const JobDev& jd = stub.upload(w, n_reads, Q, n_ent, 1, S, a.slot, a.ll, a.has);
        const JobDev* jd_dev = stub.publish(w);

        // the level's parameters as LevelWalk::run_level states them
        LevelParams& P = *w.Ph;
        for (int s = 0; s < S; s++) {
            P.sp[s] = StrainParam{a.slot[s], e0 + a.lab_off[s], a.lab_len[s], 0, 1.0, hard ? hard->logpri[s] : 0.0};
            w.hp.logpri[s] = P.sp[s].logpri;
            w.gp.slot[s] = (uint8_t)a.slot[s];
            w.gp.lab[s] = f.labels[(size_t)(e0 + a.lab_off[s])];
        }
        for (int c = 0; c < n_copy; c++) {
            P.copy_src[c] = a.copy_src[c]; P.copy_dst[c] = a.copy_dst[c];
            w.gp.copy_src[c] = (uint8_t)a.copy_src[c]; w.gp.copy_dst[c] = (uint8_t)a.copy_dst[c];
        }
        std::memcpy(P.lpt, a.lpt, sizeof(double) * (size_t)S * K * K);             // compact [K][K]
        LevelHdr H{};
        H.mode = hard ? MODE_HARD : MODE_SAMPLE; H.S = S; H.e0 = e0; H.e1 = E; H.has_dups = has_dups; H.any_multi = any_multi; H.Q = (int)Q;
        H.n_sweeps = 0;                                // no sampler: level_kind gives 0, level_plain_body returns behind the update or runs the hard update
        H.n_copy = n_copy; H.copy_n = a.copy_n; H.do_update = 1; H.seq = 1;
        std::memset(w.Rh, 0, sizeof(LevelResult));
        const LevelItem it = w.level_item(jd_dev, H, K);
        if (item_kind(it.kind) != 0) throw ScError(SC_ERR_INTERNAL, "a level without sweeps asked for the sampler");
        const int done = launch_level(st, it, w.gp, w.hp, n_reads);      // as the walk of a single region launches its levels
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        if (w.Rh->seq != 1u || w.Rh->error) throw ScError(SC_ERR_INTERNAL, "the level did not complete");
        std::vector<double>& rows = stub.rows;         // the whole matrix back, without the padding of its stride
        HIPCHK(hipMemcpy(rows.data(), jd.ll, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < MAXS; r++) std::memcpy(a.ll_out + (size_t)r * n_reads, &rows[(size_t)r * jd.ll_stride], sizeof(double) * (size_t)n_reads);
        HIPCHK(hipMemcpy(a.has_out, jd.has, (size_t)n_reads, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(a.isnew_out, jd.isnew, (size_t)n_ent, hipMemcpyDeviceToHost));
        if (hard) {
            std::memcpy(hard->abund, w.Rh->abund, sizeof(double) * (size_t)S);
            std::memcpy(hard->subst, w.Rh->subst, sizeof(double) * (size_t)S * K * K);
            // the responsibilities tabA[s * qcap + q], without their stride; the draw slots as the device wrote them
            for (int s = 0; s < S; s++)
                HIPCHK(hipMemcpy(hard->resp + (size_t)s * Q, jd.tabA + (size_t)s * jd.qcap, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hard->qrid, jd.qrid, sizeof(int) * (size_t)Q, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hard->quid, jd.quid, sizeof(int) * (size_t)Q, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hard->qcode, jd.qcode, (size_t)Q, hipMemcpyDeviceToHost));
        }
        *a.done_out = done;
        return SC_OK;
    });
}

extern "C" {

// Host threads a context with `stream_count` regions in flight starts on a rank that shares its host with
// `local_world - 1` others (0: read LOCAL_WORLD_SIZE), given `cpus` CPUs for the host (0: the cgroup quota / affinity
// mask): out[0] executor threads (they run the regions' fibers), out[1] the level server, out[2] ingest threads of
// sc_aln_open.  Pure arithmetic (no device): tests/test_stage5.py checks that 8 ranks on 16 CPUs stay within them.
int sc_host_plan(int stream_count, int local_world, double cpus, int* out) {
    if (!out || stream_count < 1) return SC_ERR_ARG;
    host_plan(stream_count, local_world > 0 ? local_world : local_world_size(), cpus > 0 ? cpus : cpu_budget_host(), out);
    return SC_OK;
}

int sc_ctx_create(int device, int stream_count, sc_ctx** out) {
    if (!out) return SC_ERR_ARG;
    *out = nullptr;
    // 16 hardware queues run side by side on this GPU (more are time-sliced: measured); the launch and setup streams of the
    // context want one each.  Only effective if HIP is not initialised yet in this process (rambl_amd/__init__.py sets it too).
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    return guarded(nullptr, "sc_ctx_create", [&] {            // no context yet to keep a message: the code alone
        select_device(device);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SC_ERR_NO_DEVICE;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SC_ERR_NO_DEVICE;   // kernels are built for gfx950 only
        if (init_kernels() != 0) return SC_ERR_HIP;
        const Options opt = read_options();
        // the context's threads (they inherit the mask of the thread that starts them) and the host memory it allocates and first
        // touches here: next to the GPU; the caller's own mask comes back when this function returns
        struct Near {
            cpu_set_t before; bool moved = false;
            Near(int dev, bool bind) {
                cpu_set_t local;
                if (bind && sched_getaffinity(0, sizeof before, &before) == 0 && sc::gpu_local_cpus(dev, &local)) moved = sched_setaffinity(0, sizeof local, &local) == 0;
            }
            ~Near() { if (moved) (void)sched_setaffinity(0, sizeof before, &before); }
        } near{device, !opt.off(opt.numa_bind)};
        {
            // A region builds its graph out of ~10^5 small allocations and a few of tens of megabytes; handed back to the system
            // and mapped again for every region they cost their size in page faults.  Keep freed memory in the process.
            static std::once_flag once;
            std::call_once(once, [&opt] {
                if (opt.off(opt.malloc_tune)) return;
                mallopt(M_MMAP_THRESHOLD, 32 << 20);
                mallopt(M_TRIM_THRESHOLD, 1 << 30);
                mallopt(M_TOP_PAD, 64 << 20);
            });
        }
        *out = new sc_ctx(device, plan_context(opt, stream_count, prop.multiProcessorCount, cpu_budget_host(), local_world_size()));
        return SC_OK;
    });
}

void sc_ctx_destroy(sc_ctx* h) { delete h; }

const char* sc_last_error(sc_ctx* h) {
    if (!h) return "";
    static thread_local std::string copy;
    if (guarded(nullptr, "sc_last_error", [&] { std::lock_guard<std::mutex> lk(h->c.mu); copy = h->c.last_error; return SC_OK; }) != SC_OK) return "";
    return copy.c_str();
}

const char* sc_roi_error(sc_ctx* h, int handle) {
    if (!h) return "";
    std::lock_guard<std::mutex> lk(h->c.mu);
    auto it = h->c.jobs.find(handle);
    return (it == h->c.jobs.end() || it->second->status != 1) ? "" : it->second->err.c_str();
}

int sc_roi_submit(sc_ctx* h, const char* ref_bases, int ref_len, const int* read_pos, const char* cigar_text,
                  const int* cigar_off, const char* seq_text, const int* seq_off, const int* read_copies,
                  const int* mate_idx, const int* mate_off, int n_reads, const sc_params* params, int* handle_out) {
    if (!h || !ref_bases || ref_len < 0 || n_reads < 0 || !params || !handle_out) return SC_ERR_ARG;
    if (n_reads > 0 && (!read_pos || !cigar_text || !cigar_off || !seq_text || !seq_off || !read_copies || !mate_off)) return SC_ERR_ARG;
    // the device buffers are sized for the reference's literals (uniform stream of MAX_DRAWS values, MAXS rows)
    if (params->draw_budget < 1 || params->draw_budget > MAX_DRAWS || params->sweeps_cap < 0 || params->max_candidates < 1 ||
        params->max_candidates > MAXS)
        return SC_ERR_ARG;
    if (n_reads > 0 && (cigar_off[0] < 0 || seq_off[0] < 0 || mate_off[0] != 0)) return SC_ERR_ARG;
    for (int i = 0; i < n_reads; i++)
        if (read_copies[i] < 1 || cigar_off[i + 1] < cigar_off[i] || seq_off[i + 1] < seq_off[i] || mate_off[i + 1] < mate_off[i])
            return SC_ERR_ARG;
    Ctx* ctx = &h->c;
    return ctx_guarded(ctx, "sc_roi_submit", [&] {
        auto job = std::make_shared<Job>();
        job->t_submit = now_ms();
        job->ref.assign(ref_bases, (size_t)ref_len);
        job->reads.resize((size_t)n_reads);
        for (int i = 0; i < n_reads; i++) {
            if (read_pos[i] < 0 || read_pos[i] > ref_len) return SC_ERR_ARG;
            job->reads[i].pos = read_pos[i];
            job->reads[i].cigar.assign(cigar_text + cigar_off[i], (size_t)(cigar_off[i + 1] - cigar_off[i]));
            job->reads[i].seq.assign(seq_text + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
            job->reads[i].cn = read_copies[i];
        }
        job->mate_off.assign(mate_off ? mate_off : nullptr, mate_off ? mate_off + n_reads + 1 : nullptr);
        if (job->mate_off.empty()) job->mate_off.assign(1, 0);
        const int nm = job->mate_off.back();
        if (nm > 0 && !mate_idx) return SC_ERR_ARG;
        job->mate_idx.assign(mate_idx, mate_idx + nm);
        for (int v : job->mate_idx) if (v < -1 || v >= n_reads) return SC_ERR_ARG;
        job->params = *params;
        Worker* wake = nullptr;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            job->handle = ctx->next_handle++;
            ctx->jobs[job->handle] = job;
            ctx->queue.push_back(job);
            ctx->regions_active.fetch_add(1, std::memory_order_acq_rel);
            *handle_out = job->handle;
            if (!ctx->idle.empty()) { wake = ctx->idle.back(); ctx->idle.pop_back(); }
        }
        if (wake) ctx->pool->make_ready(wake->fib);
        return SC_OK;
    });
}

static std::shared_ptr<Job> find_job(sc_ctx* h, int handle) {
    std::lock_guard<std::mutex> lk(h->c.mu);
    auto it = h->c.jobs.find(handle);
    return it == h->c.jobs.end() ? nullptr : it->second;
}

int sc_roi_wait(sc_ctx* h, int handle) {
    if (!h) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job) return SC_ERR_ARG;
    return ctx_guarded(&h->c, "sc_roi_wait", [&] {            // the copy of the message allocates
        std::unique_lock<std::mutex> lk(h->c.mu);
        h->c.cv_done.wait(lk, [&] { return job->status == 1; });
        if (job->rc != SC_OK) h->c.last_error = job->err;
        return job->rc;
    });
}

int sc_roi_result(sc_ctx* h, int handle, char* seq_buf, long seq_cap, int* seq_off, double* abundance, int max_strains,
                  int* n_strains) {
    if (!h || !n_strains) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    if (job->rc != SC_OK) return job->rc;
    const int n = (int)job->seqs.size();
    *n_strains = n;
    long tot = 0;
    for (auto& s : job->seqs) tot += (long)s.size();
    if (n > max_strains || tot > seq_cap || !seq_buf || !seq_off || !abundance) return SC_ERR_CAPACITY;
    long o = 0;
    for (int i = 0; i < n; i++) {
        seq_off[i] = (int)o;
        std::memcpy(seq_buf + o, job->seqs[i].data(), job->seqs[i].size());
        o += (long)job->seqs[i].size();
        abundance[i] = job->abund[i];
    }
    seq_off[n] = (int)o;
    return SC_OK;
}

static int copy_text(const std::string& s, char* buf, long cap, long* len_out) {
    if (len_out) *len_out = (long)s.size();
    if (!buf || cap < (long)s.size()) return SC_ERR_CAPACITY;
    std::memcpy(buf, s.data(), s.size());
    return SC_OK;
}
int sc_roi_graph_dump(sc_ctx* h, int handle, char* buf, long cap, long* len_out) {
    if (!h) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    if (job->rc != SC_OK && job->graph_dump.empty()) return job->rc;
    return copy_text(job->graph_dump, buf, cap, len_out);
}
int sc_roi_trace(sc_ctx* h, int handle, char* buf, long cap, long* len_out) {
    if (!h) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    if (job->rc != SC_OK) return job->rc;
    return copy_text(job->trace, buf, cap, len_out);
}
int sc_roi_stats(sc_ctx* h, int handle, sc_stats* out) {
    if (!h || !out) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    *out = job->stats;
    return SC_OK;
}
int sc_roi_edge_support(sc_ctx* h, int handle, int* support, int cap, int* n_edges) {
    if (!h || !n_edges) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    if (job->rc != SC_OK) return job->rc;
    *n_edges = (int)job->edge_support.size();
    if (!support || cap < *n_edges) return SC_ERR_CAPACITY;
    std::memcpy(support, job->edge_support.data(), sizeof(int) * job->edge_support.size());
    return SC_OK;
}
int sc_roi_thread_tables(sc_ctx* h, int handle, int* count, int* first_read, int cls_cap, int* pool, long pool_cap,
                         char* symbols, int* n_cls, long* n_pool) {
    if (!h || !n_cls || !n_pool) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    *n_cls = (int)job->thr_count.size();
    *n_pool = (long)job->thr_pool.size();
    if (!count || !first_read || !pool || !symbols || cls_cap < *n_cls || pool_cap < *n_pool) return SC_ERR_CAPACITY;
    std::memcpy(count, job->thr_count.data(), sizeof(int) * job->thr_count.size());
    std::memcpy(first_read, job->thr_first.data(), sizeof(int) * job->thr_first.size());
    std::memcpy(pool, job->thr_pool.data(), sizeof(int) * job->thr_pool.size());
    std::memset(symbols, 0, 8);
    std::memcpy(symbols, job->thr_sym.data(), std::min<size_t>(8, job->thr_sym.size()));
    return SC_OK;
}
int sc_roi_thread_edges(sc_ctx* h, int handle, int* smin, int* emin, int* tmin, int cls_cap, int* n_cls) {
    if (!h || !n_cls) return SC_ERR_ARG;
    auto job = find_job(h, handle);
    if (!job || job->status != 1) return SC_ERR_ARG;
    *n_cls = (int)job->thr_smin.size();
    if (!smin || !emin || !tmin || cls_cap < *n_cls) return SC_ERR_CAPACITY;
    std::memcpy(smin, job->thr_smin.data(), sizeof(int) * job->thr_smin.size());
    std::memcpy(emin, job->thr_emin.data(), sizeof(int) * job->thr_emin.size());
    std::memcpy(tmin, job->thr_tmin.data(), sizeof(int) * job->thr_tmin.size());
    return SC_OK;
}
int sc_edge_support_tables(sc_ctx* h, int n_nodes, const int* pool_ptr, const int* pool_rid, const int* pool_cn,
                           const unsigned char* node_is_end, int n_edges, const int* edge_src, const int* edge_dst, int sorted,
                           int* support_out) {
    if (!h || n_nodes < 1 || n_edges < 0 || !pool_ptr || !node_is_end || (sorted != 0 && sorted != 1)) return SC_ERR_ARG;
    if (n_edges > 0 && (!edge_src || !edge_dst || !support_out)) return SC_ERR_ARG;
    if (pool_ptr[0] != 0) return SC_ERR_ARG;
    for (int a = 0; a < n_nodes; a++) if (pool_ptr[a + 1] < pool_ptr[a]) return SC_ERR_ARG;
    const int np = pool_ptr[n_nodes];
    if (np > 0 && (!pool_rid || !pool_cn)) return SC_ERR_ARG;
    for (int e = 0; e < n_edges; e++)
        if (edge_src[e] < 0 || edge_src[e] >= n_nodes || edge_dst[e] < 0 || edge_dst[e] >= n_nodes) return SC_ERR_ARG;
    if (sorted)                                        // the binary searches of k_edge_support need what the flag promises
        for (int a = 0; a < n_nodes; a++)
            for (int x = pool_ptr[a] + 1; x < pool_ptr[a + 1]; x++) if (pool_rid[x] < pool_rid[x - 1]) return SC_ERR_ARG;
    if (n_edges == 0) return SC_OK;
    Ctx* ctx = &h->c;
    return ctx_guarded(ctx, "sc_edge_support_tables", [&] {
        Worker w;                                      // a private worker: own stream
        w.init_private(ctx);
        const hipStream_t st = w.st;
        const std::vector<int> pptr(pool_ptr, pool_ptr + n_nodes + 1), prid(pool_rid, pool_rid + np), pcn(pool_cn, pool_cn + np);
        const std::vector<int> esrc(edge_src, edge_src + n_edges), edst(edge_dst, edge_dst + n_edges);
        const std::vector<uint8_t> isend(node_is_end, node_is_end + n_nodes);
        DevBuf b_ptr, b_rid, b_cn, b_end, b_src, b_dst, b_sup;
        const int* d_ptr = upload(w.passthrough, b_ptr, pptr, st);
        const int* d_rid = upload(w.passthrough, b_rid, prid, st);
        const int* d_cn = upload(w.passthrough, b_cn, pcn, st);
        const uint8_t* d_end = upload(w.passthrough, b_end, isend, st);
        const int* d_src = upload(w.passthrough, b_src, esrc, st);
        const int* d_dst = upload(w.passthrough, b_dst, edst, st);
        int* d_sup = (int*)b_sup.ensure(sizeof(int) * (size_t)n_edges);
        launch_edge_support(st, nullptr, d_dst, d_ptr, d_rid, d_cn, d_end, d_src, n_edges, sorted, d_sup);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(support_out, d_sup, sizeof(int) * (size_t)n_edges, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return SC_OK;
    });
}
int sc_sample_level(sc_ctx* h, int S, const double* a0, int n_reads, const double* ll, const unsigned char* has, int n_ent,
                    int e0, const int* ent_rid, const int* ent_cn, const int* ent_sym, const int* mate_off, const int* mate_idx,
                    int n_sweeps, const double* U, int n_u, unsigned* kdraw, unsigned* cnt, long* out) {
    if (!h || !a0 || !ll || !has || !ent_rid || !ent_cn || !ent_sym || !mate_off || !U || !kdraw || !cnt || !out) return SC_ERR_ARG;
    Ctx* ctx = &h->c;
    // the resident workers run the same level body; this entry launches the level itself
    if (ctx->resident || ctx->workers.size() != 1) return SC_ERR_ARG;
    if (S < 2 || S > MAXS || n_reads < 1 || n_ent < 1 || e0 < 0 || e0 > (1 << 20) || n_sweeps < 1) return SC_ERR_ARG;
    for (int s = 0; s < S; s++) if (!(a0[s] >= 0.0) || !std::isfinite(a0[s])) return SC_ERR_ARG;
    long Q = 0;
    for (int r = 0; r < n_ent; r++) {
        // (a symbol code, or 0xFF: a label that is no single symbol, as JobDev::qcode marks it -- drawn, not counted)
        const bool sym_ok = (ent_sym[r] >= 0 && ent_sym[r] < KMAX) || ent_sym[r] == 0xFF;
        if (ent_rid[r] < 0 || ent_rid[r] >= n_reads || ent_cn[r] < 1 || !sym_ok) return SC_ERR_ARG;
        Q += ent_cn[r];
    }
    if (Q * n_sweeps > MAX_DRAWS || n_u < Q * n_sweeps) return SC_ERR_ARG;
    for (long t = 0; t < Q * n_sweeps; t++) if (!(U[t] >= 0.0 && U[t] <= 1.0)) return SC_ERR_ARG;
    if (mate_off[0] != 0) return SC_ERR_ARG;
    for (int r = 0; r < n_reads; r++) if (mate_off[r + 1] < mate_off[r]) return SC_ERR_ARG;
    const int nm = mate_off[n_reads];
    if (nm > 0 && !mate_idx) return SC_ERR_ARG;
    for (int i = 0; i < nm; i++) if (mate_idx[i] < -1 || mate_idx[i] >= n_reads) return SC_ERR_ARG;
    return ctx_guarded(ctx, "sc_sample_level", [&] {
        Worker w;                                      // a private worker: own stream, own parameter / result blocks
        w.init_private(ctx);
        const int E = e0 + n_ent;
        LevelStub stub;
        FlatGraph& f = stub.f;
        f.K = KMAX; f.code_N = KMAX;
        stub.entries(e0, n_ent, n_reads, (size_t)E + 1);      // labels[E]: the strains' node label (read only by the update, which does not run)
        for (int r = 0, q = 0; r < n_ent; r++) {
            const size_t e = (size_t)(e0 + r);
            f.ent_rid[e] = ent_rid[r]; f.labels[e] = (uint8_t)ent_sym[r]; f.ent_cn[e] = ent_cn[r];
            stub.qoff[e] = q; q += ent_cn[r];
        }
        stub.mptr.assign(mate_off, mate_off + n_reads + 1);
        if (nm > 0) stub.midx.assign(mate_idx, mate_idx + nm);
        const hipStream_t st = w.st;
        // rows as in the region set-up; strain s lives in row slot(s), not in row s
        auto slot = [](int s) { return (s * 37 + 5) % MAXS; };
        std::vector<int> slots((size_t)S);
        for (int s = 0; s < S; s++) slots[(size_t)s] = slot(s);
        JobDev& jd = stub.upload(w, n_reads, std::max<long>(Q, 1), n_ent, Q * n_sweeps, S, slots.data(), ll, has);
        // the uniforms, padded by 2048 values as the context pads its stream (the chain stages windows of 1024)
        std::vector<double> u(U, U + Q * n_sweeps);
        u.resize((size_t)(Q * n_sweeps + 2048), 0.5);
        std::vector<float> uf(u.begin(), u.end());
        DevBuf b_u, b_uf;
        jd.U = upload(w.passthrough, b_u, u, st);
        jd.Uf = upload(w.passthrough, b_uf, uf, st);
        const JobDev* jd_dev = stub.publish(w);

        LevelParams& P = *w.Ph;
        for (int s = 0; s < S; s++) {
            P.sp[s] = StrainParam{slot(s), E, 1, 0, a0[s], 0.0};
            w.gp.slot[s] = (uint8_t)slot(s);
            w.gp.lab[s] = f.labels[(size_t)E];
        }
        LevelHdr H{};
        H.mode = MODE_SAMPLE; H.S = S; H.e0 = e0; H.e1 = E; H.Q = (int)Q; H.n_sweeps = n_sweeps;
        H.n_copy = 0; H.do_update = 0; H.seq = 1;
        std::memset(w.Rh, 0, sizeof(LevelResult));
        const LevelItem it = w.level_item(jd_dev, H, KMAX);
        const int kind = item_kind(it.kind);
        const int done = launch_level(st, it, w.gp, w.hp, n_reads);      // as the walk of a single region launches its levels
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        const LevelResult& R = *w.Rh;
        if (R.seq != 1u || R.error) throw ScError(SC_ERR_INTERNAL, "the sampler level did not complete");
        for (int s = 0; s < S; s++) kdraw[s] = R.kdraw[s];
        std::memcpy(cnt, R.cnt, sizeof(unsigned) * (size_t)S * KMAX);
        out[0] = (long)R.n_draws; out[1] = (long)R.n_slow; out[2] = (long)R.n_exact; out[3] = (long)R.n_pass; out[4] = kind; out[5] = done;
        return SC_OK;
    });
}
int sc_update_level(sc_ctx* h, int S, const int* slot, const int* lab_off, const int* lab_len, int K, int code_N, const double* lpt,
                    int n_reads, const double* ll, const unsigned char* has, const unsigned char* labels, int n_labels, int n_ent,
                    int e0, const int* ent_rid, const int* ent_lab_off, const int* ent_lab_len, const unsigned char* ent_first,
                    int n_copy, const int* copy_src, const int* copy_dst, int copy_n, double* ll_out, unsigned char* has_out,
                    unsigned char* isnew_out, int* done_out) {
    OneLevel a{};
    a.S = S; a.slot = slot; a.lab_off = lab_off; a.lab_len = lab_len; a.K = K; a.code_N = code_N; a.lpt = lpt; a.n_reads = n_reads;
    a.ll = ll; a.has = has; a.labels = labels; a.n_labels = n_labels; a.n_ent = n_ent; a.e0 = e0; a.ent_rid = ent_rid;
    a.ent_lab_off = ent_lab_off; a.ent_lab_len = ent_lab_len; a.ent_first = ent_first; a.n_copy = n_copy; a.copy_src = copy_src;
    a.copy_dst = copy_dst; a.copy_n = copy_n; a.ll_out = ll_out; a.has_out = has_out; a.isnew_out = isnew_out; a.done_out = done_out;
    return one_level(h, "sc_update_level", a, nullptr);
}
int sc_hard_level(sc_ctx* h, int S, const int* slot, const int* lab_off, const int* lab_len, int K, int code_N, const double* lpt,
                  const double* logpri, int n_reads, const double* ll, const unsigned char* has, const unsigned char* labels,
                  int n_labels, int n_ent, int e0, const int* ent_rid, const int* ent_cn, const int* ent_lab_off,
                  const int* ent_lab_len, const unsigned char* ent_first, const int* mate_off, const int* mate_idx, int n_copy,
                  const int* copy_src, const int* copy_dst, int copy_n, double* ll_out, unsigned char* has_out,
                  unsigned char* isnew_out, double* abund, double* subst, double* resp, int* qrid, int* quid, unsigned char* qcode,
                  int* done_out) {
    OneLevel a{};
    a.S = S; a.slot = slot; a.lab_off = lab_off; a.lab_len = lab_len; a.K = K; a.code_N = code_N; a.lpt = lpt; a.n_reads = n_reads;
    a.ll = ll; a.has = has; a.labels = labels; a.n_labels = n_labels; a.n_ent = n_ent; a.e0 = e0; a.ent_rid = ent_rid;
    a.ent_lab_off = ent_lab_off; a.ent_lab_len = ent_lab_len; a.ent_first = ent_first; a.n_copy = n_copy; a.copy_src = copy_src;
    a.copy_dst = copy_dst; a.copy_n = copy_n; a.ll_out = ll_out; a.has_out = has_out; a.isnew_out = isnew_out; a.done_out = done_out;
    const HardLevel hd{logpri, ent_cn, mate_off, mate_idx, abund, subst, resp, qrid, quid, qcode};
    return one_level(h, "sc_hard_level", a, &hd);
}
int sc_roi_release(sc_ctx* h, int handle) {
    if (!h) return SC_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->c.mu);
    auto it = h->c.jobs.find(handle);
    if (it == h->c.jobs.end() || it->second->status != 1) return SC_ERR_ARG;
    h->c.jobs.erase(it);
    return SC_OK;
}

int sc_msa_align(sc_ctx* h, const char* seq_text, const int* seq_off, int n, char* rows_out, long cap, int* ncol_out) {
    if (!h || !seq_text || !seq_off || n < 1 || !ncol_out) return SC_ERR_ARG;
    Ctx* ctx = &h->c;
    // runs on a private worker object (own stream) so it can be called while regions are in flight
    return ctx_guarded(ctx, "sc_msa_align", [&] {
        Worker w;
        w.init_private(ctx);
        std::vector<std::string> seqs((size_t)n), rows;
        for (int i = 0; i < n; i++) seqs[i].assign(seq_text + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
        int ncol;
        if (n == 1) { ncol = (int)seqs[0].size(); rows = seqs; }
        else ncol = w.msa_device(seqs, rows);
        *ncol_out = ncol;
        int rc = SC_OK;
        if (!rows_out || (long)n * (ncol + 1) > cap) rc = SC_ERR_CAPACITY;
        else for (int i = 0; i < n; i++) { std::memcpy(rows_out + (long)i * (ncol + 1), rows[i].data(), (size_t)ncol); rows_out[(long)i * (ncol + 1) + ncol] = 0; }
        return rc;
    });
}

}  // extern "C"
