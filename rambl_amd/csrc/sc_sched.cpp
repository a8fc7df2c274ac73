// The scheduler of libstraincall_hip.so: the parts of a context (staging arenas, set-up places, the level server or the
// resident grid), how a worker hands a level to the GPU and learns that it is done, and the context's life.
#include "sc_ctx.hpp"

namespace sc {

// ---- staging arenas, set-up places
PinnedArena* ArenaPool::lease(PinnedArena* passthrough) {
    if (limit <= 0) { passthrough->on = false; return passthrough; }
    for (;;) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!free_arenas.empty()) { PinnedArena* a = free_arenas.back(); free_arenas.pop_back(); a->reset(); return a; }
            if ((int)arenas.size() < limit) { arenas.emplace_back(new PinnedArena()); return arenas.back().get(); }
        }
        // every arena is with a region that is being set up: let those regions run
        if (FiberPool::in_fiber()) FiberPool::yield(); else std::this_thread::yield();
    }
}
void ArenaPool::release(PinnedArena* a) {
    std::lock_guard<std::mutex> lk(mu);
    free_arenas.push_back(a);
}
void SetupGate::enter(Worker* w) {
    {
        std::lock_guard<std::mutex> lk(mu);
        if (setups < limit) { setups++; return; }
        waiters.push_back(w);
    }
    FiberPool::park();                         // leave hands its place over and makes this fiber ready
}
void SetupGate::leave() {
    Worker* next = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!waiters.empty()) { next = waiters.front(); waiters.pop_front(); }
        else setups--;
    }
    if (next) pool->make_ready(next->fib, split_exec);          // (a set-up: for the pool's set-up threads)
}

// ---- the level server
// The level server (SC_RESIDENT=0, several slots).  Workers hand their next level to this thread and park; it is the only
// thread that launches level kernels and the only one that watches the completion stamps, so a finished level is seen
// within a microsecond however many regions are in flight, and nobody polls or contends for the launch path.
//   * A level's kernel stores its stamp into host memory after everything else it reports (system-scope release):
//     completion is seen without a stream synchronisation; the region's fiber is made ready and an executor thread
//     picks it up (no futex round trip per level).
//   * Launch streams are shared by all regions.  A stream carries one batch at a time, so kernels of different
//     regions never queue behind each other; while a stream is free, every waiting level (up to MAXB) leaves as one
//     grid, workgroup b = region b of the batch: the kernel of their kind when they all need the same one, k_level_any
//     (which calls the variant each item names) otherwise.
//   * A launch the runtime rejects fails the levels of its batch at once; a stream that drains while stamps of its
//     batch are still missing (a kernel that ended without stamping) fails them at the periodic check.
LevelServer::LevelServer(int device, int n_streams, bool sweep_log) : device(device), sweep_log(sweep_log), lstreams((size_t)n_streams) {
    thread = std::thread([this] { serve(); });
}
LevelServer::~LevelServer() {
    { std::lock_guard<std::mutex> lk(dmu); stop.store(true, std::memory_order_seq_cst); }
    dcv.notify_all();
    if (thread.joinable()) thread.join();
}
void LevelServer::serve() {
    (void)hipSetDevice(device);
    std::deque<LevelRequest> waiting;          // taken from `pending`, not launched yet
    std::vector<Flying> flying;                // launched, stamp not seen yet
    std::string dead;                          // non-empty: a launch stream has failed, every level fails from now on
    auto stamped = [](Worker* w) { return __atomic_load_n(&w->Rh->seq, __ATOMIC_ACQUIRE) == w->seq; };
    unsigned idle_spins = 0;
    double sweep_t0 = 0, sweep_sum = 0, sweep_max = 0; long sweep_n = 0, sweep_fly = 0;
    for (;;) {
        if (n_pending.load(std::memory_order_seq_cst) > 0) {
            plk.lock();
            const int took = (int)pending.size();
            waiting.insert(waiting.end(), pending.begin(), pending.end());
            pending.clear();
            plk.unlock();
            n_pending.fetch_sub(took, std::memory_order_seq_cst);
        } else if (waiting.empty() && flying.empty()) {
            // nothing to watch: sleep until a region hands a level in (announce first, then look again: submit_level looks at
            // the flag after it has counted its request)
            std::unique_lock<std::mutex> lk(dmu);
            asleep.store(true, std::memory_order_seq_cst);
            if (n_pending.load(std::memory_order_seq_cst) == 0 && !stop.load(std::memory_order_seq_cst)) dcv.wait_for(lk, std::chrono::milliseconds(50));
            asleep.store(false, std::memory_order_seq_cst);
            if (stop.load(std::memory_order_seq_cst)) break;
            continue;
        }
        bool progressed = false;
        if (sweep_log) {
            const double t = now_ms();
            if (sweep_t0 > 0 && !flying.empty()) { const double d = t - sweep_t0; sweep_sum += d; sweep_max = std::max(sweep_max, d); sweep_n++; sweep_fly += (long)flying.size(); }
            sweep_t0 = t;
        }
        // completions
        for (size_t i = 0; i < flying.size();) {
            Worker* w = flying[i].w;
            if (stamped(w)) {
                lstreams[(size_t)flying[i].stream].busy--;
                flying[i] = flying.back(); flying.pop_back();
                w->finish_level(2);
                progressed = true;
            } else {
                ++i;
            }
        }
        // launches
        while (!waiting.empty()) {
            if (!dead.empty()) { waiting.front().w->finish_level(3, dead.c_str()); waiting.pop_front(); progressed = true; continue; }
            int fs = -1;
            for (size_t i = 0; i < lstreams.size(); i++) if (lstreams[i].busy == 0) { fs = (int)i; break; }
            if (fs < 0) break;
            const int kind = waiting.front().kind;
            LevelBatch batch;
            Worker* who[MAXB];
            int n = 0;
            bool timed = false, mixed = false;
            for (auto it = waiting.begin(); it != waiting.end() && n < MAXB;) {
                mixed = mixed || it->kind != kind;
                batch.it[n] = it->item;
                who[n++] = it->w;
                timed = timed || it->timed;
                it = waiting.erase(it);
            }
            hipStream_t st = lstreams[(size_t)fs].s.st;
            (void)hipGetLastError();
            if (timed) for (int i = 0; i < n; i++) (void)hipEventRecord(who[i]->ev0, st);
            if (mixed) launch_level_any(st, batch, n);          // every waiting level, whatever variant it needs
            else launch_level_batch(st, kind, batch, n);
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) {
                // the runtime did not take the launch: nothing of this batch will ever stamp
                const std::string msg = std::string("level kernel launch: ") + hipGetErrorString(le);
                for (int i = 0; i < n; i++) who[i]->finish_level(3, msg.c_str());
                progressed = true;
                continue;
            }
            if (timed) for (int i = 0; i < n; i++) (void)hipEventRecord(who[i]->ev1, st);
            lstreams[(size_t)fs].busy = n;
            lstreams[(size_t)fs].unretired++;
            const double tl = now_ms();
            for (int i = 0; i < n; i++) { who[i]->t_batch_launched = tl; who[i]->batch_n = n; flying.push_back(Flying{who[i], fs}); }
            progressed = true;
        }
        if (progressed) { idle_spins = 0; continue; }
        if (idle_spins % 256u == 0) {
            // idle: let the runtime retire finished launches of one free stream (it does so only when asked; left alone
            // they pile up for whoever synchronises the device next, ~10 us each)
            for (auto& ls : lstreams)
                if (ls.busy == 0 && ls.unretired > 0) { if (hipStreamQuery(ls.s.st) == hipSuccess) ls.unretired = 0; break; }
        }
        __builtin_ia32_pause();
        if (++idle_spins % (1u << 20) == 0) {
            // nothing has moved for a while: has a stream died under its batch, or drained without every stamp of it?
            for (size_t si = 0; si < lstreams.size(); si++) {
                LaunchStream& ls = lstreams[si];
                if (ls.busy == 0) continue;
                const hipError_t e = hipStreamQuery(ls.s.st);
                if (e == hipErrorNotReady) continue;
                if (e != hipSuccess) { dead = std::string("level kernel: ") + hipGetErrorString(e); break; }
                // the stream is empty: every kernel of the batch has ended, so a stamp that is still missing now (read
                // again after the query) will never come
                for (size_t i = 0; i < flying.size();) {
                    Worker* w = flying[i].w;
                    if (flying[i].stream != (int)si || stamped(w)) { ++i; continue; }
                    ls.busy--;
                    flying[i] = flying.back(); flying.pop_back();
                    w->finish_level(3, "a level kernel ended without its completion stamp");
                }
            }
            if (!dead.empty()) {
                for (const Flying& fl : flying) { lstreams[(size_t)fl.stream].busy = 0; fl.w->finish_level(3, dead.c_str()); }
                flying.clear();
            }
        }
    }
    if (sweep_log && sweep_n) fprintf(stderr, "level server: %ld rounds with levels flying, %.2f us each (longest %.1f us), %.1f levels flying on average\n",
                                      sweep_n, 1e3 * sweep_sum / sweep_n, 1e3 * sweep_max, (double)sweep_fly / sweep_n);
    for (const Flying& fl : flying) fl.w->finish_level(3, "context destroyed");
    for (auto& rq : waiting) rq.w->finish_level(3, "context destroyed");
}
void LevelServer::submit(const LevelRequest& rq) {
    rq.w->level_state.store(1, std::memory_order_release);
    plk.lock();
    pending.push_back(rq);
    plk.unlock();
    n_pending.fetch_add(1, std::memory_order_seq_cst);
    if (asleep.load(std::memory_order_seq_cst)) {
        { std::lock_guard<std::mutex> lk(dmu); }
        dcv.notify_one();
    }
}

// ---- the resident grid
static int top_priority() {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    return hi;
}
ResidentGrid::ResidentGrid(Ctx& ctx, int slots, bool watch_stamps, int n_workers)
    : slots(slots), mail((size_t)slots), mail_seq((size_t)slots, 0u), mail_done((size_t)slots, 0u),
      watch(watch_stamps ? new StampWatch((size_t)n_workers) : nullptr), ctx(ctx), rstream(top_priority()), ctl(1) {
    for (int m = slots - 1; m >= 0; m--) free_mail.push_back(m);
    std::memset(mail.p, 0, (size_t)slots * sizeof(Mailbox));
    std::memset(ctl.p, 0, sizeof(ResidentCtl));
    heart = std::thread([this] {
        unsigned beats = 0;
        while (!heart_stop.load(std::memory_order_acquire)) {
            __atomic_fetch_add(&ctl.p->heartbeat, 1u, __ATOMIC_RELEASE);
            if (watch && (++beats % 50u) == 0) poll_health();
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    });
}
ResidentGrid::~ResidentGrid() {
    shutdown();
    heart_stop.store(true, std::memory_order_release);
    if (heart.joinable()) heart.join();
}
// The region's set-up is done: a mailbox to walk its levels on.  Parks until one falls free.
int ResidentGrid::acquire_mailbox(Worker* w) {
    {
        std::lock_guard<std::mutex> lk(mmu);
        if (!free_mail.empty()) { const int m = free_mail.back(); free_mail.pop_back(); return m; }
        w->mslot.store(-1, std::memory_order_release);
        mail_waiters.push_back(w);
    }
    FiberPool::park();                         // release_mailbox hands one over (w->mslot) and makes the fiber ready
    return w->mslot.load(std::memory_order_acquire);
}
void ResidentGrid::release_mailbox(int m) {
    Worker* next = nullptr;
    {
        std::lock_guard<std::mutex> lk(mmu);
        if (!mail_waiters.empty()) { next = mail_waiters.front(); mail_waiters.pop_front(); next->mslot.store(m, std::memory_order_release); }
        else free_mail.push_back(m);
    }
    if (next) ctx.pool->make_ready(next->fib);
}
// A level is about to be posted to mailbox m: make sure a generation of the resident grid is there to take it.
void ResidentGrid::ensure(int m) {
    // the ordinary case, once per level from every executor, takes no lock: the generation runs and the mailbox's workgroup is there
    if (gen_state.load(std::memory_order_acquire) == GEN_RUNNING && __atomic_load_n(&mail.p[m].state, __ATOMIC_ACQUIRE) < 2u) return;
    const double t0 = now_ms();
    for (;;) {
        if (now_ms() - t0 > 60000.0) throw HipError("resident level workers: the previous grid has not left after a minute");
        {
            std::lock_guard<std::mutex> lk(gen_mu);
            if (gen_state == GEN_RUNNING) {
                if (__atomic_load_n(&mail.p[m].state, __ATOMIC_ACQUIRE) < 2u) return;
                // the slot's workgroup has left although regions are in flight (the heartbeat limit): end this generation
                __atomic_store_n(&ctl.p->stop, 1u, __ATOMIC_RELEASE);
                gen_state = GEN_STOPPING;
            }
            if (gen_state == GEN_STOPPING) {
                const hipError_t e = hipStreamQuery(rstream.st);
                if (e == hipSuccess) gen_state = GEN_STOPPED;
                else if (e != hipErrorNotReady) throw HipError(std::string("resident level workers: ") + hipGetErrorString(e));
            }
            if (gen_state == GEN_STOPPED) {
                __atomic_store_n(&ctl.p->stop, 0u, __ATOMIC_RELEASE);
                // a workgroup starts from the last stamp its mailbox has seen completed: what is in the mailbox beyond that is new
                for (int i = 0; i < slots; i++) { mail.p[i].ack = __atomic_load_n(&mail_done[(size_t)i], __ATOMIC_ACQUIRE); mail.p[i].state = 0; }
                __atomic_thread_fence(__ATOMIC_RELEASE);
                ResidentArgs ra{mail.d, ctl.d, 300000000ull, ctx.workers[0]->Pm, ctx.workers[0]->Rd, (int)ctx.workers.size()};     // 3 s of 100 MHz ticks without a heartbeat
                (void)hipGetLastError();
                launch_resident(rstream.st, ra, slots);
                const hipError_t le = hipGetLastError();
                if (le != hipSuccess) throw HipError(std::string("resident level workers, launch: ") + hipGetErrorString(le));
                gen_state = GEN_RUNNING;
                return;
            }
        }
        if (FiberPool::in_fiber() && ctx.workers.size() > 1) FiberPool::yield(); else std::this_thread::yield();
    }
}
// No region is in flight any more: the generation ends, so that nothing of this context stays on the GPU while the
// caller does something else with it (a device synchronisation would wait for the grid).
void ResidentGrid::idle() {
    std::lock_guard<std::mutex> lk(gen_mu);
    if (gen_state == GEN_RUNNING && ctx.regions_active.load(std::memory_order_acquire) == 0) {
        __atomic_store_n(&ctl.p->stop, 1u, __ATOMIC_RELEASE);
        gen_state = GEN_STOPPING;
    }
}
void ResidentGrid::shutdown() {
    {
        std::lock_guard<std::mutex> lk(gen_mu);
        __atomic_store_n(&ctl.p->stop, 1u, __ATOMIC_RELEASE);
        if (gen_state == GEN_RUNNING) gen_state = GEN_STOPPING;
    }
    // the grid leaves within a few naps of its pollers; bounded, so that a workgroup that does not leave cannot hold the host
    const double t0 = now_ms();
    while (hipStreamQuery(rstream.st) == hipErrorNotReady && now_ms() - t0 < 10000.0) std::this_thread::sleep_for(std::chrono::microseconds(100));
    gen_state = GEN_STOPPED;
}
// Why a level posted to resident workgroup `mb` will never be stamped `want`, or nullptr while it still may be.  (The
// mailbox's state is read before the stamp: a workgroup stamps its last level before it leaves.)
static const char* resident_failure(const Mailbox& mb, const unsigned* stamp, unsigned want, double t_posted) {
    const unsigned ms = __atomic_load_n(&mb.state, __ATOMIC_ACQUIRE);
    const bool never = ms == 0u && now_ms() - t_posted > 20000.0;       // more slots than the GPU holds resident
    if ((ms < 2u && !never) || __atomic_load_n(stamp, __ATOMIC_ACQUIRE) == want) return nullptr;
    return never ? "the slot's resident level worker has not started within 20 s (more slots than the GPU holds resident workgroups?)"
         : ms == 3u ? "the slot's resident level worker received an item that was not its own"
                    : "the slot's resident level worker has left before the level was done";
}
bool ResidentGrid::poll_stamps() {
    Ctx* c = &ctx;
    return watch->poll([c](size_t i) { return &c->workers[i]->Rh->seq; }, [c](size_t i) { c->workers[i]->finish_level(2); });
}
void ResidentGrid::poll_health() {
    watch->check(
        [this](size_t i, unsigned want) -> const char* {
            const Worker* w = ctx.workers[i].get();
            const int m = w->mslot.load(std::memory_order_acquire);
            return m < 0 ? nullptr : resident_failure(mail.p[m], &w->Rh->seq, want, w->t_posted.load(std::memory_order_acquire));
        },
        [this](size_t i, const char* why) { ctx.workers[i]->finish_level(3, why); });
}

// ---- a worker and its levels
void Worker::init() {
    HIPCHK(hipSetDevice(ctx->device));
    if (!st) { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); own_stream = true; }
    HIPCHK(hipEventCreateWithFlags(&sync_ev, hipEventDisableTiming));
    if (!Ph) {
        own_blocks = true;
        HIPCHK(hipHostMalloc((void**)&Ph, sizeof(LevelParams), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipMalloc((void**)&Pd, sizeof(LevelParams)));
        HIPCHK(hipHostMalloc((void**)&Rh, sizeof(LevelResult), hipHostMallocMapped | hipHostMallocCoherent));
    }
    HIPCHK(hipHostGetDevicePointer((void**)&Pm, Ph, 0));
    HIPCHK(hipHostGetDevicePointer((void**)&Rd, Rh, 0));
    std::memset(Rh, 0, sizeof(LevelResult));
    cnt_scratch.assign((size_t)MAXS * KMAX, 0);
}
// A worker outside the context's slots, for an entry that may run while regions are in flight: its own stream and
// parameter / result blocks, its copies passed through.
void Worker::init_private(Ctx* c) {
    ctx = c;
    init();
    stage = &passthrough;
    passthrough.on = false;
}
Worker::~Worker() {
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (sync_ev) (void)hipEventDestroy(sync_ev);
    if (st && own_stream) (void)hipStreamDestroy(st);
    if (own_blocks) { (void)hipHostFree(Ph); (void)hipFree(Pd); (void)hipHostFree(Rh); }
}

// Everything this worker has put on its set-up stream is done.  The stream is shared with other regions, so the wait is
// for an event recorded now, not for the stream to drain; a fiber lets the other ready regions run meanwhile.
void Worker::sync_stream() {
    if (!FiberPool::in_fiber() || ctx->workers.size() <= 1) { HIPCHK(hipStreamSynchronize(st)); return; }
    HIPCHK(hipEventRecord(sync_ev, st));
    const double t0 = now_ms();
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = hipEventQuery(sync_ev);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) throw HipError(std::string("set-up stream: ") + hipGetErrorString(e));
        // a set-up stream that makes no progress for minutes is stuck (e.g. queued behind something that waits for this
        // region): an error for this region, not a hang of the process
        if ((spins & 0x3FFu) == 0x3FFu && now_ms() - t0 > 180000.0) throw HipError("set-up stream: no progress for 3 minutes");
        // the copies / kernels waited for take from 0.1 to a few milliseconds: while nothing else is ready, this thread sleeps a
        // little instead of going round the scheduler (its lock is the one the level server makes regions ready under)
        if (ctx->pool->ready_now() == 0) std::this_thread::sleep_for(std::chrono::microseconds(40));
        FiberPool::yield();
    }
}

// The region's fiber parks until the level server or an executor has seen the level's stamp (or failed the level).  That
// thread makes the fiber ready exactly once per level (finish_level), so the fiber parks exactly once per level -- also
// when the level is already done by the time it gets here (it then comes straight back).
void Worker::wait_level() {
    const double t_park = now_ms();
    FiberPool::park();
    const double t_back = now_ms();
    wake_acc[0] += t_park - t_posted.load(std::memory_order_relaxed);      // handing the level over
    wake_acc[1] += t_back - t_seen;             // the stamp has been seen -> this fiber runs again
    if (ctx->log) { const double us = 1e3 * (t_back - t_seen); int b = 0; while (b < 23 && us >= (double)(1 << b)) b++; ctx->log->wake_hist[b].fetch_add(1, std::memory_order_relaxed); }
    const int state = level_state.load(std::memory_order_acquire);
    if (state == 3) throw HipError(level_err);
    if (state != 2) throw HipError("a region was resumed before its level was done");
}
// The level's wait is over (2: its stamp was seen, 3: failed, `err` says why): the region's fiber may run.  Once per wait.
void Worker::finish_level(int state, const char* err) {
    if (err) level_err = err;
    t_seen = now_ms();
    level_state.store(state, std::memory_order_release);
    ctx->pool->make_ready(fib);
}
// Hands a level to the GPU and returns once its completion stamp has been seen; throws when it never will be.  A resident
// context posts the level to the region's mailbox, any other launches it: the worker itself when it is the context's
// only one, the level server otherwise.  The only worker of a context spins for the stamp itself; any other parks until
// the executors (resident) or the level server have seen it.
void Worker::complete_level(const LevelItem& it, int n_reads, bool timed) {
    const unsigned want = it.h.seq;
    level_done = it.h.done;
    const bool alone = ctx->workers.size() == 1;
    if (grid) {
        // the slot's resident workgroup takes the level from its mailbox: the item, then its stamp (release)
        const int m = mslot.load(std::memory_order_relaxed);
        grid->ensure(m);
        Mailbox& mb = grid->mail.p[m];
        mb.item = it;
        __atomic_store_n(&mb.seq, want, __ATOMIC_RELEASE);
        const double t = now_ms();
        t_posted.store(t, std::memory_order_release);
        t_batch_launched = t; batch_n = 1;
        if (alone) {
            for (unsigned spins = 0; __atomic_load_n(&Rh->seq, __ATOMIC_ACQUIRE) != want;) {
                __builtin_ia32_pause();
                if (++spins % (1u << 20) == 0)
                    if (const char* why = resident_failure(mb, &Rh->seq, want, t)) throw HipError(why);
            }
        } else {
            level_state.store(1, std::memory_order_release);
            grid->watch->arm((size_t)slot, want);        // (the mailbox and t_posted are written: an executor may look)
            ctx->pool->ensure_poller();
            wait_level();
        }
        __atomic_store_n(&grid->mail_done[(size_t)m], want, __ATOMIC_RELEASE);
    } else if (alone) {
        // nobody to batch with: the worker launches its level itself, with whatever pieces of it go on a grid in front (the
        // pair of events brackets them all)
        hipStream_t ls = ctx->launch->st;
        if (timed) HIPCHK(hipEventRecord(ev0, ls));
        (void)hipGetLastError();
        level_done = launch_level(ls, it, gp, hp, n_reads);
        { const hipError_t le = hipGetLastError(); if (le != hipSuccess) throw HipError(std::string("level kernel launch: ") + hipGetErrorString(le)); }
        if (timed) HIPCHK(hipEventRecord(ev1, ls));
        t_batch_launched = now_ms(); batch_n = 1;
        // while this level runs: let the runtime retire the launches behind it (it does so only when asked, and a
        // region leaves ~1 500 of them for whoever synchronises the device next: ~10 us each)
        (void)hipStreamQuery(ls);
        for (unsigned spins = 0; __atomic_load_n(&Rh->seq, __ATOMIC_ACQUIRE) != want;) {
            __builtin_ia32_pause();
            if ((++spins & 0x3FFFFu) == 0) {             // every few milliseconds: has the stream died?
                const hipError_t e = hipStreamQuery(ls);
                if (e == hipSuccess) { if (__atomic_load_n(&Rh->seq, __ATOMIC_ACQUIRE) != want) throw HipError("a level kernel ended without its completion stamp"); }
                else if (e != hipErrorNotReady) throw HipError(std::string("level kernel: ") + hipGetErrorString(e));
            }
        }
    } else {
        t_posted.store(now_ms(), std::memory_order_release);
        ctx->server->submit(LevelRequest{this, it, item_kind(it.kind), timed});
        wait_level();
    }
}

// The body of a slot's fiber: takes regions off the context's queue until the context stops; parks in `idle` while there
// is none (sc_roi_submit makes one idle slot ready per region it queues).
void Worker::run() {
    for (;;) {
        std::shared_ptr<Job> job;
        bool parked = false;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (!ctx->queue.empty()) { job = ctx->queue.front(); ctx->queue.pop_front(); }
            else if (ctx->stop) break;
            else { ctx->idle.push_back(this); parked = true; }
        }
        if (parked) { FiberPool::park(); continue; }
        try {
            if (!st || !Ph) throw HipError("the slot's stream or host-mapped blocks were not created");
            process(*job);
            job->rc = SC_OK;
        } catch (const ScError& ex) { job->rc = ex.code; job->err = ex.what(); }
        catch (const HipError& ex) { job->rc = SC_ERR_HIP; job->err = ex.what(); }
        catch (const std::exception& ex) { job->rc = SC_ERR_INTERNAL; job->err = ex.what(); }
        catch (...) { job->rc = SC_ERR_INTERNAL; job->err = "unknown exception"; }
        // the last region in flight takes the resident grid with it -- before the caller learns that the region is done,
        // so that whoever waits for the region and then synchronises the device finds the grid on its way out
        if (ctx->regions_active.fetch_sub(1, std::memory_order_acq_rel) == 1 && grid) grid->idle();
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            job->status = 1;
            if (job->rc != SC_OK) ctx->last_error = job->err;
        }
        ctx->cv_done.notify_all();
    }
    ctx->fibers_left.fetch_sub(1, std::memory_order_release);
}

// ---- the context, and the CPUs it runs on
// The CPUs next to a GPU: `local_cpulist` of its PCI device (the cores of the socket its root port hangs on), within what
// the process may use.  A GPU box is a two-socket host whose scheduler moves a rank's threads over both; the level
// mailboxes, the completion stamps and the host-mapped parameter blocks are read and written across PCIe by both sides
// several hundred thousand times a second, and from the far socket every one of those crosses the socket link as well.
bool gpu_local_cpus(int device, cpu_set_t* out) {
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return false;
    for (char* c = bdf; *c; c++) *c = (char)tolower((unsigned char)*c);
    FILE* f = fopen((std::string("/sys/bus/pci/devices/") + bdf + "/local_cpulist").c_str(), "r");
    if (!f) return false;
    char line[4096] = {0};
    const bool got = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!got) return false;
    cpu_set_t allowed, local;
    CPU_ZERO(&local);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return false;
    for (const char* c = line; *c && *c != '\n';) {                       // "0-63,128-191"
        char* end = nullptr;
        const long a = strtol(c, &end, 10);
        if (end == c) break;
        long b = a;
        c = end;
        if (*c == '-') { b = strtol(c + 1, &end, 10); c = end; }
        for (long k = a; k <= b && k < CPU_SETSIZE; k++) if (k >= 0 && CPU_ISSET((int)k, &allowed)) CPU_SET((int)k, &local);
        if (*c == ',') c++;
    }
    if (CPU_COUNT(&local) == 0) return false;
    *out = local;
    return true;
}

// The streams are created in this order: the grid's, the launch streams, the set-up streams.
Ctx::Ctx(int device, const CtxPlan& p)
    : device(device), plan(p), resident(p.resident), U(uniform_stream(1234u, MAX_DRAWS + 2048)),   // padded: the chain stages windows of 1024
      arenas(p.arena_limit), P_all((size_t)p.workers), R_all((size_t)p.workers), Pd_all((size_t)p.workers),
      gate(p.setup_limit, p.long_threads > 0, pool) {
    DevBuf::keep = !p.opt.off(p.opt.devbuf_keep);
    if (p.resident) grid.reset(new ResidentGrid(*this, p.res_slots, p.watch, p.workers));
    if (p.server) server.reset(new LevelServer(device, p.launch_streams, p.opt.server_log));
    else launch.reset(new Stream());
    setup_streams.reserve((size_t)p.setup_streams);
    for (int i = 0; i < p.setup_streams; i++) setup_streams.emplace_back();
    for (int i = 0; i < p.workers; i++) {
        auto w = std::make_unique<Worker>();
        w->ctx = this;
        w->grid = grid.get();
        w->slot = i;
        w->st = setup_streams[(size_t)i % setup_streams.size()].st;
        w->Ph = P_all.p + i; w->Rh = R_all.p + i; w->Pd = Pd_all.p + i;
        workers.push_back(std::move(w));
    }
    for (auto& w : workers) w->init();
    const int dev = device;
    pool.reset(new FiberPool(p.exec_threads, [dev] { (void)hipSetDevice(dev); }, p.long_threads));
    if (p.opt.server_log) {
        pool->set_diag(true);
        log.reset(new ServerLog());
        log->t_created = now_ms(); log->n_fast = p.exec_threads - p.long_threads; log->n_long = p.long_threads;
    }
    if (p.watch) { ResidentGrid* g = grid.get(); pool->set_poll([g] { return g->poll_stamps(); }); }
    fibers_left.store(p.workers, std::memory_order_release);
    for (auto& w : workers) {
        Worker* q = w.get();
        q->fib = pool->create([q] { q->run(); });
        if (!q->fib) { last_error = "cannot map a fiber stack"; fibers_left.fetch_sub(1); continue; }
        pool->make_ready(q->fib);
    }
}
Ctx::~Ctx() {
    std::vector<Worker*> wake;
    { std::lock_guard<std::mutex> lk(mu); stop = true; wake.swap(idle); }
    for (Worker* w : wake) pool->make_ready(w->fib);
    // regions still queued or in flight are finished first (as the worker threads of earlier versions did)
    while (fibers_left.load(std::memory_order_acquire) > 0) std::this_thread::sleep_for(std::chrono::microseconds(200));
    server.reset();
    pool->shutdown();
    if (log) {
        // diagnostics: how busy the two kinds of executor were (time stamp counter against the wall clock of the context's
        // life), how long their stretches inside fibers were, how long a region whose level had come back waited for one
        fprintf(stderr, "executors: %d continuation + %d set-up threads over %.1f ms; inside fibers %.1f / %.1f Mticks\n", log->n_fast, log->n_long,
                now_ms() - log->t_created, pool->busy_ticks(false) * 1e-6, pool->busy_ticks(true) * 1e-6);
        for (int l = 0; l < 2; l++) {
            fprintf(stderr, "  stretches on %s threads (log2 ticks: count):", l ? "set-up" : "continuation");
            for (int b = 0; b < 40; b++) if (pool->stretch_count(l, b)) fprintf(stderr, " %d:%ld", b, pool->stretch_count(l, b));
            fprintf(stderr, "\n");
        }
        fprintf(stderr, "  wake latency (below 2^b us: count):");
        for (int b = 0; b < 24; b++) if (log->wake_hist[b].load()) fprintf(stderr, " %d:%ld", b, log->wake_hist[b].load());
        fprintf(stderr, "\n");
    }
    (void)hipSetDevice(device);
    grid.reset();
    // (the members go from here: the workers before the slot blocks, then the streams, the arenas, the uniforms)
}

}  // namespace sc

// Binds the calling thread -- and every thread it starts afterwards -- to the CPUs next to GPU `device` (what a launcher does
// with `numactl --cpunodebind` per rank).  Returns how many CPUs that is; 0 when the topology is not known, the device does not
// exist or SC_NUMA_BIND=0: nothing is changed then.  sc_ctx_create does the same for the threads and the host memory of the
// context itself and leaves its caller where it was.
extern "C" int sc_host_bind(int device) {
    return std::max(0, sc::guarded(nullptr, "sc_host_bind", [&] {        // a failure of any kind is "nothing changed": 0
        if (!sc::has_device(device)) return 0;
        cpu_set_t local;
        const sc::Options opt = sc::read_options();
        if (opt.off(opt.numa_bind) || !sc::gpu_local_cpus(device, &local)) return 0;
        if (sched_setaffinity(0, sizeof local, &local) != 0) return 0;
        return CPU_COUNT(&local);
    }));
}
