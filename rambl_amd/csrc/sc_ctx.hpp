// The scheduler's types: a context (Ctx) of slots (Worker), each running one region (Job) at a time as a fiber, and the
// parts a context is composed of.  Each part owns what it allocates and keeps the lock that guards its fields.
//
// Per context of several regions: resident level workers whose stamps the executor threads watch (ResidentGrid::poll_stamps),
// or with SC_RESIDENT=0 the level server (LevelServer::serve), which launches the levels of different regions as one grid on
// one of a few shared streams, so that a hundred regions in flight need no more hardware queues than the GPU runs at once.
// A context has the one or the other, never both; the only worker of a context launches its levels itself.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/straincall_hip.h"
#include "sc_device.hpp"
#include "sc_fiber.hpp"
#include "sc_graph.hpp"
#include "sc_host.hpp"
#include "sc_plan.hpp"

namespace sc {

// launchers defined in sc_graph_kernels.hip ...
void launch_edge_support(hipStream_t st, const int* out_ptr, const int* out_node, const int* pool_ptr, const int* pool_rid,
                         const int* pool_cn, const uint8_t* node_is_end, const int* edge_src, int n_edges, int sorted,
                         int* support);
void launch_msa(hipStream_t st, const MsaDev& d);
void launch_thread(hipStream_t st, const ThreadDev& d, int* pool_sorted);
int init_graph_kernels();
// ... and in sc_level.hip
bool level_wants_grid(int n_reads, const LevelHdr& h);
int launch_level_grid(hipStream_t st, const JobDev* job, int n_reads, const LevelHdr& h, int kind, const GridParams& g, const HardPriors& pri,
                      const LevelParams* P, LevelResult* R, bool lone);
int launch_level(hipStream_t st, const LevelItem& it, const GridParams& g, const HardPriors& pri, int n_reads);
int level_kind(const LevelHdr& h);
int level_lds_kb(const LevelHdr& h, int K);
int level_table_capacity();
void launch_level_batch(hipStream_t st, int kind, const LevelBatch& b, int n);
void launch_level_any(hipStream_t st, const LevelBatch& b, int n);
void launch_resident(hipStream_t st, const ResidentArgs& a, int slots);
int init_level_kernels();
// the dynamic-LDS attributes of every kernel that needs one; nonzero: a HIP error
inline int init_kernels() { return init_level_kernels() | init_graph_kernels(); }

// ---------------------------------------------------------------------------
struct Job {
    int handle = 0;
    // inputs
    std::string ref;
    std::vector<AlignedRead> reads;
    std::vector<int> mate_off, mate_idx;
    sc_params params{};
    // outputs
    std::vector<std::string> seqs;
    std::vector<double> abund;
    std::string graph_dump, trace;
    std::vector<int> edge_support;
    std::vector<int> thr_count, thr_first, thr_pool;
    std::vector<int> thr_smin, thr_emin, thr_tmin;   // kept with thr_count, for sc_roi_thread_edges
    std::string thr_sym;
    sc_stats stats{};
    double t_submit = 0;
    int status = 0;       // 0 queued/running, 1 done
    int rc = SC_OK;
    std::string err;
};

typedef long double ld;               // the reference keeps abundances and counts in DoubleL = long double (x87 80-bit)

struct Ctx;
struct Worker;
// Page-locked staging arenas, shared: a region holds one only while it is set up, so a handful serves any number in flight.
struct ArenaPool {
    explicit ArenaPool(int limit) : limit(limit) {}
    PinnedArena* lease(PinnedArena* passthrough);
    void release(PinnedArena* a);
private:
    const int limit;                  // 0: staging off (one region in flight, or SC_PINNED_STAGING=0)
    std::mutex mu;
    std::vector<std::unique_ptr<PinnedArena>> arenas;
    std::vector<PinnedArena*> free_arenas;
};
// Regions being set up (graph construction: tens of milliseconds of one CPU each) at any one time: a part of the
// executor threads only, so that the others stay free for the continuations of the regions in flight.
struct SetupGate {
    SetupGate(int limit, bool split_exec, const std::unique_ptr<FiberPool>& pool) : split_exec(split_exec), limit(limit), pool(pool) {}
    void enter(Worker* w);
    void leave();
    const bool split_exec;            // the pool has threads of its own for the set-ups
private:
    const int limit;
    const std::unique_ptr<FiberPool>& pool;
    std::mutex mu;                    // set-up places: regions that found none park in line (they used to go round the scheduler)
    int setups = 0;
    std::deque<Worker*> waiters;
};
// A level waiting for its launch: the worker's slot, the level's scalars and which kernel it needs.
struct LevelRequest { Worker* w; LevelItem item; int kind; bool timed; };
// The level server (SC_RESIDENT=0, several slots): one thread launches every level and sees every stamp (serve).
struct LevelServer {
    LevelServer(int device, int n_streams, bool sweep_log);
    ~LevelServer();                   // levels still waiting or in flight fail with "context destroyed"
    void submit(const LevelRequest& rq);
private:
    // Launch streams are shared by all regions in flight.  A stream carries one batch at a time (`busy` = regions of that
    // batch whose stamp has not been seen yet), so kernels of different regions never queue behind each other: a level
    // that finds every stream busy waits in `pending` and leaves with the next batch of its kind.
    struct LaunchStream { Stream s; int busy = 0; int unretired = 0; };
    struct Flying { Worker* w; int stream; };      // a level launched, its stamp not seen yet
    void serve();
    const int device;
    const bool sweep_log;                     // SC_SERVER_LOG: how long one round of the loop takes while levels fly
    std::vector<LaunchStream> lstreams;
    sc::SpinLock plk;                         // guards pending (a few nanoseconds per level from every executor: never a sleeping lock)
    std::deque<LevelRequest> pending;         // requests the server has not taken yet
    std::atomic<int> n_pending{0};
    std::mutex dmu;                           // the server sleeps here (dcv) while nothing is pending or in flight
    std::condition_variable dcv;
    std::atomic<bool> asleep{false};
    std::atomic<bool> stop{false};
    std::thread thread;
};
// Resident level workers (k_level_resident): while regions are in flight one workgroup per slot stays on its CU and
// takes the slot's levels from a mailbox in host-mapped memory; no launch per level.  A "generation" of the grid lives
// from the first level posted after an idle period until no region is in flight any more (so that a device
// synchronisation by the caller never waits on it), or until the context goes.
// Resident contexts of several regions have no level server: a worker whose level is in its mailbox arms its slot of
// `watch` and parks; the continuation threads look at the armed slots' stamps between two fibers and while they spin
// for one (FiberPool::set_poll), and the thread that sees a stamp makes the region ready.  The CPU a server would spend
// going round the stamps is an executor's.
struct ResidentGrid {
    ResidentGrid(Ctx& ctx, int slots, bool watch_stamps, int n_workers);
    ~ResidentGrid();                  // stops the heart and the grid (shutdown)
    void ensure(int m);
    void idle();
    void shutdown();
    // A region needs a mailbox only while it walks its levels; its set-up (graph, uploads) happens on a worker of its own
    // before that.  A context has more workers than mailboxes, so the next regions are set up while every workgroup is busy,
    // and a workgroup that finishes a region finds the next one ready (mailboxes are handed from region to region).
    int acquire_mailbox(Worker* w);
    void release_mailbox(int m);
    bool poll_stamps();                                  // true: some worker is still waiting for its stamp
    void poll_health();                                  // the heart thread, once a second: armed workers whose workgroup has gone
    const int slots;                  // mailboxes = workgroups of the grid: regions that can WALK at a time
    HostMapped<Mailbox> mail;
    std::vector<unsigned> mail_seq, mail_done;     // per mailbox: last stamp posted / seen completed
    const std::unique_ptr<StampWatch> watch;             // [workers]; null in a context of one worker
private:
    enum { GEN_STOPPED = 0, GEN_RUNNING = 1, GEN_STOPPING = 2 };
    Ctx& ctx;
    // The resident grid stays in its hardware queue for as long as regions are in flight: nothing else may ever be
    // queued behind it (a set-up kernel of a region behind the grid that waits for that region's levels would never
    // start).  Streams share hardware queues once there are more streams than queues, and queues are kept per
    // priority: the grid's stream is the only one of its priority, and this context creates few other streams.
    Stream rstream;
    HostMapped<ResidentCtl> ctl;
    std::mutex mmu;
    std::vector<int> free_mail;               // mailboxes nobody walks on
    std::deque<Worker*> mail_waiters;         // regions whose set-up is done, parked until a mailbox falls free
    std::mutex gen_mu;
    std::atomic<int> gen_state{GEN_STOPPED};  // written under gen_mu
    std::thread heart;                // keeps ResidentCtl::heartbeat moving while the context lives
    std::atomic<bool> heart_stop{false};
};
// SC_SERVER_LOG: what the context prints about its executors when it goes
struct ServerLog {
    double t_created = 0; int n_fast = 0, n_long = 0;
    std::atomic<long> wake_hist[24] = {};      // wake latencies, bucket b = below 2^b us
};

// mt19937(1234) on the device: the stream every sampler call starts from (uniform_stream), and its fp32 copy
struct Uniforms {
    DevMem<double> d; DevMem<float> f;
    explicit Uniforms(const std::vector<double>& u) : d(u), f(std::vector<float>(u.begin(), u.end())) {}
};
// The members go in the reverse of this order, which is the order ~Ctx needs: a context that fails half-way through its
// constructor is taken apart by the members it has.
struct Ctx {
    Ctx(int device, const CtxPlan& plan);      // throws HipError
    ~Ctx();
    const int device;
    const CtxPlan plan;
    const bool resident;              // has a grid
    const Uniforms U;
    ArenaPool arenas;
    std::vector<Stream> setup_streams;        // uploads, graph kernels: shared round-robin by the workers
    std::unique_ptr<Stream> launch;           // the only worker's, when there is no server to launch its levels
    HostMapped<LevelParams> P_all;            // host-mapped blocks of all slots (one allocation each)
    HostMapped<LevelResult> R_all;
    DevMem<LevelParams> Pd_all;
    std::string last_error;
    std::mutex mu;                    // guards queue, jobs, idle, stop, last_error, job status
    std::condition_variable cv_done;
    std::deque<std::shared_ptr<Job>> queue;
    std::map<int, std::shared_ptr<Job>> jobs;
    int next_handle = 1;
    bool stop = false;
    std::atomic<int> regions_active{0};
    // Regions in flight are fibers (sc_fiber.hpp): `workers` are the slots (stream_count of them, each with its device
    // buffers and its host-mapped parameter / result blocks), `pool` the few host threads that run whichever of them
    // is ready -- sized from the CPU quota of this rank, not from the number of regions in flight.
    std::vector<std::unique_ptr<Worker>> workers;       // (after P_all / R_all / Pd_all: the slots' blocks are the context's)
    std::vector<Worker*> idle;                // slots without a region, parked
    std::atomic<int> fibers_left{0};
    std::unique_ptr<ResidentGrid> grid;       // one of the two, or neither (one worker, not resident)
    std::unique_ptr<FiberPool> pool;
    std::unique_ptr<LevelServer> server;
    SetupGate gate;
    std::unique_ptr<ServerLog> log;
};

struct Worker {
    Ctx* ctx = nullptr;
    ResidentGrid* grid = nullptr;     // the context's, null when it has none (read once per level: no way round by the context)
    Fiber* fib = nullptr;
    int slot = 0;                     // worker index
    hipStream_t st = nullptr;         // a setup stream of the context (not owned), or a private one (own_stream)
    bool own_stream = false;
    hipEvent_t sync_ev = nullptr;     // marks "everything this worker has put on `st` so far" (sync_stream)
    // hand-shake with whoever sees the level's stamp: 1 = a level is on its way / in flight, 2 = its stamp was seen, 3 = failed
    std::atomic<int> level_state{0};
    std::string level_err;
    double t_seen = 0, wake_acc[2] = {0, 0};
    std::atomic<int> mslot{-1};       // the mailbox (= workgroup of the resident grid) this region walks on, -1 while it has none
    std::atomic<double> t_posted{0};  // when the level was handed over (the heart thread judges resident workgroups by it)
    double t_batch_launched = 0;      // diagnostics: when the level's batch was launched, and its size
    int batch_n = 0;
    int level_done = 0;               // diagnostics: the LV_* pieces of the last level that ran on a grid
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // the pair of the level being launched (from ev_pool when timing)
    std::vector<hipEvent_t> ev_pool;  // want_timing: one pair per sampler level of the region, read when the region is done
    size_t ev_used = 0;
    LevelParams* Ph = nullptr;        // host-mapped: written here, read by the level's kernel over PCIe
    LevelParams* Pm = nullptr;        //   its device address
    GridParams gp{};                  // beside Ph: what the grid kernels of the level take as kernel arguments, filled with Ph->sp / copy_*
    HardPriors hp{};                  // ... and Ph->sp[].logpri, for the hard update on the grid
    LevelParams* Pd = nullptr;        // device copy, only for the grid kernels of very large levels in a context of several regions
    LevelResult* Rh = nullptr;        // host-mapped, written by the kernel, stamped last
    LevelResult* Rd = nullptr;
    bool own_blocks = false;          // Ph / Pd / Rh are this worker's own allocations (a private worker: init_private)
    unsigned seq = 0;                 // stamp of the last level launched (the level server waits for it)
    DevBuf b_ent_rid, b_ent_cn, b_ent_lab_off, b_ent_lab_len, b_ent_first, b_ent_qoff, b_labels, b_mate_ptr, b_mate_idx,
        b_ll, b_has, b_isnew, b_tabA, b_tabLf, b_qcode, b_qent, b_quid, b_qrid, b_dlog, b_out_ptr, b_out_node, b_pool_ptr, b_pool_rid,
        b_pool_cn, b_isend, b_esrc, b_support, b_jobdev;
    DevBuf m_seqs, m_off, m_cols0, m_cols1, m_counts, m_moves, m_trace, m_out, m_edge;
    PinnedArena* stage = nullptr;     // page-locked staging of the region's uploads / downloads: leased from the context
                                      // for the region's set-up (ArenaPool::lease), handed back when its copies have landed
    PinnedArena passthrough;          // on = false
    DevBuf t_ref, t_pos, t_seqoff, t_seq, t_cigoff, t_cigop, t_ciglen, t_lut, t_tabs, t_pool, t_pool2;
    FlatGraph flat;                   // the level-major arrays of the region being set up / walked
    std::vector<int> ent_qoff_buf;
    bool setup_held = false;          // this region holds one of the context's set-up places
    std::vector<ld> cnt_scratch;      // [MAXS][KMAX] draws per (strain, read symbol) of the level just sampled

    ~Worker();
    void init();
    void init_private(Ctx* c);
    void run();
    void process(Job& job);
    void complete_level(const LevelItem& it, int n_reads, bool timed);
    void wait_level();
    void finish_level(int state, const char* err = nullptr);
    void sync_stream();
    int msa_device(const std::vector<std::string>& seqs, std::vector<std::string>& rows);
    void thread_device(const std::string& G, const std::vector<AlignedRead>& R, const std::vector<std::vector<CigarOp>>& cig,
                       ThreadTables& T);
    JobDev job_dev(PinnedArena& ar, const FlatGraph& f, const std::vector<int>& ent_qoff, const std::vector<int>& mate_off,
                   const std::vector<int>& mate_idx, int n_reads, long qcap, int max_entries, long max_draws);
    LevelItem level_item(const JobDev* job, const LevelHdr& H, int K) const {
        return LevelItem{job, H, pack_kind(level_kind(H), level_lds_kb(H, K)), Pm, Rd};
    }
    void cluster(Job& job, const PoGraph& g, FlatGraph& f);
};
// Sweeps of a sampler level of Q draw slots (NonparametricClustering.cpp:160 / :781): what the walk runs and what the
// region's draw log is sized for.
inline int level_sweeps(const sc_params& pa, long Q) { return (int)std::min<long>(pa.sweeps_cap, pa.draw_budget / std::max<long>(Q, 1)); }
// The mailbox a region walks its levels on (resident workers): handed on after its last level, or by an exception.
struct MailHold {
    Worker* w;
    void drop() { const int m = w->mslot.load(std::memory_order_relaxed); if (m >= 0) { w->mslot.store(-1, std::memory_order_release); w->grid->release_mailbox(m); } }
    ~MailHold() { drop(); }
};

// The level walk of one region on worker `w` (sc_walk.cpp); Worker::cluster has set the region up.
void walk_levels(Worker& w, Job& job, const FlatGraph& f, const JobDev& jd, const JobDev* jd_dev, const std::vector<int>& level_hi,
                 int final_e0, long total_copies, MailHold& mail);
bool gpu_local_cpus(int device, cpu_set_t* out);

}  // namespace sc
