// What a context is made of, decided before anything is allocated: the SC_* variables read once (read_options), and the
// arithmetic from (regions in flight, CUs, CPU share, options) to workers, mailboxes, streams and host threads
// (plan_context).  No HIP in here: tests/native/ctx_plan_check.cpp checks the plan on a machine without a GPU.
#pragma once
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace sc {

// std::mt19937 + std::generate_canonical<double,53> as libstdc++ has them
struct Mt19937 {
    uint32_t x[624]; int p = 624;
    explicit Mt19937(uint32_t seed) {
        x[0] = seed;
        for (int i = 1; i < 624; i++) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
    }
    uint32_t next() {
        if (p >= 624) {
            auto twist = [this](int k, int k1, int km) {
                const uint32_t y = (x[k] & 0x80000000u) | (x[k1] & 0x7fffffffu);
                x[k] = x[km] ^ (y >> 1) ^ ((y & 1) ? 0x9908b0dfu : 0);
            };
            for (int k = 0; k < 624 - 397; ++k) twist(k, k + 1, k + 397);
            for (int k = 624 - 397; k < 623; ++k) twist(k, k + 1, k + (397 - 624));
            twist(623, 0, 396);
            p = 0;
        }
        uint32_t z = x[p++];
        z ^= (z >> 11); z ^= (z << 7) & 0x9d2c5680u; z ^= (z << 15) & 0xefc60000u; z ^= (z >> 18);
        return z;
    }
    double canonical() {
        const double lo = (double)next(), hi = (double)next();
        const double r = (lo + hi * 4294967296.0) / 18446744073709551616.0;
        return r >= 1.0 ? 0x1.fffffffffffffp-1 : r;
    }
};
// mt19937(1234) -> generate_canonical<double,53>: the stream every sampler call of the reference starts from (NonparametricClustering.cpp:142,785)
inline std::vector<double> uniform_stream(unsigned seed, int n) {
    Mt19937 gen(seed);
    std::vector<double> u(n);
    for (double& v : u) v = gen.canonical();
    return u;
}

// The SC_* variables of the context, as sc_ctx_create found them.  A variable that is not set stays "not set": what
// that means is the plan's business.  INTEGRATION.md has the table.
struct OptInt { bool set = false; int v = 0; };
struct Options {
    OptInt resident, resident_slots, setup_workers, launch_streams, exec_threads, exec_long, pinned_staging, setup_limit,
        numa_bind, malloc_tune, devbuf_keep;
    bool sync_log = false, server_log = false, level_log = false;      // diagnostics: on when the variable is there
    std::string level_log_path;
    bool off(const OptInt& o) const { return o.set && o.v == 0; }
};
// NAME=value into `o` (the environment's, or a test's); false: not a variable of the context
inline bool set_option(Options& o, const std::string& name, const char* value) {
    const struct { const char* name; OptInt Options::*at; } ints[] = {
        {"SC_RESIDENT", &Options::resident}, {"SC_RESIDENT_SLOTS", &Options::resident_slots}, {"SC_SETUP_WORKERS", &Options::setup_workers},
        {"SC_LAUNCH_STREAMS", &Options::launch_streams}, {"SC_EXEC_THREADS", &Options::exec_threads}, {"SC_EXEC_LONG", &Options::exec_long},
        {"SC_PINNED_STAGING", &Options::pinned_staging}, {"SC_SETUP_LIMIT", &Options::setup_limit}, {"SC_NUMA_BIND", &Options::numa_bind},
        {"SC_MALLOC_TUNE", &Options::malloc_tune}, {"SC_DEVBUF_KEEP", &Options::devbuf_keep}};
    for (const auto& k : ints) if (name == k.name) { (o.*k.at).set = true; (o.*k.at).v = atoi(value); return true; }
    if (name == "SC_SYNC_LOG") o.sync_log = true;
    else if (name == "SC_SERVER_LOG") o.server_log = true;
    else if (name == "SC_LEVEL_LOG") { o.level_log = true; o.level_log_path = value; }
    else return false;
    return true;
}
inline Options read_options() {
    Options o;
    for (const char* name : {"SC_RESIDENT", "SC_RESIDENT_SLOTS", "SC_SETUP_WORKERS", "SC_LAUNCH_STREAMS", "SC_EXEC_THREADS", "SC_EXEC_LONG",
                             "SC_PINNED_STAGING", "SC_SETUP_LIMIT", "SC_NUMA_BIND", "SC_MALLOC_TUNE", "SC_DEVBUF_KEEP", "SC_SYNC_LOG",
                             "SC_SERVER_LOG", "SC_LEVEL_LOG"})
        if (const char* e = getenv(name)) (void)set_option(o, name, e);
    return o;
}

// CPUs this rank may use: the cgroup quota when there is one (a GPU box hands out a share of its host), divided among the
// ranks that share the host (one process per GPU: LOCAL_WORLD_SIZE, set by torch.distributed.run and by bench.py).
inline double cpu_budget_host() {
    double n = (double)std::thread::hardware_concurrency();
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[64] = {0};
        double period = 0;
        if (fscanf(f, "%63s %lf", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0) {
            const double q = atof(quota) / period;
            if (q > 0 && (n <= 0 || q < n)) n = q;
        }
        fclose(f);
    }
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0 && k < n) n = k; }
    return n > 1 ? n : 1;
}
inline int local_world_size() {
    const char* e = getenv("LOCAL_WORLD_SIZE");
    const int k = e ? atoi(e) : 1;
    return k > 1 ? k : 1;
}

// Host threads of a context with `stream_count` regions in flight on `cpus` CPUs shared by `local_world` ranks (both
// positive): out[0] executor threads, out[1] the level server, out[2] ingest threads.  sc_host_plan's arithmetic.
inline void host_plan(int stream_count, int local_world, double cpus, int* out) {
    double n = cpus / local_world;
    if (n < 1) n = 1;
    int exec = (int)n - 1;                     // one CPU for the level server
    if (exec < 1) exec = 1;
    if (exec > stream_count) exec = stream_count;
    if (exec > 32) exec = 32;
    out[0] = exec; out[1] = stream_count > 1 ? 1 : 0;
    out[2] = (int)std::min<double>(std::max<double>(n, 1), 32);
}

struct CtxPlan {
    Options opt;
    bool resident = false;            // resident level workers (a grid) instead of a launch per level
    int res_slots = 0;                // mailboxes = workgroups of the grid: regions that can WALK at a time
    int workers = 1;                  // slots: regions in flight (walking or being set up)
    int launch_streams = 1, setup_streams = 1;
    int exec_threads = 1, long_threads = 0;       // executor threads, and how many of them take the set-ups first
    bool watch = false;               // the executors watch the stamps themselves (resident, several workers)
    bool server = false;              // a level server thread (not resident, several workers)
    int arena_limit = 0;              // 0: staging off (one region in flight, or SC_PINNED_STAGING=0)
    int setup_limit = 1;
};
// The shape of a context of `stream_count` regions in flight on a GPU of `cu_count` CUs, for a rank with `cpus` CPUs of a
// host it shares with `local_world - 1` others.
inline CtxPlan plan_context(const Options& o, int stream_count, int cu_count, double cpus, int local_world) {
    CtxPlan p;
    p.opt = o;
    if (stream_count < 1) stream_count = 1;
    if (stream_count > 512) stream_count = 512;
    {
        // resident level workers: one workgroup per slot holds a CU (and all of its LDS) while regions are in flight, so the
        // slots stop short of the 256 CUs -- the set-up kernels of the regions (read threading, MSA, edge support) need CUs too
        // Default: resident workers when several regions are in flight (no launch per level, no stream held by the slowest
        // level of a batch: +30-60 % reads/s at 128-224 in flight); a launch per level for a single region (its level
        // kernels are then kernels of their own, which the compiler allocates ~5 % faster than the same code behind a call).
        p.resident = o.resident.set ? o.resident.v != 0 : stream_count > 1;
        // Measured on MI355X: 224 resident workgroups (8 wavefronts each, 1 792 in all) start, the ones beyond do not (232: their
        // regions wait for ever, or the grid faults) -- the kernel keeps its variants as functions, their stack frames live in
        // scratch memory, and the queue's scratch holds 7 wavefronts per CU.  32 CUs stay free for the set-up kernels.
        int cap = o.resident_slots.set ? o.resident_slots.v : std::max(cu_count - 32, 1);
        cap = cap < 1 ? 1 : (cap > cu_count ? cu_count : cap);
        p.res_slots = p.resident ? std::min(stream_count, cap) : stream_count;
        // workers = regions walking (one mailbox each) + regions being set up meanwhile: those the caller asks for beyond the
        // mailboxes (stream_count above the cap) or SC_SETUP_WORKERS.  None by default: on a 16-CPU share of a host the set-ups
        // are bounded by the CPUs, not by the workers that wait for one (measured: 0 / 28 / 56 extra, no difference beyond noise)
        if (p.resident && p.res_slots > 1) {
            int extra = 0;
            if (o.setup_workers.set) extra = std::max(0, o.setup_workers.v);
            stream_count = std::min(std::max(stream_count, p.res_slots + extra), 512);
        }
        p.workers = stream_count;
    }
    {
        int nl = o.launch_streams.set ? o.launch_streams.v : 11;
        nl = nl < 1 ? 1 : (nl > 30 ? 30 : nl);
        if (p.resident) nl = 1;                    // levels are not launched: one stream for the rare grid kernels of huge levels
        if (nl > stream_count) nl = stream_count;
        p.launch_streams = nl;
        p.setup_streams = stream_count >= 8 ? 4 : (stream_count > 1 ? 2 : 1);      // 11 + 4 + the null stream = 16 hardware queues
    }
    int plan[3] = {1, 0, 1};
    host_plan(stream_count, local_world, cpus, plan);
    // resident contexts of several regions: the executors watch the stamps themselves, and the level server's CPU is one more
    // executor's
    p.watch = p.resident && stream_count > 1;
    p.server = !p.watch && stream_count > 1;
    if (p.watch && plan[1] > 0) plan[0] = std::min(plan[0] + 1, std::min(stream_count, 32));
    if (o.exec_threads.set && o.exec_threads.v >= 1) plan[0] = std::min(o.exec_threads.v, stream_count);
    p.exec_threads = plan[0];
    {
        // page-locked staging of the regions' transfers: only worth it while other regions are in flight (it is their queues
        // that a pageable copy suspends); as many arenas as regions can be set up at once on this rank's executor threads
        const bool want = o.pinned_staging.set ? o.pinned_staging.v != 0 : stream_count > 1;
        p.arena_limit = want ? std::max(plan[0] + 1, 2) : 0;
        p.setup_limit = std::max(1, (plan[0] + 1) / 2);
        if (o.setup_limit.set) p.setup_limit = std::max(1, o.setup_limit.v);
    }
    // half of the executor threads take the regions' set-ups first (graph construction: tens of milliseconds each), the other
    // half never do: the continuation of a region whose level has come back is a few tens of microseconds and must not wait
    p.long_threads = plan[0] >= 2 ? plan[0] / 2 : 0;
    if (o.exec_long.set) p.long_threads = std::max(0, std::min(o.exec_long.v, plan[0] - 1));
    if (!o.setup_limit.set && p.long_threads > 0) p.setup_limit = 2 * p.long_threads;      // a set-up waits for the GPU part of its time
    return p;
}

}  // namespace sc
