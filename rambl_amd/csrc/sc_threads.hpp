// Host threads of the ingest and of a region's bulk copies: how many this rank may use, and the one pool they run on.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

namespace sc {

// Threads sc_aln_open, sc_aln_load_reads and sc_depth_scan may use: the cgroup quota rounded up ("<quota> <period>" or
// "max <period>"), divided among the ranks sharing the host, replaced by SC_INGEST_THREADS, 1..32.  Read at every call.
inline int ingest_threads() {
    long quota = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        long q = 0, per = 0;
        if (fscanf(f, "%ld %ld", &q, &per) == 2 && q > 0 && per > 0) quota = (q + per - 1) / per;
        fclose(f);
    }
    long n = (long)std::thread::hardware_concurrency();
    if (quota > 0 && quota < n) n = quota;
    if (const char* e = getenv("LOCAL_WORLD_SIZE")) { const long k = atol(e); if (k > 1) n = std::max<long>(n / k, 1); }
    if (const char* e = getenv("SC_INGEST_THREADS")) n = atol(e);
    return (int)std::min<long>(std::max<long>(n, 1), 32);
}

// fn(i, scratch) for i in [0, n), on up to `threads` threads taking indices from a shared counter (the items differ in size
// by orders of magnitude: a backbone class of 59 000 reads beside a sibling of three); every thread makes a scratch of its
// own with scratch().  On one thread the items run in order.  Exceptions of a helper end the process as they would on the
// calling thread.
template <class S, class F>
void parallel_items(int n, int threads, const S& scratch, const F& fn) {
    std::atomic<int> next{0};
    auto body = [&] {
        auto s = scratch();
        for (int i = next.fetch_add(1, std::memory_order_relaxed); i < n; i = next.fetch_add(1, std::memory_order_relaxed)) fn(i, s);
    };
    std::vector<std::thread> ts;
    for (int t = 1; t < threads && n >= 2; t++) ts.emplace_back(body);
    body();
    for (auto& t : ts) t.join();
}
template <class F>
void parallel_items(int n, int threads, const F& fn) {
    parallel_items(n, threads, [] { return 0; }, [&](int i, int&) { fn(i); });
}

}  // namespace sc
