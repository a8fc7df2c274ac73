// Phase times of an experiment build (-DSC_GRAPH_TIMING, never the product): phase(name) prints the time since the
// phase before it, or since construction, to stderr as "<prefix><name, padded to width> <ms> ms".  Without the flag the
// struct is empty and `on` lets a caller leave out what it does only for the timing (a stream synchronisation).
#pragma once
#ifdef SC_GRAPH_TIMING
#include <chrono>
#include <cstdio>
#endif

namespace sc {

struct PhaseTimer {
#ifdef SC_GRAPH_TIMING
    static constexpr bool on = true;
    const char* prefix;
    int width;
    double t0;
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    PhaseTimer(const char* prefix, int width) : prefix(prefix), width(width), t0(now()) {}
    void phase(const char* name) {
        const double t = now();
        fprintf(stderr, "%s%-*s %.2f ms\n", prefix, width, name, t - t0);
        t0 = t;
    }
#else
    static constexpr bool on = false;
    PhaseTimer(const char*, int) {}
    void phase(const char*) {}
#endif
};

}  // namespace sc
