// Host-side plumbing of libstraincall_hip.so: HIPCHK over the errors of sc_error.hpp, the device selection, and the HIP
// resources it owns by scope.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/straincall_hip.h"
#include "sc_error.hpp"

namespace sc {

static_assert(ERR_HIP == SC_ERR_HIP && ERR_INTERNAL == SC_ERR_INTERNAL, "sc_error.hpp restates two codes of the public header");
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw ::sc::HipError(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The one device selection of the library: the calling thread's HIP calls go to `device` from here on.
inline bool has_device(int device) {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev;
}
inline void select_device(int device) {
    if (!has_device(device)) throw ScError(SC_ERR_NO_DEVICE, "no HIP device");
    if (hipSetDevice(device) != hipSuccess) throw ScError(SC_ERR_HIP, "hipSetDevice failed");
}

// How many device allocations DevBuf and DevMem have made on this thread: a call that wants to report what it had to set
// aside takes the difference.
inline thread_local long device_allocs = 0;

// growable device buffer
// A device buffer that only grows.  While regions are in flight nothing is handed back to the driver (hipFree waits for
// the device): an outgrown buffer is kept until the worker goes; growth is geometric, so that is at most as much again --
// nothing next to 288 GB.  (Measured: no difference to freeing at once; the stalls under load came from pageable copies,
// see PinnedArena.  SC_DEVBUF_KEEP=0 restores the old behaviour: `keep`, for the whole process, set by the contexts.)
struct DevBuf {
    static inline bool keep = true;
    void* p = nullptr; size_t cap = 0;
    std::vector<void*> outgrown;
    void* ensure(size_t n) {
        if (n > cap) {
            if (p) { if (keep) outgrown.push_back(p); else (void)hipFree(p); }
            size_t want = keep ? std::max<size_t>(n + n / 2 + 4096, 2 * cap) : n + n / 4 + 256;
            HIPCHK(hipMalloc(&p, want));
            cap = want; device_allocs++;
        }
        return p;
    }
    ~DevBuf() { if (p) (void)hipFree(p); for (void* q : outgrown) (void)hipFree(q); }
};
// A DevBuf of T: ensure(n) is room for n elements (null while nothing was ever asked for), get() the array as it stands.
template <class T> struct DevArr {
    DevBuf b;
    T* ensure(size_t n) { return (T*)b.ensure(n * sizeof(T)); }
    T* get() const { return (T*)b.p; }
};
// Pinned staging for a region's transfers.  A copy between the device and ordinary (pageable) host memory makes the
// runtime pin those pages for the copy and let them go afterwards; with regions in flight that costs far more than the
// copy -- registering and releasing user pages suspends every queue of the process (level kernels of ALL regions lasting
// ~30 ms at once, a few times per region).  So every sizeable transfer goes through page-locked memory the worker owns:
// grow-only chunks, handed out by a bump pointer, reused by the next region.
struct PinnedArena {
    struct Chunk { char* p; size_t cap, used; };
    struct Back { void* dst; const void* src; size_t n; };      // device-to-host copies still to be moved to their vectors
    std::vector<Chunk> chunks;
    std::vector<Back> back;
    bool on = true;                   // false: pass the copies through (a single region in flight suspends nobody)
    void* take(size_t n) {
        n = (n + 255) & ~(size_t)255;
        for (Chunk& c : chunks) if (c.cap - c.used >= n) { void* r = c.p + c.used; c.used += n; return r; }
        size_t cap = std::max<size_t>(n, (size_t)8 << 20);
        if (!chunks.empty()) cap = std::max(cap, 2 * chunks.back().cap);
        char* q = nullptr;
        HIPCHK(hipHostMalloc((void**)&q, cap, hipHostMallocDefault));
        chunks.push_back(Chunk{q, cap, n});
        return q;
    }
    void reset() { for (Chunk& c : chunks) c.used = 0; back.clear(); }
    void h2d(void* dst, const void* src, size_t n, hipStream_t st) {
        if (n == 0) return;
        if (!on) { HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st)); return; }
        void* q = take(n);
        memcpy(q, src, n);
        HIPCHK(hipMemcpyAsync(dst, q, n, hipMemcpyHostToDevice, st));
    }
    void d2h(void* dst, const void* src, size_t n, hipStream_t st) {          // complete after the stream's synchronisation + land()
        if (n == 0) return;
        if (!on) { HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st)); return; }
        void* q = take(n);
        HIPCHK(hipMemcpyAsync(q, src, n, hipMemcpyDeviceToHost, st));
        back.push_back(Back{dst, q, n});
    }
    void land() { for (const Back& b : back) memcpy(b.dst, b.src, b.n); back.clear(); }
    ~PinnedArena() { for (Chunk& c : chunks) (void)hipHostFree(c.p); }
};
template <class T> T* upload(PinnedArena& ar, DevBuf& b, const std::vector<T>& v, hipStream_t st) {
    T* d = (T*)b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T));
    ar.h2d(d, v.data(), v.size() * sizeof(T), st);
    return d;
}

// Owned HIP resources of a context: acquired by the constructor (HipError when that fails), released by the destructor.
struct Stream {
    hipStream_t st = nullptr;
    Stream() { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
    explicit Stream(int priority) { HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority)); }
    Stream(Stream&& o) noexcept : st(o.st) { o.st = nullptr; }
    Stream(const Stream&) = delete;
    ~Stream() { if (st) (void)hipStreamDestroy(st); }
};
template <class T> struct HostMapped {                    // host memory the device reads and writes over PCIe: p there is d
    T* p = nullptr; T* d = nullptr;
    explicit HostMapped(size_t n) {
        HIPCHK(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent));
        if (hipHostGetDevicePointer((void**)&d, p, 0) != hipSuccess) { (void)hipHostFree(p); throw HipError("hipHostGetDevicePointer"); }
    }
    HostMapped(const HostMapped&) = delete;
    ~HostMapped() { (void)hipHostFree(p); }
};
template <class T> struct DevMem {                        // never null: an empty array is still a device address for a kernel
    T* p = nullptr;
    explicit DevMem(size_t n) { HIPCHK(hipMalloc((void**)&p, std::max<size_t>(n * sizeof(T), 16))); device_allocs++; }
    DevMem(const std::vector<T>& v) : DevMem(v.size()) {
        if (hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); throw HipError("hipMemcpy"); }
    }
    DevMem(const DevMem&) = delete;
    ~DevMem() { (void)hipFree(p); }
};
template <class T> struct PinMem {                        // page-locked host memory
    T* p = nullptr;
    explicit PinMem(size_t n) { HIPCHK(hipHostMalloc((void**)&p, std::max<size_t>(n * sizeof(T), 16), hipHostMallocDefault)); }
    PinMem(const PinMem&) = delete;
    ~PinMem() { (void)hipHostFree(p); }
};
// A stream of one call with the events that time its phases: mark(name) records one where the stream stands, ms(a, b) is
// the device time between two of them once the stream was synchronised.  A phase that recurs is a span: span(name, body)
// records an event before and after what body enqueues, as often as it is called, and span_ms(name) is the sum of the
// device times of that name's pairs.  Copies of no bytes are left out.
struct TimedStream {
    Stream s;
    std::vector<std::pair<const char*, hipEvent_t>> marks;      // the marks of a span's name alternate: begin, end
    ~TimedStream() { for (auto& m : marks) (void)hipEventDestroy(m.second); }
    operator hipStream_t() const { return s.st; }
    void mark(const char* name) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        marks.emplace_back(name, e);
        HIPCHK(hipEventRecord(e, s.st));
    }
    float ms(const char* a, const char* b) const { return elapsed(event(a), event(b)); }
    template <class F> void span(const char* name, F&& body) {
        mark(name);
        body();
        mark(name);
    }
    double span_ms(const char* name) const {
        double t = 0;
        hipEvent_t begin = nullptr;
        for (auto& m : marks) {
            if (strcmp(m.first, name)) continue;
            if (begin) t += elapsed(begin, m.second);
            begin = begin ? nullptr : m.second;
        }
        return t;
    }
    void h2d(void* dst, const void* src, size_t n) { if (n) HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s.st)); }
    void d2h(void* dst, const void* src, size_t n) { if (n) HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s.st)); }
    template <class T> void h2d(DevMem<T>& d, const std::vector<T>& v) { h2d(d.p, v.data(), v.size() * sizeof(T)); }
    template <class T> void d2h(std::vector<T>& v, const DevMem<T>& d) { d2h(v.data(), d.p, v.size() * sizeof(T)); }
    void zero(void* dst, size_t n) { HIPCHK(hipMemsetAsync(dst, 0, n, s.st)); }
    void launched() { HIPCHK(hipGetLastError()); }
    void sync() { HIPCHK(hipStreamSynchronize(s.st)); }

private:
    static float elapsed(hipEvent_t a, hipEvent_t b) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, a, b));
        return t;
    }
    hipEvent_t event(const char* name) const {
        for (auto& m : marks) if (!strcmp(m.first, name)) return m.second;
        throw HipError(std::string("no mark ") + name);
    }
};

}  // namespace sc
