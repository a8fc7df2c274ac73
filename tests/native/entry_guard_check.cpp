// Stand-alone driver of rambl_amd/csrc/sc_error.hpp, the guard every entry point of the library returns through: no HIP, no
// public header, no library -- that this file compiles from sc_error.hpp alone is part of the check.
// stdout: one line per case, `NAME<TAB>CODE<TAB>TEXT` (TEXT as sc_*_error() would hand it out; `-` for a null error slot);
// tests/test_entry_guard_host.py holds the table they must equal.
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <new>
#include <thread>

#include "../../rambl_amd/csrc/sc_error.hpp"

static const int OK = 0, CAPACITY = -5;          // SC_OK, SC_ERR_CAPACITY: any code that is neither ERR_HIP nor ERR_INTERNAL

// One failure of every kind the guard tells apart, by name; `pass` and `code` return without throwing.
static int body(const std::string& kind, sc::LastError* err) {
    if (kind == "pass") { if (err) err->text = "left by the body"; return OK; }
    if (kind == "code") { return err ? err->fail(CAPACITY, "sc_x: 7 hits, room for 3") : CAPACITY; }
    if (kind == "sc") throw sc::ScError(CAPACITY, "x");
    if (kind == "hip") throw sc::HipError("hipMalloc(&p, n): out of memory");
    if (kind == "bad_alloc") throw std::bad_alloc();
    if (kind == "length") throw std::length_error("y");
    throw 7;
}

static void line(const std::string& name, int rc, const sc::LastError* err) { printf("%s\t%d\t%s\n", name.c_str(), rc, err ? err->text.c_str() : "-"); }

static thread_local sc::LastError tl_error;

int main() {
    auto nothing = [] { return 0; };
    static_assert(noexcept(sc::guarded(nullptr, "", nothing)), "the guard promises to let nothing out");
    const char* kinds[] = {"pass", "code", "sc", "hip", "bad_alloc", "length", "int"};
    for (const char* k : kinds) {
        sc::LastError err;
        err.text = "stale";
        line(k, sc::guarded(&err, "sc_x", [&] { return body(k, &err); }), &err);
    }
    for (const char* k : kinds) line(std::string("null ") + k, sc::guarded(nullptr, "sc_x", [&] { return body(k, nullptr); }), nullptr);

    // a family's slot is thread_local: both threads have failed before either reads its message back
    std::mutex mu;
    std::condition_variable cv;
    int failed = 0;
    std::string seen[2];
    int codes[2] = {0, 0};
    auto work = [&](int t) {
        tl_error.clear();
        codes[t] = sc::guarded(&tl_error, "sc_x", [&]() -> int { throw sc::ScError(CAPACITY - t, "message of thread " + std::to_string(t)); });
        std::unique_lock<std::mutex> lk(mu);
        failed++;
        cv.notify_all();
        cv.wait(lk, [&] { return failed == 2; });
        seen[t] = tl_error.text;
    };
    std::thread a(work, 0), b(work, 1);
    a.join(); b.join();
    for (int t = 0; t < 2; t++) printf("thread %d\t%d\t%s\n", t, codes[t], seen[t].c_str());
    line("main after threads", OK, &tl_error);

    tl_error.fail(CAPACITY, "an earlier failure");
    tl_error.clear();
    line("clear then pass", sc::guarded(&tl_error, "sc_x", [] { return OK; }), &tl_error);
    return 0;
}
