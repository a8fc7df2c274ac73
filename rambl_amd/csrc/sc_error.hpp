// How a failure inside libstraincall_hip.so becomes an SC_* code and a message at the C boundary: the two errors the code
// throws, a family's last message on the calling thread, and the one guard every entry point returns through (DESIGN.md
// §1, "The boundary on the C++ side").  No HIP and no public header here: the stand-alone check tests/native/entry_guard_check.cpp includes this alone.
#pragma once
#include <stdexcept>
#include <string>

namespace sc {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ScError : std::runtime_error {
    int code;
    ScError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// SC_ERR_HIP and SC_ERR_INTERNAL of include/straincall_hip.h (sc_host.hpp, which sees both, asserts that they are)
enum : int { ERR_HIP = -2, ERR_INTERNAL = -6 };

// The last error of a family's entry points on this thread: one `thread_local` per exported sc_*_error().
struct LastError {
    std::string text;
    int fail(int rc, const std::string& msg) { text = msg; return rc; }
    void clear() { text.clear(); }
};

// Runs body() (which returns an SC_* code) and lets nothing out: the one place that maps an exception to a code and a message.
//   ScError               its own code, the message as thrown
//   HipError              SC_ERR_HIP,      "<fn>: a HIP call failed: <what>"
//   other std::exception  SC_ERR_INTERNAL, "<fn>: <what>"
//   anything else         SC_ERR_INTERNAL, "<fn>: unknown exception"
// A null `err`: the code alone.  So it is when there is no memory left for the message.
template <class F> int guarded(LastError* err, const char* fn, F&& body) noexcept {
    int rc = ERR_INTERNAL;
    try {
        std::string msg;
        try { return body(); }
        catch (const ScError& e) { rc = e.code; msg = e.what(); }
        catch (const HipError& e) { rc = ERR_HIP; msg = std::string(fn) + ": a HIP call failed: " + e.what(); }
        catch (const std::exception& e) { msg = std::string(fn) + ": " + e.what(); }
        catch (...) { msg = std::string(fn) + ": unknown exception"; }
        if (err) err->text.swap(msg);
    } catch (...) {}
    return rc;
}

}  // namespace sc
