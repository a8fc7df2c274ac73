// The two CIGAR readings of the ingest and the window crop.  No HIP, no other project header: a plain C++ compiler and a
// host sanitizer take it (tests/native/ingest_check.cpp).  The graph stage's parse_cigar (sc_graph.cpp) is a third reading
// on purpose: it ignores stray characters where the rule here fails on them, and sc_roi_submit reaches it directly.
#pragma once
#include <algorithm>
#include <vector>

namespace sc_ingest {

// std::stoi on a field: leading blanks, sign, digits; anything after is ignored; no digits = error
inline bool lead_int(const char* s, int n, int& out) {
    int i = 0;
    while (i < n && (s[i] == ' ' || s[i] == '\t')) i++;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    if (i >= n || s[i] < '0' || s[i] > '9') return false;
    long v = 0;
    while (i < n && s[i] >= '0' && s[i] <= '9') { v = v * 10 + (s[i] - '0'); if (v > 0x7fffffffL) return false; i++; }
    out = (int)(neg ? -v : v);
    return true;
}

struct Op { char op; int len; };
// The reference's rule, PartialOrderGraph.cpp:13-59: a number, then one of MIDNSHP (kept) or = X (become M); other
// characters join the number
inline bool parse_cigar(const char* c, int n, std::vector<Op>& out) {
    out.clear();
    int start = 0;
    for (int i = 0; i < n; i++) {
        const char ch = c[i];
        const bool plain = ch == 'M' || ch == 'I' || ch == 'D' || ch == 'N' || ch == 'S' || ch == 'H' || ch == 'P';
        if (plain || ch == '=' || ch == 'X') {
            int len;
            if (!lead_int(c + start, i - start, len)) return false;
            out.push_back({plain ? ch : 'M', len});
            start = i + 1;
        }
    }
    return true;
}

// samtools' rule: digits, then any other character as the operation; fn(op, len) with len a long
template <class F>
inline void for_each_op(const char* c, int n, const F& fn) {
    long v = 0;
    for (int i = 0; i < n; i++) {
        const char ch = c[i];
        if (ch >= '0' && ch <= '9') { v = v * 10 + (ch - '0'); continue; }
        fn(ch, v);
        v = 0;
    }
}
inline int ref_span_end(int pos, const char* c, int n) {      // samtools' notion: M D N = X consume the reference
    long tot = 0;
    for_each_op(c, n, [&](char op, long len) { if (op == 'M' || op == 'D' || op == 'N' || op == '=' || op == 'X') tot += len; });
    return pos + (int)(tot > 1 ? tot : 1) - 1;
}

// The front of a read that starts before the window, the back of one that ends after it, and soft clips are cut
// away; what is left is the read inside the window (crop_read_within_window, StrainCall.cpp:291-414).  A reference
// coordinate map of the operations decides: M and D operations are clipped to the window position by position, an
// insertion lying before the first / after the last kept reference position goes with its bases, operations that
// consume neither (H, P) or that the reference does not know to consume the reference (N) stay as they are.
struct Cropped { int lead = 0, trail = 0; std::vector<Op> ops; bool ok = true; };
inline void crop_to_window(int w0, int w1, const std::vector<Op>& ops, int r0, int r1, Cropped& out) {
    out.lead = out.trail = 0; out.ops.clear(); out.ok = true;
    const int n = (int)ops.size();
    if (n == 0) { out.ok = false; return; }
    int first = 0;
    if (ops[0].op == 'S') { out.lead = ops[0].len; first = 1; }
    if (first >= n) { out.ok = false; return; }
    // ---- front: walk the reference cursor up to the window start
    int k = first;
    if (r0 < w0 && r0 < w1) {
        int cur = r0, used_last = 0;
        Op last{0, 0};
        while (cur < w0 && cur < w1) {
            if (k >= n) { out.ok = false; return; }            // the read never reaches the window (the reference reads past its vector here)
            const Op o = ops[k++];
            int used = 0;
            if (o.op == 'M' || o.op == 'D') {
                used = std::max(0, std::min(o.len, w0 - cur));
                cur += used;
                if (o.op == 'M') out.lead += used;
            } else if (o.op == 'I') {
                out.lead += o.len;                               // an insertion in front of the window leaves with its bases
            }
            last = o; used_last = used;
        }
        if (used_last < last.len) out.ops.push_back(Op{last.op, last.len - used_last});      // the operation the window starts in
    } else {
        if (ops[k].len > 0) out.ops.push_back(ops[k]);
        k++;
    }
    for (; k < n; k++) out.ops.push_back(ops[k]);
    // ---- back: the same from the other end, on the operations still held
    int last = n - 1;
    if (ops[last].op == 'S') {
        out.trail = ops[last].len;
        last--;
        if (out.ops.empty()) { out.ok = false; return; }
        out.ops.pop_back();
    }
    int cur = r1;
    while (cur > w1 && cur > w0) {
        if (last < 0 || out.ops.empty()) { out.ok = false; return; }
        const Op o = ops[last--];
        int used = 0;
        if (o.op == 'M' || o.op == 'D') {
            used = std::min(o.len, cur - w1);
            if (used < 0) used = 0;
            cur -= used;
            if (o.op == 'M') out.trail += used;
        } else if (o.op == 'I') {
            out.trail += o.len;
        }
        if (used == o.len || o.op == 'I') out.ops.pop_back();
        else out.ops.back().len -= used;
    }
}

}  // namespace sc_ingest
