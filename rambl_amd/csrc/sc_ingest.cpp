// Native read ingest of the StrainCall path, the region side, host code of libstraincall_hip.so.
//
// Replaces the text that crosses the reference's samtools boundary and what it does with it:
//   samtools view <aln> -q mq -F 1804 gene:p0-p1     /root/reference/StrainCall/StrainCall.cpp:496
//   samtools mpileup -q mq -Q0 -A -r gene:P-Q <aln>  :696 (only "is there a '+' / a '-' or '*' in column 5" is read, :712-735)
//   load_mapping_reads                               :480-670  (depth -> rho, filters, crop to the window,
//                                                     mt19937(1234) thinning, exact-duplicate collapse, mate table)
// The alignment file is read once and indexed by reference name (sc_aln_file.cpp); a region's reads come back as the
// packed arrays sc_roi_submit takes, so the caller hands them on without touching a read.  Nothing here uses the GPU.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/straincall_hip.h"
#include "sc_cigar.hpp"
#include "sc_ingest.hpp"
#include "sc_plan.hpp"       // Mt19937

thread_local sc::LastError sc_ingest::tl_error;

struct sc_reads {
    std::vector<int> pos, cigar_off, seq_off, copies, mate_idx, mate_off;
    std::string cigar_text, seq_text;
    long n_input = 0;
    int depth = 0;
};

namespace {
using namespace sc_ingest;
struct SortPlan { int nt; size_t min_stretch; };       // threads of a sort, and the elements worth one

// ---- samtools view -q mq -F 1804 gene:p0-p1
std::vector<const Rec*> view_region(const sc_aln& a, const char* gene, int p0, int p1, int mq) {
    std::vector<const Rec*> view;
    auto it = a.by_ref.find(gene);
    if (it != a.by_ref.end())
        for (const Rec& r : it->second) {
            if ((r.flag & 1804) || r.mapq < mq || r.ref_end < p0 || r.pos > p1) continue;      // -F, -q, no overlap
            view.push_back(&r);
        }
    return view;
}

// reference positions of the M and D operations: what read_align_end_pos adds up (StrainCall.cpp:276-289)
int md_span(const std::vector<Op>& ops) { int n = 0; for (const Op& o : ops) if (o.op == 'M' || o.op == 'D') n += o.len; return n; }

// ---- depth over the window, which gives the keep probability (StrainCall.cpp:503-529); false: a malformed CIGAR
bool window_depth(const std::vector<const Rec*>& view, int p0, int p1, int& depth) {
    std::vector<Op> ops;
    depth = 0;
    for (const Rec* r : view) {
        if (!parse_cigar(r->cigar, r->clen, ops)) { tl_error.text = "malformed CIGAR"; return false; }
        const int r0 = r->pos, r1 = r0 + md_span(ops) - 1;
        if (p0 <= r0 && p1 > r1) depth += r1 - r0 + 1;
        else if (p0 <= r0 && p1 <= r1) depth += p1 - r0 + 1;
        else if (p0 > r0 && p1 <= r1) depth += p1 - p0 + 1;
        else if (p0 > r0 && p1 > r1) depth += r1 - p0 + 1;
    }
    depth /= (p1 - p0 + 1);
    return true;
}

// ---- filters (length, N, insertions), crop, thinning (:531-592); false: a read that cannot be cropped
bool keep_reads(const std::vector<const Rec*>& view, int p0, int p1, int rl, int max_ins, double rho, std::vector<Kept>& kept,
                std::string& cig_pool) {
    sc::Mt19937 gen(1234u);
    std::vector<Op> ops;
    Cropped cr;
    for (const Rec* r : view) {
        if ((size_t)r->slen < (size_t)(long)rl) continue;                      // f10.length() < rl (rl widened like the reference's)
        if (memchr(r->seq, 'N', (size_t)r->slen) || memchr(r->seq, 'n', (size_t)r->slen)) continue;
        const char suffix = (r->flag & 65) == 65 ? '1' : (r->flag & 129) == 129 ? '2' : 0;
        parse_cigar(r->cigar, r->clen, ops);
        const int rp0 = r->pos, rp1 = rp0 + md_span(ops) - 1;
        crop_to_window(p0, p1, ops, rp0, rp1, cr);
        if (!cr.ok || cr.lead > r->slen || cr.trail > r->quallen) {
            tl_error.text = "a read cannot be cropped to the window (soft clips / CIGAR longer than its bases)";
            return false;
        }
        const int cnt = r->slen - cr.lead - cr.trail;
        const int seq_len = cnt < 0 ? r->slen - cr.lead : cnt;                  // substr(i, npos-like count)
        int maxins = 0;
        for (const Op& o : cr.ops) if (o.op == 'I' && o.len > maxins) maxins = o.len;
        if (!((size_t)seq_len > (size_t)(long)rl && maxins < max_ins)) continue;
        if (gen.canonical() > rho) continue;                                    // drawn only for reads that passed
        Kept kp;
        kp.relpos = std::max(rp0 - p0, 0);
        kp.cig_off = (uint32_t)cig_pool.size();
        for (const Op& o : cr.ops) { cig_pool += std::to_string(o.len); cig_pool.push_back(o.op); }
        kp.cig_len = (uint32_t)cig_pool.size() - kp.cig_off;
        kp.seq = r->seq + cr.lead; kp.seq_len = seq_len;
        kp.name = r->qname; kp.name_len = r->qlen; kp.suffix = suffix;
        kept.push_back(kp);
    }
    return true;
}

// ---- exact duplicates collapse; unique reads in (position, CIGAR text, bases) order (std::map<AlignRead,...>, :594-627).
// `order`: the kept reads in that order, input order among equals; uid_of[i]: the unique read of kept[i]
void collapse_duplicates(const std::vector<Kept>& kept, const std::string& cig_pool, SortPlan sp, sc_reads& R, std::vector<uint32_t>& order,
                         std::vector<int>& uid_of) {
    const size_t nk = kept.size();
    const Cmp3 cmp3{cig_pool.data()};
    order.resize(nk);
    std::iota(order.begin(), order.end(), 0u);
    stable_sort_mt(order, [&](uint32_t i, uint32_t j) { return cmp3(kept[i], kept[j]) < 0; }, sp.nt, sp.min_stretch);
    uid_of.resize(nk);
    for (size_t k = 0; k < nk; k++) {
        const Kept& cur = kept[order[k]];
        if (k == 0 || cmp3(kept[order[k - 1]], cur) != 0) {
            R.pos.push_back(cur.relpos);
            R.cigar_off.push_back((int)R.cigar_text.size());
            R.cigar_text.append(cig_pool.data() + cur.cig_off, cur.cig_len);
            R.seq_off.push_back((int)R.seq_text.size());
            R.seq_text.append(cur.seq, (size_t)cur.seq_len);
            R.copies.push_back(0);
        }
        R.copies.back()++;
        uid_of[order[k]] = (int)R.pos.size() - 1;
    }
    R.cigar_off.push_back((int)R.cigar_text.size());
    R.seq_off.push_back((int)R.seq_text.size());
}

// ---- mates (:630-665): names in byte order; a name met again keeps its last unique read (the last in `order`: unique-read
// order, then input order); mate = the same name with the other /1 /2 ending
void mate_table(const std::vector<Kept>& kept, const std::vector<uint32_t>& order, const std::vector<int>& uid_of, SortPlan sp, sc_reads& R) {
    const size_t nk = kept.size();
    auto at = [&](uint32_t pos_in_order) -> const Kept& { return kept[order[pos_in_order]]; };
    std::vector<uint32_t> by_name(nk);          // positions in `order`
    std::iota(by_name.begin(), by_name.end(), 0u);
    stable_sort_mt(by_name, [&](uint32_t i, uint32_t j) { return name_cmp(at(i), at(j)) < 0; }, sp.nt, sp.min_stretch);
    std::vector<uint32_t> names;                // positions in `order`, one per distinct name (the last assignment)
    for (size_t k = 0; k < nk; k++)
        if (k + 1 == nk || name_cmp(at(by_name[k]), at(by_name[k + 1])) != 0) names.push_back(by_name[k]);
    std::vector<std::vector<int>> mates(R.pos.size());
    for (uint32_t pos_in_order : names) {
        const Kept& kp = at(pos_in_order);
        // paired: the suffixed name ends in "/1" or "/2" -- by the flag, or because the read name itself does
        char ending = kp.suffix;
        int base_len = kp.name_len;
        if (!ending && kp.name_len >= 2 && kp.name[kp.name_len - 2] == '/' && (kp.name[kp.name_len - 1] == '1' || kp.name[kp.name_len - 1] == '2')) {
            ending = kp.name[kp.name_len - 1];
            base_len = kp.name_len - 2;
        }
        int mate = -1;
        if (ending == '1' || ending == '2') {
            // binary search for base + "/" + other among the distinct names
            Kept probe = kp;
            std::string pn;
            if (kp.suffix) { probe.suffix = ending == '1' ? '2' : '1'; }
            else { pn.assign(kp.name, (size_t)base_len); pn += '/'; pn += (ending == '1' ? '2' : '1'); probe.name = pn.data(); probe.name_len = (int)pn.size(); probe.suffix = 0; }
            size_t lo = 0, hi = names.size();
            while (lo < hi) {
                const size_t mid = (lo + hi) / 2;
                if (name_cmp(at(names[mid]), probe) < 0) lo = mid + 1; else hi = mid;
            }
            if (lo < names.size() && name_cmp(at(names[lo]), probe) == 0) mate = uid_of[order[names[lo]]];
        }
        mates[(size_t)uid_of[order[pos_in_order]]].push_back(mate);
    }
    R.mate_off.push_back(0);
    for (const std::vector<int>& ms : mates) {
        R.mate_idx.insert(R.mate_idx.end(), ms.begin(), ms.end());
        R.mate_off.push_back((int)R.mate_idx.size());
    }
}

}  // namespace

extern "C" {

const char* sc_aln_error(sc_aln* a) {
    if (!tl_error.text.empty()) return tl_error.text.c_str();
    return a ? a->error.c_str() : "";
}

int sc_aln_pileup_flags(sc_aln* a, const char* gene, int P, int Q, int mq, unsigned char* covered, unsigned char* has_ins,
                        unsigned char* has_del) {
    if (!a || !gene || Q < P || !covered || !has_ins || !has_del) return SC_ERR_ARG;
    return sc::guarded(&tl_error, "sc_aln_pileup_flags", [&] {
        const int n = Q - P + 1;
        std::vector<int> diff((size_t)n + 1, 0);
        memset(has_ins, 0, (size_t)n); memset(has_del, 0, (size_t)n);
        auto it = a->by_ref.find(gene);
        if (it != a->by_ref.end()) {
            auto mark = [&](unsigned char* arr, int p) { if (p >= P && p <= Q) arr[p - P] = 1; };
            // [p, p + ln) counts towards the coverage; the part of it inside the window as lo..hi (empty: lo > hi)
            auto cover = [&](int p, int ln, int& lo, int& hi) {
                lo = std::max(p, P); hi = std::min(p + ln - 1, Q);
                if (lo <= hi) { diff[(size_t)(lo - P)]++; diff[(size_t)(hi - P + 1)]--; }
            };
            std::vector<Op> ops;
            for (const Rec& r : it->second) {
                if ((r.flag & 1796) || r.mapq < mq) continue;
                if (r.ref_end < P || r.pos > Q) continue;
                // samtools' own CIGAR reading here (= X distinct from M does not matter: all three align bases)
                ops.clear();
                for_each_op(r.cigar, r.clen, [&](char op, long len) { if (op != 'H' && op != 'P') ops.push_back({op, (int)len}); });
                const int mq_char = 33 + std::min(r.mapq, 93);
                int p = r.pos, lo, hi;
                bool first = true;
                for (size_t k = 0; k < ops.size(); k++) {
                    const char op = ops[k].op; const int ln = ops[k].len;
                    if (op == 'M' || op == '=' || op == 'X') {
                        cover(p, ln, lo, hi);
                        if (first) {
                            // '^' + the mapping quality character in front of the first base: '+', '-' and '*' read as indel marks
                            if (mq_char == '+') mark(has_ins, p);
                            else if (mq_char == '-' || mq_char == '*') mark(has_del, p);
                            first = false;
                        }
                        if (k + 1 < ops.size()) {
                            if (ops[k + 1].op == 'I') mark(has_ins, p + ln - 1);
                            else if (ops[k + 1].op == 'D') mark(has_del, p + ln - 1);
                        }
                        p += ln;
                    } else if (op == 'D' || op == 'N') {
                        // a deleted base prints '*' (read as a deletion mark, StrainCall.cpp:712-735); a reference skip (N)
                        // prints '>' or '<', which window_adjust does not look for: it only counts towards the coverage
                        cover(p, ln, lo, hi);
                        if (op == 'D' && lo <= hi) memset(has_del + (lo - P), 1, (size_t)(hi - lo + 1));
                        p += ln;
                    }
                }
            }
        }
        int depth = 0;
        for (int i = 0; i < n; i++) {
            depth += diff[(size_t)i];
            covered[i] = depth > 0;
            if (!covered[i]) { has_ins[i] = 0; has_del[i] = 0; }
        }
        return SC_OK;
    });
}

int sc_aln_load_reads(sc_aln* a, const char* gene, int p0, int p1, int mq, int rl, int max_ins, int max_depth, sc_reads** out) {
    if (!a || !gene || !out) return SC_ERR_ARG;
    *out = nullptr;
    tl_error.clear();
    return sc::guarded(&tl_error, "sc_aln_load_reads", [&] {
        std::unique_ptr<sc_reads> R(new sc_reads());
        const std::vector<const Rec*> view = view_region(*a, gene, p0, p1, mq);
        R->n_input = (long)view.size();
        if (!window_depth(view, p0, p1, R->depth)) return SC_ERR_ARG;
        const double rho = std::min(1.0, (double)max_depth / ((double)R->depth + 0.0));
        std::vector<Kept> kept;
        std::string cig_pool;
        if (!keep_reads(view, p0, p1, rl, max_ins, rho, kept, cig_pool)) return SC_ERR_ARG;
        // the two sorts run on the rank's ingest threads; SC_INGEST_SORT_MIN: elements worth a thread (tests lower it to reach the merges)
        const char* e = getenv("SC_INGEST_SORT_MIN");
        const SortPlan sp{std::min(sc::ingest_threads(), 16), (size_t)std::max(e ? atol(e) : 65536L, 2L)};
        std::vector<uint32_t> order;
        std::vector<int> uid_of;
        collapse_duplicates(kept, cig_pool, sp, *R, order, uid_of);
        mate_table(kept, order, uid_of, sp, *R);
        *out = R.release();
        return SC_OK;
    });
}

int sc_reads_get(sc_reads* r, int* n_reads, const int** pos, const char** cigar_text, const int** cigar_off, const char** seq_text,
                 const int** seq_off, const int** copies, const int** mate_idx, const int** mate_off, long* n_input, int* depth) {
    if (!r) return SC_ERR_ARG;
    static const int none = 0;
    if (n_reads) *n_reads = (int)r->pos.size();
    if (pos) *pos = r->pos.empty() ? &none : r->pos.data();
    if (cigar_text) *cigar_text = r->cigar_text.c_str();
    if (cigar_off) *cigar_off = r->cigar_off.data();
    if (seq_text) *seq_text = r->seq_text.c_str();
    if (seq_off) *seq_off = r->seq_off.data();
    if (copies) *copies = r->copies.empty() ? &none : r->copies.data();
    if (mate_idx) *mate_idx = r->mate_idx.empty() ? &none : r->mate_idx.data();
    if (mate_off) *mate_off = r->mate_off.data();
    if (n_input) *n_input = r->n_input;
    if (depth) *depth = r->depth;
    return SC_OK;
}

void sc_reads_free(sc_reads* r) { delete r; }

}  // extern "C"
