// Native read ingest of the StrainCall path, the file side: the alignment file (SAM text, or BAM = BGZF-compressed
// records, SAM specification section 4) is read once and indexed by reference name.  What a region's reads become is in
// sc_ingest.cpp.  Nothing here uses the GPU.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/straincall_hip.h"
#include "sc_cigar.hpp"
#include "sc_ingest.hpp"

namespace {
using namespace sc_ingest;

// One stretch of the text (whole lines): the records of the references this handle keeps, per reference in file order,
// and the statistics of every reference.
struct SamPart {
    std::vector<std::pair<std::string, std::vector<Rec>>> buckets;      // in order of first appearance
    std::unordered_map<std::string, size_t> index;
    std::unordered_map<std::string, sc_aln::RefStat> stats;
    long n_records = 0;
    std::string error;
};
void parse_sam_part(const sc_aln& a, const char* p, const char* end, SamPart& out) {      // out.error: a record that cannot be read
    std::string last_name;
    std::vector<Rec>* bucket = nullptr;
    sc_aln::RefStat* stat = nullptr;
    bool wanted = false;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        const char* next = nl ? nl + 1 : end;
        if (le > p && le[-1] == '\r') le--;
        if (le > p && *p != '@') {
            const char* f[12];
            int nf = 0;
            f[0] = p;
            for (const char* q = p; q < le && nf < 11; q++)
                if (*q == '\t') f[++nf] = q + 1;
            // f[k] = start of field k; field k ends one before f[k+1] (or at the end of the line for the last one found)
            if (nf >= 10) {
                auto fend = [&](int k) { return k < nf ? f[k + 1] - 1 : le; };
                Rec r{};
                r.qname = f[0]; r.qlen = (int)(fend(0) - f[0]);
                bool ok = lead_int(f[1], (int)(fend(1) - f[1]), r.flag) && lead_int(f[3], (int)(fend(3) - f[3]), r.pos) &&
                          lead_int(f[4], (int)(fend(4) - f[4]), r.mapq);
                if (!ok) { out.error = "SAM record with a non-numeric FLAG, POS or MAPQ"; return; }
                r.cigar = f[5]; r.clen = (int)(fend(5) - f[5]);
                r.seq = f[9]; r.slen = (int)(fend(9) - f[9]);
                r.qual = f[10]; r.quallen = (int)(fend(10) - f[10]);
                r.ord = (long)(p - (const char*)a.map);
                r.ref_end = ref_span_end(r.pos, r.cigar, r.clen);
                const size_t rl = (size_t)(fend(2) - f[2]);
                if (!stat || last_name.size() != rl || memcmp(last_name.data(), f[2], rl) != 0) {
                    last_name.assign(f[2], rl);
                    stat = &out.stats[last_name];
                    wanted = a.wants(f[2], rl);
                    bucket = nullptr;
                    if (wanted) {
                        auto it = out.index.find(last_name);
                        if (it == out.index.end()) { it = out.index.emplace(last_name, out.buckets.size()).first; out.buckets.emplace_back(last_name, std::vector<Rec>()); }
                        bucket = &out.buckets[it->second].second;
                    }
                }
                stat->add((long)(r.ref_end - r.pos + 1));
                if (wanted) bucket->push_back(r);
                out.n_records++;
            }
        }
        p = next;
    }
}
// The text is cut at line ends into as many stretches as this rank has host threads; the stretches are parsed side by
// side and joined in file order (a reference's records keep the order of the file).
bool load_sam_text(sc_aln& a, const char* text, size_t len) {
    int nt = sc::ingest_threads();
    size_t min_chunk = (size_t)1 << 20;                                   // a stretch below this is not worth a thread
    if (const char* e = getenv("SC_INGEST_MIN_CHUNK")) min_chunk = (size_t)std::max(atol(e), 64L);
    nt = (int)std::max<size_t>(std::min<size_t>((size_t)nt, len / min_chunk), 1);
    std::vector<const char*> cut((size_t)nt + 1, text + len);
    cut[0] = text;
    for (int k = 1; k < nt; k++) {
        const char* q = text + len / (size_t)nt * (size_t)k;
        if (q < cut[(size_t)k - 1]) q = cut[(size_t)k - 1];
        const char* nl = (const char*)memchr(q, '\n', (size_t)(text + len - q));
        cut[(size_t)k] = nl ? nl + 1 : text + len;
    }
    std::vector<SamPart> parts((size_t)nt);
    sc::parallel_items(nt, nt, [&](int k) { parse_sam_part(a, cut[(size_t)k], cut[(size_t)k + 1], parts[(size_t)k]); });
    for (int k = 0; k < nt; k++) {
        if (!parts[(size_t)k].error.empty()) { a.error = parts[(size_t)k].error; return false; }
        for (auto& b : parts[(size_t)k].buckets) {
            std::vector<Rec>& dst = a.by_ref[b.first];
            if (dst.empty()) dst.swap(b.second); else dst.insert(dst.end(), b.second.begin(), b.second.end());
        }
        for (auto& st : parts[(size_t)k].stats) { sc_aln::RefStat& d = a.stats[st.first]; d.n += st.second.n; d.bases += st.second.bases; }
        a.n_records += parts[(size_t)k].n_records;
    }
    return true;
}

// BGZF: a series of gzip members, each with the BC extra field; the payload is raw deflate (SAM spec 4.1).
// The members are independent: one pass over the headers finds where each one's bytes go, then the host threads
// the process may use inflate them side by side.
bool inflate_bgzf(const unsigned char* src, size_t n, std::vector<unsigned char>& out, std::string& err) {
    struct Member { size_t cdata, clen, at; unsigned isize, crc; };
    std::vector<Member> members;
    size_t o = 0, total = 0;
    while (o + 18 <= n) {
        if (src[o] != 0x1f || src[o + 1] != 0x8b || src[o + 2] != 8 || !(src[o + 3] & 4)) { err = "not a BGZF block"; return false; }
        const unsigned xlen = src[o + 10] | (src[o + 11] << 8);
        size_t x = o + 12, xe = x + xlen;
        long bsize = -1;
        if (xe + 8 > n) { err = "truncated BGZF block"; return false; }
        while (x + 4 <= xe) {
            const unsigned slen = src[x + 2] | (src[x + 3] << 8);
            if (x + 4 + slen > xe) break;                                 // a subfield that runs past the extra field: not ours to read
            if (src[x] == 'B' && src[x + 1] == 'C' && slen == 2) bsize = (src[x + 4] | (src[x + 5] << 8)) + 1L;
            x += 4 + slen;
        }
        if (bsize < (long)xlen + 20 || o + (size_t)bsize > n) { err = "BGZF block without a BC field or truncated"; return false; }
        const unsigned isize = src[o + bsize - 4] | (src[o + bsize - 3] << 8) | (src[o + bsize - 2] << 16) | ((unsigned)src[o + bsize - 1] << 24);
        const unsigned crc = src[o + bsize - 8] | (src[o + bsize - 7] << 8) | (src[o + bsize - 6] << 16) | ((unsigned)src[o + bsize - 5] << 24);
        if (isize > 65536u) { err = "BGZF block claims more than 64 KiB of data"; return false; }      // SAM spec 4.1
        members.push_back(Member{o + 12 + xlen, (size_t)bsize - xlen - 20, total, isize, crc});
        total += isize;
        if (total > ((size_t)1 << 40) || members.size() >= 0x7fffffffu) { err = "BGZF file larger than this reader accepts"; return false; }
        o += (size_t)bsize;
    }
    out.resize(total);
    std::atomic<bool> bad{false};
    const int nt = (int)std::min<size_t>((size_t)sc::ingest_threads(), std::max<size_t>(members.size() / 4, 1));
    sc::parallel_items((int)members.size(), nt, [&](int k) {
        if (bad.load(std::memory_order_relaxed)) return;                  // one corrupt member: the rest are not inflated
        const Member& m = members[(size_t)k];
        if (!m.isize) { if (m.crc != 0u) bad = true; return; }
        z_stream zs{};
        if (inflateInit2(&zs, -15) != Z_OK) { bad = true; return; }
        zs.next_in = const_cast<unsigned char*>(src + m.cdata); zs.avail_in = (unsigned)m.clen;
        zs.next_out = out.data() + m.at; zs.avail_out = m.isize;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        if (rc != Z_STREAM_END || zs.avail_out != 0) { bad = true; return; }
        if ((unsigned)crc32(crc32(0L, Z_NULL, 0), out.data() + m.at, m.isize) != m.crc) bad = true;   // the member's CRC-32 of its data
    });
    if (bad) { err = "corrupt BGZF block (inflate or CRC-32)"; return false; }
    return true;
}

// One kept BAM record into strings of the handle's arena: the SAM fields the path reads, as text.  `d + o` is the record
// after block_size, already checked to lie inside the data; `span` its reference span.
Rec decode_bam_record(sc_aln& a, const unsigned char* d, size_t o, int span) {
    static const char SEQ[] = "=ACMGRSVTWYHKDBN", CIG[] = "MIDNSHP=X???????";
    int32_t pos, l_seq;
    memcpy(&pos, d + o + 4, 4); memcpy(&l_seq, d + o + 16, 4);
    const unsigned l_read_name = d[o + 8], n_cigar = d[o + 12] | (d[o + 13] << 8);
    size_t p = o + 32;
    Rec r{};
    r.qlen = l_read_name ? (int)l_read_name - 1 : 0;
    char* qn = a.alloc((size_t)r.qlen + 1);
    memcpy(qn, d + p, (size_t)r.qlen);
    r.qname = qn;
    p += l_read_name;
    std::string cig;
    for (unsigned k = 0; k < n_cigar; k++) {
        uint32_t c; memcpy(&c, d + p + 4ul * k, 4);
        cig += std::to_string(c >> 4);
        cig += CIG[c & 15];
    }
    if (cig.empty()) cig = "*";
    p += 4ul * n_cigar;
    char* cg = a.alloc(cig.size() + 1);
    memcpy(cg, cig.data(), cig.size());
    r.cigar = cg; r.clen = (int)cig.size();
    char* sq = a.alloc((size_t)std::max(l_seq, 1) + 1);
    for (int k = 0; k < l_seq; k++) { const unsigned b = d[p + (size_t)k / 2]; sq[k] = SEQ[(k & 1) ? (b & 15) : (b >> 4)]; }
    if (l_seq == 0) sq[0] = '*';
    r.seq = sq; r.slen = std::max(l_seq, 1);
    p += (size_t)(l_seq + 1) / 2;
    r.quallen = (l_seq == 0 || d[p] == 0xff) ? 1 : l_seq;            // "*" when absent
    char* ql = a.alloc((size_t)r.quallen + 1);
    if (r.quallen == 1 && (l_seq == 0 || d[p] == 0xff)) ql[0] = '*';
    else for (int k = 0; k < l_seq; k++) ql[k] = (char)(d[p + (size_t)k] + 33);
    r.qual = ql;
    r.ord = (long)o;
    r.flag = (int)(d[o + 14] | (d[o + 15] << 8)); r.pos = pos + 1; r.mapq = (int)d[o + 9];
    r.ref_end = r.pos + span - 1;
    return r;
}

bool load_bam(sc_aln& a, const unsigned char* src, size_t n) {
    std::vector<unsigned char> d;
    if (!inflate_bgzf(src, n, d, a.error)) return false;
    auto i32 = [&](size_t o) { int32_t v; memcpy(&v, d.data() + o, 4); return v; };
    if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0) { a.error = "not a BAM file"; return false; }
    size_t o = 8 + (size_t)i32(4);
    if (o + 4 > d.size()) { a.error = "truncated BAM header"; return false; }
    const int n_ref = i32(o);
    o += 4;
    std::vector<std::string> refs;
    for (int k = 0; k < n_ref; k++) {
        if (o + 4 > d.size()) { a.error = "truncated BAM header"; return false; }
        const int l_name = i32(o);
        o += 4;
        if (l_name < 1 || o + (size_t)l_name + 4 > d.size()) { a.error = "truncated BAM header"; return false; }
        refs.emplace_back((const char*)d.data() + o, (size_t)l_name - 1);
        o += (size_t)l_name + 4;
    }
    const std::string star("*");
    while (o + 4 <= d.size()) {
        // ---- bounds
        const int block = i32(o);
        o += 4;
        if (block < 32 || o + (size_t)block > d.size()) { a.error = "truncated BAM record"; return false; }
        const unsigned l_read_name = d[o + 8], n_cigar = d[o + 12] | (d[o + 13] << 8);
        const int l_seq = i32(o + 16);
        if (l_seq < 0 || o + 32 + l_read_name + 4ul * n_cigar + (size_t)(l_seq + 1) / 2 + (size_t)l_seq > o + (size_t)block) { a.error = "corrupt BAM record"; return false; }
        // ---- reference name
        const int ref_id = i32(o);
        const std::string& rname = (ref_id >= 0 && ref_id < n_ref) ? refs[(size_t)ref_id] : star;
        // ---- statistics, of every reference: the span of the binary operations M D N = X, which is what ref_span_end
        // gives for the text decode_bam_record writes (operation codes 9-15 print '?', which consumes nothing)
        long tot = 0;
        for (unsigned k = 0; k < n_cigar; k++) {
            uint32_t c; memcpy(&c, d.data() + o + 32 + l_read_name + 4ul * k, 4);
            const unsigned op = c & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) tot += (long)(c >> 4);
        }
        const int span = (int)(tot > 1 ? tot : 1);
        a.stats[rname].add(span);
        a.n_records++;
        // ---- keep or skip
        if (a.wants(rname.data(), rname.size())) a.by_ref[rname].push_back(decode_bam_record(a, d.data(), o, span));
        o += (size_t)block;
    }
    return true;
}

}  // namespace

extern "C" {

int sc_aln_open(const char* path, sc_aln** out) { return sc_aln_open_filtered(path, nullptr, -1, out); }

int sc_aln_open_filtered(const char* path, const char* const* names, int n_names, sc_aln** out) {
    if (!path || !out || (n_names > 0 && !names)) return SC_ERR_ARG;
    *out = nullptr;
    return sc::guarded(nullptr, "sc_aln_open", [&] {          // the handle's own message needs a handle: without one, the code alone
        std::unique_ptr<sc_aln> a(new sc_aln());
        if (n_names >= 0) {
            a->keep_all = false;
            for (int i = 0; i < n_names; i++) if (names[i]) a->keep.insert(names[i]);
        }
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return SC_ERR_ARG;
        struct stat stt;
        if (fstat(fd, &stt) != 0) { close(fd); return SC_ERR_ARG; }
        a->map_len = (size_t)stt.st_size;
        bool ok = true;
        if (a->map_len > 0) {
            a->map = mmap(nullptr, a->map_len, PROT_READ, MAP_PRIVATE, fd, 0);
            if (a->map == MAP_FAILED) { a->map = nullptr; close(fd); return SC_ERR_INTERNAL; }
            const unsigned char* b = (const unsigned char*)a->map;
            try {
                if (a->map_len >= 2 && b[0] == 0x1f && b[1] == 0x8b) {
                    ok = load_bam(*a, b, a->map_len);
                    munmap(a->map, a->map_len);            // every string was copied out
                    a->map = nullptr;
                } else {
                    ok = load_sam_text(*a, (const char*)a->map, a->map_len);
                }
            } catch (const std::bad_alloc&) { a->error = "out of memory while reading the alignments"; ok = false; }
            catch (const std::exception& ex) { a->error = ex.what(); ok = false; }
        }
        close(fd);
        *out = a.release();
        return ok ? SC_OK : SC_ERR_ARG;                // on a parse error the handle carries the message (sc_aln_error)
    });
}

void sc_aln_close(sc_aln* a) { delete a; }

long sc_aln_records(sc_aln* a) { return a ? a->n_records : 0; }

int sc_aln_ref_stats(sc_aln* a, const char* gene, long* n_records, long* aligned_bases) {
    if (!a || !gene) return SC_ERR_ARG;
    return sc::guarded(nullptr, "sc_aln_ref_stats", [&] {      // the key of the look-up is a string
        long n = 0, b = 0;
        auto it = a->stats.find(gene);
        if (it != a->stats.end()) { n = it->second.n; b = it->second.bases; }
        if (n_records) *n_records = n;
        if (aligned_bases) *aligned_bases = b;
        return SC_OK;
    });
}

int sc_aln_walk(sc_aln* a, long first, long n, char* buf, long cap, long* n_out, long* len_out) {
    if (!a || first < 0 || n < 0 || (n > 0 && !buf) || !n_out || !len_out) return SC_ERR_ARG;
    return sc::guarded(nullptr, "sc_aln_walk", [&] {
        std::call_once(a->order_once, [a] {
            a->order.reserve((size_t)a->n_records);
            for (auto& kv : a->by_ref) for (const Rec& r : kv.second) a->order.push_back(&r);
            std::sort(a->order.begin(), a->order.end(), [](const Rec* x, const Rec* y) { return x->ord < y->ord; });
        });
        *n_out = 0; *len_out = 0;
        long used = 0, k = 0;
        for (; k < n && first + k < (long)a->order.size(); k++) {
            const Rec& r = *a->order[(size_t)(first + k)];
            char num[16];
            const int nl = snprintf(num, sizeof num, "%d", r.flag);
            const long need = (long)r.qlen + nl + r.slen + r.quallen + 4;
            if (used + need > cap) break;
            char* o = buf + used;
            memcpy(o, r.qname, (size_t)r.qlen); o += r.qlen; *o++ = '\t';
            memcpy(o, num, (size_t)nl); o += nl; *o++ = '\t';
            memcpy(o, r.seq, (size_t)r.slen); o += r.slen; *o++ = '\t';
            memcpy(o, r.qual, (size_t)r.quallen); o += r.quallen; *o++ = '\n';
            used += need;
        }
        *n_out = k; *len_out = used;
        return (k == 0 && n > 0 && first < (long)a->order.size()) ? SC_ERR_CAPACITY : SC_OK;
    });
}

}  // extern "C"
