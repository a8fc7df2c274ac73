// Records of an alignment file as the library holds them (sc_aln_file.cpp reads the file, sc_ingest.cpp a region's reads,
// sc_depth.hip scans them), and the two orders sc_aln_load_reads sorts a region's reads by.
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "sc_error.hpp"
#include "sc_threads.hpp"

namespace sc_ingest {
struct Rec {                       // the SAM fields the path reads: 1 2 4 5 6 10 11
    const char* qname; const char* cigar; const char* seq; const char* qual;
    int qlen, clen, slen, quallen;
    int flag, pos, mapq;
    int ref_end;                   // last reference position covered, ops M D N = X (what `view` and `mpileup` overlap on)
    long ord;                      // where the record starts in the (inflated) file: file order across references
};
// The message of the last failing call of THIS thread on any handle (windows are ingested side by side on several
// threads: a message kept on the shared handle could be another window's); the handle itself keeps what sc_aln_open said.
extern thread_local sc::LastError tl_error;

struct Kept {                      // a read that survived the filters, before duplicates collapse
    int relpos; uint32_t cig_off, cig_len; const char* seq; int seq_len; const char* name; int name_len; char suffix;   // suffix: 0, '1' or '2'
};
inline int cmp_bytes(const char* a, size_t la, const char* b, size_t lb) {      // as std::string compares; <0, 0, >0
    const int c = memcmp(a, b, std::min(la, lb));
    return c != 0 ? c : (la < lb ? -1 : la > lb);
}
// (position, CIGAR text, bases): the order of std::map<AlignRead,...> (StrainCall.cpp:594-627); <0, 0, >0
struct Cmp3 {
    const char* cig_pool;
    int operator()(const Kept& x, const Kept& y) const {
        if (x.relpos != y.relpos) return x.relpos < y.relpos ? -1 : 1;
        const int c = cmp_bytes(cig_pool + x.cig_off, x.cig_len, cig_pool + y.cig_off, y.cig_len);
        return c != 0 ? c : cmp_bytes(x.seq, (size_t)x.seq_len, y.seq, (size_t)y.seq_len);
    }
};
// compares name + ("/" suffix): the suffixed names as strings
inline int name_cmp(const Kept& x, const Kept& y) {
    const int l = std::min(x.name_len, y.name_len);
    const int c = memcmp(x.name, y.name, (size_t)l);
    if (c != 0) return c;
    // one name is a prefix of the other (or equal): compare the remainders, where a remainder is the rest of the
    // name followed by "/s" when the read is paired
    auto at = [](const Kept& z, int i) -> int {   // character i of the suffixed name, -1 past the end
        if (i < z.name_len) return (unsigned char)z.name[i];
        if (!z.suffix) return -1;
        if (i == z.name_len) return '/';
        if (i == z.name_len + 1) return (unsigned char)z.suffix;
        return -1;
    };
    for (int i = l;; i++) {
        const int cx = at(x, i), cy = at(y, i);
        if (cx != cy) return cx < cy ? -1 : 1;
        if (cx < 0) return 0;
    }
}

// std::stable_sort on up to `nt` threads: stretches of at least `min_stretch` elements sorted side by side, then merged
// pairwise (std::inplace_merge keeps equal elements in order, so the result is the one a single stable sort gives).  A
// million reads of a deep region are compared by position, CIGAR text and bases: two such sorts were half of its ingest.
template <class T, class Less>
void stable_sort_mt(std::vector<T>& v, const Less& less, int nt, size_t min_stretch) {
    const size_t n = v.size();
    while (nt > 1 && n / (size_t)nt < min_stretch) nt--;
    if (nt <= 1) { std::stable_sort(v.begin(), v.end(), less); return; }
    std::vector<size_t> cut((size_t)nt + 1);
    for (int t = 0; t <= nt; t++) cut[(size_t)t] = n * (size_t)t / (size_t)nt;
    sc::parallel_items(nt, nt, [&](int t) { std::stable_sort(v.begin() + (long)cut[(size_t)t], v.begin() + (long)cut[(size_t)t + 1], less); });
    for (int width = 1; width < nt; width *= 2) {
        const int pairs = (nt - width + 2 * width - 1) / (2 * width);      // stretches lo with lo + width < nt
        sc::parallel_items(pairs, pairs, [&](int k) {
            const int lo = 2 * width * k;
            std::inplace_merge(v.begin() + (long)cut[(size_t)lo], v.begin() + (long)cut[(size_t)(lo + width)],
                               v.begin() + (long)cut[(size_t)std::min(lo + 2 * width, nt)], less);
        });
    }
}
}  // namespace sc_ingest

struct sc_aln {
    std::string error;
    // backing store of the record text: the mapped SAM file, or strings decoded from BAM
    void* map = nullptr; size_t map_len = 0;
    std::vector<std::unique_ptr<char[]>> arenas; size_t arena_used = 0, arena_cap = 0;
    std::unordered_map<std::string, std::vector<sc_ingest::Rec>> by_ref;      // records of a reference, in file order
    long n_records = 0;
    // what a scheduler prices a region with, for EVERY reference of the file -- also for those whose records were not
    // kept (sc_aln_open_filtered: a rank of a multi-GPU run keeps the records of its own shard only)
    struct RefStat { long n = 0, bases = 0; void add(long span) { n++; bases += span; } };
    std::unordered_map<std::string, RefStat> stats;
    bool keep_all = true;
    std::unordered_set<std::string> keep;                                     // references whose records are kept when !keep_all
    std::once_flag order_once;
    std::vector<const sc_ingest::Rec*> order;                                 // every kept record in file order (sc_aln_walk)
    bool wants(const char* name, size_t n) const { return keep_all || keep.count(std::string(name, n)) != 0; }

    char* alloc(size_t n) {
        if (arena_used + n > arena_cap) {
            arena_cap = std::max<size_t>(n, 1 << 24);
            arenas.emplace_back(new char[arena_cap]);
            arena_used = 0;
        }
        char* p = arenas.back().get() + arena_used;
        arena_used += n;
        return p;
    }
    ~sc_aln() { if (map) munmap(map, map_len); }
};

