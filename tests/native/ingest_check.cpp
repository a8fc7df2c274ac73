// The pure parts of the read ingest on their own, built with g++ under the address and undefined-behaviour sanitizers
// (tests/test_host_side.py::test_ingest_native_check): no GPU, no library, nothing loaded into Python.
//   ingest_check crop        lines "w0 w1 pos cigar seqlen" on stdin -> "lead trail cigar" or "FAIL" per line
//                            (parse_cigar + crop_to_window + the substr check of sc_aln_load_reads)
//   ingest_check order       stable_sort_mt against std::stable_sort, name_cmp against std::string; prints "order ok"
//   ingest_check open F...   sc_aln_open on each file -> "rc records message" per file
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/straincall_hip.h"
#include "../../rambl_amd/csrc/sc_cigar.hpp"
#include "../../rambl_amd/csrc/sc_ingest.hpp"

using namespace sc_ingest;

static int crop_lines() {
    int w0, w1, pos, seqlen;
    char cigar[4096];
    std::vector<Op> ops;
    Cropped cr;
    while (scanf("%d %d %d %4095s %d", &w0, &w1, &pos, cigar, &seqlen) == 5) {
        bool ok = parse_cigar(cigar, (int)strlen(cigar), ops);
        if (ok) {
            int r1 = pos;
            for (const Op& o : ops) if (o.op == 'M' || o.op == 'D') r1 += o.len;
            crop_to_window(w0, w1, ops, pos, r1 - 1, cr);
            ok = cr.ok && cr.lead <= seqlen && cr.trail <= seqlen;
        }
        if (!ok) { puts("FAIL"); continue; }
        printf("%d %d ", cr.lead, cr.trail);
        for (const Op& o : cr.ops) printf("%d%c", o.len, o.op);
        putchar('\n');
    }
    return 0;
}

static int sort_against_std() {
    typedef std::pair<int, int> KI;                      // (key, original index), compared by the key alone
    auto less = [](const KI& a, const KI& b) { return a.first < b.first; };
    unsigned state = 12345u;
    long cases = 0;
    for (int nt : {1, 2, 3, 5, 8})
        for (size_t min_stretch : {(size_t)2, (size_t)50}) {
            const size_t edge = (size_t)nt * min_stretch;
            for (size_t n : {(size_t)0, (size_t)1, (size_t)2, edge - 1, edge, edge + 1}) {
                std::vector<KI> v(n);
                for (size_t i = 0; i < n; i++) { state = state * 1664525u + 1013904223u; v[i] = KI((int)((state >> 16) % 7u), (int)i); }
                std::vector<KI> want(v);
                std::stable_sort(want.begin(), want.end(), less);
                stable_sort_mt(v, less, nt, min_stretch);
                if (v != want) { printf("stable_sort_mt differs: nt %d min_stretch %zu n %zu\n", nt, min_stretch, n); return 1; }
                cases++;
            }
        }
    printf("%ld sorts equal\n", cases);
    return 0;
}

static int names_against_string() {
    // a name that is a prefix of another, names that end in /1 themselves, equal names with every suffix, the empty name,
    // a byte above 127
    const struct { const char* name; char suffix; } rows[] = {
        {"r1", 0}, {"r1", '1'}, {"r1", '2'}, {"r1/1", 0}, {"r1/2", 0}, {"r1/1", '2'}, {"r1", 0}, {"r", 0}, {"r", '1'}, {"r10", 0},
        {"r10", '2'}, {"r1/", 0}, {"r1/10", 0}, {"r1.", 0}, {"r1.", '1'}, {"r1A", '1'}, {"", 0}, {"", '1'}, {"/1", 0}, {"r\xff", 0}, {"r\xff", '2'}};
    std::vector<Kept> ks;
    std::vector<std::string> full;
    for (const auto& r : rows) {
        Kept k{};
        k.name = r.name; k.name_len = (int)strlen(r.name); k.suffix = r.suffix;
        ks.push_back(k);
        full.push_back(std::string(r.name) + (r.suffix ? std::string("/") + r.suffix : std::string()));
    }
    // agreeing in sign with a total order of strings on every ordered pair makes name_cmp a strict weak order
    auto sign = [](int c) { return (c > 0) - (c < 0); };
    for (size_t i = 0; i < ks.size(); i++)
        for (size_t j = 0; j < ks.size(); j++)
            if (sign(name_cmp(ks[i], ks[j])) != sign(full[i].compare(full[j]))) {
                printf("name_cmp differs from std::string on '%s' and '%s'\n", full[i].c_str(), full[j].c_str());
                return 1;
            }
    printf("%zu names ordered as strings\n", ks.size());
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "crop") return crop_lines();
    if (mode == "order") {
        if (sort_against_std() || names_against_string()) return 1;
        puts("order ok");
        return 0;
    }
    if (mode == "open") {
        for (int i = 2; i < argc; i++) {
            sc_aln* a = nullptr;
            const int rc = sc_aln_open(argv[i], &a);
            printf("%d %ld %s\n", rc, sc_aln_records(a), sc_aln_error(a));
            sc_aln_close(a);
        }
        return 0;
    }
    fprintf(stderr, "usage: ingest_check crop | order | open FILE...\n");
    return 2;
}
