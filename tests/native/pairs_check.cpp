// Stand-alone driver of rambl_amd/csrc/sc_pairs_core.hpp, the word arithmetic k_pairs runs on the device: no HIP, no library.
// stdin: one pair per line, `PATTERN TEXT` (two words of 1..2048 bytes).  stdout: per line the distance computed at every listed W,
// `-` where the pattern does not fit 64 W bases, separated by blanks -- every W that fits must agree, which the caller checks.
// `pairs_check widths` prints the W list instead.  `pairs_check time` reads the same lines, runs each at its least W only and
// prints one line `pairs N word_steps S ms T checksum C` (tools/otu_bench.py: the one-core figure).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../rambl_amd/csrc/sc_pairs_core.hpp"

using namespace sc_pairs;

template <int W>
static int run(const std::string& pattern, const std::string& text) {
    const int m = (int)pattern.size(), n = (int)text.size();
    std::vector<uint32_t> p((size_t)packed_dwords(m)), t((size_t)packed_dwords(n));          // exact sizes: a read behind them is the sanitizer's
    pack_codes(pattern.data(), m, p.data());
    pack_codes(text.data(), n, t.data());
    std::vector<uint64_t> peq((size_t)N_CODES * W, 0);
    for (int c = 0; c < 4; c++)
        for (int w = 0; w <= (m - 1) / 64; w++) peq[(size_t)c * W + w] = match_word(p.data(), (long)p.size(), w, (unsigned)c);
    return distance<W>(peq.data(), m, t.data(), n);
}

using Run = int (*)(const std::string&, const std::string&);
static const Run RUN[N_WIDTHS] = {run<WIDTHS[0]>, run<WIDTHS[1]>, run<WIDTHS[2]>, run<WIDTHS[3]>};

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "widths")) {
        for (int k = 0; k < N_WIDTHS; k++) printf("%d%c", WIDTHS[k], k + 1 < N_WIDTHS ? ' ' : '\n');
        return 0;
    }
    const bool timed = argc > 1 && !strcmp(argv[1], "time");
    std::vector<std::pair<std::string, std::string>> pairs;
    std::string a, b;
    while (std::cin >> a >> b) {
        if (a.empty() || b.empty() || (long)a.size() > MAX_LEN || (long)b.size() > MAX_LEN) {
            fprintf(stderr, "pairs_check: line %zu is outside 1..%d bytes\n", pairs.size() + 1, MAX_LEN);
            return 2;
        }
        pairs.emplace_back(a, b);
    }
    if (timed) {
        long steps = 0, sum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (const auto& p : pairs) {
            sum += RUN[width_class((long)p.first.size())](p.first, p.second);
            steps += (long)p.second.size() * (((long)p.first.size() + 63) / 64);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("pairs %zu word_steps %ld ms %.3f checksum %ld\n", pairs.size(), steps, ms, sum);
        return 0;
    }
    for (const auto& p : pairs) {
        for (int k = 0; k < N_WIDTHS; k++) {
            if ((long)p.first.size() <= 64L * WIDTHS[k]) printf("%d", RUN[k](p.first, p.second));
            else printf("-");
            putchar(k + 1 < N_WIDTHS ? ' ' : '\n');
        }
    }
    return 0;
}
