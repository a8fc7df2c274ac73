// Plain restatement of the hit contract of the per-sample gene profile, written from the contract and not from
// the kernels: the full local-alignment DP of every segment against every gene on both strands, the whole matrix kept, the
// traceback walked through it, E in double.  No window, no packing, no threshold before the traceback.
// argv:   <min identity %> <max E> <lambda> <K>
// stdin:  "G <n>" then n gene lines; "Q <m>" then m segment lines.
// stdout: one line per emitted hit, in (segment, gene) order:
//         "<segment> <gene> <strand> <score doubled> <identity> <align_len> <qfrom> <qto> <hfrom> <hto> <E as %.17g>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

namespace {

int code(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

std::string revcomp(const std::string& x) {
    std::string y(x.rbegin(), x.rend());
    for (char& c : y) {
        switch (c) {
            case 'A': case 'a': c = 'T'; break;
            case 'C': case 'c': c = 'G'; break;
            case 'G': case 'g': c = 'C'; break;
            case 'T': case 't': c = 'A'; break;
            default: break;
        }
    }
    return y;
}

// doubled scores: match +2, mismatch (and any base outside ACGT) -4, a gap base -5
struct Dp {
    int L, N;
    std::vector<int> H;                // (L+1) x (N+1), row / column 0 = outside the matrix
    const std::string &q, &g;
    Dp(const std::string& q_, const std::string& g_) : L((int)q_.size()), N((int)g_.size()), q(q_), g(g_) {
        H.assign((size_t)(L + 1) * (N + 1), 0);
        for (int i = 1; i <= L; i++)
            for (int j = 1; j <= N; j++) {
                int h = 0;
                h = std::max(h, H[at(i - 1, j - 1)] + sub(i - 1, j - 1));
                h = std::max(h, H[at(i, j - 1)] - 5);
                h = std::max(h, H[at(i - 1, j)] - 5);
                H[at(i, j)] = h;
            }
    }
    size_t at(int i, int j) const { return (size_t)i * (N + 1) + j; }
    bool same(int i, int j) const { return code(q[i]) >= 0 && code(q[i]) == code(g[j]); }
    int sub(int i, int j) const { return same(i, j) ? 2 : -4; }
    // best cell: highest score, then smallest end column, then smallest end row (0-based)
    void best(int& score, int& col, int& row) const {
        score = 0; col = 0; row = 0;
        for (int j = 1; j <= N; j++)
            for (int i = 1; i <= L; i++)
                if (H[at(i, j)] > score) { score = H[at(i, j)]; col = j - 1; row = i - 1; }
    }
    // traceback from (row, col): diagonal, then left (gap in the segment), then up (gap in the gene); a diagonal step from a
    // zero cell is the first column of the alignment
    void trace(int row, int col, int& row0, int& col0, int& ident, int& alen) const {
        int i = row + 1, j = col + 1;
        ident = 0; alen = 0;
        while (true) {
            const int h = H[at(i, j)];
            alen++;
            if (h == H[at(i - 1, j - 1)] + sub(i - 1, j - 1)) {
                if (same(i - 1, j - 1)) ident++;
                if (H[at(i - 1, j - 1)] == 0) break;
                i--; j--;
            } else if (h == H[at(i, j - 1)] - 5) {
                j--;
            } else {
                i--;
            }
        }
        row0 = i - 1; col0 = j - 1;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: blast_hits_check MIN_IDENTITY MAX_EVALUE LAMBDA K < input\n"); return 2; }
    const double min_identity = atof(argv[1]), max_evalue = atof(argv[2]), lambda = atof(argv[3]), K = atof(argv[4]);
    std::string tag;
    int n = 0;
    std::cin >> tag >> n;
    std::vector<std::string> genes((size_t)n);
    long total = 0;
    for (auto& s : genes) { std::cin >> s; total += (long)s.size(); }
    std::cin >> tag >> n;
    for (int k = 0; k < n; k++) {
        std::string seg;
        std::cin >> seg;
        const std::string rc = revcomp(seg);
        const int L = (int)seg.size();
        for (int g = 0; g < (int)genes.size(); g++) {
            int bs = 0, bstrand = 0, brow = 0, bcol = 0;
            for (int strand = 0; strand < 2; strand++) {           // strict >: the forward strand keeps a tie
                Dp dp(strand ? rc : seg, genes[(size_t)g]);
                int s, c, r;
                dp.best(s, c, r);
                if (s > bs) { bs = s; bstrand = strand; brow = r; bcol = c; }
            }
            if (bs <= 0) continue;
            Dp dp(bstrand ? rc : seg, genes[(size_t)g]);
            int row0, col0, ident, alen;
            dp.trace(brow, bcol, row0, col0, ident, alen);
            const double e = K * (double)L * (double)total * std::exp(-lambda * (0.5 * (double)bs));
            if (!(100.0 * (double)ident / (double)alen >= min_identity) || !(e <= max_evalue)) continue;
            const int qfrom = bstrand ? L - brow : row0 + 1, qto = bstrand ? L - row0 : brow + 1;
            const int hfrom = bstrand ? bcol + 1 : col0 + 1, hto = bstrand ? col0 + 1 : bcol + 1;
            printf("%d %d %d %d %d %d %d %d %d %d %.17g\n", k, g, bstrand, bs, ident, alen, qfrom, qto, hfrom, hto, e);
        }
    }
    return 0;
}
