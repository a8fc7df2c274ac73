// Plain restatement of the stage-4 alignment contract, written from the contract and not from the kernels:
// the full local-alignment DP of every read against every seed on both strands, no window, no packing.
// stdin:  "S <n>" then n seed lines; "R <m>" then m lines "<SEQ> <QUAL>" (QUAL "*": Q40 everywhere).
// stdout: one line per read: "<AS> <XS> <seed> <strand> <pos> <CIGAR> <NM>" -- XS -1 when none; seed -1, pos 0, CIGAR "*"
// and NM 0 when the best score is below 20 + 8 ln(length).
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

namespace {

const int NEG = -1000000000;

int code(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

struct Best { int score = -1, col = 0, row = 0; };

// the DP of read `r` (bases already on the strand) with Phred values q against seed `s`
struct Dp {
    int L, N;
    std::vector<int> H, E, F;          // (L+1) x (N+1), row/column 0 = outside the matrix
    const std::string &r, &s;
    const std::vector<int>& q;
    Dp(const std::string& r_, const std::vector<int>& q_, const std::string& s_) : L((int)r_.size()), N((int)s_.size()), r(r_), s(s_), q(q_) {
        H.assign((size_t)(L + 1) * (N + 1), 0);
        E.assign(H.size(), NEG);
        F.assign(H.size(), NEG);
        for (int i = 1; i <= L; i++)
            for (int j = 1; j <= N; j++) {
                const bool gap_ok = (i - 1) >= 4 && (i - 1) < L - 4;         // --gbar 4 on the 0-based read row
                if (gap_ok) {
                    E[at(i, j)] = std::max(H[at(i, j - 1)] - 8, E[at(i, j - 1)] == NEG ? NEG : E[at(i, j - 1)] - 3);
                    F[at(i, j)] = std::max(H[at(i - 1, j)] - 8, F[at(i - 1, j)] == NEG ? NEG : F[at(i - 1, j)] - 3);
                }
                const int d = H[at(i - 1, j - 1)] + sub(i - 1, j - 1);
                H[at(i, j)] = std::max(std::max(0, d), std::max(E[at(i, j)], F[at(i, j)]));
            }
    }
    size_t at(int i, int j) const { return (size_t)i * (N + 1) + j; }
    int sub(int i, int j) const {
        const int a = code(r[i]), b = code(s[j]);
        if (a < 0 || b < 0) return -1;
        if (a == b) return 2;
        return -(2 + (4 * std::min(q[i], 40)) / 40);
    }
    Best best() const {                 // smallest end column, then smallest end row
        Best b;
        for (int j = 1; j <= N; j++)
            for (int i = 1; i <= L; i++)
                if (H[at(i, j)] > b.score) { b.score = H[at(i, j)]; b.col = j - 1; b.row = i - 1; }
        return b;
    }
    // traceback from (row, col), 0-based: diagonal, then D, then I; extension before opening
    void trace(int row, int col, int& pos, std::string& cigar, int& nm) const {
        std::vector<char> ops;
        int i = row + 1, j = col + 1, st = 0;
        nm = 0;
        while (true) {
            if (st == 0) {
                const int h = H[at(i, j)], hd = H[at(i - 1, j - 1)];
                if (h == hd + sub(i - 1, j - 1)) {
                    ops.push_back('M');
                    if (code(r[i - 1]) < 0 || code(r[i - 1]) != code(s[j - 1])) nm++;
                    if (hd == 0) break;
                    i--; j--;
                } else if (h == E[at(i, j)]) {
                    st = 1;
                } else {
                    st = 2;
                }
            } else if (st == 1) {
                ops.push_back('D'); nm++;
                const bool ext = E[at(i, j - 1)] != NEG && E[at(i, j)] == E[at(i, j - 1)] - 3;
                j--;
                st = ext ? 1 : 0;
            } else {
                ops.push_back('I'); nm++;
                const bool ext = F[at(i - 1, j)] != NEG && F[at(i, j)] == F[at(i - 1, j)] - 3;
                i--;
                st = ext ? 2 : 0;
            }
        }
        pos = j;                           // 1-based column of the first M
        std::vector<char> all((size_t)(i - 1), 'S');
        for (size_t k = ops.size(); k-- > 0;) all.push_back(ops[k]);
        for (int k = row + 1; k < L; k++) all.push_back('S');
        cigar.clear();
        for (size_t k = 0; k < all.size();) {
            size_t e = k;
            while (e < all.size() && all[e] == all[k]) e++;
            cigar += std::to_string(e - k) + all[k];
            k = e;
        }
    }
};

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

}  // namespace

int main() {
    std::string tag;
    int n = 0;
    std::cin >> tag >> n;
    std::vector<std::string> seeds((size_t)n);
    for (auto& s : seeds) std::cin >> s;
    std::cin >> tag >> n;
    for (int k = 0; k < n; k++) {
        std::string seq, qual;
        std::cin >> seq >> qual;
        const int L = (int)seq.size();
        std::vector<int> q((size_t)L, 40);
        if (qual != "*")
            for (int i = 0; i < L; i++) q[(size_t)i] = std::max(0, qual[(size_t)i] - 33);
        std::vector<int> qr(q.rbegin(), q.rend());
        const std::string rc = revcomp(seq);
        // every (seed, strand) in tie-break order: strict > keeps the first
        int bs = -1, bseed = -1, bstrand = 0, brow = 0, bcol = 0;
        std::vector<int> pair_best;
        for (int s = 0; s < (int)seeds.size(); s++)
            for (int strand = 0; strand < 2; strand++) {
                Dp dp(strand ? rc : seq, strand ? qr : q, seeds[(size_t)s]);
                const Best b = dp.best();
                pair_best.push_back(b.score);
                if (b.score > bs) { bs = b.score; bseed = s; bstrand = strand; brow = b.row; bcol = b.col; }
            }
        const double thr = 20.0 + 8.0 * std::log((double)L);
        int xs = -1;
        for (size_t p = 0; p < pair_best.size(); p++)
            if ((int)p != bseed * 2 + bstrand && (double)pair_best[p] >= thr) xs = std::max(xs, pair_best[p]);
        if ((double)bs < thr) {
            printf("%d %d -1 0 0 * 0\n", bs, xs);
            continue;
        }
        Dp dp(bstrand ? rc : seq, bstrand ? qr : q, seeds[(size_t)bseed]);
        int pos = 0, nm = 0;
        std::string cigar;
        dp.trace(brow, bcol, pos, cigar, nm);
        printf("%d %d %d %d %d %s %d\n", bs, xs, bseed, bstrand, pos, cigar.c_str(), nm);
    }
    return 0;
}
