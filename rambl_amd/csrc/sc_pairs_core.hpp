// The word arithmetic of the gene-against-gene edit distance: the Myers / Hyyrö block bit-vector step, the
// column of W such steps, and the codes both sides of a pair are packed in.  No HIP in here: plain g++ compiles it
// (tests/native/pairs_check.cpp), and sc_pairs.hip runs the same text on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SC_PAIRS_HD __host__ __device__
#define SC_PAIRS_UNROLL _Pragma("unroll")          // the per-word loops must unroll on the device: pv and mv stay in registers
#else
#define SC_PAIRS_HD
#define SC_PAIRS_UNROLL
#endif

namespace sc_pairs {

constexpr int WIDTHS[] = {8, 16, 24, 32};          // the instantiated W: a pattern of up to 64 W bases runs at the least W that holds it
constexpr int N_WIDTHS = (int)(sizeof(WIDTHS) / sizeof(WIDTHS[0]));
constexpr int MAX_LEN = 64 * WIDTHS[N_WIDTHS - 1];          // 2 048
constexpr int N_CODES = 5;                         // A C G T and "other"
constexpr unsigned OTHER = 4;                      // matches nothing, itself included: its row of the match masks is all zero
constexpr int CODES_PER_DWORD = 8;                 // 4 bits a code
constexpr uint32_t PAD_DWORD = 0x44444444u;        // eight "other" codes: what lies behind a sequence's last base

SC_PAIRS_HD inline unsigned base_code(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return OTHER;
    }
}

// The least listed W with 64 W >= len, as an index into WIDTHS; -1 when there is none.
SC_PAIRS_HD inline int width_class(long len) {
    for (int k = 0; k < N_WIDTHS; k++)
        if (len <= 64L * WIDTHS[k]) return k;
    return -1;
}

// bound(a, b) of the contract: (max(|a|, |b|) * diff_num) / diff_den in 64 bits.
SC_PAIRS_HD inline long pair_bound(long len_a, long len_b, long diff_num, long diff_den) {
    return ((len_a > len_b ? len_a : len_b) * diff_num) / diff_den;
}

// Dwords that hold `len` codes.
SC_PAIRS_HD inline long packed_dwords(long len) { return (len + CODES_PER_DWORD - 1) / CODES_PER_DWORD; }

// Packs text[0..len) into out[0..packed_dwords(len)), first base in the low bits, "other" behind the last base.
inline void pack_codes(const char* text, long len, uint32_t* out) {
    for (long d = 0, nd = packed_dwords(len); d < nd; d++) {
        uint32_t x = PAD_DWORD;
        for (int k = 0; k < CODES_PER_DWORD && d * CODES_PER_DWORD + k < len; k++)
            x = (x & ~(15u << (4 * k))) | (base_code(text[d * CODES_PER_DWORD + k]) << (4 * k));
        out[d] = x;
    }
}

// The word `w` of the pattern's match mask for code `c` (0..3): bit i is set where pattern base 64 w + i is c.  `packed` holds
// the pattern's n_dwords dwords; what lies behind them reads as "other".
SC_PAIRS_HD inline uint64_t match_word(const uint32_t* packed, long n_dwords, int w, unsigned c) {
    uint64_t bits = 0;
    for (int k = 0; k < 8; k++) {
        const long d = (long)w * 8 + k;
        const uint32_t x = d < n_dwords ? packed[d] : PAD_DWORD;
        for (int i = 0; i < CODES_PER_DWORD; i++)
            if (((x >> (4 * i)) & 15u) == c) bits |= (uint64_t)1 << (8 * k + i);
    }
    return bits;
}

// One 64-row block of the DP table moves one text base to the right.  eq: the pattern rows of the block that match the base;
// pv, mv: the block's vertical differences +1 / -1 (bit i: D[r0 + i + 1][j] - D[r0 + i][j] over the block's rows), updated in place;
// hin: the horizontal difference D[r0][j] - D[r0][j - 1] on the row above the block, in {-1, 0, +1}.  Returns the horizontal
// difference below row `bit` of the block: 63 hands it to the next block, the pattern's last row follows the score.
SC_PAIRS_HD inline int block_step(uint64_t eq, uint64_t& pv, uint64_t& mv, int hin, int bit) {
    const uint64_t hin_neg = hin < 0 ? 1u : 0u, hin_pos = hin > 0 ? 1u : 0u;
    const uint64_t xv = eq | mv;
    eq |= hin_neg;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    const int hout = (int)((ph >> bit) & 1u) - (int)((mh >> bit) & 1u);
    ph = (ph << 1) | hin_pos;
    mh = (mh << 1) | hin_neg;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// One text base through the pattern's words 0..last_word: eq_row[w] is the base's match mask of word w (any indexable thing:
// an array on the host, LDS on the device).  The top row of the table is D[0][j] = j, so word 0 takes +1.  Returns the
// score's change, read below bit last_bit of word last_word; the words above it are not touched.
template <int W, class EqRow>
SC_PAIRS_HD inline int column_step(const EqRow& eq_row, uint64_t (&pv)[W], uint64_t (&mv)[W], int last_word, int last_bit) {
    int h = 1;
    SC_PAIRS_UNROLL
    for (int w = 0; w < W; w++) {
        if (w <= last_word) h = block_step(eq_row[w], pv[w], mv[w], h, w == last_word ? last_bit : 63);
    }
    return h;
}

// The unit-cost edit distance of a pattern of m bases (1..64 W), given as its match masks peq[c * W + w], and a packed text of n
// bases: the host's whole walk, as a lane of k_pairs makes it.
template <int W>
inline int distance(const uint64_t* peq, int m, const uint32_t* text, int n) {
    uint64_t pv[W], mv[W];
    for (int w = 0; w < W; w++) { pv[w] = ~(uint64_t)0; mv[w] = 0; }
    const int last_word = (m - 1) / 64, last_bit = (m - 1) % 64;
    int score = m;
    for (int j = 0; j < n; j++) {
        const unsigned c = (text[j / CODES_PER_DWORD] >> (4 * (j % CODES_PER_DWORD))) & 15u;
        score += column_step<W>(peq + (long)c * W, pv, mv, last_word, last_bit);
    }
    return score;
}

}  // namespace sc_pairs
