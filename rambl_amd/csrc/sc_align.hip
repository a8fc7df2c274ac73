// Stage 4 of rambl.py on the device: every gene read aligned to every seed OTU on both strands, the exact optimum of
// bowtie2's --local scoring (DESIGN.md §8.7 is the contract) -- what scripts/recluster_data_to_seed_otus.py:198-277
// runs bowtie2 --sensitive-local for.  The sweep, the traceback window and its block loop are sc_wave_dp.hpp; the cell, the
// score kernel and the traceback kernel are sc_sw.hpp, which the read mapper (sc_map.hip) shares.  This file holds the entry
// point: the full product of reads and seeds through k_sw_score, then k_sw_trace over the reads that align.
#include <cmath>
#include <cstring>

#include "sc_sw.hpp"

namespace {

thread_local sc::LastError tl_error;

}  // namespace

extern "C" {

const char* sc_align_error(void) { return tl_error.text.c_str(); }

int sc_align_reads(int device, const char* seed_text, const long* seed_off, int n_seeds, const char* read_text, const char* qual_text,
                   const long* read_off, int n_reads, int* as, int* xs, int* seed, int* strand, int* pos, int* nm, unsigned* cigar,
                   int cigar_stride, int* n_cigar, sc_align_stats* stats) {
    tl_error.clear();
    if (stats) std::memset(stats, 0, sizeof *stats);
    return sc::guarded(&tl_error, "sc_align_reads", [&] {
        if (!seed_text || !seed_off || n_seeds < 1 || n_reads < 0 || (n_reads > 0 && (!read_text || !read_off)) || !as || !xs || !seed ||
            !strand || !pos || !nm || !cigar || cigar_stride < 1 || !n_cigar)
            return tl_error.fail(SC_ERR_ARG, "sc_align_reads: missing argument");
        if (n_seeds > MAX_SEEDS) return tl_error.fail(SC_ERR_UNSUPPORTED, "sc_align_reads: more than 1048575 seeds");
        Packed sd, rd;
        std::string why;
        if (!sd.rebase(seed_off, n_seeds, MAX_COLS, "sc_align_reads", "seed", why) ||
            (n_reads > 0 && !rd.rebase(read_off, n_reads, MAX_ROWS, "sc_align_reads", "read", why)))
            return tl_error.fail(SC_ERR_UNSUPPORTED, why);
        long max_len = 0;
        for (int r = 0; r < n_reads; r++) max_len = std::max(max_len, rd.len(r));
        if (cigar_stride < max_len / 2 + 4) return tl_error.fail(SC_ERR_CAPACITY, "sc_align_reads: cigar_stride below max read length / 2 + 4");
        sc::select_device(device);
        if (n_reads == 0) return SC_OK;
        const double t0 = sc::now_ms();
        // ---- host packing: seed codes, read code | penalty << 4, reads bucketed by rows per lane
        sd.pack(seed_text + seed_off[0], [](long, int c) { return c < 0 ? REF_OTHER : c; });
        rd.pack(read_text + read_off[0], [&](long k, int c) { return read_row_byte(c, qual_text ? qual_text + read_off[0] : nullptr, k); });
        Buckets by_r;
        for (int r = 0; r < n_reads; r++) by_r.add(r, rd.len(r));
        const std::vector<int> rids = by_r.order();
        // ---- device: the score pass
        sc::DevMem<uint8_t> d_sq(sd.codes.size()), d_rq(rd.codes.size());
        sc::DevMem<long> d_so(sd.off.size()), d_ro(rd.off.size());
        sc::DevMem<int> d_rids(rids.size());
        sc::DevMem<unsigned long long> d_best((size_t)n_reads), d_second((size_t)n_reads);
        sc::TimedStream st;
        st.mark("upload");
        st.h2d(d_sq, sd.codes); st.h2d(d_so, sd.off); st.h2d(d_rq, rd.codes); st.h2d(d_ro, rd.off); st.h2d(d_rids, rids);
        st.zero(d_best.p, (size_t)n_reads * 8);
        st.zero(d_second.p, (size_t)n_reads * 8);
        st.mark("score");
        by_r.each([&](auto r, long at, const std::vector<int>& ids) {
            const long n_tiles = (long)ids.size() * 2L * n_seeds;
            hipLaunchKernelGGL(k_sw_score<decltype(r)::value>, score_grid(n_tiles), dim3(64 * SCORE_WAVES), 0, st, d_sq.p, d_so.p, d_rq.p,
                               d_ro.p, AllTiles{n_seeds, d_rids.p + at}, n_tiles, d_best.p, d_second.p);
            st.launched();
            if (stats) for (int id : ids) stats->score_cells += 2L * rd.len(id) * sd.bytes();
        });
        st.mark("scored");
        std::vector<unsigned long long> best((size_t)n_reads), second((size_t)n_reads);
        st.d2h(best, d_best); st.d2h(second, d_second);
        st.sync();
        // ---- which reads align; the traceback of those, bucketed by rows per lane again
        const int n_tr = trace_aligned(st, d_sq.p, d_so.p, d_rq.p, d_ro.p, d_best.p, rd, best, second, as, xs, seed, strand, pos, nm, cigar,
                                       cigar_stride, n_cigar, stats ? &stats->trace_cells : nullptr);
        int rc = SC_OK;
        if (n_tr < 0) rc = tl_error.fail(SC_ERR_INTERNAL, "sc_align_reads: traceback of read " + std::to_string(-1 - n_tr) + " failed");
        if (stats && rc == SC_OK) {
            read_phase_ms(st, stats);
            stats->n_traced = n_tr;
        }
        if (stats) stats->total_ms = sc::now_ms() - t0;
        return rc;
    });
}

}  // extern "C"
