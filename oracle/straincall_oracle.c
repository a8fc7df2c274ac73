/* TEST INFRASTRUCTURE ONLY -- the ORACLE.
 *
 * A plain-C CPU restatement of the reference's StrainCall path
 * (/root/reference/StrainCall/), used by tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg to CHECK the HIP
 * product path.  Nothing under rambl_amd/ imports, links or executes it.
 *
 * Parity status: PINNED.  The reference has no tests or golden vectors of its own
 * (SURVEY.md section 4); this restatement is pinned against outputs of the
 * reference itself run in the build container -- the shipped binary
 * /root/reference/StrainCall/StrainCall and oracle/_ref/StrainCall_ref built from
 * the reference sources by oracle/Makefile -- via the fixtures committed under
 * tests/golden/ (FASTA, -G graph dumps, per-level traces, MSA vectors) and the
 * differential test tests/test_oracle_vs_ref.py.
 *
 * Arithmetic: x87 long double exactly as the reference (DoubleL).  The command
 * line is the reference's (StrainCall.cpp:98-154); like the reference it shells
 * out to `samtools`.  Extra switches, for tests only, come from the environment:
 *   SC_TRACE=1 [SC_TRACE_PREC=n]  per-level strain/abundance trace on stderr
 *                                 (same text as the reference's dormant blocks,
 *                                 NonparametricClustering.cpp:287-298,460-471)
 */
#include "o_util.h"
#include "o_graph.h"
#include "o_msa.h"
#include "o_cluster.h"
#include "o_ingest.h"

static void help(void) {                                               /* StrainCall.cpp:34-55 */
    fputs("StrainCall marker_gene read_mapping\n"
          "           [-r gn:p0-p1] [-w window_size]\n"
          "           [-e error_rate] [-q map_qual]\n"
          "\n"
          "Options\n"
          "-r,--roi           region of interesting, gn is gene name,\n"
          "                   p0 is starting position, p1 is ending position (inclusive)\n"
          "-w,--window        the size of scanning window [500]\n"
          "-o,--overlap       the size of window-window overlap [100]\n"
          "-e,--error-rate    sequencing error rate [0.01]\n"
          "-D,--max-depth     downsample data to the specified depth [800]\n"
          "-q,--map-qual      only include reads with mapping quality >= INT [3]\n"
          "-I,--max-ins       only include reads with insertions <= INT [10]\n"
          "-l,--read-len      only include reads with length >=INT [80]\n"
          "-t,--tau           only include strains with abundance level >=FLT [0.02]\n"
          "-d,--diff-rate     only include strains with difference rate >=FLT [0.01]\n"
          "-G,--plot-graph    print graph\n"
          "-h,--help          print this message\n"
          "\n", stderr);
}

/* StrainCall.cpp:972-1059 */
int oracle_main(int argc, char **argv) {
    ScParam pa; sc_param_init(&pa);
    --argc; ++argv;
    sc_parse_cmd_line(argc, argv, &pa);
    if (pa.print_help || argc == 0) { help(); return 0; }
    WindowVec windows; vec_init(windows);
    make_scan_window(&pa, &windows);
    long total_draws = 0;
    for (int wi = 0; wi < windows.n; wi++) {
        ScWindow *w = &windows.v[wi];
        char roi[1024];
        snprintf(roi, sizeof roi, "%s:%d-%d", w->gn, w->p0, w->p1);
        char *gene_seq = load_gene_seq(pa.gene_file, roi);
        AReadVec reads; vec_init(reads);
        ReadPairs rp; rp.mates = NULL; rp.n = 0;
        load_mapping_reads(gene_seq, pa.mapping_file, pa.mapping_qual, pa.read_len, pa.max_ins, pa.max_depth, roi, &reads, &rp);
        if (getenv("SC_ORACLE_DUMP_READS")) {
            /* test fixture: what crosses from ingest (a1-a4) into the graph stage */
            char path[4096];
            snprintf(path, sizeof path, "%s.%d", getenv("SC_ORACLE_DUMP_READS"), wi);
            FILE *df = fopen(path, "w");
            if (df) {
                fprintf(df, "WINDOW\t%s\t%d\t%d\n", w->gn, w->p0, w->p1);
                fprintf(df, "REF\t%s\n", gene_seq);
                for (int i = 0; i < reads.n; i++) {
                    fprintf(df, "READ\t%d\t%s\t%s\t%d\t", reads.v[i].pos, reads.v[i].cigar, reads.v[i].seq, reads.v[i].cn);
                    for (int k = 0; k < rp.mates[i].n; k++) fprintf(df, "%s%d", k ? "," : "", rp.mates[i].v[k]);
                    fprintf(df, "\n");
                }
                fclose(df);
            }
        }
        if (reads.n == 0) { free(gene_seq); continue; }
        Graph *g = graph_build(gene_seq, reads.v, reads.n);
        if (!pa.plot_graph) {
            ClusterCtx cx; cx.g = g; cx.rp = &rp; cx.draws = 0;
            cx.trace = getenv("SC_TRACE") != NULL;
            cx.trace_prec = getenv("SC_TRACE_PREC") ? atoi(getenv("SC_TRACE_PREC")) : 6;
            cx.trace_fp = stderr;
            StrainVec strains; vec_init(strains);
            streaming_clustering(&cx, &strains, 5000, (ld)pa.error_rate, (ld)pa.tau, (ld)pa.diff_rate, reads.n);
            read_assign(&cx, &strains, reads.v, reads.n, 5000);
            sort_strains(&strains);                                    /* :1027 */
            char *gene_seq0 = load_gene_seq(pa.gene_file, w->gn);      /* :1031 (result unused) */
            free(gene_seq0);
            for (int si = 0; si < strains.n; si++) {
                if (strains.v[si].abundance >= (ld)pa.tau) {
                    char *out = strain_plain_seq(&strains.v[si]);
                    printf(">contig%s%d%d%d\n%s\n", w->gn, w->p0, w->p1, si, out);
                    free(out);
                }
            }
            for (int si = 0; si < strains.n; si++) strain_free(&strains.v[si]);
            vec_free(strains);
            total_draws += cx.draws;
        } else {
            output_edge(g, stdout);
        }
        graph_free(g);
        for (int i = 0; i < reads.n; i++) { free(reads.v[i].cigar); free(reads.v[i].seq); }
        vec_free(reads);
        for (int i = 0; i < rp.n; i++) vec_free(rp.mates[i]);
        free(rp.mates);
        free(gene_seq);
    }
    if (getenv("SC_ORACLE_STATS")) fprintf(stderr, "oracle_draws %ld\n", total_draws);
    fflush(stdout);
    return 0;
}

/* ---- entry points for ctypes-driven unit tests (liboracle.so) -------------- */
/* Sum-of-pairs MSA of `n` NUL-terminated sequences (row a7).  `out` receives the
 * n padded rows, each `*ncol` chars + NUL, packed back to back. Returns 0. */
int oracle_msa_align(const char **seqs, int n, char *out, int out_cap, int *ncol) {
    char **rows = NULL;
    int nc = msa_sp_align((char **)seqs, n, &rows);
    *ncol = nc;
    int rc = 0;
    if ((long)n * (nc + 1) > out_cap) rc = -1;
    for (int t = 0; t < n; t++) {
        if (!rc) memcpy(out + (long)t * (nc + 1), rows[t], (size_t)nc + 1);
        free(rows[t]);
    }
    free(rows);
    return rc;
}
/* libstdc++ std::sort permutation of n keys, descending (`a > b` comparator). */
static int key_gt(void *ctx, int a, int b) { const double *k = (const double *)ctx; return k[a] > k[b]; }
void oracle_sort_desc_perm(const double *keys, int n, int *perm) {
    for (int i = 0; i < n; i++) perm[i] = i;
    std_sort_perm(perm, n, key_gt, (void *)keys);
}
/* first `n` outputs of generate_canonical<double,53>(mt19937(seed)) */
void oracle_mt_canonical(unsigned seed, int n, double *out) {
    MT m; mt_seed(&m, seed);
    for (int i = 0; i < n; i++) out[i] = mt_canonical(&m);
}

/* One sampler level's draws (the draw loop of np_bayes_clustering) on chosen
 * inputs and uniforms.  S strains with urn weights a0[S] and read
 * log-likelihood rows ll[s * n_reads + r] (widened to long double, as the
 * reference holds them), present where has[r] != 0; the level's Q draw slots
 * in draw order: read rid[q], mate uid[q] (-1: none), read symbol sym[q]
 * (0..n_sym-1); n_sweeps sweeps, draw t = i * Q + q taking U[t].  Out:
 * choice[n_sweeps * Q], kdraw[S] (draws per strain), cnt[S * n_sym] (draws per
 * strain and read symbol).  Returns 0, or -1 on an argument out of range. */
int oracle_urn_draws(int S, const double *a0, int n_reads, const double *ll, const unsigned char *has, int Q,
                     const int *rid, const int *uid, const int *sym, int n_sym, int n_sweeps, const double *U,
                     int *choice, long *kdraw, long *cnt) {
    if (S < 1 || n_reads < 1 || Q < 1 || n_sweeps < 0 || n_sym < 1) return -1;
    for (int q = 0; q < Q; q++)
        if (rid[q] < 0 || rid[q] >= n_reads || uid[q] < -1 || uid[q] >= n_reads || sym[q] < 0 || sym[q] >= n_sym) return -1;
    Strain *st = (Strain *)xmalloc(sizeof(Strain) * (size_t)S);
    ld *a = (ld *)xmalloc(sizeof(ld) * (size_t)S), *p = (ld *)xmalloc(sizeof(ld) * (size_t)S);
    double *prob = (double *)xmalloc(sizeof(double) * (size_t)S), *cp = (double *)xmalloc(sizeof(double) * (size_t)S);
    for (int s = 0; s < S; s++) {
        memset(&st[s], 0, sizeof(Strain));
        st[s].nreads = n_reads;
        st[s].rll = (ld *)xmalloc(sizeof(ld) * (size_t)n_reads);
        st[s].has = (unsigned char *)xmalloc((size_t)n_reads);
        for (int r = 0; r < n_reads; r++) {
            st[s].has[r] = has[r] != 0;
            st[s].rll[r] = has[r] ? (ld)ll[(long)s * n_reads + r] : 0;
        }
        a[s] = a0[s];
    }
    urn_draw_loop(st, S, a, rid, uid, Q, n_sweeps, U, choice, p, prob, cp);
    for (int s = 0; s < S; s++) kdraw[s] = 0;
    for (long i = 0; i < (long)S * n_sym; i++) cnt[i] = 0;
    for (long t = 0; t < (long)n_sweeps * Q; t++) {
        kdraw[choice[t]]++;
        cnt[(long)choice[t] * n_sym + sym[t % Q]]++;
    }
    for (int s = 0; s < S; s++) { free(st[s].rll); free(st[s].has); }
    free(st); free(a); free(p); free(prob); free(cp);
    return 0;
}

/* The same level through np_bayes_clustering itself (its own mt19937(1234)
 * stream): reads ent_rid[n_ent] with copy numbers ent_cn and one-symbol labels
 * ent_sym (index into "ACGT-="), mates as a CSR over the reads; ll / has / a0 as
 * above.  abund_out[S] receives the level's abundances (normalized urn
 * weights times the number of draw slots).  Returns 0, or -1 on bad input. */
int oracle_np_bayes_level(int S, const double *a0, int n_reads, const double *ll, const unsigned char *has, int n_ent,
                          const int *ent_rid, const int *ent_cn, const int *ent_sym, const int *mate_off,
                          const int *mate_idx, int n_sweeps, double *abund_out) {
    static char labs[6][2] = { "A", "C", "G", "T", "-", "=" };
    if (S < 1 || n_reads < 1 || n_ent < 1 || n_sweeps < 1) return -1;
    for (int r = 0; r < n_ent; r++)
        if (ent_rid[r] < 0 || ent_rid[r] >= n_reads || ent_cn[r] < 1 || ent_sym[r] < 0 || ent_sym[r] >= 6) return -1;
    Node node; memset(&node, 0, sizeof node); node.lab = labs[0];
    StrainVec sv; vec_init(sv);
    for (int s = 0; s < S; s++) {
        Strain st; strain_init(&st, 100, 0.01L, n_reads);
        for (int r = 0; r < n_reads; r++) { st.has[r] = has[r] != 0; st.rll[r] = has[r] ? (ld)ll[(long)s * n_reads + r] : 0; }
        st.abundance = a0[s];
        vec_push(st.path, &node);
        vec_push(sv, st);
    }
    RBVec reads; vec_init(reads);
    for (int r = 0; r < n_ent; r++) { RB b = { ent_rid[r], labs[ent_sym[r]], ent_cn[r] }; vec_push(reads, b); }
    ReadPairs rp; rp.n = n_reads; rp.mates = (IntVec *)xmalloc(sizeof(IntVec) * (size_t)n_reads);
    for (int r = 0; r < n_reads; r++) {
        vec_init(rp.mates[r]);
        for (int k = mate_off[r]; k < mate_off[r + 1]; k++) vec_push(rp.mates[r], mate_idx[k]);
    }
    ClusterCtx cx; memset(&cx, 0, sizeof cx); cx.rp = &rp;
    ld *ab = NULL;
    np_bayes_clustering(&cx, &sv, &reads, n_sweeps, &ab);
    for (int s = 0; s < S; s++) abund_out[s] = (double)ab[s];
    free(ab);
    for (int s = 0; s < S; s++) strain_free(&sv.v[s]);
    vec_free(sv); vec_free(reads);
    for (int r = 0; r < n_reads; r++) vec_free(rp.mates[r]);
    free(rp.mates);
    return 0;
}

#ifndef ORACLE_NO_MAIN
int main(int argc, char **argv) { return oracle_main(argc, argv); }
#endif
