/* C-ABI of libstraincall_hip.so -- the MI355X (gfx950) implementation of the
 * StrainCall hot path of homopolymer/RAMBL.
 *
 * The reference exposes this path only as a process (StrainCall argv -> FASTA on
 * stdout, /root/reference/StrainCall/StrainCall.cpp:972-1059, launched per region
 * by /root/reference/scripts/rambl.py:169-201).  Inside that process the path is
 * the sequence
 *
 *     PartialOrderGraph(gene_seq, reads)          StrainCall.cpp:1017
 *     pog->infer_strains(strains, read_pairs, 5000, e, tau, diff)   :1021
 *     pog->read_assign(strains, reads, read_pairs, 5000)            :1024
 *     sort by abundance, print                     :1027-1046
 *     pog->output_edge(cout)   (with -G)           :1050
 *
 * and this library is the drop-in for exactly that sequence: the caller (the
 * Python entry point rambl_amd/cli.py, or a cgo/JNI/ctypes binding written by a
 * maintainer) hands over what load_gene_seq and
 * load_mapping_reads produced (StrainCall.cpp:157-185, :480-670) as plain
 * arrays and receives strains, abundances, the -G dump and the per-level trace.
 *
 * Conventions: the caller owns every buffer; every function returns 0 on success
 * or a negative SC_ERR_* code and never throws; a context is bound to one HIP
 * device; sc_roi_submit may be called from one host thread at a time; up to
 * `stream_count` regions are in flight at once, as fibers on a few host threads
 * sized from the CPU quota of the rank (sc_host_plan), not one thread per region.
 * There is no CPU fallback: if no gfx950 device is present sc_ctx_create fails.
 */
#ifndef STRAINCALL_HIP_H
#define STRAINCALL_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_NO_DEVICE (-1)     /* no HIP device / wrong architecture */
#define SC_ERR_HIP (-2)           /* a HIP runtime call failed (see sc_last_error) */
#define SC_ERR_ARG (-3)           /* invalid argument / unknown handle */
#define SC_ERR_UNSUPPORTED (-4)   /* graph shape outside the device model (message in sc_last_error) */
#define SC_ERR_CAPACITY (-5)      /* caller buffer too small, or more than 128 live candidates */
#define SC_ERR_INTERNAL (-6)

typedef struct sc_ctx sc_ctx;

/* sc_parameter fields that reach the path (StrainCall.cpp:58-95) plus the three
 * literals of the reference's call sites (:1021,:1024 n=5000; budget 40000 at
 * NonparametricClustering.cpp:160,781; candidate cap 80 at :532). */
typedef struct sc_params {
    float error_rate;      /* -e */
    float tau;             /* -t */
    float diff_rate;       /* -d */
    int sweeps_cap;        /* 5000 */
    int draw_budget;       /* 40000 */
    int max_candidates;    /* 80 */
    int graph_only;        /* -G: build + dump the graph, no clustering */
    int want_trace;        /* keep the per-level strain/abundance trace */
    int want_timing;       /* time every sampler launch with HIP events on the region's stream (sc_stats) */
    int want_graph;        /* keep the -G text (sc_roi_graph_dump) and the threading tables of a full run too */
} sc_params;

typedef struct sc_stats {
    double graph_ms;          /* host graph build + flatten + upload */
    double cluster_ms;        /* level walk incl. kernels */
    double sampler_kernel_ms; /* sum of HIP-event times of the SAMPLE-mode launches */
    long sampler_launches;
    long sampler_read_copies; /* sum over SAMPLE launches of the read copies (draw slots) of the level */
    long level_launches;
    long draws;               /* categorical draws made on the device */
    long slow_draws;          /* of which needed the fp64 scan tier */
    long exact_draws;         /* of which resolved by the literal fp64 path */
    long sampler_strains;     /* sum over SAMPLE launches of the candidate count */
    long chain_passes;        /* window passes of the sampler chain (draws / passes = draws accepted per pass) */
    long chain_cycles;        /* shader cycles spent inside the urn chains */
    long chain_wall_ticks;    /* the same in 100 MHz ticks */
    long level_kernel_ticks;  /* 100 MHz ticks inside the level kernels (start of the kernel to its completion stamp) */
    long sampler_level_ticks; /* the part of it spent in sampler levels (one workgroup of k_level_sample each) */
    long xcd_levels[8];       /* level kernels that ran on each of the 8 XCDs (HW_REG_XCC_ID) */
    long msa_calls;
    int n_nodes, n_levels, n_unique_reads;
    long n_read_copies;
    double setup_ms;          /* the part of cluster_ms before the first level: uploads of the level-major arrays, edge support */
    double queue_ms;          /* from sc_roi_submit until a slot took the region */
    double place_ms;          /* the part of graph_ms spent waiting for one of the context's set-up places */
    double mailbox_ms;        /* set-up done, waiting for a resident workgroup to fall free (the part of cluster_ms after setup_ms) */
    double host_us[3];        /* host work between the levels, summed over the walk: [0] the level's parameters (log tables into the
                               * host-mapped block), [1] its results into the candidates' models + pruning, [2] candidate extension */
    double wake_us[2];        /* with several regions in flight, summed over the walk: [0] handing the levels to the level server, [1] from
                               * the server seeing a level's stamp until the region's fiber runs again */
    long kind_levels[17];     /* levels served by each variant of the level kernel: [0] no sampler (k_level); [1 + 2 * (NB - 1) + L]
                               * the sampler for NB = ceil(candidates / 16) register blocks, L = 1 weight rows in LDS, 0 in HBM */
} sc_stats;

/* Replaces process start-up; `device` is a HIP ordinal, `stream_count` the number of regions that walk their levels at a
 * time (with several, on resident level workers: at most 224 of them, and the context sets up to a quarter more regions up
 * meanwhile, so that a workgroup that finishes a region finds the next one ready).  Fails with SC_ERR_NO_DEVICE when there
 * is no GPU. */
int sc_ctx_create(int device, int stream_count, sc_ctx** ctx_out);
void sc_ctx_destroy(sc_ctx* ctx);
const char* sc_last_error(sc_ctx* ctx);
/* The message of one region (sc_last_error holds the context's latest, which may be another region's when several
 * fail side by side).  Valid until sc_roi_release. */
const char* sc_roi_error(sc_ctx* ctx, int handle);
/* Binds the calling thread, and the threads it starts afterwards, to the CPUs next to GPU `device` (local_cpulist of its
 * PCI device; what `numactl --cpunodebind` does for a rank).  Returns the number of CPUs, 0 when nothing was changed (topology
 * unknown, no such device, SC_NUMA_BIND=0).  sc_ctx_create places the context's own threads and host memory the same way
 * without moving its caller.  (No counterpart in the reference: rambl.py:190-194 leaves placement to the OS.) */
int sc_host_bind(int device);

/* Host threads a context with `stream_count` regions in flight starts: out[0] executor threads (they run the regions'
 * fibers), out[1] the level server (0 or 1; a context on resident level workers starts one more executor instead: its
 * executors watch the levels' completion stamps themselves), out[2] threads sc_aln_open inflates BGZF members on.  `cpus` = CPUs of the
 * host share (0: the cgroup quota / affinity mask of the process), divided by `local_world` ranks sharing it (0: the
 * environment's LOCAL_WORLD_SIZE, as torch.distributed.run sets it) -- rambl.py's Pool(cores) (scripts/rambl.py:190-194)
 * gives every region a process; here eight ranks on one host must fit its cores.  No device needed. */
int sc_host_plan(int stream_count, int local_world, double cpus, int* out);

/* Replaces `new PartialOrderGraph(gene_seq, reads)` + infer_strains + read_assign
 * + the sort (StrainCall.cpp:1017-1027).
 *   ref_bases[ref_len]            window substring of the gene (load_gene_seq)
 *   read_pos[i]                   0-based offset in the window (AlignRead<0>)
 *   cigar_text/cigar_off[n+1]     cropped CIGAR strings (AlignRead<1>)
 *   seq_text/seq_off[n+1]         cropped read bases (AlignRead<2>)
 *   read_copies[i]                copy number (AlignRead<4>)
 *   mate_idx/mate_off[n+1]        ReadPairs: mate uid (or -1) per copy of read i
 * Reads must be in the order load_mapping_reads emits them (StrainCall.cpp:610). */
int sc_roi_submit(sc_ctx* ctx, const char* ref_bases, int ref_len, const int* read_pos, const char* cigar_text,
                  const int* cigar_off, const char* seq_text, const int* seq_off, const int* read_copies,
                  const int* mate_idx, const int* mate_off, int n_reads, const sc_params* params, int* handle_out);
int sc_roi_wait(sc_ctx* ctx, int handle);

/* Strains in output order (abundance descending, libstdc++ sort order for ties,
 * StrainCall.cpp:1027).  seq_buf receives the ungapped sequences back to back
 * (Strain::plain_seq), seq_off[n_strains+1] their offsets. */
int sc_roi_result(sc_ctx* ctx, int handle, char* seq_buf, long seq_cap, int* seq_off, double* abundance,
                  int max_strains, int* n_strains);
/* Replaces pog->output_edge(cout) (PartialOrderGraph.cpp:318-337). */
int sc_roi_graph_dump(sc_ctx* ctx, int handle, char* buf, long cap, long* len_out);
/* Text of the reference's dormant debug blocks (NonparametricClustering.cpp:287-298,
 * :460-471), abundances printed with %.17g. */
int sc_roi_trace(sc_ctx* ctx, int handle, char* buf, long cap, long* len_out);
int sc_roi_stats(sc_ctx* ctx, int handle, sc_stats* out);
int sc_roi_release(sc_ctx* ctx, int handle);

/* Row a7 on its own: MultipleSequenceAlignmentSP<...>::align + MSA<>::get
 * (MultipleSequenceAlignmentSP.cpp:10-49, MultipleSequenceAlignment.hpp:59-70).
 * rows_out receives n rows of (*ncol_out) characters + NUL, back to back. */
int sc_msa_align(sc_ctx* ctx, const char* seq_text, const int* seq_off, int n, char* rows_out, long cap, int* ncol_out);

/* Row a16 on its own: number_of_reads_cover_nodes for every edge of a region
 * (PartialOrderGraph.cpp:1218-1244), in the edge order of the -G dump. */
int sc_roi_edge_support(sc_ctx* ctx, int handle, int* support, int cap, int* n_edges);

/* Row a5 on its own: the class tables of the read-threading kernels for a region
 * (the per-base M loop of PartialOrderGraph::build, PartialOrderGraph.cpp:129-177):
 * count[i*8+c] = reads whose base aligned to window position i is symbol c,
 * first_read[i*8+c] = the first such read (it creates the node), pool = the read ids
 * of every class back to back in class order, ascending inside a class.
 * symbols[8] receives the symbol of every code (0 = unused). */
int sc_roi_thread_tables(sc_ctx* ctx, int handle, int* count, int* first_read, int cls_cap, int* pool, long pool_cap,
                         char* symbols, int* n_cls, long* n_pool);

/* The other three tables of row a5, for tests: which read adds each edge, as the threading kernels return them before
 * the host stitches nodes and edges from them.  smin[i*8+c] = the first read whose first CIGAR operation is M and whose
 * first base lands in class (i, c); emin[i*8+c] = the first read whose last operation is M and whose last base lands
 * there; tmin[i*64 + cp*8 + c] = the first read with symbols cp, c on window positions i-1, i inside one M run or across two
 * adjacent M operations.  Absent entries are INT_MAX.  smin and emin hold *n_cls = glen*8 values, tmin 8 * *n_cls; kept for
 * a region submitted with graph_only or want_graph, as the tables of sc_roi_thread_tables are. */
int sc_roi_thread_edges(sc_ctx* ctx, int handle, int* smin, int* emin, int* tmin, int cls_cap, int* n_cls);

/* Row a16 on raw arrays, for tests: the edge-support kernel on a graph the caller states as CSR pools
 * (pool_ptr[n_nodes+1], pool_rid, pool_cn: the reads of every node with their copy numbers), node_is_end[n_nodes] and the
 * edges (edge_src[e] -> edge_dst[e]); node 0 is the source.  sorted = 1 promises pools in ascending read order (checked:
 * SC_ERR_ARG otherwise) and takes the kernel's binary searches, sorted = 0 its linear count.  support_out[n_edges].
 * Uploads, launches and copies back; nothing else. */
int sc_edge_support_tables(sc_ctx* ctx, int n_nodes, const int* pool_ptr, const int* pool_rid, const int* pool_cn,
                           const unsigned char* node_is_end, int n_edges, const int* edge_src, const int* edge_dst, int sorted,
                           int* support_out);

/* Row a14 on its own, for tests: one sampler level (the Polya-urn draws of np_bayes_clustering,
 * NonparametricClustering.cpp:230-249) through the production level kernel, on chosen inputs and
 * chosen uniforms.  S (2..128) strains with urn weights a0[S] and read log-likelihood rows
 * ll[s*n_reads + r], present where has[r] != 0; the level's n_ent entries (read ent_rid, copy number
 * ent_cn, one-symbol label ent_sym < 16, or 0xFF: no single symbol, drawn but not counted) start
 * at entry index e0 (the entries in front name other reads); mates as a CSR over the reads (mate_off[n_reads+1], mate_idx, -1: none); n_sweeps sweeps,
 * draw t taking U[t] (n_u >= n_sweeps * sum ent_cn <= 40000).  Out: kdraw[S] draws per strain,
 * cnt[S*16] draws per (strain, read symbol), out[6] = draws, draws of the fp64 scan tier, draws of
 * the literal tier, window passes, kernel variant, the pieces of the level that ran on a grid in front of it (LV_* bits).  Only on a context of one stream (SC_ERR_ARG
 * otherwise: resident level workers run the same level body). */
int sc_sample_level(sc_ctx* ctx, int S, const double* a0, int n_reads, const double* ll, const unsigned char* has,
                    int n_ent, int e0, const int* ent_rid, const int* ent_cn, const int* ent_sym, const int* mate_off,
                    const int* mate_idx, int n_sweeps, const double* U, int n_u, unsigned* kdraw, unsigned* cnt, long* out);

/* Row a13 on its own, for tests: the read log-likelihood update of one level (NonparametricClustering.cpp:343-391) and the
 * row copies in front of it (Strain.cpp:73-83), through the production level kernel and, where the level goes there, the
 * grid kernels in front of it -- no sampler, no hard update.  S (1..128) strains: strain s owns row slot[s] (distinct,
 * < 128) of the matrix and has the node label labels[lab_off[s] .. + lab_len[s]) and the log table lpt[s*K*K + a*K + b];
 * K symbols (6..16), code_N the code of N (-1: none, else 6..K-1).  ll[s*n_reads + r] are the strains' rows before the
 * level (every other row of the matrix starts as zeros), has[n_reads] the reads present.  The level's n_ent entries start
 * at entry index e0 (the entries in front name other reads): read ent_rid, label labels[ent_lab_off .. + ent_lab_len),
 * ent_first (0: the read occurred earlier in this level).  n_copy row copies copy_src[c] -> copy_dst[c] of the leading
 * copy_n cells run first; a destination is no other pair's destination and nobody's source.  S*K*K fits the level
 * kernel's log tables.  A label of one symbol may hold any code; every code of a longer label is below K (or code_N in a
 * strain's label), and so is every entry's once a strain's label is longer than one symbol.  SC_ERR_ARG otherwise, before
 * anything is launched, and on a context of more than one stream.  Out: ll_out[128*n_reads] the whole matrix,
 * has_out[n_reads], isnew_out[n_ent] (the entry's read was entered by this level), *done_out the pieces of the level that
 * ran on a grid (LV_* bits). */
int sc_update_level(sc_ctx* ctx, int S, const int* slot, const int* lab_off, const int* lab_len, int K, int code_N,
                    const double* lpt, int n_reads, const double* ll, const unsigned char* has, const unsigned char* labels,
                    int n_labels, int n_ent, int e0, const int* ent_rid, const int* ent_lab_off, const int* ent_lab_len,
                    const unsigned char* ent_first, int n_copy, const int* copy_src, const int* copy_dst, int copy_n,
                    double* ll_out, unsigned char* has_out, unsigned char* isnew_out, int* done_out);

/* Row a15 on its own, for tests: the hard update of one level (hard_clustering, NonparametricClustering.cpp:17-125) behind
 * the level's update, as every level in front of the first branching runs it: the level of sc_update_level with mode hard,
 * through the production level kernel and, where the level goes there, the grid kernels in front of it.  Everything
 * sc_update_level takes, with its checks, and: logpri[S] the strains' log priors (-inf is log 0; NaN and +inf are refused),
 * ent_cn[n_ent] >= 1 the entries' copy numbers, the mates as a CSR over the reads (mate_off[n_reads+1], mate_idx in
 * [-1, n_reads), -1: none).  Entry r yields ent_cn[r] draw slots, Q of them in all (1 .. 2^20).  In a level with any label of
 * more than one symbol every code of every entry's label is below K (the hard update walks each against every strain's);
 * a strain's single symbol may hold any code ("^" and "$" carry 0xFF), it then counts nowhere.  Out, beside what
 * sc_update_level returns (now behind the hard update: a mate not seen before has a zero in the rows of the level's
 * strains and is present): abund[S], subst[S*K*K], the responsibilities resp[s*Q + q], and the draw slots as the device
 * wrote them, qrid[Q], quid[Q], qcode[Q]. */
int sc_hard_level(sc_ctx* ctx, int S, const int* slot, const int* lab_off, const int* lab_len, int K, int code_N,
                  const double* lpt, const double* logpri, int n_reads, const double* ll, const unsigned char* has,
                  const unsigned char* labels, int n_labels, int n_ent, int e0, const int* ent_rid, const int* ent_cn,
                  const int* ent_lab_off, const int* ent_lab_len, const unsigned char* ent_first, const int* mate_off,
                  const int* mate_idx, int n_copy, const int* copy_src, const int* copy_dst, int copy_n, double* ll_out,
                  unsigned char* has_out, unsigned char* isnew_out, double* abund, double* subst, double* resp, int* qrid,
                  int* quid, unsigned char* qcode, int* done_out);

/* ---- rows a2-a4 on the host: the alignment file and a window's reads (rambl_amd/csrc/sc_aln_file.cpp, sc_ingest.cpp) ----------
 *
 * The reference shells out to samtools for every window (StrainCall.cpp:496 `view -q mq -F 1804 region`, :696
 * `mpileup -q mq -Q0 -A -r region`) and parses the text.  Here the file (SAM text, or BAM read natively: BGZF +
 * the record layout of the SAM specification, section 4) is read once and indexed by reference name. */
typedef struct sc_aln sc_aln;
typedef struct sc_reads sc_reads;

int sc_aln_open(const char* path, sc_aln** out);     /* on a parse error *out still carries the message */
/* The same, keeping the records of the named references only (n_names = 0: of none; n_names < 0: of all) while
 * sc_aln_ref_stats still answers for every reference of the file: a rank of a multi-GPU run opens the file once without
 * records to price the regions, and once with the names of its own shard (rambl_amd/stage5.py). */
int sc_aln_open_filtered(const char* path, const char* const* names, int n_names, sc_aln** out);
void sc_aln_close(sc_aln* aln);
const char* sc_aln_error(sc_aln* aln);
long sc_aln_records(sc_aln* aln);
/* alignments of one reference and the reference bases they cover: what a scheduler needs to price a region */
int sc_aln_ref_stats(sc_aln* aln, const char* gene, long* n_records, long* aligned_bases);
/* Every record of the file in file order, whatever its reference (the reads stage 4 extracts, extract_reads.py:46-112):
 * records [first, first + n) as lines "QNAME\tFLAG\tSEQ\tQUAL\n" (SAM columns 1, 2, 10, 11, as the file holds them) into
 * buf.  Stops early at a record that does not fit: *n_out records, *len_out bytes (SC_ERR_CAPACITY when not even the first
 * fits).  Needs a handle that kept all records (sc_aln_open). */
int sc_aln_walk(sc_aln* aln, long first, long n, char* buf, long cap, long* n_out, long* len_out);

/* What window_adjust reads out of the pileup of gene:P-Q (StrainCall.cpp:702-736): for position P+i, whether any
 * read covers it, and whether column 5 of its pileup line would hold a '+' (insertion) / a '-' or '*' (deletion) --
 * including the mapping-quality character after '^' that the reference mistakes for one.  Arrays of Q-P+1 bytes. */
int sc_aln_pileup_flags(sc_aln* aln, const char* gene, int P, int Q, int mq, unsigned char* covered,
                        unsigned char* has_ins, unsigned char* has_del);

/* load_mapping_reads (StrainCall.cpp:480-670) for the window gene:p0-p1: view filter, depth -> keep probability,
 * length / N / insertion filters, crop to the window, mt19937(1234) thinning (drawn only for reads that pass),
 * exact-duplicate collapse in (position, CIGAR, bases) order, mate table. */
int sc_aln_load_reads(sc_aln* aln, const char* gene, int p0, int p1, int mq, int rl, int max_ins, int max_depth,
                      sc_reads** out);
/* The packed arrays sc_roi_submit takes, owned by `reads` (valid until sc_reads_free); n_input = alignments the
 * view returned, depth = the integer mean depth the keep probability came from. */
int sc_reads_get(sc_reads* reads, int* n_reads, const int** pos, const char** cigar_text, const int** cigar_off,
                 const char** seq_text, const int** seq_off, const int** copies, const int** mate_idx,
                 const int** mate_off, long* n_input, int* depth);
void sc_reads_free(sc_reads* reads);

/* ---- rambl.py stage 1 on the device (rambl_amd/csrc/sc_depth.hip) --------------------------------------------
 *
 * /root/reference/scripts/coverage_all_samples.py:21-186 pipes `samtools depth <bams>` (per-base depth per file,
 * deleted and skipped bases not counted, flags 0x704 excluded) through awk (sum over the files), sort and
 * `bedtools merge -c 4 -o mean -d 10` (one-base records [p, p+1) merged while at most 10 uncovered bases separate
 * them; mean of the merged depths).  sc_depth_scan does the same from alignment files the library has read (one
 * kernel: the per-base depth never exists in HBM, a wavefront builds it for its reference in LDS):
 * intervals come back sorted by (reference index, start), 1-based inclusive, with the sum of the depths of their
 * covered positions and their number (mean = sum / n).  Returns SC_ERR_CAPACITY (with *n_intervals set) when `cap`
 * is too small.  samtools' per-file depth cap (8000) is not applied; parity at that tool boundary is unpinned.
 * Limits, checked before anything is launched (SC_ERR_ARG): 0 <= max_gap <= SC_DEPTH_MAX_GAP and no reference longer than
 * 2^30 bases -- the kernel keeps positions and "no position yet" (-2^30) in int and compares with max_gap + 1. */
#define SC_DEPTH_MAX_GAP ((1 << 30) - (1 << 24))
typedef struct sc_depth_stats {
    long cells;            /* reference bases scanned */
    long runs;             /* aligned runs (CIGAR M = X operations) */
    double extract_ms;     /* host: CIGAR walk of the records -> runs, on the rank's host threads (sc_depth_scan only) */
    double prepare_ms;     /* host: runs bucketed by reference into page-locked memory (+ start order inside long references) */
    double upload_ms;      /* HIP events: runs (8 bytes each) and the reference tables to the device */
    double kernel_ms;      /* HIP events: k_depth_fused (difference array in LDS -> depths -> intervals) */
} sc_depth_stats;
int sc_depth_scan(int device, sc_aln* const* alns, int n_alns, const char* const* ref_names, const int* ref_len, int n_refs,
                  int max_gap, int* iv_ref, int* iv_start, int* iv_end, long* iv_sum, int* iv_n, int cap, int* n_intervals,
                  sc_depth_stats* stats);
/* The same from bare runs: run i covers positions run_start[i]..run_end[i] (1-based, inclusive) of reference run_ref[i]. */
int sc_depth_scan_runs(int device, const int* ref_len, int n_refs, const int* run_ref, const int* run_start, const int* run_end,
                       long n_runs, int max_gap, int* iv_ref, int* iv_start, int* iv_end, long* iv_sum, int* iv_n, int cap,
                       int* n_intervals, sc_depth_stats* stats);

/* ---- rambl.py stage 4 on the device (rambl_amd/csrc/sc_align.hip) --------------------------------------------
 *
 * scripts/recluster_data_to_seed_otus.py:198-277 extracts the reads the gene-database BAMs mapped,
 * aligns them again with `bowtie2 --sensitive-local` to the seed OTUs and keeps what `samtools view -F1804` keeps.
 * sc_align_reads computes the exact optimum of bowtie2's --local scoring instead (match +2, mismatch -(2 + floor(4 *
 * min(Q,40) / 40)), a base outside ACGT -1, a gap of n -(5 + 3n), no gap within 4 rows of either read end), every seed on
 * both strands, ties to the lower seed index, then the forward strand, then the smaller end column on the seed, then the
 * smaller end row; traceback diagonal before D before I, extension before opening.
 *   seed_text/seed_off[n_seeds+1]     the seeds back to back (1..8192 bases each)
 *   read_text/qual_text/read_off[n+1] the reads as they were sequenced (1..512 bases each; QUAL Phred+33, NULL: Q40)
 * Out, per read: as = best score (whether or not it is valid); xs = best valid score of any other (seed, strand), -1 when
 * none; and where as >= 20 + 8 ln(length) (in double): seed (else -1), strand (1: the reverse complement of the read
 * aligned), pos (1-based on the seed), nm, and n_cigar operations at cigar[read * cigar_stride] in BAM form (length << 4 |
 * op; M 0, I 1, D 2, S 4).  cigar_stride >= longest read / 2 + 4 always suffices.  Reads or seeds outside the limits:
 * SC_ERR_UNSUPPORTED; the message of the calling thread's last failure is in sc_align_error(). */
typedef struct sc_align_stats {
    double upload_ms;      /* HIP events: seeds and reads to the device */
    double score_ms;       /* HIP events: k_sw_score, every (read, seed, strand) tile */
    double trace_ms;       /* HIP events: k_sw_trace, one window per aligned read */
    double total_ms;       /* wall time of the call, host packing included */
    long score_cells;      /* DP cells of the score pass: sum of 2 * read length * total seed length */
    long trace_cells;      /* DP cells the traceback pass swept (its column blocks recompute from the window start) */
    long n_traced;         /* reads that aligned */
} sc_align_stats;
int sc_align_reads(int device, const char* seed_text, const long* seed_off, int n_seeds, const char* read_text, const char* qual_text,
                   const long* read_off, int n_reads, int* as, int* xs, int* seed, int* strand, int* pos, int* nm, unsigned* cigar,
                   int cigar_stride, int* n_cigar, sc_align_stats* stats);
const char* sc_align_error(void);

/* ---- the per-sample gene profile on the device (rambl_amd/csrc/sc_profile.hip and sc_profile_*.hpp) -------------
 *
 * scripts/per_sample_gene_profile_fast.py:80-153 searches a sample's read segments in the assembled genes with
 * makeblastdb and `blastn -reward 1 -penalty -2` and turns the XML into a CSV with bigBlastParser and sqlite3.
 * sc_profile_hits computes, for every (segment, gene), the exact optimum of that scoring instead (match +1, mismatch and
 * any base outside ACGT -2, a gap of n bases -2.5 n, local), the better of the two strands (ties: forward, then the
 * smaller end column on the gene, then the smaller end row), the alignment traced back from that cell diagonal before
 * gap-in-segment before gap-in-gene, and E = ka_k * m * n * exp(-ka_lambda * S) with m the segment length and n the sum of
 * the gene lengths.  No word-size seeding, no effective-length correction, no cap on targets.
 *   gene_text/gene_off[n_genes+1]   the genes back to back (1..8192 bases each)
 *   seg_text/seg_off[n_segs+1]      the segments as stored (1..512 bases each)
 * Out: the hits with 100 * identity / align_len >= min_identity_pct and E <= max_evalue, sorted by (segment, gene):
 * strand (1: the reverse complement of the segment aligned), raw score (may be x.5), identity (columns with equal ACGT
 * bases), align_len (columns), query from/to (1-based on the segment as given), hit from/to (1-based on the gene; from > to
 * on the reverse strand, as blastn prints it), E.  More than `cap` hits: SC_ERR_CAPACITY with *n_hits set to a capacity
 * that suffices.  Lengths outside the limits: SC_ERR_UNSUPPORTED; the message of the calling thread's last failure is in
 * sc_profile_error(). */
typedef struct sc_profile_stats {
    double upload_ms;      /* HIP events: genes and segments to the device */
    double score_ms;       /* HIP events: k_bl_score, every (segment, gene, strand) tile */
    double trace_ms;       /* HIP events: k_bl_trace, one window per (segment, gene) whose score passes the E-value */
    double total_ms;       /* wall time of the call, host packing included */
    long score_cells;      /* DP cells of the score pass: sum of 2 * segment length * total gene length */
    long trace_cells;      /* DP cells the traceback pass swept */
    long n_tiles;          /* (segment, gene, strand) tiles of the score pass */
    long n_candidates;     /* tiles whose best score passes the E-value threshold */
    long n_traced;         /* (segment, gene) pairs traced back */
    long n_hits;           /* hits that pass both thresholds */
} sc_profile_stats;
int sc_profile_hits(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                    int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg, int* hit_gene,
                    int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto, int* hfrom, int* hto,
                    double* evalue, long cap, long* n_hits, sc_profile_stats* stats);
const char* sc_profile_error(void);

/* The seeded mode of the gene profile: the same hits as sc_profile_hits, row for row, from the (segment, gene) pairs that
 * share an exact k-mer only.  The reference never scores every pair either: its `blastn -word_size 22`
 * (scripts/per_sample_gene_profile_fast.py:94-117) extends from exact word hits -- but a 22-mer loses hits, and the k here
 * does not.  A hit that passes both thresholds has i identity columns and m others with i <= segment length,
 * 100.0 * i / (i + m) >= min_identity_pct and 2 i - 4 m >= the least passing doubled score; the identity columns fall into
 * at most m + 1 diagonal runs, so one run has ceil(i / (m + 1)) columns, a k-mer common to the gene and the segment on the
 * hit's strand.  sc_profile_seed_length returns the least such bound over the given segment lengths that can pass at all
 * (gene_bases: the sum of the gene lengths), at most 16 (2 bits per base in 32), and 0 where the bound is below 11 or no
 * length can pass: the call then scores the full product as sc_profile_hits does (seed_k == 0).  *lossless_k (may be
 * null): the bound before both clamps.  Lengths outside 1..512: SC_ERR_UNSUPPORTED (negative).
 * A pair is the unit: when either strand shares a k-mer both strands of the pair are scored, since the better strand is
 * chosen before the filters.  The genes' k-mers (forward strand, inside one gene, ACGT only) are indexed per call
 * (DESIGN.md §8.10). */
typedef struct sc_profile_seed_stats {
    double upload_ms, score_ms, trace_ms, total_ms;      /* as in sc_profile_stats; score_ms of the pairs' tiles only */
    long score_cells;      /* sum of 2 * segment length * gene length over the scored pairs (seed_k == 0: as sc_profile_stats) */
    long trace_cells;
    long n_tiles;          /* 2 * n_pairs (seed_k == 0: the full product) */
    long n_candidates, n_traced, n_hits;
    int seed_k;            /* the k-mer length of the call; 0: ran unseeded */
    long n_gene_kmers;     /* k-mers of the genes in the index (one per window, repeats included) */
    long n_pairs;          /* (segment, gene) pairs that share a k-mer on either strand */
    double index_ms;       /* HIP events: the k-mer keys and their sort */
    double lookup_ms;      /* HIP events: counting and filling the pair list, the host's scan between them included */
} sc_profile_seed_stats;
int sc_profile_hits_seeded(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                           int n_segs, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k, int* hit_seg,
                           int* hit_gene, int* hit_strand, double* hit_score, int* identity, int* align_len, int* qfrom, int* qto,
                           int* hfrom, int* hto, double* evalue, long cap, long* n_hits, sc_profile_seed_stats* stats);
int sc_profile_seed_length(const int* seg_len, int n_segs, long gene_bases, double min_identity_pct, double max_evalue, double ka_lambda,
                           double ka_k, int* lossless_k);

/* The counts mode of the gene profile: the table of blastout2abundance.cpp:70-196 over the hits of
 * sc_profile_hits without the hit list.  Per (segment, gene) the better strand is picked on the device; per read (a set
 * of segments: seg_read[n_segs] holds one read index in 0..n_reads-1 per segment) the pairs are ordered by
 * E6 = strtod(sprintf("%.6g", E)), the E-value as the hit CSV holds it, and only the pairs of the read's smallest E6 are
 * traced back; when none of them has 100 * identity / align_len >= min_identity_pct the read moves to its next E6, and a
 * read with no E6 left counts nowhere.  A pair counts only with E <= max_evalue and E6 <= max_evalue.  Among the read's
 * kept hits the genes hit most often share the read.
 * Out: the distinct triples (gene, times_hit, number of such genes) in ascending order with the number of reads behind
 * each; the read's share of the gene is times_hit / number_of_such_genes.  More than `cap` triples: SC_ERR_CAPACITY with
 * *n_out set to the number that suffices.
 *   seeded      not 0: score only the pairs that share a k-mer, k from the lengths of all the call's segments; the genes
 *               are indexed once per call
 *   cand_room   the candidate records (one per passing tile) held on the device at a time; 0: the library's default.  The
 *               segments go through in stretches of whole reads that fit (a read alone gets the room it needs).
 * Limits and messages as sc_profile_hits; besides, bits(n_genes) * 2 + bits(most segments in a read) may not exceed 64. */
typedef struct sc_profile_count_stats {
    double upload_ms, score_ms;
    double trace_ms;       /* HIP events: the rounds -- selecting a group per read, k_bl_trace, the identity test, the reads' move */
    double total_ms;
    long score_cells, trace_cells, n_tiles, n_candidates;
    long n_traced;         /* (segment, gene) pairs actually traced back */
    long n_hits;           /* traced pairs that pass the identity threshold */
    int seed_k;
    long n_gene_kmers;     /* of the one index of the call */
    long n_pairs;
    double index_ms, lookup_ms;
    int n_rounds;          /* trace rounds, summed over the stretches */
    int n_stretches;
    long n_reads_counted;  /* reads that count somewhere */
    double select_ms;      /* HIP events: strand pick, E6 ranks and the two sorts */
    double count_ms;       /* HIP events: the reads' triples, their sort and reduction */
} sc_profile_count_stats;
int sc_profile_counts(int device, const char* gene_text, const long* gene_off, int n_genes, const char* seg_text, const long* seg_off,
                      int n_segs, const int* seg_read, int n_reads, double min_identity_pct, double max_evalue, double ka_lambda,
                      double ka_k, int seeded, long cand_room, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap,
                      long* n_out, sc_profile_count_stats* stats);
/* A cohort against one resident gene index.  sc_profile_index_create packs the genes (limits and messages
 * as sc_profile_counts: 1..8192 bases each, checked here) and copies them to `device`, where they stay until
 * sc_profile_index_free.  The index also keeps, from call to call, the sorted k-mer keys of every seed length a call has
 * needed so far (k is 11..16: at most six sets, each built by the first call that needs it) and every array a call sets
 * aside on the device, grown when a call needs more.  One call at a time per index: the calls share those arrays.
 * sc_profile_index_info: the number of genes, their bases, and the cached seed lengths ascending (cached_k: room for 6);
 * every out pointer may be null.
 * sc_profile_index_counts is sc_profile_counts over the reads of several samples at once: read_sample[n_reads] holds the
 * sample (0..n_samples-1, n_samples in 1..65536) of every read and is non-decreasing -- the samples come one after the
 * other; a sample may have no read.  Anything else: SC_ERR_ARG.  Out: the distinct rows (sample, gene, times_hit, number of
 * such genes) in ascending order with the number of reads behind each.  The rows of one sample are exactly the triples
 * sc_profile_counts returns for that sample's segments alone with the same genes, thresholds and `seeded`: E depends on
 * the segment's length and the genes' bases only, the order by E6 is an order whatever other lengths the call holds, and
 * the seed length, taken from all the call's lengths, is a lossless bound for each of them.  Reads of different samples
 * are different reads; stretches (cand_room) are not cut where a sample ends.  Of the statistics only seed_k may differ
 * from the per-sample calls'.
 *   n_index_builds  key sets this call built: 0 when its k was cached or it ran unseeded
 *   n_allocs        device allocations this call made: 0 when a call that fitted before is repeated */
typedef struct sc_profile_index sc_profile_index;
typedef struct sc_profile_cohort_stats {
    sc_profile_count_stats counts;     /* summed over the call's stretches, as sc_profile_counts fills it */
    int n_samples;
    int n_index_builds;
    long n_allocs;
} sc_profile_cohort_stats;
int sc_profile_index_create(int device, const char* gene_text, const long* gene_off, int n_genes, sc_profile_index** index);
int sc_profile_index_info(const sc_profile_index* index, int* n_genes, long* gene_bases, int* n_cached_k, int* cached_k);
int sc_profile_index_counts(sc_profile_index* index, const char* seg_text, const long* seg_off, int n_segs, const int* seg_read, int n_reads,
                            const int* read_sample, int n_samples, double min_identity_pct, double max_evalue, double ka_lambda, double ka_k,
                            int seeded, long cand_room, int* out_sample, int* out_gene, int* out_times, int* out_share, long* out_reads, long cap,
                            long* n_out, sc_profile_cohort_stats* stats);
void sc_profile_index_free(sc_profile_index* index);
/* E6 of a segment of L bases with doubled raw score score2 against gene_bases gene bases; no device is touched. */
double sc_profile_evalue6(int L, long gene_bases, int score2, double ka_lambda, double ka_k);

/* ---- genus assignment of gene sequences on the device (rambl_amd/csrc/sc_taxa.hip) ---------------
 *
 * scripts/per_sample_gene_profile_fast.py:223-246 and scripts/per_sample_taxon_profile.py:47-52 run the RDP classifier, a
 * Java program, on the assembled genes.  These entry points compute RDP's stated rule instead -- naive Bayes over 8-mers
 * with bootstrap trials -- under a contract of this project's own: parity with RDP's output is not claimed.
 *   words     2 bits per base (A C G T/U = 0 1 2 3, either case), first base most significant; a window with any other
 *             character is no word; a sequence's word list is its words in order, repeats included
 *   training  n(w), m_g(w): the sequences (of genus g) that hold w; P_w = (n(w) + 0.5) / (N + 1),
 *             P(w|g) = (m_g(w) + P_w) / (M_g + 1), cell q[w * G + g] = llrint(log2(P(w|g)) * 1024) computed in fp64
 *   score     the sum of q over a query's word list (forward strand only); the largest wins, the lowest genus on a tie
 *   trials    trial t draws D = max(W / 8, 5) positions of the W-word list, draw j at (hi32(z) * W) >> 32 with
 *             z = splitmix64's finaliser of (seed ^ key) + (t * 65536 + j + 1) * 0x9E3779B97F4A7C15; key is per query
 * Limits: 1..16384 genera, 1..2^24 training sequences of at most 2^24 bases and 2^32 in all, queries of 1..8192 bases,
 * 1..1024 trials;
 * outside them SC_ERR_UNSUPPORTED.  The message of the calling thread's last failure is in sc_taxa_error().
 * grid_cap bounds the blocks of every launch of a call (0: the library's own bound). */
typedef struct sc_taxa_model sc_taxa_model;
typedef struct sc_taxa_stats {
    double upload_ms;      /* HIP events: sequences (train) or word lists and keys (classify) to the device */
    double words_ms;       /* HIP events: k_taxa_words (train only) */
    double table_ms;       /* HIP events: k_taxa_table (train only) */
    double score_ms;       /* HIP events: k_taxa_score and k_taxa_pick (classify only) */
    double total_ms;       /* wall time of the call, host packing included */
    long n_seqs;           /* training sequences, or queries */
    long n_words;          /* train: distinct (sequence, word) pairs counted; classify: words of all queries' lists */
    long n_genera;
    long table_bytes;      /* the model's table on the device: 65536 * n_genera * 4 */
} sc_taxa_stats;
/* seq_genus[n_seqs]: the genus index (0..n_genera-1) of every training sequence; a genus may have none.  keep_counts not 0:
 * the model also keeps m as it stood before it became the table (as much memory again), for sc_taxa_model_counts. */
int sc_taxa_train(int device, const char* seq_text, const long* seq_off, int n_seqs, const int* seq_genus, int n_genera, int grid_cap,
                  int keep_counts, sc_taxa_model** model, sc_taxa_stats* stats);
/* Out per query: best_genus (-1 for a query without a word: it has no trials either), trial_winner[n_queries * n_trials],
 * n_words (W). */
int sc_taxa_classify(const sc_taxa_model* model, const char* query_text, const long* query_off, int n_queries,
                     const unsigned long long* query_key, unsigned long long seed, int n_trials, int grid_cap, int* best_genus,
                     int* trial_winner, int* n_words, sc_taxa_stats* stats);
/* Read-backs for tests and diagnostics, 65536 values each: a genus' m with the model's n (SC_ERR_UNSUPPORTED unless the
 * model was trained with keep_counts: the table replaces m in place), and its column of the table. */
int sc_taxa_model_counts(const sc_taxa_model* model, int genus, unsigned* m_out, unsigned* n_out);
int sc_taxa_model_table(const sc_taxa_model* model, int genus, int* q_out);
void sc_taxa_free(sc_taxa_model* model);
const char* sc_taxa_error(void);
/* The word-list position of draw `draw` of trial `trial` for a list of W words (-1 when W < 1); no device is touched. */
long sc_taxa_draw(unsigned long long seed, unsigned long long key, int trial, int draw, int W);

/* ---- gene against gene on the device: exact edit distances and the pairs within an identity (rambl_amd/csrc/sc_pairs.hip,
 * DESIGN.md §8.16) -------------------------------------------------------------------------------------------------------
 *
 * The reference has no counterpart that runs (its strain_identity is dead code); the contract is this project's own.
 *   distance  ed(a, b): the unit-cost edit distance (substitution, insertion, deletion 1 each) of the two whole sequences, no
 *             free end gaps; A C G T compared in either case, every other byte matches nothing, itself included
 *   bound     a difference rate is the rational diff_num / diff_den (97 % identity: 3 / 100; 0 <= diff_num <= diff_den);
 *             bound(a, b) = (max(|a|, |b|) * diff_num) / diff_den in 64-bit integer division; a pair qualifies iff
 *             ed(a, b) <= bound(a, b).  No floating point takes part.
 *   gene_text/gene_off[n_genes+1]   the genes back to back, 1..2048 bases each: an empty gene is SC_ERR_ARG, a longer one
 *             SC_ERR_UNSUPPORTED; the message of the calling thread's last failure is in sc_pairs_error()
 * sc_gene_distances: dist_out[p] = ed(gene pair_a[p], gene pair_b[p]) for n_pairs arbitrary index pairs (a == b allowed).
 * sc_gene_pairs: every qualifying pair a < b (indices as the caller numbers the genes) with its distance, sorted by (a, b),
 * the same on every call; pairs whose lengths differ by more than the bound are never scored.  More than `cap` pairs:
 * SC_ERR_CAPACITY with *n_pairs set to the number that suffices.
 * sc_pairs_widths: the words-per-pattern W the kernel is built for, ascending (a pattern of up to 64 W bases runs at the
 * least listed W that holds it); returns their number and fills the first `cap`.  No device is touched.
 * stats (may be null) receives the first n_stats of the SC_PAIRS_N_STATS slots below. */
#define SC_PAIRS_STAT_UPLOAD_MS 0       /* HIP events: genes and tiles to the device */
#define SC_PAIRS_STAT_KERNEL_MS 1       /* HIP events: k_pairs, every width class */
#define SC_PAIRS_STAT_TOTAL_MS 2        /* wall time of the call, host packing included */
#define SC_PAIRS_STAT_TILES 3           /* tiles: a pattern gene with up to 64 text genes */
#define SC_PAIRS_STAT_PAIRS_SCORED 4    /* pairs that went through the DP */
#define SC_PAIRS_STAT_PAIRS_SKIPPED 5   /* sc_gene_pairs: pairs a < b left out by their lengths alone */
#define SC_PAIRS_STAT_WORD_STEPS 6      /* 64-row block steps: text bases * pattern words, summed over the scored pairs */
#define SC_PAIRS_N_STATS 7
int sc_gene_distances(int device, const char* gene_text, const long* gene_off, int n_genes, const int* pair_a, const int* pair_b,
                      long n_pairs, int* dist_out, double* stats, int n_stats);
int sc_gene_pairs(int device, const char* gene_text, const long* gene_off, int n_genes, int diff_num, int diff_den, int* pair_a,
                  int* pair_b, int* pair_dist, long cap, long* n_pairs, double* stats, int n_stats);
int sc_pairs_widths(int* widths, int cap);
const char* sc_pairs_error(void);

/* ---- a sample's reads mapped to the gene database on the device (rambl_amd/csrc/sc_map.hip) --------------
 *
 * scripts/get_sra_and_mapping.py:49-90 runs `bowtie2 --local -x <gene database>` and `samtools view -F4 -bht`, sort and index
 * per sample.  Here a read's candidate genes come from k-mer votes, and the alignment is sc_align_reads' (§8.7) over them:
 *   index       every window of seed_k bases (11..16) inside one gene, forward strand, ACGT only, is a key (code, gene); sorted
 *   votes       v(r, g, s) = the windows of read r on strand s (1: its reverse complement), ACGT only, whose k-mer occurs in
 *               gene g at least once; a k-mer whose run in the index has more than max_occ entries casts no vote;
 *               v(r, g) = max over the strands
 *   candidates  the genes with v(r, g) >= min_votes; when max_cand > 0 only the max_cand with the largest v, ties to the lower
 *               gene index (max_cand == 0: all)
 *   result      what sc_align_reads returns for r against its candidates in ascending gene order, `gene` being the index in
 *               the database; a read without candidates has as 0, xs -1, gene -1
 * Limits: reads of 1..512 bases, genes of 1..8192 bases, at most 1048575 genes, max_occ >= 1, max_cand >= 0, min_votes >= 1;
 * anything else is SC_ERR_ARG or SC_ERR_UNSUPPORTED before any kernel is launched, with the message of the calling thread's
 * last failure in sc_map_error().  The genes and their keys stay on the device of the index; one call at a time runs on an
 * index.  Reads go through in stretches whose pairs fit pair_room (0: the library's default; a read that needs more on its
 * own gets it); no result depends on the stretches. */
typedef struct sc_map_index sc_map_index;
struct sc_map_stats {
    double index_ms;       /* HIP events: k_seed_keys and the sort, when the index was made */
    double votes_ms;       /* HIP events: k_map_votes, the counting pass and the filling pass of every stretch */
    double score_ms;       /* HIP events: k_sw_score_pairs, both strands of every (read, candidate) pair */
    double trace_ms;       /* HIP events: k_sw_trace, one window per mapped read */
    double total_ms;       /* wall time of the call, host packing included */
    long n_keys;           /* keys of the index */
    long n_windows;        /* ACGT windows of the reads, both strands counted, whose k-mer was looked up */
    long n_skipped;        /* of those, the windows whose run has more than max_occ entries */
    long n_pairs;          /* (read, candidate) pairs */
    long score_cells;      /* DP cells of the score pass: sum of 2 * read length * gene length over the pairs */
    long trace_cells;      /* DP cells the traceback pass swept */
    long n_traced;         /* reads that mapped */
    long n_stretches;      /* stretches the reads went through in */
};
typedef struct sc_map_stats sc_map_stats;
/* get_sra_and_mapping.py:49-90, `bowtie2-build`: the genes to `device`, their keys made and sorted there. */
int sc_map_index_create(int device, const char* gene_text, const long* gene_off, int n_genes, int seed_k, sc_map_index** index);
/* get_sra_and_mapping.py:49-90: what an index holds (any pointer may be null). */
int sc_map_index_info(const sc_map_index* index, int* n_genes, long* gene_bases, int* seed_k, long* n_keys, double* index_ms);
void sc_map_index_free(sc_map_index* index);
/* get_sra_and_mapping.py:49-90, `bowtie2 --local`: per read as, xs, gene, strand, pos, nm and the CIGAR as sc_align_reads
 * returns them, and n_cand = the number of its candidates. */
int sc_map_reads(sc_map_index* index, const char* read_text, const char* qual_text, const long* read_off, int n_reads, int max_occ,
                 int max_cand, int min_votes, long pair_room, int* as, int* xs, int* gene, int* strand, int* pos, int* nm,
                 unsigned* cigar, int cigar_stride, int* n_cigar, int* n_cand, sc_map_stats* stats);
/* get_sra_and_mapping.py:49-90, a test and diagnostic entry: every read's candidates through the same two kernels, read r's at
 * [cand_off[r], cand_off[r + 1]) in ascending gene order with the votes of both strands.  More than `cap`: SC_ERR_CAPACITY
 * with *n_cand set to the number that suffices. */
int sc_map_candidates(sc_map_index* index, const char* read_text, const long* read_off, int n_reads, int max_occ, int max_cand,
                      int min_votes, long* cand_off, int* cand_gene, int* cand_fw, int* cand_rc, long cap, long* n_cand);
/* get_sra_and_mapping.py:49-90: the genes one pass of the vote kernel counts in LDS and the most votes a pair can have. */
int sc_map_limits(int* range_genes, int* max_votes);
const char* sc_map_error(void);

#ifdef __cplusplus
}
#endif
#endif
