"""ctypes binding of libstraincall_hip.so (include/straincall_hip.h).

There is no CPU fallback: importing this module fails loudly when the HIP
library has not been built, and `Context()` fails when no gfx950 device exists.

The ABI is stated once, in ENTRIES (one row per function of the header) and the Structure mirrors above it;
tests/test_capi_table.py holds both against the header, declaration by declaration and member by member.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstraincall_hip.so")

SC_OK = 0
ERRORS = dict(zip(range(-1, -7, -1), ("SC_ERR_NO_DEVICE", "SC_ERR_HIP", "SC_ERR_ARG", "SC_ERR_UNSUPPORTED", "SC_ERR_CAPACITY", "SC_ERR_INTERNAL")))
SC_ERR_NO_DEVICE, SC_ERR_HIP, SC_ERR_ARG, SC_ERR_UNSUPPORTED, SC_ERR_CAPACITY, SC_ERR_INTERNAL = ERRORS


class ScParams(C.Structure):
    _fields_ = [("error_rate", C.c_float), ("tau", C.c_float), ("diff_rate", C.c_float),
                ("sweeps_cap", C.c_int), ("draw_budget", C.c_int), ("max_candidates", C.c_int),
                ("graph_only", C.c_int), ("want_trace", C.c_int), ("want_timing", C.c_int), ("want_graph", C.c_int)]


class Stats(C.Structure):
    """The statistics structs of the header; the derived mirrors below state the header's flat member lists by concatenation."""

    def as_dict(self):
        return {k: (list(getattr(self, k)) if issubclass(t, C.Array) else getattr(self, k)) for k, t in self._fields_}


class ScStats(Stats):
    _fields_ = [("graph_ms", C.c_double), ("cluster_ms", C.c_double), ("sampler_kernel_ms", C.c_double),
                ("sampler_launches", C.c_long), ("sampler_read_copies", C.c_long), ("level_launches", C.c_long), ("draws", C.c_long),
                ("slow_draws", C.c_long), ("exact_draws", C.c_long), ("sampler_strains", C.c_long), ("chain_passes", C.c_long), ("chain_cycles", C.c_long), ("chain_wall_ticks", C.c_long), ("level_kernel_ticks", C.c_long), ("sampler_level_ticks", C.c_long), ("xcd_levels", C.c_long * 8), ("msa_calls", C.c_long), ("n_nodes", C.c_int), ("n_levels", C.c_int),
                ("n_unique_reads", C.c_int), ("n_read_copies", C.c_long), ("setup_ms", C.c_double), ("queue_ms", C.c_double), ("place_ms", C.c_double), ("mailbox_ms", C.c_double), ("host_us", C.c_double * 3), ("wake_us", C.c_double * 2), ("kind_levels", C.c_long * 17)]


class ScDepthStats(Stats):
    _fields_ = [("cells", C.c_long), ("runs", C.c_long), ("extract_ms", C.c_double), ("prepare_ms", C.c_double),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class ScAlignStats(Stats):
    _fields_ = [("upload_ms", C.c_double), ("score_ms", C.c_double), ("trace_ms", C.c_double), ("total_ms", C.c_double),
                ("score_cells", C.c_long), ("trace_cells", C.c_long), ("n_traced", C.c_long)]


class ScProfileStats(Stats):
    _fields_ = [("upload_ms", C.c_double), ("score_ms", C.c_double), ("trace_ms", C.c_double), ("total_ms", C.c_double),
                ("score_cells", C.c_long), ("trace_cells", C.c_long), ("n_tiles", C.c_long), ("n_candidates", C.c_long),
                ("n_traced", C.c_long), ("n_hits", C.c_long)]


class ScProfileSeedStats(Stats):
    _fields_ = ScProfileStats._fields_ + [("seed_k", C.c_int), ("n_gene_kmers", C.c_long), ("n_pairs", C.c_long),
                                          ("index_ms", C.c_double), ("lookup_ms", C.c_double)]


class ScProfileCountStats(Stats):
    _fields_ = ScProfileSeedStats._fields_ + [("n_rounds", C.c_int), ("n_stretches", C.c_int), ("n_reads_counted", C.c_long),
                                              ("select_ms", C.c_double), ("count_ms", C.c_double)]


class ScProfileCohortStats(Stats):
    """The header nests a sc_profile_count_stats as `counts`; the mirror holds its members flat, under their own names."""
    _fields_ = ScProfileCountStats._fields_ + [("n_samples", C.c_int), ("n_index_builds", C.c_int), ("n_allocs", C.c_long)]


class ScTaxaStats(Stats):
    _fields_ = [("upload_ms", C.c_double), ("words_ms", C.c_double), ("table_ms", C.c_double), ("score_ms", C.c_double), ("total_ms", C.c_double),
                ("n_seqs", C.c_long), ("n_words", C.c_long), ("n_genera", C.c_long), ("table_bytes", C.c_long)]


class ScMapStats(Stats):
    _fields_ = [("index_ms", C.c_double), ("votes_ms", C.c_double), ("score_ms", C.c_double), ("trace_ms", C.c_double), ("total_ms", C.c_double),
                ("n_keys", C.c_long), ("n_windows", C.c_long), ("n_skipped", C.c_long), ("n_pairs", C.c_long), ("score_cells", C.c_long),
                ("trace_cells", C.c_long), ("n_traced", C.c_long), ("n_stretches", C.c_long)]


class StrainCallError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d)%s" % (ERRORS.get(code, "error"), code, (": " + msg) if msg else ""))
        self.code = code


# ---- the prototype table: (name, return type, argument types) of every function the header declares, in its order

_i, _l, _d, _u64, _s, _vp = C.c_int, C.c_long, C.c_double, C.c_ulonglong, C.c_char_p, C.c_void_p      # _vp: a pointer to one of the opaque structs
_ip, _lp, _dp, _up, _bp, _u64p = (C.POINTER(t) for t in (C.c_int, C.c_long, C.c_double, C.c_uint, C.c_ubyte, C.c_ulonglong))
_vpp, _sp, _ipp = C.POINTER(_vp), C.POINTER(_s), C.POINTER(_ip)
_HITS = [_i, _s, _lp, _i, _s, _lp, _i, _d, _d, _d, _d, _ip, _ip, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _ip, _dp, _l, _lp]      # sc_profile_hits*, up to the statistics
_INTERVALS = [_ip, _ip, _ip, _lp, _ip, _i, _ip, C.POINTER(ScDepthStats)]                                                     # sc_depth_scan*, from iv_ref on

ENTRIES = [
    ("sc_ctx_create", _i, [_i, _i, _vpp]),
    ("sc_ctx_destroy", None, [_vp]),
    ("sc_last_error", _s, [_vp]),
    ("sc_roi_error", _s, [_vp, _i]),
    ("sc_host_bind", _i, [_i]),
    ("sc_host_plan", _i, [_i, _i, _d, _ip]),
    ("sc_roi_submit", _i, [_vp, _s, _i, _ip, _s, _ip, _s, _ip, _ip, _ip, _ip, _i, C.POINTER(ScParams), _ip]),
    ("sc_roi_wait", _i, [_vp, _i]),
    ("sc_roi_result", _i, [_vp, _i, _s, _l, _ip, _dp, _i, _ip]),
    ("sc_roi_graph_dump", _i, [_vp, _i, _s, _l, _lp]),
    ("sc_roi_trace", _i, [_vp, _i, _s, _l, _lp]),
    ("sc_roi_stats", _i, [_vp, _i, C.POINTER(ScStats)]),
    ("sc_roi_release", _i, [_vp, _i]),
    ("sc_msa_align", _i, [_vp, _s, _ip, _i, _s, _l, _ip]),
    ("sc_roi_edge_support", _i, [_vp, _i, _ip, _i, _ip]),
    ("sc_roi_thread_tables", _i, [_vp, _i, _ip, _ip, _i, _ip, _l, _s, _ip, _lp]),
    ("sc_roi_thread_edges", _i, [_vp, _i, _ip, _ip, _ip, _i, _ip]),
    ("sc_edge_support_tables", _i, [_vp, _i, _ip, _ip, _ip, _bp, _i, _ip, _ip, _i, _ip]),
    ("sc_sample_level", _i, [_vp, _i, _dp, _i, _dp, _bp, _i, _i, _ip, _ip, _ip, _ip, _ip, _i, _dp, _i, _up, _up, _lp]),
    ("sc_update_level", _i, [_vp, _i, _ip, _ip, _ip, _i, _i, _dp, _i, _dp, _bp, _bp, _i, _i, _i, _ip, _ip, _ip, _bp, _i, _ip, _ip, _i,
                             _dp, _bp, _bp, _ip]),
    ("sc_hard_level", _i, [_vp, _i, _ip, _ip, _ip, _i, _i, _dp, _dp, _i, _dp, _bp, _bp, _i, _i, _i, _ip, _ip, _ip, _ip, _bp, _ip, _ip, _i,
                           _ip, _ip, _i, _dp, _bp, _bp, _dp, _dp, _dp, _ip, _ip, _bp, _ip]),
    ("sc_aln_open", _i, [_s, _vpp]),
    ("sc_aln_open_filtered", _i, [_s, _sp, _i, _vpp]),
    ("sc_aln_close", None, [_vp]),
    ("sc_aln_error", _s, [_vp]),
    ("sc_aln_records", _l, [_vp]),
    ("sc_aln_ref_stats", _i, [_vp, _s, _lp, _lp]),
    ("sc_aln_walk", _i, [_vp, _l, _l, _s, _l, _lp, _lp]),
    ("sc_aln_pileup_flags", _i, [_vp, _s, _i, _i, _i, _bp, _bp, _bp]),
    ("sc_aln_load_reads", _i, [_vp, _s, _i, _i, _i, _i, _i, _i, _vpp]),
    ("sc_reads_get", _i, [_vp, _ip, _ipp, _sp, _ipp, _sp, _ipp, _ipp, _ipp, _ipp, _lp, _ip]),
    ("sc_reads_free", None, [_vp]),
    ("sc_depth_scan", _i, [_i, _vpp, _i, _sp, _ip, _i, _i] + _INTERVALS),
    ("sc_depth_scan_runs", _i, [_i, _ip, _i, _ip, _ip, _ip, _l, _i] + _INTERVALS),
    ("sc_align_reads", _i, [_i, _s, _lp, _i, _s, _s, _lp, _i, _ip, _ip, _ip, _ip, _ip, _ip, _up, _i, _ip, C.POINTER(ScAlignStats)]),
    ("sc_align_error", _s, []),
    ("sc_profile_hits", _i, _HITS + [C.POINTER(ScProfileStats)]),
    ("sc_profile_error", _s, []),
    ("sc_profile_hits_seeded", _i, _HITS + [C.POINTER(ScProfileSeedStats)]),
    ("sc_profile_seed_length", _i, [_ip, _i, _l, _d, _d, _d, _d, _ip]),
    ("sc_profile_counts", _i, [_i, _s, _lp, _i, _s, _lp, _i, _ip, _i, _d, _d, _d, _d, _i, _l, _ip, _ip, _ip, _lp, _l, _lp,
                               C.POINTER(ScProfileCountStats)]),
    ("sc_profile_index_create", _i, [_i, _s, _lp, _i, _vpp]),
    ("sc_profile_index_info", _i, [_vp, _ip, _lp, _ip, _ip]),
    ("sc_profile_index_counts", _i, [_vp, _s, _lp, _i, _ip, _i, _ip, _i, _d, _d, _d, _d, _i, _l, _ip, _ip, _ip, _ip, _lp, _l, _lp,
                                     C.POINTER(ScProfileCohortStats)]),
    ("sc_profile_index_free", None, [_vp]),
    ("sc_profile_evalue6", _d, [_i, _l, _i, _d, _d]),
    ("sc_taxa_train", _i, [_i, _s, _lp, _i, _ip, _i, _i, _i, _vpp, C.POINTER(ScTaxaStats)]),
    ("sc_taxa_classify", _i, [_vp, _s, _lp, _i, _u64p, _u64, _i, _i, _ip, _ip, _ip, C.POINTER(ScTaxaStats)]),
    ("sc_taxa_model_counts", _i, [_vp, _i, _up, _up]),
    ("sc_taxa_model_table", _i, [_vp, _i, _ip]),
    ("sc_taxa_free", None, [_vp]),
    ("sc_taxa_error", _s, []),
    ("sc_taxa_draw", _l, [_u64, _u64, _i, _i, _i]),
    ("sc_gene_distances", _i, [_i, _s, _lp, _i, _ip, _ip, _l, _ip, _dp, _i]),
    ("sc_gene_pairs", _i, [_i, _s, _lp, _i, _i, _i, _ip, _ip, _ip, _l, _lp, _dp, _i]),
    ("sc_pairs_widths", _i, [_ip, _i]),
    ("sc_pairs_error", _s, []),
    ("sc_map_index_create", _i, [_i, _s, _lp, _i, _i, _vpp]),
    ("sc_map_index_info", _i, [_vp, _ip, _lp, _ip, _lp, _dp]),
    ("sc_map_index_free", None, [_vp]),
    ("sc_map_reads", _i, [_vp, _s, _s, _lp, _i, _i, _i, _i, _l, _ip, _ip, _ip, _ip, _ip, _ip, _up, _i, _ip, _ip, _vp]),      # the last: a ScMapStats
    ("sc_map_candidates", _i, [_vp, _s, _lp, _i, _i, _i, _i, _lp, _ip, _ip, _ip, _l, _lp]),
    ("sc_map_limits", _i, [_ip, _ip]),
    ("sc_map_error", _s, []),
]
EXPORTS = [name for name, _, _ in ENTRIES]


def load_library():
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback for the StrainCall path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in ENTRIES:
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = load_library()
    return _LIB


# ---- what the wrappers below share

_PTR = {"<i4": _ip, "<i8": _lp, "<f8": _dp, "<u4": _up, "|u1": _bp, "<u8": _u64p}


def _ptr(a):
    """The data of a numpy array as the pointer its dtype stands for."""
    return a.ctypes.data_as(_PTR[a.dtype.str])


def _pack(strings):
    off = (C.c_int * (len(strings) + 1))()
    n = 0
    for i, s in enumerate(strings):
        off[i] = n
        n += len(s)
    off[len(strings)] = n
    return "".join(strings).encode("ascii"), off


def _pack_long(seqs):
    """A list of bytes as (the text back to back, its int64 offsets)."""
    import numpy as np
    return b"".join(seqs), np.array([0] + [len(x) for x in seqs], dtype=np.int64).cumsum()


def with_room(cap, attempt):
    """The entries that answer SC_ERR_CAPACITY with the number that suffices: attempt(cap) sets room for `cap` results aside,
    calls, and returns (rc, the number the call reports, what the caller keeps); it is repeated with the reported number while
    that is the answer.  Returns the last attempt's triple."""
    while True:
        rc, n, kept = attempt(cap)
        if rc != SC_ERR_CAPACITY or n <= cap:
            return rc, n, kept
        cap = n


def _check(rc, message=None):
    """StrainCallError unless rc is SC_OK; message: the entry that returns the calling thread's last message."""
    if rc != SC_OK:
        raise StrainCallError(rc, message().decode() if message else "")


class Handle:
    """Owner of one handle of the library, `_h`, given back by the entry `_free` names: on close(), at the end of a `with`
    block, or with the object."""
    _free = None
    _h = None

    def close(self):
        if self._h:
            try:
                getattr(lib(), self._free)(self._h)
            except TypeError:          # interpreter shutdown: the module globals are gone, the process frees the memory
                pass
            self._h = C.c_void_p()

    def _open(self):
        """The handle, for a call of the library; ValueError once it was given back."""
        if not self._h:
            raise ValueError("the index is closed")
        return self._h

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def default_params(error_rate=0.01, tau=0.02, diff_rate=0.01, graph_only=False, want_trace=False, want_timing=False, want_graph=False):
    return ScParams(error_rate, tau, diff_rate, 5000, 40000, 80, int(graph_only), int(want_trace), int(want_timing), int(want_graph))


def host_bind(device=0):
    """This process's main thread (and every thread started after the call) onto the CPUs next to GPU `device`; the number of
    CPUs, 0 when nothing was changed."""
    return int(lib().sc_host_bind(int(device)))


def host_plan(streams, local_world=0, cpus=0.0):
    """(executor threads, level-server threads, ingest threads) a Context(streams) starts on this host share."""
    out = (C.c_int * 3)()
    rc = lib().sc_host_plan(streams, local_world, cpus, out)
    _check(rc)
    return tuple(out)


class NativeReads(Handle):
    """A window's reads as load_mapping_reads leaves them (rows a2-a4), held by the library as the packed arrays
    sc_roi_submit takes.  The list views (pos, cigar, seq, copies, mates) are built on demand, for tests and tools."""
    _free = "sc_reads_free"

    def __init__(self, handle, gene_seq):
        self._h = handle
        self.gene_seq = gene_seq
        n, depth, n_in = C.c_int(), C.c_int(), C.c_long()
        self._pos, self._cig_off, self._seq_off, self._cn, self._mate_idx, self._mate_off = _ip(), _ip(), _ip(), _ip(), _ip(), _ip()
        self._cig, self._seq = C.c_char_p(), C.c_char_p()
        rc = lib().sc_reads_get(handle, C.byref(n), C.byref(self._pos), C.byref(self._cig), C.byref(self._cig_off), C.byref(self._seq),
                                C.byref(self._seq_off), C.byref(self._cn), C.byref(self._mate_idx), C.byref(self._mate_off),
                                C.byref(n_in), C.byref(depth))
        _check(rc)
        self.n = n.value
        self.n_input = n_in.value          # alignments the view returned for the window
        self.depth = depth.value

    def __len__(self):
        return self.n

    def _texts(self, text, off):
        raw = C.string_at(text, off[self.n]) if self.n else b""
        return [raw[off[i]:off[i + 1]].decode("ascii") for i in range(self.n)]

    def _view(self, name, build):
        """The list views are built once (an access inside a loop would otherwise rebuild the whole list every time)."""
        cache = self.__dict__.setdefault("_views", {})
        if name not in cache:
            cache[name] = build()
        return cache[name]

    @property
    def pos(self):
        return self._view("pos", lambda: [self._pos[i] for i in range(self.n)])

    @property
    def copies(self):
        return self._view("copies", lambda: [self._cn[i] for i in range(self.n)])

    @property
    def cigar(self):
        return self._view("cigar", lambda: self._texts(self._cig, self._cig_off))

    @property
    def seq(self):
        return self._view("seq", lambda: self._texts(self._seq, self._seq_off))

    @property
    def mates(self):
        return self._view("mates", lambda: [[self._mate_idx[k] for k in range(self._mate_off[i], self._mate_off[i + 1])] for i in range(self.n)])


class NativeAln(Handle):
    """An alignment file (SAM text or BAM) read and indexed by the library (sc_aln_*)."""
    _free = "sc_aln_close"

    def __init__(self, path, only=None):
        """only: keep the records of these references only ([]: of none -- statistics for pricing the regions; None: all)."""
        self.path = path
        self._h = C.c_void_p()
        if only is None:
            rc = lib().sc_aln_open(path.encode(), C.byref(self._h))
        else:
            names = (C.c_char_p * max(len(only), 1))(*[n.encode() for n in only])
            rc = lib().sc_aln_open_filtered(path.encode(), names, len(only), C.byref(self._h))
        if rc != SC_OK:
            msg = lib().sc_aln_error(self._h).decode() if self._h else "cannot open"
            self.close()
            raise StrainCallError(rc, "%s: %s" % (path, msg))

    def records(self):
        return lib().sc_aln_records(self._h)

    def walk(self, chunk=1 << 24):
        """(QNAME, FLAG, SEQ, QUAL) of every record in file order, whatever its reference (sc_aln_walk)."""
        buf = C.create_string_buffer(chunk)
        first, n_out, used = 0, C.c_long(), C.c_long()
        while True:
            rc = lib().sc_aln_walk(self._h, first, 1 << 20, buf, len(buf), C.byref(n_out), C.byref(used))
            if rc == SC_ERR_CAPACITY:
                buf = C.create_string_buffer(len(buf) * 4)
                continue
            if rc != SC_OK:
                raise StrainCallError(rc, self.path)
            if n_out.value == 0:
                return
            for line in buf.raw[:used.value].split(b"\n")[:-1]:
                q, f, seq, qual = line.split(b"\t")
                yield q, int(f), seq, qual
            first += n_out.value

    def ref_stats(self, gene):
        """(alignments of the reference, reference bases they cover)."""
        n, b = C.c_long(), C.c_long()
        lib().sc_aln_ref_stats(self._h, gene.encode(), C.byref(n), C.byref(b))
        return n.value, b.value

    def pileup_flags(self, mq, gene, P, Q):
        """{position: (has_insert, has_delete)} for the covered positions of gene:P-Q."""
        import numpy as np
        n = Q - P + 1
        if n <= 0:
            return {}
        cov, ins, dele = (np.zeros(n, dtype=np.uint8) for _ in range(3))
        rc = lib().sc_aln_pileup_flags(self._h, gene.encode(), P, Q, mq, _ptr(cov), _ptr(ins), _ptr(dele))
        _check(rc)
        idx = np.nonzero(cov)[0]
        return {int(k) + P: (bool(ins[k]), bool(dele[k])) for k in idx}

    def load_reads(self, gene_seq, gene, p0, p1, mq, rl, max_ins, max_depth):
        h = C.c_void_p()
        rc = lib().sc_aln_load_reads(self._h, gene.encode(), p0, p1, mq, rl, max_ins, max_depth, C.byref(h))
        if rc != SC_OK:
            raise StrainCallError(rc, lib().sc_aln_error(self._h).decode())
        return NativeReads(h, gene_seq)


class RegionResult:
    def __init__(self, seqs, abundance, graph, trace, stats):
        self.seqs = seqs
        self.abundance = abundance
        self.graph = graph
        self.trace = trace
        self.stats = stats


class _LevelArrays:
    """What Context.update_level and Context.hard_level both pass: one level's strains, labels, rows and entries as the
    arrays the library takes, and the buffers of what both return."""

    def __init__(self, slot, strain_labels, K, lpt, ll, has, ent_rid, ent_labels, ent_first, copies):
        import numpy as np
        self.ll = np.ascontiguousarray(ll, dtype=np.float64)
        self.S, self.n_reads = S, n_reads = self.ll.shape
        self.lpt = np.ascontiguousarray(lpt, dtype=np.float64)
        assert self.lpt.shape == (S, K, K) and len(slot) == len(strain_labels) == S
        self.has = np.ascontiguousarray(has, dtype=np.uint8)
        assert self.has.shape == (n_reads,) and len(ent_rid) == len(ent_labels) == len(ent_first)
        labels = [list(x) for x in list(strain_labels) + list(ent_labels)]
        lab_len = np.array([len(x) for x in labels], dtype=np.int32)
        lab_off = np.ascontiguousarray(np.concatenate(([0], np.cumsum(lab_len)[:-1])), dtype=np.int32)
        self.codes = np.array([c for x in labels for c in x] or [0], dtype=np.uint8)
        self.slot, self.rid = (np.ascontiguousarray(x, dtype=np.int32) for x in (slot, ent_rid))
        self.first = np.ascontiguousarray(ent_first, dtype=np.uint8)
        self.src, self.dst = (np.array([p[k] for p in copies] or [0], dtype=np.int32) for k in (0, 1))
        self.s_off, self.s_len, self.e_off, self.e_len = (np.ascontiguousarray(x) for x in (lab_off[:S], lab_len[:S], lab_off[S:], lab_len[S:]))
        self.ll_out = np.zeros((128, n_reads), dtype=np.float64)
        self.has_out = np.zeros(n_reads, dtype=np.uint8)
        self.isnew = np.zeros(max(len(self.rid), 1), dtype=np.uint8)
        self.done = C.c_int()

    def result(self):
        return dict(ll=self.ll_out, has=self.has_out, isnew=self.isnew[:len(self.rid)], done=self.done.value)


class Context:
    """One HIP device, `streams` regions in flight."""

    def __init__(self, device=0, streams=1):
        self.lib = lib()
        self.h = C.c_void_p()
        rc = self.lib.sc_ctx_create(device, streams, C.byref(self.h))
        if rc != SC_OK:
            raise StrainCallError(rc, "no gfx950 HIP device %d (the StrainCall path has no CPU fallback)" % device)

    def close(self):
        if self.h:
            self.lib.sc_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _err(self, rc):
        msg = self.lib.sc_last_error(self.h)
        return StrainCallError(rc, msg.decode("utf-8", "replace") if msg else "")

    def submit(self, region, params):
        """region: ingest.RegionReads or NativeReads.  Returns a handle."""
        n = len(region)
        if isinstance(region, NativeReads):
            pos, cig, cig_off, seq, seq_off = region._pos, region._cig, region._cig_off, region._seq, region._seq_off
            cn, mate_idx, mate_off = region._cn, region._mate_idx, region._mate_off
        else:
            pos = (C.c_int * max(n, 1))(*region.pos)
            cn = (C.c_int * max(n, 1))(*region.copies)
            cig, cig_off = _pack(region.cigar)
            seq, seq_off = _pack(region.seq)
            mate_off = (C.c_int * (n + 1))()
            flat = []
            for i, m in enumerate(region.mates):
                mate_off[i] = len(flat)
                flat.extend(m)
            mate_off[n] = len(flat)
            mate_idx = (C.c_int * max(len(flat), 1))(*flat)
        ref = region.gene_seq.encode("ascii")
        handle = C.c_int()
        rc = self.lib.sc_roi_submit(self.h, ref, len(ref), pos, cig, cig_off, seq, seq_off, cn, mate_idx, mate_off, n,
                                    C.byref(params), C.byref(handle))
        if rc != SC_OK:
            raise self._err(rc)
        return handle.value

    def wait(self, handle, want_graph=False, want_trace=False, release=True):
        rc = self.lib.sc_roi_wait(self.h, handle)
        graph = trace = None
        stats = ScStats()
        self.lib.sc_roi_stats(self.h, handle, C.byref(stats))
        if want_graph or rc != SC_OK:
            ln = C.c_long()
            self.lib.sc_roi_graph_dump(self.h, handle, None, 0, C.byref(ln))
            buf = C.create_string_buffer(ln.value + 1)
            if self.lib.sc_roi_graph_dump(self.h, handle, buf, ln.value, C.byref(ln)) == SC_OK:
                graph = buf.raw[:ln.value].decode("ascii")
        if rc != SC_OK:
            msg = self.lib.sc_roi_error(self.h, handle)            # this region's own message
            err = StrainCallError(rc, msg.decode("utf-8", "replace") if msg else "")
            if release:
                self.lib.sc_roi_release(self.h, handle)
            err.graph = graph
            raise err
        nst = C.c_int()
        cap, maxs = 1 << 16, 256
        while True:
            buf = C.create_string_buffer(cap)
            off = (C.c_int * (maxs + 1))()
            ab = (C.c_double * maxs)()
            rc = self.lib.sc_roi_result(self.h, handle, buf, cap, off, ab, maxs, C.byref(nst))
            if rc == SC_ERR_CAPACITY and cap < (1 << 30):
                cap *= 8
                maxs *= 4
                continue
            break
        if rc != SC_OK:
            raise self._err(rc)
        seqs = [buf.raw[off[i]:off[i + 1]].decode("ascii") for i in range(nst.value)]
        abundance = [ab[i] for i in range(nst.value)]
        if want_trace:
            ln = C.c_long()
            self.lib.sc_roi_trace(self.h, handle, None, 0, C.byref(ln))
            tb = C.create_string_buffer(ln.value + 1)
            if self.lib.sc_roi_trace(self.h, handle, tb, ln.value, C.byref(ln)) == SC_OK:
                trace = tb.raw[:ln.value].decode("ascii")
        if release:
            self.lib.sc_roi_release(self.h, handle)
        return RegionResult(seqs, abundance, graph, trace, stats.as_dict())

    def run(self, region, params, want_graph=False, want_trace=False):
        return self.wait(self.submit(region, params), want_graph, want_trace)

    def edge_support(self, handle):
        n = C.c_int()
        self.lib.sc_roi_edge_support(self.h, handle, None, 0, C.byref(n))
        arr = (C.c_int * max(n.value, 1))()
        rc = self.lib.sc_roi_edge_support(self.h, handle, arr, n.value, C.byref(n))
        if rc != SC_OK:
            raise self._err(rc)
        return list(arr[:n.value])

    def thread_tables(self, handle):
        """Row a5: (count[glen*8], first_read[glen*8], pool[], symbols) of a finished region."""
        ncls, npool = C.c_int(), C.c_long()
        self.lib.sc_roi_thread_tables(self.h, handle, None, None, 0, None, 0, None, C.byref(ncls), C.byref(npool))
        cnt = (C.c_int * max(ncls.value, 1))()
        first = (C.c_int * max(ncls.value, 1))()
        pool = (C.c_int * max(npool.value, 1))()
        sym = C.create_string_buffer(8)
        rc = self.lib.sc_roi_thread_tables(self.h, handle, cnt, first, ncls.value, pool, npool.value, sym, C.byref(ncls),
                                           C.byref(npool))
        if rc != SC_OK:
            raise self._err(rc)
        return list(cnt[:ncls.value]), list(first[:ncls.value]), list(pool[:npool.value]), sym.raw

    def thread_edges(self, handle):
        """Row a5, a test entry: (smin[glen*8], emin[glen*8], tmin[glen*64]) of a finished region; absent entries INT_MAX."""
        ncls = C.c_int()
        self.lib.sc_roi_thread_edges(self.h, handle, None, None, None, 0, C.byref(ncls))
        n = ncls.value
        smin, emin, tmin = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), (C.c_int * max(8 * n, 1))()
        rc = self.lib.sc_roi_thread_edges(self.h, handle, smin, emin, tmin, n, C.byref(ncls))
        if rc != SC_OK:
            raise self._err(rc)
        return list(smin[:n]), list(emin[:n]), list(tmin[:8 * n])

    def edge_support_tables(self, pool_ptr, pool_rid, pool_cn, node_is_end, edge_src, edge_dst, sorted_pools):
        """Row a16 on raw arrays, a test entry: the support of every edge (edge_src[e] -> edge_dst[e])."""
        import numpy as np
        ptr_, rid, cn, src, dst = (np.ascontiguousarray(x, dtype=np.int32) for x in (pool_ptr, pool_rid, pool_cn, edge_src, edge_dst))
        end = np.ascontiguousarray(node_is_end, dtype=np.uint8)
        assert rid.shape == cn.shape and src.shape == dst.shape and ptr_.size == end.size + 1
        out = np.zeros(max(src.size, 1), dtype=np.int32)
        rc = self.lib.sc_edge_support_tables(self.h, end.size, _ptr(ptr_), _ptr(rid), _ptr(cn), _ptr(end), src.size, _ptr(src), _ptr(dst),
                                             int(sorted_pools), _ptr(out))
        if rc != SC_OK:
            raise self._err(rc)
        return out[:src.size].tolist()

    def sample_level(self, a0, ll, has, ent_rid, ent_cn, ent_sym, mates, n_sweeps, U, e0=1):
        """Row a14 on its own (a test entry): one sampler level through the production kernel with the uniforms `U`.
        ll: [S][n_reads] log-likelihoods, has: [n_reads] presence, mates: per read a list of mate ids (-1: none).
        Returns dict(kdraw[S], cnt[S][16], n_draws, n_slow, n_exact, n_pass, kind, done: the pieces that ran on a grid)."""
        import numpy as np
        a0 = np.ascontiguousarray(a0, dtype=np.float64)
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        S, n_reads = ll.shape
        assert a0.shape == (S,)
        has = np.ascontiguousarray(has, dtype=np.uint8)
        assert has.shape == (n_reads,)
        ent = [np.ascontiguousarray(x, dtype=np.int32) for x in (ent_rid, ent_cn, ent_sym)]
        assert ent[0].shape == ent[1].shape == ent[2].shape
        mate_off = np.zeros(n_reads + 1, dtype=np.int32)
        mate_off[1:] = np.cumsum([len(mates[r]) if r < len(mates) else 0 for r in range(n_reads)])
        mate_idx = np.array([m for r in range(min(len(mates), n_reads)) for m in mates[r]] or [0], dtype=np.int32)
        U = np.ascontiguousarray(U, dtype=np.float64)
        kdraw = np.zeros(S, dtype=np.uint32)
        cnt = np.zeros((S, 16), dtype=np.uint32)
        out = (C.c_long * 6)()
        rc = self.lib.sc_sample_level(self.h, S, _ptr(a0), n_reads, _ptr(ll), _ptr(has), len(ent[0]), e0, _ptr(ent[0]), _ptr(ent[1]),
                                      _ptr(ent[2]), _ptr(mate_off), _ptr(mate_idx), n_sweeps, _ptr(U), len(U), _ptr(kdraw), _ptr(cnt), out)
        if rc != SC_OK:
            raise self._err(rc)
        return dict(kdraw=kdraw, cnt=cnt, n_draws=out[0], n_slow=out[1], n_exact=out[2], n_pass=out[3], kind=out[4], done=out[5])

    def update_level(self, slot, strain_labels, K, code_N, lpt, ll, has, ent_rid, ent_labels, ent_first, copies=(), copy_n=0, e0=1):
        """Row a13 on its own (a test entry): the row copies and the read log-likelihood update of one level through the
        production kernels.  slot: [S] rows of the strains, strain_labels / ent_labels: per strain / entry its label as a
        sequence of symbol codes, lpt: [S][K][K], ll: [S][n_reads] the strains' rows before the level, has: [n_reads],
        ent_first: [n_ent] (0: the read occurred earlier in the level), copies: (source row, destination row) pairs.
        Returns dict(ll[128][n_reads]: the whole matrix, has, isnew[n_ent], done: the pieces that ran on a grid)."""
        a = _LevelArrays(slot, strain_labels, K, lpt, ll, has, ent_rid, ent_labels, ent_first, copies)
        rc = self.lib.sc_update_level(self.h, a.S, _ptr(a.slot), _ptr(a.s_off), _ptr(a.s_len), K, code_N, _ptr(a.lpt), a.n_reads, _ptr(a.ll),
                                      _ptr(a.has), _ptr(a.codes), len(a.codes), len(a.rid), e0, _ptr(a.rid), _ptr(a.e_off), _ptr(a.e_len),
                                      _ptr(a.first), len(copies), _ptr(a.src), _ptr(a.dst), copy_n, _ptr(a.ll_out), _ptr(a.has_out),
                                      _ptr(a.isnew), C.byref(a.done))
        if rc != SC_OK:
            raise self._err(rc)
        return a.result()

    def hard_level(self, slot, strain_labels, K, code_N, lpt, ll, has, ent_rid, ent_labels, ent_first, logpri, ent_cn, mates, copies=(),
                   copy_n=0, e0=1):
        """Row a15 on its own (a test entry): the level of update_level with the hard update behind its update.  logpri: [S] the
        strains' log priors, ent_cn: [n_ent] copy numbers, mates: per read a list of mate ids (-1: none), as sample_level.
        Returns what update_level returns (behind the hard update) and abund[S], subst[S][K][K], resp[S][Q], qrid[Q], quid[Q],
        qcode[Q]."""
        import numpy as np
        a = _LevelArrays(slot, strain_labels, K, lpt, ll, has, ent_rid, ent_labels, ent_first, copies)
        logpri = np.ascontiguousarray(logpri, dtype=np.float64)
        cn = np.ascontiguousarray(ent_cn, dtype=np.int32)
        assert logpri.shape == (a.S,) and cn.shape == a.rid.shape
        mate_off = np.zeros(a.n_reads + 1, dtype=np.int32)
        mate_off[1:] = np.cumsum([len(mates[r]) if r < len(mates) else 0 for r in range(a.n_reads)])
        mate_idx = np.array([m for r in range(min(len(mates), a.n_reads)) for m in mates[r]] or [0], dtype=np.int32)
        Q = max(int(cn.sum()), 1)
        abund, subst, resp = np.zeros(a.S), np.zeros((a.S, K, K)), np.zeros((a.S, Q))
        qrid, quid, qcode = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.uint8)
        rc = self.lib.sc_hard_level(self.h, a.S, _ptr(a.slot), _ptr(a.s_off), _ptr(a.s_len), K, code_N, _ptr(a.lpt), _ptr(logpri), a.n_reads,
                                    _ptr(a.ll), _ptr(a.has), _ptr(a.codes), len(a.codes), len(a.rid), e0, _ptr(a.rid), _ptr(cn), _ptr(a.e_off),
                                    _ptr(a.e_len), _ptr(a.first), _ptr(mate_off), _ptr(mate_idx), len(copies), _ptr(a.src), _ptr(a.dst), copy_n,
                                    _ptr(a.ll_out), _ptr(a.has_out), _ptr(a.isnew), _ptr(abund), _ptr(subst), _ptr(resp), _ptr(qrid),
                                    _ptr(quid), _ptr(qcode), C.byref(a.done))
        if rc != SC_OK:
            raise self._err(rc)
        return dict(a.result(), abund=abund, subst=subst, resp=resp, qrid=qrid, quid=quid, qcode=qcode)

    def msa_align(self, seqs):
        """Row a7: rows of the progressive sum-of-pairs MSA of `seqs` (in the given order)."""
        txt, off = _pack(seqs)
        cap = (len(txt) + 2) * max(len(seqs), 1) + 16
        out = C.create_string_buffer(cap)
        ncol = C.c_int()
        rc = self.lib.sc_msa_align(self.h, txt, off, len(seqs), out, cap, C.byref(ncol))
        if rc != SC_OK:
            raise self._err(rc)
        w = ncol.value + 1
        return [out.raw[i * w:i * w + ncol.value].decode("ascii") for i in range(len(seqs))]


class AlignResult:
    """Per read: as_ (best score), xs (-1: none), seed (-1: no valid alignment), strand, pos (1-based), nm, cigar (text)."""

    def __init__(self, as_, xs, seed, strand, pos, nm, cigar, stats):
        self.as_, self.xs, self.seed, self.strand, self.pos, self.nm, self.cigar, self.stats = as_, xs, seed, strand, pos, nm, cigar, stats


def _read_args(reads, quals):
    """What an alignment entry takes of the reads: (text, offsets, the qualities' text or None, the CIGAR stride).  quals
    None: no qualities; an entry b"*", or one of another length than its read, is Q40 throughout."""
    rtext, rl = _pack_long(reads)
    qtext = None
    if quals is not None:
        qtext = b"".join(q if (q != b"*" and len(q) == len(r)) else b"I" * len(r) for r, q in zip(reads, quals))
    return rtext, rl, qtext, max([len(x) for x in reads] + [0]) // 2 + 4


def _align_out(n, stride):
    """The arrays an alignment entry fills for n reads: (as, xs, seed, strand, pos, nm), the CIGAR words, their counts."""
    import numpy as np
    cols = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(6)]
    return cols, np.zeros(max(n, 1) * stride, dtype=np.uint32), np.zeros(max(n, 1), dtype=np.int32)


def _cigar_texts(cig, ncig, stride, n):
    """The CIGAR text of each of n reads from its ncig[r] words (length << 4 | op) at cig[r * stride]; "*" for none."""
    return ["".join("%d%s" % (int(v) >> 4, "MIDNSHP=X"[int(v) & 15]) for v in cig[r * stride:r * stride + ncig[r]]) if ncig[r] else "*"
            for r in range(n)]


def align_reads(seeds, reads, quals=None, device=0):
    """sc_align_reads: every read against every seed on both strands (stage 4).  seeds, reads, quals:
    lists of bytes (quals None, or an entry b"*": Q40)."""
    n = len(reads)
    stext, sl = _pack_long(seeds)
    rtext, rl, qtext, stride = _read_args(reads, quals)
    cols, cig, ncig = _align_out(n, stride)
    st = ScAlignStats()
    rc = lib().sc_align_reads(device, stext, _ptr(sl), len(seeds), rtext, qtext, _ptr(rl), n, *[_ptr(c) for c in cols], _ptr(cig), stride,
                              _ptr(ncig), C.byref(st))
    _check(rc, lib().sc_align_error)
    return AlignResult(*[c[:n] for c in cols], _cigar_texts(cig, ncig, stride, n), st)


class ProfileHits:
    """The hits of sc_profile_hits in (segment, gene) order, one entry per hit in every array: seg, gene (indices), strand
    (1: reverse), score (raw, may be x.5), identity, align_len, qfrom, qto, hfrom, hto (1-based), evalue."""
    FIELDS = ("seg", "gene", "strand", "score", "identity", "align_len", "qfrom", "qto", "hfrom", "hto", "evalue")

    def __init__(self, arrays, stats):
        for k, v in zip(self.FIELDS, arrays):
            setattr(self, k, v)
        self.stats = stats

    def __len__(self):
        return len(self.seg)


def _profile_call(gtext, gl, n_genes, segs, thresholds, device, cap, seeded=False):
    import numpy as np
    stext, sl = _pack_long(segs)
    entry, stats = (lib().sc_profile_hits_seeded, ScProfileSeedStats) if seeded else (lib().sc_profile_hits, ScProfileStats)

    def attempt(cap):
        ints = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(9)]
        score, ev = np.zeros(max(cap, 1), dtype=np.float64), np.zeros(max(cap, 1), dtype=np.float64)
        st, nh = stats(), C.c_long()
        iptr = [_ptr(a) for a in ints]
        rc = entry(device, gtext, _ptr(gl), n_genes, stext, _ptr(sl), len(segs), *thresholds, iptr[0], iptr[1], iptr[2], _ptr(score),
                   iptr[3], iptr[4], iptr[5], iptr[6], iptr[7], iptr[8], _ptr(ev), cap, C.byref(nh), C.byref(st))
        return rc, nh.value, (ints, score, ev, st)
    rc, k, (ints, score, ev, st) = with_room(cap, attempt)
    _check(rc, lib().sc_profile_error)
    seg, gene, strand, identity, align_len, qfrom, qto, hfrom, hto = (a[:k] for a in ints)
    return [seg, gene, strand, score[:k], identity, align_len, qfrom, qto, hfrom, hto, ev[:k]], st


def profile_seed_length(seg_lens, gene_bases, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46, lossless=False):
    """sc_profile_seed_length (host only, no device): the k-mer length a seeded call over segments of these lengths and genes
    of `gene_bases` bases in all uses, 0 when it runs unseeded.  lossless=True: the bound k* itself, before it is cut to 16 and
    dropped below 11 (None when no length can pass)."""
    import numpy as np
    lens = np.ascontiguousarray(seg_lens, dtype=np.int32)
    raw = C.c_int()
    k = lib().sc_profile_seed_length(_ptr(lens), len(lens), int(gene_bases), float(min_identity), float(max_evalue),
                                     float(ka_lambda), float(ka_k), C.byref(raw))
    if k < 0:
        raise StrainCallError(k)
    return (raw.value or None) if lossless else k


def profile_hits(genes, segs, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46, device=0, cap=None, seeded=False):
    """sc_profile_hits: every segment against every gene on both strands under blastn's 1/-2 scoring.
    genes, segs: lists of bytes.  The room for hits starts at `cap` (default: 4 per segment, at least 65 536) and grows to
    what the library asks for when it does not suffice.  Segments go to the library in stretches of at most 2^30 (segment,
    gene, strand) tiles; the statistics are summed over the stretches.
    seeded: sc_profile_hits_seeded, the same hits from the pairs that share a k-mer; the statistics are
    ScProfileSeedStats, the genes are indexed again per stretch, and seed_k is the smallest of the stretches' (0 as soon as one
    ran unseeded)."""
    import numpy as np
    gtext, gl = _pack_long(genes)
    thresholds = (float(min_identity), float(max_evalue), float(ka_lambda), float(ka_k))
    step = max(1, (1 << 30) // (2 * max(len(genes), 1)))
    parts, total, seed_ks = [], (ScProfileSeedStats if seeded else ScProfileStats)(), []
    for a in range(0, max(len(segs), 1), step):
        chunk = segs[a:a + step]
        arrays, st = _profile_call(gtext, gl, len(genes), chunk, thresholds, device, max(1 << 16, 4 * len(chunk)) if cap is None else int(cap),
                                   seeded)
        arrays[0] = arrays[0] + a
        parts.append(arrays)
        for k, _ in total._fields_:
            setattr(total, k, getattr(total, k) + getattr(st, k))
        if seeded:
            seed_ks.append(st.seed_k)
    if seeded:
        total.seed_k = min(seed_ks)
    return ProfileHits([np.concatenate([p[f] for p in parts]) for f in range(11)], total)


class ProfileCounts:
    """The result of sc_profile_counts: triples = [(gene index, times_hit, number_of_such_genes, reads)] ascending, one entry
    per distinct triple; a read behind a triple gives its gene times_hit / number_of_such_genes."""

    def __init__(self, triples, stats):
        self.triples = triples
        self.stats = stats

    def __len__(self):
        return len(self.triples)


def profile_evalue6(seg_len, gene_bases, score2, ka_lambda=1.28, ka_k=0.46):
    """sc_profile_evalue6 (host only): the E-value of a segment of seg_len bases with doubled raw score score2 against
    gene_bases gene bases as the hit CSV holds it, six significant digits read back -- the E-value the counting rule compares."""
    return float(lib().sc_profile_evalue6(int(seg_len), int(gene_bases), int(score2), float(ka_lambda), float(ka_k)))


def _count_rows(entry, lead, segs, seg_read, read_args, options, cap, n_cols, stats):
    """What sc_profile_counts and sc_profile_index_counts share: entry(*lead, the segments, their read indices,
    *read_args(read indices), *options, n_cols int32 columns, the reads column, cap, n, statistics).  Returns (the rows as
    tuples, the statistics)."""
    import numpy as np
    stext, sl = _pack_long(segs)
    reads = np.ascontiguousarray(seg_read, dtype=np.int32)
    if len(reads) != len(segs):
        raise ValueError("%d read indices for %d segments" % (len(reads), len(segs)))
    args = list(lead) + [stext, _ptr(sl), len(segs), _ptr(reads)] + read_args(reads) + list(options)

    def attempt(cap):
        cols = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(n_cols)] + [np.zeros(max(cap, 1), dtype=np.int64)]
        st, n = stats(), C.c_long()
        return entry(*args, *[_ptr(c) for c in cols], cap, C.byref(n), C.byref(st)), n.value, (cols, st)
    rc, k, (cols, st) = with_room(1 << 16 if cap is None else int(cap), attempt)
    _check(rc, lib().sc_profile_error)
    return list(zip(*(c[:k].tolist() for c in cols))), st


def profile_counts(genes, segs, seg_read, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46, device=0, cap=None, seeded=False,
                   cand_room=0):
    """sc_profile_counts: the counting rule over the hits of profile_hits without the hit list.  genes, segs:
    lists of bytes; seg_read: one read index per segment (profile.read_index).  The room for triples starts at `cap`
    (default 65 536) and grows to what the library asks for.  The library itself passes the segments through in stretches of
    whole reads that fit `cand_room` candidate records (0: its default); the genes are uploaded and indexed once."""
    gtext, gl = _pack_long(genes)
    options = (float(min_identity), float(max_evalue), float(ka_lambda), float(ka_k), int(bool(seeded)), int(cand_room))
    return ProfileCounts(*_count_rows(lib().sc_profile_counts, (device, gtext, _ptr(gl), len(genes)), segs, seg_read,
                                      lambda reads: [int(reads.max()) + 1 if len(reads) else 0], options, cap, 3, ScProfileCountStats))


class ProfileCohortCounts:
    """The result of sc_profile_index_counts: rows = [(sample, gene index, times_hit, number_of_such_genes, reads)] ascending,
    one entry per distinct row; stats is the ScProfileCohortStats of the call."""

    def __init__(self, rows, stats):
        self.rows = rows
        self.stats = stats

    def __len__(self):
        return len(self.rows)

    def by_sample(self, s):
        """The (gene index, times_hit, number_of_such_genes, reads) of sample s, as profile.counts_from_triples takes them."""
        return [r[1:] for r in self.rows if r[0] == s]


class ProfileIndex(Handle):
    """The genes of a cohort held on one device until close() (sc_profile_index_create): uploaded once, with
    the k-mer keys of every seed length a call has needed and the arrays the calls work in.  genes: a list of bytes.  One
    call at a time."""
    _free = "sc_profile_index_free"

    def __init__(self, genes, device=0):
        gtext, gl = _pack_long(genes)
        self._h = C.c_void_p()
        rc = lib().sc_profile_index_create(int(device), gtext, _ptr(gl), len(genes), C.byref(self._h))
        _check(rc, lib().sc_profile_error)

    def info(self):
        """sc_profile_index_info: {"n_genes", "gene_bases", "cached_k": the seed lengths whose keys are kept, ascending}."""
        n_genes, bases, n_k, ks = C.c_int(), C.c_long(), C.c_int(), (C.c_int * 6)()
        rc = lib().sc_profile_index_info(self._open(), C.byref(n_genes), C.byref(bases), C.byref(n_k), ks)
        _check(rc, lib().sc_profile_error)
        return {"n_genes": n_genes.value, "gene_bases": bases.value, "cached_k": [int(ks[i]) for i in range(n_k.value)]}

    def counts(self, segs, seg_read, read_sample, n_samples, min_identity=95.0, max_evalue=1e-10, ka_lambda=1.28, ka_k=0.46, cap=None,
               seeded=False, cand_room=0):
        """sc_profile_index_counts: profile_counts over the reads of several samples at once.  segs: a list of bytes; seg_read:
        one read index per segment; read_sample: the sample (0..n_samples-1) of every read, non-decreasing.  The room for rows
        starts at `cap` (default 65 536) and grows to what the library asks for.  Returns a ProfileCohortCounts."""
        import numpy as np
        h = self._open()
        samples = np.ascontiguousarray(read_sample, dtype=np.int32)

        def read_args(reads):
            if len(reads) and int(reads.max()) >= len(samples):
                raise ValueError("read %d of %d reads with a sample" % (int(reads.max()), len(samples)))
            return [len(samples), _ptr(samples), int(n_samples)]
        options = (float(min_identity), float(max_evalue), float(ka_lambda), float(ka_k), int(bool(seeded)), int(cand_room))
        return ProfileCohortCounts(*_count_rows(lib().sc_profile_index_counts, (h,), segs, seg_read, read_args, options, cap, 4,
                                                ScProfileCohortStats))


TAXA_WORDS = 65536
TAXA_TRIALS = 100


def taxa_draw(seed, key, trial, draw, n_words):
    """sc_taxa_draw (host only): the word-list position of draw `draw` of trial `trial` for a list of n_words words."""
    return int(lib().sc_taxa_draw(int(seed), int(key), int(trial), int(draw), int(n_words)))


class TaxaModel(Handle):
    """A model trained by sc_taxa_train, held on one device until close().  seqs: the training sequences
    (bytes), genus: one genus index in 0..n_genera-1 per sequence.  grid_cap bounds the blocks of every launch (0: the
    library's own bound); keep_counts: also keep m for counts(), as much device memory again; stats is the ScTaxaStats of the
    training."""
    _free = "sc_taxa_free"

    def __init__(self, seqs, genus, n_genera, device=0, grid_cap=0, keep_counts=False):
        import numpy as np
        if len(genus) != len(seqs):
            raise ValueError("%d genus indices for %d sequences" % (len(genus), len(seqs)))
        text, off = _pack_long(seqs)
        gi = np.ascontiguousarray(genus, dtype=np.int32)
        self.n_genera = int(n_genera)
        self._h = C.c_void_p()
        self.stats = ScTaxaStats()
        rc = lib().sc_taxa_train(int(device), text, _ptr(off), len(seqs), _ptr(gi), self.n_genera, int(grid_cap), int(bool(keep_counts)),
                                 C.byref(self._h), C.byref(self.stats))
        _check(rc, lib().sc_taxa_error)

    def classify(self, queries, keys, seed=0, n_trials=TAXA_TRIALS, grid_cap=0):
        """sc_taxa_classify: queries (bytes) with one 64-bit key each.  Returns (best_genus[n], trial_winner[n][n_trials],
        n_words[n], ScTaxaStats); a query without a word has -1 in the first two."""
        import numpy as np
        n = len(queries)
        if len(keys) != n:
            raise ValueError("%d keys for %d queries" % (len(keys), n))
        text, off = _pack_long(queries)
        key = np.ascontiguousarray(keys, dtype=np.uint64)
        best, words = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        winner = np.zeros((max(n, 1), max(int(n_trials), 1)), dtype=np.int32)
        st = ScTaxaStats()
        rc = lib().sc_taxa_classify(self._h, text, _ptr(off), n, _ptr(key), int(seed), int(n_trials), int(grid_cap), _ptr(best),
                                    _ptr(winner), _ptr(words), C.byref(st))
        _check(rc, lib().sc_taxa_error)
        return best[:n], winner[:n], words[:n], st

    def counts(self, genus):
        """sc_taxa_model_counts: (m of the genus, n), 65 536 uint32 each; of a model trained with keep_counts."""
        import numpy as np
        m, n = np.zeros(TAXA_WORDS, dtype=np.uint32), np.zeros(TAXA_WORDS, dtype=np.uint32)
        rc = lib().sc_taxa_model_counts(self._h, int(genus), _ptr(m), _ptr(n))
        _check(rc, lib().sc_taxa_error)
        return m, n

    def table(self, genus):
        """sc_taxa_model_table: the genus' column of the table, 65 536 int32."""
        import numpy as np
        q = np.zeros(TAXA_WORDS, dtype=np.int32)
        rc = lib().sc_taxa_model_table(self._h, int(genus), _ptr(q))
        _check(rc, lib().sc_taxa_error)
        return q


MAP_DEFAULTS = dict(seed_k=16, max_occ=1024, max_cand=16, min_votes=1)


def map_limits():
    """sc_map_limits (host only): (the genes one pass of the vote kernel counts in LDS, the most votes a pair can have)."""
    rg, mv = C.c_int(), C.c_int()
    _check(lib().sc_map_limits(C.byref(rg), C.byref(mv)))
    return rg.value, mv.value


class MapResult(AlignResult):
    """AlignResult with `seed` the gene's index in the database (also as `gene`) and n_cand, the candidates of every read."""

    def __init__(self, *fields, n_cand):
        super().__init__(*fields)
        self.gene, self.n_cand = self.seed, n_cand


class MapIndex(Handle):
    """The gene database of the read mapper held on one device until close() (sc_map_index_create): the
    genes and their sorted k-mer keys.  genes: a list of bytes.  One call at a time."""
    _free = "sc_map_index_free"

    def __init__(self, genes, seed_k=MAP_DEFAULTS["seed_k"], device=0):
        gtext, gl = _pack_long(genes)
        self._h = C.c_void_p()
        rc = lib().sc_map_index_create(int(device), gtext, _ptr(gl), len(genes), int(seed_k), C.byref(self._h))
        _check(rc, lib().sc_map_error)

    def info(self):
        """sc_map_index_info: {"n_genes", "gene_bases", "seed_k", "n_keys", "index_ms"}."""
        n_genes, bases, k, n_keys, ms = C.c_int(), C.c_long(), C.c_int(), C.c_long(), C.c_double()
        rc = lib().sc_map_index_info(self._open(), C.byref(n_genes), C.byref(bases), C.byref(k), C.byref(n_keys), C.byref(ms))
        _check(rc, lib().sc_map_error)
        return {"n_genes": n_genes.value, "gene_bases": bases.value, "seed_k": k.value, "n_keys": n_keys.value, "index_ms": ms.value}

    def map_reads(self, reads, quals=None, max_occ=MAP_DEFAULTS["max_occ"], max_cand=MAP_DEFAULTS["max_cand"],
                  min_votes=MAP_DEFAULTS["min_votes"], pair_room=0):
        """sc_map_reads: every read against its candidate genes on both strands.  reads, quals: lists of bytes (quals None, or
        an entry b"*": Q40).  Returns a MapResult."""
        import numpy as np
        h = self._open()
        n = len(reads)
        rtext, rl, qtext, stride = _read_args(reads, quals)
        cols, cig, ncig = _align_out(n, stride)
        ncand = np.zeros(max(n, 1), dtype=np.int32)
        st = ScMapStats()
        rc = lib().sc_map_reads(h, rtext, qtext, _ptr(rl), n, int(max_occ), int(max_cand), int(min_votes), int(pair_room),
                                *[_ptr(c) for c in cols], _ptr(cig), stride, _ptr(ncig), _ptr(ncand), C.byref(st))
        _check(rc, lib().sc_map_error)
        return MapResult(*[c[:n] for c in cols], _cigar_texts(cig, ncig, stride, n), st, n_cand=ncand[:n])

    def candidates(self, reads, max_occ=MAP_DEFAULTS["max_occ"], max_cand=MAP_DEFAULTS["max_cand"], min_votes=MAP_DEFAULTS["min_votes"],
                   cap=None):
        """sc_map_candidates, a test and diagnostic entry: (cand_off[n + 1], gene, forward votes, reverse votes), read r's
        candidates at [cand_off[r], cand_off[r + 1]) in ascending gene order.  The room starts at `cap` (default 65 536) and
        grows to what the library asks for."""
        import numpy as np
        h = self._open()
        rtext, rl = _pack_long(reads)
        off = np.zeros(len(reads) + 1, dtype=np.int64)

        def attempt(cap):
            cols = [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(3)]
            n = C.c_long()
            rc = lib().sc_map_candidates(h, rtext, _ptr(rl), len(reads), int(max_occ), int(max_cand), int(min_votes), _ptr(off),
                                         *[_ptr(c) for c in cols], cap, C.byref(n))
            return rc, n.value, cols
        rc, k, cols = with_room(1 << 16 if cap is None else int(cap), attempt)
        _check(rc, lib().sc_map_error)
        return (off,) + tuple(c[:k] for c in cols)
