"""ctypes binding of include/sketchlib_dist.h.

Used by tests/ and bench.py (and as the model for any other FFI: the Rust binding in
INTEGRATION.md is the same call sequence).  Host buffers are numpy arrays; device
buffers are anything with a `data_ptr()` (torch tensors).  Loading fails loudly when
the in-tree HIP library is missing -- there is no fallback implementation.
"""
import ctypes as C
import os

import numpy as np

from .build import library_path

COREACC = 0
JACCARD = 1

OK = 0
ERR_INVALID_ARG = 1
ERR_NO_DEVICE = 2
ERR_HIP = 3
ERR_OOM = 4
ERR_KMER_COUNT = 5
ERR_EMPTY_DB = 6
ERR_KMER_NOT_FOUND = 7
ERR_INCOMPATIBLE = 8


class SklError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[skl error {code}] {message}")
        self.code = code
        self.message = message


class DistParams(C.Structure):
    _fields_ = [
        ("dist_type", C.c_int32),
        ("ani", C.c_int32),
        ("k_idx", C.c_uint64),
        ("completeness_cutoff", C.c_double),
    ]


class HistGrid(C.Structure):
    """skl_hist_grid: [lo0, hi0] in n0 cells, [lo1, hi1] in n1 cells (the second column: core/accessory only)."""
    _fields_ = [
        ("lo0", C.c_double),
        ("hi0", C.c_double),
        ("lo1", C.c_double),
        ("hi1", C.c_double),
        ("n0", C.c_uint32),
        ("n1", C.c_uint32),
    ]


# every symbol include/sketchlib_dist.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SIG = [
    ("skl_last_error", C.c_char_p, []),
    ("skl_abi_version", C.c_int, []),
    ("skl_device_count", C.c_int, []),
    ("skl_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("skl_ctx_destroy", C.c_int, [_P]),
    ("skl_ctx_set_stream", C.c_int, [_P, _P]),
    ("skl_ctx_use_default_stream", C.c_int, [_P]),
    ("skl_ctx_synchronize", C.c_int, [_P]),
    ("skl_ctx_reload_env", C.c_int, [_P]),
    ("skl_ctx_timing_enable", C.c_int, [_P, C.c_int]),
    ("skl_ctx_timing_reset", C.c_int, [_P]),
    ("skl_ctx_kernel_ms", C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("skl_ctx_last_kernel", C.c_char_p, [_P]),
    ("skl_log_variant", C.c_int, []),
    ("skl_ctx_flags", C.c_uint, [_P]),
    ("skl_ctx_set_knn_ties", C.c_int, [_P, C.c_int]),
    ("skl_self_dists_knn_window", C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P]),
    ("skl_knn_heaps_clear", C.c_int, [_P, C.c_size_t, C.c_size_t, _P, _P]),
    ("skl_self_dists_knn_window_logged", C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P,
                                                   _P, _P, _P, C.c_size_t]),
    ("skl_gather_bands_rccl", C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, C.c_int]),
    ("skl_knn_heaps_replay", C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    ("skl_knn_heaps_finalize", C.c_int, [_P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, C.c_int, _P, _P, _P]),
    ("skl_device_malloc", C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    ("skl_device_free", C.c_int, [_P, _P]),
    ("skl_device_memcpy", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    ("skl_ctx_get_knn_ties", C.c_int, [_P]),
    ("skl_ctx_early_break_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("skl_ctx_unit_table", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("skl_ctx_set_unit_table", C.c_int, [_P, C.c_int]),
    ("skl_ctx_early_break_blocks", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.c_size_t]),
    ("skl_ctx_knn_prune_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    ("skl_clock_sampler_start", C.c_int, [_P, C.c_uint32, C.c_uint32]),
    ("skl_clock_sampler_stop", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("skl_device_log", C.c_int, [_P, _P, C.c_size_t, _P]),
    ("skl_sketches_create", C.c_int, [_P, _P, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t,
                                      C.POINTER(_P)]),
    ("skl_sketches_set_completeness", C.c_int, [_P, _P]),
    ("skl_sketches_destroy", C.c_int, [_P]),
    ("skl_sketches_n_samples", C.c_size_t, [_P]),
    ("skl_sketches_select", C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(_P)]),
    ("skl_sketches_concat", C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    ("skl_set_k", C.c_int, [_P, C.c_size_t, C.c_int, C.c_double, C.POINTER(DistParams)]),
    ("skl_self_dists_all", C.c_int, [_P, _P, C.POINTER(DistParams), _P, C.c_int]),
    ("skl_self_dists_rows", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, _P,
                                      C.c_int]),
    ("skl_cross_dists_all", C.c_int, [_P, _P, _P, C.POINTER(DistParams), _P, C.c_int]),
    ("skl_cross_dists_rows", C.c_int, [_P, _P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t,
                                       _P, C.c_int]),
    ("skl_self_dists_within", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, C.c_double, C.c_double, _P, _P, _P,
                                        C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("skl_cross_dists_within", C.c_int, [_P, _P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, C.c_double, C.c_double, _P, _P, _P,
                                         C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("skl_self_clusters_within", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, C.c_double, C.c_double, _P, C.c_int, C.c_int,
                                           C.POINTER(C.c_uint64)]),
    ("skl_clusters_merge", C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("skl_self_dists_hist", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, C.POINTER(HistGrid), _P, C.c_int, C.c_int, _P]),
    ("skl_cross_dists_hist", C.c_int, [_P, _P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, C.POINTER(HistGrid), _P, C.c_int, C.c_int, _P]),
    ("skl_self_mst", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_int, C.c_double, _P, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("skl_clusters_from_edges", C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    ("skl_self_dists_knn", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, _P, _P, _P,
                                     C.c_int]),
    ("skl_self_dists_knn_rows", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t,
                                          C.c_size_t, _P, _P, _P, C.c_int]),
    ("skl_cross_dists_knn", C.c_int, [_P, _P, _P, C.POINTER(DistParams), C.c_size_t, _P, _P, _P,
                                      C.c_int]),
    ("skl_cross_dists_knn_rows", C.c_int, [_P, _P, _P, C.POINTER(DistParams), C.c_size_t,
                                           C.c_size_t, C.c_size_t, _P, _P, _P, C.c_int]),
    ("skl_self_dists_knn_candidates", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, _P, _P, _P, _P]),
    ("skl_self_dists_pairs", C.c_int, [_P, _P, C.POINTER(DistParams), _P, _P, C.c_size_t, _P, C.c_int]),
    ("skl_cross_dists_pairs", C.c_int, [_P, _P, _P, C.POINTER(DistParams), _P, _P, C.c_size_t, _P, C.c_int]),
    ("skl_shared_bins_max_samples", C.c_size_t, []),
    ("skl_self_dists_knn_shared_bins", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, _P, C.c_size_t, _P, _P, _P]),
    ("skl_knn_band_rows", C.c_size_t, [_P, C.POINTER(DistParams), C.c_size_t]),
    ("skl_self_dists_knn_partial", C.c_int, [_P, _P, C.POINTER(DistParams), C.c_size_t, C.c_size_t, _P, C.c_size_t,
                                             _P, _P, _P, C.c_int]),
    ("skl_knn_merge_states", C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_int, C.c_int,
                                       _P, _P, _P, C.c_int]),
    ("skl_inverted_create", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    ("skl_inverted_destroy", C.c_int, [_P]),
    ("skl_inverted_query", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P]),
    ("skl_inverted_band_queries", C.c_size_t, [_P, _P, C.c_int]),
    ("skl_inverted_query_top", C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, _P]),
    ("skl_sketch_signs", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, _P]),
    ("skl_sketch_signs_packed", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, _P]),
    ("skl_sketch_signs_aa", C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, C.c_int, _P]),
    ("skl_sketch_aa_shape", C.c_int, [C.c_int, C.c_size_t]),
    ("skl_sketch_finish", C.c_int, [_P, _P, C.c_size_t, C.c_uint64, _P, _P, _P]),
    ("skl_sketch_usigs_packed", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, _P, _P, _P]),
    ("skl_sketch_finish_u16", C.c_int, [_P, _P, C.c_size_t, C.c_uint64, _P, _P]),
    ("skl_sketch_bins_u16_packed", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_size_t, C.c_uint64, C.c_int, _P, _P]),
    ("skl_sketch_usigs_aa", C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, C.c_int, _P, _P, _P]),
    ("skl_reads_create", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(_P)]),
    ("skl_reads_survivors", C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, _P]),
    ("skl_reads_destroy", C.c_int, [_P]),
    ("skl_self_binmatch", C.c_int, [_P, _P, _P, C.c_int]),
    ("skl_cross_binmatch", C.c_int, [_P, _P, _P, _P, C.c_int]),
    ("skl_self_dists_all_host", C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t,
                                          C.POINTER(DistParams), _P, _P]),
    ("skl_cross_dists_all_host", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P,
                                           C.c_size_t, C.POINTER(DistParams), _P, _P, _P]),
]
DECLARED_SYMBOLS = [s[0] for s in _SIG]

_lib = None


def load():
    """dlopen the in-tree library and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C sketchlib.rust_amd/csrc`).  There is no CPU fallback."
            )
        # If torch is going to share this process (device tensors, torch.distributed), let it
        # load ITS HIP runtime first: two different libamdhip64 copies in one process leave
        # the second one without devices ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = _open(path)
    return _lib


def _open(path):
    L = C.CDLL(path)
    # SKL_LIBRARY_OLD=1: an older build of the library (round-over-round timing on one box) may lack newer entry points
    tolerant = bool(os.environ.get("SKL_LIBRARY_OLD")) and bool(os.environ.get("SKL_LIBRARY"))
    for name, restype, argtypes in _SIG:
        try:
            fn = getattr(L, name)  # AttributeError if the export is missing
        except AttributeError:
            if tolerant:
                continue
            raise
        fn.restype = restype
        fn.argtypes = argtypes
    return L


class using_library:
    """with using_library(path): ...  -- the binding calls into another build of the library (the A/B
    build) inside the block.  Handles created inside belong to that build: close them before leaving."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        global _lib
        load()
        self.saved = _lib
        _lib = _open(self.path)
        return self

    def __exit__(self, *exc):
        global _lib
        _lib = self.saved
        return False


def _check(rc):
    if rc != OK:
        raise SklError(rc, load().skl_last_error().decode("utf-8", "replace"))


def _ptr(buf):
    """(address, on_device) of a numpy array or a device tensor."""
    if buf is None:
        return None, 0
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data, 0
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr(), 1 if buf.is_cuda else 0
    raise TypeError(f"unsupported buffer type {type(buf)}")


LOG_UNMATCHED = 1
TIES_CANONICAL, TIES_REFERENCE = 0, 1


def ctx_flags(ctx=None):
    """skl_ctx_flags(): conditions worth telling the user about (LOG_UNMATCHED: see the header)."""
    return int(load().skl_ctx_flags(ctx._h if ctx is not None else None))


def log_variant():
    """Which restated form of glibc's log() reproduces this host's libm: 0 FMA, 1 SSE2, -1 neither."""
    return int(load().skl_log_variant())


def device_log(ctx, x):
    """ln(x) as the kernels evaluate it on the completeness path (csrc/glibc_log.hpp), on the device."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    _check(load().skl_device_log(ctx._h, x.ctypes.data, x.size, out.ctypes.data))
    return out


def device_count():
    return load().skl_device_count()


class Context:
    """skl_ctx: one per (thread, device)."""

    def __init__(self, device=0, stream=None):
        self._h = _P()
        _check(load().skl_ctx_create(device, C.byref(self._h)))
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        """stream: integer hipStream_t handle (torch.cuda.current_stream().cuda_stream): 0 is
        the device's default stream; None restores the context's own (non-blocking) stream."""
        if stream is None:
            _check(load().skl_ctx_set_stream(self._h, None))
        elif int(stream) == 0:
            _check(load().skl_ctx_use_default_stream(self._h))
        else:
            _check(load().skl_ctx_set_stream(self._h, _P(stream)))

    def synchronize(self):
        _check(load().skl_ctx_synchronize(self._h))

    def reload_env(self):
        """Re-read the SKL_* environment switches (they are otherwise read when the context is created)."""
        _check(load().skl_ctx_reload_env(self._h))

    def timing_enable(self, every=1):
        """Bracket every `every`-th pair-kernel launch with HIP events (0: off, the library's default)."""
        _check(load().skl_ctx_timing_enable(self._h, int(every)))

    def timing_reset(self):
        _check(load().skl_ctx_timing_reset(self._h))

    def kernel_ms(self):
        """(summed pair-kernel device ms, launches) since the last timing_reset()."""
        ms = C.c_float()
        n = C.c_int()
        _check(load().skl_ctx_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def early_break_stats(self):
        """(pairs of early-break core/accessory launches, pairs among them completed one by one) since the context was made."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(load().skl_ctx_early_break_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def early_break_blocks(self):
        """What the last dense core/accessory call decided: {"blocks": (rows, cols), "shifts": (rows, cols), "pooled_lengths": ke or 0,
        "mixed": bool, "block_lengths": uint8 [rows, cols] or None}."""
        br, bc, sr, sc = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        pooled, mixed = C.c_int(), C.c_int()
        _check(load().skl_ctx_early_break_blocks(self._h, C.byref(br), C.byref(bc), C.byref(sr), C.byref(sc), C.byref(pooled), C.byref(mixed), None, 0))
        table = None
        if mixed.value:
            table = np.zeros((br.value, bc.value), dtype=np.uint8)
            _check(load().skl_ctx_early_break_blocks(self._h, None, None, None, None, None, None, table.ctypes.data, table.size))
        return {"blocks": (br.value, bc.value), "shifts": (sr.value, sc.value), "pooled_lengths": pooled.value, "mixed": bool(mixed.value),
                "block_lengths": table}

    def unit_table(self):
        """(the last pair launch read a unit table, launches that found theirs in the cache, launches that had one built) -- see the header."""
        used, hits, builds = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(load().skl_ctx_unit_table(self._h, C.byref(used), C.byref(hits), C.byref(builds)))
        return bool(used.value), hits.value, builds.value

    def set_unit_table(self, mode):
        """-1 (default): the dense calls' launches within the table's cap read a unit table; 0: none does; 1: every launch whose form allows it."""
        _check(load().skl_ctx_set_unit_table(self._h, int(mode)))

    def knn_prune_stats(self, full=False):
        """(tiles, tiles left early) of the last self kNN call's prunable launches; full=True: + (stages of a whole tile,
        stages the pruned tiles had walked) and the share of the walk actually made."""
        a, b, c, d, e = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load().skl_ctx_knn_prune_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        if not full:
            return a.value, b.value
        walked = ((a.value - b.value) * c.value + d.value) / (a.value * c.value) if a.value and c.value else 1.0
        return {"tiles": a.value, "tiles_left_early": b.value, "tiles_sparse_walk": e.value, "stages_per_tile": c.value, "stages_walked_in_pruned_tiles": d.value,
                "share_of_the_walk_made": walked}

    def set_knn_ties(self, mode):
        """TIES_REFERENCE (the library's default: the reference binary's lists) or TIES_CANONICAL: see the header."""
        _check(load().skl_ctx_set_knn_ties(self._h, int(mode)))

    def clock_sampler_start(self, interval_us=20, max_samples=1 << 16):
        """One-wave shader-clock sampler next to the context's kernels (diagnostic; see the header)."""
        _check(load().skl_clock_sampler_start(self._h, interval_us, max_samples))

    def clock_sampler_stop(self):
        """-> {"ghz": median, "p10", "p90", "mean", "intervals"}; call after synchronize(), never after a device-wide sync."""
        med, p10, p90, mean, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _check(load().skl_clock_sampler_stop(self._h, C.byref(med), C.byref(p10), C.byref(p90), C.byref(mean), C.byref(n)))
        return {"ghz": med.value, "p10": p10.value, "p90": p90.value, "mean": mean.value, "intervals": n.value}

    def last_kernel(self):
        return load().skl_ctx_last_kernel(self._h).decode()

    def close(self):
        if self._h:
            load().skl_ctx_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- slabs ----
    def sketches(self, bins, n, kmers, sketchsize64, completeness=None):
        return Sketches(self, bins, n, kmers, sketchsize64, completeness)


class Sketches:
    """skl_sketches: a MultiSketch's bins resident on the device."""

    def __init__(self, ctx, bins, n, kmers, sketchsize64, completeness=None):
        self.ctx = ctx
        self.n = int(n)
        self.kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
        self.nk = len(self.kmers)
        self.ss64 = int(sketchsize64)
        if isinstance(bins, np.ndarray):
            if bins.dtype == np.int64:      # (what torch hands over: the same bits, no 8-bytes-per-word conversion pass)
                bins = bins.view(np.uint64)
            bins = np.ascontiguousarray(bins, dtype="<u8").reshape(-1)
            assert bins.size == self.n * self.nk * self.ss64 * 14, "bins size mismatch"
        addr, on_dev = _ptr(bins)
        self._h = _P()
        _check(load().skl_sketches_create(ctx._h, addr, on_dev, self.n, self.nk,
                                          self.kmers.ctypes.data, self.ss64, C.byref(self._h)))
        if completeness is not None:
            self.set_completeness(completeness)

    def set_completeness(self, completeness):
        if completeness is None:
            _check(load().skl_sketches_set_completeness(self._h, None))
            return
        comp = np.ascontiguousarray(completeness, dtype=np.float64)
        assert comp.size == self.n
        _check(load().skl_sketches_set_completeness(self._h, comp.ctypes.data))

    @classmethod
    def _adopt(cls, ctx, handle, n, kmers, sketchsize64):
        """A Sketches around a handle the library made (select / concat)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.n = int(n)
        self.kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
        self.nk = len(self.kmers)
        self.ss64 = int(sketchsize64)
        self._h = handle
        return self

    def select(self, ids):
        """skl_sketches_select: a NEW slab of samples ids[0], ids[1], .. (repeats allowed); this one is untouched."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        h = _P()
        _check(load().skl_sketches_select(self.ctx._h, self._h, ids.ctypes.data, ids.size, C.byref(h)))
        return Sketches._adopt(self.ctx, h, ids.size, self.kmers, self.ss64)

    def set_k(self, kmer=None, ani=False, cutoff=0.64):
        """distances::set_k (mod.rs:25-37)."""
        p = DistParams()
        _check(load().skl_set_k(self._h, 0 if kmer is None else int(kmer), int(ani), cutoff,
                                C.byref(p)))
        return p

    def close(self):
        if self._h:
            load().skl_sketches_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def concat(a, b):
    """skl_sketches_concat: a NEW slab of a's samples, then b's; both inputs are untouched."""
    h = _P()
    _check(load().skl_sketches_concat(a.ctx._h, a._h, b._h, C.byref(h)))
    return Sketches._adopt(a.ctx, h, a.n + b.n, a.kmers, a.ss64)


def params(dist_type=COREACC, k_idx=0, ani=False, cutoff=0.64):
    return DistParams(dist_type, int(ani), k_idx, cutoff)


def ncols(p):
    return 2 if p.dist_type == COREACC else 1


def self_pairs(n, r0=0, r1=None):
    r1 = n if r1 is None else r1
    r1 = min(r1, max(n - 1, 0))
    if r1 <= r0:
        return 0
    upto = lambda r: r * n - r * (r + 1) // 2  # noqa: E731
    return upto(r1) - upto(r0)


# ---- dense ----

def self_dists_all(ctx, s, p, out=None):
    """distances::self_dists_all (mod.rs:58-130) -> [n(n-1)/2, ncols] f32."""
    n_pairs = self_pairs(s.n)
    if out is None:
        out = np.zeros((n_pairs, ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_self_dists_all(ctx._h, s._h, C.byref(p), addr, dev))
    return out


def self_dists_rows(ctx, s, p, r0, r1, out=None):
    if out is None:
        out = np.zeros((self_pairs(s.n, r0, r1), ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_self_dists_rows(ctx._h, s._h, C.byref(p), r0, r1, addr, dev))
    return out


def cross_dists_all(ctx, r, q, p, out=None):
    """distances::cross_dists_all (mod.rs:227-297) -> [n_ref, n_query, ncols] f32."""
    if out is None:
        out = np.zeros((r.n, q.n, ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_cross_dists_all(ctx._h, r._h, q._h, C.byref(p), addr, dev))
    return out


def cross_dists_rows(ctx, r, q, p, r0, r1, out=None):
    if out is None:
        out = np.zeros((r1 - r0, q.n, ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_cross_dists_rows(ctx._h, r._h, q._h, C.byref(p), r0, r1, addr, dev))
    return out


# ---- all pairs within a distance cap ----

WITHIN_CHUNK = 2048        # WITHIN_CHUNK of csrc/within_plan.hpp: pair positions a workgroup of the filter owns
WITHIN_SCAN_STEP = 1024    # WITHIN_SCAN_STEP: chunk counts the scan takes per step


def dists_within_into(ctx, s, p, max_dist, max_acc=np.inf, r0=0, r1=None, out=None, capacity=0, query=None):
    """skl_self_dists_within (query=None) / skl_cross_dists_within as they are: rows [r0, r1), `out` = (i, j, d) numpy arrays or
    device tensors taking `capacity` records (None with capacity 0: count only) -> n_found, which may exceed capacity."""
    r1 = (s.n) if r1 is None else r1
    oi, oj, od = out if out is not None else (None, None, None)
    (ai, dev), (aj, dev_j), (ad, dev_d) = _ptr(oi), _ptr(oj), _ptr(od)
    if not dev == dev_j == dev_d:
        raise ValueError("the three outputs must live on the same side")
    found = C.c_uint64(0)
    if query is None:
        _check(load().skl_self_dists_within(ctx._h, s._h, C.byref(p), r0, r1, max_dist, max_acc, ai, aj, ad, capacity, dev, C.byref(found)))
    else:
        _check(load().skl_cross_dists_within(ctx._h, s._h, query._h, C.byref(p), r0, r1, max_dist, max_acc, ai, aj, ad, capacity, dev,
                                             C.byref(found)))
    return int(found.value)


def count_within(ctx, s, p, max_dist, max_acc=np.inf, r0=0, r1=None, query=None):
    """How many pairs of rows [r0, r1) lie within the cap (the count-only form: nothing is scattered or copied)."""
    return dists_within_into(ctx, s, p, max_dist, max_acc, r0, r1, query=query)


def _dists_within(ctx, s, p, max_dist, max_acc, r0, r1, capacity, query):
    # Without a capacity the call runs twice: the count-only form sizes the arrays, the second call fills them.  The dense
    # evaluation -- nearly all of the time -- is paid twice; a caller who can bound the answer passes `capacity` and pays once.
    cap = count_within(ctx, s, p, max_dist, max_acc, r0, r1, query) if capacity is None else int(capacity)
    out = (np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros((cap, ncols(p)), dtype=np.float32))
    found = dists_within_into(ctx, s, p, max_dist, max_acc, r0, r1, out, cap, query) if cap else 0
    if capacity is None and found != cap:
        raise RuntimeError(f"{found} pairs within the cap after {cap} were counted")
    if capacity is not None and found > cap:   # the arrays held the first `cap`: once more with the exact size
        return _dists_within(ctx, s, p, max_dist, max_acc, r0, r1, found, query)
    return tuple(x[:found] for x in out)


def self_dists_within(ctx, s, p, max_dist, max_acc=np.inf, r0=0, r1=None, capacity=None):
    """All pairs i < j of rows [r0, r1) whose distance is within the cap, in condensed order -> (i, j, d): uint32 [n_found],
    uint32 [n_found], f32 [n_found, ncols] -- the dense listing with lines removed (skl_self_dists_within: d[:, 0] <= max_dist,
    for ANI d >= 1 - max_dist; core/accessory also d[:, 1] <= max_acc unless it is inf).  Always exactly n_found records.
    capacity=None counts first and then fills arrays of the exact size (two evaluations of the rows); capacity=N evaluates
    once into arrays of N records and repeats with the exact size only if more than N pairs passed."""
    return _dists_within(ctx, s, p, max_dist, max_acc, r0, r1, capacity, None)


def cross_dists_within(ctx, r, q, p, max_dist, max_acc=np.inf, r0=0, r1=None, capacity=None):
    """The same for reference rows [r0, r1) against every query -> (i_ref, j_query, d), ascending i_ref * n_query + j_query."""
    return _dists_within(ctx, r, p, max_dist, max_acc, r0, r1, capacity, q)


# ---- single-linkage clusters under a distance cap ----

CLUSTERS_CONTINUE = 1      # SKL_CLUSTERS_CONTINUE


def clusters_within(ctx, s, p, max_dist, max_acc=np.inf, r0=0, r1=None, labels=None):
    """skl_self_clusters_within: the pairs self_dists_within would list for rows [r0, r1), followed to their connected
    components -> (labels uint32 [n], n_clusters); labels[i] is the lowest sample index of i's cluster.  labels=None starts
    from the identity and returns a new numpy array; a uint32 numpy array or a device tensor of n elements (int32 bits) holds
    the result of earlier calls, is built upon in place (SKL_CLUSTERS_CONTINUE: labels[i] <= i is checked) and returned."""
    r1 = s.n if r1 is None else r1
    flags = 0 if labels is None else CLUSTERS_CONTINUE
    if labels is None:
        labels = np.empty(s.n, dtype=np.uint32)
    elif isinstance(labels, np.ndarray):
        if labels.dtype != np.uint32 or not labels.flags.c_contiguous or labels.size < s.n:
            raise ValueError("labels: a contiguous uint32 array of n elements")
    addr, dev = _ptr(labels)
    found = C.c_uint64(0)
    _check(load().skl_self_clusters_within(ctx._h, s._h, C.byref(p), r0, r1, max_dist, max_acc, addr, dev, flags, C.byref(found)))
    return labels, int(found.value)


def clusters_merge(ctx, a, b):
    """skl_clusters_merge: the clusters connected through either of two partitions of the same samples -> (labels, n_clusters).
    Two numpy arrays give a new array; two device tensors are merged into `a` in place, which is returned."""
    (_pa, dev_a), (_pb, dev_b) = _ptr(a), _ptr(b)
    if dev_a != dev_b:
        raise ValueError("the two partitions must live on the same side")
    if not dev_a:
        a = np.array(a, dtype=np.uint32, copy=True).reshape(-1)
        b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1)
    n = a.size if not dev_a else a.numel()
    if n != (b.size if not dev_b else b.numel()):
        raise ValueError("the two partitions differ in length")
    found = C.c_uint64(0)
    _check(load().skl_clusters_merge(ctx._h, _ptr(a)[0], _ptr(b)[0], n, dev_a, C.byref(found)))
    return a, int(found.value)


def dereplicate(ctx, s, p, max_dist, max_acc=np.inf):
    """One representative per cluster under the cap -> (Sketches, ids): ids is the ascending list of the samples that are their
    own label (the lowest index of each cluster), the new slab s.select(ids); `s` is untouched and stays on the device."""
    labels, n_clusters = clusters_within(ctx, s, p, max_dist, max_acc)
    ids = np.flatnonzero(labels == np.arange(s.n, dtype=np.uint32)).astype(np.uint32)
    assert ids.size == n_clusters
    return s.select(ids), ids


# ---- histogram of the stored values ----

HIST_ACCUMULATE = 1        # SKL_HIST_ACCUMULATE


def dists_hist(ctx, s, p, grid, r0=0, r1=None, query=None, counts=None):
    """skl_self_dists_hist (query=None) / skl_cross_dists_hist: the histogram of the f32 values the dense call stores for rows
    [r0, r1) -> (counts, outside, nan).  grid: (lo0, hi0, n0), or (lo0, hi0, n0, lo1, hi1, n1) for core/accessory; the cell rule is
    the header's.  counts=None gives a new numpy uint64 array of shape (n0,) or (n0, n1); a uint64 numpy array or a device tensor
    (int64 bits) of n0 * n1 elements is ACCUMULATED into (SKL_HIST_ACCUMULATE) and returned as the same object.  outside: the
    pairs off the grid in some column; nan: the pairs with a NaN in some column; both of this call alone."""
    r1 = s.n if r1 is None else r1
    two = ncols(p) == 2
    if len(grid) != (6 if two else 3):
        raise ValueError("grid: (lo0, hi0, n0) for one stored column, (lo0, hi0, n0, lo1, hi1, n1) for core/accessory")
    g = HistGrid(grid[0], grid[1], grid[3] if two else 0.0, grid[4] if two else 0.0, int(grid[2]), int(grid[5]) if two else 1)
    cells = g.n0 * g.n1
    flags = 0 if counts is None else HIST_ACCUMULATE
    if counts is None:
        counts = np.zeros((g.n0, g.n1) if two else (g.n0,), dtype=np.uint64)
    elif isinstance(counts, np.ndarray):
        if counts.dtype != np.uint64 or not counts.flags.c_contiguous or counts.size < cells:
            raise ValueError("counts: a contiguous uint64 array of n0 * n1 elements")
    elif counts.numel() < cells or counts.element_size() != 8 or not counts.is_contiguous():
        raise ValueError("counts: a contiguous device tensor of n0 * n1 8-byte elements")
    addr, dev = _ptr(counts)
    outside = (C.c_uint64 * 2)(0, 0)
    if query is None:
        _check(load().skl_self_dists_hist(ctx._h, s._h, C.byref(p), r0, r1, C.byref(g), addr, dev, flags, outside))
    else:
        _check(load().skl_cross_dists_hist(ctx._h, s._h, query._h, C.byref(p), r0, r1, C.byref(g), addr, dev, flags, outside))
    return counts, int(outside[0]), int(outside[1])


# ---- minimum spanning tree of the distances ----

def mst(ctx, s, p, column=0, max_dist=np.inf, labels=False):
    """skl_self_mst: the minimum spanning forest of the graph whose edges are the pairs with a stored value <= max_dist in
    `column` (0: core or single-k distance, 1: accessory) -> (i, j, w, rounds): uint32 [n_edges], uint32 [n_edges], f32 [n_edges]
    in ascending (w, i, j) -- the order in which single linkage merges -- and the number of Boruvka rounds that added an edge.
    labels=True appends the uint32 [n] component labels (lowest index of the component).  The edges with w <= t, handed to
    clusters_from_edges, give the single-linkage clusters at threshold t."""
    room = max(s.n - 1, 0)
    oi, oj, ow = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.float32)
    lab = np.zeros(s.n, dtype=np.uint32) if labels else None
    found, rounds = C.c_uint64(0), C.c_uint32(0)
    _check(load().skl_self_mst(ctx._h, s._h, C.byref(p), int(column), float(max_dist), oi.ctypes.data, oj.ctypes.data, ow.ctypes.data,
                               lab.ctypes.data if labels else None, C.byref(found), C.byref(rounds)))
    k = int(found.value)
    out = (oi[:k], oj[:k], ow[:k], int(rounds.value))
    return out + (lab,) if labels else out


def clusters_from_edges(ctx, i, j, n):
    """skl_clusters_from_edges: the components of n samples under the edges (i[k], j[k]) -> (labels uint32 [n], n_clusters), in
    the label form of clusters_within.  On a prefix of mst()'s edges: the single-linkage clusters at that threshold."""
    i = np.ascontiguousarray(i, dtype=np.uint32).reshape(-1)
    j = np.ascontiguousarray(j, dtype=np.uint32).reshape(-1)
    if i.size != j.size:
        raise ValueError("the two edge arrays differ in length")
    lab = np.zeros(int(n), dtype=np.uint32)
    found = C.c_uint64(0)
    _check(load().skl_clusters_from_edges(ctx._h, i.ctypes.data if i.size else None, j.ctypes.data if j.size else None, i.size, int(n),
                                          lab.ctypes.data if n else None, C.byref(found)))
    return lab, int(found.value)


# ---- sparse ----

def _knn_out(rows, knn):
    return (np.zeros((rows, knn), dtype=np.uint64), np.zeros((rows, knn), dtype=np.float32),
            np.zeros((rows, knn), dtype=np.float32))


def self_dists_knn(ctx, s, p, knn, r0=0, r1=None):
    """distances::self_dists_knn (mod.rs:133-224) -> (idx, d0, d1) each [rows, knn]."""
    r1 = s.n if r1 is None else r1
    idx, d0, d1 = _knn_out(r1 - r0, knn)
    _check(load().skl_self_dists_knn_rows(ctx._h, s._h, C.byref(p), knn, r0, r1, idx.ctypes.data,
                                          d0.ctypes.data, d1.ctypes.data, 0))
    return idx, d0, d1


def cross_dists_knn(ctx, r, q, p, knn, q0=0, q1=None):
    """distances::cross_dists_knn (mod.rs:306-395); rows = queries, idx into refs."""
    q1 = q.n if q1 is None else q1
    idx, d0, d1 = _knn_out(q1 - q0, knn)
    _check(load().skl_cross_dists_knn_rows(ctx._h, r._h, q._h, C.byref(p), knn, q0, q1,
                                           idx.ctypes.data, d0.ctypes.data, d1.ctypes.data, 0))
    return idx, d0, d1


def knn_band_rows(s, p, participants=1):
    """Band height of the one-evaluation self kNN that every participant agrees on."""
    return int(load().skl_knn_band_rows(s._h, C.byref(p), participants))


def self_dists_knn_partial(ctx, s, p, knn, band_rows, bands, out=None):
    """This participant's share (ascending band indices) of the one-evaluation self kNN:
    -> (state_key u32, state_idx u32, state_d1 f32 | None), each [n, knn], for ALL n rows.
    `out` = a tuple of preallocated numpy arrays or device tensors (int32 bit patterns) instead."""
    bands = np.ascontiguousarray(bands, dtype=np.uint32)
    coreacc = p.dist_type == COREACC
    if out is None:
        out = (np.empty((s.n, knn), dtype=np.uint32), np.empty((s.n, knn), dtype=np.uint32),
               np.empty((s.n, knn), dtype=np.float32) if coreacc else None)
    (ka, dev), (ia, _), (da, _) = _ptr(out[0]), _ptr(out[1]), _ptr(out[2])
    _check(load().skl_self_dists_knn_partial(ctx._h, s._h, C.byref(p), knn, band_rows,
                                             bands.ctypes.data if bands.size else None, bands.size, ka, ia, da, dev))
    return out


def knn_merge_states(ctx, state_key, state_idx, state_d1, ani=False, out=None):
    """Partial states of the same rows, stacked [n_states, rows, knn] (numpy or device tensors)
    -> (idx u64, d0 f32, d1 f32 | None) [rows, knn] as self_dists_knn returns them."""
    n_states, rows, knn = state_key.shape
    (ka, dev), (ia, _), (da, _) = _ptr(state_key), _ptr(state_idx), _ptr(state_d1)
    if out is None:
        out = _knn_out(rows, knn)
    (oi, odev), (o0, _), (o1, _) = _ptr(out[0]), _ptr(out[1]), _ptr(out[2])
    _check(load().skl_knn_merge_states(ctx._h, n_states, rows, knn, ka, ia, da, dev, int(ani), oi, o0,
                                       o1 if state_d1 is not None else None, odev))
    return out


def knn_heaps_alloc(n, knn, coreacc, device):
    """Travelling heaps of the reference-order pipeline (skl_self_dists_knn_window): device tensors for ALL n rows, empty."""
    import torch

    return {"h_key": torch.zeros((n, knn), dtype=torch.float32, device=device),
            "h_id": torch.zeros((n, knn), dtype=torch.int32, device=device),
            "h_d1": torch.zeros((n, knn), dtype=torch.float32, device=device) if coreacc else None,
            "h_len": torch.zeros((n,), dtype=torch.int32, device=device),
            "thr": torch.full((n,), -1, dtype=torch.int32, device=device)}     # 0xFFFFFFFF: not full


def self_dists_knn_window(ctx, s, p, knn, band_rows, band, col_lo, col_hi, heaps):
    """One row band of one participant's column window (the header's skl_self_dists_knn_window): heaps updated in place."""
    ptr = lambda t: _ptr(t)[0]
    _check(load().skl_self_dists_knn_window(ctx._h, s._h, C.byref(p), knn, band_rows, band, col_lo, col_hi, ptr(heaps["h_key"]),
                                            ptr(heaps["h_id"]), ptr(heaps["h_d1"]), ptr(heaps["h_len"]), ptr(heaps["thr"])))


def gather_bands_rccl(ctxs, bands, dst, offsets_bytes, loopback_through_rccl=False):
    """skl_gather_bands_rccl: device tensors bands[d] (made on ctxs[d]'s device and stream) land at byte offsets offsets_bytes[d]
    of the device tensor `dst` on ctxs[0]'s device; asynchronous on the contexts' streams."""
    n = len(ctxs)
    handles = (_P * n)(*[c._h for c in ctxs])
    ptrs = (_P * n)(*[_ptr(b)[0] for b in bands])
    sizes = (C.c_size_t * n)(*[b.numel() * b.element_size() for b in bands])
    offs = (C.c_size_t * n)(*[int(o) for o in offsets_bytes])
    _check(load().skl_gather_bands_rccl(handles, n, ptrs, sizes, _ptr(dst)[0], offs, int(bool(loopback_through_rccl))))


def knn_logs_alloc(n, cap, coreacc, device):
    """Accept logs of the decoupled column windows (skl_self_dists_knn_window_logged): device tensors for n rows, empty."""
    import torch

    return {"rec": torch.zeros((n, cap, 2 if coreacc else 1), dtype=torch.float32, device=device),
            "id": torch.zeros((n, cap), dtype=torch.int32, device=device),
            "len": torch.zeros((n,), dtype=torch.int32, device=device), "cap": cap}


def self_dists_knn_window_logged(ctx, s, p, knn, band_rows, band, col_lo, col_hi, heaps, logs):
    """skl_self_dists_knn_window_logged: as self_dists_knn_window, and every candidate a heap takes is appended to the row's log."""
    ptr = lambda t: _ptr(t)[0]
    _check(load().skl_self_dists_knn_window_logged(ctx._h, s._h, C.byref(p), knn, band_rows, band, col_lo, col_hi, ptr(heaps["h_key"]),
                                                   ptr(heaps["h_id"]), ptr(heaps["h_d1"]), ptr(heaps["h_len"]), ptr(heaps["thr"]),
                                                   ptr(logs["rec"]), ptr(logs["id"]), ptr(logs["len"]), logs["cap"]))


def knn_heaps_replay(ctx, heaps, r0, r1, knn, rec, ids, lens):
    """skl_knn_heaps_replay: the heaps of rows [r0, r1) (of `heaps`, arrays over all rows) are fed the logged candidates
    rec [r1 - r0, cap, 1 | 2] f32 / ids [r1 - r0, cap] i32 / lens [r1 - r0] i32 (device tensors), each row's in the order logged.
    The call is asynchronous on the CONTEXT's stream: tensors made on another stream must be complete (and stay alive) until it ran."""
    if r1 <= r0:
        return
    coreacc = heaps["h_d1"] is not None
    cap = int(rec.shape[1])
    if cap == 0:
        return
    rec, ids, lens = rec.contiguous(), ids.contiguous(), lens.contiguous()
    sl = lambda t: None if t is None else t[r0:r1]
    ptr = lambda t: _ptr(t)[0]
    _check(load().skl_knn_heaps_replay(ctx._h, r1 - r0, knn, int(coreacc), ptr(rec), ptr(ids), ptr(lens), cap, ptr(sl(heaps["h_key"])),
                                       ptr(sl(heaps["h_id"])), ptr(sl(heaps["h_d1"])), ptr(sl(heaps["h_len"])), ptr(sl(heaps["thr"]))))


def knn_heaps_finalize(ctx, heaps, r0, r1, knn, ani=False):
    """into_sorted_vec of the heaps of rows [r0, r1) -> (idx i64, d0 f32, d1 f32 | None) device tensors."""
    import torch

    dev = heaps["h_key"].device
    rows = r1 - r0
    idx = torch.empty((rows, knn), dtype=torch.int64, device=dev)
    d0 = torch.empty((rows, knn), dtype=torch.float32, device=dev)
    d1 = torch.empty((rows, knn), dtype=torch.float32, device=dev) if heaps["h_d1"] is not None else None
    if rows:
        ptr = lambda t: _ptr(t)[0]
        _check(load().skl_knn_heaps_finalize(ctx._h, rows, knn, ptr(heaps["h_key"][r0:]), ptr(heaps["h_id"][r0:]),
                                             ptr(heaps["h_d1"][r0:]) if d1 is not None else None, ptr(heaps["h_len"][r0:]), int(ani),
                                             ptr(idx), ptr(d0), ptr(d1)))
    return idx, d0, d1


def self_dists_knn_candidates(ctx, s, p, knn, row_offsets, cand):
    """Candidate-list kNN (device half of self_dists_knn_precluster, mod.rs:399-553): row i is
    compared with cand[row_offsets[i]:row_offsets[i+1]] only (ascending ids, i excluded)."""
    row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
    cand = np.ascontiguousarray(cand, dtype=np.uint32)
    assert row_offsets.size == s.n + 1 and int(row_offsets[-1]) == cand.size
    idx, d0, _ = _knn_out(s.n, knn)
    _check(load().skl_self_dists_knn_candidates(ctx._h, s._h, C.byref(p), knn, row_offsets.ctypes.data,
                                                cand.ctypes.data if cand.size else None, idx.ctypes.data,
                                                d0.ctypes.data))
    return idx, d0


def _pair_list(x):
    x = np.asarray(x)
    if x.dtype != np.uint32:
        if x.size and not np.issubdtype(x.dtype, np.integer):
            raise ValueError(f"sample indices must be integers, not {x.dtype}")
        if x.size and (int(x.min()) < 0 or int(x.max()) > 0xFFFFFFFF):   # (would wrap in the conversion)
            raise ValueError("sample index out of the uint32 range")
    return np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)


def _pair_lists(a, b):
    a, b = _pair_list(a), _pair_list(b)
    if a.size != b.size:
        raise ValueError(f"the two index lists differ in length ({a.size} and {b.size})")
    return a, b


def self_dists_pairs(ctx, s, p, a, b, out=None):
    """Distances of the listed pairs (a[x], b[x]) of one slab -> [len(a), ncols] f32, entry x at out[x]
    (skl_self_dists_pairs: any order, orientation and repeats; a[x] == b[x] allowed).  `out`: a numpy array or a
    device tensor of that shape instead."""
    a, b = _pair_lists(a, b)
    if out is None:
        out = np.zeros((a.size, ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_self_dists_pairs(ctx._h, s._h, C.byref(p), a.ctypes.data, b.ctypes.data, a.size, addr, dev))
    return out


def cross_dists_pairs(ctx, r, q, p, a, b, out=None):
    """Distances of the listed pairs (reference a[x], query b[x]) -> [len(a), ncols] f32 (skl_cross_dists_pairs)."""
    a, b = _pair_lists(a, b)
    if out is None:
        out = np.zeros((a.size, ncols(p)), dtype=np.float32)
    addr, dev = _ptr(out)
    _check(load().skl_cross_dists_pairs(ctx._h, r._h, q._h, C.byref(p), a.ctypes.data, b.ctypes.data, a.size, addr, dev))
    return out


def self_dists_knn_shared_bins(ctx, s, p, knn, skq):
    """Precluster kNN with the candidate lists built on the device from the index sketches
    (skq: [n, sketch_size] u16, row i = sample i).  -> (idx, d0, total candidate pairs)."""
    skq = np.ascontiguousarray(skq, dtype=np.uint16)
    assert skq.shape[0] == s.n
    idx, d0, _ = _knn_out(s.n, knn)
    total = C.c_uint64(0)
    _check(load().skl_self_dists_knn_shared_bins(ctx._h, s._h, C.byref(p), knn, skq.ctypes.data, skq.shape[1],
                                                 idx.ctypes.data, d0.ctypes.data, C.byref(total)))
    return idx, d0, int(total.value)


INVQ_MATCH_COUNT, INVQ_ANY_BINS, INVQ_ALL_BINS = 0, 1, 2
INVQ_TOP_MAX = 1024   # SKL_INVQ_TOP_MAX: hits per query of Inverted.top


class Inverted:
    """skl_inverted: the dense bins of an inverted index ([n_samples, sketch_size] u16, row = .ski sample index)
    resident on the device (src/inverted.rs:229-269)."""

    def __init__(self, ctx, bins):
        bins = np.ascontiguousarray(bins, dtype=np.uint16)
        assert bins.ndim == 2
        self.ctx = ctx
        self.n, self.sketch_size = bins.shape
        self._h = _P()
        _check(load().skl_inverted_create(ctx._h, bins.ctypes.data if bins.size else None, self.n, self.sketch_size,
                                          C.byref(self._h)))

    def band_queries(self, mode=INVQ_MATCH_COUNT):
        """Queries one band of skl_inverted_query takes under the context's memory budget."""
        return int(load().skl_inverted_band_queries(self.ctx._h, self._h, int(mode)))

    def query(self, queries, mode=INVQ_MATCH_COUNT):
        """queries: [n_queries, sketch_size] u16.  MATCH_COUNT -> uint32 [n_queries, n] bin-match counts;
        ANY_BINS / ALL_BINS -> uint64 [n_queries, ceil(n / 64)] bitmaps (count > 0 / count == sketch_size)."""
        queries = np.ascontiguousarray(queries, dtype=np.uint16)
        assert queries.ndim == 2 and queries.shape[1] == self.sketch_size
        nq = queries.shape[0]
        if mode == INVQ_MATCH_COUNT:
            out = np.zeros((nq, self.n), dtype=np.uint32)
        else:
            out = np.zeros((nq, (self.n + 63) // 64), dtype=np.uint64)
        _check(load().skl_inverted_query(self.ctx._h, self._h, queries.ctypes.data if queries.size else None, nq,
                                         int(mode), out.ctypes.data if out.size else None))
        return out

    def top(self, queries, top):
        """The `top` best hits of every query, selected on the device (src/lib.rs:1019-1109): (ids, counts), two uint32
        arrays [n_queries, top] ordered by the key (count << 32) | index descending -- at equal count the higher .ski index
        first; entries past min(top, n) are id 0xFFFFFFFF, count 0.  top: 1 to INVQ_TOP_MAX."""
        queries = np.ascontiguousarray(queries, dtype=np.uint16)
        assert queries.ndim == 2 and queries.shape[1] == self.sketch_size
        nq, top = queries.shape[0], int(top)
        shape = (nq, top) if 0 < top <= INVQ_TOP_MAX else (0, 0)   # (the library refuses the rest)
        ids, counts = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32)
        _check(load().skl_inverted_query_top(self.ctx._h, self._h, queries.ctypes.data if queries.size else None, nq, top,
                                             ids.ctypes.data if ids.size else None, counts.ctypes.data if counts.size else None))
        return ids, counts

    def close(self):
        if self._h:
            load().skl_inverted_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_bitmap(bits, n):
    """[n_queries, ceil(n / 64)] uint64 bitmaps -> bool [n_queries, n] (bit s % 64 of word s // 64)."""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8).reshape(bits.shape[0], -1)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :n].astype(bool)


def sketch_signs(ctx, codes, code_begin, offsets, offset_begin, kmers, num_bins, rc=True):
    """GPU bin minima of the canonical ntHash (get_signs_no_densify, sketch/mod.rs:156-176):
    -> [n_samples, nk, num_bins] uint64, u64::MAX for empty bins."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    offset_begin = np.ascontiguousarray(offset_begin, dtype=np.uint64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    n = code_begin.size - 1
    out = np.zeros((n, kmers.size, num_bins), dtype=np.uint64)
    _check(load().skl_sketch_signs(ctx._h, codes.ctypes.data if codes.size else None, code_begin.ctypes.data,
                                   offsets.ctypes.data if offsets.size else None, offset_begin.ctypes.data, n,
                                   kmers.ctypes.data, kmers.size, num_bins, int(rc), out.ctypes.data))
    return out


def pack_codes(codes, code_begin):
    """One-byte 2-bit codes -> the packed form skl_sketch_signs_packed takes: per sample ceil(len / 16) u32 words, code c at
    bits 2 (c % 16) of word c / 16, the last word zero-padded."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
    parts = []
    for s in range(code_begin.size - 1):
        c = codes[int(code_begin[s]):int(code_begin[s + 1])] & 3
        pad = (-c.size) % 16
        if pad:
            c = np.concatenate([c, np.zeros(pad, dtype=np.uint8)])
        c = c.reshape(-1, 16).astype(np.uint32)
        parts.append((c << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1, dtype=np.uint32))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)


def sketch_signs_packed(ctx, packed, code_begin, offsets, offset_begin, kmers, num_bins, rc=True):
    """skl_sketch_signs_packed: as sketch_signs, the bases already at 2 bits each (pack_codes)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    offset_begin = np.ascontiguousarray(offset_begin, dtype=np.uint64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    n = code_begin.size - 1
    out = np.zeros((n, kmers.size, num_bins), dtype=np.uint64)
    _check(load().skl_sketch_signs_packed(ctx._h, packed.ctypes.data if packed.size else None, code_begin.ctypes.data,
                                          offsets.ctypes.data if offsets.size else None, offset_begin.ctypes.data, n,
                                          kmers.ctypes.data, kmers.size, num_bins, int(rc), out.ctypes.data))
    return out


AA_LETTERS = "ACDEFGHIKLMNPQRSTVWY"


def aa_codes(seq):
    """Residue bytes -> the class codes skl_sketch_signs_aa takes: 1..20 for the letters of AA_LETTERS (either case), 0 (a
    separator) for everything else."""
    table = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(AA_LETTERS):
        table[ord(ch)] = table[ord(ch.lower())] = i + 1
    return table[np.frombuffer(bytes(seq), dtype=np.uint8)]


def sketch_aa_shape():
    """Shapes of the two kernels behind sketch_signs_aa (skl_sketch_aa_shape); short_span is a function of the longest k-mer."""
    f = load().skl_sketch_aa_shape
    return {"span_lds": f(0, 0), "wg_lds": f(1, 0), "lds_bins_max": f(2, 0), "k_staged_max": f(3, 0), "long_min": f(4, 0),
            "short_span": lambda kmax: f(5, int(kmax)), "wg_short": f(6, 0)}


def sketch_signs_aa(ctx, residues, res_begin, kmers, num_bins, level=1, concat_end_rule=False):
    """skl_sketch_signs_aa: GPU bin minima of the forward aaHash over every window of k valid residues (class codes as
    aa_codes gives them, 0 = separator) -> [n_samples, nk, num_bins] uint64, u64::MAX for empty bins."""
    residues = np.ascontiguousarray(residues, dtype=np.uint8)
    res_begin = np.ascontiguousarray(res_begin, dtype=np.uint64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    n = res_begin.size - 1
    out = np.zeros((n, kmers.size, num_bins), dtype=np.uint64)
    _check(load().skl_sketch_signs_aa(ctx._h, residues.ctypes.data if residues.size else None, res_begin.ctypes.data, n,
                                      kmers.ctypes.data, kmers.size, num_bins, int(level), int(bool(concat_end_rule)),
                                      out.ctypes.data))
    return out

FINISH_DENSIFIED, FINISH_EMPTY, FINISH_UNFINISHED = 1, 2, 4
BBITS = 14


def sketch_finish(ctx, signs, num_bins=None):
    """skl_sketch_finish: densify_bin + the 14-plane transpose of [..., num_bins] uint64 bin minima on the device ->
    (usigs [..., num_bins // 64 * 14] uint64, first_sign [...] uint64, flags [...] uint8: FINISH_* bits)."""
    signs = np.ascontiguousarray(signs, dtype=np.uint64)
    num_bins = signs.shape[-1] if num_bins is None else int(num_bins)
    lead = signs.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    usigs = np.zeros(lead + (num_bins // 64 * BBITS,), dtype=np.uint64)
    first = np.zeros(lead, dtype=np.uint64)
    flags = np.zeros(lead, dtype=np.uint8)
    _check(load().skl_sketch_finish(ctx._h, signs.ctypes.data, n, num_bins, usigs.ctypes.data, first.ctypes.data, flags.ctypes.data))
    return usigs, first, flags


def sketch_usigs_packed(ctx, packed, code_begin, offsets, offset_begin, kmers, num_bins, rc=True):
    """skl_sketch_usigs_packed: sketch_signs_packed with every (sample, k) stream finished on the device ->
    (usigs [n, nk, num_bins // 64 * 14], first_sign [n, nk], flags [n, nk]) as sketch_finish."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    offset_begin = np.ascontiguousarray(offset_begin, dtype=np.uint64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    n = code_begin.size - 1
    usigs = np.zeros((n, kmers.size, num_bins // 64 * BBITS), dtype=np.uint64)
    first = np.zeros((n, kmers.size), dtype=np.uint64)
    flags = np.zeros((n, kmers.size), dtype=np.uint8)
    _check(load().skl_sketch_usigs_packed(ctx._h, packed.ctypes.data if packed.size else None, code_begin.ctypes.data,
                                          offsets.ctypes.data if offsets.size else None, offset_begin.ctypes.data, n,
                                          kmers.ctypes.data, kmers.size, num_bins, int(rc), usigs.ctypes.data, first.ctypes.data,
                                          flags.ctypes.data))
    return usigs, first, flags


def sketch_finish_u16(ctx, signs, num_bins=None):
    """skl_sketch_finish_u16: densify_bin + `sign as u16` of [..., num_bins] uint64 bin minima on the device, any num_bins ->
    (bins [..., num_bins] uint16, flags [...] uint8: FINISH_* bits)."""
    signs = np.ascontiguousarray(signs, dtype=np.uint64)
    num_bins = signs.shape[-1] if num_bins is None else int(num_bins)
    lead = signs.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    bins = np.zeros(lead + (num_bins,), dtype=np.uint16)
    flags = np.zeros(lead, dtype=np.uint8)
    _check(load().skl_sketch_finish_u16(ctx._h, signs.ctypes.data, n, num_bins, bins.ctypes.data, flags.ctypes.data))
    return bins, flags


def sketch_bins_u16_packed(ctx, packed, code_begin, offsets, offset_begin, kmer, num_bins, rc=True):
    """skl_sketch_bins_u16_packed: sketch_signs_packed at one k-mer length with the u16 finish behind it ->
    (bins [n, num_bins] uint16, flags [n] uint8) as sketch_finish_u16."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    offset_begin = np.ascontiguousarray(offset_begin, dtype=np.uint64)
    n = code_begin.size - 1
    bins = np.zeros((n, num_bins), dtype=np.uint16)
    flags = np.zeros(n, dtype=np.uint8)
    _check(load().skl_sketch_bins_u16_packed(ctx._h, packed.ctypes.data if packed.size else None, code_begin.ctypes.data,
                                             offsets.ctypes.data if offsets.size else None, offset_begin.ctypes.data, n,
                                             int(kmer), num_bins, int(rc), bins.ctypes.data, flags.ctypes.data))
    return bins, flags


def sketch_usigs_aa(ctx, residues, res_begin, kmers, num_bins, level=1, concat_end_rule=False):
    """skl_sketch_usigs_aa: sketch_signs_aa with every (sample, k) stream finished on the device; returns as sketch_usigs_packed."""
    residues = np.ascontiguousarray(residues, dtype=np.uint8)
    res_begin = np.ascontiguousarray(res_begin, dtype=np.uint64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    n = res_begin.size - 1
    usigs = np.zeros((n, kmers.size, num_bins // 64 * BBITS), dtype=np.uint64)
    first = np.zeros((n, kmers.size), dtype=np.uint64)
    flags = np.zeros((n, kmers.size), dtype=np.uint8)
    _check(load().skl_sketch_usigs_aa(ctx._h, residues.ctypes.data if residues.size else None, res_begin.ctypes.data, n,
                                      kmers.ctypes.data, kmers.size, num_bins, int(level), int(bool(concat_end_rule)),
                                      usigs.ctypes.data, first.ctypes.data, flags.ctypes.data))
    return usigs, first, flags


class Reads:
    """skl_reads: a batch of read sets resident on the device, in the reference's padded layout (packed as
    pack_codes packs them), for skl_reads_survivors.  ctx=None asks without a device."""

    def __init__(self, ctx, packed, code_begin, offsets, offset_begin, kmers, num_bins, rc=True):
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        self.code_begin = np.ascontiguousarray(code_begin, dtype=np.uint64)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        offset_begin = np.ascontiguousarray(offset_begin, dtype=np.uint64)
        kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
        self.n, self.nk, self.num_bins = self.code_begin.size - 1, kmers.size, int(num_bins)
        self._h = _P()
        _check(load().skl_reads_create(ctx._h if ctx is not None else None, packed.ctypes.data if packed.size else None,
                                       self.code_begin.ctypes.data, offsets.ctypes.data if offsets.size else None,
                                       offset_begin.ctypes.data, self.n, kmers.ctypes.data, self.nk, self.num_bins,
                                       int(rc), C.byref(self._h)))

    def survivors(self, win_begin, win_end, thresholds, capacity):
        """-> (records uint64 [n * nk, capacity, 2] of (window start, sign), counts uint64 [n * nk]); a stream whose
        count exceeds capacity holds only `capacity` of its survivors."""
        win_begin = np.ascontiguousarray(win_begin, dtype=np.uint64)
        win_end = np.ascontiguousarray(win_end, dtype=np.uint64)
        thresholds = np.ascontiguousarray(thresholds, dtype=np.uint64)
        assert win_begin.size == self.n and win_end.size == self.n and thresholds.size == self.n * self.nk * self.num_bins
        recs = np.zeros((self.n * self.nk, int(capacity), 2), dtype=np.uint64)
        counts = np.zeros(self.n * self.nk, dtype=np.uint64)
        _check(load().skl_reads_survivors(self._h, win_begin.ctypes.data, win_end.ctypes.data, thresholds.ctypes.data,
                                          int(capacity), recs.ctypes.data if recs.size else None, counts.ctypes.data))
        return recs, counts

    def close(self):
        if self._h:
            load().skl_reads_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

# ---- raw counts ----

def self_binmatch(ctx, s):
    out = np.zeros((self_pairs(s.n), s.nk), dtype=np.uint32)
    _check(load().skl_self_binmatch(ctx._h, s._h, out.ctypes.data, 0))
    return out


def cross_binmatch(ctx, r, q):
    out = np.zeros((r.n, q.n, r.nk), dtype=np.uint32)
    _check(load().skl_cross_binmatch(ctx._h, r._h, q._h, out.ctypes.data, 0))
    return out


# ---- one-shot host forms ----

def self_dists_all_host(bins, n, kmers, sketchsize64, p, completeness=None):
    bins = np.ascontiguousarray(bins, dtype="<u8").reshape(-1)
    kmers = np.ascontiguousarray(kmers, dtype=np.uintp)
    out = np.zeros((self_pairs(n), ncols(p)), dtype=np.float32)
    comp = None if completeness is None else np.ascontiguousarray(completeness, dtype=np.float64)
    _check(load().skl_self_dists_all_host(bins.ctypes.data, n, len(kmers), kmers.ctypes.data,
                                          sketchsize64, C.byref(p),
                                          None if comp is None else comp.ctypes.data,
                                          out.ctypes.data))
    return out
