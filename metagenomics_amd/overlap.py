"""Python binding of the in-tree native library ``metagenomics_amd/lib/libmgovl.so``.

Thin ctypes layer over the C-ABI in ``include/mg_overlap.h`` (device hot path)
and ``include/mg_host.h`` (host Dataset mirror).  There is no Python or CPU
implementation of the hot path here: without the library, or without a HIP
device, every call raises.  Used by tests/ and bench.py.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Iterable, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MG_LIB") or os.path.join(_HERE, "lib", "libmgovl.so")  # MG_LIB: A/B builds (tools/)

# exchange-mode record kinds (include/mg_overlap.h); their sizes on the wire
# come from the library (mg_record_bytes: keys and runs 8 B, rows 12 B)
MG_KEYS, MG_RUNS, MG_ROWS = 0, 1, 2

EDGE_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("offset", "<u2"), ("orient", "u1"), ("flags", "u1")])
# one discovery of a read's list D(A) (mg_disc, include/mg_overlap.h): 8 bytes
DISC_DTYPE = np.dtype([("dst", "<u4"), ("offset", "<u2"), ("orient", "u1"), ("o", "u1")])
# one connected component of the discovery lists (mg_comp, include/mg_overlap.h): 16 bytes
COMP_DTYPE = np.dtype([("root", "<u4"), ("n_reads", "<u4"), ("n_disc", "<u4"), ("n_self", "<u4")])
# one entry of a read's mate list (mg_mate, include/mg_overlap.h): 8 bytes
MATE_DTYPE = np.dtype([("id", "<u4"), ("orient", "u1"), ("dataset", "u1"), ("pad", "<u2")])
# one edge whose string is spelled (mg_contig_edge, include/mg_overlap.h): 40 bytes
CONTIG_EDGE_DTYPE = np.dtype({"names": ["src", "dst", "offset", "first", "n", "tail", "orient"],
                              "formats": ["<u4", "<u4", "<u8", "<u8", "<u4", "<u4", "u1"],
                              "offsets": [0, 4, 8, 16, 24, 28, 32], "itemsize": 40})
# one placement of a read on an edge (mg_place, include/mg_overlap.h): 16 bytes
PLACE_DTYPE = np.dtype([("edge", "<u4"), ("flags", "<u4"), ("distance", "<u8")])
# the reference's bound on an insert size (OverlapGraph.cpp:1168)
MAX_INSERT_DISTANCE = 1000
# one supported pair of edges (mg_pair_support, include/mg_overlap.h): 16 bytes
PAIR_DTYPE = np.dtype([("edge1", "<u4"), ("edge2", "<u4"), ("support", "<u8")])
# status of a mate entry's path search (MG_PATH_*, include/mg_overlap.h)
PATH_SKIPPED, PATH_SAME_EDGE, PATH_NONE, PATH_FOUND, PATH_DEFERRED = range(5)
# the reference's minimumSupport (Common.h:43)
MIN_SUPPORT = 3
# one edge pair the scaffolder's mate entries support (mg_scaffold_pair, include/mg_overlap.h): 24 bytes
SCAFFOLD_PAIR_DTYPE = np.dtype([("edge1", "<u4"), ("edge2", "<u4"), ("support", "<u8"), ("distance", "<u8")])
# status of a mate entry in the scaffolder's scoring (MG_SCAF_*, include/mg_overlap.h)
SCAF_SKIPPED, SCAF_NOT_UNIQUE, SCAF_FAR, SCAF_SAME_EDGE, SCAF_COUNTED = range(5)
# one half-edge of a replayed graph's CSR (mg_chain_edge, include/mg_overlap.h): 12 bytes
CHAIN_EDGE_DTYPE = np.dtype([("dst", "<u4"), ("twin", "<u4"), ("offset", "<u2"), ("orient", "u1"), ("pad", "u1")])
# one safe chain (mg_chain, include/mg_overlap.h): 48 bytes
CHAIN_DTYPE = np.dtype({"names": ["a", "b", "pa", "pb", "n", "orient_fwd", "orient_rev", "offset_fwd", "offset_rev",
                                  "first"],
                        "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "u1", "u1", "<u8", "<u8", "<u8"],
                        "offsets": [0, 4, 8, 12, 16, 20, 21, 24, 32, 40], "itemsize": 48})
# the counters of a chain build (MG_CHAIN_*, include/mg_overlap.h)
CHAIN_INFO = ("n_interior", "n_chains", "n_contracted", "n_unsafe_chains", "n_unresolved_states", "rounds")


class Chains:
    """The safe chains of a replayed graph (OverlapEngine.chains / host_chains):
    chains[CHAIN_DTYPE] in ascending start[a] + pa, the SoA read lists of their
    edges (forward [first, first + n), reverse [first + n, first + 2 n)) and the
    build's counters (info, keys CHAIN_INFO)."""

    def __init__(self, chains, reads, offs, ors, info):
        self.chains, self.reads, self.offs, self.ors = chains, reads, offs, ors
        self.info = dict(zip(CHAIN_INFO, (int(v) for v in info)))

    def arrays(self):
        return self.chains, self.reads, self.offs, self.ors


class MgError(RuntimeError):
    pass


class _Timings(C.Structure):
    _fields_ = [("pack_ms", C.c_float), ("index_ms", C.c_float), ("contained_ms", C.c_float),
                ("overlap_ms", C.c_float), ("total_ms", C.c_float), ("scan_ms", C.c_float),
                ("probe_ms", C.c_float), ("verify_ms", C.c_float), ("upload_ms", C.c_float),
                ("ingest_ms", C.c_float), ("sort_ms", C.c_float), ("layout_ms", C.c_float)]


class _Counters(C.Structure):
    _fields_ = [("sources", C.c_uint64), ("runs", C.c_uint64), ("entries", C.c_uint64),
                ("verified", C.c_uint64), ("rows", C.c_uint64), ("live_cells", C.c_uint64),
                ("c_runs", C.c_uint64), ("c_entries", C.c_uint64), ("c_verified", C.c_uint64),
                ("c_contained", C.c_uint64), ("scan_runs", C.c_uint64), ("row_reruns", C.c_uint64),
                ("run_reruns", C.c_uint64), ("probe_vsplit", C.c_uint64)]


_lib = None


def lib() -> C.CDLL:
    """Load the native library (raises MgError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgError(f"native library missing: {LIB_PATH} (run __graft_entry__.build())")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same
    # SONAME, libamdhip64.so.7).  Loading torch first makes the library bind to
    # that instance, so device buffers are shared with torch (the multi-GPU
    # exchange buffers, sharded.py) instead of two runtimes fighting over the GPU.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    u64, u32, i32, i64 = C.c_uint64, C.c_uint32, C.c_int, C.c_int64
    vp, P = C.c_void_p, C.POINTER
    sig = {
        "mg_create": (i32, [P(vp), i32]),
        "mg_destroy": (None, [vp]),
        "mg_last_error": (C.c_char_p, [vp]),
        "mg_device_count": (i32, []),
        "mg_upload_reads_packed": (i32, [vp, vp, vp, u64, u32]),
        "mg_upload_reads_ascii": (i32, [vp, C.c_char_p, vp, u64]),
        "mg_num_reads": (u64, [vp]),
        "mg_num_rows": (u64, [vp]),
        "mg_download_reads_packed": (i32, [vp, vp, vp, P(u32)]),
        "mg_read_slots": (i32, [vp, vp]),
        "mg_build_index": (i32, [vp, u32, u32]),
        "mg_lookup_key": (i32, [vp, C.c_char_p, u32, vp, u64, P(u64)]),
        "mg_mark_contained": (i32, [vp, vp]),
        "mg_find_overlaps": (i32, [vp, P(u64)]),
        "mg_copy_rows": (i32, [vp, vp, u64, P(u64)]),
        "mg_build_discoveries": (i32, [vp, P(u64), P(C.c_float)]),
        "mg_copy_discoveries": (i32, [vp, vp, vp, u64, P(u64)]),
        "mg_build_components": (i32, [vp, P(u64), P(C.c_float)]),
        "mg_copy_components": (i32, [vp, vp, vp, u64, P(u64)]),
        "mg_find_reads": (i32, [vp, C.c_char_p, vp, u64, u32, vp, vp, P(C.c_float)]),
        "mg_build_mate_pairs": (i32, [vp, C.c_char_p, vp, u64, vp, u32, u32, i32, P(u64), vp, P(C.c_float)]),
        "mg_copy_mate_pairs": (i32, [vp, vp, vp, u64, P(u64)]),
        "mg_set_shard": (i32, [vp, u32, u32, u64, u64]),
        "mg_get_timings": (i32, [vp, P(_Timings)]),
        "mg_get_counters": (i32, [vp, P(_Counters)]),
        "mg_set_option": (i32, [vp, C.c_char_p, i64]),
        "mg_stream": (vp, [vp]),
        "mg_record_bytes": (u32, [i32]),
        "mg_ingest_ascii": (i32, [vp, C.c_char_p, vp, u64, u32, P(u64)]),
        "mg_ingest_codes": (i32, [vp, vp, u64, u64, vp, u32, P(u64)]),
        "mg_dataset_counts": (i32, [vp, P(u64), P(u64)]),
        "mg_download_frequency": (i32, [vp, vp]),
        "mg_xchg_caps": (i32, [vp, u32, u32, vp]),
        "mg_xchg_begin": (i32, [vp, u32, u32]),
        "mg_xchg_pack": (i32, [vp, i32, vp, u64, u32, vp, vp]),
        "mg_xchg_insert_keys": (i32, [vp, vp, u64, u32, vp]),
        "mg_xchg_probe": (i32, [vp, i32, vp, u64, u32, vp]),
        "mg_xchg_probe_own": (i32, [vp, vp, u64, u32, vp]),
        "mg_xchg_keys_first": (i32, [vp]),
        "mg_slots_digest": (i32, [vp, vp, u64, u32, vp, vp]),
        "mg_begin_contained": (i32, [vp, vp, P(i32)]),
        "mg_xchg_prefix_marks": (i32, [vp, vp]),
        "mg_finalize_contained": (i32, [vp, vp]),
        "mg_rows_digest": (i32, [vp, vp, u64, vp]),
        "mg_super_digest": (i32, [vp, vp]),
        "mgh_dataset_from_files": (i32, [P(C.c_char_p), i32, u64, P(vp)]),
        "mgh_dataset_from_codes": (i32, [vp, u64, u64, vp, u64, i32, P(vp)]),
        "mgh_dataset_free": (None, [vp]),
        "mgh_num_reads": (u64, [vp]),
        "mgh_num_unique": (u64, [vp]),
        "mgh_shortest": (u64, [vp]),
        "mgh_longest": (u64, [vp]),
        "mgh_packed": (i32, [vp, P(vp), P(vp), P(u32)]),
        "mgh_read_string": (i64, [vp, u64, C.c_char_p, u64]),
        "mgh_frequency": (u32, [vp, u64]),
        "mgh_find_read": (u64, [vp, C.c_char_p, u64]),
        "mgh_graph_replay": (i32, [vp, u64, vp, u64, u32, P(vp)]),
        "mgh_graph_replay_disc": (i32, [vp, vp, u64, vp, u64, u32, P(vp)]),
        "mgh_discoveries_build": (i32, [vp, u64, vp, u64, u32, vp, vp, u64, P(u64)]),
        "mgh_discoveries_check": (i32, [vp, vp, u64, vp, u64, u32]),
        "mgh_components_build": (i32, [vp, vp, u64, u64, vp, vp, u64, P(u64)]),
        "mgh_graph_replay_comp": (i32, [vp, vp, u64, vp, u64, u32, vp, vp, u64, u32, P(vp)]),
        "mgh_graph_free": (None, [vp]),
        "mgh_graph_nodes": (u64, [vp]),
        "mgh_graph_edges": (u64, [vp]),
        "mgh_graph_rows": (u64, [vp, vp, u64]),
        "mgh_parse_file": (i32, [C.c_char_p, i32, P(vp), P(vp), P(u64), P(C.c_double)]),
        "mgh_parse_files": (i32, [P(C.c_char_p), i32, i32, P(vp), P(vp), P(u64), P(C.c_double)]),
        "mgh_parse_buffer": (i32, [vp, u64, i32, P(vp), P(vp), P(u64), P(C.c_double)]),
        "mgh_parse_free": (None, [vp]),
        "mgh_read_pairs": (i32, [P(C.c_char_p), i32, P(vp), P(vp), P(u64), vp, P(C.c_double)]),
        "mgh_read_pairs_buffer": (i32, [vp, u64, P(vp), P(vp), P(u64)]),
        "mgh_mate_pairs_build": (i32, [vp, vp, u64, u32, vp, C.c_char_p, vp, u64, vp, u32, u32, vp, vp, u64, P(u64),
                                       vp, P(i64)]),
        "mgh_parse_set_min_chunk": (None, [u64]),
        "mgh_graph_contract": (i32, [vp, i32, P(u64), P(u64), P(u64)]),
        "mgh_graph_read_unitig": (i32, [C.c_char_p, vp, u64, P(vp)]),
        "mgh_graph_sort_edges": (i32, [vp]),
        "mgh_graph_save_unitig": (i32, [vp, C.c_char_p]),
        "mgh_graph_save_lists": (i32, [vp, C.c_char_p]),
        "mgh_graph_unitig_edges": (u64, [vp, vp, u64, vp, vp, vp, vp, u64, P(u64)]),
        "mg_build_contigs": (i32, [vp, vp, u64, vp, vp, vp, u64, P(u64), P(C.c_float)]),
        "mg_copy_contigs": (i32, [vp, vp, vp, u64, P(u64)]),
        "mgh_graph_contig_edges": (u64, [vp, i32, vp, u64, vp, vp, vp, u64, P(u64)]),
        "mgh_contigs_build": (i32, [vp, vp, u64, u32, vp, u64, vp, vp, vp, u64, vp, vp, u64, P(u64), C.c_char_p, u64]),
        "mgh_graph_print": (i32, [vp, vp, vp, u64, u32, vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, u64]),
        "mg_build_placements": (i32, [vp, vp, u64, vp, vp, vp, u64, P(u64), P(C.c_float)]),
        "mg_copy_placements": (i32, [vp, vp, vp, u64, P(u64)]),
        "mg_insert_sizes": (i32, [vp, vp, vp, u32, u64, vp, P(C.c_float)]),
        "mg_edge_coverage": (i32, [vp, vp, vp, P(C.c_float)]),
        "mgh_placements_build": (i32, [u64, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, P(u64), C.c_char_p, u64]),
        "mgh_insert_sizes": (i32, [u64, vp, vp, vp, vp, u32, u64, vp, C.c_char_p, u64]),
        "mgh_edge_coverage": (i32, [vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, C.c_char_p, u64]),
        "mgh_mean_sd": (None, [u64, u64, u64, P(u64), P(u64)]),
        "mgh_graph_read_locations": (u64, [vp, P(u64), vp, vp, u64]),
        "mg_mate_paths": (i32, [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, u32, vp, P(u64), P(u64), P(C.c_float)]),
        "mg_mate_paths_info": (i32, [vp, vp, vp]),
        "mg_copy_mate_paths": (i32, [vp, vp, vp, vp, vp, vp, u64]),
        "mg_copy_path_pairs": (i32, [vp, vp, u64, P(u64)]),
        "mgh_graph_edge_twins": (u64, [vp, vp, u64]),
        "mgh_graph_location_lists": (u64, [vp, P(u64), vp, vp, u64]),
        "mgh_mate_paths": (i32, [u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                 vp, u64, P(u64), vp, u64, P(u64), vp, C.c_char_p, u64]),
        "mgh_graph_merge_supported": (i32, [vp, vp, u64, u64, P(u64), C.c_char_p, u64]),
        "mg_scaffold_pairs": (i32, [vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, u32, vp, P(u64), P(C.c_float)]),
        "mg_copy_scaffold_entries": (i32, [vp, vp]),
        "mg_copy_scaffold_pairs": (i32, [vp, vp, u64, P(u64)]),
        "mg_scaffold_info": (i32, [vp, vp, vp]),
        "mgh_scaffold_pairs": (i32, [u64, vp, u64, vp, vp, vp, vp, vp, vp, u32, vp, vp, u64, P(u64), vp, C.c_char_p,
                                     u64]),
        "mgh_graph_merge_scaffold": (i32, [vp, vp, u64, u64, vp, vp, u64, u32, vp, u64, P(u64), P(u64), C.c_char_p, u64]),
        "mg_build_chains": (i32, [vp, vp, vp, u64, u64, P(u64), P(u64), vp, P(C.c_float)]),
        "mg_copy_chains": (i32, [vp, vp, u64, vp, vp, vp, u64]),
        "mgh_graph_simple_csr": (u64, [vp, vp, vp, u64]),
        "mgh_graph_from_csr": (i32, [vp, vp, u64, u64, P(vp)]),
        "mgh_chains_build": (i32, [vp, vp, u64, u64, u32, vp, u64, vp, vp, vp, u64, P(u64), P(u64), vp, C.c_char_p,
                                   u64]),
        "mgh_graph_contract_chains": (i32, [vp, vp, u64, vp, vp, vp, u64, i32, P(u64), P(u64), P(u64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name, None)
        if fn is None and os.environ.get("MG_LIB"):  # (an older variant library in an A/B: what it lacks stays unbound)
            continue
        if fn is None:
            raise AttributeError(f"{LIB_PATH}: {name} not exported")
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def device_count() -> int:
    return int(lib().mg_device_count())


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


class Dataset:
    """Host Dataset mirror (Dataset.cpp:39-65 semantics), packed reads in ID order."""

    def __init__(self, handle: C.c_void_p, keepalive=None):
        self._h = handle
        self._keep = keepalive

    @classmethod
    def from_files(cls, files: Sequence[str], min_overlap: int) -> "Dataset":
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        h = C.c_void_p()
        rc = lib().mgh_dataset_from_files(arr, len(files), min_overlap, C.byref(h))
        if rc:
            raise MgError(f"Dataset from {list(files)} failed ({'unreadable' if rc == -1 else 'unknown format'})")
        return cls(h)

    @classmethod
    def from_codes(cls, codes: np.ndarray, lens: np.ndarray, min_overlap: int, nthreads: int = 0) -> "Dataset":
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        n = codes.shape[0]
        stride = codes.shape[1] if codes.ndim == 2 else 0
        h = C.c_void_p()
        rc = lib().mgh_dataset_from_codes(_ptr(codes), n, stride, _ptr(lens), min_overlap, nthreads, C.byref(h))
        if rc:
            raise MgError("Dataset.from_codes failed")
        return cls(h)

    @classmethod
    def from_strings(cls, seqs: Iterable[str], min_overlap: int) -> "Dataset":
        seqs = list(seqs)
        maxlen = max((len(s) for s in seqs), default=1)
        table = np.full(256, 4, dtype=np.uint8)
        for ch, v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
            table[ch] = v
        codes = np.full((len(seqs), max(maxlen, 1)), 4, dtype=np.uint8)
        lens = np.zeros(len(seqs), dtype=np.uint16)
        for i, s in enumerate(seqs):
            b = np.frombuffer(s.encode(), dtype=np.uint8)
            codes[i, : len(b)] = table[b]
            lens[i] = len(b)
        return cls.from_codes(codes, lens, min_overlap)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgh_dataset_free(self._h)
            self._h = None

    @property
    def num_unique(self) -> int:
        return int(lib().mgh_num_unique(self._h))

    @property
    def num_reads(self) -> int:
        return int(lib().mgh_num_reads(self._h))

    @property
    def shortest(self) -> int:
        return int(lib().mgh_shortest(self._h))

    @property
    def longest(self) -> int:
        return int(lib().mgh_longest(self._h))

    def packed(self):
        """(words [N, wpr] uint64, lens [N] uint16) views, ID order."""
        w, l, wpr = C.c_void_p(), C.c_void_p(), C.c_uint32()
        lib().mgh_packed(self._h, C.byref(w), C.byref(l), C.byref(wpr))
        n = self.num_unique
        if n == 0:
            return np.zeros((0, wpr.value), np.uint64), np.zeros(0, np.uint16)
        words = np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_uint64)), shape=(n * wpr.value,))
        lens = np.ctypeslib.as_array(C.cast(l, C.POINTER(C.c_uint16)), shape=(n,))
        return words.reshape(n, wpr.value), lens

    def read(self, rid: int) -> str:
        n = lib().mgh_read_string(self._h, rid, None, 0)
        if n < 0:
            raise MgError(f"ID {rid} out of bound.")
        buf = C.create_string_buffer(n + 1)
        lib().mgh_read_string(self._h, rid, buf, n + 1)
        return buf.value.decode()

    def frequency(self, rid: int) -> int:
        return int(lib().mgh_frequency(self._h, rid))

    def find(self, s: str) -> int:
        b = s.encode()
        return int(lib().mgh_find_read(self._h, b, len(b)))


class OverlapEngine:
    """One device context (include/mg_overlap.h)."""

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        rc = L.mg_create(C.byref(h), device)
        if rc == -3:
            raise MgError("no HIP device available: the overlap path has no CPU fallback")
        if rc:
            raise MgError(f"mg_create({device}) failed: {rc}")
        self._h = h
        self.n_reads = 0
        self.lengths_differ = False
        self.max_len = 0  # longest uploaded read (> 1024 bp: long-read kernels, no exchange mode)

    def close(self):
        if getattr(self, "_h", None):
            lib().mg_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int, what: str):
        if rc:
            msg = lib().mg_last_error(self._h)
            raise MgError(f"{what}: {msg.decode() if msg else rc}")

    # --- reads
    def upload(self, ds: Dataset):
        words, lens = ds.packed()
        self.upload_packed(words, lens)

    def upload_packed(self, words: np.ndarray, lens: np.ndarray):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        wpr = words.shape[1] if words.ndim == 2 else 1
        self._check(lib().mg_upload_reads_packed(self._h, _ptr(words), _ptr(lens), lens.shape[0], wpr), "upload")
        self.n_reads = int(lens.shape[0])
        self.lengths_differ = bool(lens.shape[0]) and int(lens.min()) != int(lens.max())
        self.max_len = int(lens.max()) if lens.shape[0] else 0

    def upload_ascii(self, seqs: Sequence[str]):
        data = "".join(seqs).encode()
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        self._check(lib().mg_upload_reads_ascii(self._h, data, _ptr(off), len(seqs)), "upload_ascii")
        self.n_reads = len(seqs)
        self.lengths_differ = len({len(x) for x in seqs}) > 1
        self.max_len = max((len(x) for x in seqs), default=0)

    def ingest_ascii(self, seqs: Sequence[str] | None = None, min_overlap: int = 0, text: bytes | None = None,
                     offsets: np.ndarray | None = None) -> int:
        """Dataset ingest on the device (mg_ingest_ascii): raw reads -> unique
        canonical reads in ID order, resident for build_index.  Returns the
        number of unique reads."""
        if text is None:
            text = "".join(seqs).encode()
            offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(s) for s in seqs])
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nu = C.c_uint64()
        self._check(lib().mg_ingest_ascii(self._h, text, _ptr(offsets), offsets.shape[0] - 1, min_overlap,
                                          C.byref(nu)), "ingest_ascii")
        self._after_ingest()
        return int(nu.value)

    def ingest_files(self, files: Sequence[str], min_overlap: int, nthreads: int = 0) -> dict:
        """Dataset(pe, se, l) on the device from FASTA/FASTQ files: the host
        splits the records (mgh_parse_files: mmap, all threads), the device
        canonicalises, sorts and deduplicates them (mg_ingest_ascii).  The
        record buffers go straight from the splitter to the device.  Returns
        {"n_unique", "n_records", "parse_s", "ingest_s"}."""
        L = lib()
        arr = (C.c_char_p * len(files))(*[os.fsencode(f) for f in files])
        t, o, n, sec = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
        rc = L.mgh_parse_files(arr, len(files), nthreads, C.byref(t), C.byref(o), C.byref(n), C.byref(sec))
        if rc:
            raise MgError({-1: f"Unable to open file: {list(files)}", -2: f"Unknown input file format: {list(files)}"}
                          .get(rc, f"parse failed ({rc})"))
        try:
            nu = C.c_uint64()
            t0 = time.perf_counter()
            self._check(L.mg_ingest_ascii(self._h, C.cast(t, C.c_char_p), o, n.value, min_overlap, C.byref(nu)),
                        "ingest_files")
            t1 = time.perf_counter()
        finally:
            L.mgh_parse_free(t)
            L.mgh_parse_free(o)
        self._after_ingest()
        return {"n_unique": int(nu.value), "n_records": int(n.value), "parse_s": sec.value, "ingest_s": t1 - t0}

    def ingest_codes(self, codes: np.ndarray, lens: np.ndarray, min_overlap: int) -> int:
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        stride = codes.shape[1] if codes.ndim == 2 else 0
        nu = C.c_uint64()
        self._check(lib().mg_ingest_codes(self._h, _ptr(codes), lens.shape[0], stride, _ptr(lens), min_overlap,
                                          C.byref(nu)), "ingest_codes")
        self._after_ingest()
        return int(nu.value)

    def _after_ingest(self):
        self.n_reads = int(lib().mg_num_reads(self._h))
        if self.n_reads:
            _, lens = self.download_packed()
            self.lengths_differ = int(lens.min()) != int(lens.max())
            self.max_len = int(lens.max())
        else:
            self.lengths_differ = False
            self.max_len = 0

    def dataset_counts(self):
        g, u = C.c_uint64(), C.c_uint64()
        lib().mg_dataset_counts(self._h, C.byref(g), C.byref(u))
        return int(g.value), int(u.value)

    def frequency(self) -> np.ndarray:
        f = np.zeros(self.n_reads, dtype=np.uint32)
        self._check(lib().mg_download_frequency(self._h, _ptr(f)), "download_frequency")
        return f

    def download_packed(self):
        wpr = C.c_uint32()
        lib().mg_download_reads_packed(self._h, None, None, C.byref(wpr))
        words = np.zeros((self.n_reads, wpr.value), np.uint64)
        lens = np.zeros(self.n_reads, np.uint16)
        self._check(lib().mg_download_reads_packed(self._h, _ptr(words), _ptr(lens), C.byref(wpr)), "download")
        return words, lens

    def slot_of_ids(self) -> np.ndarray:
        """Device slot of each read, indexed by ID - 1 (mg_read_slots)."""
        s = np.zeros(self.n_reads, dtype=np.uint32)
        self._check(lib().mg_read_slots(self._h, _ptr(s)), "read_slots")
        return s.astype(np.int64)

    # --- hot path
    def set_option(self, name: str, value: int):
        self._check(lib().mg_set_option(self._h, name.encode(), int(value)), f"option {name}")

    def set_shard(self, rank: int, nranks: int, read_lo: int = 0, read_hi: int = 0):
        self._check(lib().mg_set_shard(self._h, rank, nranks, read_lo, read_hi), "set_shard")

    def build_index(self, min_overlap: int, seed_k: int = 0):
        self._check(lib().mg_build_index(self._h, min_overlap, seed_k), "build_index")

    def mark_contained(self, copy: bool = True):
        """superReadID per ID (index 0 unused); copy=False keeps it on the device."""
        if not copy:
            self._check(lib().mg_mark_contained(self._h, None), "mark_contained")
            return None
        sup = np.zeros(self.n_reads + 1, dtype=np.uint32)
        self._check(lib().mg_mark_contained(self._h, _ptr(sup)), "mark_contained")
        return sup

    def find_overlaps(self) -> int:
        n = C.c_uint64()
        self._check(lib().mg_find_overlaps(self._h, C.byref(n)), "find_overlaps")
        return int(n.value)

    def rows(self, n_rows: int | None = None) -> np.ndarray:
        if n_rows is None:
            n_rows = self.find_overlaps()
        out = np.zeros(n_rows, dtype=EDGE_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_rows(self._h, _ptr(out), n_rows, C.byref(got)), "copy_rows")
        return out[: got.value]

    def num_rows(self) -> int:
        """Rows held after the last find_overlaps / xchg_probe(0) (mg_num_rows)."""
        return int(lib().mg_num_rows(self._h))

    def copy_rows_to(self, host_ptr: int, cap: int) -> int:
        """mg_copy_rows into caller-owned host memory (e.g. a pinned buffer of cap * 12 bytes)."""
        got = C.c_uint64()
        self._check(lib().mg_copy_rows(self._h, C.c_void_p(host_ptr), cap, C.byref(got)), "copy_rows")
        return int(got.value)

    # --- per-read discovery lists D(A), grouped and ordered on the device
    def build_discoveries(self) -> int:
        """mg_build_discoveries: the rows of the last find_overlaps grouped into
        every read's D(A) in insertAllEdgesOfRead's loop order.  Returns the total
        list length; disc_ms keeps the device time of the grouping."""
        n, ms = C.c_uint64(), C.c_float()
        self._check(lib().mg_build_discoveries(self._h, C.byref(n), C.byref(ms)), "build_discoveries")
        self.disc_ms = float(ms.value)
        self._n_disc = int(n.value)
        return self._n_disc

    def discoveries(self):
        """(start uint64[n_reads + 2], disc[DISC_DTYPE]): D(A) = disc[start[A]:start[A + 1]]."""
        n = getattr(self, "_n_disc", 0)
        start = np.zeros(self.n_reads + 2, dtype=np.uint64)
        disc = np.zeros(n, dtype=DISC_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_discoveries(self._h, _ptr(start), _ptr(disc), n, C.byref(got)), "copy_discoveries")
        return start, disc[: got.value]

    # --- read lookup and mate pairs
    @staticmethod
    def _records(seqs, text, offsets):
        if text is None:
            text = "".join(seqs).encode()
            offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(s) for s in seqs])
        return text, np.ascontiguousarray(offsets, dtype=np.uint64)

    def find_reads(self, seqs: Sequence[str] | None = None, min_overlap: int = 0, text: bytes | None = None,
                   offsets: np.ndarray | None = None):
        """mg_find_reads: Dataset::getReadFromString for a batch of raw records
        (any case), over the resident reads.  Returns (ids uint32, flags uint8):
        ids[i] = the ID of the read equal to the record's canonical string, 0
        when the record fails the ingest's filter or no read equals it; flags
        bit 0 = passed the filter, bit 1 = the record itself is the stored
        string.  find_ms keeps the device time."""
        text, offsets = self._records(seqs, text, offsets)
        n = offsets.shape[0] - 1
        ids = np.zeros(n, dtype=np.uint32)
        flags = np.zeros(n, dtype=np.uint8)
        ms = C.c_float()
        self._check(lib().mg_find_reads(self._h, text, _ptr(offsets), n, min_overlap, _ptr(ids), _ptr(flags),
                                        C.byref(ms)), "find_reads")
        self.find_ms = float(ms.value)
        return ids, flags

    def build_mate_pairs(self, text: bytes, offsets: np.ndarray, pairs_per_dataset, min_overlap: int,
                         use_super: bool = True) -> int:
        """mg_build_mate_pairs over parsed pairs (records 2p, 2p + 1 = pair p).
        Returns the total list length; mates_ms, good_pairs, bad_pairs keep
        the device time and the pair counts."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ppd = np.ascontiguousarray(pairs_per_dataset, dtype=np.uint64)
        n, ms = C.c_uint64(), C.c_float()
        gb = np.zeros(2, dtype=np.uint64)
        self._n_mates = 0
        rc = lib().mg_build_mate_pairs(self._h, text, _ptr(offsets), offsets.shape[0] - 1, _ptr(ppd), ppd.shape[0],
                                       min_overlap, int(bool(use_super)), C.byref(n), _ptr(gb), C.byref(ms))
        self.good_pairs, self.bad_pairs = int(gb[0]), int(gb[1])
        self._check(rc, "build_mate_pairs")
        self.mates_ms = float(ms.value)
        self._n_mates = int(n.value)
        return self._n_mates

    def mate_lists(self):
        """(start uint64[n_reads + 2], records[MATE_DTYPE]): the mate list of read
        A = records[start[A]:start[A + 1]] in addMatePair's order."""
        n = getattr(self, "_n_mates", 0)
        start = np.zeros(int(lib().mg_num_reads(self._h)) + 2, dtype=np.uint64)
        recs = np.zeros(n, dtype=MATE_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_mate_pairs(self._h, _ptr(start), _ptr(recs), n, C.byref(got)), "copy_mate_pairs")
        return start, recs[: got.value]

    def mate_pairs(self, files: Sequence[str], min_overlap: int, use_super: bool = True):
        """storeMatePairInformation of the paired-end `files` on the device:
        the serial pair reader (mgh_read_pairs), then mg_build_mate_pairs and
        mg_copy_mate_pairs.  Returns (start, records)."""
        text, offsets, ppd, _ = read_pairs(files)
        self.build_mate_pairs(text, offsets, ppd, min_overlap, use_super)
        return self.mate_lists()

    # --- contig strings (getStringInEdge of many edges at once)
    def build_contigs(self, edges: np.ndarray, reads: np.ndarray, offs: np.ndarray, ors: np.ndarray):
        """mg_build_contigs + mg_copy_contigs: the strings of `edges`
        (CONTIG_EDGE_DTYPE; UnitigGraph.contig_edges gives them) over the resident
        reads.  Returns (start uint64[n_edges + 1], bytes): the string of edge k
        is bytes[start[k]:start[k + 1]].  contigs_ms keeps the device time of the
        kernels.  An invalid piece raises MgError naming the edge (-2)."""
        edges, reads, offs, ors = _contig_args(edges, reads, offs, ors)
        total, ms = C.c_uint64(), C.c_float()
        self._check(lib().mg_build_contigs(self._h, _ptr(edges), edges.shape[0], _ptr(reads), _ptr(offs), _ptr(ors),
                                           reads.shape[0], C.byref(total), C.byref(ms)), "build_contigs")
        self.contigs_ms = float(ms.value)
        start = np.zeros(edges.shape[0] + 1, dtype=np.uint64)
        out = np.zeros(max(int(total.value), 1), dtype=np.uint8)
        got = C.c_uint64()
        self._check(lib().mg_copy_contigs(self._h, _ptr(start), _ptr(out), total.value, C.byref(got)), "copy_contigs")
        return start, out[: got.value].tobytes()

    # --- read placements, insert sizes and edge coverage
    def build_placements(self, edges: np.ndarray, reads: np.ndarray, offs: np.ndarray, ors: np.ndarray) -> int:
        """mg_build_placements (updateReadLocations of every edge): `edges` and
        the lists as UnitigGraph.contig_edges(all_edges=True) gives them.  Returns
        the number of placements; places_ms keeps the device time of the kernels.
        A read ID outside 1..n_reads raises MgError naming the edge and entry (-2)."""
        edges, reads, offs, ors = _contig_args(edges, reads, offs, ors)
        n, ms = C.c_uint64(), C.c_float()
        self._n_places, self._n_place_edges = 0, 0
        self._check(lib().mg_build_placements(self._h, _ptr(edges), edges.shape[0], _ptr(reads), _ptr(offs), _ptr(ors),
                                              reads.shape[0], C.byref(n), C.byref(ms)), "build_placements")
        self.places_ms = float(ms.value)
        self._n_places, self._n_place_edges = int(n.value), int(edges.shape[0])
        return self._n_places

    def placements(self):
        """(start uint64[n_reads + 2], records[PLACE_DTYPE]): the placements of read
        A = records[start[A]:start[A + 1]] in ascending (edge, list position)."""
        n = getattr(self, "_n_places", 0)
        start = np.zeros(int(lib().mg_num_reads(self._h)) + 2, dtype=np.uint64)
        recs = np.zeros(n, dtype=PLACE_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_placements(self._h, _ptr(start), _ptr(recs), n, C.byref(got)), "copy_placements")
        return start, recs[: got.value]

    def insert_size_sums(self, n_datasets: int, mates=None, max_distance: int = MAX_INSERT_DISTANCE) -> np.ndarray:
        """mg_insert_sizes: uint64[n_datasets, 3] = count, sum and sum of squares
        of the insert sizes per dataset (mean_sd finishes them).  mates = None:
        the resident lists of build_mate_pairs; else a (start, records) CSR as
        mate_lists returns.  insert_ms keeps the kernel's device time."""
        sums = np.zeros((n_datasets, 3), dtype=np.uint64)
        ms = C.c_float()
        if mates is None:
            rc = lib().mg_insert_sizes(self._h, None, None, n_datasets, max_distance, _ptr(sums), C.byref(ms))
        else:
            mstart = np.ascontiguousarray(mates[0], dtype=np.uint64)
            recs = np.ascontiguousarray(mates[1], dtype=MATE_DTYPE)
            if mstart.shape[0] != int(lib().mg_num_reads(self._h)) + 2 or (mstart.shape[0] and
                                                                           int(mstart[-1]) > recs.shape[0]):
                raise MgError("insert_size_sums: the mate CSR does not fit the resident reads")
            rc = lib().mg_insert_sizes(self._h, _ptr(mstart), _ptr(recs), n_datasets, max_distance, _ptr(sums),
                                       C.byref(ms))
        self._check(rc, "insert_sizes")
        self.insert_ms = float(ms.value)
        return sums

    def edge_coverage(self, freq=None) -> np.ndarray:
        """mg_edge_coverage over the edges of the last build_placements:
        uint64[n_edges, 3] = count, sum and sum of squares over each edge's
        non-zero per-base counters (getBaseByBaseCoverage; mean_sd finishes
        them).  freq = frequency per read ID (freq[id - 1]), or None: the
        frequencies the device ingest left.  coverage_ms keeps the device time."""
        out = np.zeros((getattr(self, "_n_place_edges", 0), 3), dtype=np.uint64)
        ms = C.c_float()
        if freq is not None:
            freq = np.ascontiguousarray(freq, dtype=np.uint32)
            if freq.shape[0] != int(lib().mg_num_reads(self._h)):
                raise MgError("edge_coverage: one frequency per resident read")
        self._check(lib().mg_edge_coverage(self._h, None if freq is None else _ptr(freq), _ptr(out), C.byref(ms)),
                    "edge_coverage")
        self.coverage_ms = float(ms.value)
        return out

    # --- mate-pair path support
    def mate_paths(self, edges, twin, mean, sd, places=None, mates=None, n_reads: int | None = None) -> "PathSupport":
        """mg_mate_paths: the scoring half of findSupportByMatepairsAndMerge
        (OverlapGraph.cpp:1892-1966) on the device.  edges / twin as
        UnitigGraph.contig_edges(all_edges=True) / edge_twins give them; places =
        a (start, records) placement CSR in the reference's list order
        (UnitigGraph.location_lists), or None: the resident placements of
        build_placements (the same supported set; multiplicities can differ only
        when a path repeats an adjacent pair); mates = a (start, records) mate
        CSR, or None: the resident lists; mean / sd per dataset.  Returns the
        device's PathSupport; entries the device deferred (option path_budget)
        are still PATH_DEFERRED in it: PathSupport.finish() (or
        UnitigGraph.mate_support) completes them with the host mirror.
        paths_ms = (explore kernels, aggregate) device time."""
        edges = np.ascontiguousarray(edges, dtype=CONTIG_EDGE_DTYPE)
        twin = np.ascontiguousarray(twin, dtype=np.uint32)
        mean = np.ascontiguousarray(mean, dtype=np.uint64)
        sd = np.ascontiguousarray(sd, dtype=np.uint64)
        if twin.shape[0] != edges.shape[0] or mean.shape != sd.shape or mean.ndim != 1:
            raise MgError("mate_paths: one twin per edge, one mean and one sd per dataset")
        if places is not None:
            places = (np.ascontiguousarray(places[0], dtype=np.uint64), np.ascontiguousarray(places[1], dtype=PLACE_DTYPE))
        if mates is not None:
            mates = (np.ascontiguousarray(mates[0], dtype=np.uint64), np.ascontiguousarray(mates[1], dtype=MATE_DTYPE))
        if n_reads is None:
            n_reads = (places[0].shape[0] - 2 if places is not None else
                       mates[0].shape[0] - 2 if mates is not None else int(lib().mg_num_reads(self._h)))
        for csr in (places, mates):
            if csr is not None and (csr[0].shape[0] != n_reads + 2 or int(csr[0][-1]) > csr[1].shape[0]):
                raise MgError("mate_paths: a CSR does not fit n_reads")
        counters = np.zeros(3, dtype=np.uint64)
        npairs, ndef, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        self._check(lib().mg_mate_paths(self._h, _ptr(edges), _ptr(twin), edges.shape[0], n_reads,
                                        None if places is None else _ptr(places[0]),
                                        None if places is None else _ptr(places[1]),
                                        None if mates is None else _ptr(mates[0]),
                                        None if mates is None else _ptr(mates[1]), _ptr(mean), _ptr(sd), mean.shape[0],
                                        _ptr(counters), C.byref(npairs), C.byref(ndef), C.byref(ms)), "mate_paths")
        info, times = np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.float32)
        self._check(lib().mg_mate_paths_info(self._h, _ptr(info), _ptr(times)), "mate_paths_info")
        self.paths_ms = (float(times[0]), float(times[1]))
        m, npath = int(info[0]), int(info[1])
        status, visits = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint32)
        start = np.zeros(m + 1, dtype=np.uint64)
        path, flags = np.zeros(npath, dtype=np.uint32), np.zeros(npath, dtype=np.uint8)
        self._check(lib().mg_copy_mate_paths(self._h, _ptr(status), _ptr(visits), _ptr(start), _ptr(path), _ptr(flags),
                                             npath), "copy_mate_paths")
        pairs = np.zeros(npairs.value, dtype=PAIR_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_path_pairs(self._h, _ptr(pairs), pairs.shape[0], C.byref(got)), "copy_path_pairs")
        # the resident CSRs come back to the host only if finish() has deferred entries to search
        return PathSupport(status, visits, start, path, flags, pairs[: got.value], counters, int(ndef.value),
                           (n_reads, edges, twin, places if places is not None else self.placements,
                            mates if mates is not None else self.mate_lists, mean, sd))

    # --- scaffolder support
    def scaffold_pairs(self, twin, n_edges: int, mean, sd, places=None, mates=None,
                       n_reads: int | None = None) -> "ScaffoldSupport":
        """mg_scaffold_pairs: the scoring half of OverlapGraph::scaffolder
        (OverlapGraph.cpp:2120-2195) on the device.  twin as
        UnitigGraph.edge_twins gives it (n_edges entries); places = a (start,
        records) placement CSR, or None: the resident placements of
        build_placements (identical results: only lists of one placement are
        read); mates = a (start, records) mate CSR, or None: the resident lists;
        mean / sd per dataset.  scaffold_ms = (score kernel, aggregate) device
        time."""
        twin = np.ascontiguousarray(twin, dtype=np.uint32)
        mean = np.ascontiguousarray(mean, dtype=np.uint64)
        sd = np.ascontiguousarray(sd, dtype=np.uint64)
        if twin.shape[0] != n_edges or mean.shape != sd.shape or mean.ndim != 1:
            raise MgError("scaffold_pairs: one twin per edge, one mean and one sd per dataset")
        if places is not None:
            places = (np.ascontiguousarray(places[0], dtype=np.uint64), np.ascontiguousarray(places[1], dtype=PLACE_DTYPE))
        if mates is not None:
            mates = (np.ascontiguousarray(mates[0], dtype=np.uint64), np.ascontiguousarray(mates[1], dtype=MATE_DTYPE))
        if n_reads is None:
            n_reads = (places[0].shape[0] - 2 if places is not None else
                       mates[0].shape[0] - 2 if mates is not None else int(lib().mg_num_reads(self._h)))
        for csr in (places, mates):
            if csr is not None and (csr[0].shape[0] != n_reads + 2 or int(csr[0][-1]) > csr[1].shape[0]):
                raise MgError("scaffold_pairs: a CSR does not fit n_reads")
        counters = np.zeros(5, dtype=np.uint64)
        npairs, ms = C.c_uint64(), C.c_float()
        self._check(lib().mg_scaffold_pairs(self._h, _ptr(twin), n_edges, n_reads,
                                            None if places is None else _ptr(places[0]),
                                            None if places is None else _ptr(places[1]),
                                            None if mates is None else _ptr(mates[0]),
                                            None if mates is None else _ptr(mates[1]), _ptr(mean), _ptr(sd),
                                            mean.shape[0], _ptr(counters), C.byref(npairs), C.byref(ms)),
                    "scaffold_pairs")
        info, times = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.float32)
        self._check(lib().mg_scaffold_info(self._h, _ptr(info), _ptr(times)), "scaffold_info")
        self.scaffold_ms = (float(times[0]), float(times[1]))
        status = np.zeros(int(info[0]), dtype=np.uint8)
        self._check(lib().mg_copy_scaffold_entries(self._h, _ptr(status)), "copy_scaffold_entries")
        pairs = np.zeros(npairs.value, dtype=SCAFFOLD_PAIR_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_scaffold_pairs(self._h, _ptr(pairs), pairs.shape[0], C.byref(got)),
                    "copy_scaffold_pairs")
        return ScaffoldSupport(status, pairs[: got.value], counters)

    # --- connected components of the lists, labelled on the device
    def build_components(self) -> int:
        """mg_build_components: label every read with the smallest read ID its
        discovery records connect it to and list the components that hold
        records, on the device.  Returns the number of components; comp_ms keeps
        the device time."""
        n, ms = C.c_uint64(), C.c_float()
        self._n_comp = None
        self._check(lib().mg_build_components(self._h, C.byref(n), C.byref(ms)), "build_components")
        self.comp_ms = float(ms.value)
        self._n_comp = int(n.value)
        return self._n_comp

    def components(self):
        """(label uint32[n_reads + 1], comps[COMP_DTYPE] in ascending root): label[0] = 0."""
        n = getattr(self, "_n_comp", None) or 0
        label = np.zeros(int(lib().mg_num_reads(self._h)) + 1, dtype=np.uint32)
        comps = np.zeros(n, dtype=COMP_DTYPE)
        got = C.c_uint64()
        self._check(lib().mg_copy_components(self._h, _ptr(label), _ptr(comps), n, C.byref(got)), "copy_components")
        return label, comps[: got.value]

    # --- safe chains of a replayed graph, ranked on the device
    def build_chains(self, start: np.ndarray, edges: np.ndarray) -> int:
        """mg_build_chains on a replayed graph's CSR (simple_csr): finds the safe
        chains by list ranking and emits the read lists of their edges, on the
        device.  Needs no reads and no index.  Returns the number of chains;
        chains_ms keeps the device time, chain_info the counters (CHAIN_INFO)."""
        start, edges = _chain_csr(start, edges)
        self._chain_csr = (start, edges)  # (the arrays outlive the call)
        n, nl, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        info = np.zeros(len(CHAIN_INFO), dtype=np.uint64)
        self._n_chains = None
        rc = lib().mg_build_chains(self._h, _ptr(start), _ptr(edges), start.shape[0] - 2, edges.shape[0], C.byref(n),
                                   C.byref(nl), _ptr(info), C.byref(ms))
        self._check(rc, "build_chains")
        self.chains_ms = float(ms.value)
        self.chain_info = dict(zip(CHAIN_INFO, (int(v) for v in info)))
        self._n_chains = (int(n.value), int(nl.value))
        return int(n.value)

    def chains(self) -> "Chains":
        """mg_copy_chains: the table and lists of the last build_chains."""
        n, nl = getattr(self, "_n_chains", None) or (0, 0)
        ch = np.zeros(n, dtype=CHAIN_DTYPE)
        reads, offs, ors = np.zeros(nl, dtype=np.uint32), np.zeros(nl, dtype=np.uint16), np.zeros(nl, dtype=np.uint8)
        self._check(lib().mg_copy_chains(self._h, _ptr(ch), n, _ptr(reads), _ptr(offs), _ptr(ors), nl), "copy_chains")
        return Chains(ch, reads, offs, ors, [self.chain_info[k] for k in CHAIN_INFO])

    def lookup(self, key: str):
        n = C.c_uint64()
        cap = 1024
        while True:
            buf = np.zeros(cap, dtype=np.uint64)
            self._check(lib().mg_lookup_key(self._h, key.encode(), len(key), _ptr(buf), cap, C.byref(n)), "lookup")
            if n.value <= cap:
                return [(int(x & ((1 << 62) - 1)), int(x >> 62)) for x in buf[: n.value]]
            cap = int(n.value)

    # --- exchange mode (one process per GPU; metagenomics_amd/sharded.py drives it).
    # Buffers and counts are device pointers in the slot layout of include/mg_overlap.h.
    def xchg_caps(self, min_overlap: int, seed_k: int = 0) -> np.ndarray:
        c = np.zeros(3, dtype=np.uint64)
        self._check(lib().mg_xchg_caps(self._h, min_overlap, seed_k, _ptr(c)), "xchg_caps")
        return c

    @staticmethod
    def record_bytes(what: int) -> int:
        """Bytes per exchange record of kind what (mg_record_bytes)."""
        return int(lib().mg_record_bytes(what))

    def xchg_begin(self, min_overlap: int, seed_k: int = 0):
        self._check(lib().mg_xchg_begin(self._h, min_overlap, seed_k), "xchg_begin")

    def xchg_pack(self, what: int, dptr: int, slot: int, rounds: int, counts_dptr: int, self_dptr: int = 0):
        """self_dptr: the receive buffer; this rank's own stream is written there directly."""
        self._check(lib().mg_xchg_pack(self._h, what, C.c_void_p(dptr or 0), slot, rounds, C.c_void_p(counts_dptr),
                                       C.c_void_p(self_dptr or 0)), "xchg_pack")

    def xchg_insert_keys(self, dptr: int, slot: int, rounds: int, counts_dptr: int):
        self._check(lib().mg_xchg_insert_keys(self._h, C.c_void_p(dptr), slot, rounds, C.c_void_p(counts_dptr)),
                    "xchg_insert_keys")

    def xchg_probe(self, contain: bool, dptr: int, slot: int, rounds: int, counts_dptr: int):
        self._check(lib().mg_xchg_probe(self._h, int(contain), C.c_void_p(dptr), slot, rounds,
                                        C.c_void_p(counts_dptr)), "xchg_probe")

    def xchg_probe_own(self, dptr: int, slot: int, rounds: int, send_counts_dptr: int):
        """mg_xchg_probe_own: the discovery probe of this rank's own run stream (already in the
        receive buffer after xchg_pack) while the peers' streams travel; xchg_probe(False) then
        probes theirs and appends.  A no-op where the step cannot split (one rank, mixed lengths)."""
        self._check(lib().mg_xchg_probe_own(self._h, C.c_void_p(dptr), slot, rounds, C.c_void_p(send_counts_dptr)),
                    "xchg_probe_own")

    def xchg_prefix_marks(self, marks_dptr: int | None):
        """mg_xchg_prefix_marks: this rank's offset-0 containments now, their marks
        (n_reads bytes) for the caller's MAX all-reduce before xchg_probe(True)."""
        self._check(lib().mg_xchg_prefix_marks(self._h, C.c_void_p(marks_dptr or 0)), "xchg_prefix_marks")

    def begin_contained(self, superkey_dptr: int | None) -> bool:
        need = C.c_int()
        self._check(lib().mg_begin_contained(self._h, C.c_void_p(superkey_dptr or 0), C.byref(need)),
                    "begin_contained")
        return bool(need.value)

    def finalize_contained(self, copy: bool = False):
        if not copy:
            self._check(lib().mg_finalize_contained(self._h, None), "finalize_contained")
            return None
        sup = np.zeros(self.n_reads + 1, dtype=np.uint32)
        self._check(lib().mg_finalize_contained(self._h, _ptr(sup)), "finalize_contained")
        return sup

    # --- parity digests (include/mg_overlap.h; tests/digest.py restates them)
    @staticmethod
    def _digest(a: np.ndarray) -> dict:
        return {"n": int(a[0]), "sum": int(a[1]), "xor": int(a[2]), "sum2": int(a[3])}

    def rows_digest(self, dptr: int | None = None, n: int = 0) -> dict:
        """Digest of the context's rows (dptr None) or of n mg_edge rows at device pointer dptr."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().mg_rows_digest(self._h, C.c_void_p(dptr or 0), n, _ptr(out)), "rows_digest")
        return self._digest(out)

    def slots_digest(self, dptr: int, slot: int, rounds: int, counts_dptr: int) -> dict:
        """Digest of exchange-mode rows received in the slot layout."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().mg_slots_digest(self._h, C.c_void_p(dptr), slot, rounds, C.c_void_p(counts_dptr),
                                          _ptr(out)), "slots_digest")
        return self._digest(out)

    def super_digest(self) -> dict:
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().mg_super_digest(self._h, _ptr(out)), "super_digest")
        return self._digest(out)

    def timings(self) -> dict:
        t = _Timings()
        lib().mg_get_timings(self._h, C.byref(t))
        return {k: float(getattr(t, k)) for k, _ in _Timings._fields_}

    def counters(self) -> dict:
        c = _Counters()
        lib().mg_get_counters(self._h, C.byref(c))
        return {k: int(getattr(c, k)) for k, _ in _Counters._fields_}

    def stream(self) -> int:
        return int(lib().mg_stream(self._h) or 0)


def replay_graph(rows: np.ndarray, lens: np.ndarray, min_overlap: int):
    """The reference's graph after buildOverlapGraphFromHashTable's exploration
    and transitive reduction (OverlapGraph.cpp:144-204, 574-661), replayed on a
    discovery multiset (mgh_graph_replay, host C++).  Returns (numberOfNodes,
    numberOfEdges, rows of every graph[u] list in list order, u ascending)."""
    rows = np.ascontiguousarray(rows, dtype=EDGE_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    L = lib()
    g = C.c_void_p()
    rc = L.mgh_graph_replay(_ptr(rows), rows.shape[0], _ptr(lens), lens.shape[0], min_overlap - 1, C.byref(g))
    if rc:
        raise MgError(f"graph replay failed ({rc})")
    try:
        n = int(L.mgh_graph_rows(g, None, 0))
        out = np.zeros(n, dtype=EDGE_DTYPE)
        L.mgh_graph_rows(g, _ptr(out), n)
        return int(L.mgh_graph_nodes(g)), int(L.mgh_graph_edges(g)), out
    finally:
        L.mgh_graph_free(g)


def _replay_disc(start: np.ndarray, disc: np.ndarray, lens: np.ndarray, min_overlap: int, components=None,
                 threads: int = 0) -> C.c_void_p:
    start = np.ascontiguousarray(start, dtype=np.uint64)
    disc = np.ascontiguousarray(disc, dtype=DISC_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    if start.shape[0] != lens.shape[0] + 2:
        raise MgError("discovery lists: start must have n_reads + 2 entries")
    g = C.c_void_p()
    if components is None:
        rc = lib().mgh_graph_replay_disc(_ptr(start), _ptr(disc), disc.shape[0], _ptr(lens), lens.shape[0],
                                         min_overlap - 1, C.byref(g))
    else:
        label = np.ascontiguousarray(components[0], dtype=np.uint32)
        comps = np.ascontiguousarray(components[1], dtype=COMP_DTYPE)
        if label.shape[0] != lens.shape[0] + 1:
            raise MgError("components: label must have n_reads + 1 entries")
        rc = lib().mgh_graph_replay_comp(_ptr(start), _ptr(disc), disc.shape[0], _ptr(lens), lens.shape[0],
                                         min_overlap - 1, _ptr(label), _ptr(comps), comps.shape[0], max(0, threads),
                                         C.byref(g))
    if rc:
        raise MgError(f"graph replay failed ({rc})")
    return g


def _chain_csr(start, edges):
    start = np.ascontiguousarray(start, dtype=np.uint64)
    edges = np.ascontiguousarray(edges, dtype=CHAIN_EDGE_DTYPE)
    if start.shape[0] < 2:
        raise MgError("chain CSR: start must have n_reads + 2 entries")
    return start, edges


def simple_csr(rows: np.ndarray, lens: np.ndarray, min_overlap: int):
    """(start uint64[n_reads + 2], edges[CHAIN_EDGE_DTYPE]) of the replayed graph
    of a discovery multiset (mgh_graph_replay + mgh_graph_simple_csr): u order,
    each list in list order, twin = CSR index of the reverse edge: the input
    of OverlapEngine.build_chains and host_chains."""
    rows = np.ascontiguousarray(rows, dtype=EDGE_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    L = lib()
    g = C.c_void_p()
    rc = L.mgh_graph_replay(_ptr(rows), rows.shape[0], _ptr(lens), lens.shape[0], min_overlap - 1, C.byref(g))
    if rc:
        raise MgError(f"graph replay failed ({rc})")
    try:
        return _graph_csr(g, lens.shape[0])
    finally:
        L.mgh_graph_free(g)


def _graph_csr(g, n_reads: int):
    L = lib()
    n = int(L.mgh_graph_simple_csr(g, None, None, 0))
    start = np.zeros(n_reads + 2, dtype=np.uint64)
    edges = np.zeros(n, dtype=CHAIN_EDGE_DTYPE)
    L.mgh_graph_simple_csr(g, _ptr(start), _ptr(edges), n)
    return start, edges


def host_chains(start: np.ndarray, edges: np.ndarray, rounds: int = 0) -> Chains:
    """The safe chains from the host's serial walk (mgh_chains_build,
    mg::chains_build): what OverlapEngine.chains gives, in the same order;
    rounds as the engine's option chain_rounds.  MgError (-2) names the first
    malformed entry of the CSR."""
    start, edges = _chain_csr(start, edges)
    L = lib()
    n, nl = C.c_uint64(), C.c_uint64()
    info = np.zeros(len(CHAIN_INFO), dtype=np.uint64)
    err = C.create_string_buffer(512)
    args = (_ptr(start), _ptr(edges), start.shape[0] - 2, edges.shape[0], rounds)
    chain_cap, list_cap = min(edges.shape[0], 1 << 20), 2 * (start.shape[0] - 2)  # one call, unless the table is longer
    while True:
        ch = np.zeros(chain_cap, dtype=CHAIN_DTYPE)
        reads, offs, ors = (np.zeros(list_cap, dtype=t) for t in (np.uint32, np.uint16, np.uint8))
        rc = L.mgh_chains_build(*args, _ptr(ch), chain_cap, _ptr(reads), _ptr(offs), _ptr(ors), list_cap, C.byref(n),
                                C.byref(nl), _ptr(info), err, 512)
        if rc:
            raise MgError(f"host chains failed ({rc}): {err.value.decode()}")
        if n.value <= chain_cap and nl.value <= list_cap:
            break
        chain_cap, list_cap = max(chain_cap, n.value), max(list_cap, nl.value)
    ch, reads, offs, ors = ch[: n.value], reads[: nl.value], offs[: nl.value], ors[: nl.value]
    return Chains(ch, reads, offs, ors, info)


def host_components(start: np.ndarray, disc: np.ndarray):
    """The components of the lists from the host union-find (mgh_components_build,
    mg::Components::build): (label, comps) as OverlapEngine.components gives them."""
    start = np.ascontiguousarray(start, dtype=np.uint64)
    disc = np.ascontiguousarray(disc, dtype=DISC_DTYPE)
    if start.shape[0] < 2:
        raise MgError("discovery lists: start must have n_reads + 2 entries")
    n_reads = start.shape[0] - 2
    label = np.zeros(n_reads + 1, dtype=np.uint32)
    comps = np.zeros(n_reads // 2 + 1, dtype=COMP_DTYPE)
    n = C.c_uint64()
    rc = lib().mgh_components_build(_ptr(start), _ptr(disc), disc.shape[0], n_reads, _ptr(label), _ptr(comps),
                                    comps.shape[0], C.byref(n))
    if rc:
        raise MgError(f"host components failed ({rc})")
    return label, comps[: n.value]


def host_discoveries(rows: np.ndarray, lens: np.ndarray, min_overlap: int):
    """The host grouping of rows into per-read lists (mgh_discoveries_build,
    mg::Discoveries::build): (start, disc) as OverlapEngine.discoveries gives them."""
    rows = np.ascontiguousarray(rows, dtype=EDGE_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    start = np.zeros(lens.shape[0] + 2, dtype=np.uint64)
    disc = np.zeros(rows.shape[0], dtype=DISC_DTYPE)
    n = C.c_uint64()
    rc = lib().mgh_discoveries_build(_ptr(rows), rows.shape[0], _ptr(lens), lens.shape[0], min_overlap - 1,
                                     _ptr(start), _ptr(disc), disc.shape[0], C.byref(n))
    if rc:
        raise MgError(f"host grouping failed ({rc})")
    return start, disc[: n.value]


def check_discoveries(start: np.ndarray, disc: np.ndarray, lens: np.ndarray, min_overlap: int) -> int:
    """mgh_discoveries_check: 0 when the lists are well formed (mg::Discoveries::from_lists), else its code."""
    start = np.ascontiguousarray(start, dtype=np.uint64)
    disc = np.ascontiguousarray(disc, dtype=DISC_DTYPE)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    if start.shape[0] != lens.shape[0] + 2:
        raise MgError("discovery lists: start must have n_reads + 2 entries")
    return int(lib().mgh_discoveries_check(_ptr(start), _ptr(disc), disc.shape[0], _ptr(lens), lens.shape[0],
                                           min_overlap - 1))


def replay_discoveries(start: np.ndarray, disc: np.ndarray, lens: np.ndarray, min_overlap: int, components=None,
                       threads: int = 0):
    """replay_graph on the per-read discovery lists (OverlapEngine.discoveries,
    mgh_graph_replay_disc): the same (numberOfNodes, numberOfEdges, list rows).
    components = (label, comps) (OverlapEngine.components / host_components):
    the components are replayed in parallel by `threads` host threads (0 = the
    default, mgh_graph_replay_comp); the same result, or MgError (-4) for a
    table that is not the lists'."""
    L = lib()
    g = _replay_disc(start, disc, lens, min_overlap, components, threads)
    try:
        n = int(L.mgh_graph_rows(g, None, 0))
        out = np.zeros(n, dtype=EDGE_DTYPE)
        L.mgh_graph_rows(g, _ptr(out), n)
        return int(L.mgh_graph_nodes(g)), int(L.mgh_graph_edges(g)), out
    finally:
        L.mgh_graph_free(g)


def _contig_args(edges, reads, offs, ors):
    return (np.ascontiguousarray(edges, dtype=CONTIG_EDGE_DTYPE), np.ascontiguousarray(reads, dtype=np.uint32),
            np.ascontiguousarray(offs, dtype=np.uint16), np.ascontiguousarray(ors, dtype=np.uint8))


def host_contigs(words: np.ndarray, lens: np.ndarray, edges: np.ndarray, reads: np.ndarray, offs: np.ndarray,
                 ors: np.ndarray):
    """mg::contigs_build (mgh_contigs_build): the host mirror of
    OverlapEngine.build_contigs on packed reads in ID order, on the CPU.
    Returns (start, bytes); an invalid piece raises MgError naming the edge."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    edges, reads, offs, ors = _contig_args(edges, reads, offs, ors)
    wpr = words.shape[1] if words.ndim == 2 else 1
    start = np.zeros(edges.shape[0] + 1, dtype=np.uint64)
    total = C.c_uint64()
    err = C.create_string_buffer(512)
    args = (_ptr(words), _ptr(lens), lens.shape[0], wpr, _ptr(edges), edges.shape[0], _ptr(reads), _ptr(offs),
            _ptr(ors), reads.shape[0])
    rc = lib().mgh_contigs_build(*args, _ptr(start), None, 0, C.byref(total), err, 512)
    out = np.zeros(max(int(total.value), 1), dtype=np.uint8)
    if rc == 0:
        rc = lib().mgh_contigs_build(*args, _ptr(start), _ptr(out), total.value, C.byref(total), err, 512)
    if rc:
        raise MgError(f"host_contigs: {err.value.decode() or 'bad arguments'} ({rc})")
    return start, out[: total.value].tobytes()


def mean_sd(count: int, total: int, sumsq: int):
    """(mean, sd, count) from count, sum and sum of squares as the reference
    finishes them (mgh_mean_sd: integer mean, wrapping 64-bit variance, sd
    truncated from a double); count == 0 gives (0, 0, 0)."""
    m, sd = C.c_uint64(), C.c_uint64()
    lib().mgh_mean_sd(int(count), int(total), int(sumsq), C.byref(m), C.byref(sd))
    return int(m.value), int(sd.value), int(count)


def host_placements(n_reads: int, edges, reads, offs, ors):
    """mg::placements_build (mgh_placements_build): the host mirror of
    build_placements + placements.  Returns (start, records, fwd_count)."""
    edges, reads, offs, ors = _contig_args(edges, reads, offs, ors)
    start = np.zeros(n_reads + 2, dtype=np.uint64)
    fwd = np.zeros(n_reads + 2, dtype=np.uint32)
    n = C.c_uint64()
    err = C.create_string_buffer(512)
    args = (n_reads, _ptr(edges), edges.shape[0], _ptr(reads), _ptr(offs), _ptr(ors), reads.shape[0])
    rc = lib().mgh_placements_build(*args, None, None, 0, None, C.byref(n), err, 512)
    recs = np.zeros(n.value, dtype=PLACE_DTYPE)
    if rc == 0:
        rc = lib().mgh_placements_build(*args, _ptr(start), _ptr(recs), n.value, _ptr(fwd), C.byref(n), err, 512)
    if rc:
        raise MgError(f"host_placements: {err.value.decode() or 'bad arguments'} ({rc})")
    return start, recs, fwd


def host_insert_size_sums(places, mates, n_datasets: int, max_distance: int = MAX_INSERT_DISTANCE) -> np.ndarray:
    """mg::insert_sizes (mgh_insert_sizes): the host mirror of
    insert_size_sums over a placement CSR and a mate CSR ((start, records) each)."""
    pstart = np.ascontiguousarray(places[0], dtype=np.uint64)
    precs = np.ascontiguousarray(places[1], dtype=PLACE_DTYPE)
    mstart = np.ascontiguousarray(mates[0], dtype=np.uint64)
    mrecs = np.ascontiguousarray(mates[1], dtype=MATE_DTYPE)
    if pstart.shape[0] < 2 or mstart.shape[0] != pstart.shape[0] or int(pstart[-1]) > precs.shape[0] or \
            int(mstart[-1]) > mrecs.shape[0]:
        raise MgError("host_insert_size_sums: the two CSRs do not fit each other")
    sums = np.zeros((n_datasets, 3), dtype=np.uint64)
    err = C.create_string_buffer(512)
    rc = lib().mgh_insert_sizes(pstart.shape[0] - 2, _ptr(pstart), _ptr(precs), _ptr(mstart), _ptr(mrecs), n_datasets,
                                max_distance, _ptr(sums), err, 512)
    if rc:
        raise MgError(f"host_insert_size_sums: {err.value.decode() or 'bad arguments'} ({rc})")
    return sums


def host_edge_coverage(lens: np.ndarray, freq: np.ndarray, edges, reads, offs, ors) -> np.ndarray:
    """mg::edge_coverage (mgh_edge_coverage): the host mirror of
    build_placements + edge_coverage; lens[id - 1], freq[id - 1]."""
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    if freq.shape[0] != lens.shape[0]:
        raise MgError("host_edge_coverage: one frequency per read")
    edges, reads, offs, ors = _contig_args(edges, reads, offs, ors)
    out = np.zeros((edges.shape[0], 3), dtype=np.uint64)
    err = C.create_string_buffer(512)
    rc = lib().mgh_edge_coverage(_ptr(lens), lens.shape[0], _ptr(edges), edges.shape[0], _ptr(reads), _ptr(offs),
                                 _ptr(ors), reads.shape[0], _ptr(freq), _ptr(out), err, 512)
    if rc:
        raise MgError(f"host_edge_coverage: {err.value.decode() or 'bad arguments'} ({rc})")
    return out


class PathSupport:
    """What mate_paths / host_mate_paths return: per mate entry (in (A, j)
    order) status[t] (PATH_*), visits[t] (work units) and its path
    path[start[t]:start[t + 1]] (edge indices) with flags (flags[p] = 1: the
    pair (path[p], path[p + 1]) is supported); pairs[PAIR_DTYPE] in first-seen
    order; counters = (noPathsFound, pathsFound, mpOnSameEdge); deferred = the
    entries still PATH_DEFERRED (pairs and counters then leave them out)."""

    def __init__(self, status, visits, start, path, flags, pairs, counters, deferred, inputs):
        self.status, self.visits, self.start, self.path, self.flags = status, visits, start, path, flags
        self.pairs, self.counters, self.deferred = pairs, tuple(int(x) for x in counters), int(deferred)
        self._inputs = inputs

    def paths(self):
        """[(path, flags)] per mate entry, flags without the last position's 0"""
        s = self.start
        return [(self.path[int(s[t]):int(s[t + 1])].tolist(), self.flags[int(s[t]):max(int(s[t + 1]) - 1, int(s[t]))].tolist())
                for t in range(self.status.shape[0])]

    def finish(self) -> "PathSupport":
        """The deferred entries searched by the host mirror without a limit and
        spliced in at their positions: the undeferred result.  A result of
        OverlapEngine.mate_paths over resident CSRs fetches them from its
        engine here, so call this while that engine is open and before
        build_placements or mate_pairs runs on it again: the fetched CSRs are
        checked against the entry count, not against the earlier contents."""
        if not self.deferred:
            return self
        inputs = [x() if callable(x) else x for x in self._inputs]  # (a resident CSR is fetched here, while its engine lives)
        return host_mate_paths(*inputs, prior=self)


def host_mate_paths(n_reads: int, edges, twin, places, mates, mean, sd, budget: int = 0, prior=None) -> PathSupport:
    """mg::mate_paths + mg::path_pairs (mgh_mate_paths): the host mirror of
    OverlapEngine.mate_paths over the same arrays; places / mates = (start,
    records) CSRs.  budget = work units per entry (0 = no limit).  prior = a
    PathSupport over the same input: only its PATH_DEFERRED entries are searched."""
    edges = np.ascontiguousarray(edges, dtype=CONTIG_EDGE_DTYPE)
    twin = np.ascontiguousarray(twin, dtype=np.uint32)
    pstart, precs = np.ascontiguousarray(places[0], dtype=np.uint64), np.ascontiguousarray(places[1], dtype=PLACE_DTYPE)
    mstart, mrecs = np.ascontiguousarray(mates[0], dtype=np.uint64), np.ascontiguousarray(mates[1], dtype=MATE_DTYPE)
    mean = np.ascontiguousarray(mean, dtype=np.uint64)
    sd = np.ascontiguousarray(sd, dtype=np.uint64)
    if twin.shape[0] != edges.shape[0] or mean.shape != sd.shape or mean.ndim != 1 or \
            pstart.shape[0] != n_reads + 2 or mstart.shape[0] != n_reads + 2 or \
            int(pstart[-1]) > precs.shape[0] or int(mstart[-1]) > mrecs.shape[0]:
        raise MgError("host_mate_paths: the arrays do not fit each other")
    m = int(mstart[-1])
    pr = [None] * 5
    if prior is not None:
        pr = [np.ascontiguousarray(prior.status, dtype=np.uint8), np.ascontiguousarray(prior.visits, dtype=np.uint32),
              np.ascontiguousarray(prior.start, dtype=np.uint64), np.ascontiguousarray(prior.path, dtype=np.uint32),
              np.ascontiguousarray(prior.flags, dtype=np.uint8)]
        if pr[0].shape[0] != m or pr[1].shape[0] != m or pr[2].shape[0] != m + 1 or \
                pr[3].shape[0] != int(pr[2][-1]) or pr[4].shape[0] != pr[3].shape[0]:
            raise MgError("host_mate_paths: prior does not fit the mate lists")
    status, visits = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint32)
    start = np.zeros(m + 1, dtype=np.uint64)
    counters = np.zeros(3, dtype=np.uint64)
    npath, npairs = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(512)
    path_cap, pair_cap = 4 * m + 1024, m + 1024
    while True:
        path, flags = np.zeros(path_cap, dtype=np.uint32), np.zeros(path_cap, dtype=np.uint8)
        pairs = np.zeros(pair_cap, dtype=PAIR_DTYPE)
        rc = lib().mgh_mate_paths(n_reads, _ptr(edges), _ptr(twin), edges.shape[0], _ptr(pstart), _ptr(precs),
                                  _ptr(mstart), _ptr(mrecs), _ptr(mean), _ptr(sd), mean.shape[0], budget,
                                  *(None if a is None else _ptr(a) for a in pr), _ptr(status), _ptr(visits),
                                  _ptr(start), _ptr(path), _ptr(flags), path_cap, C.byref(npath), _ptr(pairs), pair_cap,
                                  C.byref(npairs), _ptr(counters), err, 512)
        if rc:
            raise MgError(f"host_mate_paths: {err.value.decode() or 'bad arguments'} ({rc})")
        if npath.value <= path_cap and npairs.value <= pair_cap:
            break
        path_cap, pair_cap = max(path_cap, npath.value), max(pair_cap, npairs.value)  # (sized now: once more)
    return PathSupport(status, visits, start, path[: npath.value], flags[: npath.value], pairs[: npairs.value], counters,
                       int((status == PATH_DEFERRED).sum()), (n_reads, edges, twin, (pstart, precs), (mstart, mrecs), mean, sd))


class ScaffoldSupport:
    """What scaffold_pairs / host_scaffold_pairs return: status[t] (SCAF_*) per
    mate entry in (A, j) order; pairs[SCAFFOLD_PAIR_DTYPE] in first-seen order
    (listOfPairedEdges before its sort; distance = the sum over the record's
    entries); counters = the entries of each status, indexed by SCAF_*."""

    def __init__(self, status, pairs, counters):
        self.status, self.pairs = status, pairs
        self.counters = tuple(int(x) for x in counters)


def host_scaffold_pairs(n_reads: int, twin, places, mates, mean, sd) -> ScaffoldSupport:
    """mg::scaffold_pairs (mgh_scaffold_pairs): the host mirror of
    OverlapEngine.scaffold_pairs over the same arrays; places / mates = (start,
    records) CSRs."""
    twin = np.ascontiguousarray(twin, dtype=np.uint32)
    pstart, precs = np.ascontiguousarray(places[0], dtype=np.uint64), np.ascontiguousarray(places[1], dtype=PLACE_DTYPE)
    mstart, mrecs = np.ascontiguousarray(mates[0], dtype=np.uint64), np.ascontiguousarray(mates[1], dtype=MATE_DTYPE)
    mean = np.ascontiguousarray(mean, dtype=np.uint64)
    sd = np.ascontiguousarray(sd, dtype=np.uint64)
    if mean.shape != sd.shape or mean.ndim != 1 or pstart.shape[0] != n_reads + 2 or mstart.shape[0] != n_reads + 2 or \
            int(pstart[-1]) > precs.shape[0] or int(mstart[-1]) > mrecs.shape[0]:
        raise MgError("host_scaffold_pairs: the arrays do not fit each other")
    m = int(mstart[-1])
    status = np.zeros(m, dtype=np.uint8)
    pairs = np.zeros(m, dtype=SCAFFOLD_PAIR_DTYPE)  # (every record holds at least one entry)
    counters = np.zeros(5, dtype=np.uint64)
    npairs = C.c_uint64()
    err = C.create_string_buffer(512)
    rc = lib().mgh_scaffold_pairs(n_reads, _ptr(twin), twin.shape[0], _ptr(pstart), _ptr(precs), _ptr(mstart),
                                  _ptr(mrecs), _ptr(mean), _ptr(sd), mean.shape[0], _ptr(status), _ptr(pairs), m,
                                  C.byref(npairs), _ptr(counters), err, 512)
    if rc:
        raise MgError(f"host_scaffold_pairs: {err.value.decode() or 'bad arguments'} ({rc})")
    return ScaffoldSupport(status, pairs[: npairs.value], counters)


def read_pairs(files: Sequence[str] | None = None, data: bytes | None = None):
    """The mates of every pair as storeMatePairInformation's loop reads them
    (mgh_read_pairs; `data`: one file's bytes).  Returns (text bytes, offsets
    uint64[n + 1], pairs_per_file uint64, seconds): records 2p, 2p + 1 = pair p."""
    L = lib()
    t, o, n, sec = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
    if data is not None:
        ppf = np.zeros(1, dtype=np.uint64)
        buf = np.frombuffer(data, dtype=np.uint8)
        rc = L.mgh_read_pairs_buffer(_ptr(buf) if len(data) else None, len(data), C.byref(t), C.byref(o), C.byref(n))
    else:
        ppf = np.zeros(len(files), dtype=np.uint64)
        arr = (C.c_char_p * len(files))(*[os.fsencode(f) for f in files])
        rc = L.mgh_read_pairs(arr, len(files), C.byref(t), C.byref(o), C.byref(n), _ptr(ppf), C.byref(sec))
    if rc:
        raise MgError({-1: "Unable to open file", -2: "Unknown input file format."}.get(rc, f"read_pairs failed ({rc})"))
    try:
        offsets = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n.value + 1,)).copy()
        text = C.string_at(t, int(offsets[-1]))
    finally:
        L.mgh_parse_free(t)
        L.mgh_parse_free(o)
    if data is not None:
        ppf[0] = n.value // 2
    return text, offsets, ppf, sec.value


def host_mate_pairs(words: np.ndarray, lens: np.ndarray, text: bytes, offsets: np.ndarray, pairs_per_dataset,
                    min_overlap: int, super_ids: np.ndarray | None = None):
    """mg::MatePairs::build (mgh_mate_pairs_build): the host mirror of
    build_mate_pairs + mate_lists, on the CPU.  super_ids = superReadID per ID
    (n + 1 entries) or None (all 0).  Returns (start, records, good, bad)."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ppd = np.ascontiguousarray(pairs_per_dataset, dtype=np.uint64)
    n = lens.shape[0]
    wpr = words.shape[1] if words.ndim == 2 else 1
    n_raw = offsets.shape[0] - 1
    sup = None if super_ids is None else np.ascontiguousarray(super_ids, dtype=np.uint32)
    start = np.zeros(n + 2, dtype=np.uint64)
    recs = np.zeros(n_raw, dtype=MATE_DTYPE)
    cnt, nf = C.c_uint64(), C.c_int64()
    gb = np.zeros(2, dtype=np.uint64)
    rc = lib().mgh_mate_pairs_build(_ptr(words), _ptr(lens), n, wpr, None if sup is None else _ptr(sup), text,
                                    _ptr(offsets), n_raw, _ptr(ppd), ppd.shape[0], min_overlap, _ptr(start),
                                    _ptr(recs), n_raw, C.byref(cnt), _ptr(gb), C.byref(nf))
    if rc == -2:
        raise MgError(f"String not found in Dataset: raw record {nf.value}")
    if rc:
        raise MgError(f"host_mate_pairs: bad arguments ({rc})")
    return start, recs[: cnt.value], int(gb[0]), int(gb[1])


def _parse_result(L, rc, t, o, n, what):
    if rc:
        raise MgError({-1: f"Unable to open file: {what}", -2: f"Unknown input file format: {what}"}.get(
            rc, f"parse failed ({rc})"))
    try:
        offs = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n.value + 1,)).copy()
        size = int(offs[-1])
        text = (np.ctypeslib.as_array(C.cast(t, C.POINTER(C.c_uint8)), shape=(size,)).copy() if size
                else np.zeros(0, np.uint8))
    finally:
        L.mgh_parse_free(t)
        L.mgh_parse_free(o)
    return text, offs


def parse_file(path: str, nthreads: int = 0):
    """Dataset::readDataset's record splitting (Dataset.cpp:110-193) on a
    memory-mapped file with all host threads (mgh_parse_file).  Returns
    (text uint8, offsets uint64[n+1], seconds): record i's raw sequence is
    text[offsets[i]:offsets[i+1]], the input of OverlapEngine.ingest_ascii."""
    L = lib()
    t, o, n, sec = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
    rc = L.mgh_parse_file(os.fsencode(path), nthreads, C.byref(t), C.byref(o), C.byref(n), C.byref(sec))
    text, offs = _parse_result(L, rc, t, o, n, path)
    return text, offs, sec.value


def parse_buffer(data: bytes, nthreads: int = 0, min_chunk: int = 0):
    """parse_file on bytes in memory; min_chunk > 0 lowers the per-thread chunk
    size (tests: exercises the chunk seams on small inputs)."""
    L = lib()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    t, o, n, sec = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_double()
    L.mgh_parse_set_min_chunk(min_chunk)
    try:
        rc = L.mgh_parse_buffer(_ptr(buf), len(data), nthreads, C.byref(t), C.byref(o), C.byref(n), C.byref(sec))
    finally:
        L.mgh_parse_set_min_chunk(0)
    text, offs = _parse_result(L, rc, t, o, n, "<buffer>")
    return text, offs


UNITIG_EDGE_DTYPE = np.dtype({"names": ["src", "dst", "offset", "n_reads", "orient"],
                              "formats": ["<u4", "<u4", "<u8", "<u4", "u1"],
                              "offsets": [0, 4, 8, 16, 20], "itemsize": 24})


class UnitigGraph:
    """The graph new OverlapGraph(ht) returns (OverlapGraph.cpp:107-218): the
    exploration + transitive reduction replay (mgh_graph_replay), then the
    contraction loop :211-215 (contractCompositePaths + removeDeadEndNodes,
    mgh_graph_contract), on host C++.  main.cpp:48-50's sortEdges +
    saveGraphToFile are sort_edges() / save_unitig()."""

    def __init__(self, rows: np.ndarray, lens: np.ndarray, min_overlap: int, track_locations: bool = True,
                 chains=None):
        """chains: None = the reference's loop alone; "host" = the safe chains of
        the replayed graph from the host mirror contracted first; an
        OverlapEngine = the same from the device (build_chains); a Chains = that
        table (any subset of the safe chains; MgError -4 for anything else).
        The contracted graph is the same in every field."""
        rows = np.ascontiguousarray(rows, dtype=EDGE_DTYPE)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        L = self._L = lib()
        self._g = C.c_void_p()
        t0 = time.perf_counter()
        rc = L.mgh_graph_replay(_ptr(rows), rows.shape[0], _ptr(lens), lens.shape[0], min_overlap - 1,
                                C.byref(self._g))
        if rc:
            raise MgError(f"graph replay failed ({rc})")
        self._contract(t0, track_locations, chains, lens.shape[0])

    @classmethod
    def from_discoveries(cls, start: np.ndarray, disc: np.ndarray, lens: np.ndarray, min_overlap: int,
                         track_locations: bool = True, components=None, threads: int = 0,
                         chains=None) -> "UnitigGraph":
        """The same graph from the per-read discovery lists (OverlapEngine.discoveries);
        components / threads as in replay_discoveries; chains as in __init__."""
        self = cls.__new__(cls)
        self._L = lib()
        self._g = C.c_void_p()
        t0 = time.perf_counter()
        self._g = _replay_disc(start, disc, lens, min_overlap, components, threads)
        self._contract(t0, track_locations, chains, np.asarray(lens).shape[0])
        return self

    @classmethod
    def from_csr(cls, start: np.ndarray, edges: np.ndarray, track_locations: bool = True,
                 chains=None) -> "UnitigGraph":
        """The contraction of a graph given as a CSR (simple_csr's layout;
        mgh_graph_from_csr), for graphs no discovery multiset produced; chains
        as in __init__."""
        start, edges = _chain_csr(start, edges)
        self = cls.__new__(cls)
        L = self._L = lib()
        self._g = C.c_void_p()
        t0 = time.perf_counter()
        rc = L.mgh_graph_from_csr(_ptr(start), _ptr(edges), start.shape[0] - 2, edges.shape[0], C.byref(self._g))
        if rc:
            raise MgError(f"malformed CSR ({rc})")
        self._contract(t0, track_locations, chains, start.shape[0] - 2)
        return self

    def _contract(self, t0: float, track_locations: bool, chains=None, n_reads: int = 0):
        L = self._L
        self.replay_nodes, self.replay_edges = int(L.mgh_graph_nodes(self._g)), int(L.mgh_graph_edges(self._g))
        t1 = time.perf_counter()
        it, merged, dead = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.chain_info = None
        if chains is None:
            rc = L.mgh_graph_contract(self._g, int(track_locations), C.byref(it), C.byref(merged), C.byref(dead))
        else:
            if not isinstance(chains, Chains):
                csr = _graph_csr(self._g, n_reads)
                if isinstance(chains, str) and chains == "host":
                    chains = host_chains(*csr)
                elif isinstance(chains, OverlapEngine):
                    chains.build_chains(*csr)
                    chains = chains.chains()
                else:
                    self.close()
                    raise MgError("chains: None, \"host\", an OverlapEngine or a Chains")
            self.chain_info = chains.info
            ch = np.ascontiguousarray(chains.chains, dtype=CHAIN_DTYPE)
            reads = np.ascontiguousarray(chains.reads, dtype=np.uint32)
            offs = np.ascontiguousarray(chains.offs, dtype=np.uint16)
            ors = np.ascontiguousarray(chains.ors, dtype=np.uint8)
            if not (reads.shape[0] == offs.shape[0] == ors.shape[0]):
                self.close()
                raise MgError("chains: reads, offs and ors differ in length")
            rc = L.mgh_graph_contract_chains(self._g, _ptr(ch), ch.shape[0], _ptr(reads), _ptr(offs), _ptr(ors),
                                             reads.shape[0], int(track_locations), C.byref(it), C.byref(merged),
                                             C.byref(dead))
        if rc:
            self.close()
            raise MgError(f"contraction failed ({rc})")
        self.replay_s, self.contract_s = t1 - t0, time.perf_counter() - t1
        self.iterations, self.merged, self.dead_end_nodes = it.value, merged.value, dead.value

    @classmethod
    def from_unitig_file(cls, path: str, lens: np.ndarray) -> "UnitigGraph":
        """OverlapGraph::readGraphFromFile (OverlapGraph.cpp:1270-1367): the
        .unitig checkpoint of a Dataset with these read lengths back into lists."""
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        self = cls.__new__(cls)
        L = self._L = lib()
        self._g = C.c_void_p()
        rc = L.mgh_graph_read_unitig(os.fsencode(path), _ptr(lens), lens.shape[0], C.byref(self._g))
        if rc:
            raise MgError({-1: f"Unable to open file: {path}"}.get(rc, f"readGraphFromFile failed ({rc})"))
        self.replay_s = self.contract_s = 0.0
        self.replay_nodes = self.replay_edges = None
        self.iterations = self.merged = self.dead_end_nodes = 0
        return self

    @property
    def nodes(self) -> int:
        return int(self._L.mgh_graph_nodes(self._g))

    @property
    def edges(self) -> int:
        return int(self._L.mgh_graph_edges(self._g))

    def sort_edges(self):
        if self._L.mgh_graph_sort_edges(self._g):
            raise MgError("sort_edges failed")

    def save_unitig(self, path: str):
        if self._L.mgh_graph_save_unitig(self._g, os.fsencode(path)):
            raise MgError(f"cannot write {path}")

    def save_lists(self, path: str):
        if self._L.mgh_graph_save_lists(self._g, os.fsencode(path)):
            raise MgError(f"cannot write {path}")

    def unitig_edges(self):
        """(edges[UNITIG_EDGE_DTYPE], read_start, reads, offs, ors) of the current lists in list order."""
        L = self._L
        nr = C.c_uint64()
        n = int(L.mgh_graph_unitig_edges(self._g, None, 0, None, None, None, None, 0, C.byref(nr)))
        e = np.zeros(n, dtype=UNITIG_EDGE_DTYPE)
        st = np.zeros(n, dtype=np.uint64)
        reads = np.zeros(nr.value, dtype=np.uint32)
        offs = np.zeros(nr.value, dtype=np.uint16)
        ors = np.zeros(nr.value, dtype=np.uint8)
        L.mgh_graph_unitig_edges(self._g, _ptr(e), n, _ptr(st), _ptr(reads), _ptr(offs), _ptr(ors), nr.value,
                                 C.byref(nr))
        return e, st, reads, offs, ors

    def contig_edges(self, all_edges: bool = False):
        """(edges[CONTIG_EDGE_DTYPE], reads, offs, ors): printGraph's contigs in
        its selection order (OverlapGraph.cpp:460), or with all_edges every edge
        of every list in list order, as build_contigs / host_contigs take them."""
        L = self._L
        nl = C.c_uint64()
        n = int(L.mgh_graph_contig_edges(self._g, int(all_edges), None, 0, None, None, None, 0, C.byref(nl)))
        e = np.zeros(n, dtype=CONTIG_EDGE_DTYPE)
        reads = np.zeros(nl.value, dtype=np.uint32)
        offs = np.zeros(nl.value, dtype=np.uint16)
        ors = np.zeros(nl.value, dtype=np.uint8)
        L.mgh_graph_contig_edges(self._g, int(all_edges), _ptr(e), n, _ptr(reads), _ptr(offs), _ptr(ors), nl.value,
                                 C.byref(nl))
        return e, reads, offs, ors

    def read_locations(self):
        """(start uint64[n_reads + 2], records[PLACE_DTYPE]): the read locations the
        contraction (or readGraphFromFile) tracked, as placements on the edges of
        contig_edges(all_edges=True), each read's records sorted by (edge,
        distance, flags).  None when the handle tracked none."""
        nr = C.c_uint64(0)
        n = int(self._L.mgh_graph_read_locations(self._g, C.byref(nr), None, None, 0))
        if not nr.value:
            return None
        start = np.zeros(nr.value + 2, dtype=np.uint64)
        recs = np.zeros(n, dtype=PLACE_DTYPE)
        self._L.mgh_graph_read_locations(self._g, C.byref(nr), _ptr(start), _ptr(recs), n)
        return start, recs

    def location_lists(self):
        """(start uint64[n_reads + 2], records[PLACE_DTYPE]): read_locations in
        the reference's list order -- per read its forward list in list order,
        then its reverse list in list order -- the order
        findPathBetweenMatepairs walks.  None when the handle tracked none."""
        nr = C.c_uint64(0)
        n = int(self._L.mgh_graph_location_lists(self._g, C.byref(nr), None, None, 0))
        if not nr.value:
            return None
        start = np.zeros(nr.value + 2, dtype=np.uint64)
        recs = np.zeros(n, dtype=PLACE_DTYPE)
        self._L.mgh_graph_location_lists(self._g, C.byref(nr), _ptr(start), _ptr(recs), n)
        return start, recs

    def edge_twins(self) -> np.ndarray:
        """twin[k] = the index of edge k's reverse edge, both in contig_edges(all_edges=True) order"""
        n = int(self._L.mgh_graph_edge_twins(self._g, None, 0))
        twin = np.zeros(n, dtype=np.uint32)
        self._L.mgh_graph_edge_twins(self._g, _ptr(twin), n)
        return twin

    def mate_support(self, mates, mean, sd, engine=None) -> PathSupport:
        """The scoring half of findSupportByMatepairsAndMerge
        (OverlapGraph.cpp:1892-1966) over this graph: status, paths, flags,
        pairs and counters (PathSupport).  mates = a (start, records) mate CSR;
        mean / sd per dataset (insert_sizes).  With an engine: the device call,
        its deferred entries finished by the host mirror; otherwise the mirror."""
        locs = self.location_lists()
        if locs is None:
            raise MgError("mate_support: the graph tracked no read locations")
        edges = self.contig_edges(all_edges=True)[0]
        twin = self.edge_twins()
        if engine is not None:
            return engine.mate_paths(edges, twin, mean, sd, places=locs, mates=mates).finish()
        return host_mate_paths(locs[0].shape[0] - 2, edges, twin, locs, mates, mean, sd)

    def scaffold_support(self, mates, mean, sd, engine=None) -> "ScaffoldSupport":
        """The scoring half of scaffolder() (OverlapGraph.cpp:2120-2195) over
        this graph: statuses, records and counters (ScaffoldSupport).  mates = a
        (start, records) mate CSR; mean / sd per dataset (insert_sizes).  With
        an engine: the device call; otherwise the host mirror."""
        locs = self.location_lists()
        if locs is None:
            raise MgError("scaffold_support: the graph tracked no read locations")
        twin = self.edge_twins()
        if engine is not None:
            return engine.scaffold_pairs(twin, twin.shape[0], mean, sd, places=locs, mates=mates)
        return host_scaffold_pairs(locs[0].shape[0] - 2, twin, locs, mates, mean, sd)

    def merge_scaffold(self, pairs, words, lens, min_support: int = MIN_SUPPORT):
        """The merging half of scaffolder() (OverlapGraph.cpp:2197-2219): std::sort
        of the records by support, then, for every record no earlier merge freed
        with support >= min_support, the reference's "are supported" line and
        mergeEdgesDisconnected.  pairs[SCAFFOLD_PAIR_DTYPE] index
        contig_edges(all_edges=True) of the graph as it is now; words / lens =
        the packed reads in ID order (Dataset.packed()).  Returns
        (pairsOfEdgesMerged, the lines as one string)."""
        pairs = np.ascontiguousarray(pairs, dtype=SCAFFOLD_PAIR_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        wpr = words.shape[1] if words.ndim == 2 else 1
        merged, used = C.c_uint64(), C.c_uint64()
        err = C.create_string_buffer(512)
        cap = 192 * pairs.shape[0] + 1
        lines = C.create_string_buffer(cap)
        rc = self._L.mgh_graph_merge_scaffold(self._g, _ptr(pairs), pairs.shape[0], min_support, _ptr(words), _ptr(lens),
                                              lens.shape[0], wpr, lines, cap, C.byref(used), C.byref(merged), err, 512)
        if rc:
            raise MgError(f"merge_scaffold: {err.value.decode() or 'bad arguments'} ({rc})")
        return int(merged.value), lines.raw[: used.value].decode()

    def merge_supported(self, pairs, min_support: int = MIN_SUPPORT) -> int:
        """The merging half (OverlapGraph.cpp:1968-1992): std::sort of the pairs
        by support, then mergeEdges of every pair no earlier merge freed with
        support >= min_support.  pairs[PAIR_DTYPE] index contig_edges(all_edges=True)
        of the graph as it is now.  Returns pairsOfEdgesMerged."""
        pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        merged = C.c_uint64()
        err = C.create_string_buffer(512)
        rc = self._L.mgh_graph_merge_supported(self._g, _ptr(pairs), pairs.shape[0], min_support, C.byref(merged), err,
                                               512)
        if rc:
            raise MgError(f"merge_supported: {err.value.decode() or 'bad arguments'} ({rc})")
        return int(merged.value)

    def insert_sizes(self, mates, n_datasets: int, engine=None, max_distance: int = MAX_INSERT_DISTANCE):
        """calculateMeanAndSdOfInsertSize (OverlapGraph.cpp:1124-1211) over this
        graph's edges: [(mean, sd, count)] per dataset.  mates = a (start, records)
        mate CSR, or None with an engine that holds build_mate_pairs' lists.  With
        an engine that holds the reads the placements and the sums are built on
        the device, otherwise by the host mirrors."""
        args = self.contig_edges(all_edges=True)
        if engine is not None:
            engine.build_placements(*args)
            sums = engine.insert_size_sums(n_datasets, mates, max_distance)
        else:
            if mates is None:
                raise MgError("insert_sizes: the host mirror needs the mate lists")
            start, recs, _ = host_placements(np.asarray(mates[0]).shape[0] - 2, *args)
            sums = host_insert_size_sums((start, recs), mates, n_datasets, max_distance)
        return [mean_sd(*(int(x) for x in row)) for row in sums]

    def edge_coverage(self, lens=None, freq=None, engine=None):
        """getBaseByBaseCoverage (OverlapGraph.cpp:2722-2792) of every edge of
        contig_edges(all_edges=True): [(coverageDepth, SD, non-zero bases)] per
        edge.  With an engine that holds the reads: one device call (freq = None
        takes the ingest's frequencies); otherwise the host mirror over lens and
        freq (per read ID)."""
        args = self.contig_edges(all_edges=True)
        if engine is not None:
            engine.build_placements(*args)
            sums = engine.edge_coverage(freq)
        else:
            if lens is None or freq is None:
                raise MgError("edge_coverage: the host mirror needs lens and freq")
            sums = host_edge_coverage(lens, freq, *args)
        return [mean_sd(*(int(x) for x in row)) for row in sums]

    def print_graph(self, ds, gdl: str, fasta: str, engine=None):
        """printGraph (OverlapGraph.cpp:428-520): the .gdl file and the contigs as
        FASTA.  ds = the Dataset (or a (words, lens) pair in ID order).  With an
        engine that holds these reads the strings are built on the device
        (OverlapEngine.build_contigs), otherwise by the host mirror."""
        words, lens = ds.packed() if hasattr(ds, "packed") else ds
        words = np.ascontiguousarray(words, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        wpr = words.shape[1] if words.ndim == 2 else 1
        start = strings = None
        if engine is not None:
            start, strings = engine.build_contigs(*self.contig_edges())
            strings = np.frombuffer(strings + b"\0", dtype=np.uint8)
        err = C.create_string_buffer(512)
        rc = self._L.mgh_graph_print(self._g, _ptr(words), _ptr(lens), lens.shape[0], wpr,
                                     None if start is None else _ptr(start),
                                     None if strings is None else _ptr(strings), os.fsencode(gdl), os.fsencode(fasta),
                                     err, 512)
        if rc:
            raise MgError(f"print_graph: {err.value.decode() or 'cannot write ' + gdl + ' / ' + fasta} ({rc})")

    def close(self):
        if self._g:
            self._L.mgh_graph_free(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sort_rows(rows: np.ndarray) -> np.ndarray:
    """Canonical order (src, dst, orient, offset) for multiset comparison."""
    order = np.lexsort((rows["offset"], rows["orient"], rows["dst"], rows["src"]))
    return rows[order]


def rows_to_tuples(rows: np.ndarray) -> np.ndarray:
    r = sort_rows(rows)
    return np.stack([r["src"].astype(np.int64), r["dst"].astype(np.int64), r["orient"].astype(np.int64),
                     r["offset"].astype(np.int64)], axis=1)
