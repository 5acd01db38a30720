"""stellar_random_walk_amd — Python binding (ctypes) of libstellar_rw.so, the MI355X-native engine behind the
`--cmd randomwalk` path of data61/stellar-random-walk.

This module is plumbing: every computation happens in hand-written HIP kernels behind the C ABI declared in
include/stellar_rw.h.  There is no CPU fallback — importing works anywhere (so the symbols can be checked), but
creating an Engine without a usable gfx950 device raises.
"""
import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRW_LIB") or os.path.join(_DIR, "libstellar_rw.so")   # SRW_LIB: an instrumented build (tools/)
CLI_PATH = os.path.join(_DIR, "stellar-rw")

OK, ERR_INVALID, ERR_IO, ERR_PARSE, ERR_HIP, ERR_EXISTS, ERR_NOMEM = range(7)
SAMPLER_REFERENCE, SAMPLER_ALIAS = 0, 1
RNG_CONST, RNG_PHILOX = 0, 1
CFG_OWNER_FROM_PARTITIONS = 1
CFG_COMPACT_IDS = 2
CFG_NO_MEMBERSHIP = 4
CFG_OWNER_HASH_PARTITIONER = 8
IDS_I32, IDS_I64 = 0, 1          # srw_load_coo_device: element type of the id arrays
WALK_FORCE_GENERAL = 1
WALK_NT_LOADS = 2
WALK_CACHED_LOADS = 4
WALK_LEGACY_FLUSH = 8
WALK_NO_COMPACT = 16
WALK_NO_PREFIX = 32
WALK_NO_EDGE_HASH = 64
WALK_NO_BINNED = 128
WALK_NO_HUB_BITMAPS = 65536
WALK_DEVICE_FORMAT = 131072
WALK_NO_EDGE_TABLES = 262144
WALK_EDGE_TABLES_ALL = 524288
NBR_NO_COMPACT = 1               # srw_neighbor_params.flags
NBR_MAX_LAYERS, NBR_MAX_FANOUT, NBR_MAX_DISTINCT_FANOUT = 8, 4096, 64      # srw_sample_neighbors' limits
IMP_KEEP_SEED, IMP_NO_COMPACT = 1, 2                                       # srw_importance_params.flags
IMP_MAX_WALKS, IMP_MAX_LENGTH, IMP_MAX_VISITS, IMP_MAX_TOP = 4096, 4096, 4096, 64   # srw_importance_neighbors' limits


class W2vParams(C.Structure):
    _fields_ = [("dim", C.c_int32), ("window", C.c_int32), ("iterations", C.c_int32), ("learning_rate", C.c_float),
                ("seed", C.c_uint32), ("threads", C.c_int32)]


def w2v_save(vocab_ids, vectors, output_dir, n_parts=1):
    """<output_dir>/vec/part-* ("id\\tv0\\t..." lines, Main.scala:88-91) + <output_dir>/bin."""
    ids = np.ascontiguousarray(vocab_ids, dtype=np.int32); vec = np.ascontiguousarray(vectors, dtype=np.float32)
    rc = lib().srw_w2v_save(_i32(ids), _f32(vec), len(ids), vec.shape[1] if vec.ndim == 2 else 1, os.fsencode(output_dir), n_parts)
    if rc != 0:
        raise SrwError(rc, "srw_w2v_save: %s" % lib().srw_last_error(None).decode())


class SkipgramParams(C.Structure):
    _fields_ = [("context", C.c_int32), ("num_negatives", C.c_int32), ("seed", C.c_uint32), ("epoch", C.c_uint32)]


class SkipgramBatchParams(C.Structure):
    _fields_ = [("context", C.c_int32), ("num_negatives", C.c_int32), ("seed", C.c_uint32), ("epoch", C.c_uint32),
                ("exclude_window", C.c_int32), ("max_draws", C.c_int32)]


class SgnsParams(C.Structure):
    _fields_ = [("context", C.c_int32), ("num_negatives", C.c_int32), ("dim", C.c_int32), ("center", C.c_int32),
                ("lr", C.c_float), ("reserved", C.c_int32)]


class TopkParams(C.Structure):
    _fields_ = [("dim", C.c_int32), ("k", C.c_int32), ("metric", C.c_int32), ("reserved", C.c_int32)]


TOPK_METRICS = {"cosine": 0, "dot": 1}     # srw_topk_params.metric


class NeighborParams(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("epoch", C.c_uint32), ("replace", C.c_int32), ("flags", C.c_int32)]


class ImportanceParams(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("epoch", C.c_uint32), ("base", C.c_uint32), ("num_walks", C.c_int32),
                ("walk_length", C.c_int32), ("top", C.c_int32), ("restart_m", C.c_uint32), ("flags", C.c_int32)]


class SrwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("srw error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("flags", C.c_int32)]


class WalkParams(C.Structure):
    _fields_ = [("p", C.c_float), ("q", C.c_float), ("walk_length", C.c_int32), ("num_walks", C.c_int32),
                ("first_walk", C.c_int32), ("rng_mode", C.c_int32), ("const_r", C.c_float), ("seed", C.c_uint32),
                ("sampler", C.c_int32), ("flags", C.c_int32)]


class WalkStats(C.Structure):
    _fields_ = [("n_walkers", C.c_int64), ("n_steps", C.c_int64), ("dead_ends", C.c_int64),
                ("sum_deg_curr", C.c_int64), ("sum_deg_prev", C.c_int64), ("ent_reads", C.c_int64),
                ("fallbacks", C.c_int64), ("trials", C.c_int64), ("kernel_ms", C.c_double), ("kernel_kind", C.c_int32),
                ("record_bytes", C.c_int32), ("strategy_steps", C.c_int64 * 12), ("edge_tables", C.c_int64),
                ("edge_table_bytes", C.c_int64), ("setup_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["strategy_steps"] = dict(zip(STRATEGIES, list(self.strategy_steps)))
        return d


class ShardLayout(C.Structure):
    _fields_ = [("cap_walkers", C.c_int64), ("cap_rets", C.c_int64), ("chunk_bytes", C.c_int64)]


STRATEGIES = ("edge_table", "p1", "p2", "w", "p3", "scan", "prefix", "chain", "edge_mask", "q1_lane", "handed_over_walkers", "ties_resolved")   # SRW_STRAT_*


# every symbol include/stellar_rw.h declares
EXPORTS = [
    "srw_create", "srw_destroy", "srw_last_error", "srw_set_stream", "srw_plan_walks", "srw_load_edgelist", "srw_load_coo", "srw_load_coo_device",
    "srw_load_adjacency", "srw_generate_rmat", "srw_graph_stats", "srw_graph_vertices", "srw_graph_neighbors",
    "srw_graph_partition", "srw_alias_row", "srw_walk", "srw_walk_to_host", "srw_walk_and_save", "srw_set_sources", "srw_set_sources_device", "srw_clear_sources", "srw_sources", "srw_vertex_types_set", "srw_vertex_types", "srw_walk_metapath", "srw_sample_neighbors", "srw_importance_neighbors", "srw_host_alloc", "srw_host_free", "srw_fetch_paths", "srw_device_paths", "srw_write_paths",
    "srw_shard_capacity", "srw_shard_vertex_ranks", "srw_shard_layout_for", "srw_shard_begin", "srw_shard_superstep",
    "srw_shard_flush", "srw_shard_finish", "srw_shard_rows_count", "srw_shard_rows_export", "srw_shard_rows_merge",
    "srw_shard_rows_commit", "srw_shard_rows_release", "srw_device_alloc", "srw_device_free", "srw_cluster_create", "srw_cluster_destroy", "srw_cluster_last_error",
    "srw_cluster_shard", "srw_cluster_load_edgelist", "srw_cluster_load_coo", "srw_cluster_generate_rmat",
    "srw_cluster_graph_stats", "srw_cluster_walk", "srw_cluster_fetch_paths", "srw_cluster_walk_and_save",
    "srw_cluster_set_sources", "srw_cluster_clear_sources", "srw_cluster_sources",
    "srw_shard_select", "srw_w2v_fit", "srw_w2v_fit_device", "srw_skipgram_windows", "srw_negative_weights_set", "srw_graph_degrees_device", "srw_path_vertex_counts", "srw_skipgram_batch", "srw_sgns_step", "srw_topk_rows", "srw_vertex_rows", "srw_w2v_huffman", "srw_w2v_save", "srw_w2v_save_words", "srw_probe_request_rate", "srw_result_scan_sums", "srw_sample", "srw_second_order_weights",
    "srw_second_order_sample", "srw_rng_uniform", "srw_cfo_pick", "srw_parse_edgelist", "srw_parse_sources", "srw_free", "srw_save_paths", "srw_table_geometry", "srw_version",
]

_lib = None


def lib():
    """Loads libstellar_rw.so.  Fails loudly if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libstellar_rw.so is missing at %s — build it with `make -C %s/csrc` "
                          "(there is no CPU fallback)" % (LIB_PATH, _DIR))
    L = C.CDLL(LIB_PATH)
    vp, i32p, i64p, f32p, u32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), \
        C.POINTER(C.c_uint32)
    L.srw_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.srw_destroy.argtypes = [vp]
    L.srw_destroy.restype = None
    L.srw_last_error.argtypes = [vp]
    L.srw_last_error.restype = C.c_char_p
    L.srw_set_stream.argtypes = [vp, vp]
    L.srw_plan_walks.argtypes = [vp, C.c_int64]
    L.srw_load_edgelist.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.srw_load_coo.argtypes = [vp, i32p, i32p, f32p, i32p, C.c_int64, C.c_int32]
    L.srw_load_coo_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32]
    L.srw_load_adjacency.argtypes = [vp, i32p, i64p, C.c_int64, i32p, f32p, i32p]
    L.srw_generate_rmat.argtypes = [vp, C.c_int32, C.c_int64, C.c_uint32, C.c_int32, C.c_int32]
    L.srw_graph_stats.argtypes = [vp, i64p, i64p]
    L.srw_graph_vertices.argtypes = [vp, i32p]
    L.srw_graph_neighbors.argtypes = [vp, C.c_int32, i32p, f32p, C.c_int64, i64p]
    L.srw_graph_partition.argtypes = [vp, C.c_int32, i32p, i32p]
    L.srw_alias_row.argtypes = [vp, C.c_int32, f32p, i32p, C.c_int64, i64p, i32p]
    L.srw_walk.argtypes = [vp, C.POINTER(WalkParams), C.POINTER(WalkStats)]
    L.srw_walk_to_host.argtypes = [vp, C.POINTER(WalkParams), i32p, i32p, C.POINTER(WalkStats)]
    L.srw_walk_and_save.argtypes = [vp, C.POINTER(WalkParams), C.c_char_p, C.c_int32, C.c_int32, C.POINTER(WalkStats), i64p]
    L.srw_set_sources.argtypes = [vp, i32p, C.c_int64]
    L.srw_set_sources_device.argtypes = [vp, vp, C.c_int64]
    L.srw_clear_sources.argtypes = [vp]
    L.srw_sources.argtypes = [vp, i64p]
    L.srw_vertex_types_set.argtypes = [vp, vp, C.c_int64]
    L.srw_vertex_types.argtypes = [vp, i64p]
    L.srw_walk_metapath.argtypes = [vp, C.POINTER(WalkParams), i32p, C.c_int32, C.POINTER(WalkStats)]
    L.srw_sample_neighbors.argtypes = [vp, vp, C.c_int64, i32p, C.c_int32, C.POINTER(NeighborParams), C.POINTER(vp), i64p]
    L.srw_importance_neighbors.argtypes = [vp, vp, C.c_int64, C.POINTER(ImportanceParams), vp, vp, vp, i64p]
    L.srw_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.srw_host_free.argtypes = [vp]
    L.srw_host_free.restype = None
    L.srw_fetch_paths.argtypes = [vp, i32p, i32p]
    L.srw_device_paths.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i64p, i32p]
    L.srw_write_paths.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
    L.srw_shard_capacity.argtypes = [vp, i64p, i64p]
    L.srw_shard_vertex_ranks.argtypes = [vp, i32p]
    L.srw_shard_layout_for.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(ShardLayout)]
    L.srw_shard_begin.argtypes = [vp, C.POINTER(WalkParams), C.c_int32, C.POINTER(ShardLayout), vp, vp, vp]
    L.srw_shard_superstep.argtypes = [vp, C.POINTER(WalkParams), C.c_int32, C.c_int32, C.POINTER(ShardLayout), vp,
                                      C.POINTER(vp), vp, vp]
    L.srw_shard_flush.argtypes = [vp, C.POINTER(WalkParams), C.c_int32, C.POINTER(ShardLayout), vp, vp, vp]
    L.srw_shard_finish.argtypes = [vp, C.POINTER(WalkStats), i32p]
    L.srw_shard_rows_count.argtypes = [vp, i64p]
    L.srw_shard_rows_export.argtypes = [vp, vp, C.c_int64]
    L.srw_shard_rows_merge.argtypes = [vp, vp, vp, C.c_int64]
    L.srw_shard_rows_commit.argtypes = [vp, vp, C.c_int64, i32p]
    L.srw_shard_rows_release.argtypes = [vp]
    L.srw_device_alloc.argtypes = [vp, C.c_int64, C.POINTER(vp)]
    L.srw_device_free.argtypes = [vp, vp]
    L.srw_cluster_create.argtypes = [i32p, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.srw_cluster_destroy.argtypes = [vp]
    L.srw_cluster_destroy.restype = None
    L.srw_cluster_last_error.argtypes = [vp]
    L.srw_cluster_last_error.restype = C.c_char_p
    L.srw_cluster_shard.argtypes = [vp, C.c_int32]
    L.srw_cluster_shard.restype = vp
    L.srw_cluster_load_edgelist.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.srw_cluster_load_coo.argtypes = [vp, i32p, i32p, f32p, i32p, C.c_int64, C.c_int32]
    L.srw_cluster_generate_rmat.argtypes = [vp, C.c_int32, C.c_int64, C.c_uint32, C.c_int32, C.c_int32]
    L.srw_cluster_graph_stats.argtypes = [vp, i64p, i64p]
    L.srw_cluster_walk.argtypes = [vp, C.POINTER(WalkParams), C.c_int32, C.POINTER(WalkStats)]
    L.srw_cluster_fetch_paths.argtypes = [vp, i32p, i32p]
    L.srw_cluster_walk_and_save.argtypes = [vp, C.POINTER(WalkParams), C.c_char_p, C.c_int32, C.c_int32, C.POINTER(WalkStats)]
    L.srw_cluster_set_sources.argtypes = [vp, i32p, C.c_int64]
    L.srw_cluster_clear_sources.argtypes = [vp]
    L.srw_cluster_sources.argtypes = [vp, i64p]
    L.srw_shard_select.argtypes = [vp, C.c_int32]
    L.srw_w2v_fit.argtypes = [vp, i32p, i32p, C.c_int64, C.c_int64, C.POINTER(W2vParams), C.POINTER(i32p), C.POINTER(f32p), C.POINTER(C.c_int64)]
    L.srw_w2v_fit_device.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.POINTER(W2vParams), C.POINTER(i32p), C.POINTER(f32p), C.POINTER(C.c_int64)]
    L.srw_skipgram_windows.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.POINTER(SkipgramParams), vp, vp, C.c_int64, i64p]
    L.srw_negative_weights_set.argtypes = [vp, vp, C.c_int64]
    L.srw_graph_degrees_device.argtypes = [vp, vp]
    L.srw_path_vertex_counts.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, vp, i64p]
    L.srw_skipgram_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.POINTER(SkipgramBatchParams), vp, vp, C.c_int64, i64p]
    L.srw_sgns_step.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(SgnsParams), vp, vp, vp, vp, C.c_int64, vp, i64p]
    L.srw_topk_rows.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(TopkParams), vp, vp, i64p]
    L.srw_vertex_rows.argtypes = [vp, vp, C.c_int64, vp, i64p]
    L.srw_w2v_save_words.argtypes = [C.POINTER(C.c_char_p), f32p, C.c_int64, C.c_int32, C.c_char_p, C.c_int32]
    L.srw_w2v_huffman.argtypes = [C.POINTER(C.c_int64), C.c_int64, i32p, C.POINTER(C.c_uint8), i32p]
    L.srw_w2v_save.argtypes = [i32p, f32p, C.c_int64, C.c_int32, C.c_char_p, C.c_int32]
    L.srw_probe_request_rate.argtypes = [vp, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.srw_result_scan_sums.argtypes = [vp, i64p]
    L.srw_sample.argtypes = [vp, f32p, C.c_int64, C.c_float, i64p]
    L.srw_second_order_weights.argtypes = [vp, C.c_float, C.c_float, C.c_int32, i32p, C.c_int64, i32p, f32p,
                                           C.c_int64, f32p]
    L.srw_second_order_sample.argtypes = [vp, C.c_float, C.c_float, C.c_int32, i32p, C.c_int64, i32p, f32p,
                                          C.c_int64, C.c_float, i64p]
    L.srw_rng_uniform.argtypes = [vp, C.c_uint32, u32p, u32p, u32p, C.c_int64, f32p]
    L.srw_cfo_pick.argtypes = [vp, C.c_int32, u32p, C.c_int64, i32p, i32p]
    L.srw_parse_edgelist.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(i32p), C.POINTER(i32p),
                                     C.POINTER(f32p), C.POINTER(i32p), i64p, C.c_char_p, C.c_size_t]
    L.srw_parse_sources.argtypes = [C.c_char_p, C.POINTER(i32p), i64p, C.c_char_p, C.c_size_t]
    L.srw_free.argtypes = [vp]
    L.srw_free.restype = None
    L.srw_save_paths.argtypes = [i32p, i32p, C.c_int64, C.c_int64, C.c_char_p, C.c_int32, C.c_int32]
    L.srw_table_geometry.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.srw_version.restype = C.c_char_p
    _lib = L
    return L


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def version():
    return lib().srw_version().decode()


def parse_edgelist(path, weighted=True, partitioned=False):
    """Host-only: the edge-list tokenizer (UniformRandomWalk.scala:26-34 / VCutRandomWalk.scala:21-34 rules).
    Returns (src, dst, w, pid) numpy arrays in file order; raises SrwError(ERR_PARSE) where the reference throws."""
    L = lib()
    s, d, p = (C.POINTER(C.c_int32)() for _ in range(3))
    w = C.POINTER(C.c_float)()
    n = C.c_int64(0)
    err = C.create_string_buffer(512)
    rc = L.srw_parse_edgelist(os.fsencode(path), int(weighted), int(partitioned), C.byref(s), C.byref(d), C.byref(w),
                              C.byref(p), C.byref(n), err, 512)
    if rc != OK:
        raise SrwError(rc, err.value.decode())
    k = n.value
    out = tuple(np.ctypeslib.as_array(x, shape=(max(k, 1),))[:k].copy() for x in (s, d, w, p))
    for x in (s, d, w, p):
        L.srw_free(x)
    return out


def parse_sources(path):
    """Host-only: the ids of a --sources file (white-space separated, the edge list's id rule), in file order."""
    L = lib()
    ids, n = C.POINTER(C.c_int32)(), C.c_int64(0)
    err = C.create_string_buffer(512)
    rc = L.srw_parse_sources(os.fsencode(path), C.byref(ids), C.byref(n), err, 512)
    if rc != OK:
        raise SrwError(rc, err.value.decode(errors="replace"))
    out = np.ctypeslib.as_array(ids, shape=(max(n.value, 1),))[:n.value].copy()
    L.srw_free(ids)
    return out


def save_paths(paths, lens, output_dir, n_parts=1, write_crc=False):
    paths = np.ascontiguousarray(paths, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    rc = lib().srw_save_paths(_i32(paths), _i32(lens), len(lens), paths.shape[1] if paths.ndim == 2 else 0,
                              os.fsencode(output_dir), n_parts, int(write_crc))
    if rc != OK:
        raise SrwError(rc, lib().srw_last_error(None).decode())


class _DeviceArray:
    """int32 words in HBM that the library owns, as the CUDA array interface spells them (what torch.as_tensor wraps without a copy)."""

    def __init__(self, ptr, shape, owner):
        self.owner = owner               # the Engine stays alive as long as a tensor over its memory does
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": "<i4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Engine:
    """One handle = one GPU.  Mirrors the life of the reference's SparkContext + GraphMap + RandomWalk object."""

    def __init__(self, device=0, rank=0, world=1, owner_from_partitions=False, compact_ids=False, membership=True, hash_partitioner=False):
        self.h = C.c_void_p()
        cfg = Config(device, rank, world, (CFG_OWNER_FROM_PARTITIONS if owner_from_partitions else 0) |
                     (CFG_COMPACT_IDS if compact_ids else 0) | (0 if membership else CFG_NO_MEMBERSHIP) |
                     (CFG_OWNER_HASH_PARTITIONER if hash_partitioner else 0))
        rc = lib().srw_create(C.byref(cfg), C.byref(self.h))
        if rc != OK:
            self.h = None
            raise SrwError(rc, lib().srw_last_error(None).decode())
        self.rank, self.world, self.device = rank, world, device

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owned", True):
                lib().srw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: module globals may already be gone
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != OK:
            raise SrwError(rc, lib().srw_last_error(self.h).decode())

    def set_stream(self, stream_ptr):
        self._ck(lib().srw_set_stream(self.h, C.c_void_p(stream_ptr)))

    def plan_walks(self, num_walks):
        """The job's --numWalks (total walk iterations over the tables the next walk builds): steers what is worth building."""
        self._ck(lib().srw_plan_walks(self.h, int(num_walks)))
        return self

    # ---- graph ----
    def load_edgelist(self, path, directed=False, weighted=True, partitioned=False, rdd_partitions=200):
        self._ck(lib().srw_load_edgelist(self.h, os.fsencode(path), int(directed), int(weighted), int(partitioned),
                                         rdd_partitions))
        return self

    def load_coo(self, src, dst=None, w=None, pid=None, directed=False):
        """The graph from already-parsed lines in file order.  numpy arrays / sequences (src, dst, optional w and pid) go through the
        host entry point (srw_load_coo).  Objects with data_ptr() and is_cuda (torch tensors) on the handle's device go through
        srw_load_coo_device, without leaving HBM: src, dst one-dimensional, contiguous, of one length and one dtype (torch.int32 or
        torch.int64) — or src alone, one contiguous [2, E] tensor (an edge_index); w a tensor of E weights (converted to float32 on
        the device if need be).  Anything else about such tensors — another dtype, rows that are not contiguous, differing lengths,
        another device, pid= (partition ids stay a host matter) — is a TypeError before the library is called.  An int64 id
        outside int32 is SrwError(ERR_INVALID) and leaves the graph loaded before in place.  CPU tensors take the host path."""
        if hasattr(src, "data_ptr") and hasattr(src, "is_cuda"):
            host = self._load_coo_tensors(src, dst, w, pid, directed)
            if host is None:
                return self
            src, dst, w = host                                           # CPU tensors: as numpy arrays, below
        if dst is None:
            raise TypeError("load_coo: dst is missing (src alone is the [2, E] form of a device tensor)")
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        wp = pp = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            wp = _f32(w)
        if pid is not None:
            pid = np.ascontiguousarray(pid, dtype=np.int32)
            pp = _i32(pid)
        self._ck(lib().srw_load_coo(self.h, _i32(src), _i32(dst), wp, pp, len(src), int(directed)))
        return self

    def _load_coo_tensors(self, src, dst, w, pid, directed):
        """load_coo's tensor form.  Device tensors: checks, then srw_load_coo_device -> None.  CPU tensors: -> (src, dst, w) as numpy."""
        is_t = lambda x: hasattr(x, "data_ptr") and hasattr(x, "is_cuda")      # noqa: E731
        if dst is None:
            if src.dim() != 2 or src.shape[0] != 2:
                raise TypeError("load_coo: one tensor must have shape [2, E] (got %s)" % (tuple(src.shape),))
            if not src.is_contiguous():
                raise TypeError("load_coo: the [2, E] tensor must be contiguous")
            src, dst = src[0], src[1]
        elif not is_t(dst):
            raise TypeError("load_coo: src is a tensor, dst is not")
        if src.dim() != 1 or dst.dim() != 1 or src.shape[0] != dst.shape[0]:
            raise TypeError("load_coo: src and dst must be one-dimensional and of one length (got %s, %s)" % (tuple(src.shape), tuple(dst.shape)))
        if not (src.is_contiguous() and dst.is_contiguous()):
            raise TypeError("load_coo: the rows of ids must be contiguous")
        if src.dtype != dst.dtype or str(src.dtype) not in ("torch.int32", "torch.int64"):
            raise TypeError("load_coo: ids must be torch.int32 or torch.int64, src and dst alike (got %s, %s)" % (src.dtype, dst.dtype))
        if src.is_cuda != dst.is_cuda or (is_t(w) and w.is_cuda != src.is_cuda):
            raise TypeError("load_coo: the tensors are on different devices")
        if not src.is_cuda:
            return src.numpy(), dst.numpy(), (w.numpy() if is_t(w) else w)
        import torch
        dev = src.device
        mine = getattr(self, "device", None)                             # (a Cluster.shard() view does not know its device)
        if dst.device != dev or (mine is not None and dev.index != mine):
            raise TypeError("load_coo: the tensors must be on the handle's device (cuda:%s), got %s, %s" % (mine, dev, dst.device))
        if pid is not None:
            raise TypeError("load_coo: pid= goes with host arrays (partition ids are not taken from the device)")
        n = int(src.shape[0])
        if w is not None:
            if not is_t(w):
                w = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32), device=dev)
            if w.device != dev:
                raise TypeError("load_coo: w must be on the ids' device (%s), got %s" % (dev, w.device))
            if w.dim() != 1 or w.shape[0] != n:
                raise TypeError("load_coo: w must hold one weight per line (%d), got shape %s" % (n, tuple(w.shape)))
            w = w.to(torch.float32).contiguous()                         # (both return w itself when there is nothing to do)
        torch.cuda.current_stream(dev).synchronize()                     # the arrays are written before the handle's stream reads them
        self._ck(lib().srw_load_coo_device(self.h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                           C.c_void_p(w.data_ptr()) if w is not None else None, n,
                                           IDS_I64 if str(src.dtype) == "torch.int64" else IDS_I32, int(directed)))
        return None

    def load_adjacency(self, rows):
        """rows: list of (vid, [(dst, w)] or [(dst, pid, w)]) — the GraphMap.addVertex surface."""
        vids = np.ascontiguousarray([r[0] for r in rows], dtype=np.int32)
        offs = np.zeros(len(rows) + 1, dtype=np.int64)
        ids, ws, pids = [], [], []
        has_pid = any(len(e) == 3 for _, nb in rows for e in nb)
        for i, (_, nb) in enumerate(rows):
            for e in nb:
                ids.append(e[0])
                ws.append(e[-1])
                pids.append(e[1] if len(e) == 3 else -1)
            offs[i + 1] = len(ids)
        ids = np.ascontiguousarray(ids if ids else [0], dtype=np.int32)
        ws = np.ascontiguousarray(ws if ws else [0], dtype=np.float32)
        pids = np.ascontiguousarray(pids if pids else [0], dtype=np.int32)
        self._ck(lib().srw_load_adjacency(self.h, _i32(vids), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(rows),
                                          _i32(ids), _f32(ws), _i32(pids) if has_pid else None))
        return self

    def generate_rmat(self, scale, n_edges=None, seed=42, weighted=False, directed=False):
        if n_edges is None:
            n_edges = 16 << scale
        self._ck(lib().srw_generate_rmat(self.h, scale, n_edges, seed, int(weighted), int(directed)))
        return self

    def stats(self):
        v, e = C.c_int64(0), C.c_int64(0)
        self._ck(lib().srw_graph_stats(self.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    @property
    def num_vertices(self):
        return self.stats()[0]

    @property
    def num_entries(self):
        return self.stats()[1]

    def shard_capacity(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(lib().srw_shard_capacity(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def vertices(self):
        n = self.shard_capacity()[0]
        out = np.zeros(max(n, 1), dtype=np.int32)
        self._ck(lib().srw_graph_vertices(self.h, _i32(out)))
        return out[:n]

    def neighbors(self, v):
        """GraphMap.getNeighbors: None for an unknown vertex, else (ids, w)."""
        n = C.c_int64(0)
        self._ck(lib().srw_graph_neighbors(self.h, v, None, None, 0, C.byref(n)))
        if n.value < 0:
            return None
        ids = np.zeros(max(n.value, 1), dtype=np.int32)
        w = np.zeros(max(n.value, 1), dtype=np.float32)
        self._ck(lib().srw_graph_neighbors(self.h, v, _i32(ids), _f32(w), n.value, C.byref(n)))
        return ids[:n.value], w[:n.value]

    def partition(self, v):
        pid, known = C.c_int32(0), C.c_int32(0)
        self._ck(lib().srw_graph_partition(self.h, v, C.byref(pid), C.byref(known)))
        return pid.value if known.value else None

    def alias_row(self, v):
        """Mode A table of vertex v: None if absent, else (regular, prob, alias)."""
        n, reg = C.c_int64(0), C.c_int32(0)
        self._ck(lib().srw_alias_row(self.h, v, None, None, 0, C.byref(n), C.byref(reg)))
        if n.value < 0:
            return None
        prob = np.zeros(max(n.value, 1), dtype=np.float32)
        alias = np.zeros(max(n.value, 1), dtype=np.int32)
        self._ck(lib().srw_alias_row(self.h, v, _f32(prob), _i32(alias), n.value, C.byref(n), C.byref(reg)))
        return reg.value, prob[:n.value], alias[:n.value]

    # ---- start vertices ----
    def set_sources(self, ids):
        """Walk from these vertex ids (any order, duplicates allowed) instead of from every vertex, until clear_sources() or the
        next load: walker index = iteration * len(ids) + position.  A numpy array / sequence goes through the host entry point; an
        object with data_ptr() and is_cuda (a torch tensor on the handle's device) through the device one — it must be int32 and
        contiguous, else TypeError."""
        if hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda"):
            if "int32" not in str(ids.dtype) or ids.dim() != 1 or not ids.is_contiguous():
                raise TypeError("set_sources: a tensor of ids must be one-dimensional, int32 and contiguous (got %s)" % ids.dtype)
            if ids.is_cuda:
                import torch
                torch.cuda.current_stream(ids.device).synchronize()      # the ids are written before the handle's stream reads them
                self._ck(lib().srw_set_sources_device(self.h, C.c_void_p(ids.data_ptr()), int(ids.numel())))
                self._src_ids = ids.clone()                              # what _with_sources restores
                return self
            ids = ids.numpy()
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("set_sources: vertex ids must be integers (got %s)" % a.dtype)
        if a.size and (int(a.min()) < -2**31 or int(a.max()) > 2**31 - 1):
            raise ValueError("set_sources: a vertex id is outside int32")
        a = np.array(a.reshape(-1), dtype=np.int32)                      # (a copy: the caller may reuse its array)
        self._ck(lib().srw_set_sources(self.h, _i32(a) if a.size else None, a.size))
        self._src_ids = a
        return self

    def clear_sources(self):
        self._ck(lib().srw_clear_sources(self.h))
        self._src_ids = None
        return self

    def sources_len(self):
        """Length of the list in force, None when there is none (walks start from every vertex)."""
        n = C.c_int64(0)
        self._ck(lib().srw_sources(self.h, C.byref(n)))
        return None if n.value < 0 else n.value

    def _with_sources(self, sources, call):
        """call() with `sources` as the list in force; the state from before (a list, or none) is back afterwards."""
        if sources is None:
            return call()
        before = getattr(self, "_src_ids", None) if self.sources_len() is not None else None    # (a load clears the handle's list)
        self.set_sources(sources)
        try:
            return call()
        finally:
            if before is None:
                self.clear_sources()
            else:
                self.set_sources(before)

    # ---- walk ----
    @staticmethod
    def params(p=1.0, q=1.0, walk_length=80, num_walks=1, first_walk=0, rng="philox", const_r=0.0, seed=42,
               sampler=SAMPLER_REFERENCE, force_general=False, nt_loads=None, occ=0, compact=True, prefix=True, edge_hash=True, binned=True, binned_tune=0, hub_bitmaps=True, device_format=False, edge_tables=True, edge_tables_all=False, legacy_flush=False):
        if sampler == "alias":
            sampler = SAMPLER_ALIAS
        elif sampler == "reference":
            sampler = SAMPLER_REFERENCE
        return WalkParams(np.float32(p), np.float32(q), walk_length, num_walks, first_walk,
                          RNG_CONST if rng == "const" else RNG_PHILOX, np.float32(const_r), seed, sampler,
                          (WALK_FORCE_GENERAL if force_general else 0) | (0 if nt_loads is None else WALK_NT_LOADS if nt_loads else WALK_CACHED_LOADS) | (occ << 8) | (0 if compact else WALK_NO_COMPACT) | (0 if prefix else WALK_NO_PREFIX) | (0 if edge_hash else WALK_NO_EDGE_HASH) | (0 if binned else WALK_NO_BINNED) | (0 if hub_bitmaps else WALK_NO_HUB_BITMAPS) | (WALK_DEVICE_FORMAT if device_format else 0) | (binned_tune << 12) | (0 if edge_tables else WALK_NO_EDGE_TABLES) | (WALK_EDGE_TABLES_ALL if edge_tables_all else 0) | (WALK_LEGACY_FLUSH if legacy_flush else 0))

    def walk(self, fetch=True, sources=None, **kw):
        """Runs srw_walk.  Returns (paths [nWalkers, L+2] int32 (-1 tail), lens, stats dict) or just stats.
        sources=ids: from these vertices only, for this call (set_sources before, the previous state back afterwards)."""
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk(fetch=fetch, **kw))
        P = self.params(**kw)
        st = WalkStats()
        self._ck(lib().srw_walk(self.h, C.byref(P), C.byref(st)))
        if not fetch:
            return st.as_dict()
        paths = np.empty((max(st.n_walkers, 1), P.walk_length + 2), dtype=np.int32)
        lens = np.empty(max(st.n_walkers, 1), dtype=np.int32)
        self._ck(lib().srw_fetch_paths(self.h, _i32(paths), _i32(lens)))
        return paths[:st.n_walkers], lens[:st.n_walkers], st.as_dict()

    # ---- metapath walks: steps restricted to vertex types (srw_vertex_types_set / srw_walk_metapath) ----
    def set_vertex_types(self, types):
        """One type (0 .. 255) per present vertex, indexed like vertices(): a torch.uint8 tensor [nV], contiguous, on the handle's
        device, or a list / numpy array of integers in 0 .. 255, which is uploaded.  None clears.  The types last until the next load.
        A wrong dtype, shape, device or range is a TypeError before the library is called; a wrong length is the library's refusal."""
        if types is None:
            self._ck(lib().srw_vertex_types_set(self.h, None, 0))
            return self
        import torch
        mine = getattr(self, "device", None)
        if hasattr(types, "data_ptr") and hasattr(types, "is_cuda"):
            t = types
            # (shape, contiguity and dtype first, the device last — skipgram's order: each refusal can be met without a GPU)
            if t.dim() != 1:
                raise TypeError("set_vertex_types: types must be one-dimensional [nV] (got %s)" % (tuple(t.shape),))
            if not t.is_contiguous():
                raise TypeError("set_vertex_types: types must be contiguous")
            if str(t.dtype) != "torch.uint8":
                raise TypeError("set_vertex_types: a tensor of types must be torch.uint8 (got %s)" % t.dtype)
            if not t.is_cuda:
                raise TypeError("set_vertex_types: a tensor of types must be in device memory (got %s)" % t.device)
            if mine is not None and t.device.index != mine:
                raise TypeError("set_vertex_types: the tensor must be on the handle's device (cuda:%s), got %s" % (mine, t.device))
        else:
            a = np.asarray(types)
            if a.ndim != 1:
                raise TypeError("set_vertex_types: types must be one-dimensional [nV] (got %s)" % (a.shape,))
            if a.size and a.dtype.kind not in "iu":
                raise TypeError("set_vertex_types: types must be integers (got %s)" % a.dtype)
            if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
                raise TypeError("set_vertex_types: a type is outside the range 0 .. 255")
            t = torch.as_tensor(np.array(a, dtype=np.uint8)).to(torch.device("cuda", mine or 0))
        n = int(t.numel())
        if not n:
            t = torch.zeros(1, dtype=torch.uint8, device=t.device)       # (a pointer that is not NULL: NULL clears)
        torch.cuda.current_stream(t.device).synchronize()                # the types are written before the handle's stream reads them
        self._ck(lib().srw_vertex_types_set(self.h, C.c_void_p(t.data_ptr()), n))
        return self

    def vertex_types_len(self):
        """nV when vertex types are in force, -1 when there are none."""
        n = C.c_int64(0)
        self._ck(lib().srw_vertex_types(self.h, C.byref(n)))
        return n.value

    @staticmethod
    def _metapath_pattern(pattern):
        """walk_metapath's pattern as int32 [m]; TypeError before the library is called."""
        if isinstance(pattern, (str, bytes)) or not hasattr(pattern, "__len__"):
            raise TypeError("walk_metapath: pattern must be a sequence of integers (got %s)" % type(pattern).__name__)
        a = np.asarray(pattern)
        if a.ndim != 1 or not 1 <= a.size <= 64:
            raise TypeError("walk_metapath: pattern must have 1 .. 64 entries (got shape %s)" % (a.shape,))
        if a.dtype.kind not in "iu":
            raise TypeError("walk_metapath: pattern entries must be integers (got %s)" % a.dtype)
        if int(a.min()) < -1 or int(a.max()) > 255:
            raise TypeError("walk_metapath: a pattern entry is outside -1 .. 255 (a type, or -1 for any)")
        return np.array(a, dtype=np.int32)

    def walk_metapath(self, pattern, fetch=True, sources=None, **kw):
        """Runs srw_walk_metapath: the vertex at path position j has the type pattern[j mod m] (-1: any type); StellarGraph's metapath
        [a, p, a] is pattern=[a, p].  Needs set_vertex_types.  Returns what walk returns, and the result replaces the last walk's:
        paths_tensor, skipgram, skipgram_batch, visit_counts, write_paths and w2v_fit_device then act on it.  kw as params (p and q
        must stay 1, the sampler the reference one); sources as in walk.  A source of the wrong type gives the one-entry path."""
        pat = self._metapath_pattern(pattern)
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk_metapath(pat, fetch=fetch, **kw))
        P = self.params(**kw)
        st = WalkStats()
        self._ck(lib().srw_walk_metapath(self.h, C.byref(P), _i32(pat), int(pat.size), C.byref(st)))
        if not fetch:
            return st.as_dict()
        paths = np.empty((max(st.n_walkers, 1), P.walk_length + 2), dtype=np.int32)
        lens = np.empty(max(st.n_walkers, 1), dtype=np.int32)
        self._ck(lib().srw_fetch_paths(self.h, _i32(paths), _i32(lens)))
        return paths[:st.n_walkers], lens[:st.n_walkers], st.as_dict()

    # ---- neighbour sampling: the layered fan-out sample of a mini-batch of seeds (srw_sample_neighbors) ----
    @staticmethod
    def _neighbor_fanouts(fanouts, replace):
        """sample_neighbors' fanouts as int32 [n_layers]; TypeError before the library is called."""
        if isinstance(fanouts, (str, bytes)) or not hasattr(fanouts, "__len__"):
            raise TypeError("sample_neighbors: fanouts must be a sequence of integers (got %s)" % type(fanouts).__name__)
        a = np.asarray(fanouts)
        if a.ndim != 1 or not 1 <= a.size <= NBR_MAX_LAYERS:
            raise TypeError("sample_neighbors: fanouts must have 1 .. %d entries (got shape %s)" % (NBR_MAX_LAYERS, a.shape))
        if a.dtype.kind not in "iu":
            raise TypeError("sample_neighbors: fanouts must be integers (got %s)" % a.dtype)
        if int(a.min()) < 1 or int(a.max()) > NBR_MAX_FANOUT:
            raise TypeError("sample_neighbors: a fanout is outside 1 .. %d" % NBR_MAX_FANOUT)
        if not replace and int(a.max()) > NBR_MAX_DISTINCT_FANOUT:
            raise TypeError("sample_neighbors: a fanout above %d needs replace=True" % NBR_MAX_DISTINCT_FANOUT)
        total = 1
        for f in a.tolist():
            total *= int(f)
        if total >= 2**31:
            raise TypeError("sample_neighbors: the product of the fanouts must stay below 2^31 (got %d)" % total)
        return np.array(a, dtype=np.int32)

    def _seed_tensor(self, seeds, what):
        """the seeds of sample_neighbors / importance_neighbors as a contiguous int32 tensor [B] on the handle's device; TypeError for a
        wrong dtype, rank, contiguity or device before the library is called"""
        mine = getattr(self, "device", None)
        if hasattr(seeds, "data_ptr") and hasattr(seeds, "is_cuda"):
            t = seeds
            # (shape, contiguity and dtype first, the device last — skipgram's order: each refusal can be met without a GPU)
            if t.dim() != 1:
                raise TypeError("%s: seeds must be one-dimensional [B] (got %s)" % (what, tuple(t.shape)))
            if not t.is_contiguous():
                raise TypeError("%s: seeds must be contiguous" % what)
            if str(t.dtype) not in ("torch.int32", "torch.int64"):
                raise TypeError("%s: a tensor of seeds must be torch.int32 or torch.int64 (got %s)" % (what, t.dtype))
            if not t.is_cuda:
                raise TypeError("%s: a tensor of seeds must be in device memory (got %s)" % (what, t.device))
            if mine is not None and t.device.index != mine:
                raise TypeError("%s: seeds must be on the handle's device (cuda:%s), got %s" % (what, mine, t.device))
            import torch
            if str(t.dtype) == "torch.int64":
                if t.numel() and (int(t.min()) < -2**31 or int(t.max()) > 2**31 - 1):
                    raise ValueError("%s: a seed is outside int32" % what)
                t = t.to(torch.int32)
        else:
            a = np.asarray(seeds)
            if a.ndim != 1:
                raise TypeError("%s: seeds must be one-dimensional [B] (got %s)" % (what, a.shape))
            if a.size and a.dtype.kind not in "iu":
                raise TypeError("%s: seeds must be integers (got %s)" % (what, a.dtype))
            if a.size and (int(a.min()) < -2**31 or int(a.max()) > 2**31 - 1):
                raise ValueError("%s: a seed is outside int32" % what)
            import torch
            t = torch.as_tensor(np.array(a, dtype=np.int32)).to(torch.device("cuda", mine or 0))
        return t

    def sample_neighbors(self, seeds, fanouts, seed=1, epoch=0, replace=True, return_unknown=False, no_compact=False):
        """Runs srw_sample_neighbors: the fixed fan-out neighbour sample of a mini-batch (StellarGraph's SampledBreadthFirstWalk, the
        sampler behind PyG's NeighborLoader / DGL's sample_neighbors).  seeds: a one-dimensional contiguous int32 / int64 torch tensor
        [B] on the handle's device (int64 is narrowed after a range check), or a host array-like of integers, which is uploaded.
        Returns a list of len(fanouts) int32 device tensors, layer l of shape [B, F_l] with F_l = fanouts[0] * ... * fanouts[l];
        with return_unknown the number of seeds that are no vertex of the graph is appended.  Layout rule: the parent of
        layers[l][b, j] is layers[l-1][b, parent] with parent = j // f_l, f_l = fanouts[l] (the seeds are the parents of layers[0]) —
        so layers[l].view(B, -1, f_l) groups the children by parent, and a mean aggregation over a feature table X laid out like
        vertices() is  X[e.rows_of(layer.reshape(-1)).long()].view(B, -1, f_l, D).mean(dim=2)  (rows_of gives -1 for the -1 padding:
        mask it).  -1 marks a child of -1, of an id that is no vertex, or of a vertex without neighbours.
        replace=True draws every child by RandomSample.sample over the parent's weighted row (what step 1 of walk does);
        replace=False takes distinct row positions uniformly, ignoring weights (the whole row, then -1, when it has at most f_l
        entries; fanouts up to 64).  The draw is keyed by (seed, epoch, the seed's index b, j, layer), never by the vertex id.
        no_compact: test switch (the 32-byte first-order records).  A wrong dtype, rank, contiguity or device of seeds, fanouts that
        are no integers or outside the limits: TypeError before the library is called."""
        fan = self._neighbor_fanouts(fanouts, replace)
        t = self._seed_tensor(seeds, "sample_neighbors")
        import torch
        B = int(t.numel())
        layers, F = [], 1
        for f in fan.tolist():
            F *= f
            layers.append(torch.empty((B, F), dtype=torch.int32, device=t.device))
        ptrs = (C.c_void_p * len(layers))(*[x.data_ptr() for x in layers])
        P = NeighborParams(int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, int(bool(replace)), NBR_NO_COMPACT if no_compact else 0)
        unknown = C.c_int64(0)
        torch.cuda.current_stream(t.device).synchronize()                # the seeds are written before the handle's stream reads them
        self._ck(lib().srw_sample_neighbors(self.h, C.c_void_p(t.data_ptr()), B, _i32(fan), int(fan.size), C.byref(P), ptrs,
                                            C.byref(unknown)))
        return layers + [unknown.value] if return_unknown else layers

    # ---- importance neighbours: walks with restart, the top-T vertices by visit count (srw_importance_neighbors) ----
    @staticmethod
    def _importance_shape(num_walks, walk_length, top):
        """importance_neighbors' (R, L, T) as ints; TypeError before the library is called."""
        out = []
        for name, v, hi in (("num_walks", num_walks, IMP_MAX_WALKS), ("walk_length", walk_length, IMP_MAX_LENGTH), ("top", top, IMP_MAX_TOP)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError("importance_neighbors: %s must be an integer (got %s)" % (name, type(v).__name__))
            if not 1 <= int(v) <= hi:
                raise TypeError("importance_neighbors: %s is outside 1 .. %d (got %d)" % (name, hi, int(v)))
            out.append(int(v))
        if out[0] * out[1] > IMP_MAX_VISITS:
            raise TypeError("importance_neighbors: num_walks * walk_length must not exceed %d (got %d)" % (IMP_MAX_VISITS, out[0] * out[1]))
        return tuple(out)

    @staticmethod
    def _importance_restart(restart, restart_m=None):
        """restart in [0, 1] -> restart_m = round(restart * 2^24) in 0 .. 2^24 (an integer restart_m overrides it); TypeError otherwise."""
        if restart_m is not None:
            if isinstance(restart_m, (bool, np.bool_)) or not isinstance(restart_m, (int, np.integer)) or not 0 <= int(restart_m) <= 2**24:
                raise TypeError("importance_neighbors: restart_m must be an integer in 0 .. 2^24 (got %r)" % (restart_m,))
            return int(restart_m)
        if isinstance(restart, (bool, np.bool_)) or not isinstance(restart, (int, float, np.integer, np.floating)):
            raise TypeError("importance_neighbors: restart must be a number in [0, 1] (got %s)" % type(restart).__name__)
        if not 0.0 <= float(restart) <= 1.0:                             # (NaN fails both compares)
            raise TypeError("importance_neighbors: restart must be in [0, 1] (got %r)" % (restart,))
        return int(round(float(restart) * 2**24))

    def importance_neighbors(self, seeds, num_walks, walk_length, top, restart=0.5, seed=1, epoch=0, base=0, keep_seed=False,
                             return_total=False, return_unknown=False, no_compact=False, restart_m=None):
        """Runs srw_importance_neighbors: PinSAGE's importance neighbourhood (DGL's PinSAGESampler / RandomWalkNeighborSampler).  Every
        seed runs num_walks first-order random walks of at most walk_length steps; before every step but the first a walk ends with
        probability restart; the top vertices by visit count, ties by id ascending, are the seed's neighbours.  seeds: as in
        sample_neighbors — a one-dimensional contiguous int32 / int64 torch tensor [B] on the handle's device (int64 is narrowed after
        a range check), or a host array-like of integers, which is uploaded.  Returns (ids, counts), int32 device tensors [B, top]
        (padding: id -1, count 0), followed by total [B] (all visits of the seed, before the cut to top) with return_total and by the
        number of seeds that are no vertex with return_unknown.  Visits of the seed itself are dropped unless keep_seed.  The draw is
        keyed by (seed, epoch, base + the seed's index b, walk, step), never by the vertex id: a list split over several calls with
        base = the offset of each part gives what one call gives.
        PinSAGE use: the neighbours of a batch and their edge weights are
            ids, counts, total = e.importance_neighbors(batch, 200, 2, 50, return_total=True)
            weights = counts.float() / total.clamp(min=1)[:, None]          # importance pooling; mask ids == -1
        and X[e.rows_of(ids.reshape(-1)).long()] gathers their features.  PPR reading: with keep_seed, counts / (num_walks summed over
        epochs) estimates sum_{k=1..walk_length} (1 - restart)^(k-1) (P^k)[seed, v], the personalised PageRank mass truncated at
        walk_length steps (up to the factor restart and the k = 0 term).
        restart_m: an integer in 0 .. 2^24 that overrides round(restart * 2^24), for tests.  no_compact: test switch (the 32-byte
        first-order records).  A wrong dtype, rank, contiguity or device of seeds, num_walks / walk_length / top that are no integers or
        outside the limits (1 .. 4096, 1 .. 4096 with a product of at most 4096, 1 .. 64), restart outside [0, 1]: TypeError before
        the library is called."""
        R, L, T = self._importance_shape(num_walks, walk_length, top)
        rm = self._importance_restart(restart, restart_m)
        t = self._seed_tensor(seeds, "importance_neighbors")
        import torch
        B = int(t.numel())
        ids = torch.empty((B, T), dtype=torch.int32, device=t.device)
        counts = torch.empty((B, T), dtype=torch.int32, device=t.device)
        total = torch.empty((B,), dtype=torch.int32, device=t.device) if return_total else None
        P = ImportanceParams(int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, int(base) & 0xFFFFFFFF, R, L, T, rm,
                             (IMP_KEEP_SEED if keep_seed else 0) | (IMP_NO_COMPACT if no_compact else 0))
        unknown = C.c_int64(0)
        torch.cuda.current_stream(t.device).synchronize()                # the seeds are written before the handle's stream reads them
        self._ck(lib().srw_importance_neighbors(self.h, C.c_void_p(t.data_ptr()), B, C.byref(P), C.c_void_p(ids.data_ptr()),
                                                C.c_void_p(counts.data_ptr()), C.c_void_p(total.data_ptr()) if return_total else None,
                                                C.byref(unknown)))
        out = (ids, counts) + ((total,) if return_total else ()) + ((unknown.value,) if return_unknown else ())
        return out

    def walk_to_host(self, pinned=True, sources=None, **kw):
        """srw_walk_to_host: all num_walks iterations streamed into host buffers (kernel i overlaps the copy of i-1).
        Returns (paths, lens, stats); with pinned=True the arrays are copies of pinned staging memory."""
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk_to_host(pinned=pinned, **kw))
        P = self.params(**kw)
        nv = self.sources_len()                 # walkers per iteration: the list in force, else every vertex
        if nv is None:
            nv = self.num_vertices
        n, stride = P.num_walks * nv, P.walk_length + 2
        st = WalkStats()
        if pinned:
            pp, pl = C.c_void_p(), C.c_void_p()
            if lib().srw_host_alloc(max(n * stride * 4, 4), C.byref(pp)) != OK or \
                    lib().srw_host_alloc(max(n * 4, 4), C.byref(pl)) != OK:
                raise SrwError(ERR_NOMEM, "pinned host allocation failed")
            try:
                self._ck(lib().srw_walk_to_host(self.h, C.byref(P), C.cast(pp, C.POINTER(C.c_int32)),
                                                C.cast(pl, C.POINTER(C.c_int32)), C.byref(st)))
                paths = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_int32)), shape=(max(n, 1), stride))[:n].copy()
                lens = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_int32)), shape=(max(n, 1),))[:n].copy()
            finally:
                lib().srw_host_free(pp)
                lib().srw_host_free(pl)
        else:
            paths = np.empty((max(n, 1), stride), dtype=np.int32)
            lens = np.empty(max(n, 1), dtype=np.int32)
            self._ck(lib().srw_walk_to_host(self.h, C.byref(P), _i32(paths), _i32(lens), C.byref(st)))
            paths, lens = paths[:n], lens[:n]
        return paths, lens, st.as_dict()

    def walk_and_save(self, output_dir, n_parts=1, write_crc=False, sources=None, **kw):
        """srw_walk_and_save: Main.doRandomWalk fused and streamed.  Returns (stats, dead_ends_per_iteration)."""
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk_and_save(output_dir, n_parts=n_parts, write_crc=write_crc, **kw))
        P = self.params(**kw)
        st = WalkStats()
        dead = (C.c_int64 * max(P.num_walks, 1))()
        self._ck(lib().srw_walk_and_save(self.h, C.byref(P), os.fsencode(output_dir), n_parts, int(write_crc),
                                         C.byref(st), dead))
        return st.as_dict(), list(dead)[:P.num_walks]

    def device_paths(self):
        dp, dl, n, s = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int32(0)
        self._ck(lib().srw_device_paths(self.h, C.byref(dp), C.byref(dl), C.byref(n), C.byref(s)))
        return dp.value, dl.value, n.value, s.value

    def paths_tensor(self):
        """(paths, lens) of the last walk as torch int32 tensors [n_walkers, stride] and [n_walkers] on the handle's device: VIEWS of the
        result where srw_walk left it in HBM (the pointers of srw_device_paths; no copy).  They are valid until the next walk or load
        on this handle, or its close — clone() what has to outlive that.  Zero walkers give empty tensors."""
        import torch
        dp, dl, n, stride = self.device_paths()
        dev = torch.device("cuda", getattr(self, "device", None) or 0)
        if n == 0:
            return torch.empty((0, stride), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
        return (torch.as_tensor(_DeviceArray(dp, (n, stride), self), device=dev),
                torch.as_tensor(_DeviceArray(dl, (n,), self), device=dev))

    # ---- skip-gram training batches (srw_skipgram_windows) ----
    def skipgram(self, context, num_negatives=0, seed=1, epoch=0, paths=None, lens=None):
        """(pos, neg): every window of `context` consecutive vertices of every path as a torch int32 tensor [W, context], and
        num_negatives vertices per window drawn uniformly from the graph's vertices, [W, num_negatives] (None when num_negatives == 0)
        — both on the handle's device, allocated by torch and owned by the caller (no views of library memory: they survive the
        next walk).  Order: path row major, then window start ascending; a dead-ended row gives the windows it has, none holds a -1.
        Negative k of window (r, j) is keyed by (seed, epoch, r, j, k) alone (include/stellar_rw.h), not filtered against the window.
        paths / lens default to the last walk's result where it lies in HBM; otherwise contiguous int32 tensors [n, stride] / [n] on
        the handle's device in the layout of paths_tensor() — anything else is a TypeError before the library is called.
        Sizing: one count-only call (a reduction over lens) gives W, the tensors are allocated exactly, one fill call follows; the
        alternative — allocating the bound n * (stride - context + 1) and returning [:W] — would pin the bound's memory behind the
        view, which on a directed graph is many times W."""
        import torch
        if (paths is None) != (lens is None):
            raise TypeError("skipgram: paths and lens go together")
        pp = pl = None
        n, stride = 0, 1
        if paths is not None:
            is_t = lambda x: hasattr(x, "data_ptr") and hasattr(x, "is_cuda")      # noqa: E731
            if not (is_t(paths) and is_t(lens)):
                raise TypeError("skipgram: paths and lens must be torch tensors")
            # (shape, contiguity and dtype first, the device last — _load_coo_tensors' order: each refusal can be met without a GPU)
            if paths.dim() != 2 or lens.dim() != 1 or paths.shape[0] != lens.shape[0]:
                raise TypeError("skipgram: paths must be [n, stride] and lens [n] (got %s, %s)" % (tuple(paths.shape), tuple(lens.shape)))
            if not (paths.is_contiguous() and lens.is_contiguous()):
                raise TypeError("skipgram: paths and lens must be contiguous")
            if str(paths.dtype) != "torch.int32" or str(lens.dtype) != "torch.int32":
                raise TypeError("skipgram: paths and lens must be torch.int32 (got %s, %s)" % (paths.dtype, lens.dtype))
            if not (paths.is_cuda and lens.is_cuda):
                raise TypeError("skipgram: paths and lens must be in device memory (got %s, %s)" % (paths.device, lens.device))
            mine = getattr(self, "device", None)
            if lens.device != paths.device or (mine is not None and paths.device.index != mine):
                raise TypeError("skipgram: the tensors must be on the handle's device (cuda:%s), got %s, %s" % (mine, paths.device, lens.device))
            n, stride = int(paths.shape[0]), int(paths.shape[1])
            dev = paths.device
            if n == 0 or stride == 0:
                return (torch.empty((0, context), dtype=torch.int32, device=dev),
                        torch.empty((0, num_negatives), dtype=torch.int32, device=dev) if num_negatives else None)
            pp, pl = C.c_void_p(paths.data_ptr()), C.c_void_p(lens.data_ptr())
            torch.cuda.current_stream(dev).synchronize()                 # the paths are written before the handle's stream reads them
        else:
            dev = torch.device("cuda", getattr(self, "device", None) or 0)
        sp = SkipgramParams(int(context), int(num_negatives), int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF)
        W = C.c_int64(0)
        self._ck(lib().srw_skipgram_windows(self.h, pp, pl, n, stride, C.byref(sp), None, None, 0, C.byref(W)))
        pos = torch.empty((W.value, sp.context), dtype=torch.int32, device=dev)
        neg = torch.empty((W.value, sp.num_negatives), dtype=torch.int32, device=dev) if sp.num_negatives else None
        if W.value:
            torch.cuda.current_stream(dev).synchronize()                 # whatever torch last did with this memory is over
            self._ck(lib().srw_skipgram_windows(self.h, pp, pl, n, stride, C.byref(sp), C.c_void_p(pos.data_ptr()),
                                                C.c_void_p(neg.data_ptr()) if neg is not None else None, W.value, C.byref(W)))
        return pos, neg                                                  # (the library call has completed: nothing to wait for)

    def walk_skipgram(self, sources, context, num_negatives=0, sg_seed=1, epoch=0, **walk_kw):
        """The per-step call of a training loop: walk(fetch=False, sources=sources, **walk_kw), then skipgram(context, num_negatives,
        seed=sg_seed, epoch=epoch) over the result where it lies.  sources: a sequence or an int32 tensor, as set_sources takes."""
        self.walk(fetch=False, sources=sources, **walk_kw)
        return self.skipgram(context, num_negatives, seed=sg_seed, epoch=epoch)

    # ---- negatives by vertex weight, kept out of their own window (srw_skipgram_batch) ----
    def _paths_args(self, what, paths, lens):
        """skipgram's checks of paths= / lens= -> (pointer to paths, pointer to lens, n, stride, device); the pointers are None for the
        last walk's result.  TypeError before the library is called."""
        import torch
        if (paths is None) != (lens is None):
            raise TypeError("%s: paths and lens go together" % what)
        if paths is None:
            return None, None, 0, 1, torch.device("cuda", getattr(self, "device", None) or 0)
        is_t = lambda x: hasattr(x, "data_ptr") and hasattr(x, "is_cuda")      # noqa: E731
        if not (is_t(paths) and is_t(lens)):
            raise TypeError("%s: paths and lens must be torch tensors" % what)
        if paths.dim() != 2 or lens.dim() != 1 or paths.shape[0] != lens.shape[0]:
            raise TypeError("%s: paths must be [n, stride] and lens [n] (got %s, %s)" % (what, tuple(paths.shape), tuple(lens.shape)))
        if not (paths.is_contiguous() and lens.is_contiguous()):
            raise TypeError("%s: paths and lens must be contiguous" % what)
        if str(paths.dtype) != "torch.int32" or str(lens.dtype) != "torch.int32":
            raise TypeError("%s: paths and lens must be torch.int32 (got %s, %s)" % (what, paths.dtype, lens.dtype))
        if not (paths.is_cuda and lens.is_cuda):
            raise TypeError("%s: paths and lens must be in device memory (got %s, %s)" % (what, paths.device, lens.device))
        mine = getattr(self, "device", None)
        if lens.device != paths.device or (mine is not None and paths.device.index != mine):
            raise TypeError("%s: the tensors must be on the handle's device (cuda:%s), got %s, %s" % (what, mine, paths.device, lens.device))
        return C.c_void_p(paths.data_ptr()), C.c_void_p(lens.data_ptr()), int(paths.shape[0]), int(paths.shape[1]), paths.device

    def degrees_tensor(self):
        """int64 [nV] on the handle's device: the row length of every present vertex, in the order of vertices() (what neighbors(v)
        reports; 0 for a destination-only vertex of a directed graph)."""
        import torch
        dev = torch.device("cuda", getattr(self, "device", None) or 0)
        out = torch.empty((self.num_vertices,), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._ck(lib().srw_graph_degrees_device(self.h, C.c_void_p(out.data_ptr())))
        return out

    def visit_counts(self, paths=None, lens=None):
        """int64 [nV] on the handle's device: how often every present vertex, in the order of vertices(), occurs in the paths — the last
        walk's result, or tensors as skipgram takes them (the same checks, TypeError before the library is called).  The corpus's
        unigram counts.  An id in a caller's tensor that is no vertex of the graph is counted in self.last_unknown_ids only."""
        import torch
        pp, pl, n, stride, dev = self._paths_args("visit_counts", paths, lens)
        out = torch.empty((self.num_vertices,), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if paths is not None and (n == 0 or stride == 0):                # (an empty tensor's pointer is arbitrary, NULL included)
            self.last_unknown_ids = 0
            return out.zero_()
        unknown = C.c_int64(0)
        self._ck(lib().srw_path_vertex_counts(self.h, pp, pl, n, stride, C.c_void_p(out.data_ptr()), C.byref(unknown)))
        self.last_unknown_ids = unknown.value
        return out

    def set_negative_weights(self, weights):
        """The weight table of skipgram_batch's negatives: a torch tensor [nV] on the handle's device, indexed like vertices().  Returns
        the int64 tensor of quantised weights now in force; None clears the table (uniform draws again) and returns None.  An integer
        dtype is taken exactly (a value below 0 or at or above 2^32: ValueError).  A floating dtype is quantised in float64 as
        q = floor(w / max(w) * (2^32 - 1)), then q = max(q, 1) wherever w > 0 (negative or non-finite values: ValueError).  A vertex of
        weight 0 is never drawn; all zero is an error of the library.  The table lasts until the next load.  Recipes:
            e.set_negative_weights(e.visit_counts().double().pow(0.75))      # word2vec's unigram^0.75 table
            e.set_negative_weights(e.degrees_tensor().double().pow(0.75))    # the degree variant"""
        if weights is None:
            self._ck(lib().srw_negative_weights_set(self.h, None, 0))
            return None
        import torch
        if not (hasattr(weights, "data_ptr") and hasattr(weights, "is_cuda")):
            raise TypeError("set_negative_weights: weights must be a torch tensor")
        if weights.dim() != 1:
            raise TypeError("set_negative_weights: weights must be one-dimensional (got %s)" % (tuple(weights.shape),))
        if weights.dtype == torch.bool or weights.is_complex():
            raise TypeError("set_negative_weights: weights must be an integer or floating tensor (got %s)" % weights.dtype)
        # (the values before the device, skipgram's order: each refusal can be met without a GPU)
        if weights.is_floating_point():
            w = weights.double()
            if w.numel() and (not bool(torch.isfinite(w).all()) or bool((w < 0).any())):
                raise ValueError("set_negative_weights: a weight is negative or not finite")
            q = torch.floor(w / w.max() * 4294967295.0) if w.numel() and float(w.max()) > 0 else torch.zeros_like(w)
            q = torch.where(w > 0, torch.clamp(q, min=1.0), q).to(torch.int64)
        else:
            q = weights.to(torch.int64)
            if q.numel() and (int(q.min()) < 0 or int(q.max()) >= 2**32):
                raise ValueError("set_negative_weights: an integer weight is below 0 or at or above 2^32")
        if not weights.is_cuda:
            raise TypeError("set_negative_weights: weights must be in device memory (got %s)" % weights.device)
        mine = getattr(self, "device", None)
        if mine is not None and weights.device.index != mine:
            raise TypeError("set_negative_weights: the tensor must be on the handle's device (cuda:%s), got %s" % (mine, weights.device))
        w32 = torch.where(q >= 2**31, q - 2**32, q).to(torch.int32)      # uint32 words in an int32 tensor
        if not w32.numel():
            w32 = torch.zeros(1, dtype=torch.int32, device=weights.device)   # (a pointer that is not NULL: n = 0 is refused as a wrong length)
        torch.cuda.current_stream(weights.device).synchronize()          # the weights are written before the handle's stream reads them
        self._ck(lib().srw_negative_weights_set(self.h, C.c_void_p(w32.data_ptr()), int(q.numel())))
        return q

    def skipgram_batch(self, context, num_negatives=0, seed=1, epoch=0, paths=None, lens=None, exclude_window=False, max_draws=8):
        """skipgram with the negatives drawn by the weight table in force (set_negative_weights; uniform without one) and, with
        exclude_window, none that repeats a vertex of its own window: a draw that does is redrawn, up to max_draws attempts (1 .. 16);
        the last attempt's vertex stands if all are rejected.  (pos, neg) as skipgram returns them, with its allocation and
        synchronisation rules; negative k of window (r, j) is keyed by (seed, epoch, r, j, k, attempt) alone (include/stellar_rw.h).
        With no table and exclude_window=False the result is skipgram's, bit for bit."""
        import torch
        pp, pl, n, stride, dev = self._paths_args("skipgram_batch", paths, lens)
        if paths is not None:
            if n == 0 or stride == 0:
                return (torch.empty((0, context), dtype=torch.int32, device=dev),
                        torch.empty((0, num_negatives), dtype=torch.int32, device=dev) if num_negatives else None)
            torch.cuda.current_stream(dev).synchronize()                 # the paths are written before the handle's stream reads them
        bp = SkipgramBatchParams(int(context), int(num_negatives), int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
                                 1 if exclude_window else 0, int(max_draws))
        W = C.c_int64(0)
        self._ck(lib().srw_skipgram_batch(self.h, pp, pl, n, stride, C.byref(bp), None, None, 0, C.byref(W)))
        pos = torch.empty((W.value, bp.context), dtype=torch.int32, device=dev)
        neg = torch.empty((W.value, bp.num_negatives), dtype=torch.int32, device=dev) if bp.num_negatives else None
        if W.value:
            torch.cuda.current_stream(dev).synchronize()                 # whatever torch last did with this memory is over
            self._ck(lib().srw_skipgram_batch(self.h, pp, pl, n, stride, C.byref(bp), C.c_void_p(pos.data_ptr()),
                                              C.c_void_p(neg.data_ptr()) if neg is not None else None, W.value, C.byref(W)))
        return pos, neg

    def walk_skipgram_batch(self, sources, context, num_negatives=0, sg_seed=1, epoch=0, exclude_window=False, max_draws=8, **walk_kw):
        """walk(fetch=False, sources=sources, **walk_kw), then skipgram_batch(context, num_negatives, seed=sg_seed, epoch=epoch,
        exclude_window=exclude_window, max_draws=max_draws) over the result where it lies — walk_skipgram with the weighted draw."""
        self.walk(fetch=False, sources=sources, **walk_kw)
        return self.skipgram_batch(context, num_negatives, seed=sg_seed, epoch=epoch, exclude_window=exclude_window, max_draws=max_draws)

    # ---- the negative-sampling training step over those batches (srw_sgns_step) ----
    def _sgns_args(self, what, pos, neg, emb_in, emb_out, into):
        """The tensor checks of sgns_step: TypeError before the library is called -> (W, C, K, nV, D, device)."""
        is_t = lambda x: hasattr(x, "data_ptr") and hasattr(x, "is_cuda")      # noqa: E731
        ids = [("pos", pos)] + ([("neg", neg)] if neg is not None else [])
        tabs = [("emb_in", emb_in), ("emb_out", emb_out)]
        if into is not None:
            if not (isinstance(into, (tuple, list)) and len(into) == 2):
                raise TypeError("%s: into must be a pair (new_in, new_out)" % what)
            tabs += [("into[0]", into[0]), ("into[1]", into[1])]
        for name, t in ids + tabs:
            if not is_t(t):
                raise TypeError("%s: %s must be a torch tensor" % (what, name))
        # (shape, contiguity and dtype first, the device last — skipgram's order: each refusal can be met without a GPU)
        if pos.dim() != 2 or (neg is not None and (neg.dim() != 2 or neg.shape[0] != pos.shape[0])):
            raise TypeError("%s: pos must be [W, C] and neg [W, K] (got %s, %s)"
                            % (what, tuple(pos.shape), None if neg is None else tuple(neg.shape)))
        if emb_in.dim() != 2 or any(tuple(t.shape) != tuple(emb_in.shape) for _, t in tabs):
            raise TypeError("%s: the tables must all be [nV, D] (got %s)" % (what, ", ".join(str(tuple(t.shape)) for _, t in tabs)))
        for name, t in ids + tabs:
            if not t.is_contiguous():
                raise TypeError("%s: %s must be contiguous" % (what, name))
        for name, t in ids:
            if str(t.dtype) != "torch.int32":
                raise TypeError("%s: %s must be torch.int32 (got %s)" % (what, name, t.dtype))
        for name, t in tabs:
            if str(t.dtype) != "torch.float32":
                raise TypeError("%s: %s must be torch.float32 (got %s)" % (what, name, t.dtype))
        mine = getattr(self, "device", None)
        for name, t in ids + tabs:
            if not t.is_cuda:
                raise TypeError("%s: %s must be in device memory (got %s)" % (what, name, t.device))
            if t.device != pos.device or (mine is not None and t.device.index != mine):
                raise TypeError("%s: the tensors must be on the handle's device (cuda:%s), got %s for %s" % (what, mine, t.device, name))
        return (int(pos.shape[0]), int(pos.shape[1]), 0 if neg is None else int(neg.shape[1]), int(emb_in.shape[0]),
                int(emb_in.shape[1]), pos.device)

    def sgns_step(self, pos, neg, emb_in, emb_out, lr, center=0, into=None, loss=False):
        """One skip-gram negative-sampling step over (pos, neg) as skipgram / skipgram_batch return them, on the caller's tables
        emb_in / emb_out: float32 [nV, D] on the handle's device, rows in the order of vertices(), D a multiple of 64 up to 512.  For
        every window: centre = pos[w, center], the other entries of pos[w] are targets with label 1, neg[w] (None: K = 0) targets with
        label 0; f = <emb_in[centre], emb_out[target]>, g = label - sigmoid(f); emb_out[target] += lr g emb_in[centre] and
        emb_in[centre] += lr sum g emb_out[target], every read from the values before the call (include/stellar_rw.h; no clamp at
        +-6, no sigmoid table).  into=None: in place (Hogwild: where rows repeat in the call a read may see another window's add;
        no add is lost).  into=(new_in, new_out): the exact step — every add goes into these tensors (clones of the tables, or
        zeros), the tables themselves are only read.  emb_in may be emb_out (one table for both roles); then new_in must be new_out.
        A window that holds an id which is no vertex of the graph is skipped whole.  Returns (loss, n_skipped): loss is a float32
        tensor [W] of the windows' losses at the old values when loss=True, else None.  Tensor checks raise TypeError before the
        library is called; the synchronisation rule is skipgram_batch's (torch's stream is waited for, the call is complete on
        return)."""
        import torch
        W, C_, K, nV, D, dev = self._sgns_args("sgns_step", pos, neg, emb_in, emb_out, into)
        out_loss = torch.empty((W,), dtype=torch.float32, device=dev) if loss else None
        sp = SgnsParams(C_, K, D, int(center), float(lr), 0)
        skipped = C.c_int64(0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
        torch.cuda.current_stream(dev).synchronize()                     # the tensors are written before the handle's stream reads them
        self._ck(lib().srw_sgns_step(self.h, ptr(pos), ptr(neg), W, C.byref(sp), ptr(emb_in), ptr(emb_out),
                                     ptr(into[0]) if into is not None else None, ptr(into[1]) if into is not None else None,
                                     nV, ptr(out_loss), C.byref(skipped)))
        return out_loss, skipped.value

    def sgns_grad(self, pos, neg, emb_in, emb_out, center=0):
        """(grad_in, grad_out, loss): dLoss/d emb_in and dLoss/d emb_out, Loss = loss.sum(), loss [W] the windows' negative-sampling
        losses — sgns_step's exact form into zeroed tables with lr = -1: what the backward of a torch.autograd.Function returns.
        With emb_in is emb_out (one table for both roles) grad_in is grad_out: the one table's gradient."""
        import torch
        self._sgns_args("sgns_grad", pos, neg, emb_in, emb_out, None)
        grad_in = torch.zeros_like(emb_in)
        grad_out = grad_in if emb_out.data_ptr() == emb_in.data_ptr() else torch.zeros_like(emb_out)
        loss, _ = self.sgns_step(pos, neg, emb_in, emb_out, -1.0, center=center, into=(grad_in, grad_out), loss=True)
        return grad_in, grad_out, loss

    def train_sgns(self, dim, context, num_negatives, epochs, batch_sources, lr=0.025, seed=1, **walk_kw):
        """node2vec with negative sampling, everything on the device: per epoch the vertices are shuffled (a torch generator seeded
        with `seed`), per batch of batch_sources start vertices one walk_skipgram_batch (epoch = the step number, sg_seed = seed; the
        negatives follow the weight table in force) and one sgns_step in place (center 0), the learning rate decaying linearly from lr
        to 1e-4 lr over all steps.  emb_in starts uniform in (-0.5, 0.5) / dim, emb_out at zero (word2vec's start).  walk_kw goes to
        walk(); epoch k walks iterations first_walk + k * num_walks onwards, so every epoch sees fresh walks from the same seed.
        Returns (emb_in, emb_out, mean loss per window of every epoch); rows in the order of vertices()."""
        import torch
        dev = torch.device("cuda", getattr(self, "device", None) or 0)
        V = torch.as_tensor(self.vertices(), dtype=torch.int32)
        nV = int(V.numel())
        gen = torch.Generator().manual_seed(int(seed))
        emb_in = ((torch.rand((nV, dim), generator=gen, dtype=torch.float32) - 0.5) / dim).to(dev)
        emb_out = torch.zeros((nV, dim), dtype=torch.float32, device=dev)
        per_epoch = (nV + batch_sources - 1) // batch_sources if nV else 0
        total, step, means = max(per_epoch * epochs, 1), 0, []
        first, per_call = int(walk_kw.pop("first_walk", 0)), int(walk_kw.get("num_walks", 1))
        for k in range(epochs):
            order = V[torch.randperm(nV, generator=gen)].to(dev)
            loss_sum, n_win = 0.0, 0
            for b in range(per_epoch):
                pos, neg = self.walk_skipgram_batch(order[b * batch_sources:(b + 1) * batch_sources].contiguous(), context, num_negatives,
                                                    sg_seed=seed, epoch=step, first_walk=first + k * per_call, **walk_kw)
                rate = max(lr * (1.0 - step / total), lr * 1e-4)
                step += 1
                if pos.shape[0] == 0:
                    continue
                loss, _ = self.sgns_step(pos, neg, emb_in, emb_out, rate, loss=True)
                loss_sum += float(loss.double().sum())
                n_win += int(pos.shape[0])
            means.append(loss_sum / max(n_win, 1))
        return emb_in, emb_out, means

    # ---- asking a table of vectors: the k nearest rows (srw_topk_rows, srw_vertex_rows) ----
    def _topk_args(self, what, table, rows, vectors):
        """The tensor checks of topk_rows, in _sgns_args' order: TypeError before the library is called -> (Q, n, D, device)."""
        is_t = lambda x: hasattr(x, "data_ptr") and hasattr(x, "is_cuda")      # noqa: E731
        if rows is None and vectors is None:
            raise TypeError("%s: at least one of rows and vectors is required" % what)
        ids = [("rows", rows)] if rows is not None else []
        tabs = [("table", table)] + ([("vectors", vectors)] if vectors is not None else [])
        for name, t in ids + tabs:
            if not is_t(t):
                raise TypeError("%s: %s must be a torch tensor" % (what, name))
        # (shape, contiguity and dtype first, the device last — skipgram's order: each refusal can be met without a GPU)
        if table.dim() != 2:
            raise TypeError("%s: table must be [n, D] (got %s)" % (what, tuple(table.shape)))
        if vectors is not None and (vectors.dim() != 2 or vectors.shape[1] != table.shape[1]):
            raise TypeError("%s: vectors must be [Q, D] with the table's D (got %s for a table %s)"
                            % (what, tuple(vectors.shape), tuple(table.shape)))
        if rows is not None and (rows.dim() != 1 or (vectors is not None and rows.shape[0] != vectors.shape[0])):
            raise TypeError("%s: rows must be [Q] (got %s%s)"
                            % (what, tuple(rows.shape), "" if vectors is None else " for vectors %s" % (tuple(vectors.shape),)))
        for name, t in ids + tabs:
            if not t.is_contiguous():
                raise TypeError("%s: %s must be contiguous" % (what, name))
        for name, t in ids:
            if str(t.dtype) != "torch.int32":
                raise TypeError("%s: %s must be torch.int32 (got %s)" % (what, name, t.dtype))
        for name, t in tabs:
            if str(t.dtype) != "torch.float32":
                raise TypeError("%s: %s must be torch.float32 (got %s)" % (what, name, t.dtype))
        mine = getattr(self, "device", None)
        for name, t in ids + tabs:
            if not t.is_cuda:
                raise TypeError("%s: %s must be in device memory (got %s)" % (what, name, t.device))
            if t.device != (ids + tabs)[0][1].device or (mine is not None and t.device.index != mine):
                raise TypeError("%s: the tensors must be on the handle's device (cuda:%s), got %s for %s" % (what, mine, t.device, name))
        Q = int(rows.shape[0]) if rows is not None else int(vectors.shape[0])
        return Q, int(table.shape[0]), int(table.shape[1]), table.device

    def topk_rows(self, table, k, rows=None, vectors=None, metric="cosine"):
        """The k nearest rows of table (float32 [n, D] on the handle's device, D up to 1024, k up to 64) for every query, by
        metric="cosine" or "dot", without forming the Q x n scores.  rows (int32 [Q]): query i is table[rows[i]], and that row is left
        out of its own result; vectors (float32 [Q, D]): query i is vectors[i]; both: the vector is the query, rows[i] is left out
        (-1: none).  A rows[i] that is no row of the table skips the query.  Returns (rows int32 [Q, k], scores float32 [Q, k],
        n_skipped): best first by (score descending, row ascending); a result with fewer than k eligible rows, and every skipped
        query's, ends in padding (row -1, score -inf).  Arithmetic and order: include/stellar_rw.h.  Tensor checks raise TypeError
        before the library is called; the synchronisation rule is sgns_step's (torch's stream is waited for, the call is complete on
        return)."""
        import torch
        Q, n, D, dev = self._topk_args("topk_rows", table, rows, vectors)
        if metric not in TOPK_METRICS:
            raise ValueError("topk_rows: metric must be 'cosine' or 'dot' (got %r)" % (metric,))
        tp = TopkParams(D, int(k), TOPK_METRICS[metric], 0)
        out_rows = torch.empty((Q, max(tp.k, 0)), dtype=torch.int32, device=dev)
        out_scores = torch.empty((Q, max(tp.k, 0)), dtype=torch.float32, device=dev)
        skipped = C.c_int64(0)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
        torch.cuda.current_stream(dev).synchronize()                     # the tensors are written before the handle's stream reads them
        self._ck(lib().srw_topk_rows(self.h, ptr(table), n, ptr(vectors), ptr(rows), Q, C.byref(tp), ptr(out_rows), ptr(out_scores),
                                     C.byref(skipped)))
        return out_rows, out_scores, skipped.value

    def rows_of(self, ids, return_unknown=False):
        """The rows of vertex ids in a table laid out like vertices(): an int32 tensor on the handle's device, -1 for an id that is no
        vertex of the graph.  ids: an int32 tensor [n] on the handle's device, or a list / numpy array of ids, which is uploaded.
        return_unknown=True: (rows, the number of unknown ids)."""
        import torch
        if not (hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda")):
            dev = torch.device("cuda", getattr(self, "device", None) or 0)
            ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        if ids.dim() != 1 or not ids.is_contiguous() or str(ids.dtype) != "torch.int32":
            raise TypeError("rows_of: ids must be a contiguous one-dimensional torch.int32 tensor (got %s, %s)" % (tuple(ids.shape), ids.dtype))
        mine = getattr(self, "device", None)
        if not ids.is_cuda or (mine is not None and ids.device.index != mine):
            raise TypeError("rows_of: ids must be on the handle's device (cuda:%s), got %s" % (mine, ids.device))
        out = torch.empty_like(ids)
        unknown = C.c_int64(0)
        torch.cuda.current_stream(ids.device).synchronize()              # the ids are written before the handle's stream reads them
        self._ck(lib().srw_vertex_rows(self.h, C.c_void_p(ids.data_ptr()), int(ids.numel()), C.c_void_p(out.data_ptr()), C.byref(unknown)))
        return (out, unknown.value) if return_unknown else out

    def most_similar(self, emb, ids, k=10, metric="cosine"):
        """findSynonyms for a table in the order of vertices() (train_sgns' emb_in): for every vertex id in ids its k nearest other
        vertices -> (neighbour_ids int32 [Q, k], scores float32 [Q, k]), best first.  It is rows_of(ids), topk_rows(emb, k, rows=...)
        and a device gather through vertices(); padding stays -1 / -inf, and an id that is no vertex gives a row of padding.
        w2v_fit / w2v_fit_device return (vocab_ids, vectors) in VOCABULARY order instead; there the row of a word is its index in
        vocab_ids:  t = torch.as_tensor(vectors).cuda(); r, s, _ = e.topk_rows(t, k, rows=torch.tensor([row_of_word], dtype=torch.int32,
        device="cuda")); vocab_ids[r.cpu()] are the neighbours."""
        import torch
        rows = self.rows_of(ids)
        r, scores, _ = self.topk_rows(emb, k, rows=rows, metric=metric)
        V = torch.as_tensor(self.vertices(), dtype=torch.int32).to(r.device)
        if V.numel() == 0:
            return torch.full_like(r, -1), scores
        return torch.where(r >= 0, V[r.clamp(min=0).long()], torch.full_like(r, -1)), scores

    def write_paths(self, output_dir, n_parts=1, write_crc=False):
        self._ck(lib().srw_write_paths(self.h, os.fsencode(output_dir), n_parts, int(write_crc)))

    # ---- the embedding stage (--cmd node2vec / embedding; include/stellar_rw.h: parity unpinned) ----
    def w2v_fit(self, paths, lens, dim=128, window=10, iterations=10, lr=0.025, seed=1, threads=0):
        """Skip-gram + hierarchical softmax over host paths [n, stride] on the GPU: (vocab ids by descending count, vectors [vocab, dim])."""
        paths = np.ascontiguousarray(paths, dtype=np.int32); lens = np.ascontiguousarray(lens, dtype=np.int32)
        P = W2vParams(dim, window, iterations, lr, seed, threads)
        ids, vec, nv = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int64(0)
        n, stride = (paths.shape[0], paths.shape[1]) if paths.ndim == 2 else (0, 1)
        self._ck(lib().srw_w2v_fit(self.h, _i32(paths), _i32(lens), n, stride, C.byref(P), C.byref(ids), C.byref(vec), C.byref(nv)))
        k = nv.value
        out_ids = np.ctypeslib.as_array(ids, shape=(max(k, 1),))[:k].copy()
        out_vec = np.ctypeslib.as_array(vec, shape=(max(k * dim, 1),))[:k * dim].copy().reshape(k, dim)
        lib().srw_free(ids); lib().srw_free(vec)
        return out_ids, out_vec

    def w2v_fit_device(self, dim=128, window=10, iterations=10, lr=0.025, seed=1, threads=0):
        """The same over the LAST WALK's paths where they are — in HBM (srw_w2v_fit_device with NULL pointers): no PCIe round trip."""
        P = W2vParams(dim, window, iterations, lr, seed, threads)
        ids, vec, nv = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int64(0)
        self._ck(lib().srw_w2v_fit_device(self.h, None, None, 0, 1, C.byref(P), C.byref(ids), C.byref(vec), C.byref(nv)))
        k = nv.value
        out_ids = np.ctypeslib.as_array(ids, shape=(max(k, 1),))[:k].copy()
        out_vec = np.ctypeslib.as_array(vec, shape=(max(k * dim, 1),))[:k * dim].copy().reshape(k, dim)
        lib().srw_free(ids); lib().srw_free(vec)
        return out_ids, out_vec

    # ---- measurement hooks (bench.py's roofline object) ----
    def probe_request_rate(self, table_bytes=0):
        """(dependent random 16-byte reads per second on this GPU, GiB of table used) — csrc/probe.hip."""
        r, g = C.c_double(0.0), C.c_double(0.0)
        self._ck(lib().srw_probe_request_rate(self.h, int(table_bytes), C.byref(r), C.byref(g)))
        return r.value, g.value

    def result_scan_sums(self):
        """(sum of deg(curr) over the steps, sum of deg(prev) over the second-order steps, steps) of the last srw_walk."""
        out = (C.c_int64 * 3)()
        self._ck(lib().srw_result_scan_sums(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    # ---- unit hooks: RandomSample on the GPU ----
    def sample(self, w, r):
        w = np.ascontiguousarray(w, dtype=np.float32)
        k = C.c_int64(0)
        self._ck(lib().srw_sample(self.h, _f32(w), len(w), C.c_float(r), C.byref(k)))
        return k.value

    def second_order_weights(self, p, q, prev_id, prev_ids, curr_ids, curr_w):
        prev_ids = np.ascontiguousarray(prev_ids, dtype=np.int32)
        curr_ids = np.ascontiguousarray(curr_ids, dtype=np.int32)
        curr_w = np.ascontiguousarray(curr_w, dtype=np.float32)
        out = np.empty_like(curr_w)
        self._ck(lib().srw_second_order_weights(self.h, C.c_float(p), C.c_float(q), prev_id, _i32(prev_ids),
                                                len(prev_ids), _i32(curr_ids), _f32(curr_w), len(curr_ids), _f32(out)))
        return out

    def second_order_sample(self, p, q, prev_id, prev_ids, curr_ids, curr_w, r):
        prev_ids = np.ascontiguousarray(prev_ids, dtype=np.int32)
        curr_ids = np.ascontiguousarray(curr_ids, dtype=np.int32)
        curr_w = np.ascontiguousarray(curr_w, dtype=np.float32)
        k = C.c_int64(0)
        self._ck(lib().srw_second_order_sample(self.h, C.c_float(p), C.c_float(q), prev_id, _i32(prev_ids),
                                               len(prev_ids), _i32(curr_ids), _f32(curr_w), len(curr_ids),
                                               C.c_float(r), C.byref(k)))
        return k.value

    def rng_uniform(self, seed, it, src, step):
        it, src, step = (np.ascontiguousarray(x, dtype=np.uint32) for x in (it, src, step))
        out = np.empty(len(it), dtype=np.float32)
        u32p = C.POINTER(C.c_uint32)
        self._ck(lib().srw_rng_uniform(self.h, seed, it.ctypes.data_as(u32p), src.ctypes.data_as(u32p),
                                       step.ctypes.data_as(u32p), len(it), _f32(out)))
        return out

    def cfo_pick(self, vertex, m):
        """The compact-record pick (csrc/sampling.h:cfo_pick) on the row of `vertex` for the 24-bit lattice draws m (p = m * 2^-24):
        (positions inside the row, 16-byte records each pick loaded).  Builds the compact first-order table if need be."""
        m = np.ascontiguousarray(m, dtype=np.uint32)
        pos = np.empty(len(m), dtype=np.int32); reads = np.empty(len(m), dtype=np.int32)
        self._ck(lib().srw_cfo_pick(self.h, int(vertex), m.ctypes.data_as(C.POINTER(C.c_uint32)), len(m), _i32(pos), _i32(reads)))
        return pos, reads


def w2v_huffman(counts):
    """srw_w2v_huffman (host only): [(code bits, syn1 rows)] per word of a vocabulary given by its counts in descending order."""
    cn = np.ascontiguousarray(counts, dtype=np.int64)
    V = len(cn)
    cl = np.zeros(max(V, 1), np.int32); codes = np.zeros((max(V, 1), 40), np.uint8); points = np.zeros((max(V, 1), 40), np.int32)
    rc = lib().srw_w2v_huffman(cn.ctypes.data_as(C.POINTER(C.c_int64)), V, _i32(cl), codes.ctypes.data_as(C.POINTER(C.c_uint8)), _i32(points))
    if rc != OK:
        raise SrwError(rc, lib().srw_last_error(None).decode())
    return [(codes[a, :cl[a]].tolist(), points[a, :cl[a]].tolist()) for a in range(V)]


class Cluster:
    """srw_cluster_*: the vertex-sharded walk inside one process over several devices (peer stores over xGMI, no
    collective).  `devices` may repeat an ordinal: several shards on one GPU (how single-GPU boxes test the protocol)."""

    def __init__(self, devices, owner_from_partitions=False, membership=True, hash_partitioner=False):
        """membership=False (SRW_CFG_NO_MEMBERSHIP): the shards skip the replicated neighbor-id structure; q == 1 walks only."""
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self.h = C.c_void_p()
        rc = lib().srw_cluster_create(_i32(devs), len(devs), (CFG_OWNER_FROM_PARTITIONS if owner_from_partitions else 0) |
                                      (0 if membership else CFG_NO_MEMBERSHIP) | (CFG_OWNER_HASH_PARTITIONER if hash_partitioner else 0), C.byref(self.h))
        if rc != OK:
            raise SrwError(rc, lib().srw_last_error(None).decode())
        self.world = len(devs)

    def close(self):
        if self.h:
            lib().srw_cluster_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != OK:
            raise SrwError(rc, lib().srw_cluster_last_error(self.h).decode())

    def plan_walks(self, num_walks):
        """srw_plan_walks on every shard: the job's --numWalks."""
        for r in range(self.world):
            rc = lib().srw_plan_walks(C.c_void_p(lib().srw_cluster_shard(self.h, r)), int(num_walks))
            if rc != OK:
                raise SrwError(rc, "srw_plan_walks on shard %d" % r)
        return self

    def load_edgelist(self, path, directed=False, weighted=True, partitioned=False, rdd_partitions=200):
        self._ck(lib().srw_cluster_load_edgelist(self.h, os.fsencode(path), int(directed), int(weighted), int(partitioned),
                                                 rdd_partitions))
        return self

    def load_coo(self, src, dst, w=None, pid=None, directed=False):
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
        pid = None if pid is None else np.ascontiguousarray(pid, dtype=np.int32)
        self._ck(lib().srw_cluster_load_coo(self.h, _i32(src), _i32(dst), None if w is None else _f32(w),
                                            None if pid is None else _i32(pid), len(src), int(directed)))
        return self

    def generate_rmat(self, scale, n_edges=None, seed=42, weighted=False, directed=False):
        self._ck(lib().srw_cluster_generate_rmat(self.h, scale, (16 << scale) if n_edges is None else n_edges, seed,
                                                 int(weighted), int(directed)))
        return self

    def stats(self):
        v, e = C.c_int64(0), C.c_int64(0)
        self._ck(lib().srw_cluster_graph_stats(self.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    def shard(self, rank):
        """Non-owning Engine view of one shard's handle (graph queries, tests)."""
        e = Engine.__new__(Engine)
        e.h = C.c_void_p(lib().srw_cluster_shard(self.h, rank))
        e._owned = False
        e.rank, e.world = rank, self.world
        return e

    # ---- start vertices (srw_cluster_set_sources) ----
    def set_sources(self, ids):
        """Walk from these vertex ids (numpy array or sequence; any order, duplicates allowed) instead of from every vertex, until
        clear_sources() or the next load: canonical walker = iteration * len(ids) + position.  Each shard keeps what it owns."""
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("set_sources: vertex ids must be integers (got %s)" % a.dtype)
        if a.size and (int(a.min()) < -2**31 or int(a.max()) > 2**31 - 1):
            raise ValueError("set_sources: a vertex id is outside int32")
        a = np.array(a.reshape(-1), dtype=np.int32)                      # (a copy: the caller may reuse its array)
        self._ck(lib().srw_cluster_set_sources(self.h, _i32(a) if a.size else None, a.size))
        self._src_ids = a
        return self

    def clear_sources(self):
        self._ck(lib().srw_cluster_clear_sources(self.h))
        self._src_ids = None
        return self

    def sources_len(self):
        """Length of the list in force, None when there is none (walks start from every vertex)."""
        n = C.c_int64(0)
        self._ck(lib().srw_cluster_sources(self.h, C.byref(n)))
        return None if n.value < 0 else n.value

    _with_sources = Engine._with_sources

    def walk(self, fetch=True, batch=0, sources=None, **kw):
        """srw_cluster_walk (+ srw_cluster_fetch_paths).  sources=ids: from these vertices only, for this call (the previous state
        is back afterwards)."""
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk(fetch=fetch, batch=batch, **kw))
        P = Engine.params(**kw)
        st = WalkStats()
        self._ck(lib().srw_cluster_walk(self.h, C.byref(P), batch, C.byref(st)))
        if not fetch:
            return st.as_dict()
        nv = self.sources_len()                 # walkers per iteration: the list in force, else every vertex
        if nv is None:
            nv = self.stats()[0]
        n = P.num_walks * nv
        paths = np.empty((max(n, 1), P.walk_length + 2), dtype=np.int32)
        lens = np.empty(max(n, 1), dtype=np.int32)
        self._ck(lib().srw_cluster_fetch_paths(self.h, _i32(paths), _i32(lens)))
        return paths[:n], lens[:n], st.as_dict()

    def walk_and_save(self, output_dir, n_parts=1, write_crc=False, sources=None, **kw):
        if sources is not None:
            return self._with_sources(sources, lambda: self.walk_and_save(output_dir, n_parts=n_parts, write_crc=write_crc, **kw))
        P = Engine.params(**kw)
        st = WalkStats()
        self._ck(lib().srw_cluster_walk_and_save(self.h, C.byref(P), os.fsencode(output_dir), n_parts, int(write_crc), C.byref(st)))
        return st.as_dict()
