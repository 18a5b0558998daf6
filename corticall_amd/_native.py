"""ctypes binding of libldbg.so (include/ldbg.h).

The library is the product: hand-written HIP kernels for gfx950 behind a C ABI.  There is no
Python or CPU implementation behind these calls — if the shared object is missing, or no MI355X is
visible, every compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libldbg.so")
if os.environ.get("LDBG_DIAG_LIB") == "1":
    # the same sources built with the walk kernel's timers compiled in (make -C corticall_amd/csrc diag): profiling sessions only (tools/)
    LIB_PATH = os.path.join(_HERE, "_build_diag", "libldbg.so")
elif os.environ.get("LDBG_DIAG_LIB", "").startswith("variant"):
    # a tuning variant (make -C corticall_amd/csrc variant VARIANT_FLAGS=...; copies kept as _build_variantNAME): experiments of tools/ only
    LIB_PATH = os.path.join(_HERE, "_build_" + os.environ["LDBG_DIAG_LIB"], "libldbg.so")

LDBG_OK = 0
STATUS_NAMES = {
    1: "CortexJDKException", 2: "NullPointerException", 3: "NoSuchElementException", 4: "UnsupportedOperation",
    5: "HipError", 6: "IllegalArgument", 7: "CapacityError",
}
MAX_COLORS = 32


class CortexJDKException(RuntimeError):
    """uk.ac.ox.well.cortexjdk.utils.exceptions.CortexJDKException"""


class JavaNullPointerException(RuntimeError):
    pass


class NoSuchElementException(RuntimeError):
    pass


class LdbgError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class EngineConfig(C.Structure):
    _fields_ = [
        ("graph", C.c_void_p), ("rois", C.c_void_p), ("links", C.POINTER(C.c_void_p)), ("nlinks", C.c_int),
        ("traversal_colors", C.c_int * MAX_COLORS), ("n_traversal", C.c_int),
        ("joining_colors", C.c_int * MAX_COLORS), ("n_joining", C.c_int),
        ("recruitment_colors", C.c_int * MAX_COLORS), ("n_recruitment", C.c_int),
        ("secondary_colors", C.c_int * MAX_COLORS), ("n_secondary", C.c_int),
        ("direction", C.c_int), ("combination_operator", C.c_int), ("stopping_rule", C.c_int),
        ("max_branch_length", C.c_int), ("connect_all_neighbors", C.c_int), ("strict_java_flip", C.c_int),
    ]


class RecordFilter(C.Structure):
    """ldbg_record_filter"""
    _fields_ = [
        ("all_zero", C.c_uint64), ("all_positive", C.c_uint64), ("any_positive", C.c_uint64), ("none_positive", C.c_uint64),
        ("cov_color", C.c_int32), ("cov_below", C.c_int32), ("degree_color", C.c_int32), ("degree_above", C.c_int32),
    ]


SEED_MAX_COVERED, SEED_MAX_UNIQUE = 3, 8


class SeedCovered(C.Structure):
    """ldbg_seed_covered"""
    _fields_ = [("mask", C.c_uint64), ("at_least", C.c_int32), ("at_most", C.c_int32)]


class SeedUnique(C.Structure):
    """ldbg_seed_unique"""
    _fields_ = [("colour", C.c_int32), ("occurrences", C.c_void_p), ("d_unique", C.c_void_p)]


class SeedFilter(C.Structure):
    """ldbg_seed_filter"""
    _fields_ = [("all_zero", C.c_uint64), ("n_covered", C.c_int32), ("covered", SeedCovered * SEED_MAX_COVERED),
                ("n_unique", C.c_int32), ("unique", SeedUnique * SEED_MAX_UNIQUE)]


class SeedCounts(C.Structure):
    """ldbg_seed_counts"""
    _fields_ = [("n_seeds", C.c_int64), ("n_unique", C.c_int64), ("n_good", C.c_int64), ("device_ms", C.c_double)]


class CursorStop(C.Structure):
    """ldbg_cursor_stop"""
    _fields_ = [("colour", C.c_int), ("arrival_degree_one", C.c_int), ("targets", C.c_void_p)]


VARIANT_FIELDS = ("status", "source_rec", "dest_rec", "n_child", "n_parent", "st", "s0end", "s1end", "child_sum", "child_flag", "parent_sum",
                  "parent_flag", "allele_offsets", "alleles", "child_offsets", "child_words", "child_rec", "parent_offsets", "parent_words", "parent_rec")


class VariantArrays(C.Structure):
    """ldbg_variant_arrays"""
    _fields_ = [(name, C.c_void_p) for name in VARIANT_FIELDS]


class MosaicParams(C.Structure):
    """ldbg_mosaic_params"""
    _fields_ = [("del_", C.c_double), ("eps", C.c_double), ("rho", C.c_double), ("term", C.c_double)]


MOSAIC_FIELDS = ("status", "llk", "path_off", "copy", "state", "pos")


class MosaicArrays(C.Structure):
    """ldbg_mosaic_arrays"""
    _fields_ = [(name, C.c_void_p) for name in MOSAIC_FIELDS]


SW_FIELDS = ("status", "score", "end_q", "end_s", "begin_q", "begin_s", "aligned_len", "edits", "col_off", "cols", "q_off", "q_letters", "s_off",
             "s_letters")


class SwArrays(C.Structure):
    """ldbg_sw_arrays"""
    _fields_ = [(name, C.c_void_p) for name in SW_FIELDS]


class BuildSample(C.Structure):
    """ldbg_build_sample"""
    _fields_ = [("sample_name", C.c_char_p), ("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_sequences", C.c_int64)]


class ColorInfo(C.Structure):
    _fields_ = [
        ("mean_read_length", C.c_uint32), ("total_sequence", C.c_uint64),
        ("tip_clipping", C.c_uint8), ("low_covg_supernodes_removed", C.c_uint8),
        ("low_covg_kmers_removed", C.c_uint8), ("cleaned_against_graph", C.c_uint8),
        ("low_cov_supernodes_threshold", C.c_uint32), ("low_cov_kmer_threshold", C.c_uint32),
    ]


# every symbol include/ldbg.h declares (tests check that the built library exports all of them)
EXPORTS = [
    "ldbg_last_error", "ldbg_version", "ldbg_device_count", "ldbg_kmer_encode", "ldbg_kmer_decode",
    "ldbg_sort_ctx", "ldbg_join_ctx", "ldbg_ctx_write_records", "ldbg_graph_open", "ldbg_graph_open_memory", "ldbg_graph_open_device", "ldbg_graph_open_collection", "ldbg_graph_close", "ldbg_graph_info", "ldbg_graph_device", "ldbg_graph_set_shard",
    "ldbg_graph_sample_name", "ldbg_graph_color_info", "ldbg_graph_color_for_sample_name",
    "ldbg_graph_records", "ldbg_graph_records_dev", "ldbg_graph_find", "ldbg_graph_find_ascii", "ldbg_graph_find_dev", "ldbg_shard_owner_dev", "ldbg_shard_owner", "ldbg_shard_nbr_queries", "ldbg_shard_set_nbr",
    "ldbg_image_create", "ldbg_image_destroy", "ldbg_image_graph", "ldbg_image_row_bytes", "ldbg_image_clear", "ldbg_image_request", "ldbg_image_reset_requests", "ldbg_image_bucket",
    "ldbg_image_serve", "ldbg_image_serve_chain", "ldbg_image_insert", "ldbg_image_lookup", "ldbg_image_counters",
    "ldbg_engine_sharded_walk_begin", "ldbg_engine_sharded_walk_round", "ldbg_engine_sharded_walk_finish", "ldbg_engine_sharded_dfs_batch",
    "ldbg_links_open", "ldbg_links_close", "ldbg_links_index", "ldbg_links_source", "ldbg_links_info", "ldbg_links_sample_name", "ldbg_links_get",
    "ldbg_engine_config_default", "ldbg_engine_create", "ldbg_engine_destroy",
    "ldbg_engine_walk_batch", "ldbg_engine_walk_batch_run", "ldbg_engine_walk_batch_run_device", "ldbg_engine_walk_batch_fetch", "ldbg_host_alloc", "ldbg_host_free", "ldbg_engine_walk_vertices", "ldbg_engine_walk_roi_hits",
    "ldbg_engine_dfs_batch", "ldbg_dfs_result_sizes", "ldbg_dfs_result_get", "ldbg_dfs_result_walk", "ldbg_dfs_result_merge", "ldbg_dfs_result_free", "ldbg_engine_neighbours_batch", "ldbg_engine_assemble",
    "ldbg_engine_dfs_kmers_traversed",
    "ldbg_engine_seek", "ldbg_engine_has_next", "ldbg_engine_has_previous", "ldbg_engine_next", "ldbg_engine_previous",
    "ldbg_engine_cursor_batch", "ldbg_engine_cursor_batch_device", "ldbg_cursor_result_sizes", "ldbg_cursor_result_get", "ldbg_cursor_result_get_dev",
    "ldbg_cursor_result_free",
    "ldbg_engine_variant_batch", "ldbg_engine_variant_batch_device", "ldbg_variant_result_sizes", "ldbg_variant_result_get", "ldbg_variant_result_get_dev",
    "ldbg_variant_result_free",
    "ldbg_mosaic_align_batch", "ldbg_mosaic_result_sizes", "ldbg_mosaic_result_get", "ldbg_mosaic_result_free", "ldbg_mosaic_tb_roundtrip",
    "ldbg_sw_align_batch", "ldbg_sw_result_sizes", "ldbg_sw_result_get", "ldbg_sw_result_free",
    "ldbg_profile_reset", "ldbg_profile_get",
    "ldbg_graph_unitigs", "ldbg_unitigs_info", "ldbg_unitigs_get", "ldbg_unitigs_get_dev", "ldbg_unitigs_coverage", "ldbg_unitigs_of_records",
    "ldbg_unitigs_write_fasta", "ldbg_unitigs_write_gfa1", "ldbg_unitigs_free",
    "ldbg_graph_select", "ldbg_graph_select_lookup", "ldbg_selection_count", "ldbg_selection_indices", "ldbg_selection_indices_dev",
    "ldbg_selection_write_ctx", "ldbg_selection_open_graph", "ldbg_selection_free",
    "ldbg_graph_recover", "ldbg_selection_recovered_coverage", "ldbg_selection_write_recovered", "ldbg_selection_open_recovered",
    "ldbg_graph_build", "ldbg_graph_build_ctx",
    "ldbg_links_build", "ldbg_links_build_ctp",
    "ldbg_graph_thread", "ldbg_graph_thread_dev", "ldbg_threading_info", "ldbg_threading_windows", "ldbg_threading_windows_dev", "ldbg_threading_coverage",
    "ldbg_threading_summary", "ldbg_threading_regions", "ldbg_threading_free",
    "ldbg_threading_occurrences", "ldbg_occurrences_info", "ldbg_occurrences_get", "ldbg_occurrences_get_dev", "ldbg_occurrences_free",
    "ldbg_graph_variant_seeds",
]


class NativeLib:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C corticall_amd/csrc).  corticall_amd has no CPU fallback.")
        self.path = path
        self.dll = C.CDLL(path)
        d = self.dll
        d.ldbg_last_error.restype = C.c_char_p
        d.ldbg_version.restype = C.c_char_p
        for name in EXPORTS:
            getattr(d, name)   # raises AttributeError if a declared symbol is not exported
        d.ldbg_engine_config_default.restype = None
        try:                    # the host simulation of the test suite (tests/hostsim) exports this; libldbg.so does not
            d.ldbg_hostsim_set_lanes
            self.is_hostsim = True
        except AttributeError:
            self.is_hostsim = False

    def check(self, status):
        if status == LDBG_OK:
            return
        msg = self.dll.ldbg_last_error().decode(errors="replace")
        if status == 1:
            raise CortexJDKException(msg)
        if status == 2:
            raise JavaNullPointerException(msg)
        if status == 3:
            raise NoSuchElementException(msg)
        raise LdbgError(status, msg)

    def device_count(self):
        n = C.c_int()
        self.dll.ldbg_device_count(C.byref(n))
        return n.value


_default = None


def default_lib():
    global _default
    if _default is None:
        _default = NativeLib()
    return _default
