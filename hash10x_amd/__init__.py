"""hash10x_amd — MI355X (gfx950) implementation of hash10x's mosh-construction + clustering path.

This package is plumbing only: a ctypes binding of the C session layer (hash10x_amd/host/,
`libh10x_host.so`) which drives the HIP kernels through the C ABI of include/h10x.h
(`libh10x_hip.so`). There is no Python or CPU compute path: if the native libraries are missing or
no gfx950 device is present, construction fails loudly.

`Hash10x` mirrors the reference's command surface (hash10x.c:1200-1269):
    --readFQB -> read_fqb / read_fqb_file      --readHash  -> read_hash
    --writeHash -> write_hash                  --hashDepthRange -> depth_range
    --cluster -> cluster                       --clusterSplit -> cluster_split
with -k -w -r -B -N -c -ct as constructor / method arguments.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_HIP_SO = os.path.join(_HERE, "libh10x_hip.so")
_HOST_SO = os.path.join(_HERE, "libh10x_host.so")
ABI_VERSION = 3          # include/h10x.h H10X_ABI_VERSION this binding was written for (load_native checks the library's)


class Hash10xError(RuntimeError):
    """Raised with the reference's die() text where the reference would have died."""


class _Counters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "pairs", "kmers", "entries", "distinct", "clustered_codes", "sum_good", "sum_good_depth",
        "sum_hash_clustered", "fallback_blocks")] + [("cluster_class_counts", ctypes.c_uint64 * 4), ("cluster_first_mode", ctypes.c_uint64), ("cluster_overflow_blocks", ctypes.c_uint64), ("cluster_main", ctypes.c_uint64 * 4), ("cluster_phase_ticks", ctypes.c_uint64 * 8), ("list_words", ctypes.c_uint64 * 2), ("index_table_form", ctypes.c_uint64), ("shard_reply_path", ctypes.c_uint64)]


class _Sizes(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("hashNumber", ctypes.c_uint32), ("nBlocks", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("nClusHash", ctypes.c_uint64), ("nRecords", ctypes.c_uint64)]


class _ShardInfo(ctypes.Structure):
    _fields_ = [("rank", ctypes.c_int32), ("nranks", ctypes.c_int32), ("B", ctypes.c_int32), ("hashNumber", ctypes.c_uint32),
                ("nBlocksGlobal", ctypes.c_uint32), ("nSegs", ctypes.c_uint32), ("nEntriesGlobal", ctypes.c_uint64), ("nRecordsGlobal", ctypes.c_uint64)]


class _ShardSeg(ctypes.Structure):
    _fields_ = [("rank", ctypes.c_uint32), ("localStart", ctypes.c_uint32), ("count", ctypes.c_uint32), ("globalBase", ctypes.c_uint32),
                ("entries", ctypes.c_uint64), ("localEntryStart", ctypes.c_uint64), ("globalEntryStart", ctypes.c_uint64)]


class _MoshInfo(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("k", ctypes.c_int32), ("w", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("factor1", ctypes.c_uint64), ("factor2", ctypes.c_uint64), ("max", ctypes.c_uint32), ("size", ctypes.c_uint32)]


class _MoshCounters(ctypes.Structure):
    _fields_ = [("scan_retries", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 3)]


class _SeqhashRec(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("w", ctypes.c_int32), ("mask", ctypes.c_uint64), ("shift1", ctypes.c_int32), ("shift2", ctypes.c_int32),
                ("factor1", ctypes.c_uint64), ("factor2", ctypes.c_uint64), ("patternRC", ctypes.c_uint64 * 4)]


class _MoshFile(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("size", ctypes.c_uint32), ("sh", _SeqhashRec), ("index", ctypes.c_void_p), ("value", ctypes.c_void_p),
                ("depth", ctypes.c_void_p), ("info", ctypes.c_void_p)]


class _ReadsetInfo(ctypes.Structure):
    _fields_ = [("nReads", ctypes.c_uint32), ("dim", ctypes.c_uint32), ("totHit", ctypes.c_uint64)]


class _RefmapInfo(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("max", ctypes.c_uint32), ("setMax", ctypes.c_uint32), ("packed", ctypes.c_int32)]


class _ReadsetFile(ctypes.Structure):
    _fields_ = [("totHit", ctypes.c_uint64), ("dim", ctypes.c_uint32), ("max", ctypes.c_uint32), ("reads", ctypes.c_void_p), ("hit", ctypes.c_void_p),
                ("dx", ctypes.c_void_p)]


# h10x_read_t (the 72-byte Read of the RSMSHv2 file) and h10x_overlap_t (include/h10x.h)
READ_DTYPE = np.dtype([("len", "<i4"), ("nHit", "<i4"), ("hitPtr", "<u8"), ("dxPtr", "<u8"), ("bad", "u1"), ("otherFlags", "u1"), ("pad1", "<u2"), ("nMiss", "<i4"),
                       ("contained", "<i4"), ("nCopy", "<i4", (4,)), ("pad2", "<u4", (4,)), ("tail", "<u4")])
OVERLAP_DTYPE = np.dtype([("iy", "<u4"), ("nHit", "<i4"), ("offset", "<i4"), ("isPlus", "u1"), ("isBad", "u1"), ("visited", "u1"), ("pad", "u1"), ("nPlus", "<i4"),
                          ("nMinus", "<i4"), ("d", "<f8"), ("sd", "<f8"), ("sumZ", "<i8"), ("sumZ2", "<i8")])
assert READ_DTYPE.itemsize == 72 and OVERLAP_DTYPE.itemsize == 56

_BLOCK_REP = np.dtype([("nGood", "<u4"), ("nClusHash", "<u4"), ("nClusRead", "<u4"), ("reserved", "<u4")])
_CLUSTER_REP = np.dtype([("n", "<u4"), ("nRead", "<u4"), ("nt", "<u4", (5,)), ("nBad", "<u4"), ("chr", "<i2"), ("pMin", "<u2"), ("pMax", "<u2"), ("nOtherListed", "<u2"), ("other", "<u4", (10,))])
assert _BLOCK_REP.itemsize == 16 and _CLUSTER_REP.itemsize == 80       # h10x_block_rep / h10x_cluster_rep (include/h10x.h)

_libs = None


def load_native():
    """Load libh10x_hip.so + libh10x_host.so (built in-tree by __graft_entry__.build()). No fallback."""
    global _libs
    if _libs is not None:
        return _libs
    for p in (_HIP_SO, _HOST_SO):
        if not os.path.exists(p):
            raise Hash10xError("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hash10x_amd has no CPU fallback)" % p)
    hip = ctypes.CDLL(_HIP_SO, mode=ctypes.RTLD_GLOBAL)
    host = ctypes.CDLL(_HOST_SO, mode=ctypes.RTLD_GLOBAL)
    vp, ci, cu64, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p
    host.h10x_session_new.restype = vp
    host.h10x_session_free.argtypes = [vp]
    host.h10x_session_set.argtypes = [vp, cs, ci]
    host.h10x_session_get.argtypes = [vp, cs]
    host.h10x_session_error.restype = cs
    host.h10x_session_error.argtypes = [vp]
    host.h10x_session_ctx.restype = vp
    host.h10x_session_ctx.argtypes = [vp]
    host.h10x_session_readFQB.argtypes = [vp, cs]
    host.h10x_session_begin.argtypes = [vp]
    host.h10x_session_after_read.argtypes = [vp]
    host.h10x_session_readFQB_mem.argtypes = [vp, vp, cu64]
    host.h10x_session_readFQB_dev.argtypes = [vp, vp, cu64]
    host.h10x_session_readHash.argtypes = [vp, cs]
    host.h10x_session_writeHash.argtypes = [vp, cs]
    host.h10x_session_hashDepthRange.argtypes = [vp, ci, ci]
    host.h10x_session_cluster.argtypes = [vp, ci, ci]
    host.h10x_session_clusterSplit.argtypes = [vp]
    host.h10x_host_array_dim.argtypes = [ci, ci, ctypes.c_int64]
    host.h10x_host_check_chunks.restype = ctypes.c_int64
    host.h10x_host_check_chunks.argtypes = [vp, cu64, ci, ci, cs, ci]
    host.h10x_host_partition.argtypes = [vp, cu64, ci, vp]
    host.h10x_session_shardReadFQB_mem.argtypes = [vp, vp, vp, cu64]
    host.h10x_session_shardReadFQB_dev.argtypes = [vp, vp, vp, cu64]
    host.h10x_session_shardGather.argtypes = [vp]
    host.h10x_session_shardReadHash.argtypes = [vp, vp, cs]
    host.h10x_session_shardReadFQB_file.argtypes = [vp, vp, cs, cu64, cu64]
    host.h10x_host_partition_file.argtypes = [cs, cu64, ci, vp, cs, ci]
    host.h10x_session_cribBuild.argtypes = [vp, cs, cs, vp, ci]
    host.h10x_session_clusterReport.argtypes = [vp, ci, ci, vp]
    host.h10x_session_cribSummary.argtypes = [vp, vp]
    host.h10x_session_hashStats.argtypes = [vp, vp]
    host.h10x_session_codeStats.argtypes = [vp, vp]
    hip.h10x_shard_info.argtypes = [vp, ctypes.POINTER(_ShardInfo)]
    hip.h10x_shard_segments.argtypes = [vp, vp, ctypes.c_uint32]
    hip.h10x_export_slice.argtypes = [vp, ci, cu64, cu64, vp]
    hip.h10x_shard_prepare_export.argtypes = [vp]
    hip.h10x_comm_unique_id.argtypes = [vp]
    hip.h10x_comm_create_rccl.argtypes = [ctypes.POINTER(vp), ci, ci, vp, ci, cs, ci]
    hip.h10x_comm_create_local.argtypes = [ctypes.POINTER(vp), ci]
    hip.h10x_comm_create_socket.argtypes = [ctypes.POINTER(vp), ci, ci, cs, ci, cs, ci]
    hip.h10x_comm_destroy.argtypes = [vp]
    hip.h10x_shard_barrier.argtypes = [vp]
    hip.h10x_shard_allreduce_max.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    hip.h10x_shard_allreduce_sum_u64.argtypes = [vp, vp, ctypes.c_uint32]
    hip.h10x_shard_allreduce_max_u64.argtypes = [vp, vp, ctypes.c_uint32]
    hip.h10x_ingest_fqb.argtypes = [vp, vp, cu64, ci]
    hip.h10x_ingest_reserve.argtypes = [vp, cu64]
    hip.h10x_build_id.restype = cs
    hip.h10x_device_malloc.restype = vp
    hip.h10x_device_malloc.argtypes = [ci, cu64]
    hip.h10x_device_free.argtypes = [ci, vp]
    hip.h10x_device_upload.argtypes = [ci, vp, vp, cu64]
    hip.h10x_device_synchronize.argtypes = [ci]
    hip.h10x_device_download.argtypes = [ci, vp, vp, cu64]
    hip.h10x_device_mem_info.argtypes = [ci, ctypes.POINTER(cu64), ctypes.POINTER(cu64)]
    hip.h10x_crib_genome.argtypes = [vp, vp, vp, ctypes.c_uint32, ci, ctypes.POINTER(cu64), ctypes.POINTER(cu64)]
    hip.h10x_crib_finish.argtypes = [vp]
    hip.h10x_cluster_report.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, cu64, ctypes.POINTER(cu64)]
    hip.h10x_device_count.restype = ci
    hip.h10x_warm.restype = ci; hip.h10x_warm.argtypes = [ci]
    hip.h10x_alloc_stats.restype = None; hip.h10x_alloc_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.h10x_abi_version.restype = ci
    hip.h10x_factor1_from_seed.restype = cu64
    hip.h10x_factor1_from_seed.argtypes = [ctypes.c_int32]
    hip.h10x_timing_enable.argtypes = [vp, ci]
    hip.h10x_timing_count.argtypes = [vp]
    hip.h10x_timing_name.restype = cs
    hip.h10x_timing_name.argtypes = [vp, ci]
    hip.h10x_timing_get.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(cu64)]
    hip.h10x_timing_reset.argtypes = [vp]
    hip.h10x_exchange_name.restype = cs; hip.h10x_exchange_name.argtypes = [ci]
    hip.h10x_exchange_beside.restype = ci; hip.h10x_exchange_beside.argtypes = [vp, ci]
    hip.h10x_timing_wait_get.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    hip.h10x_exchange_get.argtypes = [vp, ci, ctypes.POINTER(cu64), ctypes.POINTER(cu64), ctypes.POINTER(cu64), ctypes.POINTER(cu64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    hip.h10x_comm_local_serialize.argtypes = [vp, ci]
    hip.h10x_comm_turn_begin.argtypes = [vp]
    hip.h10x_comm_turn_end.argtypes = [vp, ci]
    hip.h10x_get_counters.argtypes = [vp, ctypes.POINTER(_Counters)]
    hip.h10x_get_sizes.argtypes = [vp, ctypes.POINTER(_Sizes)]
    hip.h10x_set_option.argtypes = [vp, cs, ctypes.c_int64]
    hip.h10x_last_error.restype = cs
    hip.h10x_last_error.argtypes = [vp]
    hip.h10x_export.argtypes = [vp, vp, vp, vp, vp, vp]
    hip.h10x_neighbours.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, cu64, vp]
    hip.h10x_neighbour_max.argtypes = [vp, vp, ctypes.c_uint32, vp, vp]
    hip.h10x_neighbour_hist.argtypes = [vp, vp, ctypes.c_uint32, vp, vp]
    hip.h10x_neighbour_stats.argtypes = [vp, vp, ci]
    hip.h10x_code_share.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, cu64]
    hip.h10x_code_explore.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp]
    hip.h10x_code_crib_counts.argtypes = [vp, vp, ctypes.c_uint32, vp]
    # barcode census and whitelist correction (csrc/stage_j.hip)
    hip.h10x_census_begin.argtypes = [vp, cu64]
    hip.h10x_census_add.argtypes = [vp, vp, cu64]
    hip.h10x_census_add_device.argtypes = [vp, vp, cu64]
    hip.h10x_census_close.argtypes = [vp, ctypes.c_int64, vp]
    hip.h10x_census_export.argtypes = [vp, ci, vp, vp, cu64]
    hip.h10x_whitelist_set.argtypes = [vp, vp, cu64]
    hip.h10x_fix_fqb.argtypes = [vp, vp, cu64, vp, ctypes.POINTER(cu64), vp]
    hip.h10x_fix_fqb_device.argtypes = [vp, vp, cu64, vp, ctypes.POINTER(cu64), vp]
    host.h10x_session_codeCensus.argtypes = [vp, ci, cs, cs, vp]
    host.h10x_session_fixFQB.argtypes = [vp, cs, cs, cs, vp]
    host.h10x_session_fixFQBThresh.argtypes = [vp, ci, cs, cs, vp]
    host.h10x_host_whitelist_read.argtypes = [cs, ctypes.POINTER(vp), ctypes.POINTER(cu64), cs, ci]
    host.h10x_host_whitelist_free.restype = None; host.h10x_host_whitelist_free.argtypes = [vp]
    host.h10x_host_whitelist_write.argtypes = [cs, vp, cu64, cs, ci]
    host.h10x_host_whitelist_lines.argtypes = [vp, cu64, vp, cu64, vp]
    # the molecule of every read pair, the records in molecule order (csrc/stage_k.hip)
    hip.h10x_molecule_map.argtypes = [vp, vp, vp, cu64, vp]
    hip.h10x_molecule_map_device.argtypes = [vp, vp, vp, cu64, vp]
    hip.h10x_split_fqb.argtypes = [vp, vp, cu64, vp, vp, cu64]
    hip.h10x_split_fqb_device.argtypes = [vp, vp, cu64, vp, vp, cu64]
    host.h10x_session_moleculeMap.argtypes = [vp, cs, vp]
    host.h10x_session_splitFQB.argtypes = [vp, cs, cs, vp]
    host.h10x_host_write_molmap.argtypes = [cs, vp, vp, vp, cs, ci]
    host.h10x_host_write_split_index.argtypes = [cs, vp, ctypes.c_uint32, ctypes.c_uint32, cs, ci]
    # the share graph (csrc/stage_l.hip)
    hip.h10x_share_graph_run.argtypes = [vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, vp]
    hip.h10x_share_graph_get.argtypes = [vp, vp, vp, vp, cu64]
    hip.h10x_share_graph_get_device.argtypes = [vp, vp, vp, vp, cu64]
    host.h10x_session_shareGraph.argtypes = [vp, ci, cs, vp]
    # the components of the share graph (csrc/stage_m.hip)
    hip.h10x_share_components_begin.argtypes = [vp, ctypes.c_int64]
    hip.h10x_share_components_add.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    hip.h10x_share_components_finish.argtypes = [vp, vp]
    hip.h10x_share_components_get.argtypes = [vp, vp, vp, vp, vp, vp, cu64, cu64]
    host.h10x_session_shareComponents.argtypes = [vp, ci, cs, vp]
    host.h10x_session_shareComponentsRun.argtypes = [vp, ci, vp]
    # the per-hash linkage groups (csrc/stage_n.hip)
    hip.h10x_hash_copies_run.argtypes = [vp, ctypes.c_int64, vp]
    hip.h10x_hash_copies_get.argtypes = [vp, vp, cu64, cu64]
    hip.h10x_hash_copies_get_device.argtypes = [vp, vp, cu64, cu64]
    hip.h10x_hash_copies_tally.argtypes = [vp, vp]
    hip.h10x_crib_export.argtypes = [vp, vp, vp, vp, vp]
    hip.h10x_crib_sizes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), vp]
    hip.h10x_crib_summary.argtypes = [vp, vp, vp, vp]
    hip.h10x_crib_words.argtypes = [vp, cu64, cu64, vp]
    host.h10x_session_hashCopies.argtypes = [vp, ci, cs, vp]
    host.h10x_session_hashCopiesRun.argtypes = [vp, ci, vp]
    # the state as a mosh set (csrc/stage_o.hip)
    hip.h10x_mosh_from_state.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp), vp]
    host.h10x_session_moshSet.argtypes = [vp, ci, ci, ci, ci, ctypes.POINTER(vp), vp]
    host.h10x_session_writeMosh.argtypes = [vp, ci, ci, ci, ci, cs, vp, vp]
    # from sequences to blocks (csrc/stage_p.hip)
    hip.h10x_seq_hashes.argtypes = [vp, vp, vp, ctypes.c_uint32, vp]
    hip.h10x_seq_hashes_get.argtypes = [vp, vp, vp, cu64]
    hip.h10x_list_share_run.argtypes = [vp, ctypes.c_int64, vp, vp, ctypes.c_uint32, vp]
    hip.h10x_seq_blocks_run.argtypes = [vp, ctypes.c_int64, vp, vp, ctypes.c_uint32, vp, vp]
    hip.h10x_list_share_get.argtypes = [vp, vp, vp, vp, cu64]
    hip.h10x_list_share_get_device.argtypes = [vp, vp, vp, vp, cu64]
    host.h10x_session_seqBlocks.argtypes = [vp, ci, cs, cs, vp, ci]
    # row links (csrc/stage_q.hip)
    hip.h10x_row_links_begin.argtypes = [vp, ctypes.c_uint32]
    hip.h10x_row_links_add.argtypes = [vp, vp, vp, cu64]
    hip.h10x_row_links_add_kept.argtypes = [vp]
    hip.h10x_row_links_finish.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, vp]
    hip.h10x_row_links_get.argtypes = [vp, vp, vp, vp, cu64]
    hip.h10x_row_links_get_device.argtypes = [vp, vp, vp, vp, cu64]
    hip.h10x_row_links_get_range.argtypes = [vp, cu64, cu64, vp, vp]
    host.h10x_session_seqLinks.argtypes = [vp, ci, ci, ci, ci, cs, cs, vp, ci]
    # sequence spans (csrc/stage_r.hip)
    hip.h10x_seq_spans_run.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.c_uint32, vp, vp]
    hip.h10x_seq_spans_get.argtypes = [vp, vp, vp, vp, vp, vp, cu64]
    hip.h10x_seq_spans_get_range.argtypes = [vp, cu64, cu64, vp, vp, vp, vp]
    hip.h10x_seq_spans_cover_get.argtypes = [vp, vp, vp, cu64]
    host.h10x_session_seqSpans.argtypes = [vp, ci, ci, ci, ci, cs, cs, vp, ci]
    # sequence spectrum (csrc/stage_s.hip)
    hip.h10x_seq_spectrum_begin.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    hip.h10x_seq_spectrum_add.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp]
    hip.h10x_seq_spectrum_windows_get.argtypes = [vp, vp, vp, cu64]
    hip.h10x_seq_spectrum_finish.argtypes = [vp, vp, vp, vp]
    hip.h10x_seq_spectrum_copies_get.argtypes = [vp, cu64, cu64, vp]
    host.h10x_session_seqSpectrum.argtypes = [vp, ci, ci, ci, ci, cs, cs, vp, ci]
    host.h10x_host_qv.restype = ctypes.c_double; host.h10x_host_qv.argtypes = [cu64, cu64, ci]
    # mosh sets (csrc/stage_g.hip, host/mosh_host.c)
    pvp, ci32, cu32 =ctypes.POINTER(vp), ctypes.c_int32, ctypes.c_uint32
    hip.h10x_factors_from_seed.restype = None; hip.h10x_factors_from_seed.argtypes = [ci32, ctypes.POINTER(cu64), ctypes.POINTER(cu64)]
    hip.h10x_mosh_create.argtypes = [pvp, ci32, ci32, ci32, ci32, ci, cs, ci]
    hip.h10x_mosh_load.argtypes = [pvp, ci32, ci32, ci32, cu64, cu64, vp, vp, vp, vp, cu32, ci, cs, ci]
    hip.h10x_mosh_destroy.restype = None; hip.h10x_mosh_destroy.argtypes = [vp]
    hip.h10x_mosh_error.restype = cs; hip.h10x_mosh_error.argtypes = [vp]
    hip.h10x_mosh_info.argtypes = [vp, ctypes.POINTER(_MoshInfo)]
    hip.h10x_mosh_set_option.argtypes = [vp, cs, ctypes.c_int64]
    hip.h10x_mosh_counters.argtypes = [vp, ctypes.POINTER(_MoshCounters)]
    hip.h10x_get_scan_retries.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    hip.h10x_readset_chunks.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    hip.h10x_mosh_add.argtypes = [vp, vp, vp, cu32, ci, cu64, ctypes.POINTER(cu64)]
    hip.h10x_mosh_scan.argtypes = [vp, vp, vp, cu32, ci, cu64, vp, vp, vp, cu64, ctypes.POINTER(cu64)]
    hip.h10x_mosh_merge.argtypes = [vp, ci32, ci32, cu64, vp, vp, vp, cu32, ctypes.POINTER(ci)]
    hip.h10x_mosh_prune.argtypes = [vp, ci32, ci32, ctypes.POINTER(cu32), ctypes.POINTER(cu32)]
    hip.h10x_mosh_set_copy.argtypes = [vp, ci32, ci32, ci32]
    hip.h10x_mosh_set_copy_m.argtypes = [vp, ci32]
    hip.h10x_mosh_summary.argtypes = [vp, vp, vp]
    hip.h10x_mosh_export.argtypes = [vp, cu64, cu64, vp, vp, vp, vp]
    hip.h10x_mosh_lookup.argtypes = [vp, vp, cu64, vp, vp]
    host.h10x_seq_open.restype = vp; host.h10x_seq_open.argtypes = [cs, cs, ci, ctypes.POINTER(ci)]
    host.h10x_seq_next.argtypes = [vp, cu64, pvp, pvp, ctypes.POINTER(cu32)]
    host.h10x_seq_error.restype = cs; host.h10x_seq_error.argtypes = [vp]
    host.h10x_seq_warning.restype = cs; host.h10x_seq_warning.argtypes = [vp]
    host.h10x_seq_close.restype = None; host.h10x_seq_close.argtypes = [vp]
    host.h10x_moshfile_read.argtypes = [cs, ctypes.POINTER(_MoshFile), cs, ci]
    host.h10x_moshfile_free.restype = None; host.h10x_moshfile_free.argtypes = [ctypes.POINTER(_MoshFile)]
    host.h10x_mosh_set_write.argtypes = [vp, cs, cs, ci]
    host.h10x_mosh_set_add_file.argtypes = [vp, cs, ci, cu64, ctypes.POINTER(cu64), ctypes.POINTER(cu64), ctypes.POINTER(cu64), cs, ci, cs, ci]
    # readsets (csrc/stage_h.hip, host/asm_host.c)
    hip.h10x_readset_create.argtypes = [pvp, vp]
    hip.h10x_readset_load.argtypes = [pvp, vp, vp, cu32, cu32, vp, vp]
    hip.h10x_readset_destroy.restype = None; hip.h10x_readset_destroy.argtypes = [vp]
    hip.h10x_readset_error.restype = cs; hip.h10x_readset_error.argtypes = [vp]
    hip.h10x_readset_add.argtypes = [vp, vp, vp, cu32]
    hip.h10x_readset_info.argtypes = [vp, ctypes.POINTER(_ReadsetInfo)]
    hip.h10x_readset_export.argtypes = [vp, pvp, pvp, pvp, pvp]
    hip.h10x_readset_overlap_cap.argtypes = [vp, cu32, ctypes.POINTER(cu32)]
    hip.h10x_readset_overlaps.argtypes = [vp, cu32, vp, cu32, ctypes.POINTER(cu32), vp]
    hip.h10x_readset_mark_bad.argtypes = [vp, vp]
    hip.h10x_readset_mark_contained.argtypes = [vp, ctypes.POINTER(ci32), ctypes.POINTER(ci32), ctypes.POINTER(cu64)]
    hip.h10x_readset_stats_sums.argtypes = [vp, vp]
    host.h10x_readsetfile_read.argtypes = [cs, cu32, ctypes.POINTER(_ReadsetFile), cs, ci]
    host.h10x_readsetfile_free.restype = None; host.h10x_readsetfile_free.argtypes = [ctypes.POINTER(_ReadsetFile)]
    host.h10x_readsetfile_write.argtypes = [cs, cu64, cu32, vp, cu32, vp, vp, vp, cs, ci]
    host.h10x_readset_write_file.argtypes = [vp, cs, cs, ci]
    host.h10x_readset_add_file.argtypes = [vp, cs, cu64, cs, ci, cs, ci]
    # reference maps (csrc/stage_i.hip)
    hip.h10x_refmap_create.argtypes = [pvp, vp, cu32]
    hip.h10x_refmap_load.argtypes = [pvp, vp, vp, vp, vp, vp, vp, vp, cu32, cu32]
    hip.h10x_refmap_destroy.restype = None; hip.h10x_refmap_destroy.argtypes = [vp]
    hip.h10x_refmap_error.restype = cs; hip.h10x_refmap_error.argtypes = [vp]
    hip.h10x_refmap_info.argtypes = [vp, ctypes.POINTER(_RefmapInfo)]
    hip.h10x_refmap_add.argtypes = [vp, vp, vp, cu32, cu32, ctypes.POINTER(cu64)]
    hip.h10x_refmap_pack.argtypes = [vp, ctypes.POINTER(cu32), ctypes.POINTER(cu32), ctypes.POINTER(cu32)]
    hip.h10x_refmap_export.argtypes = [vp, pvp, pvp, pvp, pvp, pvp, pvp]
    hip.h10x_refmap_query.argtypes = [vp, vp, vp, cu32, ci]
    hip.h10x_refmap_results.argtypes = [vp, ctypes.POINTER(cu32), pvp, pvp, pvp, pvp, pvp, pvp]
    if hip.h10x_abi_version() != ABI_VERSION:
        raise RuntimeError("libh10x_hip.so speaks ABI %d, hash10x_amd/__init__.py was written for %d (include/h10x.h H10X_ABI_VERSION): rebuild with "
                           "`python -c 'import __graft_entry__ as g; g.build()'`" % (hip.h10x_abi_version(), ABI_VERSION))
    _libs = (hip, host)
    return _libs


def device_count():
    return load_native()[0].h10x_device_count()


def device_mem_info(device=0):
    """(free, total) bytes of the device's memory as the driver reports them"""
    hip, _ = load_native()
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if hip.h10x_device_mem_info(int(device), ctypes.byref(f), ctypes.byref(t)):
        raise Hash10xError("h10x_device_mem_info failed")
    return f.value, t.value


def warm(device=0):
    """load the library's device code on `device` ahead of its first use (h10x_warm): 0 on success"""
    return load_native()[0].h10x_warm(int(device))


def alloc_stats():
    """(blocks, bytes) this process has obtained from hipMalloc so far (h10x_alloc_stats)"""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    load_native()[0].h10x_alloc_stats(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def build_id():
    """what libh10x_hip.so was built from: "src:<sha256 over its sources and compile flags, 16 hex>" (embedded at build time by csrc/Makefile)"""
    return load_native()[0].h10x_build_id().decode()


class DeviceRecords:
    """A sorted .fqb image resident in HBM (hipMalloc through the library, no torch involved)."""

    def __init__(self, records, device=0, _words=0):
        hip = load_native()[0]
        r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
        self.n_records, self.device, self._hip = r.size // 30, device, hip
        nbytes = max(r.nbytes, 4 * int(_words))                 # _words: room for that many words, contents undefined (an output buffer)
        self.ptr = hip.h10x_device_malloc(device, nbytes)
        if not self.ptr:
            raise Hash10xError("hipMalloc of %d bytes failed on device %d" % (nbytes, device))
        if r.nbytes and hip.h10x_device_upload(device, self.ptr, r.ctypes.data, r.nbytes):
            raise Hash10xError("upload to device %d failed" % device)

    def download(self):
        """the records as an (n_records, 30) uint32 array"""
        out = np.zeros(max(self.n_records * 30, 1), dtype=np.uint32)
        if self.n_records and self._hip.h10x_device_download(self.device, out.ctypes.data, self.ptr, self.n_records * 120):
            raise Hash10xError("download from device %d failed" % self.device)
        return out[:self.n_records * 30].reshape(-1, 30)

    def free(self):
        if getattr(self, "ptr", None):
            self._hip.h10x_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def synchronize(device=0):
    load_native()[0].h10x_device_synchronize(device)


class Comm:
    """Communicator of the sharded path: RCCL (one process per GPU) or in-process (N ranks = N threads)."""

    def __init__(self, handle, rank, size):
        self.handle, self.rank, self.size = handle, rank, size

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        if load_native()[0].h10x_comm_unique_id(buf):
            raise Hash10xError("ncclGetUniqueId failed")
        return buf.raw

    @staticmethod
    def rccl(rank, size, unique_id, device):
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if load_native()[0].h10x_comm_create_rccl(ctypes.byref(h), rank, size, unique_id, device, err, 512):
            raise Hash10xError(err.value.decode())
        return Comm(h, rank, size)

    @staticmethod
    def socket(rank, size, addr="127.0.0.1", base_port=29700):
        """One process per rank, host-staged over TCP: the multi-process path where RCCL cannot run (ranks sharing a GPU)."""
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if load_native()[0].h10x_comm_create_socket(ctypes.byref(h), rank, size, addr.encode(), int(base_port), err, 512):
            raise Hash10xError(err.value.decode())
        return Comm(h, rank, size)

    @staticmethod
    def local(size):
        arr = (ctypes.c_void_p * size)()
        load_native()[0].h10x_comm_create_local(arr, size)
        return [Comm(ctypes.c_void_p(arr[i]), i, size) for i in range(size)]

    def serialize(self, on=True):
        """in-process communicators: the ranks take turns on the device they share (h10x_comm_local_serialize); bracket every command with turn_begin / turn_end"""
        if load_native()[0].h10x_comm_local_serialize(self.handle, 1 if on else 0):
            raise Hash10xError("not an in-process communicator")

    def turn_begin(self):
        load_native()[0].h10x_comm_turn_begin(self.handle)

    def turn_end(self, device=0):
        load_native()[0].h10x_comm_turn_end(self.handle, int(device))

    def destroy(self):
        if self.handle:
            load_native()[0].h10x_comm_destroy(self.handle)
            self.handle = None


def partition(records, parts):
    """Record index cuts of contiguous barcode-range shards (h10x_host_partition)."""
    r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
    cut = (ctypes.c_uint64 * (parts + 1))()
    if load_native()[1].h10x_host_partition(r.ctypes.data, r.size // 30, parts, cut):
        raise Hash10xError("partition failed")
    return [int(x) for x in cut]


def read_molecule_map(path):
    """A .mol file of --moleculeMap: (mol, slot, info), as Hash10x.molecule_map() returns them."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 32 or data[:4] != b"10XM":
        raise Hash10xError("%s is not a molecule map (magic 10XM)" % path)
    version = int.from_bytes(data[4:8], "little")
    if version != 1:
        raise Hash10xError("%s: molecule map version %d, this reader knows 1" % (path, version))
    info = {"nRecords": int.from_bytes(data[8:16], "little"), "nClustered": int.from_bytes(data[24:32], "little"),
            "nBlocks": int.from_bytes(data[16:20], "little"), "nMolecules": int.from_bytes(data[20:24], "little")}
    if len(data) != 32 + 8 * info["nRecords"]:
        raise Hash10xError("%s: %d bytes, %d records need %d" % (path, len(data), info["nRecords"], 32 + 8 * info["nRecords"]))
    pairs = np.frombuffer(data, dtype="<u4", offset=32).reshape(-1, 2)
    return pairs[:, 0].copy(), pairs[:, 1].copy(), info


def read_split_index(path):
    """The .idx file beside a split .fqb: (start, nBlocks, nMolecules); records [start[m], start[m + 1]) are block m's."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 16 or data[:4] != b"10XS":
        raise Hash10xError("%s is not a split index (magic 10XS)" % path)
    version = int.from_bytes(data[4:8], "little")
    if version != 1:
        raise Hash10xError("%s: split index version %d, this reader knows 1" % (path, version))
    n_blocks, n_mol = int.from_bytes(data[8:12], "little"), int.from_bytes(data[12:16], "little")
    if len(data) != 16 + 8 * (n_blocks + n_mol + 1):
        raise Hash10xError("%s: %d bytes, %d starts need %d" % (path, len(data), n_blocks + n_mol + 1, 16 + 8 * (n_blocks + n_mol + 1)))
    return np.frombuffer(data, dtype="<u8", offset=16).copy(), n_blocks, n_mol


class _MolInfo(ctypes.Structure):
    _fields_ = [("nRecords", ctypes.c_uint64), ("nClustered", ctypes.c_uint64), ("nBlocks", ctypes.c_uint32), ("nMolecules", ctypes.c_uint32)]


class Hash10x:
    """One hash10x session on one GPU (the reference's process-global state, hash10x.c:85-104)."""

    def __init__(self, k=21, w=31, r=17, B=28, device=0):
        self._hip, self._host = load_native()
        self._s = self._host.h10x_session_new()
        if not self._s:
            raise Hash10xError("out of memory")
        for n, v in (("k", k), ("w", w), ("r", r), ("B", B), ("device", device)):
            self._host.h10x_session_set(self._s, n.encode(), int(v))
        self._timing = False

    def close(self):
        if getattr(self, "_s", None):
            self._host.h10x_session_free(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise Hash10xError(self._host.h10x_session_error(self._s).decode())

    def _ctx(self):
        return self._host.h10x_session_ctx(self._s)

    def _after_init(self):
        ctx = self._ctx()
        if ctx and self._timing:
            self._hip.h10x_timing_enable(ctx, 1)

    # ---- commands ------------------------------------------------------------------------------
    def _pre(self, N, chunk):
        self._host.h10x_session_set(self._s, b"N", int(N))
        self._host.h10x_session_set(self._s, b"c", int(chunk))

    def read_fqb(self, records, N=0, chunk=100000):
        """--readFQB on an in-memory image of the sorted .fqb file (30 uint32 per read pair)."""
        r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
        if r.size % 30:
            r = r[: r.size - r.size % 30]
        self._pre(N, chunk)
        self._chk(self._host.h10x_session_readFQB_mem(self._s, r.ctypes.data, r.size // 30))
        self._after_init()

    def ingest_fqb(self, chunks, N=0, chunk=100000, reserve=0):
        """--readFQB through the streaming C ABI (h10x_ingest_fqb): `chunks` = an iterable of record arrays (any sizes), appended on the
        device one by one; the last call closes the ingest. The session's parameters are latched as for read_fqb."""
        self._pre(N, chunk)
        self._chk(self._host.h10x_session_begin(self._s))
        if self._hip.h10x_set_option(self._ctx(), b"chunk_size", int(chunk)):
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())
        if reserve:
            self._chk_ctx(self._hip.h10x_ingest_reserve(self._ctx(), int(reserve)))
        fed, cut = 0, False                                  # -N n: the first n records, and then no end-of-file pass (hash10x.c:202-208), as read_fqb does it
        for part in chunks:
            r = np.ascontiguousarray(part, dtype=np.uint32).reshape(-1)
            take = r.size // 30
            if N > 0 and fed + take >= N:
                take, cut = N - fed, True
            if take:
                self._chk_ctx(self._hip.h10x_ingest_fqb(self._ctx(), r.ctypes.data, take, 0))
            fed += take
            if cut:
                break
        if self._hip.h10x_set_option(self._ctx(), b"chunk_eof_pass", 0 if cut else 1):
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())
        self._chk_ctx(self._hip.h10x_ingest_fqb(self._ctx(), None, 0, 1))
        self._chk(self._host.h10x_session_after_read(self._s))
        self._after_init()

    def read_fqb_file(self, path, N=0, chunk=100000):
        self._pre(N, chunk)
        self._chk(self._host.h10x_session_readFQB(self._s, os.fsencode(path)))
        self._after_init()

    def read_fqb_device(self, dev_ptr, n_records, N=0):
        """--readFQB with the records already resident in HBM (dev_ptr = device address)."""
        self._pre(N, 100000)
        self._chk(self._host.h10x_session_readFQB_dev(self._s, ctypes.c_void_p(dev_ptr), int(n_records)))
        self._after_init()

    def shard_read_fqb(self, comm, shard_records):
        """Sharded --readFQB: this rank's barcode range (host image); collective over comm."""
        r = np.ascontiguousarray(shard_records, dtype=np.uint32).reshape(-1)
        self._chk(self._host.h10x_session_shardReadFQB_mem(self._s, comm.handle, r.ctypes.data, r.size // 30))
        self._after_init()

    def shard_read_fqb_device(self, comm, dev_ptr, n_records):
        self._chk(self._host.h10x_session_shardReadFQB_dev(self._s, comm.handle, ctypes.c_void_p(dev_ptr), int(n_records)))
        self._after_init()

    def shard_read_hash(self, comm, path):
        """Sharded --readHash (collective): every rank loads the replicated tables and its own cut of the file's blocks."""
        self._chk(self._host.h10x_session_shardReadHash(self._s, comm.handle, os.fsencode(path)))
        self._after_init()

    def shard_gather(self):
        """Collective: rank 0 ends up with the whole state (then write_hash there)."""
        self._chk(self._host.h10x_session_shardGather(self._s))

    def shard_read_fqb_file(self, comm, path, first, n, chunk=100000):
        """Sharded --readFQB from a file: this rank's records [first, first + n), streamed into HBM; the reference's chunk
        semantics (-c) are applied over the whole file."""
        self._host.h10x_session_set(self._s, b"c", int(chunk))
        self._chk(self._host.h10x_session_shardReadFQB_file(self._s, comm.handle, os.fsencode(path), int(first), int(n)))
        self._after_init()

    def _chk_ctx(self, rc):
        if rc != 0:
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())

    def shard_barrier(self):
        self._chk_ctx(self._hip.h10x_shard_barrier(self._ctx()))

    def shard_allreduce_max(self, value):
        v = ctypes.c_double(value)
        self._chk_ctx(self._hip.h10x_shard_allreduce_max(self._ctx(), ctypes.byref(v)))
        return v.value

    def shard_allreduce_sum_u64(self, values):
        """sums (mod 2^64) over the ranks of a small list of integers; the identity on an unsharded context"""
        v = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in values], dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_shard_allreduce_sum_u64(self._ctx(), v.ctypes.data, len(v)))
        return [int(x) for x in v]

    def shard_allreduce_max_u64(self, values):
        """maxima over the ranks of a small list of integers; the identity on an unsharded context"""
        v = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in values], dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_shard_allreduce_max_u64(self._ctx(), v.ctypes.data, len(v)))
        return [int(x) for x in v]

    def export_slice(self, table, first, count):
        """elements [first, first + count) of one table of THIS rank (h10x_export_slice; works on shards): 3 = blocks (32 B), 4 = ClusterHash (8 B)"""
        width = {0: 4, 1: 8, 2: 4, 3: 32, 4: 8, 5: 4}[table]
        out = np.zeros(max(int(count), 1) * width, dtype=np.uint8)
        self._chk_ctx(self._hip.h10x_export_slice(self._ctx(), table, int(first), int(count), out.ctypes.data))
        return out[: int(count) * width]

    def shard_info(self):
        z = _ShardInfo()
        self._chk_ctx(self._hip.h10x_shard_info(self._ctx(), ctypes.byref(z)))
        return {n: int(getattr(z, n)) for n, _ in _ShardInfo._fields_}

    def shard_segments(self):
        n = self.shard_info()["nSegs"]
        arr = (_ShardSeg * (n + 1))()
        self._chk_ctx(self._hip.h10x_shard_segments(self._ctx(), arr, n + 1))
        return [{f: int(getattr(arr[i], f)) for f, _ in _ShardSeg._fields_} for i in range(n)]

    # ---- text commands: `out` = a path (this rank prints there) or None (take part only) ----------------
    def _with_file(self, out, fn):
        libc = ctypes.CDLL(None)
        libc.fopen.restype = ctypes.c_void_p
        libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        libc.fclose.argtypes = [ctypes.c_void_p]
        f = libc.fopen(os.fsencode(out), b"a") if out else None
        try:
            self._chk(fn(ctypes.c_void_p(f) if f else None))
        finally:
            if f:
                libc.fclose(f)

    def crib_build(self, fa1, fa2, out=None, tables=False):
        self._with_file(out, lambda f: self._host.h10x_session_cribBuild(self._s, os.fsencode(fa1), os.fsencode(fa2), f, 1 if tables else 0))

    def crib_genomes(self, codes_a, codes_b, piece=60000000):
        """--cribBuild through the C ABI without FASTA files (h10x_crib_genome x 2 + h10x_crib_finish, hash10x.c:426-494): each haplotype as base codes 0..3, cut into
        sequences of `piece` bases as the truth FASTAs of gen_fqb are. Returns [(known, unknown) moshes of genome 1, of genome 2]."""
        out = []
        for which, codes in enumerate((codes_a, codes_b)):
            codes = np.ascontiguousarray(codes, dtype=np.uint8)
            starts = np.arange(0, codes.size + piece, piece, dtype=np.uint64)
            starts[-1] = codes.size
            if starts.size >= 2 and starts[-2] >= codes.size:
                starts = starts[:-1]; starts[-1] = codes.size
            known, unknown = ctypes.c_uint64(0), ctypes.c_uint64(0)
            self._chk_ctx(self._hip.h10x_crib_genome(self._ctx(), codes.ctypes.data, starts.ctypes.data, int(starts.size - 1), which, ctypes.byref(known), ctypes.byref(unknown)))
            out.append((known.value, unknown.value))
        self._chk_ctx(self._hip.h10x_crib_finish(self._ctx()))
        return out

    def crib_sequences(self, seqs_a, seqs_b):
        """crib_genomes with the sequence starts of the caller: each haplotype as a list of sequences (text or codes 0..3, as seq_hashes takes them; a sequence
        may be shorter than k, or empty). Returns [(known, unknown) moshes of genome 1, of genome 2]."""
        out = []
        for which, seqs in enumerate((seqs_a, seqs_b)):
            codes, starts = self._flatten_seqs(seqs)
            known, unknown = ctypes.c_uint64(0), ctypes.c_uint64(0)
            self._chk_ctx(self._hip.h10x_crib_genome(self._seq_ctx("crib_sequences"), codes.ctypes.data, starts.ctypes.data, int(starts.size - 1), which, ctypes.byref(known), ctypes.byref(unknown)))
            out.append((known.value, unknown.value))
        self._chk_ctx(self._hip.h10x_crib_finish(self._ctx()))
        return out

    def crib_export(self):
        """the crib as h10x_crib_export gives it: chr (int16), pos (uint16) and type (uint8) per hash index, the four depth histograms hist[0..3] = err, het, hom,
        mul (uint32, one row each, as long as the deepest hash needs) and arrayMax[4] = one past the deepest hash of each class (0: none). Fails before a crib."""
        dim, amax = ctypes.c_uint32(0), np.zeros(4, dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_crib_sizes(self._seq_ctx("crib_export"), ctypes.byref(dim), amax.ctypes.data))
        n = self.sizes()["hashNumber"]
        chrom, pos, typ = np.zeros(n, dtype=np.int16), np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint8)
        hist = np.zeros((4, dim.value), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_crib_export(self._ctx(), chrom.ctypes.data, pos.ctypes.data, typ.ctypes.data, hist.ctypes.data))
        return {"chr": chrom, "pos": pos, "type": typ, "hist": hist, "arrayMax": amax}

    def cluster_report_raw(self, first, n):
        """h10x_cluster_report over blocks [first, first + n) of THIS rank: (one record per block: nGood, nClusHash, nClusRead; one per sub-cluster, the blocks'
        min(nSubCluster, 255) records one after the other: n, nRead, nt[5], nBad, chr, pMin, pMax, nOtherListed, other[10])."""
        brep = np.zeros(max(int(n), 1), dtype=_BLOCK_REP)
        crep = np.zeros(255 * int(n) + 1, dtype=_CLUSTER_REP)
        ncl = ctypes.c_uint64(0)
        self._chk_ctx(self._hip.h10x_cluster_report(self._seq_ctx("cluster_report_raw"), int(first), int(n), brep.ctypes.data, crep.ctypes.data, ctypes.c_uint64(crep.size), ctypes.byref(ncl)))
        return brep[: int(n)], crep[: ncl.value]

    def crib_summary_raw(self):
        """h10x_crib_summary: (counts[12] = records per crib type in base blocks, in blocks --clusterSplit made, base blocks without block 0, split blocks;
        seen_base, seen_cluster = per hash index whether a block of that kind holds it, as bool arrays)."""
        n = self.sizes()["hashNumber"]
        words = (n + 31) // 32
        counts, seen = np.zeros(12, dtype=np.uint64), np.zeros((2, words), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_crib_summary(self._seq_ctx("crib_summary_raw"), counts.ctypes.data, seen[0].ctypes.data, seen[1].ctypes.data))
        bits = [((seen[i][np.arange(n) >> 5] >> (np.arange(n, dtype=np.uint32) & 31)) & 1).astype(bool) for i in range(2)]
        return counts, bits[0], bits[1]

    def crib_words(self, first, count):
        """h10x_crib_words: records [first, first + count) of this rank's ClusterHash table as cribSummary's words (bit 31 split block, 28-30 crib type, 0-27 hash index)."""
        out = np.zeros(max(int(count), 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_crib_words(self._seq_ctx("crib_words"), int(first), int(count), out.ctypes.data))
        return out[: int(count)]

    def cluster_report_figures(self, first_block=1, n_blocks=None, run=1 << 16):
        """codeClusterReport's figures (hash10x.c:870-952) reduced over blocks [first, first + n) of THIS rank without forming the text: the sums tests/orc.report_digest reads
        off the reference's CODE_CLUSTER lines — clusters printed (n > 0), those without an OTHER list, those with a location, the sums of their spans, reads and hashes —
        plus the sum of nGoodHash and of nClusHash over the blocks."""
        z = self.sizes()
        if n_blocks is None:
            n_blocks = z["nBlocks"] - first_block
        tot = dict(clusters=0, clusters_without_OTHER=0, clusters_located=0, sum_span=0, sum_reads=0, sum_hashes=0, sum_nGood=0, sum_nClusHash=0)
        brep = np.zeros(run, dtype=_BLOCK_REP)
        crep = np.zeros(run * 16, dtype=_CLUSTER_REP)
        at = first_block
        while at < first_block + n_blocks:
            nb = min(run, first_block + n_blocks - at)
            ncl = ctypes.c_uint64(0)
            rc = self._hip.h10x_cluster_report(self._ctx(), int(at), int(nb), brep.ctypes.data, crep.ctypes.data, ctypes.c_uint64(crep.size), ctypes.byref(ncl))
            if rc and ncl.value > crep.size:                 # more clusters than the buffer holds: the call says how many
                crep = np.zeros(int(ncl.value) + 1024, dtype=_CLUSTER_REP)
                rc = self._hip.h10x_cluster_report(self._ctx(), int(at), int(nb), brep.ctypes.data, crep.ctypes.data, ctypes.c_uint64(crep.size), ctypes.byref(ncl))
            self._chk_ctx(rc)
            c = crep[: ncl.value]
            c = c[c["n"] > 0]
            loc = c["chr"] != 0
            tot["clusters"] += int(c.size); tot["clusters_without_OTHER"] += int((c["nBad"] == 0).sum()); tot["clusters_located"] += int(loc.sum())
            tot["sum_span"] += int((c["pMax"][loc].astype(np.int64) - c["pMin"][loc].astype(np.int64) + 1).sum())
            tot["sum_reads"] += int(c["nRead"].sum(dtype=np.int64)); tot["sum_hashes"] += int(c["n"].sum(dtype=np.int64))
            tot["sum_nGood"] += int(brep["nGood"][:nb].sum(dtype=np.int64)); tot["sum_nClusHash"] += int(brep["nClusHash"][:nb].sum(dtype=np.int64))
            at += nb
        return tot

    def cluster_report(self, code_min, code_max, out=None):
        self._with_file(out, lambda f: self._host.h10x_session_clusterReport(self._s, int(code_min), int(code_max), f))

    def crib_summary(self, out=None):
        self._with_file(out, lambda f: self._host.h10x_session_cribSummary(self._s, f))

    def hash_stats(self, out=None):
        self._with_file(out, lambda f: self._host.h10x_session_hashStats(self._s, f))

    def code_stats(self, out=None):
        self._with_file(out, lambda f: self._host.h10x_session_codeStats(self._s, f))

    def read_hash(self, path):
        self._chk(self._host.h10x_session_readHash(self._s, os.fsencode(path)))
        self._after_init()

    def write_hash(self, path):
        self._chk(self._host.h10x_session_writeHash(self._s, os.fsencode(path)))

    def depth_range(self, lo, hi):
        self._chk(self._host.h10x_session_hashDepthRange(self._s, int(lo), int(hi)))

    def cluster(self, code_min=1, code_max=0, threshold=5):
        self._host.h10x_session_set(self._s, b"ct", int(threshold))
        self._chk(self._host.h10x_session_cluster(self._s, int(code_min), int(code_max)))

    def cluster_split(self):
        self._chk(self._host.h10x_session_clusterSplit(self._s))

    # ---- measurement / test hooks ---------------------------------------------------------------
    def enable_timing(self, on=True):
        self._timing = bool(on)
        self._host.h10x_session_set(self._s, b"timing", 1 if on else 0)
        if self._ctx():
            self._hip.h10x_timing_enable(self._ctx(), 1 if on else 0)

    def set_option(self, name, value):
        """Test knobs (e.g. stage_a_max_slots) forwarded to the context of the next read_fqb/read_hash."""
        if self._host.h10x_session_set(self._s, name.encode(), int(value)):
            raise Hash10xError(self._host.h10x_session_error(self._s).decode())

    def timings(self):
        ctx = self._ctx()
        out = {}
        if not ctx:
            return out
        for i in range(self._hip.h10x_timing_count(ctx)):
            ms, n = ctypes.c_double(), ctypes.c_uint64()
            self._hip.h10x_timing_get(ctx, i, ctypes.byref(ms), ctypes.byref(n))
            out[self._hip.h10x_timing_name(ctx, i).decode()] = (ms.value, n.value)
        return out

    def stage_waits(self):
        """per stage timer: the ms of it spent inside exchanges (sharded contexts)"""
        out = {}
        for i in range(self._hip.h10x_timing_count(self._ctx())):
            ms = ctypes.c_double(0)
            self._hip.h10x_timing_wait_get(self._ctx(), i, ctypes.byref(ms))
            if ms.value:
                out[self._hip.h10x_timing_name(self._ctx(), i).decode()] = ms.value
        return out

    def exchanges(self):
        """per kind of collective of the sharded path: calls, bytes to / from other ranks, bytes the busiest peer got, ms (waits included) and the part of it inside stage timers"""
        out = {}
        for i in range(self._hip.h10x_exchange_count()):
            v = [ctypes.c_uint64(0) for _ in range(4)]; ms, ms_in = ctypes.c_double(0), ctypes.c_double(0)
            self._hip.h10x_exchange_get(self._ctx(), i, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(v[3]), ctypes.byref(ms), ctypes.byref(ms_in))
            if v[0].value:
                b = self._hip.h10x_exchange_beside(self._ctx(), i)
                out[self._hip.h10x_exchange_name(i).decode()] = {"calls": v[0].value, "bytes_out": v[1].value, "bytes_in": v[2].value, "max_peer_out": v[3].value, "ms": ms.value, "ms_in_stages": ms_in.value,
                                                                 "beside": self._hip.h10x_timing_name(self._ctx(), b).decode() if b >= 0 else None}
        return out

    def reset_timings(self):
        if self._ctx():
            self._hip.h10x_timing_reset(self._ctx())

    def counters(self):
        c = _Counters()
        if self._ctx():
            self._hip.h10x_get_counters(self._ctx(), ctypes.byref(c))
        out = {n: int(getattr(c, n)) for n, _ in _Counters._fields_ if n not in ("cluster_phase_ticks", "cluster_class_counts", "cluster_main", "list_words")}
        out["list_words"] = [int(x) for x in c.list_words]
        out["cluster_main"] = [int(x) for x in c.cluster_main]
        out["cluster_class_counts"] = [int(x) for x in c.cluster_class_counts]
        out["cluster_phase_ticks"] = [int(x) for x in c.cluster_phase_ticks]
        n = ctypes.c_uint64(0)
        if self._ctx():
            self._hip.h10x_get_scan_retries(self._ctx(), ctypes.byref(n))
        out["scan_retries"] = n.value                           # seq_hashes / seq_blocks / seq_links batches scanned a second time: the mosh list overflowed its estimate
        return out

    def sizes(self):
        z = _Sizes()
        if not self._ctx() or self._hip.h10x_get_sizes(self._ctx(), ctypes.byref(z)):
            raise Hash10xError("no hash state loaded")
        return {n: int(getattr(z, n)) for n, _ in _Sizes._fields_ if n != "reserved"}

    def export_blocks(self):
        """nBlocks ClusterBlock records as a structured array (for tests/bench sanity checks)."""
        z = self.sizes()
        dt = np.dtype([("nRead", "<u4"), ("nHash", "<u4"), ("nSubCluster", "<u4"), ("clusterParent", "<u4"),
                       ("ptr", "<u8"), ("pointToMin", "<f8")])
        b = np.zeros(z["nBlocks"], dtype=dt)
        if self._hip.h10x_export(self._ctx(), None, None, None, b.ctypes.data, None):
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())
        return b

    def export_clushash(self):
        """All ClusterHash records (blocks 1.. concatenated) as a structured array."""
        z = self.sizes()
        dt = np.dtype([("hash", "<u4"), ("read", "<u2"), ("subCluster", "u1"), ("flags", "u1")])
        ch = np.zeros(max(z["nClusHash"], 1), dtype=dt)
        if self._hip.h10x_export(self._ctx(), None, None, None, None, ch.ctypes.data):
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())
        return ch[: z["nClusHash"]]

    def export_depth(self):
        """hashDepth[0 .. hashNumber) as uint32."""
        z = self.sizes()
        d = np.zeros(z["hashNumber"], dtype=np.uint32)
        if self._hip.h10x_export(self._ctx(), None, None, d.ctypes.data, None, None):
            raise Hash10xError(self._hip.h10x_last_error(self._ctx()).decode())
        return d

    # ---- neighbour census (h10x_neighbours / _max / _hist: hashNeighbours / countHashNeighbours, hash10x.c:541-586) ----
    def neighbours(self, x):
        """N(x) ascending in h: (hash, count = shared blocks, firstCode = lowest barcode of h) as three uint32 arrays."""
        n = ctypes.c_uint64(0)
        self._chk_ctx(self._hip.h10x_neighbours(self._ctx(), int(x), None, None, None, 0, ctypes.byref(n)))
        m = n.value
        h, c, f = (np.zeros(max(m, 1), dtype=np.uint32) for _ in range(3))
        self._chk_ctx(self._hip.h10x_neighbours(self._ctx(), int(x), h.ctypes.data, c.ctypes.data, f.ctypes.data, m, ctypes.byref(n)))
        return h[:m], c[:m], f[:m]

    def neighbour_max(self, xs):
        """per query: (maxKey = max of (count mod 2^16) << 32 | h, |N(x)|) as uint64 / uint32 arrays."""
        q = np.ascontiguousarray(xs, dtype=np.uint32).reshape(-1)
        mk = np.zeros(max(q.size, 1), dtype=np.uint64); nn = np.zeros(max(q.size, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_neighbour_max(self._ctx(), q.ctypes.data, q.size, mk.ctypes.data, nn.ctypes.data))
        return mk[:q.size], nn[:q.size]

    def neighbour_hist(self, xs, depth=None):
        """per query the histogram H_x[0 .. depth(x)] of shared-block counts: a list of uint32 arrays."""
        q = np.ascontiguousarray(xs, dtype=np.uint32).reshape(-1)
        d = self.export_depth() if depth is None else depth
        off = np.zeros(q.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum(d[q].astype(np.uint64) + 1)
        hist = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_neighbour_hist(self._ctx(), q.ctypes.data, q.size, off.ctypes.data, hist.ctypes.data))
        return [hist[int(off[i]):int(off[i + 1])] for i in range(q.size)]

    def neighbour_stats(self, reset=True):
        """census work since the last reset: records gathered, in-range keys sorted, batches, windows"""
        v = np.zeros(4, dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_neighbour_stats(self._ctx(), v.ctypes.data, 1 if reset else 0))
        return dict(zip(("gathered", "sorted", "batches", "windows"), (int(a) for a in v)))

    # ---- barcode census and --codeExplore (h10x_code_share / _explore / _crib_counts: codeExplore, hash10x.c:1351-1470) ----
    def code_share(self, codes):
        """per query barcode: (barcode, count = countShare, firstRank, firstHash) of the barcodes sharing its good hashes'
        lists, ascending in barcode — a list of dicts of uint32 arrays."""
        q = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1)
        off = np.zeros(q.size + 1, dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_code_share(self._ctx(), q.ctypes.data, q.size, off.ctypes.data, None, None, None, None, 0))
        m = int(off[-1])
        cols = [np.zeros(max(m, 1), dtype=np.uint32) for _ in range(4)]
        self._chk_ctx(self._hip.h10x_code_share(self._ctx(), q.ctypes.data, q.size, off.ctypes.data, *(c.ctypes.data for c in cols), m))
        names = ("barcode", "count", "firstRank", "firstHash")
        return [{n: c[int(off[i]):int(off[i + 1])] for n, c in zip(names, cols)} for i in range(q.size)]

    def code_explore(self, code, threshold=5):
        """codeExplore's re-clustering of one barcode (state change only, no text): nHash, nGood, clustered, raw, merged, abandoned,
        histMax (the largest countShare), nShare (barcodes sharing)."""
        rep = np.zeros(8, dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_code_explore(self._ctx(), int(code), int(threshold), rep.ctypes.data))
        return dict(zip(("nHash", "nGood", "clustered", "raw", "merged", "abandoned", "histMax", "nShare"), (int(v) for v in rep)))

    def code_crib_counts(self, codes):
        """per barcode the CRIB_HTA and CRIB_HTB records of its block: an (n, 2) uint32 array (needs a crib)."""
        q = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1)
        out = np.zeros((max(q.size, 1), 2), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_code_crib_counts(self._ctx(), q.ctypes.data, q.size, out.ctypes.data))
        return out[:q.size]

    # ---- barcode census and whitelist correction of unsorted records (h10x_census_* / h10x_whitelist_set / h10x_fix_fqb: fq2b.c:71-104) ----
    def _need_ctx(self):
        if not self._ctx():
            self._chk(self._host.h10x_session_begin(self._s))
            self._after_init()
        return self._ctx()

    def code_census(self, records, thresh):
        """Census of the barcodes (record word 0) of an unsorted .fqb image, a host array or DeviceRecords: (codes, counts, good) =
        the distinct barcodes ascending by packed word, how often each occurs, and those that occur at least `thresh` times.
        The good barcodes become the session's whitelist, in ascending order."""
        ctx = self._need_ctx()
        if isinstance(records, DeviceRecords):
            self._chk_ctx(self._hip.h10x_census_begin(ctx, records.n_records))
            self._chk_ctx(self._hip.h10x_census_add_device(ctx, records.ptr, records.n_records))
        else:
            r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
            if r.size % 30:
                raise Hash10xError("records: %d words are no multiple of the 30-word record" % r.size)
            self._chk_ctx(self._hip.h10x_census_begin(ctx, r.size // 30))
            self._chk_ctx(self._hip.h10x_census_add(ctx, r.ctypes.data, r.size // 30))
        z = np.zeros(4, dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_census_close(ctx, int(thresh), z.ctypes.data))
        d, g = int(z[1]), int(z[2])
        codes, counts, good = np.zeros(max(d, 1), dtype=np.uint32), np.zeros(max(d, 1), dtype=np.uint32), np.zeros(max(g, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_census_export(ctx, 0, codes.ctypes.data, counts.ctypes.data, d))
        self._chk_ctx(self._hip.h10x_census_export(ctx, 1, good.ctypes.data, None, g))
        return codes[:d], counts[:d], good[:g]

    def set_whitelist(self, codes):
        """The whitelist from packed barcodes in line order (read10xWhitelist, fq2b.c:71-94): a repeated code keeps its latest line."""
        c = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1)
        self._chk_ctx(self._hip.h10x_whitelist_set(self._need_ctx(), c.ctypes.data, c.size))

    def fix_fqb(self, records):
        """What fq2b -10x does to the reads, on records (a host array or DeviceRecords): (records_out, stats). Records without a
        whitelist barcode within one substitution are dropped, the others get the candidate of the latest whitelist line as
        word 0 and keep their order. records_out is an (n_kept, 30) uint32 array, or for DeviceRecords a DeviceRecords holding
        n_records = n_kept; stats = {"dropped", "corrected", "correctedAt": 16 counts by base position}."""
        ctx = self._need_ctx()
        st, kept = np.zeros(18, dtype=np.uint64), ctypes.c_uint64(0)
        if isinstance(records, DeviceRecords):
            out = DeviceRecords(np.zeros(0, dtype=np.uint32), records.device, _words=records.n_records * 30)
            self._chk_ctx(self._hip.h10x_fix_fqb_device(ctx, records.ptr, records.n_records, out.ptr, ctypes.byref(kept), st.ctypes.data))
            out.n_records = kept.value
        else:
            r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
            if r.size % 30:
                raise Hash10xError("records: %d words are no multiple of the 30-word record" % r.size)
            buf = np.zeros(max(r.size, 30), dtype=np.uint32)
            self._chk_ctx(self._hip.h10x_fix_fqb(ctx, r.ctypes.data, r.size // 30, buf.ctypes.data, ctypes.byref(kept), st.ctypes.data))
            out = buf[:kept.value * 30].reshape(-1, 30)
        return out, {"dropped": int(st[0]), "corrected": int(st[1]), "correctedAt": [int(v) for v in st[2:]]}

    # ---- the molecule of every read pair (h10x_molecule_map / h10x_split_fqb: hash10x.c:897-920, 979-989 per record) ----
    def molecule_map(self):
        """After cluster(), before cluster_split(): (mol, slot, info). Record i of the sorted file the state was read from belongs to
        block mol[i] of the state cluster_split() would make — a new block (mol >= info["nBlocks"]) for a clustered read pair, its
        own barcode otherwise — as that block's read number slot[i]. info = {"nRecords", "nClustered", "nBlocks", "nMolecules"}."""
        ctx = self._ctx()
        if not ctx:
            raise Hash10xError("moleculeMap: no hash state loaded: use readFQB or readHash first")
        z = _MolInfo()
        self._chk_ctx(self._hip.h10x_molecule_map(ctx, None, None, 0, ctypes.byref(z)))
        n = int(z.nRecords)
        mol, slot = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_molecule_map(ctx, mol.ctypes.data, slot.ctypes.data, n, ctypes.byref(z)))
        return mol[:n], slot[:n], {k: int(getattr(z, k)) for k, _ in _MolInfo._fields_}

    def split_fqb(self, records):
        """The records of the sorted file the state was read from (a host array or DeviceRecords, exactly nRecords of them) in split
        order: (records_out, start). records_out[start[m]: start[m + 1]] are the read pairs of block m after cluster_split(), a
        molecule's in slot order; records_out is an (n, 30) uint32 array, or a DeviceRecords for DeviceRecords."""
        ctx = self._ctx()
        if not ctx:
            raise Hash10xError("splitFQB: no hash state loaded: use readFQB or readHash first")
        z = _MolInfo()
        self._chk_ctx(self._hip.h10x_molecule_map(ctx, None, None, 0, ctypes.byref(z)))
        start = np.zeros(int(z.nBlocks) + int(z.nMolecules) + 1, dtype=np.uint64)
        if isinstance(records, DeviceRecords):
            out = DeviceRecords(np.zeros(0, dtype=np.uint32), records.device, _words=records.n_records * 30)
            try:
                self._chk_ctx(self._hip.h10x_split_fqb_device(ctx, records.ptr, records.n_records, out.ptr, start.ctypes.data, start.size))
            except Hash10xError:
                out.free()
                raise
            out.n_records = records.n_records
        else:
            r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1)
            if r.size % 30:
                raise Hash10xError("records: %d words are no multiple of the 30-word record" % r.size)
            buf = np.zeros(max(r.size, 30), dtype=np.uint32)
            self._chk_ctx(self._hip.h10x_split_fqb(ctx, r.ctypes.data, r.size // 30, buf.ctypes.data, start.ctypes.data, start.size))
            out = buf[:r.size].reshape(-1, 30)
        return out, start

    # ---- the share graph (h10x_share_graph_run / _get): every block's sharing blocks at a threshold, one census ----
    def share_graph(self, min_share, code_min=1, code_max=0):
        """The blocks sharing at least min_share good hashes with each block of [code_min, code_max) (code_max = 0: nBlocks), in CSR
        form: (offsets uint64[code_max - code_min + 1], block uint32[], count uint32[]); the row of block code_min + i is
        [offsets[i], offsets[i + 1]), ascending in block, count = countShare as code_share gives it. The figures of the run (rows,
        listEntries, entriesRead, maxCount, batches, windows, codeMin, codeMax, nBlocks) are kept in self.share_graph_info."""
        ctx = self._ctx()
        if not ctx:
            raise Hash10xError("shareGraph: no hash state loaded: use readFQB or readHash first")
        z = np.zeros(1, dtype=_SHARE_GRAPH_INFO)
        self._chk_ctx(self._hip.h10x_share_graph_run(ctx, int(min_share), int(code_min), int(code_max), z.ctypes.data))
        self.share_graph_info = {n: int(z[n][0]) for n in _SHARE_GRAPH_INFO.names}
        m = self.share_graph_info["rows"]
        off = np.zeros(self.share_graph_info["codeMax"] - self.share_graph_info["codeMin"] + 1, dtype=np.uint64)
        blk, cnt = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_share_graph_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, m))
        return off, blk[:m], cnt[:m]

    def write_share_graph(self, min_share, path, out=None):
        """--shareGraph <min_share> <path>: the graph of all blocks written range by range (read_share_graph reads it); one line of
        counts is appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_shareGraph(self._s, int(min_share), os.fsencode(path), f))

    # ---- the components of the share graph (h10x_share_components_*): each range's rows are hooked into a label array on the device ----
    def share_components(self, min_share):
        """The connected components of the share graph at min_share over all blocks (every row entry (c, d) an undirected edge), walked
        in ranges of the option "share_graph_blocks": (comp uint32[nBlocks], root uint32[nBlocks], rootOf uint32[nComponents + 1],
        blocks uint32[nComponents + 1], records uint64[nComponents + 1]). root[c] = the smallest block of c's component, the components
        of blocks 1 .. are numbered 1 .. nComponents by ascending root, comp[c] = that number (comp[0] = 0), and per component its root,
        member count and sum of nHash (entry 0 all zero). The figures of the run (nBlocks, minShare, rows, listEntries, nComponents,
        largest, singletons, batches, windows, hookRounds) are kept in self.share_components_info."""
        if not self._ctx():
            raise Hash10xError("shareComponents: no hash state loaded: use readFQB or readHash first")
        z = np.zeros(1, dtype=_SHARE_COMPONENTS_INFO)
        min_share = max(-2 ** 31, min(int(min_share), 2 ** 31 - 1))
        self._chk(self._host.h10x_session_shareComponentsRun(self._s, min_share, z.ctypes.data))
        self.share_components_info = {n: int(z[n][0]) for n in _SHARE_COMPONENTS_INFO.names}
        nb, nc = self.share_components_info["nBlocks"], self.share_components_info["nComponents"] + 1
        comp, root = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32)
        root_of, blocks, records = np.zeros(nc, dtype=np.uint32), np.zeros(nc, dtype=np.uint32), np.zeros(nc, dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_share_components_get(self._ctx(), comp.ctypes.data, root.ctypes.data, root_of.ctypes.data, blocks.ctypes.data,
                                                          records.ctypes.data, nb, nc))
        return comp, root, root_of, blocks, records

    def write_share_components(self, min_share, path, out=None):
        """--shareComponents <min_share> <path>: the components of all blocks written as a .sc file (read_share_components reads it);
        one line of counts is appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_shareComponents(self._s, int(min_share), os.fsencode(path), f))

    # ---- the per-hash linkage groups (h10x_hash_copies_*): one wave per in-range hash reads the share graph restricted to its own blocks ----
    def hash_copies(self, min_share):
        """For every hash index the linkage groups of the blocks that hold it, at min_share: a (hashNumber, 4) uint16 array of
        (distinct, groups, largest, second) — the distinct blocks of the hash's barcode list, the connected components of the share
        graph at min_share restricted to them (either direction joins), the member counts of the largest and the second largest
        component (0 with one group). Hashes outside the depth range, and index 0, hold zeros. The figures of the run (hashNumber,
        minShare, inRange, rows, listEntries, deepest, oneGroup, split, batches, windows) are kept in self.hash_copies_info."""
        if not self._ctx():
            raise Hash10xError("hashCopies: no hash state loaded: use readFQB or readHash first")
        z = np.zeros(1, dtype=_HASH_COPIES_INFO)
        min_share = max(-2 ** 31, min(int(min_share), 2 ** 31 - 1))
        self._chk(self._host.h10x_session_hashCopiesRun(self._s, min_share, z.ctypes.data))
        self.hash_copies_info = {n: int(z[n][0]) for n in _HASH_COPIES_INFO.names if n != "reserved"}
        n = self.hash_copies_info["hashNumber"]
        out = np.zeros((max(n, 1), 4), dtype=np.uint16)
        self._chk_ctx(self._hip.h10x_hash_copies_get(self._ctx(), out.ctypes.data, 0, n))
        return out[:n]

    def hash_copies_tally(self):
        """Of the kept hash_copies result, per crib type (err, htA, htB, hom, mul; all under err when no crib was built): a (5, 3)
        uint64 array of the in-range hashes, those with groups == 1 and those with second >= 2."""
        if not self._ctx():
            raise Hash10xError("hashCopies: no hash state loaded: use readFQB or readHash first")
        counts = np.zeros((5, 3), dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_hash_copies_tally(self._ctx(), counts.ctypes.data))
        return counts

    def export_crib_type(self):
        """cribType[0 .. hashNumber) as uint8 (0 err, 1 htA, 2 htB, 3 hom, 4 mul; fails before --cribBuild): the classes hash_copies_tally counts by."""
        z = self.sizes()
        t = np.zeros(max(z["hashNumber"], 1), dtype=np.uint8)
        self._chk_ctx(self._hip.h10x_crib_export(self._ctx(), None, None, t.ctypes.data, None))
        return t[:z["hashNumber"]]

    def write_hash_copies(self, min_share, path, out=None):
        """--hashCopies <min_share> <path>: the table written as a .hc file (read_hash_copies reads it); one line of counts, and with a
        crib the five HASH_COPIES lines, are appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_hashCopies(self._s, int(min_share), os.fsencode(path), f))

    # ---- the state as a mosh set (h10x_mosh_from_state, csrc/stage_o.hip): the in-range hashes with 16-bit depths and copy classes ----
    def mosh_set(self, copy1min, copy2min, copyMmin, bits=0):
        """The hashes in the depth range as a MoshSet, built on the device from the state: value = the hash, depth = min(hashDepth, 65535),
        class from the saturated depth by the three thresholds of moshutils -s and, where a hash_copies result is kept, corrected by linkage
        (second >= 2 -> M, otherwise largest < 2 -> 0). bits = the table bits of the set, 0 = the state's B. The figures (kept, copy[4], toM,
        to0, saturated, crib[5][4], hashNumber, bits, minShare: 0 = depth only) are kept in self.mosh_set_info. The kept hash_copies result stays."""
        if not self._ctx():
            raise Hash10xError("!! you must set hashDepthRange before writeMosh")
        z = np.zeros(1, dtype=_STATE_MOSH_INFO)
        h = ctypes.c_void_p()
        self._chk(self._host.h10x_session_moshSet(self._s, int(bits), int(copy1min), int(copy2min), int(copyMmin), ctypes.byref(h), z.ctypes.data))
        self.mosh_set_info = _state_mosh_info(z)
        return MoshSet(_handle=h)

    def write_mosh(self, bits, copy1min, copy2min, copyMmin, path, out=None):
        """--writeMosh <bits> <copy1min> <copy2min> <copyMmin> <path>: that set written as an MSHSTv1 file; one line of counts, and with a crib
        the five WRITE_MOSH lines, are appended to the file `out`. The figures are kept in self.mosh_set_info, as by mosh_set."""
        z = np.zeros(1, dtype=_STATE_MOSH_INFO)
        self._with_file(out, lambda f: self._host.h10x_session_writeMosh(self._s, int(bits), int(copy1min), int(copy2min), int(copyMmin), os.fsencode(path), f, z.ctypes.data))
        self.mosh_set_info = _state_mosh_info(z)

    # ---- from sequences to blocks (h10x_seq_hashes / h10x_list_share_* / h10x_seq_blocks_run, csrc/stage_p.hip) ----
    @staticmethod
    def _flatten_seqs(seqs):
        """a list of sequences -> (codes uint8, seq_start uint64): a byte string is text (ACGT in either case, anything else 0 as N),
        an array holds the codes 0 .. 3 themselves"""
        out = []
        for s in seqs:
            if isinstance(s, (bytes, bytearray, str)):
                s = np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8)
                s = _SEQ_CODE[s]
            out.append(np.ascontiguousarray(s, dtype=np.uint8).reshape(-1))
        start = np.zeros(len(out) + 1, dtype=np.uint64)
        if out:
            start[1:] = np.cumsum([len(s) for s in out])
        return (np.ascontiguousarray(np.concatenate(out)) if out else np.zeros(0, np.uint8)), start

    def _seq_ctx(self, cmd):
        ctx = self._ctx()
        if not ctx:
            raise Hash10xError("%s: no hash state loaded: use readFQB or readHash first" % cmd)
        return ctx

    def seq_hashes(self, seqs):
        """Per sequence the distinct hash indices of its moshes that the state holds within the depth range, ascending: (offsets
        uint64[n + 1], hash uint32[], figures) with figures a structured array of (moshes, found, query, entries) per sequence: the mosh
        occurrences, those found in the state's table, the length of the list and the sum of hashDepth over it."""
        ctx = self._seq_ctx("seqHashes")
        codes, start = self._flatten_seqs(seqs)
        n = len(start) - 1
        fig = np.zeros(max(n, 1), dtype=_SEQ_FIGURES)
        self._chk_ctx(self._hip.h10x_seq_hashes(ctx, codes.ctypes.data, start.ctypes.data, n, fig.ctypes.data))
        off = np.zeros(n + 1, dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_seq_hashes_get(ctx, off.ctypes.data, None, 0))
        m = int(off[-1])
        hsh = np.zeros(max(m, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_seq_hashes_get(ctx, None, hsh.ctypes.data, m))
        return off, hsh[:m], fig[:n][["moshes", "found", "query", "entries"]]

    def _list_share_rows(self, ctx, z):
        self.seq_blocks_info = {k: int(z[k][0]) for k in _LIST_SHARE_INFO.names}
        m = self.seq_blocks_info["rows"]
        off = np.zeros(self.seq_blocks_info["lists"] + 1, dtype=np.uint64)
        blk, cnt = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_list_share_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, m))
        return off, blk[:m], cnt[:m]

    def list_share(self, offsets, hashes, min_share):
        """The list census: per list of hash indices (CSR: offsets[nq + 1], hashes[]) the blocks that stand at least min_share times in
        the barcode lists of its hashes, as (offsets uint64[nq + 1], block uint32[], count uint32[]), ascending in block. No block is
        left out and the depth range is not applied. The figures of the run (rows, listEntries, listHashes, maxCount, batches, windows,
        wideBatches, nBlocks, lists) are kept in self.seq_blocks_info."""
        ctx = self._seq_ctx("listShare")
        o = np.ascontiguousarray(offsets, dtype=np.uint64); x = np.ascontiguousarray(hashes, dtype=np.uint32)
        if len(o) < 1 or int(o[-1]) > len(x):
            raise Hash10xError("listShare: offsets must hold nq + 1 entries and end within the hashes")
        z = np.zeros(1, dtype=_LIST_SHARE_INFO)
        self._chk_ctx(self._hip.h10x_list_share_run(ctx, int(min_share), o.ctypes.data, x.ctypes.data, len(o) - 1, z.ctypes.data))
        return self._list_share_rows(ctx, z)

    def seq_blocks(self, seqs, min_share):
        """Per sequence the blocks that stand at least min_share times in the barcode lists of its in-range hashes (seq_hashes fed into
        list_share on the device): (offsets, block, count, figures). The figures of the run are kept in self.seq_blocks_info."""
        ctx = self._seq_ctx("seqBlocks")
        codes, start = self._flatten_seqs(seqs)
        n = len(start) - 1
        fig = np.zeros(max(n, 1), dtype=_SEQ_FIGURES); z = np.zeros(1, dtype=_LIST_SHARE_INFO)
        self._chk_ctx(self._hip.h10x_seq_blocks_run(ctx, int(min_share), codes.ctypes.data, start.ctypes.data, n, fig.ctypes.data, z.ctypes.data))
        return self._list_share_rows(ctx, z) + (fig[:n][["moshes", "found", "query", "entries"]],)

    def write_seq_blocks(self, min_share, seqfile, path, out=None, verbose=False):
        """--seqBlocks <min_share> <seqfile> <path>: the rows of every sequence of a FASTA / FASTQ file (gzip or plain) written slab by slab
        as a .sb file (read_seq_blocks reads it); one line of counts, and with verbose one SEQ_BLOCKS line per sequence, are appended to
        the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_seqBlocks(self._s, int(min_share), os.fsencode(seqfile), os.fsencode(path), f, 1 if verbose else 0))

    # ---- sequence spans (h10x_seq_spans_*, csrc/stage_r.hip) ----
    def seq_spans(self, seqs, min_share, max_gap=0, window=0):
        """Per sequence the extents of the blocks on it: the hits of a block (one per entry of the barcode list of every in-range mosh occurrence,
        at the occurrence's position) cut where they lie more than max_gap apart (0: never), kept at min_share hits, ascending by (block, first);
        and for window >= 1 the number of kept extents that span each multiple of window inside the sequence. Returns (offsets uint64[n + 1],
        block, first, last, hits uint32[], cover_offsets uint64[n + 1], cover uint32[]). The figures of the run are kept in self.seq_spans_info,
        the per-sequence ones (len, moshes, found, inRange, extents) as its entry "figures"."""
        ctx = self._seq_ctx("seqSpans")
        codes, start = self._flatten_seqs(seqs)
        n = len(start) - 1
        fig = np.zeros(max(n, 1), dtype=_SEQ_SPAN_FIGURES); z = np.zeros(1, dtype=_SEQ_SPANS_INFO)
        self._chk_ctx(self._hip.h10x_seq_spans_run(ctx, int(min_share), int(max_gap), int(window), codes.ctypes.data, start.ctypes.data, n, fig.ctypes.data, z.ctypes.data))
        self.seq_spans_info = {k: int(z[k][0]) for k in _SEQ_SPANS_INFO.names if k != "reserved"}
        self.seq_spans_info["figures"] = fig[:n].copy()
        m, nb = self.seq_spans_info["extents"], self.seq_spans_info["boundaries"]
        off, coff = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        cols = [np.zeros(max(m, 1), dtype=np.uint32) for _ in range(4)]
        cover = np.zeros(max(nb, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_seq_spans_get(ctx, off.ctypes.data, *[c.ctypes.data for c in cols], m))
        self._chk_ctx(self._hip.h10x_seq_spans_cover_get(ctx, coff.ctypes.data, cover.ctypes.data, nb))
        return (off,) + tuple(c[:m] for c in cols) + (coff, cover[:nb])

    def write_seq_spans(self, min_share, max_gap, window, min_cover, seqfile, path, out=None, verbose=False):
        """--seqSpans <min_share> <max_gap> <window> <min_cover> <seqfile> <path>: the extents and the spanning coverage of every sequence of a
        FASTA / FASTQ file (gzip or plain) written slab by slab as a .ss file (read_seq_spans reads it); one line of counts, and with verbose
        one SEQ_SPANS line per sequence and one SEQ_WEAK line per run of boundaries below min_cover, are appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_seqSpans(self._s, int(min_share), int(max_gap), int(window), int(min_cover), os.fsencode(seqfile),
                                                                        os.fsencode(path), f, 1 if verbose else 0))

    # ---- sequence spectrum (h10x_seq_spectrum_*, csrc/stage_s.hip) ----
    def seq_spectrum(self, seqs, copy1min, copy2min, copyMmin, window=0):
        """The moshes of the sequences against the read depths of the state (no depth range needed). Every mosh occurrence is absent from the
        state or of depth class 0 (hashDepth < copy1min), 1 (< copy2min), 2 (< copyMmin) or M. Returns (figures, win_offsets, windows, spectrum,
        totals): figures per sequence (len, moshes, absent, n0, n1, n2, nM, depthSum), windows the same fields without len per window of
        `window` bases (window 0: none) in CSR form by win_offsets uint64[n + 1], spectrum uint64[1024, 8] counting the state's hashes by
        (min(depth, 1023), min(copies, 7)) with copies = the times the sequences hold the hash, totals uint64[2, 4] = the hashes of each class
        and those of them held at least once. The sums of the run are kept in self.seq_spectrum_info, copies[] for seq_copies()."""
        ctx = self._seq_ctx("seqSpectrum")
        codes, start = self._flatten_seqs(seqs)
        n = len(start) - 1
        self._chk_ctx(self._hip.h10x_seq_spectrum_begin(ctx, int(copy1min), int(copy2min), int(copyMmin), int(window)))
        fig = np.zeros(max(n, 1), dtype=_SEQ_SPECTRUM_FIGURES); z = np.zeros(1, dtype=_SEQ_SPECTRUM_INFO)
        self._chk_ctx(self._hip.h10x_seq_spectrum_add(ctx, codes.ctypes.data, start.ctypes.data, n, fig.ctypes.data, z.ctypes.data))
        m = int(z["windows"][0])
        off = np.zeros(n + 1, dtype=np.uint64); win = np.zeros(max(m, 1), dtype=_SEQ_SPECTRUM_WINDOW)
        self._chk_ctx(self._hip.h10x_seq_spectrum_windows_get(ctx, off.ctypes.data, win.ctypes.data, m))
        spectrum = np.zeros((SPECTRUM_DEPTH_BINS, SPECTRUM_COPY_BINS), dtype=np.uint64); totals = np.zeros((2, 4), dtype=np.uint64)
        self._chk_ctx(self._hip.h10x_seq_spectrum_finish(ctx, spectrum.ctypes.data, totals.ctypes.data, z.ctypes.data))
        self.seq_spectrum_info = {k: int(z[k][0]) for k in _SEQ_SPECTRUM_INFO.names}
        return fig[:n].copy(), off, win[:m].copy(), spectrum, totals

    def seq_copies(self, first=0, count=None):
        """copies[first .. first + count) of the kept sequence spectrum as uint32 (count None: to the end): the times the sequences of the run
        hold each hash of the state; copies[0] is 0."""
        ctx = self._seq_ctx("seqSpectrum")
        if count is None:
            count = max(self.sizes()["hashNumber"] - int(first), 0)
        out = np.zeros(max(int(count), 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_seq_spectrum_copies_get(ctx, int(first), int(count), out.ctypes.data))
        return out[:int(count)]

    def write_seq_spectrum(self, copy1min, copy2min, copyMmin, window, seqfile, path, out=None, verbose=False):
        """--seqSpectrum <copy1min> <copy2min> <copyMmin> <window> <seqfile> <path>: the spectrum of every sequence of a FASTA / FASTQ file (gzip
        or plain) against the state, read slab by slab, written as a .sp file (read_seq_spectrum reads it); one line of counts with QV and
        completeness, and with verbose one SEQ_SPECTRUM line per sequence, are appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_seqSpectrum(self._s, int(copy1min), int(copy2min), int(copyMmin), int(window), os.fsencode(seqfile),
                                                                           os.fsencode(path), f, 1 if verbose else 0))

    # ---- row links (h10x_row_links_*, csrc/stage_q.hip) ----
    def _row_links_ctx(self, cmd):
        """the session's context (it comes with the first state; the row layer itself reads none)"""
        if not self._ctx():
            raise Hash10xError("%s: no hash state loaded: use readFQB or readHash first" % cmd)
        return self._ctx()

    def _row_links_finish(self, ctx, min_blocks, max_lists, siblings):
        z = np.zeros(1, dtype=_ROW_LINKS_INFO)
        self._chk_ctx(self._hip.h10x_row_links_finish(ctx, int(min_blocks), int(max_lists), 1 if siblings else 0, z.ctypes.data))
        info = {k: int(z[k][0]) for k in _ROW_LINKS_INFO.names}
        m = info["links"]
        off = np.zeros(info["lists"] + 1, dtype=np.uint64)
        other, shared = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
        self._chk_ctx(self._hip.h10x_row_links_get(ctx, off.ctypes.data, other.ctypes.data, shared.ctypes.data, m))
        return info, (off, other[:m], shared[:m])

    def row_links(self, offsets, block, min_blocks, max_lists=0, siblings=False, n_blocks=None):
        """Which lists of block numbers share blocks. The lists come in CSR form (offsets[n + 1], block[]), each strictly ascending, every block
        below n_blocks (default: the state's). A block that stands in more than max_lists lists is left out (0: none is); with siblings
        lists 2s and 2s + 1 are never linked. Returns (offsets uint64[n + 1], other uint32[], shared uint32[]): per list e the lists f > e
        that share at least min_blocks blocks with it, ascending, with the number shared. The figures of the run (lists, rowEntries,
        blocksUsed, skippedBlocks, pairs, links, maxShared, batches, windows, wideBatches) are kept in self.row_links_info."""
        ctx = self._row_links_ctx("rowLinks")
        o = np.ascontiguousarray(offsets, dtype=np.uint64); b = np.ascontiguousarray(block, dtype=np.uint32)
        if len(o) < 1 or int(o[-1]) > len(b):
            raise Hash10xError("rowLinks: offsets must hold n + 1 entries and end within the blocks")
        self._chk_ctx(self._hip.h10x_row_links_begin(ctx, int(self.sizes()["nBlocks"] if n_blocks is None else n_blocks)))
        self._chk_ctx(self._hip.h10x_row_links_add(ctx, o.ctypes.data, b.ctypes.data, len(o) - 1))
        self.row_links_info, out = self._row_links_finish(ctx, min_blocks, max_lists, siblings)
        return out

    @staticmethod
    def _cut_ends(seqs, end_len):
        """the two ends of every sequence, as sequences: the first and the last min(len, end_len) bases; end_len 0: the whole and none"""
        codes, start = Hash10x._flatten_seqs(seqs)
        ends = []
        for a, b in zip(start[:-1], start[1:]):
            a, b = int(a), int(b)
            m = min(b - a, int(end_len)) if end_len else b - a
            ends += [codes[a:a + m], codes[b - m:b] if end_len else codes[:0]]
        return ends

    def seq_links(self, seqs, min_share, min_blocks, end_len, max_ends=0):
        """Which ends of the sequences share blocks (after --clusterSplit and a new range: molecules). Sequence s gives end 2s, its first
        min(len, end_len) bases, and end 2s + 1, its last (end_len 0: the whole sequence and an empty end). The row of an end is its
        seq_blocks row at min_share; the rows go from seq_blocks to the join on the device. Returns (offsets uint64[2 n + 1], other, shared)
        as row_links with siblings on and max_lists = max_ends. The figures are kept in self.seq_links_info."""
        ctx = self._seq_ctx("seqLinks")
        if int(end_len) < 0 or int(max_ends) < 0:
            raise Hash10xError("!! seqLinks %s %d must be >= 0" % (("endLen", int(end_len)) if int(end_len) < 0 else ("maxEnds", int(max_ends))))
        codes, start = self._flatten_seqs(self._cut_ends(seqs, end_len))
        n = len(start) - 1
        z = np.zeros(1, dtype=_LIST_SHARE_INFO)
        if self._hip.h10x_seq_blocks_run(ctx, int(min_share), codes.ctypes.data, start.ctypes.data, n, None, z.ctypes.data):
            raise Hash10xError(self._hip.h10x_last_error(ctx).decode(errors="replace").replace("seqBlocks", "seqLinks"))
        self._chk_ctx(self._hip.h10x_row_links_begin(ctx, int(z["nBlocks"][0])))
        self._chk_ctx(self._hip.h10x_row_links_add_kept(ctx))
        self.seq_links_info, out = self._row_links_finish(ctx, min_blocks, max_ends, True)
        return out

    def write_seq_links(self, min_share, min_blocks, end_len, max_ends, seqfile, path, out=None, verbose=False):
        """--seqLinks <min_share> <min_blocks> <end_len> <max_ends> <seqfile> <path>: the links between the ends of the sequences of a FASTA /
        FASTQ file (gzip or plain) written as a .sl file (read_seq_links reads it); one line of counts, and with verbose one SEQ_LINKS line
        per link, are appended to the file `out`."""
        self._with_file(out, lambda f: self._host.h10x_session_seqLinks(self._s, int(min_share), int(min_blocks), int(end_len), int(max_ends), os.fsencode(seqfile),
                                                                        os.fsencode(path), f, 1 if verbose else 0))

    def export_within(self):
        """hashWithinRange[0 .. hashNumber) as uint8 (fails before --hashDepthRange)."""
        z = self.sizes()
        w = np.zeros(max(z["hashNumber"], 1), dtype=np.uint8)
        self._chk_ctx(self._hip.h10x_export_slice(self._ctx(), 7, 0, z["hashNumber"], w.ctypes.data))
        return w[:z["hashNumber"]]


_SEQ_FIGURES = np.dtype([("moshes", "<u4"), ("found", "<u4"), ("query", "<u4"), ("reserved", "<u4"), ("entries", "<u8")])
_LIST_SHARE_INFO = np.dtype([("rows", "<u8"), ("listEntries", "<u8"), ("listHashes", "<u8"), ("maxCount", "<u4"), ("batches", "<u4"), ("windows", "<u4"),
                             ("wideBatches", "<u4"), ("nBlocks", "<u4"), ("lists", "<u4")])
_ROW_LINKS_INFO = np.dtype([("lists", "<u8"), ("rowEntries", "<u8"), ("blocksUsed", "<u8"), ("skippedBlocks", "<u8"), ("pairs", "<u8"), ("links", "<u8"),
                            ("maxShared", "<u4"), ("batches", "<u4"), ("windows", "<u4"), ("wideBatches", "<u4")])
_SEQ_SPAN_FIGURES = np.dtype([("len", "<u8"), ("moshes", "<u4"), ("found", "<u4"), ("inRange", "<u4"), ("extents", "<u4")])
_SEQ_SPANS_INFO = np.dtype([(k, "<u8") for k in ("sequences", "bases", "moshes", "found", "inRange", "hits", "extentsAll", "extents", "sumSpan", "boundaries")] +
                           [(k, "<u4") for k in ("maxHits", "maxSpan", "batches", "windows", "nBlocks", "reserved")])
SPECTRUM_DEPTH_BINS, SPECTRUM_COPY_BINS = 1024, 8            # H10X_SPECTRUM_DEPTH_BINS, H10X_SPECTRUM_COPY_BINS (include/h10x.h)
_SEQ_SPECTRUM_WINDOW = np.dtype([(k, "<u4") for k in ("moshes", "absent", "n0", "n1", "n2", "nM")] + [("depthSum", "<u8")])
_SEQ_SPECTRUM_FIGURES = np.dtype([("len", "<u8")] + [(k, "<u4") for k in ("moshes", "absent", "n0", "n1", "n2", "nM")] + [("depthSum", "<u8")])
_SEQ_SPECTRUM_INFO = np.dtype([(k, "<u8") for k in ("sequences", "bases", "moshes", "absent", "n0", "n1", "n2", "nM", "depthSum", "windows")] +
                              [("hashNumber", "<u4"), ("maxCopies", "<u4")])
_SEQ_CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _SEQ_CODE[ord(_c)] = _SEQ_CODE[ord(_c.lower())] = _i

_SHARE_GRAPH_INFO = np.dtype([("rows", "<u8"), ("listEntries", "<u8"), ("entriesRead", "<u8"), ("maxCount", "<u4"), ("batches", "<u4"), ("windows", "<u4"),
                              ("codeMin", "<u4"), ("codeMax", "<u4"), ("nBlocks", "<u4")])


def read_share_graph(path):
    """A --shareGraph file (magic "10XG", u32 version 1, u32 nBlocks, u32 minShare, u64 rows, nBlocks + 1 u64 offsets, rows pairs
    {u32 block, u32 count}, little-endian; needs no device): ({"version", "nBlocks", "minShare", "rows"}, offsets, block, count). The row
    of block c is [offsets[c], offsets[c + 1]). Raises Hash10xError for a file that is not one or does not hold together."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 24 or data[:4] != b"10XG":
        raise Hash10xError("%s: not a share graph file (magic 10XG)" % path)
    version, n_blocks, min_share = (int(v) for v in np.frombuffer(data, dtype="<u4", count=3, offset=4))
    rows = int(np.frombuffer(data, dtype="<u8", count=1, offset=16)[0])
    if version != 1:
        raise Hash10xError("%s: share graph version %d, this reader knows 1" % (path, version))
    if len(data) != 24 + 8 * (n_blocks + 1) + 8 * rows:
        raise Hash10xError("%s: %d bytes, %d blocks and %d rows need %d" % (path, len(data), n_blocks, rows, 24 + 8 * (n_blocks + 1) + 8 * rows))
    off = np.frombuffer(data, dtype="<u8", count=n_blocks + 1, offset=24).copy()
    if off[0] != 0 or int(off[-1]) != rows or np.any(off[1:] < off[:-1]):
        raise Hash10xError("%s: the offsets do not ascend from 0 to the %d rows" % (path, rows))
    pairs = np.frombuffer(data, dtype="<u4", count=2 * rows, offset=24 + 8 * (n_blocks + 1)).reshape(-1, 2)
    return {"version": version, "nBlocks": n_blocks, "minShare": min_share, "rows": rows}, off, pairs[:, 0].copy(), pairs[:, 1].copy()


_SB_RECORD = np.dtype([("len", "<u8"), ("moshes", "<u4"), ("found", "<u4"), ("query", "<u4"), ("reserved", "<u4")])


def read_seq_blocks(path):
    """A --seqBlocks file (magic "10XQ", u32 version 1, u32 nBlocks, u32 minShare, u64 nSeq, u64 rows, u64 nameBytes; rows pairs {u32 block,
    u32 count}; nSeq records {u64 len, u32 moshes, u32 found, u32 query, u32 0}; nSeq + 1 u64 offsets; nSeq + 1 u64 name offsets; the names,
    NUL-terminated; little-endian; needs no device): ({"version", "nBlocks", "minShare", "nSeq", "rows", "nameBytes"}, offsets, block, count,
    table, names). The row of sequence s is [offsets[s], offsets[s + 1]). Raises Hash10xError for a file that is not one or does not hold
    together: the sizes against the file's length, both offset arrays, blocks ascending within a row and below nBlocks, counts >= minShare."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 40 or data[:4] != b"10XQ":
        raise Hash10xError("%s: not a seq blocks file (magic 10XQ)" % path)
    version, n_blocks, min_share = (int(v) for v in np.frombuffer(data, dtype="<u4", count=3, offset=4))
    n_seq, rows, name_bytes = (int(v) for v in np.frombuffer(data, dtype="<u8", count=3, offset=16))
    if version != 1:
        raise Hash10xError("%s: seq blocks version %d, this reader knows 1" % (path, version))
    need = 40 + 8 * rows + 24 * n_seq + 16 * (n_seq + 1) + name_bytes
    if len(data) != need:
        raise Hash10xError("%s: %d bytes, %d sequences, %d rows and %d name bytes need %d" % (path, len(data), n_seq, rows, name_bytes, need))
    at = 40
    pairs = np.frombuffer(data, dtype="<u4", count=2 * rows, offset=at).reshape(-1, 2); at += 8 * rows
    table = np.frombuffer(data, dtype=_SB_RECORD, count=n_seq, offset=at).copy(); at += 24 * n_seq
    off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    name_off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    blob = data[at:]
    if off[0] != 0 or int(off[-1]) != rows or np.any(off[1:] < off[:-1]):
        raise Hash10xError("%s: the offsets do not ascend from 0 to the %d rows" % (path, rows))
    if name_off[0] != 0 or int(name_off[-1]) != name_bytes or np.any(name_off[1:] <= name_off[:-1]):
        raise Hash10xError("%s: the name offsets do not ascend from 0 to the %d name bytes" % (path, name_bytes))
    if any(blob[int(e) - 1] != 0 for e in name_off[1:]):
        raise Hash10xError("%s: a name does not end in NUL" % path)
    blk, cnt = pairs[:, 0].copy(), pairs[:, 1].copy()
    if rows:
        if int(blk.max()) >= n_blocks:
            raise Hash10xError("%s: a row's block is beyond the %d blocks" % (path, n_blocks))
        if int(cnt.min()) < max(min_share, 1):
            raise Hash10xError("%s: a row's count is below minShare %d" % (path, min_share))
        inner = np.ones(rows, dtype=bool)
        inner[off[:-1][off[:-1] < rows].astype(np.int64)] = False   # the first entry of a row has no predecessor in it
        if np.any(inner[1:] & (blk[1:] <= blk[:-1])):
            raise Hash10xError("%s: the blocks of a row do not ascend" % path)
    if np.any(table["reserved"] != 0):
        raise Hash10xError("%s: a reserved word of the table is not 0" % path)
    names = [blob[int(a):int(b) - 1].decode(errors="replace") for a, b in zip(name_off[:-1], name_off[1:])]
    info = {"version": version, "nBlocks": n_blocks, "minShare": min_share, "nSeq": n_seq, "rows": rows, "nameBytes": name_bytes}
    return info, off, blk, cnt, table, names


_SS_RECORD = np.dtype([("len", "<u8"), ("moshes", "<u4"), ("found", "<u4"), ("inRange", "<u4"), ("weak", "<u4")])


def read_seq_spans(path):
    """A --seqSpans file (magic "10XE", u32 version 1, u32 nBlocks, u32 minShare, u32 maxGap, u32 window, u32 minCover, u32 0, u64 nSeq, u64 extents,
    u64 boundaries, u64 nameBytes; extents records {u32 block, u32 first, u32 last, u32 hits}; nSeq records {u64 len, u32 moshes, u32 found, u32
    inRange, u32 weak}; nSeq + 1 u64 offsets; nSeq + 1 u64 cover offsets; boundaries u32 cover; nSeq + 1 u64 name offsets; the names, NUL-terminated;
    little-endian; needs no device): (info, offsets, block, first, last, hits, cover_offsets, cover, table, names). Raises Hash10xError for a file
    that is not one or does not hold together: magic and version, the file's length, the offsets ascending to `extents`, the cover offsets against
    (len - 1) // window, first <= last < len, blocks below nBlocks, rows ascending by (block, first), hits >= minShare, weak against cover and
    minCover, the names."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 64 or data[:4] != b"10XE":
        raise Hash10xError("%s: not a seq spans file (magic 10XE)" % path)
    version, n_blocks, min_share, max_gap, window, min_cover, zero = (int(v) for v in np.frombuffer(data, dtype="<u4", count=7, offset=4))
    n_seq, extents, boundaries, name_bytes = (int(v) for v in np.frombuffer(data, dtype="<u8", count=4, offset=32))
    if version != 1:
        raise Hash10xError("%s: seq spans version %d, this reader knows 1" % (path, version))
    need = 64 + 16 * extents + 24 * n_seq + 24 * (n_seq + 1) + 4 * boundaries + name_bytes
    if len(data) != need:
        raise Hash10xError("%s: %d bytes, %d sequences, %d extents, %d boundaries and %d name bytes need %d" % (path, len(data), n_seq, extents, boundaries, name_bytes, need))
    if zero:
        raise Hash10xError("%s: the reserved word of the header is not 0" % path)
    at = 64
    quad = np.frombuffer(data, dtype="<u4", count=4 * extents, offset=at).reshape(-1, 4); at += 16 * extents
    table = np.frombuffer(data, dtype=_SS_RECORD, count=n_seq, offset=at).copy(); at += 24 * n_seq
    off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    coff = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    cover = np.frombuffer(data, dtype="<u4", count=boundaries, offset=at).copy(); at += 4 * boundaries
    name_off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    blob = data[at:]
    if off[0] != 0 or int(off[-1]) != extents or np.any(off[1:] < off[:-1]):
        raise Hash10xError("%s: the offsets do not ascend from 0 to the %d extents" % (path, extents))
    lens = table["len"].astype(np.int64)
    exp = np.zeros(n_seq + 1, dtype=np.uint64)
    if window:
        exp[1:] = np.cumsum(np.where(lens > 0, (lens - 1) // window, 0))
    if not np.array_equal(coff, exp) or int(coff[-1]) != boundaries:
        raise Hash10xError("%s: the cover offsets are not those of the lengths at window %d" % (path, window))
    if name_off[0] != 0 or int(name_off[-1]) != name_bytes or np.any(name_off[1:] <= name_off[:-1]):
        raise Hash10xError("%s: the name offsets do not ascend from 0 to the %d name bytes" % (path, name_bytes))
    if any(blob[int(e) - 1] != 0 for e in name_off[1:]):
        raise Hash10xError("%s: a name does not end in NUL" % path)
    blk, first, last, hits = (quad[:, i].copy() for i in range(4))
    if extents:
        row_len = np.repeat(lens, np.diff(off.astype(np.int64)))
        if np.any(first > last) or np.any(last.astype(np.int64) >= row_len):
            raise Hash10xError("%s: an extent does not lie in its sequence (first <= last < len)" % path)
        if int(blk.max()) >= n_blocks:
            raise Hash10xError("%s: an extent's block is beyond the %d blocks" % (path, n_blocks))
        if int(hits.min()) < max(min_share, 1):
            raise Hash10xError("%s: an extent's hits are below minShare %d" % (path, min_share))
        inner = np.ones(extents, dtype=bool)
        inner[off[:-1][off[:-1] < extents].astype(np.int64)] = False   # the first extent of a row has no predecessor in it
        key = blk.astype(np.uint64) << np.uint64(32) | first.astype(np.uint64)
        if np.any(inner[1:] & (key[1:] <= key[:-1])):
            raise Hash10xError("%s: the extents of a row do not ascend by (block, first)" % path)
    weak = np.add.reduceat(np.r_[(cover < min_cover).astype(np.int64), 0], coff[:-1].astype(np.int64)) * (np.diff(coff.astype(np.int64)) > 0) if n_seq else np.zeros(0, np.int64)
    if not np.array_equal(weak, table["weak"].astype(np.int64)):
        raise Hash10xError("%s: a sequence's weak count is not that of its cover at minCover %d" % (path, min_cover))
    names = [blob[int(a):int(b) - 1].decode(errors="replace") for a, b in zip(name_off[:-1], name_off[1:])]
    info = {"version": version, "nBlocks": n_blocks, "minShare": min_share, "maxGap": max_gap, "window": window, "minCover": min_cover, "nSeq": n_seq,
            "extents": extents, "boundaries": boundaries, "nameBytes": name_bytes}
    return info, off, blk, first, last, hits, coff, cover, table, names


def seq_qv(moshes, unsupported, k):
    """QV of --seqSpectrum: -10 log10(1 - (1 - unsupported / moshes) ** (1 / k)); inf when nothing is unsupported, 0 without moshes"""
    if not moshes:
        return 0.0
    if not unsupported:
        return float("inf")
    return -10.0 * float(np.log10(1.0 - (1.0 - unsupported / moshes) ** (1.0 / k))) + 0.0


def read_seq_spectrum(path):
    """A --seqSpectrum file (magic "10XP", u32 version 1, u32 hashNumber, u32 copy1min, u32 copy2min, u32 copyMmin, u32 window, u32 depthBins,
    u32 copyBins, u32 0, u64 nSeq, u64 windows, u64 nameBytes; windows records {u32 moshes, absent, n0, n1, n2, nM; u64 depthSum}; nSeq records
    {u64 len; the same seven}; nSeq + 1 u64 window offsets; 8 u64 totals; depthBins x copyBins u64 spectrum; hashNumber bytes min(copies, 255);
    nSeq + 1 u64 name offsets; the names, NUL-terminated; little-endian; needs no device): (info, figures, win_offsets, windows, spectrum,
    totals uint64[2, 4], copies uint8[hashNumber], names). Raises Hash10xError for a file that is not one or does not hold together: magic,
    version, the bins, the file's length, the thresholds' order, the window offsets against ceil(len / window), moshes = absent + the four
    classes in every record, the windows of a sequence summing to its figures, the spectrum and the totals summing to hashNumber - 1, the
    totals against the spectrum's rows (thresholds up to 1023), present <= total, the spectrum's columns and the present hashes against the
    copies bytes, the bytes' sum against the found occurrences, the names."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 64 or data[:4] != b"10XP":
        raise Hash10xError("%s: not a seq spectrum file (magic 10XP)" % path)
    version, hash_number, c1, c2, cm, window, dbins, cbins, zero = (int(v) for v in np.frombuffer(data, dtype="<u4", count=9, offset=4))
    n_seq, n_win, name_bytes = (int(v) for v in np.frombuffer(data, dtype="<u8", count=3, offset=40))
    if version != 1:
        raise Hash10xError("%s: seq spectrum version %d, this reader knows 1" % (path, version))
    if (dbins, cbins) != (SPECTRUM_DEPTH_BINS, SPECTRUM_COPY_BINS):
        raise Hash10xError("%s: a spectrum of %d x %d bins, this reader knows %d x %d" % (path, dbins, cbins, SPECTRUM_DEPTH_BINS, SPECTRUM_COPY_BINS))
    need = 64 + 32 * n_win + 40 * n_seq + 16 * (n_seq + 1) + 64 + 8 * dbins * cbins + hash_number + name_bytes
    if len(data) != need:
        raise Hash10xError("%s: %d bytes, %d sequences, %d windows, %d hashes and %d name bytes need %d" % (path, len(data), n_seq, n_win, hash_number, name_bytes, need))
    if zero:
        raise Hash10xError("%s: the reserved word of the header is not 0" % path)
    if not c1 <= c2 <= cm:
        raise Hash10xError("%s: the thresholds %d %d %d do not ascend" % (path, c1, c2, cm))
    at = 64
    win = np.frombuffer(data, dtype=_SEQ_SPECTRUM_WINDOW, count=n_win, offset=at).copy(); at += 32 * n_win
    fig = np.frombuffer(data, dtype=_SEQ_SPECTRUM_FIGURES, count=n_seq, offset=at).copy(); at += 40 * n_seq
    off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    totals = np.frombuffer(data, dtype="<u8", count=8, offset=at).copy().reshape(2, 4); at += 64
    spectrum = np.frombuffer(data, dtype="<u8", count=dbins * cbins, offset=at).copy().reshape(dbins, cbins); at += 8 * dbins * cbins
    copies = np.frombuffer(data, dtype=np.uint8, count=hash_number, offset=at).copy(); at += hash_number
    name_off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    blob = data[at:]
    lens = fig["len"].astype(np.int64)
    exp = np.zeros(n_seq + 1, dtype=np.uint64)
    if window:
        exp[1:] = np.cumsum((lens + window - 1) // window)
    if not np.array_equal(off, exp) or int(off[-1]) != n_win:
        raise Hash10xError("%s: the window offsets are not those of the lengths at window %d" % (path, window))
    fields = ("moshes", "absent", "n0", "n1", "n2", "nM", "depthSum")
    for rec, what in ((win, "window"), (fig, "sequence")):
        if np.any(rec["moshes"].astype(np.int64) != sum(rec[k].astype(np.int64) for k in fields[1:6])):
            raise Hash10xError("%s: a %s's moshes are not its absent and its four classes" % (path, what))
    if window and n_seq:
        live = off[:-1] < off[1:]
        for k in fields:
            sums = np.zeros(n_seq, dtype=np.uint64)
            if n_win:
                sums[live] = np.add.reduceat(win[k].astype(np.uint64), off[:-1][live].astype(np.int64))
            if not np.array_equal(sums, fig[k].astype(np.uint64)):
                raise Hash10xError("%s: the windows of a sequence do not sum to its %s" % (path, k))
    hashes = max(hash_number - 1, 0)
    if int(spectrum.sum()) != hashes or int(totals[0].sum()) != hashes:
        raise Hash10xError("%s: the spectrum and the totals do not sum to the %d hashes" % (path, hashes))
    if np.any(totals[1] > totals[0]):
        raise Hash10xError("%s: more hashes of a class are present than there are" % path)
    if cm <= SPECTRUM_DEPTH_BINS - 1:
        edges = (0, c1, c2, cm, SPECTRUM_DEPTH_BINS)
        for q in range(4):
            rows = spectrum[edges[q]:edges[q + 1]]
            if int(rows.sum()) != int(totals[0, q]) or int(rows[:, 1:].sum()) != int(totals[1, q]):
                raise Hash10xError("%s: the totals of class %d are not those of the spectrum's rows" % (path, q))
    if hash_number and copies[0]:
        raise Hash10xError("%s: byte 0 of the copies is not 0" % path)
    held = np.bincount(np.minimum(copies[1:], cbins - 1), minlength=cbins) if hash_number > 1 else np.zeros(cbins, dtype=np.int64)
    if not np.array_equal(held.astype(np.uint64), spectrum.sum(axis=0)) or int((copies[1:] > 0).sum()) != int(totals[1].sum()):
        raise Hash10xError("%s: the copies are not those of the spectrum's columns" % path)
    found = int(fig["moshes"].astype(np.int64).sum() - fig["absent"].astype(np.int64).sum())
    held_sum = int(copies.astype(np.int64).sum())
    if held_sum > found or (held_sum < found and not np.any(copies == 255)):
        raise Hash10xError("%s: the copies sum to %d and the sequences found %d" % (path, held_sum, found))
    if name_off[0] != 0 or int(name_off[-1]) != name_bytes or np.any(name_off[1:] <= name_off[:-1]):
        raise Hash10xError("%s: the name offsets do not ascend from 0 to the %d name bytes" % (path, name_bytes))
    if any(blob[int(e) - 1] != 0 for e in name_off[1:]):
        raise Hash10xError("%s: a name does not end in NUL" % path)
    names = [blob[int(a):int(b) - 1].decode(errors="replace") for a, b in zip(name_off[:-1], name_off[1:])]
    info = {"version": version, "hashNumber": hash_number, "copy1min": c1, "copy2min": c2, "copyMmin": cm, "window": window, "depthBins": dbins,
            "copyBins": cbins, "nSeq": n_seq, "windows": n_win, "nameBytes": name_bytes}
    return info, fig, off, win, spectrum, totals, copies, names


_SL_RECORD = np.dtype([("len", "<u8"), ("headRows", "<u4"), ("tailRows", "<u4")])


def read_seq_links(path):
    """A --seqLinks file (magic "10XL", u32 version 1, u32 nBlocks, u32 minShare, u32 minBlocks, u32 endLen, u32 maxEnds, u32 0, u64 nSeq, u64 links,
    u64 skippedBlocks, u64 nameBytes; nSeq records {u64 len, u32 headRows, u32 tailRows}; 2 nSeq + 1 u64 offsets; links pairs {u32 end, u32
    shared}; nSeq + 1 u64 name offsets; the names, NUL-terminated; little-endian; needs no device): (info, offsets, other, shared, table, names).
    The row of end e (2s = the head of sequence s, 2s + 1 its tail) is [offsets[e], offsets[e + 1]). Raises Hash10xError for a file that is not
    one or does not hold together: the sizes against the file's length, both offset arrays, every end below 2 nSeq and above its row's own,
    ascending within a row, no link between the two ends of one sequence, shared >= minBlocks."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 64 or data[:4] != b"10XL":
        raise Hash10xError("%s: not a seq links file (magic 10XL)" % path)
    version, n_blocks, min_share, min_blocks, end_len, max_ends, zero = (int(v) for v in np.frombuffer(data, dtype="<u4", count=7, offset=4))
    n_seq, links, skipped, name_bytes = (int(v) for v in np.frombuffer(data, dtype="<u8", count=4, offset=32))
    if version != 1:
        raise Hash10xError("%s: seq links version %d, this reader knows 1" % (path, version))
    n_ends = 2 * n_seq
    need = 64 + 16 * n_seq + 8 * (n_ends + 1) + 8 * links + 8 * (n_seq + 1) + name_bytes
    if len(data) != need:
        raise Hash10xError("%s: %d bytes, %d sequences, %d links and %d name bytes need %d" % (path, len(data), n_seq, links, name_bytes, need))
    if zero:
        raise Hash10xError("%s: the reserved word of the header is not 0" % path)
    at = 64
    table = np.frombuffer(data, dtype=_SL_RECORD, count=n_seq, offset=at).copy(); at += 16 * n_seq
    off = np.frombuffer(data, dtype="<u8", count=n_ends + 1, offset=at).copy(); at += 8 * (n_ends + 1)
    pairs = np.frombuffer(data, dtype="<u4", count=2 * links, offset=at).reshape(-1, 2); at += 8 * links
    name_off = np.frombuffer(data, dtype="<u8", count=n_seq + 1, offset=at).copy(); at += 8 * (n_seq + 1)
    blob = data[at:]
    if off[0] != 0 or int(off[-1]) != links or np.any(off[1:] < off[:-1]):
        raise Hash10xError("%s: the offsets do not ascend from 0 to the %d links" % (path, links))
    if name_off[0] != 0 or int(name_off[-1]) != name_bytes or np.any(name_off[1:] <= name_off[:-1]):
        raise Hash10xError("%s: the name offsets do not ascend from 0 to the %d name bytes" % (path, name_bytes))
    if any(blob[int(e) - 1] != 0 for e in name_off[1:]):
        raise Hash10xError("%s: a name does not end in NUL" % path)
    other, shared = pairs[:, 0].copy(), pairs[:, 1].copy()
    if links:
        own = np.repeat(np.arange(n_ends, dtype=np.int64), np.diff(off.astype(np.int64)))
        if int(other.max()) >= n_ends:
            raise Hash10xError("%s: a link's end is beyond the %d ends" % (path, n_ends))
        if np.any(other.astype(np.int64) <= own):
            raise Hash10xError("%s: a link's end is not above its row's own end" % path)
        if np.any((other.astype(np.int64) >> 1) == (own >> 1)):
            raise Hash10xError("%s: a link joins the two ends of one sequence" % path)
        if np.any((own[1:] == own[:-1]) & (other[1:] <= other[:-1])):
            raise Hash10xError("%s: the ends of a row do not ascend" % path)
        if int(shared.min()) < max(min_blocks, 1):
            raise Hash10xError("%s: a link shares fewer than minBlocks %d" % (path, min_blocks))
    names = [blob[int(a):int(b) - 1].decode(errors="replace") for a, b in zip(name_off[:-1], name_off[1:])]
    info = {"version": version, "nBlocks": n_blocks, "minShare": min_share, "minBlocks": min_blocks, "endLen": end_len, "maxEnds": max_ends, "nSeq": n_seq,
            "links": links, "skippedBlocks": skipped, "nameBytes": name_bytes}
    return info, off, other, shared, table, names


def symmetric_links(offsets, other, shared):
    """The upper-triangle rows of row_links / seq_links / read_seq_links as full rows: (offsets uint64[n + 1], other uint32[], shared uint32[])
    in which list e stands in the row of f wherever f stands in the row of e, every row ascending."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    e = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    f = np.asarray(other, dtype=np.int64)
    a, b, c = np.concatenate([e, f]), np.concatenate([f, e]), np.concatenate([np.asarray(shared, dtype=np.uint32)] * 2)
    order = np.lexsort((b, a))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(a, minlength=n)[:n])
    return off, b[order].astype(np.uint32), c[order]


_SHARE_COMPONENTS_INFO = np.dtype([("rows", "<u8"), ("listEntries", "<u8"), ("nBlocks", "<u4"), ("minShare", "<u4"), ("nComponents", "<u4"), ("largest", "<u4"),
                                   ("singletons", "<u4"), ("batches", "<u4"), ("windows", "<u4"), ("hookRounds", "<u4")])
_SC_ENTRY = np.dtype([("root", "<u4"), ("blocks", "<u4"), ("records", "<u8")])


def read_share_components(path):
    """A --shareComponents file (magic "10XC", u32 version 1, u32 nBlocks, u32 minShare, u32 nComponents, u32 largest, u64 rows,
    comp[nBlocks] as u32, nComponents + 1 entries {u32 root, u32 blocks, u64 records}, little-endian; needs no device):
    ({"version", "nBlocks", "minShare", "nComponents", "largest", "rows"}, comp, rootOf, blocks, records). Raises Hash10xError for a file
    that is not one or does not hold together: lengths, comp < nComponents + 1, the member counts summing to nBlocks - 1, rootOf ascending."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 32 or data[:4] != b"10XC":
        raise Hash10xError("%s: not a share components file (magic 10XC)" % path)
    version, n_blocks, min_share, n_comp, largest = (int(v) for v in np.frombuffer(data, dtype="<u4", count=5, offset=4))
    rows = int(np.frombuffer(data, dtype="<u8", count=1, offset=24)[0])
    if version != 1:
        raise Hash10xError("%s: share components version %d, this reader knows 1" % (path, version))
    need = 32 + 4 * n_blocks + 16 * (n_comp + 1)
    if len(data) != need:
        raise Hash10xError("%s: %d bytes, %d blocks and %d components need %d" % (path, len(data), n_blocks, n_comp, need))
    comp = np.frombuffer(data, dtype="<u4", count=n_blocks, offset=32).copy()
    ent = np.frombuffer(data, dtype=_SC_ENTRY, count=n_comp + 1, offset=32 + 4 * n_blocks)
    root_of, blocks, records = ent["root"].copy(), ent["blocks"].copy(), ent["records"].copy()
    if n_blocks and int(comp.max()) >= n_comp + 1:
        raise Hash10xError("%s: a block's component is beyond the %d components" % (path, n_comp))
    if int(blocks.sum(dtype=np.uint64)) != max(n_blocks - 1, 0) or blocks[0] != 0:
        raise Hash10xError("%s: the components' member counts do not sum to the %d blocks" % (path, max(n_blocks - 1, 0)))
    if root_of[0] != 0 or np.any(root_of[1:] <= root_of[:-1]) or (n_comp and int(root_of[-1]) >= n_blocks):
        raise Hash10xError("%s: the components' roots do not ascend within the %d blocks" % (path, n_blocks))
    return ({"version": version, "nBlocks": n_blocks, "minShare": min_share, "nComponents": n_comp, "largest": largest, "rows": rows},
            comp, root_of, blocks, records)


_HASH_COPIES_INFO = np.dtype([("inRange", "<u8"), ("rows", "<u8"), ("listEntries", "<u8"), ("oneGroup", "<u8"), ("split", "<u8"), ("hashNumber", "<u4"),
                              ("minShare", "<u4"), ("deepest", "<u4"), ("batches", "<u4"), ("windows", "<u4"), ("reserved", "<u4")])


_STATE_MOSH_INFO = np.dtype([("kept", "<u8"), ("copy", "<u8", (4,)), ("toM", "<u8"), ("to0", "<u8"), ("saturated", "<u8"), ("crib", "<u8", (5, 4)),
                             ("hashNumber", "<u4"), ("bits", "<u4"), ("minShare", "<u4"), ("reserved", "<u4")])   # h10x_state_mosh_info


def _state_mosh_info(z):
    return {n: (z[n][0].tolist() if z[n][0].ndim else int(z[n][0])) for n in _STATE_MOSH_INFO.names if n != "reserved"}


def read_hash_copies(path):
    """A --hashCopies file (magic "10XK", u32 version 1, u32 hashNumber, u32 minShare, u64 inRange, u64 rows, hashNumber records
    {u16 distinct, u16 groups, u16 largest, u16 second}, little-endian; needs no device): ({"version", "hashNumber", "minShare",
    "inRange", "rows"}, a (hashNumber, 4) uint16 array). Raises Hash10xError for a file that is not one or whose length is not what its
    header says."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 32 or data[:4] != b"10XK":
        raise Hash10xError("%s: not a hash copies file (magic 10XK)" % path)
    version, n_hash, min_share = (int(v) for v in np.frombuffer(data, dtype="<u4", count=3, offset=4))
    in_range, rows = (int(v) for v in np.frombuffer(data, dtype="<u8", count=2, offset=16))
    if version != 1:
        raise Hash10xError("%s: hash copies version %d, this reader knows 1" % (path, version))
    if len(data) != 32 + 8 * n_hash:
        raise Hash10xError("%s: %d bytes, %d hashes need %d" % (path, len(data), n_hash, 32 + 8 * n_hash))
    table = np.frombuffer(data, dtype="<u2", count=4 * n_hash, offset=32).reshape(-1, 4).copy()
    return {"version": version, "hashNumber": n_hash, "minShare": min_share, "inRange": in_range, "rows": rows}, table


# ---- mosh sets: the reference's moshutils (moshset.c, moshutils.c) on the GPU — csrc/stage_g.hip, host/mosh_host.c -------------------
def _from_ptr(ptr, dtype, n):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * (np.dtype(dtype).itemsize * n)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def read_sequences(path, slab=0):
    """A FASTA / FASTQ file (gzip or plain) through the host reader (seqio.c's rules; no device needed): returns
    (codes uint8, seq_start uint64 with nSeq + 1 entries, warning text). Raises Hash10xError with the reference's message."""
    _, host = load_native()
    msg = ctypes.create_string_buffer(512); fatal = ctypes.c_int(0)
    r = host.h10x_seq_open(os.fsencode(path), msg, 512, ctypes.byref(fatal))
    if not r:
        raise Hash10xError((msg.value.decode() + "\n" if msg.value and not fatal.value else "") +
                           (msg.value.decode() if fatal.value else "failed to open sequence file %s" % path))
    try:
        codes, starts = [], [np.zeros(1, np.uint64)]
        total = 0
        while True:
            c, st, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32(0)
            rc = host.h10x_seq_next(r, int(slab), ctypes.byref(c), ctypes.byref(st), ctypes.byref(n))
            if rc < 0:
                raise Hash10xError(host.h10x_seq_error(r).decode())
            if rc == 0:
                break
            s = _from_ptr(st.value, np.uint64, n.value + 1)
            codes.append(_from_ptr(c.value, np.uint8, int(s[-1])))
            starts.append(s[1:] + np.uint64(total))
            total += int(s[-1])
        return (np.concatenate(codes) if codes else np.zeros(0, np.uint8)), np.concatenate(starts), host.h10x_seq_warning(r).decode()
    finally:
        host.h10x_seq_close(r)


def read_mosh_file(path):
    """A MSHSTv1 file through the host reader's checks: dict with B, size, k, w, factor1, factor2, index, value, depth, info."""
    _, host = load_native()
    m = _MoshFile(); err = ctypes.create_string_buffer(512)
    if host.h10x_moshfile_read(os.fsencode(path), ctypes.byref(m), err, 512):
        raise Hash10xError(err.value.decode())
    try:
        return dict(B=m.B, size=m.size, k=m.sh.k, w=m.sh.w, factor1=m.sh.factor1, factor2=m.sh.factor2,
                    index=_from_ptr(m.index, np.uint32, 1 << m.B), value=_from_ptr(m.value, np.uint64, m.size),
                    depth=_from_ptr(m.depth, np.uint16, m.size), info=_from_ptr(m.info, np.uint8, m.size))
    finally:
        host.h10x_moshfile_free(ctypes.byref(m))


class MoshSet:
    """The reference's Moshset on one MI355X: -c / -r / -w / -a / -x / -m / -p / -s / -sM / -H / -d of moshutils as methods."""

    def __init__(self, B=28, k=19, w=31, seed=17, device=0, _handle=None):
        self._hip, self._host = load_native()
        self.h = _handle
        if self.h is None:
            h = ctypes.c_void_p(); err = ctypes.create_string_buffer(512)
            if self._hip.h10x_mosh_create(ctypes.byref(h), B, k, w, seed, device, err, 512):
                raise Hash10xError(err.value.decode())
            self.h = h

    @classmethod
    def read(cls, path, device=0):
        """-r: a set read from a file is full (moshsetRead sizes the arrays to the file)"""
        f = read_mosh_file(path)
        return cls.from_arrays(f["B"], f["k"], f["w"], f["factor1"], f["factor2"], f["index"], f["value"], f["depth"], f["info"], device)

    @classmethod
    def from_arrays(cls, B, k, w, factor1, factor2, index, value, depth, info, device=0):
        hip, _ = load_native()
        index = np.ascontiguousarray(index, np.uint32); value = np.ascontiguousarray(value, np.uint64)
        depth = np.ascontiguousarray(depth, np.uint16); info = np.ascontiguousarray(info, np.uint8)
        assert len(index) == 1 << B and len(value) == len(depth) == len(info)
        h = ctypes.c_void_p(); err = ctypes.create_string_buffer(512)
        if hip.h10x_mosh_load(ctypes.byref(h), B, k, w, int(factor1), int(factor2), index.ctypes.data, value.ctypes.data, depth.ctypes.data,
                              info.ctypes.data, len(value), device, err, 512):
            raise Hash10xError(err.value.decode())
        return cls(_handle=h)

    def close(self):
        if getattr(self, "h", None):
            self._hip.h10x_mosh_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise Hash10xError(self._hip.h10x_mosh_error(self.h).decode())

    def info(self):
        i = _MoshInfo()
        self._hip.h10x_mosh_info(self.h, ctypes.byref(i))
        return i

    @property
    def max(self):
        return self.info().max

    def set_option(self, name, value):
        if self._hip.h10x_mosh_set_option(self.h, name.encode(), int(value)):
            raise Hash10xError("unknown mosh option %s, or a value outside its range" % name)

    def counters(self):
        """dict: scan_retries = device batches of add / scan (and of a ReadSet's or RefMap's over this set) whose list overflowed its estimated
        size and were scanned a second time"""
        c = _MoshCounters()
        self._hip.h10x_mosh_counters(self.h, ctypes.byref(c))
        return {"scan_retries": int(c.scan_retries)}

    @staticmethod
    def _seqs(codes, seq_start):
        c = np.ascontiguousarray(codes, np.uint8); s = np.ascontiguousarray(seq_start, np.uint64)
        assert len(s) >= 1 and int(s[-1]) <= len(c)
        return c, s

    def add(self, codes, seq_start, is10x=False, seq_base=0):
        """-a / -x over sequences in memory; returns the number of mosh occurrences"""
        c, s = self._seqs(codes, seq_start)
        n = ctypes.c_uint64(0)
        self._chk(self._hip.h10x_mosh_add(self.h, c.ctypes.data, s.ctypes.data, len(s) - 1, int(bool(is10x)), int(seq_base), ctypes.byref(n)))
        return n.value

    def add_file(self, path, is10x=False, slab=0):
        """-a / -x of a sequence file: (sequences, bases, occurrences, warning)"""
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        msg = ctypes.create_string_buffer(512); warn = ctypes.create_string_buffer(256)
        rc = self._host.h10x_mosh_set_add_file(self.h, os.fsencode(path), int(bool(is10x)), int(slab), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), msg, 512, warn, 256)
        if rc > 0:
            raise Hash10xError((msg.value.decode() + "\n" if msg.value else "") + "failed to open sequence file %s" % path)
        if rc < 0:
            raise Hash10xError(msg.value.decode())
        return a.value, b.value, c.value, warn.value.decode()

    def scan(self, codes, seq_start, is10x=False, seq_base=0):
        """every mosh of the sequences in order: (hash uint64, sequence uint32, position uint32); the set is not changed"""
        c, s = self._seqs(codes, seq_start)
        n = ctypes.c_uint64(0)
        cap = max(1024, 2 * len(c) // max(1, self.info().w) + 1024)
        while True:
            h = np.zeros(cap, np.uint64); q = np.zeros(cap, np.uint32); p = np.zeros(cap, np.uint32)
            self._chk(self._hip.h10x_mosh_scan(self.h, c.ctypes.data, s.ctypes.data, len(s) - 1, int(bool(is10x)), int(seq_base),
                                               h.ctypes.data, q.ctypes.data, p.ctypes.data, cap, ctypes.byref(n)))
            if n.value <= cap:
                return h[:n.value], q[:n.value], p[:n.value]
            cap = n.value

    def merge_arrays(self, k, w, factor1, value, depth, info):
        value = np.ascontiguousarray(value, np.uint64); depth = np.ascontiguousarray(depth, np.uint16); info = np.ascontiguousarray(info, np.uint8)
        ok = ctypes.c_int(0)
        self._chk(self._hip.h10x_mosh_merge(self.h, k, w, int(factor1), value.ctypes.data, depth.ctypes.data, info.ctypes.data, len(value), ctypes.byref(ok)))
        return bool(ok.value)

    def merge(self, path):
        """-m: False when the file's k, w or factor1 differ (nothing merged)"""
        f = read_mosh_file(path)
        return self.merge_arrays(f["k"], f["w"], f["factor1"], f["value"], f["depth"], f["info"])

    def prune(self, lo, hi):
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._chk(self._hip.h10x_mosh_prune(self.h, lo, hi, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_copy(self, c1, c2, cM):
        self._chk(self._hip.h10x_mosh_set_copy(self.h, c1, c2, cM))

    def set_copy_m(self, cM):
        self._chk(self._hip.h10x_mosh_set_copy_m(self.h, cM))

    def hist(self):
        """(depth histogram with 65536 bins, the four copy counts)"""
        h = np.zeros(65536, np.uint32); c = np.zeros(4, np.uint32)
        self._chk(self._hip.h10x_mosh_summary(self.h, h.ctypes.data, c.ctypes.data))
        return h, c

    def export(self, index=True):
        """(index or None, value, depth, info) as moshsetWrite stores them"""
        i = self.info()
        ix = np.zeros(1 << i.B, np.uint32) if index else None
        v = np.zeros(i.max + 1, np.uint64); d = np.zeros(i.max + 1, np.uint16); f = np.zeros(i.max + 1, np.uint8)
        self._chk(self._hip.h10x_mosh_export(self.h, 0, len(ix) if index else 0, ix.ctypes.data if index else None, v.ctypes.data, d.ctypes.data, f.ctypes.data))
        return ix, v, d, f

    def lookup(self, hashes):
        """(index, depth) per hash; 0, 0 where the set does not hold it"""
        q = np.ascontiguousarray(hashes, np.uint64)
        ix = np.zeros(len(q), np.uint32); d = np.zeros(len(q), np.uint16)
        self._chk(self._hip.h10x_mosh_lookup(self.h, q.ctypes.data, len(q), ix.ctypes.data, d.ctypes.data))
        return ix, d

    def write(self, path):
        err = ctypes.create_string_buffer(512)
        if self._host.h10x_mosh_set_write(self.h, os.fsencode(path), err, 512):
            raise Hash10xError(err.value.decode())


def mosh_scan(codes, seq_start, k, w, seed, device=0):
    """The moshes of these sequences as the reference's moshRCiterator yields them: (hash, sequence, position)."""
    s = MoshSet(B=20, k=k, w=w, seed=seed, device=device)
    try:
        return s.scan(codes, seq_start)
    finally:
        s.close()


# ---- readsets: the reference's moshasm (moshasm.c) on the GPU — csrc/stage_h.hip, host/asm_host.c --------------------------------
def read_readset_file(path, set_max):
    """A RSMSHv2 file through the host reader's checks (no device needed): dict with totHit, dim, reads (READ_DTYPE), hit, dx."""
    _, host = load_native()
    r = _ReadsetFile(); err = ctypes.create_string_buffer(512)
    if host.h10x_readsetfile_read(os.fsencode(path), int(set_max), ctypes.byref(r), err, 512):
        raise Hash10xError(err.value.decode())
    try:
        return dict(totHit=r.totHit, dim=r.dim, reads=_from_ptr(r.reads, READ_DTYPE, r.max), hit=_from_ptr(r.hit, np.uint32, r.totHit), dx=_from_ptr(r.dx, np.uint16, r.totHit))
    finally:
        host.h10x_readsetfile_free(ctypes.byref(r))


def write_readset_file(path, tot_hit, dim, reads, hit_start, hit, dx):
    _, host = load_native()
    reads = np.ascontiguousarray(reads, READ_DTYPE); hs = np.ascontiguousarray(hit_start, np.uint64)
    hit = np.ascontiguousarray(hit, np.uint32); dx = np.ascontiguousarray(dx, np.uint16)
    assert len(hs) == len(reads) + 1 and int(hs[-1]) <= len(hit) and len(hit) == len(dx)
    err = ctypes.create_string_buffer(512)
    if host.h10x_readsetfile_write(os.fsencode(path), int(tot_hit), int(dim), reads.ctypes.data, len(reads), hs.ctypes.data, hit.ctypes.data, dx.ctypes.data, err, 512):
        raise Hash10xError(err.value.decode())


class ReadSet:
    """The reference's Readset over a MoshSet on one MI355X: -f / -r / -w / -S / -o1 / -b / -c of moshasm as methods. The readset borrows
    the set: keep the set open while the readset lives. A new ReadSet zeroes the set's depths, which its reads then rebuild."""

    def __init__(self, moshset, _handle=None):
        self._hip, self._host = load_native()
        self.ms = moshset
        self.h = _handle
        if self.h is None:
            h = ctypes.c_void_p()
            if self._hip.h10x_readset_create(ctypes.byref(h), moshset.h):
                raise Hash10xError(self._hip.h10x_mosh_error(moshset.h).decode())
            self.h = h

    @classmethod
    def from_arrays(cls, moshset, reads, dim, hit, dx):
        hip, _ = load_native()
        reads = np.ascontiguousarray(reads, READ_DTYPE); hit = np.ascontiguousarray(hit, np.uint32); dx = np.ascontiguousarray(dx, np.uint16)
        h = ctypes.c_void_p()
        if hip.h10x_readset_load(ctypes.byref(h), moshset.h, reads.ctypes.data, len(reads), int(dim), hit.ctypes.data, dx.ctypes.data):
            raise Hash10xError(hip.h10x_mosh_error(moshset.h).decode())
        rs = cls(moshset, _handle=h)
        rs.export()                                             # invBuild: the set's depths must be this readset's
        return rs

    @classmethod
    def read(cls, stem, device=0):
        """-r: <stem>.mosh and <stem>.readset; returns the ReadSet (its set is .ms)"""
        f = read_mosh_file(stem + ".mosh")
        r = read_readset_file(stem + ".readset", f["size"] - 1)
        ms = MoshSet.from_arrays(f["B"], f["k"], f["w"], f["factor1"], f["factor2"], f["index"], f["value"], f["depth"], f["info"], device)
        return cls.from_arrays(ms, r["reads"], r["dim"], r["hit"], r["dx"])

    def close(self):
        if getattr(self, "h", None):
            self._hip.h10x_readset_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise Hash10xError(self._hip.h10x_readset_error(self.h).decode())

    def info(self):
        i = _ReadsetInfo()
        self._chk(self._hip.h10x_readset_info(self.h, ctypes.byref(i)))
        n = ctypes.c_uint32(0)
        self._hip.h10x_readset_chunks(self.h, ctypes.byref(n))
        i.chunks = n.value                                      # chunks of queries of the overlap table as built; 0 = no table yet (set options "overlap_chunk", "overlap_chunk_reads")
        return i

    def add(self, codes, seq_start):
        """the reads of -f from memory, appended in order"""
        c, s = MoshSet._seqs(codes, seq_start)
        self._chk(self._hip.h10x_readset_add(self.h, c.ctypes.data, s.ctypes.data, len(s) - 1))

    def add_file(self, path, slab=0):
        """-f: returns the reader's warning text"""
        msg = ctypes.create_string_buffer(512); warn = ctypes.create_string_buffer(256)
        rc = self._host.h10x_readset_add_file(self.h, os.fsencode(path), int(slab), msg, 512, warn, 256)
        if rc > 0:
            raise Hash10xError((msg.value.decode() + "\n" if msg.value else "") + "failed to open sequence file %s" % path)
        if rc < 0:
            raise Hash10xError(msg.value.decode())
        return warn.value.decode()

    def export(self):
        """(reads as READ_DTYPE records, hit_start uint64, hit uint32, dx uint16): what -w stores"""
        i = self.info()
        r, s, h, d = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(self._hip.h10x_readset_export(self.h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(h), ctypes.byref(d)))
        return (_from_ptr(r.value, READ_DTYPE, i.nReads), _from_ptr(s.value, np.uint64, i.nReads + 1), _from_ptr(h.value, np.uint32, i.totHit),
                _from_ptr(d.value, np.uint16, i.totHit))

    def write(self, stem):
        """-w: <stem>.mosh and <stem>.readset"""
        self.ms.write(stem + ".mosh")
        err = ctypes.create_string_buffer(512)
        if self._host.h10x_readset_write_file(self.h, os.fsencode(stem + ".readset"), err, 512):
            raise Hash10xError(err.value.decode())

    def stats(self):
        """the sums of -S: dict with reads (records), totHit and, per copy class, nCopy, hitCopy, hit2Copy, depthCopy of the set"""
        s = np.zeros(16, np.uint64)
        self._chk(self._hip.h10x_readset_stats_sums(self.h, s.ctypes.data))
        return dict(reads=self.export()[0], totHit=self.info().totHit, nCopy=s[0:4], hitCopy=s[4:8], hit2Copy=s[8:12], depthCopy=s[12:16])

    def overlaps(self, ix):
        """findOverlaps for read ix, flags of ix updated as it does: (array of OVERLAP_DTYPE, nRepeat, nGood, nBad)"""
        cap = ctypes.c_uint32(0); n = ctypes.c_uint32(0)
        self._chk(self._hip.h10x_readset_overlap_cap(self.h, int(ix), ctypes.byref(cap)))
        out = np.zeros(cap.value, OVERLAP_DTYPE); cnt = np.zeros(3, np.int32)
        self._chk(self._hip.h10x_readset_overlaps(self.h, int(ix), out.ctypes.data, cap.value, ctypes.byref(n), cnt.ctypes.data))
        return out[:n.value], int(cnt[0]), int(cnt[1]), int(cnt[2])

    def mark_bad(self):
        """-b: the reads each of the three passes marks"""
        f = np.zeros(3, np.int32)
        self._chk(self._hip.h10x_readset_mark_bad(self.h, f.ctypes.data))
        return [int(x) for x in f]

    def mark_contained(self):
        """-c: (contained, not contained, total length of the reads not contained)"""
        a, b, t = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_uint64(0)
        self._chk(self._hip.h10x_readset_mark_contained(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t)))
        return a.value, b.value, t.value


# ---- reference maps: the Reference of the reference's moshmap (moshmap.c) on the GPU — csrc/stage_i.hip ------------------------------------
MAPSEED_DTYPE = np.dtype([("loc", "<u4"), ("loc2", "<u4"), ("idClass", "<u4"), ("id2", "<u4")])
MAPREC_DTYPE = np.dtype([("pos0", "<u4"), ("posN", "<u4"), ("loc0", "<u4"), ("locN", "<u4"), ("n1", "<u4"), ("n2", "<u4"), ("query", "<u4")])


class RefMap:
    """The reference's Reference over a MoshSet on one MI355X: the loop of -f (add), its end (pack) and -q (query) of moshmap as methods.
    The map borrows the set: keep the set open while the map lives (closing the set first leaves the map's handle unreleased: close() then
    only forgets it). A new RefMap needs a set whose 16-bit depths are all 0, as MoshSet(...) leaves them — add() keeps them 0, the counts
    live in the map's own 32-bit depth — and is refused over any other. Names and lengths of the sequences are the caller's."""

    def __init__(self, moshset, size=1 << 26, _handle=None):
        self._hip, self._host = load_native()
        self.ms = moshset
        self.h = _handle
        if self.h is None:
            h = ctypes.c_void_p()
            if self._hip.h10x_refmap_create(ctypes.byref(h), moshset.h, int(size)):
                raise Hash10xError(self._hip.h10x_mosh_error(moshset.h).decode())
            self.h = h

    @classmethod
    def from_arrays(cls, moshset, index, offset, id, depth, rev, loc, n_ids):
        """-r: the arrays of a .ref file over the set of its .mosh file"""
        hip, _ = load_native()
        a = [np.ascontiguousarray(x, np.uint32) for x in (index, offset, id, depth, rev, loc)]
        assert len(a[0]) == len(a[1]) == len(a[2]) == len(a[4]) and len(a[3]) == len(a[5]) == moshset.max + 1
        h = ctypes.c_void_p()
        if hip.h10x_refmap_load(ctypes.byref(h), moshset.h, *[x.ctypes.data for x in a], len(a[0]), int(n_ids)):
            raise Hash10xError(hip.h10x_mosh_error(moshset.h).decode())
        return cls(moshset, _handle=h)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ms, "h", None):     # (the destroy reads the set: not after the set is gone)
            self._hip.h10x_refmap_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise Hash10xError(self._hip.h10x_refmap_error(self.h).decode())

    def info(self):
        i = _RefmapInfo()
        self._chk(self._hip.h10x_refmap_info(self.h, ctypes.byref(i)))
        return i

    def add(self, codes, seq_start, id_base=0):
        """the reference sequences of -f from memory, appended in order; returns the hits appended"""
        c, s = MoshSet._seqs(codes, seq_start)
        n = ctypes.c_uint64(0)
        self._chk(self._hip.h10x_refmap_add(self.h, c.ctypes.data, s.ctypes.data, len(s) - 1, int(id_base), ctypes.byref(n)))
        return n.value

    def pack(self):
        """copy classes, loc and rev: (copy 1, copy 2, multiple)"""
        a, b, c = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._chk(self._hip.h10x_refmap_pack(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def export(self):
        """dict of index, offset, id, rev (max entries) and depth, loc (the set's max + 1): what -w stores"""
        i = self.info()
        p = [ctypes.c_void_p() for _ in range(6)]
        self._chk(self._hip.h10x_refmap_export(self.h, *[ctypes.byref(x) for x in p]))
        n = dict(index=i.max, offset=i.max, id=i.max, depth=i.setMax + 1, rev=i.max, loc=i.setMax + 1)
        return {k: _from_ptr(x.value, np.uint32, n[k]) for k, x in zip(("index", "offset", "id", "depth", "rev", "loc"), p)}

    def query(self, codes, seq_start, seeds=False):
        """-q over sequences in memory: dict of counts (n x 4: missed, copy 1, copy 2, multi), rec_start (n + 1), recs (MAPREC_DTYPE) and,
        with seeds=True, seed_start, seeds (MAPSEED_DTYPE), seed_pos"""
        c, s = MoshSet._seqs(codes, seq_start)
        self._chk(self._hip.h10x_refmap_query(self.h, c.ctypes.data, s.ctypes.data, len(s) - 1, int(bool(seeds))))
        n = ctypes.c_uint32(0)
        p = [ctypes.c_void_p() for _ in range(6)]
        self._chk(self._hip.h10x_refmap_results(self.h, ctypes.byref(n), *[ctypes.byref(x) for x in p]))
        rec_start = _from_ptr(p[1].value, np.uint64, n.value + 1)
        out = dict(counts=_from_ptr(p[0].value, np.uint32, 4 * n.value).reshape(-1, 4), rec_start=rec_start, recs=_from_ptr(p[2].value, MAPREC_DTYPE, int(rec_start[-1])))
        if seeds:
            out["seed_start"] = _from_ptr(p[3].value, np.uint64, n.value + 1)
            out["seeds"] = _from_ptr(p[4].value, MAPSEED_DTYPE, int(out["seed_start"][-1]))
            out["seed_pos"] = _from_ptr(p[5].value, np.uint32, int(out["seed_start"][-1]))
        return out
