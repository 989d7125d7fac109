"""ctypes binding of libmdeflate.so (the C ABI of include/mdeflate.h).

There is no fallback: if the HIP library is missing this module raises, and
every compute call goes through the .so.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MD_LIBMDEFLATE: another build of the same library (measurement builds of tools/dbg; there is still no fallback)
SO = os.environ.get("MD_LIBMDEFLATE") or os.path.join(HERE, "libmdeflate.so")

c_sz = ctypes.c_size_t
c_u8p = ctypes.c_void_p
c_vp = ctypes.c_void_p
MD_STREAM_NULL = ctypes.c_void_p(-1).value  # md_create: enqueue on the legacy default stream

class GzHeader(ctypes.Structure):
    """md_gz_header of include/mdeflate.h"""
    _fields_ = [("mtime", ctypes.c_uint32), ("os", ctypes.c_int), ("hcrc", ctypes.c_int), ("ascii", ctypes.c_int),
                ("filename", ctypes.c_char_p), ("comment", ctypes.c_char_p)]


class InfResume(ctypes.Structure):
    """md_inf_resume (mdeflate.h): the last block boundary inside a piece of a stream"""
    _fields_ = [("bits", ctypes.c_uint64), ("out", ctypes.c_uint64), ("adler", ctypes.c_uint32), ("last", ctypes.c_uint32),
                ("consumed", ctypes.c_uint64), ("checksum", ctypes.c_uint32), ("crc_out", ctypes.c_uint32), ("crc_end", ctypes.c_uint32)]


class DeflateParams(ctypes.Structure):
    """md_deflate_params of include/mdeflate.h"""
    _fields_ = [("level", ctypes.c_int), ("queue_len", ctypes.c_int), ("driver", ctypes.c_int), ("dynamic", ctypes.c_int),
                ("matcher", ctypes.c_int), ("gz_header", ctypes.POINTER(GzHeader)), ("wbits", ctypes.c_int),
                ("total_in_bytes", ctypes.c_size_t)]


c_pp = ctypes.POINTER(DeflateParams)
c_szp = ctypes.POINTER(c_sz)

# every symbol include/mdeflate.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("md_version", ctypes.c_int, []),
    ("md_status_string", ctypes.c_char_p, [ctypes.c_int]),
    ("md_shard_plan", ctypes.c_int, [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("md_last_error_string", ctypes.c_char_p, [c_vp]),
    ("md_device_count", ctypes.c_int, []),
    ("md_create", c_vp, [ctypes.c_int, c_vp]),
    ("md_destroy", None, [c_vp]),
    ("md_synchronize", ctypes.c_int, [c_vp]),
    ("md_set_option", ctypes.c_int, [c_vp, ctypes.c_char_p, ctypes.c_int]),
    ("md_def_batch_open", c_vp, [c_vp, ctypes.c_int, c_pp, c_sz]),
    ("md_def_batch_src", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz]),
    ("md_def_batch_encode", ctypes.c_int, [c_vp]),
    ("md_def_batch_pending", c_sz, [c_vp, c_sz]),
    ("md_def_batch_out", c_sz, [c_vp, c_sz, c_vp, c_sz]),
    ("md_def_batch_status", ctypes.c_int, [c_vp, c_sz]),
    ("md_def_batch_error", ctypes.c_int, [c_vp, c_sz]),
    ("md_def_batch_checksum", ctypes.c_uint32, [c_vp, c_sz]),
    ("md_def_batch_close", None, [c_vp]),
    ("md_inf_batch_open", c_vp, [c_vp, ctypes.c_int, c_sz]),
    ("md_inf_batch_src", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz]),
    ("md_inf_batch_decode", ctypes.c_int, [c_vp]),
    ("md_inf_batch_pending", c_sz, [c_vp, c_sz]),
    ("md_inf_batch_out", c_sz, [c_vp, c_sz, c_vp, c_sz]),
    ("md_inf_batch_status", ctypes.c_int, [c_vp, c_sz]),
    ("md_inf_batch_error", ctypes.c_int, [c_vp, c_sz]),
    ("md_inf_batch_message", ctypes.c_char_p, [c_vp, c_sz]),
    ("md_inf_batch_checksum", ctypes.c_uint32, [c_vp, c_sz]),
    ("md_inf_batch_src_rem", c_sz, [c_vp, c_sz]),
    ("md_inf_batch_reset", None, [c_vp, c_sz]),
    ("md_inf_batch_close", None, [c_vp]),
    ("md_host_alloc", c_vp, [c_vp, c_sz]),
    ("md_host_free", None, [c_vp, c_vp]),
    ("md_timing_begin", ctypes.c_int, [c_vp]),
    ("md_timing_end", ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_float)]),
    ("md_inflate_batch_device", ctypes.c_int,
     [c_vp, ctypes.c_int, c_sz] + [c_vp] * 10),
    ("md_inflate_batch_host", ctypes.c_int,
     [c_vp, ctypes.c_int, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_inflate_sizes_batch_device", ctypes.c_int, [c_vp, ctypes.c_int, c_sz] + [c_vp] * 6),
    ("md_inflate_sizes_batch_host", ctypes.c_int, [c_vp, ctypes.c_int, c_sz, c_vp, c_sz] + [c_vp] * 5),
    ("md_inflate_plan_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    ("md_deflate_batch_device", ctypes.c_int, [c_vp, ctypes.c_int, c_pp, c_sz] + [c_vp] * 9),
    ("md_deflate_batch_host", ctypes.c_int,
     [c_vp, ctypes.c_int, c_pp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_de_higher_uncompress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_zl_higher_uncompress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_de_lz77_compress", ctypes.c_int,
     [c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, c_szp, c_vp, c_vp]),
    ("md_de_def_encode", ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_de_def_run", ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, c_szp, c_vp, c_sz, c_szp]),
    ("md_de_def_ns_deflate", ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_zl_def_ns_deflate", ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_de_def_ns_compress_bound", c_sz, [c_sz]),
    ("md_zl_def_ns_compress_bound", c_sz, [c_sz]),
    ("md_def_ns_batch_device", ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, c_sz, c_sz] + [c_vp] * 9),
    ("md_inf_decoder", c_vp, [c_vp, ctypes.c_int, c_vp, c_sz]),
    ("md_inf_src", ctypes.c_int, [c_vp, c_vp, c_sz, c_sz]),
    ("md_inf_decode", ctypes.c_int, [c_vp]),
    ("md_inf_flush", None, [c_vp]),
    ("md_inf_dst_rem", c_sz, [c_vp]),
    ("md_inf_src_rem", c_sz, [c_vp]),
    ("md_inf_status", ctypes.c_int, [c_vp]),
    ("md_inf_checksum", ctypes.c_uint32, [c_vp]),
    ("md_inf_free", None, [c_vp]),
    ("md_inf_reset", None, [c_vp]),
    ("md_inf_chunk_bytes", None, [c_vp, c_sz]),
    ("md_inflate_continue_batch_device", ctypes.c_int, [c_vp, c_sz] + [c_vp] * 17),
    ("md_de_inf_continue_host", ctypes.c_int, [c_vp, c_vp, c_sz, ctypes.c_uint, c_vp, c_sz, c_sz, ctypes.c_uint32, ctypes.c_uint, c_vp, c_vp, c_vp]),
    ("md_inf_message", ctypes.c_char_p, [c_vp]),
    ("md_def_encoder", c_vp, [c_vp, ctypes.c_int, c_pp, c_vp, c_sz]),
    ("md_def_src", ctypes.c_int, [c_vp, c_vp, c_sz, c_sz]),
    ("md_def_encode", ctypes.c_int, [c_vp]),
    ("md_def_dst", None, [c_vp, c_vp, c_sz]),
    ("md_def_dst_rem", c_sz, [c_vp]),
    ("md_def_status", ctypes.c_int, [c_vp]),
    ("md_def_checksum", ctypes.c_uint32, [c_vp]),
    ("md_def_free", None, [c_vp]),
    ("md_de_higher_compress", ctypes.c_int,
     [c_vp, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    ("md_zl_higher_compress", ctypes.c_int,
     [c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    ("md_de_inf_ns_inflate", ctypes.c_int,
     [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz), ctypes.POINTER(c_sz)]),
    ("md_zl_inf_ns_inflate", ctypes.c_int,
     [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz), ctypes.POINTER(c_sz)]),
    ("md_gz_higher_compress", ctypes.c_int,
     [c_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GzHeader), c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    ("md_gz_higher_uncompress", ctypes.c_int,
     [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz), ctypes.POINTER(c_sz), c_vp]),
    ("md_crc32_batch_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    ("md_lzo_uncompress_batch_device", ctypes.c_int, [c_vp, c_sz] + [c_vp] * 8),
    ("md_lzo_compress_batch_device", ctypes.c_int, [c_vp, c_sz] + [c_vp] * 8),
    ("md_lzo_uncompress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    ("md_lzo_compress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    ("md_lzo_sizes_batch_device", ctypes.c_int, [c_vp, c_sz] + [c_vp] * 5),
    ("md_lzo_sizes_batch_host", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz] + [c_vp] * 4),
    ("md_lzo_uncompress_with_buffer", ctypes.c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_vp), c_szp]),
    ("md_gz_members_scan", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_sz]),
    ("md_gz_members_uncompress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp]),
    ("md_gz_members_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_bgzf_compress_bound", c_sz, [c_sz, c_sz]),
    ("md_bgzf_compress", ctypes.c_int, [c_vp, ctypes.c_int, c_sz, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_deflate_spans_bound", c_sz, [ctypes.c_int, c_sz, c_sz, ctypes.POINTER(GzHeader)]),
    ("md_deflate_spans_host", ctypes.c_int, [c_vp, ctypes.c_int, c_pp, c_sz, c_vp, c_sz, c_vp, c_sz, c_szp, ctypes.POINTER(ctypes.c_uint32)]),
    ("md_deflate_spans_device", ctypes.c_int, [c_vp, ctypes.c_int, c_pp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    ("md_deflate_spans_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_zip_directory", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_sz]),
    ("md_zip_uncompress", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    ("md_zip_compress_bound", c_sz, [c_sz, c_vp]),
    ("md_zip_compress", ctypes.c_int, [c_vp, ctypes.c_int, c_sz, c_vp, c_vp, c_sz, c_vp, c_sz, c_szp]),
    ("md_inflate_index_build", ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_sz, ctypes.c_uint64, c_vp, c_sz, ctypes.POINTER(c_vp), c_vp]),
    ("md_inflate_index_get", ctypes.c_int, [c_vp, c_vp]),
    ("md_inflate_index_points", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz]),
    ("md_inflate_index_save_size", c_sz, [c_vp]),
    ("md_inflate_index_save", ctypes.c_int, [c_vp, c_vp, c_sz, c_szp]),
    ("md_inflate_index_load", ctypes.c_int, [c_vp, c_sz, ctypes.POINTER(c_vp)]),
    ("md_inflate_index_free", None, [c_vp]),
    ("md_inflate_index_read", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_inflate_index_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_bgzf_index_build", ctypes.c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    ("md_bgzf_index_from_gzi", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    ("md_bgzf_index_gzi_size", c_sz, [c_vp]),
    ("md_bgzf_index_to_gzi", ctypes.c_int, [c_vp, c_vp, c_sz, c_szp]),
    ("md_bgzf_index_get", ctypes.c_int, [c_vp, c_vp]),
    ("md_bgzf_index_entries", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz]),
    ("md_bgzf_index_free", None, [c_vp]),
    ("md_bgzf_read", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_bgzf_read_virtual", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_bgzf_read_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_index", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_sz]),
    ("md_pack_open", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    ("md_pack_get", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_objects", ctypes.c_int, [c_vp, c_vp, c_sz]),
    ("md_pack_find", ctypes.c_int64, [c_vp, c_vp]),
    ("md_pack_free", None, [c_vp]),
    ("md_pack_read", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.c_uint, c_vp, c_sz, c_vp, c_vp, c_vp]),
    ("md_pack_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_verify", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, ctypes.c_uint, c_vp, c_vp]),
    ("md_pack_check_trailers", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("md_pack_index_write", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_sz, c_szp]),
    ("md_pack_index_build", ctypes.c_int, [c_vp, c_vp, c_sz, ctypes.c_uint, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp]),
    ("md_pack_build_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_sha1_batch_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint64, c_vp]),
    ("md_sha1_batch_host", ctypes.c_int, [c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    ("md_sha1_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_delta_batch_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("md_pack_delta_batch_host", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    ("md_pack_write_bound", c_sz, [c_sz, c_vp]),
    ("md_pack_write", ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_uint, ctypes.c_uint32, c_sz, c_vp, c_vp, c_sz, c_vp, c_sz, c_szp, c_vp, c_vp]),
    ("md_pack_write_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_sketch_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    ("md_pack_sketch_host", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_sz, c_vp]),
    ("md_pack_delta_sizes_device", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    ("md_pack_delta_sizes_host", ctypes.c_int, [c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp]),
    ("md_pack_choose_bases", ctypes.c_int, [c_vp, ctypes.c_uint32, ctypes.c_uint32, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp]),
    ("md_pack_search_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_graph_build", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, ctypes.POINTER(c_vp)]),
    ("md_pack_graph_get", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_graph_edges", ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_sz]),
    ("md_pack_graph_status", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_reachable", ctypes.c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    ("md_pack_reach_last", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_graph_free", None, [c_vp]),
    ("md_pack_diff", ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, ctypes.c_uint, ctypes.POINTER(c_vp)]),
    ("md_pack_diff_get", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_diff_changes", ctypes.c_int, [c_vp, c_vp, c_sz, c_vp, c_sz]),
    ("md_pack_diff_status", ctypes.c_int, [c_vp, c_vp]),
    ("md_pack_diff_free", None, [c_vp]),
]


class InflateIndexInfo(ctypes.Structure):
    """md_inflate_index_info of include/mdeflate.h"""
    _fields_ = [("format", ctypes.c_int32), ("checksum", ctypes.c_uint32)] + \
               [(k, ctypes.c_uint64) for k in ("src_len", "header_len", "consumed", "size", "span", "points")]


class InflateIndexStats(ctypes.Structure):
    """md_inflate_index_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("pieces", "launches", "bytes_in", "bytes_windows", "bytes_scratch")]


class BgzfIndexInfo(ctypes.Structure):
    """md_bgzf_index_info of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("src_len", "members", "size")]


class BgzfReadStats(ctypes.Structure):
    """md_bgzf_read_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("members", "launches", "bytes_in", "bytes_scratch")]


class PackIndexEntry(ctypes.Structure):
    """md_pack_index_entry of include/mdeflate.h"""
    _fields_ = [("offset", ctypes.c_uint64), ("crc32", ctypes.c_uint32), ("name", ctypes.c_uint8 * 20)]


class PackIndexInfo(ctypes.Structure):
    """md_pack_index_info of include/mdeflate.h"""
    _fields_ = [("n", ctypes.c_uint64), ("has_64bit_table", ctypes.c_int), ("pack_checksum", ctypes.c_uint8 * 20)]


class PackInfo(ctypes.Structure):
    """md_pack_info of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "deltas", "max_depth", "total_size", "failed")]


class PackObject(ctypes.Structure):
    """md_pack_object of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("size", "offset", "packed_len", "base")] + \
               [("depth", ctypes.c_uint32), ("type", ctypes.c_uint32), ("status", ctypes.c_int32), ("name", ctypes.c_uint8 * 20)]


class PackResult(ctypes.Structure):
    """md_pack_result of include/mdeflate.h"""
    _fields_ = [("entries", c_sz), ("failed", c_sz), ("written", ctypes.c_uint64)]


class PackStats(ctypes.Structure):
    """md_pack_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("rounds", "inflate_launches", "apply_launches", "objects", "bytes_in", "apply_ns")]


class PackBuildResult(ctypes.Structure):
    """md_pack_build_result of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "failed", "idx_len", "bad_offset")] + [("bad_status", ctypes.c_int32)]


class PackBuildStats(ctypes.Structure):
    """md_pack_build_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("candidates", "generations", "rounds", "inflate_launches", "apply_launches", "objects", "bytes_in")]


class Sha1Stats(ctypes.Structure):
    """md_sha1_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("messages", "blocks", "launches", "device_ns")]


class PackDeltaPair(ctypes.Structure):
    """md_pack_delta_pair of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("base_off", "base_len", "tgt_off", "tgt_len", "out_off", "out_cap")]


class PackSource(ctypes.Structure):
    """md_pack_source of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("off", "len", "base")] + [("type", ctypes.c_uint32)]


class PackWriteResult(ctypes.Structure):
    """md_pack_write_result of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "deltas", "max_depth")]


class PackSearchStats(ctypes.Structure):
    """md_pack_search_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("featured", "pairs", "fitted", "chosen", "launches", "sketch_ns", "score_ns", "host_ns")]


class PackGraphInfo(ctypes.Structure):
    """md_pack_graph_info of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "edges", "absent", "mistyped", "malformed", "failed", "parsed", "rounds", "parse_launches",
                                                "device_ns")]


class TreeChange(ctypes.Structure):
    """md_tree_change of include/mdeflate.h"""
    _fields_ = [("pair", ctypes.c_uint32), ("parent", ctypes.c_uint32), ("kind", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("a_mode", ctypes.c_uint32), ("b_mode", ctypes.c_uint32), ("a_obj", ctypes.c_uint32), ("b_obj", ctypes.c_uint32),
                ("name_len", ctypes.c_uint32), ("name_off", ctypes.c_uint64), ("a_name", ctypes.c_uint8 * 20), ("b_name", ctypes.c_uint8 * 20)]


class PackDiffInfo(ctypes.Structure):
    """md_pack_diff_info of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("pairs", "changes", "name_bytes", "levels", "opaque", "failed", "trees_read", "launches", "device_ns")]


class PackReachStats(ctypes.Structure):
    """md_pack_reach_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("host_closed", "seeds", "rounds", "expanded", "marked", "device_ns")]


class PackWriteStats(ctypes.Structure):
    """md_pack_write_stats of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("pairs", "kept", "dropped_size", "dropped_depth", "payload_before", "payload_after", "launches",
                                                "delta_ns")]


class ZipEntry(ctypes.Structure):
    """md_zip_entry of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("header_off", "csize", "usize", "name_off")] + \
               [(k, ctypes.c_uint32) for k in ("crc32", "external_attr")] + \
               [(k, ctypes.c_uint16) for k in ("name_len", "method", "flags", "dos_time", "dos_date")] + \
               [("reserved", ctypes.c_uint16 * 3)]


class ZipInfo(ctypes.Structure):
    """md_zip_info of include/mdeflate.h"""
    _fields_ = [("entries", c_sz)] + [(k, ctypes.c_uint64) for k in ("total_usize", "dir_off", "dir_size", "prefix", "comment_off")] + \
               [("comment_len", ctypes.c_uint32), ("zip64", ctypes.c_int)]


class ZipResult(ctypes.Structure):
    """md_zip_result of include/mdeflate.h"""
    _fields_ = [("entries", c_sz), ("failed", c_sz), ("written", ctypes.c_uint64)]


class ZipSource(ctypes.Structure):
    """md_zip_source of include/mdeflate.h"""
    _fields_ = [("name", ctypes.c_char_p), ("name_len", c_sz), ("off", ctypes.c_uint64), ("len", ctypes.c_uint64),
                ("external_attr", ctypes.c_uint32), ("dos_time", ctypes.c_uint16), ("dos_date", ctypes.c_uint16)]


class GzMembersInfo(ctypes.Structure):
    """md_gz_members_info of include/mdeflate.h"""
    _fields_ = [("members", c_sz), ("consumed", c_sz), ("written", c_sz), ("indexed", ctypes.c_int)]


class GzMembersStats(ctypes.Structure):
    """md_gz_members_stats of include/mdeflate.h"""
    _fields_ = [("path", ctypes.c_int)] + [(k, c_sz) for k in ("candidates", "spans_decoded", "members_device", "members_host",
                                                                "spans_long", "spans_no_room", "spans_implausible")]


class DeflateSpansInfo(ctypes.Structure):
    """md_deflate_spans_info of include/mdeflate.h"""
    _fields_ = [(k, c_sz) for k in ("spans", "stored_spans", "span_bytes")]


class GzMeta(ctypes.Structure):
    """md_gz_meta of include/mdeflate.h"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("flg", "mtime", "xfl", "os")] + \
               [(k, ctypes.c_int) for k in ("has_extra", "has_name", "has_comment")] + \
               [(k, c_sz) for k in ("extra_off", "extra_len", "name_off", "name_len", "comment_off", "comment_len")]
# exported but not part of the public header (tuning knobs)
EXTRA = [("md_get_profile", ctypes.c_int, [c_vp, c_vp]), ("md_i_link_segments", ctypes.c_int, [c_vp]),
         ("md_i_inf_batch_launches", ctypes.c_longlong, [c_vp]), ("md_i_inf_batch_attempts", ctypes.c_longlong, [c_vp, c_sz])]

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(
                "decompress_amd: %s is missing — build it with "
                "`python -m decompress_amd.build` (there is no CPU fallback)" % SO)
        lib = ctypes.CDLL(SO)
        for name, res, args in SYMBOLS + EXTRA:
            fn = getattr(lib, name)  # AttributeError = ABI drift: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
