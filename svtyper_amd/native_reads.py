"""ctypes binding of the native BAM reader + fragment summariser (include/svtyper_reads.h).

`NativeBam` offers the handful of `pysam.AlignmentFile` attributes the library / sample layer needs
(header['RG'], references, lengths, gettid) and `summarise()`, which fetches, assembles and
condenses the read-fragments of many (breakpoint, sample) units in C++ threads.  The summaries feed
the device geometry stage directly (`geometry="device"`), so with `reader="native"` no per-read
Python object is created at all.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import hip
from .geometry import BREAKPOINT_DTYPE, FRAGMENT_DTYPE

FETCH_DTYPE = np.dtype([("tid_a", "<i4"), ("lo_a", "<i4"), ("hi_a", "<i4"),
                        ("tid_b", "<i4"), ("lo_b", "<i4"), ("hi_b", "<i4")])
assert FETCH_DTYPE.itemsize == 24

COUNT_CLASSIC, COUNT_SSO = 0, 1


class _Args(C.Structure):
    _fields_ = [("n_units", C.c_uint64), ("windows", C.c_void_p), ("breakpoints", C.c_void_p),
                ("n_read_groups", C.c_uint32), ("read_groups", C.POINTER(C.c_char_p)),
                ("read_group_lib", C.POINTER(C.c_int32)), ("max_reads", C.c_int64), ("count_mode", C.c_int32),
                ("n_threads", C.c_int32)]


class _Summaries(C.Structure):
    _fields_ = [("frag_offset", C.POINTER(C.c_uint64)), ("fragments", C.c_void_p), ("skipped", C.POINTER(C.c_uint8))]


class _EvidenceParams(C.Structure):
    _fields_ = [("n_libs", C.c_uint32), ("lib_flank", C.POINTER(C.c_double)), ("min_aligned", C.c_int32), ("split_slop", C.c_int32)]


class _Evidence(C.Structure):
    _fields_ = [("rec_offset", C.POINTER(C.c_uint64)), ("records", C.c_void_p), ("skipped", C.POINTER(C.c_uint8))]


class _LibraryScan(C.Structure):
    _fields_ = [("read_length", C.c_int64), ("in_lib", C.c_uint64), ("total", C.c_uint64), ("n_hist", C.c_uint64),
                ("hist_keys", C.POINTER(C.c_int64)), ("hist_counts", C.POINTER(C.c_uint64))]


LIBSCAN_REASONS = {0: None, 1: "no_index", 2: "tables", 3: "record", 4: "overflow", 5: "member", 6: "no_rg", 7: "index"}
LIBSCAN_CAPACITIES = ("libraries", "read_groups", "dense_keys", "overflow", "record", "round_bytes")


class _LibraryScanStats(C.Structure):
    """include/svtyper_reads.h: svt_library_scan_stats"""
    _fields_ = [("rounds", C.c_uint64), ("segments", C.c_uint64), ("members_inflated", C.c_uint64), ("compressed_bytes", C.c_uint64),
                ("inflated_bytes", C.c_uint64), ("overflow_entries", C.c_uint64), ("records_walked", C.c_uint64),
                ("index_s", C.c_double), ("upload_s", C.c_double), ("inflate_s", C.c_double), ("count_s", C.c_double),
                ("accumulate_s", C.c_double), ("merge_s", C.c_double), ("host_scan_s", C.c_double),
                ("host_reason", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["host_reason"] = LIBSCAN_REASONS.get(int(self.host_reason), int(self.host_reason))
        return d


def library_scan_capacities() -> Dict[str, int]:
    """the fixed capacities of the library walk (svt_library_walk.h)"""
    L = _lib()
    return {name: int(L.svt_library_scan_capacity(k)) for k, name in enumerate(LIBSCAN_CAPACITIES)}


def library_scan_overflow_limit(entries: int) -> None:
    """svt_library_scan_overflow_limit: a smaller overflow list for this thread's later scans (0: the capacity again)"""
    _lib().svt_library_scan_overflow_limit(int(entries))


WALK_REASONS = {2: "range", 3: "reads", 4: "name", 5: "cigar", 6: "sa_cap", 7: "no_rg", 8: "unknown_rg", 9: "malformed", 10: "mapq"}
WALK_CAPACITIES = ("reads", "name", "cigar", "sa_entries", "sa_bytes", "record", "reads_lds")


class _DeviceStats(C.Structure):
    """include/svtyper_reads.h: svt_evidence_device_stats"""
    _fields_ = [("n_units", C.c_uint64), ("reads_walked", C.c_uint64), ("units_skipped", C.c_uint64), ("units_host", C.c_uint64),
                ("units_host_by_reason", C.c_uint64 * 11), ("n_records", C.c_uint64), ("bytes_uploaded", C.c_uint64),
                ("host_arena_s", C.c_double), ("upload_s", C.c_double), ("device_walk_s", C.c_double),
                ("host_fallback_s", C.c_double), ("batch_create_s", C.c_double)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "units_host_by_reason"}
        d["units_host_by_reason"] = {WALK_REASONS[r]: int(self.units_host_by_reason[r]) for r in WALK_REASONS
                                     if self.units_host_by_reason[r]}
        return d


class _DeepStats(C.Structure):
    """include/svtyper_reads.h: svt_evidence_deep_stats"""
    _fields_ = [("units_deep", C.c_uint64), ("reads_deep", C.c_uint64), ("workspace_bytes", C.c_uint64), ("deep_walk_s", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def deep_stats() -> dict:
    """svt_evidence_device_deep_stats: the deep tier's share of this thread's last evidence_device() call"""
    st = _DeepStats()
    hip._check(_lib().svt_evidence_device_deep_stats(C.byref(st)))
    return st.as_dict()


INFLATE_REASONS = {1: "input", 2: "btype", 3: "stored", 4: "lengths", 5: "symbol", 6: "distance", 7: "output", 8: "short", 9: "member",
                   10: "crc"}
INFLATE_CRC = 10


class _VerifyStats(C.Structure):
    """include/svtyper_reads.h: svt_bgzf_verify_counts"""
    _fields_ = [("members_verified", C.c_uint64), ("members_failed", C.c_uint64), ("host_crc_s", C.c_double), ("device_crc_s", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def verify_stats() -> dict:
    """svt_bgzf_verify_stats: what verify did in this thread's last call that took a BAM handle"""
    st = _VerifyStats()
    hip._check(_lib().svt_bgzf_verify_stats(C.byref(st)))
    return st.as_dict()


class _DeflateTimes(C.Structure):
    """include/svtyper_reads.h: svt_deflate_times"""
    _fields_ = [("crc_kernel_s", C.c_double), ("deflate_kernel_s", C.c_double), ("pack_kernel_s", C.c_double), ("total_s", C.c_double)]


class _LinesTimes(C.Structure):
    """include/svtyper_reads.h: svt_vcf_lines_times"""
    _fields_ = [("count_kernel_s", C.c_double), ("starts_kernel_s", C.c_double), ("parse_kernel_s", C.c_double),
                ("gather_kernel_s", C.c_double), ("total_s", C.c_double)]


class _PasteInfo(C.Structure):
    """include/svtyper_reads.h: svt_paste_info"""
    _fields_ = [("out_len", C.c_uint64), ("host_lines", C.c_uint64), ("bad_line", C.c_uint64), ("bad_file", C.c_uint32),
                ("bad_kind", C.c_uint32), ("bad_field", C.c_uint32), ("reserved", C.c_uint32)]


class _PasteTimes(C.Structure):
    """include/svtyper_reads.h: svt_vcf_paste_times"""
    _fields_ = [(name, C.c_double) for name in ("lines_kernels_s", "measure_kernel_s", "write_kernel_s", "upload_s", "download_s", "host_s",
                                                "total_s")]


class _ClassifyInfo(C.Structure):
    """include/svtyper_reads.h: svt_classify_info"""
    _fields_ = [("out_len", C.c_uint64), ("host_lines", C.c_uint64), ("near_lines", C.c_uint64), ("bad_line", C.c_uint64),
                ("bad_kind", C.c_uint32), ("bad_sample", C.c_uint32), ("bad_text", C.c_char * 48)]


class _ClassifyTimes(C.Structure):
    """include/svtyper_reads.h: svt_vcf_classify_times"""
    _fields_ = [(name, C.c_double) for name in ("lines_kernels_s", "classify_kernel_s", "upload_s", "download_s", "host_s", "total_s")]


class _UpdateInfoReport(C.Structure):
    """include/svtyper_reads.h: svt_update_info_report"""
    _fields_ = [("out_len", C.c_uint64), ("host_lines", C.c_uint64), ("bad_line", C.c_uint64), ("bad_kind", C.c_uint32),
                ("bad_sample", C.c_uint32), ("bad_text", C.c_char * 48)]


class _UpdateInfoTimes(C.Structure):
    """include/svtyper_reads.h: svt_vcf_update_info_times"""
    _fields_ = [(name, C.c_double) for name in ("lines_kernels_s", "update_info_kernel_s", "upload_s", "download_s", "host_s", "total_s")]


class _GroupReport(C.Structure):
    """include/svtyper_reads.h: svt_group_report"""
    _fields_ = [("out_len", C.c_uint64), ("host_lines", C.c_uint64), ("bad_line", C.c_uint64), ("bad_kind", C.c_uint32),
                ("bad_sample", C.c_uint32), ("host_join", C.c_uint32), ("n_bnd", C.c_uint32), ("bad_text", C.c_char * 48)]


class _GroupTimes(C.Structure):
    """include/svtyper_reads.h: svt_vcf_group_times"""
    _fields_ = [(name, C.c_double) for name in ("lines_kernels_s", "scan_kernel_s", "compact_kernels_s", "sort_kernels_s", "match_kernel_s",
                                                "plan_kernels_s", "upload_s", "download_s", "host_s", "total_s")]


class _BamSortTimes(C.Structure):
    """include/svtyper_reads.h: svt_bam_sort_times"""
    _fields_ = [("keys_kernel_s", C.c_double), ("histogram_kernel_s", C.c_double), ("scan_kernel_s", C.c_double),
                ("scatter_kernel_s", C.c_double), ("gather_kernel_s", C.c_double), ("total_s", C.c_double), ("passes", C.c_uint32),
                ("reserved", C.c_uint32)]


class _BamFirstTimes(C.Structure):
    """include/svtyper_reads.h: svt_bam_first_times"""
    _fields_ = [("hash_kernel_s", C.c_double), ("histogram_kernel_s", C.c_double), ("scan_kernel_s", C.c_double),
                ("scatter_kernel_s", C.c_double), ("mark_kernel_s", C.c_double), ("total_s", C.c_double), ("passes", C.c_uint32),
                ("reserved", C.c_uint32)]


class _BamIndexTimes(C.Structure):
    _fields_ = [(name, C.c_double) for name in ("record_kernel_s", "scan_kernel_s", "sort_kernel_s", "loffset_kernel_s", "reference_kernel_s",
                                                "total_s")] + [("runs", C.c_uint64), ("passes", C.c_uint32), ("reserved", C.c_uint32)]


class _InflateStats(C.Structure):
    """include/svtyper_reads.h: svt_evidence_inflate_stats"""
    _fields_ = [("blocks_inflated", C.c_uint64), ("blocks_failed", C.c_uint64), ("compressed_bytes", C.c_uint64),
                ("inflated_bytes", C.c_uint64), ("blocks_host_route", C.c_uint64), ("host_index_s", C.c_double),
                ("compressed_upload_s", C.c_double), ("inflate_kernel_s", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class _Dump(C.Structure):
    """include/svtyper_reads.h: svt_evidence_dump"""
    _fields_ = [("bytes", C.c_void_p), ("unit_offset", C.POINTER(C.c_uint64)), ("unit_host", C.POINTER(C.c_uint8)),
                ("n_bytes", C.c_uint64), ("n_reads", C.c_uint64), ("units_dumped", C.c_uint64), ("units_host", C.c_uint64),
                ("units_outside_dump", C.c_uint64), ("dump_s", C.c_double)]

    COUNTERS = ("n_bytes", "n_reads", "units_dumped", "units_host", "units_outside_dump", "dump_s")

    def take(self, lib, n: int):
        """(bytes, unit_offset uint64 [n + 1], unit_host uint8 [n], counters) copied out; the C buffers are released"""
        try:
            off = np.ctypeslib.as_array(self.unit_offset, shape=(n + 1,)).copy()
            host = np.ctypeslib.as_array(self.unit_host, shape=(max(n, 1),))[:n].copy()
            data = C.string_at(self.bytes, int(self.n_bytes)) if self.n_bytes else b""
            return data, off, host, {k: getattr(self, k) for k in self.COUNTERS}
        finally:
            lib.svt_evidence_dump_free(C.byref(self))


NO_DUMP = {k: 0 for k in _Dump.COUNTERS}     # the dump counters of a call without a dump


def has_dump() -> bool:
    """this libsvtyper_hip.so has the evidence dump (svt_bam_evidence_device_dump: added without a new ABI number)"""
    return hasattr(_lib(), "svt_bam_evidence_device_dump")


def walk_capacities() -> Dict[str, int]:
    """the fixed capacities of the evidence walk (svt_evidence_walk.h)"""
    L = _lib()
    return {name: int(L.svt_evidence_walk_capacity(k)) for k, name in enumerate(WALK_CAPACITIES)}


_declared = False


def _lib():
    global _declared
    L = hip.load()
    if not _declared:
        L.svt_bam_open.restype = C.c_int
        L.svt_bam_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.svt_bam_close.restype = None
        L.svt_bam_close.argtypes = [C.c_void_p]
        if hasattr(L, "svt_bam_index_info"):       # (added under ABI 19: a library built before it lacks the symbol)
            L.svt_bam_index_info.restype = C.c_int
            L.svt_bam_index_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.svt_bam_n_references.restype = C.c_int32
        L.svt_bam_n_references.argtypes = [C.c_void_p]
        L.svt_bam_reference_name.restype = C.c_char_p
        L.svt_bam_reference_name.argtypes = [C.c_void_p, C.c_int32]
        L.svt_bam_reference_length.restype = C.c_int64
        L.svt_bam_reference_length.argtypes = [C.c_void_p, C.c_int32]
        L.svt_bam_tid.restype = C.c_int32
        L.svt_bam_tid.argtypes = [C.c_void_p, C.c_char_p]
        L.svt_bam_header_text.restype = C.c_char_p
        L.svt_bam_header_text.argtypes = [C.c_void_p]
        L.svt_bam_summarise.restype = C.c_int
        L.svt_bam_summarise.argtypes = [C.c_void_p, C.POINTER(_Args), C.POINTER(_Summaries)]
        L.svt_summaries_free.restype = None
        L.svt_summaries_free.argtypes = [C.POINTER(_Summaries)]
        L.svt_bam_evidence.restype = C.c_int
        L.svt_bam_evidence.argtypes = [C.c_void_p, C.POINTER(_Args), C.POINTER(_EvidenceParams), C.POINTER(_Evidence)]
        L.svt_evidence_free.restype = None
        L.svt_evidence_free.argtypes = [C.POINTER(_Evidence)]
        L.svt_bam_evidence_walk_host.restype = C.c_int
        L.svt_bam_evidence_walk_host.argtypes = [C.c_void_p, C.POINTER(_Args), C.POINTER(_EvidenceParams), C.POINTER(_Evidence),
                                                 C.c_void_p, C.c_void_p]
        L.svt_evidence_walk_capacity.restype = C.c_uint32
        L.svt_evidence_walk_capacity.argtypes = [C.c_int]
        L.svt_bam_evidence_device.restype = C.c_int
        L.svt_bam_evidence_device.argtypes = [C.c_void_p, C.POINTER(_Args), C.POINTER(_EvidenceParams), C.c_void_p, C.c_int, C.c_uint,
                                              C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(_DeviceStats)]
        L.svt_bam_evidence_walk_open_host.restype = C.c_int
        L.svt_bam_evidence_walk_open_host.argtypes = L.svt_bam_evidence_walk_host.argtypes
        L.svt_bam_evidence_device_inflate.restype = C.c_int
        L.svt_bam_evidence_device_inflate.argtypes = L.svt_bam_evidence_device.argtypes + [C.POINTER(_InflateStats), C.c_int]
        if hasattr(L, "svt_bam_evidence_device_dump"):      # (added without a new ABI number: a library built before it lacks the symbols)
            L.svt_bam_evidence_device_dump.restype = C.c_int
            L.svt_bam_evidence_device_dump.argtypes = L.svt_bam_evidence_device_inflate.argtypes + [C.c_int, C.POINTER(_Dump)]
            L.svt_bam_evidence_dump_walk_host.restype = C.c_int
            L.svt_bam_evidence_dump_walk_host.argtypes = [C.c_void_p, C.POINTER(_Args), C.POINTER(_EvidenceParams), C.c_void_p, C.c_uint64,
                                                          C.POINTER(_Evidence), C.c_void_p, C.POINTER(_Dump)]
            L.svt_evidence_dump_free.restype = None
            L.svt_evidence_dump_free.argtypes = [C.POINTER(_Dump)]
        L.svt_bgzf_inflate_host.restype = C.c_int
        L.svt_bgzf_inflate_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svt_bgzf_inflate_device.restype = C.c_int
        L.svt_bgzf_inflate_device.argtypes = L.svt_bgzf_inflate_host.argtypes + [C.c_int]
        L.svt_bgzf_inflate_host_verified.restype = C.c_int
        L.svt_bgzf_inflate_host_verified.argtypes = L.svt_bgzf_inflate_host.argtypes
        L.svt_bgzf_inflate_device_verified.restype = C.c_int
        L.svt_bgzf_inflate_device_verified.argtypes = L.svt_bgzf_inflate_device.argtypes
        L.svt_bgzf_crc32_host.restype = C.c_int
        L.svt_bgzf_crc32_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.svt_bgzf_crc32_device.restype = C.c_int
        L.svt_bgzf_crc32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        if hasattr(L, "svt_bgzf_deflate_host"):    # (added without a new ABI number: a library built before it lacks the symbols)
            host = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
            for name, argtypes in (("svt_bgzf_deflate_host", host), ("svt_bgzf_deflate_device", host + [C.c_int]),
                                   ("svt_bgzf_deflate_last_times", [C.POINTER(_DeflateTimes)])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        if hasattr(L, "svt_bgzf_deflate_host_mode"):   # (likewise: the dynamic block and the code-length rule on its own)
            host, lengths = L.svt_bgzf_deflate_host.argtypes, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
            for name, argtypes in (("svt_bgzf_deflate_host_mode", host + [C.c_uint32]), ("svt_bgzf_deflate_device_mode", host + [C.c_uint32, C.c_int]),
                                   ("svt_huffman_lengths_host", lengths), ("svt_huffman_lengths_device", lengths + [C.c_int])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        if hasattr(L, "svt_vcf_lines_host"):       # (likewise: VCF text as lines, the sorted and indexed BGZF output)
            P, U64 = C.c_void_p, C.c_uint64
            for name, argtypes in (("svt_vcf_lines_host", [P, U64, P, U64, P]), ("svt_vcf_lines_device", [P, U64, P, U64, P, C.c_int]),
                                   ("svt_vcf_gather_host", [P, U64, P, U64, P, U64, P, U64]),
                                   ("svt_vcf_gather_device", [P, U64, P, U64, P, U64, P, U64, C.c_int]),
                                   ("svt_vcf_sort_order", [P, U64, P, U64, P, P]),
                                   ("svt_vcf_bgzf_device", [P, U64, C.c_int, C.c_uint32, P, U64, P, P, U64, P, P, P, C.c_int]),
                                   ("svt_vcf_lines_last_times", [C.POINTER(_LinesTimes)]),
                                   ("svt_tbx_build", [P, U64, P, P, U64, P, U64, C.c_uint32, P, P, P]), ("svt_tbx_take", [P, U64])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        if hasattr(L, "svt_vcf_paste_host"):       # (likewise: per-sample VCFs joined by line number, AF and NSAMP)
            P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
            host = [P, U64, P, U32, U64, U32, P, U64, P, U64, P, C.POINTER(_PasteInfo)]
            for name, argtypes in (("svt_vcf_paste_host", host), ("svt_vcf_paste_device", host + [C.c_int]),
                                   ("svt_vcf_paste_last_times", [C.POINTER(_PasteTimes)])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        for rule in (_CLASSIFY, _UPDATE_INFO, _GROUP):      # (likewise: the rules over the lines of a cohort VCF, BND mates grouped)
            rule.declare(L)
        if hasattr(L, "svt_bam_spans_host"):       # (likewise: BAM records as spans, the sorted and indexed `-w` dump)
            P, U64, I32 = C.c_void_p, C.c_uint64, C.c_int32
            for name, argtypes in (("svt_bam_spans_host", [P, U64, P, U64, I32, P, P, P]), ("svt_bam_spans_device", [P, U64, P, U64, I32, P, P, P, C.c_int]),
                                   ("svt_bam_sort_order_host", [P, U64, P, P, P]), ("svt_bam_sort_order_device", [P, U64, P, P, P, C.c_int]),
                                   ("svt_bam_sorted_bgzf_device", [P, U64, P, U64, I32, C.c_int, C.c_uint32, P, U64, P, U64, P, P, P, P, P, P, C.c_int]),
                                   ("svt_bam_sort_last_times", [C.POINTER(_BamSortTimes)]),
                                   ("svt_bai_build", [P, U64, I32, P, P, U64, P, P, P]), ("svt_bai_take", [P, U64])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        if hasattr(L, "svt_csi_build_bam"):        # (likewise: a CSI index for the sorted outputs, the BAM's fold on the device)
            P, U64, I32 = C.c_void_p, C.c_uint64, C.c_int32
            L.svt_csi_depth.restype = C.c_uint32
            L.svt_csi_depth.argtypes = [U64]
            for name, argtypes in (("svt_csi_build_bam", [P, U64, I32, U64, P, P, U64, P, P, P]),
                                   ("svt_csi_build_vcf", [P, U64, P, P, U64, P, U64, C.c_uint32, P, P, P]), ("svt_csi_take", [P, U64]),
                                   ("svt_bam_index_fold_device", [P, U64, I32, U64, P, P, U64, P, P, P, C.c_int]),
                                   ("svt_bam_sorted_bgzf_csi_device", [P, U64, P, U64, I32, U64, C.c_int, C.c_uint32, P, U64, P, U64, P, P, P, P, P, P, P, P,
                                                                       P, C.c_int]),
                                   ("svt_bam_index_last_times", [C.POINTER(_BamIndexTimes)])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        if hasattr(L, "svt_bam_first_host"):       # (likewise: first occurrences of a record stream, the gathered `-w` dump)
            P, U64 = C.c_void_p, C.c_uint64
            for name, argtypes in (("svt_bam_first_host", [P, U64, P, U64, P, P, P]),
                                   ("svt_bam_first_device", [P, U64, P, U64, P, P, P, C.c_uint32, C.c_int]),
                                   ("svt_bam_first_last_times", [C.POINTER(_BamFirstTimes)])):
                getattr(L, name).restype = C.c_int
                getattr(L, name).argtypes = argtypes
        L.svt_bam_set_verify.restype = C.c_int
        L.svt_bam_set_verify.argtypes = [C.c_void_p, C.c_int]
        L.svt_bam_get_verify.restype = C.c_int
        L.svt_bam_get_verify.argtypes = [C.c_void_p]
        L.svt_bgzf_verify_stats.restype = C.c_int
        L.svt_bgzf_verify_stats.argtypes = [C.POINTER(_VerifyStats)]
        L.svt_evidence_device_deep_stats.restype = C.c_int
        L.svt_evidence_device_deep_stats.argtypes = [C.POINTER(_DeepStats)]
        L.svt_debug_batch_records.restype = C.c_int
        L.svt_debug_batch_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.svt_bam_scan_library.restype = C.c_int
        L.svt_bam_scan_library.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_int64, C.POINTER(_LibraryScan)]
        L.svt_library_scan_free.restype = None
        L.svt_library_scan_free.argtypes = [C.POINTER(_LibraryScan)]
        L.svt_library_scan_capacity.restype = C.c_uint32
        L.svt_library_scan_capacity.argtypes = [C.c_int]
        L.svt_library_scan_overflow_limit.restype = None
        L.svt_library_scan_overflow_limit.argtypes = [C.c_uint32]
        L.svt_bam_scan_libraries_walk_host.restype = C.c_int
        L.svt_bam_scan_libraries_walk_host.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_int64,
                                                       C.c_uint64, C.POINTER(_LibraryScan), C.POINTER(_LibraryScanStats)]
        L.svt_bam_scan_libraries_device.restype = C.c_int
        L.svt_bam_scan_libraries_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.c_int64,
                                                    C.c_uint64, C.c_int, C.c_int, C.POINTER(_LibraryScan), C.POINTER(_LibraryScanStats)]
        _declared = True
    return L


# the groups of entry points that came without a new ABI number, for _need: a symbol of the group and what the group came with
_LINES = ("svt_vcf_lines_host", "sorted, indexed BGZF output")
_PASTE = ("svt_vcf_paste_host", "svtyper_amd.paste")
_SPANS = ("svt_bam_spans_host", "the sorted, indexed -w dump")
_FIRST = ("svt_bam_first_host", "the gathered -w dump")
_CSI = ("svt_csi_build_bam", "CSI indexes were written")


def _need(symbol: str, since: str):
    """_lib(), which has `symbol`: one of the entry points that came without a new ABI number, `since` names what they came with"""
    L = _lib()
    if not hasattr(L, symbol):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no %s (built before %s)" % (symbol, since))
    return L


def _times(struct, entry, ints=()) -> dict:
    """what a *_last_times entry point says: entry(&t) over a fresh `struct`, every field by its name as a float (`ints`: as an int)"""
    t = struct()
    hip._check(entry(C.byref(t)))
    return {name: (int if name in ints else float)(getattr(t, name)) for name, _ in struct._fields_ if name != "reserved"}


class NativeBam:
    """An indexed BAM opened by the C++ reader."""

    def __init__(self, path: str, verify: bool = False):
        L = _lib()
        self._L = L
        self._h = C.c_void_p()
        hip._check(L.svt_bam_open(path.encode(), C.byref(self._h)))
        # svt_bgzf_verify_stats summed over this object's calls (each read on the thread that made the call)
        self.verify_stats = {"members_verified": 0, "members_failed": 0, "host_crc_s": 0.0, "device_crc_s": 0.0}
        self._verify_lock = threading.Lock()
        if verify:
            self.verify = True
        self.filename = path
        n = L.svt_bam_n_references(self._h)
        self.references = tuple(L.svt_bam_reference_name(self._h, i).decode() for i in range(n))
        self.lengths = tuple(int(L.svt_bam_reference_length(self._h, i)) for i in range(n))
        self._tid = {r: i for i, r in enumerate(self.references)}
        text = (L.svt_bam_header_text(self._h) or b"").decode("ascii", "replace")
        self.header: Dict[str, list] = {}
        for line in text.splitlines():
            if not line.startswith("@") or line.startswith("@CO"):
                continue
            parts = line.split("\t")
            rec = {f[:2]: f[3:] for f in parts[1:] if len(f) >= 3 and f[2] == ":"}
            self.header.setdefault(parts[0][1:], []).append(rec)

    @property
    def verify(self) -> bool:
        """svt_bam_get_verify / svt_bam_set_verify: every call on this handle checks the CRC32 of the BGZF members it inflates"""
        return bool(self._L.svt_bam_get_verify(self._h))

    @verify.setter
    def verify(self, on: bool) -> None:
        hip._check(self._L.svt_bam_set_verify(self._h, 1 if on else 0))

    def _call(self, rc: int) -> None:
        """hip._check for a call that took the handle: its share of the verify figures is noted first, also when it failed"""
        st = _VerifyStats()
        if self._L.svt_bgzf_verify_stats(C.byref(st)) == 0 and (st.members_verified or st.members_failed):
            with self._verify_lock:
                for k, v in st.as_dict().items():
                    self.verify_stats[k] += v
        hip._check(rc)

    def gettid(self, name: str) -> int:
        return self._tid.get(name, -1)

    def index_info(self) -> Dict[str, object]:
        """svt_bam_index_info: which index the handle was opened with -- {"kind": "bai" | "csi", "min_shift", "depth"}"""
        if not hasattr(self._L, "svt_bam_index_info"):
            raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bam_index_info (built before CSI indexes were read)")
        kind, min_shift, depth = C.c_int(), C.c_int(), C.c_int()
        hip._check(self._L.svt_bam_index_info(self._h, C.byref(kind), C.byref(min_shift), C.byref(depth)))
        return {"kind": {1: "bai", 2: "csi"}[kind.value], "min_shift": min_shift.value, "depth": depth.value}

    def close(self):
        if self._h:
            self._L.svt_bam_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scan_library(self, read_groups: Sequence[str], num_samp: int):
        """(read_length, {template_length: count}, reads of the library among the first 100 000, that total):
        the three scans of Library.from_bam (svtyper/parsers.py:501-576) in C++."""
        names = (C.c_char_p * max(1, len(read_groups)))(*[rg.encode() for rg in read_groups])
        out = _LibraryScan()
        self._call(self._L.svt_bam_scan_library(self._h, len(read_groups), names, int(num_samp), C.byref(out)))
        try:
            return int(out.read_length), dict(_histogram(out)), int(out.in_lib), int(out.total)
        finally:
            self._L.svt_library_scan_free(C.byref(out))

    def scan_libraries(self, read_groups: Sequence[Sequence[str]], num_samp: int, route: str = "device", inflate: str = "device",
                       device: int = 0, round_bytes: int = 0, ordered: bool = False):
        """scan_library() for all libraries of the file in one segmented walk (svt_library_walk.h): a list with one
        (read_length, {template_length: count}, in_lib, total) per entry of `read_groups`, the dicts in the order of the keys'
        first occurrence.  route="device": svt_bam_scan_libraries_device, with the BGZF members inflated on the GPU
        (inflate="device") or by host threads (inflate="host"); route="walk_host": the same walk on the CPU.  Whatever is
        outside the walk's envelope is answered by the host scan (self.library_scan_stats["host_reason"] says why).
        `ordered`: the histograms as lists of (key, count) instead of dicts."""
        if route not in ("device", "walk_host"):
            raise ValueError('route must be "device" or "walk_host", not %r' % (route,))
        if inflate not in ("device", "host"):
            raise ValueError('inflate must be "device" or "host", not %r' % (inflate,))
        n_libs = len(read_groups)
        flat = [rg.encode() for lib in read_groups for rg in lib]
        names = (C.c_char_p * max(1, len(flat)))(*flat)
        counts = (C.c_uint32 * max(1, n_libs))(*[len(lib) for lib in read_groups])
        out = (_LibraryScan * max(1, n_libs))()
        st = _LibraryScanStats()
        if route == "walk_host":
            rc = self._L.svt_bam_scan_libraries_walk_host(self._h, n_libs, counts, names, int(num_samp), int(round_bytes), out, C.byref(st))
        else:
            rc = self._L.svt_bam_scan_libraries_device(self._h, n_libs, counts, names, int(num_samp), int(round_bytes),
                                                       1 if inflate == "device" else 0, int(device), out, C.byref(st))
        self.library_scan_stats = st.as_dict()
        self._call(rc)
        try:
            result = []
            for l in range(n_libs):
                hist = _histogram(out[l]) if ordered else dict(_histogram(out[l]))
                result.append((int(out[l].read_length), hist, int(out[l].in_lib), int(out[l].total)))
            return result
        finally:
            for l in range(n_libs):
                self._L.svt_library_scan_free(C.byref(out[l]))

    def evidence(self, windows: np.ndarray, breakpoints: np.ndarray, read_groups: Sequence[str],
                 read_group_lib: Sequence[int], max_reads: Optional[int], count_mode: int, lib_flank: Sequence[float],
                 min_aligned: int, split_slop: int, n_threads: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """svt_bam_evidence: (rec_offset uint64 [n+1], records RECORD_DTYPE, skipped uint8 [n]) -- the units' 16-byte
        evidence records, the geometry predicates evaluated in the reader's threads (`lib_flank`: mean + 3 sd of every
        library of the batch).  What summarise() + the device geometry stage produce, byte for byte."""
        from .evidence import RECORD_DTYPE
        n, a, g, _keep = self._walk_args(windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads,
                                         lib_flank, min_aligned, split_slop)
        out = _Evidence()
        self._call(self._L.svt_bam_evidence(self._h, C.byref(a), C.byref(g), C.byref(out)))
        return _owned_arrays(self._L.svt_evidence_free, out, n, RECORD_DTYPE)

    def _walk_args(self, windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads, lib_flank=None,
                   min_aligned=0, split_slop=0):
        """(n, svt_summarise_args, svt_evidence_params -- None without `lib_flank` --, what has to outlive the C call)"""
        windows = np.ascontiguousarray(windows, dtype=FETCH_DTYPE)
        breakpoints = np.ascontiguousarray(breakpoints, dtype=BREAKPOINT_DTYPE)
        n = int(windows.shape[0])
        if breakpoints.shape[0] != n:
            raise ValueError("windows and breakpoints must have the same length")
        names = (C.c_char_p * max(1, len(read_groups)))(*[rg.encode() for rg in read_groups])
        libs = (C.c_int32 * max(1, len(read_groups)))(*[int(x) for x in read_group_lib])
        a = _Args(n, windows.ctypes.data, breakpoints.ctypes.data, len(read_groups), names, libs,
                  -1 if max_reads is None else int(max_reads), int(count_mode), int(n_threads))
        if lib_flank is None:
            return n, a, None, (windows, breakpoints, names, libs)
        flank = (C.c_double * max(1, len(lib_flank)))(*[float(x) for x in lib_flank])
        g = _EvidenceParams(len(lib_flank), flank, int(min_aligned), int(split_slop))
        return n, a, g, (windows, breakpoints, names, libs, flank)

    def evidence_walk_open_host(self, *a, **kw):
        """svt_bam_evidence_walk_open_host: evidence_walk_host() over the arena of inflate="device" -- laid out from BGZF headers,
        inflated by the one-source decoder (svt_inflate.h) on the CPU, open ranges ended by the walk.  Same arguments and result."""
        return self.evidence_walk_host(*a, _entry="svt_bam_evidence_walk_open_host", **kw)

    def evidence_walk_host(self, windows: np.ndarray, breakpoints: np.ndarray, read_groups: Sequence[str],
                           read_group_lib: Sequence[int], max_reads: Optional[int], count_mode: int, lib_flank: Sequence[float],
                           min_aligned: int, split_slop: int, n_threads: int = 0, _entry: str = "svt_bam_evidence_walk_host"):
        """svt_bam_evidence_walk_host: evidence() computed by the one-source walk (svt_evidence_walk.h) over host memory, without
        a fallback: (rec_offset, records, skipped, out_of_envelope uint8 [n] -- 0 or a WALK_REASONS key, such a unit has no
        records --, kept_reads uint32 [n])."""
        from .evidence import RECORD_DTYPE
        n, a, g, _keep = self._walk_args(windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads,
                                         lib_flank, min_aligned, split_slop)
        out = _Evidence()
        flagged = np.zeros(max(n, 1), np.uint8)
        kept = np.zeros(max(n, 1), np.uint32)
        self._call(getattr(self._L, _entry)(self._h, C.byref(a), C.byref(g), C.byref(out), flagged.ctypes.data, kept.ctypes.data))
        try:
            off = np.ctypeslib.as_array(out.rec_offset, shape=(n + 1,)).copy()
            total = int(off[-1])
            skipped = np.ctypeslib.as_array(out.skipped, shape=(max(n, 1),))[:n].copy()
            recs = np.zeros(total, RECORD_DTYPE)
            if total:
                C.memmove(recs.ctypes.data, out.records, total * RECORD_DTYPE.itemsize)
        finally:
            self._L.svt_evidence_free(C.byref(out))
        return off, recs, skipped, flagged[:n], kept[:n]

    def evidence_dump_walk_host(self, windows: np.ndarray, breakpoints: np.ndarray, read_groups: Sequence[str],
                                read_group_lib: Sequence[int], max_reads: Optional[int], count_mode: int, lib_flank: Sequence[float],
                                min_aligned: int, split_slop: int, verdicts: np.ndarray, n_threads: int = 0):
        """svt_bam_evidence_dump_walk_host: the evidence dump of `svtyper -w` with no GPU -- evidence_walk_host() with source
        rows plus the dump rules (svt_dump_rules.h) on one lane.  `verdicts`: uint8, one per record of evidence_walk_host() on the
        same arguments, in its record order (there is no host implementation of the verdicts).  Returns (bytes -- finished BAM
        records, unit after unit --, unit_offset uint64 [n + 1], unit_host uint8 [n]: 1 = outside the walk's or the dump's
        envelope, no bytes; counters dict)."""
        if not hasattr(self._L, "svt_bam_evidence_dump_walk_host"):
            raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bam_evidence_dump_walk_host (built before it was added): rebuild it")
        n, a, g, _keep = self._walk_args(windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads,
                                         lib_flank, min_aligned, split_slop)
        verdicts = np.ascontiguousarray(verdicts, dtype=np.uint8)
        out, dump = _Evidence(), _Dump()
        flagged = np.zeros(max(n, 1), np.uint8)
        self._call(self._L.svt_bam_evidence_dump_walk_host(self._h, C.byref(a), C.byref(g), verdicts.ctypes.data if verdicts.size else None,
                                                           int(verdicts.size), C.byref(out), flagged.ctypes.data, C.byref(dump)))
        self._L.svt_evidence_free(C.byref(out))
        return dump.take(self._L, n)

    def evidence_device(self, windows: np.ndarray, breakpoints: np.ndarray, read_groups: Sequence[str],
                        read_group_lib: Sequence[int], max_reads: Optional[int], count_mode: int, lib_flank: Sequence[float],
                        min_aligned: int, split_slop: int, header, device: int = 0, flags: int = 0, n_threads: int = 0,
                        inflate: str = "host", count_host_blocks: bool = False, dump: bool = False):
        """svt_bam_evidence_device: the reader stage with the walk on the GPU.  `header`: an EvidenceBatch whose units,
        libraries and weights describe the batch (its rec_offset / records are ignored).  Returns (hip.DeviceBatch resident
        in HBM -- what DeviceBatch(EvidenceBatch(*evidence(...))) builds --, skipped uint8 [n], stats dict; under "deep" the
        share of the units of more than walk_capacities()["reads_lds"] kept reads: svt_evidence_deep_stats).
        inflate="device" (svt_bam_evidence_device_inflate): the BGZF members are inflated on the GPU as well; the stats then
        carry svt_evidence_inflate_stats under "inflate" (`count_host_blocks`: also count the blocks of the host-inflate route).
        dump=True (svt_bam_evidence_device_dump): a fourth value, the evidence dump of `svtyper -w` built on the GPU behind the
        batch -- (bytes, unit_offset, unit_host) as evidence_dump_walk_host() gives them; its counters are stats["dump"], which
        a call without it reports as zeros."""
        if inflate not in ("host", "device"):
            raise ValueError("inflate must be 'host' or 'device'")
        if dump and not hasattr(self._L, "svt_bam_evidence_device_dump"):
            raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bam_evidence_device_dump (built before it was added): rebuild it")
        n, a, g, _keep = self._walk_args(windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads,
                                         lib_flank, min_aligned, split_slop)
        if header.n_units != n:
            raise ValueError("header and windows must have the same number of units")
        cb = header.as_c()
        handle = C.c_void_p()
        skipped = np.zeros(max(n, 1), np.uint8)
        st, ist, dmp = _DeviceStats(), _InflateStats(), _Dump()
        if dump:       # the three entry points share their first arguments; each later one took the one before and added a tail
            entry, tail = self._L.svt_bam_evidence_device_dump, [C.byref(ist), 1 if count_host_blocks else 0, 1 if inflate == "device" else 0, C.byref(dmp)]
        elif inflate == "device":
            entry, tail = self._L.svt_bam_evidence_device_inflate, [C.byref(ist), 1 if count_host_blocks else 0]
        else:
            entry, tail = self._L.svt_bam_evidence_device, []
        self._call(entry(self._h, C.byref(a), C.byref(g), C.byref(cb), int(device), int(flags), C.byref(handle), skipped.ctypes.data,
                         C.byref(st), *tail))
        batch = hip.DeviceBatch.adopt(handle, n, int(st.n_records), device)
        dumped = dmp.take(self._L, n) if dump else None
        stats = st.as_dict()
        if inflate == "device":
            stats["inflate"] = ist.as_dict()
        stats["deep"] = deep_stats()
        stats["dump"] = dumped[3] if dump else dict(NO_DUMP)
        return (batch, skipped[:n], stats, dumped[:3]) if dump else (batch, skipped[:n], stats)

    def summarise(self, windows: np.ndarray, breakpoints: np.ndarray, read_groups: Sequence[str],
                  read_group_lib: Sequence[int], max_reads: Optional[int], count_mode: int,
                  n_threads: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(frag_offset uint64 [n+1], fragments FRAGMENT_DTYPE, skipped uint8 [n])"""
        n, a, _g, _keep = self._walk_args(windows, breakpoints, read_groups, read_group_lib, max_reads, count_mode, n_threads)
        out = _Summaries()
        self._call(self._L.svt_bam_summarise(self._h, C.byref(a), C.byref(out)))
        return _owned_arrays(self._L.svt_summaries_free, out, n, FRAGMENT_DTYPE)


class _Owner:
    """frees the C buffers of a result struct once the arrays that view them are gone"""

    def __init__(self, free, struct):
        self._free, self._struct = free, struct

    def __del__(self):
        try:
            self._free(C.byref(self._struct))
        except Exception:
            pass


def _owned_arrays(free, out, n: int, dtype) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(offsets uint64 [n + 1] copied, elements viewed in place, skipped uint8 [n] copied) of an svt_summaries / svt_evidence
    (offsets, elements, skipped); `free` runs when the elements are gone"""
    owner = _Owner(free, out)
    offsets, elements = (getattr(out, name) for name, _ in out._fields_[:2])
    off = np.ctypeslib.as_array(offsets, shape=(n + 1,)).copy()
    total = int(off[-1])
    skipped = np.ctypeslib.as_array(out.skipped, shape=(max(n, 1),))[:n].copy()
    if not total:
        return off, np.zeros(0, dtype), skipped
    raw = (C.c_uint8 * (total * dtype.itemsize)).from_address(elements)    # zero-copy view of the C array (1.4 GB for 10 M fragments)
    raw._svt_owner = owner     # every numpy view keeps `raw` alive through .base, and raw keeps the owner
    return off, np.frombuffer(raw, dtype=dtype), skipped


def _histogram(scan) -> list:
    """the (template_length, count) pairs of an svt_library_scan, in the order of the keys' first occurrence"""
    n = int(scan.n_hist)
    keys = np.ctypeslib.as_array(scan.hist_keys, shape=(max(n, 1),))[:n].tolist()
    counts = np.ctypeslib.as_array(scan.hist_counts, shape=(max(n, 1),))[:n].tolist()
    return list(zip(keys, counts))


def batch_offsets(dbatch) -> np.ndarray:
    """svt_debug_batch_records without the records: rec_offset uint64 [n_units + 1] of a resident batch of canonical records"""
    off = np.zeros(dbatch.n_units + 1, np.uint64)
    hip._check(_lib().svt_debug_batch_records(dbatch._h, off.ctypes.data, None))
    return off


def batch_records(dbatch) -> Tuple[np.ndarray, np.ndarray]:
    """svt_debug_batch_records: (rec_offset, records) of a resident batch of canonical records, read back from HBM"""
    from .evidence import RECORD_DTYPE
    L = _lib()
    off = np.zeros(dbatch.n_units + 1, np.uint64)
    hip._check(L.svt_debug_batch_records(dbatch._h, off.ctypes.data, None))
    recs = np.zeros(int(off[-1]), RECORD_DTYPE)
    hip._check(L.svt_debug_batch_records(dbatch._h, off.ctypes.data, recs.ctypes.data if recs.size else None))
    return off, recs


def bgzf_members(data: bytes) -> Tuple[np.ndarray, np.ndarray]:
    """(block_off uint64 [n], out_off uint64 [n + 1]) of the BGZF members that lie side by side in `data`, from their headers and
    trailers alone: what svt_bgzf_inflate_host / _device take.  Stops at the first bytes that are no member."""
    offs, sizes, at = [], [0], 0
    while at + 18 <= len(data) and data[at] == 31 and data[at + 1] == 139:
        xlen = data[at + 10] | data[at + 11] << 8
        bsize, i = -1, 0
        while i + 4 <= xlen:
            x = at + 12 + i
            if data[x] == 66 and data[x + 1] == 67 and i + 6 <= xlen:
                bsize = data[x + 4] | data[x + 5] << 8
            i += 4 + (data[x + 2] | data[x + 3] << 8)
        if bsize < 0 or at + bsize + 1 > len(data) or bsize - xlen - 19 < 0:
            break
        offs.append(at)
        sizes.append(sizes[-1] + int.from_bytes(data[at + bsize - 3:at + bsize + 1], "little"))
        at += bsize + 1
    return np.array(offs, np.uint64), np.array(sizes, np.uint64)


def bgzf_crc32(data, off: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """svt_bgzf_crc32_host (device None) / svt_bgzf_crc32_device: the CRC-32 of data[off[k] .. off[k + 1]) for every k, by the
    one-source code of svt_crc32.h.  For the device `data` is put into HBM first: the entry point takes a device pointer."""
    L = _lib()
    off = np.ascontiguousarray(off, np.uint64)
    n = int(off.shape[0]) - 1
    if n < 0:
        raise ValueError("off must hold n + 1 entries")
    crc = np.zeros(max(n, 1), np.uint32)
    if device is None:
        buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        hip._check(L.svt_bgzf_crc32_host(buf.ctypes.data, off.ctypes.data, n, crc.ctypes.data))
        return crc[:n]
    host = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    rt = _hip_runtime()
    ptr = C.c_void_p()
    _hip_ok(rt.hipSetDevice(int(device)), "hipSetDevice")
    _hip_ok(rt.hipMalloc(C.byref(ptr), C.c_size_t(max(host.size, 16))), "hipMalloc")
    try:
        _hip_ok(rt.hipMemcpy(ptr, C.c_void_p(host.ctypes.data), C.c_size_t(host.size), 1), "hipMemcpy")     # hipMemcpyHostToDevice
        hip._check(L.svt_bgzf_crc32_device(ptr, off.ctypes.data, n, crc.ctypes.data, int(device)))
    finally:
        rt.hipFree(ptr)
    return crc[:n]


_hip_rt = None


def _hip_runtime():
    """the HIP runtime libsvtyper_hip.so is linked against, as this process has it loaded (bgzf_crc32 puts its bytes into HBM
    itself: svt_bgzf_crc32_device takes a device pointer)"""
    global _hip_rt
    if _hip_rt is None:
        _lib()
        path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), "libamdhip64.so")
        _hip_rt = C.CDLL(path)
        _hip_rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip_rt.hipFree.argtypes = [C.c_void_p]
        _hip_rt.hipSetDevice.argtypes = [C.c_int]
    return _hip_rt


def _hip_ok(rc: int, what: str) -> None:
    if rc != 0:
        raise hip.SvtyperHipError("%s failed with HIP error %d" % (what, rc))


def bgzf_inflate(data: bytes, block_off: np.ndarray, out_off: np.ndarray, device: Optional[int] = None,
                 verified: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """svt_bgzf_inflate_host (device None) / svt_bgzf_inflate_device: the members of `data` at `block_off` inflated by the
    one-source decoder (svt_inflate.h) to out_off[k] .. out_off[k + 1].  Returns (bytes uint8 [out_off[-1]], status uint32 [n]:
    0 or an INFLATE_REASONS key -- the bytes of such a member are undefined).  `verified`: the _verified entry points, which
    also check every member's CRC-32 (INFLATE_CRC)."""
    L = _lib()
    block_off = np.ascontiguousarray(block_off, np.uint64)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    n = int(block_off.shape[0])
    if out_off.shape[0] != n + 1:
        raise ValueError("out_off must hold one entry more than block_off")
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(max(int(out_off[-1]), 1), np.uint8)
    status = np.zeros(max(n, 1), np.uint32)
    args = [buf.ctypes.data, len(data), block_off.ctypes.data, n, out.ctypes.data, out_off.ctypes.data, status.ctypes.data]
    if device is None:
        hip._check((L.svt_bgzf_inflate_host_verified if verified else L.svt_bgzf_inflate_host)(*args))
    else:
        hip._check((L.svt_bgzf_inflate_device_verified if verified else L.svt_bgzf_inflate_device)(*args, int(device)))
    return out[:int(out_off[-1])], status[:n]


DEFLATE_MAX_PAYLOAD = 65280      # bytes of payload in one member (svt_deflate.h: dfl::kMaxPayload)
DEFLATE_SLOT_EXTRA = 31          # what a member takes beyond its payload at the most: header, a stored block's 5 bytes, trailer
HUFFMAN_CHOICES = ("fixed", "dynamic")   # include/svtyper_reads.h: SVT_DEFLATE_FIXED, SVT_DEFLATE_DYNAMIC


def check_huffman(huffman) -> str:
    if huffman not in HUFFMAN_CHOICES:
        raise ValueError("huffman must be one of %s, not %r" % (", ".join(repr(c) for c in HUFFMAN_CHOICES), huffman))
    return huffman


def bgzf_deflate(payloads: Sequence[bytes], device: Optional[int] = None, capacity: Optional[int] = None,
                 huffman: str = "fixed") -> Tuple[np.ndarray, np.ndarray]:
    """svt_bgzf_deflate_host (device None) / svt_bgzf_deflate_device: every payload (at most 65 280 bytes) as one whole BGZF
    member, by the one-source compressor (svt_deflate.h).  Returns (members uint8 [out_off[-1]], out_off uint64 [n + 1]).
    `capacity`: the room offered for the members (default: what always suffices).  `huffman`: "fixed", or "dynamic" (the
    _mode entries with SVT_DEFLATE_DYNAMIC): a dynamic-Huffman block for every member that is shorter that way."""
    sizes = np.fromiter((len(p) for p in payloads), np.uint64, len(payloads))
    off = np.zeros(len(payloads) + 1, np.uint64)
    np.cumsum(sizes, out=off[1:])
    return bgzf_deflate_at(b"".join(payloads), off, device, capacity, huffman)


def bgzf_deflate_at(data: bytes, off: np.ndarray, device: Optional[int] = None, capacity: Optional[int] = None,
                    huffman: str = "fixed") -> Tuple[np.ndarray, np.ndarray]:
    """bgzf_deflate over payloads that lie in `data` already: payload k is data[off[k] .. off[k + 1])"""
    L = _lib()
    dynamic = check_huffman(huffman) == "dynamic"
    if not hasattr(L, "svt_bgzf_deflate_host"):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bgzf_deflate_host (built before BGZF deflate)")
    if dynamic and not hasattr(L, "svt_bgzf_deflate_host_mode"):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bgzf_deflate_host_mode (built before dynamic Huffman blocks)")
    off = np.ascontiguousarray(off, np.uint64)
    n = int(off.shape[0]) - 1
    if n < 0:
        raise ValueError("off must hold n + 1 entries")
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    if capacity is None:
        capacity = int(off[-1] - off[0]) + DEFLATE_SLOT_EXTRA * n if int(off[-1]) >= int(off[0]) else 0
    out = np.zeros(max(int(capacity), 1), np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    args = [buf.ctypes.data, off.ctypes.data, n, out.ctypes.data, int(capacity), out_off.ctypes.data]
    if dynamic:
        if device is None:
            hip._check(L.svt_bgzf_deflate_host_mode(*args, 1))
        else:
            hip._check(L.svt_bgzf_deflate_device_mode(*args, 1, int(device)))
    elif device is None:
        hip._check(L.svt_bgzf_deflate_host(*args))
    else:
        hip._check(L.svt_bgzf_deflate_device(*args, int(device)))
    return out[:int(out_off[-1])], out_off


def huffman_lengths(freq, limit: int, device: Optional[int] = None) -> np.ndarray:
    """svt_huffman_lengths_host (device None) / _device: the dynamic block's code-length rule on its own.  `freq`: one histogram
    [symbols] or several [sets, symbols] (symbols <= 286); returns uint8 code lengths of at most `limit` (7 or 15) bits in the
    same shape."""
    L = _lib()
    if not hasattr(L, "svt_huffman_lengths_host"):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_huffman_lengths_host (built before dynamic Huffman blocks)")
    f = np.ascontiguousarray(freq, np.uint32)
    if f.ndim not in (1, 2) or f.shape[-1] < 1:
        raise ValueError("freq must be [symbols] or [sets, symbols]")
    sets, symbols = (1, f.shape[0]) if f.ndim == 1 else f.shape
    out = np.zeros(f.shape, np.uint8)
    src = f if f.size else np.zeros(1, np.uint32)
    dst = out if out.size else np.zeros(1, np.uint8)
    args = [src.ctypes.data, int(sets), int(symbols), int(limit), dst.ctypes.data]
    if device is None:
        hip._check(L.svt_huffman_lengths_host(*args))
    else:
        hip._check(L.svt_huffman_lengths_device(*args, int(device)))
    return out


def bgzf_deflate_last_times() -> Dict[str, float]:
    """svt_bgzf_deflate_last_times: the kernels of this thread's last bgzf_deflate on a device, from HIP events, and the call's
    wall time"""
    return _times(_DeflateTimes, _lib().svt_bgzf_deflate_last_times)


# ---- VCF text as lines: the line table, the order --sort writes, the gather, the .tbi fold (include/svtyper_reads.h) ----------
TBX_LINE = np.dtype([("off", np.uint64), ("len", np.uint64), ("beg", np.uint32), ("end", np.uint32), ("chrom_len", np.uint32),
                     ("flags", np.uint32)])      # svt_tbx_line
TBX_META, TBX_BAD, TBX_RANGE = 1, 2, 4
TBX_NOT_DATA, TBX_BEYOND, TBX_CONTIG_AGAIN, TBX_POS_BACK = 1, 2, 3, 4


def _text_array(text: bytes) -> np.ndarray:
    return np.frombuffer(text, np.uint8) if len(text) else np.zeros(1, np.uint8)


def vcf_lines(text: bytes, device: Optional[int] = None) -> np.ndarray:
    """svt_vcf_lines_host (device None) / _device: the line table of `text`, one TBX_LINE record per line in text order"""
    L = _need(*_LINES)
    buf = _text_array(text)
    capacity = text.count(b"\n") + 1
    lines = np.zeros(capacity, TBX_LINE)
    n = C.c_uint64(0)
    args = [buf.ctypes.data, len(text), lines.ctypes.data, capacity, C.addressof(n)]
    if device is None:
        hip._check(L.svt_vcf_lines_host(*args))
    else:
        hip._check(L.svt_vcf_lines_device(*args, int(device)))
    return lines[:n.value]


def vcf_gather(text: bytes, lines: np.ndarray, perm, device: Optional[int] = None) -> bytes:
    """svt_vcf_gather_host (device None) / _device: the lines lines[perm[0]], lines[perm[1]], ... of `text` side by side"""
    L = _need(*_LINES)
    buf = _text_array(text)
    lines = np.ascontiguousarray(lines, TBX_LINE)
    perm = np.ascontiguousarray(perm, np.uint64)
    if perm.size and int(perm.max()) >= lines.shape[0]:
        raise ValueError("an entry of perm is no line")
    out_len = int(lines["len"][perm].sum()) if perm.size else 0
    out = np.zeros(max(out_len, 1), np.uint8)
    args = [buf.ctypes.data, len(text), lines.ctypes.data if lines.size else None, lines.shape[0], perm.ctypes.data if perm.size else None,
            perm.shape[0], out.ctypes.data, out_len]
    if device is None:
        hip._check(L.svt_vcf_gather_host(*args))
    else:
        hip._check(L.svt_vcf_gather_device(*args, int(device)))
    return out[:out_len].tobytes()


def vcf_sort_order(text: bytes, lines: np.ndarray) -> Tuple[np.ndarray, int]:
    """svt_vcf_sort_order: (perm, 0), or (None, the 1-based number of a body line that is no data line)"""
    L = _need(*_LINES)
    buf = _text_array(text)
    lines = np.ascontiguousarray(lines, TBX_LINE)
    perm = np.zeros(max(lines.shape[0], 1), np.uint64)
    bad = C.c_uint64(0)
    hip._check(L.svt_vcf_sort_order(buf.ctypes.data, len(text), lines.ctypes.data if lines.size else None, lines.shape[0], perm.ctypes.data,
                                    C.addressof(bad)))
    return (None, int(bad.value)) if bad.value else (perm[:lines.shape[0]], 0)


def vcf_bgzf_device(text: bytes, sort: bool, huffman: str = "fixed", device: int = 0):
    """svt_vcf_bgzf_device: `text` up once; (members uint8, out_off uint64 [n + 1], lines as written, src_off uint64, 0), or
    (None, None, None, None, bad_line) where sorting met a body line that is no data line"""
    L = _need(*_LINES)
    buf = _text_array(text)
    n = (len(text) + DEFLATE_MAX_PAYLOAD - 1) // DEFLATE_MAX_PAYLOAD
    capacity = len(text) + DEFLATE_SLOT_EXTRA * n
    out = np.zeros(max(capacity, 1), np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    line_capacity = text.count(b"\n") + 1
    lines = np.zeros(line_capacity, TBX_LINE)
    src_off = np.zeros(line_capacity, np.uint64)
    n_lines, bad = C.c_uint64(0), C.c_uint64(0)
    hip._check(L.svt_vcf_bgzf_device(buf.ctypes.data, len(text), int(bool(sort)), int(check_huffman(huffman) == "dynamic"), out.ctypes.data, capacity,
                                     out_off.ctypes.data, lines.ctypes.data, line_capacity, C.addressof(n_lines), src_off.ctypes.data,
                                     C.addressof(bad), int(device)))
    if bad.value:
        return None, None, None, None, int(bad.value)
    return out[:int(out_off[-1])], out_off, lines[:n_lines.value], src_off[:n_lines.value], 0


def vcf_lines_last_times() -> Dict[str, float]:
    """svt_vcf_lines_last_times: the line-table and gather kernels of this thread's last device call, from HIP events"""
    return _times(_LinesTimes, _need(*_LINES).svt_vcf_lines_last_times)


PASTE_LINE = np.dtype([("qual", np.float64), ("counts", np.uint32, (8,)), ("nonref", np.uint32), ("flags", np.uint32),
                       ("bad_input", np.uint32), ("bad_field", np.uint32), ("part_len", np.uint32), ("line_len", np.uint32)])    # svt_paste_line
PASTE_SUM_QUALS, PASTE_AFREQ, PASTE_SAFE, PASTE_LAYOUT_SHIFT = 1, 2, 4, 8
PASTE_SLOW_QUAL, PASTE_SLOW_COLUMNS, PASTE_SLOW_GT, PASTE_SLOW_ALLELE, PASTE_SLOW_ALT, PASTE_UNSAFE = 1, 2, 4, 8, 16, 32
PASTE_SLOW = PASTE_SLOW_QUAL | PASTE_SLOW_COLUMNS | PASTE_SLOW_GT | PASTE_SLOW_ALLELE | PASTE_SLOW_ALT
PASTE_BAD_QUAL, PASTE_BAD_COLUMNS, PASTE_BAD_GT, PASTE_BAD_ALLELE, PASTE_BAD_POS, PASTE_BAD_UNSAFE = 1, 2, 3, 4, 5, 6
PASTE_LAYOUTS = {"default": 0, "lane": 1, "quarter": 2, "wave": 3}


def vcf_paste(text: bytes, first_line, n_inputs: int, n_lines: int, flags: int, info_table: bytes = b"", device: Optional[int] = None,
              layout: str = "default"):
    """svt_vcf_paste_host (device None) / _device over one block: `text` holds n_lines lines of the master and of every input, file
    f's from line first_line[f] on.  (the pasted lines as bytes, results PASTE_LINE [n_lines], info); info: host_lines, and where a
    line cannot be written bad_line (1-based in the block), bad_file (0: the master, f: input f - 1), bad_kind, bad_field -- the
    bytes are then empty"""
    L = _need(*_PASTE)
    buf = _text_array(text)
    first_line = np.ascontiguousarray(first_line, np.uint64)
    if first_line.shape[0] != n_inputs + 1:
        raise ValueError("first_line has one entry for the master and one per input")
    info_buf = _text_array(info_table)
    # an output line is its master's and inputs' bytes, a QUAL and -- under PASTE_AFREQ -- "AF=...;NSAMP=..." with up to
    # 12 bytes per ALT, of which the master's line has less than it has bytes
    capacity = 14 * len(text) + (400 + len(info_table)) * max(n_lines, 1)
    out = np.empty(max(capacity, 1), np.uint8)
    results = np.zeros(max(n_lines, 1), PASTE_LINE)
    info = _PasteInfo()
    args = [buf.ctypes.data, len(text), first_line.ctypes.data, n_inputs, n_lines, int(flags) | PASTE_LAYOUTS[layout] << PASTE_LAYOUT_SHIFT,
            info_buf.ctypes.data, len(info_table), out.ctypes.data, capacity, results.ctypes.data, C.byref(info)]
    if device is None:
        hip._check(L.svt_vcf_paste_host(*args))
    else:
        hip._check(L.svt_vcf_paste_device(*args, int(device)))
    report = {name: int(getattr(info, name)) for name, _ in _PasteInfo._fields_ if name != "reserved"}
    return out[:info.out_len].tobytes(), results[:n_lines], report


def vcf_paste_last_times() -> Dict[str, float]:
    """svt_vcf_paste_last_times: the kernels of this thread's last svt_vcf_paste_device from HIP events, its copies on the host's clock"""
    return _times(_PasteTimes, _need(*_PASTE).svt_vcf_paste_last_times)


class _CohortRule:
    """the ctypes side of one rule over the lines of a cohort VCF: svt_vcf_<rule>_host, _device, _write, _take and _last_times.
    `middle`: the argument types of _host between (text, len) and (results, capacity, n_lines); `extra`, `device_extra` and
    `write_extra`: those of the rule's further arrays, in front of _host's info, of _device's device and of _write's out_off.
    `program`: the module the rule came with"""

    def __init__(self, rule, line, info, times, middle, extra=(), device_extra=(), write_extra=(), program=None):
        self.rule, self.line, self.info, self.times, self.middle = rule, line, info, times, middle
        self.extra, self.device_extra, self.write_extra, self.program = list(extra), list(device_extra), list(write_extra), program or rule

    def entry(self, L, name):
        return getattr(L, "svt_vcf_%s_%s" % (self.rule, name))

    def declare(self, L):
        if not hasattr(L, "svt_vcf_%s_host" % self.rule):           # (a library built before the rule lacks the symbols)
            return
        P, U64 = C.c_void_p, C.c_uint64
        host = [P, U64] + self.middle + [P, U64, P] + self.extra + [C.POINTER(self.info)]
        for name, argtypes in (("host", host), ("device", host + self.device_extra + [C.c_int]), ("take", [P, U64]),
                               ("last_times", [C.POINTER(self.times)]),
                               ("write", [P, U64, C.c_uint32, P, U64, P, U64, P, U64] + self.write_extra + [P, C.POINTER(self.info)])):
            self.entry(L, name).restype = C.c_int
            self.entry(L, name).argtypes = argtypes

    def lib(self):
        return _need("svt_vcf_%s_host" % self.rule, "svtyper_amd.%s" % self.program)

    def report(self, info) -> dict:
        report = {name: int(getattr(info, name)) for name, _ in self.info._fields_ if name != "bad_text"}
        report["bad_text"] = bytes(info.bad_text).decode("utf-8", "surrogateescape")
        return report

    def records(self, text, middle, device, extra=None, device_extra=()):
        """_host (device None) / _device over one block: (the records, one per line, the report).  extra(capacity) and
        `device_extra`: the values of the rule's further arguments, the former for `capacity` lines"""
        L = self.lib()
        buf = _text_array(text)
        capacity = text.count(b"\n") + 1
        extra = extra(capacity) if extra is not None else []
        results = np.zeros(capacity, self.line)
        n_lines = C.c_uint64(0)
        info = self.info()
        args = [buf.ctypes.data, len(text)] + middle + [results.ctypes.data, capacity, C.addressof(n_lines)] + list(extra) + [C.byref(info)]
        if device is None:
            hip._check(self.entry(L, "host")(*args))
        else:
            hip._check(self.entry(L, "device")(*args, *device_extra, int(device)))
        return results[:n_lines.value], self.report(info)

    def write(self, text, n_samples, info_table, format_table, results, extra=(), entries=None):
        """_write + _take: (the output text, out_off [entries + 1], the report).  `extra`: the values of the rule's further
        arguments; `entries`: how many pieces of text the call writes (None: one per record)"""
        L = self.lib()
        buf, inf, fmt = _text_array(text), _text_array(info_table), _text_array(format_table)
        results = np.ascontiguousarray(results, self.line)
        out_off = np.zeros((results.shape[0] if entries is None else entries) + 1, np.uint64)
        info = self.info()
        hip._check(self.entry(L, "write")(buf.ctypes.data, len(text), int(n_samples), inf.ctypes.data, len(info_table), fmt.ctypes.data,
                                          len(format_table), results.ctypes.data if results.shape[0] else None, results.shape[0], *extra,
                                          out_off.ctypes.data, C.byref(info)))
        out = np.empty(max(info.out_len, 1), np.uint8)
        hip._check(self.entry(L, "take")(out.ctypes.data, info.out_len))
        return out[:info.out_len].tobytes(), out_off, self.report(info)

    def last_times(self) -> Dict[str, float]:
        return _times(self.times, self.entry(self.lib(), "last_times"))


CLASSIFY_LINE = np.dtype([("median", np.float64), ("mad", np.float64), ("slope", np.float64), ("r2", np.float64), ("route", np.uint32),
                          ("verdict", np.uint32), ("n_pos", np.uint32), ("n_ref", np.uint32), ("n_alt", np.uint32), ("quorum", np.uint32),
                          ("n_regressed", np.uint32), ("flags", np.uint32)])         # svt_classify_line
CLASSIFY_CAPACITY, CLASSIFY_NO_GENDER = 4096, 255
CLASSIFY_VERBATIM, CLASSIFY_LOW, CLASSIFY_HIGH, CLASSIFY_DROPPED, CLASSIFY_SKIPPED = 0, 1, 2, 3, 4
(CLASSIFY_SLOW_HEAD, CLASSIFY_SLOW_FORMAT, CLASSIFY_SLOW_COLUMNS, CLASSIFY_SLOW_SAMPLE, CLASSIFY_SLOW_TOKEN, CLASSIFY_SLOW_CAPACITY,
 CLASSIFY_SLOW_GENDER, CLASSIFY_SLOW_KEYS) = 1, 2, 4, 8, 16, 32, 64, 128
CLASSIFY_SLOW, CLASSIFY_NEAR, CLASSIFY_DEL = 255, 256, 512
(CLASSIFY_BAD_COLUMNS, CLASSIFY_BAD_POS, CLASSIFY_BAD_QUAL, CLASSIFY_BAD_FORMAT, CLASSIFY_BAD_KEY, CLASSIFY_BAD_NUMBER, CLASSIFY_BAD_NONFINITE,
 CLASSIFY_BAD_GENDER) = 1, 2, 3, 4, 5, 6, 7, 8


_CLASSIFY = _CohortRule("classify", CLASSIFY_LINE, _ClassifyInfo, _ClassifyTimes,
                        [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_double, C.c_double])


def vcf_classify(text: bytes, male, female, excluded, format_table: bytes, slope_threshold: float, rsquared_threshold: float, skip=None,
                 device: Optional[int] = None):
    """svt_vcf_classify_host (device None) / _device over one block of body lines: (records CLASSIFY_LINE, one per line, info);
    male, female, excluded: one byte per sample of the header; skip: one byte per line or None.  info: host_lines, near_lines and,
    where the script dies on a line, bad_line (1-based in the block), bad_kind, bad_sample, bad_text"""
    tables = [np.ascontiguousarray(t, np.uint8) for t in (male, female, excluded)]
    n_samples = tables[0].shape[0]
    if any(t.shape != (n_samples,) for t in tables):
        raise ValueError("male, female and excluded hold one byte per sample")
    tables = [t if n_samples else np.zeros(1, np.uint8) for t in tables]
    if skip is not None:
        skip = np.ascontiguousarray(skip, np.uint8)
        if skip.shape[0] < text.count(b"\n") + 1 - (text.endswith(b"\n") or not text):
            raise ValueError("skip holds one byte per line")
    fmt = _text_array(format_table)
    return _CLASSIFY.records(text, [n_samples, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, fmt.ctypes.data,
                                    len(format_table), skip.ctypes.data if skip is not None else None, float(slope_threshold),
                                    float(rsquared_threshold)], device)


def vcf_classify_write(text: bytes, n_samples: int, info_table: bytes, format_table: bytes, results: np.ndarray):
    """svt_vcf_classify_write + _take: (the block's output text, out_off [lines + 1], info); where a line cannot be written (an
    unsupported call without END, SVLEN or a confidence interval) info has bad_line, bad_kind, bad_text and the text ends in
    front of that line"""
    return _CLASSIFY.write(text, n_samples, info_table, format_table, results)


def vcf_classify_last_times() -> Dict[str, float]:
    """svt_vcf_classify_last_times: the kernels of this thread's last svt_vcf_classify_device from HIP events, its copies on the host's clock"""
    return _CLASSIFY.last_times()


UPDATE_INFO_LINE = np.dtype([("pe", np.int64), ("sr", np.int64), ("sum_sq", np.uint64), ("num_pos", np.uint32), ("route", np.uint32),
                             ("flags", np.uint32), ("reserved", np.uint32)])      # svt_update_info_line; sum_sq: the double's bits
UPDATE_INFO_CAPACITY = 4096
UPDATE_INFO_RULE, UPDATE_INFO_PLAIN = 0, 1
(UPDATE_INFO_SLOW_HEAD, UPDATE_INFO_SLOW_FORMAT, UPDATE_INFO_SLOW_COLUMNS, UPDATE_INFO_SLOW_SAMPLE, UPDATE_INFO_SLOW_TOKEN,
 UPDATE_INFO_SLOW_CAPACITY, UPDATE_INFO_SLOW_KEYS) = 1, 2, 4, 8, 16, 32, 64
UPDATE_INFO_SLOW = 127
(UPDATE_INFO_BAD_COLUMNS, UPDATE_INFO_BAD_POS, UPDATE_INFO_BAD_QUAL, UPDATE_INFO_BAD_FORMAT, UPDATE_INFO_BAD_KEY, UPDATE_INFO_BAD_NUMBER,
 UPDATE_INFO_BAD_NONFINITE, UPDATE_INFO_BAD_OVERFLOW, UPDATE_INFO_BAD_EIGHT) = 1, 2, 3, 4, 5, 6, 7, 8, 9


_UPDATE_INFO = _CohortRule("update_info", UPDATE_INFO_LINE, _UpdateInfoReport, _UpdateInfoTimes, [C.c_uint32, C.c_void_p, C.c_uint64])


def vcf_update_info(text: bytes, n_samples: int, format_table: bytes, device: Optional[int] = None):
    """svt_vcf_update_info_host (device None) / _device over one block of body lines: (records UPDATE_INFO_LINE, one per line, info).
    info: host_lines and, where the script dies on a line, bad_line (1-based in the block), bad_kind, bad_sample, bad_text"""
    fmt = _text_array(format_table)
    return _UPDATE_INFO.records(text, [int(n_samples), fmt.ctypes.data, len(format_table)], device)


def vcf_update_info_write(text: bytes, n_samples: int, info_table: bytes, format_table: bytes, results: np.ndarray):
    """svt_vcf_update_info_write + _take: (the block's output text, out_off [lines + 1], info); where a line cannot be written info has
    bad_line, bad_kind, bad_text and the text ends in front of that line"""
    return _UPDATE_INFO.write(text, n_samples, info_table, format_table, results)


def vcf_update_info_last_times() -> Dict[str, float]:
    """svt_vcf_update_info_last_times: the kernels of this thread's last svt_vcf_update_info_device from HIP events, its copies on the
    host's clock"""
    return _UPDATE_INFO.last_times()


GROUP_LINE = np.dtype([("off", np.uint64), ("len", np.uint32), ("id_b", np.uint32), ("id_n", np.uint32), ("mate_b", np.uint32),
                       ("mate_n", np.uint32), ("flags", np.uint32), ("slow", np.uint32), ("bad", np.uint32)])     # svt_group_line
GROUP_OUT = np.dtype([("line", np.uint32), ("source", np.uint32)])                                                 # svt_group_out
GROUP_BND, GROUP_HAS_MATE, GROUP_CI = 1, 2, 4
GROUP_SLOW_HEAD, GROUP_SLOW_FORMAT, GROUP_SLOW_BARE, GROUP_SLOW_TOKEN, GROUP_SLOW_ALT = 1, 2, 4, 8, 16
GROUP_SLOW = 31
(GROUP_BAD_COLUMNS, GROUP_BAD_POS, GROUP_BAD_QUAL, GROUP_BAD_FORMAT, GROUP_BAD_KEY, GROUP_BAD_NUMBER, GROUP_BAD_BARE, GROUP_BAD_ALT,
 GROUP_BAD_EIGHT) = 1, 2, 3, 4, 5, 6, 7, 8, 9
GROUP_KEYS = ("SVTYPE", "MATEID", "END", "CIPOS", "CIEND")


_GROUP = _CohortRule("group", GROUP_LINE, _GroupReport, _GroupTimes, [C.c_uint32, C.c_void_p, C.c_uint64], extra=[C.c_void_p, C.c_void_p],
                     device_extra=[C.c_uint32], write_extra=[C.c_void_p, C.c_uint64], program="group_multiline")


def vcf_group(text: bytes, n_samples: int, format_table: bytes, device: Optional[int] = None, hash_bits: int = 64):
    """svt_vcf_group_host (device None) / _device over the WHOLE body: (lines GROUP_LINE, one per line, plan GROUP_OUT in output
    order, report).  report: host_lines, host_join, n_bnd and, where the script dies on a line, bad_line (1-based), bad_kind,
    bad_text; the plan then ends in front of that line"""
    fmt = _text_array(format_table)
    plan, n_plan = [], C.c_uint64(0)

    def plan_for(capacity):                         # (the records' capacity, from the one count of the body's lines)
        plan.append(np.zeros(2 * capacity, GROUP_OUT))
        return [plan[0].ctypes.data, C.addressof(n_plan)]

    lines, report = _GROUP.records(text, [int(n_samples), fmt.ctypes.data, len(format_table)], device, extra=plan_for,
                                   device_extra=[int(hash_bits)])
    return lines, plan[0][:n_plan.value], report


def vcf_group_write(text: bytes, n_samples: int, info_table: bytes, format_table: bytes, lines: np.ndarray, plan: np.ndarray):
    """svt_vcf_group_write + _take: (the output text of the plan, out_off [entries + 1], report)"""
    plan = np.ascontiguousarray(plan, GROUP_OUT)
    return _GROUP.write(text, n_samples, info_table, format_table, lines, extra=[plan.ctypes.data if plan.shape[0] else None, plan.shape[0]],
                        entries=plan.shape[0])


def vcf_group_last_times() -> Dict[str, float]:
    """svt_vcf_group_last_times: the kernels of this thread's last svt_vcf_group_device from HIP events, its copies on the host's clock"""
    return _GROUP.last_times()


def tbx_build(text: bytes, lines: np.ndarray, member_off, src_off=None, payload: int = DEFLATE_MAX_PAYLOAD, csi: bool = False):
    """svt_tbx_build + svt_tbx_take: (the uncompressed bytes of the .tbi, 0, 0), or (None, bad_line, bad_kind); csi=True:
    svt_csi_build_vcf + svt_csi_take, the uncompressed bytes of the .csi"""
    L = _need(*_CSI) if csi else _need(*_LINES)
    build, take = (L.svt_csi_build_vcf, L.svt_csi_take) if csi else (L.svt_tbx_build, L.svt_tbx_take)
    buf = _text_array(text)
    lines = np.ascontiguousarray(lines, TBX_LINE)
    member_off = np.ascontiguousarray(member_off, np.uint64)
    if member_off.shape[0] < 1:
        raise ValueError("member_off must hold n + 1 entries")
    src = None if src_off is None else np.ascontiguousarray(src_off, np.uint64)
    if src is not None and src.shape[0] != lines.shape[0]:
        raise ValueError("src_off must hold an entry per line")
    size, bad, kind = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    hip._check(build(buf.ctypes.data, len(text), src.ctypes.data if src is not None and src.size else None,
                     lines.ctypes.data if lines.size else None, lines.shape[0], member_off.ctypes.data, member_off.shape[0] - 1,
                     int(payload), C.addressof(size), C.addressof(bad), C.addressof(kind)))
    if bad.value:
        return None, int(bad.value), int(kind.value)
    out = np.zeros(max(size.value, 1), np.uint8)
    hip._check(take(out.ctypes.data, size.value))
    return out[:size.value].tobytes(), 0, 0


# ---- BAM records as spans: the span table, the order --sort-alignment writes, the .bai fold (include/svtyper_reads.h) -----------
BAM_SPAN = np.dtype([("off", np.uint64), ("len", np.uint64), ("key", np.uint64), ("tid", np.int32), ("beg", np.uint32),
                     ("end", np.uint32), ("flags", np.uint32)])      # svt_bam_span
BAM_UNMAPPED, BAM_NO_COOR, BAM_BAD, BAM_BEYOND = 1, 2, 4, 8
BAM_BAD_RECORD, BAM_BAD_TID, BAM_BAD_POS = 0x100, 0x200, 0x400
BAM_KIND_RECORD, BAM_KIND_TID, BAM_KIND_POS, BAM_KIND_BEYOND, BAM_KIND_KEY_BACK = 1, 2, 3, 4, 5


def bam_spans(data: bytes, rec_off, n_ref: int, device: Optional[int] = None) -> Tuple[np.ndarray, int, int]:
    """svt_bam_spans_host (device None) / _device: (the span table of the records data[rec_off[i] .. rec_off[i + 1]), one BAM_SPAN
    each; the AND of their keys; the OR)"""
    L = _need(*_SPANS)
    buf = _text_array(data)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = int(rec_off.shape[0]) - 1
    if n < 0:
        raise ValueError("rec_off must hold n + 1 entries")
    spans = np.zeros(max(n, 1), BAM_SPAN)
    key_and, key_or = C.c_uint64(0), C.c_uint64(0)
    args = [buf.ctypes.data, len(data), rec_off.ctypes.data, n, int(n_ref), spans.ctypes.data, C.addressof(key_and), C.addressof(key_or)]
    if device is None:
        hip._check(L.svt_bam_spans_host(*args))
    else:
        hip._check(L.svt_bam_spans_device(*args, int(device)))
    return spans[:n], int(key_and.value), int(key_or.value)


def bam_sort_order(spans: np.ndarray, device: Optional[int] = None):
    """svt_bam_sort_order_host (device None) / _device: (perm, 0, 0), or (None, the 1-based number of a record that cannot be
    sorted, why: BAM_KIND_*)"""
    L = _need(*_SPANS)
    spans = np.ascontiguousarray(spans, BAM_SPAN)
    n = spans.shape[0]
    perm = np.zeros(max(n, 1), np.uint64)
    bad, kind = C.c_uint64(0), C.c_uint32(0)
    args = [spans.ctypes.data if n else None, n, perm.ctypes.data, C.addressof(bad), C.addressof(kind)]
    if device is None:
        hip._check(L.svt_bam_sort_order_host(*args))
    else:
        hip._check(L.svt_bam_sort_order_device(*args, int(device)))
    return (None, int(bad.value), int(kind.value)) if bad.value else (perm[:n], 0, 0)


def bam_sorted_bgzf_device(data: bytes, rec_off, n_ref: int, sort: bool, huffman: str = "fixed", device: int = 0):
    """svt_bam_sorted_bgzf_device: `data` (the header in front of rec_off[0], the records behind it) up once; (members uint8,
    out_off uint64 [m + 1], member_start uint64 [m + 1], spans as written, perm uint64, 0, 0), or (None, None, None, None, None,
    bad_record, bad_kind) where sorting met a record that cannot be sorted"""
    L = _need(*_SPANS)
    buf = _text_array(data)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = int(rec_off.shape[0]) - 1
    if n < 0:
        raise ValueError("rec_off must hold n + 1 entries")
    member_capacity = n + len(data) // DEFLATE_MAX_PAYLOAD + 2
    capacity = len(data) + DEFLATE_SLOT_EXTRA * member_capacity
    out = np.zeros(max(capacity, 1), np.uint8)
    out_off = np.zeros(member_capacity + 1, np.uint64)
    member_start = np.zeros(member_capacity + 1, np.uint64)
    spans = np.zeros(max(n, 1), BAM_SPAN)
    perm = np.zeros(max(n, 1), np.uint64)
    n_members, bad, kind = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    hip._check(L.svt_bam_sorted_bgzf_device(buf.ctypes.data, len(data), rec_off.ctypes.data, n, int(n_ref), int(bool(sort)),
                                            int(check_huffman(huffman) == "dynamic"), out.ctypes.data, capacity, out_off.ctypes.data,
                                            member_capacity, C.addressof(n_members), member_start.ctypes.data, spans.ctypes.data,
                                            perm.ctypes.data, C.addressof(bad), C.addressof(kind), int(device)))
    if bad.value:
        return None, None, None, None, None, int(bad.value), int(kind.value)
    m = int(n_members.value)
    return out[:int(out_off[m])], out_off[:m + 1], member_start[:m + 1], spans[:n], perm[:n], 0, 0


def bam_sort_last_times() -> Dict[str, float]:
    """svt_bam_sort_last_times: the kernels of this thread's last device call over BAM spans, from HIP events (the sort's three
    summed over its passes), and `passes`: the digits the sort took"""
    return _times(_BamSortTimes, _need(*_SPANS).svt_bam_sort_last_times, ints=("passes",))


def bam_first(data, rec_off, device: Optional[int] = None, hash_bits: int = 64) -> Tuple[Optional[np.ndarray], int]:
    """svt_bam_first_host (device None) / _device: (keep, 0) -- keep[i] = 1 iff no record in front of record i of
    data[rec_off[i] .. rec_off[i + 1]) has its (query name, flag), one uint8 each --, or (None, the 1-based number of the first
    record that is not well-formed).  `hash_bits` (the device alone): the low bits of the key's hash the device sorts by."""
    L = _need(*_FIRST)
    buf = _text_array(data)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = int(rec_off.shape[0]) - 1
    if n < 0:
        raise ValueError("rec_off must hold n + 1 entries")
    keep = np.zeros(max(n, 1), np.uint8)
    n_kept, bad = C.c_uint64(0), C.c_uint64(0)
    args = [buf.ctypes.data, len(data), rec_off.ctypes.data, n, keep.ctypes.data, C.addressof(n_kept), C.addressof(bad)]
    if device is None:
        hip._check(L.svt_bam_first_host(*args))
    else:
        hip._check(L.svt_bam_first_device(*args, int(hash_bits), int(device)))
    if bad.value:
        return None, int(bad.value)
    keep = keep[:n]
    if int(keep.sum()) != n_kept.value:
        raise hip.SvtyperHipError("svt_bam_first: n_kept is not the sum of keep")
    return keep, 0


def bam_first_last_times() -> Dict[str, float]:
    """svt_bam_first_last_times: the kernels of this thread's last svt_bam_first_device, from HIP events (the sort's three summed
    over its passes), and `passes`: the digits the sort took"""
    return _times(_BamFirstTimes, _need(*_FIRST).svt_bam_first_last_times, ints=("passes",))


def bai_build(spans: np.ndarray, n_ref: int, member_start, member_off):
    """svt_bai_build + svt_bai_take: (the bytes of the .bai, 0, 0), or (None, bad_record, bad_kind).  `spans`: the table of the
    stream as written; member k holds its bytes [member_start[k], member_start[k + 1]) and begins at file offset member_off[k]"""
    L = _need(*_SPANS)
    spans = np.ascontiguousarray(spans, BAM_SPAN)
    member_start = np.ascontiguousarray(member_start, np.uint64)
    member_off = np.ascontiguousarray(member_off, np.uint64)
    if member_start.shape[0] < 1 or member_start.shape[0] != member_off.shape[0]:
        raise ValueError("member_start and member_off must hold n + 1 entries each")
    size, bad, kind = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    hip._check(L.svt_bai_build(spans.ctypes.data if spans.size else None, spans.shape[0], int(n_ref), member_start.ctypes.data,
                               member_off.ctypes.data, member_start.shape[0] - 1, C.addressof(size), C.addressof(bad), C.addressof(kind)))
    if bad.value:
        return None, int(bad.value), int(kind.value)
    out = np.zeros(max(size.value, 1), np.uint8)
    hip._check(L.svt_bai_take(out.ctypes.data, size.value))
    return out[:size.value].tobytes(), 0, 0


# ---- a CSI index for the sorted outputs: the depth, the BAM's fold on the host and on the device (include/svtyper_reads.h) ----------
def csi_depth(max_end: int) -> int:
    """svt_csi_depth: the depth of the scheme (14, depth) a file gets whose largest end (BAM: longest l_ref) is `max_end`"""
    return int(_need(*_CSI).svt_csi_depth(int(max_end)))


def _member_tables(member_start, member_off):
    member_start = np.ascontiguousarray(member_start, np.uint64)
    member_off = np.ascontiguousarray(member_off, np.uint64)
    if member_start.shape[0] < 1 or member_start.shape[0] != member_off.shape[0]:
        raise ValueError("member_start and member_off must hold n + 1 entries each")
    return member_start, member_off


def _csi_taken(L, size, bad, kind):
    if bad.value:
        return None, int(bad.value), int(kind.value)
    out = np.zeros(max(size.value, 1), np.uint8)
    hip._check(L.svt_csi_take(out.ctypes.data, size.value))
    return out[:size.value].tobytes(), 0, 0


def csi_build_bam(spans: np.ndarray, n_ref: int, l_ref_max: int, member_start, member_off, device: Optional[int] = None):
    """svt_csi_build_bam (device None) / svt_bam_index_fold_device, + svt_csi_take: (the uncompressed bytes of the .csi, 0, 0), or
    (None, bad_record, bad_kind).  Arguments as bai_build; `l_ref_max`: the longest reference of the header"""
    L = _need(*_CSI)
    spans = np.ascontiguousarray(spans, BAM_SPAN)
    member_start, member_off = _member_tables(member_start, member_off)
    size, bad, kind = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    args = [spans.ctypes.data if spans.size else None, spans.shape[0], int(n_ref), int(l_ref_max), member_start.ctypes.data, member_off.ctypes.data,
            member_start.shape[0] - 1, C.addressof(size), C.addressof(bad), C.addressof(kind)]
    if device is None:
        hip._check(L.svt_csi_build_bam(*args))
    else:
        hip._check(L.svt_bam_index_fold_device(*args, int(device)))
    return _csi_taken(L, size, bad, kind)


def bam_sorted_bgzf_csi_device(data: bytes, rec_off, n_ref: int, l_ref_max: int, sort: bool, huffman: str = "fixed", device: int = 0):
    """svt_bam_sorted_bgzf_csi_device: bam_sorted_bgzf_device with the CSI fold on the device behind the members -- (members, out_off,
    member_start, spans, perm, csi bytes or None, index_bad, index_kind, 0, 0), or (None, ..., bad_record, bad_kind) where sorting
    met a record that cannot be sorted.  index_bad: the 1-based number, in written order, of a record the index cannot hold"""
    L = _need(*_CSI)
    buf = _text_array(data)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n = int(rec_off.shape[0]) - 1
    if n < 0:
        raise ValueError("rec_off must hold n + 1 entries")
    member_capacity = n + len(data) // DEFLATE_MAX_PAYLOAD + 2
    capacity = len(data) + DEFLATE_SLOT_EXTRA * member_capacity
    out = np.zeros(max(capacity, 1), np.uint8)
    out_off = np.zeros(member_capacity + 1, np.uint64)
    member_start = np.zeros(member_capacity + 1, np.uint64)
    spans = np.zeros(max(n, 1), BAM_SPAN)
    perm = np.zeros(max(n, 1), np.uint64)
    n_members, bad, kind, size = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    index_bad, index_kind = C.c_uint64(0), C.c_uint32(0)
    hip._check(L.svt_bam_sorted_bgzf_csi_device(buf.ctypes.data, len(data), rec_off.ctypes.data, n, int(n_ref), int(l_ref_max), int(bool(sort)),
                                                int(check_huffman(huffman) == "dynamic"), out.ctypes.data, capacity, out_off.ctypes.data,
                                                member_capacity, C.addressof(n_members), member_start.ctypes.data, spans.ctypes.data,
                                                perm.ctypes.data, C.addressof(bad), C.addressof(kind), C.addressof(size),
                                                C.addressof(index_bad), C.addressof(index_kind), int(device)))
    if bad.value:
        return None, None, None, None, None, None, 0, 0, int(bad.value), int(kind.value)
    m = int(n_members.value)
    csi, ibad, ikind = _csi_taken(L, size, index_bad, index_kind)
    return out[:int(out_off[m])], out_off[:m + 1], member_start[:m + 1], spans[:n], perm[:n], csi, ibad, ikind, 0, 0


def bam_index_last_times() -> Dict[str, float]:
    """svt_bam_index_last_times: the kernels of this thread's last device fold, from HIP events; `runs`, and `passes` of the runs' sort"""
    return _times(_BamIndexTimes, _need(*_CSI).svt_bam_index_last_times, ints=("runs", "passes"))


# ---- VCF text as a BCF2.2 stream: the records on the host and on the device (include/svtyper_bcf.h) ----------
BCF_KINDS = {1: "columns", 2: "contig", 3: "pos", 4: "filter", 5: "info_key", 6: "format_key", 7: "info_value", 8: "format_value",
             9: "samples", 10: "qual"}     # SVT_BCF_KIND_*
BCF_SORT, BCF_EXACT_FLOATS = 1, 2


class _BcfInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("bytes_len", "n_offsets", "n_records", "header_len", "stream_len", "bad_line", "host_lines",
                                                "l_ref_max")] + [("bad_kind", C.c_uint32), ("bad_at", C.c_uint32), ("n_ref", C.c_int32),
                                                                 ("n_sample", C.c_uint32)]


class _BcfTimes(C.Structure):
    _fields_ = [("measure_kernel_s", C.c_double), ("write_kernel_s", C.c_double), ("total_s", C.c_double)]


_bcf_declared = False


def _bcf_lib():
    global _bcf_declared
    L = _lib()
    if not hasattr(L, "svt_bcf_encode_host"):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bcf_encode_host (built before BCF output)")
    if not _bcf_declared:
        P, U64, U32, INFO = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(_BcfInfo)
        for name, argtypes in (("svt_bcf_encode_host", [P, U64, U32, INFO]), ("svt_bcf_encode_device", [P, U64, U32, INFO, C.c_int]),
                               ("svt_bcf_bgzf_device", [P, U64, U32, U32, INFO, C.c_int]), ("svt_bcf_take", [P, U64, P, U64, P, P, U64]),
                               ("svt_bcf_last_times", [C.POINTER(_BcfTimes)])):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = argtypes
        _bcf_declared = True
    return L


def _bcf_taken(L, info, members: bool) -> dict:
    """the fields of `info`, and with no refusal what the call left: bytes (uint8), offsets (uint64), spans (BAM_SPAN) and, for
    members, starts (uint64)"""
    got = {name: int(getattr(info, name)) for name, _ in _BcfInfo._fields_}
    if info.bad_line:
        return got
    data = np.zeros(max(info.bytes_len, 1), np.uint8)
    offsets = np.zeros(max(info.n_offsets, 1), np.uint64)
    starts = np.zeros(max(info.n_offsets, 1), np.uint64)
    spans = np.zeros(max(info.n_records, 1), BAM_SPAN)
    hip._check(L.svt_bcf_take(data.ctypes.data, info.bytes_len, offsets.ctypes.data, info.n_offsets, starts.ctypes.data if members else None,
                              spans.ctypes.data, info.n_records))
    got.update(bytes=data[:info.bytes_len], offsets=offsets[:info.n_offsets], spans=spans[:info.n_records])
    if members:
        got["starts"] = starts[:info.n_offsets]
    return got


def bcf_encode(text: bytes, sort: bool = False, device: Optional[int] = None, exact_floats: bool = False) -> dict:
    """svt_bcf_encode_host (device None) / _device, + svt_bcf_take: the BCF2.2 stream of the VCF `text` -- a dict of svt_bcf_info's
    fields and, where bad_line is 0, `bytes` (header_len bytes of header, then the records), `offsets` (records + 1) and `spans`.
    `exact_floats` (the host alone): floats by the device's rule first, so that host_lines counts what the device would hand over"""
    L = _bcf_lib()
    buf = _text_array(text)
    info = _BcfInfo()
    flags = (BCF_SORT if sort else 0) | (BCF_EXACT_FLOATS if exact_floats and device is None else 0)
    if device is None:
        hip._check(L.svt_bcf_encode_host(buf.ctypes.data, len(text), flags, C.byref(info)))
    else:
        hip._check(L.svt_bcf_encode_device(buf.ctypes.data, len(text), flags, C.byref(info), int(device)))
    return _bcf_taken(L, info, False)


def bcf_bgzf_device(text: bytes, sort: bool = False, huffman: str = "fixed", device: int = 0) -> dict:
    """svt_bcf_bgzf_device + svt_bcf_take: `text` up once; as bcf_encode, with `bytes` the BGZF members of the stream side by side,
    `offsets` where each begins in them and `starts` where each member's payload begins in the stream (members + 1 each)"""
    L = _bcf_lib()
    buf = _text_array(text)
    info = _BcfInfo()
    hip._check(L.svt_bcf_bgzf_device(buf.ctypes.data, len(text), BCF_SORT if sort else 0, int(check_huffman(huffman) == "dynamic"), C.byref(info),
                                     int(device)))
    return _bcf_taken(L, info, True)


def bcf_last_times() -> Dict[str, float]:
    """svt_bcf_last_times: the two kernels of this thread's last device call over BCF records, from HIP events"""
    return _times(_BcfTimes, _bcf_lib().svt_bcf_last_times)


# ---- an inflated BCF2.2 stream back to VCF text: the lines on the host and on the device (include/svtyper_bcf.h) ----------
BCF_TEXT_KINDS = {1: "truncated", 2: "index", 3: "samples", 4: "type", 5: "count", 6: "gt", 7: "length"}     # SVT_BCF_TEXT_KIND_*
BCF_TEXT_EXACT_FLOATS = 2


class _BcfTextInfo(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("text_len", "n_offsets", "n_records", "header_len", "bad_record", "host_lines", "chunks")] + [
        ("bad_kind", C.c_uint32), ("n_sample", C.c_uint32)]


class _BcfTextTimes(C.Structure):
    _fields_ = [(name, C.c_double) for name in ("measure_kernel_s", "write_kernel_s", "upload_s", "download_s", "total_s")]


_bcf_text_declared = False


def _bcf_text_lib():
    global _bcf_text_declared
    L = _lib()
    if not hasattr(L, "svt_bcf_text_host"):
        raise hip.SvtyperHipError("this libsvtyper_hip.so has no svt_bcf_text_host (built before BCF input)")
    if not _bcf_text_declared:
        P, U64, U32, INFO = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(_BcfTextInfo)
        for name, argtypes in (("svt_bcf_text_host", [P, U64, U32, U64, INFO]), ("svt_bcf_text_device", [P, U64, U32, U64, INFO, C.c_int]),
                               ("svt_bcf_text_take", [P, U64, P, U64, P, U64]), ("svt_bcf_text_last_times", [C.POINTER(_BcfTextTimes)])):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = argtypes
        _bcf_text_declared = True
    return L


def bcf_text(stream: bytes, device: Optional[int] = None, block_bytes: Optional[int] = None, exact_floats: bool = False) -> dict:
    """svt_bcf_text_host (device None) / _device, + svt_bcf_text_take: the VCF text of the inflated BCF2.2 `stream` -- a dict of
    svt_bcf_text_info's fields and, where bad_record is 0, `text` (uint8: header_len bytes of header, then one line per record),
    `offsets` (records + 1: where each line begins) and `marks` (uint8 per record: 1 where the host twin wrote it for a float outside
    the device's envelope).  `block_bytes`: the records run in chunks of at most that much stream (None: one chunk).  `exact_floats`
    (the host alone): floats by the device's rule first, so that host_lines and marks are what the device route reports"""
    L = _bcf_text_lib()
    buf = _text_array(stream)
    info = _BcfTextInfo()
    block = 0 if block_bytes is None else max(int(block_bytes), 1)
    if device is None:
        hip._check(L.svt_bcf_text_host(buf.ctypes.data, len(stream), BCF_TEXT_EXACT_FLOATS if exact_floats else 0, block, C.byref(info)))
    else:
        hip._check(L.svt_bcf_text_device(buf.ctypes.data, len(stream), 0, block, C.byref(info), int(device)))
    got = {name: int(getattr(info, name)) for name, _ in _BcfTextInfo._fields_}
    if info.bad_record:
        return got
    text = np.zeros(max(info.text_len, 1), np.uint8)
    offsets = np.zeros(max(info.n_offsets, 1), np.uint64)
    marks = np.zeros(max(info.n_records, 1), np.uint8)
    hip._check(L.svt_bcf_text_take(text.ctypes.data, info.text_len, offsets.ctypes.data, info.n_offsets, marks.ctypes.data, info.n_records))
    got.update(text=text[:info.text_len], offsets=offsets[:info.n_offsets], marks=marks[:info.n_records])
    return got


def bcf_text_last_times() -> Dict[str, float]:
    """svt_bcf_text_last_times: the kernels and copies of this thread's last bcf_text on a device, from HIP events, summed over its
    chunks, and the call's wall time"""
    return _times(_BcfTextTimes, _bcf_text_lib().svt_bcf_text_last_times)
