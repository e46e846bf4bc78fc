"""ctypes mirror of include/ngm_pipeline.h: HBM-resident reference + k-mer index, candidate search and the
single-end mapping path.  Used by the tests, bench.py and the ngm-style command line (nextgenmap_amd.cli)."""
import ctypes as C

import numpy as np

from .engine import NgmHipError, load_library


class RefParams(C.Structure):
    _fields_ = [("kmer", C.c_int), ("kmer_skip", C.c_int), ("bin_size", C.c_int)]


class MapperParams(C.Structure):
    _fields_ = [("qry_max_len", C.c_int), ("corridor", C.c_int), ("match_bonus", C.c_int), ("mismatch_penalty", C.c_int),
                ("gap_read_penalty", C.c_int), ("gap_ref_penalty", C.c_int), ("mode", C.c_int), ("variant", C.c_int),
                ("sensitivity", C.c_float), ("kmer_min", C.c_float), ("max_cmrs", C.c_int), ("max_kfreq", C.c_int),
                ("hard_clip", C.c_int), ("silent_clip", C.c_int), ("personality", C.c_int), ("gap_extend_penalty", C.c_int),
                ("min_insert_size", C.c_int), ("max_insert_size", C.c_int), ("pair_score_cutoff", C.c_float),
                ("topn", C.c_int), ("strata", C.c_int), ("bs_mapping", C.c_int), ("bs_cutoff", C.c_int), ("bs_read_skip", C.c_int),
                ("match_bonus_tt", C.c_int), ("match_bonus_tc", C.c_int), ("slam_seq", C.c_int)]


class SamOptions(C.Structure):   # ngm_sam_options
    _fields_ = [("paired", C.c_int), ("min_insert_size", C.c_int), ("max_insert_size", C.c_int), ("min_mq", C.c_int),
                ("min_identity", C.c_float), ("min_residues", C.c_float), ("no_unal", C.c_int), ("rg_id", C.c_char_p),
                ("bs_mapping", C.c_int), ("slam_seq", C.c_int), ("bam", C.c_int)]


HIT_DTYPE = np.dtype([("mapped", "i4"), ("contig", "i4"), ("pos", "u8"), ("reverse", "i4"), ("mapq", "i4"),
                      ("score", "f4"), ("identity", "f4"), ("nm", "i4"), ("qstart", "i4"), ("qend", "i4"),
                      ("n_candidates", "i4"), ("n_best", "i4"), ("max_votes", "f4"), ("pair_flags", "i4")], align=True)

_bound = False


class BamSortParams(C.Structure):   # ngm_bam_sort_params
    _fields_ = [("device", C.c_int), ("chunk_bytes", C.c_size_t), ("max_bytes", C.c_size_t)]


class CoverageParams(C.Structure):   # ngm_coverage_params
    _fields_ = [("device", C.c_int), ("n_ref", C.c_int), ("ref_len", C.POINTER(C.c_uint32)), ("ref_name", C.POINTER(C.c_char_p)), ("scan_chunk", C.c_size_t)]


class SnpParams(C.Structure):   # ngm_snp_params
    _fields_ = [("device", C.c_int), ("n_ref", C.c_int), ("ref_len", C.POINTER(C.c_uint32)), ("ref_name", C.POINTER(C.c_char_p)), ("ref_seq", C.POINTER(C.c_char_p)),
                ("min_cov", C.c_uint32), ("min_frac", C.c_double), ("min_qual", C.c_int), ("min_frac_text", C.c_char_p), ("scan_chunk", C.c_size_t)]


class CountParams(C.Structure):   # ngm_count_params
    _fields_ = [("device", C.c_int), ("n_ref", C.c_int), ("ref_len", C.POINTER(C.c_uint32)), ("ref_name", C.POINTER(C.c_char_p)), ("ref_seq", C.POINTER(C.c_char_p)),
                ("min_qual", C.c_int), ("n_regions", C.c_size_t), ("region_ref", C.c_void_p), ("region_start", C.c_void_p), ("region_end", C.c_void_p), ("region_strand", C.c_char_p)]


class MethylParams(C.Structure):   # ngm_methyl_params
    _fields_ = [("device", C.c_int), ("n_ref", C.c_int), ("ref_len", C.POINTER(C.c_uint32)), ("ref_name", C.POINTER(C.c_char_p)), ("ref_seq", C.POINTER(C.c_char_p)),
                ("min_qual", C.c_int), ("min_depth", C.c_int), ("context", C.c_char_p), ("scan_chunk", C.c_size_t)]


def _lib():
    global _bound
    lib = load_library()
    if not _bound:
        lib.ngm_pipeline_last_error.restype = C.c_char_p
        lib.ngm_ref_create.restype = C.c_void_p
        lib.ngm_ref_create.argtypes = [C.c_int, C.POINTER(RefParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_ref_create_from_fasta.restype = C.c_void_p
        lib.ngm_ref_create_from_fasta.argtypes = [C.c_int, C.POINTER(RefParams), C.c_char_p]
        lib.ngm_ref_create_from_fasta_vcf.restype = C.c_void_p
        lib.ngm_ref_create_from_fasta_vcf.argtypes = [C.c_int, C.POINTER(RefParams), C.c_char_p, C.c_char_p]
        lib.ngm_ref_vcf_summary.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_vcf_parse_text.restype = C.c_longlong
        lib.ngm_vcf_parse_text.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.ngm_ref_create_from_cache.restype = C.c_void_p
        lib.ngm_ref_create_from_cache.argtypes = [C.c_int, C.POINTER(RefParams), C.c_char_p]
        lib.ngm_ref_destroy.argtypes = [C.c_void_p]
        lib.ngm_ref_contig_count.argtypes = [C.c_void_p]
        lib.ngm_ref_contig_name.restype = C.c_char_p
        lib.ngm_ref_contig_name.argtypes = [C.c_void_p, C.c_int]
        for f in ("ngm_ref_contig_start", "ngm_ref_contig_len"):
            getattr(lib, f).restype = C.c_uint64
            getattr(lib, f).argtypes = [C.c_void_p, C.c_int]
        for f in ("ngm_ref_concat_len", "ngm_ref_index_entries"):
            getattr(lib, f).restype = C.c_uint64
            getattr(lib, f).argtypes = [C.c_void_p]
        lib.ngm_ref_auto_max_kfreq.argtypes = [C.c_void_p]
        lib.ngm_ref_index_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if not hasattr(lib, "ngm_mapper_create"):
            raise NgmHipError("libngm_hip.so was built without the mapping pipeline")
        lib.ngm_ref_write_ngm_cache.argtypes = [C.c_void_p, C.c_char_p]
        lib.ngm_ref_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        lib.ngm_ref_convert.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        lib.ngm_mapper_create.restype = C.c_void_p
        lib.ngm_mapper_create.argtypes = [C.c_void_p, C.POINTER(MapperParams)]
        lib.ngm_mapper_destroy.argtypes = [C.c_void_p]
        lib.ngm_mapper_cs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_cs_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_map_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_map_se_resident.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_map_pe_resident.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_cs_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_path_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_order_table_reads.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_heavy_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_search_turn_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_cs_dispatch.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_cs_max_combined.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        lib.ngm_mapper_last_order_replay_ms.restype = C.c_float
        lib.ngm_mapper_last_order_replay_ms.argtypes = [C.c_void_p]
        lib.ngm_mapper_set_argos.argtypes = [C.c_void_p, C.c_float]
        lib.ngm_mapper_map_argos.restype = C.c_longlong
        lib.ngm_mapper_map_argos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.POINTER(C.c_float)]
        lib.ngm_mapper_sam_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_mapper_set_sam_options.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_map_sam_trimmed.restype = C.c_longlong
        lib.ngm_mapper_map_sam_trimmed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
        lib.ngm_argos_prolog.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
        lib.ngm_mapper_argos_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_argos_path_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_debug_argos_order.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.ngm_debug_gather_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
        lib.ngm_debug_sam_records.restype = C.c_longlong
        lib.ngm_debug_sam_records.argtypes = ([C.c_int, C.POINTER(SamOptions)] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 +
                                              [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
        lib.ngm_bgzf_create.restype = C.c_void_p
        lib.ngm_bgzf_create.argtypes = [C.c_int]
        lib.ngm_bgzf_destroy.argtypes = [C.c_void_p]
        lib.ngm_bgzf_bound.restype = C.c_size_t
        lib.ngm_bgzf_bound.argtypes = [C.c_size_t]
        lib.ngm_bgzf_compress.restype = C.c_longlong
        lib.ngm_bgzf_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.ngm_bgzf_inflated_size.restype = C.c_size_t
        lib.ngm_bgzf_inflated_size.argtypes = [C.c_char_p, C.c_size_t]
        lib.ngm_bgzf_inflate.restype = C.c_longlong
        lib.ngm_bgzf_inflate.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.ngm_bgzf_last_kernel_ms.restype = C.c_float
        lib.ngm_bgzf_last_kernel_ms.argtypes = [C.c_void_p]
        lib.ngm_bam_sort_create.restype = C.c_void_p
        lib.ngm_bam_sort_create.argtypes = [C.POINTER(BamSortParams)]
        lib.ngm_bam_sort_destroy.argtypes = [C.c_void_p]
        lib.ngm_bam_sort_add.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        lib.ngm_bam_sort_finish.argtypes = [C.c_void_p, C.c_int]
        lib.ngm_bam_sort_next.restype = C.c_longlong
        lib.ngm_bam_sort_next.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_bam_sort_index.restype = C.c_longlong
        lib.ngm_bam_sort_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
        lib.ngm_bam_sort_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_bam_sort_set_markdup.argtypes = [C.c_void_p, C.c_int]
        lib.ngm_bam_sort_markdup_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_set_bam_sorter.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_coverage_create.restype = C.c_void_p
        lib.ngm_coverage_create.argtypes = [C.POINTER(CoverageParams)]
        lib.ngm_coverage_destroy.argtypes = [C.c_void_p]
        lib.ngm_coverage_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.ngm_coverage_finish.argtypes = [C.c_void_p]
        lib.ngm_coverage_next.restype = C.c_longlong
        lib.ngm_coverage_next.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_coverage_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_set_coverage.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_snp_create.restype = C.c_void_p
        lib.ngm_snp_create.argtypes = [C.POINTER(SnpParams)]
        lib.ngm_snp_create_for_ref.restype = C.c_void_p
        lib.ngm_snp_create_for_ref.argtypes = [C.c_void_p, C.POINTER(SnpParams)]
        lib.ngm_snp_destroy.argtypes = [C.c_void_p]
        lib.ngm_snp_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
        lib.ngm_snp_finish.argtypes = [C.c_void_p]
        lib.ngm_snp_next.restype = C.c_longlong
        lib.ngm_snp_next.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_snp_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_set_snp.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_count_create.restype = C.c_void_p
        lib.ngm_count_create.argtypes = [C.POINTER(CountParams)]
        lib.ngm_count_create_for_ref.restype = C.c_void_p
        lib.ngm_count_create_for_ref.argtypes = [C.c_void_p, C.POINTER(CountParams)]
        lib.ngm_count_destroy.argtypes = [C.c_void_p]
        lib.ngm_count_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t]
        lib.ngm_count_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_count_finish.argtypes = [C.c_void_p]
        lib.ngm_count_read.restype = C.c_longlong
        lib.ngm_count_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_count_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_methyl_create.restype = C.c_void_p
        lib.ngm_methyl_create.argtypes = [C.POINTER(MethylParams)]
        lib.ngm_methyl_create_for_ref.restype = C.c_void_p
        lib.ngm_methyl_create_for_ref.argtypes = [C.c_void_p, C.POINTER(MethylParams)]
        lib.ngm_methyl_destroy.argtypes = [C.c_void_p]
        lib.ngm_methyl_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t]
        lib.ngm_methyl_finish.argtypes = [C.c_void_p]
        lib.ngm_methyl_next.restype = C.c_longlong
        lib.ngm_methyl_next.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.ngm_methyl_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ngm_mapper_set_methyl.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_mapper_set_count.argtypes = [C.c_void_p, C.c_void_p]
        lib.ngm_debug_live_memory.argtypes = [C.c_void_p]
        _bound = True
    return lib


def _err():
    return NgmHipError(_lib().ngm_pipeline_last_error().decode())


def live_memory():
    """what the library holds in this process (ngm_debug_live_memory): device bytes live, pinned host bytes live, device allocations so
    far, pinned allocations so far"""
    out = np.zeros(4, np.uint64)
    if _lib().ngm_debug_live_memory(out.ctypes.data) < 0:
        raise _err()
    return dict(zip(("device_bytes", "pinned_bytes", "device_allocations", "pinned_allocations"), (int(x) for x in out)))


class Bgzf:
    """BGZF blocks written by the GPU (include/ngm_pipeline.h, ngm_bgzf_*): `ngm --bam`'s block compressor."""

    def __init__(self, device=0):
        self._h = _lib().ngm_bgzf_create(device)
        if not self._h:
            raise _err()

    def compress(self, data):
        lib = _lib()
        data = bytes(data)
        cap = lib.ngm_bgzf_bound(len(data))
        out = C.create_string_buffer(cap)
        n = lib.ngm_bgzf_compress(self._h, data, len(data), out, cap)
        if n < 0:
            raise _err()
        return out.raw[:n]

    def decompress(self, data):
        """the text of a run of whole BGZF members, inflated and CRC-checked by the GPU; raises on anything that is not one, and on the
        first member the GPU refuses (the message names its index)"""
        lib = _lib()
        data = bytes(data)
        cap = lib.ngm_bgzf_inflated_size(data, len(data))
        if cap == C.c_size_t(-1).value:
            raise RuntimeError("not a run of whole BGZF members")
        out = C.create_string_buffer(max(1, cap))
        n = lib.ngm_bgzf_inflate(self._h, data, len(data), out, cap)
        if n < 0:
            raise _err()
        return out.raw[:n]

    def last_kernel_ms(self):
        return float(_lib().ngm_bgzf_last_kernel_ms(self._h))

    def close(self):
        if self._h:
            _lib().ngm_bgzf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """A run-long object of the library behind self._h; _prefix names its functions (ngm_<prefix>_finish, ngm_<prefix>_destroy)."""
    _prefix = None
    _h = None

    def _fn(self, name):
        return getattr(_lib(), "ngm_%s_%s" % (self._prefix, name))

    def finish(self):
        if self._fn("finish")(self._h) < 0:
            raise _err()

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LineStream(_Handle):
    """... whose file comes back as text, in pieces of whole lines (ngm_<prefix>_next)."""

    def next(self, cap, out=None):
        """one ngm_<prefix>_next call with a buffer of cap bytes: (return value, the bytes copied)"""
        if out is None:
            out = C.create_string_buffer(max(1, cap))
        n = self._fn("next")(self._h, out, cap)
        if n < 0:
            raise _err()
        return n, (C.string_at(out, n) if n <= cap else b"")

    def pieces(self, cap=1 << 20):
        """the file, in pieces of whole lines (an SnpCaller's header is the first)"""
        out = C.create_string_buffer(cap)
        while True:
            n, data = self.next(cap, out)
            if n == 0:
                return
            if n > cap:
                cap = n
                out = C.create_string_buffer(cap)
                continue
            yield data


def _pack_records(records, with_reverse):
    """the arrays of ngm_snp_add (and, with the strands, of ngm_count_add) from [(contig index, position, CIGAR, sequence, qualities or None
    [, reverse])]"""
    records = list(records)
    b = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    cig = [b(r[2]) for r in records]
    seq = [b(r[3]) for r in records]
    with_q = [r[4] is not None for r in records]
    if any(with_q) and not all(with_q):
        raise ValueError("records with and without qualities go into separate calls")
    qual = None
    if records and all(with_q):
        if any(len(r[4]) != len(sq) for r, sq in zip(records, seq)):
            raise ValueError("a quality string has another length than its sequence")
        qual = b"".join(b(r[4]) for r in records)
    off = np.zeros(len(cig) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c in cig], dtype=np.uint64)
    soff = np.zeros(len(seq) + 1, dtype=np.uint32)
    soff[1:] = np.cumsum([len(c) for c in seq], dtype=np.uint64)
    arrays = (np.array([r[0] for r in records], dtype=np.int32), np.array([r[1] for r in records], dtype=np.int32), off, b"".join(cig), soff, b"".join(seq), qual)
    return arrays + ((np.array([1 if r[5] else 0 for r in records], dtype=np.uint8),) if with_reverse else ())


class BamSorter(_Handle):
    """The BAM records of a run kept in GPU memory, sorted there into coordinate order and handed back as the BGZF members of the sorted
    file plus its BAI index (include/ngm_pipeline.h, ngm_bam_sort_*): what `ngm-hip --sort` writes.  markdup=True: finish() sets flag 0x400
    on duplicate records before it sorts them (`--markdup`; the rules: INTEGRATION.md)."""

    _prefix = "bam_sort"

    def __init__(self, device=0, chunk_bytes=0, max_bytes=0, markdup=False):
        p = BamSortParams(device, chunk_bytes, max_bytes)
        self._h = _lib().ngm_bam_sort_create(C.byref(p))
        if not self._h:
            raise _err()
        if markdup:
            self.set_markdup(True)

    def set_markdup(self, on):
        """only before the first add()"""
        if _lib().ngm_bam_sort_set_markdup(self._h, 1 if on else 0) < 0:
            raise _err()

    def markdup_stats(self):
        """after finish() with marking on"""
        counts = (C.c_uint64 * 6)()
        ms = (C.c_float * 2)()
        if _lib().ngm_bam_sort_markdup_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "newly_marked"), (int(x) for x in counts)))
        d.update(zip(("mark_ms", "sort_ms"), (float(x) for x in ms)))
        return d

    def add(self, seq, records):
        """a run of whole uncompressed BAM records; seq orders the runs"""
        records = bytes(records)
        if _lib().ngm_bam_sort_add(self._h, seq, records, len(records)) < 0:
            raise _err()

    def finish(self, n_ref):
        if _lib().ngm_bam_sort_finish(self._h, n_ref) < 0:
            raise _err()

    def members(self):
        """the sorted stream, one run of whole BGZF members per chunk"""
        lib = _lib()
        cap = 1 << 16
        out = C.create_string_buffer(cap)
        while True:
            n = lib.ngm_bam_sort_next(self._h, out, cap)
            if n < 0:
                raise _err()
            if n == 0:
                return
            if n > cap:
                cap = n
                out = C.create_string_buffer(cap)
                continue
            yield out.raw[:n]

    def index(self, first_member_offset):
        """the BAI file's bytes, after the last of members()"""
        lib = _lib()
        n = lib.ngm_bam_sort_index(self._h, first_member_offset, None, 0)
        if n < 0:
            raise _err()
        out = C.create_string_buffer(max(1, n))
        if lib.ngm_bam_sort_index(self._h, first_member_offset, out, n) != n:
            raise _err()
        return out.raw[:n]

    def stats(self):
        counts = (C.c_uint64 * 5)()
        ms = (C.c_float * 5)()
        if _lib().ngm_bam_sort_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(("records", "record_bytes", "members", "chunks", "bins"), (int(x) for x in counts)))
        d.update(zip(("keys_ms", "sort_ms", "gather_ms", "deflate_ms", "index_ms"), (float(x) for x in ms)))
        return d


class Coverage(_LineStream):
    """The per-base read depth of a run, counted in GPU memory and handed back as bedGraph text (include/ngm_pipeline.h, ngm_coverage_*):
    what `ngm-hip --coverage` writes.  contigs: [(name, length)]."""

    _prefix = "coverage"

    def __init__(self, contigs, device=0, scan_chunk=0):
        n = len(contigs)
        self._len = (C.c_uint32 * max(1, n))(*[int(l) for _, l in contigs])
        self._name = (C.c_char_p * max(1, n))(*[nm.encode() if isinstance(nm, str) else bytes(nm) for nm, _ in contigs])
        p = CoverageParams(device, n, self._len, self._name, scan_chunk)
        self._h = _lib().ngm_coverage_create(C.byref(p))
        if not self._h:
            raise _err()

    def add(self, alignments):
        """[(contig index, 0-based position, CIGAR text)]; raises on the first alignment the validator refuses, adding nothing"""
        alignments = list(alignments)
        cig = [c.encode() if isinstance(c, str) else bytes(c) for _, _, c in alignments]
        off = np.zeros(len(cig) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(c) for c in cig], dtype=np.uint64)
        self.add_arrays(np.array([a[0] for a in alignments], dtype=np.int32), np.array([a[1] for a in alignments], dtype=np.int32), off, b"".join(cig))

    def add_arrays(self, ref_id, pos0, cigar_off, cigar_text):
        ref_id = np.ascontiguousarray(ref_id, dtype=np.int32)
        pos0 = np.ascontiguousarray(pos0, dtype=np.int32)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint32)
        if len(pos0) != len(ref_id) or len(cigar_off) != len(ref_id) + 1:
            raise ValueError("ref_id, pos0 of n entries and cigar_off of n + 1")
        if _lib().ngm_coverage_add(self._h, ref_id.ctypes.data, pos0.ctypes.data, cigar_off.ctypes.data, bytes(cigar_text), len(ref_id)) < 0:
            raise _err()

    def stats(self):
        counts = (C.c_uint64 * 4)()
        ms = (C.c_float * 4)()
        if _lib().ngm_coverage_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(("alignments", "covered_bases", "runs", "text_bytes"), (int(x) for x in counts)))
        d.update(zip(("add_ms", "scan_ms", "runs_ms", "text_ms"), (float(x) for x in ms)))
        return d


class ConversionCounter(_Handle):
    """T>C conversion counts per region, counted in GPU memory (include/ngm_pipeline.h, ngm_count_*): what `ngm-hip --count` writes.
    contigs: [(name, sequence)]; regions: [(contig index, start, end, name, strand)], start 0-based, end exclusive, strand '+', '-' or '.';
    reference: a Reference whose resident genome is read instead (contigs then only names the contigs for tsv())."""

    _prefix = "count"
    HEADER = "#chrom\tstart\tend\tname\tstrand\tt_bases\tmasked\tcov_on_ts\tconv_on_ts\treads\ttc_reads\n"

    def __init__(self, contigs, regions, device=0, min_qual=27, reference=None):
        b = lambda x: x.encode() if isinstance(x, str) else bytes(x)
        self._regions = [(int(c), int(s), int(e), name, strand) for c, s, e, name, strand in regions]
        self._names = [nm.decode() if isinstance(nm, bytes) else nm for nm, _ in contigs]
        self._r_ref = np.array([r[0] for r in self._regions], dtype=np.int32)
        self._r_start = np.array([r[1] for r in self._regions], dtype=np.uint32)
        self._r_end = np.array([r[2] for r in self._regions], dtype=np.uint32)
        self._r_strand = b("".join(r[4] if r[4] else "?" for r in self._regions))
        p = CountParams()
        p.device, p.min_qual, p.n_regions = device, min_qual, len(self._regions)
        p.region_ref, p.region_start, p.region_end, p.region_strand = self._r_ref.ctypes.data, self._r_start.ctypes.data, self._r_end.ctypes.data, self._r_strand
        if reference is not None:
            self._ref = reference   # (it must outlive this object)
            self._h = _lib().ngm_count_create_for_ref(reference.h, C.byref(p))
        else:
            n = len(contigs)
            self._seq_bytes = [b(sq) for _, sq in contigs]
            self._len = (C.c_uint32 * max(1, n))(*[len(sq) for sq in self._seq_bytes])
            self._name = (C.c_char_p * max(1, n))(*[b(nm) for nm, _ in contigs])
            self._seq = (C.c_char_p * max(1, n))(*self._seq_bytes)
            p.n_ref, p.ref_len, p.ref_name, p.ref_seq = n, self._len, self._name, self._seq
            self._h = _lib().ngm_count_create(C.byref(p))
        if not self._h:
            raise _err()

    def add(self, records):
        """[(contig index, 0-based position, CIGAR text, sequence, qualities or None, reverse)]: all with qualities or all without; raises
        on the first record the validator refuses, adding nothing"""
        self.add_arrays(*_pack_records(records, True))

    def add_arrays(self, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text, reverse):
        ref_id = np.ascontiguousarray(ref_id, dtype=np.int32)
        pos0 = np.ascontiguousarray(pos0, dtype=np.int32)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint32)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint32)
        reverse = np.ascontiguousarray(reverse, dtype=np.uint8)
        if len(pos0) != len(ref_id) or len(reverse) != len(ref_id) or len(cigar_off) != len(ref_id) + 1 or len(seq_off) != len(ref_id) + 1:
            raise ValueError("ref_id, pos0, reverse of n entries and cigar_off, seq_off of n + 1")
        if _lib().ngm_count_add(self._h, ref_id.ctypes.data, pos0.ctypes.data, cigar_off.ctypes.data, bytes(cigar_text), seq_off.ctypes.data, bytes(seq_text),
                                None if qual_text is None else bytes(qual_text), reverse.ctypes.data, len(ref_id)) < 0:
            raise _err()

    def mask(self, positions):
        """[(contig index, 0-based position)] join the mask; positions outside every region are ignored"""
        positions = list(positions)
        ref_id = np.array([c for c, _ in positions], dtype=np.int32)
        pos0 = np.array([p for _, p in positions], dtype=np.int32)
        if _lib().ngm_count_mask(self._h, ref_id.ctypes.data, pos0.ctypes.data, len(positions)) < 0:
            raise _err()

    def read(self):
        """after finish(): int64[n_regions, 6] -- t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads"""
        out = np.zeros((len(self._regions), 6), dtype=np.int64)
        if _lib().ngm_count_read(self._h, out.ctypes.data, len(self._regions)) < 0:
            raise _err()
        return out

    def tsv(self):
        """after finish(): the file `ngm-hip --count-out` writes, as bytes"""
        rows = self.read().tolist()
        return (self.HEADER + "".join("%s\t%d\t%d\t%s\t%s\t%s\n" % (self._names[c], s, e, name, strand, "\t".join(str(x) for x in row))
                                      for (c, s, e, name, strand), row in zip(self._regions, rows))).encode()

    def stats(self):
        counts = (C.c_uint64 * 5)()
        ms = (C.c_float * 2)()
        if _lib().ngm_count_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(("alignments", "met_a_region", "eligible_columns", "conversions", "masked_positions"), (int(x) for x in counts)))
        d.update(zip(("add_ms", "reduce_ms"), (float(x) for x in ms)))
        return d


class SnpCaller(_LineStream):
    """The mismatch pileup of a run, counted in GPU memory, and its single-base substitution calls handed back as VCF text
    (include/ngm_pipeline.h, ngm_snp_*): what `ngm-hip --snp` writes.  contigs: [(name, sequence)]; min_frac: a number, or the text the
    header prints (its float() is the threshold); reference: a Reference whose resident genome is read instead (contigs is then not used)."""

    _prefix = "snp"

    def __init__(self, contigs, device=0, min_cov=10, min_frac="0.8", min_qual=15, scan_chunk=0, reference=None):
        b = lambda x: x.encode() if isinstance(x, str) else bytes(x)
        text = min_frac if isinstance(min_frac, (str, bytes)) else repr(float(min_frac))
        p = SnpParams()
        p.device, p.min_cov, p.min_frac, p.min_qual, p.min_frac_text, p.scan_chunk = device, min_cov, float(text), min_qual, b(text), scan_chunk
        if reference is not None:
            self._ref = reference   # (it must outlive this object)
            self._h = _lib().ngm_snp_create_for_ref(reference.h, C.byref(p))
        else:
            n = len(contigs)
            self._seq_bytes = [b(sq) for _, sq in contigs]
            self._len = (C.c_uint32 * max(1, n))(*[len(sq) for sq in self._seq_bytes])
            self._name = (C.c_char_p * max(1, n))(*[b(nm) for nm, _ in contigs])
            self._seq = (C.c_char_p * max(1, n))(*self._seq_bytes)
            p.n_ref, p.ref_len, p.ref_name, p.ref_seq = n, self._len, self._name, self._seq
            self._h = _lib().ngm_snp_create(C.byref(p))
        if not self._h:
            raise _err()

    def add(self, records):
        """[(contig index, 0-based position, CIGAR text, sequence, qualities or None)]: all with qualities or all without; raises on the
        first record the validator refuses, adding nothing"""
        self.add_arrays(*_pack_records(records, False))

    def add_arrays(self, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text=None):
        ref_id = np.ascontiguousarray(ref_id, dtype=np.int32)
        pos0 = np.ascontiguousarray(pos0, dtype=np.int32)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint32)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint32)
        if len(pos0) != len(ref_id) or len(cigar_off) != len(ref_id) + 1 or len(seq_off) != len(ref_id) + 1:
            raise ValueError("ref_id, pos0 of n entries and cigar_off, seq_off of n + 1")
        if _lib().ngm_snp_add(self._h, ref_id.ctypes.data, pos0.ctypes.data, cigar_off.ctypes.data, bytes(cigar_text), seq_off.ctypes.data, bytes(seq_text),
                              None if qual_text is None else bytes(qual_text), len(ref_id)) < 0:
            raise _err()

    def stats(self):
        counts = (C.c_uint64 * 5)()
        ms = (C.c_float * 4)()
        if _lib().ngm_snp_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(("alignments", "alt_bases", "calls", "text_bytes", "covered_bases"), (int(x) for x in counts)))
        d.update(zip(("add_ms", "scan_ms", "flag_ms", "text_ms"), (float(x) for x in ms)))
        return d


class MethylationCounter(_LineStream):
    """The per-cytosine methylation calls of a bisulfite run, counted in GPU memory, handed back as Bismark's cytosine report
    (include/ngm_pipeline.h, ngm_methyl_*): what `ngm-hip --bs-mapping --methyl` writes.  contigs: [(name, sequence)]; context: "all", "CpG",
    "CHG" or "CHH"; reference: a Reference whose resident genome is read instead (contigs is then not used)."""

    _prefix = "methyl"
    STATS = ("alignments", "lines", "cpg_meth", "cpg_unmeth", "chg_meth", "chg_unmeth", "chh_meth", "chh_unmeth")

    def __init__(self, contigs, device=0, min_qual=5, min_depth=1, context="all", scan_chunk=0, reference=None):
        b = lambda x: x.encode() if isinstance(x, str) else bytes(x)
        p = MethylParams()
        p.device, p.min_qual, p.min_depth, p.context, p.scan_chunk = device, min_qual, min_depth, b(context), scan_chunk
        if reference is not None:
            self._ref = reference   # (it must outlive this object)
            self._h = _lib().ngm_methyl_create_for_ref(reference.h, C.byref(p))
        else:
            n = len(contigs)
            self._seq_bytes = [b(sq) for _, sq in contigs]
            self._len = (C.c_uint32 * max(1, n))(*[len(sq) for sq in self._seq_bytes])
            self._name = (C.c_char_p * max(1, n))(*[b(nm) for nm, _ in contigs])
            self._seq = (C.c_char_p * max(1, n))(*self._seq_bytes)
            p.n_ref, p.ref_len, p.ref_name, p.ref_seq = n, self._len, self._name, self._seq
            self._h = _lib().ngm_methyl_create(C.byref(p))
        if not self._h:
            raise _err()

    def add(self, records):
        """[(contig index, 0-based position, CIGAR text, sequence, qualities or None, bottom)]: all with qualities or all without; raises
        on the first record the validator refuses, adding nothing"""
        self.add_arrays(*_pack_records(records, True))

    def add_arrays(self, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text, bottom):
        ref_id = np.ascontiguousarray(ref_id, dtype=np.int32)
        pos0 = np.ascontiguousarray(pos0, dtype=np.int32)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint32)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint32)
        bottom = np.ascontiguousarray(bottom, dtype=np.uint8)
        if len(pos0) != len(ref_id) or len(bottom) != len(ref_id) or len(cigar_off) != len(ref_id) + 1 or len(seq_off) != len(ref_id) + 1:
            raise ValueError("ref_id, pos0, bottom of n entries and cigar_off, seq_off of n + 1")
        if _lib().ngm_methyl_add(self._h, ref_id.ctypes.data, pos0.ctypes.data, cigar_off.ctypes.data, bytes(cigar_text), seq_off.ctypes.data, bytes(seq_text),
                                 None if qual_text is None else bytes(qual_text), bottom.ctypes.data, len(ref_id)) < 0:
            raise _err()

    def text(self, cap=1 << 20):
        """after finish(): the whole report"""
        return b"".join(self.pieces(cap))

    def stats(self):
        counts = (C.c_uint64 * 8)()
        ms = (C.c_float * 4)()
        if _lib().ngm_methyl_stats(self._h, counts, ms) < 0:
            raise _err()
        d = dict(zip(self.STATS, (int(x) for x in counts)))
        d.update(zip(("add_ms", "flag_ms", "select_ms", "text_ms"), (float(x) for x in ms)))
        return d


SAM_READ_DTYPE = np.dtype([("name_off", np.uint32), ("name_len", np.uint16), ("qual_len", np.uint16)])   # ngm_sam_read


def debug_sam_records(options, reads, quals, names, meta, hits, cigars, mds, contig_names, contig_lens, polya=None, reference=None, hard_clip=0, silent_clip=0,
                      variant=0, alt_scoring=0, device=0):
    """ngm_debug_sam_records: the GPU record writers over constructed results.  options: a SamOptions; reads, quals: n x q uint8; names: the
    name bytes; meta: SAM_READ_DTYPE[n]; hits: HIT_DTYPE[n]; cigars, mds: n byte strings; the contig table; polya: uint16[n] or None; reference:
    a Reference (needed with slam_seq).  Returns (the text or the uncompressed BAM records, the seven counters); raises NgmHipError, whose
    `code` is the entry's return value (-22: an input the kernels would index out of bounds with; nothing was launched)."""
    lib = _lib()
    reads, quals = np.ascontiguousarray(reads, dtype=np.uint8), np.ascontiguousarray(quals, dtype=np.uint8)
    n, q = reads.shape
    meta, hits = np.ascontiguousarray(meta, dtype=SAM_READ_DTYPE), np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if quals.shape != (n, q) or len(meta) != n or len(hits) != n or len(cigars) != n or len(mds) != n or (polya is not None and len(polya) != n):
        raise ValueError("one quality row, name, hit, CIGAR, MD and poly-A count per read")
    names = bytes(names)
    cg, md = (C.c_char_p * max(n, 1))(*cigars), (C.c_char_p * max(n, 1))(*mds)
    nc = len(contig_names)
    cn = (C.c_char_p * max(nc, 1))(*[s.encode() if isinstance(s, str) else s for s in contig_names])
    cl = (C.c_uint64 * max(nc, 1))(*contig_lens)
    pa = None if polya is None else np.ascontiguousarray(polya, dtype=np.uint16)
    counters = np.zeros(7, np.uint64)
    cap = max(1 << 16, n * (2 * q + 512))
    for _ in range(2):
        out = np.zeros(cap, np.uint8)
        total = lib.ngm_debug_sam_records(device, C.byref(options), int(hard_clip), int(silent_clip), int(variant), int(alt_scoring), n, q, reads.ctypes.data, quals.ctypes.data,
                                          names, len(names), meta.ctypes.data, hits.ctypes.data, cg, md, None if pa is None else pa.ctypes.data, nc, cn, cl,
                                          None if reference is None else reference.h, out.ctypes.data, cap, counters.ctypes.data)
        if total < 0:
            e = _err()
            e.code = int(total)
            raise e
        if total <= cap:
            return out[:total].tobytes(), [int(x) for x in counters]
        cap = int(total)
    raise NgmHipError("ngm_debug_sam_records: the text grew between two calls")


class Reference:
    """Encoded reference + k-mer index resident in HBM (SequenceProvider + CompactPrefixTable of NGM)."""

    def __init__(self, handle, kmer):
        self.lib = _lib()
        self.h = handle
        self.kmer = kmer

    @classmethod
    def from_contigs(cls, contigs, names=None, device=0, kmer=13, kmer_skip=2, bin_size=2):
        lib = _lib()
        n = len(contigs)
        arrs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]
        names = [("chr%d" % (i + 1)) if names is None else names[i] for i in range(n)]
        cn = (C.c_char_p * n)(*[s.encode() for s in names])
        cs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        cl = (C.c_uint64 * n)(*[a.size for a in arrs])
        p = RefParams(kmer, kmer_skip, bin_size)
        h = lib.ngm_ref_create(device, C.byref(p), n, cn, cs, cl)
        if not h:
            raise _err()
        return cls(h, kmer)

    @classmethod
    def from_fasta(cls, path, device=0, kmer=13, kmer_skip=2, bin_size=2, vcf=None):
        """vcf: a plain or gzip VCF whose variants' k-mers go into the index (ngm --vcf); not read when a cache is loaded"""
        lib = _lib()
        p = RefParams(kmer, kmer_skip, bin_size)
        if vcf is not None:
            h = lib.ngm_ref_create_from_fasta_vcf(device, C.byref(p), path.encode(), vcf.encode())
        else:
            h = lib.ngm_ref_create_from_fasta(device, C.byref(p), path.encode())
        if not h:
            raise _err()
        return cls(h, kmer)

    @classmethod
    def from_cache(cls, fasta_path, device=0, kmer=13, kmer_skip=2, bin_size=2):
        """NextGenMap's own <fasta>-enc.2.ngm / <fasta>-ht-<k>-<skip>.3.ngm cache files."""
        lib = _lib()
        p = RefParams(kmer, kmer_skip, bin_size)
        h = lib.ngm_ref_create_from_cache(device, C.byref(p), fasta_path.encode())
        if not h:
            raise _err()
        return cls(h, kmer)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ngm_ref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def vcf_summary(self):
        """dict of what the VCF added (None when the index was not built with one): the reference's `Loaded VCF` /
        `Built SNP region table` counts, the region entries stored and the zero slots"""
        out = (C.c_uint64 * 6)()
        if self.lib.ngm_ref_vcf_summary(self.h, out) != 1:
            return None
        return dict(zip(("variations", "snps", "indels", "ignored", "entries", "zero_slots"), [int(x) for x in out]))

    @property
    def contigs(self):
        return [(self.lib.ngm_ref_contig_name(self.h, i).decode(), int(self.lib.ngm_ref_contig_start(self.h, i)),
                 int(self.lib.ngm_ref_contig_len(self.h, i))) for i in range(self.lib.ngm_ref_contig_count(self.h))]

    @property
    def concat_len(self):
        return int(self.lib.ngm_ref_concat_len(self.h))

    @property
    def auto_max_kfreq(self):
        return self.lib.ngm_ref_auto_max_kfreq(self.h)

    @property
    def index_entries(self):
        return int(self.lib.ngm_ref_index_entries(self.h))

    def index_copy(self):
        nk = 1 << (2 * self.kmer)
        counts = np.zeros(nk, np.uint32)
        raw = np.zeros(nk, np.uint32)
        pos = np.zeros(max(1, self.index_entries), np.uint32)
        if self.lib.ngm_ref_index_copy(self.h, counts.ctypes.data, raw.ctypes.data, pos.ctypes.data) < 0:
            raise _err()
        return counts, raw, pos[:self.index_entries]

    def write_ngm_cache(self, fasta_path):
        """Write NextGenMap's own index/genome cache files next to fasta_path (the reference program then loads
        them instead of rebuilding)."""
        if self.lib.ngm_ref_write_ngm_cache(self.h, fasta_path.encode()) < 0:
            raise _err()

    def decode(self, offset, buffer_len):
        out = np.zeros(buffer_len, np.uint8)
        r = self.lib.ngm_ref_decode(self.h, offset, buffer_len, out.ctypes.data)
        if r < 0:
            raise _err()
        return bool(r), bytes(out)

    def argos_prolog(self, total_reads):
        """ScoreWriter::DoWriteProlog for this reference (ngm_argos_prolog)"""
        lib = _lib()
        n = lib.ngm_argos_prolog(self.h, total_reads, None, 0)
        if n < 0:
            raise _err()
        buf = C.create_string_buffer(n + 1)
        lib.ngm_argos_prolog(self.h, total_reads, buf, n + 1)
        return buf.raw[:n]

    def convert(self, pos):
        c, p = C.c_int(0), C.c_uint64(0)
        ok = self.lib.ngm_ref_convert(self.h, pos, C.byref(c), C.byref(p))
        return (c.value, p.value) if ok else None


class Mapper:
    """CS -> gather -> score -> top-1 selection -> align for single-end reads (one CS thread's worth of NGM)."""

    def __init__(self, ref, qry_max_len, corridor, sensitivity=0.5, match=10, mismatch=15, gap_read=20, gap_ref=20,
                 mode=0, variant=0, kmer_min=0.0, max_cmrs=2 ** 31 - 1, max_kfreq=0, hard_clip=0, silent_clip=0, personality=0,
                 gap_extend=0, min_insert_size=0, max_insert_size=1000, pair_score_cutoff=0.9, topn=1,
                 strata=0, bs_mapping=0, bs_cutoff=6, bs_read_skip=2, match_bonus_tt=4, match_bonus_tc=4, slam_seq=0):
        self.lib = _lib()
        self.ref = ref
        self.q, self.c = qry_max_len, corridor
        p = MapperParams(qry_max_len, corridor, match, mismatch, gap_read, gap_ref, mode, variant, sensitivity, kmer_min,
                         max_cmrs, max_kfreq, hard_clip, silent_clip, personality, gap_extend, min_insert_size, max_insert_size,
                         pair_score_cutoff, topn, strata, bs_mapping, bs_cutoff, bs_read_skip, match_bonus_tt, match_bonus_tc, slam_seq)
        self.topn = max(1, topn)
        self.h = self.lib.ngm_mapper_create(ref.h, C.byref(p))
        if not self.h:
            raise _err()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ngm_mapper_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def reads_to_rows(reads, q):
        """list of uint8 arrays / bytes -> [n, q] NUL padded, upper-cased, non-ACGT -> N, truncated to q-1
        (IParser.h:59-121)."""
        out = np.zeros((len(reads), q), np.uint8)
        lut = np.full(256, ord("N"), np.uint8)
        for a, b in zip(b"ACGTacgt", b"ACGTACGT"):
            lut[a] = b
        for i, r in enumerate(reads):
            a = np.frombuffer(bytes(r), dtype=np.uint8)[:q - 1]
            out[i, :a.size] = lut[a]
        return out

    def candidate_search(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n = rows.shape[0]
        offs = np.zeros(n + 1, np.uint32)
        mx = np.zeros(n, np.float32)
        if self.lib.ngm_mapper_cs(self.h, n, rows.ctypes.data, offs.ctypes.data, mx.ctypes.data) < 0:
            raise _err()
        tot = int(offs[-1])
        loc = np.zeros(max(1, tot), np.uint64)
        strand = np.zeros(max(1, tot), np.uint8)
        votes = np.zeros(max(1, tot), np.float32)
        if self.lib.ngm_mapper_cs_fetch(self.h, loc.ctypes.data, strand.ctypes.data, votes.ctypes.data) < 0:
            raise _err()
        return offs, mx, loc[:tot], strand[:tot], votes[:tot]

    def debug_gather_pairs(self, rows, pair_read, pair_loc, pair_sv, alt_dir=0, align_stage=False):
        """ngm_debug_gather_pairs: gather_pairs_kernel as the score stage (align_stage: the align stage) launches it, for pairs (read index,
        location, bit 0 of pair_sv = reverse strand) over `rows`.  -> (words uint32 [blocks, RW + FW, 64], lens uint16 [pairs], blk_rows
        uint16 [blocks], RW, FW)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        pr, pl, ps = (np.ascontiguousarray(a, dtype=np.uint32) for a in (pair_read, pair_loc, pair_sv))
        n = len(pr)
        assert rows.shape[1] == self.q and len(pl) == n and len(ps) == n
        dims = np.zeros(2, np.int32)
        if self.lib.ngm_debug_gather_pairs(self.h, 0, None, 0, None, None, None, 0, 0, dims.ctypes.data, None, None, None) < 0:
            raise _err()
        rw, fw, nb = int(dims[0]), int(dims[1]), (n + 63) // 64
        words, lens, blk_rows = np.zeros((nb, rw + fw, 64), np.uint32), np.zeros(max(n, 1), np.uint16), np.zeros(max(nb, 1), np.uint16)
        if self.lib.ngm_debug_gather_pairs(self.h, rows.shape[0], rows.ctypes.data, n, pr.ctypes.data, pl.ctypes.data, ps.ctypes.data, int(alt_dir), int(bool(align_stage)),
                                           dims.ctypes.data, words.ctypes.data, lens.ctypes.data, blk_rows.ctypes.data) < 0:
            raise _err()
        return words, lens[:n], blk_rows[:nb], rw, fw

    def map_pe_raw(self, rows, d_rows=None, out=None):
        """Paired-end: rows 2i and 2i+1 are mates.  Same outputs as map_se_raw."""
        return self.map_se_raw(rows, d_rows, out, paired=True)

    def map_pe(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        hits, cig, md = self.map_pe_raw(rows)
        return hits, [bytes(r).split(b"\0", 1)[0] for r in cig], [bytes(r).split(b"\0", 1)[0] for r in md]

    def map_se_raw(self, rows, d_rows=None, out=None, paired=False):
        """rows: [n, q] uint8 host array; d_rows: optional device copy (torch tensor / pointer).  Returns
        (hits, cigar bytes [n, 4q], md bytes [n, 4q]) without turning the strings into Python objects."""
        n = rows.shape[0]
        stride = 4 * max(1, self.q)
        if out is None:
            no = n * (1 if paired else self.topn)
            out = (np.zeros(no, HIT_DTYPE), np.zeros((no, stride), np.uint8), np.zeros((no, stride), np.uint8))
        hits, cig, md = out
        dp = None if d_rows is None else (d_rows.data_ptr() if hasattr(d_rows, "data_ptr") else int(d_rows))
        fn = self.lib.ngm_mapper_map_pe_resident if paired else self.lib.ngm_mapper_map_se_resident
        r = fn(self.h, n, rows.ctypes.data, dp, hits.ctypes.data, cig.ctypes.data, md.ctypes.data)
        if r < 0:
            raise _err()
        return hits, cig, md

    def map_se(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        hits, cig, md = self.map_se_raw(rows)
        return hits, [bytes(r).split(b"\0", 1)[0] for r in cig], [bytes(r).split(b"\0", 1)[0] for r in md]

    def set_coverage(self, coverage):
        """every batch map_sam finishes adds its mapped primary records to `coverage` (a Coverage, or None to detach)"""
        if self.lib.ngm_mapper_set_coverage(self.h, coverage._h if coverage is not None else None) < 0:
            raise _err()

    def set_count(self, count):
        """every batch map_sam finishes adds its mapped primary records to `count` (a ConversionCounter, or None to detach)"""
        if self.lib.ngm_mapper_set_count(self.h, count._h if count is not None else None) < 0:
            raise _err()
        self._count = count

    def set_methyl(self, methyl):
        """every batch map_sam finishes adds its mapped primary records to `methyl` (a MethylationCounter, or None to detach)"""
        if self.lib.ngm_mapper_set_methyl(self.h, methyl._h if methyl is not None else None) < 0:
            raise _err()
        self._methyl = methyl

    def set_snp(self, snp):
        """every batch map_sam finishes adds its mapped primary records to `snp` (a SnpCaller, or None to detach)"""
        if self.lib.ngm_mapper_set_snp(self.h, snp._h if snp is not None else None) < 0:
            raise _err()

    def set_bam_sorter(self, sorter):
        """map_sam(bam=True) hands its records to `sorter` (a BamSorter, or None to detach) instead of returning BGZF members"""
        if self.lib.ngm_mapper_set_bam_sorter(self.h, sorter._h if sorter is not None else None) < 0:
            raise _err()

    def last_kernel_ms(self):
        ms = (C.c_float * 8)()
        self.lib.ngm_mapper_last_kernel_ms(self.h, ms)
        return list(ms)

    def last_order_replay_ms(self):
        """GPU time of the candidate-order replays of the last call (their own stream)"""
        return float(self.lib.ngm_mapper_last_order_replay_ms(self.h))

    def path_counters(self):
        """summed over all batches: reads searched, candidates, reads re-run by the exact search (LDS table / global-memory table),
        reads whose candidate order was replayed, of those by the exact global-memory replay, reads left with an undetermined order"""
        out = np.zeros(8, np.uint64)
        self.lib.ngm_mapper_path_counters(self.h, out.ctypes.data)
        return dict(zip(("reads", "candidates", "exact_lds", "exact_global", "order_replayed", "order_exact_global", "order_undetermined", "heavy"), (int(x) for x in out[:8])))

    def heavy_counters(self):
        """of path_counters()["heavy"]: second passes, table passes started over, reads sent on to the exact kernels, regrown table pools"""
        out = np.zeros(4, np.uint64)
        self.lib.ngm_mapper_heavy_counters(self.h, out.ctypes.data)
        return dict(zip(("second_passes", "table_pass_restarts", "sent_on", "pool_regrown"), (int(x) for x in out)))

    def search_turn_counters(self):
        """of the last map call: per-read search arrays deferred behind the score stage (0/1), search attempts, buffers regrown inside the turn"""
        out = np.zeros(3, np.uint64)
        self.lib.ngm_mapper_search_turn_counters(self.h, out.ctypes.data)
        return dict(zip(("arrays_deferred", "search_attempts", "buffers_regrown"), (int(x) for x in out)))

    def cs_dispatch(self):
        """which first-pass kernel the last candidate search launched: canonical shape (0: one bucket per k-mer), waves per read of the
        fast path, work items per lane, 16-bit work items (0/1)"""
        out = np.zeros(4, np.uint64)
        self.lib.ngm_mapper_cs_dispatch(self.h, out.ctypes.data)
        return dict(zip(("cs_canon", "cs_waves", "cs_fast_items", "items16"), (int(x) for x in out)))

    def cs_max_combined(self, n):
        """after candidate_search of n reads: per read, the largest forward + reverse vote sum of one bin"""
        out = np.zeros(max(1, n), np.float32)
        if self.lib.ngm_mapper_cs_max_combined(self.h, out.ctypes.data) < 0:
            raise _err()
        return out[:n]

    def order_table_reads(self):
        """of path_counters()["order_exact_global"]: the reads the bucket replay left to the replay with a table in global memory"""
        out = np.zeros(1, np.uint64)
        self.lib.ngm_mapper_order_table_reads(self.h, out.ctypes.data)
        return int(out[0])

    def map_argos(self, reads, names, min_score=0.0):
        """`--argos` for one batch (ngm_mapper_map_argos): reads -- rows as from reads_to_rows, or a list of sequences --, names -- one
        per read (bytes or str) --, min_score: --argos-min-score (< 0: the mode off again).  Returns ScoreWriter's text for these reads
        (bytes: one line per read with candidates) and the stats (reads, reads with a line, 0)."""
        rows = reads if isinstance(reads, np.ndarray) else self.reads_to_rows(reads, self.q)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n = rows.shape[0]
        if len(names) != n:
            raise ValueError("one name per read")
        if self.lib.ngm_mapper_set_argos(self.h, float(min_score)) < 0:
            raise _err()
        nb = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        meta = np.zeros((n, 2), np.uint32)   # ngm_sam_read: name_off, name_len (qual_len unused)
        off = 0
        for i, b in enumerate(nb):
            meta[i, 0], meta[i, 1] = off, min(len(b), 0xFFFF)
            off += len(b)
        blob = np.frombuffer(b"".join(nb) + b"\0", np.uint8)
        stats = np.zeros(3, np.uint64)
        kms = C.c_float(0)
        cap = max(1 << 16, n * 64)
        out = np.zeros(cap, np.uint8)
        total = self.lib.ngm_mapper_map_argos(self.h, n, rows.ctypes.data, blob.ctypes.data, off, meta.ctypes.data, out.ctypes.data, cap,
                                              stats.ctypes.data, C.byref(kms))
        if total < 0:
            raise _err()
        if total > cap:
            out = np.zeros(total, np.uint8)
            if self.lib.ngm_mapper_sam_fetch(self.h, out.ctypes.data, total) < 0:
                raise _err()
        return out[:total].tobytes(), [int(x) for x in stats]

    def map_sam(self, reads, quals, names, polya_trimmed=None, paired=False, rg_id=None, slam_seq=0, bam=False, min_insert_size=0,
                max_insert_size=1000, min_mq=0, min_identity=0.65, min_residues=0.5, no_unal=False):
        """The records of one batch, written by the GPU (ngm_mapper_set_sam_options + ngm_mapper_map_sam_trimmed).  reads -- rows as from
        reads_to_rows, or a list of sequences, already trimmed (`-5`, `--max-polya`; an empty read is legal) --, quals -- one quality
        string per read (b"" for none) --, names -- one per read --, polya_trimmed -- per read, the bases --max-polya cut off: given, every
        record carries it as XA:i; None, no such tag (ngm_mapper_map_sam).  Returns the SAM text (bam: a piece of the BAM file, whole
        BGZF members) and the stats (reads counted, reads mapped, records written)."""
        rows = reads if isinstance(reads, np.ndarray) else self.reads_to_rows(reads, self.q)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n = rows.shape[0]
        if len(names) != n or len(quals) != n or (polya_trimmed is not None and len(polya_trimmed) != n):
            raise ValueError("one name, one quality string and one poly-A count per read")
        so = SamOptions(int(paired), min_insert_size, max_insert_size, min_mq, min_identity, min_residues, int(no_unal),
                        rg_id.encode() if isinstance(rg_id, str) else rg_id, 0, int(slam_seq), int(bam))
        if self.lib.ngm_mapper_set_sam_options(self.h, C.byref(so)) < 0:
            raise _err()
        nb = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        qrows = np.zeros((n, self.q), np.uint8)
        meta = np.zeros(n, np.dtype([("name_off", np.uint32), ("name_len", np.uint16), ("qual_len", np.uint16)]))   # ngm_sam_read
        off = 0
        for i, b in enumerate(nb):
            ql = quals[i].encode() if isinstance(quals[i], str) else bytes(quals[i])
            qrows[i, :min(len(ql), self.q - 1)] = np.frombuffer(ql[:self.q - 1], np.uint8)
            meta[i] = (off, min(len(b), 0xFFFF), min(len(ql), 0x7FFF))
            off += len(b)
        blob = np.frombuffer(b"".join(nb) + b"\0", np.uint8)
        polya = None if polya_trimmed is None else np.ascontiguousarray(polya_trimmed, dtype=np.uint16)
        stats = np.zeros(3, np.uint64)
        kms = C.c_float(0)
        cap = max(1 << 16, n * (2 * self.q + 512))
        out = np.zeros(cap, np.uint8)
        total = self.lib.ngm_mapper_map_sam_trimmed(self.h, n, rows.ctypes.data, qrows.ctypes.data, blob.ctypes.data, off, meta.ctypes.data,
                                                    None if polya is None else polya.ctypes.data, out.ctypes.data, cap, stats.ctypes.data, C.byref(kms))
        if total < 0:
            raise _err()
        if total > cap:
            out = np.zeros(total, np.uint8)
            got = self.lib.ngm_mapper_sam_fetch(self.h, out.ctypes.data, total)
            if got < 0:
                raise _err()
            if bam:
                total = got
        return out[:total].tobytes(), [int(x) for x in stats]

    def argos_counters(self):
        """summed over the map_argos calls: reads ordered in class U / S / H, entries written, reads of the long-list path, reads of class
        S / H ordered by position (candidate order unknown)"""
        out = np.zeros(4, np.uint64)
        self.lib.ngm_mapper_argos_counters(self.h, out.ctypes.data)
        p = np.zeros(2, np.uint64)
        self.lib.ngm_mapper_argos_path_counters(self.h, p.ctypes.data)
        return dict(zip(("U", "S", "H", "entries", "long_list", "unknown_order"), [int(x) for x in out] + [int(x) for x in p]))

    def cs_counters(self):
        """(k-mers looked up, index hits voted, candidates) of the last candidate search."""
        out = np.zeros(3, np.uint64)
        self.lib.ngm_mapper_cs_counters(self.h, out.ctypes.data)
        return [int(x) for x in out]
