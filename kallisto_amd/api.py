"""ctypes mirror of include/kallisto_amd.h plus the `quant` driver flow of the reference (src/main.cpp:2620-2798).

Names follow the reference: an *index* (KmerIndex), *pseudoalignment* of read batches into equivalence-class (EC)
counts (ProcessReads / MinCollector), the fragment-length distribution (FLD), effective lengths, the EM
(EMAlgorithm::run) and TPM.  Everything that computes goes through libkallisto_amd.so; if the library or a GPU is
missing the calls raise KallistoAmdError -- there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_FRAG_LEN = 1000


class KallistoAmdError(RuntimeError):
    pass


def library_path() -> str:
    return os.path.join(HERE, "libkallisto_amd.so")


class _View(C.Structure):
    _fields_ = ([("k", C.c_int32)] +
                [(n, C.c_uint64) for n in ("n_kmers", "n_unitigs", "n_blocks", "n_uec", "n_ecs", "ec_nnz", "n_targets",
                                           "dlist_size", "n_buckets", "pad_buckets")] +
                [(n, C.c_void_p) for n in ("table", "slot_block", "slot_dist", "uec_ec", "ec_off", "ec_ids",
                                           "unitig_blk_off", "unitig_len", "blk_unitig", "blk_lb", "blk_ub", "blk_ec",
                                           "blk_pos_off", "blk_posw", "blk_sense", "target_lens", "onlist_bits")] +
                [("onlist_words", C.c_uint64), ("dtable", C.c_void_p), ("n_dbuckets", C.c_uint64), ("dpad_buckets", C.c_uint64),
                 ("dummy_slot", C.c_uint64), ("dummy_uec", C.c_uint32), ("dummy_strand", C.c_uint32),
                 ("utext", C.c_void_p), ("utext_words", C.c_uint64), ("text_bases", C.c_uint64), ("unitig_gpos", C.c_void_p)] +
                [(n, C.c_uint32) for n in ("table_layout", "slots_per_bucket", "tag_q", "tag_dsh", "tag_w")] +
                # the shade tables: their addresses as integers, 0 when the index has no shade (n_shades == 0)
                [("n_shades", C.c_uint64), ("shade_colour", C.c_size_t),
                 ("core_off", C.c_size_t), ("core_ids", C.c_size_t), ("core_nnz", C.c_uint64),
                 ("shade_off", C.c_size_t), ("shade_ids", C.c_size_t), ("shade_nnz", C.c_uint64)])


class QuantOpts(C.Structure):
    """kamd_quant_opts: the subset of ProgramOptions (src/common.h:93-209) the hot path reads."""
    _fields_ = [("paired", C.c_int32), ("fld", C.c_double), ("sd", C.c_double), ("single_overhang", C.c_int32),
                ("strand", C.c_int32), ("no_jump", C.c_int32), ("do_union", C.c_int32)]


class _Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_processed", "n_single", "n_multi", "n_probes", "n_bucket_reads",
                                          "n_distinct_tuples", "n_stream_words", "n_raw_words", "n_text_hits", "n_wave_iters",
                                          "n_lane_iters", "n_classify_counted", "n_three_exact", "n_three_hashed")]


class Tuning(C.Structure):
    """kamd_tuning: which of the equivalent kernels / EM forms run (0 = keep the current value; on/off fields: 1 on, 2 off)."""
    _fields_ = [(n, C.c_int32) for n in ("text_verify", "items_per_wave", "refill_min", "lds_pad", "em_form", "em_entries_per_lane", "em_windowed", "em_graph", "em_row_lanes",
                                         "em_fin_blocks", "em_local_block", "em_group_div", "em_split_len", "dedup_form", "align_chunks", "em_small_nnz", "em_reg_slices",
                                         "em_hybrid", "overflow_second_pass", "em_giant_nnz", "em_blocked", "fld_list_cap", "fld_first_chunk", "classify_counts_short",
                                         "short_id_bits", "tup_max_probe", "classify_max_blocks", "match_continuous", "match_grant", "match_max_blocks")]


EM_FORMS = {"streamed": 1, "csr": 2, "local": 3}
ABI_VERSION = 16  # KAMD_ABI_VERSION of include/kallisto_amd.h


class _Profile(C.Structure):
    _fields_ = [("last_align_kernel_ms", C.c_float), ("last_em_ms", C.c_float), ("last_em_iters", C.c_uint64),
                ("last_classify_ms", C.c_float), ("kernel_a_version", C.c_int32), ("last_em_nnz", C.c_uint64),
                ("last_em_nnz_multi", C.c_uint64), ("last_em_nseg", C.c_uint64), ("last_em_necs", C.c_uint64),
                ("last_em_k", C.c_int32), ("last_em_grid", C.c_uint32), ("last_em_lds", C.c_uint32),
                ("last_em_plan_cached", C.c_int32), ("last_finalize_ms", C.c_float), ("last_fin_records", C.c_uint64),
                ("last_fin_stream_words", C.c_uint64), ("last_fin_cand_words", C.c_uint64), ("absorb_ms", C.c_float),
                ("n_distinct_tuples", C.c_uint64), ("tuple_store_words", C.c_uint64), ("tuple_table_slots", C.c_uint64),
                ("last_em_max_comp_nnz", C.c_uint64), ("last_em_giant_nnz", C.c_uint64), ("last_em_giant_rows", C.c_uint64),
                ("last_em_giant_tr", C.c_uint64), ("last_em_giant_chunks", C.c_uint32), ("last_em_graph_fallback", C.c_int32),
                ("last_em_plan_ms", C.c_float), ("n_overflow_items", C.c_uint64), ("overflow_ms", C.c_float),
                ("last_merge_ms", C.c_float), ("em_collective_ms", C.c_float), ("em_collectives", C.c_uint32), ("n_overflow_second_pass", C.c_uint64), ("last_em_giant_pieces", C.c_uint64),
                ("last_fld_chunks", C.c_uint32), ("last_fld_candidates", C.c_uint64), ("last_fld_list_overflows", C.c_uint64), ("last_fld_prefetched", C.c_int32)]


class _AaStats(C.Structure):
    """kamd_aa_stats: what the translated search did with the reads since the last reset."""
    _fields_ = [("n_processed", C.c_uint64), ("n_rejected_offlist", C.c_uint64), ("n_all_empty", C.c_uint64), ("n_frame_clashes", C.c_uint64),
                ("n_winner", C.c_uint64 * 6), ("last_translate_ms", C.c_float), ("last_match_ms", C.c_float),
                ("last_chunks", C.c_uint32), ("last_match_blocks", C.c_uint32), ("last_list_cap", C.c_uint32), ("reserved", C.c_uint32)]


class _ReadEcsStats(C.Structure):
    """kamd_read_ecs_stats: what one kamd_read_ecs call found."""
    _fields_ = [("n_items", C.c_uint64), ("n_mapped", C.c_uint64), ("n_none", C.c_uint64), ("n_foreign", C.c_uint64), ("last_ms", C.c_float)]


READ_EC_NONE = -1      # KAMD_READ_EC_NONE: the item is not pseudoaligned
READ_EC_FOREIGN = -2   # KAMD_READ_EC_FOREIGN: the item has a set that the context's EC result does not hold


BUS_MAX_PARTS = 8   # KAMD_BUS_MAX_PARTS
BUS_TAG_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("flags", "<u4"), ("bc_len", "<u2"), ("umi_len", "<u2")])            # kamd_bus_tag
BUS_RECORD_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])   # kamd_bus_record = BUSData
BUS_ENTRY_DTYPE = np.dtype([("row", "<u4"), ("ec", "<i4"), ("value", "<u4")])   # kamd_bus_entry
BUS_COUNT_UMIS, BUS_COUNT_READS = 0, 1   # KAMD_BUS_COUNT_*


class BusSubstr(C.Structure):
    """kamd_bus_substr: (file, start, stop) of one part of a field; stop == 0: to the end of the read; file == -1: the field is absent."""
    _fields_ = [("file", C.c_int32), ("start", C.c_int32), ("stop", C.c_int32)]


class BusLayout(C.Structure):
    """kamd_bus_layout: where barcode, UMI and sequence lie in the reads of a technology (`bus -x`)."""
    _fields_ = [("n_files", C.c_int32), ("n_bc", C.c_int32), ("n_umi", C.c_int32), ("reserved", C.c_int32),
                ("bc", BusSubstr * BUS_MAX_PARTS), ("umi", BusSubstr * BUS_MAX_PARTS), ("seq", BusSubstr)]

    @classmethod
    def parse(cls, technology: str):
        """kamd_bus_layout_parse: a technology name (10XV3, SURECELL, ...; any case) or a custom "bc:umi:seq" string -> (layout, the strand the
        reference gives the technology by default: 0 unstranded, 1 --fr-stranded, 2 --rf-stranded).  Raises KallistoAmdError with the parser's text."""
        L, strand, err = cls(), C.c_int32(0), C.create_string_buffer(512)
        if load_library().kamd_bus_layout_parse(technology.encode(), C.byref(L), C.byref(strand), err, len(err)) != 0:
            raise KallistoAmdError(f"technology {technology!r}: {err.value.decode(errors='replace')}")
        return L, int(strand.value)

    def parts(self, which: str):
        a, n = (self.bc, self.n_bc) if which == "bc" else (self.umi, self.n_umi)
        return [(a[i].file, a[i].start, a[i].stop) for i in range(n)]

    def seq_max_len(self, max_len: int) -> int:
        """kamd_bus_seq_max_len: no cut sequence of a batch with reads of up to max_len bases is longer."""
        return int(load_library().kamd_bus_seq_max_len(C.byref(self), int(max_len)))

    def header_lens(self, bc_len_hist, umi_len_hist):
        """(bclen, umilen) of the BUS header: the layout's fixed sums, or, where a part is open-ended or the field absent, the modes of the length
        histograms of the run (the first of equal bins; src/main.cpp:2472-2496)."""
        out = []
        for parts, hist in ((self.parts("bc"), bc_len_hist), (self.parts("umi"), umi_len_hist)):
            if parts[0][0] >= 0 and all(b != 0 for _, _, b in parts):
                out.append(sum(b - a for _, a, b in parts))
            else:
                out.append(int(np.argmax(np.asarray(hist))))
        return tuple(out)


class _BusSplitStats(C.Structure):
    """kamd_bus_split_stats"""
    _fields_ = [("n_items", C.c_uint64), ("n_valid", C.c_uint64), ("n_dropped_umi", C.c_uint64), ("n_dropped_bc", C.c_uint64),
                ("bc_len_hist", C.c_uint64 * 33), ("umi_len_hist", C.c_uint64 * 33), ("max_seq_len", C.c_int32), ("last_ms", C.c_float)]


class _BusSortStats(C.Structure):
    """kamd_bus_sort_stats"""
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("passes", C.c_uint32), ("key_bits", C.c_uint32), ("last_ms", C.c_float)]


class _BusCountStats(C.Structure):
    """kamd_bus_count_stats"""
    _fields_ = [("n_records", C.c_uint64), ("n_barcodes", C.c_uint64), ("n_entries", C.c_uint64), ("n_umis", C.c_uint64), ("n_multi_groups", C.c_uint64),
                ("n_multi_records", C.c_uint64), ("last_ms", C.c_float)]


class _BusWhitelistStats(C.Structure):
    """kamd_bus_whitelist_stats"""
    _fields_ = [("n_in", C.c_uint64), ("n_distinct", C.c_uint64), ("n_buckets", C.c_uint64), ("bytes", C.c_uint64), ("max_chain", C.c_uint32), ("bc_len", C.c_int32),
                ("last_ms", C.c_float)]


class _BusCorrectStats(C.Structure):
    """kamd_bus_correct_stats"""
    _fields_ = [("n_in", C.c_uint64), ("n_exact", C.c_uint64), ("n_corrected", C.c_uint64), ("n_ambiguous", C.c_uint64), ("n_uncorrectable", C.c_uint64),
                ("n_out", C.c_uint64), ("last_ms", C.c_float), ("neigh_ms", C.c_float)]


class _BusGenesStats(C.Structure):
    """kamd_bus_genes_stats"""
    _fields_ = [("n_classes", C.c_uint64), ("n_entries_in", C.c_uint64), ("n_pairs", C.c_uint64), ("n_empty", C.c_uint64), ("max_list", C.c_uint32), ("n_genes", C.c_int32),
                ("last_ms", C.c_float)]


class _BusGeneCountStats(C.Structure):
    """kamd_bus_gene_count_stats"""
    _fields_ = [("n_records", C.c_uint64), ("n_barcodes", C.c_uint64), ("n_entries", C.c_uint64), ("n_umis", C.c_uint64), ("n_counted", C.c_uint64),
                ("n_no_gene", C.c_uint64), ("n_multi_gene", C.c_uint64), ("n_wave_groups", C.c_uint64), ("last_ms", C.c_float), ("resolve_ms", C.c_float)]


BUS_COR_EXACT, BUS_COR_CORRECTED, BUS_COR_AMBIGUOUS, BUS_COR_UNCORRECTABLE = 0, 1, 2, 3   # KAMD_BUS_COR_*


class BusWhitelist:
    """a whitelist of a Context (kamd_bus_whitelist): the handle Context.bus_correct takes, the barcode length and what kamd_bus_whitelist_create
    reported (n_in, n_distinct, n_buckets, max_chain, bytes, ms).  Context.close frees it; free() does so earlier."""

    def __init__(self, ctx, handle, stats):
        self._ctx, self._h, self.stats, self.bc_len = ctx, handle, stats, stats["bc_len"]

    def free(self):
        if self._h is not None and self._ctx._h is not None:
            _check(load_library().kamd_bus_whitelist_free(self._ctx._h, self._h), "kamd_bus_whitelist_free")
        self._h = None


class BusGenes:
    """a gene table of a Context (kamd_bus_genes): the handle Context.bus_count_genes takes and what kamd_bus_genes_create reported (n_classes,
    n_entries_in, n_pairs, n_empty, max_list, n_genes, ms).  Context.close frees it; free() does so earlier."""

    def __init__(self, ctx, handle, stats):
        self._ctx, self._h, self.stats, self.n_genes, self.n_classes = ctx, handle, stats, stats["n_genes"], stats["n_classes"]

    def lists(self):
        """kamd_bus_genes_download: the table's CSR -> (off uint64 [n_classes + 1], ids int32 [n_pairs]) on the host"""
        if self._h is None or self._ctx._h is None:
            raise KallistoAmdError("BusGenes.lists: the table was freed")
        off, ids = np.zeros(self.n_classes + 1, np.uint64), np.zeros(max(self.stats["n_pairs"], 1), np.int32)
        _check(load_library().kamd_bus_genes_download(self._ctx._h, self._h, off.ctypes.data, ids.ctypes.data), "kamd_bus_genes_download")
        return off, ids[:self.stats["n_pairs"]]

    def free(self):
        if self._h is not None and self._ctx._h is not None:
            _check(load_library().kamd_bus_genes_free(self._ctx._h, self._h), "kamd_bus_genes_free")
        self._h = None


class BgzfMember(C.Structure):
    """kamd_bgzf_member: one BGZF member of a kamd_bgzf_inflate call (raw deflate stream at src_off of the compressed bytes -> isize bytes at dst_off)."""
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint32), ("isize", C.c_uint32), ("crc32", C.c_uint32), ("reserved", C.c_uint32),
                ("dst_off", C.c_uint64)]


class _InflateResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("first_bad_member", C.c_uint64), ("n_bytes", C.c_uint64), ("n_newlines", C.c_uint64)]


class _TableInfo(C.Structure):
    """kamd_table_info: geometry of the context's device k-mer table, and what its build took when kamd_index_upload built it."""
    _fields_ = [("n_buckets", C.c_uint64), ("pad_buckets", C.c_uint64), ("table_layout", C.c_uint32), ("slots_per_bucket", C.c_uint32),
                ("tag_q", C.c_uint32), ("tag_dsh", C.c_uint32), ("tag_w", C.c_uint32), ("n_dbuckets", C.c_uint64), ("dpad_buckets", C.c_uint64),
                ("dummy_slot", C.c_uint64), ("dummy_uec", C.c_uint32), ("dummy_strand", C.c_uint32), ("built_on_device", C.c_int32),
                ("build_rounds", C.c_int32), ("build_ms", C.c_float), ("build_count_ms", C.c_float), ("build_place_ms", C.c_float),
                ("build_order_ms", C.c_float), ("build_fill_ms", C.c_float), ("build_dlist_ms", C.c_float)]


class _FastqUnit(C.Structure):
    _fields_ = [("d_words", C.c_void_p), ("d_len", C.c_void_p), ("n_items", C.c_uint64), ("max_len", C.c_int32), ("status", C.c_int32),
                ("first_bad_record", C.c_uint64)]


class _Batch(C.Structure):
    _fields_ = [("d_words", C.c_void_p), ("d_len", C.c_void_p), ("n_items", C.c_uint64), ("max_len", C.c_int32)]


class _QuantOut(C.Structure):
    _fields_ = [("n_processed", C.c_uint64), ("em_rounds", C.c_int32), ("flens", C.c_void_p), ("eff_lens", C.c_void_p), ("est_counts", C.c_void_p),
                ("alpha_before_zeroes", C.c_void_p), ("tpm", C.c_void_p)]


class _EcResult(C.Structure):
    _fields_ = [("n_ecs", C.c_uint64), ("nnz", C.c_uint64), ("n_pseudoaligned", C.c_uint64), ("d_ec_off", C.c_void_p),
                ("d_ec_ids", C.c_void_p), ("d_counts", C.c_void_p)]


_LIB = None

_SYMBOLS = {
    # name: (restype, argtypes)
    "kamd_last_error": (C.c_char_p, []),
    "kamd_abi_version": (C.c_uint32, []),
    "kamd_index_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "kamd_index_load_layout": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "kamd_index_load_deferred": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "kamd_index_free": (None, [C.c_void_p]),
    "kamd_index_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kamd_index_get_view": (C.c_int, [C.c_void_p, C.POINTER(_View)]),
    "kamd_index_target_name": (C.c_char_p, [C.c_void_p, C.c_uint64]),
    "kamd_index_check_opts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "kamd_ctx_destroy": (None, [C.c_void_p]),
    "kamd_ctx_tune": (C.c_int, [C.c_void_p, C.POINTER(Tuning)]),
    "kamd_ctx_get_tuning": (C.c_int, [C.c_void_p, C.POINTER(Tuning)]),
    "kamd_index_upload": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_ec_reset": (C.c_int, [C.c_void_p]),
    "kamd_ctx_table_info": (C.c_int, [C.c_void_p, C.POINTER(_TableInfo)]),
    "kamd_ctx_table_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kamd_ec_track_order": (C.c_int, [C.c_void_p, C.c_int]),
    "kamd_packed_record_words": (C.c_uint64, [C.c_int32]),
    "kamd_pack_reads_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    "kamd_pack_reads_host_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_uint64, C.c_uint64]),
    "kamd_pack_reads_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    "kamd_fastq_unit_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(_FastqUnit)]),
    "kamd_fastq_unit_parse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(_FastqUnit)]),
    "kamd_fastq_batch_pack": (C.c_int, [C.c_void_p, C.POINTER(_FastqUnit)]),
    "kamd_pseudoalign": (C.c_int, [C.c_void_p, C.POINTER(QuantOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "kamd_fld_prefetch": (C.c_int, [C.c_void_p, C.POINTER(QuantOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "kamd_fld_from_batch": (C.c_int, [C.c_void_p, C.POINTER(QuantOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p,
                                      C.POINTER(C.c_uint64)]),
    "kamd_align_stats_get": (C.c_int, [C.c_void_p, C.POINTER(_Stats)]),
    "kamd_profile_get": (C.c_int, [C.c_void_p, C.POINTER(_Profile)]),
    "kamd_debug_random_lines": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "kamd_debug_random_lines_span": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double)]),
    "kamd_ec_dense_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "kamd_ec_tuples_export": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kamd_ec_tuples_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "kamd_ec_tuples_replace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "kamd_ec_explicit_export": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kamd_ec_explicit_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "kamd_ec_explicit_replace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "kamd_flat_index_matches": (C.c_int, [C.c_char_p, C.c_char_p]),
    "kamd_comm_unique_id": (C.c_int, [C.c_void_p]),
    "kamd_comm_create_rccl": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "kamd_comm_create_callbacks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "kamd_comm_destroy": (None, [C.c_void_p]),
    "kamd_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kamd_ec_allreduce": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_comm_broadcast_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "kamd_comm_sum_u64_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kamd_em_run_comm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int32)]),
    "kamd_ec_finalize": (C.c_int, [C.c_void_p, C.POINTER(_EcResult)]),
    "kamd_ec_finalize_result": (C.c_int, [C.c_void_p, C.POINTER(_EcResult)]),
    "kamd_ec_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kamd_ec_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kamd_ec_set_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_read_ecs": (C.c_int, [C.c_void_p, C.POINTER(QuantOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(_ReadEcsStats)]),
    "kamd_debug_read_ecs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
    "kamd_bus_layout_parse": (C.c_int, [C.c_char_p, C.POINTER(BusLayout), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    "kamd_bus_seq_max_len": (C.c_int32, [C.POINTER(BusLayout), C.c_int32]),
    "kamd_bus_split": (C.c_int, [C.c_void_p, C.POINTER(BusLayout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.POINTER(_BusSplitStats)]),
    "kamd_bus_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "kamd_bus_sort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(_BusSortStats)]),
    "kamd_bus_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_BusCountStats)]),
    "kamd_bus_whitelist_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    "kamd_bus_whitelist_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(_BusWhitelistStats)]),
    "kamd_bus_whitelist_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_bus_correct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(_BusCorrectStats)]),
    "kamd_bus_genes_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(_BusGenesStats)]),
    "kamd_bus_genes_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kamd_bus_genes_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kamd_bus_count_genes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(_BusGeneCountStats)]),
    "kamd_em_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "kamd_em_run_partitioned": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "kamd_bootstrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                 C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "kamd_bootstrap_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "kamd_bootstrap_seeds": (None, [C.c_uint64, C.c_int32, C.c_void_p]),
    "kamd_cfc_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    "kamd_pseudoalign_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "kamd_aa_stats_get": (C.c_int, [C.c_void_p, C.POINTER(_AaStats)]),
    "kamd_bgzf_inflate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(_InflateResult)]),
    "kamd_debug_bgzf_inflate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(_InflateResult),
                                          C.POINTER(C.c_float)]),
    "kamd_text_cut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "kamd_quant_batches": (C.c_int, [C.c_void_p, C.POINTER(QuantOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(_QuantOut)]),
    "kamd_mean_frag_lens_trunc": (None, [C.c_void_p, C.c_void_p]),
    "kamd_trunc_gaussian_fld": (None, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p]),
    "kamd_eff_lens": (None, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "kamd_counts_to_tpm": (None, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
}


def exported_symbols():
    """Every entry point include/kallisto_amd.h declares (used by the symbol-presence test)."""
    return sorted(_SYMBOLS)


def _load_hip_runtime():
    """libkallisto_amd.so carries no DT_NEEDED for the HIP runtime (see csrc/Makefile): bind it to the runtime this
    process uses -- PyTorch's bundled libamdhip64.so when torch is importable, else the ROCm installation's."""
    cands = []
    try:
        import torch
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:
        pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            return C.CDLL(c, mode=C.RTLD_GLOBAL)
        except OSError:
            continue
    raise KallistoAmdError("no HIP runtime (libamdhip64.so) found")


def load_library():
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise KallistoAmdError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950); kallisto_amd has no CPU path")
        _load_hip_runtime()
        lib = C.CDLL(path)
        lib.kamd_abi_version.restype = C.c_uint32
        if lib.kamd_abi_version() != ABI_VERSION:   # (the structures of include/kallisto_amd.h are mirrored here field by field)
            raise KallistoAmdError(f"{path} was built with KAMD_ABI_VERSION {lib.kamd_abi_version()}, this binding mirrors version {ABI_VERSION}: rebuild the library")
        for name, (res, args) in _SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _check(rc: int, what: str):
    if rc != 0:
        raise KallistoAmdError(f"{what} failed ({rc}): {load_library().kamd_last_error().decode(errors='replace')}")


def bus_tags_numpy(tags) -> np.ndarray:
    """the int64 [n, 3] tensor of Context.bus_split -> a host array of BUS_TAG_DTYPE"""
    return np.ascontiguousarray(tags.cpu().numpy()).reshape(-1).view(BUS_TAG_DTYPE)


def bus_records_numpy(records) -> np.ndarray:
    """the int64 [n, 4] tensor of Context.bus_records -> a host array of BUS_RECORD_DTYPE (the 32-byte records of a BUS file)"""
    return np.ascontiguousarray(records.cpu().numpy()).reshape(-1).view(BUS_RECORD_DTYPE)


def bus_entries_numpy(entries) -> np.ndarray:
    """the int32 [n, 3] tensor of Context.bus_count -> a host array of BUS_ENTRY_DTYPE"""
    return np.ascontiguousarray(entries.cpu().numpy()).reshape(-1).view(BUS_ENTRY_DTYPE)


def bus_whitelist_parse(text: bytes):
    """kamd_bus_whitelist_parse: the bytes of a whitelist file (one barcode per line) -> (codes uint64 [n], barcode length).  Raises KallistoAmdError
    with the parser's text, which names the line."""
    lib = load_library()
    text = bytes(text)
    n, L, err = C.c_uint64(0), C.c_int32(0), C.create_string_buffer(256)
    if lib.kamd_bus_whitelist_parse(text, len(text), None, 0, C.byref(n), C.byref(L), err, len(err)) != 0:
        raise KallistoAmdError(err.value.decode(errors="replace"))
    codes = np.zeros(int(n.value), np.uint64)
    if lib.kamd_bus_whitelist_parse(text, len(text), codes.ctypes.data, len(codes), C.byref(n), C.byref(L), err, len(err)) != 0:
        raise KallistoAmdError(err.value.decode(errors="replace"))
    return codes, int(L.value)


def bus_whitelist_read(path: str):
    """a whitelist file, plain text or gzip (told by its first bytes) -> (codes uint64 [n], barcode length); the text goes through the C parser"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        import gzip
        data = gzip.decompress(data)
    try:
        return bus_whitelist_parse(data)
    except KallistoAmdError as e:
        raise KallistoAmdError(f"{path}: {e}") from None


def genemap_read(path: str, target_names):
    """a transcripts-to-genes file (`-g`) -> (tr_gene int32 [n_targets], -1 = no gene; gene names; common names), by the rules and with the messages
    of the C++ front-end's parser (kamd_genes.h parse_genemap): columns separated by white space, genes numbered by first appearance, the last
    line of a transcript named twice wins, the first of equal target names wins.  Raises KallistoAmdError."""
    tr_of = {}
    for i, name in enumerate(target_names):
        tr_of.setdefault(name, i)
    tr_gene = np.full(len(target_names), -1, np.int32)
    gene_of, names, common = {}, [], []
    try:
        f = open(path, "r")
    except OSError:
        raise KallistoAmdError(f"Error: could not open file {path}") from None
    with f:
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            cols = (line.split() + ["", "", ""])[:3]
            if not cols[1]:
                raise KallistoAmdError(f"Error: No gene associated with transcript {cols[0]} in {path}")
            t = tr_of.get(cols[0])
            if t is None:
                raise KallistoAmdError(f"Error: Invalid transcript: {cols[0]} in {path}")
            g = gene_of.get(cols[1])
            if g is None:
                g = gene_of[cols[1]] = len(names)
                names.append(cols[1])
                common.append(cols[2])
            tr_gene[t] = g
    return tr_gene, names, common


def packed_record_words(max_len: int) -> int:
    return int(load_library().kamd_packed_record_words(max_len))


def _np(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    buf = (C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=int(n))


class Index:
    """Flattened kallisto index (format v13).  Mirrors KmerIndex::load (src/KmerIndex.cpp:1330)."""

    TABLE_LAYOUTS = {"wide": 0, "compact": 1, "auto": 2}

    def __init__(self, path: str, threads: int = 0, table_layout: str | None = None, table_load: float = 0.0, deferred: bool = False):
        """table_layout: None = kamd_index_load (the environment's KAMD_TABLE_LAYOUT, default auto: compact when it fits); "wide" / "compact" / "auto" =
        kamd_index_load_layout with that layout of the k-mer table (and table_load as the compact table's load factor, 0 = the library's choice).
        deferred: kamd_index_load_deferred -- the k-mer table is not built here but by Context.upload on the device (Context.table_info says what
        was built); the view's table pointers are null."""
        lib = load_library()
        self._h = C.c_void_p()
        self.deferred = bool(deferred)
        if deferred:
            _check(lib.kamd_index_load_deferred(os.fsencode(path), threads, -1 if table_layout is None else self.TABLE_LAYOUTS[table_layout], float(table_load),
                                                C.byref(self._h)), "kamd_index_load_deferred")
        elif table_layout is None:
            _check(lib.kamd_index_load(os.fsencode(path), threads, C.byref(self._h)), "kamd_index_load")
        else:
            _check(lib.kamd_index_load_layout(os.fsencode(path), threads, self.TABLE_LAYOUTS[table_layout], float(table_load), C.byref(self._h)),
                   "kamd_index_load_layout")
        self.view = _View()
        _check(lib.kamd_index_get_view(self._h, C.byref(self.view)), "kamd_index_get_view")
        v = self.view
        self.k = v.k
        self.num_kmers, self.num_unitigs, self.num_blocks = v.n_kmers, v.n_unitigs, v.n_blocks
        self.num_ecs, self.num_targets = v.n_ecs, v.n_targets
        self.target_lens = _np(v.target_lens, v.n_targets, np.int32).copy()
        # shades (targets named <base>_shade_<variant>): their number, and per target its base target (0xFFFFFFFF for a target that is no shade)
        self.n_shades = int(v.n_shades)
        self.shade_colour = (_np(v.shade_colour, v.n_targets, np.uint32).copy() if self.n_shades
                             else np.full(int(v.n_targets), 0xFFFFFFFF, np.uint32))

    @property
    def handle(self):
        return self._h

    def target_names(self):
        lib = load_library()
        return [lib.kamd_index_target_name(self._h, i).decode() for i in range(self.num_targets)]

    def ec_sets(self):
        """(ec_off, ec_ids) of the de-duplicated index transcript sets (host views)."""
        v = self.view
        return _np(v.ec_off, v.n_ecs + 1, np.uint64), _np(v.ec_ids, v.ec_nnz, np.uint32)

    def check_opts(self, opts: "QuantOpts"):
        """kamd_index_check_opts: raises for options this index cannot run with (an index with shades and -l / -s without --single-overhang)"""
        _check(load_library().kamd_index_check_opts(self._h, C.byref(opts)), "kamd_index_check_opts")

    def shade_sets(self):
        """(core_off, core_ids, shade_off, shade_ids): every transcript set split into its members that are no shades and those that are
        (host views; four empty arrays when the index has no shade)."""
        v = self.view
        if not self.n_shades:
            return tuple(np.zeros(0, t) for t in (np.uint64, np.uint32, np.uint64, np.uint32))
        return (_np(v.core_off, v.n_ecs + 1, np.uint64), _np(v.core_ids, v.core_nnz, np.uint32),
                _np(v.shade_off, v.n_ecs + 1, np.uint64), _np(v.shade_ids, v.shade_nnz, np.uint32))

    def save(self, path: str):
        """kamd_index_save: the flattened tables as a file that Index(path) / kamd_index_load reads back without rebuilding them."""
        _check(load_library().kamd_index_save(self._h, path.encode()), "kamd_index_save")

    def close(self):
        if getattr(self, "_h", None):
            load_library().kamd_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ECs:
    """EC multiset {sorted transcript set -> count} as CSR (index.ecmapinv x MinCollector::counts)."""
    ec_off: np.ndarray
    ec_ids: np.ndarray
    counts: np.ndarray

    def multiset(self):
        return {tuple(self.ec_ids[self.ec_off[i]:self.ec_off[i + 1]].tolist()): int(self.counts[i])
                for i in range(len(self.counts))}


class Context:
    """One GPU: device copy of the index and the EC state.  All work runs on torch's current stream of `device`."""

    def __init__(self, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise KallistoAmdError("no GPU visible: kallisto_amd has no CPU path")
        self.torch = torch
        self.device = device
        torch.cuda.set_device(device)
        self.stream = torch.cuda.current_stream(device)
        self._h = C.c_void_p()
        _check(load_library().kamd_ctx_create(device, C.c_void_p(self.stream.cuda_stream), C.byref(self._h)), "kamd_ctx_create")
        self.index = None

    def upload(self, index: Index):
        _check(load_library().kamd_index_upload(self._h, index.handle), "kamd_index_upload")
        self.index = index

    def reset(self):
        _check(load_library().kamd_ec_reset(self._h), "kamd_ec_reset")

    def table_info(self) -> dict:
        """kamd_ctx_table_info: geometry of the device k-mer table; built_on_device and the build's milliseconds after the upload of a deferred index."""
        t = _TableInfo()
        _check(load_library().kamd_ctx_table_info(self._h, C.byref(t)), "kamd_ctx_table_info")
        return {n: getattr(t, n) for n, _ in _TableInfo._fields_}

    def table_download(self) -> dict:
        """kamd_ctx_table_download: the device tables as host arrays {table, slot_block, slot_dist, dtable} (dtable empty without a D-list)."""
        t = self.table_info()
        lines = t["n_buckets"] + t["pad_buckets"]
        out = {"table": np.zeros(lines * 8, np.uint64), "slot_block": np.zeros(lines * t["slots_per_bucket"], np.uint32),
               "slot_dist": np.zeros(lines * t["slots_per_bucket"], np.uint32), "dtable": np.zeros((t["n_dbuckets"] + t["dpad_buckets"]) * 8, np.uint64)}
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        _check(load_library().kamd_ctx_table_download(self._h, p(out["table"]), p(out["slot_block"]), p(out["slot_dist"]), p(out["dtable"])), "kamd_ctx_table_download")
        return out

    def tune(self, **kw):
        """kamd_ctx_tune: e.g. tune(text_verify=False), tune(em_form="streamed", em_entries_per_lane=16).  Returns the tuning in force."""
        t = Tuning()
        for k, v in kw.items():
            if k == "em_form" and isinstance(v, str):
                v = EM_FORMS[v]
            if isinstance(v, bool):
                v = 1 if v else 2
            setattr(t, k, int(v))
        _check(load_library().kamd_ctx_tune(self._h, C.byref(t)), "kamd_ctx_tune")
        cur = Tuning()
        _check(load_library().kamd_ctx_get_tuning(self._h, C.byref(cur)), "kamd_ctx_get_tuning")
        return {n: int(getattr(cur, n)) for n, _ in Tuning._fields_}

    def track_order(self, on: bool = True):
        """finalize() then emits the sets in first-occurrence order (the reference's ids at -t 1); call before the first batch."""
        _check(load_library().kamd_ec_track_order(self._h, 1 if on else 0), "kamd_ec_track_order")

    # ---- reads ----
    def pack_reads(self, seqs_u8, max_len: int | None = None):
        """(n_reads, L) uint8 ASCII tensor on the device -> (words, lens) packed records (kamd_pack_reads_device)."""
        torch = self.torch
        assert seqs_u8.dtype == torch.uint8 and seqs_u8.is_cuda and seqs_u8.dim() == 2
        seqs_u8 = seqs_u8.contiguous()
        n, L = seqs_u8.shape
        max_len = max_len or L
        rec = packed_record_words(max_len)
        off = torch.arange(n, device=seqs_u8.device, dtype=torch.int64) * L
        ln = torch.full((n,), L, device=seqs_u8.device, dtype=torch.int32)
        words = torch.empty(n * rec, device=seqs_u8.device, dtype=torch.int32)
        lens = torch.empty(n, device=seqs_u8.device, dtype=torch.int16)
        _check(load_library().kamd_pack_reads_device(self._h, seqs_u8.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                     words.data_ptr(), lens.data_ptr()), "kamd_pack_reads_device")
        return words, lens

    def pack_reads_host(self, seqs, max_len: int | None = None):
        """list of bytes -> packed device tensors through the host packer (kamd_pack_reads_host)."""
        torch = self.torch
        n = len(seqs)
        lens = np.array([len(s) for s in seqs], np.int32)
        max_len = max_len or int(lens.max(initial=1))
        off = np.zeros(n, np.uint64)
        if n:
            off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        buf = b"".join(seqs)
        rec = packed_record_words(max_len)
        words = np.zeros(n * rec, np.uint32)
        l16 = np.zeros(n, np.uint16)
        _check(load_library().kamd_pack_reads_host(buf, off.ctypes.data, lens.ctypes.data, n, max_len, words.ctypes.data,
                                                   l16.ctypes.data), "kamd_pack_reads_host")
        dw = torch.from_numpy(words.view(np.int32)).to(f"cuda:{self.device}")
        dl = torch.from_numpy(l16.view(np.int16)).to(f"cuda:{self.device}")
        return dw, dl, max_len

    def _fastq_texts(self, texts):
        torch = self.torch
        dev = f"cuda:{self.device}"
        keep = []
        for t in texts:
            if isinstance(t, (bytes, bytearray)):
                pad = torch.zeros(len(t) + 64, dtype=torch.uint8)
                pad[:len(t)] = torch.frombuffer(bytearray(t), dtype=torch.uint8)
                keep.append((pad.to(dev), len(t)))
            else:
                assert t.dtype == torch.uint8 and t.is_cuda
                # the ABI wants the text readable up to 32 bytes behind n_bytes (k_fq_pack loads whole groups of 32 bases).  A tensor that is a
                # view of a larger storage with that much behind it -- a unit cut out of a device text buffer -- is passed as it is; only an
                # exactly-sized one is copied into a padded tensor rather than read past its allocation (the copy was unconditional,
                # a device-to-device copy of every text unit)
                n = t.numel()
                flat = t.reshape(-1)
                slack = flat.untyped_storage().nbytes() - (flat.storage_offset() + n) if flat.is_contiguous() else -1
                if slack >= 32 and flat.data_ptr() % 16 == 0:
                    keep.append((flat, n))
                else:
                    pad = torch.zeros(n + 64, dtype=torch.uint8, device=t.device)
                    pad[:n] = flat
                    keep.append((pad, n))
        ptrs = (C.c_void_p * 2)(*[k[0].data_ptr() for k in keep], *([None] * (2 - len(keep))))
        nb = (C.c_uint64 * 2)(*[k[1] for k in keep], *([0] * (2 - len(keep))))
        return keep, ptrs, nb

    def _fastq_result(self, u, n_files):
        torch = self.torch
        words = lens = None
        if u.status == 0 and u.n_items and u.d_words:
            n_reads = int(u.n_items) * n_files
            words = _alias_tensor(torch, u.d_words, n_reads * packed_record_words(int(u.max_len)), torch.int32, self.device)
            lens = _alias_tensor(torch, u.d_len, n_reads, torch.int16, self.device)
        return words, lens, int(u.n_items), int(u.max_len), int(u.status), int(u.first_bad_record)

    def fastq_unit_pack(self, texts, n_records: int):
        """kamd_fastq_unit_pack: one unit of strict 4-line FASTQ text per file (bytes, or uint8 device tensors) -> the packed batch
        (views of the context's buffers, valid until the next call).  Returns (words, lens, n_items, max_len, status, first_bad)."""
        keep, ptrs, nb = self._fastq_texts(texts)
        u = _FastqUnit()
        _check(load_library().kamd_fastq_unit_pack(self._h, ptrs, nb, len(keep), int(n_records), C.byref(u)), "kamd_fastq_unit_pack")
        return self._fastq_result(u, len(keep))

    def fastq_unit_parse(self, texts, n_records: int):
        """kamd_fastq_unit_parse: adds a unit to the batch under construction; the device copies of the texts are kept alive until
        fastq_batch_pack.  Returns (status, first_bad, max_len)."""
        keep, ptrs, nb = self._fastq_texts(texts)
        u = _FastqUnit()
        _check(load_library().kamd_fastq_unit_parse(self._h, ptrs, nb, len(keep), int(n_records), C.byref(u)), "kamd_fastq_unit_parse")
        self._fq_keep = getattr(self, "_fq_keep", []) + [keep]
        self._fq_files = len(keep)
        return int(u.status), int(u.first_bad_record), int(u.max_len)

    def fastq_batch_pack(self):
        u = _FastqUnit()
        _check(load_library().kamd_fastq_batch_pack(self._h, C.byref(u)), "kamd_fastq_batch_pack")
        self.torch.cuda.synchronize(self.device)
        self._fq_keep = []
        return self._fastq_result(u, getattr(self, "_fq_files", 1))

    # ---- pseudoalignment ----
    def pseudoalign(self, opts: QuantOpts, words, lens, n_items: int, max_len: int):
        _check(load_library().kamd_pseudoalign(self._h, C.byref(opts), words.data_ptr(), lens.data_ptr(), n_items, max_len),
               "kamd_pseudoalign")

    def read_ecs(self, opts: QuantOpts, words, lens, n_items: int, max_len: int):
        """kamd_read_ecs: per item of the batch the row of the context's finalized EC result it was counted under (READ_EC_NONE: not
        pseudoaligned, READ_EC_FOREIGN: a set the result does not hold).  Returns (int32 device tensor [n_items], stats dict)."""
        torch = self.torch
        out = torch.empty(max(n_items, 1), dtype=torch.int32, device=f"cuda:{self.device}")
        s = _ReadEcsStats()
        _check(load_library().kamd_read_ecs(self._h, C.byref(opts), words.data_ptr(), lens.data_ptr(), n_items, max_len, out.data_ptr(), C.byref(s)),
               "kamd_read_ecs")
        return out[:n_items], {"n_items": int(s.n_items), "n_mapped": int(s.n_mapped), "n_none": int(s.n_none), "n_foreign": int(s.n_foreign),
                               "ms": float(s.last_ms)}

    def debug_read_ecs(self, chunk_items: int = 0, list_cap: int = 0) -> dict:
        """kamd_debug_read_ecs: sets the items per chunk of read_ecs and the entries of its first tier's lists (0 = the defaults) and returns what the
        table build and the per-item launches of the last read_ecs took and how many of its items went to the second tier."""
        a, b, n = C.c_float(0), C.c_float(0), C.c_uint64(0)
        _check(load_library().kamd_debug_read_ecs(self._h, int(chunk_items), int(list_cap), C.byref(a), C.byref(b), C.byref(n)), "kamd_debug_read_ecs")
        return {"table_ms": float(a.value), "items_ms": float(b.value), "n_second_tier": int(n.value)}

    # ---- barcode / UMI technologies (bus -x <technology>) ----
    def bus_split(self, layout: BusLayout, words, lens, n_items: int, max_len: int, seq_max_len: int | None = None) -> dict:
        """kamd_bus_split: a batch of items (layout.n_files consecutive records each) -> its surviving items, compact and in input order.  Returns
        tags (int64 [n_valid, 3]: kamd_bus_tag, see bus_tags_numpy), src (int32 [n_valid]: the input item), the cut sequences as a single-end batch
        (seq_words, seq_len, n_valid, seq_max_len: what pseudoalign / read_ecs take) and stats (drops, length histograms, ms)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        if seq_max_len is None:
            seq_max_len = layout.seq_max_len(max_len)
        n = max(int(n_items), 1)
        tags = torch.empty((n, 3), dtype=torch.int64, device=dev)
        src = torch.empty(n, dtype=torch.int32, device=dev)
        seq_words = torch.empty(n * packed_record_words(seq_max_len), dtype=torch.int32, device=dev)
        seq_len = torch.empty(n, dtype=torch.int16, device=dev)
        st = _BusSplitStats()
        _check(load_library().kamd_bus_split(self._h, C.byref(layout), words.data_ptr(), lens.data_ptr(), int(n_items), int(max_len), tags.data_ptr(), src.data_ptr(),
                                             seq_words.data_ptr(), seq_len.data_ptr(), int(seq_max_len), C.byref(st)), "kamd_bus_split")
        nv = int(st.n_valid)
        stats = {"n_items": int(st.n_items), "n_valid": nv, "n_dropped_umi": int(st.n_dropped_umi), "n_dropped_bc": int(st.n_dropped_bc),
                 "bc_len_hist": [int(x) for x in st.bc_len_hist], "umi_len_hist": [int(x) for x in st.umi_len_hist], "max_seq_len": int(st.max_seq_len),
                 "ms": float(st.last_ms)}
        return {"tags": tags[:nv], "src": src[:nv], "seq_words": seq_words[:nv * packed_record_words(seq_max_len)], "seq_len": seq_len[:nv], "n_valid": nv,
                "seq_max_len": int(seq_max_len), "stats": stats}

    def bus_records(self, tags, d_ec, n: int):
        """kamd_bus_records: the tags of a cut batch and the rows read_ecs named for it -> the BUS records of the items with a row, in order, as an
        int64 device tensor [n_out, 4] (kamd_bus_record: see bus_records_numpy).  A READ_EC_FOREIGN row raises."""
        torch = self.torch
        out = torch.empty((max(int(n), 1), 4), dtype=torch.int64, device=f"cuda:{self.device}")
        n_out = C.c_uint64(0)
        _check(load_library().kamd_bus_records(self._h, tags.data_ptr(), d_ec.data_ptr(), int(n), out.data_ptr(), C.byref(n_out)), "kamd_bus_records")
        return out[:int(n_out.value)]

    # ---- BUS records -> cells x classes (bustools sort | bustools count) ----
    def bus_sort(self, records, ec_map=None, collapse: bool = True):
        """kamd_bus_sort: the int64 device tensor [n, 4] of BUS records (Context.bus_records) is sorted IN PLACE by (barcode, umi, ec, flags), stably;
        with `collapse` equal records are merged, counts summed.  ec_map (int32 device tensor, optional): every ec is replaced by ec_map[ec] first; an
        ec outside the map raises and leaves `records` as it was.  Returns (records[:n_out], stats dict)."""
        n = int(records.shape[0])
        if n and not records.is_contiguous():
            raise KallistoAmdError("bus_sort: the records must be a contiguous int64 [n, 4] tensor")
        n_out, st = C.c_uint64(0), _BusSortStats()
        _check(load_library().kamd_bus_sort(self._h, records.data_ptr() if n else None, n, ec_map.data_ptr() if ec_map is not None else None,
                                            int(ec_map.numel()) if ec_map is not None else 0, 1 if collapse else 0, C.byref(n_out), C.byref(st)), "kamd_bus_sort")
        return records[:int(n_out.value)], {"n_in": int(st.n_in), "n_out": int(st.n_out), "passes": int(st.passes), "key_bits": int(st.key_bits), "ms": float(st.last_ms)}

    def bus_count(self, sorted_records, mode: int) -> dict:
        """kamd_bus_count: records in key order (Context.bus_sort) -> barcodes (int64 [n_barcodes]: the rows, the barcodes' bits), entries (int32
        [n_entries, 3]: kamd_bus_entry, see bus_entries_numpy; sorted by (row, ec), unique), multi (int64 [n_multi_records, 4]: the records of the
        multi-class groups in input order, pad = row) and stats.  mode: BUS_COUNT_UMIS or BUS_COUNT_READS.  Unsorted input raises."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        n = int(sorted_records.shape[0])
        if n and not sorted_records.is_contiguous():
            raise KallistoAmdError("bus_count: the records must be a contiguous int64 [n, 4] tensor")
        m = max(n, 1)
        barcodes = torch.empty(m, dtype=torch.int64, device=dev)
        entries = torch.empty((m, 3), dtype=torch.int32, device=dev)
        multi = torch.empty((m, 4), dtype=torch.int64, device=dev)
        st = _BusCountStats()
        _check(load_library().kamd_bus_count(self._h, sorted_records.data_ptr() if n else None, n, int(mode), barcodes.data_ptr(), entries.data_ptr(),
                                             multi.data_ptr(), C.byref(st)), "kamd_bus_count")
        stats = {"n_records": int(st.n_records), "n_barcodes": int(st.n_barcodes), "n_entries": int(st.n_entries), "n_umis": int(st.n_umis),
                 "n_multi_groups": int(st.n_multi_groups), "n_multi_records": int(st.n_multi_records), "ms": float(st.last_ms)}
        return {"barcodes": barcodes[:stats["n_barcodes"]], "entries": entries[:stats["n_entries"]], "multi": multi[:stats["n_multi_records"]], "stats": stats}

    # ---- BUS records -> cells x genes (bustools count --genecounts) ----
    def bus_genes(self, tr_gene, n_genes: int, ec_sets_or_csr) -> BusGenes:
        """kamd_bus_genes_create: a gene map (int32 per transcript, -1 = no gene) and the classes the records name -- a sequence of transcript-id
        sequences, or a CSR (ec_off [n_classes + 1], ec_ids) -- -> a BusGenes whose gene lists lie on the device."""
        tr_gene = np.ascontiguousarray(tr_gene, np.int32)
        if isinstance(ec_sets_or_csr, tuple) and len(ec_sets_or_csr) == 2 and isinstance(ec_sets_or_csr[0], np.ndarray):
            ec_off, ec_ids = ec_sets_or_csr
        else:
            sets = list(ec_sets_or_csr)
            ec_off = np.zeros(len(sets) + 1, np.uint64)
            if sets:
                ec_off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64)
            ec_ids = np.fromiter((t for x in sets for t in x), np.int64, int(ec_off[-1]))
            if len(ec_ids) and (int(ec_ids.min()) < 0 or int(ec_ids.max()) > 0xFFFFFFFF):
                raise KallistoAmdError("bus_genes: a transcript id outside 32 bits")
        ec_off, ec_ids = np.ascontiguousarray(ec_off, np.uint64), np.ascontiguousarray(ec_ids, np.uint32)
        if len(ec_off) < 1:
            raise KallistoAmdError("bus_genes: the offsets need n_classes + 1 entries")
        h, st = C.c_void_p(None), _BusGenesStats()
        _check(load_library().kamd_bus_genes_create(self._h, tr_gene.ctypes.data if len(tr_gene) else None, len(tr_gene), int(n_genes), ec_off.ctypes.data,
                                                    ec_ids.ctypes.data if len(ec_ids) else None, len(ec_off) - 1, C.byref(h), C.byref(st)), "kamd_bus_genes_create")
        return BusGenes(self, h, {"n_classes": int(st.n_classes), "n_entries_in": int(st.n_entries_in), "n_pairs": int(st.n_pairs), "n_empty": int(st.n_empty),
                                  "max_list": int(st.max_list), "n_genes": int(st.n_genes), "ms": float(st.last_ms)})

    def bus_count_genes(self, genes: BusGenes, sorted_records, mode: int) -> dict:
        """kamd_bus_count_genes: records in key order (Context.bus_sort) whose classes the table knows -> barcodes (int64 [n_barcodes]: the rows),
        entries (int32 [n_entries, 3]: kamd_bus_entry with the gene id in `ec`, see bus_entries_numpy; sorted by (row, gene), unique) and stats.
        mode: BUS_COUNT_UMIS or BUS_COUNT_READS.  Unsorted input and a class outside the table raise."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        n = int(sorted_records.shape[0])
        if n and not sorted_records.is_contiguous():
            raise KallistoAmdError("bus_count_genes: the records must be a contiguous int64 [n, 4] tensor")
        if genes._h is None or genes._ctx is not self:
            raise KallistoAmdError("bus_count_genes: not a (live) gene table of this context")
        m = max(n, 1)
        barcodes = torch.empty(m, dtype=torch.int64, device=dev)
        entries = torch.empty((m, 3), dtype=torch.int32, device=dev)
        st = _BusGeneCountStats()
        _check(load_library().kamd_bus_count_genes(self._h, genes._h, sorted_records.data_ptr() if n else None, n, int(mode), barcodes.data_ptr(), entries.data_ptr(),
                                                   C.byref(st)), "kamd_bus_count_genes")
        stats = {k: int(getattr(st, k)) for k, _ in _BusGeneCountStats._fields_ if k not in ("last_ms", "resolve_ms")}
        stats["ms"], stats["resolve_ms"] = float(st.last_ms), float(st.resolve_ms)
        return {"barcodes": barcodes[:stats["n_barcodes"]], "entries": entries[:stats["n_entries"]], "stats": stats}

    # ---- barcode whitelists (bustools correct) ----
    def bus_whitelist(self, codes_or_path, bc_len: int | None = None) -> BusWhitelist:
        """kamd_bus_whitelist_create: a whitelist file (a path: bus_whitelist_read) or an array of codes with their barcode length -> a BusWhitelist
        whose membership table lies on the device.  Duplicates are stored once; a code with a bit above 2 * bc_len raises."""
        if isinstance(codes_or_path, (str, os.PathLike)):
            codes, bc_len = bus_whitelist_read(os.fspath(codes_or_path))
        else:
            if bc_len is None:
                raise KallistoAmdError("bus_whitelist: an array of codes needs its barcode length")
            codes = np.ascontiguousarray(codes_or_path, np.uint64)
        h, st = C.c_void_p(None), _BusWhitelistStats()
        _check(load_library().kamd_bus_whitelist_create(self._h, codes.ctypes.data if len(codes) else None, len(codes), int(bc_len), C.byref(h), C.byref(st)),
               "kamd_bus_whitelist_create")
        return BusWhitelist(self, h, {"n_in": int(st.n_in), "n_distinct": int(st.n_distinct), "n_buckets": int(st.n_buckets), "max_chain": int(st.max_chain),
                                      "bytes": int(st.bytes), "bc_len": int(st.bc_len), "ms": float(st.last_ms)})

    def bus_correct(self, wl: BusWhitelist, records, want_status: bool = False):
        """kamd_bus_correct: the int64 device tensor [n, 4] of BUS records (Context.bus_records) against a whitelist -> (the records that are on it or
        one substitution away from exactly one member, the barcode of the latter replaced, compact and in input order: a new tensor [n_out, 4]; stats
        dict: n_in, n_exact, n_corrected, n_ambiguous, n_uncorrectable, n_out, ms, neigh_ms[; the uint8 status of every input record, BUS_COR_*])."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        n = int(records.shape[0])
        if n and not records.is_contiguous():
            raise KallistoAmdError("bus_correct: the records must be a contiguous int64 [n, 4] tensor")
        if wl._h is None or wl._ctx is not self:
            raise KallistoAmdError("bus_correct: not a (live) whitelist of this context")
        out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev) if want_status else None
        n_out, st = C.c_uint64(0), _BusCorrectStats()
        _check(load_library().kamd_bus_correct(self._h, wl._h, records.data_ptr() if n else None, n, out.data_ptr(), status.data_ptr() if want_status else None,
                                               C.byref(n_out), C.byref(st)), "kamd_bus_correct")
        stats = {"n_in": int(st.n_in), "n_exact": int(st.n_exact), "n_corrected": int(st.n_corrected), "n_ambiguous": int(st.n_ambiguous),
                 "n_uncorrectable": int(st.n_uncorrectable), "n_out": int(st.n_out), "ms": float(st.last_ms), "neigh_ms": float(st.neigh_ms)}
        res = (out[:int(n_out.value)], stats)
        return res + (status[:n],) if want_status else res

    # ---- translated search (bus --aa) ----
    def cfc_frames(self, words, lens, n_reads: int, max_len: int):
        """kamd_cfc_frames: the six comma-free frames of every read as packed records (record 6 * r + f, the layout of the input) and
        their translated lengths.  Returns (words int32 [6 * n_reads * packed_record_words(max_len)], lens int16 [6 * n_reads])."""
        torch = self.torch
        rec = packed_record_words(max_len)
        out_w = torch.zeros(max(6 * n_reads * rec, 1), dtype=torch.int32, device=f"cuda:{self.device}")
        out_l = torch.zeros(max(6 * n_reads, 1), dtype=torch.int16, device=f"cuda:{self.device}")
        _check(load_library().kamd_cfc_frames(self._h, words.data_ptr(), lens.data_ptr(), n_reads, max_len, out_w.data_ptr(), out_l.data_ptr()),
               "kamd_cfc_frames")
        return out_w[:6 * n_reads * rec], out_l[:6 * n_reads]

    def pseudoalign_aa(self, words, lens, n_reads: int, max_len: int):
        """kamd_pseudoalign_aa: one batch of single-end reads against an amino-acid index, accumulated into the context's EC state."""
        _check(load_library().kamd_pseudoalign_aa(self._h, words.data_ptr(), lens.data_ptr(), n_reads, max_len), "kamd_pseudoalign_aa")

    def aa_stats(self) -> dict:
        s = _AaStats()
        _check(load_library().kamd_aa_stats_get(self._h, C.byref(s)), "kamd_aa_stats_get")
        return {"n_processed": int(s.n_processed), "n_rejected_offlist": int(s.n_rejected_offlist), "n_all_empty": int(s.n_all_empty),
                "n_frame_clashes": int(s.n_frame_clashes), "n_winner": [int(x) for x in s.n_winner],
                "translate_ms": float(s.last_translate_ms), "match_ms": float(s.last_match_ms),
                "last_chunks": int(s.last_chunks), "last_match_blocks": int(s.last_match_blocks), "last_list_cap": int(s.last_list_cap)}

    # ---- BGZF input inflated on the device ----
    def bgzf_inflate(self, comp, members, text, comp_bytes=None, text_cap=None, debug_check_crc=None) -> dict:
        """kamd_bgzf_inflate: `members` (a sequence of (src_off, src_len, isize, crc32, dst_off)) of the compressed bytes in the uint8 device
        tensor `comp` -> the uint8 device tensor `text`.  Returns status, reason, first_bad_member, n_bytes, n_newlines.
        debug_check_crc True / False: kamd_debug_bgzf_inflate instead (with / without the kernel's CRC pass); the result also has kernel_ms."""
        arr = (BgzfMember * max(len(members), 1))()
        for i, (so, sl, isz, crc, do) in enumerate(members):
            arr[i] = BgzfMember(int(so), int(sl), int(isz), int(crc), 0, int(do))
        res = _InflateResult()
        if debug_check_crc is not None:
            ms = C.c_float(0.0)
            _check(load_library().kamd_debug_bgzf_inflate(self._h, comp.data_ptr(), int(comp.numel() if comp_bytes is None else comp_bytes), arr, len(members),
                                                          text.data_ptr(), int(text.numel() if text_cap is None else text_cap), 1 if debug_check_crc else 0,
                                                          C.byref(res), C.byref(ms)), "kamd_debug_bgzf_inflate")
            return {"status": int(res.status), "reason": int(res.reason), "first_bad_member": int(res.first_bad_member), "n_bytes": int(res.n_bytes),
                    "n_newlines": int(res.n_newlines), "kernel_ms": float(ms.value)}
        _check(load_library().kamd_bgzf_inflate(self._h, comp.data_ptr(), int(comp.numel() if comp_bytes is None else comp_bytes), arr, len(members),
                                                text.data_ptr(), int(text.numel() if text_cap is None else text_cap), C.byref(res)), "kamd_bgzf_inflate")
        return {"status": int(res.status), "reason": int(res.reason), "first_bad_member": int(res.first_bad_member), "n_bytes": int(res.n_bytes),
                "n_newlines": int(res.n_newlines)}

    def text_cut(self, texts, n_bytes, max_records: int):
        """kamd_text_cut: whole records at the head of 1 or 2 uint8 device tensors (16-byte aligned, 32 readable bytes behind n_bytes[f]).
        Returns (n_records, [end per text])."""
        ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in texts], *([None] * (2 - len(texts))))
        nb = (C.c_uint64 * 2)(*[int(n) for n in n_bytes], *([0] * (2 - len(texts))))
        nrec, end = C.c_uint64(0), (C.c_uint64 * 2)(0, 0)
        _check(load_library().kamd_text_cut(self._h, ptrs, nb, len(texts), int(max_records), C.byref(nrec), end), "kamd_text_cut")
        return int(nrec.value), [int(end[i]) for i in range(len(texts))]

    def fld_prefetch(self, opts: QuantOpts, words, lens, n_items: int, max_len: int):
        """Start the FLD kernel for the first prefix of a batch on a side stream (kamd_fld_prefetch); fld_from_batch on the same
        batch then only waits for it."""
        _check(load_library().kamd_fld_prefetch(self._h, C.byref(opts), words.data_ptr(), lens.data_ptr(), n_items, max_len),
               "kamd_fld_prefetch")

    def fld_from_batch(self, opts: QuantOpts, words, lens, n_items: int, max_len: int, flens=None, used: int = 0):
        """Fragment-length sample of the first 10000 qualifying pairs in input order.  `flens` / `used` continue a sample
        started on earlier batches (the reference carries tlencount across batches, src/ProcessReads.cpp:981-1008)."""
        if flens is None:
            flens = np.zeros(MAX_FRAG_LEN, np.uint32)
        used = C.c_uint64(used)
        _check(load_library().kamd_fld_from_batch(self._h, C.byref(opts), words.data_ptr(), lens.data_ptr(), n_items, max_len,
                                                  flens.ctypes.data, C.byref(used)), "kamd_fld_from_batch")
        return flens, int(used.value)

    def stats(self) -> dict:
        s = _Stats()
        _check(load_library().kamd_align_stats_get(self._h, C.byref(s)), "kamd_align_stats_get")
        return {n: int(getattr(s, n)) for n, _ in _Stats._fields_}

    def random_lines(self, n_blocks: int, block_threads: int = 256, iters: int = 256, span_mb: int = 0, access_bytes: int = 64):
        """Diagnostic: (GB/s, M lines/s) of dependent random reads of the k-mer table (span_mb: only its first MiB; access_bytes 64 / 8)."""
        g, m = C.c_double(0), C.c_double(0)
        _check(load_library().kamd_debug_random_lines_span(self._h, n_blocks, block_threads, iters, span_mb, access_bytes, C.byref(g), C.byref(m)),
               "kamd_debug_random_lines_span")
        return g.value, m.value

    def profile(self) -> dict:
        p = _Profile()
        _check(load_library().kamd_profile_get(self._h, C.byref(p)), "kamd_profile_get")
        return {"align_kernel_ms": float(p.last_align_kernel_ms), "em_ms": float(p.last_em_ms), "em_iters": int(p.last_em_iters),
                "classify_ms": float(p.last_classify_ms), "kernel_a_version": int(p.kernel_a_version),
                "em_nnz": int(p.last_em_nnz), "em_nnz_multi": int(p.last_em_nnz_multi), "em_nseg": int(p.last_em_nseg),
                "em_necs": int(p.last_em_necs), "em_k": int(p.last_em_k), "em_grid": int(p.last_em_grid), "em_lds": int(p.last_em_lds),
                "em_plan_cached": int(p.last_em_plan_cached), "finalize_ms": float(p.last_finalize_ms),
                "fin_records": int(p.last_fin_records), "fin_stream_words": int(p.last_fin_stream_words),
                "fin_cand_words": int(p.last_fin_cand_words), "absorb_ms": float(p.absorb_ms), "n_distinct_tuples": int(p.n_distinct_tuples),
                "tuple_store_words": int(p.tuple_store_words), "tuple_table_slots": int(p.tuple_table_slots),
                "em_max_comp_nnz": int(p.last_em_max_comp_nnz), "em_giant_nnz": int(p.last_em_giant_nnz), "em_giant_rows": int(p.last_em_giant_rows),
                "em_giant_tr": int(p.last_em_giant_tr), "em_giant_chunks": int(p.last_em_giant_chunks), "em_graph_fallback": int(p.last_em_graph_fallback), "em_giant_pieces": int(p.last_em_giant_pieces),
                "em_plan_ms": float(p.last_em_plan_ms), "n_overflow_items": int(p.n_overflow_items), "overflow_ms": float(p.overflow_ms),
                "merge_ms": float(p.last_merge_ms), "em_collective_ms": float(p.em_collective_ms), "em_collectives": int(p.em_collectives), "n_overflow_second_pass": int(p.n_overflow_second_pass),
                "last_fld_chunks": int(p.last_fld_chunks), "last_fld_candidates": int(p.last_fld_candidates),
                "last_fld_list_overflows": int(p.last_fld_list_overflows), "last_fld_prefetched": int(p.last_fld_prefetched)}

    # ---- multi-GPU exchange: all-reduce of the dense EC count vector + all-gather of the tuple records ----
    def dense_counts(self):
        """The dense per-index-set count vector as a torch tensor aliasing the context's device memory."""
        torch = self.torch
        p, n = C.c_void_p(), C.c_uint64(0)
        _check(load_library().kamd_ec_dense_counts(self._h, C.byref(p), C.byref(n)), "kamd_ec_dense_counts")
        return _alias_tensor(torch, p.value, int(n.value), torch.int32, self.device)

    def tuples_export(self):
        torch = self.torch
        nw, nt = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().kamd_ec_tuples_export(self._h, C.byref(nw), C.byref(nt)), "kamd_ec_tuples_export")
        words = torch.zeros(max(int(nw.value), 1), dtype=torch.int32, device=f"cuda:{self.device}")
        offs = torch.zeros(max(int(nt.value), 1), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(load_library().kamd_ec_tuples_copy(self._h, words.data_ptr(), offs.data_ptr()), "kamd_ec_tuples_copy")
        return words[:int(nw.value)], offs[:int(nt.value)]

    def tuples_replace(self, words, offs):
        _check(load_library().kamd_ec_tuples_replace(self._h, words.data_ptr() if words.numel() else None, words.numel(),
                                                     offs.data_ptr() if offs.numel() else None, offs.numel()),
               "kamd_ec_tuples_replace")

    def explicit_export(self):
        torch = self.torch
        nw, nr = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().kamd_ec_explicit_export(self._h, C.byref(nw), C.byref(nr)), "kamd_ec_explicit_export")
        words = torch.zeros(max(int(nw.value), 1), dtype=torch.int32, device=f"cuda:{self.device}")
        offs = torch.zeros(max(int(nr.value), 1), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(load_library().kamd_ec_explicit_copy(self._h, words.data_ptr(), offs.data_ptr()), "kamd_ec_explicit_copy")
        return words[:int(nw.value)], offs[:int(nr.value)]

    def explicit_replace(self, words, offs):
        _check(load_library().kamd_ec_explicit_replace(self._h, words.data_ptr() if words.numel() else None, words.numel(),
                                                       offs.data_ptr() if offs.numel() else None, offs.numel()),
               "kamd_ec_explicit_replace")

    def ec_allreduce(self, comm: "Comm"):
        """kamd_ec_allreduce: merge the EC state of all ranks inside the library (one all-reduce of the dense count vector +
        all-gathers of the tuple / explicit-set records, RCCL over xGMI)."""
        _check(load_library().kamd_ec_allreduce(self._h, comm._h), "kamd_ec_allreduce")

    def em_run_comm(self, comm: "Comm", eff_lens: np.ndarray, n_iter: int = 10000, min_rounds: int = 50):
        """kamd_em_run_comm: the EM partitioned over the communicator's ranks by connected component; every rank returns the
        same (alpha, alpha_before_zeroes, rounds)."""
        eff = np.ascontiguousarray(eff_lens, np.float64)
        T = len(eff)
        alpha = np.zeros(T, np.float64)
        abz = np.zeros(T, np.float64)
        rounds = C.c_int32(0)
        _check(load_library().kamd_em_run_comm(self._h, comm._h, eff.ctypes.data, T, n_iter, min_rounds, alpha.ctypes.data,
                                               abz.ctypes.data, C.byref(rounds)), "kamd_em_run_comm")
        return alpha, abz, int(rounds.value)

    # ---- finalize / EM ----
    def finalize(self, download: bool = True):
        res = _EcResult()
        _check(load_library().kamd_ec_finalize(self._h, C.byref(res)), "kamd_ec_finalize")
        self.ec_result = res
        if not download:
            return None
        return self.download_ecs()

    def download_ecs(self):
        """kamd_ec_download of the finalized result (self.ec_result)"""
        res = self.ec_result
        ec_off = np.zeros(res.n_ecs + 1, np.uint64)
        ec_ids = np.zeros(max(res.nnz, 1), np.uint32)
        counts = np.zeros(max(res.n_ecs, 1), np.uint32)
        _check(load_library().kamd_ec_download(self._h, ec_off.ctypes.data, ec_ids.ctypes.data, counts.ctypes.data),
               "kamd_ec_download")
        return ECs(ec_off, ec_ids[:res.nnz], counts[:res.n_ecs])

    def ec_upload(self, ec_off, ec_ids, counts=None):
        """quant-tcc: the ECs of a file become the context's EC result (KmerIndex::loadECsFromFile + the TCC counts of one sample)."""
        off = np.ascontiguousarray(ec_off, np.uint64)
        ids = np.ascontiguousarray(ec_ids, np.uint32)
        cnt = None if counts is None else np.ascontiguousarray(counts, np.uint32)
        _check(load_library().kamd_ec_upload(self._h, off.ctypes.data, ids.ctypes.data if ids.size else None,
                                             None if cnt is None else cnt.ctypes.data, len(off) - 1), "kamd_ec_upload")

    def ec_set_counts(self, counts):
        """Another sample's counts on the same EC matrix (the EM plan is reused)."""
        cnt = np.ascontiguousarray(counts, np.uint32)
        _check(load_library().kamd_ec_set_counts(self._h, cnt.ctypes.data), "kamd_ec_set_counts")

    def em_run(self, eff_lens: np.ndarray, n_iter: int = 10000, min_rounds: int = 50, csr=None):
        """EMAlgorithm(counts, ...).run(n_iter, min_rounds) on the finalized ECs (or on a device CSR triple)."""
        eff = np.ascontiguousarray(eff_lens, np.float64)
        T = len(eff)
        alpha = np.zeros(T, np.float64)
        abz = np.zeros(T, np.float64)
        rounds = C.c_int32(0)
        if csr is None:
            args = (None, None, None, None, 0)
        else:
            off, ids, cnt = csr
            args = (off.data_ptr(), ids.data_ptr(), cnt.data_ptr(), None, cnt.numel())
        _check(load_library().kamd_em_run(self._h, *args, eff.ctypes.data, T, n_iter, min_rounds, alpha.ctypes.data,
                                          abz.ctypes.data, C.byref(rounds)), "kamd_em_run")
        return alpha, abz, int(rounds.value)

    def em_run_partitioned(self, eff_lens: np.ndarray, group=None, n_iter: int = 10000, min_rounds: int = 50):
        """The EM over all ranks of `group`: every rank (holding the same finalized ECs) runs the connected components it
        owns; the only collective inside is the sum of the per-round change counters once per chunk of rounds, plus
        one all-reduce of the result.  Returns the same (alpha, alpha_before_zeroes, rounds) on every rank."""
        import torch.distributed as dist
        torch = self.torch
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        eff = np.ascontiguousarray(eff_lens, np.float64)
        T = len(eff)
        alpha = np.zeros(T, np.float64)
        abz = np.zeros(T, np.float64)
        rounds = C.c_int32(0)
        device = self.device

        def _sum(user, d_counts, n):
            try:
                t = _alias_tensor(torch, d_counts, int(n), torch.int32, device)
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                torch.cuda.synchronize(device)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32)(_sum)
        _check(load_library().kamd_em_run_partitioned(self._h, rank, world, cb, None, eff.ctypes.data, T, n_iter, min_rounds,
                                                      alpha.ctypes.data, abz.ctypes.data, C.byref(rounds)), "kamd_em_run_partitioned")
        both = torch.from_numpy(np.stack([alpha, abz])).to(f"cuda:{device}")
        dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)  # every transcript is non-zero on exactly one rank
        both = both.cpu().numpy()
        return both[0].copy(), both[1].copy(), int(rounds.value)

    def bootstrap(self, seed: int, eff_lens: np.ndarray, csr=None, want_sample: bool = False):
        """One bootstrap replicate (Bootstrap::run_em): multinomial resample of the EC counts + EM.  Returns
        (alpha, rounds[, resampled counts])."""
        eff = np.ascontiguousarray(eff_lens, np.float64)
        T = len(eff)
        alpha = np.zeros(T, np.float64)
        rounds = C.c_int32(0)
        if csr is None:
            args, n = (None, None, None, 0), int(self.ec_result.n_ecs)
        else:
            off, ids, cnt = csr
            args, n = (off.data_ptr(), ids.data_ptr(), cnt.data_ptr(), cnt.numel()), cnt.numel()
        samp = np.zeros(max(n, 1), np.uint32) if want_sample else None
        _check(load_library().kamd_bootstrap(self._h, *args, int(seed), eff.ctypes.data, T, alpha.ctypes.data, C.byref(rounds),
                                             samp.ctypes.data if want_sample else None), "kamd_bootstrap")
        return (alpha, int(rounds.value), samp[:n]) if want_sample else (alpha, int(rounds.value))

    def bootstrap_batch(self, seeds, eff_lens: np.ndarray):
        """kamd_bootstrap_batch: len(seeds) replicates on the finalized ECs -> (alpha [n_rep, T], rounds [n_rep])."""
        eff = np.ascontiguousarray(eff_lens, np.float64)
        sd = np.ascontiguousarray(seeds, np.uint64)
        T, n = len(eff), len(sd)
        alpha = np.zeros((n, T), np.float64)
        rounds = np.zeros(n, np.int32)
        _check(load_library().kamd_bootstrap_batch(self._h, sd.ctypes.data, n, eff.ctypes.data, T, alpha.ctypes.data, rounds.ctypes.data),
               "kamd_bootstrap_batch")
        return alpha, rounds

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)

    def close(self):
        # a communicator cached by quant() holds this context's device and stream: it goes first (kamd_comm_destroy
        # dereferences the context)
        comm = getattr(self, "_comm", None)
        if comm is not None:
            comm.close()
            self._comm = None
        if getattr(self, "_h", None):
            load_library().kamd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CommCallbacks(C.Structure):
    _fields_ = [("allreduce_sum", C.c_void_p), ("allgather", C.c_void_p), ("broadcast", C.c_void_p)]


COMM_ID_BYTES = 128


class Comm:
    """kamd_comm: the context's place among `world` ranks (one process per GPU).

    Comm.rccl(ctx, rank, world, uid): RCCL inside the library (ncclCommInitRank; uid = Comm.unique_id() of rank 0, handed to
    the other ranks by the launcher).  Comm.over_process_group(ctx, group): the collectives of torch.distributed as callbacks
    (gloo in the tests -- two ranks on one GPU; device buffers are staged through the host there).
    Comm.for_context(ctx): RCCL when the default process group runs on nccl (the id is broadcast through it), else callbacks."""

    def __init__(self, ctx: "Context", handle, keep=None, rank: int = 0, world: int = 1, transport: str = "callbacks"):
        self.ctx, self._h, self._keep = ctx, handle, keep
        self.rank, self.world = int(rank), int(world)
        self.transport = transport   # what actually carries the collectives: "rccl (inside libkallisto_amd.so)" or "callbacks over <backend>"

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(load_library().kamd_comm_unique_id(buf), "kamd_comm_unique_id")
        return buf.raw

    @classmethod
    def rccl(cls, ctx: "Context", rank: int, world: int, uid: bytes | None):
        h = C.c_void_p()
        buf = C.create_string_buffer(uid, COMM_ID_BYTES) if uid is not None else None
        _check(load_library().kamd_comm_create_rccl(ctx._h, rank, world, buf, C.byref(h)), "kamd_comm_create_rccl")
        return cls(ctx, h, rank=rank, world=world, transport="rccl (kamd_comm, inside libkallisto_amd.so)")

    @classmethod
    def over_process_group(cls, ctx: "Context", group=None):
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        device = ctx.device
        via_host = dist.get_backend(group) == "gloo"
        tmap = {0: (torch.int32, 4), 1: (torch.int32, 4), 2: (torch.int64, 8), 3: (torch.float64, 8)}   # sums of u32 / u64 as signed: same bits

        def _wrap(fn):
            def g(*a):
                try:
                    fn(*a)
                    torch.cuda.synchronize(device)
                    return 0
                except Exception:   # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            return g

        def _allreduce(user, d_buf, count, typ):
            dt, _ = tmap[int(typ)]
            t = _alias_tensor(torch, d_buf, int(count), dt, device)
            if via_host:
                h = t.cpu(); dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group); t.copy_(h)
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

        def _allgather(user, d_send, d_recv, nbytes):
            n = int(nbytes)
            if n == 0:
                return
            src = _alias_tensor(torch, d_send, n, torch.uint8, device)
            dst = _alias_tensor(torch, d_recv, n * world, torch.uint8, device)
            if via_host:
                parts = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
                dist.all_gather(parts, src.cpu(), group=group)
                dst.copy_(torch.cat(parts))
            else:
                dist.all_gather_into_tensor(dst, src, group=group)

        def _broadcast(user, d_buf, nbytes, root):
            t = _alias_tensor(torch, d_buf, int(nbytes), torch.uint8, device)
            if via_host:
                h = t.cpu(); dist.broadcast(h, src=int(root), group=group); t.copy_(h)
            else:
                dist.broadcast(t, src=int(root), group=group)

        f1 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32)(_wrap(_allreduce))
        f2 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)(_wrap(_allgather))
        f3 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32)(_wrap(_broadcast))
        cbs = _CommCallbacks(C.cast(f1, C.c_void_p), C.cast(f2, C.c_void_p), C.cast(f3, C.c_void_p))
        h = C.c_void_p()
        _check(load_library().kamd_comm_create_callbacks(ctx._h, rank, world, C.byref(cbs), None, C.byref(h)), "kamd_comm_create_callbacks")
        return cls(ctx, h, keep=(f1, f2, f3, cbs), rank=rank, world=world,
                   transport=f"callbacks over torch.distributed ({dist.get_backend(group)}{', staged through the host' if via_host else ''})")

    @classmethod
    def for_context(cls, ctx: "Context", group=None):
        import torch.distributed as dist
        if dist.get_backend(group) != "nccl" or os.environ.get("KAMD_COMM") == "callbacks":
            return cls.over_process_group(ctx, group)
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        # RCCL inside the library; if the library cannot get at RCCL at all (no librccl to dlopen -- the same on every rank of a
        # node) the same collectives run through torch.distributed's nccl backend as callbacks
        try:
            uid = cls.unique_id() if rank == 0 else None
            ok = 1
        except KallistoAmdError as e:
            uid, ok = None, 0
            if rank == 0:
                print(f"[kallisto_amd] RCCL not reachable from the library ({e}); using torch.distributed callbacks", file=sys.stderr)
        box = [uid, ok]
        dist.broadcast_object_list(box, src=0, group=group)
        if not box[1]:
            return cls.over_process_group(ctx, group)
        # every rank runs ncclCommInitRank on its context's device (kamd_comm_create_rccl sets it first); the ranks then agree -- through
        # the process group, not through the communicator under test -- that all of them hold a communicator that counts `world` ranks
        # and sums correctly.  Otherwise all of them drop it and take the callbacks: no rank may be left alone in a collective.
        comm, err = None, ""
        # OPT-IN watchdog over ncclCommInitRank and the first collective (KAMD_COMM_INIT_TIMEOUT_S, set by bench.py's self_launch for the ranks it starts;
        # unset = no watchdog: a library user gets exceptions and the fall-back below, never a hard exit).  A rank that never comes back from those
        # calls cannot be cancelled (the call is inside the library) but it can end its process: the launcher then takes the other ranks down and
        # starts the run again with the collectives carried by torch.distributed (KAMD_COMM=callbacks) instead of waiting out its whole limit on a
        # hang.  The watchdog is disarmed on EVERY way out of the guarded region (try / finally), exceptions included.
        import threading
        done = threading.Event()
        limit = float(os.environ.get("KAMD_COMM_INIT_TIMEOUT_S", "0") or 0)
        if limit > 0:
            def _watch():
                if not done.wait(limit):
                    print(f"[kallisto_amd] rank {rank}: the RCCL communicator did not come up within {limit:.0f} s (KAMD_COMM_INIT_TIMEOUT_S); giving up "
                          f"(exit code 3)", file=sys.stderr, flush=True)
                    os._exit(3)
            threading.Thread(target=_watch, daemon=True).start()
        flags = [None] * world
        try:
            try:
                comm = cls.rccl(ctx, rank, world, box[0])
                seen = comm.info()["ranks_seen"]
                if seen != world:
                    err = f"ncclCommCount says {seen} ranks, the process group has {world}"
            except (KallistoAmdError, OSError, RuntimeError) as e:
                err = str(e) or type(e).__name__
            dist.all_gather_object(flags, err, group=group)
            if not any(flags):
                try:
                    if comm.sum_int(rank + 1) != world * (world + 1) // 2:
                        err = "the all-reduce over the new communicator returned a wrong sum"
                except (KallistoAmdError, OSError, RuntimeError) as e:
                    err = str(e) or type(e).__name__
                dist.all_gather_object(flags, err, group=group)
        finally:
            done.set()
        if any(flags):
            if rank == 0:
                print(f"[kallisto_amd] RCCL communicator inside the library unusable ({next(f for f in flags if f)}); using torch.distributed "
                      f"callbacks", file=sys.stderr)
            if comm is not None:
                comm.close()
            return cls.over_process_group(ctx, group)
        return comm

    def info(self) -> dict:
        """rank / world as created, ranks the transport itself counts (ncclCommCount), backend name"""
        r, w, seen, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(load_library().kamd_comm_info(self._h, C.byref(r), C.byref(w), C.byref(seen), C.byref(b)), "kamd_comm_info")
        return {"rank": r.value, "world": w.value, "ranks_seen": seen.value, "backend": {0: "none", 1: "rccl", 2: "callbacks"}[b.value]}

    def broadcast_np(self, arr: np.ndarray, root: int = 0) -> np.ndarray:
        a = np.ascontiguousarray(arr).copy()
        _check(load_library().kamd_comm_broadcast_host(self.ctx._h, self._h, a.ctypes.data, a.nbytes, root), "kamd_comm_broadcast_host")
        return a

    def sum_int(self, v: int) -> int:
        a = np.array([int(v)], np.uint64)
        _check(load_library().kamd_comm_sum_u64_host(self.ctx._h, self._h, a.ctypes.data, 1), "kamd_comm_sum_u64_host")
        return int(a[0])

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):   # the context is still alive (Context.close() closes its communicator first)
                load_library().kamd_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _alias_tensor(torch, ptr: int, n: int, dtype, device: int):
    """torch tensor over device memory owned by the library (no copy) via __cuda_array_interface__."""
    class _Holder:
        pass
    h = _Holder()
    typestr = {torch.int32: "<i4", torch.int64: "<i8", torch.uint8: "|u1", torch.float64: "<f8", torch.int16: "<i2"}[dtype]
    h.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}
    return torch.as_tensor(h, device=f"cuda:{device}")


# ---- host-side FP64 helpers (bit-exact with the reference) ------------------------------------------------------------

def mean_frag_lens_trunc(flens: np.ndarray) -> np.ndarray:
    fl = np.ascontiguousarray(flens, np.uint32)
    out = np.zeros(MAX_FRAG_LEN, np.float64)
    load_library().kamd_mean_frag_lens_trunc(fl.ctypes.data, out.ctypes.data)
    return out


def trunc_gaussian_fld(mean: float, sd: float) -> np.ndarray:
    out = np.zeros(MAX_FRAG_LEN, np.float64)
    load_library().kamd_trunc_gaussian_fld(0, MAX_FRAG_LEN, mean, sd, out.ctypes.data)
    return out


def eff_lens(target_lens: np.ndarray, mean_fl_trunc: np.ndarray) -> np.ndarray:
    tl = np.ascontiguousarray(target_lens, np.int32)
    t = np.ascontiguousarray(mean_fl_trunc, np.float64)
    out = np.zeros(len(tl), np.float64)
    load_library().kamd_eff_lens(tl.ctypes.data, len(tl), t.ctypes.data, out.ctypes.data)
    return out


def bootstrap_seeds(seed: int, n: int) -> np.ndarray:
    out = np.zeros(n, np.uint64)
    load_library().kamd_bootstrap_seeds(int(seed), n, out.ctypes.data)
    return out


def counts_to_tpm(est_counts: np.ndarray, eff: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(est_counts, np.float64)
    e = np.ascontiguousarray(eff, np.float64)
    out = np.zeros(len(a), np.float64)
    load_library().kamd_counts_to_tpm(a.ctypes.data, e.ctypes.data, len(a), out.ctypes.data)
    return out


@dataclass
class QuantResult:
    n_processed: int
    n_pseudoaligned: int
    n_unique: int
    ecs: ECs | None
    flens: np.ndarray
    eff_lens: np.ndarray
    est_counts: np.ndarray
    alpha_before_zeroes: np.ndarray
    tpm: np.ndarray
    em_rounds: int
    stats: dict = field(default_factory=dict)


def quant(ctx: Context, opts: QuantOpts, batches, download_ecs: bool = True, group=None, comm: Comm | None = None) -> QuantResult:
    """The `kallisto quant` flow (src/main.cpp:2654-2730) over device-resident read batches.

    batches: iterable of (words, lens, n_items, max_len).  Several ranks (torch.distributed initialised, or `comm` given):
    every rank passes its own shard of the reads; the EC counts are merged inside the library (kamd_ec_allreduce: one
    all-reduce + all-gathers over RCCL) before the EM, which runs partitioned over the ranks (kamd_em_run_comm).
    comm=False: this rank on its own, even inside an initialised process group.
    """
    index = ctx.index
    batches = list(batches)
    n_proc = 0
    if comm is False:
        comm = None
    elif comm is None and (group is not None or _dist_on()):
        comm = getattr(ctx, "_comm", None)
        if comm is None:
            comm = ctx._comm = Comm.for_context(ctx, group)
    # the flow itself runs inside the library (kamd_quant_batches); this function only marshals
    T = int(index.num_targets)
    arr = (_Batch * max(len(batches), 1))()
    for i, (words, lens, n_items, max_len) in enumerate(batches):
        arr[i] = _Batch(words.data_ptr(), lens.data_ptr(), int(n_items), int(max_len))
    flens = np.zeros(MAX_FRAG_LEN, np.uint32)
    eff = np.zeros(T, np.float64); alpha = np.zeros(T, np.float64); abz = np.zeros(T, np.float64); tpm = np.zeros(T, np.float64)
    tl = np.ascontiguousarray(index.target_lens, np.int32)
    q = _QuantOut(0, 0, flens.ctypes.data, eff.ctypes.data, alpha.ctypes.data, abz.ctypes.data, tpm.ctypes.data)
    _check(load_library().kamd_quant_batches(ctx._h, C.byref(opts), arr, len(batches), tl.ctypes.data, T, comm._h if comm is not None else None, C.byref(q)),
           "kamd_quant_batches")
    res = _EcResult()
    _check(load_library().kamd_ec_finalize_result(ctx._h, C.byref(res)), "kamd_ec_finalize_result")
    ctx.ec_result = res
    ecs = ctx.download_ecs() if download_ecs else None
    n_aln = n_uniq = 0
    if ecs is not None:
        n_aln = int(ecs.counts.sum(dtype=np.uint64))
        sizes = np.diff(ecs.ec_off.astype(np.int64))
        n_uniq = int(ecs.counts[sizes == 1].sum(dtype=np.uint64))
    return QuantResult(int(q.n_processed), n_aln, n_uniq, ecs, flens, eff, alpha, abz, tpm, int(q.em_rounds), ctx.stats())


def _dist_rank_of(comm: Comm, group=None) -> int:
    return int(comm.rank)   # the communicator knows its place (with or without torch.distributed)


def _dist_on() -> bool:
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:
        return False


def _dist_rank(group=None) -> int:
    import torch.distributed as dist
    return dist.get_rank(group)


def _sum_int(ctx: Context, v: int, group=None) -> int:
    import torch
    import torch.distributed as dist
    t = torch.tensor([int(v)], dtype=torch.int64, device=f"cuda:{ctx.device}")
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return int(t.item())


def _broadcast_np(ctx: Context, arr: np.ndarray, group=None) -> np.ndarray:
    import torch
    import torch.distributed as dist
    t = torch.from_numpy(arr.astype(np.int64)).to(f"cuda:{ctx.device}")
    dist.broadcast(t, src=0, group=group)
    return t.cpu().numpy().astype(arr.dtype)
