"""ctypes mirror of include/svx.h (struct layouts + helpers to wrap numpy arrays)."""
import ctypes as C

import numpy as np

SVX_DEL, SVX_INS, SVX_INV, SVX_DUP_TAN, SVX_BND, SVX_DUP_INT = range(6)
TYPE_NAMES = ("DEL", "INS", "INV", "DUP_TAN", "BND", "DUP_INT")
TYPE_CODE = {n: i for i, n in enumerate(TYPE_NAMES)}
INV_DIRECTIONS = ("left_fwd", "left_rev", "right_fwd", "right_rev", "all")
INV_DIR_CODE = {n: i for i, n in enumerate(INV_DIRECTIONS)}
SRC_NAMES = ("cigar", "suppl")
SVX_FLAG_SKIP = 0x8000
NIBBLE = "=ACMGRSVTWYHKDBN"

ERRORS = {-1: "SVX_E_NODEVICE", -2: "SVX_E_HIP", -3: "SVX_E_ARG", -4: "SVX_E_CAPACITY", -5: "SVX_E_STATE", -6: "SVX_E_FASTA_SYMBOL", -7: "SVX_E_FASTA_HOST",
          -8: "SVX_E_NO_DELETION", -9: "SVX_E_ORDER", -10: "SVX_E_RANGE", -11: "SVX_E_IO"}
SVX_E_STATE, SVX_E_FASTA_SYMBOL, SVX_E_FASTA_HOST, SVX_E_NO_DELETION = -5, -6, -7, -8
SVX_E_CAPACITY, SVX_E_ORDER, SVX_E_RANGE = -4, -9, -10
SVX_E_ARG = -3
SVX_E_IO = -11
# candidate classes in the order of combine_clusters' return tuple (include/svx.h: SVX_CAND_*)
CAND_DEL, CAND_INV, CAND_DUP_INT, CAND_DUP_TAN, CAND_INS, CAND_BND = range(6)
CAND_NAMES = ("DEL", "INV", "DUP_INT", "DUP_TAN", "INS", "BND")
# the FASTA loader (include/svx.h, csrc/fasta.hip): tile of raw bytes per workgroup, page-locked staging piece, bytes fetched behind every '>'
FASTA_TILE, FASTA_PIECE, FASTA_NAME_BYTES = 4096, 8 << 20, 256
FASTA_KINDS = ("plain", "bgzf", "gzip")
FASTA_HOST_REASONS = ("none", "blanks", "budget", "names", "container")

# translation table: ASCII (any case) -> 4-bit code; 255 marks symbols outside the BAM alphabet
_ENC = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(NIBBLE):
    _ENC[ord(_c)] = _i
    _ENC[ord(_c.lower())] = _i
_DEC = np.frombuffer(NIBBLE.encode("ascii"), dtype=np.uint8)
_DEC_TABLE = bytes(NIBBLE.encode("ascii")[i & 15] for i in range(256))        # bytes.translate table: code -> symbol (codes are < 16)


def encode_bases(s):
    """str/bytes -> uint8 codes (upper-cased); ValueError for symbols outside '=ACMGRSVTWYHKDBN'."""
    if isinstance(s, str):
        s = s.encode("ascii")
    codes = _ENC[np.frombuffer(s, dtype=np.uint8)]
    if codes.size and codes.max() == 255:
        bad = sorted(set(chr(b) for b, c in zip(s, codes) if c == 255))
        raise ValueError("sequence symbol(s) %r outside the IUPAC/BAM alphabet %r" % (bad, NIBBLE))
    return codes


def decode_bases(codes):
    # bytes.translate: one C loop over the codes (a numpy look-up of the same table costs 20 ms per 5 M bases - half of what building a table's objects took)
    return np.ascontiguousarray(codes, dtype=np.uint8).tobytes().translate(_DEC_TABLE).decode("ascii")


class Params(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("min_sv_size", C.c_int32), ("max_sv_size", C.c_int32),
                ("segment_gap_tolerance", C.c_int32), ("segment_overlap_tolerance", C.c_int32),
                ("all_bnds", C.c_int32), ("partition_max_distance", C.c_int64),
                ("position_distance_normalizer", C.c_double), ("edit_distance_normalizer", C.c_double),
                ("cluster_max_distance", C.c_double)]

    @classmethod
    def from_options(cls, o):
        g = lambda k, d: getattr(o, k, d)      # noqa: E731
        return cls(int(g("min_mapq", 20)), int(g("min_sv_size", 40)), int(g("max_sv_size", 100000)),
                   int(g("segment_gap_tolerance", 10)), int(g("segment_overlap_tolerance", 5)),
                   1 if g("all_bnds", False) else 0, int(g("partition_max_distance", 1000)),
                   float(g("position_distance_normalizer", 900)), float(g("edit_distance_normalizer", 1.0)),
                   float(g("cluster_max_distance", 0.5)))


_P = C.c_void_p


class Batch(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("n_rec", C.c_int64),
                ("flag", _P), ("tid", _P), ("pos", _P), ("mapq", _P), ("lseq", _P), ("read_id", _P),
                ("order", _P), ("seg_order", _P), ("cigar_off", _P), ("cigar", _P), ("seq_off", _P), ("seq", _P),
                ("seg_off", _P), ("n_seg", C.c_int64), ("seg_tid", _P), ("seg_pos", _P), ("seg_rev", _P),
                ("seg_mapq", _P), ("seg_lseq", _P), ("seg_cigar_off", _P), ("seg_cigar", _P),
                ("n_contig", C.c_int32), ("contig_rank", _P),
                ("seq_rng_off", _P), ("seq_rng_q0", _P), ("seq_rng_len", _P), ("seq_rng_byte", _P), ("n_seq_rng", C.c_int64)]


BATCH_DTYPES = dict(flag=np.uint16, tid=np.int32, pos=np.int32, mapq=np.uint8, lseq=np.int32, read_id=np.int32,
                    order=np.uint32, seg_order=np.uint32, cigar_off=np.uint64, cigar=np.uint32, seq_off=np.uint64,
                    seq=np.uint8, seg_off=np.uint32, seg_tid=np.int32, seg_pos=np.int32, seg_rev=np.uint8,
                    seg_mapq=np.uint8, seg_lseq=np.int32, seg_cigar_off=np.uint64, seg_cigar=np.uint32,
                    contig_rank=np.int32)


class SigView(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("n", C.c_int64), ("key", _P), ("type", _P), ("src", _P), ("aux", _P),
                ("contig", _P), ("start", _P), ("end", _P), ("contig2", _P), ("pos2", _P), ("read_id", _P),
                ("seq_off", _P), ("seq", _P)]


SIG_DTYPES = dict(key=np.uint64, type=np.uint8, src=np.uint8, aux=np.uint8, contig=np.int32, start=np.int32,
                  end=np.int32, contig2=np.int32, pos2=np.int32, read_id=np.int32)


class Genome(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("n_contig", C.c_int32), ("off", _P), ("codes", _P)]


class FastaStats(C.Structure):
    _fields_ = [("kind", C.c_int32), ("host_reason", C.c_int32), ("raw_bytes", C.c_int64), ("seq_bytes", C.c_int64), ("dropped_bytes", C.c_int64),
                ("blank_bytes", C.c_int64), ("bases_kept", C.c_int64), ("records_in_file", C.c_int64), ("records_kept", C.c_int64), ("blocks", C.c_int64),
                ("t_read_stage_s", C.c_double), ("t_inflate_s", C.c_double), ("t_kernels_s", C.c_double), ("t_total_s", C.c_double),
                ("bad_mask", C.c_uint32 * 8)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "bad_mask"}
        d["kind"] = FASTA_KINDS[self.kind] if 0 <= self.kind < len(FASTA_KINDS) else self.kind
        d["host_reason"] = FASTA_HOST_REASONS[self.host_reason] if 0 <= self.host_reason < len(FASTA_HOST_REASONS) else self.host_reason
        d["bad_symbols"] = [chr(b) for b in range(256) if (self.bad_mask[b >> 5] >> (b & 31)) & 1]
        return d


class ClusterView(C.Structure):
    _fields_ = [("n", C.c_int64), ("type_count", C.c_int64 * 6), ("type", _P), ("contig", _P), ("start", _P),
                ("end", _P), ("contig2", _P), ("start2", _P), ("end2", _P), ("aux", _P), ("score", _P),
                ("std_span", _P), ("std_pos", _P), ("size", _P), ("member_off", _P), ("members", _P),
                ("n_members", C.c_int64)]


class CombineParams(C.Structure):
    _fields_ = [("trans_sv_max_distance", C.c_int64), ("del_ins_dup_max_distance", C.c_double), ("position_distance_normalizer", C.c_double),
                ("partition_max_distance", C.c_int64), ("cluster_max_distance", C.c_double)]

    @classmethod
    def from_options(cls, o):
        g = lambda k, d: getattr(o, k, d)      # noqa: E731
        return cls(int(g("trans_sv_max_distance", 500)), float(g("del_ins_dup_max_distance", 1.0)), float(g("position_distance_normalizer", 900)),
                   int(g("partition_max_distance", 1000)), float(g("cluster_max_distance", 0.5)))


class CandidateView(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_members", C.c_int64), ("class_count", C.c_int64 * 6), ("cls", _P), ("contig", _P), ("start", _P), ("end", _P),
                ("contig2", _P), ("start2", _P), ("end2", _P), ("aux", _P), ("copies", _P), ("score", _P), ("std_span", _P), ("std_pos", _P),
                ("member_off", _P), ("members", _P)]


class CombineStats(C.Structure):
    _fields_ = [("t_combine_ms", C.c_double), ("t_cutpaste_ms", C.c_double)] + \
               [(n, C.c_int64) for n in ("n_clusters_in", "n_bnd_mirrored", "n_merged", "n_insertion_from", "n_deletions", "n_cutpaste_pairs", "n_cutpaste",
                                         "n_remove_1", "n_remove_2", "n_dup_partitions", "n_dup_large_partitions", "n_candidates", "n_candidate_members")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# ID labels of VCF lines = bits of VcfParams.types_mask (include/svx.h: SVX_VCF_*), under the names options.types uses
VCF_LABELS = ("DEL", "INV", "INS", "DUP:TANDEM", "DUP:INT", "BND")
VCF_GT = {"./.": 0, "0/0": 1, "0/1": 2, "1/1": 3}


class VcfParams(C.Structure):
    _fields_ = [("types_mask", C.c_uint32), ("sequence_alleles", C.c_int32), ("insertion_sequences", C.c_int32), ("read_names", C.c_int32), ("zmws", C.c_int32),
                ("tandem_duplications_as_insertions", C.c_int32), ("interspersed_duplications_as_insertions", C.c_int32)]

    @classmethod
    def from_options(cls, o, types_to_output=None, sequence_alleles=None):
        g = lambda k: 1 if getattr(o, k, False) else 0      # noqa: E731
        types = VCF_LABELS if types_to_output is None else types_to_output
        mask = sum(1 << k for k, name in enumerate(VCF_LABELS) if name in types)
        seq = (not getattr(o, "symbolic_alleles", False)) if sequence_alleles is None else sequence_alleles
        p = cls(mask, 1 if seq else 0, g("insertion_sequences"), g("read_names"), g("zmws"), g("tandem_duplications_as_insertions"),
                g("interspersed_duplications_as_insertions"))
        p.position_order = bool(g("position_order"))      # (not a field of svx_vcf_params: Engine.vcf passes it through svx_vcf_position_order)
        return p


class VcfInputs(C.Structure):
    _fields_ = [("gt", _P), ("ref_reads", _P), ("alt_reads", _P), ("contig_names_nul_separated", _P), ("n_contig", C.c_int32), ("contig_natural_rank", _P),
                ("read_names_blob", _P), ("read_name_off", _P), ("n_reads", C.c_int64), ("zmw_id", _P)]


class VcfStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_upload_ms", "t_entries_ms", "t_distinct_ms", "t_lengths_ms", "t_skeleton_ms", "t_payload_ms")] + \
               [(n, C.c_int64) for n in ("n_candidates", "n_lines", "n_bytes", "n_tiles")] + [("lines_per_label", C.c_int64 * 6)] + \
               [(n, C.c_int64) for n in ("bytes_ref_forward", "bytes_ref_revcomp", "bytes_ref_repeat", "bytes_seqs", "bytes_reads")]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "lines_per_label"}
        d["lines_per_label"] = dict(zip(VCF_LABELS, list(self.lines_per_label)))
        return d


# products of svx_bed (include/svx.h: SVX_BED_*) and the files of each, in the order the text holds them
BED_SIGNATURE_BEDS, BED_SIGNATURE_VCF, BED_CANDIDATE_BEDS = 0, 1, 2
BED_MAX_FILES = 8


class BedInputs(C.Structure):
    _fields_ = [("contig_names_nul_separated", _P), ("n_contig", C.c_int32), ("contig_str_rank", _P), ("debug_short_line", C.c_int64)]


class BedStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_upload_ms", "t_entries_ms", "t_lengths_ms", "t_skeleton_ms", "t_payload_ms")] + \
               [(n, C.c_int64) for n in ("n_rows", "n_members", "n_lines", "n_bytes", "n_tiles", "n_files", "bytes_members")] + \
               [("lines_per_file", C.c_int64 * BED_MAX_FILES)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "lines_per_file"}
        d["lines_per_file"] = list(self.lines_per_file)[:self.n_files]
        return d


# BGZF output (include/svx.h: svx_text_gz*): text bytes per block, the end-of-file block every file ends with, the sources of Engine.text_gz
TEXT_GZ_BLOCK = 65280
TEXT_GZ_NHIST, TEXT_GZ_CODES_WORDS = 320, 692                 # DEF_NHIST; sizeof(DefBlockCodes) / 4 (csrc/deflate_core.hpp): svx_text_gz_phase
TEXT_GZ_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
TEXT_GZ_VCF, TEXT_GZ_BED, TEXT_GZ_HOST = 0, 1, 2


class TextGzStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_upload_ms", "t_crc_ms", "t_matches_ms", "t_codes_ms", "t_bits_ms", "t_compaction_ms")] + \
               [(n, C.c_int64) for n in ("n_files", "n_blocks", "blocks_eof", "blocks_stored", "blocks_dynamic", "bytes_in", "bytes_out")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# tabix index (include/svx.h: svx_text_index*): presets, and the status of a file that has none
INDEX_VCF, INDEX_BED = 0, 1
# the format of an index (SVX_INDEX_CLASSIC: .bai / .tbi, SVX_INDEX_CSI: .csi, svim_amd/csi.py)
INDEX_CLASSIC, INDEX_CSI = 0, 1
CSI_MIN_REFERENCE = 1 << 29      # "auto": a .csi exactly when a reference of the header is longer than this, the rule samtools users know


def index_format(fmt, classic):
    """`classic` (the name of the five-level index of this kind of file: "bai" for a BAM, "tbi" for a text) or "csi", or a number the library is to
    judge -> the library's constant.  The other kind's name is refused: a BAM has no .tbi, a text no .bai"""
    if isinstance(fmt, str):
        if fmt not in (classic, "csi"):
            raise ValueError("unknown index format %r (%s, csi)" % (fmt, classic))
        return INDEX_CSI if fmt == "csi" else INDEX_CLASSIC
    return int(fmt)


def auto_index_format(lengths, classic):
    """"auto" resolved before the pass: "csi" when a reference length exceeds 2^29, else `classic` ("bai" / "tbi")"""
    return "csi" if any(int(n) > CSI_MIN_REFERENCE for n in lengths) else classic


class TextIndexStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_lines_ms", "t_records_ms", "t_contigs_ms", "t_chunks_ms", "t_linear_ms", "t_serialise_ms")] + \
               [(n, C.c_int64) for n in ("n_files", "n_files_indexed", "n_lines", "n_records", "n_contigs", "n_chunks", "n_bins", "n_slots", "bytes_text", "bytes_out")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# BAM index from the device reader's record stream (include/svx.h: svx_bam_index*)
class BamIndexStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_append_ms", "t_check_ms", "t_chunks_ms", "t_sort_ms", "t_linear_ms", "t_serialise_ms")] + \
               [(n, C.c_int64) for n in ("n_rows", "n_placed", "n_refs", "n_refs_with_rows", "n_chunks", "n_bins", "n_slots", "n_long_cigars", "bytes_out")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


REGION_RULES = {"overlap": 0, "start": 1}      # SVX_REGION_OVERLAP, SVX_REGION_START (svim_amd/regions.py)


class BamRegionStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_seen", "n_kept", "n_marked", "bytes_compressed", "bytes_inflated")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GenotypeParams(C.Structure):
    _fields_ = [("minimum_score", C.c_double), ("min_mapq", C.c_int32), ("minimum_depth", C.c_int32), ("homozygous_threshold", C.c_double),
                ("heterozygous_threshold", C.c_double)]

    @classmethod
    def from_options(cls, o):
        return cls(float(o.minimum_score), int(o.min_mapq), int(o.minimum_depth), float(o.homozygous_threshold), float(o.heterozygous_threshold))


class BamSortStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_append_ms", "t_finish_ms", "t_sort_ms", "t_layout_ms", "t_encode_ms", "t_gather_ms", "t_crc_ms", "t_matches_ms", "t_codes_ms",
                                          "t_bits_ms", "t_compaction_ms", "t_index_ms")] + \
               [(n, C.c_int64) for n in ("n_records", "n_slabs", "arena_bytes", "stream_bytes", "n_blocks", "key_bits", "n_pieces", "gather_bytes", "piece_bytes_max",
                                         "blocks_stored", "blocks_dynamic", "blocks_eof", "bytes_out")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BamSortSpillStats(C.Structure):
    """svx_bam_sort_spill_stats: the spilled sort (svx_bam_sort_begin_spill); valid after any sort_finish"""
    _fields_ = [(n, C.c_int64) for n in ("n_runs", "spilled_bytes", "max_chunk_bytes", "max_run_bytes", "max_stage_bytes", "readback_bytes")] + \
               [(n, C.c_double) for n in ("t_spill_ms", "t_readback_ms", "t_merge_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SORT_ORDERS = {"coordinate": 0, "queryname": 1}      # SVX_SORT_COORDINATE, SVX_SORT_QUERYNAME (svim_amd/bamsort.py)


def sort_order(order):
    if order not in SORT_ORDERS:
        raise ValueError("order is 'coordinate' or 'queryname', not %r" % (order,))
    return SORT_ORDERS[order]


class BamNameSortStats(C.Structure):
    """svx_bam_name_sort_stats: the permutation of a query-name sort (svx_bam_sort_begin_order); zeros after any other sort"""
    _fields_ = [(n, C.c_double) for n in ("t_names_ms", "t_rank_ms", "t_rounds_ms", "t_layout_ms")] + \
               [(n, C.c_int64) for n in ("n_records", "word_bytes", "rounds", "active_total", "active_max")] + [("active_rows", C.c_int64 * 64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "active_rows"}
        d["active_rows"] = list(self.active_rows)[:self.rounds]
        return d


class BamNameSpillStats(C.Structure):
    """svx_bam_name_spill_stats: the runs a merge session closed in query-name order (svx_bam_merge_open_order with a spill directory); zeros without any"""
    _fields_ = [(n, C.c_int64) for n in ("n_runs", "run_rounds", "run_active_rows", "table_bytes")] + [(n, C.c_double) for n in ("t_run_sort_ms", "t_pack_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BamMergeStats(C.Structure):
    """svx_bam_merge_stats: a merge session (svx_bam_merge_*): its files, the merged dictionary, what k_bs_translate did"""
    _fields_ = [(n, C.c_int64) for n in ("n_files", "n_added", "n_ref_merged", "header_bytes", "n_translated_files", "n_translated_chunks", "n_translated_records",
                                         "translate_bytes")] + \
               [(n, C.c_double) for n in ("t_open_ms", "t_add_ms", "t_translate_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SPILL_WRITE_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_uint8), C.c_int64)
SPILL_READ_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_uint8), C.c_int64)


# SAM text through the device reader (include/svx.h: svx_sam_*)
class SamStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_stage_ms", "t_lines_ms", "t_measure_ms", "t_emit_ms", "t_patch_ms", "t_measure_kernel_ms", "t_emit_kernel_ms")] + \
               [(n, C.c_int64) for n in ("n_chunks", "n_lines", "n_records", "text_bytes", "stream_bytes", "n_long_cigars", "n_patched_floats")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GenotypeStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_total_ms", "t_tables_ms", "t_distinct_ms", "t_walk_ms", "t_call_ms")] + \
               [(n, C.c_int64) for n in ("n_candidates", "n_members", "n_alignments")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlignmentsStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_append_ms", "t_span_ms", "t_finalise_ms")] + [(n, C.c_int64) for n in ("n_records", "n_ops_read", "n_long_records")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SVX_ALN_SORT, SVX_ALN_FILE_FLAGS = 1, 2      # svx_collect_keep_alignments_mode


class AlignmentSortStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_key_ms", "t_sort_ms", "t_gather_ms")] + [("n_rows", C.c_int64), ("sorted", C.c_int32), ("key_bits", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


GT_NAMES = ("./.", "0/0", "0/1", "1/1")     # codes of svx_vcf_inputs.gt / svx_genotype_fetch


class AlnIndex(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_contig", C.c_int32), ("reserved", C.c_int32), ("contig_first", _P), ("contig_len", _P),
                ("pos", _P), ("end", _P), ("flag", _P), ("mapq", _P), ("name_id", _P)]


CLU_DTYPES = dict(type=np.uint8, contig=np.int32, start=np.int32, end=np.int32, contig2=np.int32, start2=np.int32,
                  end2=np.int32, aux=np.uint8, score=np.float64, std_span=np.float64, std_pos=np.float64,
                  size=np.int32)


CAND_DTYPES = dict(cls=np.uint8, contig=np.int32, start=np.int32, end=np.int32, contig2=np.int32, start2=np.int32, end2=np.int32, aux=np.uint8,
                   copies=np.int32, score=np.float64, std_span=np.float64, std_pos=np.float64)


class Stats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("t_collect_ms", "t_cluster_ms", "t_cigar_scan_ms", "t_segments_ms",
                                          "t_sort_ms", "t_partition_ms", "t_edit_ms", "t_linkage_ms", "t_gather_ms")] + \
               [(n, C.c_int64) for n in ("n_rec_used", "n_ops", "n_seg", "n_seg_ops", "n_sig", "n_bnd_side",
                                         "n_ins_bases", "n_partitions", "n_large_partitions", "n_pairs",
                                         "n_edit_pairs", "n_edit_cells", "n_clusters", "n_hap_bytes",
                                         "n_edit_wordcols_issued", "n_edit_wordcols_useful", "n_edit_wordcols_retry",
                                         "n_edit_wordcols_band")] + [("edit_guess", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def ptr(a):
    """numpy array (C-contiguous) or torch tensor or int -> c_void_p"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())          # torch tensor


class SigTable(object):
    """Host-side signature table (numpy SoA) - the currency between COLLECT, CLUSTER and the Python objects."""
    __slots__ = tuple(SIG_DTYPES) + ("seq_off", "seq", "n")

    def __init__(self, n, n_seq=0):
        self.n = n
        for k, dt in SIG_DTYPES.items():
            setattr(self, k, np.zeros(n, dtype=dt))
        self.seq_off = np.zeros(n + 1, dtype=np.int64)
        self.seq = np.zeros(max(1, n_seq), dtype=np.uint8)

    def view(self):
        v = SigView()
        v.on_device = 0
        v.n = self.n
        for k in SIG_DTYPES:
            setattr(v, k, ptr(getattr(self, k)))
        v.seq_off = ptr(self.seq_off)
        v.seq = ptr(self.seq)
        return v

    def sequence(self, i):
        return decode_bases(self.seq[self.seq_off[i]:self.seq_off[i + 1]])

    def equal(self, other, with_key=True):
        if self.n != other.n:
            return False
        for k in SIG_DTYPES:
            if k == "key" and not with_key:
                continue
            if not np.array_equal(getattr(self, k), getattr(other, k)):
                return False
        if not np.array_equal(self.seq_off, other.seq_off):
            return False
        m = int(self.seq_off[self.n])
        return np.array_equal(self.seq[:m], other.seq[:m])

    def first_difference(self, other):
        if self.n != other.n:
            return "n: %d != %d" % (self.n, other.n)
        for k in list(SIG_DTYPES) + ["seq_off"]:
            a, b = getattr(self, k), getattr(other, k)
            if not np.array_equal(a, b):
                i = int(np.nonzero(a != b)[0][0])
                return "%s[%d]: %r != %r" % (k, i, a[i], b[i])
        m = int(self.seq_off[self.n])
        if not np.array_equal(self.seq[:m], other.seq[:m]):
            return "seq differs"
        return None


class ClusterTable(object):
    __slots__ = tuple(CLU_DTYPES) + ("member_off", "members", "n", "n_members", "type_count")

    def __init__(self, n, n_members):
        self.n, self.n_members = n, n_members
        for k, dt in CLU_DTYPES.items():
            setattr(self, k, np.zeros(max(1, n), dtype=dt))
        self.member_off = np.zeros(n + 1, dtype=np.int64)
        self.members = np.zeros(max(1, n_members), dtype=np.int32)
        self.type_count = [0] * 6

    def view(self):
        v = ClusterView()
        v.n = self.n
        v.n_members = self.n_members
        for k in CLU_DTYPES:
            setattr(v, k, ptr(getattr(self, k)))
        v.member_off = ptr(self.member_off)
        v.members = ptr(self.members)
        return v

    def finish(self, v):
        self.type_count = list(v.type_count)
        for k in CLU_DTYPES:
            setattr(self, k, getattr(self, k)[:self.n])
        self.members = self.members[:self.n_members]

    def first_difference(self, other, rtol=0.0):
        if self.n != other.n:
            return "n: %d != %d" % (self.n, other.n)
        if list(self.type_count) != list(other.type_count):
            return "type_count %r != %r" % (self.type_count, other.type_count)
        for k in CLU_DTYPES:
            a, b = getattr(self, k), getattr(other, k)
            if a.dtype == np.float64:
                same = (np.isnan(a) & np.isnan(b)) | (a == b) if rtol == 0.0 else \
                    (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))
            else:
                same = a == b
            if not same.all():
                i = int(np.nonzero(~same)[0][0])
                return "%s[%d]: %r != %r" % (k, i, a[i], b[i])
        if not np.array_equal(self.member_off, other.member_off):
            return "member_off differs"
        if not np.array_equal(self.members, other.members):
            return "members differ"
        return None


class CandidateTable(object):
    """Host-side candidate table (numpy SoA; include/svx.h: svx_candidate_view), grouped by class in CAND_* order."""
    __slots__ = tuple(CAND_DTYPES) + ("member_off", "members", "n", "n_members", "class_count", "genotypes")

    def __init__(self, n, n_members):
        self.n, self.n_members = n, n_members
        self.genotypes = None             # SVIM_genotyping.genotype_resident: the columns of Engine.fetch_genotypes() for this table
        for k, dt in CAND_DTYPES.items():
            setattr(self, k, np.zeros(max(1, n), dtype=dt))
        self.member_off = np.zeros(n + 1, dtype=np.int64)
        self.members = np.zeros(max(1, n_members), dtype=np.int32)
        self.class_count = [0] * 6

    def view(self):
        v = CandidateView()
        v.n, v.n_members = self.n, self.n_members
        for k in CAND_DTYPES:
            setattr(v, k, ptr(getattr(self, k)))
        v.member_off = ptr(self.member_off)
        v.members = ptr(self.members)
        return v

    def finish(self, v):
        self.class_count = list(v.class_count)
        for k in CAND_DTYPES:
            setattr(self, k, getattr(self, k)[:self.n])
        self.members = self.members[:self.n_members]
        return self

    def bounds(self):
        b = [0]
        for c in self.class_count:
            b.append(b[-1] + int(c))
        return b

    def first_difference(self, other, rtol=0.0):
        if self.n != other.n:
            return "n: %d != %d" % (self.n, other.n)
        if list(self.class_count) != list(other.class_count):
            return "class_count %r != %r" % (self.class_count, other.class_count)
        for k in CAND_DTYPES:
            a, b = getattr(self, k), getattr(other, k)
            if a.dtype == np.float64:
                same = (np.isnan(a) & np.isnan(b)) | (a == b) if rtol == 0.0 else \
                    (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))
            else:
                same = a == b
            if not same.all():
                i = int(np.nonzero(~same)[0][0])
                return "%s[%d]: %r != %r" % (k, i, a[i], b[i])
        if not np.array_equal(self.member_off, other.member_off):
            return "member_off differs"
        if not np.array_equal(self.members, other.members):
            return "members differ"
        return None
