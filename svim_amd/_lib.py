"""ctypes binding of svim_amd/libsvx.so (the C ABI declared in include/svx.h).

There is no CPU fallback: if the HIP library is missing, or no MI355X is visible, every entry point of the
package raises (SvxError) instead of silently computing somewhere else.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi
from ._abi import ClusterTable, SigTable, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("SVX_LIB") or os.path.join(_HERE, "libsvx.so")      # SVX_LIB: an experiment build (tools/build_variants.sh)
_LIB = None
_ENGINES = {}

SYMBOLS = ["svx_ctx_create", "svx_ctx_destroy", "svx_last_error", "svx_version", "svx_get_stats", "svx_stream", "svx_cluster_partitions_fetch", "svx_memcpy_d2h", "svx_memcpy_h2d", "svx_dev_alloc", "svx_dev_free", "svx_host_alloc", "svx_host_free", "svx_device_synchronize", "svx_selftest_prims", "svx_bam_set_device_decode",
           "svx_collect", "svx_collect_count", "svx_collect_fetch", "svx_collect_geom_fetch", "svx_collect_accumulate", "svx_collect_set_slot_base", "svx_set_genome", "svx_cluster",
           "svx_cluster_count", "svx_cluster_fetch", "svx_cluster_set_ranks", "svx_cluster_abort_ranks", "svx_cluster_stream_positions",
           "svx_set_alignment_index", "svx_genotype",
           "svx_collect_keep_alignments", "svx_alignments_count", "svx_alignments_fetch", "svx_alignments_get_stats",
           "svx_collect_keep_alignments_mode", "svx_alignments_permutation", "svx_alignments_get_sort_stats",
           "svx_genotype_resident", "svx_genotype_count", "svx_genotype_fetch", "svx_genotype_get_stats", "svx_vcf_use_resident_genotypes",
           "svx_cigar_indel", "svx_edit_distance", "svx_linkage_fcluster", "svx_pair_distances",
           "svx_bam_open", "svx_bam_close", "svx_bam_header", "svx_bam_read_batch", "svx_bam_read_names", "svx_bam_set_seq_filter", "svx_bam_rewind", "svx_bam_seek", "svx_bam_seek_region", "svx_bam_region_stats", "svx_bam_set_gpu_inflate", "svx_bam_gpu_inflate_stats",
           "svx_inflater_create", "svx_inflater_destroy", "svx_inflater_staging", "svx_inflater_enqueue", "svx_inflater_wait",
           "svx_inflater_run",
           "svx_genome_load_fasta", "svx_genome_fetch", "svx_fasta_probe", "svx_fasta_plan",
           "svx_combine", "svx_combine_count", "svx_combine_fetch", "svx_combine_stages_fetch", "svx_combine_get_stats", "svx_py_sample100", "svx_sample_used_host",
           "svx_vcf", "svx_vcf_count", "svx_vcf_fetch", "svx_vcf_get_stats", "svx_vcf_format_std",
           "svx_format_repr", "svx_format_repr_many", "svx_format_repr_device",
           "svx_bed", "svx_bed_set_read_names", "svx_bed_count", "svx_bed_fetch", "svx_bed_get_stats",
           "svx_text_gz", "svx_text_gz_count", "svx_text_gz_fetch", "svx_text_gz_get_stats", "svx_text_gz_host", "svx_text_gz_phase", "svx_text_gz_phase_host",
           "svx_vcf_position_order", "svx_text_index", "svx_text_index_count", "svx_text_index_fetch", "svx_text_index_get_stats", "svx_text_index_host",
           "svx_text_index_fmt", "svx_text_index_csi_host", "svx_bam_index_finish_fmt", "svx_bam_sort_index_fmt", "svx_bam_index_csi_host",
           "svx_bam_index_begin", "svx_bam_index_finish", "svx_bam_index_abort", "svx_bam_index_count", "svx_bam_index_fetch", "svx_bam_index_get_stats", "svx_bam_index_host",
           "svx_bam_sort_begin", "svx_bam_sort_finish", "svx_bam_sort_abort", "svx_bam_sort_count", "svx_bam_sort_encode", "svx_bam_sort_fetch", "svx_bam_sort_index",
           "svx_bam_sort_permutation", "svx_bam_sort_get_stats", "svx_bam_sort_host", "svx_bam_sort_header_host", "svx_bam_sort_begin_spill", "svx_bam_sort_get_spill_stats",
           "svx_bam_sort_spill_host",
           "svx_bam_sort_begin_order", "svx_bam_sort_get_name_stats", "svx_bam_sort_host_order", "svx_bam_sort_header_host_order",
           "svx_bam_merge_header_host", "svx_bam_merge_host", "svx_bam_merge_header_host_order", "svx_bam_merge_host_order", "svx_bam_name_tab_check_host",
           "svx_bam_merge_open_order", "svx_bam_merge_get_name_stats", "svx_bam_merge_get_name_spill_stats",
           "svx_bam_merge_open", "svx_bam_merge_add", "svx_bam_merge_finish", "svx_bam_merge_count", "svx_bam_merge_encode", "svx_bam_merge_fetch", "svx_bam_merge_index_fmt",
           "svx_bam_merge_index_count", "svx_bam_merge_index_fetch", "svx_bam_merge_permutation", "svx_bam_merge_get_stats", "svx_bam_merge_get_spill_stats",
           "svx_bam_merge_get_merge_stats", "svx_bam_merge_close",
           "svx_sam_open", "svx_sam_get_stats", "svx_sam_convert_host", "svx_sam_header_host"]


class SvxError(RuntimeError):
    pass


class FastaHostRoute(SvxError):
    """svx_genome_load_fasta left the file to the host parser (SVX_E_FASTA_HOST) or met symbols outside the alphabet in a requested record
    (SVX_E_FASTA_SYMBOL): convert.load_genome then takes the genome_arrays route, which loads the file or raises the ValueError.  `stats`: what the call measured"""

    def __init__(self, msg, code, stats):
        SvxError.__init__(self, msg)
        self.code = code
        self.stats = stats


def _names_blob(references):
    names = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in references]
    if any(b"\0" in n for n in names):
        raise ValueError("contig names must not contain NUL")
    return b"".join(n + b"\0" for n in names)


def fasta_probe(path):
    """host-only (no GPU needed): (container kind 'plain' / 'bgzf' / 'gzip', bytes of text or -1 when only inflating tells, BGZF blocks)"""
    kind, raw, nb = C.c_int32(), C.c_int64(), C.c_int64()
    _check(lib().svx_fasta_probe(os.fsencode(path), C.byref(kind), C.byref(raw), C.byref(nb)), "svx_fasta_probe")
    return _abi.FASTA_KINDS[kind.value], raw.value, nb.value


def fasta_plan(name_blob, hdr_pos, hdr_rank, raw_bytes, references):
    """host-only step of the FASTA loader from the header table to the placement (svx_fasta_plan, include/svx.h) -> (dest int64[n_hdr], off int64[n+1], records kept);
    FastaHostRoute when the names are left to the host parser"""
    hdr_pos = np.ascontiguousarray(hdr_pos, dtype=np.int64)
    hdr_rank = np.ascontiguousarray(hdr_rank, dtype=np.int64)
    n_hdr = int(hdr_pos.size)
    blob = np.frombuffer(bytes(name_blob), dtype=np.uint8) if n_hdr else np.zeros(1, np.uint8)
    if hdr_rank.size != n_hdr + 1 or (n_hdr and blob.size != n_hdr * _abi.FASTA_NAME_BYTES):
        raise ValueError("fasta_plan: hdr_rank needs n_hdr + 1 entries, name_blob n_hdr * %d bytes" % _abi.FASTA_NAME_BYTES)
    dest = np.zeros(max(1, n_hdr), dtype=np.int64)
    off = np.zeros(len(references) + 1, dtype=np.int64)
    kept = C.c_int64()
    rc = lib().svx_fasta_plan(C.c_int64(n_hdr), ptr(blob), ptr(hdr_pos if n_hdr else np.zeros(1, np.int64)), ptr(hdr_rank), C.c_int64(int(raw_bytes)),
                              C.c_int32(len(references)), _names_blob(references), ptr(dest), ptr(off), C.byref(kept))
    if rc == _abi.SVX_E_FASTA_HOST:
        raise FastaHostRoute(lib().svx_last_error().decode("utf-8", "replace"), rc, None)
    _check(rc, "svx_fasta_plan")
    return dest[:n_hdr], off, kept.value


class NoDeletionClusters(SvxError):
    """svx_combine met insertion-from clusters but no deletion cluster (SVX_E_NO_DELETION): the reference raises IndexError there
    (src/svim/SVIM_merging.py:20), and so does svim_amd.SVIM_COMBINE.combine_clusters"""


def py_sample100(sizes):
    """host-only (no GPU needed): random.seed(1524) followed by random.sample(range(n), 100) for every n of `sizes`, as the library's stage 5 of COMBINE
    draws them -> int32 array [len(sizes), 100]"""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    out = np.zeros((max(1, sizes.size), 100), dtype=np.int32)
    _check(lib().svx_py_sample100(C.c_int64(sizes.size), ptr(sizes if sizes.size else np.zeros(1, np.int64)), ptr(out)), "svx_py_sample100")
    return out[:sizes.size]


def sample_used_host(stream, n, lo, width, method="sweep", chunk=0, margin=0):
    """svx_sample_used_host (host-only, no GPU needed): the window [lo, lo + width) of CLUSTER's consumption table for a partition of n members by the host build
    of csrc/sample_core.hpp -> uint16 array; stream: the uint32 words of random.Random(1524).  method "walk": one walk per start (k_sample_tables); "sweep": the
    backward sweep (k_sample_sweep) in chunks of `chunk` starts with a margin of `margin` words (0, 0: the kernel's constants)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint32)
    out = np.zeros(max(1, int(width)), dtype=np.uint16)
    _check(lib().svx_sample_used_host(ptr(stream if stream.size else np.zeros(1, np.uint32)), C.c_int64(stream.size), C.c_int32(int(n)), C.c_int64(int(lo)),
                                      C.c_int32(int(width)), C.c_int32({"walk": 0, "sweep": 1}[method]), C.c_int32(int(chunk)), C.c_int32(int(margin)), ptr(out)),
           "svx_sample_used_host")
    return out[:int(width)]


def vcf_format_std(x):
    """svx_vcf_format_std (host-only): the text get_std_span() / get_std_pos() contribute to a VCF line for x - "." for NaN and 0.0, else str(round(x, 2)) -
    by the integer arithmetic of the kernels.  SvxError (SVX_E_ARG) for |x| >= 1e10."""
    out = C.create_string_buffer(32)
    _check(lib().svx_vcf_format_std(C.c_double(float(x)), out), "svx_vcf_format_std")
    return out.value.decode("ascii")


def format_repr(x):
    """svx_format_repr (host-only): repr(float(x)) by the integer arithmetic of csrc/fmt_repr.hpp"""
    out = C.create_string_buffer(32)
    _check(lib().svx_format_repr(C.c_double(float(x)), out), "svx_format_repr")
    return out.value.decode("ascii")


def format_repr_many(values):
    """svx_format_repr_many (host-only): float64 array -> list of str, one call for the whole array"""
    x = np.ascontiguousarray(values, dtype=np.float64)
    out = np.zeros((max(1, x.size), 32), dtype=np.uint8)
    _check(lib().svx_format_repr_many(C.c_int64(x.size), ptr(x if x.size else np.zeros(1)), ptr(out)), "svx_format_repr_many")
    return [b.decode("ascii") for b in out[:x.size].view("S32").ravel().tolist()]


def text_gz_host(data):
    """svx_text_gz_host (host-only, no GPU needed): the BGZF stream of one file of bytes by the host build of csrc/deflate_core.hpp - the bytes
    Engine.text_gz makes of the same text on the device"""
    data = bytes(data)
    cap = len(data) + 64 * (len(data) // _abi.TEXT_GZ_BLOCK + 2)
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_int64()
    src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    _check(lib().svx_text_gz_host(ptr(src), C.c_int64(len(data)), ptr(out), C.c_int64(cap), C.byref(n)), "svx_text_gz_host")
    return out[:n.value].tobytes()


def text_gz_phase(phase, n, text=b"", text_off=None, crc=None, tok=None, nt=None, hist=None, codes=None, engine=None):
    """svx_text_gz_phase (engine: an Engine) / svx_text_gz_phase_host (engine None; no GPU needed): one phase of the encoder of csrc/deflate_core.hpp over a
    batch of blocks - test infrastructure.  phase "match": text, text_off, n -> (tok uint32[nb, 65280], nt uint32[nb], hist uint32[nb, 320]); "codes": hist, n,
    crc -> codes uint32[nb, 692] (the words of DefBlockCodes); "bits": text, text_off, n, tok, nt, codes -> slots uint8[nb, 65536].  Layouts: include/svx.h."""
    ph = {"match": 0, "codes": 1, "bits": 2}[phase]
    n = np.ascontiguousarray(n, dtype=np.uint32)
    nb = int(n.size)
    text = bytes(text)
    src = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    off = np.ascontiguousarray(text_off if text_off is not None else np.zeros(nb + 1), dtype=np.int64)
    if off.size != nb + 1 or (ph != 1 and int(off[-1]) != len(text)):
        raise ValueError("text_gz_phase: text_off must hold one offset per block and len(text)")
    want = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint32).reshape(shape) if a is not None else np.zeros(shape, dtype=np.uint32)       # noqa: E731
    crc, nt = want(crc, (nb,)), want(nt, (nb,)).copy()
    hist, codes = want(hist, (nb, _abi.TEXT_GZ_NHIST)).copy(), want(codes, (nb, _abi.TEXT_GZ_CODES_WORDS)).copy()
    tok = want(tok, (nb, _abi.TEXT_GZ_BLOCK)) if ph == 2 else np.zeros((nb, _abi.TEXT_GZ_BLOCK) if ph == 0 else (1, 1), dtype=np.uint32)
    slots = np.zeros((nb, 65536) if ph == 2 else (1, 1), dtype=np.uint8)
    args = (C.c_int(ph), C.c_int64(nb), ptr(src), ptr(off), ptr(n), ptr(crc), ptr(tok), ptr(nt), ptr(hist), ptr(codes), ptr(slots))
    if engine is None:
        _check(lib().svx_text_gz_phase_host(*args), "svx_text_gz_phase_host")
    else:
        _check(engine.L.svx_text_gz_phase(engine.ctx, *args), "svx_text_gz_phase")
    return {0: (tok, nt, hist), 1: codes, 2: slots}[ph]


def text_index_host(text, block_coff, block_uoff, preset, stream_base=0, fmt="tbi"):
    """svx_text_index_host (host-only, no GPU needed): the uncompressed .tbi bytes of one file by the host build of csrc/textindex_core.hpp - the bytes
    Engine.text_index makes of the same text and block table on the device, and svim_amd.tabix.build_index by the definition.  block_coff / block_uoff:
    n_blocks + 1 entries each, the last block the end-of-file block.  svim_amd.tabix.TabixError (code E_ORDER / E_RANGE) for a text that has no index.
    fmt="csi": svx_text_index_csi_host, the uncompressed .csi bytes (svim_amd.csi.build_text_index by the definition)."""
    fn = lib().svx_text_index_csi_host if _abi.index_format(fmt, "tbi") == _abi.INDEX_CSI else lib().svx_text_index_host
    from . import tabix
    text = bytes(text)
    co, uo = np.ascontiguousarray(block_coff, dtype=np.int64), np.ascontiguousarray(block_uoff, dtype=np.int64)
    if co.size != uo.size or co.size < 2:
        raise ValueError("text_index_host: the block table needs n_blocks + 1 entries")
    src = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    n, cap = C.c_int64(), 0
    for _ in range(2):
        out = np.zeros(max(1, cap), dtype=np.uint8)
        rc = fn(ptr(src), C.c_int64(len(text)), ptr(co), ptr(uo), C.c_int64(co.size - 1), C.c_int(preset), C.c_int64(stream_base), ptr(out),
                                       C.c_int64(cap), C.byref(n))
        if rc in (_abi.SVX_E_ORDER, _abi.SVX_E_RANGE):
            raise tabix.TabixError(rc, "text_index_host: " + _abi.ERRORS[rc])
        if rc != _abi.SVX_E_CAPACITY:
            break
        cap = n.value
    if rc != 0:
        raise SvxError("svx_text_index_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:n.value].tobytes()


def bam_index_host(n_ref, rows, v_end, fmt="bai"):
    """svx_bam_index_host (host-only, no GPU needed): the .bai bytes of a row table by the host build of csrc/bamindex_core.hpp - the bytes NativeBam.index_finish
    makes of the same file on the device, and svim_amd.bai.build_index by the definition.  rows: (tid, pos, end, flag, vbeg) per record, as bai.rows_of_bam lists
    them, or the five columns as arrays.  svim_amd.bai.BaiError (code E_ORDER / E_RANGE) for a file that has no index.
    fmt="csi": svx_bam_index_csi_host, the uncompressed .csi bytes (svim_amd.csi.build_bam_index by the definition)."""
    fn = lib().svx_bam_index_csi_host if _abi.index_format(fmt, "bai") == _abi.INDEX_CSI else lib().svx_bam_index_host
    from . import bai
    if isinstance(rows, (tuple, list)) and len(rows) == 5 and all(isinstance(c, np.ndarray) for c in rows):
        cols = rows
    else:
        rows = list(rows)
        cols = [[r[k] for r in rows] for k in range(5)]
    dts = (np.int32, np.int32, np.int64, np.uint16, np.uint64)
    n_rows = len(cols[0])
    cols = [np.ascontiguousarray(c, dtype=dt) if n_rows else np.zeros(1, dtype=dt) for c, dt in zip(cols, dts)]
    n, cap = C.c_int64(), 0
    for _ in range(2):
        out = np.zeros(max(1, cap), dtype=np.uint8)
        rc = fn(C.c_int32(int(n_ref)), C.c_int64(n_rows), *[ptr(c) for c in cols], C.c_uint64(int(v_end)), ptr(out), C.c_int64(cap), C.byref(n))
        if rc in (_abi.SVX_E_ORDER, _abi.SVX_E_RANGE):
            raise bai.BaiError(rc, "bam_index_host: " + _abi.ERRORS[rc])
        if rc != _abi.SVX_E_CAPACITY:
            break
        cap = n.value
    if rc != 0:
        raise SvxError("svx_bam_index_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:n.value].tobytes()


def bam_sort_host(records, n_ref, order="coordinate"):
    """svx_bam_sort_host_order (host-only, no GPU needed): records in file order (bytes: block_size + body each) -> (the sorted record stream, the permutation
    as a uint32 array) by the host build of csrc/bamsort_core.hpp - what NativeBam.sort_finish leaves on the device, and svim_amd.bamsort.sort_records by the
    definition.  order: "coordinate" or "queryname".  svim_amd.bamsort.BamSortError (code E_ARG / E_RANGE) for a stream the definition refuses."""
    from . import bamsort
    which = _abi.sort_order(order)
    records = bytes(records)
    src = np.frombuffer(records, dtype=np.uint8) if records else np.zeros(1, np.uint8)
    out = np.zeros(max(1, len(records)), dtype=np.uint8)
    cap = len(records) // 36 + 1
    perm, n = np.zeros(cap, dtype=np.uint32), C.c_int64()
    rc = lib().svx_bam_sort_host_order(ptr(src), C.c_int64(len(records)), C.c_int32(int(n_ref)), C.c_int(which), ptr(out), ptr(perm), C.c_int64(cap), C.byref(n))
    if rc in (_abi.SVX_E_ARG, _abi.SVX_E_RANGE):
        raise bamsort.BamSortError(rc, "bam_sort_host: " + _abi.ERRORS[rc])
    if rc != 0:
        raise SvxError("svx_bam_sort_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:len(records)].tobytes(), perm[:n.value].copy()


def bam_sort_spill_host(records, n_ref, run_ends, piece_blocks=4096, write=None, read=None):
    """svx_bam_sort_spill_host (host-only): the spilled sort by the rules of the kernels - runs that end in front of the records run_ends (the last one the
    number of records), a run file, one contiguous byte range per run and piece of piece_blocks blocks (svim_amd.bamsort.runs_of / merge_runs / piece_cuts say
    it in Python) -> (the sorted record stream, the permutation): what bam_sort_host gives.  write(offset, data) / read(offset, n_bytes) -> bytes: the run file
    is the caller's (both or neither; what they return may be short: SvxError with .code SVX_E_IO)."""
    from . import bamsort
    records = bytes(records)
    src = np.frombuffer(records, dtype=np.uint8) if records else np.zeros(1, np.uint8)
    out = np.zeros(max(1, len(records)), dtype=np.uint8)
    cap = len(records) // 36 + 1
    perm, n = np.zeros(cap, dtype=np.uint32), C.c_int64()
    ends = np.asarray(list(run_ends), dtype=np.int64)
    ends_p = ptr(ends) if len(ends) else None

    def _write(user, offset, data, n_bytes):
        return int(write(int(offset), C.string_at(data, n_bytes)))

    def _read(user, offset, dst, n_bytes):
        got = bytes(read(int(offset), int(n_bytes)))[:n_bytes]
        C.memmove(dst, got, len(got))
        return len(got)
    wf = _abi.SPILL_WRITE_FN(_write) if write else C.cast(None, _abi.SPILL_WRITE_FN)
    rf = _abi.SPILL_READ_FN(_read) if read else C.cast(None, _abi.SPILL_READ_FN)
    rc = lib().svx_bam_sort_spill_host(ptr(src), C.c_int64(len(records)), C.c_int32(int(n_ref)), ends_p, C.c_int64(len(ends)), C.c_int64(int(piece_blocks)), ptr(out), ptr(perm),
                                       C.c_int64(cap), C.byref(n), wf, rf, None)
    if rc in (_abi.SVX_E_ARG, _abi.SVX_E_RANGE):
        raise bamsort.BamSortError(rc, "bam_sort_spill_host: " + _abi.ERRORS[rc])
    if rc != 0:
        e = SvxError("svx_bam_sort_spill_host failed: %s" % _abi.ERRORS.get(rc, rc))
        e.code = rc
        raise e
    return out[:len(records)].tobytes(), perm[:n.value].copy()


def bam_sort_header_host(header, order="coordinate"):
    """svx_bam_sort_header_host_order (host-only): the header of the sorted file in that order, as svim_amd.bamsort.sorted_header defines it"""
    which = _abi.sort_order(order)
    header = bytes(header)
    src = np.frombuffer(header, dtype=np.uint8) if header else np.zeros(1, np.uint8)
    cap = len(header) + 64
    out, n = np.zeros(cap, dtype=np.uint8), C.c_int64()
    rc = lib().svx_bam_sort_header_host_order(ptr(src), C.c_int64(len(header)), C.c_int(which), ptr(out), C.c_int64(cap), C.byref(n))
    if rc != 0:
        raise SvxError("svx_bam_sort_header_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:n.value].tobytes()


def bam_merge_header_host(headers, order="coordinate"):
    """svx_bam_merge_header_host_order (host-only; order: "coordinate" or "queryname"): the header of the merged file of the files whose headers (magic .. dictionary) are given, in that order, and the
    maps of their reference ids into the merged dictionary -> (header bytes, [map per file]), as svim_amd.bammerge.merged_header and tid_maps define them.
    svim_amd.bammerge.BamMergeError (code E_ARG) for what the definition refuses."""
    from . import bammerge
    which = _abi.sort_order(order)
    headers = [bytes(h) for h in headers]
    k = len(headers)
    if k < 1:
        raise bammerge.BamMergeError(_abi.SVX_E_ARG, "bam_merge_header_host: no input")
    bufs = [np.frombuffer(h, dtype=np.uint8) if h else np.zeros(1, np.uint8) for h in headers]
    ptrs = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
    sizes = np.array([len(h) for h in headers], dtype=np.int64)
    n_refs = []
    for h in headers:       # (the count sits behind the text; a header too short to hold one is the library's to refuse)
        l_text = int.from_bytes(h[4:8], "little", signed=True) if len(h) >= 12 else -1
        n_refs.append(min(len(h) // 8, int.from_bytes(h[8 + l_text:12 + l_text], "little", signed=True)) if 0 <= l_text <= len(h) - 12 else 0)
    maps = np.zeros(max(1, sum(max(0, n) for n in n_refs)), dtype=np.int32)
    n, cap = C.c_int64(), 0
    for _ in range(2):
        out = np.zeros(max(1, cap), dtype=np.uint8)
        rc = lib().svx_bam_merge_header_host_order(ptrs, ptr(sizes), C.c_int64(k), C.c_int(which), ptr(out), C.c_int64(cap), C.byref(n), ptr(maps))
        if rc != _abi.SVX_E_CAPACITY:
            break
        cap = n.value
    if rc == _abi.SVX_E_ARG:
        raise bammerge.BamMergeError(rc, "bam_merge_header_host: " + _abi.ERRORS[rc])
    if rc != 0:
        raise SvxError("svx_bam_merge_header_host failed: %s" % _abi.ERRORS.get(rc, rc))
    out_maps, at = [], 0
    for nr in n_refs:
        out_maps.append([int(x) for x in maps[at:at + nr]])
        at += nr
    return out[:n.value].tobytes(), out_maps


def bam_merge_host(files, n_ref_merged, order="coordinate"):
    """svx_bam_merge_host_order (host-only; order: "coordinate" or "queryname"): files: per input (record stream in file order, n_ref, tid_map) -> (the merged record stream, the permutation over global
    record numbers as a uint32 array), what svim_amd.bammerge.merge gives.  svim_amd.bammerge.BamMergeError (code E_ARG / E_RANGE) for what it refuses."""
    from . import bammerge
    which = _abi.sort_order(order)
    files = [(bytes(s), int(nr), [int(t) for t in m]) for s, nr, m in files]
    k = len(files)
    if k < 1 or any(len(m) != nr for _, nr, m in files):
        raise bammerge.BamMergeError(_abi.SVX_E_ARG, "bam_merge_host: no input, or a map that has not one entry per reference of its file")
    bufs = [np.frombuffer(s, dtype=np.uint8) if s else np.zeros(1, np.uint8) for s, _, _ in files]
    ptrs = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
    sizes = np.array([len(s) for s, _, _ in files], dtype=np.int64)
    n_refs = np.array([nr for _, nr, _ in files], dtype=np.int32)
    maps = np.array([t for _, _, m in files for t in m] or [0], dtype=np.int32)
    total = int(sizes.sum())
    out = np.zeros(max(1, total), dtype=np.uint8)
    cap = total // 36 + 1
    perm, n = np.zeros(cap, dtype=np.uint32), C.c_int64()
    rc = lib().svx_bam_merge_host_order(ptrs, ptr(sizes), ptr(n_refs), C.c_int64(k), C.c_int32(int(n_ref_merged)), ptr(maps), C.c_int(which), ptr(out), ptr(perm), C.c_int64(cap),
                                        C.byref(n))
    if rc in (_abi.SVX_E_ARG, _abi.SVX_E_RANGE):
        raise bammerge.BamMergeError(rc, "bam_merge_host: " + _abi.ERRORS[rc])
    if rc != 0:
        raise SvxError("svx_bam_merge_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:total].tobytes(), perm[:n.value].copy()


def bam_name_tab_check_host(name, word_off, tab_words):
    """svx_bam_name_tab_check_host (host-only): `name` (1..255 bytes) packed at word word_off of a name table of tab_words words (csrc/bamsort_core.hpp:
    bsort_name_tab_pack) -> the rounds 0..63 at which bsort_name_tab_word differs from bsort_name_word, plus the words written outside the name's own"""
    name = bytes(name)
    buf = np.frombuffer(name, dtype=np.uint8) if name else np.zeros(1, np.uint8)
    rc = lib().svx_bam_name_tab_check_host(ptr(buf), C.c_int32(len(name)), C.c_int64(int(word_off)), C.c_int64(int(tab_words)))
    if rc < 0:
        raise SvxError("svx_bam_name_tab_check_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return rc


def sam_convert_host(text, references, cap=None):
    """svx_sam_convert_host (host-only, no GPU needed): SAM text (bytes; header lines in front are skipped) -> (the BAM records of its alignment lines back to
    back, their number) by the host build of csrc/sam_core.hpp - what the device reader makes of the same text, and svim_amd.sam.record_bytes by the definition.
    references: the names of the @SQ dictionary in order.  svim_amd.sam.SamError (code E_ARG / E_RANGE, .line) for a line the definition refuses.  cap: the
    room to offer (tests); too little raises SvxError with .code SVX_E_CAPACITY and .needed"""
    from . import sam
    text = bytes(text)
    src = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    blob = b"".join(r.encode("latin-1") + b"\0" for r in references) + b"\0"
    n, nrec, bad = C.c_int64(), C.c_int64(), C.c_int64()
    want = len(text) * 2 + 64 if cap is None else int(cap)
    while True:
        out = np.zeros(max(1, want), dtype=np.uint8)
        rc = lib().svx_sam_convert_host(ptr(src), C.c_int64(len(text)), C.c_int32(len(references)), C.c_char_p(blob), ptr(out), C.c_int64(want), C.byref(n), C.byref(nrec),
                                        C.byref(bad))
        if rc == _abi.SVX_E_CAPACITY and cap is None:
            want = n.value
            continue
        break
    if rc in (_abi.SVX_E_ARG, _abi.SVX_E_RANGE) and bad.value:
        raise sam.SamError(rc, lib().svx_last_error().decode("utf-8", "replace"), bad.value)
    if rc != 0:
        e = SvxError("svx_sam_convert_host failed: %s" % _abi.ERRORS.get(rc, rc))
        e.code, e.needed = rc, n.value
        raise e
    return out[:n.value].tobytes(), nrec.value


def sam_header_host(header_text):
    """svx_sam_header_host (host-only): the BAM header of a SAM header text, as svim_amd.sam.header_bytes defines it"""
    header_text = bytes(header_text)
    cap = len(header_text) * 2 + 64
    out, n = np.zeros(cap, dtype=np.uint8), C.c_int64()
    rc = lib().svx_sam_header_host(C.c_char_p(header_text), C.c_int64(len(header_text)), ptr(out), C.c_int64(cap), C.byref(n))
    if rc == _abi.SVX_E_CAPACITY:
        cap = n.value
        out = np.zeros(cap, dtype=np.uint8)
        rc = lib().svx_sam_header_host(C.c_char_p(header_text), C.c_int64(len(header_text)), ptr(out), C.c_int64(cap), C.byref(n))
    if rc != 0:
        raise SvxError("svx_sam_header_host failed: %s" % _abi.ERRORS.get(rc, rc))
    return out[:n.value].tobytes()


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")])
    return _LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise SvxError("svim_amd/libsvx.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C svim_amd/csrc`); the GPU path has no CPU fallback")
        L = C.CDLL(_LIB_PATH)
        L.svx_last_error.restype = C.c_char_p
        L.svx_stream.restype = C.c_void_p
        _LIB = L
    return _LIB


def host_empty(n, dtype):
    """numpy array of n elements in page-locked memory the LIBRARY owns (svx_host_alloc, include/svx.h): svx_collect uploads such an array without the bounce
    pass a pageable numpy array costs.  The block goes back to the library when the array (and every view of it) is gone.  Raises SvxError when the memory
    cannot be had (no GPU): callers that only want the speed-up fall back to numpy themselves."""
    import weakref
    L = lib()
    L.svx_host_alloc.restype = C.c_void_p
    L.svx_host_alloc.argtypes = [C.c_uint64]
    L.svx_host_free.argtypes = [C.c_void_p]
    dt = np.dtype(dtype)
    nbytes = max(1, int(n) * dt.itemsize)
    p = L.svx_host_alloc(C.c_uint64(nbytes))
    if not p:
        raise SvxError("svx_host_alloc(%d) failed: %s" % (nbytes, L.svx_last_error().decode("utf-8", "replace")))
    buf = (C.c_uint8 * nbytes).from_address(p)
    weakref.finalize(buf, L.svx_host_free, C.c_void_p(p))
    return np.frombuffer(buf, dtype=dt, count=int(n))


def _check(rc, what):
    if rc != 0:
        msg = lib().svx_last_error().decode("utf-8", "replace")
        raise SvxError("%s failed: %s (%s)" % (what, _abi.ERRORS.get(rc, rc), msg))


class Engine(object):
    """One libsvx context on one GPU."""

    def __init__(self, device=0):
        self.L = lib()
        self.ctx = C.c_void_p()
        _check(self.L.svx_ctx_create(C.c_int(device), C.byref(self.ctx)), "svx_ctx_create")
        self.device = device
        self._keep = []
        self.collect_generation = 0          # bumped by every svx_collect: identifies which tables the context holds (svim_amd/lazy.py)

    def close(self):
        if self.ctx:
            self.L.svx_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- COLLECT ----
    def collect(self, hb, params, fetch=True):
        b = hb.struct() if hasattr(hb, "struct") else hb
        self.collect_generation += 1
        _check(self.L.svx_collect(self.ctx, C.byref(b), C.byref(params)), "svx_collect")
        if not fetch:
            return None
        return self.fetch_signatures(0), self.fetch_signatures(1)

    def accumulate(self, on):
        """on: every following collect() appends to the resident signature lists (the batches of one file); off: one batch per call"""
        _check(self.L.svx_collect_accumulate(self.ctx, C.c_int(1 if on else 0)), "svx_collect_accumulate")
        self.collect_generation += 1

    def set_slot_base(self, base):
        _check(self.L.svx_collect_set_slot_base(self.ctx, C.c_uint64(int(base))), "svx_collect_set_slot_base")

    def collect_counts(self):
        n, ns, nb = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.L.svx_collect_count(self.ctx, C.byref(n), C.byref(ns), C.byref(nb)), "svx_collect_count")
        return n.value, ns.value, nb.value

    def fetch_signatures(self, which):
        n, ns, nb = self.collect_counts()
        t = SigTable(n if which == 0 else nb, ns if which == 0 else 0)
        v = t.view()
        _check(self.L.svx_collect_fetch(self.ctx, which, C.byref(v)), "svx_collect_fetch")
        return t

    def collect_geometry(self):
        """geometry table of the last collect() (svx_collect_geom_fetch): (records int32[n_rec, 5], segment rows int32[n_seg, 5]); which entries are defined: svx.h"""
        nr, ns = C.c_int64(), C.c_int64()
        _check(self.L.svx_collect_geom_fetch(self.ctx, C.byref(nr), C.byref(ns), None), "svx_collect_geom_fetch")
        g = np.zeros((max(1, nr.value + ns.value), 5), dtype=np.int32)
        _check(self.L.svx_collect_geom_fetch(self.ctx, None, None, ptr(g)), "svx_collect_geom_fetch")
        return g[:nr.value], g[nr.value:nr.value + ns.value]

    # ---- CLUSTER ----
    def set_genome(self, off, codes, on_device=False):
        g = _abi.Genome(1 if on_device else 0, len(off) - 1 if not on_device else int(off.shape[0]) - 1, ptr(off), ptr(codes))
        self._keep = [off, codes]
        _check(self.L.svx_set_genome(self.ctx, C.byref(g)), "svx_set_genome")

    def load_genome_fasta(self, path, references):
        """The genome of a FASTA file (plain, BGZF, gzip) parsed, compacted and encoded on the device (svx_genome_load_fasta) and set in the context, as
        set_genome(*convert.genome_arrays(path, references)) would -> (off int64[n + 1], stats dict).  FastaHostRoute: the file is one for the host parser
        (convert.load_genome takes that route by itself)."""
        references = list(references)
        off = np.zeros(len(references) + 1, dtype=np.int64)
        st = _abi.FastaStats()
        rc = self.L.svx_genome_load_fasta(self.ctx, os.fsencode(path), C.c_int32(len(references)), _names_blob(references), ptr(off), C.byref(st))
        if rc in (_abi.SVX_E_FASTA_HOST, _abi.SVX_E_FASTA_SYMBOL):
            raise FastaHostRoute("%s: %s" % (_abi.ERRORS[rc], self.L.svx_last_error().decode("utf-8", "replace")), rc, st.as_dict())
        _check(rc, "svx_genome_load_fasta")
        self._keep = []
        return off, st.as_dict()

    def fetch_genome(self):
        """(off, codes) of the genome resident in the context, however it was set"""
        n, total = C.c_int32(), C.c_int64()
        _check(self.L.svx_genome_fetch(self.ctx, C.byref(n), C.byref(total), None, None), "svx_genome_fetch")
        off = np.zeros(n.value + 1, dtype=np.int64)
        codes = np.zeros(max(1, total.value), dtype=np.uint8)
        _check(self.L.svx_genome_fetch(self.ctx, None, None, ptr(off), ptr(codes)), "svx_genome_fetch")
        return off, codes

    def cluster(self, params, contig_rank, table=None, source=2, fetch=True):
        v = table.view() if (table is not None and hasattr(table, "view")) else (table if table is not None else _abi.SigView())
        rank = np.ascontiguousarray(contig_rank, dtype=np.int32)
        self._resident_ct, self._last_contig_rank = None, rank
        self._resident_cand = None
        _check(self.L.svx_cluster(self.ctx, source, C.byref(v), len(rank), ptr(rank), C.byref(params)), "svx_cluster")
        if not fetch:
            return None
        ct = self._resident_ct = self.fetch_clusters()       # (SVIM_COMBINE: lists that are views of this very table combine without an upload)
        return ct

    def partitions(self):
        """partitions of the last cluster() call (svx_cluster_partitions_fetch): list of lists of signature indices, in the order they were formed"""
        n, npart = C.c_int64(), C.c_int64()
        _check(self.L.svx_cluster_partitions_fetch(self.ctx, C.byref(n), C.byref(npart), None, None), "svx_cluster_partitions_fetch")
        if n.value <= 0:
            return []
        sidx, start = np.zeros(n.value, dtype=np.uint32), np.zeros(npart.value + 1, dtype=np.int64)
        _check(self.L.svx_cluster_partitions_fetch(self.ctx, None, None, ptr(sidx), ptr(start)), "svx_cluster_partitions_fetch")
        return [[int(i) for i in sidx[int(start[k]):int(start[k + 1])]] for k in range(npart.value)]

    def fetch_clusters(self):
        n, nm = C.c_int64(), C.c_int64()
        _check(self.L.svx_cluster_count(self.ctx, C.byref(n), C.byref(nm)), "svx_cluster_count")
        ct = ClusterTable(n.value, nm.value)
        cv = ct.view()
        _check(self.L.svx_cluster_fetch(self.ctx, C.byref(cv)), "svx_cluster_fetch")
        ct.finish(cv)
        return ct

    # ---- COMBINE ----
    def combine(self, cparams, contig_rank, table=None, sig_aux=None, fetch=True):
        """svx_combine: the clusters resident from the last cluster() call (table None, source 0) or the ClusterTable `table` whose members index the
        signatures of the aux column `sig_aux` (source 2) -> CandidateTable (fetch False: it stays on the device).  NoDeletionClusters: see there."""
        rank = np.ascontiguousarray(contig_rank, dtype=np.int32)
        if table is None:
            rc = self.L.svx_combine(self.ctx, 0, None, None, C.c_int64(0), C.c_int32(0), C.c_int32(len(rank)), ptr(rank if rank.size else np.zeros(1, np.int32)),
                                    C.byref(cparams))
        else:
            v = table.view()
            for k in range(6):
                v.type_count[k] = int(table.type_count[k])
            aux = np.ascontiguousarray(sig_aux if sig_aux is not None else np.zeros(0, np.uint8), dtype=np.uint8)
            rc = self.L.svx_combine(self.ctx, 2, C.byref(v), ptr(aux if aux.size else np.zeros(1, np.uint8)), C.c_int64(aux.size), C.c_int32(0),
                                    C.c_int32(len(rank)), ptr(rank if rank.size else np.zeros(1, np.int32)), C.byref(cparams))
        if rc == _abi.SVX_E_NO_DELETION:
            raise NoDeletionClusters(self.L.svx_last_error().decode("utf-8", "replace"))
        _check(rc, "svx_combine")
        self._resident_cand = self._resident_gt_table = None
        if not fetch:
            return None
        t = self.fetch_candidates()
        if table is None:      # (SVIM_COMBINE.write_final_vcf: lists that are views of this very table are written without an upload)
            self._resident_cand, self._resident_cand_generation = t, self.collect_generation
        return t

    def fetch_candidates(self):
        n, nm = C.c_int64(), C.c_int64()
        _check(self.L.svx_combine_count(self.ctx, C.byref(n), C.byref(nm)), "svx_combine_count")
        t = _abi.CandidateTable(n.value, nm.value)
        v = t.view()
        _check(self.L.svx_combine_fetch(self.ctx, C.byref(v)), "svx_combine_fetch")
        return t.finish(v)

    def combine_stages(self):
        """intermediates of the last combine() (svx_combine_stages_fetch) -> dict: merged (the DUP_INT clusters merged from an insertion and two breakend
        clusters, as a CandidateTable of cluster rows), remove_1 / remove_2 (insertion list indices, int32), flagged (DUP_INT candidates before re-clustering)"""
        mv, fv = _abi.CandidateView(), _abi.CandidateView()
        n1, n2 = C.c_int64(), C.c_int64()
        _check(self.L.svx_combine_stages_fetch(self.ctx, C.byref(mv), C.byref(n1), None, C.byref(n2), None, C.byref(fv)), "svx_combine_stages_fetch")
        merged, flagged = _abi.CandidateTable(mv.n, mv.n_members), _abi.CandidateTable(fv.n, fv.n_members)
        r1, r2 = np.zeros(max(1, n1.value), np.int32), np.zeros(max(1, n2.value), np.int32)
        mv, fv = merged.view(), flagged.view()
        _check(self.L.svx_combine_stages_fetch(self.ctx, C.byref(mv), C.byref(n1), ptr(r1), C.byref(n2), ptr(r2), C.byref(fv)), "svx_combine_stages_fetch")
        return {"merged": merged.finish(mv), "remove_1": r1[:n1.value], "remove_2": r2[:n2.value], "flagged": flagged.finish(fv)}

    def combine_stats(self):
        s = _abi.CombineStats()
        _check(self.L.svx_combine_get_stats(self.ctx, C.byref(s)), "svx_combine_get_stats")
        return s.as_dict()

    # ---- VCF text ----
    def vcf(self, vparams, references, table=None, sig_read_id=None, sig_seq_off=None, sig_seq=None, gt=None, ref_reads=None, alt_reads=None, read_names=None,
            zmw_id=None, resident_genotypes=False, position_order=None):
        """svx_vcf: the body of variants.vcf (every line behind the header) of the candidates resident from the last combine() of the resident clusters
        (table None, source 0) or of the CandidateTable `table` whose members index signatures with the columns sig_read_id / sig_seq_off / sig_seq (source 2).
        references: names of the table's contig ids.  gt (codes of _abi.VCF_GT) / ref_reads / alt_reads (-1 = None): genotype columns, default "./." / None.
        resident_genotypes (table None, no column given): the columns the last genotype_resident() left for the resident candidates, read in place.
        read_names: names by read id (vparams.read_names); zmw_id: convert.zmw_ids of them (vparams.zmws).  position_order (None: vparams.position_order,
        off by default): the same lines with the same ids sorted by (contig, POS) - what tabix asks for (svx_vcf_position_order).  The text stays on the device:
        -> (number of lines, number of bytes); vcf_fetch() / vcf_line_offsets() bring it over."""
        from . import convert
        references = list(references)
        keep = []

        def arr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return ptr(a if a.size else np.zeros(1, dt))
        blob = b"".join(os.fsencode(r) + b"\0" for r in references) or b"\0"
        rank = convert.natural_ranks(references)
        inp = _abi.VcfInputs()
        inp.gt, inp.ref_reads, inp.alt_reads = arr(gt, np.uint8), arr(ref_reads, np.int32), arr(alt_reads, np.int32)
        cbuf = C.create_string_buffer(blob, len(blob))
        inp.contig_names_nul_separated, inp.n_contig, inp.contig_natural_rank = C.cast(cbuf, C.c_void_p), len(references), arr(rank, np.int32)
        rbuf = None
        if vparams.read_names or vparams.zmws:
            if read_names is None:
                raise ValueError("Engine.vcf: read_names / zmws need the read names")
            inp.n_reads = len(read_names)
        if vparams.read_names:
            enc = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in read_names]
            off = np.zeros(len(enc) + 1, dtype=np.int64)
            if enc:
                np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
            data = b"".join(enc) or b"\0"
            rbuf = C.create_string_buffer(data, len(data))
            inp.read_names_blob, inp.read_name_off = C.cast(rbuf, C.c_void_p), arr(off, np.int64)
        if vparams.zmws:
            inp.zmw_id = arr(convert.zmw_ids(read_names) if zmw_id is None else zmw_id, np.int32)
        if position_order is None:
            position_order = bool(getattr(vparams, "position_order", False))
        _check(self.L.svx_vcf_position_order(self.ctx, C.c_int(1 if position_order else 0)), "svx_vcf_position_order")
        try:
            rc = self._vcf_call(vparams, inp, table, sig_read_id, sig_seq_off, sig_seq, resident_genotypes, arr, keep)
        finally:
            self.L.svx_vcf_position_order(self.ctx, C.c_int(0))
        _check(rc, "svx_vcf")
        del keep, cbuf, rbuf
        return self.vcf_count()

    def _vcf_call(self, vparams, inp, table, sig_read_id, sig_seq_off, sig_seq, resident_genotypes, arr, keep):
        if table is None:
            _check(self.L.svx_vcf_use_resident_genotypes(self.ctx, C.c_int(1 if resident_genotypes else 0)), "svx_vcf_use_resident_genotypes")
            try:
                rc = self.L.svx_vcf(self.ctx, 0, None, None, C.byref(vparams), C.byref(inp))
            finally:
                self.L.svx_vcf_use_resident_genotypes(self.ctx, C.c_int(0))
        else:
            v = table.view()
            for k in range(6):
                v.class_count[k] = int(table.class_count[k])
            sv = _abi.SigView()
            rid = np.ascontiguousarray(sig_read_id if sig_read_id is not None else np.zeros(0, np.int32), dtype=np.int32)
            sv.on_device, sv.n, sv.read_id = 0, rid.size, ptr(rid if rid.size else np.zeros(1, np.int32))
            keep.append(rid)
            if sig_seq_off is not None:
                sv.seq_off, sv.seq = arr(sig_seq_off, np.int64), arr(sig_seq if sig_seq is not None else np.zeros(1, np.uint8), np.uint8)
            rc = self.L.svx_vcf(self.ctx, 2, C.byref(v), C.byref(sv), C.byref(vparams), C.byref(inp))
        return rc

    def vcf_count(self):
        n, nb = C.c_int64(), C.c_int64()
        _check(self.L.svx_vcf_count(self.ctx, C.byref(n), C.byref(nb)), "svx_vcf_count")
        return n.value, nb.value

    def vcf_fetch(self, offset=0, nbytes=None):
        """bytes [offset, offset + nbytes) of the text of the last vcf() call (svx_vcf_fetch; nbytes None: to the end) -> bytes"""
        _, total = self.vcf_count()
        nbytes = total - offset if nbytes is None else nbytes
        buf = np.zeros(max(1, nbytes), dtype=np.uint8)
        _check(self.L.svx_vcf_fetch(self.ctx, C.c_int64(offset), C.c_int64(nbytes), ptr(buf), None), "svx_vcf_fetch")
        return buf[:nbytes].tobytes()

    def vcf_line_offsets(self):
        """int64[n_lines + 1]: where every line of the last vcf() call starts in its text"""
        n, _ = self.vcf_count()
        off = np.zeros(n + 1, dtype=np.int64)
        _check(self.L.svx_vcf_fetch(self.ctx, C.c_int64(0), C.c_int64(0), None, ptr(off)), "svx_vcf_fetch")
        return off

    def vcf_stats(self):
        s = _abi.VcfStats()
        _check(self.L.svx_vcf_get_stats(self.ctx, C.byref(s)), "svx_vcf_get_stats")
        return s.as_dict()

    # ---- BED / signature-VCF text ----
    def format_repr(self, values):
        """svx_format_repr_device: repr of every float64 of `values` by the device build of csrc/fmt_repr.hpp -> list of str"""
        x = np.ascontiguousarray(values, dtype=np.float64)
        out = np.zeros((max(1, x.size), 32), dtype=np.uint8)
        _check(self.L.svx_format_repr_device(self.ctx, C.c_int64(x.size), ptr(x if x.size else np.zeros(1)), ptr(out)), "svx_format_repr_device")
        return [b.decode("ascii") for b in out[:x.size].view("S32").ravel().tolist()]

    def bed_set_read_names(self, read_names):
        """svx_bed_set_read_names: the names by read id every member piece ends with, uploaded once and kept in the context until replaced.  The list handed in
        last is remembered by identity: handing the same list again uploads nothing."""
        if read_names is getattr(self, "_bed_names", None):
            return
        enc = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in read_names]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        if enc:
            np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
        data = b"".join(enc) or b"\0"
        rbuf = C.create_string_buffer(data, len(data))
        self._bed_names = None
        _check(self.L.svx_bed_set_read_names(self.ctx, C.cast(rbuf, C.c_void_p), ptr(off), C.c_int64(len(enc))), "svx_bed_set_read_names")
        self._bed_names = read_names

    def bed(self, product, references, table=None, sigs=None, read_names=None, debug_short_line=0):
        """svx_bed: the text of one product (_abi.BED_SIGNATURE_BEDS: 7 files, BED_SIGNATURE_VCF: the lines of all.vcf behind the header, BED_CANDIDATE_BEDS:
        8 files) from the tables resident in the context (table None, source 0: the clusters of the last cluster(), the candidates of the last combine()) or
        from `table` (a ClusterTable, for BED_CANDIDATE_BEDS a CandidateTable) whose members index the SigTable `sigs` (source 2).  references: names of the
        tables' contig ids; read_names: names by read id (uploaded only when it is another list than last time).  The text stays on the device:
        -> (number of files, lines, bytes); bed_fetch() / bed_file_offsets() / bed_line_offsets() bring it over."""
        from . import batch
        references = list(references)
        if read_names is not None:
            self.bed_set_read_names(read_names)
        blob = b"".join(os.fsencode(r) + b"\0" for r in references) or b"\0"
        cbuf = C.create_string_buffer(blob, len(blob))
        rank = np.ascontiguousarray(batch.contig_ranks(references), dtype=np.int32)
        inp = _abi.BedInputs()
        inp.contig_names_nul_separated, inp.n_contig = C.cast(cbuf, C.c_void_p), len(references)
        inp.contig_str_rank = ptr(rank if rank.size else np.zeros(1, np.int32))
        inp.debug_short_line = int(debug_short_line)
        if table is None:
            rc = self.L.svx_bed(self.ctx, C.c_int(product), 0, None, None, None, C.byref(inp))
        else:
            v = table.view()
            counts = table.class_count if product == _abi.BED_CANDIDATE_BEDS else table.type_count
            for k in range(6):
                (v.class_count if product == _abi.BED_CANDIDATE_BEDS else v.type_count)[k] = int(counts[k])
            sv = sigs.view() if sigs is not None else None
            cl, cv = (None, C.byref(v)) if product == _abi.BED_CANDIDATE_BEDS else (C.byref(v), None)
            rc = self.L.svx_bed(self.ctx, C.c_int(product), 2, cl, cv, C.byref(sv) if sv is not None else None, C.byref(inp))
        _check(rc, "svx_bed")
        del cbuf
        return self.bed_count()

    def bed_count(self):
        nf, n, nb = C.c_int32(), C.c_int64(), C.c_int64()
        _check(self.L.svx_bed_count(self.ctx, C.byref(nf), C.byref(n), C.byref(nb)), "svx_bed_count")
        return nf.value, n.value, nb.value

    def bed_fetch(self, offset=0, nbytes=None):
        """bytes [offset, offset + nbytes) of the text of the last bed() call (svx_bed_fetch; nbytes None: to the end) -> bytes"""
        _, _, total = self.bed_count()
        nbytes = total - offset if nbytes is None else nbytes
        buf = np.zeros(max(1, nbytes), dtype=np.uint8)
        _check(self.L.svx_bed_fetch(self.ctx, C.c_int64(offset), C.c_int64(nbytes), ptr(buf), None, None, None), "svx_bed_fetch")
        return buf[:nbytes].tobytes()

    def bed_file_offsets(self):
        """(int64[n_files + 1] byte offsets of the files in the text of the last bed() call, int64[n_files + 1] first line of every file)"""
        nf, _, _ = self.bed_count()
        off, lines = np.zeros(_abi.BED_MAX_FILES + 1, dtype=np.int64), np.zeros(_abi.BED_MAX_FILES + 1, dtype=np.int64)
        _check(self.L.svx_bed_fetch(self.ctx, C.c_int64(0), C.c_int64(0), None, ptr(off), ptr(lines), None), "svx_bed_fetch")
        return off[:nf + 1], lines[:nf + 1]

    def bed_line_offsets(self):
        """int64[n_lines + 1]: where every line of the last bed() call starts in its text"""
        _, n, _ = self.bed_count()
        off = np.zeros(n + 1, dtype=np.int64)
        _check(self.L.svx_bed_fetch(self.ctx, C.c_int64(0), C.c_int64(0), None, None, None, ptr(off)), "svx_bed_fetch")
        return off

    def bed_stats(self):
        s = _abi.BedStats()
        _check(self.L.svx_bed_get_stats(self.ctx, C.byref(s)), "svx_bed_get_stats")
        return s.as_dict()

    # ---- BGZF output ----
    def text_gz(self, source, data=None, file_off=None):
        """svx_text_gz: the BGZF stream of a text, made and kept on the device.  source _abi.TEXT_GZ_VCF: the text of the last vcf() (one file); TEXT_GZ_BED:
        the text of the last bed() (its files); TEXT_GZ_HOST: `data` (bytes), uploaded - one file, or the files data[file_off[k]:file_off[k + 1]].
        -> (number of files, blocks, bytes); text_gz_fetch() / text_gz_tables() bring the stream and its tables over.  A later vcf() / bed() voids the stream
        of its text."""
        if source == _abi.TEXT_GZ_HOST:
            data = bytes(data if data is not None else b"")
            off = np.ascontiguousarray(file_off if file_off is not None else [0, len(data)], dtype=np.int64)
            if off.size < 2 or int(off[-1]) != len(data):
                raise ValueError("text_gz: file_off must hold n_files + 1 offsets and end at len(data)")
            src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
            rc = self.L.svx_text_gz(self.ctx, C.c_int(2), ptr(src), ptr(off), C.c_int32(off.size - 1))
        else:
            rc = self.L.svx_text_gz(self.ctx, C.c_int(source), None, None, C.c_int32(0))
        _check(rc, "svx_text_gz")
        return self.text_gz_count()

    def text_gz_count(self):
        nf, nb, n = C.c_int32(), C.c_int64(), C.c_int64()
        _check(self.L.svx_text_gz_count(self.ctx, C.byref(nf), C.byref(nb), C.byref(n)), "svx_text_gz_count")
        return nf.value, nb.value, n.value

    def text_gz_fetch(self, offset=0, nbytes=None):
        """bytes [offset, offset + nbytes) of the stream of the last text_gz() call (svx_text_gz_fetch; nbytes None: to the end) -> bytes"""
        _, _, total = self.text_gz_count()
        nbytes = total - offset if nbytes is None else nbytes
        buf = np.zeros(max(1, nbytes), dtype=np.uint8)
        _check(self.L.svx_text_gz_fetch(self.ctx, C.c_int64(offset), C.c_int64(nbytes), ptr(buf), None, None, None), "svx_text_gz_fetch")
        return buf[:nbytes].tobytes()

    def text_gz_tables(self):
        """(int64[n_files + 1] offsets of the files in the stream, int64[n_blocks + 1] offsets of the blocks in the stream, int64[n_blocks + 1] offsets of
        their text in the text) of the last text_gz() call: what a .gzi or tabix index would be built from"""
        nf, nb, _ = self.text_gz_count()
        fo, co, uo = np.zeros(nf + 1, dtype=np.int64), np.zeros(nb + 1, dtype=np.int64), np.zeros(nb + 1, dtype=np.int64)
        _check(self.L.svx_text_gz_fetch(self.ctx, C.c_int64(0), C.c_int64(0), None, ptr(fo), ptr(co), ptr(uo)), "svx_text_gz_fetch")
        return fo, co, uo

    def text_gz_stats(self):
        s = _abi.TextGzStats()
        _check(self.L.svx_text_gz_get_stats(self.ctx, C.byref(s)), "svx_text_gz_get_stats")
        return s.as_dict()

    # ---- tabix index of the BGZF stream ----
    def text_index(self, preset, stream_base=None, fmt="tbi"):
        """svx_text_index: the uncompressed .tbi bytes of every file of the last text_gz() call, built on the device from its text and block table.
        preset: _abi.INDEX_VCF / INDEX_BED; stream_base: per file, the bytes written in front of its stream in its .gz file (a header compressed on the host;
        None: 0; a number: one file).  -> (number of files, bytes); text_index_fetch() brings them over.  Void whenever the stream is.
        fmt="csi": the uncompressed .csi bytes (svx_text_index_fmt; svim_amd/csi.py): no file is out of range in that format."""
        nf = self.text_gz_count()[0]
        sb = None
        if stream_base is not None:
            sb = np.ascontiguousarray(np.atleast_1d(stream_base), dtype=np.int64)
            if sb.size != nf:
                raise ValueError("text_index: stream_base needs one entry per file (%d)" % nf)
        if fmt == "tbi":
            _check(self.L.svx_text_index(self.ctx, C.c_int(preset), ptr(sb) if sb is not None else None), "svx_text_index")
        else:
            _check(self.L.svx_text_index_fmt(self.ctx, C.c_int(preset), ptr(sb) if sb is not None else None, C.c_int(_abi.index_format(fmt, "tbi"))), "svx_text_index_fmt")
        return self.text_index_count()

    def text_index_count(self):
        nf, n = C.c_int32(), C.c_int64()
        _check(self.L.svx_text_index_count(self.ctx, C.byref(nf), C.byref(n)), "svx_text_index_count")
        return nf.value, n.value

    def text_index_fetch(self):
        """-> (list of bytes, one uncompressed .tbi per file, b"" for a file without one; int32[n_files] status: 0, _abi.SVX_E_ORDER, _abi.SVX_E_RANGE)"""
        nf, n = self.text_index_count()
        buf, off, status = np.zeros(max(1, n), dtype=np.uint8), np.zeros(nf + 1, dtype=np.int64), np.zeros(max(1, nf), dtype=np.int32)
        _check(self.L.svx_text_index_fetch(self.ctx, ptr(buf), ptr(off), ptr(status)), "svx_text_index_fetch")
        return [buf[int(off[k]):int(off[k + 1])].tobytes() for k in range(nf)], status[:nf]

    def text_index_stats(self):
        s = _abi.TextIndexStats()
        _check(self.L.svx_text_index_get_stats(self.ctx, C.byref(s)), "svx_text_index_get_stats")
        return s.as_dict()

    def set_alignment_index(self, index):
        """index: svim_amd.SVIM_genotyping.AlignmentIndex (arrays are copied to the device)"""
        v = index.view()
        _check(self.L.svx_set_alignment_index(self.ctx, C.byref(v)), "svx_set_alignment_index")

    def genotype(self, mode, tid, start, end, member_off, member_names, min_mapq):
        n = len(tid)
        out = np.zeros(max(1, n), dtype=np.int32)
        tid = np.ascontiguousarray(tid, dtype=np.int32); start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32); member_off = np.ascontiguousarray(member_off, dtype=np.int64)
        member_names = np.ascontiguousarray(member_names, dtype=np.int32)
        _check(self.L.svx_genotype(self.ctx, C.c_int32(mode), C.c_int64(n), ptr(tid), ptr(start), ptr(end), ptr(member_off),
                                   ptr(member_names if member_names.size else np.zeros(1, np.int32)), C.c_int32(min_mapq), ptr(out)), "svx_genotype")
        return out[:n]

    # ---- GENOTYPE from resident tables ----
    def keep_alignments(self, on, order="file", file_flags=False):
        """on: while accumulate() is on too, every collect() appends its batch's records to the alignment table resident in the context
        (svx_collect_keep_alignments) - what genotype_resident() joins the candidates with.
        order="sort": the records may come in any order; the table is brought into coordinate order (svim_amd/bamsort.py, ties in append order) on the
        device when it is first used, instead of being refused.  file_flags: a record marked SVX_FLAG_SKIP by the query-name front end keeps its own flag
        and the end its CIGAR gives (svx_collect_keep_alignments_mode)"""
        if order not in ("file", "sort"):
            raise ValueError("order: 'file' or 'sort'")
        flags = (_abi.SVX_ALN_SORT if order == "sort" else 0) | (_abi.SVX_ALN_FILE_FLAGS if file_flags else 0)
        if flags == 0:
            _check(self.L.svx_collect_keep_alignments(self.ctx, C.c_int(1 if on else 0)), "svx_collect_keep_alignments")
        else:
            _check(self.L.svx_collect_keep_alignments_mode(self.ctx, C.c_int(1 if on else 0), C.c_uint32(flags)), "svx_collect_keep_alignments_mode")

    def alignments_permutation(self):
        """the append position of every row of the resident alignment table (svx_alignments_permutation) -> uint32[n]; the identity when no finalisation
        had to sort.  SvxError before the table has been finalised (the first genotype_resident() after an append does that)"""
        n = C.c_int64()
        _check(self.L.svx_alignments_count(self.ctx, C.byref(n)), "svx_alignments_count")
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        _check(self.L.svx_alignments_permutation(self.ctx, ptr(out)), "svx_alignments_permutation")
        return out[:n.value]

    def alignment_sort_stats(self):
        s = _abi.AlignmentSortStats()
        _check(self.L.svx_alignments_get_sort_stats(self.ctx, C.byref(s)), "svx_alignments_get_sort_stats")
        return s.as_dict()

    def alignments(self):
        """the resident alignment table (svx_alignments_fetch) -> dict of numpy columns tid, pos, end, flag, mapq, read_id, in the table's current order:
        file (append) order, or coordinate order once a finalisation of keep_alignments(order="sort") has sorted it"""
        n = C.c_int64()
        _check(self.L.svx_alignments_count(self.ctx, C.byref(n)), "svx_alignments_count")
        cols = dict(tid=np.int32, pos=np.int32, end=np.int32, flag=np.uint16, mapq=np.uint8, read_id=np.int32)
        out = {k: np.zeros(max(1, n.value), dtype=dt) for k, dt in cols.items()}
        _check(self.L.svx_alignments_fetch(self.ctx, *[ptr(out[k]) for k in cols]), "svx_alignments_fetch")
        return {k: a[:n.value] for k, a in out.items()}

    def alignments_stats(self):
        s = _abi.AlignmentsStats()
        _check(self.L.svx_alignments_get_stats(self.ctx, C.byref(s)), "svx_alignments_get_stats")
        return s.as_dict()

    def genotype_resident(self, options, lengths, table=None, sig_read_id=None):
        """svx_genotype_resident: genotype() of the reference for the DEL, INV, INS and DUP_INT rows of the candidates resident from the last combine() of
        resident clusters (table None, source 0) or of the CandidateTable `table` whose members index signatures with the read ids `sig_read_id` (source 2),
        against the resident alignment table.  options: minimum_score, min_mapq, minimum_depth, homozygous_threshold, heterozygous_threshold (or a
        _abi.GenotypeParams); lengths: reference lengths by contig id.  The columns stay on the device: fetch_genotypes() brings them over."""
        gp = options if isinstance(options, _abi.GenotypeParams) else _abi.GenotypeParams.from_options(options)
        clen = np.ascontiguousarray(lengths, dtype=np.int64)
        self._resident_gt_table = None
        if table is None:
            rc = self.L.svx_genotype_resident(self.ctx, 0, None, None, C.c_int64(0), C.c_int32(clen.size), ptr(clen if clen.size else np.zeros(1, np.int64)),
                                              C.byref(gp))
        else:
            v = table.view()
            for k in range(6):
                v.class_count[k] = int(table.class_count[k])
            rid = np.ascontiguousarray(sig_read_id if sig_read_id is not None else np.zeros(0, np.int32), dtype=np.int32)
            rc = self.L.svx_genotype_resident(self.ctx, 2, C.byref(v), ptr(rid if rid.size else np.zeros(1, np.int32)), C.c_int64(rid.size), C.c_int32(clen.size),
                                              ptr(clen if clen.size else np.zeros(1, np.int64)), C.byref(gp))
        _check(rc, "svx_genotype_resident")
        if table is None:      # (SVIM_COMBINE.vcf_body_device: views of this very table are written with these columns, read in place)
            self._resident_gt_table = getattr(self, "_resident_cand", None)

    def fetch_genotypes(self):
        """columns of the last genotype_resident() (svx_genotype_fetch) -> dict: gt (uint8 codes of _abi.GT_NAMES), ref_reads / alt_reads (int32, -1 = None),
        support_fraction (float64, NaN = ".")"""
        n = C.c_int64()
        _check(self.L.svx_genotype_count(self.ctx, C.byref(n)), "svx_genotype_count")
        out = dict(gt=np.zeros(max(1, n.value), np.uint8), ref_reads=np.zeros(max(1, n.value), np.int32), alt_reads=np.zeros(max(1, n.value), np.int32),
                   support_fraction=np.zeros(max(1, n.value), np.float64))
        _check(self.L.svx_genotype_fetch(self.ctx, ptr(out["gt"]), ptr(out["ref_reads"]), ptr(out["alt_reads"]), ptr(out["support_fraction"])), "svx_genotype_fetch")
        return {k: a[:n.value] for k, a in out.items()}

    def genotype_stats(self):
        s = _abi.GenotypeStats()
        _check(self.L.svx_genotype_get_stats(self.ctx, C.byref(s)), "svx_genotype_get_stats")
        return s.as_dict()

    def set_ranks(self, rank, world, allgather=None):
        """Contig-sharded ranks (svx_cluster_set_ranks): this engine is rank `rank` of `world`; allgather(send: bytes) -> bytes of all ranks, rank-major
        (len(send) * world) - or an object that also has gather_into(send_addr, recv_addr, nbytes) - is the transport svx_cluster uses to find where its random.sample streams start.  allgather None / world 1: single rank."""
        if allgather is None or world <= 1:
            self._ag_cb = None
            _check(self.L.svx_cluster_set_ranks(self.ctx, 0, 1, None, None), "svx_cluster_set_ranks")
            return
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)

        into = getattr(allgather, "gather_into", None)      # a transport that works on the buffers themselves (multigpu.TorchAllGather)

        def tramp(user, send, recv, nbytes):
            try:
                if into is not None and nbytes > 0:
                    into(int(send), int(recv), int(nbytes))
                    return 0
                got = allgather(C.string_at(send, nbytes))
                if len(got) != nbytes * world:
                    raise ValueError("all-gather callback returned %d bytes, expected %d" % (len(got), nbytes * world))
                C.memmove(recv, got, len(got))
                return 0
            except Exception:                       # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._ag_cb = proto(tramp)
        _check(self.L.svx_cluster_set_ranks(self.ctx, int(rank), int(world), self._ag_cb, None), "svx_cluster_set_ranks")

    def abort_ranks(self):
        """tell the other ranks this one will not reach svx_cluster (they fail instead of waiting in the rank exchange)"""
        _check(self.L.svx_cluster_abort_ranks(self.ctx), "svx_cluster_abort_ranks")

    def stream_positions(self):
        """(start[6], end[6]): where each type's random.sample stream started / stopped on this rank in the last cluster call"""
        a, b = (C.c_int64 * 6)(), (C.c_int64 * 6)()
        _check(self.L.svx_cluster_stream_positions(self.ctx, a, b), "svx_cluster_stream_positions")
        return list(a), list(b)

    def stats(self):
        s = _abi.Stats()
        _check(self.L.svx_get_stats(self.ctx, C.byref(s)), "svx_get_stats")
        return s.as_dict()

    def stream(self):
        return self.L.svx_stream(self.ctx)

    def selftest_prims(self, n, begin_bit=0, end_bit=64, seed=1):
        """the library's own radix sort + exclusive scan on n pseudo-random elements against std::stable_sort / a serial sum (raises on a difference)"""
        _check(self.L.svx_selftest_prims(self.ctx, C.c_int64(n), C.c_int32(begin_bit), C.c_int32(end_bit), C.c_uint64(seed)), "svx_selftest_prims")

    # ---- single-function entry points ----
    def cigar_indel(self, tuples, min_length):
        c = np.array([(l << 4) | op for op, l in tuples] or [0], dtype=np.uint32)
        n = len(tuples)
        o_ref = np.zeros(max(1, n), dtype=np.int64)
        o_read = np.zeros(max(1, n), dtype=np.int64)
        o_len = np.zeros(max(1, n), dtype=np.int32)
        o_del = np.zeros(max(1, n), dtype=np.uint8)
        m = C.c_int64()
        _check(self.L.svx_cigar_indel(self.ctx, ptr(c), C.c_int64(n), C.c_int32(min_length), ptr(o_ref), ptr(o_read),
                                      ptr(o_len), ptr(o_del), C.byref(m)), "svx_cigar_indel")
        return [(int(o_ref[i]), int(o_read[i]), int(o_len[i]), "DEL" if o_del[i] else "INS") for i in range(m.value)]

    def edit_distances(self, pairs):
        """pairs: list of (a, b) strings -> list of unit-cost global edit distances."""
        chunks, a_off, b_off = [], [0], [0]
        pos = 0
        # layout: all a strings, then all b strings; a_off/b_off index into the same code array
        for a, _ in pairs:
            c = _abi.encode_bases(a)
            chunks.append(c)
            pos += c.size
            a_off.append(pos)
        b_off = [pos]
        for _, b in pairs:
            c = _abi.encode_bases(b)
            chunks.append(c)
            pos += c.size
            b_off.append(pos)
        codes = np.concatenate(chunks + [np.zeros(1, np.uint8)])
        a_off = np.array(a_off, dtype=np.int64)
        b_off = np.array(b_off, dtype=np.int64)
        out = np.zeros(max(1, len(pairs)), dtype=np.int32)
        _check(self.L.svx_edit_distance(self.ctx, C.c_int64(len(pairs)), ptr(codes), ptr(a_off), ptr(b_off), ptr(out)),
               "svx_edit_distance")
        return [int(x) for x in out[:len(pairs)]]

    def pair_distances(self, table, pairs, params):
        """span_position_distance of (i, j) pairs of a host SigTable through the device path -> float64 array"""
        ia = np.ascontiguousarray([i for i, _ in pairs], dtype=np.int64)
        ib = np.ascontiguousarray([j for _, j in pairs], dtype=np.int64)
        out = np.zeros(max(1, len(pairs)), dtype=np.float64)
        v = table.view()
        _check(self.L.svx_pair_distances(self.ctx, C.byref(v), C.c_int64(len(pairs)), ptr(ia), ptr(ib), C.byref(params), ptr(out)), "svx_pair_distances")
        return out[:len(pairs)]

    def linkage_fcluster(self, problems, cutoff):
        """problems: list of (n, condensed distance array) -> list of label arrays (1-based, scipy numbering)."""
        ns = np.array([p[0] for p in problems], dtype=np.int32)
        d_off = np.zeros(len(problems) + 1, dtype=np.int64)
        l_off = np.zeros(len(problems) + 1, dtype=np.int64)
        for i, (n, d) in enumerate(problems):
            d_off[i + 1] = d_off[i] + n * (n - 1) // 2
            l_off[i + 1] = l_off[i] + n
        d = np.concatenate([np.asarray(p[1], dtype=np.float64).ravel() for p in problems] + [np.zeros(1)])
        lab = np.zeros(max(1, int(l_off[-1])), dtype=np.int32)
        _check(self.L.svx_linkage_fcluster(self.ctx, C.c_int64(len(problems)), ptr(ns), ptr(d_off), ptr(d), C.c_double(cutoff),
                                           ptr(l_off), ptr(lab)), "svx_linkage_fcluster")
        return [lab[l_off[i]:l_off[i + 1]].copy() for i in range(len(problems))]


def engine(device=None):
    """Process-wide engine for `device` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    e = _ENGINES.get(device)
    if e is None:
        e = _ENGINES[device] = Engine(device)
    return e


def bgzf_blocks(path):
    """(payload bytes, ISIZE) of every BGZF block of a file: the raw DEFLATE stream between the block header and its CRC32 / ISIZE trailer"""
    import struct
    with open(path, "rb") as fh:
        data = fh.read()
    at, out = 0, []
    while at + 18 <= len(data):
        if data[at:at + 2] != b"\x1f\x8b":
            raise ValueError("not a BGZF block at %d" % at)
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        p, bsize = at + 12, None
        while p + 4 <= at + 12 + xlen:
            si, sl = data[p:p + 2], struct.unpack_from("<H", data, p + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, p + 4)[0]
            p += 4 + sl
        if bsize is None:
            raise ValueError("no BC subfield")
        blen = bsize + 1
        out.append((data[at + 12 + xlen:at + blen - 8], struct.unpack_from("<I", data, at + blen - 4)[0]))
        at += blen
    return out


class Inflater(object):
    """svx_inflater: BGZF payloads inflated on the GPU, one wavefront per block (svim_amd/csrc/bgzf.hip).  No CPU fallback."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.L.svx_inflater_staging.restype = C.c_void_p
        _check(self.L.svx_inflater_create(C.c_int(device), C.byref(self.h)), "svx_inflater_create")
        self.kernel_ms = 0.0

    def close(self):
        if self.h:
            self.L.svx_inflater_destroy(self.h)
            self.h = None

    def inflate(self, blocks):
        """blocks: [(payload bytes, isize)] -> the inflated stream as a numpy uint8 array (host); self.kernel_ms = duration of the launch"""
        n = len(blocks)
        in_off = np.zeros(max(1, n), dtype=np.uint64)
        clen = np.array([len(b) for b, _ in blocks] or [0], dtype=np.uint32)
        isize = np.array([s for _, s in blocks] or [0], dtype=np.uint32)
        out_at = np.zeros(max(1, n), dtype=np.uint64)
        at = 0
        for i, (b, _) in enumerate(blocks):
            in_off[i] = at
            at += (len(b) + 7) & ~7
        if n > 1:
            out_at[1:n] = np.cumsum(isize[:n - 1].astype(np.uint64))
        total_out = int(isize[:n].astype(np.uint64).sum()) if n else 0
        stage = self.L.svx_inflater_staging(self.h, C.c_int(0), C.c_uint64(max(at, 8)))
        if not stage:
            raise SvxError("svx_inflater_staging failed")
        buf = (C.c_uint8 * max(at, 8)).from_address(stage)
        view = np.frombuffer(buf, dtype=np.uint8)
        for i, (b, _) in enumerate(blocks):
            o = int(in_off[i])
            view[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        out = np.zeros(max(1, total_out), dtype=np.uint8)
        ms = C.c_float(0)
        _check(self.L.svx_inflater_run(self.h, C.c_int64(n), ptr(in_off), ptr(clen), ptr(isize), ptr(out_at), C.c_uint64(at), ptr(out),
                                       C.c_uint64(total_out), C.c_int(0), C.byref(ms)), "svx_inflater_run")
        self.kernel_ms = float(ms.value)
        return out[:total_out]
