"""ctypes wrapper of the native BAM front-end (svim_amd/csrc/bamio.cpp): BGZF inflate + record decode into the record
batch, on the host, without pysam.  Needs only libsvx.so - no GPU - so it is usable (and tested) on CPU.
A path that holds SAM text is opened through svx_sam_open: such a handle is read by the device reader only (svim_amd/sam.py says what its records are)."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._lib import SvxError, lib


def is_sam_text(path):
    """SAM text: the first byte is '@', or the file does not start with the gzip magic (a BAM file is BGZF, which does) and its first byte may start a QNAME
    ('!' to '~').  Everything else is left to svx_bam_open and its messages: an empty file, a file that cannot be read, bytes that are neither"""
    try:
        with open(path, "rb") as fh:
            head = fh.read(2)
    except OSError:
        return False
    return head[:1] == b"@" or (len(head) > 0 and head != b"\x1f\x8b" and 0x21 <= head[0] <= 0x7e)


class _SortedOutput(object):
    """What a finished sort on the device gives, written once for its two owners: a reader's own sort (NativeBam.sort_*: svx_bam_sort_*) and a merge session
    (BamMerge: svx_bam_merge_*).  The owner brings L, h, _out_prefix - what the names of its C functions start with - and _out_error(rc, what), its error
    factory; an owner whose handle may be gone overrides _out_open(what), and one that keeps its index elsewhere _out_index_bytes()."""
    _out_prefix = None

    def _out_open(self, what):
        pass

    def _out_call(self, name, *args):
        what = self._out_prefix + name
        self._out_open(what)
        rc = getattr(self.L, what)(self.h, *args)
        if rc != 0:
            if rc in (_abi.SVX_E_ORDER, _abi.SVX_E_RANGE) and name == "index_fmt":
                from . import bai
                raise bai.BaiError(rc, "%s failed: %s (%s)" % (what, _abi.ERRORS.get(rc, rc), self.L.svx_last_error().decode("utf-8", "replace")))
            raise self._out_error(rc, what)

    def _out_count(self):
        n, nbytes, nb = C.c_int64(), C.c_int64(), C.c_int64()
        self._out_call("count", C.byref(n), C.byref(nbytes), C.byref(nb))
        return n.value, nbytes.value, nb.value

    def _out_encode(self, first_block, n_blocks, stream=False):
        n = C.c_int64()
        self._out_call("encode", C.c_int64(int(first_block)), C.c_int64(int(n_blocks)), C.byref(n))
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        raw, nraw = None, 0
        if stream:
            total = self._out_count()[1]
            nraw = min(total, (int(first_block) + int(n_blocks)) * _abi.TEXT_GZ_BLOCK) - min(total, int(first_block) * _abi.TEXT_GZ_BLOCK)
            raw = np.zeros(max(1, nraw), dtype=np.uint8)
        self._out_call("fetch", out.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p) if stream else None)
        return (out[:n.value].tobytes(), raw[:nraw].tobytes()) if stream else out[:n.value].tobytes()

    def _out_index(self, fmt):
        self._out_call("index_fmt", C.c_int(_abi.index_format(fmt, "bai")))
        return self._out_index_bytes()

    def _out_index_bytes(self):
        n = C.c_int64()
        self._out_call("index_count", C.byref(n))
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        self._out_call("index_fetch", out.ctypes.data_as(C.c_void_p))
        return out[:n.value].tobytes()

    def _out_permutation(self):
        n = self._out_count()[0]
        perm = np.zeros(max(1, n), dtype=np.uint32)
        self._out_call("permutation", perm.ctypes.data_as(C.c_void_p))
        return perm[:n]

    def _out_stats(self, name, struct, checked=True):
        """checked=False: a reader's stats have never raised (zeros from a handle that is closed)"""
        s = struct()
        if checked:
            self._out_call(name, C.byref(s))
        else:
            getattr(self.L, self._out_prefix + name)(self.h, C.byref(s))
        return s.as_dict()


class NativeBam(_SortedOutput):
    """BAM reader with the handful of pysam.AlignmentFile members SVIM's COLLECT driver uses (references, lengths,
    get_tid/getrname, header['HD']['SO']) plus read_batch(), which yields ready-made svx_batch structs."""
    _out_prefix = "svx_bam_sort_"

    def __init__(self, path, threads=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.is_sam = is_sam_text(path)
        if self.is_sam:
            rc = self.L.svx_sam_open(path.encode(), C.c_int(threads), C.byref(self.h))
        else:
            rc = self.L.svx_bam_open(path.encode(), C.c_int(threads), C.byref(self.h))
        if rc != 0:
            raise SvxError("%s(%r) failed: %s" % ("svx_sam_open" if self.is_sam else "svx_bam_open", path, self.L.svx_last_error().decode()))
        n = C.c_int32()
        names, lens, so = C.c_char_p(), C.POINTER(C.c_int32)(), C.c_char_p()
        blob = C.c_void_p()
        self.L.svx_bam_header(self.h, C.byref(n), C.byref(blob), C.byref(lens), C.byref(so))
        # names: NUL separated, n of them
        out, p = [], blob.value
        for _ in range(n.value):
            s = C.string_at(p)
            out.append(s.decode("ascii"))
            p += len(s) + 1
        self.references = out
        self.lengths = [lens[i] for i in range(n.value)]
        self.sort_order = (so.value or b"").decode("ascii")
        self.header = {"HD": {"SO": self.sort_order}} if self.sort_order else {}
        self._tid = {r: i for i, r in enumerate(self.references)}
        self.filename = path

    def get_tid(self, name):
        return self._tid.get(name, -1)

    def getrname(self, tid):
        return self.references[tid]

    get_reference_name = getrname

    def set_seq_filter(self, min_ins_len):
        """coordinate mode: keep only the SEQ ranges COLLECT can read (svx_bam_set_seq_filter); pass options.min_sv_size"""
        rc = self.L.svx_bam_set_seq_filter(self.h, C.c_int(int(min_ins_len)))
        if rc != 0:
            raise self._error(rc, "svx_bam_set_seq_filter")

    def set_gpu_inflate(self, device):
        """BGZF inflate shared between the GPU (device >= 0) and the host's cores (svx_bam_set_gpu_inflate); device < 0 switches it off"""
        rc = self.L.svx_bam_set_gpu_inflate(self.h, C.c_int(int(device)))
        if rc != 0:
            raise self._error(rc, "svx_bam_set_gpu_inflate")

    def set_device_decode(self, device):
        """coordinate mode: BGZF inflate, record discovery and decode on GPU `device` (svx_bam_set_device_decode); read_batch then returns
        batches whose arrays live in HBM.  device < 0: back to the host reader"""
        rc = self.L.svx_bam_set_device_decode(self.h, C.c_int(int(device)))
        if rc != 0:
            raise self._error(rc, "svx_bam_set_device_decode")
        self.device_decode = int(device) >= 0

    def gpu_inflate_stats(self):
        g, c, ms = C.c_int64(), C.c_int64(), C.c_double()
        self.L.svx_bam_gpu_inflate_stats(self.h, C.byref(g), C.byref(c), C.byref(ms))
        return {"gpu_blocks": g.value, "cpu_blocks": c.value, "gpu_kernel_ms": ms.value}

    def seek(self, voff, last_tid=-2):
        """continue at BGZF virtual offset `voff`; records beyond reference id `last_tid` end the reading (svx_bam_seek)"""
        rc = self.L.svx_bam_seek(self.h, C.c_uint64(int(voff)), C.c_int32(int(last_tid)))
        if rc != 0:
            raise self._error(rc, "svx_bam_seek")

    def seek_region(self, voff, tid, beg, end, rule="overlap"):
        """region read (svx_bam_seek_region; svim_amd/regions.py says what it hands out): continue at virtual offset `voff` (regions.plan) and hand out the run
        of records from the first one the rule keeps on reference `tid` in [beg, end) to the last one in front of the stop; records of the run that the
        rule does not keep carry SVX_FLAG_SKIP.  rule: "overlap" (samtools view) or "start" (beg <= pos < end).  rewind() and seek() lift the bound"""
        from . import regions
        if rule not in (regions.RULE_OVERLAP, regions.RULE_START):
            raise ValueError("seek_region: rule is %r or %r" % (regions.RULE_OVERLAP, regions.RULE_START))
        rc = self.L.svx_bam_seek_region(self.h, C.c_uint64(int(voff)), C.c_int32(int(tid)), C.c_int32(int(beg)), C.c_int32(int(end)),
                                        C.c_int(_abi.REGION_RULES[rule]))
        if rc != 0:
            raise self._error(rc, "svx_bam_seek_region")

    def region_stats(self):
        """since the last seek_region: records examined in front of the stop, kept, handed out marked; bytes of the BGZF blocks loaded (svx_bam_region_stats)"""
        s = _abi.BamRegionStats()
        self.L.svx_bam_region_stats(self.h, C.byref(s))
        return s.as_dict()

    def rewind(self):
        """back to the first record; buffers, threads and interned names are kept (svx_bam_rewind)"""
        rc = self.L.svx_bam_rewind(self.h)
        if rc != 0:
            raise self._error(rc, "svx_bam_rewind")

    def index_begin(self):
        """the pass that follows builds the file's BAM index as a by-product (svx_bam_index_begin): device decode must be on and nothing read yet since open /
        rewind.  Every chunk the reader loads then appends its records to a row table on the device; seek() and rewind() raise until index_finish()
        or index_abort()"""
        rc = self.L.svx_bam_index_begin(self.h)
        if rc != 0:
            raise self._index_error(rc, "svx_bam_index_begin")

    def index_finish(self, fmt="bai"):
        """-> the bytes of the .bai (svim_amd/bai.py says what they hold), once read_batch has returned 0 records at the end of the file
        (svx_bam_index_finish).  svim_amd.bai.BaiError for a file that has no index (not in coordinate order, a record beyond 2^29): the handle stays usable.
        fmt="csi": the uncompressed bytes of the .csi (svim_amd/csi.py; svx_bam_index_finish_fmt), which has no limit at 2^29"""
        if fmt == "bai":
            rc = self.L.svx_bam_index_finish(self.h)
        else:
            rc = self.L.svx_bam_index_finish_fmt(self.h, C.c_int(_abi.index_format(fmt, "bai")))
        if rc != 0:
            raise self._index_error(rc, "svx_bam_index_finish")
        return self.index_bytes()

    def index_abort(self):
        """give up the index of a pass that will not reach the end of the file (an interrupt, a failed read): the row table is dropped, the handle stays where
        it is and seek() / rewind() work again (svx_bam_index_abort)"""
        rc = self.L.svx_bam_index_abort(self.h)
        if rc != 0:
            raise self._index_error(rc, "svx_bam_index_abort")

    def index_bytes(self):
        """the bytes of the last index_finish() (svx_bam_index_count / svx_bam_index_fetch)"""
        n = C.c_int64()
        rc = self.L.svx_bam_index_count(self.h, C.byref(n))
        if rc != 0:
            raise self._index_error(rc, "svx_bam_index_count")
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        rc = self.L.svx_bam_index_fetch(self.h, out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise self._index_error(rc, "svx_bam_index_fetch")
        return out[:n.value].tobytes()

    def index_stats(self):
        s = _abi.BamIndexStats()
        self.L.svx_bam_index_get_stats(self.h, C.byref(s))
        return s.as_dict()

    def sort_begin(self, max_bytes=0, spill_dir=None, order="coordinate"):
        """the pass that follows keeps every record on the device to put the file into coordinate order (svx_bam_sort_begin; svim_amd/bamsort.py says what the
        sorted file is): device decode must be on, nothing read yet since open / rewind and no index pass on.  max_bytes: the most the records may take on the
        device (0: what is free); the read that would pass it raises with .code SVX_E_CAPACITY, the sort is dropped and the handle rewinds.  seek() and
        rewind() raise until sort_finish() or sort_abort().
        spill_dir: a directory the process can write to (svx_bam_sort_begin_spill).  The read that would pass max_bytes (0: what is free) then closes a run -
        sorted, written to one spill file there that is unlinked as soon as it is open - and goes on; only a chunk that alone passes the limit raises.
        sort_finish() merges the runs; the file, its index and the permutation are those of the in-memory sort.  None: no spill file, the limit raises.
        order="queryname" (svx_bam_sort_begin_order): the sorted file is in query-name order, `samtools sort -N` - the input of the query-name front end.  It
        sorts in memory only (with a spill_dir: ValueError) and has no index (sort_index() raises with .code SVX_E_STATE); sort_name_stats() says what the
        rounds did"""
        which = _abi.sort_order(order)
        if which and spill_dir is not None:
            raise ValueError("sort_begin: a spilled sort is in coordinate order (order='queryname' sorts in memory only)")
        if which:
            self._out_call("begin_order", C.c_int64(int(max_bytes)), C.c_int(which))
        elif spill_dir is None:
            self._out_call("begin", C.c_int64(int(max_bytes)))
        else:
            self._out_call("begin_spill", C.c_int64(int(max_bytes)), os.fsencode(spill_dir))

    def sort_finish(self):
        """-> (records, bytes of the sorted stream, BGZF blocks of the sorted file), once read_batch has returned 0 records at the end of the file
        (svx_bam_sort_finish): the records are sorted and laid out; sort_encode() makes the file, piece by piece"""
        self._out_call("finish")
        return self.sort_count()

    def sort_count(self):
        return self._out_count()

    def sort_abort(self):
        """give the sort up at any point (svx_bam_sort_abort): the records on the device are dropped, seek() / rewind() work again"""
        self._out_call("abort")

    def sort_encode(self, first_block, n_blocks, stream=False):
        """blocks [first_block, first_block + n_blocks) of the sorted file (svx_bam_sort_encode / svx_bam_sort_fetch) -> their compressed bytes, or
        (compressed bytes, their stream bytes) with stream=True.  Ranges go in ascending order without gaps when sort_index() is to follow"""
        return self._out_encode(first_block, n_blocks, stream)

    def sort_index(self, fmt="bai"):
        """-> the bytes of the sorted file's .bai, after every block has been encoded (svx_bam_sort_index_fmt); svim_amd.bai.BaiError (E_RANGE) when a record
        ends beyond 2^29.  fmt="csi": the uncompressed bytes of its .csi, which has no such limit"""
        return self._out_index(fmt)

    def _out_index_bytes(self):
        return self.index_bytes()                           # (the sorted file's index lies where an index pass of the reader leaves its own)

    def sort_permutation(self):
        """uint32 array: the file index of every record of the sorted order (svx_bam_sort_permutation)"""
        return self._out_permutation()

    def sort_stats(self):
        return self._out_stats("get_stats", _abi.BamSortStats, checked=False)

    def sort_spill_stats(self):
        """runs, bytes written to and read from the spill file, the largest chunk, run and staging buffer, the time spent spilling, reading back and merging
        (svx_bam_sort_get_spill_stats); after a sort that spilled nothing: n_runs 1 (0 without records), spilled_bytes 0"""
        return self._out_stats("get_spill_stats", _abi.BamSortSpillStats, checked=False)

    def sort_name_stats(self):
        """the permutation of a query-name sort (svx_bam_sort_get_name_stats): rounds, the rows that took part in each ("active_rows"), their sum and maximum,
        the times of the name pass, the rank pass, the rounds and the layout; zeros after a coordinate sort"""
        return self._out_stats("get_name_stats", _abi.BamNameSortStats, checked=False)

    def sam_stats(self):
        """what the SAM text front end has done for this handle (svx_sam_get_stats); zeros for a BAM file"""
        s = _abi.SamStats()
        self.L.svx_sam_get_stats(self.h, C.byref(s))
        return s.as_dict()

    def _out_error(self, rc, what):
        from . import bamsort
        return bamsort.BamSortError(rc, "%s failed: %s (%s)" % (what, _abi.ERRORS.get(rc, rc), self.L.svx_last_error().decode("utf-8", "replace")))

    def _error(self, rc, what):
        """the SvxError of a call that returned status rc, the status in its `.code`"""
        e = SvxError("%s failed: %s" % (what, self.L.svx_last_error().decode("utf-8", "replace")))
        e.code = rc
        return e

    def _index_error(self, rc, what):
        from . import bai
        if rc in (_abi.SVX_E_ORDER, _abi.SVX_E_RANGE):
            return bai.BaiError(rc, "%s failed: %s (%s)" % (what, _abi.ERRORS.get(rc, rc), self.L.svx_last_error().decode("utf-8", "replace")))
        return self._error(rc, what)

    def read_batch(self, max_records, min_mapq, mode="coordinate"):
        """-> (svx_batch struct with host pointers owned by the reader, n_records); n_records == 0 at EOF."""
        b = _abi.Batch()
        n = C.c_int64()
        rc = self.L.svx_bam_read_batch(self.h, C.c_int64(max_records), C.c_int(0 if mode == "coordinate" else 1), C.c_int(min_mapq),
                                       C.byref(b), C.byref(n))
        if rc != 0:
            raise self._error(rc, "svx_bam_read_batch")
        return b, n.value

    def batch_arrays(self, b):
        """numpy copies of a batch returned by read_batch (tests / inspection)."""
        n, ns = b.n_rec, b.n_seg
        if b.on_device:
            return self._device_batch_arrays(b)

        def arr(ptr, count, dt):
            if count == 0:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,)).view(dt).copy()
        A = {}
        for k in ("flag", "tid", "pos", "mapq", "lseq", "read_id", "order", "seg_order"):
            A[k] = arr(getattr(b, k), n, _abi.BATCH_DTYPES[k])
        A["cigar_off"] = arr(b.cigar_off, n + 1, np.uint64)
        A["cigar"] = arr(b.cigar, int(A["cigar_off"][-1]) if n else 0, np.uint32)
        A["seq_off"] = arr(b.seq_off, n + 1, np.uint64)
        A["seq"] = arr(b.seq, int(A["seq_off"][-1]) if n else 0, np.uint8)
        A["seg_off"] = arr(b.seg_off, n + 1, np.uint32)
        for k in ("seg_tid", "seg_pos", "seg_rev", "seg_mapq", "seg_lseq"):
            A[k] = arr(getattr(b, k), ns, _abi.BATCH_DTYPES[k])
        A["seg_cigar_off"] = arr(b.seg_cigar_off, ns + 1, np.uint64)
        A["seg_cigar"] = arr(b.seg_cigar, int(A["seg_cigar_off"][-1]) if ns else 0, np.uint32)
        A["contig_rank"] = arr(b.contig_rank, b.n_contig, np.int32)
        if b.seq_rng_off:
            nr = int(b.n_seq_rng)
            A["seq_rng_off"] = arr(b.seq_rng_off, n + 1, np.uint32)
            A["seq_rng_q0"], A["seq_rng_len"] = arr(b.seq_rng_q0, nr, np.int32), arr(b.seq_rng_len, nr, np.int32)
            A["seq_rng_byte"] = arr(b.seq_rng_byte, nr, np.uint64)
        return A

    def _device_batch_arrays(self, b):
        """a device-resident batch (svx_bam_set_device_decode) copied to the host in the layout of a host batch: offsets rebased to the batch, one
        packed SEQ per record (the device batch points into the inflated stream instead)"""
        n, ns = int(b.n_rec), int(b.n_seg)

        def arr(ptr, count, dt, skip=0):
            out = np.zeros(count, dtype=dt)
            if count:
                base = C.cast(ptr, C.c_void_p).value
                src = C.c_void_p(base + skip * np.dtype(dt).itemsize)
                if self.L.svx_memcpy_d2h(out.ctypes.data_as(C.c_void_p), src, C.c_uint64(out.nbytes)) != 0:
                    raise SvxError("svx_memcpy_d2h of %d x %s from %#x + %d elements failed: %s" % (count, np.dtype(dt).name, base or 0, skip, self.L.svx_last_error().decode()))
            return out
        A = {}
        for k in ("flag", "tid", "pos", "mapq", "lseq", "read_id", "order", "seg_order"):
            A[k] = arr(getattr(b, k), n, _abi.BATCH_DTYPES[k])
        co = arr(b.cigar_off, n + 1, np.uint64)
        A["cigar"] = arr(b.cigar, int(co[-1] - co[0]) if n else 0, np.uint32, skip=int(co[0]) if n else 0)
        A["cigar_off"] = (co - co[0]).astype(np.uint64) if n else np.zeros(1, np.uint64)
        so = arr(b.seq_off, n + 1, np.uint64)
        nb = (A["lseq"].astype(np.int64) + 1) // 2
        parts = []
        if n:
            lo, hi = int(so[0]), int(so[n - 1] + nb[n - 1])
            raw = arr(b.seq, hi - lo, np.uint8, skip=lo)
            parts = [raw[int(so[i]) - lo:int(so[i]) - lo + int(nb[i])] for i in range(n)]
        A["seq"] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        A["seq_off"] = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
        sg = arr(b.seg_off, n + 1, np.uint32)
        s0, s1 = (int(sg[0]), int(sg[-1])) if n else (0, 0)
        A["seg_off"] = (sg - sg[0]).astype(np.uint32) if n else np.zeros(1, np.uint32)
        for k in ("seg_tid", "seg_pos", "seg_rev", "seg_mapq", "seg_lseq"):
            A[k] = arr(getattr(b, k), s1 - s0, _abi.BATCH_DTYPES[k], skip=s0)
        sc = arr(b.seg_cigar_off, s1 - s0 + 1, np.uint64, skip=s0) if ns else np.zeros(1, np.uint64)
        A["seg_cigar"] = arr(b.seg_cigar, int(sc[-1] - sc[0]), np.uint32, skip=int(sc[0]))
        A["seg_cigar_off"] = (sc - sc[0]).astype(np.uint64)
        A["contig_rank"] = arr(b.contig_rank, b.n_contig, np.int32)
        return A

    def read_names(self):
        n, blob, ln = C.c_int64(), C.c_void_p(), C.c_int64()
        self.L.svx_bam_read_names(self.h, C.byref(n), C.byref(blob), C.byref(ln))
        if n.value == 0:
            return []
        raw = C.string_at(blob, ln.value)
        return raw[:-1].decode("ascii").split("\0")

    def close(self):
        if self.h:
            self.L.svx_bam_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamMerge(_SortedOutput):
    """A merge session on the device (svx_bam_merge_*; svim_amd/bammerge.py says what the merged file is): several files, in the order given, into one file in
    coordinate order, or with order="queryname" in query-name order (no index then; with a spill_dir the runs are sorted by name and merged from a table of
    their names that stays on the device: a session over one file is the spilled query-name sort of that file).  The session owns its sort, its stream and
    its index; readers only feed it.
        m = BamMerge.open(readers, device=0)     # reads headers and dictionaries; keeps nothing of the readers, which may be closed at once
        for r in readers: m.add(r)               # file by file, in the order of open: the call reads the whole file and returns when the reader is idle again
        n_records, n_bytes, n_blocks = m.finish()
        m.encode(first_block, n_blocks) ...; m.index("bai"); m.permutation(); m.stats(); m.close()
    What the definition refuses - header clashes at open, records at finish - and the state rules are svim_amd.bammerge.BamMergeError with the library's status
    in .code; an add that fails (SVX_E_CAPACITY, SVX_E_IO) breaks the session: close() is all that is left, the reader works again after rewind()."""
    _out_prefix = "svx_bam_merge_"

    def __init__(self, handle, L):
        self.h, self.L = handle, L

    @classmethod
    def open(cls, readers, device=0, max_bytes=0, spill_dir=None, order="coordinate"):
        L = lib()
        readers = list(readers)
        if not readers:
            raise ValueError("BamMerge.open: no reader")
        arr = (C.c_void_p * len(readers))(*[r.h for r in readers])
        h = C.c_void_p()
        rc = L.svx_bam_merge_open_order(arr, C.c_int64(len(readers)), C.c_int(int(device)), C.c_int64(int(max_bytes)), None if spill_dir is None else os.fsencode(spill_dir),
                                        C.c_int(_abi.sort_order(order)), C.byref(h))
        if rc != 0:
            raise cls._error_of(L, rc, "svx_bam_merge_open")
        return cls(h, L)

    @staticmethod
    def _error_of(L, rc, what):
        from . import bammerge
        return bammerge.BamMergeError(rc, "%s failed: %s (%s)" % (what, _abi.ERRORS.get(rc, rc), L.svx_last_error().decode("utf-8", "replace")))

    def _out_error(self, rc, what):
        return self._error_of(self.L, rc, what)

    def _out_open(self, what):
        if not self.h:
            raise self._error_of(self.L, _abi.SVX_E_STATE, what + " on a closed session")

    def add(self, reader):
        """the next file of the session: `reader` (a NativeBam with device decode on, at its first record) is read to its end inside this call"""
        self._out_call("add", reader.h)

    def finish(self):
        """-> (records, bytes of the merged stream, BGZF blocks of the merged file), once every file has been added"""
        self._out_call("finish")
        return self.count()

    def count(self):
        return self._out_count()

    def encode(self, first_block, n_blocks, stream=False):
        """blocks [first_block, first_block + n_blocks) of the merged file -> their compressed bytes, or (compressed bytes, stream bytes) with stream=True;
        ascending ranges without gaps when index() is to follow"""
        return self._out_encode(first_block, n_blocks, stream)

    def index(self, fmt="bai"):
        """-> the bytes of the merged file's .bai, or with fmt="csi" the uncompressed bytes of its .csi, after every block has been encoded; svim_amd.bai.BaiError
        (E_RANGE) when a record ends beyond 2^29 of a .bai.  A session in query-name order has no index: BamMergeError with .code SVX_E_STATE"""
        return self._out_index(fmt)

    def name_stats(self):
        """the permutation of a session in query-name order (svx_bam_merge_get_name_stats: NativeBam.sort_name_stats for the session; after a finish over
        closed runs the merge's rounds), and under "spill" the runs closed in that order (svx_bam_merge_get_name_spill_stats): their number, rounds and
        active rows summed over the runs' sorts, the name table's bytes, the times of the runs' name sorts and of the table's packing"""
        d = self._out_stats("get_name_stats", _abi.BamNameSortStats)
        d["spill"] = self._out_stats("get_name_spill_stats", _abi.BamNameSpillStats)
        return d

    def permutation(self):
        """uint32 array: for every record of the merged order its place in the concatenation of the files"""
        return self._out_permutation()

    def stats(self):
        """the sort's stats (svx_bam_sort_stats), the spill's under "spill", the session's own under "merge" """
        d = self._out_stats("get_stats", _abi.BamSortStats)
        d["spill"], d["merge"] = self._out_stats("get_spill_stats", _abi.BamSortSpillStats), self._out_stats("get_merge_stats", _abi.BamMergeStats)
        return d

    def close(self):
        if self.h:
            self.L.svx_bam_merge_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
