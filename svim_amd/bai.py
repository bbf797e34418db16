"""The BAM index (.bai) of a coordinate-sorted BAM file: the definition the device build (csrc/bamindex.hip, fed by the device reader's record stream) and
the host build (csrc/bamindex_host.cpp) are held against, a parser of the index, and a region query that uses it.  Pure Python, no GPU, no library.

What an index says (a .bai is not BGZF-framed: these are the bytes of the file):
  rows           one per record of the file, in file order: (tid, pos, end, flag, vbeg).  EVERY record counts - secondary, supplementary, unmapped, duplicate,
                 any mapping quality: an index describes the file, not COLLECT's filters.
  interval       of a placed record (tid >= 0), 0-based, half-open: beg = pos (a negative pos is read as 0), end = beg + the summed lengths of the M D N = X
                 operations of its CIGAR.  Where the placeholder rule applies (a placed record whose first operation is a soft clip of l_seq bases and whose
                 first aux field named CG is a B,I / B,i array at least as long as the CIGAR field: htslib's kSmN for more than 65 535 operations) the
                 operations are those of the CG tag, as both readers have it.  The sum is taken in 32 bits, as the alignment table's is.  A record with flag
                 bit 4 set, or with a reference length of 0, has end = beg + 1.
  order          tid does not decrease, pos does not decrease inside a tid, every unplaced record (tid < 0) lies behind every placed one; otherwise E_ORDER.
                 An end beyond 2^29 is E_RANGE (a file with both is E_ORDER, as in tabix.py).
  virtual offset of inflated offset u: (coff[b] << 16) | (u - uoff[b]), b the last block that starts at or before u (tabix.py with stream_base = 0): a record
                 that starts where a block's data ends belongs to the next block at offset 0, and an empty block never holds one.  A record's vbeg is that
                 of the first byte of its block_size field, its vend the vbeg of the next record; the last record's vend is v_end: the file offset of the
                 block behind the last data byte, shifted left by 16.
  bins           reg2bin of the five-level scheme (16 kb leaves, 37 449 bins).  The chunks of a bin are the maximal runs, in file order, of records with the
                 same (tid, bin): (vbeg of the first, vend of the last).  htslib's later merging of bins and chunks is not reproduced.
  pseudo-bin     37450, last per reference: (vbeg of the reference's first record, vend of its last), (records without flag bit 4, records with it).
  linear index   1 + max((end - 1) >> 14) slots; a slot is the smallest vbeg of the records that overlap its 16 kb window, an empty slot takes the value of
                 the next one that is not.
  no records     a reference without records has n_bin = 0 and n_intv = 0.
  trailer        the uint64 count of unplaced records, always written.
Byte equality with the .bai samtools writes is not claimed (htslib merges chunks and bins); every reader of the format reads this one, records.read_bai
included."""
import bisect
import struct
import zlib

from .tabix import MAX_END, PSEUDO_BIN, contig_part, parse_part, reg2bin, reg2bins      # noqa: F401 (PSEUDO_BIN and reg2bin stay names of this module)

E_ORDER, E_RANGE = -9, -10
_REF_OPS = (0, 2, 3, 7, 8)


class BaiError(ValueError):
    """the file cannot be indexed: code E_ORDER (not in coordinate order) or E_RANGE (a record ends beyond 2^29)"""

    def __init__(self, code, msg):
        ValueError.__init__(self, msg)
        self.code = code


def bgzf_blocks(data):
    """every BGZF block of the file -> list of (file offset, size in the file, inflated bytes)"""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 18 or data[at:at + 3] != b"\x1f\x8b\x08" or not data[at + 3] & 4:
            raise ValueError("not a BGZF block at %d" % at)
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        p, bsize = at + 12, None
        while p + 4 <= at + 12 + xlen:
            slen = struct.unpack_from("<H", data, p + 2)[0]
            if data[p:p + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", data, p + 4)[0]
            p += 4 + slen
        if bsize is None or at + bsize + 1 > len(data):
            raise ValueError("truncated BGZF block at %d" % at)
        out.append((at, bsize + 1, zlib.decompress(data[at + 12 + xlen:at + bsize + 1 - 8], -15)))
        at += bsize + 1
    return out


def _cg_cigar(rec, at, end, n_cig):
    """the array of the first aux field named CG when it is B,I / B,i, non-empty and at least n_cig long -> (offset of its words, count), else None"""
    sizes = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
    while at + 3 <= end:
        tag, ty = rec[at:at + 2], rec[at + 2:at + 3]
        at += 3
        if ty in sizes:
            size = sizes[ty]
        elif ty in (b"Z", b"H"):
            size = rec.index(b"\0", at, end) - at + 1
        elif ty == b"B":
            sub, count = rec[at:at + 1], struct.unpack_from("<I", rec, at + 1)[0]
            size = 5 + count * sizes.get(sub, 4)
            if tag == b"CG":
                return (at + 5, count) if at + size <= end and sub in (b"I", b"i") and 0 < count < (1 << 29) and count >= n_cig else None
        else:
            raise ValueError("malformed BAM aux field")
        if tag == b"CG":
            return None
        at += size
    return None


def record_row(rec, vbeg):
    """rec: the bytes of one record behind its block_size field -> (tid, pos, end, flag, vbeg)"""
    tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
    if tid < 0:
        return (tid, pos, pos + 1, flag, vbeg)
    cig_at, count = 32 + l_name, n_cig
    if n_cig >= 1 and pos >= 0:
        first = struct.unpack_from("<I", rec, cig_at)[0]
        if first & 15 == 4 and first >> 4 == l_seq:
            cg = _cg_cigar(rec, cig_at + 4 * n_cig + (l_seq + 1) // 2 + l_seq, len(rec), n_cig)
            if cg:
                cig_at, count = cg
    span = sum(w >> 4 for w in struct.unpack_from("<%dI" % count, rec, cig_at) if w & 15 in _REF_OPS) & 0xffffffff
    beg = max(pos, 0)
    return (tid, pos, beg + 1 if flag & 4 or span == 0 else beg + span, flag, vbeg)


def rows_of_bam(path):
    """-> (n_ref of the header, rows, v_end): a row (tid, pos, end, flag, vbeg) for every record of the file, in file order"""
    with open(path, "rb") as fh:
        blocks = bgzf_blocks(fh.read())
    raw = b"".join(b[2] for b in blocks)
    coff, uoff, u, v_end = [], [], 0, 0
    for at, size, payload in blocks:
        coff.append(at), uoff.append(u)
        u += len(payload)
        if payload:
            v_end = (at + size) << 16
    if raw[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    rows = []
    while p < len(raw):
        size = struct.unpack_from("<i", raw, p)[0]
        if size < 32 or p + 4 + size > len(raw):
            raise ValueError("truncated BAM record")
        b = bisect.bisect_right(uoff, p) - 1
        rows.append(record_row(raw[p + 4:p + 4 + size], (coff[b] << 16) | (p - uoff[b])))
        p += 4 + size
    return n_ref, rows, v_end


def interval(row):
    """(beg, end) of a row as the index takes it: an end that is not beyond beg is read as beg + 1"""
    beg = max(row[1], 0)
    return beg, (row[2] if row[2] > beg else beg + 1)


def check_order(rows):
    """0, E_ORDER or E_RANGE for the rows of one file"""
    status, prev = 0, None
    for r in rows:
        if prev is not None and (prev[0] < 0 <= r[0] or (prev[0] >= 0 and r[0] >= 0 and (r[0] < prev[0] or (r[0] == prev[0] and r[1] < prev[1])))):
            return E_ORDER
        if r[0] >= 0 and interval(r)[1] > MAX_END:
            status = E_RANGE
        prev = r
    return status


def build_index(n_ref, rows, v_end):
    """the bytes of the .bai of a file with n_ref references whose records are `rows` and whose data ends at virtual offset v_end.  BaiError when it has none;
    ValueError for a tid outside the references"""
    if any(r[0] >= n_ref for r in rows):
        raise ValueError("a record names a reference the header does not have")
    status = check_order(rows)
    if status:
        raise BaiError(status, "records out of order" if status == E_ORDER else "a record ends beyond 2^29")
    vend = [r[4] for r in rows[1:]] + [v_end]
    per = [[] for _ in range(n_ref)]
    for k, r in enumerate(rows):
        if r[0] >= 0:
            per[r[0]].append((interval(r), r[3], r[4], vend[k]))
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for rs in per:
        if not rs:
            out.append(struct.pack("<ii", 0, 0))
            continue
        n_unmapped = sum(1 for r in rs if r[1] & 4)
        out.append(contig_part([r[0] + r[2:] for r in rs], len(rs) - n_unmapped, n_unmapped))
    out.append(struct.pack("<Q", sum(1 for r in rows if r[0] < 0)))
    return b"".join(out)


def parse_index(data):
    """.bai bytes -> dict(n_ref, bins: per reference {bin: [(beg, end)]}, pseudo: per reference the two pairs of bin 37450 or None, linear: per reference list,
    n_no_coor); ValueError for bytes that are not one index exactly"""
    data = bytes(data)
    if data[:4] != b"BAI\1":
        raise ValueError("not a BAM index")
    try:
        return _parse(data)
    except struct.error:
        raise ValueError("BAM index: truncated")


def _parse(data):
    n_ref, = struct.unpack_from("<i", data, 4)
    at, bins, pseudo, linear = 8, [], [], []
    for _ in range(n_ref):
        d, ps, lin, at = parse_part(data, at, "BAM index", may_be_empty=True)
        bins.append(d), pseudo.append(ps), linear.append(lin)
    n_no_coor, = struct.unpack_from("<Q", data, at)
    if at + 8 != len(data):
        raise ValueError("BAM index: %d bytes behind the trailer" % (len(data) - at - 8))
    return dict(n_ref=n_ref, bins=bins, pseudo=pseudo, linear=linear, n_no_coor=n_no_coor)


def query(index, tid, beg, end):
    """-> (chunks, linear_min): the merged chunks (vbeg, vend), ascending, that hold every record of reference `tid` overlapping [beg, end), and the linear
    index's lower bound for the region's first window.  ([], None) when the index shows that nothing overlaps.  index: parse_index's dict or the bytes"""
    ix = index if isinstance(index, dict) else parse_index(index)
    if not 0 <= tid < ix["n_ref"] or end <= beg or end <= 0:
        return [], None
    lin = ix["linear"][tid]
    if (max(beg, 0) >> 14) >= len(lin):
        return [], None
    low = lin[max(beg, 0) >> 14]
    merged = []
    for c in sorted(c for b in reg2bins(beg, end) for c in ix["bins"][tid].get(b, ()) if c[1] > low):
        if merged and c[0] <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append(list(c))
    return [tuple(c) for c in merged], low


def brute_force(rows, tid, beg, end):
    """the rows query() must cover, by a scan over every row: those of reference `tid` whose interval overlaps [beg, end)"""
    return [r for r in rows if r[0] == tid and tid >= 0 and end > beg and interval(r)[0] < end and interval(r)[1] > beg]
