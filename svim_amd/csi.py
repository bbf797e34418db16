"""The CSI index (.csi) of a coordinate-sorted BAM file or of a BGZF-compressed VCF or BED text: the definition the device builds (csrc/bamindex.hip,
csrc/textindex.hip with SVX_INDEX_CSI) and the host builds (svx_bam_index_csi_host, svx_text_index_csi_host) are held against, a parser of the index, and
region queries that use it.  Pure Python, no GPU, no library.  A .csi is what a .bai / .tbi is, without the limit at 2^29: contigs of any length.

What an index says (the uncompressed bytes; the .csi file is these bytes BGZF-framed, as a .tbi is):
  rows, interval, order, virtual offsets, chunks
                 exactly those of bai.py (BAM) and tabix.py (text): this module imports them.  The chunks of a bin are the maximal runs, in file order, of
                 rows with the same (group, bin); a group is a reference of a BAM, a contig run of a text.
  min_shift      14, fixed: 16 kb leaves.
  depth          the smallest d >= 5 with max_end <= 2^(14 + 3 d), max_end the largest interval end over all rows of the file that get bytes (no rows: 5).
                 A BAM (int32 pos, a 32-bit span) never needs more than 7, the text parser's cap of 2^40 plus len(REF) never more than 9.  So no file is
                 E_RANGE in this format; E_ORDER stays what it is.  The depth stops at 9: a row of a hand-made table that ends beyond 2^41 gets bin 0.
  bins           reg2bin(beg, end, 14, depth), the CSI specification's general form (at depth 5: tabix.reg2bin).  The largest bin at depth 6 is 299 592, at
                 depth 9 153 391 688.
  loffset        of a bin: the value the FILLED linear index of bai.py / tabix.py (contig_part) would hold at the window bin_start(bin) >> 14 - the smallest
                 vbeg of the rows that overlap that 16 kb window, or the next window's that has one (htslib's rule).  The same value without a linear index
                 (loffset_by_running_max; tested against the first form): the vbeg of the first row j of the group, in file order, whose running maximum of
                 ends max(end_0 .. end_j) exceeds bin_start(bin).  The begs of a group do not decrease, so the first row that reaches beyond bin_start is
                 the first that overlaps the window or a later one.  This is what the kernels use: a 2^40 coordinate would mean a 512 MB linear index.
  bytes          header: "CSI\\1", min_shift i32, depth i32, l_aux i32, aux, n_ref i32.  Per group: n_bin i32, then per bin (ascending) bin u32, loffset u64,
                 n_chunk i32 and the chunks (vbeg u64, vend u64).  The pseudo-bin ((1 << (3 depth + 3)) - 1) / 7 + 1 comes last, has loffset 0 and the two
                 pairs of bai.py / tabix.py.  A group without rows is n_bin = 0 alone.  Trailer: n_no_coor u64, always written.
                 BAM: l_aux = 0.  Text: aux = the seven int32 of the .tbi header (format, col_seq, col_beg, col_end, meta, skip, l_nm) and the names.
  query          candidate bins from reg2bins at the file's depth; the lower bound is the largest loffset among the bins that exist on the chain from the leaf
                 bin of beg up through its ancestors (each is a valid bound: every ancestor starts at or before beg); chunks that end at or below it are dropped.
Byte equality with the .csi htslib writes is not claimed (it merges chunks and compacts bins, see bai.py); every reader of the format reads this one."""
import struct
import zlib

from . import bai, tabix
from .bai import brute_force      # noqa: F401 (re-exported)

MIN_SHIFT = 14
MIN_DEPTH, MAX_DEPTH = 5, 9
E_ORDER = -9
_EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def depth_for(max_end):
    """the depth of a file whose largest end is max_end.  It stops at MAX_DEPTH, as binidx_depth_for does: no reader of this project makes a row beyond 2^41
    (a row table handed to the host build could hold one: it lands in bin 0, here and there)"""
    d = MIN_DEPTH
    while d < MAX_DEPTH and max_end > 1 << (MIN_SHIFT + 3 * d):
        d += 1
    return d


def reg2bin(beg, end, min_shift=MIN_SHIFT, depth=MIN_DEPTH):
    end -= 1
    level, s, t = depth, min_shift, ((1 << (3 * depth)) - 1) // 7
    while level > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        level -= 1
        s += 3
        t -= 1 << (3 * level)
    return 0


def reg2bins(beg, end, min_shift=MIN_SHIFT, depth=MIN_DEPTH):
    """every bin whose rows can overlap [beg, end)"""
    end = min(end, 1 << (min_shift + 3 * depth)) - 1
    beg = max(0, min(beg, end))
    bins, t = [], 0
    for level in range(depth + 1):
        s = min_shift + 3 * (depth - level)
        bins.extend(range(t + (beg >> s), t + (end >> s) + 1))
        t += 1 << (3 * level)
    return bins


def bin_level(b, depth):
    """(level of the bin, first bin of that level)"""
    level, first = 0, 0
    while level < depth and b >= first + (1 << (3 * level)):
        first += 1 << (3 * level)
        level += 1
    return level, first


def bin_start(b, depth, min_shift=MIN_SHIFT):
    """the first coordinate the bin covers"""
    level, first = bin_level(b, depth)
    return (b - first) << (min_shift + 3 * (depth - level))


def bin_parent(b):
    return (b - 1) >> 3


def pseudo_bin(depth):
    return ((1 << (3 * depth + 3)) - 1) // 7 + 1


def loffset_by_linear(rows, start):
    """rows (beg, end, vbeg, vend) of one group -> the filled linear index's value at window start >> 14, by the linear index of tabix.contig_part"""
    part = tabix.contig_part(rows, len(rows), 0)
    _, _, lin, _ = tabix.parse_part(part, 0, "part")
    return lin[start >> MIN_SHIFT]


def loffset_by_running_max(rows, start):
    """the same value without a linear index: the vbeg of the first row whose running maximum of ends exceeds `start`"""
    top = 0
    for _beg, end, vbeg, _vend in rows:
        top = max(top, end)
        if top > start:
            return vbeg
    raise ValueError("no row of the group ends beyond %d" % start)


def group_part(rows, n_mapped, n_unmapped, depth):
    """the bytes of the part of one group from its rows (beg, end, vbeg, vend), in file order and at least one"""
    bins, prev = {}, None
    for beg, end, vbeg, vend in rows:
        b = reg2bin(beg, end, MIN_SHIFT, depth)
        if b == prev:
            bins[b][-1][1] = vend
        else:
            bins.setdefault(b, []).append([vbeg, vend])
        prev = b
    # the loffsets of all bins in one walk over the rows: the bins by ascending start, the running maximum moving forward
    loff, top, j = {}, 0, -1
    for start, b in sorted((bin_start(b, depth), b) for b in bins):
        while top <= start:
            j += 1
            top = max(top, rows[j][1])
        loff[b] = rows[max(j, 0)][2]
    out = [struct.pack("<i", len(bins) + 1)]
    for b in sorted(bins):
        out.append(struct.pack("<IQi", b, loff[b], len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
    out.append(struct.pack("<IQiQQQQ", pseudo_bin(depth), 0, 2, rows[0][2], rows[-1][3], n_mapped, n_unmapped))
    return b"".join(out)


def build_bam_index(n_ref, rows, v_end):
    """the uncompressed bytes of the .csi of a BAM file with n_ref references whose records are `rows` (tid, pos, end, flag, vbeg: bai.rows_of_bam) and whose
    data ends at virtual offset v_end.  bai.BaiError (E_ORDER) when it has none; ValueError for a tid outside the references"""
    if any(r[0] >= n_ref for r in rows):
        raise ValueError("a record names a reference the header does not have")
    if bai.check_order(rows) == E_ORDER:
        raise bai.BaiError(E_ORDER, "records out of order")
    vend = [r[4] for r in rows[1:]] + [v_end]
    per = [[] for _ in range(n_ref)]
    max_end = 0
    for k, r in enumerate(rows):
        if r[0] >= 0:
            iv = bai.interval(r)
            per[r[0]].append((iv, r[3], r[4], vend[k]))
            max_end = max(max_end, iv[1])
    depth = depth_for(max_end)
    out = [b"CSI\1", struct.pack("<iiii", MIN_SHIFT, depth, 0, n_ref)]
    for rs in per:
        if not rs:
            out.append(struct.pack("<i", 0))
            continue
        n_unmapped = sum(1 for r in rs if r[1] & 4)
        out.append(group_part([r[0] + r[2:] for r in rs], len(rs) - n_unmapped, n_unmapped, depth))
    out.append(struct.pack("<Q", sum(1 for r in rows if r[0] < 0)))
    return b"".join(out)


def build_text_index(text, block_coff, block_uoff, preset, stream_base=0):
    """the uncompressed .csi bytes of `text`; arguments of tabix.build_index.  tabix.TabixError (E_ORDER) when it has none."""
    recs = tabix.records(bytes(text), block_coff, block_uoff, preset, stream_base)
    if tabix.check_order(recs) == E_ORDER:
        raise tabix.TabixError(E_ORDER, "records out of order")
    contigs = []
    for r in recs:
        if not contigs or contigs[-1][0] != r[0]:
            contigs.append([r[0], []])
        contigs[-1][1].append(r)
    depth = depth_for(max([r[2] for r in recs] or [0]))
    names = b"".join(c[0] + b"\0" for c in contigs)
    aux = struct.pack("<7i", *tabix._FORMAT[preset], ord("#"), 0, len(names)) + names
    out = [b"CSI\1", struct.pack("<iii", MIN_SHIFT, depth, len(aux)), aux, struct.pack("<i", len(contigs))]
    for _, rs in contigs:
        out.append(group_part([r[1:5] for r in rs], len(rs), 0, depth))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def parse_index(data):
    """uncompressed .csi bytes -> dict(min_shift, depth, aux, n_ref, bins: per group {bin: [(beg, end)]}, loffset: per group {bin: loffset}, pseudo: per group
    the two pairs of the pseudo-bin or None, n_no_coor; for a text also format, col_seq, col_beg, col_end, meta, skip, names); ValueError for bytes that are
    not one index exactly"""
    data = bytes(data)
    if data[:4] != b"CSI\1":
        raise ValueError("not a CSI index")
    try:
        return _parse(data)
    except struct.error:
        raise ValueError("CSI index: truncated")


def _parse(data):
    min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
    if min_shift != MIN_SHIFT or not MIN_DEPTH <= depth <= MAX_DEPTH or l_aux < 0 or 16 + l_aux + 4 > len(data):
        raise ValueError("CSI index: header out of range")
    aux = data[16:16 + l_aux]
    ix = dict(min_shift=min_shift, depth=depth, aux=aux)
    if l_aux:
        fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<7i", aux, 0)
        names = aux[28:28 + l_nm].split(b"\0")[:-1] if l_nm else []
        if 28 + l_nm != l_aux or (l_nm and aux[-1:] != b"\0"):
            raise ValueError("CSI index: aux is not a tabix header")
        ix.update(format=fmt, col_seq=cs, col_beg=cb, col_end=ce, meta=meta, skip=skip, names=names)
    at = 16 + l_aux
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    if l_aux and len(ix["names"]) != n_ref:
        raise ValueError("CSI index: the names do not match n_ref")
    bins, loffset, pseudo, ps_bin = [], [], [], pseudo_bin(depth)
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, at)
        at += 4
        d, lo, order, ps = {}, {}, [], None
        for _ in range(n_bin):
            b, loff, n_chunk = struct.unpack_from("<IQi", data, at)
            at += 16
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == ps_bin:
                ps = chunks
                if loff != 0 or n_chunk != 2:
                    raise ValueError("CSI index: bad pseudo-bin")
            else:
                d[b], lo[b] = chunks, loff
            order.append(b)
        if order != sorted(order) or len(set(order)) != len(order) or (ps is None) != (n_bin == 0) or (order and order[-1] != ps_bin):
            raise ValueError("CSI index: bins not ascending, or no pseudo-bin")
        bins.append(d), loffset.append(lo), pseudo.append(ps)
    n_no_coor, = struct.unpack_from("<Q", data, at)
    if at + 8 != len(data):
        raise ValueError("CSI index: %d bytes behind the trailer" % (len(data) - at - 8))
    ix.update(n_ref=n_ref, bins=bins, loffset=loffset, pseudo=pseudo, n_no_coor=n_no_coor)
    return ix


def lower_bound(ix, tid, beg):
    """the largest loffset among the bins that exist on the chain from the leaf bin of beg up through its ancestors (0 when none exists)"""
    depth = ix["depth"]
    beg = max(beg, 0)
    if beg >= 1 << (MIN_SHIFT + 3 * depth):
        return None
    b, low = reg2bin(beg, beg + 1, MIN_SHIFT, depth), 0
    while True:
        low = max(low, ix["loffset"][tid].get(b, 0))
        if b == 0:
            return low
        b = bin_parent(b)


def candidate_bins(ix, tid, beg, end):
    """the bins of reg2bins(beg, end) at the index's depth that group `tid` has"""
    have, depth = ix["bins"][tid], ix["depth"]
    hi = min(end, 1 << (MIN_SHIFT + 3 * depth)) - 1
    lo = max(0, min(beg, hi))
    if sum((hi >> (MIN_SHIFT + 3 * k)) - (lo >> (MIN_SHIFT + 3 * k)) + 1 for k in range(depth + 1)) <= len(have):
        return [b for b in reg2bins(beg, end, MIN_SHIFT, depth) if b in have]
    # a wide region in a deep index names millions of bins: ask the bins the group has instead - the same set
    return [b for b in have if bin_start(b, depth) <= hi and bin_start(b, depth) + (1 << (MIN_SHIFT + 3 * (depth - bin_level(b, depth)[0]))) > lo]


def _merged(ix, tid, beg, end):
    low = lower_bound(ix, tid, beg)
    if low is None:
        return [], None
    merged, have = [], ix["bins"][tid]
    cand = candidate_bins(ix, tid, beg, end)
    for c in sorted(c for b in cand for c in have.get(b, ()) if c[1] > low):
        if merged and c[0] <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append(list(c))
    return [tuple(c) for c in merged], low


def query(index, tid, beg, end):
    """BAM -> (chunks, lower bound): the merged chunks (vbeg, vend), ascending, that hold every record of reference `tid` overlapping [beg, end).
    ([], None) when the index shows that nothing overlaps.  index: parse_index's dict or the uncompressed bytes"""
    ix = index if isinstance(index, dict) else parse_index(index)
    if not 0 <= tid < ix["n_ref"] or end <= beg or end <= 0:
        return [], None
    return _merged(ix, tid, beg, end)


def query_text(index, bgzf, contig, beg, end, stats=None):
    """the lines (bytes, without newline) of the records of `contig` that overlap [beg, end), in file order, as tabix.query gives them.  index: parse_index's
    dict or the uncompressed bytes; bgzf: the bytes of the whole .gz file"""
    ix = index if isinstance(index, dict) else parse_index(index)
    name = contig.encode("utf-8") if isinstance(contig, str) else bytes(contig)
    if name not in ix["names"] or end <= beg or end <= 0:
        return []
    tid = ix["names"].index(name)
    merged, _ = _merged(ix, tid, beg, end)
    return tabix.read_chunks(merged, bgzf, tabix.BED if ix["format"] & 0x10000 else tabix.VCF, name, beg, end, stats)


def frame(data):
    """the bytes of the .csi file: the index BGZF-framed (stored through zlib, 65 280 bytes per block, and the end-of-file block)"""
    data, out = bytes(data), []
    for at in range(0, len(data), 65280):
        piece = data[at:at + 65280]
        comp = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = comp.compress(piece) + comp.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out) + _EOF_BLOCK


def unframe(data):
    """the bytes of a .csi file -> the uncompressed index"""
    return b"".join(b[2] for b in bai.bgzf_blocks(bytes(data)))


def read_file(path):
    """the uncompressed bytes of the .csi at `path`"""
    with open(path, "rb") as fh:
        return unframe(fh.read())
