"""The tabix index (.tbi) of a BGZF-compressed VCF or BED text: the definition the device build (csrc/textindex.hip) and the host build
(csrc/textindex_host.cpp) are held against, a parser of the index, and a region query that uses it.  Pure Python, no GPU, no library.

What an index says (the uncompressed bytes; the .tbi file is these bytes BGZF-framed):
  lines          the text split behind every '\\n'.  A line that starts with '#' or is empty is skipped.  Only the first HEAD bytes of a line are parsed.
  interval       0-based, half-open.  BED: columns 2 and 3.  VCF: beg = max(POS - 1, 0), end = beg + len(REF); the first `END=v` of INFO (at its start or behind
                 a ';') replaces end when v > beg.  end <= beg is read as beg + 1.  A number is its leading decimal digits (none: 0), capped at 2^40.
  contigs        maximal runs of records with the same column 1, numbered in order of first appearance.  A name with two runs, or a beg smaller than the one
                 before it inside a run, is SVX_E_ORDER; an end beyond 2^29 is SVX_E_RANGE (a file with both is SVX_E_ORDER).
  virtual offset of text offset u in block b: ((stream_base + block_coff[b]) << 16) | (u - block_uoff[b]), b the last block that starts at or before u.
                 A record's vbeg is that of its first byte, its vend the vbeg of the next line; the last line ends at (offset of the end-of-file block) << 16.
  bins           reg2bin of the five-level scheme (16 kb leaves, 37 449 bins).  The chunks of a bin are the maximal runs, in file order, of records with the
                 same (contig, bin): (vbeg of the first, vend of the last).  htslib's later merging of bins and chunks is not reproduced.
  pseudo-bin     37450, last: (vbeg of the contig's first record, vend of its last), (number of records, 0).
  linear index   1 + max((end - 1) >> 14) slots; a slot is the smallest vbeg of the records that overlap its 16 kb window, an empty slot takes the value of
                 the next one that is not.
Byte equality with the .tbi htslib writes is not claimed (it merges chunks); every reader of the format reads this one."""
import bisect
import struct
import zlib

VCF, BED = 0, 1
HEAD = 65280
MAX_END = 1 << 29
NUM_CAP = 1 << 40
PSEUDO_BIN = 37450
E_ORDER, E_RANGE = -9, -10
_FORMAT = {VCF: (2, 1, 2, 0), BED: (0x10000, 1, 2, 3)}      # format, col_seq, col_beg, col_end


class TabixError(ValueError):
    """the text cannot be indexed: code E_ORDER (records of a contig not contiguous, or positions decreasing inside one) or E_RANGE (an end beyond 2^29)"""

    def __init__(self, code, msg):
        ValueError.__init__(self, msg)
        self.code = code


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """every bin whose records can overlap [beg, end)"""
    end = min(end, MAX_END) - 1
    beg = max(0, min(beg, end))
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def _num(b, at=0):
    k = at
    while k < len(b) and 48 <= b[k] <= 57:
        k += 1
    return min(int(b[at:k]), NUM_CAP) if k > at else 0


def parse_line(line, preset):
    """one line (bytes, with or without its newline) -> (name, beg, end), or None for a line that is skipped"""
    if not line or line[:1] in (b"#", b"\n"):
        return None
    head = line[:HEAD].split(b"\n", 1)[0]
    col = head.split(b"\t", 8)
    col += [b""] * (8 - len(col))
    if preset == BED:
        beg, end = _num(col[1]), _num(col[2])
    else:
        beg = max(_num(col[1]) - 1, 0)
        end = beg + len(col[3])
        for item in col[7].split(b";"):
            if item.startswith(b"END="):
                v = _num(item, 4)
                if v > beg:
                    end = v
                break
    if end <= beg:
        end = beg + 1
    return col[0], beg, end


def line_starts(text):
    starts, at = [], 0
    while at < len(text):
        starts.append(at)
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
    return starts


def records(text, block_coff, block_uoff, preset, stream_base=0):
    """-> list of (name, beg, end, vbeg, vend, text offset) of the records of the text, in file order"""
    nb = len(block_coff) - 1
    uoff = [int(x) for x in block_uoff[:nb]]
    starts = line_starts(text)

    def voff(u):
        b = bisect.bisect_right(uoff, u) - 1
        return ((stream_base + int(block_coff[b])) << 16) | (u - uoff[b])
    v = [voff(s) for s in starts] + [(stream_base + int(block_coff[nb - 1])) << 16]
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(text)
        r = parse_line(text[s:min(e, s + HEAD)], preset)
        if r is not None:
            out.append(r + (v[k], v[k + 1], s))
    return out


def check_order(recs):
    """0, E_ORDER or E_RANGE for the records of one file (as `records` lists them)"""
    seen, prev, status = set(), None, 0
    for r in recs:
        if prev is None or r[0] != prev[0]:
            if r[0] in seen:
                return E_ORDER
            seen.add(r[0])
        elif r[1] < prev[1]:
            return E_ORDER
        if r[2] > MAX_END:
            status = E_RANGE
        prev = r
    return status


def contig_part(rows, n_mapped, n_unmapped):
    """the bytes of the part of one contig (of one reference in a .bai: bai.py) from its rows (beg, end, vbeg, vend), in file order and at least one: n_bin,
    the bins ascending with their chunks, the pseudo-bin with the two counts, n_intv, the linear index"""
    bins, prev_bin = {}, None
    for beg, end, vbeg, vend in rows:
        b = reg2bin(beg, end)
        if b == prev_bin:
            bins[b][-1][1] = vend
        else:
            bins.setdefault(b, []).append([vbeg, vend])
        prev_bin = b
    out = [struct.pack("<i", len(bins) + 1)]
    for b in sorted(bins):
        out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
    out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, rows[0][2], rows[-1][3], n_mapped, n_unmapped))
    n_intv = 1 + max((r[1] - 1) >> 14 for r in rows)
    lin = [None] * n_intv
    for beg, end, vbeg, _ in rows:
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if lin[w] is None or vbeg < lin[w]:
                lin[w] = vbeg
    for w in range(n_intv - 2, -1, -1):
        if lin[w] is None:
            lin[w] = lin[w + 1]
    out.append(struct.pack("<i%dQ" % n_intv, n_intv, *lin))
    return b"".join(out)


def build_index(text, block_coff, block_uoff, preset, stream_base=0):
    """the uncompressed .tbi bytes of `text` (bytes) whose BGZF stream has the block table block_coff / block_uoff (n_blocks + 1 entries each, the last block
    the end-of-file block: Engine.text_gz_tables, or block_table of the stream) and lies stream_base bytes into its file.  TabixError when it has none."""
    recs = records(bytes(text), block_coff, block_uoff, preset, stream_base)
    status = check_order(recs)
    if status:
        raise TabixError(status, "records out of order" if status == E_ORDER else "a record ends beyond 2^29")
    contigs = []      # [name, [records]]
    for r in recs:
        if not contigs or contigs[-1][0] != r[0]:
            contigs.append([r[0], []])
        contigs[-1][1].append(r)
    names = b"".join(c[0] + b"\0" for c in contigs)
    out = [b"TBI\1", struct.pack("<8i", len(contigs), *_FORMAT[preset], ord("#"), 0, len(names)), names]
    for _, rs in contigs:
        out.append(contig_part([r[1:5] for r in rs], len(rs), 0))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def parse_part(data, at, what, may_be_empty=False):
    """the part of one contig (of one reference in a .bai) at data[at:] -> ({bin: [(beg, end)]}, the pairs of bin 37450, linear list, offset behind the part).
    may_be_empty: the .bai rule - a part without bins has no pseudo-bin (None), every other has one of two pairs.  ValueError with `what` in front"""
    n_bin, = struct.unpack_from("<i", data, at)
    at += 4
    d, order, ps = {}, [], None
    for _ in range(n_bin):
        b, n_chunk = struct.unpack_from("<Ii", data, at)
        at += 8
        chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
        at += 16 * n_chunk
        if b == PSEUDO_BIN:
            ps = chunks
        else:
            d[b] = chunks
        order.append(b)
    bad_pseudo = ((ps is None) != (n_bin == 0) or (ps is not None and len(ps) != 2)) if may_be_empty else ps is None
    if order != sorted(order) or len(set(order)) != len(order) or bad_pseudo:
        raise ValueError("%s: bins not ascending, or no pseudo-bin" % what)
    n_intv, = struct.unpack_from("<i", data, at)
    at += 4
    lin = list(struct.unpack_from("<%dQ" % n_intv, data, at))
    return d, ps, lin, at + 8 * n_intv


def parse_index(data):
    """uncompressed .tbi bytes -> dict(format, col_seq, col_beg, col_end, meta, skip, names, bins: per contig {bin: [(beg, end)]}, pseudo: per contig the two
    pairs of bin 37450, linear: per contig list, n_no_coor); ValueError for bytes that are not one index exactly"""
    data = bytes(data)
    if data[:4] != b"TBI\1":
        raise ValueError("not a tabix index")
    n_ref, fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<8i", data, 4)
    at = 36
    names = data[at:at + l_nm].split(b"\0")[:-1] if l_nm else []
    if len(names) != n_ref or (l_nm and data[at + l_nm - 1:at + l_nm] != b"\0"):
        raise ValueError("tabix index: the names do not match n_ref")
    at += l_nm
    bins, pseudo, linear = [], [], []
    for _ in range(n_ref):
        d, ps, lin, at = parse_part(data, at, "tabix index")
        bins.append(d), pseudo.append(ps), linear.append(lin)
    n_no_coor, = struct.unpack_from("<Q", data, at)
    if at + 8 != len(data):
        raise ValueError("tabix index: %d bytes behind the trailer" % (len(data) - at - 8))
    return dict(format=fmt, col_seq=cs, col_beg=cb, col_end=ce, meta=meta, skip=skip, names=names, bins=bins, pseudo=pseudo, linear=linear, n_no_coor=n_no_coor)


def block_table(bgzf, lo=0, hi=None):
    """the block table of the BGZF blocks in bgzf[lo:hi], read from their headers -> (block_coff, block_uoff), n_blocks + 1 entries each, offsets from lo"""
    hi = len(bgzf) if hi is None else hi
    coff, uoff, at, u = [], [], lo, 0
    while at < hi:
        if bgzf[at:at + 4] != b"\x1f\x8b\x08\x04" or bgzf[at + 12:at + 16] != b"BC\x02\x00":
            raise ValueError("not a BGZF block at %d" % at)
        size = struct.unpack_from("<H", bgzf, at + 16)[0] + 1
        coff.append(at - lo), uoff.append(u)
        u += struct.unpack_from("<I", bgzf, at + size - 4)[0]
        at += size
    return coff + [at - lo], uoff + [u]


def inflate_block(bgzf, coff):
    """the text of the block at file offset coff -> (bytes, size of the block in the file)"""
    size = struct.unpack_from("<H", bgzf, coff + 16)[0] + 1
    return zlib.decompress(bgzf[coff + 18:coff + size - 8], -15), size


def query(index, bgzf, contig, beg, end, stats=None):
    """the lines (bytes, without newline) of the records of `contig` that overlap [beg, end), in file order.  index: parse_index's dict or the uncompressed
    bytes; bgzf: the bytes of the whole .gz file.  Candidate chunks come from reg2bins, those that end at or below the linear index's lower bound are dropped,
    and only the blocks the remaining chunks name are inflated (stats, a dict: 'blocks' counts them)."""
    ix = index if isinstance(index, dict) else parse_index(index)
    preset = BED if ix["format"] & 0x10000 else VCF
    name = contig.encode("utf-8") if isinstance(contig, str) else bytes(contig)
    if name not in ix["names"] or end <= beg:
        return []
    tid = ix["names"].index(name)
    lin = ix["linear"][tid]
    if (max(beg, 0) >> 14) >= len(lin):
        return []
    low = lin[max(beg, 0) >> 14]
    chunks = sorted(c for b in reg2bins(beg, end) for c in ix["bins"][tid].get(b, ()) if c[1] > low)
    merged = []
    for c in chunks:
        if merged and c[0] <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append(list(c))
    return read_chunks(merged, bgzf, preset, name, beg, end, stats)


def read_chunks(merged, bgzf, preset, name, beg, end, stats=None):
    """the lines of the records of contig `name` (bytes) that overlap [beg, end) inside the chunks `merged` (ascending, disjoint), in file order: the walk
    query() makes, also csi.query_text's"""
    cache, out = {}, []

    def block(coff):
        if coff not in cache:
            cache[coff] = inflate_block(bgzf, coff)
            if stats is not None:
                stats["blocks"] = stats.get("blocks", 0) + 1
        return cache[coff]
    for vbeg, vend in merged:
        coff, at = vbeg >> 16, vbeg & 0xffff
        while True:
            data, size = block(coff)
            while at >= len(data) and data:      # (a position at a block's end is the next block's start)
                coff, at = coff + size, 0
                data, size = block(coff)
            if ((coff << 16) | at) >= vend or not data:
                break
            parts = []
            while True:      # one line, over as many blocks as it has
                nl = data.find(b"\n", at)
                if nl >= 0:
                    parts.append(data[at:nl])
                    at = nl + 1
                    break
                parts.append(data[at:])
                coff, at = coff + size, 0
                data, size = block(coff)
                if not data:
                    break
            line = b"".join(parts)
            r = parse_line(line, preset)
            if r is not None and r[0] == name and r[1] < end and r[2] > beg:
                out.append(line)
    return out


def brute_force(text, preset, contig, beg, end):
    """the answer query() must give, by a scan over every line of the plain text"""
    name = contig.encode("utf-8") if isinstance(contig, str) else bytes(contig)
    out = []
    for line in bytes(text).split(b"\n"):
        r = parse_line(line, preset)
        if r is not None and end > beg and r[0] == name and r[1] < end and r[2] > beg:
            out.append(line)
    return out
