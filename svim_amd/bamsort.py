"""A BAM file put into coordinate order: the definition the device build (csrc/bamsort.hip, fed by the device reader's record stream) and the host build
(csrc/bamsort_host.cpp) are held against.  Pure Python, no GPU, no library (only file() asks the library for the compressed bytes).

What the sorted file is:
  order       records are compared by sort_key = (uint32(refID), uint32(pos + 1), flag & 16): refID = -1 is 0xFFFFFFFF and sorts last, pos = -1 sorts first
              within its reference, a forward record precedes a reverse one at the same position.  Records with equal keys keep their file order (the sort
              is stable).  This is the coordinate order samtools documents; samtools is not at hand here and byte identity with its output is not claimed.
  refusals    BamSortError: refID < -1 or refID >= n_ref, or block_size < 32, or a stream that ends inside a record (code E_ARG); pos < -1 (code E_RANGE).
              A file with both kinds is E_ARG.
  header      magic, l_text, text, n_ref and the reference dictionary.  The text ends at its first NUL.  If its first line starts with "@HD\\t", every SO:
              field of that line becomes SO:coordinate (a line without one gets the field appended), its GO: and SS: fields are removed, every other field
              and every other line stays as it is.  A text without such a line gets "@HD\\tVN:1.6\\tSO:coordinate\\n" in front.  l_text is the new length
              (no NUL padding); the reference dictionary is copied unchanged.
  stream      the rewritten header followed by every record verbatim (its 4-byte block_size and its body, the bin field included) in sorted order.
  file        the stream cut into BGZF blocks of exactly 65 280 stream bytes (the last one shorter) and the 28-byte end-of-file block.  Block edges ignore header
              and record edges, which the BAM specification allows; htslib's own layout is not reproduced.  The compressed bytes are what
              svx_text_gz_host makes of the stream (csrc/deflate_core.hpp).
  index       bai.build_index(*bai.rows_of_bam(file)): a record that starts at stream offset u has vbeg = (coff[u // 65280] << 16) | (u % 65280).
  spilled     a file whose records do not fit on the device is sorted in runs (svx_bam_sort_begin_spill): runs_of cuts the file into consecutive ranges and
              sorts each, merge_runs merges them with ties to the lower run - the same stream and permutation, whatever the cuts - and piece_cuts says which
              contiguous range of every run a piece of the output needs.  The device and the host build (svx_bam_sort_spill_host) are held to these.

Query-name order (order="queryname"; csrc/bamsort.hip: the k_ns_* kernels, csrc/bamsort_host.cpp: svx_bam_sort_host_order) - the input of SVIM's query-name
front end, which needs the records of a read next to each other:
  order       records are compared by name_key = (name_of(body), name_rank(flag)).  name_of is body[32 : 32 + l_read_name] cut at its first NUL (the whole
              range when it holds none); names compare as unsigned bytes and a proper prefix sorts first.  name_rank puts the READ1 / READ2 bits first, then
              primary < secondary < supplementary.  Equal keys keep their file order.  This is the lexicographic order samtools calls `-N` (its `-n` is a
              natural order that compares runs of digits as numbers: not this one); samtools is not at hand here and byte identity with its output is not claimed.
  refusals    those above, and E_ARG for l_read_name = 0 and for a name field that runs past the record (32 + l_read_name > block_size).  E_ARG before E_RANGE.
  header      the same rule with SO:queryname; GO: and every SS: field are removed and SS:queryname:lexicographical is put behind the (first) SO: field.  A
              text without an @HD line gets "@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n" in front.
  stream, file  as above.  A query-name-sorted file has no index.  sort_begin / sort_bam sort in this order in memory only; beyond device memory and over several
              files the order is a merge session's (svim_amd/bammerge.py, order="queryname"; runs_of(order="queryname") forms its runs)."""
import struct

E_ARG, E_RANGE = -3, -10
BLOCK = 65280
_NEW_HD = b"@HD\tVN:1.6\tSO:coordinate\n"
ORDERS = ("coordinate", "queryname")
_SS_NAME = b"SS:queryname:lexicographical"


class BamSortError(ValueError):
    """the file cannot be sorted (code E_ARG, E_RANGE), or the device build refused it (.code: the library's status)"""

    def __init__(self, code, msg):
        ValueError.__init__(self, msg)
        self.code = code


def coordinate_key(ref_id, pos, flag):
    """the coordinate order's key from a record's fields (what SVIM_genotyping.AlignmentIndex(order="sort") and the resident alignment table sort by)"""
    return (ref_id & 0xffffffff, (pos + 1) & 0xffffffff, flag & 16)


def sort_key(body):
    """body: the bytes of one record behind its block_size field"""
    ref_id, pos = struct.unpack_from("<ii", body, 0)
    flag, = struct.unpack_from("<H", body, 14)
    return coordinate_key(ref_id, pos, flag)


def name_of(body):
    """the read name of a record: the bytes of its name field in front of the first NUL"""
    field = bytes(body[32:32 + body[8]])
    nul = field.find(b"\0")
    return field if nul < 0 else field[:nul]


def name_rank(flag):
    """READ1 / READ2 first, then primary < secondary < supplementary"""
    return ((flag >> 6) & 3) << 2 | ((flag >> 11) & 1) << 1 | ((flag >> 8) & 1)


def name_key(body):
    """body: the bytes of one record behind its block_size field -> its place in query-name order (bytes compare as unsigned, a proper prefix first)"""
    return (name_of(body), name_rank(struct.unpack_from("<H", body, 14)[0]))


def _order(order):
    if order not in ORDERS:
        raise ValueError("order is %r or %r" % ORDERS)
    return order == "queryname"


def split_header(raw):
    """raw: the inflated bytes of a BAM file -> (header bytes, n_ref, offset of the first record)"""
    if raw[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    return raw[:p], n_ref, p


def sorted_header(header, order="coordinate"):
    """the header of the sorted file (see above)"""
    by_name = _order(order)
    so = b"SO:queryname" if by_name else b"SO:coordinate"
    header = bytes(header)
    if header[:4] != b"BAM\1":
        raise ValueError("not a BAM header")
    l_text, = struct.unpack_from("<i", header, 4)
    text, rest = header[8:8 + l_text], header[8 + l_text:]
    nul = text.find(b"\0")
    if nul >= 0:
        text = text[:nul]
    if text.startswith(b"@HD\t"):
        eol = text.find(b"\n")
        line, tail = (text, b"") if eol < 0 else (text[:eol], text[eol:])
        fields, seen = [], False
        for f in line.split(b"\t")[1:]:
            if f.startswith(b"GO:") or f.startswith(b"SS:"):
                continue
            if f.startswith(b"SO:"):
                fields.append(so)
                if by_name and not seen:
                    fields.append(_SS_NAME)
                seen = True
                continue
            fields.append(f)
        if not seen:
            fields += [so, _SS_NAME] if by_name else [so]
        text = b"\t".join([b"@HD"] + fields) + tail
    else:
        text = (b"@HD\tVN:1.6\t" + so + b"\t" + _SS_NAME + b"\n" if by_name else _NEW_HD) + text
    return b"BAM\1" + struct.pack("<i", len(text)) + text + rest


def split_records(stream, n_ref, order="coordinate"):
    """stream: records in file order (block_size + body each) -> list of their byte strings; BamSortError for what the definition refuses (query-name order
    refuses a record without a name field or with one that runs past the record as well)"""
    by_name = _order(order)
    stream = bytes(stream)
    out, p, bad_arg, bad_range = [], 0, False, False
    while p < len(stream):
        if p + 4 > len(stream):
            raise BamSortError(E_ARG, "the stream ends inside a block_size field")
        size, = struct.unpack_from("<I", stream, p)
        if size < 32:
            raise BamSortError(E_ARG, "block_size %d < 32 at offset %d" % (size, p))
        if p + 4 + size > len(stream):
            raise BamSortError(E_ARG, "the stream ends inside a record")
        ref_id, pos = struct.unpack_from("<ii", stream, p + 4)
        bad_arg |= ref_id < -1 or ref_id >= n_ref
        bad_arg |= by_name and (stream[p + 12] == 0 or 32 + stream[p + 12] > size)
        bad_range |= pos < -1
        out.append(stream[p:p + 4 + size])
        p += 4 + size
    if bad_arg:
        raise BamSortError(E_ARG, "a record names a reference the header does not have" + (", has no name field or one that runs past its end" if by_name else ""))
    if bad_range:
        raise BamSortError(E_RANGE, "a record has a position below -1")
    return out


def permutation(recs, order="coordinate"):
    """the file index of every record of the sorted order (stable)"""
    key = name_key if _order(order) else sort_key
    return sorted(range(len(recs)), key=lambda k: key(recs[k][4:]))


def sort_records(stream, n_ref, order="coordinate"):
    """-> (the sorted record stream, the permutation)"""
    recs = split_records(stream, n_ref, order)
    perm = permutation(recs, order)
    return b"".join(recs[k] for k in perm), perm


def runs_of(stream, n_ref, run_ends, order="coordinate"):
    """The spilled sort (svx_bam_sort_begin_spill) forms runs: consecutive ranges of the file, each sorted on its own.  stream: records in file order;
    run_ends: the number of records in front of the end of every run, non-decreasing (equal neighbours: an empty run), the last one the number of records
    -> one list per run of (sort key, file index, record bytes), in the run's stable order.  The bytes of a run, joined, are its part of the spill file.
    order="queryname": the key is name_key (a merge session with a spill directory forms such runs); merge_runs and piece_cuts take them as they are."""
    key = name_key if _order(order) else sort_key
    recs = list(stream) if isinstance(stream, (list, tuple)) else split_records(stream, n_ref, order)      # (a list: records already split and checked)
    run_ends = [int(e) for e in run_ends]
    if any(b < a for a, b in zip([0] + run_ends, run_ends)) or (run_ends[-1] if run_ends else 0) != len(recs):
        raise ValueError("run_ends must be non-decreasing and end with the number of records")
    return [[(key(recs[k][4:]), k, recs[k]) for k in sorted(range(a, b), key=lambda k: key(recs[k][4:]))] for a, b in zip([0] + run_ends, run_ends)]


def merge_runs(runs):
    """the k-way merge of sorted runs, a tie going to the lower run (within a run the order stands) -> (the sorted record stream, the permutation).  Runs are
    consecutive ranges of the file and each is in stable order, so equal keys leave in file order: the stream and the permutation of sort_records."""
    import heapq
    heads = [(run[0][0], r, 0) for r, run in enumerate(runs) if run]
    heapq.heapify(heads)
    out, perm = [], []
    while heads:
        _, r, i = heapq.heappop(heads)
        perm.append(runs[r][i][1])
        out.append(runs[r][i][2])
        if i + 1 < len(runs[r]):
            heapq.heappush(heads, (runs[r][i + 1][0], r, i + 1))
    return b"".join(out), perm


def piece_cuts(runs, perm, first_byte, piece_bytes):
    """What a piece of the output needs of every run.  runs: runs_of(...); perm: the permutation of the sorted order; first_byte: bytes in front of the first
    record in the output stream (the header; 0 for the record stream alone); a piece is piece_bytes of the stream.
    The rule: a run's records keep their in-run order in the global order, so the global positions of a run's records, gpos, increase along the run, and among
    any CONTIGUOUS range [p0, p1) of global positions the run's records are a contiguous in-run range [a, b): a = the first i with gpos[i] >= p0, b = the
    first i with gpos[i] >= p1 (csrc/bamsort_core.hpp: bsort_piece_cut).  A piece holds bytes of the records at positions [p0, p1) - the first and the last
    may straddle its edges - and therefore reads one contiguous byte range per run.
    -> per piece (p0, p1, [(a, b) per run])."""
    import bisect
    where = {}
    for r, run in enumerate(runs):
        for i, (_, k, _) in enumerate(run):
            where[k] = (r, i)
    n = len(perm)
    gpos = [[0] * len(run) for run in runs]
    ends, at = [], first_byte
    for j, k in enumerate(perm):
        r, i = where[k]
        gpos[r][i] = j
        at += len(runs[r][i][2])
        ends.append(at)
    out = []
    for lo in range(0, at, piece_bytes):
        hi = min(lo + piece_bytes, at)
        # the records with a byte in [lo, hi): record j covers [ends[j - 1], ends[j])
        p0 = bisect.bisect_right(ends, lo) if n else 0
        p1 = bisect.bisect_left(ends, hi) + 1 if hi > first_byte and n else 0
        p0, p1 = min(p0, n), min(p1, n)
        p0 = min(p0, p1)
        out.append((p0, p1, [(bisect.bisect_left(g, p0), bisect.bisect_left(g, p1)) for g in gpos]))
    return out


def inflate(path):
    from .bai import bgzf_blocks
    with open(path, "rb") as fh:
        return b"".join(b[2] for b in bgzf_blocks(fh.read()))


def sorted_stream(path, order="coordinate"):
    """the inflated bytes of the sorted file of the BAM file at `path`"""
    raw = inflate(path)
    header, n_ref, at = split_header(raw)
    return sorted_header(header, order) + sort_records(raw[at:], n_ref, order)[0]


def n_blocks(stream_bytes):
    """BGZF blocks of a stream of that many bytes, the end-of-file block included"""
    return (stream_bytes + BLOCK - 1) // BLOCK + 1


def file(path, order="coordinate"):
    """the bytes of the sorted file (the library's host build of the encoder compresses the stream: no GPU)"""
    from ._lib import text_gz_host
    return text_gz_host(sorted_stream(path, order))
