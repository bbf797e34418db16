"""Several BAM files merged into one file in coordinate order: the definition the host build (csrc/bamsort_host.cpp: svx_bam_merge_header_host,
svx_bam_merge_host, the id rule in csrc/bamsort_core.hpp: bsort_translate) and the device build (a merge session: svx_bam_merge_*, bamio.BamMerge,
csrc/bammerge.hip; DESIGN sections 35 and 38) are both held against.  Pure Python, no GPU, no library (only file() asks the library for the compressed bytes).
It stands on svim_amd/bamsort.py: the merge of one file IS the sort of that file.

What the merged file is:
  inputs      k >= 1 files in the order given, each the inflated bytes of a BAM file (SAM text: through the BAM header and records svim_amd/sam.py defines).
              Any record order inside a file is accepted: the merge is a sort.
  dictionary  the first file's references in their order; then, file by file, the names not yet present, in that file's order.  One name with two lengths
              is BamMergeError(E_ARG), and so is a name twice in one file's dictionary.  tid_map[f][i] is the merged id of file f's reference i; the first
              file's map is always the identity.
  records     the global record number is the place in the concatenation of the inputs.  A record of a file whose map is the identity is copied verbatim
              (unchecked mate ids included: what the sort of one file does).  A record of any other file gets refID (body offset 0) and next_refID (body
              offset 20) replaced by their mapped values, -1 staying -1, every other byte verbatim, bin included; there a next_refID below -1 or not below the
              file's n_ref is E_ARG.  The refusals of bamsort.split_records hold per file, with that file's n_ref; E_ARG in any file goes before E_RANGE.
  order       bamsort.sort_key of the TRANSLATED record, stable over global record numbers: equal keys leave in file order, then in-file order.  The
              permutation is over global record numbers.
  header      one input: bamsort.sorted_header(header), so that the merge of one file is sort_bam's file byte for byte.  Several inputs - every text ends at
              its first NUL, is cut into lines at "\\n", empty lines are dropped and every line written ends in "\\n":
                1. the first line of sorted_header(first file)'s text (always an @HD line with SO:coordinate);
                2. if any input has a line that starts with "@SQ\\t": one line per merged reference in dictionary order - the first line over all inputs (file
                   order, then line order) that starts with "@SQ\\t" and has a field exactly "SN:<name>", verbatim, or "@SQ\\tSN:<name>\\tLN:<len>" without one;
                3. every other line of every file, in file order: a first line that starts with "@HD\\t" and every line that starts with "@SQ\\t" are left out,
                   and a line byte-identical to one already written is dropped;
                4. an @RG line whose ID: equals that of an @RG line already written but whose bytes differ is E_ARG: renaming a read group would mean
                   rewriting the RG:Z tags of its records, which is out of scope;
                5. an @PG line of file k >= 1 whose ID: equals that of an @PG line already written but whose bytes differ gets the id "<id>-<k>", with a
                   further "-<k>" while that id is taken too; PP:<id> fields of the @PG lines of the same file behind it follow the rename (they are rewritten
                   before the line is compared with what is written).  PG:Z tags inside records are NOT rewritten: a stated limitation.
              l_text is the new length (no NUL padding); the binary dictionary is the merged one.
  stream, file, index: as in bamsort.py - blocks of 65 280 stream bytes, the bytes svx_text_gz_host writes, the .bai / .csi of bai.py / csi.py over the merged
              dictionary.  As there, byte identity with samtools merge is not claimed.

Query-name order (order="queryname" as the last keyword of merged_text, merged_header, merge, stream_of and file; the default leaves every byte as it is) - the
input of the query-name front end when a run comes as one file per flow cell:
  records     translated exactly as above, per file.  The two name refusals of bamsort.split_records(order="queryname") - l_read_name = 0, a name field that
              runs past the record - are E_ARG like a bad refID or mate id; an E_ARG in ANY file goes before an E_RANGE in any file.
  order       bamsort.name_key of the translated record (the key ignores the ids), stable over global record numbers: equal (name, rank) leave in file
              order, then in in-file order.
  header      one input: bamsort.sorted_header(header, "queryname") - the merge of one file is the name sort of that file byte for byte.  Several inputs:
              rule 1 takes the first line of sorted_header(first file, "queryname") (SO:queryname followed by SS:queryname:lexicographical); rules 2 to 5
              are unchanged.
  index       none.
  runs        bamsort.runs_of(..., order="queryname") keys the runs by name_key; merge_runs and piece_cuts stay as they are (tuples compare)."""
import struct

from . import bamsort
from .bamsort import E_ARG, E_RANGE, BamSortError


class BamMergeError(BamSortError):
    """the files cannot be merged (code E_ARG, E_RANGE; from the host build: the library's status)"""


def parse_header(header):
    """header bytes (magic .. dictionary) -> (the text up to its first NUL, [(name, length)])"""
    header = bytes(header)
    if header[:4] != b"BAM\1" or len(header) < 12:
        raise BamMergeError(E_ARG, "not a BAM header")
    l_text, = struct.unpack_from("<i", header, 4)
    text = header[8:8 + l_text]
    nul = text.find(b"\0")
    if nul >= 0:
        text = text[:nul]
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", header, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", header, p)
        name = header[p + 4:p + 4 + l_name].split(b"\0")[0]
        length, = struct.unpack_from("<i", header, p + 4 + l_name)
        refs.append((name, length))
        p += 8 + l_name
    return text, refs


def merged_dictionary(dicts):
    """dicts: per file [(name, length)] -> the merged [(name, length)]"""
    out, length_of = [], {}
    for d in dicts:
        seen = set()
        for name, length in d:
            if name in seen:
                raise BamMergeError(E_ARG, "the name %r twice in one file's dictionary" % name)
            seen.add(name)
            if name not in length_of:
                length_of[name] = length
                out.append((name, length))
            elif length_of[name] != length:
                raise BamMergeError(E_ARG, "the reference %r has the lengths %d and %d" % (name, length_of[name], length))
    return out


def tid_maps(dicts):
    """-> per file the list tid_map[f][i] = merged id of file f's reference i"""
    at = {name: i for i, (name, _) in enumerate(merged_dictionary(dicts))}
    return [[at[name] for name, _ in d] for d in dicts]


def _field(line, tag):
    """the value of the first field of a header line that starts with tag (b"ID:"), or None"""
    for f in line.split(b"\t")[1:]:
        if f.startswith(tag):
            return f[len(tag):]
    return None


def merged_text(texts, refs, order="coordinate"):
    """the text of the merged header of several files (rule 1 to 5 above); texts: each cut at its first NUL already; refs: the merged dictionary;
    order="queryname": rule 1 takes the first line of sorted_header(first file, "queryname")"""
    lines_of = [[ln for ln in t.split(b"\n") if ln] for t in texts]
    first = parse_header(bamsort.sorted_header(b"BAM\1" + struct.pack("<i", len(texts[0])) + texts[0] + struct.pack("<i", 0), order))[0]
    out = [first.split(b"\n")[0]]
    written = set(out)
    if any(ln.startswith(b"@SQ\t") for lines in lines_of for ln in lines):
        for name, length in refs:
            want = b"SN:" + name
            line = next((ln for lines in lines_of for ln in lines if ln.startswith(b"@SQ\t") and want in ln.split(b"\t")[1:]), None)
            line = line if line is not None else b"@SQ\tSN:" + name + b"\tLN:" + str(length).encode()
            out.append(line)
            written.add(line)
    rg_ids, pg_ids = {}, set()
    for k, (text, lines) in enumerate(zip(texts, lines_of)):
        renamed = {}
        for j, ln in enumerate(lines):
            if (j == 0 and text.startswith(b"@HD\t")) or ln.startswith(b"@SQ\t"):
                continue
            if ln.startswith(b"@PG\t") and renamed:
                ln = b"\t".join(b"PP:" + renamed[f[3:]] if f.startswith(b"PP:") and f[3:] in renamed else f for f in ln.split(b"\t"))
            if ln in written:
                continue
            if ln.startswith(b"@RG\t"):
                rid = _field(ln, b"ID:")
                if rid is not None and rid in rg_ids:
                    raise BamMergeError(E_ARG, "two @RG lines with ID:%s and different bytes (read groups are not renamed: that would mean rewriting RG:Z tags, which "
                                               "is out of scope)" % rid.decode("latin-1"))
                if rid is not None:
                    rg_ids[rid] = ln
            elif ln.startswith(b"@PG\t"):
                pid = _field(ln, b"ID:")
                if pid is not None and pid in pg_ids and k >= 1:
                    new = pid + b"-%d" % k
                    while new in pg_ids:
                        new += b"-%d" % k
                    renamed[pid] = new
                    fields, done = [], False
                    for f in ln.split(b"\t"):
                        if not done and fields and f.startswith(b"ID:"):
                            f, done = b"ID:" + new, True
                        fields.append(f)
                    ln, pid = b"\t".join(fields), new
                if pid is not None:
                    pg_ids.add(pid)
            out.append(ln)
            written.add(ln)
    return b"".join(ln + b"\n" for ln in out)


def merged_header(headers, order="coordinate"):
    """headers: per file the bytes magic .. dictionary -> the header of the merged file (order: "coordinate" or "queryname")"""
    bamsort._order(order)
    headers = [bytes(h) for h in headers]
    if not headers:
        raise BamMergeError(E_ARG, "no input")
    if len(headers) == 1:
        return bamsort.sorted_header(headers[0], order)
    parsed = [parse_header(h) for h in headers]
    refs = merged_dictionary([p[1] for p in parsed])
    text = merged_text([p[0] for p in parsed], refs, order)
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out.append(struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length))
    return b"".join(out)


def translate_record(rec, tid_map):
    """rec: block_size + body of a record of a file with len(tid_map) references whose map is not the identity -> the record as the merged file holds it"""
    ref_id, = struct.unpack_from("<i", rec, 4)
    mate, = struct.unpack_from("<i", rec, 24)
    n_ref = len(tid_map)
    if ref_id < -1 or ref_id >= n_ref:
        raise BamMergeError(E_ARG, "a record names a reference its header does not have")
    if mate < -1 or mate >= n_ref:
        raise BamMergeError(E_ARG, "a record of a translated file names a mate reference its header does not have")
    m = lambda t: -1 if t < 0 else tid_map[t]       # noqa: E731
    return rec[:4] + struct.pack("<i", m(ref_id)) + rec[8:24] + struct.pack("<i", m(mate)) + rec[28:]


def _split(stream, n_ref, by_name=False):
    """bamsort.split_records, but what is wrong is handed back instead of raised: (records, a refID outside the dictionary - by_name: or one of the two name
    refusals of query-name order -, a position below -1)"""
    stream = bytes(stream)
    out, p, bad_arg, bad_range = [], 0, False, False
    while p < len(stream):
        if p + 4 > len(stream):
            raise BamMergeError(E_ARG, "the stream ends inside a block_size field")
        size, = struct.unpack_from("<I", stream, p)
        if size < 32 or p + 4 + size > len(stream):
            raise BamMergeError(E_ARG, "block_size %d at offset %d: below 32, or the stream ends inside the record" % (size, p))
        ref_id, pos = struct.unpack_from("<ii", stream, p + 4)
        bad_arg |= ref_id < -1 or ref_id >= n_ref
        bad_arg |= by_name and (stream[p + 12] == 0 or 32 + stream[p + 12] > size)
        bad_range |= pos < -1
        out.append(stream[p:p + 4 + size])
        p += 4 + size
    return out, bad_arg, bad_range


def merge(files, order="coordinate"):
    """files: per input (record stream in file order, n_ref, tid_map) -> (the merged record stream, the permutation over global record numbers);
    order="queryname": the key is bamsort.name_key of the translated record, and the two name refusals are E_ARG"""
    by_name = bamsort._order(order)
    recs, bad_arg, bad_range = [], False, False
    for stream, n_ref, tmap in files:
        tmap = [int(t) for t in tmap]
        if len(tmap) != n_ref:
            raise BamMergeError(E_ARG, "a map needs one entry per reference of its file")
        rs, a, r = _split(stream, n_ref, by_name)
        bad_arg, bad_range = bad_arg or a, bad_range or r
        if tmap != list(range(n_ref)):
            for i, rec in enumerate(rs):
                try:
                    rs[i] = translate_record(rec, tmap)
                except BamMergeError:
                    bad_arg = True
        recs += rs
    if bad_arg:
        raise BamMergeError(E_ARG, "a record names a reference, or a translated record a mate reference, that its file's header does not have"
                            + (", or has no name field or one that runs past its end" if by_name else ""))
    if bad_range:
        raise BamMergeError(E_RANGE, "a record has a position below -1")
    perm = bamsort.permutation(recs, order)
    return b"".join(recs[k] for k in perm), perm


def stream_of(raws, order="coordinate"):
    """raws: the inflated bytes of every input file -> (the inflated bytes of the merged file, the permutation)"""
    parts = [bamsort.split_header(bytes(raw)) for raw in raws]
    headers = [h for h, _, _ in parts]
    if len(raws) == 1:
        maps = [list(range(parts[0][1]))]
    else:
        maps = tid_maps([parse_header(h)[1] for h in headers])
    header = merged_header(headers, order)
    stream, perm = merge([(raw[at:], n_ref, m) for raw, (_, n_ref, at), m in zip(raws, parts, maps)], order)
    return header + stream, perm


def _header_size(raw):
    """bytes of the header the inflated file starts with, or None while `raw` is too short to tell"""
    if len(raw) < 12:
        return None
    if raw[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    if len(raw) < p + 4:
        return None
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        if len(raw) < p + 4:
            return None
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    return p if len(raw) >= p else None


def header_of(path):
    """the header (magic .. dictionary) of the BAM file at `path`: only the BGZF blocks that hold it are read and inflated"""
    import zlib
    raw = b""
    with open(path, "rb") as fh:
        while True:
            head = fh.read(12)
            if len(head) < 12 or head[:3] != b"\x1f\x8b\x08" or not head[3] & 4:
                raise ValueError("%s: the file ends inside its header, or is not BGZF" % path)
            extra = fh.read(struct.unpack_from("<H", head, 10)[0])
            p, bsize = 0, None
            while p + 4 <= len(extra):
                slen, = struct.unpack_from("<H", extra, p + 2)
                if extra[p:p + 2] == b"BC" and slen == 2:
                    bsize, = struct.unpack_from("<H", extra, p + 4)
                p += 4 + slen
            if bsize is None:
                raise ValueError("%s: a gzip member without the BGZF size field" % path)
            body = fh.read(bsize + 1 - 12 - len(extra))
            raw += zlib.decompress(body[:-8], -15)
            size = _header_size(raw)
            if size is not None:
                return raw[:size]


def file(paths, order="coordinate"):
    """the bytes of the merged file of the BAM files at `paths` (the library's host build of the encoder compresses the stream: no GPU)"""
    from ._lib import text_gz_host
    return text_gz_host(stream_of([bamsort.inflate(p) for p in paths], order)[0])
