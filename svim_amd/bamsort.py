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
  index       bai.build_index(*bai.rows_of_bam(file)): a record that starts at stream offset u has vbeg = (coff[u // 65280] << 16) | (u % 65280)."""
import struct

E_ARG, E_RANGE = -3, -10
BLOCK = 65280
_NEW_HD = b"@HD\tVN:1.6\tSO:coordinate\n"


class BamSortError(ValueError):
    """the file cannot be sorted (code E_ARG, E_RANGE), or the device build refused it (.code: the library's status)"""

    def __init__(self, code, msg):
        ValueError.__init__(self, msg)
        self.code = code


def sort_key(body):
    """body: the bytes of one record behind its block_size field"""
    ref_id, pos = struct.unpack_from("<ii", body, 0)
    flag, = struct.unpack_from("<H", body, 14)
    return (ref_id & 0xffffffff, (pos + 1) & 0xffffffff, flag & 16)


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


def sorted_header(header):
    """the header of the sorted file (see above)"""
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
                f, seen = b"SO:coordinate", True
            fields.append(f)
        if not seen:
            fields.append(b"SO:coordinate")
        text = b"\t".join([b"@HD"] + fields) + tail
    else:
        text = _NEW_HD + text
    return b"BAM\1" + struct.pack("<i", len(text)) + text + rest


def split_records(stream, n_ref):
    """stream: records in file order (block_size + body each) -> list of their byte strings; BamSortError for what the definition refuses"""
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
        bad_range |= pos < -1
        out.append(stream[p:p + 4 + size])
        p += 4 + size
    if bad_arg:
        raise BamSortError(E_ARG, "a record names a reference the header does not have")
    if bad_range:
        raise BamSortError(E_RANGE, "a record has a position below -1")
    return out


def permutation(recs):
    """the file index of every record of the sorted order (stable)"""
    return sorted(range(len(recs)), key=lambda k: sort_key(recs[k][4:]))


def sort_records(stream, n_ref):
    """-> (the sorted record stream, the permutation)"""
    recs = split_records(stream, n_ref)
    perm = permutation(recs)
    return b"".join(recs[k] for k in perm), perm


def inflate(path):
    from .bai import bgzf_blocks
    with open(path, "rb") as fh:
        return b"".join(b[2] for b in bgzf_blocks(fh.read()))


def sorted_stream(path):
    """the inflated bytes of the sorted file of the BAM file at `path`"""
    raw = inflate(path)
    header, n_ref, at = split_header(raw)
    return sorted_header(header) + sort_records(raw[at:], n_ref)[0]


def n_blocks(stream_bytes):
    """BGZF blocks of a stream of that many bytes, the end-of-file block included"""
    return (stream_bytes + BLOCK - 1) // BLOCK + 1


def file(path):
    """the bytes of the sorted file (the library's host build of the encoder compresses the stream: no GPU)"""
    from ._lib import text_gz_host
    return text_gz_host(sorted_stream(path))
