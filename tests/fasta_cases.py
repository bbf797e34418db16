"""FASTA files for the genome-loader tests: texts that exercise every rule of convert.genome_arrays, written as plain text, BGZF or one gzip stream."""
import gzip
import struct
import zlib

import numpy as np

from svim_amd import _abi

TILE, PIECE, NAME_BYTES = _abi.FASTA_TILE, _abi.FASTA_PIECE, _abi.FASTA_NAME_BYTES
IUPAC = _abi.NIBBLE.encode("ascii")


def bases(seed, n, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def record(name, seq, width=60, eol=b"\n", desc=b""):
    lines = [seq[i:i + width] for i in range(0, len(seq), width)] if width else [seq]
    return b">" + name + desc + eol + b"".join(l + eol for l in lines)


def lines_block(seed, n_bases, width=60):
    """n_bases random bases as lines of `width` (vectorised: the large files of the size tests)"""
    rng = np.random.default_rng(seed)
    rows = n_bases // width
    a = np.empty((rows, width + 1), dtype=np.uint8)
    a[:, :width] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(rows, width), dtype=np.uint8)]
    a[:, width] = 10
    return a.tobytes()


def bgzf_member(payload, level=6):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    cd = comp.compress(payload) + comp.flush()
    assert len(cd) + 26 <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cd) + 25) + cd +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf_bytes(text, cuts=None, block=0xff00, eof=True):
    """cuts: ascending offsets in text where a new block must begin (besides one every `block` bytes)"""
    edges = sorted(set([0, len(text)] + [c for c in (cuts or []) if 0 < c < len(text)]))
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        for i in range(a, b, block):
            out.append(bgzf_member(text[i:min(b, i + block)]))
    if eof:
        out.append(bgzf_member(b""))
    return b"".join(out)


def write(path, text, kind, cuts=None):
    """kind: 'plain' (name it .fa), 'bgzf' or 'gzip' (name them .fa.gz: genome_arrays picks its opener by the name)"""
    assert (kind == "plain") != str(path).endswith(".gz")
    if kind == "plain":
        data = text
    elif kind == "bgzf":
        data = bgzf_bytes(text, cuts)
    else:
        data = gzip.compress(text, 6)
    with open(path, "wb") as fh:
        fh.write(data)
    return str(path)


def path_for(tmp_path, name, kind):
    return str(tmp_path / (name + (".fa" if kind == "plain" else ".%s.fa.gz" % kind)))


def small_cases():
    """-> list of (name, text, references, BGZF cuts or None)"""
    c = []
    s1, s60, s61, s1l = bases(1, 37), bases(2, 60 * 7), bases(3, 61 * 5 + 17), bases(4, 9000)
    c.append(("widths", record(b"w1", s1, 1) + record(b"w60", s60, 60) + record(b"w61", s61, 61) + record(b"one", s1l, 0), ["w1", "w60", "w61", "one"], None))
    c.append(("crlf", record(b"a", bases(5, 500), 60, b"\r\n", b" desc") + record(b"b", bases(6, 121), 60, b"\r\n"), ["a", "b"], None))
    c.append(("crlf_cr_ends_file", b">a\r\nACGT\r\nAC\r", ["a"], None))
    c.append(("no_final_newline", record(b"a", bases(7, 130)) + b">b\n" + bases(8, 45), ["a", "b"], None))
    c.append(("header_only_no_newline", record(b"a", bases(7, 130)) + b">b", ["a", "b"], None))
    c.append(("empty_lines_and_records", b"\n\n>a\n\nAC\n\n\nGT\n>empty\n>b\nTTTT\n\n>last_is_header\n", ["a", "empty", "b", "last_is_header"], None))
    c.append(("header_longer_than_a_tile", record(b"a", bases(9, 300)) + b">long " + b"x" * (TILE + 700) + b" > tail\n" + bases(10, 77) + b"\n" + record(b"c", bases(11, 5)),
              ["a", "long", "c"], None))
    low = bases(12, 333).lower()
    c.append(("lower_case_and_iupac", record(b"mixed", IUPAC + IUPAC.lower() + low + bases(13, 50), 60) + record(b"eq", b"=" * 70, 60), ["mixed", "eq"], None))
    dup = record(b"d", bases(14, 100)) + record(b"e", bases(15, 200)) + record(b"d", bases(16, 150)) + record(b"f", bases(17, 99))
    c.append(("duplicate_names_last_wins", dup, ["d", "e", "f"], None))
    c.append(("references_reordered_absent_unrequested", dup, ["f", "nope", "d"], None))
    c.append(("nothing_requested_exists", dup, ["x", "y"], None))
    c.append(("no_references", dup, [], None))
    c.append(("text_before_the_first_header", b"#comment\nACGTNOTKEPT\n\n" + record(b"a", bases(18, 90)), ["a"], None))
    c.append(("no_header_at_all", b"ACGT\nACGT\n", ["a"], None))
    c.append(("empty_file", b"", ["a"], None))
    c.append(("gt_inside_lines_of_a_dropped_record", b">a\nACGT\n>b x>y\nAC>GT\n", ["a"], None))
    c.append(("name_ends_at_tab_and_cr", b">a\tdesc\nAC\n>b\r\nGT\r\n", ["a", "b"], None))
    # record boundaries against tile boundaries: the '>' as last byte of a tile, as first byte of the next, the header line across the boundary,
    # a newline as the last byte of a tile
    for k, shift in enumerate((-1, 0, 1, -3, -(NAME_BYTES // 2))):
        head = b">t0\n"
        fill = TILE + shift - len(head)
        body = bases(20 + k, fill)
        first = head + b"".join(body[i:i + 60] + b"\n" for i in range(0, len(body), 60))
        first = first[:TILE + shift - 1] + b"\n"
        assert len(first) == TILE + shift
        text = first + record(b"t1_straddles", bases(30 + k, 2 * TILE + 13), 60, b"\n", b" a description that runs on") + record(b"t2", bases(40 + k, 70))
        c.append(("tile_boundary_%d" % k, text, ["t2", "t1_straddles", "t0"], None))
    # several headers in one tile, a run of one-byte records
    c.append(("many_headers_in_one_tile", b"".join(record(b"r%d" % i, bases(50 + i, i % 5), 3) for i in range(300)), ["r%d" % i for i in (299, 0, 7, 150, 151, 4)], None))
    # BGZF blocks that end in the middle of a line and in the middle of a header
    t = record(b"b0", bases(60, 5000)) + record(b"b1_name", bases(61, 3000), 60, b"\n", b" descr") + record(b"b2", bases(62, 100))
    h1 = t.index(b">b1_name")
    c.append(("container_blocks_cut_lines_and_headers", t, ["b2", "b1_name", "b0"], [30, 1000, h1 + 1, h1 + 4, h1 + 12, h1 + 3000]))
    return c


def piece_boundary_case():
    """a header that straddles the staging-piece boundary and a contig that ends exactly there (second piece boundary)"""
    head = record(b"p0", b"", 60) + lines_block(70, (PIECE - 200) // 61 * 60)
    pad = PIECE - 5 - len(head)                                   # the '>' of p1 five bytes in front of the boundary
    head += bases(71, pad - 1) + b"\n"
    p1 = b">p1_straddles the piece boundary\n" + lines_block(72, 60 * 1000)
    text = head + p1
    fill = 2 * PIECE - len(text)
    text += bases(73, fill - 1) + b"\n"                            # p1 ends with the second piece
    assert len(text) == 2 * PIECE
    text += record(b"p2", bases(74, 1234))
    return "piece_boundary", text, ["p2", "p0", "p1_straddles"], [PIECE - 2, PIECE + 3]
