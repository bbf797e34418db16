"""Corner files for the coordinate sort (svim_amd/bamsort.py, csrc/bamsort_host.cpp, csrc/bamsort.hip): small BAM files in any order, built from the record
builders of tests/bai_cases.py and tests/foreign_bam.py and shuffled by seeded permutations.  tests/test_bam_sort.py holds the definition and the host
build to them on the CPU, tests/test_gpu_bam_sort.py the device build on the GPU.

    order      no record; one record; already in order; in reverse order; 40 records with 5 distinct keys and 40 distinct names (stability); forward and reverse
               records at one position; pos = -1 on a placed reference; refID = -1 with and without a position, scattered through the file
    layout     a record that ends exactly at stream offset 65 280; a record whose 4-byte length field straddles that block edge; a record longer than two
               blocks; records of 36 to 40 bytes of body; CIGARs of 4096, 4097 and 65 535 operations and a CG-tag record; input files whose own BGZF blocks
               cut records anywhere
    headers    @HD with SO:queryname, with SO:unsorted and GO:query, without SO:, no @HD line, NUL padding behind the text

Test infrastructure only."""
import os
import random
import struct
import zlib

import bai_cases as BC
import foreign_bam as FB
from svim_amd import bamsort

REFS, LENS = BC.REFS, BC.LENS


def header(text=None, refs=REFS, lens=LENS, pad=0):
    """header bytes with any text (None: foreign_bam's, SO:unsorted) and `pad` NUL bytes behind it, counted in l_text"""
    if text is None:
        return FB.header_bytes(refs, lens, "unsorted")
    text = text.encode("ascii") + b"\0" * pad
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in zip(refs, lens):
        nb = n.encode("ascii") + b"\0"
        out += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    return out


def sq_lines(refs=REFS, lens=LENS):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(refs, lens))


def write_raw(path, hdr, rec_bytes, cuts=0xff00, level=6):
    """the header and the records, cut into BGZF blocks: cuts a number (every that many bytes) or a function (stream length, record starts) -> cut offsets"""
    raw, starts = hdr, []
    for rb in rec_bytes:
        starts.append(len(raw))
        raw += rb
    at = list(range(0, len(raw), cuts)) if isinstance(cuts, int) else [0] + [c for c in cuts(len(raw), starts) if 0 < c < len(raw)]
    at = sorted(set(at)) + [len(raw)]
    with open(path, "wb") as fh:
        for a, b in zip(at, at[1:]):
            for lo in range(a, b, 0xff00):
                fh.write(FB.bgzf_block(raw[lo:min(b, lo + 0xff00)], level, zlib.Z_DEFAULT_STRATEGY))
        fh.write(FB.EOF_BLOCK)


def shuffled(items, seed):
    items = list(items)
    random.Random(seed).shuffle(items)
    return items


def tiny_record(name, tid, pos, flag):
    """a record without CIGAR, bases and aux fields: 32 bytes and its name"""
    nb = name.encode("ascii") + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nb), 0, 4680, 0, flag, 0, -1, -1, 0) + nb
    return struct.pack("<i", len(body)) + body


def padded_to(hdr, recs, target):
    """recs: records in sorted order with distinct keys (AlignedSegment objects).  One of them gets a Z tag so long that a record of the sorted stream ends exactly
    at stream offset `target` -> their bytes, in that order"""
    rb = BC.record_bytes(recs)
    at, k = len(bamsort.sorted_header(hdr)), 0
    while at + len(rb[k]) <= target - 4:
        at += len(rb[k])
        k += 1
    # (record k - 1 ends at `at` <= target - 4: a tag of target - at bytes - 3 of tag and type, the string, its NUL - behind it)
    assert k >= 1 and 4 <= target - at < 4000
    a = recs[k - 1]
    a._tags = dict(a._tags, XP="p" * (target - at - 4))
    rb[k - 1] = BC.record_bytes([a])[0]
    return rb


def _ascending(seed, n, tid=1):
    """n records of one reference at distinct ascending positions, forward"""
    rng = random.Random(seed)
    pos, out = 100, []
    for k in range(n):
        pos += rng.randrange(1, 50)
        out.append(BC.seg("a%d" % k, tid, pos, BC.random_cigar(rng), flag=0, mapq=60))
    return out


def alignment_records(seed, n):
    """n records of 36 to 160 bytes in random order: their sizes take every value mod 16, so that record starts meet every alignment in the file and in the
    sorted stream"""
    rng = random.Random(seed)
    return [tiny_record("q" * rng.randrange(3, 128), rng.choice((0, 1, 3, -1)), rng.randrange(-1, 5000), rng.choice((0, 16, 4, 20))) for _ in range(n)]


def build_all(dirpath):
    """writes every corner file into dirpath -> {name: dict(path, header, records: their bytes in file order, n_ref)}"""
    out = {}

    def add(name, rec_bytes, hdr=None, cuts=0xff00, refs=REFS):
        hdr = header() if hdr is None else hdr
        path = os.path.join(dirpath, name + ".bam")
        write_raw(path, hdr, rec_bytes, cuts)
        out[name] = dict(path=path, header=hdr, records=list(rec_bytes), n_ref=len(refs))
    mid = BC.random_records(51, 300, (1, 3, 4), LENS, n_unplaced=6)
    add("no_records", [])
    add("one_record", BC.record_bytes([BC.seg("only", 4, 12345, [(0, 100)])]))
    add("already_in_order", BC.record_bytes(mid), cuts=3001)
    add("reverse_order", BC.record_bytes(mid)[::-1], cuts=2500)
    keys = [(1, 700, 0), (1, 700, 16), (3, 5, 0), (1, 90000, 16), (-1, -1, 0)]
    rng = random.Random(52)
    forty = [BC.seg("name%02d" % k, t, p, [(0, 30 + k)] if t >= 0 else [], flag=f | (4 if t < 0 else 0)) for k, (t, p, f) in enumerate(rng.choice(keys) for _ in range(40))]
    add("five_keys_forty_names", BC.record_bytes(forty))
    add("forward_and_reverse_at_one_position", BC.record_bytes([BC.seg("s%d" % k, 3, 4242, [(0, 50)], flag=f) for k, f in enumerate((16, 0, 16, 272, 0, 256, 2064, 16, 0))]))
    add("pos_minus_one_on_a_placed_reference", BC.record_bytes(shuffled(
        [BC.seg("m%d" % k, 2, p, [(0, 20)] if p >= 0 else [], flag=f) for k, (p, f) in enumerate(((0, 0), (-1, 4), (1, 16), (-1, 20), (0, 16), (300, 0), (-1, 4)))] +
        [BC.seg("other", 1, 0, [(0, 20)]), BC.seg("tail", -1, -1, [], flag=4)], 53)))
    scattered = BC.random_records(54, 120, (0, 5), LENS, n_unplaced=15) + [BC.seg("np%d" % k, -1, 100 + 7 * (k % 4), [], flag=4 | (16 if k & 1 else 0)) for k in range(12)]
    add("unplaced_scattered", BC.record_bytes(shuffled(scattered, 55)), cuts=1500)
    hdr = header()
    add("record_ends_at_the_block_edge", shuffled(padded_to(hdr, _ascending(56, 900), 65280), 57), hdr=hdr)
    add("length_field_straddles_the_block_edge", shuffled(padded_to(hdr, _ascending(58, 900), 65280 - 2), 59), hdr=hdr)
    long_rec = BC.seg("long", 1, 5000, [(0, 150000)], flag=16)
    around = BC.random_records(60, 60, (1, 3), LENS, n_unplaced=2)
    add("record_longer_than_two_blocks", shuffled(BC.record_bytes(around) + [FB.record_bytes(long_rec, [], qual=bytes(30 + k % 11 for k in range(150000)))], 61), cuts=40000)
    rng = random.Random(62)
    add("records_of_36_to_40_bytes", [tiny_record("t" * (3 + k % 5), rng.choice((0, 1, 1, 3, -1)), rng.randrange(-1, 40), rng.choice((0, 16, 4))) for k in range(700)], cuts=997)
    cig = []
    for k, n_ops in enumerate((3, 4096, 4097, 1, 65535, 2)):
        cig.append(BC.seg("t%d" % k, 3, 1000 + 700 * (5 - k), [((0, 2, 0, 3, 7, 1, 8)[i % 7], 1 + i % 3) for i in range(n_ops)], flag=(0, 16)[k % 2]))
    add("long_cigars_and_a_cg_tag", BC.record_bytes(shuffled(cig + BC.long_cg_records(), 63)), cuts=30011)
    add("blocks_cut_records_anywhere", BC.record_bytes(shuffled(mid, 64)), cuts=BC.cuts_at_record_starts(4, 9))
    few = BC.record_bytes(shuffled(BC.random_records(65, 25, (1, 3), LENS, n_unplaced=2), 66))
    for name, text, pad in (("header_so_queryname", "@HD\tVN:1.6\tSO:queryname\n" + sq_lines(), 0),
                            ("header_so_unsorted_go_query", "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:unsorted:x\n" + sq_lines() + "@CO\tSO:queryname stays here\n", 0),
                            ("header_hd_without_so", "@HD\tVN:1.5\n" + sq_lines(), 0),
                            ("header_without_hd", sq_lines() + "@PG\tID:x\n", 0),
                            ("header_nul_padded", "@HD\tVN:1.6\tGO:none\n" + sq_lines(), 37),
                            ("header_without_text", "", 0)):
        add(name, few, hdr=header(text, pad=pad))
    return out


def definition(case):
    """-> (the sorted stream, the permutation) of a case by svim_amd/bamsort.py"""
    body, perm = bamsort.sort_records(b"".join(case["records"]), case["n_ref"])
    return bamsort.sorted_header(case["header"]) + body, perm


def large_shuffled_file(path, seed=71):
    """the records of bai_cases.large_file (150 500 short records) in a seeded random order -> (header, record bytes in file order as one array of rows)"""
    import numpy as np
    tmp = path + ".sorted"
    m = BC.large_file(tmp)
    raw = bamsort.inflate(tmp)
    os.remove(tmp)
    hdr, n_ref, at = bamsort.split_header(raw)
    recs = bamsort.split_records(raw[at:], n_ref)
    assert len(recs) == m
    order = np.random.default_rng(seed).permutation(m)
    recs = [recs[k] for k in order]
    raw = hdr + b"".join(recs)
    with open(path, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(FB.bgzf_block(raw[lo:lo + 0xff00], 1, zlib.Z_DEFAULT_STRATEGY))
        fh.write(FB.EOF_BLOCK)
    return dict(path=path, header=hdr, records=recs, n_ref=n_ref)
