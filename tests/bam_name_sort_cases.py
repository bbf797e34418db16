"""Corner files for the query-name order of the BAM sort (svim_amd/bamsort.py: name_key; csrc/bamsort_host.cpp: svx_bam_sort_host_order; csrc/bamsort.hip: the
k_ns_* kernels), built on the record builders of tests/bam_sort_cases.py.  tests/test_bam_name_sort.py holds the definition and the host build to them on the
CPU, tests/test_gpu_bam_name_sort.py the device build on the GPU.  Every case is named for the wrong rule it catches:

    name_lengths             lengths 1 .. 254, each twice with only the last byte different: the word edges of 4- and 8-byte rounds, the longest name
    prefix_chains            a, ab, abc, ... up to 17 bytes, shuffled: "longer first", a wrong zero-fill behind the name's end
    high_bytes               bytes 0x7f / 0x80 / 0xff in names: a signed compare
    padded_names             l_read_name larger than the C string - a NUL inside the field, then junk that must not take part in the order
    rank_order               one name under every name_rank value, twice, shuffled: rank order, then file order
    stable_ties              5 000 records of one name and one rank: the segment never splits, the rounds must still end, the permutation is the identity
    long_shared_prefix       3 000 records whose names share 24 bytes and differ behind them: no split for six rounds, the whole file active
    distinct_first_word      3 000 records with distinct first four bytes: one round
    duplicated_reads         the forty names of bam_sort_cases, every record under flags 0, 2048 and 256 (what the query-name front end groups)
    every_alignment          bam_sort_cases.alignment_records: name starts at every byte alignment
    no_records, one_record
    header_*                 the headers of bam_sort_cases and one whose @HD already carries SS:coordinate:x
    refused()                l_read_name = 0; a name field that runs past block_size; each together with pos < -1 (E_ARG wins)
    large_shuffled_file      bam_sort_cases.large_shuffled_file: radix passes and scans over many tiles, segment heads on tile edges

Test infrastructure only."""
import os
import random
import struct

import bai_cases as BC
import bam_sort_cases as SC
from svim_amd import bamsort

REFS, LENS = SC.REFS, SC.LENS
LENGTHS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 253, 254)
RANK_FLAGS = tuple(r1 | r2 | sup | sec for r2 in (0, 128) for r1 in (0, 64) for sup in (0, 2048) for sec in (0, 256))      # every name_rank value once, in ascending order


def name_record(name, tid=1, pos=100, flag=0, field=None):
    """tiny_record with any bytes as the name; field: the whole name field (l_read_name bytes) when it is not the name and one NUL"""
    field = bytes(name) + b"\0" if field is None else bytes(field)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(field), 0, 4680, 0, flag, 0, -1, -1, 0) + field
    return struct.pack("<i", len(body)) + body


def _ascii(rng, n):
    return bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789/_:") for _ in range(n))


def forty_names_duplicated():
    """the records of bam_sort_cases' five_keys_forty_names, each three times: as it is without the secondary and supplementary bits, as a supplementary, as a
    secondary record; shuffled"""
    keys = [(1, 700, 0), (1, 700, 16), (3, 5, 0), (1, 90000, 16), (-1, -1, 0)]
    rng = random.Random(52)
    forty = [BC.seg("name%02d" % k, t, p, [(0, 30 + k)] if t >= 0 else [], flag=f | (4 if t < 0 else 0)) for k, (t, p, f) in enumerate(rng.choice(keys) for _ in range(40))]
    out = []
    for rb in BC.record_bytes(forty):
        flag, = struct.unpack_from("<H", rb, 18)
        for extra in (0, 2048, 256):
            b = bytearray(rb)
            struct.pack_into("<H", b, 18, (flag & ~(2048 | 256)) | extra)
            out.append(bytes(b))
    return SC.shuffled(out, 151)


def build_all(dirpath):
    """writes every corner file into dirpath -> {name: dict(path, header, records: their bytes in file order, n_ref)}"""
    out = {}

    def add(name, rec_bytes, hdr=None, cuts=0xff00):
        hdr = SC.header() if hdr is None else hdr
        path = os.path.join(dirpath, name + ".bam")
        SC.write_raw(path, hdr, rec_bytes, cuts)
        out[name] = dict(path=path, header=hdr, records=list(rec_bytes), n_ref=len(REFS))
    rng = random.Random(141)
    recs = []
    for n in LENGTHS:
        stem = _ascii(rng, n - 1)
        for last in b"zy":                                                    # (the later one in file order sorts first)
            recs.append(name_record(stem + bytes([last]), rng.choice((0, 1, 3)), rng.randrange(5000)))
    add("name_lengths", SC.shuffled(recs, 142), cuts=1999)
    chain = b"abcdefghijklmnopq"
    add("prefix_chains", SC.shuffled([name_record(chain[:k]) for k in range(1, 18)] + [name_record(chain[:k] + b"!") for k in (3, 4, 8)] + [name_record(b"ab"), name_record(b"abcd")], 143))
    high = [b"r\x7f", b"r\x80", b"r\xff", b"r", b"\x80", b"\x7f", b"\xff", b"\xff\x01", b"rrr\x7fx", b"rrr\x80x", b"rrr\xffx", b"rrrAx", b"rrrr\x80", b"rrrr\x7f", b"rrrr\xff\xff\xff\xff\xff", b"rrrr\xff\xff\xff\xff"]
    add("high_bytes", SC.shuffled([name_record(h, flag=f) for h in high for f in (0, 16)], 144))
    padded = [name_record(b"", field=b"pad\0zzz\0"), name_record(b"", field=b"pad\0aaa\0"), name_record(b"pad"), name_record(b"", field=b"pa\0\xff\xff\xff\xff\0"), name_record(b"", field=b"pad\0"),
              name_record(b"", field=b"padd\0\0\0\0"), name_record(b"", field=b"pac\0dddddddd\0"), name_record(b"", field=b"p\0" + b"\x01" * 250 + b"\0"), name_record(b"paddle"),
              name_record(b"", field=b"no_nul_in_the_field"), name_record(b"no_nul_in_the_fiel"), name_record(b"no_nul_in_the_field!"), name_record(b"", field=b"Z" * 255), name_record(b"Z" * 254)]
    add("padded_names", SC.shuffled(padded, 145))
    add("rank_order", SC.shuffled([name_record(b"one_read", k % 4, 10 * k, f | s) for k, (f, s) in enumerate((f, s) for f in RANK_FLAGS for s in (0, 16))], 146))
    add("stable_ties", [name_record(b"the_same_name", rng.choice((0, 1, 3, -1)), rng.randrange(-1, 9000), rng.choice((0, 16, 4, 20, 1024))) for _ in range(5000)], cuts=30011)
    prefix = b"m64011_190830_220126/zmw"
    assert len(prefix) == 24
    add("long_shared_prefix", SC.shuffled([name_record(prefix + b"%d/ccs" % (k * 7919 % 100003), k % 5 - 1 if k % 5 != 3 else 3, k) for k in range(3000)], 147), cuts=50021)
    add("distinct_first_word", SC.shuffled([name_record(b"%04d/tail" % (k * 7 % 3000), 1, k) for k in range(3000)], 148), cuts=40009)
    add("duplicated_reads", forty_names_duplicated())
    add("every_alignment", SC.alignment_records(149, 1200), cuts=997)
    add("no_records", [])
    add("one_record", [name_record(b"only", 4, 12345)])
    few = SC.shuffled([name_record(b"h%02d" % (k % 9), 1, k, (0, 2048, 256)[k % 3]) for k in range(25)], 150)
    for name, text, pad in (("header_so_queryname", "@HD\tVN:1.6\tSO:queryname\n" + SC.sq_lines(), 0),
                            ("header_so_unsorted_go_query", "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:unsorted:x\n" + SC.sq_lines() + "@CO\tSO:queryname stays here\n", 0),
                            ("header_hd_without_so", "@HD\tVN:1.5\n" + SC.sq_lines(), 0),
                            ("header_without_hd", SC.sq_lines() + "@PG\tID:x\n", 0),
                            ("header_nul_padded", "@HD\tVN:1.6\tGO:none\n" + SC.sq_lines(), 37),
                            ("header_without_text", "", 0),
                            ("header_ss_coordinate", "@HD\tVN:1.6\tSO:coordinate\tSS:coordinate:x\n" + SC.sq_lines(), 0)):
        add(name, few, hdr=SC.header(text, pad=pad))
    return out


HEADER_TEXTS = {"header_so_queryname": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n%s",
                "header_so_unsorted_go_query": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n%s@CO\tSO:queryname stays here\n",
                "header_hd_without_so": b"@HD\tVN:1.5\tSO:queryname\tSS:queryname:lexicographical\n%s",
                "header_without_hd": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n%s@PG\tID:x\n",
                "header_nul_padded": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n%s",
                "header_without_text": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n",
                "header_ss_coordinate": b"@HD\tVN:1.6\tSO:queryname\tSS:queryname:lexicographical\n%s"}


def header_text(name):
    """the text the definition must make of the header of case `name`, written out by hand"""
    t = HEADER_TEXTS[name]
    return t % SC.sq_lines().encode() if b"%s" in t else t


def refused():
    """-> [(name, records in file order, the code the sort must refuse them with)]: the bad record lies in the middle, with more than 255 bytes of good
    records behind it"""
    good = [name_record(b"good%02d" % k, 1, 100 + k) for k in range(12)]
    no_name = name_record(b"", field=b"")                                                     # l_read_name = 0
    past = bytearray(name_record(b"abc"))
    past[12] = 200                                                                             # the name field runs past block_size
    exact = bytearray(name_record(b"abc"))
    exact[12] = 5                                                                              # 32 + 5 > block_size = 36, by one byte
    low = name_record(b"low", 1, -2)                                                           # pos < -1 alone: E_RANGE in both orders
    out = [("l_read_name_zero", good[:6] + [no_name] + good[6:], bamsort.E_ARG),
           ("name_past_block_size", good[:6] + [bytes(past)] + good[6:], bamsort.E_ARG),
           ("name_past_block_size_by_one", good[:6] + [bytes(exact)] + good[6:], bamsort.E_ARG),
           ("l_read_name_zero_and_pos_below_minus_one", good[:3] + [low] + good[3:6] + [no_name] + good[6:], bamsort.E_ARG),
           ("name_past_block_size_and_pos_below_minus_one", good[:6] + [bytes(past)] + good[6:9] + [low] + good[9:], bamsort.E_ARG),
           ("pos_below_minus_one", good[:6] + [low] + good[6:], bamsort.E_RANGE)]
    return out


def definition(case):
    """-> (the sorted stream, the permutation) of a case in query-name order by svim_amd/bamsort.py"""
    body, perm = bamsort.sort_records(b"".join(case["records"]), case["n_ref"], "queryname")
    return bamsort.sorted_header(case["header"], "queryname") + body, perm


def parsed(rec):
    """(name, rank) of a record's bytes, parsed here and not by the definition: the field at offset 36, cut at its first NUL; the flag's bits"""
    l_name = rec[12]
    field = rec[36:36 + l_name]
    name = field.split(b"\0", 1)[0]
    flag = rec[18] | (rec[19] << 8)
    first, last, sup, sec = (flag >> 6) & 1, (flag >> 7) & 1, (flag >> 11) & 1, (flag >> 8) & 1
    return name, (last * 2 + first) * 4 + sup * 2 + sec


def large_shuffled_file(path):
    return SC.large_shuffled_file(path)
