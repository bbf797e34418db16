"""Corner files and row tables for the BAM index (svim_amd/bai.py, csrc/bamindex_host.cpp, csrc/bamindex.hip): small coordinate-sorted BAM files whose block
layout is set payload by payload, seeded row tables, seeded regions.  tests/test_bai.py holds the definition and the host build to them on the CPU,
tests/test_gpu_bam_index.py the device build on the GPU.

    block layout  a record that starts exactly at a block start; records that straddle two and three blocks; empty blocks in the middle (at a record start
                  and inside a record); pieces that were concatenated (an end-of-file marker between them, another compression behind it); stored and
                  fixed-Huffman blocks; no end-of-file block
    references    without records at the start, in the middle and at the end of the header; 600 of them with three records (more references than chunks)
    records       secondary, supplementary, duplicate, mapping quality 0, placed but unmapped, reference length 0; intervals that end at and cross 2^14, 2^17,
                  2^20, 2^23 and 2^26, one that covers a thousand windows; a CG-tag CIGAR of more than 65 535 operations; unplaced records at the tail
    files         unplaced records only; no record at all; one record; 150 000 short records (large_file: beyond the table's first capacity, the scans' tile
                  and the sort's one-workgroup form)

Test infrastructure only."""
import os
import random
import zlib

import foreign_bam as FB
from svim_amd import records

REFS = ["c0", "c1", "c2", "c3", "c4", "c5"]
LENS = [1 << 20, (1 << 27) + 4000, 5000, 1 << 22, 1 << 21, 70000]
DEFAULT = ((6, zlib.Z_DEFAULT_STRATEGY),)


def seg(name, tid, pos, cigar, flag=0, mapq=60, tags=None):
    a = records.AlignedSegment()
    a.query_name, a.flag, a.reference_id, a.reference_start, a._mapq = name, flag, tid, pos, mapq
    a._cigar = list(cigar)
    n = sum(l for o, l in cigar if o in (0, 1, 4, 7, 8))
    a._seq = ("ACGT" * (n // 4 + 1))[:n] if n else ""
    a._tags = dict(tags or {})
    a.next_reference_id, a.next_reference_start, a.template_length = -1, -1, 0
    return a


def random_cigar(rng, big=False):
    ops = [(4, rng.randrange(1, 30))] if rng.random() < 0.3 else []
    for _ in range(rng.randrange(1, 40 if big else 8)):
        ops.append((0, rng.randrange(1, 400 if big else 120)))
        ops.append((rng.choice((1, 2, 2, 3, 7, 8)), rng.randrange(1, 60)))
    ops.append((0, rng.randrange(1, 90)))
    if rng.random() < 0.2:
        ops.append((5, rng.randrange(1, 50)))
    return ops


def random_records(seed, n, tids, lens, n_unplaced=0, big_every=0):
    """n placed records over the references `tids` in coordinate order - flags and mapping qualities of every kind, a placed unmapped record and one of
    reference length 0 now and then - and n_unplaced unplaced ones behind them"""
    rng = random.Random(seed)
    per = sorted((rng.choice(tids), rng.randrange(0, 1 << 30)) for _ in range(n))
    out = []
    for k, (tid, r) in enumerate(per):
        pos = r % max(1, min(lens[tid] - 30000, 400000))
        out.append((tid, pos, k))
    out.sort()
    recs = []
    for tid, pos, k in out:
        kind = rng.random()
        flag = rng.choice((0, 16, 256, 2048, 1024, 272, 2064))
        if kind < 0.04:
            recs.append(seg("u%d" % k, tid, pos, [], flag=4 | (flag & 16), mapq=0))                 # placed by its mate, unmapped
        elif kind < 0.08:
            recs.append(seg("z%d" % k, tid, pos, [(4, 20), (1, 35), (4, 5)], flag=flag))            # no reference length
        else:
            big = big_every and k % big_every == 0
            recs.append(seg("r%d" % k, tid, pos, random_cigar(rng, big), flag=flag, mapq=rng.choice((0, 3, 20, 60))))
    for k in range(n_unplaced):
        recs.append(seg("n%d" % k, -1, -1, [], flag=4, mapq=0))
    return recs


def record_bytes(recs):
    return [FB.record_bytes(a, [(t, "Z" if isinstance(v, str) else "i", v) for t, v in a._tags.items()]) for a in recs]


def write_file(path, refs, lens, rec_bytes, cuts, deflate=DEFAULT, empty_after=(), eof=True):
    """cuts: a number (the stream cut every that many bytes) or a function (stream length, record start offsets) -> ascending cut offsets.  empty_after:
    indexes of data blocks behind which an end-of-file marker is written.  -> number of data blocks"""
    raw = FB.header_bytes(refs, lens)
    starts = []
    for rb in rec_bytes:
        starts.append(len(raw))
        raw += rb
    at = list(range(0, len(raw), cuts)) if isinstance(cuts, int) else [0] + [c for c in cuts(len(raw), starts) if 0 < c < len(raw)]
    at = sorted(set(at)) + [len(raw)]
    k = 0
    with open(path, "wb") as fh:
        for a, b in zip(at, at[1:]):
            for lo in range(a, b, 0xff00):
                fh.write(FB.bgzf_block(raw[lo:min(b, lo + 0xff00)], *deflate[k % len(deflate)]))
                if k in empty_after:
                    fh.write(FB.EOF_BLOCK)
                k += 1
        if eof:
            fh.write(FB.EOF_BLOCK)
    return k


def cuts_at_record_starts(every, also_inside):
    """a cut in front of every `every`-th record, and one `also_inside` bytes into every (every + 3)-th"""
    def f(n, starts):
        return sorted(set(starts[::every]) | {s + also_inside for s in starts[1::every + 3]})
    return f


def edge_records():
    """one reference: intervals that end exactly at and one base beyond 2^14, 2^17, 2^20, 2^23 and 2^26, a record over a thousand windows, records on both sides"""
    items = []
    for k in (14, 17, 20, 23, 26):
        edge = 1 << k
        items += [(edge - 150, [(0, 150)]), (edge - 150, [(0, 100), (2, 51)]), (edge - 40, [(0, 20), (3, 30), (0, 10)]), (edge - 1, [(0, 1)]), (edge - 1, [(0, 2)]),
                  (edge, [(0, 77)]), (edge - 3000, [(0, 50), (3, 2950 + k), (0, 50)])]
    items.append((5 << 14, [(0, 30), (3, 1000 << 14), (0, 30)]))
    items.append(((1 << 27) + 100, [(0, 3000)]))
    items.sort(key=lambda x: x[0])
    return [seg("e%d" % k, 1, pos, cig) for k, (pos, cig) in enumerate(items)]


def long_cg_records():
    import helpers as H
    short, long_rec, _ = H.long_cigar_records()
    for a in (short, long_rec):
        a.reference_id = 3
        a.next_reference_id, a.next_reference_start, a.template_length = -1, -1, 0
    tail = seg("behind", 3, long_rec.reference_start + 5, [(0, 80)])
    return [short, long_rec, tail]


def build_all(dirpath):
    """writes every corner file into dirpath -> [(name, path)]"""
    out = []

    def add(name, recs, cuts, refs=REFS, lens=LENS, **kw):
        path = os.path.join(dirpath, name + ".bam")
        write_file(path, refs, lens, record_bytes(recs), cuts, **kw)
        out.append((name, path))
    big = random_records(11, 2000, (1, 3, 4), LENS, n_unplaced=40, big_every=9)
    add("straddle_two_and_three_blocks", big, 701)
    mid = random_records(12, 400, (1, 3, 4), LENS, n_unplaced=7)
    add("record_at_block_start", mid, cuts_at_record_starts(5, 17))
    add("empty_blocks_in_the_middle", mid, cuts_at_record_starts(4, 9), empty_after=(1, 2, 7, 8, 30, 31, 32))
    add("concatenated_pieces", mid, cuts_at_record_starts(60, 100), empty_after=(3,), deflate=((6, zlib.Z_DEFAULT_STRATEGY),) * 4 + ((1, zlib.Z_FILTERED),) * 40)
    add("stored_and_fixed_blocks", mid, 3001, deflate=((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)))
    add("no_end_of_file_block", mid, 5000, eof=False)
    add("references_without_records", random_records(13, 300, (1, 3, 4), LENS), 2000)
    add("first_and_last_reference_only", random_records(14, 120, (0, 5), LENS, n_unplaced=3), 1500)
    add("bin_edges", edge_records(), 997)
    add("cg_tag_long_cigar", long_cg_records(), 40000)
    add("unplaced_tail", random_records(15, 50, (2,), LENS, n_unplaced=200), 800)
    add("unplaced_only", random_records(16, 0, (1,), LENS, n_unplaced=60), 600)
    add("no_records", [], 0xff00)
    add("one_record", [seg("only", 4, 12345, [(0, 100)])], 0xff00)
    return out


LARGE_REFS, LARGE_LENS = ["L0", "Lempty", "L1", "L2"], [1 << 27, 50000, 1 << 27, 1 << 27]


def large_file(path, n=150000, n_unplaced=500, seed=31):
    """n short placed records (5M kN 5M: one in ten skips up to 100 000 bases and lands in a higher bin, between its neighbours' chunks) spread over three
    references of 2^27 bases, so that most 16 kb windows hold a chunk of their own, and an unplaced tail.  Records of one size, laid out with numpy"""
    import numpy as np
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.choice(np.array([0, 2, 3], dtype=np.int32), n))
    pos = rng.integers(0, (1 << 27) - 200000, n).astype(np.int32)
    order = np.lexsort((pos, tid))
    tid, pos = tid[order], pos[order]
    skip = np.where(rng.random(n) < 0.1, rng.integers(1, 100000, n), 1).astype(np.uint32)
    flag = rng.choice(np.array([0, 16, 256, 2048, 1024, 4], dtype=np.uint16), n)
    tid = np.concatenate([tid, np.full(n_unplaced, -1, dtype=np.int32)])
    pos = np.concatenate([pos, np.full(n_unplaced, -1, dtype=np.int32)])
    skip = np.concatenate([skip, np.ones(n_unplaced, dtype=np.uint32)])
    flag = np.concatenate([flag, np.full(n_unplaced, 4, dtype=np.uint16)])
    m = n + n_unplaced
    rec = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                    ("l_seq", "<i4"), ("next_tid", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S8"), ("cigar", "<u4", 3), ("seq", "u1", 5), ("qual", "u1", 10)])
    a = np.zeros(m, dtype=rec)
    a["block_size"], a["tid"], a["pos"], a["l_read_name"], a["mapq"], a["flag"], a["l_seq"] = rec.itemsize - 4, tid, pos, 8, 60, flag, 10
    a["next_tid"], a["next_pos"] = -1, -1
    a["name"] = np.char.zfill(np.arange(m).astype("S7"), 7)                   # (S8: the eighth byte is the name's NUL)
    a["cigar"][:, 0], a["cigar"][:, 1], a["cigar"][:, 2] = 5 << 4, (skip << 4) | 3, 5 << 4
    a["n_cigar"][:n] = 3
    a["seq"], a["qual"] = 0x12, 30
    unplaced = a[n:].copy()
    parts = [FB.header_bytes(LARGE_REFS, LARGE_LENS), a[:n].tobytes()]
    for r in unplaced:                                                        # (an unplaced record has no CIGAR: 12 bytes shorter)
        b = bytearray(r.tobytes())
        del b[44:56]
        b[0:4] = (len(b) - 4).to_bytes(4, "little")
        parts.append(bytes(b))
    raw = b"".join(parts)
    with open(path, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(FB.bgzf_block(raw[lo:lo + 0xff00], 1, zlib.Z_DEFAULT_STRATEGY))
        fh.write(FB.EOF_BLOCK)
    return m


def many_references_file(dirpath, n_ref=600):
    """three records in a header of 600 references: more references than chunks, by more than one block of lanes of the kernel that serves both -> (name, path)"""
    path = os.path.join(dirpath, "many_references_few_records.bam")
    recs = [seg("a", 0, 10, [(0, 50)]), seg("b", n_ref // 2, 70000, [(0, 50)]), seg("c", n_ref - 1, 5, [(0, 20000)])]
    write_file(path, ["r%d" % k for k in range(n_ref)], [100000] * n_ref, record_bytes(recs), 0xff00)
    return "many_references_few_records", path


def swapped_file(path):
    """two records of one reference swapped: not in coordinate order"""
    recs = random_records(21, 200, (1, 3), LENS, n_unplaced=4)
    k = next(i for i in range(50, 199) if recs[i].reference_id == recs[i + 1].reference_id and recs[i].reference_start < recs[i + 1].reference_start)
    recs[k], recs[k + 1] = recs[k + 1], recs[k]
    write_file(path, REFS, LENS, record_bytes(recs), 3000)


def beyond_range_file(path):
    """a header contig of 2^29 + 70 000 with a record that ends beyond 2^29"""
    refs, lens = ["small", "huge"], [50000, (1 << 29) + 70000]
    recs = [seg("a", 0, 100, [(0, 50)]), seg("b", 1, 1000, [(0, 50)]), seg("c", 1, (1 << 29) - 20, [(0, 50)]), seg("d", 1, (1 << 29) + 500, [(0, 50)])]
    write_file(path, refs, lens, record_bytes(recs), 0xff00)


def random_rows(seed, n, n_ref, unplaced=0.02):
    """a seeded row table in coordinate order (columns as lists): tid, pos, end, flag, vbeg, and v_end"""
    rng = random.Random(seed)
    n_un = int(n * unplaced)
    keys = sorted((rng.randrange(n_ref), rng.randrange(0, 1 << 28)) for _ in range(n - n_un))
    rows, v = [], (rng.randrange(1000) << 16) | rng.randrange(65536)
    for tid, pos in keys:
        r = rng.random()
        span = 1 if r < 0.05 else rng.randrange(1, 3000) if r < 0.9 else rng.randrange(1, 1 << 20) if r < 0.995 else rng.randrange(1, 1 << 27)
        rows.append((tid, pos, min(pos + span, 1 << 29), rng.choice((0, 16, 4, 256, 2048, 1024)), v))
        v += (rng.randrange(1, 5000) << 16) if rng.random() < 0.1 else rng.randrange(40, 700)
    for _ in range(n_un):
        rows.append((-1, -1, 0, 4, v))
        v += rng.randrange(40, 700)
    return rows, ((v >> 16) + 1) << 16


def regions(seed, rows, n_ref, count):
    """seeded regions (tid, beg, end): most around the rows' own intervals, some anywhere, some on the 16 kb window edges"""
    rng = random.Random(seed)
    placed = [r for r in rows if r[0] >= 0]
    out = []
    for k in range(count):
        kind = rng.random()
        if placed and kind < 0.7:
            r = rng.choice(placed)
            anchor = rng.choice((max(r[1], 0), r[2]))
            beg = max(0, anchor + rng.randrange(-2000, 2000))
            tid = r[0]
        else:
            tid, beg = rng.randrange(max(1, n_ref)), rng.randrange(0, 1 << 27)
        if kind > 0.9:
            beg = (beg >> 14) << 14
        out.append((tid, beg, beg + rng.choice((1, 2, 100, 5000, 1 << 14, 100000, 1 << 22))))
    return out
