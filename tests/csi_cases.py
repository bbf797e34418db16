"""Files, texts, row tables and regions for the CSI index (svim_amd/csi.py, the host builds, csrc/bamindex.hip and csrc/textindex.hip with SVX_INDEX_CSI), on
top of tests/bai_cases.py and tests/text_index_cases.py: what lies beyond 2^29, and row tables cut to the edges of the running maximum's tiles.
tests/test_csi.py holds the definition and the host builds to them on the CPU, tests/test_gpu_csi.py the device builds on the GPU.

Test infrastructure only."""
import os
import random

import bai_cases as BC
import text_index_cases as TIC

RMAX_TILE = 2048          # BINIDX_T * BINIDX_RMAX_ITEMS of csrc/binidx_kernels.hpp (tests/test_csi.py reads the #defines and checks the two agree)
VCF, BED = TIC.VCF, TIC.BED
HUGE_REFS, HUGE_LENS = ["small", "huge", "empty", "tail"], [50000, (1 << 31) - 1, 70000, 1 << 30]


def near_2_31_file(path):
    """records near 2^31 - 1, the largest position a BAM holds: leaf bins at and above 65 536 at depth 6, an end beyond 2^31, a reference without records"""
    top = (1 << 31) - 1
    recs = [BC.seg("a", 0, 100, [(0, 50)]), BC.seg("b", 1, 1000, [(0, 50)]), BC.seg("c", 1, (1 << 29) - 20, [(0, 50)]), BC.seg("d", 1, (1 << 29) + 500, [(0, 50)]),
            BC.seg("f", 1, 65536 << 14, [(0, 100)]), BC.seg("e", 1, (1 << 30) + 77, [(0, 30), (3, 1 << 20), (0, 30)]), BC.seg("g", 1, (65536 << 14) + 120, [(0, 100)]),
            BC.seg("h", 1, (100000 << 14) + 5, [(0, 70)]), BC.seg("i", 1, top - 5000, [(0, 100)]), BC.seg("j", 1, top - 300, [(0, 200)]),
            BC.seg("k", 1, top - 10, [(0, 5), (3, 40000), (0, 5)]), BC.seg("l", 3, 12, [(0, 20)]), BC.seg("m", 3, (1 << 30) - 64, [(0, 64)]),
            BC.seg("n", -1, -1, [], flag=4, mapq=0)]
    BC.write_file(path, HUGE_REFS, HUGE_LENS, BC.record_bytes(recs), 0xff00)
    return len(recs)


def beyond_texts():
    """(name, preset, text, depth): texts that a .tbi refuses"""
    v = TIC._vcf
    out = [("vcf_pos_600M", VCF, "\n".join([v("chr1", 100, "SVTYPE=DEL;END=900"), v("chr1", 600_000_000, "SVTYPE=DEL;END=600000400"), v("chr2", 5, "END=6")]) + "\n", 6),
           ("vcf_pos_5e9", VCF, "\n".join([v("chrA", 70000, "END=70100"), v("chrA", 5_000_000_000, "SVTYPE=INS"), v("chrA", 5_000_000_000, "END=5000100000"),
                                           v("chrB", 1 << 29, "END=%d" % ((1 << 29) + 1))]) + "\n", 7),
           ("bed_end_2_40", BED, "chr1\t5\t60\ta\nchr1\t1000\t%d\tb\nchr1\t%d\t%d\tc\nchr1\t%d\t%d\td\nchr2\t0\t1\te\n" % (1 << 35, 1 << 33, (1 << 33) + 10, (1 << 40) - 9, 1 << 40), 9),
           ("bed_one_past_2_29", BED, "chr1\t5\t536870913\n", 6)]
    return [(n, p, t.encode(), d) for n, p, t, d in out]


def two_file_texts():
    """two BED texts of different depths, for one call that indexes both: (text, depth) each"""
    return [(b"chr1\t5\t60\ta\nchr1\t70000\t70010\tb\n", 5), (("chr1\t5\t60\ta\nchr1\t%d\t%d\tb\nchr9\t1\t2\tc\n" % ((1 << 38) + 3, (1 << 38) + 50)).encode(), 9)]


def random_rows(seed, n, n_ref, top_bits=32, span_bits=30, unplaced=0.02):
    """a seeded row table in coordinate order as bai_cases.random_rows gives it, with positions up to 2^min(top_bits, 31) and ends up to 2^span_bits past them"""
    rng = random.Random(seed)
    n_un = int(n * unplaced)
    keys = sorted((rng.randrange(n_ref), rng.randrange(0, min(1 << top_bits, (1 << 31) - 1))) for _ in range(n - n_un))
    rows, v = [], (rng.randrange(1000) << 16) | rng.randrange(65536)
    for tid, pos in keys:
        r = rng.random()
        span = 1 if r < 0.05 else rng.randrange(1, 3000) if r < 0.9 else rng.randrange(1, 1 << 20) if r < 0.995 else rng.randrange(1, 1 << span_bits)
        rows.append((tid, pos, pos + span, rng.choice((0, 16, 4, 256, 2048, 1024)), v))
        v += (rng.randrange(1, 5000) << 16) if rng.random() < 0.1 else rng.randrange(40, 700)
    for _ in range(n_un):
        rows.append((-1, -1, 0, 4, v))
        v += rng.randrange(40, 700)
    return rows, ((v >> 16) + 1) << 16


def group_rows(seed, n, top=1 << 33, span=1 << 30, first_is_largest=False):
    """the rows (beg, end, vbeg, vend) of one group, begs ascending up to `top`, ends up to `span` past them; first_is_largest: the first row ends behind all"""
    rng = random.Random(seed)
    begs = sorted(rng.randrange(top) for _ in range(n))
    rows, v = [], rng.randrange(1 << 30)
    for k, beg in enumerate(begs):
        end = beg + 1 + (rng.randrange(span) if rng.random() < 0.1 else rng.randrange(5000))
        if first_is_largest and k == 0:
            end = top + span + 7
        nxt = v + rng.randrange(30, 90000)
        rows.append((beg, end, v, nxt))
        v = nxt
    return rows


def regions(seed, rows, n_ref, count, top=1 << 31):
    """bai_cases.regions, extended: some regions anywhere up to `top` (beyond 2^29), some on the 16 kb window edges up there"""
    rng = random.Random(seed)
    out = BC.regions(seed, rows, n_ref, count - count // 4)
    for _ in range(count // 4):
        beg = rng.randrange(0, top)
        if rng.random() < 0.5:
            beg = (beg >> 14) << 14
        out.append((rng.randrange(max(1, n_ref)), beg, beg + rng.choice((1, 2, 100, 1 << 14, 100000, 1 << 22, 1 << 30))))
    return out


def text_regions(seed, text, preset, count):
    """seeded regions (contig, beg, end) around the records of a text, on window edges, and anywhere up to 2^41"""
    from svim_amd import tabix
    rng = random.Random(seed)
    recs = [r for r in (tabix.parse_line(l, preset) for l in text.split(b"\n")) if r is not None]
    out = []
    for _ in range(count):
        kind = rng.random()
        if recs and kind < 0.7:
            name, b, e = rng.choice(recs)
            beg = max(0, rng.choice((b, e)) + rng.randrange(-2000, 2000))
        else:
            name, beg = (rng.choice(recs)[0] if recs else b"chr1"), rng.randrange(0, 1 << 41)
        if kind > 0.85:
            beg = (beg >> 14) << 14
        out.append((name, beg, beg + rng.choice((1, 2, 100, 5000, 1 << 14, 1 << 22, 1 << 34))))
    return out


def tile_edge_file(path, n_rows, group_starts, first_is_largest=()):
    """n_rows records of 1M over the references of a header of len(group_starts) + 1 contigs: reference t starts at row group_starts[t] (row 0 starts reference
    0).  A group in first_is_largest has a first record that ends behind every other of it -> the starts"""
    import numpy as np
    import zlib
    import foreign_bam as FB
    starts = [0] + sorted(group_starts)
    n_ref = len(starts)
    tid = np.zeros(n_rows, dtype=np.int32)
    for t, s in enumerate(starts):
        tid[s:] = t
    pos = np.zeros(n_rows, dtype=np.int32)
    for t, s in enumerate(starts):
        e = starts[t + 1] if t + 1 < n_ref else n_rows
        pos[s:e] = 1000 + 37 * np.arange(e - s)
    span = np.full(n_rows, 25, dtype=np.uint32)
    for t in first_is_largest:
        span[starts[t]] = 900000
    rec = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                    ("l_seq", "<i4"), ("next_tid", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S8"), ("cigar", "<u4", 3), ("seq", "u1", 5), ("qual", "u1", 10)])
    a = np.zeros(n_rows, dtype=rec)
    a["block_size"], a["tid"], a["pos"], a["l_read_name"], a["mapq"], a["l_seq"] = rec.itemsize - 4, tid, pos, 8, 60, 10
    a["next_tid"], a["next_pos"] = -1, -1
    a["name"] = np.char.zfill(np.arange(n_rows).astype("S7"), 7)
    a["cigar"][:, 0], a["cigar"][:, 1], a["cigar"][:, 2] = 5 << 4, (span << 4) | 3, 5 << 4
    a["n_cigar"] = 3
    a["seq"], a["qual"] = 0x12, 30
    raw = FB.header_bytes(["t%d" % t for t in range(n_ref)], [1 << 24] * n_ref) + a.tobytes()
    with open(path, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(FB.bgzf_block(raw[lo:lo + 0xff00], 1, zlib.Z_DEFAULT_STRATEGY))
        fh.write(FB.EOF_BLOCK)
    return starts


def tile_edge_cases(dirpath):
    """(name, path, first-is-largest groups): row counts of tile - 1, tile, tile + 1 and 2 tile + 1; groups that start at, one before and one after a tile's first
    row; a group over three tiles whose largest end is its first row's; a one-row group"""
    T = RMAX_TILE
    out = []
    for name, n, starts, big in (("rows_tile_minus_1", T - 1, [7], ()), ("rows_tile", T, [7], ()), ("rows_tile_plus_1", T + 1, [7], ()), ("rows_two_tiles_plus_1", 2 * T + 1, [T + 9], ()),
                                 ("group_at_tile_start", 3 * T, [T, 2 * T], (1,)), ("group_one_before_tile_start", 3 * T, [T - 1, 2 * T - 1], (1,)),
                                 ("group_one_after_tile_start", 3 * T, [T + 1, 2 * T + 1], (1,)), ("group_over_three_tiles", 4 * T + 5, [100, 3 * T + 300], (1,)),
                                 ("one_row_groups", T + 3, [5, 6, T - 1, T, T + 2], (0, 2))):
        path = os.path.join(dirpath, name + ".bam")
        tile_edge_file(path, n, starts, big)
        out.append((name, path, big))
    return out
