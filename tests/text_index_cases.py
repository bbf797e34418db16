"""Shared by tests/test_tabix.py and tests/test_gpu_text_index.py: the texts the tabix index is built of (svx_text_index), their block tables, and the checks
of an index against the lines it describes."""
import numpy as np

import text_gz_cases as TC
from svim_amd import tabix

BLOCK = TC.BLOCK
VCF, BED = tabix.VCF, tabix.BED


def seeded_bed_text(n=5000, seed=11):
    """a sorted BED text over 6 contigs: mostly short intervals, some that span one or several bin levels, a contig with a single line"""
    rng = np.random.default_rng(seed)
    lines = []
    for c in ("chr1", "chr2", "chr3", "chr10", "chrX"):
        rows = []
        for _ in range(n // 5):
            beg = int(rng.integers(0, 60_000_000))
            span = int(rng.choice([50, 400, 3000, 20_000, 200_000, 3_000_000, 40_000_000], p=[0.4, 0.3, 0.15, 0.08, 0.04, 0.02, 0.01]))
            rows.append((beg, beg + 1 + int(rng.integers(0, span))))
        for beg, end in sorted(rows):
            lines.append("%s\t%d\t%d\tsvim.DEL.%d;%.2f;%d\t%d\tm64011_190830_220126/%d/ccs" % (c, beg, end, len(lines), float(rng.random()), int(rng.integers(1, 9)),
                                                                                         int(rng.integers(1, 60)), int(rng.integers(1, 10 ** 6))))
    lines.append("chrY\t5\t6\tlast\t1\tr")
    return ("\n".join(lines) + "\n").encode()


def _vcf(contig, pos, info="SVTYPE=DEL", ref="N", tail="\tGT:DP:AD\t./.:.:.,."):
    return "%s\t%d\tsvim.DEL.1\t%s\t<DEL>\t7\tPASS\t%s%s" % (contig, pos, ref, info, tail)


def corner_texts():
    """(name, preset, text bytes) of the corners the issue names; all of them have an index"""
    out = []
    long_reads = ",".join("m64011_190830_220126/%d/ccs" % k for k in range(5000))                  # > 2 blocks of one line
    assert len(long_reads) > 2 * BLOCK
    out.append(("long_line", VCF, "\n".join([_vcf("chr1", 100, "SVTYPE=DEL;END=900"), _vcf("chr1", 2000, "SVTYPE=DEL;END=70000;READS=" + long_reads),
                                             _vcf("chr1", 2000, "SVTYPE=INS;READS=" + long_reads + ";END=999999"), _vcf("chr2", 5, "END=6")]) + "\n"))
    first = _vcf("chr1", 100, "SVTYPE=DEL;END=900;READS=")
    first += "r" * (BLOCK - 1 - len(first) - len("\tGT:DP:AD\t./.:.:.,.")) + "\tGT:DP:AD\t./.:.:.,."
    edge = first.replace("\tGT:DP:AD\t./.:.:.,.\tGT:DP:AD\t./.:.:.,.", "\tGT:DP:AD\t./.:.:.,.") + "\n"
    if len(edge) != BLOCK:
        edge = (_vcf("chr1", 100, "SVTYPE=DEL;END=900;READS=" + "r" * BLOCK))[:BLOCK - 1] + "\n"
    assert len(edge) == BLOCK and edge.endswith("\n")
    out.append(("line_ends_at_block_edge", VCF, edge + _vcf("chr1", 300, "SVTYPE=DEL;END=400") + "\n" + _vcf("chr1", 500, "SVTYPE=DEL;END=600") + "\n"))
    out.append(("single_record", VCF, _vcf("chr7", 12345, "SVTYPE=DEL;END=12999") + "\n"))
    out.append(("single_record_no_newline", BED, "chr7\t10\t20"))
    out.append(("spans_level_0", VCF, _vcf("chr1", 1000, "SVTYPE=INV;END=%d" % (1 << 27)) + "\n" + _vcf("chr1", 67108000, "SVTYPE=DEL;END=67109900") + "\n"))
    out.append(("end_before_pos", VCF, _vcf("chr1", 5000, "SVTYPE=DEL;END=100", ref="NACGT") + "\n" + _vcf("chr1", 5000, "SVTYPE=BND;MATEND=9;SVEND=70000") + "\n"))
    out.append(("end_at_2_29", BED, "chr1\t536860000\t%d\tx\n" % (1 << 29)))
    out.append(("end_at_2_29_vcf", VCF, _vcf("chr1", 1, "SVTYPE=INV;END=%d" % (1 << 29)) + "\n"))
    out.append(("header_and_blank_lines", VCF, "##fileformat=VCFv4.2\n#CHROM\tPOS\n" + _vcf("chr1", 10, "END=20") + "\n\n#note\n" + _vcf("chr1", 10, "END=15") + "\n" +
                _vcf("chr01", 3, "END=9") + "\n"))
    out.append(("short_columns", BED, "chr1\n" + "chr1\t7\n" + "chr1\t9\t\n" + "chr2\tx\ty\n"))
    out.append(("empty", BED, ""))
    out.append(("only_comments", VCF, "#a\n#b\n"))
    return [(n, p, t.encode()) for n, p, t in out]


def refused_texts():
    """(name, preset, text, code)"""
    return [("one_past_2_29", BED, b"chr1\t5\t536870913\n", tabix.E_RANGE),
            ("one_past_2_29_vcf", VCF, (_vcf("chr1", 1, "END=%d" % ((1 << 29) + 1)) + "\n").encode(), tabix.E_RANGE),
            ("pos_drops", VCF, (_vcf("chr1", 50, "END=60") + "\n" + _vcf("chr1", 49, "END=60") + "\n").encode(), tabix.E_ORDER),
            ("contig_returns", BED, b"chr1\t5\t6\nchr2\t5\t6\nchr1\t7\t8\n", tabix.E_ORDER),
            ("both", BED, b"chr1\t5\t536870913\nchr1\t4\t6\n", tabix.E_ORDER)]


def tables(text):
    """the BGZF stream of the host build of the encoder and its block table -> (stream, block_coff, block_uoff)"""
    from svim_amd import _lib
    stream = _lib.text_gz_host(text)
    coff, uoff = tabix.block_table(stream)
    assert uoff[-1] == len(text) and all(b - a == BLOCK for a, b in zip(uoff[:-3], uoff[1:-2]))
    return stream, coff, uoff


def python_status(text, preset):
    """0, E_ORDER or E_RANGE by the definition (a block table is not needed for that)"""
    return tabix.check_order(tabix.records(text, [0, 0], [0, len(text)], preset))


def check_structure(ix_bytes, text, coff, uoff, preset, stream_base=0):
    """the definition parses back; every record lies in exactly one chunk of exactly its bin; the chunks of a bin ascend without overlap; every chunk begins
    at a line start; no linear slot is empty -> the parsed index"""
    ix = tabix.parse_index(ix_bytes)
    recs = tabix.records(text, coff, uoff, preset, stream_base)
    starts = {r[3] for r in recs}
    assert (ix["format"], ix["col_seq"], ix["col_beg"], ix["col_end"], ix["meta"], ix["skip"], ix["n_no_coor"]) == tabix._FORMAT[preset] + (ord("#"), 0, 0)
    names = []
    for r in recs:
        if not names or names[-1] != r[0]:
            names.append(r[0])
    assert ix["names"] == names and len(set(names)) == len(names)
    for tid, name in enumerate(names):
        mine = [r for r in recs if r[0] == name]
        bins = ix["bins"][tid]
        for b, chunks in bins.items():
            assert 0 <= b < 37449 and chunks
            for (b0, e0), (b1, e1) in zip(chunks, chunks[1:]):
                assert b0 < e0 <= b1 < e1, (name, b)
            assert all(c[0] in starts and c[0] < c[1] for c in chunks), (name, b)
        for r in mine:
            hits = [(b, c) for b, chunks in bins.items() for c in chunks if c[0] <= r[3] < c[1]]
            assert len(hits) == 1 and hits[0][0] == tabix.reg2bin(r[1], r[2]), (name, r[:3], hits)
        assert ix["pseudo"][tid] == [(mine[0][3], mine[-1][4]), (len(mine), 0)]
        lin = ix["linear"][tid]
        assert len(lin) == 1 + max((r[2] - 1) >> 14 for r in mine)
        assert all(v != 0xffffffffffffffff and v in starts for v in lin) and lin == sorted(lin)
    return ix
