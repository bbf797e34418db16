"""Directed cases for GENOTYPE (csrc/genotype.hip: k_end_prefmax, k_genotype, k_geno_loci, k_geno_call; csrc/alnindex.hip: the prefix maximum of the resident
table; oracle/svx_oracle.c: svo_genotype; SVIM_genotyping.genotype / genotype_calls): a read below, on and above every comparison genotype() of the reference
makes (src/svim/SVIM_genotyping.py:34-94), the 500-alignment cap from both sides, and the shapes at which the device walk takes another step (64-record trips,
2048-record tiles of the max-scan, contig changes).  tests/golden/make_golden_genotype.py runs the reference on them (tests/golden/g_genotype_cases.json.gz) and
stops when the reference disagrees with what a case's author wrote down; tests/test_genotype_cases.py holds the oracle and the table route to that file on the
CPU, tests/test_gpu_genotype_cases.py the device.

A CASE: a family, a name, the lengths of the contigs it owns (every case lives on contigs of its own, so no case can disturb another and contig_first is
exercised across more than 100 contigs), alignment rows [name, flag, contig (the case's own numbering), pos, mapq, ref_len] (ref_len 0: a 30S record, mapped but
without reference span), candidates (type, contig, start, end, member reads, score[, source locus of a DUP_INT]), options that differ from DEFAULTS, what its
author expects per candidate - (ref_reads, alt_reads, genotype) - and `covers`: (comparison, side) pairs for the coverage table.

world() puts all cases into one coordinate-sorted file in a FIXED order: the `walk` family first, because three of its cases need a contig change at the
global records 2047, 2048, 2049, 4096 and 6145 (below, on and above a multiple of 2048).  REFUSED holds what the reference raises on; it is in no parity set.

Test infrastructure only; imports no GPU code."""
import functools
import hashlib
import json
import math

import numpy as np

DEFAULTS = {"min_mapq": 20, "minimum_score": 3, "minimum_depth": 4, "homozygous_threshold": 0.8, "heterozygous_threshold": 0.2}
SPANS = (0, 1, 2, 3, 200, 201, 301, 3999, 4000, 4001, 7001)
MEMBER_SIZES = (0, 1, 2, 63, 64, 65, 1000)
S0 = 10000                   # where a case's locus starts unless the case is about the contig's ends
UNTOUCHED = [".", "./.", None, None]


def call(alt, ref, o):
    """the genotype a case's author expects from the two counts when the case is not about the call itself (those write it down)"""
    total = alt + ref
    if total == 0 or total < o["minimum_depth"]:
        return "./."
    f = alt / total
    return "1/1" if f >= o["homozygous_threshold"] else "0/1" if f >= o["heterozygous_threshold"] else "0/0"


class Case(object):
    def __init__(self, family, name, lengths=(40000,), **options):
        self.family, self.name, self.lengths, self.options = family, name, list(lengths), dict(DEFAULTS, **options)
        self.rows, self.candidates, self.expected, self.covers, self._n = [], [], [], [], 0

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)

    def read(self, pos, ref_len, name=None, flag=0, mapq=60, contig=0):
        """one alignment record; without a name it is a read of its own; -> the read name"""
        if name is None:
            name = "r%d" % self._n
            self._n += 1
        name = "%s/%s" % (self.id, name)
        assert 0 <= pos and pos + max(ref_len, 1) <= self.lengths[contig], (self.id, pos, ref_len)
        self.rows.append([name, flag, contig, pos, mapq, ref_len])
        return name

    def span(self, rs, re, **kw):
        """a record with reference_start rs and reference_end re"""
        return self.read(rs, re - rs, **kw)

    def fillers(self, n, at, **kw):
        """n eligible records of 50 bases from `at` on, one base apart: inside a window that covers them, never supporting a locus 150 or more behind them"""
        return [self.read(at + k, 50, **kw) for k in range(n)]

    def ghost(self, k=1):
        """k member read names that no record of the file has"""
        out = ["%s/ghost%d" % (self.id, self._n + j) for j in range(k)]
        self._n += k
        return out

    def cand(self, typ, start, end, expect, members=(), score=10, contig=0, source=None, gt=None):
        """expect: ref_reads the author expects (None: the candidate stays untouched); alt_reads is the number of distinct member names"""
        self.candidates.append((typ, contig, start, end, list(members), score, source))
        if expect is None:
            self.expected.append(list(UNTOUCHED))
        else:
            alt = len(set(members))
            self.expected.append([expect, alt, gt if gt is not None else call(alt, expect, self.options)])

    def cover(self, *pairs):
        self.covers.extend(pairs)
        return self


# ---- support, DEL / INV --------------------------------------------------------------------------------------------------------------------------------------------
def support_span_cases():
    """minimum_overlap = min((end - start) / 2, 2000) (:69); clause one: reference_start < end - minimum_overlap and reference_end > end + 100; clause two:
    reference_start < start - 100 and reference_end > start + minimum_overlap (:70-71).  Per span and type eight reads, each on or next to one of the four
    thresholds with the other clause false; four of them support.  An odd span puts end - minimum_overlap between two integers: the sides are the integers
    next to it."""
    out = []
    for typ in ("DEL", "INV"):
        for span in SPANS:
            c = Case("support0", "%s_span%d" % (typ, span))
            start, end = S0, S0 + span
            mo2 = min(span, 4000)                                   # twice the minimum overlap
            lo = -((mo2 - 2 * end) // 2)                            # the smallest integer >= end - minimum_overlap
            hi = (2 * start + mo2) // 2                             # the largest integer <= start + minimum_overlap
            # clause one alone (reference_start >= start - 100 keeps clause two false)
            c.span(lo - 1, end + 101, name="a_below")               # supports
            c.span(lo, end + 101, name="a_on")                      # on end - minimum_overlap (even span) or the first integer above it (odd span): does not
            c.span(start - 100, end + 100, name="b_on")             # reference_end on end + 100: does not
            c.span(start - 100, end + 101, name="b_above")          # supports
            # clause two alone (reference_end <= end + 100 keeps clause one false)
            c.span(start - 101, end + 100, name="c_below")          # supports
            c.span(start - 100, end + 100, name="c_on")             # reference_start on start - 100: does not
            c.span(start - 101, hi, name="d_on")                    # on start + minimum_overlap (even) or the last integer below it (odd): does not
            c.span(start - 101, hi + 1, name="d_above")             # supports
            c.cand(typ, start, end, 4)
            odd = span % 2 == 1
            c.cover(("start < end - minimum_overlap", "below"), ("start < end - minimum_overlap", "above" if odd else "on"),
                    ("end > end + 100", "on"), ("end > end + 100", "above"), ("start < start - 100", "below"), ("start < start - 100", "on"),
                    ("end > start + minimum_overlap", "below" if odd else "on"), ("end > start + minimum_overlap", "above"),
                    ("span / 2 against 2000", "below" if span < 4000 else "on" if span == 4000 else "above"), ("half-integer minimum_overlap", "on" if odd else "below"))
            out.append(c)
    return out


# ---- support, INS / DUP_INT ----------------------------------------------------------------------------------------------------------------------------------------
def support_point_cases():
    """reference_start < start - 100 and reference_end > end + 100 with end = start (:45, :74): the candidate's own end plays no part"""
    out = []
    for typ in ("INS", "DUP_INT"):
        c = Case("support1", typ, lengths=(40000, 40000))
        start, end = S0, S0 + 300
        c.span(start - 101, start + 101, name="both")               # supports
        c.span(start - 100, start + 101, name="start_on")           # does not
        c.span(start - 101, start + 100, name="end_on")             # does not
        c.span(start - 150, start + 150, name="not_own_end")        # spans start +- 100 but not the candidate's end + 100 = start + 400: supports
        c.span(start - 500, start + 500, name="wide")               # supports
        for k in range(5):                                          # reads that would support the source locus of the duplication, on the other contig
            c.span(4000 + k, 7000 + k, contig=1)
        c.cand(typ, start, end, 3, members=c.ghost(1), source=(1, 5000, 5300) if typ == "DUP_INT" else None)
        c.cover(("point: start < start - 100", "below"), ("point: start < start - 100", "on"), ("point: end > start + 100", "on"), ("point: end > start + 100", "above"),
                ("point: end is start", "on"))
        if typ == "DUP_INT":
            c.cover(("DUP_INT takes its destination", "on"))
        out.append(c)
    return out


# ---- eligibility ---------------------------------------------------------------------------------------------------------------------------------------------------
def eligibility_cases():
    out = []
    start, end = S0, S0 + 200

    def locus(name, **opts):
        c = Case("eligible", name, **opts)
        out.append(c)
        return c
    for flag, counts in ((0x4, False), (0x100, False), (0x800, True), (0x400, True), (0x10, True)):
        c = locus("supporter_flag_0x%x" % flag)
        c.span(9000, 12000, flag=flag)
        c.span(9001, 12000)
        c.cand("DEL", start, end, 2 if counts else 1, members=c.ghost(3))
        c.cover(("flag 0x%x" % flag, "on"))
    c = locus("supporter_mapq")
    for q in (19, 20, 0, 255):
        c.span(9000, 12000, mapq=q)
    c.cand("DEL", start, end, 2, members=c.ghost(2))
    c.cover(("mapq < min_mapq", "below"), ("mapq < min_mapq", "on"), ("mapq < min_mapq", "above"))
    c = locus("min_mapq_0", min_mapq=0)
    for q in (0, 19, 255):
        c.span(9000, 12000, mapq=q)
    c.cand("INV", start, end, 3, members=c.ghost(1))
    c.cover(("min_mapq 0", "on"))
    c = locus("member_primary_and_supplementary")
    m = c.span(9000, 12000, name="m")
    c.span(9100, 12500, name="m", flag=0x800)
    c.span(9200, 12000)
    c.cand("DEL", start, end, 1, members=[m])
    c.cover(("member read, two records", "on"))
    c = locus("member_absent_from_file")
    c.span(9000, 12000)
    c.cand("DEL", start, end, 1, members=c.ghost(1))
    c.cover(("member absent from the file", "on"))
    c = locus("two_signatures_of_one_read")
    m = c.span(9000, 12000, name="m")
    c.span(9200, 12000)
    c.cand("INS", start, start, 1, members=[m, m])
    c.cover(("two signatures of one read", "on"))
    # member lists of 0 .. 1000 reads, every member with a SUPPORTING record in the window (a lookup that misses one shows in ref_reads); read ids follow file order,
    # so the three supporters that are no members are looked up below all, between two neighbouring and above all entries of the sorted list
    for n in MEMBER_SIZES:
        c = locus("members_%d" % n)
        c.span(50, 12000, name="below_all")
        members = []
        for k in range(n):
            if k == n // 2 and n >= 2:
                c.span(9200 + k // 4, 12000, name="between")
            members.append(c.span(9200 + k // 4, 12000, name="m%d" % k))
        c.span(9890, 12000, name="above_all")
        c.cand("DEL", start, end, 2 + (n >= 2), members=members)
        c.cover(("member list of %d" % n, "on"), ("looked-up id below all", "on"), ("looked-up id above all", "on"))
        if n >= 2:
            c.cover(("looked-up id between two entries", "on"))
    return out


# ---- the set -------------------------------------------------------------------------------------------------------------------------------------------------------
def set_cases():
    out = []
    start, end = S0, S0 + 200

    def locus(name):
        c = Case("set", name)
        out.append(c)
        return c
    c = locus("two_records_same_trip")
    c.span(9000, 12000, name="x")
    c.span(9001, 12000, name="x")
    c.span(9002, 12000)
    c.cand("DEL", start, end, 2)
    c.cover(("one read, two records, one trip", "on"))
    c = locus("two_records_different_trips")
    c.span(9000, 12000, name="x")
    c.fillers(70, 9100)
    c.span(9800, 12000, name="x")
    c.span(9801, 12000)
    c.cand("DEL", start, end, 2)
    c.cover(("one read, two records, two trips", "on"))
    c = locus("primary_plus_supplementary")
    c.span(9000, 12000, name="x")
    c.span(9500, 13000, name="x", flag=0x800)
    c.cand("INS", start, start, 1, members=c.ghost(1))
    c.cover(("one read, primary and supplementary", "on"))
    for n in (63, 64, 65, 500):
        c = locus("distinct_%d" % n)
        for k in range(n):
            c.span(9000 + k, 12000)
        c.cand("DEL", start, end, n, members=c.ghost(2))
        c.cover(("%d distinct supporters" % n, "on"))
    c = locus("500_records_of_250_reads")
    for k in range(500):
        c.span(9000 + k, 12000, name="p%d" % (k % 250), flag=0 if k < 250 else 0x800)
    c.cand("INV", start, end, 250)
    c.cover(("500 supporting records of 250 reads", "on"))
    return out


# ---- the cap -------------------------------------------------------------------------------------------------------------------------------------------------------
def cap_cases():
    """while aln_no < 500 (:56): the supporter sits at reference_start = start - 101 behind the fillers, as the 500th eligible alignment (counted) or the 501st (not)"""
    out = []
    start, end = S0, S0 + 200
    ws = start - 1000

    def finish(c, nth, members=()):
        c.span(start - 101, 12000, name="supporter")
        c.cand("DEL", start, end, 1 if nth == 500 else 0, members=list(members) + c.ghost(4))
        c.cover(("aln_no < 500", "below" if nth == 500 else "on"))
        out.append(c)
        return c
    for nth in (500, 501):
        c = Case("cap", "plain_%d" % nth)
        c.fillers(nth - 1, 9100)
        finish(c, nth)
        # records that do not consume the cap in front of the supporter: members, secondary, placed-unmapped, mapq below min_mapq
        c = Case("cap", "not_counted_interleaved_%d" % nth)
        members = []
        for k in range(nth - 1):
            c.read(9100 + k, 50)
            if k % 100 == 0:
                members.append(c.read(9100 + k, 50, name="member%d" % (k // 200)))
                c.read(9100 + k, 50, flag=0x100)
                c.read(9100 + k, 50, flag=0x4)
                c.read(9100 + k, 50, mapq=19)
        finish(c, nth, members).cover(("member does not consume the cap", "on"), ("secondary does not consume the cap", "on"),
                                      ("placed-unmapped does not consume the cap", "on"), ("low mapq does not consume the cap", "on"))
        # records that do: supplementary, duplicate, reverse, mapq == min_mapq
        c = Case("cap", "counted_kinds_%d" % nth)
        for k in range(nth - 1):
            kind = k % 4
            c.read(9100 + k, 50, flag=(0x800, 0x400, 0x10, 0)[kind], mapq=20 if kind == 3 else 60)
        finish(c, nth).cover(("supplementary consumes the cap", "on"), ("duplicate consumes the cap", "on"), ("reverse consumes the cap", "on"),
                             ("mapq == min_mapq consumes the cap", "on"))
        # records inside the walked index range that fetch does not return: one long record reaches into the window, the short ones behind it end at or before it
        c = Case("cap", "not_fetched_interleaved_%d" % nth)
        c.span(5000, ws + 1, name="reaches_in")                    # fetched, eligible, supports nothing
        for k in range(18):
            c.span(5001 + 190 * k, 5061 + 190 * k, name="short%d" % k)                             # bam_endpos <= ws
        c.span(8940, ws - 1, name="ends_before")
        c.span(8950, ws, name="ends_on")
        c.fillers(nth - 2, 9100)
        finish(c, nth).cover(("walked but not fetched", "on"))
    # the 500th eligible record 63, 64 and 65 records (modulo 64) behind the first fetched one: 499 = 7 * 64 + 51 fillers and 12, 13, 14 secondary records
    for off, n_sec in ((63, 12), (64, 13), (65, 14)):
        for nth in (500, 501):
            c = Case("cap", "offset_%d_%d" % (off, nth))
            for k in range(n_sec):
                c.read(9050 + k, 50, flag=0x100)
            c.fillers(nth - 1, 9100)
            assert (n_sec + 499) % 64 == off % 64
            finish(c, nth).cover(("500th eligible at offset %d" % off, "below" if nth == 500 else "on"))
    # the left edge of the window, observable only through the cap: bam_endpos == ws is not fetched, ws + 1 is (and is the one alignment too many)
    for kind, rows in (("ordinary", ((ws - 50, 50), (ws - 50, 51))), ("30S", ((ws - 1, 0), (ws, 0)))):
        for (pos, ln), side in zip(rows, ("on", "above")):
            c = Case("cap", "window_edge_%s_%s" % (kind, side))
            c.read(pos, ln, name="edge")
            c.fillers(499, 9100)
            c.span(start - 101, 12000, name="supporter")
            c.cand("DEL", start, end, 1 if side == "on" else 0, members=c.ghost(4))
            c.cover(("bam_endpos > start - 1000", side), ("bam_endpos of a record without reference span" if kind == "30S" else "bam_endpos of an ordinary record", side))
            out.append(c)
    return out


# ---- where the walk starts -----------------------------------------------------------------------------------------------------------------------------------------
def behind_a_long_read(c, n_short, clen, typ="DEL"):
    """one long read from 100 over the locus, n_short records behind it that end before the window, the locus: only the running maximum finds the long read"""
    start = clen - 5000
    c.span(100, start + 2000, name="long")
    step = max(1, (start - 1000 - 200 - 60) // max(1, n_short))
    for k in range(n_short):
        c.read(150 + min(k * step, start - 1000 - 200 - 60), 50)
    c.span(start - 300, start + 2000, name="near")
    c.cand(typ, start, start + 200, 2, members=c.ghost(2))
    return c


def walk_cases():
    """In file order.  The first ones are sized so that contigs begin at the global records 2047, 2048 and 2049, and again at 4096 and 6145: one below, on and
    one above a multiple of the 2048-record tile of the resident table's max-scan; the contigs that begin at 2049, 4096 and 6145 start with a long read, so the
    window behind needs the carry of the contig's own first record and nothing of the contig in front."""
    out = []
    c = Case("walk", "first_contig_2047_records", lengths=(60000,))
    c.fillers(2045, 100)
    c.span(59000 - 400, 59900, name="s0")
    c.span(59000 - 101, 59900, name="s1")
    c.cand("DEL", 59000, 59200, 2, members=c.ghost(2))                          # also: a locus within 1000 of the contig's end (we = the contig's length)
    c.cover(("first contig of the file", "on"), ("locus within 1000 of the contig's end", "on"))
    out.append(c)
    for at, side in ((2047, "below"), (2048, "on")):                             # contigs of one record: the next contig begins one record on
        c = Case("walk", "contig_begins_at_record_%d" % at, lengths=(30000,))
        c.span(9000, 12000)
        c.cand("DEL", S0, S0 + 200, 1, members=c.ghost(3))
        c.cover(("contig change at global record 2047 / 2048 / 2049", side))
        out.append(c)
    for name, n_short, covers in (("contig_begins_at_record_2049", 2045, [("contig change at global record 2047 / 2048 / 2049", "above")]),
                                  ("contig_begins_at_record_4096", 2047, [("contig change against the 2048-record tile", "on")]),
                                  ("contig_begins_at_record_6145", 150, [("contig change against the 2048-record tile", "above")])):
        c = behind_a_long_read(Case("walk", name, lengths=(60000,)), n_short, 60000)
        c.cover(*covers)
        out.append(c)
    for n_short, tiles in ((2100, "one"), (4200, "two")):
        c = behind_a_long_read(Case("walk", "long_read_%d_records_before" % n_short, lengths=(120000,)), n_short, 120000, typ="INV")
        c.cover(("long read %s tiles before the window" % tiles, "on"))
        out.append(c)
    c = Case("walk", "no_leak_from_the_contig_in_front", lengths=(100000, 30000))
    c.fillers(20, 8000)
    c.span(9000, 99000, name="ninety_kb")                                       # the last record of its contig
    for k in range(5):
        c.span(10 + k, 500 - k, contig=1)                                       # end at or before the window start of the locus behind them
    c.span(1350, 2000, contig=1)
    c.span(600, 1810, contig=1)
    c.cand("DEL", 1500, 1700, 2, members=c.ghost(2), contig=1)
    c.cand("DEL", 50000, 50200, 1, members=c.ghost(3), contig=0)
    c.cover(("maximum of the contig in front", "on"))
    out.append(c)
    c = Case("walk", "contig_without_records", lengths=(5000,))
    c.cand("DEL", 2000, 2200, 0, members=c.ghost(5))
    c.cand("INS", 2000, 2000, 0)
    c.cover(("contig without records", "on"))
    out.append(c)
    c = Case("walk", "contig_shorter_than_1000", lengths=(800,))
    c.span(100, 700)
    c.span(200, 700)
    c.span(210, 500)                                                            # neither clause
    c.cand("DEL", 300, 400, 2, members=c.ghost(2))
    c.cover(("contig shorter than 1000", "on"), ("start < 1000", "on"))
    out.append(c)
    c = Case("walk", "locus_at_the_contig_start", lengths=(30000,))
    c.span(0, 3000)
    c.span(299, 3000)
    c.span(300, 3000)
    c.cand("DEL", 400, 600, 3, members=c.ghost(1))
    c.cand("INS", 400, 400, 2, members=c.ghost(2))
    c.cover(("locus within 1000 of the contig's start", "on"), ("start < 1000", "on"))
    out.append(c)
    c = Case("walk", "locus_at_the_contig_end", lengths=(30000,))
    c.span(27000, 30000)
    c.span(29599, 30000)
    c.span(29600, 30000)
    c.cand("INS", 29700, 29700, 2, members=c.ghost(2))
    c.cand("DEL", 29700, 29850, 3, members=c.ghost(1))
    c.cover(("locus within 1000 of the contig's end", "on"))
    out.append(c)
    return out


def last_cases():
    """the end of the file: the last contig that has records, and behind it a contig without any"""
    c = Case("walk", "last_contig_with_records", lengths=(30000,))
    c.span(9000, 12000)
    c.span(9899, 10301)
    c.cand("DEL", S0, S0 + 200, 2, members=c.ghost(2))
    c.cover(("last contig of the file", "on"))
    d = Case("walk", "last_contig_without_records", lengths=(30000,))
    d.cand("INV", S0, S0 + 200, 0, members=d.ghost(4))
    d.cover(("last contig of the file", "on"), ("contig without records", "on"))
    return [c, d]


# ---- the call ------------------------------------------------------------------------------------------------------------------------------------------------------
def call_cases():
    """:77-92 from the two counts: alt member names that no record has, ref supporters"""
    out = []

    def counts(name, alt, ref, gt, typ="DEL", score=10, covers=(), **opts):
        c = Case("call", name, **opts)
        for k in range(ref):
            c.span(9000 + k, 12000)
        c.cand(typ, S0, S0 if typ in ("INS", "DUP_INT") else S0 + 200, None if gt is None else ref, members=c.ghost(alt), score=score, gt=gt,
               source=(0, 100, 300) if typ == "DUP_INT" else None)
        c.cover(*covers)
        out.append(c)
        return c
    counts("hom_on_4_of_5", 4, 1, "1/1", covers=[("fraction >= homozygous_threshold", "on")])
    counts("hom_below_4_of_6", 4, 2, "0/1", covers=[("fraction >= homozygous_threshold", "below")])
    counts("hom_above_5_of_6", 5, 1, "1/1", covers=[("fraction >= homozygous_threshold", "above")])
    counts("het_on_1_of_5", 1, 4, "0/1", covers=[("fraction >= heterozygous_threshold", "on")])
    counts("het_below_1_of_6", 1, 5, "0/0", covers=[("fraction >= heterozygous_threshold", "below")])
    counts("het_above_1_of_4", 1, 3, "0/1", covers=[("fraction >= heterozygous_threshold", "above")])
    # quotients that are NOT the double nearest to the decimal threshold: 2 / 3 is 0.6666666666666666, 3 / 10 is 0.3 and not 0.1 + 0.2
    counts("hom_one_ulp_above_2_of_3", 2, 1, "0/1", minimum_depth=3, homozygous_threshold=0.6666666666666667, covers=[("fraction one ulp from the threshold", "below")])
    counts("hom_on_2_of_3", 2, 1, "1/1", minimum_depth=3, homozygous_threshold=0.6666666666666666, covers=[("fraction one ulp from the threshold", "on")])
    counts("het_one_ulp_above_3_of_10", 3, 7, "0/0", heterozygous_threshold=0.30000000000000004, covers=[("fraction one ulp from the threshold", "below")])
    counts("het_on_3_of_10", 3, 7, "0/1", heterozygous_threshold=0.3, covers=[("fraction one ulp from the threshold", "on")])
    counts("depth_on", 2, 2, "0/1", covers=[("total >= minimum_depth", "on")])
    counts("depth_below", 2, 1, "./.", covers=[("total >= minimum_depth", "below")])
    counts("depth_above", 3, 2, "0/1", typ="INV", covers=[("total >= minimum_depth", "above")])
    counts("total_0", 0, 0, "./.", covers=[("total 0", "on")])
    counts("total_0_point", 0, 0, "./.", typ="INS", covers=[("total 0", "on")])
    counts("thresholds_equal_on", 1, 1, "1/1", minimum_depth=2, homozygous_threshold=0.5, heterozygous_threshold=0.5, covers=[("heterozygous == homozygous", "on")])
    counts("thresholds_equal_below", 1, 2, "0/0", minimum_depth=2, homozygous_threshold=0.5, heterozygous_threshold=0.5, covers=[("heterozygous == homozygous", "below")])
    counts("score_one_ulp_below", 2, 2, None, score=math.nextafter(3.0, 0.0), covers=[("score < minimum_score", "below")])
    counts("score_on", 2, 2, "0/1", score=3.0, covers=[("score < minimum_score", "on")])
    counts("score_one_ulp_above", 2, 2, "0/1", typ="DUP_INT", score=math.nextafter(3.0, 4.0), covers=[("score < minimum_score", "above")])
    counts("score_nan", 2, 2, "0/1", score=float("nan"), covers=[("NaN score", "on")])
    counts("score_nan_point", 2, 2, "0/1", typ="INS", score=float("nan"), covers=[("NaN score", "on")])
    return out


# what the reference raises on; kept in no parity set.  (name, case, exception type of the reference, what ours answers instead)
def refused():
    a = Case("refused", "contig_missing_from_the_file")
    a.span(9000, 12000)
    a.cand("DEL", S0, S0 + 200, 0, members=a.ghost(4), contig="absent")
    b = Case("refused", "minimum_depth_0_total_0", minimum_depth=0)
    b.cand("DEL", S0, S0 + 200, 0)
    c = Case("refused", "minimum_depth_negative_total_0", minimum_depth=-1)
    c.cand("INS", S0, S0, 0)
    return [a, b, c]


EXPECTED_RAISES = {"refused/contig_missing_from_the_file": "ValueError", "refused/minimum_depth_0_total_0": "ZeroDivisionError",
                   "refused/minimum_depth_negative_total_0": "ZeroDivisionError"}
# rows of the classes genotype() is never called for (src/svim/svim:164-170): they ride in the candidate table and must come back untouched
EXTRA_TABLE_ROWS = (("DUP_TAN", S0, S0 + 200), ("BND", S0, S0 + 200))

FAMILIES = ("walk", "support0", "support1", "eligible", "set", "cap", "call")


@functools.lru_cache(maxsize=None)
def cases():
    """every case of the parity set in file order (world() puts the refused ones in front of the last two)"""
    out = walk_cases() + support_span_cases() + support_point_cases() + eligibility_cases() + set_cases() + cap_cases() + call_cases() + last_cases()
    assert len({c.id for c in out}) == len(out) and {c.family for c in out} == set(FAMILIES)
    return out


class World(object):
    """all cases, the refused ones too (on contigs of their own), as one coordinate-sorted file"""

    def __init__(self, case_list):
        self.cases = case_list
        self.references, self.lengths, self.first_contig = [], [], {}
        rows = []
        for c in case_list:
            self.first_contig[c.id] = len(self.references)
            per = [[] for _ in c.lengths]
            for r in c.rows:
                per[r[2]].append(r)
            for k, ln in enumerate(c.lengths):
                tid = len(self.references)
                self.references.append("g%03d" % tid)
                self.lengths.append(ln)
                rows += [[r[0], r[1], tid, r[3], r[4], r[5]] for r in sorted(per[k], key=lambda r: r[3])]      # (stable: equal positions keep the author's order)
        self.rows = rows

    def contig_name(self, c, k):
        return k if isinstance(k, str) else self.references[self.first_contig[c.id] + k]

    def candidates(self, c):
        """(type, contig name, start, end, members, score, source locus or None) of one case"""
        return [(t, self.contig_name(c, k), s, e, m, sc, None if src is None else (self.contig_name(c, src[0]), src[1], src[2])) for t, k, s, e, m, sc, src in c.candidates]

    def rows_sha256(self):
        return hashlib.sha256(json.dumps(self.rows, separators=(",", ":")).encode("ascii")).hexdigest()

    def cases_sha256(self):
        """candidates, options and expectations (a NaN score prints as NaN)"""
        text = json.dumps([[c.id, c.lengths, self.candidates(c), sorted(c.options.items()), c.expected] for c in self.cases], separators=(",", ":"))
        return hashlib.sha256(text.encode("ascii")).hexdigest()

    def sam_text(self):
        head = ["@HD\tVN:1.6\tSO:coordinate"] + ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in zip(self.references, self.lengths)]
        body = ["%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*" % (r[0], r[1], self.references[r[2]], r[3] + 1, r[4], "%dM" % r[5] if r[5] else "30S", "*" if r[5] else "A" * 30)
                for r in self.rows]
        return "\n".join(head + body) + "\n"


@functools.lru_cache(maxsize=None)
def world():
    return World(cases()[:-2] + refused() + cases()[-2:])


class RowsIndex(object):
    """SVIM_genotyping.AlignmentIndex of world().rows without the detour through SAM text (tests/test_genotype_cases.py holds it to the real one, column by
    column): what the child process of the mutant test hands the oracle"""

    def __init__(self, w):
        from svim_amd import _abi
        self._abi = _abi
        self.references, self.lengths = list(w.references), list(w.lengths)
        self.name_ids = {}
        for r in w.rows:
            self.name_ids.setdefault(r[0], len(self.name_ids))
        tid = np.asarray([r[2] for r in w.rows], dtype=np.int32)
        self.n, self.n_contig = int(tid.size), len(self.references)
        self.contig_first = np.searchsorted(tid, np.arange(self.n_contig + 1), side="left").astype(np.int64)
        self.contig_len = np.asarray(self.lengths, dtype=np.int64)
        self.pos = np.asarray([r[3] for r in w.rows], dtype=np.int32)
        self.end = np.asarray([r[3] if r[1] & 4 else r[3] + r[5] for r in w.rows], dtype=np.int32)
        self.flag = np.asarray([r[1] for r in w.rows], dtype=np.uint16)
        self.mapq = np.asarray([r[4] for r in w.rows], dtype=np.uint8)
        self.name_id = np.asarray([self.name_ids[r[0]] for r in w.rows], dtype=np.int32)

    def view(self):
        from svim_amd._abi import ptr
        v = self._abi.AlnIndex()
        v.n, v.n_contig = self.n, self.n_contig
        self._keep = [self.contig_first, self.contig_len, self.pos, self.end, self.flag, self.mapq, self.name_id]
        v.contig_first, v.contig_len, v.pos, v.end, v.flag, v.mapq, v.name_id = [ptr(a) for a in self._keep]
        return v


class Sig(object):
    def __init__(self, read):
        self.read = read


class Candidate(object):
    """Quacks like the reference's candidates (src/svim/SVCandidate.py) as far as genotype() looks; a DUP_INT has a source locus of its own"""

    def __init__(self, typ, contig, start, end, members, score, source=None):
        self.type, self.locus, self.members, self.score, self.source = typ, (contig, start, end), [Sig(m) for m in members], score, source
        self.support_fraction, self.genotype, self.ref_reads, self.alt_reads = ".", "./.", None, None

    def get_source(self):
        return self.locus if self.type in ("DEL", "INV") else self.source

    def get_destination(self):
        return self.locus

    def fields(self):
        return [self.support_fraction, self.genotype, self.ref_reads, self.alt_reads]


def expected_fields(e):
    """a case's (ref_reads, alt_reads, genotype) -> the four fields of the golden"""
    if e == UNTOUCHED:
        return list(e)
    ref, alt, gt = e
    return [alt / (alt + ref) if alt + ref else ".", gt, ref, alt]


def option_key(o):
    return tuple(sorted(o.items()))


def table_of(cands, references, read_id):
    """[(type, contig name, start, end, members, score, source)] -> (CandidateTable grouped by class, sig_read_id int32, row of every input candidate).  One
    signature per member; DEL / INV / DUP_TAN rows carry their locus in the source columns, INS rows in the destination columns, DUP_INT rows both, BND rows one
    end in each."""
    from svim_amd import _abi
    cls_of = {n: k for k, n in enumerate(_abi.CAND_NAMES)}
    order = sorted(range(len(cands)), key=lambda k: (cls_of[cands[k][0]], k))
    row_of = {k: r for r, k in enumerate(order)}
    t = _abi.CandidateTable(len(cands), sum(len(c[4]) for c in cands))
    t.std_span[:] = np.nan
    t.std_pos[:] = np.nan
    rid, at = [], 0
    for r, k in enumerate(order):
        typ, contig, start, end, members, score, source = cands[k]
        t.cls[r], t.score[r] = cls_of[typ], score
        tid = references.index(contig)
        if typ in ("DEL", "INV", "DUP_TAN"):
            t.contig[r], t.start[r], t.end[r], t.contig2[r] = tid, start, end, -1
        elif typ == "INS":
            t.contig[r], t.contig2[r], t.start2[r], t.end2[r] = -1, tid, start, end
        elif typ == "DUP_INT":
            t.contig[r], t.start[r], t.end[r] = references.index(source[0]), source[1], source[2]
            t.contig2[r], t.start2[r], t.end2[r] = tid, start, end
        else:
            t.contig[r], t.start[r], t.end[r], t.contig2[r], t.start2[r], t.end2[r] = tid, start, start + 1, tid, end, end + 1
        for m in members:
            t.members[at] = at
            rid.append(read_id(m))
            at += 1
        t.member_off[r + 1] = at
    v = t.view()
    for k in range(6):
        v.class_count[k] = sum(1 for c in cands if cls_of[c[0]] == k)
    t.finish(v)
    return t, np.asarray(rid, dtype=np.int32), [row_of[k] for k in range(len(cands))]


# ---- the coverage table --------------------------------------------------------------------------------------------------------------------------------------------
# every comparison of the issue -> the sides that need a case
_BOTH = ("below", "on")
REQUIRED = {
    "start < end - minimum_overlap": ("below", "on", "above"), "end > end + 100": ("on", "above"), "start < start - 100": ("below", "on"),
    "end > start + minimum_overlap": ("below", "on", "above"), "span / 2 against 2000": ("below", "on", "above"), "half-integer minimum_overlap": ("below", "on"),
    "point: start < start - 100": _BOTH, "point: end > start + 100": ("on", "above"), "point: end is start": ("on",), "DUP_INT takes its destination": ("on",),
    "flag 0x4": ("on",), "flag 0x100": ("on",), "flag 0x800": ("on",), "flag 0x400": ("on",), "flag 0x10": ("on",),
    "mapq < min_mapq": ("below", "on", "above"), "min_mapq 0": ("on",), "member read, two records": ("on",), "member absent from the file": ("on",),
    "two signatures of one read": ("on",), "looked-up id below all": ("on",), "looked-up id above all": ("on",), "looked-up id between two entries": ("on",),
    "one read, two records, one trip": ("on",), "one read, two records, two trips": ("on",), "one read, primary and supplementary": ("on",),
    "500 supporting records of 250 reads": ("on",),
    "aln_no < 500": _BOTH, "member does not consume the cap": ("on",), "secondary does not consume the cap": ("on",), "placed-unmapped does not consume the cap": ("on",),
    "low mapq does not consume the cap": ("on",), "supplementary consumes the cap": ("on",), "duplicate consumes the cap": ("on",), "reverse consumes the cap": ("on",),
    "mapq == min_mapq consumes the cap": ("on",), "walked but not fetched": ("on",),
    "500th eligible at offset 63": _BOTH, "500th eligible at offset 64": _BOTH, "500th eligible at offset 65": _BOTH,
    "bam_endpos > start - 1000": ("on", "above"), "bam_endpos of an ordinary record": ("on", "above"), "bam_endpos of a record without reference span": ("on", "above"),
    "contig change at global record 2047 / 2048 / 2049": ("below", "on", "above"), "contig change against the 2048-record tile": ("on", "above"), "long read one tiles before the window": ("on",), "long read two tiles before the window": ("on",),
    "maximum of the contig in front": ("on",), "contig without records": ("on",), "first contig of the file": ("on",), "last contig of the file": ("on",),
    "contig shorter than 1000": ("on",), "locus within 1000 of the contig's start": ("on",), "locus within 1000 of the contig's end": ("on",), "start < 1000": ("on",),
    "fraction >= homozygous_threshold": ("below", "on", "above"), "fraction >= heterozygous_threshold": ("below", "on", "above"),
    "fraction one ulp from the threshold": _BOTH, "total >= minimum_depth": ("below", "on", "above"), "total 0": ("on",), "heterozygous == homozygous": _BOTH,
    "score < minimum_score": ("below", "on", "above"), "NaN score": ("on",),
}
REQUIRED.update({"member list of %d" % n: ("on",) for n in MEMBER_SIZES})
REQUIRED.update({"%d distinct supporters" % n: ("on",) for n in (63, 64, 65, 500)})


def coverage(case_list):
    """{comparison: {side: [case ids]}}"""
    out = {}
    for c in case_list:
        for name, side in c.covers:
            out.setdefault(name, {}).setdefault(side, []).append(c.id)
    return out
