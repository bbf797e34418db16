"""Directed cases for the split-read decision tree (k_segments, svim_amd/csrc/collect.hip; collect_segments, oracle/svx_oracle.c): one read on each side of
every threshold of analyze_read_segments (src/svim/SVIM_inter.py:24-302) and one exactly on it.  No GPU and no reference needed to import.

A case is a list of reads, a read a list of segments (q_start, q_end, tid, ref_start, reverse, mapq) in READ orientation plus its options.  Every CIGAR is
xS yM zS (H where the segment says so; a reverse segment's clips are written in reference orientation, synth.Segment.clipped_cigar), so ref_end = ref_start +
q_end - q_start and every number the tree compares is the one the case states.  The same records serve both file orders: the primary carries an SA tag (coordinate
mode), the other segments are real supplementary records (query-name mode).

Every case carries the outcome its author expects: the signatures of the main list, in order, as tokens ("DEL", "INS", "INV left_fwd", "DUP_TAN 2 full",
"DUP_INT", "BND fr" = directions fwd / rev after the canonical order).  tests/golden/make_golden_segments.py asserts that the reference agrees before it writes
tests/golden/g_segments_cases.json.gz; tests/test_segments.py and tests/test_gpu_segments.py hold the oracle and the device to that file.

Thresholds of most families: min_sv_size MIN = 40, max_sv_size MAX = 2000, segment_gap_tolerance GAP = 10, segment_overlap_tolerance OVL = 5.
"""
from svim_amd import synth
from svim_amd.records import AlignedSegment, cigar_to_string

REFERENCES = ["chr1", "chr2", "chr10"]               # index order != string order: "chr10" < "chr2"
LENGTHS = [3000000, 3000000, 3000000]
MIN, MAX, GAP, OVL = 40, 2000, 10, 5
SMALL = dict(min_mapq=20, min_sv_size=MIN, max_sv_size=MAX, segment_gap_tolerance=GAP, segment_overlap_tolerance=OVL)
MODES = ("coordinate", "queryname")


def seg(q_start, q_end, tid, ref_start, reverse=False, mapq=60, hard=False, cigar=None):
    """one alignment of a read; hard: its own record is hard-clipped (query-name mode sees that record); cigar: operations in place of yM"""
    return dict(q_start=q_start, q_end=q_end, tid=tid, ref_start=ref_start, reverse=bool(reverse), mapq=mapq, hard=hard, cigar=cigar)


def read(segs, primary=0, seq=True, length=None):
    """segs[primary] is the primary record, the others supplementary in the order given (SA tag and file alike); seq False: SEQ '*'; length: the read's length
    (default: the largest q_end)"""
    return dict(segs=list(segs), primary=primary, seq=seq, length=length)


class Case(object):
    def __init__(self, family, name, reads, expect, note=""):
        self.family, self.name, self.reads, self.note = family, name, reads if isinstance(reads, list) else [reads], note
        self.expect = expect if isinstance(expect, dict) else {m: list(expect) for m in MODES}      # mode -> tokens

    def read_names(self):
        return ["%s|%s|%d" % (self.family, self.name, k) for k in range(len(self.reads))]


def case_of_read(read_name):
    return tuple(read_name.split("|")[:2])


def token(row):
    """a golden row (helpers.sig_row layout) -> the token a case states"""
    t = row[0]
    if t == "INV":
        return "INV " + row[6]
    if t == "DUP_TAN":
        return "DUP_TAN %d %s" % (row[6], "full" if row[7] else "part")
    if t == "BND":
        return "BND " + row[3][0] + row[6][0]
    return t


# ---- SAM rendering ---------------------------------------------------------------------------------------------------------------------------------------------
def records_of_read(name, rd, seed):
    import random
    segs = rd["segs"]
    L = rd["length"] if rd["length"] is not None else max(s["q_end"] for s in segs)
    bases = synth.random_seq(random.Random(seed), max(L, 600))[:L]
    long_bases = synth.random_seq(random.Random(seed + 1), 600)          # for records whose own CIGAR states another read length
    order = [rd["primary"]] + [i for i in range(len(segs)) if i != rd["primary"]]
    ss = [synth.Segment(s["q_start"], s["q_end"], s["tid"], s["ref_start"], s["reverse"], s["cigar"] or [(0, s["q_end"] - s["q_start"])], s["mapq"]) for s in segs]

    def cig(i, hard):
        return ss[i].clipped_cigar(L, hard=hard) if segs[i]["cigar"] is None else list(segs[i]["cigar"])

    recs = []
    for rank, i in enumerate(order):
        s = segs[i]
        a = AlignedSegment()
        a.query_name = name
        a.flag = (16 if s["reverse"] else 0) | (2048 if rank else 0)
        a.reference_id, a.reference_start, a._mapq = s["tid"], s["ref_start"], s["mapq"]
        a.cigartuples = cig(i, s["hard"])
        full = synth.revcomp(bases) if s["reverse"] else bases
        lo = a.cigartuples[0][1] if a.cigartuples[0][0] == 5 else 0
        hi = a.cigartuples[-1][1] if a.cigartuples[-1][0] == 5 else 0
        if s["cigar"] is not None:
            n = sum(l for op, l in s["cigar"] if op in (0, 1, 4, 7, 8))
            a.query_sequence = long_bases[:n] if (rd["seq"] and n) else None
        else:
            a.query_sequence = full[lo:L - hi] if rd["seq"] else None
        sa = ["%s,%d,%s,%s,%d,0" % (REFERENCES[segs[j]["tid"]], segs[j]["ref_start"] + 1, "-" if segs[j]["reverse"] else "+", cigar_to_string(cig(j, False)),
                                  segs[j]["mapq"]) for j in order if j != i]
        if sa:
            a.set_tag("SA", ";".join(sa) + ";")
        recs.append(a)
    return recs


def sam_texts(cases):
    """{mode: SAM text} of the reads of `cases`, in the order given (query-name mode) and sorted by position (coordinate mode)"""
    recs = []
    for c in cases:
        for nm, rd in zip(c.read_names(), c.reads):
            recs.extend(records_of_read(nm, rd, seed=sum(map(ord, nm))))
    return {"coordinate": synth.sam_text(REFERENCES, LENGTHS, synth.coordinate_sort(recs), sort_order="coordinate"),
            "queryname": synth.sam_text(REFERENCES, LENGTHS, recs, sort_order="queryname")}


# ---- pair builders: the second segment from the numbers the tree compares ---------------------------------------------------------------------------------------
def same(dr, dref, reverse=False, la=100, lb=100, q0=20, r0=100000, tid=0):
    """same contig, same strand: distance_on_read dr, distance_on_reference dref"""
    a = seg(q0, q0 + la, tid, r0, reverse)
    b = seg(q0 + la + dr, q0 + la + dr + lb, tid, (r0 - dref - lb) if reverse else (r0 + la + dref), reverse)
    return [a, b]


def inv(kind, dr, d, la=100, lb=100, q0=20, r0=100000, tid=0):
    """the four inversion geometries; d is the reference test the case is entered by:
    1 fwd->rev, next.ref_start - cur.ref_end = d (left_fwd, size d + lb)      3 fwd->rev, cur.ref_start - next.ref_end = d (left_rev, size la + d)
    2 rev->fwd, next.ref_start - cur.ref_end = d (right_fwd, size la + d)     4 rev->fwd, cur.ref_start - next.ref_end = d (right_rev, size d + lb)"""
    a = seg(q0, q0 + la, tid, r0, kind in (2, 4))
    nrs = r0 + la + d if kind in (1, 2) else r0 - d - lb
    return [a, seg(q0 + la + dr, q0 + la + dr + lb, tid, nrs, kind in (1, 3))]


def other(dr, rev1, rev2, t1=0, t2=1, la=100, lb=100, q0=20, r1=100000, r2=200000):
    return [seg(q0, q0 + la, t1, r1, rev1), seg(q0 + la + dr, q0 + la + dr + lb, t2, r2, rev2)]


def chain(specs, q0=0, dr=0):
    """segments laid one behind the other on the read: specs = (tid, ref_start, length, reverse)"""
    out, q = [], q0
    for tid, rs, ln, rev in specs:
        out.append(seg(q, q + ln, tid, rs, rev))
        q += ln + dr
    return out


INV_DIR = {1: "left_fwd", 2: "right_fwd", 3: "left_rev", 4: "right_rev"}
INV_BND = {1: "BND fr", 3: "BND fr", 2: "BND rf", 4: "BND rf"}


# ---- families -----------------------------------------------------------------------------------------------------------------------------------------------------
def families():
    """-> list of (family name, options, [Case])"""
    F = []

    # segment_overlap_tolerance: -OVL-1, -OVL, -OVL+1
    cs = []
    for rev in (False, True):
        st = "rev" if rev else "fwd"
        for dr in (-OVL - 1, -OVL, -OVL + 1):                              # read distance; dref 200: deviation dr - 200, a deletion
            cs.append(Case("overlap", "%s read dr=%d" % (st, dr), read(same(dr, 200, rev)), ["DEL"] if dr >= -OVL else []))
        for dref in (-OVL - 1, -OVL, -OVL + 1):                            # reference distance; dr 60: deviation 60 - dref, an insertion
            cs.append(Case("overlap", "%s ref dref=%d" % (st, dref), read(same(60, dref, rev)), ["INS"] if dref >= -OVL else [],
                           "dref -OVL-1 is neither 'no overlap' nor <= -MIN: nothing"))
    for kind in (1, 2, 3, 4):
        for dr in (-OVL - 1, -OVL, -OVL + 1):
            cs.append(Case("overlap", "inv%d read dr=%d" % (kind, dr), read(inv(kind, dr, 0)), ["INV " + INV_DIR[kind]] if dr >= -OVL else []))
        for d in (-OVL - 1, -OVL, -OVL + 1):                               # cases 1, 2: the first reference test; cases 3, 4: the second
            cs.append(Case("overlap", "inv%d ref d=%d" % (kind, d), read(inv(kind, 0, d)), ["INV " + INV_DIR[kind]] if d >= -OVL else [],
                           "size 100 + d"))
    for r1, r2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for dr in (-OVL - 1, -OVL, -OVL + 1):
            cs.append(Case("overlap", "other contig %d%d dr=%d" % (r1, r2, dr), read(other(dr, r1, r2)), ["BND " + "fr"[r1] + "fr"[r2]] if dr >= -OVL else []))
    F.append(("overlap", SMALL, cs))

    # segment_gap_tolerance: GAP-1, GAP, GAP+1 at its five uses
    cs = []
    for rev in (False, True):
        st = "rev" if rev else "fwd"
        for g in (GAP - 1, GAP, GAP + 1):
            cs.append(Case("gap", "%s INS dref=%d" % (st, g), read(same(g + 50, g, rev)), ["INS"] if g <= GAP else [], "deviation 50"))
            cs.append(Case("gap", "%s DEL dr=%d" % (st, g), read(same(g, g + 100, rev)), ["DEL"] if g <= GAP else [], "deviation -100"))
            cs.append(Case("gap", "%s large DEL dr=%d" % (st, g), read(same(g, g + MAX + 500, rev)), ["BND ff"] if g <= GAP else [],
                           "deviation -MAX-500; the reverse strand's (rev, rev) breakend has p1 > p2 and is swapped to (fwd, fwd)"))
    for kind in (1, 2, 3, 4):
        for g in (GAP - 1, GAP, GAP + 1):
            cs.append(Case("gap", "inv%d dr=%d" % (kind, g), read(inv(kind, g, 0)), ["INV " + INV_DIR[kind]] if g <= GAP else []))
    for r1, r2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for g in (GAP - 1, GAP, GAP + 1):
            cs.append(Case("gap", "other contig %d%d dr=%d" % (r1, r2, g), read(other(g, r1, r2)), ["BND " + "fr"[r1] + "fr"[r2]] if g <= GAP else []))
    F.append(("gap", SMALL, cs))

    # deviation = dr - dref, both strands (the golden holds the starts: DEL from next.ref_end, INS from current.ref_start on the reverse strand)
    def deviation_cases(fam, mx):
        out = []
        for rev in (False, True):
            st = "rev" if rev else "fwd"
            for dev, exp in ((MIN - 1, []), (MIN, ["INS"]), (-MIN + 1, []), (-MIN, ["DEL"]), (-mx, ["DEL"]), (-mx - 1, ["BND ff"])):
                dr = dev + 1 if dev > 0 else 0
                out.append(Case(fam, "%s deviation %d" % (st, dev), read(same(dr, dr - dev, rev)), exp))
        return out
    F.append(("deviation", SMALL, deviation_cases("deviation", MAX)))
    F.append(("deviation_default_max", dict(SMALL, max_sv_size=100000), deviation_cases("deviation_default_max", 100000)))

    # overlap on the reference (dr 0, both segments 100 long)
    cs = []
    for rev in (False, True):
        st, bb = ("rev" if rev else "fwd"), "BND rr"          # fwd: (fwd, fwd) with p1 > p2, swapped; rev: (rev, rev) kept
        for dref, exp in ((-MIN + 1, []), (-MIN, ["DUP_TAN 1 full"]), (-MAX, ["DUP_TAN 1 part"]), (-MAX - 1, [bb])):
            cs.append(Case("ref_overlap", "%s dref=%d" % (st, dref), read(same(0, dref, rev)), exp))
        # fwd: next.ref_end - cur.ref_start = dref + 200; rev: next.ref_start - cur.ref_end = -dref - 200.  Fully covered only when the next segment reaches INTO the current one
        for k in (-1, 0, 1):
            cs.append(Case("ref_overlap", "%s covered by %d" % (st, k), read(same(0, -200 + k, rev)), ["DUP_TAN 1 " + ("full" if k > 0 else "part")],
                           "next.ref_end - cur.ref_start = %d (fwd) / cur.ref_end - next.ref_start = %d (rev)" % (k, k)))
    F.append(("ref_overlap", SMALL, cs))

    # inversion sizes
    cs = []
    for kind in (1, 2, 3, 4):
        for sz, exp in ((MIN - 1, []), (MIN, ["INV " + INV_DIR[kind]]), (MAX, ["INV " + INV_DIR[kind]]), (MAX + 1, [INV_BND[kind]])):
            small = sz < 100
            l_var = sz if small else 100                       # the segment whose length is part of the size
            d = 0 if small else sz - 100
            kw = dict(lb=l_var) if kind in (1, 4) else dict(la=l_var)
            cs.append(Case("inv_size", "inv%d size %d" % (kind, sz), read(inv(kind, 0, d, **kw)), exp))
    F.append(("inv_size", SMALL, cs))

    # tandem runs.  A duplication is (next.ref_start, cur.ref_end) on the forward strand, (cur.ref_start, next.ref_end) on the reverse strand
    cs = []
    T = "tandem"
    for k, exp in ((269, ["DUP_TAN 2 full"]), (270, ["DUP_TAN 1 full", "DUP_TAN 1 full"])):
        # (10000, 10200) and (10000 + k, 10200 + k): equal spans, centres k apart: 269 / 900 < 0.3, 270 / 900 == 0.3 in doubles (not smaller)
        cs.append(Case(T, "two, centres %d apart" % k, read(chain([(0, 9900, 300, 0), (0, 10000, 200 + k, 0), (0, 10000 + k, 100, 0)])), exp,
                       "the merged run's means are 10134.5 and 10334.5: int(mean) truncates"))
    for span, exp in ((71, ["DUP_TAN 2 full"]), (70, ["DUP_TAN 1 full", "DUP_TAN 1 full"])):
        # (10000, 10100) and (10050 - span // 2 .., span long) around the same centre: span distance 29 / 100 and 30 / 100 (0.3 in doubles: not smaller)
        s2 = 10050 - span // 2
        cs.append(Case(T, "two, spans 100 and %d" % span, read(chain([(0, 9900, 200, 0), (0, 10000, s2 + span - 10000, 0), (0, s2, 60, 0)])), exp))
    cs.append(Case(T, "two, 0.1 + 0.2 in doubles", read(chain([(0, 9900, 200, 0), (0, 10000, 180, 0), (0, 10100, 60, 0)])), ["DUP_TAN 1 full", "DUP_TAN 1 full"],
                   "(10000, 10100) and (10100, 10180): 90 / 900 + 20 / 100 = 0.30000000000000004 in doubles, not smaller than 0.3 although the exact sum is"))
    for s3, exp in ((10403, ["DUP_TAN 3 full"]), (10404, ["DUP_TAN 2 full", "DUP_TAN 1 full"])):
        # run of (10000, 10200), (10269, 10469): means 10134.5 / 10334.5, centre (20469.0) // 2 = 10234.0; third (s3, s3 + 200) with centre s3 + 100
        cs.append(Case(T, "three, third at %d" % s3, read(chain([(0, 9900, 300, 0), (0, 10000, 469, 0), (0, 10269, s3 + 200 - 10269, 0), (0, s3, 100, 0)])), exp,
                       "the floor of a float mean: without it the centre were 10234.5 and 10404 would still merge"))
    cs.append(Case(T, "run ends on a change of contig", read(chain([(0, 9900, 300, 0), (0, 10000, 300, 0), (1, 9900, 300, 0), (1, 10000, 300, 0)])),
                   ["BND ff", "DUP_TAN 1 full", "DUP_TAN 1 full"], "the same coordinates on chr1 and chr2"))
    cs.append(Case(T, "fully covered only in the later member", read(chain([(0, 10300, 100, 0), (0, 10000, 200, 0), (0, 9800, 300, 0)])), ["DUP_TAN 2 full"],
                   "(10000, 10400) not covered, (9800, 10200) covered"))
    cs.append(Case(T, "fully covered in no member", read(chain([(0, 10300, 100, 0), (0, 10000, 200, 0), (0, 9800, 100, 0)])), ["DUP_TAN 2 part"]))
    ffrr = [(0, 9900, 300, 0), (0, 10000, 300, 0), (0, 20000, 300, 1), (0, 19900, 300, 1)]
    cs.append(Case(T, "fwd fwd rev rev", read(chain(ffrr)), ["BND fr", "DUP_TAN 1 full", "DUP_TAN 1 full"]))
    cs.append(Case(T, "fwd fwd rev rev rev", read(chain(ffrr + [(0, 19800, 300, 1)])), ["BND fr", "DUP_TAN 1 full", "DUP_TAN 1 full", "DUP_TAN 1 full"],
                   "the second run keeps the first run's direction: the two reverse duplications are similar and still do not merge"))
    cs.append(Case(T, "rev rev rev", read(chain(ffrr[2:] + [(0, 19800, 300, 1)])), ["DUP_TAN 2 full"], "the same reverse duplications without the stale direction"))
    cs.append(Case(T, "fwd fwd rev rev fwd fwd", read(chain(ffrr + [(0, 19900, 310, 0), (0, 20010, 100, 0)])), ["BND fr", "DUP_TAN 1 full", "DUP_TAN 2 full"],
                   "a forward duplication merges into the reverse run, by the stale direction"))
    cs.append(Case(T, "one duplication below min size", read(same(0, -MIN + 1)), []))
    F.append((T, SMALL, cs))

    # insertions with a detected origin; MAX 300 so that the origin's size needs no long read.  A (chr1) -> B (chr2) -> C (chr1)
    IMAX = 300
    cs = []
    Fm = "ins_from"

    def abc(rev, lb=100, c_off=0):
        """forward: destination positions A.ref_end - 1 and C.ref_start = A.ref_end - 1 + c_off; reverse: A.ref_start and C.ref_end - 1 = A.ref_start + c_off"""
        if not rev:
            return chain([(0, 10000, 100, 0), (1, 5000, lb, 0), (0, 10099 + c_off, 100, 0)])
        return chain([(0, 10000, 100, 1), (1, 5000, lb, 1), (0, 10000 + c_off + 1 - 100, 100, 1)])

    for rev in (False, True):
        st = "rev" if rev else "fwd"
        bb2 = ["BND rr", "BND ff"] if rev else ["BND ff", "BND rr"]          # the breakend back from chr2 to chr1 is swapped
        for off, note in ((89, "89 / 900 < 0.1"), (90, "90 / 900 is the double 0.1 itself: not smaller"), (91, "")):
            cs.append(Case(Fm, "%s destination %d apart" % (st, off), read(abc(rev, c_off=off)), bb2 + (["DUP_INT"] if off < 90 else []), note))
            cs.append(Case(Fm, "%s destination -%d apart" % (st, off), read(abc(rev, c_off=-off)), bb2 + (["DUP_INT"] if off < 90 else []), note))
        for sz, ok in ((MIN - 1, 0), (MIN, 1), (IMAX, 1), (IMAX + 1, 0)):
            cs.append(Case(Fm, "%s size %d" % (st, sz), read(abc(rev, lb=sz + (1 if rev else 0))), bb2 + (["DUP_INT"] if ok else []),
                           "fwd: this_pos1 - before_pos2 + 1 = len(B); rev: before_pos2 - this_pos1 = len(B) - 1"))
    cs.append(Case(Fm, "origin on another contig", read(chain([(0, 10000, 100, 0), (1, 5000, 100, 0), (2, 5000, 100, 0), (0, 10100, 100, 0)])), ["BND ff", "BND rr", "BND rr"],
                   "before_chr2 chr2 != this_chr1 chr10; the size would be 100"))
    cs.append(Case(Fm, "mixed directions", read(chain([(0, 10000, 100, 0), (1, 5000, 100, 1), (1, 5200, 100, 1), (0, 10100, 100, 0)])), ["BND fr", "BND rf", "DUP_TAN 1 part"],
                   "before (fwd, rev), this (rev, fwd): every test but before_dir2 == before_dir1 holds and the size were 102"))
    cs.append(Case(Fm, "before_dir1 != this_dir2", read(chain([(0, 10000, 100, 0), (1, 5000, 100, 0), (0, 10000, 100, 1)])), ["BND ff", "BND fr"]))
    cs.append(Case(Fm, "before_dir2 != this_dir1", read(chain([(0, 10000, 100, 0), (1, 5000, 100, 0), (1, 5060, 100, 1), (0, 10100, 100, 0)])), ["BND ff", "BND rf"]))
    cs.append(Case(Fm, "four translocations", read(chain([(0, 10000, 100, 0), (1, 5000, 100, 0), (0, 10100, 100, 0), (1, 5100, 100, 0), (0, 10150, 100, 0)])),
                   ["BND ff", "BND rr"] * 2 + ["DUP_INT"] * 4, "pairs (this, before) = (2,1) (3,2) (4,1) (4,3) in that order"))
    cs.append(Case(Fm, "nothing", read(abc(False)[:1] + [seg(111, 211, 1, 5000)]), [], "read distance GAP + 1"))
    F.append((Fm, dict(SMALL, max_sv_size=IMAX), cs))

    # the canonical order of a breakend
    cs = []
    Fm = "bnd_order"
    cs.append(Case(Fm, "same contig p1 < p2", read(same(0, MAX + 500)), ["BND ff"]))
    cs.append(Case(Fm, "same contig p1 > p2", read(same(0, -MAX - 500)), ["BND rr"], "swapped: both directions flip"))
    cs.append(Case(Fm, "same contig p1 > p2 rev", read(same(0, -MAX - 500, True)), ["BND rr"], "(rev, rev) at (cur.ref_start, next.ref_end - 1): p1 < p2, kept"))
    cs.append(Case(Fm, "same contig p1 < p2 rev", read(same(0, MAX + 500, True)), ["BND ff"], "swapped"))
    for t1, t2 in ((0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)):
        for r1, r2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            keep = REFERENCES[t1] < REFERENCES[t2]
            d = "fr"[r1] + "fr"[r2] if keep else "fr"[1 - r2] + "fr"[1 - r1]
            cs.append(Case(Fm, "%s -> %s %d%d" % (REFERENCES[t1], REFERENCES[t2], r1, r2), read(other(0, r1, r2, t1, t2)), ["BND " + d]))
    cs.append(Case(Fm, "nothing", read(other(GAP + 1, 0, 0)), []))
    F.append((Fm, SMALL, cs))
    # p1 == p2 needs min_sv_size 1 and no overlap tolerance: a tandem duplication of one base, whose breakend goes to the side list (all_bnds)
    cs = [Case("bnd_order_equal", "fwd", read(same(0, -1)), ["DUP_TAN 1 full"], "side list: (fwd, fwd) at p1 == p2 is swapped to (rev, rev)"),
          Case("bnd_order_equal", "rev", read(same(0, -1, True)), ["DUP_TAN 1 full"], "side list: (rev, rev) at p1 == p2 is swapped to (fwd, fwd)"),
          Case("bnd_order_equal", "nothing", read(same(0, 0)), [])]
    F.append(("bnd_order_equal", dict(SMALL, min_sv_size=1, segment_overlap_tolerance=0), cs))

    # sorting and filtering.  Equal (q_start, q_end) needs segments no longer than OVL
    cs = []
    Fm = "sort_filter"
    lo, hi = seg(50, 55, 0, 1000), seg(50, 55, 0, 3000)
    cs.append(Case(Fm, "tie primary first low", read([lo, hi], primary=0), ["DEL"], "order (1000, 3000): dr -5, dref 1995"))
    cs.append(Case(Fm, "tie primary first high", read([lo, hi], primary=1), ["BND rr"], "order (3000, 1000): dref -2005"))
    far = seg(0, 40, 1, 7000)                                             # primary on chr2; chr2 > chr1: its breakend to chr1 is swapped, (rev, rev)
    cs.append(Case(Fm, "tie of two supplementaries low high", read([far, lo, hi]), ["BND rr", "DEL"]))
    cs.append(Case(Fm, "tie of two supplementaries high low", read([far, hi, lo]), ["BND rr", "BND rr"]))
    lo6 = seg(50, 56, 0, 1000)
    cs.append(Case(Fm, "tie in q_start only, given sorted", read([far, hi, lo6]), ["BND rr", "BND rr"], "(50, 55) before (50, 56)"))
    cs.append(Case(Fm, "tie in q_start only, given unsorted", read([far, lo6, hi]), ["BND rr", "BND rr"]))
    a, c = seg(0, 100, 0, 10000), seg(200, 300, 0, 10300)

    def mid(mapq, **kw):
        return seg(100, 200, 0, 50000, mapq=mapq, **kw)
    cs.append(Case(Fm, "supplementary below min_mapq between two good ones", read([a, mid(19), c]), [], "A -> C: dr 100 > GAP"))
    cs.append(Case(Fm, "supplementary at min_mapq between two good ones", read([a, mid(20), c]), ["BND ff", "BND rr"]))
    a2, c2 = seg(0, 100, 0, 10000), seg(100, 200, 0, 10300)
    cs.append(Case(Fm, "low supplementary in front of an adjacent pair", read([a2, seg(50, 150, 0, 50000, mapq=5), c2]), ["DEL"]))
    cs.append(Case(Fm, "primary below min_mapq", read([seg(0, 100, 0, 10000, mapq=19), c2]), []))
    cs.append(Case(Fm, "primary at min_mapq", read([seg(0, 100, 0, 10000, mapq=20), c2]), ["DEL"]))
    cs.append(Case(Fm, "reverse segment without a read length", read([a2, seg(50, 150, 0, 50000, True, cigar=[(2, 30)]), c2]), ["DEL"],
                   "CIGAR 30D: infer_read_length() is None, the alignment is skipped"))
    cs.append(Case(Fm, "forward segment without a read length", read([a2, seg(50, 150, 0, 50000, False, cigar=[(2, 30)]), c2]),
                   {"coordinate": [], "queryname": ["BND rr", "DEL"]},
                   "the same on the forward strand is used: as query 0-0 in query-name mode (sorted first, a breakend to A), as 0-200 with the primary's SEQ in coordinate mode"))
    cs.append(Case(Fm, "hard-clipped primary", read([seg(0, 100, 0, 10000, hard=True), c2]), {"coordinate": [], "queryname": ["DEL"]},
                   "coordinate mode: the SA rebuild is void"))
    cs.append(Case(Fm, "primary hard-clipped by one base", read([seg(0, 100, 0, 10000, hard=True), seg(100, 101, 0, 10300)]),
                   {"coordinate": [], "queryname": ["DEL"]}, "100M1H"))
    cs.append(Case(Fm, "hard-clipped supplementary fwd", read([a2, seg(100, 200, 0, 10300, hard=True)]), {"coordinate": ["DEL"], "queryname": []},
                   "query-name mode: query_alignment_start skips H, the segment sits at query 0-100"))
    cs.append(Case(Fm, "hard-clipped supplementary rev, H behind", read([seg(0, 100, 0, 10300, True), seg(100, 200, 0, 10000, True, hard=True)]), ["DEL"],
                   "100M100H: the read length counts H, query 100-200 either way"))
    cs.append(Case(Fm, "hard-clipped supplementary rev, H in front", read([seg(100, 200, 0, 10000, True), seg(0, 100, 0, 10300, True, hard=True)], primary=0),
                   {"coordinate": ["DEL"], "queryname": []}, "100H100M: query 100-200 in query-name mode, a tie with the primary"))
    cs.append(Case(Fm, "only the primary is good", read([a2, seg(100, 200, 0, 10300, mapq=5)]), []))
    F.append((Fm, SMALL, cs))

    # inserted bases: primary.query_sequence[a:a + deviation], a = cur.q_end (fwd) / primary.infer_read_length() - next.q_start (rev)
    cs = []
    Fm = "ins_bases"
    for rev in (False, True):
        st = "rev" if rev else "fwd"
        cs.append(Case(Fm, st + " inside", read(same(60, 0, rev)), ["INS"]))
        cs.append(Case(Fm, st + " no SEQ", read(same(60, 0, rev), seq=False), ["INS"], "TypeError -> empty sequence"))
        cs.append(Case(Fm, st + " below min size", read(same(MIN - 1, 0, rev)), []))
    cs.append(Case(Fm, "fwd past the end", read([seg(0, 100, 0, 10000), seg(160, 163, 0, 10095)]), ["INS"], "deviation 65 from 100 in a SEQ of 163"))
    cs.append(Case(Fm, "rev past the end", read([seg(0, 3, 0, 10000, True), seg(63, 163, 0, 9905, True)], length=300), ["INS"],
                   "a = 300 - 63, deviation 65 in a SEQ of 300"))
    cs.append(Case(Fm, "rev negative start, empty", read([seg(0, 100, 0, 10000, True, cigar=[(4, 50), (0, 100)]),
                                                          seg(160, 260, 0, 9900, True, cigar=[(4, 140), (0, 100), (4, 160)])]), ["INS"],
                   "query-name mode: the primary's CIGAR says 150 bases, the other's 400: a = 150 - 160, [-10:50] of 150 bases is empty; "
                   "coordinate mode: the rebuilt alignment takes the primary's SEQ, its query end comes out negative, the slice starts below -150"))
    cs.append(Case(Fm, "rev negative start and end", read([seg(0, 100, 1, 10000, True, cigar=[(4, 50), (0, 100)]),
                                                           seg(90, 190, 0, 10000, True, cigar=[(4, 310), (0, 100), (4, 90)]),
                                                           seg(250, 350, 0, 9900, True, cigar=[(4, 150), (0, 100), (4, 250)])]), ["INS"],
                  "query-name mode: the primary (chr2) says 150 bases, the others 500: a = 150 - 250, deviation 60, [-100:-40] of 150 bases"))
    F.append((Fm, SMALL, cs))
    return F


def all_cases():
    return [c for _, _, cs in families() for c in cs]


# ---- batches for the kernel's placement and capacity (tests/test_gpu_segments.py; the oracle walks them in tests/test_segments.py) ---------------------------------
PLACEMENT_N_REC = (255, 256, 257, 513)
INS_FROM_OPTIONS = dict(SMALL, max_sv_size=300)          # the family "ins_from": placed once more on its own, in a batch of 257 records
PLACEMENT_OWNERS = (0, 63, 64, 255, 256)             # and n_rec - 1: the first and last lane of a wave and of a 256-thread block


def placement_batch(n_rec, options=None, seed=5):
    """every case of the families that share `options` (default SMALL: nine families, 205 reads; one batch takes one set of options) as ONE coordinate-mode batch of n_rec records: the primaries (each with its SA tag) at chosen
    record indices - PLACEMENT_OWNERS and n_rec - 1 among them - , plain primaries without an SA tag everywhere else, and a permuted `order`, so that the keys do
    not follow the record index.  -> (HostBatch, options dict, read name per record or None, key rank per record)"""
    import random
    import types
    import numpy as np
    from svim_amd import batch, records
    options = dict(SMALL if options is None else options)
    prim = []
    for _, opt, cs in families():
        if opt == options:
            for c in cs:
                for nm, rd in zip(c.read_names(), c.reads):
                    prim.append(records_of_read(nm, rd, seed=sum(map(ord, nm)))[0])
    assert len(prim) <= n_rec
    must = sorted({i for i in PLACEMENT_OWNERS if i < n_rec} | {n_rec - 1})
    free = [i for i in range(n_rec) if i not in must]
    need = len(prim) - len(must)
    slots = must + [free[(j * len(free)) // need] for j in range(need)]          # the first reads (family "overlap": all own rows) take the named indices
    assert len(set(slots)) == len(prim)
    rng = random.Random(seed)
    recs, names = [None] * n_rec, [None] * n_rec
    for a, i in zip(prim, slots):
        recs[i], names[i] = a, a.query_name
    for i in range(n_rec):
        if recs[i] is None:
            a = AlignedSegment()
            a.query_name, a.flag, a.reference_id, a.reference_start, a._mapq = "filler%d" % i, 16 * (i & 1), i % 3, 500 + 7 * i, 60
            a.cigartuples, a.query_sequence = [(0, 50)], synth.random_seq(rng, 50)
            recs[i] = a
    bam = records.AlignmentFile(text=synth.sam_text(REFERENCES, LENGTHS, []))
    hb = batch.build_batch(bam, types.SimpleNamespace(**options), mode="coordinate", records=recs)
    perm = list(range(n_rec))
    rng.shuffle(perm)
    hb.arrays["order"] = np.array([2 * p for p in perm], dtype=np.uint32)
    hb.arrays["seg_order"] = hb.arrays["order"] + np.uint32(1)
    return hb, options, names, perm


def _clip_ops(q_start, length, read_len):
    import cigar_layouts as CL
    out = [CL.w(CL.S, q_start)] if q_start else []
    out.append(CL.w(CL.M, length))
    if read_len - q_start - length:
        out.append(CL.w(CL.S, read_len - q_start - length))
    return out


def _read_of(specs, pos_of_record, bad_rows=0):
    """a cigar_layouts record: forward segments (tid, ref_start, length) laid end to end on the read, the first one the primary, the others its rows (rebuilt from
    an SA tag: stored length 0); bad_rows more rows below min_mapq behind them"""
    import cigar_layouts as CL
    L = sum(ln for _, _, ln in specs)
    q, rows = specs[0][2], []
    for tid, rs, ln in specs[1:]:
        rows.append(CL.row(_clip_ops(q, ln, L), tid=tid, pos=rs, rev=0, mapq=60, lseq=0))
        q += ln
    rows += [CL.row(_clip_ops(0, 10, L), tid=0, pos=77, mapq=CL.MIN_MAPQ - 1) for _ in range(bad_rows)]
    assert specs[0][1] == pos_of_record
    return CL.rec(_clip_ops(0, specs[0][2], L), pos=specs[0][1], tid=specs[0][0], rows=rows)


MANY_ROWS_K = (1, 2, 63, 64, 65, 300)


def many_rows_case():
    """reads with k good rows (k + 1 alignments) next to reads with none, in two layouts that fill one of the kernel's per-read lists to the capacity of the
    read's workspace (n_seg entries, at ws + seg_off[r] + r):
    "bnd": contigs alternate, 1000 bases apart on each: every adjacent pair is a breakend (k entries in the translocation list), no two destinations similar;
    "tan": every alignment at the same place: every adjacent pair is a fully covered tandem duplication (k entries in the tandem list), all of one run.
    Every k once with good rows only (n_seg = k: the list is full) and, for k = 63 and 64, once more with a row below min_mapq behind them (n_seg = k + 1).
    -> (cigar_layouts.Case, main-list rows expected, side-list rows expected under all_bnds, {record index: (layout, rows below min_mapq)})"""
    import cigar_layouts as CL
    recs, layouts, n_main, n_side = [], {}, 0, 0
    for k, bad in [(k, 0) for k in MANY_ROWS_K] + [(63, 1), (64, 1)]:
        layouts[len(recs)] = ("bnd", bad)
        recs.append(_read_of([(i & 1, 10000 + 1000 * i, 50) for i in range(k + 1)], 10000, bad_rows=bad))
        recs.append(CL.rec([CL.w(CL.M, 50)], pos=300 + k))
        layouts[len(recs)] = ("tan", bad)
        recs.append(_read_of([(0, 100000, 100)] * (k + 1), 100000, bad_rows=bad))
        recs.append(CL.rec([CL.w(CL.M, 50)], pos=400 + k, flag=16))
        n_main += k + 1                    # k breakends; one DUP_TAN of k copies
        n_side += k                        # the k duplications' breakends
    return CL.Case("many rows on one read", recs, min_sv_size=40, seed=41), n_main, n_side, layouts


RAW_SHARDS = 8192                          # svim_amd/csrc/collect.hip
N_TANDEM_PREFIX = 10


def first_pass_capacity(n_ops, n_seg):
    """rows svx_collect_impl sizes its first pass for (svim_amd/csrc/collect.hip, want_sig)"""
    return n_ops // 256 + 4 * n_seg + 16 * RAW_SHARDS


def second_pass_case():
    """ONE read whose main list outgrows the first sizing pass of svx_collect_impl: ten alignments at one place on chr1 (nine tandem duplications: one DUP_TAN, and
    nine breakends for the side list under all_bnds; these lists stay far below the read's n_seg), then s alignments of 50 bases that alternate between chr2:5000 and chr1:10000.  The alternating part holds
    t = s - 1 translocations of two kinds by turns, and every one of them matches every earlier one of the OTHER kind (destinations 49 bases apart, origin 50 long):
    floor(t * t / 4) insertions with detected origin.  s is the smallest size at which the rows are more than twice the first pass's capacity.
    -> (cigar_layouts.Case, main-list rows expected, side-list rows expected under all_bnds, first-pass capacity)"""
    import cigar_layouts as CL

    def rows_of(s):
        return 1 + 1 + (s - 1) + ((s - 1) * (s - 1)) // 4       # DUP_TAN, the breakend from the prefix to the first chr2 alignment, t breakends, the pairs
    s = 2
    while rows_of(s) <= 2 * first_pass_capacity(3, N_TANDEM_PREFIX + s - 1):
        s += 1
    specs = [(0, 500000, 50)] * N_TANDEM_PREFIX + [((i + 1) & 1, 5000 if not (i & 1) else 10000, 50) for i in range(s)]
    case = CL.Case("one read of %d alignments" % len(specs), [_read_of(specs, 500000)], min_sv_size=40, seed=43)
    return case, rows_of(s), N_TANDEM_PREFIX - 1, first_pass_capacity(len(case.recs[0]["ops"]), len(case.recs[0]["rows"]))
