"""Directed cases for CLUSTER (csrc/cluster.hip: k_part_flags, k_cluster, linkage_fcluster_lds, consolidate_one; oracle/svx_oracle.c: svo_form_partitions,
svo_cluster, span_position_distance, svo_linkage_fcluster, consolidate, calc_score): one case on each side of every comparison of form_partitions,
clusters_from_partitions, span_position_distance, fcluster and the consolidation (SVIM_clustering.py:17-29, :47-96, :122-180, :183-303), and the sizes at which the
device kernel takes another path.  tests/golden/make_golden_cluster.py runs the reference on them (tests/golden/g_cluster_cases.json.gz) and stops when the
reference disagrees with what a case's author wrote down; tests/test_cluster_cases.py holds the oracle to that file on the CPU, tests/test_gpu_cluster_cases.py the
device.

A CASE: a name, a family, signature rows in the row layout of g5_cluster.json.gz, and what its author expects of the reference - `parts` (the partitions as lists of
the case's own row numbers, type by type in the order DEL INS INV DUP_TAN BND DUP_INT, each type's in the order they are formed), `clusters` (the member lists, as
a set) and/or `counts` (clusters per type) - , the pairs whose distance is recorded bit for bit, and `covers`: (threshold, side) with side one of below / on / above.

A FAMILY: cases that share their options and go through CLUSTER as one table.  Every case gets a stretch of coordinates of its own (non-insertions one million
bases per case, insertions a stretch of chr1 of the reference genome at least 3000 bases from the next), so no case changes another's partitions, and duplicates
and clusters never leave a partition.  The exception is `sample`: partitions of more than 100 draw from one random.sample stream per type, so that family has a
fixed order and its cases are not independent of each other.  REFUSED holds what the reference raises on; it is in no parity set.

Test infrastructure only; imports no GPU code."""
import random

REFS = ["chr1", "chr2", "chr10"]          # helpers.REFS: string order chr1 < chr10 < chr2
CHR1_LEN = 180000
OPTIONS = {"min_mapq": 20, "min_sv_size": 40, "max_sv_size": 100000, "segment_gap_tolerance": 10, "segment_overlap_tolerance": 5, "partition_max_distance": 1000,
           "position_distance_normalizer": 900, "edit_distance_normalizer": 1.0, "cluster_max_distance": 0.5, "all_bnds": False}
TYPES = ("DEL", "INS", "INV", "DUP_TAN", "BND", "DUP_INT")
SIDES = ("below", "on", "above")
STRIDE = 1000000


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------------------------
def DEL(s, e, read, contig="chr1"):
    return ["DEL", contig, s, e, "cigar", read]


def INS(s, seq, read, contig="chr1", span=None):
    return ["INS", contig, s, s + (len(seq) if span is None else span), "cigar", read, seq]


def INV(s, e, read, direction="all", contig="chr1"):
    return ["INV", contig, s, e, "suppl", read, direction]


def TAN(s, e, read, copies=1, contig="chr1"):
    return ["DUP_TAN", contig, s, e, "suppl", read, copies, True]


def DINT(s, e, read, pos, contig="chr1", contig2="chr2"):
    return ["DUP_INT", contig, s, e, "suppl", read, contig2, pos]


def BND(p1, p2, read, d1="fwd", d2="fwd", contig="chr1", contig2="chr2"):
    assert contig < contig2 or (contig == contig2 and p1 < p2)          # canonical order: the constructor would swap the ends and flip the directions
    return ["BND", contig, p1, d1, contig2, p2, d2, "suppl", read]


def span_row(typ, s, e, read, contig="chr1"):
    """a row of a type that has a span (not BND, not INS), its destination - where it has one - moving with its start"""
    if typ == "DEL":
        return DEL(s, e, read, contig)
    if typ == "INV":
        return INV(s, e, read, "all", contig)
    if typ == "DUP_TAN":
        return TAN(s, e, read, 1, contig)
    assert typ == "DUP_INT"
    return DINT(s, e, read, s + 500000, contig)


class Case(object):
    def __init__(self, name, rows, parts=None, clusters=None, counts=None, covers=(), pairs="all"):
        self.name, self.rows, self.parts, self.counts, self.covers = name, rows, parts, counts, list(covers)
        self.clusters = None if clusters is None else sorted(sorted(c) for c in clusters)
        assert parts is not None or clusters is not None or counts is not None, name
        for r in rows:                                        # read names of a case are its own
            k = 8 if r[0] == "BND" else 5
            r[k] = "%s/%s" % (name, r[k])
        n = len(rows)
        if pairs == "all":
            pairs = [(i, j) for i in range(n) for j in range(n) if i != j and rows[i][0] == rows[j][0]] if n <= 8 else "some"
        if pairs == "some":
            pairs = [(i, j) for i in range(n - 1) for j in (i + 1, n - 1 - i) if j != i and rows[i][0] == rows[j][0]]
            pairs += [(j, i) for i, j in pairs[:40]]
        self.pairs = [p for p in pairs if rows[p[0]][0] != "INS" or rows[p[0]][1] == rows[p[1]][1]]


class Family(object):
    def __init__(self, name, independent=True, **opts):
        self.name, self.options, self.cases, self.independent = name, dict(OPTIONS, **opts), [], independent
        self.n_base, self.ins_at = 0, 2000

    def base(self):
        """the start of a fresh million-base stretch (non-insertions)"""
        self.n_base += 1
        assert self.n_base * STRIDE < 2000000000
        return self.n_base * STRIDE

    def ins_base(self, length):
        """the start of a fresh stretch of chr1 for insertions that reach `length` bases"""
        at = self.ins_at
        self.ins_at += length + 3000
        assert self.ins_at < CHR1_LEN - 1000, self.name
        return at

    def add(self, name, rows, **kw):
        assert name not in [c.name for c in self.cases]
        self.cases.append(Case(name, rows, **kw))

    def rows(self):
        return [r for c in self.cases for r in c.rows]

    def ranges(self):
        out, at = [], 0
        for c in self.cases:
            out.append((at, at + len(c.rows)))
            at += len(c.rows)
        return out


def rseq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


# ---- partitions: form_partitions, get_key, downstream_distance_to (family `wide`: a normalizer of 9000 and an edit normalizer of 100 let two signatures a whole
# partition_max_distance apart still cluster, so the CLUSTERS show the partition boundary too) ---------------------------------------------------------------------
def gap_rows(typ, b, gap, seq="ACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCA"):
    """two signatures of two reads whose downstream distance, measured as the type measures it, is `gap`"""
    if typ == "INS":
        return [INS(b, seq, "a"), INS(b + gap, seq, "b")]
    if typ == "BND":
        return [BND(b, b + 700000, "a"), BND(b + 1 + gap, b + 700000, "b")]
    if typ == "DUP_INT":
        return [DINT(b, b + 200, "a", b + 500000), DINT(b + 30, b + 230, "b", b + 500000 + gap)]
    return [span_row(typ, b, b + 200, "a"), span_row(typ, b + 200 + gap, b + 400 + gap, "b")]


def wide():
    f = Family("wide", position_distance_normalizer=9000, edit_distance_normalizer=100.0)
    for typ in TYPES:
        for gap, side in ((999, "below"), (1000, "on"), (1001, "above")):
            b = f.ins_base(1100) if typ == "INS" else f.base()
            one = side != "above"
            f.add("%s gap %d" % (typ, gap), gap_rows(typ, b, gap), parts=[[0, 1]] if one else [[0], [1]], clusters=[[0, 1]] if one else [[0], [1]],
                  covers=[("partition gap " + typ, side)])
    # the wrong measure of each type joins / splits: an insertion's END is inside the distance (start to start is not), a deletion's START to START is outside
    b = f.ins_base(1100)
    f.add("INS gap by start, not by end", [INS(b, "A" * 40, "a", span=300), INS(b + 1001, "A" * 40, "b", span=300)], parts=[[0], [1]], covers=[("partition gap INS", "above")])
    b = f.base()
    f.add("DUP_INT gap by destination start, not destination end", [DINT(b, b + 600, "a", b + 500000), DINT(b + 10, b + 610, "b", b + 501001)], parts=[[0], [1]],
          covers=[("partition gap DUP_INT", "above")])
    b = f.base()
    f.add("BND gap from pos1 + 1", [BND(b, b + 700000, "a"), BND(b + 1001, b + 700000, "b"), BND(b + 2003, b + 700000, "c")], parts=[[0, 1], [2]],
          covers=[("partition gap BND", "on"), ("partition gap BND", "above")])
    # a negative gap: a long deletion that contains later, shorter ones - sorted by END, so the long one comes last and its start lies far before the previous end
    b = f.base()
    f.add("DEL long contains shorter, sorted by end", [DEL(b, b + 9000, "long"), DEL(b + 100, b + 300, "s1"), DEL(b + 4000, b + 4100, "s2"), DEL(b + 5000, b + 5200, "s3")],
          parts=[[1], [2, 3, 0]], covers=[("partition gap DEL", "below"), ("negative gap", "below")])
    b = f.base()
    f.add("INV negative gap keeps the partition", [INV(b + 3000, b + 3100, "a"), INV(b, b + 5000, "b"), INV(b + 5500, b + 5600, "c")], parts=[[0, 1, 2]],
          covers=[("negative gap", "below")])
    # sorted by start (INS) and not by end: the longer insertion starts first and ends last
    b = f.ins_base(400)
    f.add("INS key is the start", [INS(b + 200, "ACGT" * 10, "b", span=50), INS(b + 100, "ACGT" * 10, "a", span=500)], parts=[[1, 0]])
    # equal keys keep list order, in both list orders (which duplicate is dropped depends on it: the LATER one of the same read)
    b = f.base()
    f.add("DEL equal keys, list order a b", [DEL(b, b + 300, "x"), DEL(b + 100, b + 300, "x"), DEL(b + 50, b + 300, "y")], parts=[[0, 1, 2]], clusters=[[0, 2]])
    b = f.base()
    f.add("DEL equal keys, list order b a", [DEL(b + 100, b + 300, "x"), DEL(b, b + 300, "x"), DEL(b + 50, b + 300, "y")], parts=[[0, 1, 2]], clusters=[[0, 2]])
    b = f.base()
    f.add("BND equal keys both orders", [BND(b, b + 700200, "x"), BND(b, b + 700000, "x"), BND(b, b + 700100, "y")], parts=[[0, 1, 2]], clusters=[[0, 2]])
    # BND: one source contig, different destination contigs, inside the distance: ONE partition; the cluster's destination contig is its first member's
    b = f.base()
    f.add("BND destinations on two contigs", [BND(b, 5000, "a", contig2="chr2"), BND(b + 100, 5100, "b", contig2="chr10"), BND(b + 200, 5050, "c", contig2="chr2")],
          parts=[[0, 1, 2]], clusters=[[0, 1, 2]])
    b = f.base()
    f.add("BND destinations on two contigs, chr10 first", [BND(b, 5000, "a", contig2="chr10"), BND(b + 100, 5100, "b", contig2="chr2")], parts=[[0, 1]], clusters=[[0, 1]])
    # DUP_INT: one destination contig, different source contigs, inside the distance: separate partitions (key: destination contig, SOURCE contig, destination start)
    b = f.base()
    f.add("DUP_INT sources on two contigs", [DINT(b, b + 300, "a", b + 500000, contig="chr1", contig2="chr2"), DINT(b, b + 300, "b", b + 500100, contig="chr10", contig2="chr2"),
                                             DINT(b, b + 300, "c", b + 500050, contig="chr1", contig2="chr2"), DINT(b, b + 300, "d", b + 500150, contig="chr2", contig2="chr2")],
          parts=[[0, 2], [1], [3]], clusters=[[0, 2], [1], [3]])
    b = f.base()
    f.add("DUP_INT key order: destination contig before source contig",
          [DINT(b, b + 300, "a", b + 500000, contig="chr2", contig2="chr1"), DINT(b, b + 300, "b", b + 500000, contig="chr1", contig2="chr2"),
           DINT(b, b + 300, "c", b + 500000, contig="chr1", contig2="chr10"), DINT(b, b + 300, "d", b + 500000, contig="chr10", contig2="chr1")], parts=[[3], [0], [2], [1]])
    # contig names whose string order differs from their numeric order: chr10 sorts before chr2
    b = f.base()
    f.add("DEL on chr2, chr10, chr1", [DEL(b, b + 100, "a", "chr2"), DEL(b, b + 100, "b", "chr10"), DEL(b, b + 100, "c", "chr1"), DEL(b + 50, b + 150, "d", "chr10")],
          parts=[[2], [1, 3], [0]], clusters=[[2], [1, 3], [0]])
    return f


def pmd0():
    f = Family("pmd0", partition_max_distance=0)
    for typ in TYPES:
        for gap, side in ((0, "on"), (1, "above")):
            b = f.ins_base(100) if typ == "INS" else f.base()
            one = side == "on"
            f.add("%s gap %d" % (typ, gap), gap_rows(typ, b, gap), parts=[[0, 1]] if one else [[0], [1]], covers=[("partition_max_distance 0", side)])
    b = f.base()
    f.add("DEL overlap", [DEL(b, b + 500, "a"), DEL(b + 400, b + 600, "b"), DEL(b + 601, b + 700, "c")], parts=[[0, 1], [2]], covers=[("partition_max_distance 0", "below")])
    return f


# ---- the sample switch: `> 100` before random.sample -----------------------------------------------------------------------------------------------------------------
def block(typ, b, n, prefix="r", seq="ACGTACGTTTGACCAGTACA"):
    """n identical signatures of n reads"""
    if typ == "INS":
        return [INS(b, seq, "%s%d" % (prefix, k)) for k in range(n)]
    if typ == "BND":
        return [BND(b, b + 700000, "%s%d" % (prefix, k), "rev", "fwd") for k in range(n)]
    return [span_row(typ, b, b + 300, "%s%d" % (prefix, k)) for k in range(n)]


def sample():
    f = Family("sample", independent=False)
    for typ in TYPES:
        for n, side in ((100, "on"), (101, "above")):
            b = f.ins_base(100) if typ == "INS" else f.base()
            f.add("%s partition of %d" % (typ, n), block(typ, b, n), parts=[list(range(n))], counts={typ: 1}, covers=[("sample switch " + typ, side), ("cluster size 80", "above")],
                  pairs=[(0, 1), (n - 1, 0)])
    # a second and third partition of one type draw from the same stream: distinguishable members (two alleles), so the sample shows in the member lists
    b = f.base()
    rows = [DEL(b + (k % 2) * 700, b + (k % 2) * 700 + 300 + k % 3, "r%d" % k) for k in range(150)]
    f.add("DEL partition of 150, two alleles", rows, counts={"DEL": 2}, pairs=[(0, 1), (0, 2)])
    b = f.base()
    rows = [DEL(b + (k % 3) * 600, b + (k % 3) * 600 + 200, "r%d" % k) for k in range(103)]
    f.add("DEL partition of 103, three alleles", rows, counts={"DEL": 3}, pairs=[(0, 1), (0, 3)])
    return f


# ---- the default options: duplicates, the distance function, the cut, consolidation and score -----------------------------------------------------------------------
def ins_pair_seqs():
    """two 40-base insertions at one place whose haplotypes are 20 / 21 edits apart: distance 20 / 40 = 0.5 and 21 / 40"""
    a = "A" * 40
    return a, "A" * 20 + "C" * 20, "A" * 19 + "C" * 21


def main():
    f = Family("main")
    rng = random.Random(20250131)
    # -- same-read duplicates: the distance of two signatures of ONE read exactly at the cut (dropped) and just above it (kept, distance 99999) --
    for typ in ("DEL", "DUP_TAN"):
        for d, side in ((450, "on"), (451, "above")):
            b = f.base()
            f.add("%s same read %d apart" % (typ, d), [span_row(typ, b, b + 200, "x"), span_row(typ, b + d, b + 200 + d, "x")], parts=[[0, 1]],
                  clusters=[[0]] if side == "on" else [[0], [1]], covers=[("same-read duplicate " + typ, side)])
    for d, side in ((450, "on"), (451, "above")):          # DUP_INT: the DESTINATION term carries it over (sources identical)
        b = f.base()
        f.add("DUP_INT same read, destinations %d apart" % d, [DINT(b, b + 200, "x", b + 500000), DINT(b, b + 200, "x", b + 500000 + d)], parts=[[0, 1]],
              clusters=[[0]] if side == "on" else [[0], [1]], covers=[("same-read duplicate DUP_INT", side)])
    for d1, d2, side in ((700, 800, "on"), (700, 801, "above"), (1000, 500, "on"), (1000, 501, "above")):          # BND: (d1 + d2) / 3000 at 1500
        b = f.base()
        f.add("BND same read %d + %d" % (d1, d2), [BND(b, b + 700000, "x"), BND(b + d1, b + 700000 + d2, "x")], parts=[[0, 1]],
              clusters=[[0]] if side == "on" else [[0], [1]], covers=[("same-read duplicate BND", side)])
    s0, s20, s21 = ins_pair_seqs()
    for other, side in ((s20, "on"), (s21, "above")):          # INS: through the edit distance
        b = f.ins_base(100)
        f.add("INS same read, %d edits" % (20 if side == "on" else 21), [INS(b, s0, "x"), INS(b, other, "x")], parts=[[0, 1]],
              clusters=[[0]] if side == "on" else [[0], [1]], covers=[("same-read duplicate INS", side)])
    # the chain a~b, b~c, not a~c: c is dropped because of b although b is itself dropped
    b = f.base()
    f.add("DEL chain of one read", [DEL(b, b + 200, "x"), DEL(b + 300, b + 500, "x"), DEL(b + 600, b + 800, "x")], parts=[[0, 1, 2]], clusters=[[0]],
          covers=[("dropped by a dropped element", "on")])
    # the earlier element is dropped by a still earlier one, the later one is near the dropped one only, and a read between them
    b = f.base()
    f.add("DEL dropped by a dropped element, another read between", [DEL(b, b + 200, "x"), DEL(b + 150, b + 350, "y"), DEL(b + 300, b + 500, "x"), DEL(b + 600, b + 800, "x"),
                                                                   DEL(b + 650, b + 850, "y")], parts=[[0, 1, 2, 3, 4]], clusters=[[0, 1], [4]],
          covers=[("dropped by a dropped element", "on")])
    # INV is exempt: two complementary signatures of one read stay and cluster together
    b = f.base()
    f.add("INV two left signatures of one read", [INV(b, b + 800, "x", "left_fwd"), INV(b + 10, b + 810, "x", "left_rev")], clusters=[[0, 1]], covers=[("INV exemption", "on")])
    b = f.base()
    f.add("INV identical signatures of one read", [INV(b, b + 800, "x", "left_fwd"), INV(b, b + 800, "x", "right_rev"), INV(b + 5, b + 800, "y", "all")], clusters=[[0, 1, 2]],
          covers=[("INV exemption", "on")])
    # the removal leaves exactly one member (no linkage); every row from one read
    b = f.base()
    f.add("DUP_TAN five of one read, one survivor", [TAN(b + 7 * k, b + 300 + 7 * k, "x", 1 + k % 3) for k in range(5)], parts=[[0, 1, 2, 3, 4]], clusters=[[0]],
          covers=[("members n > 1", "on")])
    b = f.base()
    f.add("DEL all of one read, none a duplicate", [DEL(b + 460 * k, b + 100 + 460 * k, "x") for k in range(4)], parts=[[0, 1, 2, 3]], clusters=[[0], [1], [2], [3]])
    # survivors of one read that are not duplicates: 99999, never merged - although a member of another read between them is near both (average 0.45 without it)
    b = f.base()
    f.add("DEL survivors of one read and a bridge", [DEL(b, b + 100, "x"), DEL(b + 270, b + 370, "y"), DEL(b + 540, b + 640, "x")], parts=[[0, 1, 2]],
          clusters=[[0, 1], [2]], covers=[("same-read survivors 99999", "on"), ("nearest neighbour tie", "on")])
    # ... and with a whole cluster between them: with any finite distance in the place of 99999 (1.0, say) the average over six members would pass the cut
    b = f.base()
    f.add("BND survivors of one read and a cluster of five", [BND(b, b + 700000, "x"), BND(b, b + 701650, "x")] + [BND(b, b + 700600, "r%d" % k) for k in range(5)],
          parts=[list(range(7))], clusters=[[0, 2, 3, 4, 5, 6], [1]], covers=[("same-read survivors 99999", "on")])
    b = f.base()
    f.add("DEL the same bridge, three reads", [DEL(b, b + 100, "x"), DEL(b + 270, b + 370, "y"), DEL(b + 540, b + 640, "z")], parts=[[0, 1, 2]], clusters=[[0, 1, 2]])

    # -- the distance function --
    b = f.base()          # max(span1, span2) from either side; centres from odd sums (// 2)
    f.add("DEL spans 100 and 200, either order", [DEL(b, b + 100, "a"), DEL(b + 3, b + 203, "b"), DEL(b + 1, b + 102, "c"), DEL(b + 2, b + 55, "d")], parts=[[3, 0, 2, 1]])
    b = f.base()
    f.add("INV odd sums", [INV(b + 1, b + 100, "a"), INV(b + 2, b + 105, "b"), INV(b + 3, b + 104, "c"), INV(b, b + 101, "d")], counts={"INV": 1})
    b = f.base()
    f.add("DUP_TAN odd sums and unequal spans", [TAN(b + 1, b + 300, "a"), TAN(b + 4, b + 511, "b", 3), TAN(b + 2, b + 301, "c", 2)], clusters=[[0, 2], [1]])
    b = f.base()          # BND: all sixteen ordered pairs of direction pairs - equal ones finite, unequal ones 99999
    dirs = [("fwd", "fwd"), ("fwd", "rev"), ("rev", "fwd"), ("rev", "rev")]
    rows = [BND(b + 10 * k, b + 700000 + 7 * k, "a%d" % k, *dirs[k]) for k in range(4)] + [BND(b + 100 + 10 * k, b + 700050 + 7 * k, "b%d" % k, *dirs[k]) for k in range(4)]
    f.add("BND sixteen direction pairs", rows, parts=[list(range(8))], clusters=[[0, 4], [1, 5], [2, 6], [3, 7]], pairs=[(i, j) for i in range(4) for j in range(4, 8)],
          covers=[("BND directions", "on"), ("BND directions", "above")])
    b = f.base()          # DUP_INT: sources 200 apart, destinations 300 apart: 0.56 with the destination term, 0.22 without
    f.add("DUP_INT destination term", [DINT(b, b + 300, "a", b + 500000), DINT(b + 200, b + 500, "b", b + 500300)], parts=[[0, 1]], clusters=[[0], [1]])
    # INS on both sides of `> 2 * cluster_max_distance`: 900 / 900 = 1.0 is NOT above it (edit distance), 901 is (spans)
    for d, side in ((899, "below"), (900, "on"), (901, "above")):
        b = f.ins_base(1000)
        f.add("INS %d apart" % d, [INS(b, rseq(rng, 60), "a"), INS(b + d, rseq(rng, 45), "b")], parts=[[0, 1]], clusters=[[0], [1]], covers=[("INS far branch", side)])
    # INS: drop a MIDDLE element so that the survivors' numbers are not the sample's numbers (the edit distance is indexed by the number before the removal)
    b = f.ins_base(200)
    al = [rseq(rng, 50, "AC"), rseq(rng, 50, "GT")]
    rows = [INS(b, al[0], "x"), INS(b + 2, al[1], "p"), INS(b + 3, al[0], "x"), INS(b + 4, al[0], "q"), INS(b + 5, al[1], "p"), INS(b + 6, al[1], "s"), INS(b + 7, al[0], "t")]
    f.add("INS two alleles, middle elements dropped", rows, parts=[list(range(7))], clusters=[[0, 3, 6], [1, 5]], covers=[("INS edit index after removal", "on")])

    # -- the cut: fcluster(criterion='distance') --
    for d, side in ((449, "below"), (450, "on"), (451, "above")):
        for typ in ("DEL", "INV", "DUP_TAN", "DUP_INT"):
            b = f.base()
            f.add("%s two reads %d apart" % (typ, d), [span_row(typ, b, b + 200, "a"), span_row(typ, b + d, b + 200 + d, "b")] if typ != "DUP_INT" else
                  [DINT(b, b + 200, "a", b + 500000), DINT(b + d, b + 200 + d, "b", b + 500000)], clusters=[[0, 1]] if side != "above" else [[0], [1]],
                  covers=[("fcluster cut", side)])
    for d, side in ((1500, "on"), (1501, "above")):
        b = f.base()
        f.add("BND two reads %d apart" % d, [BND(b, b + 700000, "a"), BND(b + 600, b + 700000 + d - 600, "b")], clusters=[[0, 1]] if side == "on" else [[0], [1]],
              covers=[("fcluster cut", side)])
    # span term alone at the cut: equal centres, spans 100 and 200 (0.5), 100 and 202 (above)
    b = f.base()
    f.add("DEL spans 100 and 200, one centre", [DEL(b + 50, b + 150, "a"), DEL(b, b + 200, "b")], clusters=[[0, 1]], covers=[("fcluster cut", "on")])
    b = f.base()
    f.add("DEL spans 100 and 202, one centre", [DEL(b + 51, b + 151, "a"), DEL(b, b + 202, "b")], clusters=[[0], [1]], covers=[("fcluster cut", "above")])
    # two merges of equal height (the merge table is sorted stably) - bilocal, so the order of the clusters in the output is the order of their labels
    b = f.base()
    f.add("DUP_TAN two merges of equal height", [TAN(b + 600, b + 800, "a"), TAN(b, b + 200, "b"), TAN(b + 700, b + 900, "c"), TAN(b + 100, b + 300, "d"), TAN(b + 1300, b + 1500, "e")],
          clusters=[[0, 2], [1, 3], [4]], covers=[("equal merge heights", "on")])
    b = f.base()
    f.add("DUP_TAN three merges of equal height, interleaved", [TAN(b + 1200, b + 1400, "a"), TAN(b, b + 200, "b"), TAN(b + 600, b + 800, "c"), TAN(b + 1300, b + 1500, "d"),
                                                               TAN(b + 100, b + 300, "e"), TAN(b + 700, b + 900, "f")], clusters=[[0, 3], [1, 4], [2, 5]],
          covers=[("equal merge heights", "on")])
    # a three-way tie for the nearest neighbour: the lowest index wins
    b = f.base()
    # (a at 360 has b at 0, c at 720 and e - its own centre, span 120 against 200 - all at 0.4; in sorted order b e a c)
    f.add("DUP_TAN three-way tie", [TAN(b + 360, b + 560, "a"), TAN(b, b + 200, "b"), TAN(b + 720, b + 920, "c"), TAN(b + 400, b + 520, "e", 2)], clusters=[[0, 1], [2], [3]],
          covers=[("nearest neighbour tie", "on")])
    b = f.base()
    f.add("DEL equidistant line", [DEL(b + 360, b + 560, "a"), DEL(b, b + 200, "b"), DEL(b + 720, b + 920, "c")], clusters=[[0, 1], [2]], covers=[("nearest neighbour tie", "on")])

    # which slot keeps a merged pair (the higher one): a and b merge first, c sits between them in the partition's order, and p is as far from {a, b} as from c.
    # The next chain starts at the lowest live slot - c, which takes p; kept in the lower slot, {a, b} would start it and take p itself.  (BND: one pos1, so the
    # order is the list's, and the distances come from pos2 alone)
    b = f.base()
    f.add("BND merged pair keeps the higher slot", [BND(b, b + 700000, "a"), BND(b, b + 702400, "c"), BND(b, b + 700000, "b"), BND(b, b + 701200, "p")], parts=[[0, 1, 2, 3]],
          clusters=[[0, 2], [1, 3]], covers=[("nearest neighbour tie", "on")])

    # -- consolidation and score --
    # averages on exact halves, even and odd integer parts (int(round(x)) rounds half to even), start, end and the destination pair
    for k, side in ((0, "even"), (1, "odd")):
        b = f.base() + k          # b even: starts b and b + 1 average to b + 0.5 (even integer part), with k = 1 to an odd one
        f.add("DEL average on a half, %s part" % side, [DEL(b, b + 300, "a"), DEL(b + 1, b + 303, "b")], clusters=[[0, 1]], covers=[("round half, %s part" % side, "on")])
        b = f.base() + k
        f.add("DUP_INT average on a half, %s part" % side, [DINT(b, b + 300, "a", b + 500000), DINT(b + 1, b + 303, "b", b + 500003)], clusters=[[0, 1]],
              covers=[("round half, %s part" % side, "on")])
        b = f.base() + k
        f.add("BND average on a half, %s part" % side, [BND(b, b + 700000, "a", "rev", "rev"), BND(b + 1, b + 700003, "b", "rev", "rev")], clusters=[[0, 1]],
              covers=[("round half, %s part" % side, "on")])
        b = f.base() + k
        f.add("DUP_TAN average on a half, %s part" % side, [TAN(b, b + 300, "a", 1), TAN(b + 3, b + 301, "b", 4)], clusters=[[0, 1]], covers=[("round half, %s part" % side, "on")])
    b = f.base()
    f.add("DEL four members, average on .25 and .75", [DEL(b, b + 300, "a"), DEL(b, b + 301, "b"), DEL(b, b + 301, "c"), DEL(b + 1, b + 301, "d")], clusters=[[0, 1, 2, 3]])
    # one-member clusters (None deviations; the DUP_INT and BND branches that take them) and identical members (deviation exactly 0.0)
    b = f.base()
    f.add("one member of every type", [DEL(b, b + 77, "a"), INV(b, b + 77, "b", "left_fwd"), INV(b + 5000, b + 5077, "b2", "all"), TAN(b, b + 77, "c", 3),
                                        DINT(b, b + 77, "d", b + 500000), BND(b, b + 700000, "e", "rev", "fwd")], counts={"DEL": 1, "INV": 2, "DUP_TAN": 1, "DUP_INT": 1, "BND": 1},
          covers=[("members n > 1", "on")])
    for typ in TYPES:
        b = f.ins_base(100) if typ == "INS" else f.base()
        f.add("%s two identical members" % typ, block(typ, b, 2), clusters=[[0, 1]], covers=[("members n > 1", "above"), ("std / span vs 1", "below")])
    # std / span on both sides of 1 (min(1, .)): spans 10 and 11 with centres 300 apart (std_pos 212 > span 10.5: above; std_span 0.7: below), spans 1000 (below).
    # (std_span cannot pass the span inside one cluster: two spans within the cut differ by at most half the larger one)
    b = f.base()
    f.add("DEL std_pos above the span", [DEL(b, b + 10, "a"), DEL(b + 300, b + 311, "b")], clusters=[[0, 1]], covers=[("std / span vs 1", "above")])
    b = f.base()
    f.add("DUP_INT mean deviations above the span", [DINT(b, b + 10, "a", b + 500000), DINT(b + 150, b + 161, "b", b + 500150)], clusters=[[0, 1]], covers=[("std / span vs 1", "above")])
    b = f.base()
    f.add("BND deviations on both sides of 500", [BND(b, b + 700000, "a"), BND(b + 900, b + 700600, "b")], clusters=[[0, 1]], covers=[("std / span vs 1", "above"), ("std / span vs 1", "below")])
    b = f.base()
    f.add("DEL std below the span", [DEL(b, b + 1000, "a"), DEL(b + 30, b + 1040, "b"), DEL(b + 10, b + 990, "c")], clusters=[[0, 1, 2]], covers=[("std / span vs 1", "below")])
    # cluster sizes 79, 80, 81 (min(80, .)); 100 is in `shape` and `sample`
    for n, side in ((79, "below"), (80, "on"), (81, "above")):
        b = f.base()
        f.add("DEL cluster of %d" % n, [DEL(b + k % 5, b + 300 + k % 7, "r%d" % k) for k in range(n)], counts={"DEL": 1}, covers=[("cluster size 80", side)], pairs="some")
        b = f.base()
        f.add("BND cluster of %d" % n, [BND(b + k % 5, b + 700000 + k % 7, "r%d" % k, "fwd", "rev") for k in range(n)], counts={"BND": 1}, covers=[("cluster size 80", side)], pairs="some")
    # INV direction counts: min(left, right) + all
    inv = {"only left": (["left_fwd", "left_rev", "left_fwd"], "below"), "only right": (["right_rev", "right_fwd"], "above"),
           "left < right": (["left_fwd", "right_fwd", "right_rev", "right_rev"], "below"), "right < left": (["left_fwd", "left_rev", "left_rev", "right_fwd"], "above"),
           "left = right": (["left_fwd", "right_fwd", "left_rev", "right_rev"], "on"), "all alone": (["all", "all", "all"], "on"),
           "all with both sides": (["all", "left_fwd", "left_rev", "right_rev", "all"], "above")}
    for name, (ds, side) in inv.items():
        b = f.base()
        f.add("INV " + name, [INV(b + k, b + 900 + 2 * k, "r%d" % k, d) for k, d in enumerate(ds)], clusters=[list(range(len(ds)))], covers=[("INV left vs right", side)])
    for n, side in ((79, "below"), (80, "on"), (81, "above")):          # 100 signatures, 100 - n on each side and 2 n - 100 `all`: n valid
        b = f.base()
        ds = ["all"] * (2 * n - 100) + ["left_fwd"] * (100 - n) + ["right_rev"] * (100 - n)
        f.add("INV %d valid of 100" % n, [INV(b + k % 3, b + 900 + k % 4, "r%d" % k, d) for k, d in enumerate(ds)], counts={"INV": 1}, covers=[("INV valid 80", side)], pairs="some")
    # DUP_TAN: max(copies) from a member that is not the first; the destination end from the ROUNDED start and end
    b = f.base()
    f.add("DUP_TAN max copies in the middle", [TAN(b, b + 300, "a", 2), TAN(b + 2, b + 301, "b", 7), TAN(b + 1, b + 302, "c", 3)], clusters=[[0, 1, 2]])
    # DUP_INT: the mean of the source and destination deviations (sources identical, destinations spread, and the other way round)
    b = f.base()
    f.add("DUP_INT destinations spread", [DINT(b, b + 400, "a", b + 500000), DINT(b, b + 400, "b", b + 500090), DINT(b, b + 400, "c", b + 500041)], clusters=[[0, 1, 2]])
    b = f.base()
    f.add("DUP_INT sources spread", [DINT(b, b + 400, "a", b + 500000), DINT(b + 80, b + 470, "b", b + 500000), DINT(b + 33, b + 440, "c", b + 500000)], clusters=[[0, 1, 2]])
    # BND: (source std_pos, destination std_pos) with 500 as the span
    b = f.base()
    f.add("BND source spread only", [BND(b, b + 700000, "a", "rev", "rev"), BND(b + 300, b + 700000, "b", "rev", "rev"), BND(b + 100, b + 700000, "c", "rev", "rev")], clusters=[[0, 1, 2]])
    b = f.base()
    f.add("BND destination spread only", [BND(b, b + 700000, "a", "fwd", "rev"), BND(b, b + 700700, "b", "fwd", "rev"), BND(b, b + 700350, "c", "fwd", "rev")], clusters=[[0, 1, 2]])
    # a table that mixes insertions and the other types in one stretch of chr1 (the device runs the two in different phases)
    b = f.ins_base(1500)
    al = [rseq(rng, 70, "AC"), rseq(rng, 64, "GT")]
    rows = []
    for k in range(12):
        rows.append(INS(b + k // 2, al[k % 2], "i%d" % k))
        rows.append(DEL(b + 3 * k, b + 200 + 3 * k + 300 * (k % 2), "d%d" % k))
        if k % 4 == 0:
            rows.append(INV(b + k, b + 700 + k, "v%d" % k, ("left_fwd", "right_rev", "all")[k // 4]))
    f.add("mixed types on one stretch", rows, counts={"INS": 2, "DEL": 2, "INV": 1}, pairs="some")
    return f


def cmd0():
    """cluster_max_distance 0.0: height 0 <= 0 merges identical signatures, anything else stays apart; a same-read duplicate needs distance 0"""
    f = Family("cmd0", cluster_max_distance=0.0)
    for typ in TYPES:
        b = f.ins_base(100) if typ == "INS" else f.base()
        f.add("%s identical" % typ, block(typ, b, 3), clusters=[[0, 1, 2]], covers=[("cluster_max_distance 0", "on")])
    b = f.base()
    f.add("DEL one base apart", [DEL(b, b + 200, "a"), DEL(b + 2, b + 202, "b"), DEL(b, b + 200, "c")], clusters=[[0, 2], [1]], covers=[("cluster_max_distance 0", "above")])
    b = f.base()
    f.add("BND same read identical and not", [BND(b, b + 700000, "x"), BND(b, b + 700000, "x"), BND(b, b + 700001, "x")], clusters=[[0], [2]], covers=[("cluster_max_distance 0", "on")])
    b = f.ins_base(100)
    f.add("INS every pair takes the far branch but the identical ones", [INS(b, "ACGTAACCGGTT" * 3, "a"), INS(b + 1, "ACGTAACCGGTT" * 3, "b"), INS(b, "ACGTAACCGGTT" * 3, "c")],
          clusters=[[0, 2], [1]], covers=[("cluster_max_distance 0", "above")])
    return f


def int32():
    """coordinates near 2^31 - 1, every output of the reference still an int32 (DUP_TAN's destination end = end + copies * span is the largest)"""
    f = Family("int32")
    top = 2 ** 31 - 1
    b = top - 5000
    f.add("DEL near the top", [DEL(b, b + 300, "a"), DEL(b + 101, b + 400, "b"), DEL(top - 201, top, "c"), DEL(top - 200, top - 1, "d")], parts=[[0, 1], [3, 2]], clusters=[[0, 1], [2, 3]])
    f.add("INV near the top", [INV(b, b + 301, "a", "left_fwd"), INV(b + 100, b + 400, "a", "right_rev"), INV(top - 3, top, "c")], parts=[[0, 1], [2]], clusters=[[0, 1], [2]])
    f.add("DUP_TAN near the top", [TAN(b, b + 300, "a", 2), TAN(b + 1, b + 301, "b", 9), TAN(top - 150, top - 50, "c", 0)], parts=[[0, 1], [2]], clusters=[[0, 1], [2]])
    f.add("DUP_INT near the top", [DINT(b, b + 300, "a", top - 700), DINT(b + 1, b + 303, "b", top - 603), DINT(top - 100, top, "c", 5)], clusters=[[0, 1], [2]])
    f.add("BND near the top", [BND(top - 3, top - 1, "a", "rev", "rev"), BND(top - 2, top - 2, "b", "rev", "rev"), BND(top - 1600, top - 1, "c", "rev", "rev")], clusters=[[0, 1], [2]])
    return f


# ---- the device's own edges (csrc/cluster.hip: k_cluster) ----------------------------------------------------------------------------------------------------------
SHAPE_SIZES = (48, 49, 72, 73, 100)
SHAPE_TYPES = ("DEL", "DUP_INT", "INS")          # a unilocal type, a bilocal type, insertions


def spread(typ, b, k, read, seq, step):
    """member k of a partition whose neighbours are `step` bases apart (inside partition_max_distance, outside cluster_max_distance)"""
    if typ == "INS":
        return INS(b + step * k, seq, read)
    if typ == "DUP_INT":
        return DINT(b + step * k, b + step * k + 100, read, b + 500000 + 10 * k)
    if typ == "BND":
        return BND(b + 800 * k, b + 700000 + 800 * k, read, "rev", "fwd")
    return span_row(typ, b + step * k, b + step * k + 100, read)


def interleaved(typ, b, k, read, seq):
    """member k of a partition of two clusters whose members alternate in the partition's order (even k one cluster, odd k the other)"""
    if typ == "INS":
        return INS(b, seq if k % 2 == 0 else seq.translate(str.maketrans("ACGT", "GTAC")), read)
    if typ == "DUP_INT":
        return DINT(b + 600 * (k % 2), b + 600 * (k % 2) + 100, read, b + 500000 + k)
    return span_row(typ, b + 1000 + k - (100, 300)[k % 2], b + 1000 + k, read)


def shape():
    f = Family("shape")
    rng = random.Random(48497273)
    seq = rseq(rng, 24)
    for typ in SHAPE_TYPES:
        for n in SHAPE_SIZES:
            b = f.ins_base(100) if typ == "INS" else f.base()
            cov = [("LDS class 48 | 49", {48: "on", 49: "above"}.get(n)), ("LDS class 72 | 73", {72: "on", 73: "above"}.get(n)), ("LDS class 100", "on" if n == 100 else None)]
            f.add("%s %d in one cluster" % (typ, n), block(typ, b, n, seq=seq), parts=[list(range(n))], clusters=[list(range(n))],
                  covers=[c for c in cov if c[1]] + [("clusters per partition 64", "below")], pairs=[(0, 1), (n - 1, 0)])
        for n in (65, 100):
            step = 451 if typ == "INS" else 500
            b = f.ins_base(step * n) if typ == "INS" else f.base()
            f.add("%s %d singletons" % (typ, n), [spread(typ, b, k, "r%d" % k, seq, step) for k in range(n)], parts=[list(range(n))], clusters=[[k] for k in range(n)],
                  covers=[("clusters per partition 64", "above")], pairs="some")
        # mixed cluster sizes in a partition of 100: neighbouring scratch ranges both in use
        step = 460 if typ == "INS" else 600
        b = f.ins_base(step) if typ == "INS" else f.base()
        f.add("%s 1 + 99" % typ, [spread(typ, b, 0, "r0", seq, step)] + [spread(typ, b, 1, "r%d" % k, seq, step) for k in range(1, 100)], parts=[list(range(100))],
              clusters=[[0], list(range(1, 100))], pairs=[(0, 1), (1, 2)])
        b = f.ins_base(step) if typ == "INS" else f.base()
        f.add("%s 50 + 50 interleaved" % typ, [interleaved(typ, b, k, "r%d" % k, seq) for k in range(100)], parts=[list(range(100))],
              clusters=[list(range(0, 100, 2)), list(range(1, 100, 2))], pairs=[(0, 1), (0, 2)])
        b = f.ins_base(step * 50) if typ == "INS" else f.base()
        f.add("%s fifty pairs" % typ, [spread(typ, b, k // 2, "r%d" % k, seq, step) for k in range(100)], clusters=[[2 * k, 2 * k + 1] for k in range(50)], pairs=[(0, 1), (1, 2)])
    b = f.base()
    f.add("BND 100 singletons", [spread("BND", b, k, "r%d" % k, seq, 0) for k in range(100)], parts=[list(range(100))], clusters=[[k] for k in range(100)],
          covers=[("clusters per partition 64", "above")], pairs="some")
    b = f.base()
    f.add("BND fifty pairs", [spread("BND", b, k // 2, "r%d" % k, seq, 0) for k in range(100)], clusters=[[2 * k, 2 * k + 1] for k in range(50)], pairs=[(0, 1), (1, 2)])
    # a large class that the duplicate removal brings down to 2 and to 1 (the class is chosen before the duplicates go)
    for typ in SHAPE_TYPES:
        b = f.ins_base(100) if typ == "INS" else f.base()
        rows = block(typ, b, 73, seq=seq)
        for k, r in enumerate(rows):
            r[5] = "x" if k != 40 else "y"
        f.add("%s 73 of two reads, 2 survive" % typ, rows, parts=[list(range(73))], clusters=[[0, 40]], pairs=[(0, 1)])
        b = f.ins_base(100) if typ == "INS" else f.base()
        rows = block(typ, b, 100, seq=seq)
        for r in rows:
            r[5] = "x"
        f.add("%s 100 of one read, 1 survives" % typ, rows, parts=[list(range(100))], clusters=[[0]], pairs=[(0, 99)])
    # survivors that are not the first elements: every third of 90 survives (orig[] far from the identity), two alleles among the survivors
    b = f.ins_base(100)
    al = [seq, rseq(rng, 24)]
    rows = [INS(b + (k // 3) % 2, al[(k // 3) % 2], "r%d" % (k // 3)) for k in range(90)]
    f.add("INS 90, every third survives", rows, parts=None, clusters=[[k for k in range(0, 90, 3) if (k // 3) % 2 == a] for a in (0, 1)], pairs=[(0, 3), (0, 6)])
    return f


def families():
    return [wide(), pmd0(), sample(), main(), cmd0(), int32(), shape()]


# ---- what the reference refuses -----------------------------------------------------------------------------------------------------------------------------------
REFUSED = [("DEL both spans zero", dict(OPTIONS), [DEL(5000, 5000, "a"), DEL(5000, 5000, "b")]),
           ("DUP_INT both spans zero, one read", dict(OPTIONS), [DINT(5000, 5000, "x", 900000), DINT(5000, 5000, "x", 900010)]),
           ("INS both spans zero, far apart", dict(OPTIONS), [INS(5000, "", "a"), INS(5950, "", "b")])]
EXPECTED_RAISES = {"DEL both spans zero": "ZeroDivisionError", "DUP_INT both spans zero, one read": "ZeroDivisionError", "INS both spans zero, far apart": "ZeroDivisionError"}


# ---- the coverage table: every threshold with the sides that must have a case -----------------------------------------------------------------------------------------
REQUIRED = dict([("partition gap " + t, ("on", "above")) for t in TYPES] + [("sample switch " + t, ("on", "above")) for t in TYPES] +
                [("same-read duplicate " + t, ("on", "above")) for t in ("DEL", "DUP_TAN", "DUP_INT", "BND", "INS")])
REQUIRED.update({"partition gap DEL": SIDES, "negative gap": ("below",), "partition_max_distance 0": SIDES, "dropped by a dropped element": ("on",), "INV exemption": ("on",),
                 "same-read survivors 99999": ("on",), "BND directions": ("on", "above"), "INS far branch": SIDES, "INS edit index after removal": ("on",),
                 "fcluster cut": SIDES, "cluster_max_distance 0": ("on", "above"), "equal merge heights": ("on",), "nearest neighbour tie": ("on",),
                 "round half, even part": ("on",), "round half, odd part": ("on",), "members n > 1": ("on", "above"), "std / span vs 1": ("below", "above"),
                 "cluster size 80": SIDES, "INV left vs right": SIDES, "INV valid 80": SIDES, "LDS class 48 | 49": ("on", "above"), "LDS class 72 | 73": ("on", "above"),
                 "LDS class 100": ("on",), "clusters per partition 64": ("below", "above")})


def coverage(fams=None):
    """{threshold: {side: [family / case, ...]}}"""
    table = {}
    for f in fams or families():
        for c in f.cases:
            for name, side in c.covers:
                assert side in SIDES, (c.name, name, side)
                table.setdefault(name, {}).setdefault(side, []).append("%s / %s" % (f.name, c.name))
    return table
