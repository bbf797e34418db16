"""Directed cases for COMBINE (csrc/combine.hip, five stages; tests/combine_consumer.py, the Python replay): a case below, on and above every comparison the
reference's merge_translocations_at_insertions, flag_cutpaste_candidates (src/svim/SVIM_merging.py:12-159) and combine_clusters (src/svim/SVIM_COMBINE.py:332-478,
with partition_and_cluster_candidates behind it) make, and the shapes at which the device takes another step: 8 insertion-from clusters per workgroup and 256
deletions per trip of k_cutpaste_min, the 64-entry register window and the 64-insertion tile of k_walk, the wave-wide member copies, the LDS classes of the linkage.
tests/golden/make_golden_combine_thresholds.py runs the reference on them (tests/golden/g_combine_threshold_cases.json.gz) and stops when the reference disagrees
with what a case's author wrote down; tests/test_combine_threshold_cases.py holds the replay to that file on the CPU, tests/test_gpu_combine_threshold_cases.py
the device.

A CASE is six lists of cluster rows over stand-in signatures, as tests/golden/make_golden_combine.py builds them (uni [contig, start, end, score, std_span,
std_pos, members]; bi [sc, ss, se, dc, ds, de, score, std_span, std_pos, members(, direction1, direction2)]), its options, `expect` - what its author says the
reference does - and `covers`: (comparison, side) pairs for the coverage table.  Keys of `expect` (each optional, each confirmed by the generator):
    remove_1, remove_2   insertion indices stage 2 merges / the stage 4 walk removes
    merged_src           [source_start, source_end] of every merged row = the destination starts of the two breakends that were chosen: says WHICH entry a search took
    merged_scores        score of every merged row (None: not stated)
    merged_members       member indices of every merged row
    cutpaste             the flag of every insertion-from cluster, CLUSTER's rows first, stage 2's behind them
    copies, fully        of every tandem candidate
    counts               candidates per class in combine_clusters' return order
    final_range          [fewest, most] re-clustered duplications
    final                [source_start, source_end, dest_start, dest_end, std_span, std_pos, cutpaste, score, members] of every re-clustered duplication
REFUSED: what the reference raises on; in no parity set.

Test infrastructure only; imports no GPU code and nothing of the reference."""
import random

OPT = dict(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000, cluster_max_distance=0.5,
           skip_consensus=True)
R = ["chr1", "chr2", "chr10"]                       # tid order != name order ("chr10" < "chr2")
TYPES = ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")
FAMILIES = ("stage1", "s2_distance", "s2_ratio", "s2_search", "s2_score", "stage3", "s3_shapes", "stage4", "s4_shapes", "stage5", "s5_shapes")
FAR = ("chr10", 90000000, 90000100)                 # a deletion no insertion-from cluster of any case is near


class Case(object):
    def __init__(self, family, name, **opt):
        self.family, self.name, self.references, self.opt = family, "%s/%s" % (family, name), list(R), dict(OPT, **opt)
        self.sigs, self.expect, self.covers = [], {}, []
        self.lists = {k: [] for k in TYPES}

    def mem(self, n, fully_covered=False, fc_at=()):
        out = []
        for k in range(n):
            self.sigs.append(bool(fully_covered) or k in fc_at)
            out.append(len(self.sigs) - 1)
        return out

    def uni(self, t, contig, start, end, score=10.0, std_span=1.5, std_pos=2.5, n=2):
        self.lists[t].append([contig, start, end, score, std_span, std_pos, self.mem(n)])
        return len(self.lists[t]) - 1

    def bi(self, t, sc, ss, se, dc, ds, de, score=10.0, std_span=1.5, std_pos=2.5, n=2, dirs=None, fully_covered=False, fc_at=()):
        row = [sc, ss, se, dc, ds, de, score, std_span, std_pos, self.mem(n, fully_covered, fc_at)]
        self.lists[t].append(row + (list(dirs) if dirs else []))
        return len(self.lists[t]) - 1

    def bnd(self, d, contig, pos, dest_contig, dest, end=None, dest_end=None, **kw):
        """one breakend cluster with both directions `d`; source end pos + 1 unless given"""
        return self.bi("BND", contig, pos, pos + 1 if end is None else end, dest_contig, dest, dest + 1 if dest_end is None else dest_end, dirs=(d, d), **kw)

    def flank(self, contig, fwd_pos, rev_pos, dest_contig, d1, d2, **kw):
        """fwd/fwd breakend at fwd_pos -> (dest_contig, d1) and rev/rev breakend at rev_pos -> (dest_contig, d2)"""
        self.bnd("fwd", contig, fwd_pos, dest_contig, d1, **kw)
        self.bnd("rev", contig, rev_pos, dest_contig, d2, **kw)

    def far_deletion(self, score=0.0):
        self.uni("DEL", FAR[0], FAR[1], FAR[2], score=score, n=1)

    def cover(self, *pairs):
        self.covers.extend(pairs)
        return self

    def says(self, **kw):
        self.expect.update(kw)
        return self


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------------------------------------------
def stage1_cases():
    out = []
    c = Case("stage1", "scores")                    # `score > 0` of the deletion and the novel insertion candidates (:464, prepare_insertion_candidates)
    for k, sc in enumerate((-1.0, 0.0, 5e-324, 1e-300)):
        c.uni("DEL", "chr1", 1000 + 1000 * k, 1100 + 1000 * k, score=sc)
        c.uni("INS", "chr2", 1000 + 1000 * k, 1100 + 1000 * k, score=sc)
    c.says(counts=[2, 0, 0, 0, 2, 0], remove_1=[], remove_2=[])
    c.cover(("DEL score > 0", "below"), ("DEL score > 0", "on"), ("DEL score > 0", "above"), ("INS score > 0", "below"), ("INS score > 0", "on"), ("INS score > 0", "above"))
    out.append(c)

    c = Case("stage1", "tandem_copies")             # int(round(quotient)): half-even
    for k, (src, dst) in enumerate(((200, 100), (200, 300), (200, 500), (200, 700), (200, 900), (200000000, 499999999), (200000000, 500000001))):
        s = 1000 + 5000 * k if src == 200 else 0
        c.bi("DUP_TAN", R[k % 3], s, s + src, R[k % 3], s + src, s + src + dst)
    c.says(copies=[0, 2, 2, 4, 4, 2, 3], counts=[0, 0, 0, 7, 0, 0])
    c.cover(("round(copies)", "x.5, x even"), ("round(copies)", "x.5, x odd"), ("round(copies)", "below x.5"), ("round(copies)", "above x.5"))
    out.append(c)

    c = Case("stage1", "fully_covered")             # True if sum(...) over the members: first only, last only, none; lists across the 64-lane copy
    want = []
    for n in (1, 64, 65, 130):
        for k, at in enumerate(((0,), (n - 1,), ())):
            s = 1000 * len(want) + 1000
            c.bi("DUP_TAN", "chr2", s, s + 100, "chr2", s + 100, s + 200, n=n, fc_at=at)
            want.append(bool(at))
    c.says(fully=want, copies=[1] * 12)
    c.cover(("fully_covered", "first"), ("fully_covered", "last"), ("fully_covered", "none"), ("member list", "1"), ("member list", "64"), ("member list", "65"), ("member list", "130"))
    out.append(c)

    c = Case("stage1", "start_clamps")              # max(0, start) of every candidate class; the clusters keep their negative starts
    c.uni("DEL", "chr1", -3, 400)
    c.uni("INS", "chr10", -3, 400)
    c.uni("INV", "chr2", -1, 50)
    c.bi("DUP_TAN", "chr2", -5, 95, "chr2", 95, 245)
    c.bi("DUP_INT", "chr2", -4, 300, "chr1", -7, 297)
    c.bi("BND", "chr1", -2, -1, "chr10", -9, -8, dirs=("fwd", "rev"))
    c.says(counts=[1, 1, 1, 1, 1, 1], copies=[2])
    c.cover(("max(0, start)", "DEL"), ("max(0, start)", "INS"), ("max(0, start)", "INV"), ("max(0, start)", "DUP_TAN"), ("max(0, start)", "DUP_INT"), ("max(0, start)", "BND"))
    out.append(c)

    c = Case("stage1", "bnd_directions")
    for k, d in enumerate((("fwd", "fwd"), ("fwd", "rev"), ("rev", "fwd"), ("rev", "rev"))):
        c.bi("BND", R[k % 3], 100 + k, 101 + k, R[(k + 1) % 3], 900 + k, 901 + k, dirs=d, std_span=None if k % 2 else 1.0, std_pos=None if k > 1 else 2.0)
    c.says(counts=[0, 0, 0, 0, 0, 4])
    c.cover(("BND directions", "fwd/fwd"), ("BND directions", "fwd/rev"), ("BND directions", "rev/fwd"), ("BND directions", "rev/rev"))
    out.append(c)
    return out


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------------------------------------------
def _ins(c, contig, s, ln=300, **kw):
    return c.uni("INS", contig, s, s + ln, **kw)


def s2_distance_cases():
    """abs(mean - ins_start) <= trans_sv_max_distance for the fwd/fwd AND the rev/rev list (:143): one list displaced to either side, the other on the insertion"""
    out = []
    c = Case("s2_distance", "one_list_displaced")
    c.far_deletion()
    rm = []
    k = 0
    for which in ("fwd", "rev"):
        for sgn in (1, -1):
            for d in (499, 500, 501):
                s = 100000 + 10000 * k
                i = _ins(c, "chr1", s)
                off = sgn * d
                c.flank("chr1", s + off if which == "fwd" else s, s + off if which == "rev" else s, "chr2", 100000 + 10000 * k, 100300 + 10000 * k)
                if d <= 500:
                    rm.append(i)
                c.cover(("%s: abs(mean - start) <= trans_sv_max_distance, mean %s start" % (which, ">" if sgn > 0 else "<"), "below" if d < 500 else "on" if d == 500 else "above"))
                k += 1
    for a, b in ((501, 501), (501, -501), (-501, -501), (500, -500), (-500, 500)):          # both outside / both on it, opposite sides
        s = 100000 + 10000 * k
        i = _ins(c, "chr1", s)
        c.flank("chr1", s + a, s + b, "chr2", 100000 + 10000 * k, 100300 + 10000 * k)
        if abs(a) <= 500:
            rm.append(i)
        k += 1
    c.cover(("both lists outside", "on"), ("both lists on the limit, opposite sides", "on"))
    c.says(remove_1=rm)
    out.append(c)

    c = Case("s2_distance", "limit_zero", trans_sv_max_distance=0)
    c.far_deletion()
    rm = []
    for k, (a, b) in enumerate(((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))):
        s = 100000 + 10000 * k
        i = _ins(c, "chr2", s)
        c.flank("chr2", s + a, s + b, "chr1", 100000 + 10000 * k, 100300 + 10000 * k)
        if (a, b) == (0, 0):
            rm.append(i)
    c.says(remove_1=rm)
    c.cover(("trans_sv_max_distance = 0", "on"), ("trans_sv_max_distance = 0", "above"))
    out.append(c)
    return out


def s2_ratio_cases():
    """0.95 <= (ins_end - ins_start + 1) / (distance + 1) <= 1.1 (:150), distance = abs of the difference of the two destination starts"""
    out = []
    c = Case("s2_ratio", "bounds")
    c.far_deletion()
    rm = []
    table = [  # (length, distance, merged, bound, side)
        (18998, 19999, False, "0.95", "below"), (188, 199, False, "0.95", "below"), (18, 19, True, "0.95", "on"), (189, 199, True, "0.95", "on"), (18999, 19999, True, "0.95", "on"),
        (19000, 19999, True, "0.95", "above"), (190, 199, True, "0.95", "above"),
        (21998, 19999, True, "1.1", "below"), (218, 199, True, "1.1", "below"), (10, 9, True, "1.1", "on"), (219, 199, True, "1.1", "on"), (21999, 19999, True, "1.1", "on"),
        (22000, 19999, False, "1.1", "above"), (220, 199, False, "1.1", "above")]
    for k, (ln, dist, merged, bound, side) in enumerate(table):
        s = 100000 + 50000 * k
        i = _ins(c, "chr1", s, ln)
        d = 100000 + 50000 * k
        if k % 2:
            c.flank("chr1", s, s, "chr2", d + dist, d)             # the rev/rev destination in front of the fwd/fwd one: abs(), min / max of the merged row
        else:
            c.flank("chr1", s, s, "chr2", d, d + dist)
        if merged:
            rm.append(i)
        c.cover(("%s against the length ratio" % bound, side))
    c.says(remove_1=rm, merged_src=[[100000 + 50000 * k, 100000 + 50000 * k + t[1]] for k, t in enumerate(table) if t[2]])
    out.append(c)

    c = Case("s2_ratio", "contigs_and_zero_distance")
    c.far_deletion()
    i0 = _ins(c, "chr1", 100000)                                     # destinations on different contigs, the ratio would be 1
    c.bnd("fwd", "chr1", 100000, "chr2", 5000)
    c.bnd("rev", "chr1", 100000, "chr10", 5300)
    i1 = _ins(c, "chr1", 200000, 0)                                  # distance 0 and an insertion of length 0: ratio 1 / 1
    c.flank("chr1", 200000, 200000, "chr2", 7000, 7000)
    i2 = _ins(c, "chr1", 300000, 300)                                # distance 0: ratio 301
    c.flank("chr1", 300000, 300000, "chr2", 9000, 9000)
    i3 = _ins(c, "chr1", 400000, 300)                                # the distance is between the destination STARTS: 300; the ends are 850 apart
    c.bnd("fwd", "chr1", 400000, "chr2", 15000, dest_end=15050)
    c.bnd("rev", "chr1", 400000, "chr2", 15300, dest_end=15900)
    c.says(remove_1=[i1, i3], merged_src=[[7000, 7000], [15000, 15300]])
    c.cover(("destination contigs equal", "below"), ("destination contigs equal", "on"), ("distance = 0", "on"), ("distance from destination starts", "on"))
    assert (i0, i2) == (0, 2)
    out.append(c)
    return out


def s2_search_cases():
    """get_closest_index (:32-50): bisect_left over the source STARTS of a list ordered by get_key() = source END"""
    out = []
    for n in (1, 2, 3, 40):
        c = Case("s2_search", "list_of_%d" % n)
        c.far_deletion()
        p0 = 100000
        for k in range(n):                                           # breakend k of either list at p0 + 200 k; only the pair (k, k) has destinations 300 apart
            c.bnd("fwd", "chr1", p0 + 200 * k, "chr2", 10000 * (k + 1))
        for k in reversed(range(n)):                                 # (the rev/rev list is handed over in descending order: the sort by key is what orders it)
            c.bnd("rev", "chr1", p0 + 200 * k, "chr2", 10000 * (k + 1) + 300)
        probes = [(p0 - 100, 0), (p0, 0), (p0 + 200 * (n - 1) + 50, n - 1)]           # pos == 0; on an entry; pos == len
        if n > 1:
            probes += [(p0 + 100, 0), (p0 + 101, 1), (p0 + 99, 0)]                    # a tie: the lower index; one step to either side
        if n > 3:
            probes += [(p0 + 200 * 19 + 100, 19), (p0 + 200 * 38 + 101, 39), (p0 + 200 * 39, 39)]
        src = []
        for s, k in probes:
            _ins(c, "chr1", s)
            src.append([10000 * (k + 1), 10000 * (k + 1) + 300])
        c.says(remove_1=list(range(len(probes))), merged_src=src)
        c.cover(("breakends per contig", str(n)), ("bisect: pos == 0", "on"), ("bisect: pos == len", "on"))
        if n > 1:
            c.cover(("after - x < x - before", "on"), ("after - x < x - before", "below"), ("after - x < x - before", "above"))
        out.append(c)

    c = Case("s2_search", "unsorted_starts")
    c.far_deletion()
    # fwd/fwd list on chr1 in key order (source end): B [1300, 1400), A [1000, 1600), C [1500, 1700): the starts 1300, 1000, 1500 are NOT sorted
    c.bnd("fwd", "chr1", 1000, "chr2", 10000, end=1600)              # A
    c.bnd("fwd", "chr1", 1300, "chr2", 20000, end=1400)              # B
    c.bnd("fwd", "chr1", 1500, "chr2", 30000, end=1700)              # C
    c.bnd("rev", "chr1", 1290, "chr2", 30300)                        # for the insertion at 1290: 300 behind C's destination
    c.bnd("rev", "chr1", 900, "chr2", 20300)                         # for the insertion at 900: 300 behind B's
    _ins(c, "chr1", 1290)     # bisect: mid 1 (1000 < 1290) -> lo 2; mid 2 (1500) -> pos 2; before 1000, after 1500: 210 < 290 -> C, although B at 1300 is 10 away
    _ins(c, "chr1", 900)      # mid 1 (1000 >= 900) -> hi 1; mid 0 (1300 >= 900) -> pos 0 -> B, 400 away, although A at 1000 is 100 away
    # the same through the rev/rev list and on chr2, where the list is made of MIRRORED clusters (source = the original's destination, any end)
    c.bi("BND", "chr10", 50000, 50001, "chr2", 1300, 1400, dirs=("fwd", "fwd"))       # mirrored: rev/rev chr2 [1300, 1400) -> chr10:50000     X
    c.bi("BND", "chr10", 60000, 60001, "chr2", 1000, 1600, dirs=("fwd", "fwd"))       # mirrored: rev/rev chr2 [1000, 1600) -> chr10:60000     Y
    c.bi("BND", "chr10", 70000, 70001, "chr2", 1500, 1700, dirs=("fwd", "fwd"))       # mirrored: rev/rev chr2 [1500, 1700) -> chr10:70000     Z
    c.bi("BND", "chr10", 70300, 70301, "chr2", 1290, 1291, dirs=("rev", "rev"))       # mirrored: fwd/fwd chr2:1290 -> chr10:70300
    _ins(c, "chr2", 1290)     # rev/rev starts in key order 1300, 1000, 1500 (then the mirrors of the chr1 breakends, far behind): Z at 1500, not X at 1300
    c.says(remove_1=[0, 1, 2], merged_src=[[30000, 30300], [20000, 20300], [70000, 70300]])
    c.cover(("bisect lands beside the nearest start", "pos inside"), ("bisect lands beside the nearest start", "pos == 0"), ("starts in key order", "unsorted"))
    out.append(c)

    c = Case("s2_search", "unsorted_pos_len")
    c.far_deletion()
    # key order by end: P [1500, 1550), Q [1000, 1600), S [1300, 1700): starts 1500, 1000, 1300; x = 1600: every start < x -> pos == len -> S at 1300, 300 away, P is 100 away
    c.bnd("rev", "chr2", 1300, "chr1", 30300, end=1700)              # S
    c.bnd("rev", "chr2", 1000, "chr1", 20300, end=1600)              # Q
    c.bnd("rev", "chr2", 1500, "chr1", 10300, end=1550)              # P
    c.bnd("fwd", "chr2", 1600, "chr1", 30000)
    _ins(c, "chr2", 1600)
    c.says(remove_1=[0], merged_src=[[30000, 30300]])
    c.cover(("bisect lands beside the nearest start", "pos == len"))
    out.append(c)

    c = Case("s2_search", "equal_keys_stable")
    c.far_deletion()
    c.bnd("fwd", "chr1", 5000, "chr2", 10000, end=5010)              # X and Y share the key (end 5010): list order X, Y -> starts 5000, 5004
    c.bnd("fwd", "chr1", 5004, "chr2", 20000, end=5010)
    c.bnd("rev", "chr1", 5003, "chr2", 20300)
    _ins(c, "chr1", 5003)     # pos 1; 5004 - 5003 < 5003 - 5000 -> Y.  In the other order (5004, 5000): pos == len -> the entry at 5000 = X: no merge
    # an original and a mirrored cluster with one key: the original comes first in the extended list
    c.bi("BND", "chr10", 8000, 8010, "chr2", 40000, 40001, dirs=("rev", "rev"))                 # original rev/rev chr10 [8000, 8010)
    c.bi("BND", "chr2", 50000, 50001, "chr10", 8004, 8010, dirs=("fwd", "fwd"))                 # mirrored: rev/rev chr10 [8004, 8010) -> chr2:50000
    c.bnd("fwd", "chr10", 8003, "chr2", 49700)
    _ins(c, "chr10", 8003)    # starts 8000, 8004 -> pos 1 -> the mirrored one at 8004 (destination chr2:50000; 300 from 49700)
    c.says(remove_1=[0, 1], merged_src=[[20000, 20300], [49700, 50000]])
    c.cover(("equal keys", "two originals"), ("equal keys", "original and mirrored"))
    out.append(c)

    c = Case("s2_search", "duplicate_starts")                        # bisect_left: the FIRST of two entries at the insertion's start
    c.far_deletion()
    c.bnd("fwd", "chr1", 12000, "chr2", 40000)
    c.bnd("fwd", "chr1", 12000, "chr2", 45000)
    c.bnd("rev", "chr1", 12000, "chr2", 40300)
    c.bnd("rev", "chr1", 12000, "chr2", 45300)
    _ins(c, "chr1", 12000)
    c.says(remove_1=[0], merged_src=[[40000, 40300]])
    c.cover(("two entries on the insertion's start", "on"))
    out.append(c)

    c = Case("s2_search", "mixed_directions")                        # the mirror of a fwd/rev cluster is fwd/rev, of a rev/fwd one rev/fwd: in neither list
    c.far_deletion()
    _ins(c, "chr2", 60000)
    c.bi("BND", "chr1", 70000, 70001, "chr2", 60000, 60001, dirs=("fwd", "rev"))
    c.bi("BND", "chr1", 70300, 70301, "chr2", 60000, 60001, dirs=("rev", "rev"))     # mirrored: fwd/fwd at chr2:60000 - its partner would be the mirror above
    _ins(c, "chr10", 60000)
    c.bi("BND", "chr1", 80000, 80001, "chr10", 60000, 60001, dirs=("rev", "fwd"))
    c.bi("BND", "chr1", 80300, 80301, "chr10", 60000, 60001, dirs=("fwd", "fwd"))    # mirrored: rev/rev at chr10:60000
    _ins(c, "chr2", 160000)                                          # the same with the partner in the other list
    c.bi("BND", "chr1", 170000, 170001, "chr2", 160000, 160001, dirs=("fwd", "rev"))
    c.bi("BND", "chr1", 170300, 170301, "chr2", 160000, 160001, dirs=("fwd", "fwd"))
    _ins(c, "chr10", 160000)
    c.bi("BND", "chr1", 180000, 180001, "chr10", 160000, 160001, dirs=("rev", "fwd"))
    c.bi("BND", "chr1", 180300, 180301, "chr10", 160000, 160001, dirs=("rev", "rev"))
    c.says(remove_1=[])
    c.cover(("mirror of a mixed-direction cluster", "fwd/rev"), ("mirror of a mixed-direction cluster", "rev/fwd"))
    out.append(c)

    c = Case("s2_search", "one_list_only")
    c.far_deletion()
    _ins(c, "chr10", 2000)
    c.bnd("fwd", "chr10", 2000, "chr1", 50000)                       # mirrored: rev/rev on chr1 - chr10 has no rev/rev list
    _ins(c, "chr2", 2000)
    c.bnd("rev", "chr2", 2000, "chr2", 90000)                        # mirrored: fwd/fwd on chr2 at 90000, out of reach... but chr2 now has both lists
    _ins(c, "chr1", 7000)                                            # chr1 has a rev/rev list only (the mirror of the first)
    c.says(remove_1=[])
    c.cover(("contig in one list only", "fwd/fwd only"), ("contig in one list only", "rev/rev only"))
    out.append(c)

    c = Case("s2_search", "mirrored_only")
    c.far_deletion()
    _ins(c, "chr2", 60000, score=8.0)
    c.bi("BND", "chr1", 70000, 70001, "chr2", 60010, 60011, dirs=("rev", "rev"), std_span=10.0, std_pos=30.0)     # mirrored: chr2:60010 fwd/fwd -> chr1:70000
    c.bi("BND", "chr1", 70300, 70301, "chr2", 59980, 59981, dirs=("fwd", "fwd"), std_span=50.0, std_pos=None)     # mirrored: chr2:59980 rev/rev -> chr1:70300
    # td 0.9 * 0.8; the mirror's std_span is the original's std_pos: ts 0.7 and 1 (None), ds 0.9 and 0.5
    c.says(remove_1=[0], merged_src=[[70000, 70300]], merged_scores=[pow(0.9 * 0.8 * 0.7 * 1 * 0.9 * 0.5, 1 / 6) * 8.0])
    c.cover(("matched through mirrored clusters only", "on"))
    out.append(c)
    return out


def s2_score_cases():
    """calculate_score_insertion (:57-90): max(0, 100 - x) / 100 of the two distances and the four stds (None: 1), pow(product, 1 / 6) * main score"""
    out = []
    c = Case("s2_score", "distances")
    c.far_deletion()
    want = []
    for k, (a, b) in enumerate(((99, 0), (100, 0), (101, 0), (0, -99), (0, -100), (0, -101))):
        s = 100000 + 10000 * k
        _ins(c, "chr1", s)
        c.flank("chr1", s + a, s + b, "chr2", s, s + 300, std_span=0.0, std_pos=0.0)
        d = max(abs(a), abs(b))
        want.append(pow(max(0, 100 - d) / 100, 1 / 6) * 10.0)
        c.cover(("max(0, 100 - distance)", "below" if d < 100 else "on" if d == 100 else "above"))
    c.says(remove_1=list(range(6)), merged_scores=want)
    out.append(c)

    c = Case("s2_score", "stds")
    c.far_deletion()
    want = []
    k = 0
    for slot in range(4):                                            # fwd std_span, rev std_span, fwd std_pos, rev std_pos
        for v in (99.5, 100.0, 100.5, None):
            s = 100000 + 10000 * k
            _ins(c, "chr2", s)
            std = [0.0, 0.0, 0.0, 0.0]
            std[slot] = v
            c.bnd("fwd", "chr2", s, "chr1", s, std_span=std[0], std_pos=std[2])
            c.bnd("rev", "chr2", s, "chr1", s + 300, std_span=std[1], std_pos=std[3])
            want.append(10.0 if v is None else pow(max(0, 100 - v) / 100, 1 / 6) * 10.0)
            c.cover(("max(0, 100 - std), slot %d" % slot, "None" if v is None else "below" if v < 100 else "on" if v == 100 else "above"))
            k += 1
    c.says(remove_1=list(range(16)), merged_scores=want)
    out.append(c)

    c = Case("s2_score", "main_score_zero")
    c.far_deletion()
    _ins(c, "chr1", 5000, score=0.0)
    c.flank("chr1", 5000, 5000, "chr2", 5000, 5300)
    _ins(c, "chr1", 50000, score=-2.0)
    c.flank("chr1", 50000, 50000, "chr2", 50000, 50300, std_span=None, std_pos=None)
    c.says(remove_1=[0, 1], merged_scores=[0.0, -2.0], counts=[0, 0, 2, 0, 0, 4])
    c.cover(("main score", "0"), ("main score", "negative"))
    out.append(c)

    c = Case("s2_score", "member_lists")
    c.far_deletion()
    sizes = (1, 63, 64, 65, 130)
    mem = []
    for k in range(5):
        s = 100000 + 10000 * k
        a, b, d = sizes[k], sizes[(k + 1) % 5], sizes[(k + 2) % 5]
        i = c.uni("INS", "chr1", s, s + 300, n=a)
        f = c.bnd("fwd", "chr1", s, "chr2", s, n=b)
        r = c.bnd("rev", "chr1", s, "chr2", s + 300, n=d)
        mem.append(c.lists["INS"][i][6] + c.lists["BND"][f][9] + c.lists["BND"][r][9])
        for x in (a, b, d):
            c.cover(("merged member list", str(x)))
    c.says(remove_1=list(range(5)), merged_members=mem)
    out.append(c)
    return out


# ---- stage 3 -------------------------------------------------------------------------------------------------------------------------------------------------------
def _dup(c, contig, s, e, k, **kw):
    """an insertion-from cluster with source contig:[s, e) and a destination of its own on chr10 (100000 apart: stage 5 keeps them apart)"""
    return c.bi("DUP_INT", contig, s, e, "chr10", 1000000 + 100000 * k, 1000000 + 100000 * k + (e - s), **kw)


def stage3_cases():
    """min over ALL deletion clusters of abs(centre1 - centre2) / normalizer + abs(span1 - span2) / max(span1, span2) <= del_ins_dup_max_distance (:17-23)"""
    out = []
    c = Case("stage3", "on_and_over_the_limit")
    want = []
    rows = [  # deletion [s, e), duplication source [s, e), flagged, (comparison, side)
        ((1000, 1100), (1400, 1600), True, "both terms", "on"),                 # centres 450 apart, spans 100 / 200: 0.5 + 0.5
        ((1000, 1100), (1401, 1601), False, "both terms", "above"),             # 451 / 900 + 0.5
        ((1000, 1100), (1399, 1599), True, "both terms", "below"),
        ((1050, 1050), (1000, 1100), True, "span term alone", "on"),            # spans 0 / 100: 1.0
        ((1050, 1049), (999, 1099), False, "span term alone", "above"),         # an end in front of its start: span -1, 101 / 100
        ((1000, 1099), (1000, 1100), True, "span term alone", "below"),
        ((1000, 1100), (1900, 2000), True, "position term alone", "on"),        # 900 / 900
        ((1000, 1100), (1901, 2001), False, "position term alone", "above"),
        ((1000, 1100), (1899, 1999), True, "position term alone", "below"),
        ((-5, 2), (896, 903), False, "floor of a negative centre, deletion", "on"),       # (-5 + 2) // 2 = -2 (not -1): 901 / 900
        ((896, 903), (-5, 2), False, "floor of a negative centre, duplication", "on"),
        ((-5, 2), (895, 902), True, "floor of a negative centre, deletion", "below"),     # 900 / 900
    ]
    for k, (d, s, flag, name, side) in enumerate(rows[:9]):
        base = 1000000 * k                                            # every pair a million bases from the next: the minimum is the pair's own deletion
        c.uni("DEL", R[k % 3], base + d[0], base + d[1], score=float(k + 1))
        _dup(c, R[k % 3], base + s[0], base + s[1], k)
        want.append(flag)
        c.cover((name, side))
    c.says(cutpaste=want)
    out.append(c)

    for k, (d, s, flag, name, side) in enumerate(rows[9:]):          # the pairs at the contig's start: a case each
        c = Case("stage3", "negative_centre_%d" % k)
        c.uni("DEL", "chr1", d[0], d[1])
        _dup(c, "chr1", s[0], s[1], 0)
        c.says(cutpaste=[flag])
        c.cover((name, side))
        out.append(c)

    c = Case("stage3", "limit_zero", del_ins_dup_max_distance=0.0)
    c.uni("DEL", "chr1", 1000, 1300)
    c.uni("DEL", "chr1", 500001, 500301)
    _dup(c, "chr1", 1000, 1300, 0)                                    # the deletion itself: 0.0 <= 0.0
    _dup(c, "chr1", 500000, 500300, 1)                                # one base off: 1 / 900
    c.says(cutpaste=[True, False])
    c.cover(("del_ins_dup_max_distance = 0", "on"), ("del_ins_dup_max_distance = 0", "above"))
    out.append(c)

    c = Case("stage3", "other_contig")                               # span_position_distance_clusters never looks at the contig
    c.uni("DEL", "chr2", 1000, 1300)
    _dup(c, "chr1", 1000, 1300, 0)
    c.says(cutpaste=[True])
    c.cover(("deletion on another contig", "on"))
    out.append(c)

    c = Case("stage3", "merged_rows_too")                            # a row stage 2 made, flagged through its source = the breakends' destinations
    c.uni("DEL", "chr2", 5000, 5100)
    _ins(c, "chr1", 1000, 200)
    c.flank("chr1", 1000, 1000, "chr2", 5400, 5600)                  # source chr2 [5400, 5600): centres 450 apart, spans 100 / 200: 1.0
    _ins(c, "chr1", 90000, 200)
    c.flank("chr1", 90000, 90000, "chr2", 5401, 5601)
    c.says(cutpaste=[True, False], remove_1=[0, 1])
    c.cover(("merged row against the limit", "on"), ("merged row against the limit", "above"))
    out.append(c)
    return out


S3_FROM = (1, 7, 8, 9, 17)
S3_DEL = (1, 63, 64, 65, 255, 256, 257, 513)


def s3_shape_cases():
    """k_cutpaste_min: 8 insertion-from clusters per workgroup (the tail of the last group clamped to n_from - 1), deletions walked with a stride of 256, minimum
    across a wave and across four waves.  Insertion-from cluster j has its source at chr2:[20000 (j + 1), + 200); the clusters first and last of a group of 8 and
    the last of all get ONE deletion at exactly 1.0 (span 100, centres 450 apart), at a deletion index taken in turn from 0, 63, 64, 255, 256, last; every other
    deletion is millions of bases from every source.  The last clusters of the list are rows stage 2 merged."""
    out = []
    turn = 0
    for n_from in S3_FROM:
        for n_del in S3_DEL:
            c = Case("s3_shapes", "from%d_del%d" % (n_from, n_del))
            n_new = 0 if (n_from == 1 and n_del % 2) else 1 if n_from < 17 else 2
            slots = sorted({p for p in (0, 63, 64, 255, 256, n_del - 1) if p < n_del})
            special = [j for j in range(n_from) if j % 8 in (0, 7) or j == n_from - 1]
            at = {}
            for j in special:
                for _ in range(len(slots)):
                    p = slots[turn % len(slots)]
                    turn += 1
                    if p not in at:
                        at[p] = j
                        break
            dels = [("chr1", 5000000 + 3000 * i, 5000100 + 3000 * i) for i in range(n_del)]
            for p, j in at.items():
                s = 20000 * (j + 1)
                dels[p] = ("chr2", s - 400, s - 300)                  # centre s - 350 against s + 100
                c.cover(("k_cutpaste_min: deletion index of the minimum", "last" if p == n_del - 1 and p not in (0, 63, 64, 255, 256) else str(p)),
                        ("k_cutpaste_min: slot of the cluster in its group", "first" if j % 8 == 0 else "last" if j % 8 == 7 else "tail"))
            for d in dels:
                c.uni("DEL", d[0], d[1], d[2], score=0.0, std_span=None, std_pos=None, n=1)
            for j in range(n_from - n_new):
                s = 20000 * (j + 1)
                c.bi("DUP_INT", "chr2", s, s + 200, "chr10", 1000000 + 100000 * j, 1000200 + 100000 * j, n=1)
            for j in range(n_from - n_new, n_from):
                s = 20000 * (j + 1)
                _ins(c, "chr1", 100000 * (j + 1), 200, n=1)
                c.flank("chr1", 100000 * (j + 1), 100000 * (j + 1), "chr2", s + 200, s, n=1)
            hit = set(at.values())
            c.says(cutpaste=[j in hit for j in range(n_from)], remove_1=list(range(n_new)))
            c.cover(("n_from", str(n_from)), ("n_del", str(n_del)), ("insertion-from rows", "merged" if n_new else "CLUSTER's only"))
            out.append(c)
    return out


# ---- stage 4 -------------------------------------------------------------------------------------------------------------------------------------------------------
def _sentinel(c):
    """an interspersed duplication behind every insertion of chr1, so that the list never runs out there"""
    c.bi("DUP_INT", "chr2", 50000000, 50000300, "chr1", 80000000, 80000300)


def stage4_cases():
    """the walk (:404-452): `contig2 < contig1 or (contig2 == contig1 and end2 < start1)` moves the pointer on; `start2 < end1` and
    `(length1 - length2) / max(length1, length2) < 0.2` decide"""
    out = []
    c = Case("stage4", "three_comparisons")
    c.far_deletion()
    rm = []
    rows = [  # insertion [s1, e1), destination [s2, e2) relative to a base, removed, comparison, side
        ((1000, 1300), (700, 999), False, "end2 < start1", "below"), ((1000, 1300), (700, 1000), True, "end2 < start1", "on"), ((1000, 1300), (700, 1001), True, "end2 < start1", "above"),
        ((1000, 1300), (1299, 1599), True, "start2 < end1", "below"), ((1000, 1300), (1300, 1600), False, "start2 < end1", "on"), ((1000, 1300), (1301, 1601), False, "start2 < end1", "above"),
        ((1000, 1100), (1000, 1081), True, "length ratio < 0.2", "below"), ((1000, 1100), (1000, 1080), False, "length ratio < 0.2", "on"),
        ((1000, 1100), (1000, 1079), False, "length ratio < 0.2", "above"), ((1000, 2000), (1000, 1800), False, "length ratio < 0.2", "on"),
        ((1000, 1005), (1000, 1004), False, "length ratio < 0.2", "on"), ((1000, 1100), (1000, 2000), True, "len2 > len1", "on"),
        ((1000, 1100), (500, 9000), True, "len2 > len1", "on")]
    for k, (i, d, gone, name, side) in enumerate(rows):
        base = 100000 * (k + 1)
        n = c.uni("INS", "chr1", base + i[0], base + i[1])
        c.bi("DUP_INT", "chr2", base, base + d[1] - d[0], "chr1", base + d[0], base + d[1])
        if gone:
            rm.append(n)
        c.cover((name, side))
    _sentinel(c)
    c.says(remove_1=[], remove_2=rm)
    out.append(c)

    c = Case("stage4", "three_comparisons_tandem")                   # the same rows against the tandem list: no interspersed duplication at all
    rm = []
    for k, (i, d, gone, name, side) in enumerate(rows):
        base = 100000 * (k + 1)
        n = c.uni("INS", "chr1", base + i[0], base + i[1])
        ln = d[1] - d[0]
        c.bi("DUP_TAN", "chr1", base + d[0] - ln, base + d[0], "chr1", base + d[0], base + d[1])      # one copy: destination [d0, d1)
        if gone:
            rm.append(n)
        c.cover(("tandem: " + name, side))
    c.bi("DUP_TAN", "chr1", 80000000, 80000300, "chr1", 80000300, 80000600)
    c.says(remove_1=[], remove_2=rm, copies=[1] * (len(rows) + 1))
    out.append(c)

    # the interspersed list runs out at the first, a middle and the last insertion; the tandem list takes over, runs out as well, or is empty
    for where in ("first", "middle", "last"):
        for tan in ("takes_over", "runs_out", "empty"):
            c = Case("stage4", "runs_out_%s_tandem_%s" % (where, tan))
            c.far_deletion()
            ins = [c.uni("INS", "chr1", 10000 * (k + 1), 10000 * (k + 1) + 300) for k in range(5)]
            at = {"first": 0, "middle": 2, "last": 4}[where]
            rm = []
            for k in range(at):                                       # one duplication on every insertion in front of `at`
                c.bi("DUP_INT", "chr2", 1000 * k, 1000 * k + 300, "chr1", 10000 * (k + 1), 10000 * (k + 1) + 300)
                rm.append(ins[k])
            if at == 0:
                c.bi("DUP_INT", "chr2", 0, 300, "chr1", 100, 400)     # in front of every insertion: the list ends at the first one
            if tan != "empty":
                for k in range(5):                                    # tandem destinations on EVERY insertion: only those from `at` on are ever looked at
                    if tan == "runs_out" and k > at:
                        break
                    s = 10000 * (k + 1)
                    c.bi("DUP_TAN", "chr1", s - 300, s, "chr1", s, s + 300)
                    if k >= at:
                        rm.append(ins[k])
            c.says(remove_2=sorted(rm), remove_1=[])
            c.cover(("interspersed list runs out", where), ("tandem list", tan))
            out.append(c)

    c = Case("stage4", "insertions_not_sorted")                      # a later insertion lies in front of the pointer, which does not move back
    c.far_deletion()
    c.uni("INS", "chr1", 50000, 50300)
    c.uni("INS", "chr1", 10000, 10300)
    c.uni("INS", "chr1", 50010, 50290)
    c.bi("DUP_INT", "chr2", 0, 300, "chr1", 10000, 10300)
    c.bi("DUP_INT", "chr2", 1000, 1300, "chr1", 50000, 50300)
    c.says(remove_2=[0, 2], remove_1=[])
    c.cover(("insertion in front of the pointer", "on"))
    out.append(c)

    c = Case("stage4", "ends_not_monotone")
    c.far_deletion()
    c.bi("DUP_INT", "chr2", 0, 4000, "chr1", 1000, 5000)             # sort order: (1000, 5000), (1200, 1500), (6000, 6300)
    c.bi("DUP_INT", "chr2", 10000, 10300, "chr1", 1200, 1500)
    c.bi("DUP_INT", "chr2", 20000, 20300, "chr1", 6000, 6300)
    c.uni("INS", "chr1", 1200, 1500)                                 # the pointer rests on (1000, 5000): too long by far ... but len2 > len1 always removes
    c.uni("INS", "chr1", 4000, 9000)                                 # still (1000, 5000): (5000 - 4000) / 5000 = 0.2: kept, although (6000, 6300)... is not looked at
    c.uni("INS", "chr1", 5500, 5800)                                 # moves past (1000, 5000) AND (1200, 1500) to (6000, 6300): start2 >= end1, kept
    c.uni("INS", "chr1", 6000, 6300)
    c.says(remove_2=[0, 3], remove_1=[])
    c.cover(("destination ends not monotone", "on"))
    out.append(c)

    c = Case("stage4", "contigs_by_name")                            # "chr10" < "chr2": the walk compares names, the table holds ids
    c.far_deletion()
    c.uni("INS", "chr10", 1000, 1300)
    c.uni("INS", "chr2", 1000, 1300)
    c.bi("DUP_INT", "chr1", 0, 300, "chr2", 1000, 1300)
    c.bi("DUP_INT", "chr1", 1000, 1300, "chr10", 1000, 1300)
    c.says(remove_2=[0, 1], remove_1=[])
    c.cover(("contig order", "chr10 before chr2"))
    out.append(c)

    c = Case("stage4", "contigs_by_name_tandem")
    c.uni("INS", "chr10", 1000, 1300)
    c.uni("INS", "chr2", 1000, 1300)
    c.bi("DUP_TAN", "chr2", 700, 1000, "chr2", 1000, 1300)
    c.bi("DUP_TAN", "chr10", 700, 1000, "chr10", 1000, 1300)
    c.says(remove_2=[0, 1], remove_1=[])
    c.cover(("contig order", "chr10 before chr2, tandem"))
    out.append(c)

    c = Case("stage4", "tandem_destination_clamped")                 # source_end + copies * (source_end - max(0, source_start)): [100, 300), not [100, 400)
    c.bi("DUP_TAN", "chr1", -50, 100, "chr1", 100, 400)              # 300 / 150: two copies
    c.uni("INS", "chr1", 350, 650)                                   # end2 = 300 < 350: the list runs out, kept; with 400 it would go
    c.says(remove_2=[], remove_1=[], copies=[2])
    c.cover(("tandem destination from the clamped start", "on"))
    out.append(c)
    c = Case("stage4", "tandem_destination_clamped_hit")
    c.bi("DUP_TAN", "chr1", -50, 100, "chr1", 100, 400)
    c.uni("INS", "chr1", 300, 540)                                   # end2 = 300 = start1: stays; 100 < 540; (240 - 200) / 240 < 0.2 - against 300 it would be negative, too
    c.uni("INS", "chr1", 300, 551)                                   # (251 - 200) / 251 > 0.2: kept; against a length of 300 it would go
    c.says(remove_2=[0], remove_1=[], copies=[2])
    c.cover(("tandem destination from the clamped start", "length"))
    out.append(c)
    return out


S4_LISTS = (63, 64, 65, 128, 129)
S4_INS = (63, 64, 65, 130)


def s4_shape_cases():
    """k_walk: the lists in windows of 64 entries (walk_cur), the insertions in tiles of 64"""
    out = []
    for which in ("int", "tan"):
        for n in S4_LISTS:
            # entry k has its destination at chr1:[10000 (k + 1), + 300); one insertion on each of the entries 0, 62, 63, 64, 127, 128, n - 1 (a hit decided with the
            # pointer resting there) and one in the gap behind each of them (decided on the NEXT entry, or where the list runs out)
            c = Case("s4_shapes", "%s_list_%d" % (which, n))
            if which == "int":
                c.far_deletion()
            for k in range(n):
                s = 10000 * (k + 1)
                if which == "int":
                    c.bi("DUP_INT", "chr2", 1000 * k, 1000 * k + 300, "chr1", s, s + 300, n=1)
                else:
                    c.bi("DUP_TAN", "chr1", s - 300, s, "chr1", s, s + 300, n=1)
            rm = []
            for k in sorted({p for p in (0, 62, 63, 64, 127, 128, n - 1) if p < n}):
                s = 10000 * (k + 1)
                rm.append(c.uni("INS", "chr1", s + 10, s + 290, n=1))
                c.uni("INS", "chr1", s + 5000, s + 5300, n=1)
                c.cover(("walk_cur: pointer on entry", str(k) if k in (63, 64, 128) else "other"))
            c.says(remove_2=rm, remove_1=[])
            c.cover(("%s list" % which, str(n)))
            out.append(c)
    for n_ins in S4_INS:
        for at in (62, 63, 64, 65):
            if at >= n_ins:
                continue
            # insertion i at chr1:[10000 (i + 1), + 300); interspersed duplications on the insertions 0, 31 and at - 1: the list runs out AT insertion `at`;
            # tandem duplications on `at`, on both sides of every tile edge behind it and on the last insertion
            c = Case("s4_shapes", "ins_%d_runs_out_at_%d" % (n_ins, at))
            c.far_deletion()
            for i in range(n_ins):
                c.uni("INS", "chr1", 10000 * (i + 1), 10000 * (i + 1) + 300, score=1.0, std_span=None, std_pos=None, n=1)
            rm = []
            for i in (0, 31, at - 1):
                c.bi("DUP_INT", "chr2", 1000 * i, 1000 * i + 300, "chr1", 10000 * (i + 1), 10000 * (i + 1) + 300, n=1)
                rm.append(i)
            for i in sorted({p for p in (5, at, 63, 64, 66, 127, 128, n_ins - 1) if p < n_ins}):
                s = 10000 * (i + 1)
                c.bi("DUP_TAN", "chr1", s - 300, s, "chr1", s, s + 300, n=1)
                if i >= at:
                    rm.append(i)
            c.says(remove_2=sorted(set(rm)), remove_1=[])
            c.cover(("insertion list", str(n_ins)), ("interspersed list runs out at insertion", str(at)))
            out.append(c)
    return out


# ---- stage 5 -------------------------------------------------------------------------------------------------------------------------------------------------------
def _fin(ss, se, ds, de, std_span, std_pos, cutpaste, score, members):
    return [ss, se, ds, de, std_span, std_pos, cutpaste, score, members]


def stage5_cases():
    """form_partitions over get_key() order with max(0, start - previous end) <= partition_max_distance; average linkage cut at cluster_max_distance over
    span_position_distance_intdup_candidates; consolidation (SVIM_clustering.py:306-372)"""
    out = []
    for gap, n_out in ((49, 1), (50, 1), (51, 2)):
        c = Case("stage5", "partition_gap_%d" % gap, partition_max_distance=50)
        c.far_deletion()
        c.bi("DUP_INT", "chr1", 1000, 1300, "chr2", 5000, 5300)
        c.bi("DUP_INT", "chr1", 1300 + gap, 1600 + gap, "chr2", 5000, 5300)       # centres 300 + gap apart: 0.39 - one cluster wherever they share a partition
        c.says(counts=[0, 0, n_out, 0, 0, 0])
        c.cover(("gap <= partition_max_distance", "below" if gap < 50 else "on" if gap == 50 else "above"))
        out.append(c)

    for pmd, n_out in ((0, 1), (-1, 2)):
        c = Case("stage5", "overlap_limit_%d" % pmd, partition_max_distance=pmd)
        c.far_deletion()
        c.bi("DUP_INT", "chr1", 1000, 1300, "chr2", 5000, 5300)
        c.bi("DUP_INT", "chr1", 1100, 1400, "chr2", 5000, 5300)                   # starts 200 in front of the previous end: max(0, -200) = 0
        c.says(counts=[0, 0, n_out, 0, 0, 0])
        c.cover(("max(0, start - end)", "0 <= 0" if pmd == 0 else "0 <= -1"))
        out.append(c)

    c = Case("stage5", "source_contig_change")
    c.far_deletion()
    c.bi("DUP_INT", "chr1", 1000, 1300, "chr2", 5000, 5300)
    c.bi("DUP_INT", "chr10", 1000, 1300, "chr2", 5000, 5300)
    c.bi("DUP_INT", "chr10", 1001, 1301, "chr2", 5000, 5300)
    c.says(counts=[0, 0, 2, 0, 0, 0])
    c.cover(("source contig change", "on"))
    out.append(c)

    # the cut at cluster_max_distance through each of the three terms
    terms = {"source": ((1000, 1300, 5000), (1450, 1750, 5000), (1451, 1751, 5000)), "destination": ((1000, 1300, 5000), (1000, 1300, 5450), (1000, 1300, 5451)),
             "span": ((1050, 1150, 5000), (1000, 1200, 5000), (1000, 1201, 5000))}
    for term, (a, on, over) in terms.items():
        for side, b in (("on", on), ("above", over)):
            c = Case("stage5", "cut_%s_%s" % (term, side))
            c.far_deletion()
            for s, e, d in (a, b):
                c.bi("DUP_INT", "chr1", s, e, "chr2", d, d + e - s)
            c.says(counts=[0, 0, 1 if side == "on" else 2, 0, 0, 0])
            c.cover(("distance <= cluster_max_distance, %s term" % term, side))
            out.append(c)

    c = Case("stage5", "consolidation")
    c.uni("DEL", "chr1", 100000, 100100)
    # pair 1: means 1000.5 (even: 1000), 1301.5 (odd: 1302), 5001.5 (5002), 5300.5 (5300); stds None / None and 2.0 / 4.0; scores 3 then 7
    a = c.bi("DUP_INT", "chr1", 1000, 1301, "chr2", 5001, 5300, score=3.0, std_span=None, std_pos=2.0, n=2)
    b = c.bi("DUP_INT", "chr1", 1001, 1302, "chr2", 5002, 5301, score=7.0, std_span=None, std_pos=4.0, n=3)
    # pair 2: the other parities (100399.5, 100600.5, 8000.5, 8201.5); one None and one 3.0; the SECOND in list order sorts first by source END and second by
    # source start, score 9 then 2; cutpaste on one member only: the deletion [100000, 100100) is at 1.0 from [100400, 100600) and past it from [100399, 100601)
    d = c.bi("DUP_INT", "chr1", 100399, 100601, "chr2", 8001, 8203, score=2.0, std_span=3.0, std_pos=None, n=1)
    e = c.bi("DUP_INT", "chr1", 100400, 100600, "chr2", 8000, 8200, score=9.0, std_span=None, std_pos=None, n=2)
    m = lambda k: c.lists["DUP_INT"][k][9]      # noqa: E731
    c.says(cutpaste=[False, False, False, True], counts=[1, 0, 2, 0, 0, 0],
           final=[_fin(1000, 1302, 5002, 5300, None, 3.0, False, 7.0, m(a) + m(b)), _fin(100400, 100600, 8000, 8202, 3.0, None, True, 9.0, m(e) + m(d))])
    c.cover(("rounding of a mean x.5", "x even"), ("rounding of a mean x.5", "x odd"), ("mean of the stds", "all None"), ("mean of the stds", "mixed"), ("mean of the stds", "none None"),
            ("cutpaste", "one member only"), ("score", "the maximum is not the first"), ("members", "in key order, not list order"))
    out.append(c)
    return out


def s5_shape_cases():
    """partitions of 1, 2, 100 and 101 candidates and of 48 / 49 / 72 / 73 (the LDS classes of the linkage); the sample of the 101 is carried into the partition of
    150 behind it (one seeded generator for the whole call)"""
    rng = random.Random(4242)
    c = Case("s5_shapes", "partition_sizes")
    c.uni("DEL", "chr2", 1000, 1300, score=0.0, n=1)
    sizes = (("chr2", 100, 1000), ("chr10", 101, 50000), ("chr10", 150, 900000), ("chr1", 48, 200000), ("chr1", 49, 400000), ("chr1", 72, 600000), ("chr1", 73, 800000),
             ("chr1", 1, 1000000), ("chr1", 2, 1200000))
    for part, (contig, n, base) in enumerate(sizes):
        for k in range(n):
            s = base + rng.randrange(0, 40) * 7
            ln = 300 + rng.randrange(0, 4) * 150
            d = 10000 + rng.randrange(0, 6) * 400
            c.bi("DUP_INT", contig, s, s + ln, R[part % 3], d, d + ln, score=float(rng.randrange(1, 30)), std_span=rng.choice([None, 0.5, 3.25]),
                 std_pos=rng.choice([None, 1.0, 7.125]), n=1)
        c.cover(("partition of", str(n)))
    c.says(final_range=[len(sizes) + 1, sum(n for _, n, _ in sizes) - 1])      # every partition at least one candidate, those of 48 and more at least two, not all apart
    return [c]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def refused():
    a = Case("refused", "tandem_zero_span")                          # (dest_end - dest_start) / (source_end - source_start), :349
    a.uni("INS", "chr1", 1000, 1300)
    a.flank("chr1", 1000, 1000, "chr2", 5000, 5300)
    a.uni("DEL", "chr1", 100, 300)
    a.bi("DUP_TAN", "chr1", 500, 500, "chr1", 500, 800)
    b = Case("refused", "stage3_two_zero_spans")                     # abs(span1 - span2) / max(span1, span2) with both spans 0
    b.uni("INS", "chr1", 1000, 1300)
    b.flank("chr1", 1000, 1000, "chr2", 5000, 5300)
    b.uni("DEL", "chr1", 100, 300)
    b.uni("DEL", "chr1", 7000, 7000)
    b.bi("DUP_INT", "chr2", 900, 900, "chr1", 4000, 4300)
    # not a refusal of the reference: a merged cluster whose destination end `ins_start + distance` (:156) lies beyond 2^31 - 1, which no int32 column holds.
    # The insertion ends on the last int32 position; the destinations are 150 000 000 apart: ratio 0.983
    d = Case("refused", "merged_end_beyond_int32")
    d.uni("DEL", "chr1", 100, 300)
    d.uni("INS", "chr1", 2000000000, 2147483647)
    d.flank("chr1", 2000000000, 2000000000, "chr2", 1000, 150001000)
    return [a, b, d]


EXPECTED_RAISES = {"refused/tandem_zero_span": "ZeroDivisionError", "refused/stage3_two_zero_spans": "ZeroDivisionError", "refused/merged_end_beyond_int32": None}
# the lists as the reference leaves them when it raises or returns: [insertions, insertion-from clusters, breakends]
EXPECTED_STATE = {"refused/tandem_zero_span": [1, 0, 2], "refused/stage3_two_zero_spans": [1, 2, 4], "refused/merged_end_beyond_int32": [0, 1, 4]}
BEYOND_INT32_DEST_END = 2150000000


def cases():
    out = []
    for f in (stage1_cases, s2_distance_cases, s2_ratio_cases, s2_search_cases, s2_score_cases, stage3_cases, s3_shape_cases, stage4_cases, s4_shape_cases,
              stage5_cases, s5_shape_cases):
        out.extend(f())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def coverage(cs):
    table = {}
    for c in cs:
        for name, side in c.covers:
            table.setdefault(name, {}).setdefault(side, []).append(c.name)
    return table


def _sides(*s):
    return tuple(s)


BOA = _sides("below", "on", "above")
REQUIRED = {
    "DEL score > 0": BOA, "INS score > 0": BOA,
    "round(copies)": ("x.5, x even", "x.5, x odd", "below x.5", "above x.5"),
    "fully_covered": ("first", "last", "none"), "member list": ("1", "64", "65", "130"),
    "max(0, start)": TYPES, "BND directions": ("fwd/fwd", "fwd/rev", "rev/fwd", "rev/rev"),
    "fwd: abs(mean - start) <= trans_sv_max_distance, mean > start": BOA, "fwd: abs(mean - start) <= trans_sv_max_distance, mean < start": BOA,
    "rev: abs(mean - start) <= trans_sv_max_distance, mean > start": BOA, "rev: abs(mean - start) <= trans_sv_max_distance, mean < start": BOA,
    "both lists outside": ("on",), "both lists on the limit, opposite sides": ("on",), "trans_sv_max_distance = 0": ("on", "above"),
    "0.95 against the length ratio": BOA, "1.1 against the length ratio": BOA, "destination contigs equal": ("below", "on"), "distance = 0": ("on",),
    "breakends per contig": ("1", "2", "3", "40"), "bisect: pos == 0": ("on",), "bisect: pos == len": ("on",), "after - x < x - before": BOA,
    "bisect lands beside the nearest start": ("pos inside", "pos == 0", "pos == len"), "starts in key order": ("unsorted",),
    "equal keys": ("two originals", "original and mirrored"), "contig in one list only": ("fwd/fwd only", "rev/rev only"),
    "matched through mirrored clusters only": ("on",), "two entries on the insertion's start": ("on",), "distance from destination starts": ("on",),
    "mirror of a mixed-direction cluster": ("fwd/rev", "rev/fwd"),
    "max(0, 100 - distance)": BOA, "max(0, 100 - std), slot 0": BOA + ("None",), "max(0, 100 - std), slot 1": BOA + ("None",),
    "max(0, 100 - std), slot 2": BOA + ("None",), "max(0, 100 - std), slot 3": BOA + ("None",), "main score": ("0", "negative"),
    "merged member list": ("1", "63", "64", "65", "130"),
    "both terms": BOA, "span term alone": BOA, "position term alone": BOA, "floor of a negative centre, deletion": ("on", "below"),
    "floor of a negative centre, duplication": ("on",), "del_ins_dup_max_distance = 0": ("on", "above"), "deletion on another contig": ("on",),
    "merged row against the limit": ("on", "above"),
    "k_cutpaste_min: deletion index of the minimum": ("0", "63", "64", "255", "256", "last"), "k_cutpaste_min: slot of the cluster in its group": ("first", "last", "tail"),
    "n_from": tuple(str(n) for n in S3_FROM), "n_del": tuple(str(n) for n in S3_DEL), "insertion-from rows": ("merged", "CLUSTER's only"),
    "end2 < start1": BOA, "start2 < end1": BOA, "length ratio < 0.2": BOA, "len2 > len1": ("on",),
    "tandem: end2 < start1": BOA, "tandem: start2 < end1": BOA, "tandem: length ratio < 0.2": BOA, "tandem: len2 > len1": ("on",),
    "interspersed list runs out": ("first", "middle", "last"), "tandem list": ("takes_over", "runs_out", "empty"), "insertion in front of the pointer": ("on",),
    "destination ends not monotone": ("on",), "contig order": ("chr10 before chr2", "chr10 before chr2, tandem"),
    "tandem destination from the clamped start": ("on", "length"),
    "walk_cur: pointer on entry": ("63", "64", "128"), "int list": tuple(str(n) for n in S4_LISTS), "tan list": tuple(str(n) for n in S4_LISTS),
    "insertion list": tuple(str(n) for n in S4_INS), "interspersed list runs out at insertion": ("62", "63", "64", "65"),
    "gap <= partition_max_distance": BOA, "max(0, start - end)": ("0 <= 0", "0 <= -1"), "source contig change": ("on",),
    "distance <= cluster_max_distance, source term": ("on", "above"), "distance <= cluster_max_distance, destination term": ("on", "above"),
    "distance <= cluster_max_distance, span term": ("on", "above"),
    "rounding of a mean x.5": ("x even", "x odd"), "mean of the stds": ("all None", "mixed", "none None"), "cutpaste": ("one member only",),
    "score": ("the maximum is not the first",), "members": ("in key order, not list order",),
    "partition of": ("1", "2", "48", "49", "72", "73", "100", "101", "150"),
}


def disagreement(case, exp):
    """None when the `expected` block the reference wrote for `case` is what its author says; else what differs"""
    e = case.expect
    if not e:
        return "%s: nothing stated" % case.name
    merged = exp["merged_insertion_from_clusters"]
    got = {"remove_1": exp["inserted_regions_to_remove"], "remove_2": exp["inserted_regions_to_remove_2"], "merged_src": [r[1:3] for r in merged],
           "merged_members": [r[8] for r in merged], "cutpaste": [r["cutpaste"] for r in exp["flag_cutpaste"]], "copies": [r["copies"] for r in exp["combine"][3]],
           "fully": [r["fully_covered"] for r in exp["combine"][3]], "counts": [len(x) for x in exp["combine"]],
           "final": [[r["source_start"], r["source_end"], r["dest_start"], r["dest_end"], r["std_span"], r["std_pos"], r["cutpaste"], r["score"], r["members"]]
                     for r in exp["combine"][2]]}
    for k, want in e.items():
        if k == "merged_scores":
            have = [r[6] for r in merged]
            if len(have) != len(want) or not all(w is None or abs(h - w) <= 1e-12 * abs(w) for h, w in zip(have, want)):
                return "%s: merged scores %r, the case says %r" % (case.name, have, want)
        elif k == "final_range":
            if not want[0] <= len(got["final"]) <= want[1]:
                return "%s: %d re-clustered duplications, the case says %r" % (case.name, len(got["final"]), want)
        elif got[k] != want:
            return "%s: the reference gives %s = %r, the case says %r" % (case.name, k, got[k], want)
    return None
