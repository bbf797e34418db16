"""Coordinate-window ownership (svim_amd/multigpu.py: assign_windows, Windows.local_intervals, Windows.refine_from) held to a plain partition oracle, no GPU:
whatever the ranks saw of the signatures around a proposed cut, the refined cuts must leave every partition of form_partitions with ONE owner - otherwise a
multi-rank run clusters a partition in two halves and silently differs from the single-rank run.

The oracle below restates form_partitions on integer tuples (sorted(), a loop, nothing else) and shares no code with the product.  Every case runs the product
path of cluster_step's phase 0: local_intervals on each rank's rows, concatenation, refine_from - with the rows dealt to the ranks in three different ways."""
import random

import numpy as np
import pytest

from svim_amd import _abi, multigpu

DEL, INS, INV, DUP_TAN, BND, DUP_INT = range(6)
assert (DEL, INS, INV, DUP_TAN, BND, DUP_INT) == (_abi.SVX_DEL, _abi.SVX_INS, _abi.SVX_INV, _abi.SVX_DUP_TAN, _abi.SVX_BND, _abi.SVX_DUP_INT)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------
# a row is (type, contig, start, end, contig2, pos2) with contig ids into `names`; BND rows carry start = pos1, end = pos1 + 1; DUP_INT rows carry their
# SOURCE in contig / start / end and their destination in contig2 / pos2
def oracle_partitions(rows, names, max_distance):
    """form_partitions per type on plain tuples -> list of partitions (lists of row indices)"""
    def group(r):
        t, c, _, _, c2, _ = r
        return (t, names[c2], names[c]) if t == DUP_INT else (t, names[c], "")

    def coordinate(r):
        t, _, start, end, _, pos2 = r
        return start if t in (INS, BND) else pos2 if t == DUP_INT else end

    def gap(a, b):
        if b[0] == INS:
            d = b[2] - a[2]
        elif b[0] == DUP_INT:
            d = b[5] - a[5]
        else:
            d = b[2] - a[3]
        return max(d, 0)

    order = sorted(range(len(rows)), key=lambda i: (group(rows[i]), coordinate(rows[i])))
    parts = []
    for k, i in enumerate(order):
        j = order[k - 1] if k else None
        if j is None or group(rows[j]) != group(rows[i]) or gap(rows[j], rows[i]) > max_distance:
            parts.append([])
        parts[-1].append(i)
    return parts


def test_the_oracle_on_hand_counted_rows():
    names = ["b", "a"]
    rows = [(DEL, 0, 100, 200, -1, 0), (DEL, 0, 1200, 1300, -1, 0), (DEL, 0, 2301, 2400, -1, 0),        # gaps 1000 (same partition) and 1001 (a new one)
            (DEL, 1, 150, 250, -1, 0),                                                                # another contig
            (INS, 0, 100, 900, -1, 0), (INS, 0, 1100, 1101, -1, 0), (INS, 0, 2101, 2102, -1, 0),      # INS: start - start, whatever the ends are
            (DEL, 0, 260, 150, -1, 0),                                                                # start > end: sorted by its end, distances clamp at 0
            (DUP_INT, 0, 5, 9, 1, 700), (DUP_INT, 0, 90000, 90009, 1, 1700), (DUP_INT, 1, 5, 9, 1, 800),      # keyed by (destination, source, destination start)
            (BND, 0, 500, 501, 1, 7), (BND, 0, 1501, 1502, 0, 9), (BND, 0, 2503, 2504, 1, 7)]         # pos1 against pos1 + 1 of the row before
    got = sorted(sorted(p) for p in oracle_partitions(rows, names, 1000))
    assert got == [[0, 1, 7], [2], [3], [4, 5], [6], [8, 9], [10], [11, 12], [13]]


# ---- the product path ---------------------------------------------------------------------------------------------------------------------------------
def _columns(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return {"type": a[:, 0], "contig": a[:, 1], "start": a[:, 2], "end": a[:, 3], "contig2": a[:, 4], "pos2": a[:, 5]}


def _crank(names):
    order = sorted(range(len(names)), key=lambda i: names[i])
    crank = [0] * len(names)
    for r, i in enumerate(order):
        crank[i] = r
    return crank


def _owners(W, rows):
    c = _columns(rows)
    return [int(x) for x in W.owner_of_signatures(c["type"], c["contig"], c["contig2"], c["start"], c["end"], c["pos2"])]


def _refine(W, rows, dealt, max_distance, radius):
    """what cluster_step does before anything else: every rank's merged stretches around the proposals, all of them to everybody, the same cuts everywhere"""
    parts = []
    for r in range(W.world):
        c = _columns([row for row, d in zip(rows, dealt) if d == r])
        parts.append(W.local_intervals(c["type"], c["contig"], c["start"], c["end"], radius))
    return W.refine_from(np.concatenate(parts), max_distance, radius)


def _deals(W, rows, seed):
    rng = random.Random(seed)
    return {"by the proposal": _owners(W, rows),
            "at random": [rng.randrange(W.world) for _ in rows],
            "all to one rank": [W.world - 1] * len(rows)}


def _cuts(W):
    return [(int(c), int(x)) for c, x in zip(W.cut_contig, W.cut_pos)]


def check(names, world, proposals, rows, max_distance, radius, expect=None, seed=1, windows=None):
    """proposals: [(contig id, coordinate or -1)] * (world - 1), or a Windows from assign_windows.  Returns the refined Windows."""
    crank = _crank(names)
    W0 = windows if windows is not None else multigpu.Windows(world, crank, [c for c, _ in proposals], [x for _, x in proposals])
    assert W0.world == world and W0.needs_refine() == any(x >= 0 for _, x in _cuts(W0))
    refined = {how: _refine(W0, rows, dealt, max_distance, radius) for how, dealt in _deals(W0, rows, seed).items()}
    W = refined["by the proposal"]
    for how, other in refined.items():
        assert _cuts(other) == _cuts(W), "the refined cuts depend on who collected the rows (%s): %r != %r" % (how, _cuts(other), _cuts(W))
    # the same contigs, in (contig name, coordinate) order
    assert [c for c, _ in _cuts(W)] == [c for c, _ in _cuts(W0)]
    keys = [(crank[c], x) for c, x in _cuts(W)]
    assert keys == sorted(keys), "cuts are not monotone: %r" % (_cuts(W),)
    assert not W.needs_refine()
    # one owner per partition
    own = _owners(W, rows)
    for part in oracle_partitions(rows, names, max_distance):
        owners = sorted({own[i] for i in part})
        if len(owners) > 1:
            split = " / ".join(str(sum(1 for i in part if own[i] == r)) for r in owners)
            t, c = rows[part[0]][0], rows[part[0]][1]
            pytest.fail("a partition of %d rows (type %d on %s, coordinates %d..%d) has owners %r: %s rows; cuts %r from proposals %r"
                        % (len(part), t, names[c], min(rows[i][2] for i in part), max(rows[i][3] for i in part), owners, split, _cuts(W), _cuts(W0)), pytrace=False)
    # DUP_INT rows go with the first base of their destination contig
    for (t, _, _, _, c2, _), o in zip(rows, own):
        if t == DUP_INT:
            assert o == int(W.owner_of_positions(np.asarray([c2]), np.asarray([0]))[0]), "a DUP_INT row left the owner of its destination contig's first base"
    # refining the refined cuts again changes nothing (cluster_step looks at least 64 x max_distance far; below max_distance a second look from the moved cut
    # can see less of the corridor than the first one did)
    if radius >= max_distance:
        again = _refine(W, rows, own, max_distance, radius)
        assert _cuts(again) == _cuts(W), "refine_from is not idempotent: %r -> %r" % (_cuts(W), _cuts(again))
    if expect is not None:
        assert [x for _, x in _cuts(W)] == list(expect), "cuts %r, expected coordinates %r" % (_cuts(W), expect)
    return W


def dense(t, contig, a, b, step=500, length=100, contig2=-1):
    """rows of one type every `step` bases from a (inclusive) to b (exclusive), each `length` long"""
    if t == BND:
        return [(BND, contig, s, s + 1, contig2 if contig2 >= 0 else contig, 77) for s in range(a, b, step)]
    return [(t, contig, s, s + length, -1, 0) for s in range(a, b, step)]


MAXD, RADIUS, X = 1000, 100000, 5000000


# ---- the open ends of the neighbourhood are not corridors ------------------------------------------------------------------------------------------------
def _repro(side):
    """DEL rows every 500 bases, 100 long: ONE partition that runs on beyond the radius on the named side(s) of the proposal at X"""
    if side == "both":
        return dense(DEL, 0, X - 200000, X + 200000)
    if side == "left":                    # ends in a real corridor on the right, 100 100 bases from the proposal; the run goes on to the left
        return dense(DEL, 0, X - 200000, X + 100001)
    return dense(DEL, 0, X - 100100, X + 200000)          # begins behind a real corridor on the left, 100 100 bases away; the run goes on to the right


@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_dense_run_beyond_the_radius(side):
    """no corridor inside the radius: the proposal of assign_windows (5 000 000 on a contig of 10 Mb) falls back to the contig's first base"""
    w = multigpu.assign_windows(["c"], [10000000], 2)
    assert _cuts(w) == [(0, X)]
    rows = _repro(side)
    assert len(oracle_partitions(rows, ["c"], MAXD)) == 1
    check(["c"], 2, None, rows, MAXD, RADIUS, expect=[-1], windows=w)


# ---- exactly max_distance is not a corridor, max_distance + 1 is ---------------------------------------------------------------------------------------
def _two_runs(t, left_end, right_start, length=100):
    """two dense runs of one type that leave [left_end + 1, right_start - 1] free and reach beyond the radius on both sides"""
    lo, hi = X - RADIUS - 5000, X + RADIUS + 5000
    left = dense(t, 0, lo, left_end - length - 499, length=length) + [(t, 0, left_end - length, left_end, -1, 0)]
    return left + dense(t, 0, right_start, hi, length=length)


@pytest.mark.parametrize("width", [MAXD, MAXD + 1], ids=["exactly_max_distance", "max_distance_plus_1"])
@pytest.mark.parametrize("t", [DEL, INS], ids=["interval_rule", "ins_rule"])
@pytest.mark.parametrize("where", ["proposal_in_gap", "proposal_left", "proposal_right"])
def test_gap_width_at_the_limit(t, width, where):
    """the only free stretch near the proposal: the last covered base before it is L, the first behind it R = L + width.  For DEL rows that is form_partitions' own
    distance (start - end).  INS rows are 300 long here and form_partitions measures start - start, 300 more than the free stretch: it cuts in both
    cases, the refinement may only cut where the free stretch itself is wider than max_distance (local_intervals works on [start, end] for every type) -
    and then at the coordinate of the stretch that is nearest to the proposal."""
    L = X - 300 if where != "proposal_right" else X + 7000
    if where == "proposal_left":
        L = X - 9000
    R = L + width
    rows = _two_runs(t, L, R, length=300 if t == INS else 100)
    n_parts = len(oracle_partitions(rows, ["c"], MAXD))
    assert n_parts == (2 if t == INS or width > MAXD else 1)
    check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[min(max(X, L + 1), R) if width > MAXD else -1])


def test_ins_rows_measured_start_to_start():
    """INS rows whose STARTS are max_distance apart are one partition however long the insertions are; one base more and form_partitions cuts - the refinement
    sees [start, end], i.e. less free room than that, and must not cut in either case"""
    for d in (MAXD, MAXD + 1):
        rows = _two_runs(INS, X - 100, X - 100 - 300 + d, length=300)
        assert len(oracle_partitions(rows, ["c"], MAXD)) == (1 if d == MAXD else 2)
        check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[-1])


# ---- corridors at the rim of the neighbourhood ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
def test_the_only_corridor_lies_exactly_at_the_radius(side):
    """the free stretch ends (left) / begins (right) on the last coordinate the ranks looked at: rows beyond it were not gathered, so nothing but the part inside
    the radius counts - wide enough here (max_distance + 1 bases of it are inside)"""
    if side == "left":
        R = X - RADIUS + MAXD             # free: (X - RADIUS - 1, R), the unseen row before it ends at X - RADIUS - 1 at the latest
        rows = [(DEL, 0, X - RADIUS - 101, X - RADIUS - 1, -1, 0)] + dense(DEL, 0, R, X + RADIUS + 5000)
        check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[R])
    else:
        L = X + RADIUS - MAXD             # free: (L, X + RADIUS + 1)
        rows = dense(DEL, 0, X - RADIUS - 5000, L - 599) + [(DEL, 0, L - 100, L, -1, 0), (DEL, 0, X + RADIUS + 1, X + RADIUS + 101, -1, 0)]
        W = check(["c"], 2, [(0, X)], rows, MAXD, RADIUS)
        assert L < _cuts(W)[0][1] <= X + RADIUS + 1


@pytest.mark.parametrize("side", ["left", "right"])
def test_the_corridor_at_the_radius_is_one_base_too_narrow_inside_it(side):
    """as above with max_distance bases of the free stretch inside the radius and an unseen row right behind the rim: one partition"""
    if side == "left":
        R = X - RADIUS + MAXD - 1
        rows = [(DEL, 0, X - RADIUS - 101, X - RADIUS - 1, -1, 0)] + dense(DEL, 0, R, X + RADIUS + 5000)
    else:
        L = X + RADIUS - MAXD + 1
        rows = dense(DEL, 0, X - RADIUS - 5000, L - 599) + [(DEL, 0, L - 100, L, -1, 0), (DEL, 0, X + RADIUS + 1, X + RADIUS + 101, -1, 0)]
    assert len(oracle_partitions(rows, ["c"], MAXD)) == 1
    check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[-1])


@pytest.mark.parametrize("side", ["left", "right"])
def test_a_stretch_that_begins_inside_the_radius_and_ends_outside_it(side):
    """one long row crosses the rim of the neighbourhood; the rows that continue its partition lie outside.  Behind the stretch nothing was looked at."""
    if side == "right":
        rows = dense(DEL, 0, X - 3000, X + RADIUS - 2000) + [(DEL, 0, X + RADIUS - 1500, X + RADIUS + 40000, -1, 0)] + dense(DEL, 0, X + RADIUS + 40500, X + RADIUS + 60000)
        rows += dense(DEL, 0, X - RADIUS - 60000, X - 3000 - MAXD - 100)              # a real corridor of max_distance + 1 at X - 3000
        rows[-1] = (DEL, 0, X - 3000 - MAXD - 101, X - 3000 - MAXD - 1, -1, 0)
        check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[X - 3000])
    else:
        rows = dense(DEL, 0, X - RADIUS - 60000, X - RADIUS - 40500) + [(DEL, 0, X - RADIUS - 40000, X - RADIUS + 1500, -1, 0)] + dense(DEL, 0, X - RADIUS + 2000, X + RADIUS + 60000)
        check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[-1])


def test_one_long_deletion_spans_the_proposal():
    """the proposal lies inside one signature of 150 kb: its partition (DEL rows end next to its start) must stay whole; other types have corridors under it -
    which are none, a cut inside ANY signature's [start, end] is not taken"""
    big = (DEL, 0, X - 70000, X + 80000, -1, 0)
    rows = [big] + dense(DEL, 0, X - 90000, X - 70000) + dense(INS, 0, X - 60000, X - 50000) + dense(INS, 0, X + 20000, X + 30000)
    W = check(["c"], 2, [(0, X)], rows, MAXD, RADIUS)
    assert not (big[2] < _cuts(W)[0][1] <= big[3])
    # and with the run going on beyond the radius on both sides: nothing to cut at
    rows = [big] + dense(DEL, 0, X - 200000, X - 70000) + dense(DEL, 0, X + 80100, X + 200000)
    check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[-1])


def test_rows_with_start_behind_end_and_rows_at_coordinate_zero():
    """a contig that begins with signatures: the proposal at 3000 may move down to coordinate 0 - the rows at 0 then belong above the cut together with the rest
    of their partition; rows stored with start > end (keyed by their end) are covered from end to start"""
    names = ["a", "b"]
    rows = [(DEL, 1, 0, 0, -1, 0), (DEL, 1, 0, 400, -1, 0), (INS, 1, 0, 60, -1, 0), (BND, 1, 0, 1, 0, 5)] + dense(DEL, 1, 300, 9000) + dense(INS, 1, 200, 9000)
    rows += [(DEL, 1, 4100, 3950, -1, 0), (INV, 1, 2600, 2100, -1, 0), (DUP_INT, 0, 10, 500, 1, 0), (DUP_INT, 0, 10, 500, 1, 2999), (DUP_INT, 0, 10, 500, 1, 3001)]
    check(names, 2, [(1, 3000)], rows, MAXD, 5000)
    # a reversed row closes what would be a corridor by its start alone: [X - 1200, X + 300] is covered by (start X + 300, end X - 1200)
    rows = dense(DEL, 0, X - 120000, X - 1300) + [(DEL, 0, X + 300, X - 1200, -1, 0)] + dense(DEL, 0, X + 400, X + 120000)
    check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[-1])
    # ... and leaves one where both of its ends stay clear of it
    rows = dense(DEL, 0, X - 120000, X - 2500) + [(DEL, 0, X - 1500, X - 2100, -1, 0)] + dense(DEL, 0, X - 1500 + MAXD + 1, X + 120000)
    check(["c"], 2, [(0, X)], rows, MAXD, RADIUS, expect=[X - 1500 + MAXD + 1])


# ---- several cuts in one contig ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [3, 4])
def test_all_cuts_of_a_contig_fall_back_together(world):
    """two and three proposals inside one dense contig, none with a corridor in reach: all of them end at the contig's first base, in order"""
    rows = dense(DEL, 0, 0, 3000000, step=700) + dense(INS, 0, 100, 3000000, step=900, length=30)
    props = [(0, 3000000 * r // world) for r in range(1, world)]
    check(["c"], world, props, rows, MAXD, RADIUS, expect=[-1] * (world - 1))


def test_a_cut_that_falls_back_takes_the_cuts_below_it_along():
    """three proposals in one contig: the lowest finds a corridor, the middle one none, the highest finds one.  The middle cut falls to the first base and the
    lowest has to follow it (cuts stay monotone); the highest keeps its corridor."""
    a, b, c = 1000000, 2000000, 3000000
    rows = dense(DEL, 0, a - 150000, a - 2000) + dense(DEL, 0, a + 2000, a + 150000)            # free around a
    rows += dense(DEL, 0, b - 150000, b + 150000)                                               # nothing free around b
    rows += dense(DEL, 0, c - 150000, c - 5000) + dense(DEL, 0, c - 1000, c + 150000)           # free before c - 1000
    W = check(["c"], 4, [(0, a), (0, b), (0, c)], rows, MAXD, RADIUS, expect=[-1, -1, c - 1000])
    assert sorted(set(_owners(W, rows))) == [2, 3]
    # the lowest and the highest alone keep their corridors
    check(["c", "d"], 4, [(0, a), (1, -1), (1, -1)], rows, MAXD, RADIUS, expect=[a, -1, -1])


def test_two_cuts_into_the_same_corridor():
    rows = dense(DEL, 0, 0, 400000) + dense(DEL, 0, 420000, 900000)
    W = check(["c"], 3, [(0, 405000), (0, 415000)], rows, MAXD, RADIUS)
    assert all(399600 < x <= 420000 for _, x in _cuts(W))
    assert sorted(set(_owners(W, rows))) == [0, 2]


# ---- small contigs, empty ranks, more ranks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_contig_shorter_than_max_distance_and_ranks_without_rows(world):
    """three contigs, the middle one 600 bases long (shorter than max_distance) and proposed to be cut; the proposals by contig length put several cuts into the
    long contig, whose signatures all sit in its first 40 kb - most ranks own nothing"""
    names, lengths = ["k1", "k2", "k3"], [5000000, 600, 900000]
    rows = dense(DEL, 0, 1000, 40000) + dense(INS, 0, 1200, 40000, length=20) + [(DEL, 1, 100, 180, -1, 0), (DEL, 1, 400, 470, -1, 0), (INS, 1, 590, 640, -1, 0)]
    rows += dense(BND, 2, 100000, 130000, contig2=0) + [(DUP_INT, 0, 1500, 1900, 2, 110000), (DUP_INT, 0, 1500, 1900, 1, 300), (DUP_INT, 2, 7, 90, 1, 310)]
    w = multigpu.assign_windows(names, lengths, world)
    check(names, world, None, rows, MAXD, RADIUS, windows=w)
    crank = _crank(names)
    props = sorted([(1, 300)] + [(0, 20000 + 3000 * r) for r in range(world - 2)], key=lambda cx: (crank[cx[0]], cx[1]))
    W = check(names, world, props, rows, MAXD, RADIUS)
    assert len({o for o, r in zip(_owners(W, rows), rows) if r[1] == 1 and r[0] != DUP_INT}) == 1


# ---- every type next to a cut --------------------------------------------------------------------------------------------------------------------------
def test_bnd_dup_tan_and_dup_int_rows_next_to_the_cut():
    """BND rows (one base wide, keyed by pos1) and DUP_TAN rows fill what would be a corridor of the DEL rows; DUP_INT rows (keyed by their destination, not in
    coordinate order of anything) neither open nor close one and stay with the first base of their destination contig"""
    names = ["c1", "c2"]
    dels = dense(DEL, 0, X - 120000, X - 3000) + dense(DEL, 0, X + 3000, X + 120000)
    di = [(DUP_INT, 1, 100, 900, 0, p) for p in range(X - 2000, X + 2000, 250)] + [(DUP_INT, 0, X - 500, X + 500, 1, 40)]
    # free around X but for DUP_INT rows: the cut stays at the proposal
    W = check(names, 2, [(0, X)], dels + di, MAXD, RADIUS, expect=[X])
    assert set(_owners(W, di[:-1])) == {0} and _owners(W, di[-1:]) == [1]
    # BND rows every 900 bases across it: closed
    bnd = dense(BND, 0, X - 3000, X + 3100, step=900, contig2=1)
    check(names, 2, [(0, X)], dels + di + bnd, MAXD, RADIUS, expect=[-1])
    # BND rows cover pos1 and pos1 + 1: the row at X + 200 and the next one at X + 202 + max_distance leave exactly max_distance + 1 between them - open, and the
    # nearest coordinate to the proposal is the first one behind the row; one base less and it is closed
    bnd = dense(BND, 0, X - 3000, X + 201, step=800, contig2=1)
    assert bnd[-1][2] == X + 200
    check(names, 2, [(0, X)], dels + di + bnd + dense(BND, 0, X + 202 + MAXD, X + 3100, step=800, contig2=1), MAXD, RADIUS, expect=[X + 202])
    check(names, 2, [(0, X)], dels + di + bnd + dense(BND, 0, X + 201 + MAXD, X + 3100, step=800, contig2=1), MAXD, RADIUS, expect=[-1])
    # a DUP_TAN row across the proposal, with DEL rows under it
    tan = [(DUP_TAN, 0, X - 2500, X + 2500, -1, 2)]
    W = check(names, 2, [(0, X)], dels + tan + dense(DEL, 0, X - 120000, X + 120000, step=100000, length=10), MAXD, RADIUS)
    assert not (X - 2500 < _cuts(W)[0][1] <= X + 2500)


# ---- seeded sweep ----------------------------------------------------------------------------------------------------------------------------------------
def _random_layout(rng):
    max_d = rng.choice([20, 50, 100])
    radius = rng.choice([max_d // 2, max_d, 4 * max_d, 10 * max_d, 64 * max_d])
    n_contig = rng.randint(1, 3)
    names = rng.sample(["chr1", "chr10", "chr2", "chrX", "a"], n_contig)
    lengths = [rng.choice([max_d // 2, 8 * max_d, 40 * max_d, 120 * max_d]) for _ in names]
    rows = []
    for c, ln in enumerate(lengths):
        pos = rng.randint(0, max_d)
        while pos < ln:
            # a dense run of one or two types, then a free stretch about max_distance wide (now and then a wide one)
            for t in rng.sample([DEL, INS, INV, DUP_TAN, BND], rng.randint(1, 2)):
                p = pos
                for _ in range(rng.randint(1, 12)):
                    w = rng.randint(0, max_d)
                    if t == BND:
                        rows.append((BND, c, p, p + 1, rng.randrange(n_contig), rng.randint(0, ln)))
                    elif rng.random() < 0.05:
                        rows.append((t, c, p + w, p, -1, 0))                      # start > end
                    else:
                        rows.append((t, c, p, p + w, -1, 0))
                    p += rng.randint(0, max_d)
            end = max(max(r[2], r[3]) for r in rows if r[1] == c)
            pos = end + (max_d + rng.randint(-3, 3) if rng.random() < 0.8 else rng.randint(2, 30) * max_d)
        for _ in range(rng.randint(0, 3)):
            rows.append((DUP_INT, rng.randrange(n_contig), rng.randint(0, 500), rng.randint(0, 500), c, rng.randint(0, ln)))
    world = rng.choice([2, 3, 4, 8])
    crank = _crank(names)
    props = sorted(((c, rng.choice([-1, rng.randint(1, max(1, lengths[c] - 1))])) for c in (rng.randrange(n_contig) for _ in range(world - 1))),
                   key=lambda cx: (crank[cx[0]], cx[1]))
    rng.shuffle(rows)
    return names, world, props, rows, max_d, radius


def test_seeded_sweep_of_small_layouts():
    moved = fell_back = 0
    for seed in range(400):
        names, world, props, rows, max_d, radius = _random_layout(random.Random(seed))
        try:
            W = check(names, world, props, rows, max_d, radius, seed=seed)
        except BaseException:
            print("layout seed %d: contigs %r world %d proposals %r max_distance %d radius %d, %d rows" % (seed, names, world, props, max_d, radius, len(rows)))
            raise
        for (_, x0), (_, x1) in zip(props, _cuts(W)):
            moved += x0 >= 0 and x1 > 0
            fell_back += x0 >= 0 and x1 < 0
    assert moved > 100 and fell_back > 100, (moved, fell_back)           # the sweep sees both outcomes often
