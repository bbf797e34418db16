"""COMBINE on the CPU: the Python replay of the reference's COMBINE (tests/combine_consumer.py over form_partitions, the two distance functions and
partition_and_cluster_candidates of svim_amd/SVIM_clustering.py, the linkage from the oracle) against what the REFERENCE returned for the directed cases of
tests/combine_threshold_cases.py (tests/golden/g_combine_threshold_cases.json.gz, written by tests/golden/make_golden_combine_thresholds.py, which also confirmed
every expectation the cases' author wrote down); a coverage table (every comparison has a case on each side it needs); the refusals; and two mutant tables:
MUTANTS, one-step changes of the replay and of the functions it takes from SVIM_clustering.py, each compiled into module objects of its own and held to the same
golden - the comparison must FAIL for every one of them - and EQUIVALENT, changes no input can tell from the original, which must PASS.
tests/test_gpu_combine_threshold_cases.py holds the device to the same file."""
import os
import types

import numpy as np
import pytest

import combine_cases as CC
import combine_threshold_cases as T
import helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = "g_combine_threshold_cases.json.gz"
SOURCES = {"consumer": os.path.join(HERE, "combine_consumer.py"), "clustering": os.path.join(REPO, "svim_amd", "SVIM_clustering.py")}


@pytest.fixture(scope="module")
def golden():
    return H.load(GOLDEN)


def fresh_modules(oracle, consumer_src, clustering_src):
    """the two sources compiled into module objects of their own: the replay over ITS copy of the clustering functions, the linkage served by the oracle.
    Nothing that is imported anywhere else is touched."""
    class LinkageOnly(object):
        def linkage_fcluster(self, problems, cutoff):
            return [np.asarray(oracle.linkage_fcluster(n, np.asarray(d, dtype=np.float64), cutoff)) for n, d in problems]
    clu = types.ModuleType("svim_amd.SVIM_clustering_under_test")
    clu.__package__ = "svim_amd"
    exec(compile(clustering_src, SOURCES["clustering"], "exec"), clu.__dict__)
    clu._lib = types.SimpleNamespace(engine=lambda device=None: LinkageOnly())
    con = types.ModuleType("combine_consumer_under_test")
    exec(compile(consumer_src, SOURCES["consumer"], "exec"), con.__dict__)
    con.partition_and_cluster_candidates, con.span_position_distance_clusters = clu.partition_and_cluster_candidates, clu.span_position_distance_clusters
    return con


def read_sources():
    out = {}
    for k, p in SOURCES.items():
        with open(p) as fh:
            out[k] = fh.read()
    return out


def replay_difference(con, case):
    """None when con.consume on the case's lists gives the golden's `expected` block (helpers.first_json_difference, as g_combine.json.gz is compared)"""
    lists6, idx = CC.case_objects(case)
    exp = dict(case["expected"])
    exp.pop("inserted_regions_to_remove_2")                         # (the replay keeps the walk's list to itself, as the reference does)
    lists = [list(x) for x in lists6]
    got = con.consume(lists, types.SimpleNamespace(**case["options"]), idx)
    got["n_bnd_after"] = len(lists[5])                              # (the lists are left as the reference leaves them)
    d = H.first_json_difference(got, exp)
    return None if d is None else "%s: %s" % (case["name"], d)


@pytest.fixture(scope="module")
def replay(oracle):
    src = read_sources()
    return fresh_modules(oracle, src["consumer"], src["clustering"])


def test_golden_is_the_cases_of_this_tree(golden):
    """the rows, options and expectations the golden was computed from are the ones tests/combine_threshold_cases.py builds today; the reference agreed with every
    author and raised exactly where the cases say so; the file holds data only and stays small"""
    cases = T.cases()
    assert [c["name"] for c in golden["cases"]] == [c.name for c in cases] and len(cases) == 122
    for c, g in zip(cases, golden["cases"]):
        assert (g["family"], g["references"], g["signatures_fully_covered"], g["options"]) == (c.family, c.references, c.sigs, c.opt), c.name
        assert H.first_json_difference(g["clusters"], [c.lists[t] for t in T.TYPES], rtol=0) is None, c.name
        assert T.disagreement(c, g["expected"]) is None, T.disagreement(c, g["expected"])
        gone = set(g["expected"]["inserted_regions_to_remove"]) | set(g["expected"]["inserted_regions_to_remove_2"])
        assert len(gone) == g["expected"]["n_ins_before"] - g["expected"]["n_ins_after"], c.name
    assert {c.family for c in cases} == set(T.FAMILIES)
    assert {k: v["raises"] for k, v in golden["refused"].items()} == T.EXPECTED_RAISES and {k: v["state"] for k, v in golden["refused"].items()} == T.EXPECTED_STATE
    for c in T.refused():
        assert golden["refused"][c.name]["clusters"] == [c.lists[t] for t in T.TYPES], c.name
    assert os.path.getsize(os.path.join(H.GOLDEN, GOLDEN)) < 200000


def test_every_comparison_has_a_case_on_each_side():
    """The coverage table: every case is tagged with the comparisons it sits below, on or above; every comparison of REQUIRED must have a case on each side listed
    there, so a later edit of the cases cannot silently lose one."""
    table = T.coverage(T.cases())
    assert sorted(table) == sorted(T.REQUIRED)
    for name, sides in T.REQUIRED.items():
        for side in sides:
            assert table[name].get(side), "no case %s %r" % (side, name)


@pytest.mark.parametrize("family", T.FAMILIES)
def test_replay_against_the_reference(golden, replay, family):
    ran = 0
    for case in golden["cases"]:
        if case["family"] == family:
            d = replay_difference(replay, case)
            assert d is None, d
            ran += 1
    assert ran


def test_refusals(golden, replay):
    """The reference divides by zero on a tandem duplication cluster without source span (before it touches a list) and in stage 3 on a deletion cluster and an
    insertion-from cluster that both have no span (after it extended the breakend and the insertion-from lists); the replay does the same, and so does the
    drop-in (svim_amd.SVIM_COMBINE.combine_clusters: the tandem case needs no engine; tests/test_gpu_combine_threshold_cases.py has both).  The IndexError of
    insertion-from clusters without a deletion cluster is held by the cases no_deletion_index_error and dup_int_without_deletions of g_combine_cases.json.gz."""
    from svim_amd import SVIM_COMBINE
    for name, g in golden["refused"].items():
        lists6, idx = CC.case_objects(g)
        if g["raises"] is None:          # a merged cluster that ends beyond 2^31 - 1: Python integers hold it; the device's int32 columns do not (the GPU module)
            got = replay.consume(lists6, types.SimpleNamespace(**g["options"]), idx)
            assert [r[5] for r in got["merged_insertion_from_clusters"]] == g["dup_int_dest_ends"] == [T.BEYOND_INT32_DEST_END]
            continue
        assert g["raises"] == "ZeroDivisionError"
        with pytest.raises(ZeroDivisionError):
            replay.consume(lists6, types.SimpleNamespace(**g["options"]), idx)
    g = golden["refused"]["refused/tandem_zero_span"]
    lists6, _ = CC.case_objects(g)

    class NeverCalled(object):
        def __getattr__(self, name):
            raise AssertionError("the engine is not to be asked for %s" % name)
    with pytest.raises(ZeroDivisionError):
        SVIM_COMBINE.combine_clusters(lists6, types.SimpleNamespace(**g["options"]), engine=NeverCalled())
    assert [len(lists6[k]) for k in (1, 4, 5)] == g["state"]


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------------------
# Every entry: (what it changes, which source, [(a piece of that source that occurs exactly once, its replacement)]).
_TIE = "return k if sorted_values[k] - x < x - sorted_values[k - 1] else k - 1"
_FAR = "if df > options.trans_sv_max_distance or dr > options.trans_sv_max_distance:"
_RATIO = "if cr.dest_contig != cf.dest_contig or not 0.95 <= (e - s + 1) / (dist + 1) <= 1.1:"
_DIST = "dist = abs(cr.dest_start - cf.dest_start)"
_NEW = "new_clusters.append(SignatureClusterBiLocal(cr.dest_contig, min(cr.dest_start, cf.dest_start), max(cr.dest_start, cf.dest_start), contig, s,"
_FLAG = "best = min(span_position_distance_clusters(d, c, options.position_distance_normalizer) for d in del_clusters)"
_W_INT = "            c2, s2, e2 = cur_int.get_destination()\n            while c2 < c1 or (c2 == c1 and e2 < s1):"
_W_TAN = "                c2, s2, e2 = cur_tan\n                while c2 < c1 or (c2 == c1 and e2 < s1):"
_H_INT = "            if c2 == c1 and s2 < e1 and (len1 - len2) / max(len1, len2) < 0.2:\n                remove2.append(k)\n        else:"
_H_TAN = "                if c2 == c1 and s2 < e1 and (len1 - len2) / max(len1, len2) < 0.2:\n                    remove2.append(k)\n    for k in sorted"
_TAN_DEST = "c.source_end + n * (c.source_end - max(0, c.source_start))"
_CLU = "    return abs((s1 + e1) // 2 - (s2 + e2) // 2) / position_distance_normalizer + abs((e1 - s1) - (e2 - s2)) / max(e1 - s1, e2 - s2)"
_MEAN = "int(round(sum(c.get_%s for c in cluster) / n))"


def _in(where, line, old, new):
    assert line.count(old) == 1, (line, old)
    return where, [(line, line.replace(old, new))]


def _m(what, pair):
    return (what,) + pair


def _rounding():
    out = []
    for coord in ("source()[1]", "source()[2]", "destination()[1]", "destination()[2]"):
        line = _MEAN % coord
        out.append(("mean of %s truncated" % coord, "clustering", [(line, "int(sum(c.get_%s for c in cluster) / n)" % coord)]))
        out.append(("mean of %s rounded half up" % coord, "clustering", [(line, "int(sum(c.get_%s for c in cluster) / n + 0.5)" % coord)]))
    return out


MUTANTS = [
    # get_closest_index
    ("bisect_left -> bisect_right", "consumer", [("k = bisect_left(sorted_values, x)", "k = __import__('bisect').bisect_right(sorted_values, x)")]),
    _m("tie: the upper index", _in("consumer", _TIE, "- x < x -", "- x <= x -")),
    ("nearest of the neighbours: before and after swapped", "consumer", [(_TIE, "return k - 1 if sorted_values[k] - x < x - sorted_values[k - 1] else k")]),
    ("the search by the insertion's end", "consumer", [('kf = closest_index(starts["fwd"][contig], s)', 'kf = closest_index(starts["fwd"][contig], e)')]),
    ("the rev/rev search by the insertion's end", "consumer", [('kr = closest_index(starts["rev"][contig], s)', 'kr = closest_index(starts["rev"][contig], e)')]),
    ("lists ordered by source start", "consumer", [("by[d][contig] = sorted(by[d][contig], key=lambda c: c.get_key())", "by[d][contig] = sorted(by[d][contig], key=lambda c: c.source_start)")]),
    ("lists not ordered at all", "consumer", [("by[d][contig] = sorted(by[d][contig], key=lambda c: c.get_key())", "by[d][contig] = list(by[d][contig])")]),
    ("list order among equal keys reversed", "consumer", [("by[d][contig] = sorted(by[d][contig], key=lambda c: c.get_key())",
                                                          "by[d][contig] = sorted(reversed(by[d][contig]), key=lambda c: c.get_key())")]),
    # the mirror
    ("mirror: direction1 from direction1", "consumer", [('m.direction1 = "fwd" if c.direction2 == "rev" else "rev"', 'm.direction1 = "fwd" if c.direction1 == "rev" else "rev"')]),
    ("mirror: direction2 from direction2", "consumer", [('m.direction2 = "fwd" if c.direction1 == "rev" else "rev"', 'm.direction2 = "fwd" if c.direction2 == "rev" else "rev"')]),
    ("mirror: source and destination not swapped", "consumer", [("m = SignatureClusterBiLocal(c.dest_contig, c.dest_start, c.dest_end, c.source_contig, c.source_start, c.source_end, c.score, c.size,",
                                                                "m = SignatureClusterBiLocal(c.source_contig, c.source_start, c.source_end, c.dest_contig, c.dest_start, c.dest_end, c.score, c.size,")]),
    # trans_sv_max_distance
    _m("fwd distance: > -> >=", _in("consumer", _FAR, "df > options", "df >= options")), _m("rev distance: > -> >=", _in("consumer", _FAR, "dr > options", "dr >= options")),
    _m("fwd distance: limit + 1", _in("consumer", _FAR, "df > options.trans_sv_max_distance", "df > options.trans_sv_max_distance + 1")),
    _m("fwd distance: limit - 1", _in("consumer", _FAR, "df > options.trans_sv_max_distance", "df > options.trans_sv_max_distance - 1")),
    _m("rev distance: limit + 1", _in("consumer", _FAR, "dr > options.trans_sv_max_distance:", "dr > options.trans_sv_max_distance + 1:")),
    _m("rev distance: limit - 1", _in("consumer", _FAR, "dr > options.trans_sv_max_distance:", "dr > options.trans_sv_max_distance - 1:")),
    _m("either list near is enough", _in("consumer", _FAR, " or ", " and ")),
    ("fwd distance without abs", "consumer", [('df, dr = abs(starts["fwd"][contig][kf] - s),', 'df, dr = (starts["fwd"][contig][kf] - s),')]),
    ("rev distance without abs", "consumer", [('abs(starts["rev"][contig][kr] - s)\n', '(starts["rev"][contig][kr] - s)\n')]),
    # the length ratio
    _m("0.95 <= -> <", _in("consumer", _RATIO, "0.95 <=", "0.95 <")), _m("<= 1.1 -> <", _in("consumer", _RATIO, "<= 1.1", "< 1.1")),
    _m("0.95 -> 0.9501", _in("consumer", _RATIO, "0.95", "0.9501")), _m("0.95 -> 0.9499", _in("consumer", _RATIO, "0.95", "0.9499")),
    _m("1.1 -> 1.1001", _in("consumer", _RATIO, "1.1:", "1.1001:")), _m("1.1 -> 1.0999", _in("consumer", _RATIO, "1.1:", "1.0999:")),
    _m("length without + 1", _in("consumer", _RATIO, "(e - s + 1)", "(e - s)")), _m("distance without + 1", _in("consumer", _RATIO, "(dist + 1)", "(dist)")),
    _m("length + 2", _in("consumer", _RATIO, "(e - s + 1)", "(e - s + 2)")), _m("distance + 2", _in("consumer", _RATIO, "(dist + 1)", "(dist + 2)")),
    _m("destination contigs not compared", _in("consumer", _RATIO, "cr.dest_contig != cf.dest_contig or not", "not")),
    _m("distance without abs", _in("consumer", _DIST, "abs(cr.dest_start - cf.dest_start)", "(cr.dest_start - cf.dest_start)")),
    _m("distance between destination ends", _in("consumer", _DIST, "abs(cr.dest_start - cf.dest_start)", "abs(cr.dest_end - cf.dest_end)")),
    # the merged cluster
    _m("merged source: min -> max", _in("consumer", _NEW, "min(cr.dest_start, cf.dest_start)", "max(cr.dest_start, cf.dest_start)")),
    _m("merged source end: max -> min", _in("consumer", _NEW, "max(cr.dest_start, cf.dest_start), contig", "min(cr.dest_start, cf.dest_start), contig")),
    ("merged destination end: the insertion's", "consumer", [('s + dist, score, len(members), members, "DUP_INT", ins.std_span, ins.std_pos))', 'e, score, len(members), members, "DUP_INT", ins.std_span, ins.std_pos))')]),
    ("merged stds swapped", "consumer", [('"DUP_INT", ins.std_span, ins.std_pos))', '"DUP_INT", ins.std_pos, ins.std_span))')]),
    ("member order: rev/rev before fwd/fwd", "consumer", [("members = ins.members + cf.members + cr.members", "members = ins.members + cr.members + cf.members")]),
    # the merged score
    ("distance factor: 100 -> 101", "consumer", [("f *= max(0, 100 - d) / 100", "f *= max(0, 101 - d) / 100")]), ("distance factor: 100 -> 99", "consumer", [("f *= max(0, 100 - d) / 100", "f *= max(0, 99 - d) / 100")]),
    ("distance factor: max -> min", "consumer", [("f *= max(0, 100 - d) / 100", "f *= min(0, 100 - d) / 100")]),
    ("std factor: 100 -> 101", "consumer", [("max(0, 100 - s) / 100", "max(0, 101 - s) / 100")]), ("std factor: 100 -> 99", "consumer", [("max(0, 100 - s) / 100", "max(0, 99 - s) / 100")]),
    ("std factor: None counts as 0", "consumer", [("f *= 1 if s is None else", "f *= 0 if s is None else")]),
    ("sixth root -> fifth", "consumer", [("pow(f, 1 / 6)", "pow(f, 1 / 5)")]), ("sixth root -> seventh", "consumer", [("pow(f, 1 / 6)", "pow(f, 1 / 7)")]),
    # stage 3
    _m("cut&paste: min -> max over the deletions", _in("consumer", _FLAG, "best = min(", "best = max(")),
    ("cut&paste: <= -> <", "consumer", [("cutpaste=best <= options.del_ins_dup_max_distance", "cutpaste=best < options.del_ins_dup_max_distance")]),
    _m("cluster distance: centre truncated, not floored", _in("clustering", _CLU, "abs((s1 + e1) // 2 - (s2 + e2) // 2)", "abs(int((s1 + e1) / 2) - int((s2 + e2) / 2))")),
    _m("cluster distance: max -> min of the spans", _in("clustering", _CLU, "max(e1 - s1, e2 - s2)", "min(e1 - s1, e2 - s2)")),
    _m("cluster distance: + -> - between the terms", _in("clustering", _CLU, "normalizer + abs(", "normalizer - abs(")),
    # stage 1
    ("copies truncated", "consumer", [("int(round((de - ds) / (se - ss)))", "int((de - ds) / (se - ss))")]), ("copies rounded half up", "consumer", [("int(round((de - ds) / (se - ss)))", "int((de - ds) / (se - ss) + 0.5)")]),
    ("fully_covered: all members", "consumer", [("bool(sum(m.fully_covered for m in c.members))", "all(m.fully_covered for m in c.members)")]),
    ("fully_covered: the first member", "consumer", [("bool(sum(m.fully_covered for m in c.members))", "bool(c.members[0].fully_covered)")]),
    ("DEL score >= 0", "consumer", [("for c in dele if c.score > 0]", "for c in dele if c.score >= 0]")]), ("INS score >= 0", "consumer", [("for c in insr if c.score > 0]", "for c in insr if c.score >= 0]")]),
    ("DEL start not clamped", "consumer", [('"CandidateDeletion", idx, c.members, source_contig=c.contig, source_start=max(0, c.start)', '"CandidateDeletion", idx, c.members, source_contig=c.contig, source_start=c.start')]),
    ("INV start not clamped", "consumer", [('"CandidateInversion", idx, c.members, source_contig=c.contig, source_start=max(0, c.start)', '"CandidateInversion", idx, c.members, source_contig=c.contig, source_start=c.start')]),
    ("INS start not clamped", "consumer", [("dest_start=max(0, c.start)", "dest_start=c.start")]),
    ("BND source not clamped", "consumer", [("source_start=max(0, c.source_start), source_direction", "source_start=c.source_start, source_direction")]),
    ("BND destination not clamped", "consumer", [("dest_start=max(0, c.dest_start), dest_direction", "dest_start=c.dest_start, dest_direction")]),
    ("DUP_TAN start not clamped", "consumer", [('"CandidateDuplicationTandem", idx, c.members, source_contig=c.source_contig, source_start=max(0, c.source_start)',
                                               '"CandidateDuplicationTandem", idx, c.members, source_contig=c.source_contig, source_start=c.source_start')]),
    ("DUP_INT source not clamped", "consumer", [("max(0, source_start), source_end", "source_start, source_end")]), ("DUP_INT destination not clamped", "consumer", [("max(0, dest_start), dest_end", "dest_start, dest_end")]),
    ("BND directions swapped", "consumer", [("source_direction=c.direction1,", "source_direction=c.direction2,")]),
    # the walk
    _m("interspersed: end2 < start1 -> <=", _in("consumer", _W_INT, "e2 < s1", "e2 <= s1")), _m("tandem: end2 < start1 -> <=", _in("consumer", _W_TAN, "e2 < s1", "e2 <= s1")),
    _m("interspersed: end2 + 1 < start1", _in("consumer", _W_INT, "e2 < s1", "e2 + 1 < s1")), _m("tandem: end2 + 1 < start1", _in("consumer", _W_TAN, "e2 < s1", "e2 + 1 < s1")),
    _m("interspersed: start2 < end1 -> <=", _in("consumer", _H_INT, "s2 < e1", "s2 <= e1")), _m("tandem: start2 < end1 -> <=", _in("consumer", _H_TAN, "s2 < e1", "s2 <= e1")),
    _m("interspersed: start2 + 1 < end1", _in("consumer", _H_INT, "s2 < e1", "s2 + 1 < e1")), _m("tandem: start2 + 1 < end1", _in("consumer", _H_TAN, "s2 < e1", "s2 + 1 < e1")),
    _m("interspersed: < 0.2 -> <=", _in("consumer", _H_INT, "< 0.2", "<= 0.2")), _m("tandem: < 0.2 -> <=", _in("consumer", _H_TAN, "< 0.2", "<= 0.2")),
    _m("interspersed: 0.2 -> 0.19", _in("consumer", _H_INT, "< 0.2", "< 0.19")), _m("tandem: 0.2 -> 0.19", _in("consumer", _H_TAN, "< 0.2", "< 0.19")),
    _m("interspersed: max -> min of the lengths", _in("consumer", _H_INT, "max(len1, len2)", "min(len1, len2)")), _m("tandem: max -> min of the lengths", _in("consumer", _H_TAN, "max(len1, len2)", "min(len1, len2)")),
    _m("interspersed: abs of the length difference", _in("consumer", _H_INT, "(len1 - len2)", "abs(len1 - len2)")), _m("tandem: abs of the length difference", _in("consumer", _H_TAN, "(len1 - len2)", "abs(len1 - len2)")),
    ("the tandem list consulted beside the interspersed one", "consumer", [("                remove2.append(k)\n        else:\n            if cur_tan is not None:", "                remove2.append(k)\n        if cur_int is None or True:\n            if cur_tan is not None:")]),
    ("duplications walked in source order", "consumer", [("it_int = iter(sorted(dup_cands, key=lambda c: c.get_destination()))", "it_int = iter(sorted(dup_cands, key=lambda c: c.get_source()))")]),
    ("duplications walked in list order", "consumer", [("it_int = iter(sorted(dup_cands, key=lambda c: c.get_destination()))", "it_int = iter(list(dup_cands))")]),
    _m("tandem destination from the unclamped start", _in("consumer", _TAN_DEST, "max(0, c.source_start)", "c.source_start")),
    _m("tandem destination from the source start", _in("consumer", _TAN_DEST, "c.source_end + n *", "c.source_start + n *")),
    ("only stage 2's removals applied", "consumer", [("for k in sorted(set(remove1 + remove2), reverse=True):", "for k in sorted(set(remove1), reverse=True):")]),
    ("only the walk's removals applied", "consumer", [("for k in sorted(set(remove1 + remove2), reverse=True):", "for k in sorted(set(remove2), reverse=True):")]),
    # stage 5
    ("candidate key: source start", "consumer", [("return (self.type, self.source_contig, self.source_end)", "return (self.type, self.source_contig, self.source_start)")]),
    ("partition gap without max(0, .)", "consumer", [("return max(0, other.source_start - self.source_end)", "return other.source_start - self.source_end")]),
    ("partition gap from the previous start", "consumer", [("return max(0, other.source_start - self.source_end)", "return max(0, other.source_start - self.source_start)")]),
    ("partition gap: source contig not compared", "consumer", [("if self.type == other.type and self.source_contig == other.source_contig:", "if self.type == other.type:")]),
    ("partition rule: <= -> <", "clustering", [("if parts and parts[-1][-1].downstream_distance_to(s) <= max_distance:", "if parts and parts[-1][-1].downstream_distance_to(s) < max_distance:")]),
    ("partition rule: limit + 1", "clustering", [("downstream_distance_to(s) <= max_distance:", "downstream_distance_to(s) <= max_distance + 1:")]),
    ("candidate distance: destination ends", "clustering", [("abs(signature1.get_destination()[1] - signature2.get_destination()[1])", "abs(signature1.get_destination()[2] - signature2.get_destination()[2])")]),
    ("candidate distance: max -> min of the spans", "clustering", [("abs(span1 - span2) / max(span1, span2)", "abs(span1 - span2) / min(span1, span2)")]),
    ("candidate distance: source term dropped", "clustering", [("return pd_source + pd_dest + abs(span1 - span2)", "return pd_dest + abs(span1 - span2)")]),
    ("candidate distance: destination term dropped", "clustering", [("return pd_source + pd_dest + abs(span1 - span2)", "return pd_source + abs(span1 - span2)")]),
    ("sampling from 100 on", "clustering", [("if len(partition) > 100 else partition", "if len(partition) >= 100 else partition")]),
    ("sampling above 101", "clustering", [("if len(partition) > 100 else partition", "if len(partition) > 101 else partition")]),
    ("samples of 99", "clustering", [("sample(partition, 100)", "sample(partition, 99)")]), ("seed 1525", "clustering", [("seed(1524)", "seed(1525)")]),
    ("the generator seeded for every partition", "clustering", [("        part = sample(partition, 100)", "        seed(1524)\n        part = sample(partition, 100)")]),
    ("score of the first member", "clustering", [("max(c.score for c in cluster)", "cluster[0].score")]), ("lowest score", "clustering", [("max(c.score for c in cluster)", "min(c.score for c in cluster)")]),
    ("cutpaste: all members", "clustering", [("any(c.cutpaste for c in cluster)", "all(c.cutpaste for c in cluster)")]),
    ("members in reverse order", "clustering", [("[m for c in cluster for m in c.members]", "[m for c in reversed(cluster) for m in c.members]")]),
    ("std_span where std_pos goes", "clustering", [("mean(stds_pos) if stds_pos else None,", "mean(stds_span) if stds_span else None,")]),
] + _rounding()
# No input can tell these from the original.  They must SURVIVE; one that is detected means the argument is wrong.
EQUIVALENT = [
    # the four std factors are all multiplied into ONE product: which two the mirror swaps changes the order of the factors, never the set - the scores agree to
    # the last bits, and the comparison rule (helpers.first_json_difference) is relative 1e-9
    ("the mirror's std swap undone", "consumer", [("c.members, c.type, c.std_pos, c.std_span)", "c.members, c.type, c.std_span, c.std_pos)")]),
    # the loop in front of the test ends only where neither `c2 < c1` nor `c2 == c1 and e2 < s1` holds: c2 >= c1 there, so `<=` is `==`
    _m("interspersed hit: contig2 <= contig1", _in("consumer", _H_INT, "if c2 == c1 and", "if c2 <= c1 and")), _m("tandem hit: contig2 <= contig1", _in("consumer", _H_TAN, "if c2 == c1 and", "if c2 <= c1 and")),
    # every candidate of the list is an interspersed duplication
    ("partition gap: type not compared", "consumer", [("if self.type == other.type and self.source_contig == other.source_contig:", "if self.source_contig == other.source_contig:")]),
    ("the type test of the consolidation dropped", "clustering", [('if cluster[0].type != "DUP_INT":', 'if False:')]),
]


def test_no_mutant_of_the_replay_survives_the_golden_and_the_equivalent_ones_do(golden, oracle):
    """Every entry of MUTANTS (117) and EQUIVALENT (5) names pieces of tests/combine_consumer.py or svim_amd/SVIM_clustering.py that occur exactly once and their
    replacements; the mutated text is compiled into fresh module objects (fresh_modules: the imported modules are never patched) and held to
    g_combine_threshold_cases.json.gz case by case.  A mutant must give a DIFFERENT answer on at least one case - one that only raises does not count as
    detected -; an equivalent change, and the unchanged sources, must agree on every case."""
    src = read_sources()
    assert all(replay_difference(fresh_modules(oracle, src["consumer"], src["clustering"]), c) is None for c in golden["cases"])
    seen, survivors, detected = set(), [], []
    for k, (what, where, changes) in enumerate(MUTANTS + EQUIVALENT):
        mutated = dict(src)
        for old, new in changes:
            assert src[where].count(old) == 1, "mutant %d (%s): %r occurs %d times" % (k, what, old, src[where].count(old))
            mutated[where] = mutated[where].replace(old, new)
        text = mutated["consumer"] + mutated["clustering"]
        assert mutated != src and text not in seen, "mutant %d (%s) changes nothing new" % (k, what)
        seen.add(text)
        con = fresh_modules(oracle, mutated["consumer"], mutated["clustering"])
        found = None
        for case in golden["cases"]:
            try:
                found = replay_difference(con, case)
            except Exception:          # noqa: BLE001  (a mutant that dies on a case says nothing about that case)
                continue
            if found:
                break
        if k < len(MUTANTS) and not found:
            survivors.append("%d: %s" % (k, what))
        if k >= len(MUTANTS) and found:
            detected.append("%d: %s: %s" % (k, what, found))
    assert not survivors, "%d of %d mutants not detected:\n%s" % (len(survivors), len(MUTANTS), "\n".join(survivors))
    assert not detected, "changes held to be equivalent that the golden tells from the original:\n%s" % "\n".join(detected)
    assert len(MUTANTS) == 117 and len(EQUIVALENT) == 5
