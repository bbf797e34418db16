#!/usr/bin/env python3
"""Generate tests/golden/g_combine_threshold_cases.json.gz by RUNNING THE REFERENCE's COMBINE step on the directed cases of tests/combine_threshold_cases.py.

Build container only (needs the reference checkout make_golden.py reads; make_golden_combine.py is imported for its stubs and its run()).  Every case goes
through merge_translocations_at_insertions, flag_cutpaste_candidates and combine_clusters (--skip_consensus) exactly as the cases of g_combine_cases.json.gz do;
what the reference returns must be what the case's author wrote down (`expect`), and a case on the wrong side of its threshold stops the generator with its
name.  The reference keeps the indices the stage 4 walk removes to itself: they are taken from a SECOND call of combine_clusters on the same lists with the
breakend list empty and the merged clusters of the first call appended to the insertion-from list - the same candidates walk past the same insertions, and the
insertions that are gone afterwards are the walk's alone; the union with stage 2's indices must have the size the first call's insertion list lost.
Stored: rows, options, expected rows, the two removal lists, list sizes after the call, exception names and list sizes of the refused cases.  DATA ONLY: no
reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_combine_thresholds.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_combine as MGC       # noqa: E402  (stubs, the reference on the path, tests/ on the path)
import combine_threshold_cases as T     # noqa: E402
from make_golden_combine import MG, SVIM_COMBINE, SVIM_merging     # noqa: E402


def walk_removals(case):
    """indices the stage 4 walk removes (inserted_regions_to_remove_2 of combine_clusters)"""
    o = types.SimpleNamespace(**case.opt)
    c6, _ = MGC.objects(case)
    dele, insr, inv, tan, dint, bnd = c6
    new_from, _ = SVIM_merging.merge_translocations_at_insertions(list(bnd), list(insr), o)
    before = list(insr)
    SVIM_COMBINE.combine_clusters((dele, insr, inv, tan, dint + new_from, []), o)
    left = {id(c) for c in insr}
    return [k for k, c in enumerate(before) if id(c) not in left]


def main():
    assert MGC.OPT == T.OPT
    res = []
    for c in T.cases():
        exp = MGC.run(c)
        assert "raises" not in exp, c.name
        exp["inserted_regions_to_remove_2"] = walk_removals(c)
        gone = set(exp["inserted_regions_to_remove"]) | set(exp["inserted_regions_to_remove_2"])
        assert len(gone) == exp["n_ins_before"] - exp["n_ins_after"], c.name
        assert T.disagreement(c, exp) is None, T.disagreement(c, exp)
        res.append({"name": c.name, "family": c.family, "references": c.references, "signatures_fully_covered": c.sigs, "options": c.opt,
                    "clusters": [c.lists[t] for t in T.TYPES], "expected": exp})
    table = T.coverage(T.cases())
    for name, sides in T.REQUIRED.items():
        for side in sides:
            assert table.get(name, {}).get(side), "no case %s %r" % (side, name)
    raises = {}
    for c in T.refused():
        o = types.SimpleNamespace(**c.opt)
        lists = MGC.objects(c)[0]
        what = None
        try:
            SVIM_COMBINE.combine_clusters(tuple(lists), o)
        except Exception as e:          # noqa: BLE001  (whatever the reference raises is the finding)
            what = type(e).__name__
        if True:
            raises[c.name] = {"raises": what, "dup_int_dest_ends": [x.dest_end for x in lists[4]], "state": [len(lists[1]), len(lists[4]), len(lists[5])], "references": c.references,
                              "signatures_fully_covered": c.sigs, "options": c.opt, "clusters": [c.lists[t] for t in T.TYPES]}
    assert {k: v["raises"] for k, v in raises.items()} == T.EXPECTED_RAISES, raises
    assert {k: v["state"] for k, v in raises.items()} == T.EXPECTED_STATE, {k: v["state"] for k, v in raises.items()}
    assert raises["refused/merged_end_beyond_int32"]["dup_int_dest_ends"] == [T.BEYOND_INT32_DEST_END]
    print(len(res), "cases in", len(T.FAMILIES), "families; refused:", {k: v["raises"] for k, v in raises.items()})
    MG.dump("g_combine_threshold_cases.json.gz", {"cases": res, "refused": raises,
                                                  "source": "svim.SVIM_merging.merge_translocations_at_insertions / flag_cutpaste_candidates and "
                                                            "svim.SVIM_COMBINE.combine_clusters (skip_consensus) on the directed cases of tests/combine_threshold_cases.py"})


if __name__ == "__main__":
    main()
