#!/usr/bin/env python3
"""Generate tests/golden/g_segments_cases.json.gz by RUNNING THE REFERENCE's COLLECT step on the directed split-read cases of tests/segment_cases.py.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them).  Every case runs on its own
first, through analyze_alignment_file_coordsorted and analyze_alignment_file_querysorted, with all_bnds off and on: the main list must be the tokens the case's
author wrote down (a case on the wrong side of its threshold stops the generator), an exception is recorded by its type.  The cases of a family that did not raise
are then written as ONE SAM text per file order, with the rows the reference returned for it, in the row layout of g2_collect.json.gz.  DATA ONLY: no reference
source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segments.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG    # noqa: E402  (stubs pysam / edlib, puts the reference on the path)
import segment_cases as SC   # noqa: E402


def run(cases, opt, mode, all_bnds):
    o = MG.options(all_bnds=all_bnds, **opt)
    text = SC.sam_texts(cases)[mode]
    sigs, bnds = MG.run_collect(text, o, mode)
    return text, o, [MG.sig_row(s) for s in sigs], [MG.sig_row(s) for s in bnds]


def main():
    out, expect, raises = [], {}, []
    for fam, opt, cases in SC.families():
        good = []
        for c in cases:
            assert c.family == fam
            failed = None
            for mode in SC.MODES:
                for all_bnds in (False, True):
                    try:
                        _, _, main_rows, side_rows = run([c], opt, mode, all_bnds)
                    except Exception as e:          # noqa: BLE001  (whatever the reference raises is the finding)
                        failed = type(e).__name__
                        raises.append({"family": fam, "name": c.name, "mode": mode, "all_bnds": all_bnds, "raises": failed})
                        continue
                    got = [SC.token(r) for r in main_rows]
                    assert got == c.expect[mode], "%s / %s (%s%s): the reference says %r, the case expects %r" % (fam, c.name, mode, ", all_bnds" if all_bnds else "",
                                                                                                               got, c.expect[mode])
                    assert all_bnds or not side_rows
            if failed is None:
                good.append(c)
                expect["%s|%s" % (fam, c.name)] = c.expect
        for mode in SC.MODES:
            for all_bnds in (False, True):
                text, o, main_rows, side_rows = run(good, opt, mode, all_bnds)
                # the family's rows are its cases' rows: nothing one read does depends on another
                by = {}
                for r in main_rows:
                    by.setdefault("|".join(SC.case_of_read(r[5] if r[0] != "BND" else r[8])), []).append(SC.token(r))
                for c in good:
                    assert by.get("%s|%s" % (fam, c.name), []) == c.expect[mode], (fam, c.name, mode)
                out.append({"name": fam, "sam": text if not all_bnds else None, "mode": mode, "options": MG.opt_dict(o), "signatures": main_rows, "bnds": side_rows})
        print(fam, len(good), "cases,", sum(len(c.reads) for c in good), "reads")
    MG.dump("g_segments_cases.json.gz", {"cases": out, "expect": expect, "raises": raises, "references": SC.REFERENCES, "lengths": SC.LENGTHS,
                                         "source": "svim.SVIM_COLLECT.analyze_alignment_file_{coord,query}sorted (src/svim/SVIM_COLLECT.py:96-167) on the directed "
                                                   "split-read cases of tests/segment_cases.py"})


if __name__ == "__main__":
    main()
