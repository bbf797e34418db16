"""What tests/test_segments.py (the oracle), tests/segments_child.py (a mutated oracle) and tests/test_gpu_segments.py (the device) share: comparisons of
COLLECT tables with tests/golden/g_segments_cases.json.gz and with the closed forms of the batches tests/segment_cases.py builds."""
import helpers as H
from svim_amd import _abi

GOLDEN = "g_segments_cases.json.gz"


def golden_difference(oracle, g, case):
    bam, hb, o = H.sam_case_batch(case, g)
    sig, bnd = oracle.collect(hb, _abi.Params.from_options(o))
    for what, tab, exp in (("main", sig, case["signatures"]), ("side", bnd, case["bnds"])):
        try:
            got = H.table_rows(tab, hb.references, hb.read_names)
        except AssertionError as e:            # a row no signature object can hold (end < start): a difference from the golden, whose rows are objects' rows
            return "%s / %s, %s list: a row that is no signature (%r)" % (case["name"], case["mode"], what, e)
        if got != exp:
            k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
            return "%s / %s%s, %s list row %d: got %r, the reference %r" % (case["name"], case["mode"], ", all_bnds" if case["options"]["all_bnds"] else "", what, k,
                                                                          got[k] if k < len(got) else None, exp[k] if k < len(exp) else None)
    return None


def rows_by_read(rows):
    by = {}
    for r in rows:
        by.setdefault(r[8] if r[0] == "BND" else r[5], []).append(r)
    return by


def golden_rows_by_read(options, all_bnds):
    """{read name: (main rows, side rows)} of the coordinate-mode golden entries made with these options"""
    g = H.load(GOLDEN)
    main, side = {}, {}
    for e in g["cases"]:
        if e["mode"] == "coordinate" and e["options"]["all_bnds"] == all_bnds and all(e["options"][k] == v for k, v in options.items()):
            main.update(rows_by_read(e["signatures"]))
            side.update(rows_by_read(e["bnds"]))
    return main, side


def placement_difference(hb, names, perm, sig, bnd, all_bnds, options):
    """the tables of a placement batch against the golden's rows per read, in the order of the permuted keys"""
    g_main, g_side = golden_rows_by_read(options, all_bnds)
    in_key_order = [names[i] for i in sorted(range(len(names)), key=lambda i: perm[i]) if names[i]]
    for what, tab, gold in (("main", sig, g_main), ("side", bnd, g_side)):
        got = H.table_rows(tab, hb.references, hb.read_names)
        exp = [r for nm in in_key_order for r in gold.get(nm, [])]
        if got != exp:
            k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
            return "%s list, %d rows against %d, row %d: %r != %r" % (what, len(got), len(exp), k, got[k:k + 1], exp[k:k + 1])
    return None


def placement_owners(hb):
    so = hb.arrays["seg_off"]
    return {i for i in range(hb.n_rec) if so[i + 1] > so[i]}


def many_rows_capacity_difference(hb, sig, layouts):
    """segment_cases.many_rows_case: per read, the entries of the list its layout fills - breakends of a "bnd" read (each one an entry of the translocation
    list), copies of the one DUP_TAN of a "tan" read (each one an entry of the tandem list) - against the read's n_seg, taken from seg_off of the built batch:
    equal where every row is good (the list is at the capacity of the read's workspace), lower by the rows below min_mapq otherwise"""
    so = hb.arrays["seg_off"]
    typ, rid, copies = sig.type[:sig.n], sig.read_id[:sig.n], sig.pos2[:sig.n]
    n_full = 0
    for r, (layout, bad) in sorted(layouts.items()):
        n_seg = int(so[r + 1]) - int(so[r])
        mine = rid == hb.arrays["read_id"][r]
        if layout == "bnd":
            got = int((mine & (typ == _abi.SVX_BND)).sum())
        else:
            c = copies[mine & (typ == _abi.SVX_DUP_TAN)].tolist()
            if len(c) != 1:
                return "record %d: %d DUP_TAN rows" % (r, len(c))
            got = int(c[0])
        if got != n_seg - bad:
            return "record %d (%s, n_seg %d, %d rows below min_mapq): list of %d entries" % (r, layout, n_seg, bad, got)
        n_full += bad == 0
    assert n_full >= 12
    return None
