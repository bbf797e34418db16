"""What tests/test_genotype_cases.py (oracle, CPU) and tests/test_gpu_genotype_cases.py (device) share - the object route and the table route over the cases of
tests/genotype_walk_cases.py, compared with tests/golden/g_genotype_cases.json.gz - and, run as a program, the child process of the mutant test: it holds the
oracle library that SVX_ORACLE_LIB names to the golden, case by case on the object route (SVIM_genotyping.genotype over svo_genotype).  Exit status 0:
everything agrees; DIFFERENT: a difference, printed.  Anything else (an exception ends Python with 1) is a failure of the child, not a verdict."""
import os
import sys
import types

DIFFERENT = 3
GOLDEN = "g_genotype_cases.json.gz"


class IndexHolder(object):
    """stands where SVIM_genotyping.genotype expects the alignment file: it only asks it for the index it keeps on it"""

    def __init__(self, index):
        self._svx_alignment_index = index


def golden_by_id(g):
    return {c["id"]: c["expected"] for c in g["cases"]}


def object_route(w, case, bam, engine):
    """SVIM_genotyping.genotype on the candidates of one case, type by type with the case's options -> the four fields of every candidate"""
    import genotype_walk_cases as W
    from svim_amd import SVIM_genotyping
    o = types.SimpleNamespace(**case.options)
    cands = [W.Candidate(*c) for c in w.candidates(case)]
    for typ in ("DEL", "INV", "INS", "DUP_INT"):
        some = [c for c in cands if c.type == typ]
        if some:
            SVIM_genotyping.genotype(some, bam, typ, o, engine=engine)
    return [c.fields() for c in cands]


def object_route_difference(w, g, bam, engine, family=None):
    """the first case whose object route differs from the golden, described, or None"""
    import genotype_walk_cases as W
    want = golden_by_id(g)
    for case in W.cases():
        if family is None or case.family == family:
            got = object_route(w, case, bam, engine)
            if got != want[case.id]:
                return "case %r: %r, the reference has %r" % (case.id, got, want[case.id])
    return None


def option_groups(w, g, family=None, types_kept=None, extra=True):
    """the candidates of the parity set grouped by the options of their cases -> [(options, [candidate], [the golden's fields])]; the group of the default
    options also gets a tandem duplication and a breakend row, which must come back untouched"""
    import genotype_walk_cases as W
    want = golden_by_id(g)
    groups = {}
    for case in W.cases():
        if family is not None and case.family != family:
            continue
        for cand, e in zip(w.candidates(case), want[case.id]):
            if types_kept is None or cand[0] in types_kept:
                o, cands, exp = groups.setdefault(W.option_key(case.options), (case.options, [], []))
                cands.append(cand)
                exp.append(e)
    key = W.option_key(W.DEFAULTS)
    if extra and types_kept is None and key in groups:
        for (typ, s, e), fields in zip(W.EXTRA_TABLE_ROWS, g["untouched"]):
            groups[key][1].append((typ, w.references[0], s, e, ["a_read"], 10, None))
            groups[key][2].append(fields)
    return list(groups.values())


def table_route_difference(w, g, name_ids, run, **kw):
    """run(options namespace, CandidateTable, sig_read_id) -> per-row fields in table order; the first row that differs from the golden, described, or None"""
    import genotype_walk_cases as W
    ids = dict(name_ids)
    for options, cands, exp in option_groups(w, g, **kw):
        t, rid, row_of = W.table_of(cands, w.references, lambda nm: ids.setdefault(nm, len(ids)))
        got = run(types.SimpleNamespace(**options), t, rid)
        if len(got) != len(cands):
            return "%d rows for %d candidates" % (len(got), len(cands))
        for k, e in enumerate(exp):
            if got[row_of[k]] != e:
                return "candidate %r with %r: %r, the reference has %r" % (cands[k][:4] + cands[k][5:6], options, got[row_of[k]], e)
    return None


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import genotype_walk_cases as W
    import helpers as H
    from oracle import oracle as om
    w = W.world()
    d = object_route_difference(w, H.load(GOLDEN), IndexHolder(W.RowsIndex(w)), om.Oracle())
    if d:
        print(d)
        return DIFFERENT
    return 0


if __name__ == "__main__":
    sys.exit(main())
