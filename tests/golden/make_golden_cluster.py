#!/usr/bin/env python3
"""Generate tests/golden/g_cluster_cases.json.gz by RUNNING THE REFERENCE's form_partitions, span_position_distance and CLUSTER step on the directed cases of
tests/cluster_cases.py.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them; the genome of the insertion
cases is tests/golden/ref.fa.gz).  Every case runs ALONE first: what the reference returns for it - partitions, member lists, clusters per type - must be what the
case's author wrote down, and a case on the wrong side of its threshold stops the generator.  Then every family runs as one table; in a family whose cases are
independent, the clusters of the table restricted to a case are the clusters of the case alone.  Stored per family: the signature rows, the options and the
clusters in the layout of g5_cluster.json.gz, the partitions per type in the layout of g4_partitions.json.gz, and per case its row range and a list of pairs with
span_position_distance's result as the double's hex (as in g6_distance.json.gz).  What the reference raises is recorded by exception type under "raises" and must
be exactly what tests/cluster_cases.py lists as expected.  DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cluster.py
"""
import os
import struct
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG      # noqa: E402  (stubs pysam / edlib, puts the reference on the path)
import cluster_cases as CC    # noqa: E402

SC = MG.SVIM_clustering


def partitions_of(sigs, max_distance):
    """[(type, [[row numbers]])] in the order cluster_sv_signatures goes through the types"""
    idx = {id(s): i for i, s in enumerate(sigs)}
    out = []
    for typ in CC.TYPES:
        sub = [s for s in sigs if s.type == typ]
        out.append((typ, [[idx[id(s)] for s in q] for q in SC.form_partitions(sub, max_distance)]))
    return out


def run(rows, opts):
    o = MG.options(**opts)
    sigs = [MG.row_sig(r) for r in rows]
    assert [MG.sig_row(s) for s in sigs] == rows, "a row the constructor changes"
    parts = partitions_of(sigs, o.partition_max_distance)
    clusters = MG.cluster_rows(MG.SVIM_CLUSTER.cluster_sv_signatures(sigs, o), sigs)
    return sigs, parts, clusters


def members(clusters):
    return sorted(sorted(c[7] if k < 3 else c[10]) for k, lst in enumerate(clusters) for c in lst)


def shifted(clusters, by):
    out = []
    for k, lst in enumerate(clusters):
        rows = []
        for c in lst:
            c = list(c)
            m = 7 if k < 3 else 10
            c[m] = [i + by for i in c[m]]
            rows.append(c)
        out.append(rows)
    return out


SLOT_TYPE = ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")          # the reference's return tuple


def main():
    ref = MG.FastaFile(os.path.join(HERE, "ref.fa.gz"))
    assert len(ref.seqs["chr1"]) == CC.CHR1_LEN and sorted(ref.seqs) == sorted(CC.REFS)
    fams, n_cases = [], 0
    for f in CC.families():
        o = MG.options(**f.options)
        alone = []
        for c in f.cases:
            sigs, parts, clusters = run(c.rows, f.options)
            flat = [q for _, lst in parts for q in lst]
            assert c.parts is None or flat == c.parts, "%s / %s: the reference's partitions are %r, the case says %r" % (f.name, c.name, flat, c.parts)
            assert c.clusters is None or members(clusters) == c.clusters, "%s / %s: the reference's clusters are %r, the case says %r" % (f.name, c.name, members(clusters), c.clusters)
            got = {SLOT_TYPE[k]: len(lst) for k, lst in enumerate(clusters) if lst}
            assert c.counts is None or got == c.counts, "%s / %s: the reference has %r clusters, the case says %r" % (f.name, c.name, got, c.counts)
            pairs = []
            for i, j in c.pairs:
                d = SC.span_position_distance(sigs[i], sigs[j], sigs[i].type, ref, o.position_distance_normalizer, o.edit_distance_normalizer, o.cluster_max_distance)
                pairs.append([i, j, struct.pack("<d", float(d)).hex()])
            alone.append((clusters, pairs))
            n_cases += 1
        rows = f.rows()
        sigs, parts, clusters = run(rows, f.options)
        cases = []
        for c, (lo, hi), (cl, pairs) in zip(f.cases, f.ranges(), alone):
            assert rows[lo:hi] == c.rows
            if f.independent:
                for k, lst in enumerate(shifted(cl, lo)):
                    inside = [x for x in clusters[k] if lo <= (x[7] if k < 3 else x[10])[0] < hi]
                    assert inside == lst, "%s / %s: not independent of the rest of its family" % (f.name, c.name)
            cases.append({"name": c.name, "range": [lo, hi], "pairs": [[i + lo, j + lo, h] for i, j, h in pairs]})
        fams.append({"name": f.name, "options": MG.opt_dict(o), "independent": f.independent, "signatures": rows, "clusters": clusters,
                     "partitions": [{"type": t, "partitions": p} for t, p in parts], "cases": cases})
        print(f.name, len(f.cases), "cases,", len(rows), "rows,", [len(x) for x in clusters], "clusters,", sum(len(c["pairs"]) for c in cases), "pairs")
    raises = {}
    for name, opts, rows in CC.REFUSED:
        try:
            run(rows, opts)
        except Exception as e:          # noqa: BLE001  (whatever the reference raises is the finding)
            raises[name] = type(e).__name__
    assert raises == CC.EXPECTED_RAISES, raises
    print(n_cases, "cases;", "refused:", raises)
    MG.dump("g_cluster_cases.json.gz", {"families": fams, "raises": raises, "references": CC.REFS, "lengths": [len(ref.seqs[r]) for r in CC.REFS],
                                        "source": "svim.SVIM_clustering.form_partitions / span_position_distance (src/svim/SVIM_clustering.py:17-29, :47-96) and "
                                                  "svim.SVIM_CLUSTER.cluster_sv_signatures on the directed cases of tests/cluster_cases.py"})


if __name__ == "__main__":
    main()
