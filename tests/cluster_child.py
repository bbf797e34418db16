"""What tests/test_cluster_cases.py (oracle, CPU) and tests/test_gpu_cluster_cases.py (device) share - the families of tests/golden/g_cluster_cases.json.gz as
SigTables, the genome arrays, the comparisons - and, run as a program, the child process of the mutant test: it compares the oracle library that SVX_ORACLE_LIB
names with the golden, family by family (partitions, clusters, pair distances).  Exit status 0: everything agrees; DIFFERENT: a difference, printed.  Anything else
(an exception ends Python with 1) is a failure of the child, not a verdict."""
import os
import struct
import sys

DIFFERENT = 3
GOLDEN = "g_cluster_cases.json.gz"


def bits(x):
    return struct.pack("<d", float(x)).hex()


def setup(rows):
    """rows -> (SigTable with the contig ids of helpers.REFS, contig ranks)"""
    import helpers as H
    from svim_amd import batch, convert
    tab, contigs, reads = convert.sigtable_from_objects([H.row_sig(r) for r in rows], convert.Interner(H.REFS))
    assert contigs.names == H.REFS
    return tab, batch.contig_ranks(H.REFS)


def genome_arrays():
    import helpers as H
    from svim_amd import convert
    return convert.genome_arrays(H.options({}).genome, H.REFS)


def params_of(options):
    import helpers as H
    from svim_amd import _abi
    return _abi.Params.from_options(H.options(options))


def partitions_by_type(tab, sidx, pid):
    """(sorted signature numbers, partition number of each) -> [[[row numbers]]] per type in the golden's order"""
    from svim_amd import _abi
    import cluster_cases as CC
    out = []
    for typ in CC.TYPES:
        got = {}
        for i, q in zip(sidx, pid):
            if tab.type[i] == _abi.TYPE_CODE[typ]:
                got.setdefault(int(q), []).append(int(i))
        out.append([got[k] for k in sorted(got)])
    return out


def partition_lists_by_type(tab, parts):
    """Engine.partitions() -> the same layout"""
    from svim_amd import _abi
    import cluster_cases as CC
    return [[q for q in parts if tab.type[q[0]] == _abi.TYPE_CODE[typ]] for typ in CC.TYPES]


def partitions_difference(fam, got):
    import cluster_cases as CC
    want = [p["partitions"] for p in fam["partitions"]]
    assert [p["type"] for p in fam["partitions"]] == list(CC.TYPES)
    for typ, g, w in zip(CC.TYPES, got, want):
        if g != w:
            k = next((k for k, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            return "family %r, %s: %d partitions, the reference has %d; the first that differs is number %d: %r != %r (%s)" % (
                fam["name"], typ, len(g), len(w), k, g[k] if k < len(g) else None, w[k] if k < len(w) else None, case_of(fam, (w[k] if k < len(w) else g[k])[0]))
    return None


def case_of(fam, row):
    return next(("case %r" % c["name"] for c in fam["cases"] if c["range"][0] <= row < c["range"][1]), "no case")


def clusters_difference(fam, ct):
    import helpers as H
    try:
        H.compare_cluster_rows(H.cluster_rows(ct, H.REFS), fam["clusters"])
    except AssertionError as e:
        return "family %r: %s" % (fam["name"], e)
    return None


def pairs_of(fam):
    return [(i, j) for c in fam["cases"] for i, j, _ in c["pairs"]]


def pairs_difference(fam, got_bits):
    k = 0
    for c in fam["cases"]:
        for i, j, want in c["pairs"]:
            if got_bits[k] != want:
                return "family %r, case %r, rows %d and %d (%r, %r): %s (%r) != the reference's %s (%r)" % (
                    fam["name"], c["name"], i, j, fam["signatures"][i][:4], fam["signatures"][j][:4], got_bits[k], struct.unpack("<d", bytes.fromhex(got_bits[k]))[0],
                    want, struct.unpack("<d", bytes.fromhex(want))[0])
            k += 1
    return None


def oracle_family_difference(oc, fam):
    """partitions, clusters and pair distances of one golden family through the oracle; the first difference, described, or None"""
    tab, rank = setup(fam["signatures"])
    p = params_of(fam["options"])
    sidx, pid = oc.form_partitions(tab, rank, fam["options"]["partition_max_distance"])
    d = partitions_difference(fam, partitions_by_type(tab, sidx, pid))
    if d:
        return d
    d = clusters_difference(fam, oc.cluster(p, rank, table=tab))
    if d:
        return d
    return pairs_difference(fam, [bits(oc.span_position_distance(tab, i, j, p)) for i, j in pairs_of(fam)])


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import helpers as H
    from oracle import oracle as om
    g = H.load(GOLDEN)
    oc = om.Oracle()
    oc.set_genome(*genome_arrays())
    for fam in g["families"]:
        d = oracle_family_difference(oc, fam)
        if d:
            print(d)
            return DIFFERENT
    return 0


if __name__ == "__main__":
    sys.exit(main())
