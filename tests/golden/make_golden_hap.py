#!/usr/bin/env python3
"""Generate tests/golden/g_hap_cases.json.gz by RUNNING THE REFERENCE's insertion distance and CLUSTER step on the directed haplotype cases of tests/hap_cases.py.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them).  The case genome is written to
a temporary FASTA and opened with the stub FastaFile.  For every pair of every family whose two contigs the genome holds: span_position_distance (the double's hex,
as in g6_distance.json.gz) and, where the reference took the near branch, compute_haplotype_edit_distance beside it (null on the far branch).  For every cluster
case: cluster_sv_signatures in the row layout of g5_cluster.json.gz.  What the reference raises is recorded by exception type under "raises" and must be exactly
what tests/hap_cases.py lists as expected.  The signature rows are NOT stored: tests/hap_cases.py regenerates them from its seeds and the file holds their digests.
DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hap.py
"""
import os
import struct
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG    # noqa: E402  (stubs pysam / edlib, puts the reference on the path)
import hap_cases as HC      # noqa: E402

SC = MG.SVIM_clustering


def write_fasta(path):
    with open(path, "w") as fh:
        for name in HC.REFERENCES:
            if name in HC.GENOME:
                fh.write(">%s\n" % name)
                s = HC.GENOME[name]
                for k in range(0, len(s), 60):
                    fh.write(s[k:k + 60] + "\n")


def main():
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "hap_cases.fa")
        write_fasta(fa)
        ref = MG.FastaFile(fa)
        assert ref.seqs == HC.GENOME
        fams, raises = [], {}
        for t in HC.families():
            sigs = [MG.row_sig(r) for r in t.rows]
            pairs, n_def = [], 0
            for i, j, tag, params in t.pairs:
                if sigs[i].contig not in HC.GENOME or sigs[j].contig not in HC.GENOME:
                    n_def += 1
                    continue                       # definition-only pairs: the stub FastaFile has no such contig
                dist = SC.span_position_distance(sigs[i], sigs[j], "INS", ref, *params)
                ed = SC.compute_haplotype_edit_distance(sigs[i], sigs[j], ref) if HC.needs_edit(HC.sig(t.rows[i]), HC.sig(t.rows[j]), params) else None
                pairs.append([i, j, tag, list(params), struct.pack("<d", float(dist)).hex(), ed])
            fams.append({"name": t.name, "digest": t.digest(), "n_rows": len(t.rows), "pairs": pairs, "n_definition_only": n_def})
            print(t.name, len(t.rows), "rows,", len(pairs), "pairs,", sum(1 for p in pairs if p[5] is not None), "with an edit distance,", n_def, "definition-only")
        zs = [MG.row_sig(r) for r in HC.ZERO_SPAN]
        try:
            SC.span_position_distance(zs[0], zs[1], "INS", ref, *HC.DEFAULT)
        except Exception as e:          # noqa: BLE001  (whatever the reference raises is the finding)
            raises["zero_span 0/1"] = type(e).__name__
        assert raises == HC.EXPECTED_RAISES, raises
        clusters = []
        for name, rows, opts in HC.cluster_cases():
            o = MG.options(genome=fa, **opts)
            sigs = [MG.row_sig(r) for r in rows]
            res = MG.SVIM_CLUSTER.cluster_sv_signatures(sigs, o)
            clusters.append({"name": name, "digest": HC.rows_digest(rows), "n_rows": len(rows), "options": dict(opts), "clusters": MG.cluster_rows(res, sigs)})
            print(name, len(rows), "rows,", [len(x) for x in res], "clusters")
    MG.dump("g_hap_cases.json.gz", {"families": fams, "cluster_cases": clusters, "raises": raises, "references": HC.REFERENCES,
                                    "lengths": [len(HC.GENOME.get(r, "")) for r in HC.REFERENCES],
                                    "source": "svim.SVIM_clustering.span_position_distance / compute_haplotype_edit_distance (src/svim/SVIM_clustering.py:32-77) and "
                                              "svim.SVIM_CLUSTER.cluster_sv_signatures on the directed haplotype cases of tests/hap_cases.py"})


if __name__ == "__main__":
    main()
