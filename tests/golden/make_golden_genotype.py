#!/usr/bin/env python3
"""Generate tests/golden/g_genotype_cases.json.gz by RUNNING THE REFERENCE's genotype() (src/svim/SVIM_genotyping.py:34-94) on the directed cases of
tests/genotype_walk_cases.py.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them).  All cases are ONE
coordinate-sorted file, read through svim_amd.records.AlignmentFile, whose fetch(contig, start, stop) answers with htslib's overlap rule; the candidates are the
reference's own classes (SVCandidate).  Every case runs with its own options; what the reference returns - ref_reads, alt_reads, genotype, support_fraction -
must be what the case's author wrote down, and a case on the wrong side of its threshold stops the generator with its name.  Stored: per case its id and the four
fields [support_fraction, genotype, ref_reads, alt_reads] of every candidate, the untouched fields of a tandem duplication and a breakend (genotype() is never
called for those classes, src/svim/svim:164-170), the exception type of every refused case, and the SHA-256 of the alignment rows and of the candidates, options
and expectations the file was computed from: the rows themselves are rebuilt by code.  DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_genotype.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG              # noqa: E402  (stubs pysam / edlib, puts the reference on the path)
import genotype_walk_cases as W       # noqa: E402
from svim import SVIM_genotyping, SVCandidate, SVSignature      # noqa: E402


def reference_candidate(typ, contig, start, end, members, score, source):
    sigs = [SVSignature.SignatureDeletion(contig, start, end, "cigar", m) for m in members]
    if typ == "DEL":
        return SVCandidate.CandidateDeletion(contig, start, end, sigs, score, 1.0, 1.0)
    if typ == "INV":
        return SVCandidate.CandidateInversion(contig, start, end, sigs, score, 1.0, 1.0)
    if typ == "INS":
        return SVCandidate.CandidateNovelInsertion(contig, start, end, "", sigs, score, 1.0, 1.0)
    if typ == "DUP_INT":
        return SVCandidate.CandidateDuplicationInterspersed(source[0], source[1], source[2], contig, start, end, sigs, score, 1.0, 1.0)
    if typ == "DUP_TAN":
        return SVCandidate.CandidateDuplicationTandem(contig, start, end, 1, True, sigs, score, 1.0, 1.0)
    assert typ == "BND"
    return SVCandidate.CandidateBreakend(contig, start, "fwd", contig, end, "fwd", sigs, score, 1.0, 1.0)


def fields(c):
    return [c.support_fraction, c.genotype, c.ref_reads, c.alt_reads]


def run(w, bam, case):
    o = types.SimpleNamespace(**case.options)
    out = []
    for cand in w.candidates(case):
        c = reference_candidate(*cand)
        SVIM_genotyping.genotype([c], bam, cand[0], o)
        out.append(fields(c))
    return out


def main():
    w = W.world()
    bam = MG.records.AlignmentFile(text=w.sam_text())
    assert bam.references == w.references and bam.lengths == w.lengths
    out = []
    for case in W.cases():
        got = run(w, bam, case)
        want = [W.expected_fields(e) for e in case.expected]
        assert got == want, "%s: the reference gives %r, the case says %r" % (case.id, got, want)
        for cand in w.candidates(case):                       # stays out of the set altogether: there the stand-in's fetch, not htslib, would answer
            assert cand[2] - 1000 < w.lengths[w.references.index(cand[1])], case.id
        out.append({"id": case.id, "expected": got})
    raises = {}
    for case in W.refused():
        try:
            run(w, bam, case)
        except Exception as e:          # noqa: BLE001  (whatever the reference raises is the finding)
            raises[case.id] = type(e).__name__
    assert raises == W.EXPECTED_RAISES, raises
    extra = [fields(reference_candidate(typ, w.references[0], s, e, ["a_read"], 10, None)) for typ, s, e in W.EXTRA_TABLE_ROWS]
    assert extra == [W.UNTOUCHED] * len(extra)
    print(len(out), "cases,", sum(len(c["expected"]) for c in out), "candidates,", len(w.rows), "rows on", len(w.references), "contigs; refused:", raises)
    MG.dump("g_genotype_cases.json.gz", {"cases": out, "raises": raises, "untouched": extra, "rows_sha256": w.rows_sha256(), "cases_sha256": w.cases_sha256(),
                                         "n_rows": len(w.rows), "n_contigs": len(w.references),
                                         "source": "svim.SVIM_genotyping.genotype (src/svim/SVIM_genotyping.py:34-94; reads via svim_amd.records.AlignmentFile.fetch: "
                                                   "htslib overlap rule) on the directed cases of tests/genotype_walk_cases.py"})


if __name__ == "__main__":
    main()
