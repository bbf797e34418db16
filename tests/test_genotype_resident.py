"""GENOTYPE from tables (svx_genotype_resident): the route's Python statement - locus per class, score filter, distinct member reads, the call from two counts -
over the C oracle's interval join, against what the reference's genotype() wrote (tests/golden/g_genotype.json.gz)."""
import types

import numpy as np

import genotype_cases as GC
from svim_amd import SVIM_genotyping, _abi, _lib, records, synth
from tests import helpers as H


def test_table_route_reproduces_the_reference_for_all_four_types(oracle):
    g = H.load("g_genotype.json.gz")
    bam = records.AlignmentFile(text=synth.genotype_sam_text(g["references"], g["lengths"], g["rows"]))
    index = SVIM_genotyping.AlignmentIndex(bam)
    ids = dict(index.name_ids)
    cands = GC.golden_candidates(g)
    t, rid, row_of = GC.table_from_candidates(cands, g["references"], lambda name: ids.setdefault(name, len(ids)))
    assert sorted(set(c[0] for c in cands)) == ["DEL", "DUP_INT", "INS", "INV"] and t.class_count == [70, 70, 70, 0, 70, 0]
    oracle.set_alignment_index(index)
    o = types.SimpleNamespace(**g["options"])
    got = GC.table_route_python(t, rid, oracle, o)
    exp = GC.golden_expected(g)
    assert any(e[1] == "./." and e[2] is None for e in exp) and {e[1] for e in exp} >= {"0/0", "0/1", "1/1"}      # low-score rows and every call are in there
    for k, e in enumerate(exp):
        assert got[row_of[k]] == e, (cands[k][:4], got[row_of[k]], e)


def test_rows_of_other_classes_and_low_scores_are_not_selected():
    t = _abi.CandidateTable(4, 0)
    t.cls[:] = [_abi.CAND_DEL, _abi.CAND_DUP_TAN, _abi.CAND_INS, _abi.CAND_BND]
    t.contig[:], t.start[:], t.end[:] = [1, 1, -1, 0], [10, 20, 0, 5], [90, 80, 0, 5]
    t.contig2[:], t.start2[:], t.end2[:] = [-1, -1, 2, 1], [0, 0, 300, 7], [0, 0, 340, 7]
    t.score[:] = [2.999, 50, np.nan, 50]
    sel, mode, tid, start, end = SVIM_genotyping.candidate_loci(t, 3)
    assert sel.tolist() == [False, False, True, False]                 # "not score < minimum_score": a NaN score is genotyped, as in the reference
    assert (tid.tolist(), start.tolist(), end.tolist(), int(mode[2])) == ([-1, -1, 2, -1], [0, 0, 300, 0], [0, 0, 300, 0], 1)
    sel, _, tid, start, end = SVIM_genotyping.candidate_loci(t, 2.999)
    assert sel.tolist() == [True, False, True, False] and (tid[0], start[0], end[0]) == (1, 10, 90)


def test_the_call_at_its_thresholds():
    o = types.SimpleNamespace(minimum_depth=5, homozygous_threshold=0.8, heterozygous_threshold=0.2)
    call = lambda alt, ref: SVIM_genotyping.genotype_calls(alt, ref, o)      # noqa: E731
    assert call(4, 1) == (_abi.VCF_GT["1/1"], 4 / 5)                  # 4/5 at 0.8: >= is homozygous
    assert call(1, 4) == (_abi.VCF_GT["0/1"], 1 / 5)                  # 1/5 at 0.2: >= is heterozygous
    assert call(0, 5) == (_abi.VCF_GT["0/0"], 0.0)
    assert call(3, 2) == (_abi.VCF_GT["0/1"], 0.6)                    # minimum_depth reached ...
    assert call(3, 1) == (_abi.VCF_GT["./."], 0.75)                   # ... and missed by one: the fraction is kept, the call is not made
    assert call(0, 0) == (_abi.VCF_GT["./."], ".")
    assert _abi.GT_NAMES == tuple(sorted(_abi.VCF_GT, key=_abi.VCF_GT.get))


def test_library_exports_the_resident_genotype_entry_points():
    L = _lib.lib()
    for name in ("svx_collect_keep_alignments", "svx_alignments_count", "svx_alignments_fetch", "svx_alignments_get_stats", "svx_genotype_resident",
                 "svx_genotype_count", "svx_genotype_fetch", "svx_genotype_get_stats", "svx_vcf_use_resident_genotypes"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    import ctypes
    assert ctypes.sizeof(_abi.GenotypeParams) == 32 and ctypes.sizeof(_abi.GenotypeStats) == 64 and ctypes.sizeof(_abi.AlignmentsStats) == 48


def test_candidate_views_carry_the_columns():
    from svim_amd import convert
    from svim_amd.lazy import CandidateList
    t, _, _ = GC.table_from_candidates([("DEL", "chr1", 10, 90, [], 5), ("DEL", "chr1", 200, 300, [], 1), ("INS", "chr2", 50, 90, [], 7)], ["chr1", "chr2"], lambda n: 0)
    t.genotypes = dict(gt=np.array([3, 0, 0], np.uint8), ref_reads=np.array([1, -1, 0], np.int32), alt_reads=np.array([4, -1, 0], np.int32),
                       support_fraction=np.array([0.8, np.nan, np.nan]))
    dele, _, _, _, ins, _ = convert.candidate_lists(t, [], ["chr1", "chr2"])
    assert isinstance(dele, CandidateList)
    fields = lambda c: [c.support_fraction, c.genotype, c.ref_reads, c.alt_reads]      # noqa: E731
    assert [fields(c) for c in dele] == [[0.8, "1/1", 1, 4], [".", "./.", None, None]] and fields(ins[0]) == [".", "./.", 0, 0]
