"""The alignment table in any record order, on the CPU: SVIM_genotyping.AlignmentIndex(order="sort") is the index of the records in bamsort.py's coordinate
order, genotype(alignment_order="sort") is genotype() over the sorted file, and the cases the device is held against discriminate."""
import types

import numpy as np
import pytest

import aln_order_cases as AC
import genotype_cases as GC
from svim_amd import SVIM_genotyping, _abi, _lib, bamsort
from tests import helpers as H

COLUMNS = ("contig_first", "contig_len", "pos", "end", "flag", "mapq", "name_id")


def _same_index(a, b):
    assert (a.n, a.n_contig, a.references, a.lengths) == (b.n, b.n_contig, b.references, b.lengths)
    for col in COLUMNS:
        assert (getattr(a, col) == getattr(b, col)).all(), col
    assert a.name_ids == b.name_ids


def _options(g=None, **kw):
    base = dict(minimum_score=3, min_mapq=20, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2)
    if g is not None:
        base.update(g["options"])
    return types.SimpleNamespace(**dict(base, **kw))


CASES = [(n, "random") for n in AC.SIZES if n <= 16385] + [(3000, k) for k in AC.KINDS] + [(150500, "random")]


@pytest.mark.parametrize("n,kind", CASES)
def test_sorted_index_is_the_index_of_the_sorted_records(n, kind):
    r = AC.rows(n, kind)
    perm = AC.definition_permutation(r["tid"], r["pos"], r["flag"])
    got = SVIM_genotyping.AlignmentIndex(AC.RowFile(r), order="sort")
    want = SVIM_genotyping.AlignmentIndex(AC.RowFile(r, order=perm.tolist()))          # order="file": raises if bamsort's order were not coordinate order
    _same_index(got, want)
    placed = r["tid"][perm] >= 0
    assert (got.src_row == perm[placed]).all() and (placed[:int(placed.sum())]).all()      # unplaced rows sort last
    if kind == "sorted":
        _same_index(got, SVIM_genotyping.AlignmentIndex(AC.RowFile(r)))
        assert (perm == np.arange(n)).all()
    elif n > 2 and kind != "one_key":
        with pytest.raises(ValueError, match="coordinate-sorted"):
            SVIM_genotyping.AlignmentIndex(AC.RowFile(r))
    if kind == "one_key":
        assert (perm == np.arange(n)).all() and np.unique(r["flag"]).size > 1            # equal keys: append order


def test_sorted_index_of_a_bam_file_is_the_index_of_sort_records(tmp_path):
    """through real BAM bytes: bamsort.sort_records over the file's record stream"""
    from svim_amd import records
    g = H.load("g_genotype.json.gz")
    rws = AC.shuffled(g["rows"], 3)[:700] + [["unplaced", 4, 0, 0, 0, 10]]
    recs = list(AC.text_file(g["references"], g["lengths"], rws).fetch(until_eof=True))
    recs[-1].reference_id, recs[-1].reference_start = -1, -1
    path = str(tmp_path / "unsorted.bam")
    records.write_bam(path, g["references"], g["lengths"], recs, sort_order="unsorted")
    raw = bamsort.inflate(path)
    _, n_ref, first = bamsort.split_header(raw)
    _, perm = bamsort.sort_records(raw[first:], n_ref)
    by_file = list(records.AlignmentFile(path).fetch(until_eof=True))

    class Sorted(object):
        references, lengths = g["references"], g["lengths"]

        def fetch(self, until_eof=True):
            return iter([by_file[k] for k in perm])
    got = SVIM_genotyping.AlignmentIndex(records.AlignmentFile(path), order="sort")
    _same_index(got, SVIM_genotyping.AlignmentIndex(Sorted()))
    assert got.src_row.tolist() == perm[:-1] and perm[-1] == len(recs) - 1


def test_order_keyword_is_checked_and_file_is_the_default():
    r = AC.rows(50, "reversed")
    with pytest.raises(ValueError, match="order"):
        SVIM_genotyping.AlignmentIndex(AC.RowFile(r), order="name")
    with pytest.raises(ValueError, match="genotyping needs a coordinate-sorted alignment file"):
        SVIM_genotyping.alignment_index(AC.RowFile(r))
    f = AC.RowFile(r)
    assert SVIM_genotyping.alignment_index(f, order="sort") is SVIM_genotyping.alignment_index(f, "sort")


@pytest.mark.parametrize("seed", AC.SHUFFLE_SEEDS)
def test_shuffled_golden_rows_give_the_reference_results(oracle, seed):
    g = H.load("g_genotype.json.gz")
    index = SVIM_genotyping.AlignmentIndex(AC.text_file(g["references"], g["lengths"], AC.shuffled(g["rows"], seed)), order="sort")
    ids = dict(index.name_ids)
    cands = GC.golden_candidates(g)
    t, rid, row_of = GC.table_from_candidates(cands, g["references"], lambda name: ids.setdefault(name, len(ids)))
    oracle.set_alignment_index(index)
    got = GC.table_route_python(t, rid, oracle, _options(g))
    exp = GC.golden_expected(g)
    assert len(exp) == 280
    for k, e in enumerate(exp):
        assert got[row_of[k]] == e, (cands[k][:4], got[row_of[k]], e)


def _genotype_one(oracle, bam, cand, o, order):
    c = GC.Candidate(cand[0], cand[1], cand[2], cand[3], cand[4], cand[5])
    oracle._svx_index_id = None
    SVIM_genotyping.genotype([c], bam, cand[0], o, engine=oracle, alignment_order=order)
    return c


def test_tie_pile_tells_the_tie_rule(oracle):
    references, lengths, rws, cand = AC.tie_pile()
    o = _options()
    # the append order is (tid, pos)-sorted, so the default accepts it and walks B as the 500th alignment
    assert _genotype_one(oracle, AC.text_file(references, lengths, rws), cand, o, "file").ref_reads == 1
    assert _genotype_one(oracle, AC.text_file(references, lengths, rws), cand, o, "sort").ref_reads == 0
    for seed in (0, 1):                                      # any other append order of the rest: the three at 49600 keep B, A, C among themselves
        sh = AC.shuffled([r for r in rws if r[0] not in "BAC"], seed)
        sh[100:100] = [r for r in rws if r[0] in "BAC"]
        assert [r[0] for r in sh if r[0] in "BAC"] == ["B", "A", "C"]
        assert _genotype_one(oracle, AC.text_file(references, lengths, sh), cand, o, "sort").ref_reads == 0


@pytest.mark.parametrize("min_mapq", (20, 10))
def test_flag_groups_count_as_on_the_sorted_file(oracle, min_mapq):
    references, lengths, rws, cand, expected = AC.flag_groups()
    o = _options(min_mapq=min_mapq)
    perm = AC.definition_permutation([r[2] for r in rws], [r[3] for r in rws], [r[1] for r in rws])
    on_sorted = _genotype_one(oracle, AC.text_file(references, lengths, [rws[k] for k in perm], "coordinate"), cand, o, "file")
    got = _genotype_one(oracle, AC.text_file(references, lengths, rws, "queryname"), cand, o, "sort")
    assert got.fields() == on_sorted.fields() and got.ref_reads == expected[min_mapq]


def test_library_exports_the_any_order_entry_points():
    import ctypes
    L = _lib.lib()
    for name in ("svx_collect_keep_alignments_mode", "svx_alignments_permutation", "svx_alignments_get_sort_stats"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert ctypes.sizeof(_abi.AlignmentSortStats) == 40 and ctypes.sizeof(_abi.AlignmentsStats) == 48
    assert (_abi.SVX_ALN_SORT, _abi.SVX_ALN_FILE_FLAGS) == (1, 2)


def test_pipeline_keywords_keep_the_refusals():
    from svim_amd import harness
    o = _options()
    with pytest.raises(ValueError, match="keep_alignments needs the whole coordinate-sorted file"):
        harness.BamPipeline("nowhere.bam", o, None, mode="queryname", keep_alignments=True)
    with pytest.raises(ValueError, match="alignment_order"):
        harness.BamPipeline("nowhere.bam", o, None, keep_alignments=True, alignment_order="name")
    with pytest.raises(ValueError, match="keep_alignments needs the whole coordinate-sorted file"):      # contig shards stay refused
        harness.BamPipeline("nowhere.bam", o, None, keep_alignments=True, alignment_order="sort", regions=[(0, 1)])
