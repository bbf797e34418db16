"""GENOTYPE on the device against what the REFERENCE returned for the directed cases of tests/genotype_walk_cases.py (tests/golden/g_genotype_cases.json.gz; the
oracle is held to the same file by tests/test_genotype_cases.py, which also shows that the file notices every one-step change of the walk).

Object route: SVIM_genotyping.genotype over svx_set_alignment_index / k_end_prefmax / k_genotype, family by family, equal to the golden and to the oracle.
Resident route: the cases as ONE BAM file, collected by the device reader in batches of 150 records and of the default size and once by the host reader; the
resident alignment table column by column against AlignmentIndex, then svx_genotype_resident (k_geno_loci, the distinct member ids, k_genotype per class range,
k_geno_call) on class-grouped tables of all candidates - one per set of options, tandem duplication and breakend rows riding along - , on DEL rows only and on
INS rows only.  k_geno_call: the call family's gt codes and the bit patterns of support_fraction."""
import struct
import types

import numpy as np
import pytest

import genotype_cases as GC
import genotype_child as K
import genotype_walk_cases as W
from svim_amd import SVIM_genotyping, _abi, _lib, harness, records
from tests import helpers as H

pytestmark = pytest.mark.gpu

COLLECT_OPTS = dict(min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                    position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
                    del_ins_dup_max_distance=1.0, skip_consensus=True, symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False,
                    tandem_duplications_as_insertions=False, interspersed_duplications_as_insertions=False, sample="Sample", genome=None,
                    types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(cases as one file, golden, AlignmentFile of the SAM text, its AlignmentIndex, path of the same records as a BAM file)"""
    w = W.world()
    bam = records.AlignmentFile(text=w.sam_text())
    path = str(tmp_path_factory.mktemp("genotype_cases") / "cases.bam")
    records.write_bam(path, w.references, w.lengths, list(bam.fetch(until_eof=True)))
    return w, H.load(K.GOLDEN), bam, SVIM_genotyping.alignment_index(bam), path


@pytest.mark.parametrize("family", W.FAMILIES)
def test_object_route_against_the_reference_and_the_oracle(eng, oracle, world, family):
    w, g, bam, index, _ = world
    for e in (eng, oracle):                                  # (the engine is the process's: whatever index another module left on it goes)
        e.set_alignment_index(index)
        e._svx_index_id = id(index)
    d = K.object_route_difference(w, g, bam, eng, family=family)
    assert d is None, d
    for case in W.cases():
        if case.family == family:
            assert K.object_route(w, case, bam, eng) == K.object_route(w, case, bam, oracle), case.id


def test_contig_missing_from_the_file_gives_no_reference_reads(eng, world):
    """the reference raises there (tests/test_genotype_cases.py: test_refusals); the walk returns at once for a contig id of -1"""
    w, _, bam, index, _ = world
    eng.set_alignment_index(index)
    eng._svx_index_id = id(index)
    assert K.object_route(w, W.refused()[0], bam, eng) == [[1.0, "1/1", 0, 4]]


def _collect(eng, world, device_decode, batch_records):
    w, path = world[0], world[4]
    o = types.SimpleNamespace(**dict(COLLECT_OPTS, **W.DEFAULTS))
    kw = {} if batch_records is None else {"batch_records": batch_records}
    pipe = harness.BamPipeline(path, o, eng, threads=2, device_decode=device_decode, keep_alignments=True, **kw)
    try:
        assert pipe.run() == len(w.rows)
    except BaseException:
        pipe.close()
        raise
    return pipe


@pytest.mark.parametrize("reader, batch_records", [("device", 150), ("device", None), ("host", None)])
def test_cases_from_a_bam_file_on_the_resident_route(eng, world, reader, batch_records):
    w, g, _, index, _ = world
    pipe = _collect(eng, world, reader == "device", batch_records)
    try:
        if batch_records:
            assert pipe.stats["batches"] >= len(w.rows) // batch_records
        _, names = GC.check_table_against_index(eng, pipe, index)
        ids = {nm: k for k, nm in enumerate(names)}

        def run(o, t, rid):
            eng.genotype_resident(o, w.lengths, table=t, sig_read_id=rid)
            return GC.columns_as_fields(eng.fetch_genotypes())
        for kw in ({}, {"types_kept": ("DEL",)}, {"types_kept": ("INS",)}):          # the last two leave class ranges of the table empty
            d = K.table_route_difference(w, g, ids, run, **kw)
            assert d is None, (kw, d)
        assert eng.genotype_stats()["n_alignments"] == len(w.rows)
    finally:
        pipe.close()


def test_call_family_from_a_bam_file_through_k_geno_call(eng, world):
    """gt codes and support_fraction bit for bit (one FP64 division), -1 / NaN for a row that is not genotyped; and the refused minimum_depth <= 0 with no read on
    either side: the uncalled row of total 0, where the reference divides by zero"""
    w, g, _, _, _ = world
    pipe = _collect(eng, world, True, None)
    try:
        ids = {nm: k for k, nm in enumerate(pipe.bam.read_names())}
        groups = K.option_groups(w, g, family="call", extra=False)
        groups[0][1].extend((typ, w.references[0], s, e, ["a_read"], 10, None) for typ, s, e in W.EXTRA_TABLE_ROWS)
        groups[0][2].extend(g["untouched"])
        for case in W.refused()[1:]:
            groups.append((case.options, w.candidates(case), [[".", "./.", 0, 0]]))
        assert len(groups) >= 8 and sum(len(c) for _, c, _ in groups) == 22 + 2 + 2
        for options, cands, exp in groups:
            t, rid, row_of = W.table_of(cands, w.references, lambda nm: ids.setdefault(nm, len(ids)))
            eng.genotype_resident(types.SimpleNamespace(**options), w.lengths, table=t, sig_read_id=rid)
            got = eng.fetch_genotypes()
            for k, (f, gt, ref, alt) in enumerate(exp):
                r = row_of[k]
                what = (cands[k][:4], options)
                assert got["gt"][r] == _abi.GT_NAMES.index(gt), what
                assert (got["ref_reads"][r], got["alt_reads"][r]) == ((-1, -1) if ref is None else (ref, alt)), what
                bits = struct.pack("<d", float(got["support_fraction"][r]))
                assert np.isnan(got["support_fraction"][r]) if f == "." else bits == struct.pack("<d", f), what
    finally:
        pipe.close()
