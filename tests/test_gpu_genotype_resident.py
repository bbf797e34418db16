"""GENOTYPE from resident tables on the device: the alignment table filled while COLLECT runs (svx_collect_keep_alignments, csrc/alnindex.hip) and
svx_genotype_resident (csrc/genotype.hip) against the reference's golden vectors, the object route (SVIM_genotyping.genotype over the HIP join and over the
C oracle) and records' own reference_end."""
import os
import random
import types

import numpy as np
import pytest

import genotype_cases as GC
from svim_amd import SVIM_COMBINE, SVIM_genotyping, _abi, _lib, convert, harness, records, synth
from svim_amd.lazy import SignatureList
from tests import helpers as H

pytestmark = pytest.mark.gpu

OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
            del_ins_dup_max_distance=1.0, skip_consensus=True, minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2,
            symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
            interspersed_duplications_as_insertions=False, sample="Sample", genome=None, types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")
TYPES = OPTS["types"].split(",")


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


def _options(**kw):
    return types.SimpleNamespace(**dict(OPTS, **kw))


def _rows_as_records(references, lengths, rows):
    return list(records.AlignmentFile(text=synth.genotype_sam_text(references, lengths, rows)).fetch(until_eof=True))


def _collect_file(eng, path, o, batch_records, device_decode=True, keep=True):
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=batch_records, device_decode=device_decode, keep_alignments=keep)
    n = pipe.run()
    return pipe, n


def test_golden_rows_from_a_bam_file_in_small_batches(eng, tmp_path):
    g = H.load("g_genotype.json.gz")
    recs = _rows_as_records(g["references"], g["lengths"], g["rows"])
    path = str(tmp_path / "golden.bam")
    records.write_bam(path, g["references"], g["lengths"], recs)
    o = _options(**{k: v for k, v in g["options"].items() if k in OPTS})
    pipe, n = _collect_file(eng, path, o, 150)
    try:
        assert n == len(recs) and pipe.stats["batches"] >= len(recs) // 150
        index = SVIM_genotyping.AlignmentIndex(records.AlignmentFile(text=synth.genotype_sam_text(g["references"], g["lengths"], g["rows"])))
        _, names = GC.check_table_against_index(eng, pipe, index)
        ids = {nm: k for k, nm in enumerate(names)}
        cands = GC.golden_candidates(g)
        t, rid, row_of = GC.table_from_candidates(cands, g["references"], lambda nm: ids.setdefault(nm, len(ids)))
        eng.genotype_resident(o, g["lengths"], table=t, sig_read_id=rid)
        got = GC.columns_as_fields(eng.fetch_genotypes())
        for k, e in enumerate(GC.golden_expected(g)):
            assert got[row_of[k]] == e, (cands[k][:4], got[row_of[k]], e)
        st = eng.genotype_stats()
        assert st["n_candidates"] == 280 and st["n_alignments"] == len(recs) and st["t_walk_ms"] > 0
    finally:
        pipe.close()


def _seeded_records():
    contigs = [("chr1", 120000), ("chrE", 30000), ("chr2", 50000)]                 # chrE: only the few split reads that land there
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 500, refs, references, lengths, n_sites=30, types=("DEL", "INS", "INV"))
    recs += synth.planted_reads(9, 120, refs, references, lengths, n_sites=8, types=("DEL", "INS"), tid=2)
    recs += synth.fuzz_split_reads(6, 80, references, lengths)                      # supplementary records, interspersed duplications, breakends
    # plain reads for the reference allele: piles deeper than the 500-alignment cap, piles within 1000 of both ends of a contig, secondary / unmapped-but-placed /
    # low-mapq records, second records of one read up to 3000 away
    rows = [r for r in synth.genotype_rows(31, lengths, n_reads=1800, hot=((0, 60000, 900), (2, 300, 300), (2, 49700, 300))) if r[2] != 1]
    recs += _rows_as_records(references, lengths, rows)
    z = records.AlignedSegment()                                                    # a record without reference span, inside a pile
    z.query_name, z.flag, z.reference_id, z.reference_start, z.mapping_quality = "zero_span", 0, 0, 60000, 60
    z.cigartuples, z.query_sequence = [(4, 30)], "A" * 30
    recs.append(z)
    return references, lengths, refs, synth.coordinate_sort(recs)


def _object_route(eng_join, table, sig, names, references, lengths, recs, o):
    """objects of the candidate table, genotyped by the existing SVIM_genotyping.genotype over `eng_join`'s interval join -> (six lists in write_final_vcf's
    argument order, per-row fields in table order)"""
    sigs = SignatureList(sig, references, names)
    dele, inv, int_dup, tan_dup, ins, bnd = [list(x) for x in convert.candidate_lists(table, sigs, references)]
    bam = records.AlignmentFile(text=synth.sam_text(references, lengths, recs))
    for lst, typ in ((dele, "DEL"), (inv, "INV"), (ins, "INS"), (int_dup, "DUP_INT")):
        SVIM_genotyping.genotype(lst, bam, typ, o, engine=eng_join)
    fields = [[c.support_fraction, c.genotype, c.ref_reads, c.alt_reads] for lst in (dele, inv, int_dup, tan_dup, ins, bnd) for c in lst]
    return (int_dup, inv, tan_dup, dele, ins, bnd), fields


def _body(path):
    return b"".join(l for l in open(path, "rb").read().splitlines(True) if not l.startswith(b"#"))


def test_file_to_vcf_on_the_resident_route_equals_the_object_route(eng, oracle, tmp_path):
    references, lengths, refs, recs = _seeded_records()
    path = str(tmp_path / "seeded.bam")
    records.write_bam(path, references, lengths, recs)
    o = _options()
    off, codes = convert.genome_arrays(refs, references)
    results = {}
    for label, device_decode, batch_records in (("device", True, 211), ("host", False, 389)):
        pipe, n = _collect_file(eng, path, o, batch_records, device_decode=device_decode)
        try:
            assert n == len(recs)
            pipe.cluster(genome=(off, codes))
            pipe.combine()
            pipe.genotype()
            out = str(tmp_path / ("variants_%s.vcf" % label))
            pipe.write_vcf(out)
            results[label] = dict(body=_body(out), g=eng.fetch_genotypes(), table=eng.fetch_candidates(), sig=eng.fetch_signatures(0), names=pipe.bam.read_names(),
                                  aln=eng.alignments())
        finally:
            pipe.close()
    dev = results["device"]
    table, g = dev["table"], dev["g"]
    cc = table.class_count
    assert min(cc[_abi.CAND_DEL], cc[_abi.CAND_INV], cc[_abi.CAND_INS]) > 3 and (table.score < o.minimum_score).any() and (table.score >= o.minimum_score).any()
    # the table kept every record; a supplementary record of a member read far downstream shares its read id with the primary
    assert dev["aln"]["tid"].size == len(recs) and (dev["aln"]["flag"] & 2048).any()
    first_at = {}
    far = 0
    for k, (r, p, t) in enumerate(zip(dev["aln"]["read_id"].tolist(), dev["aln"]["pos"].tolist(), dev["aln"]["tid"].tolist())):
        if r in first_at and k - first_at[r] > 211:
            far += 1
        first_at.setdefault(r, k)
    assert far > 0                                                                 # records of one read in different batches: the ids are handle-wide
    for label, join in (("hip join", eng), ("oracle", oracle)):
        lists6, fields = _object_route(join, table, dev["sig"], dev["names"], references, lengths, recs, o)
        assert GC.columns_as_fields(g) == fields, label
        want = "".join(l + "\n" for l in SVIM_COMBINE.vcf_body_python(*lists6, TYPES, o, False, None)).encode("utf-8")
        assert dev["body"] == want, label
    calls = set(g["gt"].tolist())
    assert calls >= {0, 1} and len(calls) >= 3 and int(g["ref_reads"].max()) >= 400      # a pile at the cap of 500 counted alignments
    # host-array batches give the same tables and the same text (read ids may be numbered differently: compare through the names)
    host = results["host"]
    assert host["body"] == dev["body"]
    for k in ("gt", "ref_reads", "alt_reads"):
        assert (host["g"][k] == g[k]).all()
    assert (host["g"]["support_fraction"].view(np.uint64) == g["support_fraction"].view(np.uint64)).all()      # bit-equal, NaN included
    for k in ("tid", "pos", "end", "flag", "mapq"):
        assert (host["aln"][k] == dev["aln"][k]).all(), k
    assert [host["names"][r] for r in host["aln"]["read_id"].tolist()] == [dev["names"][r] for r in dev["aln"]["read_id"].tolist()]
    # the resident route = the handed-in route on the same candidates (the alignment table of the last pass is still resident)
    eng.genotype_resident(o, lengths, table=host["table"], sig_read_id=host["sig"].read_id)
    g2 = eng.fetch_genotypes()
    for k in ("gt", "ref_reads", "alt_reads"):
        assert (g2[k] == host["g"][k]).all()
    assert (g2["support_fraction"].view(np.uint64) == host["g"]["support_fraction"].view(np.uint64)).all()


def test_reference_end_of_short_long_and_cg_tag_records(eng, tmp_path):
    short, long_rec, cig = H.long_cigar_records()
    rng = random.Random(12)
    recs = [short, long_rec]
    pos = 2000
    for n_ops in [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5000] + [rng.randint(1, 5000) for _ in range(40)]:
        a = records.AlignedSegment()
        ops, seq_len = [], 0
        for k in range(n_ops):
            op = rng.choice((0, 0, 1, 2, 3, 7, 8)) if 0 < k < n_ops - 1 else 0
            ln = rng.randint(1, 6)
            ops.append((op, ln))
            seq_len += ln if op in (0, 1, 7, 8) else 0
        a.query_name, a.flag, a.reference_id, a.reference_start, a.mapping_quality = "r%d_%d" % (n_ops, pos), rng.choice((0, 16, 2048)), 0, pos, 60
        a.cigartuples, a.query_sequence = ops, "A" * seq_len
        recs.append(a)
        pos += rng.randint(0, 50)
    recs = synth.coordinate_sort(recs)
    references, lengths = ["chr1"], [400000]
    path = str(tmp_path / "spans.bam")
    records.write_bam(path, references, lengths, recs)
    for device_decode in (True, False):
        pipe, n = _collect_file(eng, path, _options(), 17, device_decode=device_decode)
        try:
            a = eng.alignments()
            assert n == len(recs) and a["pos"].tolist() == [r.reference_start for r in recs]
            assert a["end"].tolist() == [r.reference_end for r in recs]
            st = eng.alignments_stats()
            n_long = sum(1 for r in recs if len(r.cigartuples) > 4096)
            assert n_long >= 4 and st["n_long_records"] == n_long and st["n_records"] == len(recs) and st["n_ops_read"] == sum(len(r.cigartuples) for r in recs)
        finally:
            pipe.close()
    assert len(cig) > 65535 and max(len(r.cigartuples) for r in recs) == len(cig)


def test_off_by_default_unsorted_files_and_genotypes_voided_by_combine(eng, tmp_path):
    references, lengths, refs, recs = _seeded_records()
    path = str(tmp_path / "seeded.bam")
    records.write_bam(path, references, lengths, recs)
    o = _options()
    off, codes = convert.genome_arrays(refs, references)
    vp = _abi.VcfParams.from_options(o, TYPES, False)
    # switch off: no table, svx_vcf source 0 prints ./. as before, genotyping is refused for want of a table
    pipe, _ = _collect_file(eng, path, o, 500, keep=False)
    try:
        assert eng.alignments()["tid"].size == 0
        pipe.cluster(genome=(off, codes))
        pipe.combine()
        with pytest.raises(_lib.SvxError, match="no resident alignment table"):
            eng.genotype_resident(o, lengths)
        with pytest.raises(ValueError):
            pipe.genotype()
        eng.vcf(vp, references)
        plain = eng.vcf_fetch()
        assert plain.count(b"\n") > 10 and all(l.rsplit(b"\t", 1)[1].startswith(b"./.:") and l.endswith(b":.:.,.") for l in plain.splitlines())
        with pytest.raises(_lib.SvxError, match="no resident genotypes"):
            eng.vcf(vp, references, resident_genotypes=True)
    finally:
        pipe.close()
    # switch on: the columns are printed only when asked for, and are void after a later combine
    pipe, _ = _collect_file(eng, path, o, 500)
    try:
        pipe.cluster(genome=(off, codes))
        pipe.combine()
        pipe.genotype()
        eng.vcf(vp, references)
        assert eng.vcf_fetch() == plain
        eng.vcf(vp, references, resident_genotypes=True)
        assert eng.vcf_fetch() != plain
        pipe.combine()
        with pytest.raises(_lib.SvxError, match="no resident genotypes"):
            eng.fetch_genotypes()
        with pytest.raises(_lib.SvxError, match="no resident genotypes"):
            eng.vcf(vp, references, resident_genotypes=True)
        pipe.genotype()
        assert eng.fetch_genotypes()["gt"].size == eng.fetch_candidates().n
    finally:
        pipe.close()
    with pytest.raises(ValueError):
        harness.BamPipeline(path, o, eng, mode="queryname", keep_alignments=True)
    # a file that is not coordinate-sorted: the stated error, and the context goes on working
    bad = str(tmp_path / "unsorted.bam")
    records.write_bam(bad, references, lengths, recs[200:400] + recs[:200] + recs[400:], sort_order="unsorted")
    pipe, _ = _collect_file(eng, bad, o, 300)
    try:
        pipe.cluster(genome=(off, codes))
        pipe.combine()
        with pytest.raises(_lib.SvxError, match="genotyping needs a coordinate-sorted alignment file"):
            pipe.genotype()
        assert eng.alignments()["tid"].size == len(recs)
        eng.vcf(vp, references)
        assert eng.vcf_fetch().count(b"\n") > 10
    finally:
        pipe.close()
