"""The alignment table in any record order, on the device (svx_collect_keep_alignments_mode, csrc/alnindex.hip): after its finalisation the table is
SVIM_genotyping.AlignmentIndex(order="sort") and its permutation bamsort.py's, at the sort's edges and through the three batchers; the genotype columns are
the reference's on the golden's rows in any order; query-name files are counted by the records' own flags; sorted input and the defaults are untouched."""
import types

import numpy as np
import pytest

import aln_order_cases as AC
import genotype_cases as GC
from svim_amd import SVIM_COMBINE, SVIM_genotyping, _abi, _lib, batch, convert, harness, records, synth
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


# ---- rows handed over as record batches (the Python batcher's form) -----------------------------------------------------------------------------------
def _feed(eng, r, cuts, order="sort", fresh=True, base=0):
    """rows [cuts[k], cuts[k + 1]) as one collect() each, appended to the resident table"""
    p = _abi.Params.from_options(_options())
    eng.keep_alignments(True, order=order)
    if fresh:
        eng.accumulate(True)
    try:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.set_slot_base(base)
            eng.collect(AC.rows_batch(r, lo, hi), p, fetch=False)
            base += 2 * (hi - lo) + 2
    finally:
        eng.keep_alignments(False, order=order)
    return base


def _finalise(eng, r, min_mapq=20):
    """the table is finalised when it is first used: one candidate nobody looks at"""
    t, rid, _ = GC.table_from_candidates([("DEL", r["references"][0], 10, 90, ["r0"], 5)], r["references"], lambda nm: 0)
    eng.genotype_resident(_options(min_mapq=min_mapq), r["lengths"], table=t, sig_read_id=rid)


def _check_rows(eng, r, n=None):
    """the resident table = the rows in the definition's order, its permutation the definition's, its placed part AlignmentIndex(order="sort")"""
    n = len(r["tid"]) if n is None else n
    r = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    perm = AC.definition_permutation(r["tid"], r["pos"], r["flag"])
    a, got_perm = eng.alignments(), eng.alignments_permutation()
    assert a["tid"].size == n and got_perm.dtype == np.uint32 and (got_perm == perm).all()
    for col in ("tid", "pos", "flag", "mapq", "read_id"):
        assert (a[col] == r[col][perm]).all(), col
    counts = (r["tid"] >= 0) & ((r["flag"] & (4 | 256)) == 0)
    assert (a["end"] == (r["pos"] + np.where(counts, r["span"], 0))[perm]).all()
    index = SVIM_genotyping.AlignmentIndex(AC.RowFile(r), order="sort")
    keep = np.flatnonzero(a["tid"] >= 0)
    assert keep.size == index.n and (keep == np.arange(keep.size)).all() and (got_perm[:index.n] == index.src_row).all()
    for col, exp in (("pos", index.pos), ("flag", index.flag), ("mapq", index.mapq)):
        assert (a[col][keep] == exp).all(), col
    assert (np.searchsorted(a["tid"][keep], np.arange(index.n_contig + 1)) == index.contig_first).all()
    by_id = {v: k for k, v in index.name_ids.items()}
    assert ["r%d" % i for i in a["read_id"][keep].tolist()] == [by_id[i] for i in index.name_id.tolist()]
    return a, got_perm


ROW_CASES = [(n, "random") for n in AC.SIZES] + [(3000, k) for k in AC.KINDS] + [(20000, k) for k in ("one_key", "reversed", "contigs300", "unplaced")]


@pytest.mark.parametrize("n,kind", ROW_CASES)
def test_rows_in_any_order_become_the_sorted_index(eng, n, kind):
    r = AC.rows(n, kind)
    try:
        _feed(eng, r, [0, n // 3, n] if n > 2 else [0, n])
        with pytest.raises(_lib.SvxError, match="has not been finalised"):
            eng.alignments_permutation()
        _finalise(eng, r)
        _, perm = _check_rows(eng, r)
        st, gs = eng.alignment_sort_stats(), eng.genotype_stats()
        moved = bool((perm != np.arange(n)).any())
        assert st["n_rows"] == n and st["sorted"] == int(moved) and gs["n_alignments"] == n and gs["t_tables_ms"] > 0
        if n:
            assert st["key_bits"] == 33 + {1: 1, 3: 2, 300: 9}[len(r["references"])]
        if moved:
            assert st["t_key_ms"] > 0 and st["t_sort_ms"] > 0 and st["t_gather_ms"] > 0
        else:
            assert kind in ("sorted", "one_key") or n <= 2
    finally:
        eng.accumulate(False)


def test_sorted_rows_are_left_alone_and_equal_the_default_mode(eng):
    r = AC.rows(5000, "sorted")
    try:
        _feed(eng, r, [0, 1700, 5000], order="file")
        _finalise(eng, r)
        default = eng.alignments()
        assert eng.alignment_sort_stats()["sorted"] == 0 and (eng.alignments_permutation() == np.arange(5000)).all()
        _feed(eng, r, [0, 1700, 5000], order="sort")
        _finalise(eng, r)
        st = eng.alignment_sort_stats()
        assert (st["sorted"], st["n_rows"], st["t_sort_ms"], st["t_gather_ms"]) == (0, 5000, 0.0, 0.0)
        a = eng.alignments()
        for k in default:
            assert a[k].tobytes() == default[k].tobytes(), k
        assert (eng.alignments_permutation() == np.arange(5000)).all()
    finally:
        eng.accumulate(False)


def test_append_genotype_append_genotype_equals_one_append(eng):
    r = AC.rows(40000, "random", seed=5)
    try:
        base = _feed(eng, r, [0, 9000, 23000])
        _finalise(eng, r)
        _check_rows(eng, r, n=23000)
        _feed(eng, r, [23000, 40000], fresh=False, base=base)
        with pytest.raises(_lib.SvxError, match="has not been finalised"):
            eng.alignments_permutation()
        _finalise(eng, r)
        two, perm_two = _check_rows(eng, r)                    # (the permutation is in append order: it is the definition's over all 40 000 rows)
        assert eng.alignment_sort_stats()["sorted"] == 1
        _feed(eng, r, [0, 40000])
        _finalise(eng, r)
        one = eng.alignments()
        for k in one:
            assert one[k].tobytes() == two[k].tobytes(), k
        assert (eng.alignments_permutation() == perm_two).all()
    finally:
        eng.accumulate(False)


def test_defaults_refuse_unsorted_rows_and_fetch_in_file_order(eng):
    r = AC.rows(3000, "reversed")
    try:
        _feed(eng, r, [0, 1000, 3000], order="file")
        with pytest.raises(_lib.SvxError, match="genotyping needs a coordinate-sorted alignment file"):
            _finalise(eng, r)
        a = eng.alignments()
        for col in ("tid", "pos", "flag", "mapq", "read_id"):
            assert (a[col] == r[col]).all(), col
        assert eng.alignment_sort_stats()["sorted"] == 0
        with pytest.raises(ValueError):
            harness.BamPipeline("nowhere.bam", _options(), eng, mode="queryname", keep_alignments=True)
        with pytest.raises(ValueError, match="order"):
            eng.keep_alignments(True, order="name")
    finally:
        eng.accumulate(False)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------------------
def _pipe(eng, path, o, batch_records, **kw):
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=batch_records, keep_alignments=True, alignment_order="sort", **kw)
    return pipe, pipe.run()


@pytest.mark.parametrize("seed", AC.SHUFFLE_SEEDS)
def test_shuffled_golden_bam_gives_the_reference_results(eng, tmp_path, seed):
    g = H.load("g_genotype.json.gz")
    rws = AC.shuffled(g["rows"], seed)
    recs = list(AC.text_file(g["references"], g["lengths"], rws).fetch(until_eof=True))
    path = str(tmp_path / "shuffled.bam")
    records.write_bam(path, g["references"], g["lengths"], recs, sort_order="unsorted")
    o = _options(**{k: v for k, v in g["options"].items() if k in OPTS})
    pipe, n = _pipe(eng, path, o, 150, device_decode=seed % 2 == 0)       # the device reader and the host reader take turns
    try:
        assert n == len(recs)
        names = pipe.bam.read_names()
        ids = {nm: k for k, nm in enumerate(names)}
        cands = GC.golden_candidates(g)
        t, rid, row_of = GC.table_from_candidates(cands, g["references"], lambda nm: ids.setdefault(nm, len(ids)))
        eng.genotype_resident(o, g["lengths"], table=t, sig_read_id=rid)
        got = GC.columns_as_fields(eng.fetch_genotypes())
        for k, e in enumerate(GC.golden_expected(g)):
            assert got[row_of[k]] == e, (cands[k][:4], got[row_of[k]], e)
        index = SVIM_genotyping.AlignmentIndex(AC.text_file(g["references"], g["lengths"], rws), order="sort")
        GC.check_table_against_index(eng, pipe, index)
        assert (eng.alignments_permutation()[:index.n] == index.src_row).all() and eng.alignment_sort_stats()["sorted"] == 1
    finally:
        pipe.close()


def test_tie_pile_at_the_cap_follows_the_strand_bit(eng, tmp_path):
    references, lengths, rws, cand = AC.tie_pile()
    recs = list(AC.text_file(references, lengths, rws).fetch(until_eof=True))
    path = str(tmp_path / "pile.bam")
    records.write_bam(path, references, lengths, recs, sort_order="unsorted")
    o = _options()
    got = {}
    for order in ("sort", "file"):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=200, keep_alignments=True, alignment_order=order)
        try:
            pipe.run()
            ids = {nm: k for k, nm in enumerate(pipe.bam.read_names())}
            t, rid, _ = GC.table_from_candidates([cand], references, lambda nm: ids.setdefault(nm, len(ids)))
            eng.genotype_resident(o, lengths, table=t, sig_read_id=rid)
            got[order] = int(eng.fetch_genotypes()["ref_reads"][0])
            names = [pipe.bam.read_names()[i] for i in eng.alignments()["read_id"][499:502].tolist()]
            assert names == (["A", "C", "B"] if order == "sort" else ["B", "A", "C"])
        finally:
            pipe.close()
    assert got == {"sort": 0, "file": 1}


@pytest.mark.parametrize("front", ("device", "host", "python"))
def test_queryname_front_ends_keep_the_records_own_flags(eng, tmp_path, front):
    references, lengths, rws, cand, expected = AC.flag_groups()
    recs = list(AC.text_file(references, lengths, rws, "queryname").fetch(until_eof=True))
    path = str(tmp_path / "groups.bam")
    records.write_bam(path, references, lengths, recs, sort_order="queryname")
    o = _options()
    pipe = None
    try:
        if front == "python":
            hb = batch.build_batch(records.AlignmentFile(path), o, mode="queryname")
            assert (hb.arrays["flag"] & _abi.SVX_FLAG_SKIP).sum() >= 6
            names = hb.read_names
            eng.keep_alignments(True, order="sort", file_flags=True)
            eng.accumulate(True)
            eng.set_slot_base(0)
            eng.collect(hb, _abi.Params.from_options(o), fetch=False)
            eng.keep_alignments(False, order="sort", file_flags=True)
        else:
            pipe, n = _pipe(eng, path, o, 4, mode="queryname", device_decode=front == "device")
            assert n == len(recs)
            names = pipe.bam.read_names()
        ids = {nm: k for k, nm in enumerate(names)}
        t, rid, _ = GC.table_from_candidates([cand], references, lambda nm: ids.setdefault(nm, len(ids)))
        for min_mapq in (20, 10):
            eng.genotype_resident(_options(min_mapq=min_mapq), lengths, table=t, sig_read_id=rid)
            assert int(eng.fetch_genotypes()["ref_reads"][0]) == expected[min_mapq], min_mapq
        # flag and end of the records the front end marked are the file's
        index = SVIM_genotyping.AlignmentIndex(AC.text_file(references, lengths, rws), order="sort")
        a = eng.alignments()
        assert (a["flag"] == index.flag).all() and (a["end"] == index.end).all() and (a["pos"] == index.pos).all() and (a["mapq"] == index.mapq).all()
        by_id = {v: k for k, v in index.name_ids.items()}
        assert [names[i] for i in a["read_id"].tolist()] == [by_id[i] for i in index.name_id.tolist()]
        assert (eng.alignments_permutation() == index.src_row).all()
    finally:
        if pipe is not None:
            pipe.close()
        else:
            eng.accumulate(False)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _object_route(eng_join, table, sig, names, references, lengths, recs, o):
    """objects of the candidate table, genotyped by SVIM_genotyping.genotype(alignment_order="sort") over `eng_join`'s interval join, on the records as the
    file has them -> (six lists in write_final_vcf's argument order, per-row fields in table order)"""
    sigs = SignatureList(sig, references, names)
    dele, inv, int_dup, tan_dup, ins, bnd = [list(x) for x in convert.candidate_lists(table, sigs, references)]
    bam = records.AlignmentFile(text=synth.sam_text(references, lengths, recs, sort_order="unsorted"))
    eng_join._svx_index_id = None
    for lst, typ in ((dele, "DEL"), (inv, "INV"), (ins, "INS"), (int_dup, "DUP_INT")):
        SVIM_genotyping.genotype(lst, bam, typ, o, engine=eng_join, alignment_order="sort")
    fields = [[c.support_fraction, c.genotype, c.ref_reads, c.alt_reads] for lst in (dele, inv, int_dup, tan_dup, ins, bnd) for c in lst]
    return (int_dup, inv, tan_dup, dele, ins, bnd), fields


def _body(path):
    return b"".join(l for l in open(path, "rb").read().splitlines(True) if not l.startswith(b"#"))


def _to_vcf(eng, pipe, genome, out):
    pipe.cluster(genome=genome)
    pipe.combine()
    pipe.genotype()
    pipe.write_vcf(out)
    return dict(body=_body(out), g=eng.fetch_genotypes(), table=eng.fetch_candidates(), sig=eng.fetch_signatures(0), names=pipe.bam.read_names())


@pytest.fixture(scope="module")
def seeded():
    return AC.seeded_records()


@pytest.mark.parametrize("kind", ("queryname_bam", "queryname_sam", "shuffled_bam"))
def test_file_in_any_order_to_a_genotyped_vcf(eng, oracle, tmp_path, seeded, kind):
    references, lengths, refs, sorted_recs = seeded
    o = _options()
    genome = convert.genome_arrays(refs, references)
    if kind == "shuffled_bam":
        recs, mode, so = AC.shuffled_records(sorted_recs), "coordinate", "unsorted"
    else:
        recs, mode, so = AC.name_order(sorted_recs), "queryname", "queryname"
    if kind == "queryname_sam":
        path = str(tmp_path / "reads.sam")
        with open(path, "w") as fh:
            fh.write(synth.sam_text(references, lengths, recs, sort_order=so))
    else:
        path = str(tmp_path / "reads.bam")
        records.write_bam(path, references, lengths, recs, sort_order=so)
    pipe, n = _pipe(eng, path, o, 389, mode=mode)
    try:
        assert n == len(recs)
        res = _to_vcf(eng, pipe, genome, str(tmp_path / "variants.vcf"))
        assert eng.alignment_sort_stats()["sorted"] == 1 and eng.alignments()["tid"].size == len(recs)
    finally:
        pipe.close()
    table, g = res["table"], res["g"]
    cc = table.class_count
    assert cc[_abi.CAND_DEL] > 3 and cc[_abi.CAND_INS] > 0 and len(set(g["gt"].tolist())) >= 2 and int(g["ref_reads"].max()) > 0
    lists6, fields = _object_route(oracle, table, res["sig"], res["names"], references, lengths, recs, o)
    assert GC.columns_as_fields(g) == fields
    want = "".join(l + "\n" for l in SVIM_COMBINE.vcf_body_python(*lists6, TYPES, o, False, None)).encode("utf-8")
    assert res["body"] == want
    if kind != "shuffled_bam":
        return
    # the definition: the genotype columns of the default pipeline over sort_bam(file), candidate by candidate
    by_sort = str(tmp_path / "sorted.bam")
    harness.sort_bam(path, by_sort, index=False)
    pipe = harness.BamPipeline(by_sort, o, eng, threads=2, batch_records=389, keep_alignments=True)
    try:
        assert pipe.run() == len(recs)
        ref = _to_vcf(eng, pipe, genome, str(tmp_path / "variants_sorted.vcf"))
        assert eng.alignment_sort_stats()["sorted"] == 0
    finally:
        pipe.close()
    key = lambda t: sorted(zip(t.cls[:t.n].tolist(), t.contig[:t.n].tolist(), t.start[:t.n].tolist(), t.end[:t.n].tolist(), t.contig2[:t.n].tolist(),      # noqa: E731
                               t.start2[:t.n].tolist(), range(t.n)))
    mine, theirs = key(table), key(ref["table"])
    # a difference here would be COLLECT's or CLUSTER's dependence on record order, not GENOTYPE's
    assert [m[:6] for m in mine] == [m[:6] for m in theirs], "the candidate tables of the shuffled and the sorted file differ"
    gm, gr = GC.columns_as_fields(g), GC.columns_as_fields(ref["g"])
    assert [gm[m[6]] for m in mine] == [gr[m[6]] for m in theirs]
    fm, fr = g["support_fraction"].view(np.uint64), ref["g"]["support_fraction"].view(np.uint64)
    assert [int(fm[m[6]]) for m in mine] == [int(fr[m[6]]) for m in theirs]
