"""BGZF output on the device (svx_text_gz, svim_amd/csrc/textgz.hip): the stream the kernels make equals, byte for byte, what the host build of the same header
makes of the same text (svx_text_gz_host, which tests/test_text_gz.py holds against zlib), on uploaded bytes and on the VCF and BED text of a seeded pipeline;
the block table, the state rules, the writers."""
import gzip
import os
import types

import numpy as np
import pytest

import bed_cases as BC
import text_gz_cases as TC
import vcf_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


def _stream(eng):
    """the stream of the engine's last text_gz() call, fetched in 50 000-byte pieces, with its tables checked -> (bytes, file_off, block_coff, block_uoff)"""
    n_files, n_blocks, n_bytes = eng.text_gz_count()
    s = b"".join(eng.text_gz_fetch(at, min(50_000, n_bytes - at)) for at in range(0, n_bytes, 50_000))
    fo, co, uo = eng.text_gz_tables()
    assert len(s) == n_bytes and len(fo) == n_files + 1 and len(co) == len(uo) == n_blocks + 1
    assert fo[0] == co[0] == uo[0] == 0 and fo[-1] == co[-1] == n_bytes and bool(np.all(np.diff(co) >= 28)) and bool(np.all(np.diff(uo) >= 0))
    assert set(fo.tolist()) <= set(co.tolist())
    st = eng.text_gz_stats()
    assert st["n_files"] == n_files and st["n_blocks"] == n_blocks == st["blocks_eof"] + st["blocks_stored"] + st["blocks_dynamic"] and st["blocks_eof"] == n_files
    assert st["bytes_out"] == n_bytes and st["bytes_in"] == uo[-1] and st["t_total_ms"] > 0
    return s, fo, co, uo


def _check_files(eng, texts, what):
    """the engine's stream against the texts of its files: every file's range = svx_text_gz_host of that file's text, inflates to it, and the block table says
    where every block and its text begin"""
    from svim_amd import _lib
    s, fo, co, uo = _stream(eng)
    assert len(fo) - 1 == len(texts), what
    base, blocks = 0, []
    for k, text in enumerate(texts):
        part = s[int(fo[k]):int(fo[k + 1])]
        want = _lib.text_gz_host(text)
        assert len(part) == len(want) and part == want, "%s, file %d: the device stream differs from the host build at byte %d" % (
            what, k, next((i for i, (a, b) in enumerate(zip(part, want)) if a != b), min(len(part), len(want))))
        assert gzip.decompress(part) == text, (what, k)
        if not text:
            assert part == TC.EOF_BLOCK, (what, k)
        blocks += [(int(fo[k]) + at, base + uat) for at, uat, _, _ in TC.walk(part, text)]
        base += len(text)
    assert [b[0] for b in blocks] == co[:-1].tolist() and [b[1] for b in blocks] == uo[:-1].tolist() and uo[-1] == base, what
    return s


def test_device_stream_equals_host_build_on_uploaded_bytes(eng):
    from svim_amd import _abi
    vcf, bed = TC.vcf_golden_text(), TC.bed_golden_text()
    inputs = [("vcf_golden", vcf), ("bed_golden", bed), ("vcf_golden_tiled", TC.tiled(vcf, 3 * len(vcf) + 17)), ("bed_golden_tiled", TC.tiled(bed, 2 * len(bed) + 5))] + TC.corner_inputs()
    for name, text in inputs:
        assert eng.text_gz(_abi.TEXT_GZ_HOST, text)[0] == 1
        _check_files(eng, [text], name)
    # several files in one call, empty ones among them
    files = [b"", vcf[:70000], b"", bed[:1000], TC.tiled(bed, 2 * TC.BLOCK), b"x", b""]
    off = np.cumsum([0] + [len(f) for f in files])
    assert eng.text_gz(_abi.TEXT_GZ_HOST, b"".join(files), off)[0] == len(files)
    _check_files(eng, files, "seven files")
    assert eng.text_gz_stats()["blocks_stored"] == 1                      # the file of one byte


def _options():
    return types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                                 position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False,
                                 trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, symbolic_alleles=True, tandem_duplications_as_insertions=False,
                                 interspersed_duplications_as_insertions=False, insertion_sequences=True, read_names=True, zmws=False, sample="Sample", genome=None)


def _seeded(n_reads=900, n_sites=60, n_fuzz=300):
    from svim_amd import synth
    contigs = [("chr1", 120000), ("chr2", 50000), ("chr10", 40000)]
    refs = synth.make_reference(3, contigs)
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.planted_reads(5, n_reads, refs, references, lengths, n_sites=n_sites, types=("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND"))
    recs += synth.fuzz_split_reads(6, n_fuzz, references, lengths)
    return refs, references, lengths, synth.coordinate_sort(recs)


def _resident_pipeline(eng):
    """COLLECT -> CLUSTER -> COMBINE of the seeded reads, everything resident -> (references, read names, options)"""
    from svim_amd import _abi, batch, convert, records, synth
    refs, references, lengths, recs = _seeded()
    o = _options()
    hb = batch.build_batch(records.AlignmentFile(text=synth.sam_text(references, lengths, recs)), o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    eng.set_genome(*convert.genome_arrays(refs, references))
    eng.collect(hb, p)
    eng.cluster(p, hb.contig_rank, source=0, fetch=False)
    table = eng.combine(cp, hb.contig_rank)
    assert table.n > 20
    return references, hb.read_names, o


def _bed_files(eng):
    text = eng.bed_fetch()
    off, _ = eng.bed_file_offsets()
    return [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def test_seeded_pipeline_text_of_sources_0_and_1(eng):
    from svim_amd import _abi
    references, read_names, o = _resident_pipeline(eng)
    vp = _abi.VcfParams.from_options(o, VC.ALL_TYPES, False)
    n_lines, n_bytes = eng.vcf(vp, references, read_names=read_names)
    assert n_lines > 20 and n_bytes > 5000
    text = eng.vcf_fetch()
    assert eng.text_gz(_abi.TEXT_GZ_VCF)[0] == 1
    _check_files(eng, [text], "source 0")
    assert eng.vcf_fetch() == text                                        # the text is still what it was
    for product, n_files in ((_abi.BED_SIGNATURE_BEDS, 7), (_abi.BED_SIGNATURE_VCF, 1), (_abi.BED_CANDIDATE_BEDS, 8)):
        assert eng.bed(product, references, read_names=read_names)[0] == n_files
        files = _bed_files(eng)
        assert eng.text_gz(_abi.TEXT_GZ_BED)[0] == n_files
        _check_files(eng, files, "source 1, product %d" % product)
    # a product with empty files: the golden case without clusters
    from svim_amd import bed
    G = BC.load()
    sigs = BC.signatures(G)
    case = [c for c in G["cases"] if not any(c["clusters"][s] for s in G["cluster_slots"])]
    if case:
        done = bed.signature_text(_abi.BED_SIGNATURE_BEDS, BC.cluster_lists(G, case[0], sigs), engine=eng)
        assert done is not None
    else:
        case0 = G["cases"][0]
        lists = list(BC.cluster_lists(G, case0, sigs))
        lists[0] = []                                                      # no deletion clusters: the first file is empty
        assert bed.signature_text(_abi.BED_SIGNATURE_BEDS, tuple(lists), engine=eng) is not None
    files = _bed_files(eng)
    assert any(not f for f in files)
    eng.text_gz(_abi.TEXT_GZ_BED)
    _check_files(eng, files, "a product with an empty file")


def test_device_inflate_reads_what_the_device_wrote(eng, tmp_path):
    """the blocks of the VCF stream through svx_inflater_run (csrc/bgzf.hip, the reader's decoder) = the text"""
    from svim_amd import _abi, _lib
    references, read_names, o = _resident_pipeline(eng)
    eng.vcf(_abi.VcfParams.from_options(o, VC.ALL_TYPES, False), references, read_names=read_names)
    text = eng.vcf_fetch()
    eng.text_gz(_abi.TEXT_GZ_VCF)
    path = str(tmp_path / "v.vcf.gz")
    with open(path, "wb") as fh:
        fh.write(eng.text_gz_fetch())
    blocks = _lib.bgzf_blocks(path)
    assert len(blocks) == eng.text_gz_count()[1] and sum(s for _, s in blocks) == len(text)
    f = _lib.Inflater(0)
    try:
        assert f.inflate(blocks).tobytes() == text
        big = TC.tiled(TC.vcf_golden_text(), 5 * TC.BLOCK + 100)
        eng.text_gz(_abi.TEXT_GZ_HOST, big)
        with open(path, "wb") as fh:
            fh.write(eng.text_gz_fetch())
        assert f.inflate(_lib.bgzf_blocks(path)).tobytes() == big
    finally:
        f.close()


def test_state_errors_leave_the_context_usable():
    from svim_amd import _abi, _lib, bed
    e = _lib.Engine(0)
    try:
        for source in (_abi.TEXT_GZ_VCF, _abi.TEXT_GZ_BED):
            with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
                e.text_gz(source)
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.text_gz_count()
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.text_gz_fetch(0, 0)
        G = BC.load()
        sigs = BC.signatures(G)
        ct, names, st, reads = bed.cluster_table_from_lists(BC.cluster_lists(G, G["cases"][0], sigs))
        e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads)
        files = _bed_files(e)
        e.text_gz(_abi.TEXT_GZ_BED)
        _check_files(e, files, "before")
        e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads)          # a later svx_bed: the stream of the text before is void
        for call in (e.text_gz_count, e.text_gz_fetch, e.text_gz_tables):
            with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
                call()
        e.text_gz(_abi.TEXT_GZ_BED)
        _check_files(e, files, "after")
        # the same for svx_vcf
        GV = VC.load()
        case = [c for c in GV["cases"] if c["switches"]["symbolic_alleles"]][0]
        lists6 = VC.lists6(VC.objects(VC.case_rows(GV, case), GV["sigs"]))
        from svim_amd import SVIM_COMBINE
        run = lambda: SVIM_COMBINE.vcf_body_device(*lists6, GV["contigs"], case["types"], VC.options(case), False, engine=e)      # noqa: E731
        assert run() is not None
        text = e.vcf_fetch()
        e.text_gz(_abi.TEXT_GZ_VCF)
        _check_files(e, [text], "vcf before")
        e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads)          # svx_bed leaves the stream of the VCF text alone
        _check_files(e, [text], "vcf, after a svx_bed")
        assert run() is not None
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.text_gz_count()
        e.text_gz(_abi.TEXT_GZ_HOST, b"still usable\n" * 7000)
        _check_files(e, [b"still usable\n" * 7000], "source 2 after the errors")
        with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
            e.text_gz_fetch(0, 1 << 40)
    finally:
        e.close()


def _gunzip(path):
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[-28:] == TC.EOF_BLOCK and data[:4] == b"\x1f\x8b\x08\x04", path
    return gzip.decompress(data)


def _behind_date(vcf):
    return b"\n".join(l for l in vcf.split(b"\n") if not l.startswith(b"##fileDate="))


def test_writers_compressed_equal_plain(eng, tmp_path):
    from svim_amd import convert, harness, records
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    o.min_mapq, o.types = 20, "DEL,INS,INV,DUP:TANDEM,DUP:INT,BND"
    for k, v in dict(minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2).items():
        setattr(o, k, v)
    path = str(tmp_path / "small.bam")
    records.write_bam(path, references, lengths, recs)
    eng.set_genome(*convert.genome_arrays(refs, references))
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True, keep_alignments=True)
    try:
        assert pipe.run() > 0
        pipe.cluster()
        plain, packed = str(tmp_path / "plain"), str(tmp_path / "packed")
        os.makedirs(plain), os.makedirs(packed)
        n1 = pipe.write_signature_files(plain, "2.0.0")
        assert pipe.write_signature_files(packed, "2.0.0", compress=True) == n1 > 0
        pipe.combine()
        n2 = pipe.write_candidate_files(plain)
        assert pipe.write_candidate_files(packed, compress=True) == n2 > 0
        for genotyped in (False, True):
            if genotyped:
                pipe.genotype()
            a, b = str(tmp_path / ("v%d.vcf" % genotyped)), str(tmp_path / ("v%d.vcf.gz" % genotyped))
            assert pipe.write_vcf(a) == pipe.write_vcf(b) > 0
            with open(a, "rb") as fh:
                want = fh.read()
            assert _behind_date(_gunzip(b)) == _behind_date(want) and want.count(b"\n") > 30
            assert os.path.getsize(b) < os.path.getsize(a) // 2
    finally:
        pipe.close()
    files = sorted(os.path.join(sub, f) for sub in ("signatures", "candidates") for f in os.listdir(os.path.join(plain, sub)))
    assert len(files) == 16 and [f + ".gz" for f in files] == sorted(os.path.join(sub, f) for sub in ("signatures", "candidates") for f in os.listdir(os.path.join(packed, sub)))
    some = 0
    for f in files:
        with open(os.path.join(plain, f), "rb") as fh:
            want = fh.read()
        assert _gunzip(os.path.join(packed, f + ".gz")) == want, f
        some += 1 if want else 0
    assert some >= 8


def test_write_final_vcf_bgzip_output_on_both_routes(eng, tmp_path):
    from svim_amd import SVIM_COMBINE, _abi, batch, convert, lazy, records, synth
    # the object route (source 2 of svx_text_gz: a candidate with a consensus sequence takes the Python definition) and the table route (source 0 after svx_vcf)
    G = VC.load()
    case = [c for c in G["cases"] if c["switches"]["symbolic_alleles"]][0]
    lengths = [len(G["genome"][c]) for c in G["contigs"]]
    for sub in ("table", "python"):
        out = {}
        for bgzip in (False, True):
            d = tmp_path / ("%s_%d" % (sub, bgzip))
            d.mkdir()
            objs = VC.objects(VC.case_rows(G, case), G["sigs"])
            if sub == "python":
                objs["INS"][0].sequence = "ACGTACGT"
            o = VC.options(case, working_dir=str(d), genome=None, bgzip_output=bgzip)
            SVIM_COMBINE.write_final_vcf(*VC.lists6(objs), "2.0.0", G["contigs"], lengths, case["types"], o, engine=eng)
            assert os.listdir(str(d)) == ["variants.vcf.gz" if bgzip else "variants.vcf"]
            out[bgzip] = _gunzip(str(d / "variants.vcf.gz")) if bgzip else open(str(d / "variants.vcf"), "rb").read()
        assert _behind_date(out[True]) == _behind_date(out[False]) and out[False].count(b"\n") > 20, sub
    # the resident route
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    hb = batch.build_batch(records.AlignmentFile(text=synth.sam_text(references, lengths, recs)), o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    eng.set_genome(*convert.genome_arrays(refs, references))
    sig, _ = eng.collect(hb, p)
    eng.cluster(p, hb.contig_rank, source=0, fetch=False)
    table = eng.combine(cp, hb.contig_rank)
    sigs = lazy.SignatureList(sig, references, hb.read_names)
    out = {}
    for bgzip in (False, True):
        d = tmp_path / ("resident_%d" % bgzip)
        d.mkdir()
        dl, i, di, t, n, b = convert.candidate_lists(table, sigs, references)
        lists6 = (di, i, t, dl, n, b)
        assert SVIM_COMBINE._resident_candidates(lists6, eng)
        o.working_dir, o.bgzip_output = str(d), bgzip
        SVIM_COMBINE.write_final_vcf(*lists6, "2.0.0", references, lengths, VC.ALL_TYPES, o, engine=eng)
        assert all(x._objs is None for x in lists6)
        out[bgzip] = _gunzip(str(d / "variants.vcf.gz")) if bgzip else open(str(d / "variants.vcf"), "rb").read()
    assert _behind_date(out[True]) == _behind_date(out[False]) and out[False].count(b"\n") > 40
