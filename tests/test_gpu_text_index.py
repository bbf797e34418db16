"""The tabix index on the device (svx_text_index, svim_amd/csrc/textindex.hip): the bytes the kernels make equal, byte for byte, what the host build of the same
header makes (svx_text_index_host) and what the definition says (svim_amd/tabix.py; tests/test_tabix.py holds both to region queries), on uploaded texts and on
the VCF and BED text of a seeded pipeline; position order on the device; the state rules; the writers."""
import gzip
import os

import numpy as np
import pytest

import bed_cases as BC
import text_gz_cases as TC
import text_index_cases as XC
import vcf_cases as VC
from test_gpu_text_gz import _bed_files, _options, _resident_pipeline, _seeded
from svim_amd import tabix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


def _expect(text, coff, uoff, preset, base):
    """(status, bytes) by the definition, and the host build agrees"""
    from svim_amd import _lib
    got = []
    for build in (tabix.build_index, _lib.text_index_host):
        try:
            got.append((0, build(text, coff, uoff, preset, base)))
        except tabix.TabixError as e:
            got.append((e.code, b""))
    assert got[0] == got[1]
    return got[0]


def _check_index(eng, texts, preset, bases, what):
    """the index of the engine's last text_gz() against the definition and the host build, file by file, from the block table the ENGINE reports"""
    fo, co, uo = eng.text_gz_tables()
    assert len(fo) - 1 == len(texts), what
    n_files, n_bytes = eng.text_index(preset, bases)
    blobs, status = eng.text_index_fetch()
    assert n_files == len(texts) == len(blobs) == len(status) and n_bytes == sum(len(b) for b in blobs), what
    co, uo = co.tolist(), uo.tolist()
    t_at, statuses = 0, []
    for k, text in enumerate(texts):
        b0, b1 = co.index(int(fo[k])), co.index(int(fo[k + 1]))
        coff = [c - co[b0] for c in co[b0:b1 + 1]]
        uoff = [u - t_at for u in uo[b0:b1]] + [len(text)]
        want_status, want = _expect(text, coff, uoff, preset, int(bases[k]) if bases is not None else 0)
        assert status[k] == want_status, (what, k, status[k], want_status)
        assert len(blobs[k]) == len(want) and blobs[k] == want, "%s, file %d: the device index differs from the definition at byte %d of %d" % (
            what, k, next((i for i, (a, b) in enumerate(zip(blobs[k], want)) if a != b), min(len(blobs[k]), len(want))), len(want))
        assert want_status == XC.python_status(text, preset), (what, k)
        t_at += len(text)
        statuses.append(want_status)
    st = eng.text_index_stats()
    assert st["n_files"] == len(texts) and st["n_files_indexed"] == statuses.count(0) and st["bytes_out"] == n_bytes and st["bytes_text"] == t_at and st["t_total_ms"] > 0
    return blobs, statuses


def test_device_index_equals_host_build_and_definition_on_uploaded_texts(eng):
    from svim_amd import _abi
    inputs = [("seeded_vcf", XC.VCF, TC.seeded_vcf_text()), ("seeded_bed", XC.BED, XC.seeded_bed_text())] + XC.corner_texts() + [(n, p, t) for n, p, t, _ in XC.refused_texts()]
    for name, preset, text in inputs:
        assert eng.text_gz(_abi.TEXT_GZ_HOST, text)[0] == 1
        for base in (None, [4321]):
            blobs, statuses = _check_index(eng, [text], preset, base, name)
        if name.startswith("seeded"):
            assert statuses == [0]
            fo, co, uo = eng.text_gz_tables()
            XC.check_structure(blobs[0], text, co.tolist(), uo.tolist(), preset, 4321)
            st = eng.text_index_stats()
            assert st["n_records"] == text.count(b"\n") and st["n_contigs"] == (8 if preset == XC.VCF else 6) and st["n_chunks"] >= st["n_bins"] >= st["n_contigs"]
    assert [s for n, p, t, s in XC.refused_texts()] == [XC.python_status(t, p) for n, p, t, _ in XC.refused_texts()]
    # the reference's own order is refused on the device too
    G = VC.load()
    body = [c for c in G["cases"] if len(c["body"]) == 42][0]["body"]
    text = "".join(l + "\n" for l in body).encode()
    eng.text_gz(_abi.TEXT_GZ_HOST, text)
    assert _check_index(eng, [text], XC.VCF, None, "golden body")[1] == [tabix.E_ORDER]
    # several files in one call: sorted, refused, empty, one that does not end in a newline; a status is per file and the others keep their index
    bed = XC.seeded_bed_text()
    files = [b"", bed[:70000].rsplit(b"\n", 1)[0] + b"\n", b"chr1\t9\t10\nchr1\t8\t10\n", b"", bed, b"chr2\t5\t536870913\n", b"chr3\t1\t2", b""]
    off = np.cumsum([0] + [len(f) for f in files])
    assert eng.text_gz(_abi.TEXT_GZ_HOST, b"".join(files), off)[0] == len(files)
    bases = [0, 100, 0, 5, 123456, 0, 7, 0]
    assert _check_index(eng, files, XC.BED, bases, "eight files")[1] == [0, 0, tabix.E_ORDER, 0, 0, tabix.E_RANGE, 0, 0]


def test_seeded_pipeline_position_order_and_index_of_sources_0_and_1(eng):
    from svim_amd import SVIM_COMBINE, _abi
    references, read_names, o = _resident_pipeline(eng)
    vp = _abi.VcfParams.from_options(o, VC.ALL_TYPES, False)
    assert vp.position_order is False
    n_lines, n_bytes = eng.vcf(vp, references, read_names=read_names)
    plain = eng.vcf_fetch()
    assert eng.vcf(vp, references, read_names=read_names, position_order=False) == (n_lines, n_bytes) and eng.vcf_fetch() == plain      # off: today's bytes
    eng.text_gz(_abi.TEXT_GZ_VCF)
    status = _check_index(eng, [plain], XC.VCF, [999], "source 0, the reference's order")[1]
    print("the reference's order of the seeded run: status %s" % status)
    # on: the same lines with the same ids, in the order the definition gives
    assert eng.vcf(vp, references, read_names=read_names, position_order=True) == (n_lines, n_bytes)
    ordered = eng.vcf_fetch()
    lines = plain.decode().splitlines()
    assert ordered.decode().splitlines() == SVIM_COMBINE.position_ordered(lines, references) and sorted(ordered.splitlines()) == sorted(plain.splitlines())
    assert n_lines > 20 and XC.python_status(ordered, XC.VCF) == 0
    eng.text_gz(_abi.TEXT_GZ_VCF)
    blobs, status = _check_index(eng, [ordered], XC.VCF, [999], "source 0, position order")
    assert status == [0]
    fo, co, uo = eng.text_gz_tables()
    XC.check_structure(blobs[0], ordered, co.tolist(), uo.tolist(), XC.VCF, 999)
    vp.position_order = True                                               # the switch of the parameters, and it does not stick to the context
    eng.vcf(vp, references, read_names=read_names)
    assert eng.vcf_fetch() == ordered
    vp.position_order = False
    eng.vcf(vp, references, read_names=read_names)
    assert eng.vcf_fetch() == plain
    # the BED products: a status per file, against the Python check of the fetched text
    seen = []
    for product, n_files, preset in ((_abi.BED_SIGNATURE_BEDS, 7, XC.BED), (_abi.BED_SIGNATURE_VCF, 1, XC.VCF), (_abi.BED_CANDIDATE_BEDS, 8, XC.BED)):
        assert eng.bed(product, references, read_names=read_names)[0] == n_files
        files = _bed_files(eng)
        eng.text_gz(_abi.TEXT_GZ_BED)
        seen += _check_index(eng, files, preset, list(range(10, 10 + n_files)), "source 1, product %d" % product)[1]
    print("status of the sixteen files: %s" % seen)
    assert len(seen) == 16


def test_state_rules():
    from svim_amd import SVIM_COMBINE, _abi, _lib
    e = _lib.Engine(0)
    try:
        for call in (lambda: e.text_index(_abi.INDEX_VCF), e.text_index_count, e.text_index_fetch):
            with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
                call()
        text = XC.seeded_bed_text()
        e.text_gz(_abi.TEXT_GZ_HOST, text)
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):            # a stream, but no index of it yet
            e.text_index_count()
        with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
            e.text_index(7)
        e.text_index(_abi.INDEX_BED)
        first = e.text_index_fetch()[0][0]
        e.text_gz(_abi.TEXT_GZ_HOST, text)                                 # a new stream: the index of the one before is void
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.text_index_fetch()
        e.text_index(_abi.INDEX_BED)
        assert e.text_index_fetch()[0][0] == first
        # a stream voided by a later svx_vcf takes its index with it
        GV = VC.load()
        case = [c for c in GV["cases"] if c["switches"]["symbolic_alleles"]][0]
        lists6 = VC.lists6(VC.objects(VC.case_rows(GV, case), GV["sigs"]))
        o = VC.options(case, position_order=True)
        run = lambda: SVIM_COMBINE.vcf_body_device(*lists6, GV["contigs"], case["types"], o, False, engine=e)      # noqa: E731
        assert run() is not None
        body = SVIM_COMBINE.vcf_body_python(*lists6, case["types"], o, False, None, position_order=True, contig_names=GV["contigs"])
        assert e.vcf_fetch().decode().splitlines() == body                # source 2 of svx_vcf in position order = the definition
        e.text_gz(_abi.TEXT_GZ_VCF)
        e.text_index(_abi.INDEX_VCF)
        assert e.text_index_fetch()[1].tolist() == [0]
        assert run() is not None
        for call in (e.text_index_count, e.text_index_fetch, lambda: e.text_index(_abi.INDEX_VCF)):
            with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
                call()
        e.text_gz(_abi.TEXT_GZ_VCF)
        e.text_index(_abi.INDEX_VCF)
        assert e.text_index_fetch()[1].tolist() == [0]
    finally:
        e.close()


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _query_all(gz_path, plain_text, preset, rng, n=150):
    """tabix.query through the written .tbi = brute force over the plain text, on whole contigs, records' own intervals and random windows"""
    bgzf = _read(gz_path)
    ix = tabix.parse_index(gzip.decompress(_read(gz_path + ".tbi")))
    assert _read(gz_path + ".tbi")[-28:] == TC.EOF_BLOCK
    recs = [r for r in (tabix.parse_line(l, preset) for l in plain_text.split(b"\n")) if r is not None]
    assert ix["names"] == list(dict.fromkeys(r[0] for r in recs))
    regions = [(c, 0, 1 << 29) for c in ix["names"]] + [(b"nowhere", 0, 1000)] + [(r[0], r[1], r[2]) for r in recs[::3]]
    top = max([r[2] for r in recs] + [1])
    for _ in range(n):
        beg = int(rng.integers(0, top + 2000))
        regions.append((ix["names"][int(rng.integers(0, len(ix["names"])))] if ix["names"] else b"x", beg, beg + 1 + int(rng.integers(0, 1 << int(rng.integers(2, 15))))))
    some = 0
    for c, beg, end in regions:
        want = tabix.brute_force(plain_text, preset, c, beg, end)
        assert tabix.query(ix, bgzf, c, beg, end) == want, (gz_path, c, beg, end)
        some += bool(want)
    return some


def test_writers_with_index(eng, tmp_path):
    from svim_amd import convert, harness, records
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    o.min_mapq, o.types = 20, "DEL,INS,INV,DUP:TANDEM,DUP:INT,BND"
    for k, v in dict(minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2).items():
        setattr(o, k, v)
    path = str(tmp_path / "small.bam")
    records.write_bam(path, references, lengths, recs)
    eng.set_genome(*convert.genome_arrays(refs, references))
    rng = np.random.default_rng(8)
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True, keep_alignments=True)
    try:
        assert pipe.run() > 0
        pipe.cluster()
        plain, packed = str(tmp_path / "plain"), str(tmp_path / "packed")
        os.makedirs(plain), os.makedirs(packed)
        n1 = pipe.write_signature_files(plain, "2.0.0")
        got, missing_sig = pipe.write_signature_files(packed, "2.0.0", compress=True, index=True)
        assert got == n1 > 0
        pipe.combine()
        n2 = pipe.write_candidate_files(plain)
        got, missing_cand = pipe.write_candidate_files(packed, compress=True, index=True)
        assert got == n2 > 0
        with pytest.raises(ValueError):
            pipe.write_candidate_files(packed, index=True)
        with pytest.raises(ValueError):
            pipe.write_vcf(str(tmp_path / "v.vcf"), index=True)
        for genotyped in (False, True):
            if genotyped:
                pipe.genotype()
            a, b, c = (str(tmp_path / ("v%d%s" % (genotyped, x))) for x in (".vcf", ".vcf.gz", "_idx.vcf.gz"))
            assert pipe.write_vcf(a) == pipe.write_vcf(b) == pipe.write_vcf(c, index=True) > 0
            assert not os.path.exists(b + ".tbi") and os.path.exists(c + ".tbi")
            want, ordered = _read(a), gzip.decompress(_read(c))
            strip = lambda t: sorted(l for l in t.split(b"\n") if not l.startswith(b"##fileDate="))      # noqa: E731
            assert gzip.decompress(_read(b)).split(b"\n")[3:] == want.split(b"\n")[3:]                  # without index: the reference's order, as before
            assert strip(ordered) == strip(want) and XC.python_status(ordered, XC.VCF) == 0
            assert _query_all(c, ordered, XC.VCF, rng) > 20
    finally:
        pipe.close()
    # the sixteen files: a .tbi exactly for the files the Python check takes, and it answers queries
    files = sorted(os.path.join(sub, f) for sub in ("signatures", "candidates") for f in os.listdir(os.path.join(plain, sub)))
    assert len(files) == 16
    missing = set(missing_sig) | set(missing_cand)
    indexed = 0
    for f in files:
        text = _read(os.path.join(plain, f))
        preset = XC.VCF if f.endswith(".vcf") else XC.BED
        gz = os.path.join(packed, f + ".gz")
        assert gzip.decompress(_read(gz)) == text, f
        ok = XC.python_status(text, preset) == 0
        assert os.path.exists(gz + ".tbi") == ok == (os.path.basename(f) not in missing), f
        if ok:
            _query_all(gz, text, preset, rng, 40)
            indexed += 1
    print("indexed %d of 16; without: %s" % (indexed, sorted(missing)))
    assert indexed + len(missing) == 16


def test_write_final_vcf_with_tabix_index_on_three_routes(eng, tmp_path):
    from svim_amd import SVIM_COMBINE, _abi, batch, convert, lazy, records, synth
    G = VC.load()
    case = [c for c in G["cases"] if c["switches"]["symbolic_alleles"] and len(c["body"]) == 42][0]
    lengths = [len(G["genome"][c]) for c in G["contigs"]]
    rng = np.random.default_rng(9)
    for sub in ("table", "python"):
        d = tmp_path / sub
        d.mkdir()
        objs = VC.objects(VC.case_rows(G, case), G["sigs"])
        if sub == "python":
            objs["INS"][0].sequence = "ACGTACGT"
        o = VC.options(case, working_dir=str(d), genome=None, bgzip_output=True, tabix_index=True)
        SVIM_COMBINE.write_final_vcf(*VC.lists6(objs), "2.0.0", G["contigs"], lengths, case["types"], o, engine=eng)
        assert sorted(os.listdir(str(d))) == ["variants.vcf.gz", "variants.vcf.gz.tbi"]
        text = gzip.decompress(_read(str(d / "variants.vcf.gz")))
        body = [l for l in text.decode().splitlines() if not l.startswith("#")]
        if sub == "table":
            assert body == SVIM_COMBINE.position_ordered(case["body"], G["contigs"])
        assert len(body) == 42 and XC.python_status(text, XC.VCF) == 0
        assert _query_all(str(d / "variants.vcf.gz"), text, XC.VCF, rng, 60) > 10
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    hb = batch.build_batch(records.AlignmentFile(text=synth.sam_text(references, lengths, recs)), o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    eng.set_genome(*convert.genome_arrays(refs, references))
    sig, _ = eng.collect(hb, p)
    eng.cluster(p, hb.contig_rank, source=0, fetch=False)
    table = eng.combine(cp, hb.contig_rank)
    sigs = lazy.SignatureList(sig, references, hb.read_names)
    d = tmp_path / "resident"
    d.mkdir()
    dl, i, di, t, n, b = convert.candidate_lists(table, sigs, references)
    lists6 = (di, i, t, dl, n, b)
    assert SVIM_COMBINE._resident_candidates(lists6, eng)
    o.working_dir, o.bgzip_output, o.tabix_index = str(d), True, True
    SVIM_COMBINE.write_final_vcf(*lists6, "2.0.0", references, lengths, VC.ALL_TYPES, o, engine=eng)
    assert all(x._objs is None for x in lists6)
    text = gzip.decompress(_read(str(d / "variants.vcf.gz")))
    assert text.count(b"\n") > 40 and _query_all(str(d / "variants.vcf.gz"), text, XC.VCF, rng, 60) > 10
