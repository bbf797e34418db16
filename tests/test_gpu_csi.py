"""The CSI index on the device (svx_bam_index_finish_fmt, svx_bam_sort_index_fmt, svx_text_index_fmt with SVX_INDEX_CSI; csrc/binidx_kernels.hpp): the bytes
the kernels make equal, byte for byte, what the host builds make and what the definition says (svim_amd/csi.py; tests/test_csi.py holds both to region queries)
on every corner file, on files and texts beyond 2^29, at the edges of the running maximum's tiles and with bins wider than 16 bits, whatever the chunks, the
batches and the mode; the index is a by-product of BamPipeline.run() and of sort_bam; it serves the shard plan and seeks; the state rules hold and the default
calls give the bytes they gave before."""
import os
import random
import types

import numpy as np
import pytest

import bai_cases as BC
import csi_cases as CC
import text_index_cases as XC
from test_gpu_bam_index import OPTS, _code, _device_index as _classic_device_index, _head_columns, _open, _pass, _set_chunk_blocks, _sv_file
from svim_amd import _abi, _lib, bai, csi, harness, records, tabix

pytestmark = pytest.mark.gpu


def _expect(path):
    n_ref, rows, v_end = bai.rows_of_bam(path)
    want = csi.build_bam_index(n_ref, rows, v_end)
    assert _lib.bam_index_host(n_ref, rows, v_end, fmt="csi") == want, path
    return dict(path=path, n_ref=n_ref, rows=rows, v_end=v_end, bytes=want)


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    """every corner file and the files beyond 2^29 with their rows, the definition's bytes and the host build's, computed once"""
    d = str(tmp_path_factory.mktemp("csi_cases_gpu"))
    paths = BC.build_all(d) + [BC.many_references_file(d)]
    for name, make in (("beyond_range", BC.beyond_range_file), ("near_2_31", CC.near_2_31_file)):
        make(os.path.join(d, name + ".bam"))
        paths.append((name, os.path.join(d, name + ".bam")))
    return {name: _expect(path) for name, path in paths}


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


def _device_index(path, fmt="csi", **kw):
    bam = _open(path)
    try:
        bam.index_begin()
        n = _pass(bam, **kw)
        return bam.index_finish(fmt), n, bam.index_stats()
    finally:
        bam.close()


@pytest.mark.parametrize("chunk_blocks", ["1", "3", None])
def test_csi_bytes_equal_host_build_and_definition(corner, monkeypatch, chunk_blocks):
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    for name, x in corner.items():
        got, n, st = _device_index(x["path"])
        assert n == len(x["rows"]), name
        assert got == x["bytes"], (name, chunk_blocks, len(got), len(x["bytes"]))
        ix = csi.parse_index(got)
        assert st["n_chunks"] == sum(len(c) for d in ix["bins"] for c in d.values()) and st["n_bins"] == sum(len(d) for d in ix["bins"]) and st["n_slots"] == 0, name
        assert st["bytes_out"] == len(got) and ix["depth"] == (6 if name in ("beyond_range", "near_2_31") else 5), name
    many = csi.parse_index(corner["many_references_few_records"]["bytes"])
    assert many["n_ref"] == 600 and sum(1 for p in many["pseudo"] if p) == 3                  # groups without rows between groups with rows


def test_csi_bytes_do_not_depend_on_batches_or_mode(corner, monkeypatch):
    for name in ("straddle_two_and_three_blocks", "near_2_31"):
        x = corner[name]
        for chunk_blocks in ("3", None):
            _set_chunk_blocks(monkeypatch, chunk_blocks)
            for kw in (dict(batch_records=7), dict(batch_records=200000), dict(batch_records=7, min_mapq=60), dict(mode="queryname", batch_records=50)):
                got, n, _ = _device_index(x["path"], **kw)
                assert n == len(x["rows"]) and got == x["bytes"], (name, chunk_blocks, kw)


def test_running_maximum_at_its_tile_edges(tmp_path):
    """row counts around one and two tiles, groups that start at, before and behind a tile's first row, a group over three tiles whose largest end is its
    first row's (every bin's loffset is then that row's vbeg), one-row groups"""
    for name, path, big in CC.tile_edge_cases(str(tmp_path)):
        x = _expect(path)
        got, n, _ = _device_index(path)
        assert n == len(x["rows"]) and got == x["bytes"], name
        ix = csi.parse_index(got)
        for t in big:
            first = next(r for r in x["rows"] if r[0] == t)
            assert set(ix["loffset"][t].values()) == {first[4]}, (name, t)
        if name == "group_over_three_tiles":
            assert sum(1 for r in x["rows"] if r[0] == 1) > 3 * CC.RMAX_TILE - 200 and len(ix["loffset"][1]) > 5
        if name == "one_row_groups":
            assert sum(1 for t in range(x["n_ref"]) if sum(1 for r in x["rows"] if r[0] == t) == 1) >= 3


def test_bins_wider_than_16_bits(corner, eng):
    """leaf bins at and above 65 536 at depth 6, a text at depth 9: a key that still shifts by 16 mixes the bin into the group"""
    ix = csi.parse_index(_device_index(corner["near_2_31"]["path"])[0])
    # (the leaf bins of records d, f + g, h and i + j of the file: windows 32 768, 65 536, 100 000 and 131 071 behind the 37 449 bins above the leaves)
    assert ix["depth"] == 6 and sorted(b for b in ix["bins"][1] if b >= 65536) == [37449 + w for w in (32768, 65536, 100000, 131071)]
    name, preset, text, depth = [t for t in CC.beyond_texts() if t[3] == 9][0]
    eng.text_gz(_abi.TEXT_GZ_HOST, text)
    eng.text_index(preset, fmt="csi")
    blobs, status = eng.text_index_fetch()
    _, coff, uoff = XC.tables(text)
    assert status.tolist() == [0] and blobs[0] == csi.build_text_index(text, coff, uoff, preset)
    assert csi.parse_index(blobs[0])["depth"] == 9 and max(csi.parse_index(blobs[0])["bins"][0]) > 1 << 24


def test_csi_of_a_file_beyond_the_first_table(tmp_path, monkeypatch):
    """150 500 records: the running maximum over many tiles, the sort in its tiled passes"""
    path = str(tmp_path / "large.bam")
    m = BC.large_file(path)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    want = _lib.bam_index_host(n_ref, rows, v_end, fmt="csi")   # (held to the definition on this file in tests/test_csi.py)
    _set_chunk_blocks(monkeypatch, "40")
    got, n, st = _device_index(path, batch_records=60000)
    assert n == m == 150500 and st["n_placed"] == 150000 > 70 * CC.RMAX_TILE and st["n_chunks"] > 16384
    assert got == want, (len(got), len(want))


def test_csi_is_a_by_product_of_the_pipeline_pass(eng, tmp_path):
    path, references, lengths, refs, recs = _sv_file(tmp_path)
    o = types.SimpleNamespace(**OPTS)
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True, build_index=True, index_format="csi")
    try:
        assert pipe.run() == len(recs)
        out = pipe.write_csi(str(tmp_path / "by_product.csi"))
        with pytest.raises(ValueError):
            pipe.write_bai()
    finally:
        pipe.close()
    alone = harness.index_bam(path, 0, out=str(tmp_path / "alone.csi"), fmt="csi")
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert csi.read_file(out) == alone == csi.read_file(str(tmp_path / "alone.csi")) == csi.build_bam_index(n_ref, rows, v_end)
    assert harness.index_bam(path, 0, fmt="auto") == bai.build_index(n_ref, rows, v_end)                  # small contigs: "auto" is the .bai


def test_sort_bam_writes_the_csi(tmp_path, corner):
    x = corner["near_2_31"]
    with open(x["path"], "rb") as fh:
        raw = b"".join(b[2] for b in bai.bgzf_blocks(fh.read()))
    import foreign_bam as FB
    head = len(FB.header_bytes(CC.HUGE_REFS, CC.HUGE_LENS))
    recs, at = [], head
    while at < len(raw):
        size = int.from_bytes(raw[at:at + 4], "little") + 4
        recs.append(raw[at:at + size])
        at += size
    random.Random(5).shuffle(recs)
    src = str(tmp_path / "shuffled.bam")
    BC.write_file(src, CC.HUGE_REFS, CC.HUGE_LENS, recs, 0xff00)
    plain, out, auto = str(tmp_path / "plain.bam"), str(tmp_path / "sorted.bam"), str(tmp_path / "auto.bam")
    harness.sort_bam(src, plain, 0, index=False)
    harness.sort_bam(src, out, 0, index_format="csi")
    harness.sort_bam(src, auto, 0, index_format="auto")
    assert open(plain, "rb").read() == open(out, "rb").read() == open(auto, "rb").read()
    assert not os.path.exists(out + ".bai") and not os.path.exists(auto + ".bai")
    n_ref, rows, v_end = bai.rows_of_bam(out)
    assert len(rows) == len(x["rows"]) and csi.read_file(out + ".csi") == csi.read_file(auto + ".csi") == csi.build_bam_index(n_ref, rows, v_end)
    with pytest.raises(bai.BaiError) as e:
        harness.sort_bam(src, str(tmp_path / "classic.bam"), 0)                      # the default still refuses what a .bai cannot hold
    assert e.value.code == bai.E_RANGE
    # the state rule of the sort's index: an unknown format is SVX_E_ARG and the sorted records stay; the other kind's name is refused before the call
    from svim_amd.bamio import NativeBam
    bam = NativeBam(src, threads=2)
    try:
        bam.set_device_decode(0)
        bam.sort_begin(0)
        assert _pass(bam) == len(rows)
        _, _, n_blocks = bam.sort_finish()
        bam.sort_encode(0, n_blocks)
        from svim_amd.bamsort import BamSortError
        with pytest.raises(BamSortError) as e:                              # (the sort's errors are BamSortError, the library's status in .code)
            bam.sort_index(7)
        assert _code(e) == _abi.SVX_E_ARG
        with pytest.raises(ValueError):
            bam.sort_index("tbi")
        assert bam.sort_index("csi") == csi.read_file(out + ".csi")
        bam.sort_abort()
    finally:
        bam.close()
    small = str(tmp_path / "small.bam")
    harness.sort_bam(corner["record_at_block_start"]["path"], small, 0, index_format="auto")
    assert os.path.exists(small + ".bai") and not os.path.exists(small + ".csi")
    assert open(small + ".bai", "rb").read() == bai.build_index(*bai.rows_of_bam(small))


def _check_text_index(eng, texts, preset, bases, what):
    """the .csi of every file of the engine's last text_gz() against the definition and the host build -> the statuses"""
    fo, co, uo = eng.text_gz_tables()
    eng.text_index(preset, bases, fmt="csi")
    blobs, status = eng.text_index_fetch()
    co, uo = co.tolist(), uo.tolist()
    t_at, out = 0, []
    for k, text in enumerate(texts):
        b0, b1 = co.index(int(fo[k])), co.index(int(fo[k + 1]))
        coff, uoff = [c - co[b0] for c in co[b0:b1 + 1]], [u - t_at for u in uo[b0:b1]] + [len(text)]
        base = int(bases[k]) if bases is not None else 0
        try:
            want, code = csi.build_text_index(text, coff, uoff, preset, base), 0
            assert _lib.text_index_host(text, coff, uoff, preset, base, fmt="csi") == want, (what, k)
        except tabix.TabixError as e:
            want, code = b"", e.code
        assert status[k] == code and code in (0, tabix.E_ORDER), (what, k, status[k], code)
        assert blobs[k] == want, (what, k, len(blobs[k]), len(want))
        t_at += len(text)
        out.append(code)
    return out


def test_text_csi_on_uploaded_texts(eng):
    for name, preset, text, depth in CC.beyond_texts():
        eng.text_gz(_abi.TEXT_GZ_HOST, text)
        for base in (None, [4321]):
            assert _check_text_index(eng, [text], preset, base, name) == [0]
    for name, preset, text in [("seeded_bed", XC.BED, XC.seeded_bed_text())] + XC.corner_texts() + [(n, p, t) for n, p, t, _ in XC.refused_texts()]:
        eng.text_gz(_abi.TEXT_GZ_HOST, text)
        _check_text_index(eng, [text], preset, None, name)
    # several files of different depths in one call: a depth and a status per file
    (a, da), (b, db) = CC.two_file_texts()
    files = [b"", a, b"chr1\t9\t10\nchr1\t8\t10\n", b, b"chr2\t5\t536870913\n", b"chr3\t1\t2"]
    off = np.cumsum([0] + [len(f) for f in files])
    assert eng.text_gz(_abi.TEXT_GZ_HOST, b"".join(files), off)[0] == len(files)
    assert _check_text_index(eng, files, XC.BED, [0, 100, 0, 5, 7, 0], "six files") == [0, 0, tabix.E_ORDER, 0, 0, 0]
    blobs, _ = eng.text_index_fetch()
    assert [csi.parse_index(blobs[k])["depth"] for k in (0, 1, 3, 4, 5)] == [5, da, db, 6, 5]
    # the classic call on the same stream still says what it said, and serves its own bytes
    eng.text_index(XC.BED, [0, 100, 0, 5, 7, 0])
    blobs, status = eng.text_index_fetch()
    assert status.tolist() == [0, 0, tabix.E_ORDER, tabix.E_RANGE, tabix.E_RANGE, 0] and blobs[1][:4] == b"TBI\1"


def test_text_csi_on_the_products_of_the_seeded_pipeline(eng):
    import vcf_cases as VC
    from test_gpu_text_gz import _bed_files, _resident_pipeline
    references, read_names, o = _resident_pipeline(eng)
    vp = _abi.VcfParams.from_options(o, VC.ALL_TYPES, False)
    eng.vcf(vp, references, read_names=read_names, position_order=True)
    ordered = eng.vcf_fetch()
    eng.text_gz(_abi.TEXT_GZ_VCF)
    assert _check_text_index(eng, [ordered], XC.VCF, [999], "source 0, position order") == [0]
    seen = []
    for product, n_files, preset in ((_abi.BED_SIGNATURE_BEDS, 7, XC.BED), (_abi.BED_CANDIDATE_BEDS, 8, XC.BED)):
        assert eng.bed(product, references, read_names=read_names)[0] == n_files
        files = _bed_files(eng)
        eng.text_gz(_abi.TEXT_GZ_BED)
        seen += _check_text_index(eng, files, preset, list(range(10, 10 + n_files)), "source 1, product %d" % product)
    assert len(seen) == 15 and set(seen) <= {0, tabix.E_ORDER}


def _query_written(gz_path, rng, n=60):
    """csi.query_text through the written .gz.csi = brute force over the plain text, on whole contigs, records' own intervals and random windows"""
    import gzip
    with open(gz_path, "rb") as fh:
        bgzf = fh.read()
    text = gzip.decompress(bgzf)
    preset = XC.VCF if ".vcf" in os.path.basename(gz_path) else XC.BED
    ix = csi.parse_index(csi.read_file(gz_path + ".csi"))
    recs = [r for r in (tabix.parse_line(l, preset) for l in text.split(b"\n")) if r is not None]
    assert ix["names"] == list(dict.fromkeys(r[0] for r in recs)) and ix["depth"] == 5
    regions = [(c, 0, 1 << 29) for c in ix["names"]] + [(b"nowhere", 0, 1000)] + [(r[0], r[1], r[2]) for r in recs[::3]]
    top = max([r[2] for r in recs] + [1])
    for _ in range(n if ix["names"] else 0):
        beg = rng.randrange(top + 2000)
        regions.append((rng.choice(ix["names"]), beg, beg + 1 + rng.randrange(1 << rng.randrange(2, 15))))
    some = 0
    for c, beg, end in regions:
        want = tabix.brute_force(text, preset, c, beg, end)
        assert csi.query_text(ix, bgzf, c, beg, end) == want, (gz_path, c, beg, end)
        some += bool(want)
    return some


def test_writers_with_a_csi(eng, tmp_path):
    """write_vcf, the signature and candidate files and write_final_vcf with a .csi beside the file; True stays the .tbi, "auto" follows the header's lengths"""
    import gzip
    import vcf_cases as VC
    from test_gpu_text_gz import _options, _seeded
    from svim_amd import SVIM_COMBINE, convert
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    o.min_mapq, o.types = 20, "DEL,INS,INV,DUP:TANDEM,DUP:INT,BND"
    path = str(tmp_path / "small.bam")
    records.write_bam(path, references, lengths, recs)
    eng.set_genome(*convert.genome_arrays(refs, references))
    rng = random.Random(8)
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True)
    try:
        assert pipe.run() > 0
        pipe.cluster()
        packed = str(tmp_path / "packed")
        os.makedirs(packed)
        _, missing_sig = pipe.write_signature_files(packed, "2.0.0", compress=True, index="csi")
        pipe.combine()
        _, missing_cand = pipe.write_candidate_files(packed, compress=True, index="csi")
        a, b, c, d = (str(tmp_path / ("v_%s.vcf.gz" % x)) for x in ("csi", "auto", "true", "tbi"))
        assert pipe.write_vcf(a, index="csi") == pipe.write_vcf(b, index="auto") == pipe.write_vcf(c, index=True) == pipe.write_vcf(d, index="tbi") > 0
        assert os.path.exists(a + ".csi") and not os.path.exists(a + ".tbi")
        for f in (b, c, d):                                         # small contigs: "auto" is the .tbi, and True stays it
            assert os.path.exists(f + ".tbi") and not os.path.exists(f + ".csi")
        strip = lambda p: [l for l in gzip.decompress(open(p, "rb").read()).split(b"\n") if not l.startswith(b"##fileDate=")]      # noqa: E731
        assert strip(a) == strip(c) and open(c + ".tbi", "rb").read() == open(d + ".tbi", "rb").read()
        assert _query_written(a, rng) > 20
        with pytest.raises(ValueError):
            pipe.write_vcf(str(tmp_path / "v.vcf"), index="csi")
        with pytest.raises(ValueError):
            pipe.write_vcf(a, index="bai")
    finally:
        pipe.close()
    missing, indexed = set(missing_sig) | set(missing_cand), 0
    for sub in ("signatures", "candidates"):
        for f in sorted(os.listdir(os.path.join(packed, sub))):
            if not f.endswith(".gz"):
                continue
            gz = os.path.join(packed, sub, f)
            text = gzip.decompress(open(gz, "rb").read())
            ok = XC.python_status(text, XC.VCF if f.endswith(".vcf.gz") else XC.BED) != tabix.E_ORDER
            assert os.path.exists(gz + ".csi") == ok == (f[:-3] not in missing) and not os.path.exists(gz + ".tbi"), f
            if ok:
                _query_written(gz, rng, 20)
                indexed += 1
    assert indexed + len(missing) == 16 and indexed > 4
    G = VC.load()
    case = [c for c in G["cases"] if c["switches"]["symbolic_alleles"] and len(c["body"]) == 42][0]
    glen = [len(G["genome"][c]) for c in G["contigs"]]
    for both in (False, True):
        d = tmp_path / ("final%d" % both)
        d.mkdir()
        oo = VC.options(case, working_dir=str(d), genome=None, bgzip_output=True, tabix_index=both, csi_index=True)
        SVIM_COMBINE.write_final_vcf(*VC.lists6(VC.objects(VC.case_rows(G, case), G["sigs"])), "2.0.0", G["contigs"], glen, case["types"], oo, engine=eng)
        assert sorted(os.listdir(str(d))) == ["variants.vcf.gz", "variants.vcf.gz.csi"] + (["variants.vcf.gz.tbi"] if both else [])
        assert _query_written(str(d / "variants.vcf.gz"), rng) > 10


def test_csi_serves_the_shard_plan_and_seeks(tmp_path):
    import foreign_bam as FB
    refs, lens = BC.REFS, BC.LENS
    recs = BC.random_records(41, 900, (1, 3, 4), lens, n_unplaced=9, big_every=11)
    path = str(tmp_path / "served.bam")
    FB.write(path, refs, lens, BC.record_bytes(recs), layout="flat", block_payload=2500, tids=[a.reference_id for a in recs])      # (writes the stub .bai, too)
    data = harness.index_bam(path, 0, out=path + ".csi", fmt="csi")
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert data == csi.build_bam_index(n_ref, rows, v_end)
    mine, stub = records.read_index(path + ".csi"), records.read_bai(path + ".bai")
    assert mine == stub
    for world in (1, 2, 3):
        for rank in range(world):
            assert harness.shard_plan(refs, lens, mine, rank, world)[1] == harness.shard_plan(refs, lens, stub, rank, world)[1]
    ix = csi.parse_index(data)
    at = {r[4]: k for k, r in enumerate(rows)}
    begins = sorted((c[0], t) for t, d in enumerate(ix["bins"]) for cs in d.values() for c in cs)
    rng = random.Random(8)
    bam = _open(path)
    try:
        assert len(begins) > 50
        for v, t in (rng.choice(begins) for _ in range(200)):  # a seek to a chunk begin the index names returns the record that starts there
            bam.seek(v, t)
            b, n = bam.read_batch(3, 0, "coordinate")
            tid, pos, flag = _head_columns(bam, b)
            r = rows[at[v]]
            assert n >= 1 and (int(tid[0]), int(pos[0]), int(flag[0]) & 0xfff) == (r[0], r[1], r[3] & 0xfff), (v, t)
        found = 0
        for tid, beg, end in CC.regions(6, rows, n_ref, 60):   # and the first record a scan names lies in the first chunk of the query, at or behind its begin
            want = csi.brute_force(rows, tid, beg, end)
            chunks, low = csi.query(ix, tid, beg, end)
            if want:
                assert chunks and chunks[0][0] <= want[0][4] and low <= want[0][4], (tid, beg, end)
                found += 1
    finally:
        bam.close()
    assert found > 20


def test_csi_state_rules(corner, tmp_path):
    good = corner["record_at_block_start"]
    n_ref, rows, v_end = good["n_ref"], good["rows"], good["v_end"]
    classic = bai.build_index(n_ref, rows, v_end)
    assert _lib.bam_index_host(n_ref, rows, v_end) == classic
    bam = _open(good["path"])
    try:
        bam.index_begin()
        assert bam.read_batch(10, 20)[1] == 10
        with pytest.raises(_lib.SvxError) as e:
            bam.index_finish("csi")                                        # before the end of the pass
        assert _code(e) == _abi.SVX_E_STATE
        assert 10 + _pass(bam, 77) == len(rows)
        with pytest.raises(_lib.SvxError) as e:
            bam.index_finish(7)                                            # an unknown format: the pass stays on
        assert _code(e) == _abi.SVX_E_ARG
        with pytest.raises(ValueError):
            bam.index_finish("tbi")                                        # a BAM has no .tbi: refused by name, the pass stays on
        assert bam.index_finish("csi") == good["bytes"] == bam.index_bytes()
        bam.rewind()
        bam.index_begin()
        assert bam.read_batch(10, 20)[1] == 10
        bam.index_abort()
        bam.rewind()
        bam.index_begin()
        assert _pass(bam, 1000) == len(rows) and bam.index_finish() == classic == bam.index_bytes()      # fetch after a classic build: classic bytes
        bam.rewind()
        bam.index_begin()
        assert _pass(bam, 1000) == len(rows) and bam.index_finish("csi") == good["bytes"]
    finally:
        bam.close()
    assert _classic_device_index(good["path"])[0] == classic               # the default call gives the bytes it gave before
    swapped = str(tmp_path / "swapped.bam")
    BC.swapped_file(swapped)
    bam = _open(swapped)
    try:
        bam.index_begin()
        _pass(bam)
        with pytest.raises(bai.BaiError) as e:
            bam.index_finish("csi")
        assert e.value.code == bai.E_ORDER
    finally:
        bam.close()
    e2 = _lib.Engine(0)
    try:
        text = XC.seeded_bed_text()
        e2.text_gz(_abi.TEXT_GZ_HOST, text)
        with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
            e2.text_index(_abi.INDEX_BED, fmt=9)
        with pytest.raises(ValueError):
            e2.text_index(_abi.INDEX_BED, fmt="bai")                       # a text has no .bai
        _, coff, uoff = XC.tables(text)
        e2.text_index(_abi.INDEX_BED, fmt="csi")
        assert e2.text_index_fetch()[0][0] == csi.build_text_index(text, coff, uoff, XC.BED)
        e2.text_index(_abi.INDEX_BED)
        assert e2.text_index_fetch()[0][0] == tabix.build_index(text, coff, uoff, XC.BED) == _lib.text_index_host(text, coff, uoff, XC.BED)
    finally:
        e2.close()
