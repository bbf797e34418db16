"""The coordinate sort on the device (svx_bam_sort_*, svim_amd/csrc/bamsort.hip fed by the device reader csrc/bamdev.hip): the stream the gather lays out, the
compressed bytes, the .bai and the permutation equal, byte for byte, what the definition says (svim_amd/bamsort.py; tests/test_bam_sort.py holds it and the
host build to each other) on every corner file of tests/bam_sort_cases.py, whatever the chunks, the batches, the mode and the pieces; record starts at every
source alignment against every destination alignment; a file of many slabs and tiles; the output read back by both readers and served by its index; a
query-name-sorted file sorted and genotyped; the state rules; a reader that never sorts is untouched."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import bai_cases as BC
import bam_sort_cases as SC
from svim_amd import _abi, _lib, bai, bamsort, harness, records, synth
from svim_amd.bamio import NativeBam

pytestmark = pytest.mark.gpu


def _expect(x):
    """the definition's stream, file, index and permutation of a case"""
    x["stream"], perm = SC.definition(x)
    x["perm"] = np.asarray(perm, dtype=np.uint32)
    x["file"] = _lib.text_gz_host(x["stream"])
    tmp = x["path"] + ".definition"
    with open(tmp, "wb") as fh:
        fh.write(x["file"])
    x["bai"] = bai.build_index(*bai.rows_of_bam(tmp))
    os.remove(tmp)
    host_body, host_perm = _lib.bam_sort_host(b"".join(x["records"]), x["n_ref"])
    assert (host_perm == x["perm"]).all() and x["stream"].endswith(host_body)
    return x


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_sort_cases_gpu"))
    return {name: _expect(x) for name, x in SC.build_all(d).items()}


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


def _open(path):
    bam = NativeBam(path, threads=2)
    bam.set_device_decode(0)
    return bam


def _pass(bam, batch_records=5000, mode="coordinate", min_mapq=20):
    n = 0
    while True:
        k = bam.read_batch(batch_records, min_mapq, mode)[1]
        if k == 0:
            return n
        n += k


def _encode_all(bam, n_blocks, piece_blocks):
    comp, raw = [], []
    for first in range(0, n_blocks, piece_blocks):
        c, r = bam.sort_encode(first, min(piece_blocks, n_blocks - first), stream=True)
        comp.append(c), raw.append(r)
    return b"".join(comp), b"".join(raw)


def _device_sort(path, piece_blocks=4096, **kw):
    """-> (stream, file, .bai, permutation, records read, stats)"""
    bam = _open(path)
    try:
        bam.sort_begin()
        n = _pass(bam, **kw)
        n_rec, n_bytes, n_blocks = bam.sort_finish()
        assert n_rec == n and n_blocks == bamsort.n_blocks(n_bytes)
        comp, raw = _encode_all(bam, n_blocks, piece_blocks)
        return raw, comp, bam.sort_index(), bam.sort_permutation(), n, bam.sort_stats()
    finally:
        bam.close()


def _check(x, got, what):
    raw, comp, index, perm, n, st = got
    assert n == len(x["records"]) == st["n_records"], what
    assert raw == x["stream"], (what, len(raw), len(x["stream"]))
    assert comp == x["file"], (what, len(comp), len(x["file"]))
    assert index == x["bai"], (what, len(index), len(x["bai"]))
    assert (perm == x["perm"]).all(), what
    assert st["stream_bytes"] == len(raw) and st["bytes_out"] == len(comp) and st["arena_bytes"] == sum(len(r) for r in x["records"]), what


def _set_chunk_blocks(monkeypatch, chunk_blocks):
    if chunk_blocks:
        monkeypatch.setenv("SVX_BAM_DEV_CHUNK_BLOCKS", chunk_blocks)          # (read when the handle switches device decode on)
    else:
        monkeypatch.delenv("SVX_BAM_DEV_CHUNK_BLOCKS", raising=False)


@pytest.mark.parametrize("chunk_blocks", ["1", "3", None])
def test_bam_sort_equals_host_build_and_definition(corner, monkeypatch, chunk_blocks):
    """chunks of 1 and 3 blocks: a slab per chunk, records that straddle chunk edges lie in the slab of the chunk they are completed in"""
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    for name, x in corner.items():
        got = _device_sort(x["path"])
        _check(x, got, (name, chunk_blocks))
        if chunk_blocks == "1" and len(x["records"]) > 100:
            assert got[5]["n_slabs"] > 1, name


def test_bam_sort_does_not_depend_on_batches_or_mode(corner, monkeypatch):
    x = corner["blocks_cut_records_anywhere"]
    for chunk_blocks in ("3", None):
        _set_chunk_blocks(monkeypatch, chunk_blocks)
        for kw in (dict(batch_records=7), dict(batch_records=200000), dict(batch_records=7, min_mapq=60), dict(mode="queryname", batch_records=7),
                   dict(mode="queryname", batch_records=200000)):
            _check(x, _device_sort(x["path"], **kw), (chunk_blocks, kw))


def test_bam_sort_does_not_depend_on_the_pieces(corner):
    for name in ("record_longer_than_two_blocks", "record_ends_at_the_block_edge", "long_cigars_and_a_cg_tag"):
        x = corner[name]
        assert bamsort.n_blocks(len(x["stream"])) >= 5
        for piece_blocks in (1, 3, 4096):
            got = _device_sort(x["path"], piece_blocks=piece_blocks)
            _check(x, got, (name, piece_blocks))
            assert got[5]["n_pieces"] == -(-bamsort.n_blocks(len(x["stream"])) // piece_blocks)


def test_bam_sort_gather_meets_every_alignment(tmp_path):
    """record starts at every source alignment 0..15 (the record's place in its slab: the slab starts where the file's first record starts) against every
    destination alignment 0..15 (its place in the sorted stream), in one chunk"""
    recs = SC.alignment_records(91, 4000)
    hdr = SC.header()
    path = str(tmp_path / "alignments.bam")
    SC.write_raw(path, hdr, recs)
    x = _expect(dict(path=path, header=hdr, records=recs, n_ref=len(SC.REFS)))
    src = np.cumsum([0] + [len(r) for r in recs])[:-1]
    dst = np.cumsum([len(bamsort.sorted_header(hdr))] + [len(recs[k]) for k in x["perm"]])[:-1]
    pairs = set(zip((src[x["perm"]] % 16).tolist(), (dst % 16).tolist()))
    assert len(pairs) == 256
    got = _device_sort(path)
    assert got[5]["n_slabs"] == 1
    _check(x, got, "alignments")


def test_bam_sort_of_a_large_shuffled_file(tmp_path, monkeypatch):
    """150 500 short records in random order, read in chunks of 40 blocks: several slabs, rows beyond their first capacity, scans over many tiles, the sort's
    tiled passes, a piece of many tiles"""
    x = SC.large_shuffled_file(str(tmp_path / "large_shuffled.bam"))
    body, perm = _lib.bam_sort_host(b"".join(x["records"]), x["n_ref"])          # (held to the definition on streams of this size in tests/test_bam_sort.py)
    stream = bamsort.sorted_header(x["header"]) + body
    _set_chunk_blocks(monkeypatch, "40")
    bam = _open(x["path"])
    try:
        bam.sort_begin()
        assert _pass(bam, 60000) == 150500
        n, n_bytes, n_blocks = bam.sort_finish()
        assert (n, n_bytes) == (150500, len(stream)) and n_blocks > 100
        assert (bam.sort_permutation() == perm).all()
        comp, raw = _encode_all(bam, n_blocks, 64)
        assert raw == stream
        assert comp == _lib.text_gz_host(stream)
        index = bam.sort_index()
        st = bam.sort_stats()
    finally:
        bam.close()
    out = str(tmp_path / "large_sorted.bam")
    with open(out, "wb") as fh:
        fh.write(comp)
    n_ref, rows, v_end = bai.rows_of_bam(out)
    assert index == _lib.bam_index_host(n_ref, rows, v_end)                       # (held to the definition on tables of this size in tests/test_bai.py)
    assert st["n_slabs"] >= 3 and st["n_records"] > 2 * 65536 and st["n_pieces"] == -(-n_blocks // 64) and st["blocks_dynamic"] + st["blocks_stored"] == n_blocks - 1 and st["blocks_eof"] == 1


def _batches(bam, batch_records):
    out = []
    while True:
        b, n = bam.read_batch(batch_records, 20)
        if n == 0:
            return out
        out.append(bam.batch_arrays(b))


def _head_columns(bam, b):
    n = int(b.n_rec)
    out = []
    for name in ("tid", "pos", "flag"):
        a = np.zeros(n, dtype=_abi.BATCH_DTYPES[name])
        if n:
            assert bam.L.svx_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.cast(getattr(b, name), C.c_void_p), C.c_uint64(a.nbytes)) == 0
        out.append(a)
    return out


def test_bam_sort_output_round_trip_through_both_readers_and_seeks(tmp_path):
    recs = BC.random_records(41, 900, (1, 3, 4), BC.LENS, n_unplaced=9, big_every=11)
    src = str(tmp_path / "shuffled.bam")
    SC.write_raw(src, SC.header(), SC.shuffled(BC.record_bytes(recs), 92), cuts=2500)
    out = str(tmp_path / "sorted.bam")
    st = harness.sort_bam(src, out, 0, piece_blocks=2)
    assert st["n_records"] == 909 and open(out, "rb").read() == bamsort.file(src)
    n_ref, rows, v_end = bai.rows_of_bam(out)
    data = open(out + ".bai", "rb").read()
    assert data == bai.build_index(n_ref, rows, v_end)
    dev, host = _open(out), NativeBam(out, threads=2)
    try:
        assert dev.sort_order == host.sort_order == "coordinate"
        a, b = _batches(dev, 150), _batches(host, 150)
        names_a, names_b = dev.read_names(), host.read_names()
        assert len(a) == len(b) == 7 and sorted(names_a) == sorted(names_b)
        for p, q in zip(a, b):
            assert p.keys() == q.keys()
            for k in p:
                if k == "read_id":
                    assert [names_a[i] for i in p[k].tolist()] == [names_b[i] for i in q[k].tolist()]
                else:
                    assert np.array_equal(p[k], q[k]), k
        # seek to the linear index's lower bound of the region's first window, read forward until pos >= end
        ix = bai.parse_index(data)
        at = {r[4]: k for k, r in enumerate(rows)}
        found = 0
        for tid, beg, end in BC.regions(6, rows, n_ref, 200):
            want = bai.brute_force(rows, tid, beg, end)
            _, low = bai.query(ix, tid, beg, end)
            if low is None:
                assert not want
                continue
            k0 = at[low]
            dev.seek(low, tid)
            got, done = [], False
            while not done:
                bt, n = dev.read_batch(300, 0, "coordinate")
                if n == 0:
                    break
                t, p, f = _head_columns(dev, bt)
                for i in range(n):
                    if p[i] >= end:
                        done = True
                        break
                    got.append((int(t[i]), int(p[i]), int(f[i]) & 0xfff))
            assert got == [(r[0], r[1], r[3] & 0xfff) for r in rows[k0:k0 + len(got)]], (tid, beg, end)
            assert all(k0 <= at[r[4]] < k0 + len(got) for r in want), (tid, beg, end)
            found += len(want)
        assert found > 300
    finally:
        dev.close()
        host.close()


OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
            del_ins_dup_max_distance=1.0, skip_consensus=True, minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2,
            symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
            interspersed_duplications_as_insertions=False, sample="Sample", genome=None, types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")


def _body(path):
    return b"".join(l for l in open(path, "rb").read().splitlines(True) if not l.startswith(b"#"))


def test_bam_sort_feeds_the_pipeline_with_genotypes(eng, tmp_path):
    """a query-name-sorted file, which svx_genotype_resident refuses, sorted on the device: the pipeline takes the result with no special handling"""
    from svim_amd import convert
    contigs = [("chr1", 120000), ("chrE", 30000), ("chr2", 50000), ("chrN", 9000)]
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 400, refs, references, lengths, n_sites=24, types=("DEL", "INS", "INV"))
    recs += synth.planted_reads(9, 100, refs, references, lengths, n_sites=6, types=("DEL", "INS"), tid=2)
    recs += synth.fuzz_split_reads(6, 60, references, lengths)
    rows = [r for r in synth.genotype_rows(31, lengths, n_reads=900, hot=((0, 60000, 300), (2, 300, 100))) if r[2] != 1]
    recs += list(records.AlignmentFile(text=synth.genotype_sam_text(references, lengths, rows)).fetch(until_eof=True))
    recs = sorted(recs, key=lambda a: a.query_name)
    src = str(tmp_path / "queryname.bam")
    records.write_bam(src, references, lengths, recs, sort_order="queryname")
    sorted_dev, sorted_def = str(tmp_path / "sorted_device.bam"), str(tmp_path / "sorted_definition.bam")
    st = harness.sort_bam(src, sorted_dev, 0)
    assert st["n_records"] == len(recs) and os.path.exists(sorted_dev + ".bai")
    with open(sorted_def, "wb") as fh:
        fh.write(bamsort.file(src))
    o = types.SimpleNamespace(**OPTS)
    off, codes = convert.genome_arrays(refs, references)
    bodies = []
    for path in (sorted_dev, sorted_def):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=211, device_decode=True, keep_alignments=True)
        try:
            assert pipe.run() == len(recs)
            pipe.cluster(genome=(off, codes))
            pipe.combine()
            pipe.genotype()
            out = path + ".vcf"
            pipe.write_vcf(out)
            bodies.append(_body(out))
        finally:
            pipe.close()
    assert bodies[0] == bodies[1] and bodies[0].count(b"\n") > 10
    calls = [l.split(b"\t")[9].split(b":")[0] for l in bodies[0].splitlines()]
    assert sum(1 for c in calls if c in (b"0/1", b"1/1", b"0/0")) > 3                        # genotype columns are present, not all "./."


def _code(excinfo):
    return getattr(excinfo.value, "code", None)


def test_bam_sort_state_rules(corner, tmp_path):
    good = corner["blocks_cut_records_anywhere"]
    n_all = len(good["records"])
    bam = _open(good["path"])
    try:
        for call in (bam.sort_finish, bam.sort_abort, bam.sort_count, lambda: bam.sort_encode(0, 1), bam.sort_index, bam.sort_permutation):
            with pytest.raises(bamsort.BamSortError) as e:
                call()                                                     # never begun
            assert _code(e) == _abi.SVX_E_STATE
        assert bam.read_batch(10, 20)[1] == 10
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_begin()                                               # after a read
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()
        bam.index_begin()
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_begin()                                               # while an index pass is on
        assert _code(e) == _abi.SVX_E_STATE
        bam.index_abort()
        bam.sort_begin()
        with pytest.raises(_lib.SvxError) as e:
            bam.index_begin()                                              # while a sort pass is on
        assert _code(e) == _abi.SVX_E_STATE
        assert bam.read_batch(10, 20)[1] == 10
        for call in (bam.sort_finish, lambda: bam.sort_encode(0, 1), bam.sort_index):
            with pytest.raises(bamsort.BamSortError) as e:
                call()                                                     # before the end of the file
            assert _code(e) == _abi.SVX_E_STATE
        for call in (bam.rewind, lambda: bam.seek(0, -2)):
            with pytest.raises(_lib.SvxError) as e:
                call()                                                     # rewind and seek during a sort pass
            assert _code(e) == _abi.SVX_E_STATE
        bam.sort_abort()                                                   # in the middle of the file: the handle reads on where it was
        assert 10 + _pass(bam, 77) == n_all
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_finish()
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()
        bam.sort_begin()
        assert _pass(bam, 1000) == n_all
        n, n_bytes, n_blocks = bam.sort_finish()
        assert n == n_all and n_bytes == len(good["stream"]) and n_blocks >= 3
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_finish()                                              # the pass is over
        assert _code(e) == _abi.SVX_E_STATE
        for first, nb in ((-1, 1), (0, 0), (n_blocks, 1), (1, n_blocks)):
            with pytest.raises(bamsort.BamSortError) as e:
                bam.sort_encode(first, nb)
            assert _code(e) == _abi.SVX_E_ARG
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_index()                                               # nothing encoded yet
        assert _code(e) == _abi.SVX_E_STATE
        bam.sort_encode(0, 1)
        bam.sort_encode(2, n_blocks - 2)                                   # a gap
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_index()
        assert _code(e) == _abi.SVX_E_STATE
        bam.sort_abort()
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_count()
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()                                                       # a second begin / pass / finish on the same handle
        bam.sort_begin()
        assert _pass(bam, 50, mode="queryname") == n_all
        n, n_bytes, n_blocks = bam.sort_finish()
        comp, raw = _encode_all(bam, n_blocks, 2)
        assert raw == good["stream"] and comp == good["file"] and bam.sort_index() == good["bai"] == bam.index_bytes()
        bam.rewind()                                                       # the sorted records stay while the handle reads again
        assert _pass(bam, 500) == n_all
        assert bam.sort_encode(0, n_blocks) == good["file"]
    finally:
        bam.close()
    host = NativeBam(good["path"], threads=2)
    try:
        for call in (host.sort_begin, host.sort_finish, host.sort_abort):
            with pytest.raises(bamsort.BamSortError) as e:
                call()
            assert _code(e) == _abi.SVX_E_STATE
    finally:
        host.close()


def test_bam_sort_arena_limit_then_a_clean_rewind(corner, monkeypatch):
    good = corner["already_in_order"]
    need = sum(len(r) for r in good["records"])
    _set_chunk_blocks(monkeypatch, "3")
    bam = _open(good["path"])
    try:
        bam.sort_begin(need - 1)
        with pytest.raises(_lib.SvxError) as e:
            _pass(bam, 50)
        assert _code(e) == _abi.SVX_E_CAPACITY
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_finish()                                              # the sort was dropped
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()
        assert _pass(bam, 50) == len(good["records"])                      # a plain pass
        bam.rewind()
        bam.sort_begin(need)                                               # exactly enough
        assert _pass(bam, 50) == len(good["records"])
        _, n_bytes, n_blocks = bam.sort_finish()
        assert bam.sort_encode(0, n_blocks) == good["file"] and bam.sort_stats()["arena_bytes"] == need
    finally:
        bam.close()
    out = good["path"] + ".refused.bam"
    with pytest.raises(_lib.SvxError) as e:
        harness.sort_bam(good["path"], out, 0, max_bytes=need - 1)
    assert _code(e) == _abi.SVX_E_CAPACITY and not os.path.exists(out) and not os.path.exists(out + ".bai")


def test_bam_reader_without_a_sort_is_untouched(corner):
    x = corner["blocks_cut_records_anywhere"]
    both = []
    for sorting in (False, True):
        bam = _open(x["path"])
        try:
            if sorting:
                bam.sort_begin()
            batches = _batches(bam, 50)
            if sorting:
                assert bam.sort_finish()[0] == len(x["records"])
            else:
                st = bam.sort_stats()
                assert st["n_records"] == 0 and st["arena_bytes"] == 0 and st["n_slabs"] == 0
            both.append((batches, bam.read_names()))
        finally:
            bam.close()
    (a, names_a), (b, names_b) = both
    assert sorted(names_a) == sorted(names_b) and len(a) == len(b) > 2
    for p, q in zip(a, b):
        assert p.keys() == q.keys()
        for k in p:
            if k == "read_id":
                assert [names_a[i] for i in p[k].tolist()] == [names_b[i] for i in q[k].tolist()]
            else:
                assert np.array_equal(p[k], q[k]), k
