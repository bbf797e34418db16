"""The BAM index on the device (svx_bam_index_*, svim_amd/csrc/bamindex.hip fed by the device reader csrc/bamdev.hip): the bytes the kernels make equal, byte for
byte, what the host build of the same header makes (svx_bam_index_host) and what the definition says (svim_amd/bai.py; tests/test_bai.py holds both to
region queries) on every corner file of tests/bai_cases.py, whatever the chunks, the batches and the mode the pass reads with; the index is a by-product of
BamPipeline.run(); the sharded plan and seeks by its linear index find the records; the state rules hold; a reader that never begins an index is untouched."""
import ctypes as C
import types

import numpy as np
import pytest

import bai_cases as BC
from svim_amd import _abi, _lib, bai, harness, records, synth
from svim_amd.bamio import NativeBam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    """every corner file with its rows, the definition's bytes and the host build's, computed once"""
    d = str(tmp_path_factory.mktemp("bai_cases_gpu"))
    out = {}
    for name, path in BC.build_all(d) + [BC.many_references_file(d)]:
        n_ref, rows, v_end = bai.rows_of_bam(path)
        want = bai.build_index(n_ref, rows, v_end)
        assert _lib.bam_index_host(n_ref, rows, v_end) == want, name
        out[name] = dict(path=path, n_ref=n_ref, rows=rows, v_end=v_end, bytes=want)
    return out


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


def _device_index(path, **kw):
    bam = _open(path)
    try:
        bam.index_begin()
        n = _pass(bam, **kw)
        return bam.index_finish(), n, bam.index_stats()
    finally:
        bam.close()


def _set_chunk_blocks(monkeypatch, chunk_blocks):
    if chunk_blocks:
        monkeypatch.setenv("SVX_BAM_DEV_CHUNK_BLOCKS", chunk_blocks)          # (read when the handle switches device decode on)
    else:
        monkeypatch.delenv("SVX_BAM_DEV_CHUNK_BLOCKS", raising=False)


@pytest.mark.parametrize("chunk_blocks", ["1", "3", None])
def test_bam_index_bytes_equal_host_build_and_definition(corner, monkeypatch, chunk_blocks):
    """chunks of 1 and 3 blocks: records straddle chunk edges, their virtual offsets come from the blocks of the chunk before, a chunk's last vend from the next"""
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    for name, x in corner.items():
        got, n, st = _device_index(x["path"])
        assert n == len(x["rows"]), name
        assert got == x["bytes"], (name, chunk_blocks, len(got), len(x["bytes"]))
        assert st["n_rows"] == len(x["rows"]) and st["n_placed"] == sum(1 for r in x["rows"] if r[0] >= 0) and st["bytes_out"] == len(got), name
        ix = bai.parse_index(got)
        assert st["n_chunks"] == sum(len(c) for d in ix["bins"] for c in d.values()) and st["n_bins"] == sum(len(d) for d in ix["bins"]), name
        assert st["n_slots"] == sum(len(l) for l in ix["linear"]) and st["n_refs_with_rows"] == sum(1 for p in ix["pseudo"] if p), name
    assert corner["cg_tag_long_cigar"]["rows"][1][2] - corner["cg_tag_long_cigar"]["rows"][1][1] > 65535


def test_bam_index_bytes_do_not_depend_on_batches_or_mode(corner, monkeypatch):
    x = corner["straddle_two_and_three_blocks"]
    for chunk_blocks in ("3", None):
        _set_chunk_blocks(monkeypatch, chunk_blocks)
        for kw in (dict(batch_records=7), dict(batch_records=200000), dict(batch_records=7, min_mapq=60), dict(mode="queryname", batch_records=50), dict(mode="queryname")):
            got, n, _ = _device_index(x["path"], **kw)
            assert n == len(x["rows"]) and got == x["bytes"], (chunk_blocks, kw)


def test_bam_index_of_a_file_beyond_the_first_table(tmp_path, monkeypatch):
    """150 500 records in chunks of 40 blocks (about 41 000 records each): the row table starts at 65 536 rows and doubles twice with its rows kept; the scans
    over the rows run over many tiles; more chunk heads than the sort's one-workgroup form takes (16 384), so the sort runs its tiled passes"""
    path = str(tmp_path / "large.bam")
    m = BC.large_file(path)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert len(rows) == m == 150500 and n_ref == 4
    want = _lib.bam_index_host(n_ref, rows, v_end)              # (held to the definition on tables of this size in tests/test_bai.py)
    _set_chunk_blocks(monkeypatch, "40")
    got, n, st = _device_index(path, batch_records=60000)
    assert n == m and st["n_rows"] == m > 2 * 65536 and st["n_placed"] == 150000
    assert st["n_chunks"] > 16384 and st["n_refs_with_rows"] == 3
    assert got == want, (len(got), len(want))
    ix = bai.parse_index(got)
    assert ix["n_no_coor"] == 500 and ix["pseudo"][1] is None and st["n_chunks"] == sum(len(c) for d in ix["bins"] for c in d.values())
    assert max(len(c) for d in ix["bins"] for c in d.values()) > 1          # bins of several chunks: their file order is the sort's stability


def test_bam_index_cigars_around_the_span_kernels_thresholds(tmp_path):
    """CIGARs of 4096 operations (the row form's last), 4097 and 30 001 (a wave per record) and 65 535 (the most a record holds without a CG tag; the corner
    file cg_tag_long_cigar goes beyond, to the tiled form), between short ones"""
    recs, pos = [], 1000
    for k, n_ops in enumerate((3, 4096, 4097, 1, 30001, 4095, 65535, 2, 4098)):
        cig = [((0, 2, 0, 3, 7, 1, 8)[i % 7], 1 + i % 3) for i in range(n_ops)]
        recs.append(BC.seg("t%d" % k, 3, pos, cig, flag=(0, 16)[k % 2]))
        pos += 700
    path = str(tmp_path / "thresholds.bam")
    BC.write_file(path, BC.REFS, BC.LENS, BC.record_bytes(recs), 30011)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    want = bai.build_index(n_ref, rows, v_end)
    assert len({r[2] - r[1] for r in rows}) == len(rows) == 9
    got, n, st = _device_index(path)
    assert n == 9 and got == want == _lib.bam_index_host(n_ref, rows, v_end)
    assert st["n_long_cigars"] == 4


def test_bam_index_abort_gives_the_handle_back(corner):
    good = corner["record_at_block_start"]
    bam = _open(good["path"])
    try:
        with pytest.raises(_lib.SvxError) as e:
            bam.index_abort()                                              # nothing to give up
        assert _code(e) == _abi.SVX_E_STATE
        bam.index_begin()
        assert bam.read_batch(10, 20)[1] == 10
        bam.index_abort()                                                  # in the middle of the pass: the handle reads on where it was
        with pytest.raises(_lib.SvxError) as e:
            bam.index_bytes()
        assert _code(e) == _abi.SVX_E_STATE
        assert 10 + _pass(bam, 77) == len(good["rows"])
        with pytest.raises(_lib.SvxError) as e:
            bam.index_finish()
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()
        bam.index_begin()
        assert bam.read_batch(10, 20)[1] == 10
        bam.index_abort()
        bam.seek(good["rows"][5][4], -2)                                   # seek and rewind work again
        assert _pass(bam, 50) == len(good["rows"]) - 5
        bam.rewind()
        bam.index_begin()
        assert _pass(bam, 1000) == len(good["rows"]) and bam.index_finish() == good["bytes"]
    finally:
        bam.close()


def _sv_file(tmp_path, name="sv.bam"):
    contigs = [("chr1", 120000), ("chrE", 30000), ("chr2", 50000), ("chrN", 9000)]
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 300, refs, references, lengths, n_sites=20, types=("DEL", "INS", "INV"))
    recs += synth.planted_reads(9, 80, refs, references, lengths, n_sites=6, types=("DEL", "INS"), tid=2)
    recs += synth.fuzz_split_reads(6, 60, references, lengths)
    recs = synth.coordinate_sort(recs)
    path = str(tmp_path / name)
    records.write_bam(path, references, lengths, recs)
    return path, references, lengths, refs, recs


OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False)


def test_bam_index_is_a_by_product_of_the_pipeline_pass(eng, tmp_path):
    from svim_amd import convert
    path, references, lengths, refs, recs = _sv_file(tmp_path)
    o = types.SimpleNamespace(**OPTS)
    off, codes = convert.genome_arrays(refs, references)
    tabs = []
    for build_index in (False, True):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True, build_index=build_index)
        try:
            assert pipe.run() == len(recs)
            pipe.cluster(genome=(off, codes))
            tabs.append((eng.fetch_signatures(0), eng.fetch_signatures(1), eng.fetch_clusters(), pipe.bam.read_names()))
            if build_index:
                out = pipe.write_bai(str(tmp_path / "by_product.bai"))
                assert pipe.stats["index"]["n_rows"] == len(recs) and pipe.stats["t_index_finish_wall"] > 0
            else:
                with pytest.raises(ValueError):
                    pipe.write_bai()
        finally:
            pipe.close()
    (sig_a, bnd_a, clu_a, names_a), (sig_b, bnd_b, clu_b, names_b) = tabs
    for a, b in ((sig_a, sig_b), (bnd_a, bnd_b)):
        # (the reader numbers the reads of a chunk in the order its lanes meet them: the tables are the same up to that numbering, so read ids go through the names)
        assert a.n == b.n
        for k in list(_abi.SIG_DTYPES) + ["seq_off", "seq"]:
            if k == "read_id":
                assert [names_a[i] for i in a.read_id[:a.n].tolist()] == [names_b[i] for i in b.read_id[:b.n].tolist()]
            else:
                assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert clu_a.first_difference(clu_b) is None
    assert sig_a.n > 50 and clu_a.n > 5
    alone = harness.index_bam(path, 0, out=str(tmp_path / "alone.bai"))
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert open(out, "rb").read() == alone == open(str(tmp_path / "alone.bai"), "rb").read() == bai.build_index(n_ref, rows, v_end)
    stub = records.read_bai(path + ".bai")
    with pytest.raises(ValueError):
        harness.BamPipeline(path, o, eng, threads=2, build_index=True, regions=[(stub[0][0], 0)])
    with pytest.raises(ValueError):
        harness.BamPipeline(path, o, eng, threads=2, build_index=True, device_decode=False)


def _head_columns(bam, b):
    """tid, pos, flag of a device batch"""
    n = int(b.n_rec)
    out = []
    for name in ("tid", "pos", "flag"):
        a = np.zeros(n, dtype=_abi.BATCH_DTYPES[name])
        if n:
            assert bam.L.svx_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.cast(getattr(b, name), C.c_void_p), C.c_uint64(a.nbytes)) == 0
        out.append(a)
    return out


def test_bam_index_serves_the_shard_plan_and_seeks(tmp_path):
    import foreign_bam as FB
    refs, lens = BC.REFS, BC.LENS
    recs = BC.random_records(41, 900, (1, 3, 4), lens, n_unplaced=9, big_every=11)
    path = str(tmp_path / "served.bam")
    FB.write(path, refs, lens, BC.record_bytes(recs), layout="flat", block_payload=2500, tids=[a.reference_id for a in recs])      # (writes the stub index, too)
    data = harness.index_bam(path, 0, out=str(tmp_path / "served.device.bai"))
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert data == bai.build_index(n_ref, rows, v_end)
    mine, stub = records.read_bai(str(tmp_path / "served.device.bai")), records.read_bai(path + ".bai")
    assert mine == stub
    for world in (1, 2, 3):
        for rank in range(world):
            (owner_a, runs_a), (owner_b, runs_b) = harness.shard_plan(refs, lens, mine, rank, world), harness.shard_plan(refs, lens, stub, rank, world)
            assert list(owner_a) == list(owner_b) and runs_a == runs_b and (runs_a or world > 1)
    # seek to the linear index's lower bound of the region's first window, read forward until pos >= end
    ix = bai.parse_index(data)
    at = {r[4]: k for k, r in enumerate(rows)}
    bam = _open(path)
    found = 0
    try:
        for tid, beg, end in BC.regions(6, rows, n_ref, 200):
            want = bai.brute_force(rows, tid, beg, end)
            _, low = bai.query(ix, tid, beg, end)
            if low is None:
                assert not want
                continue
            k0 = at[low]                                                  # the seek point is a record start
            bam.seek(low, tid)
            got, done = [], False
            while not done:
                b, n = bam.read_batch(300, 0, "coordinate")
                if n == 0:
                    break
                t, p, f = _head_columns(bam, b)
                for i in range(n):
                    if p[i] >= end:
                        done = True
                        break
                    got.append((int(t[i]), int(p[i]), int(f[i]) & 0xfff))
            assert got == [(r[0], r[1], r[3] & 0xfff) for r in rows[k0:k0 + len(got)]], (tid, beg, end)
            ks = [at[r[4]] for r in want]
            assert all(k0 <= k < k0 + len(got) for k in ks), (tid, beg, end)          # every record the scan names, none in front of the seek point
            found += len(want)
    finally:
        bam.close()
    assert found > 300


def _code(excinfo):
    return getattr(excinfo.value, "code", None)


def test_bam_index_state_rules(corner, tmp_path):
    good = corner["record_at_block_start"]
    bam = _open(good["path"])
    try:
        with pytest.raises(_lib.SvxError) as e:
            bam.index_bytes()                                              # never begun
        assert _code(e) == _abi.SVX_E_STATE
        with pytest.raises(_lib.SvxError) as e:
            bam.index_finish()
        assert _code(e) == _abi.SVX_E_STATE
        assert bam.read_batch(10, 20)[1] == 10
        with pytest.raises(_lib.SvxError) as e:
            bam.index_begin()                                              # after a read
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()
        bam.index_begin()
        assert bam.read_batch(10, 20)[1] == 10
        for call in (bam.index_finish, bam.rewind, lambda: bam.seek(good["rows"][5][4], -2)):
            with pytest.raises(_lib.SvxError) as e:
                call()                                                     # finish before the end of the file; rewind and seek while indexing
            assert _code(e) == _abi.SVX_E_STATE
        assert 10 + _pass(bam, 77) == len(good["rows"])
        assert bam.index_finish() == good["bytes"] == bam.index_bytes()
        with pytest.raises(_lib.SvxError) as e:
            bam.index_finish()                                             # off again
        assert _code(e) == _abi.SVX_E_STATE
        bam.rewind()                                                       # a second begin / pass / finish on the same handle
        bam.index_begin()
        assert _pass(bam, 1000) == len(good["rows"]) and bam.index_finish() == good["bytes"]
    finally:
        bam.close()
    host = NativeBam(good["path"], threads=2)
    try:
        for call in (host.index_begin, host.index_finish, host.index_bytes):
            with pytest.raises(_lib.SvxError) as e:
                call()
            assert _code(e) == _abi.SVX_E_STATE
    finally:
        host.close()
    swapped, beyond = str(tmp_path / "swapped.bam"), str(tmp_path / "beyond.bam")
    BC.swapped_file(swapped)
    BC.beyond_range_file(beyond)
    for path, code in ((swapped, bai.E_ORDER), (beyond, bai.E_RANGE)):
        n_ref, rows, v_end = bai.rows_of_bam(path)
        for build in (bai.build_index, _lib.bam_index_host):
            with pytest.raises(bai.BaiError) as e:
                build(n_ref, rows, v_end)
            assert e.value.code == code
        bam = _open(path)
        try:
            bam.index_begin()
            assert _pass(bam) == len(rows)
            with pytest.raises(bai.BaiError) as e:
                bam.index_finish()
            assert e.value.code == code
            with pytest.raises(_lib.SvxError) as e:
                bam.index_bytes()
            assert _code(e) == _abi.SVX_E_STATE
            bam.rewind()                                                   # the handle still reads the file
            assert _pass(bam, 50) == len(rows)
        finally:
            bam.close()
    assert _device_index(good["path"])[0] == good["bytes"]


def test_bam_reader_without_an_index_is_untouched(corner):
    x = corner["empty_blocks_in_the_middle"]
    both = []
    for indexing in (False, True):
        bam = _open(x["path"])
        try:
            if indexing:
                bam.index_begin()
            batches = []
            while True:
                b, n = bam.read_batch(150, 20)
                if n == 0:
                    break
                batches.append(bam.batch_arrays(b))
            if indexing:
                assert bam.index_finish() == x["bytes"]
            else:
                with pytest.raises(_lib.SvxError) as e:
                    bam.index_bytes()
                assert _code(e) == _abi.SVX_E_STATE
                st = bam.index_stats()
                assert st["n_rows"] == 0 and st["bytes_out"] == 0
            both.append((batches, bam.read_names()))
        finally:
            bam.close()
    (a, names_a), (b, names_b) = both
    assert sorted(names_a) == sorted(names_b) and len(a) == len(b) > 2
    for p, q in zip(a, b):
        assert p.keys() == q.keys()
        for k in p:
            if k == "read_id":          # (the reader numbers the reads of a chunk in the order its lanes meet them: ids are compared through the names)
                assert [names_a[i] for i in p[k].tolist()] == [names_b[i] for i in q[k].tolist()]
            else:
                assert np.array_equal(p[k], q[k]), k
