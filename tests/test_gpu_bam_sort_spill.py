"""The spilled coordinate sort on the device (svx_bam_sort_begin_spill, svim_amd/csrc/bamsort.hip): runs formed at an arena limit, written to one unlinked spill
file, merged by one radix sort and read back range by range for every piece.  Held to the SAME expectations as the in-memory sort in
tests/test_gpu_bam_sort.py - the stream, the compressed file, the .bai and the permutation of the definition (svim_amd/bamsort.py) and of the host build -
never to itself: on every corner file of tests/bam_sort_cases.py at several limits, on the directed files of tests/bam_sort_spill_cases.py (stability across
runs, a run of one record, a run of unplaced records, in order / reversed / shuffled, a 225 kB record between small ones, 70 and 257 runs, the file's end on
a run edge), whatever the pieces, on the large shuffled file, through harness.sort_bam and sam_to_bam, and the state rules.

Every case first makes a pass without spilling to read arena_bytes and max_chunk_bytes, then sets max_bytes = max(max_chunk_bytes, arena_bytes // k)."""
import os
import stat

import numpy as np
import pytest

import bai_cases as BC
import bam_sort_cases as SC
import bam_sort_spill_cases as PC
import sam_cases
import test_gpu_bam_sort as G
from svim_amd import _abi, _lib, bai, bamsort, harness, sam as samdef
from svim_amd.bamio import NativeBam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_sort_spill_corner_gpu"))
    return {name: G._expect(x) for name, x in SC.build_all(d).items()}


@pytest.fixture(scope="module")
def directed(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_sort_spill_directed_gpu"))
    return {name: G._expect(x) for name, x in PC.build_directed(d).items()}


@pytest.fixture()
def spill_dir(tmp_path):
    d = tmp_path / "spill"
    d.mkdir()
    yield str(d)
    assert os.listdir(str(d)) == []                                   # whatever the test did: nothing is left behind


def _sizes(x):
    """(arena_bytes, max_chunk_bytes, n_slabs) of a pass that does not spill, under the chunk setting of the moment; the in-memory sort is checked on the way"""
    got = G._device_sort(x["path"])
    G._check(x, got, "in memory")
    bam = G._open(x["path"])
    try:
        bam.sort_begin()
        G._pass(bam)
        bam.sort_finish()
        sp = bam.sort_spill_stats()
    finally:
        bam.close()
    assert sp["n_runs"] == (1 if x["records"] else 0) and sp["spilled_bytes"] == 0 and sp["max_run_bytes"] == got[5]["arena_bytes"]
    return got[5]["arena_bytes"], sp["max_chunk_bytes"], got[5]["n_slabs"]


def _spilled_sort(path, max_bytes, spill_dir, piece_blocks=4096, **kw):
    """-> (stream, file, .bai, permutation, records read, stats), spill stats"""
    bam = G._open(path)
    try:
        bam.sort_begin(max_bytes, spill_dir)
        n = G._pass(bam, **kw)
        assert os.listdir(spill_dir) == []                            # (the spill file is unlinked while it is open)
        n_rec, n_bytes, n_blocks = bam.sort_finish()
        assert n_rec == n and n_blocks == bamsort.n_blocks(n_bytes)
        comp, raw = G._encode_all(bam, n_blocks, piece_blocks)
        return (raw, comp, bam.sort_index(), bam.sort_permutation(), n, bam.sort_stats()), bam.sort_spill_stats()
    finally:
        bam.close()


def _check_spill(x, got, sp, max_bytes, what):
    G._check(x, got, what)
    need = sum(len(r) for r in x["records"])
    if sp["n_runs"] > 1:
        assert sp["spilled_bytes"] == need and sp["max_run_bytes"] <= max_bytes and sp["readback_bytes"] >= need and sp["max_stage_bytes"] > 0, what
    else:
        assert sp["spilled_bytes"] == 0 and sp["readback_bytes"] == 0 and sp["max_stage_bytes"] == 0, what


@pytest.mark.parametrize("k", [2, 3, 7, None])
def test_spilled_sort_of_every_corner_file(corner, monkeypatch, spill_dir, k):
    """a chunk per BGZF block; k None: max_bytes = the largest chunk, a run wherever two chunks do not fit together"""
    G._set_chunk_blocks(monkeypatch, "1")
    for name, x in corner.items():
        sizes = x.setdefault("sizes", None) or _sizes(x)
        x["sizes"] = sizes
        arena, max_chunk, n_slabs = sizes
        max_bytes = max(max_chunk, arena // k) if k else max_chunk
        if max_bytes == 0:                                            # (no record: 0 would mean "what the device has free")
            max_bytes = 1
        got, sp = _spilled_sort(x["path"], max_bytes, spill_dir)
        _check_spill(x, got, sp, max_bytes, (name, k))
        assert sp["max_chunk_bytes"] == max_chunk, name
        if n_slabs > 1:
            assert sp["n_runs"] > 1, (name, k, sp)


def test_spilled_sort_of_the_directed_files(directed, monkeypatch, spill_dir):
    G._set_chunk_blocks(monkeypatch, "1")
    for name, x in directed.items():
        arena, max_chunk, n_slabs = _sizes(x)
        if x["n_runs"] is not None:
            assert max_chunk == PC.REC * x["group"] and arena % max_chunk == 0, name                  # every chunk one size: the limit makes the runs it says
        max_bytes = x["limit"] * max_chunk
        got, sp = _spilled_sort(x["path"], max_bytes, spill_dir, piece_blocks=x["piece_blocks"])
        _check_spill(x, got, sp, max_bytes, name)
        if x["n_runs"] is not None:
            assert sp["n_runs"] == x["n_runs"], (name, sp)
        assert sp["n_runs"] >= x["min_runs"], (name, sp)
        if x["piece_blocks"] == 1:
            assert got[5]["n_pieces"] == bamsort.n_blocks(len(x["stream"])) >= 5, name
    # what the files are named for
    x = directed["five_keys_300_names"]
    assert len({bamsort.sort_key(r[4:]) for r in x["records"]}) == 5 and [r[36:43] for r in x["records"]] == [b"%07d" % k for k in range(300)]
    same = [int(x["records"][k][36:43]) for k in x["perm"] if bamsort.sort_key(x["records"][k][4:]) == (1, 701, 0)]
    assert same == sorted(same) and same[-1] - same[0] > 200                               # one key's records come from runs all over the file, in file order
    x = directed["in_order_one_run_per_piece"]
    assert x["perm"].tolist() == list(range(6000))
    x = directed["long_record_between_small_ones"]
    at = np.cumsum([len(bamsort.sorted_header(x["header"]))] + [len(x["records"][k]) for k in x["perm"]])
    j = x["perm"].tolist().index(1000)
    assert len(x["records"][1000]) > 225000 and at[j] // bamsort.BLOCK + 3 <= at[j + 1] // bamsort.BLOCK and 200 < j < 1800


@pytest.mark.parametrize("piece_blocks", [1, 3, 4096])
@pytest.mark.parametrize("k", [2, 7])
def test_spilled_sort_does_not_depend_on_the_pieces(directed, monkeypatch, spill_dir, piece_blocks, k):
    G._set_chunk_blocks(monkeypatch, "1")
    x = directed["shuffled_every_piece_draws_on_every_run"]
    sizes = x.setdefault("sizes", None) or _sizes(x)
    x["sizes"] = sizes
    max_bytes = max(sizes[1], sizes[0] // k)
    got, sp = _spilled_sort(x["path"], max_bytes, spill_dir, piece_blocks=piece_blocks)
    _check_spill(x, got, sp, max_bytes, (piece_blocks, k))
    assert sp["n_runs"] >= min(k, 6) and got[5]["n_pieces"] == -(-bamsort.n_blocks(len(x["stream"])) // piece_blocks)


def test_spilled_sort_of_a_large_shuffled_file(tmp_path, monkeypatch, spill_dir):
    """the 150 500 records of the in-memory test, chunks of 40 blocks, an eighth of the records resident at a time; every run is written in many pieces"""
    x = SC.large_shuffled_file(str(tmp_path / "large_shuffled.bam"))
    body, perm = _lib.bam_sort_host(b"".join(x["records"]), x["n_ref"])
    stream = bamsort.sorted_header(x["header"]) + body
    G._set_chunk_blocks(monkeypatch, "40")
    monkeypatch.setenv("SVX_BAM_SORT_SPILL_PIECE_KB", "80")                 # (read at sort_begin) a run of about 2 MB leaves in pieces of 80 KiB: 5 tiles each
    bam = G._open(x["path"])
    try:
        bam.sort_begin()
        assert G._pass(bam, 60000) == 150500
        bam.sort_finish()
        arena, max_chunk = bam.sort_stats()["arena_bytes"], bam.sort_spill_stats()["max_chunk_bytes"]
        bam.sort_abort()
        bam.rewind()
        max_bytes = max(max_chunk, arena // 8)
        bam.sort_begin(max_bytes, spill_dir)
        assert G._pass(bam, 60000) == 150500
        n, n_bytes, n_blocks = bam.sort_finish()
        assert (n, n_bytes) == (150500, len(stream)) and n_blocks > 100
        assert (bam.sort_permutation() == perm).all()
        comp, raw = G._encode_all(bam, n_blocks, 64)
        assert raw == stream
        assert comp == _lib.text_gz_host(stream)
        index = bam.sort_index()
        st, sp = bam.sort_stats(), bam.sort_spill_stats()
    finally:
        bam.close()
    out = str(tmp_path / "large_sorted.bam")
    with open(out, "wb") as fh:
        fh.write(comp)
    n_ref, rows, v_end = bai.rows_of_bam(out)
    assert index == _lib.bam_index_host(n_ref, rows, v_end)
    assert sp["n_runs"] >= 4 and sp["spilled_bytes"] == arena == st["arena_bytes"] and sp["max_run_bytes"] <= max_bytes and st["n_pieces"] == -(-n_blocks // 64)
    # a piece, the two records that straddle its edges, and a pad of 64 bytes per run
    assert sp["max_stage_bytes"] <= 64 * bamsort.BLOCK + 2 * max(len(r) for r in x["records"]) + 64 * sp["n_runs"]


def test_spilled_sort_through_the_harness(tmp_path, monkeypatch, spill_dir):
    G._set_chunk_blocks(monkeypatch, "1")
    recs = BC.random_records(41, 900, (1, 3, 4), BC.LENS, n_unplaced=9, big_every=11)
    src = str(tmp_path / "shuffled.bam")
    SC.write_raw(src, SC.header(), SC.shuffled(BC.record_bytes(recs), 92), cuts=2500)
    plain, out = str(tmp_path / "in_memory.bam"), str(tmp_path / "spilled.bam")
    st0 = harness.sort_bam(src, plain, 0, piece_blocks=2)
    assert st0["spill"]["n_runs"] == 1 and st0["spill"]["spilled_bytes"] == 0
    max_bytes = max(st0["spill"]["max_chunk_bytes"], st0["arena_bytes"] // 5)
    st = harness.sort_bam(src, out, 0, piece_blocks=2, max_bytes=max_bytes, spill_dir=spill_dir)
    assert st["n_records"] == 909 and st["spill"]["n_runs"] >= 5 and os.listdir(spill_dir) == []
    want = bamsort.file(src)
    assert open(out, "rb").read() == want == open(plain, "rb").read()
    assert open(out + ".bai", "rb").read() == open(plain + ".bai", "rb").read() == bai.build_index(*bai.rows_of_bam(out))
    G._set_chunk_blocks(monkeypatch, None)                                  # (the device reader's batches end where its chunks end: one chunk)
    dev, host = G._open(out), NativeBam(out, threads=2)                     # read back by both readers
    try:
        a, b = G._batches(dev, 150), G._batches(host, 150)
        assert dev.sort_order == host.sort_order == "coordinate" and len(a) == len(b) == 7
        for p, q in zip(a, b):
            for key in ("tid", "pos", "flag"):
                assert np.array_equal(p[key], q[key]), key
    finally:
        dev.close()
        host.close()
    # without a spill directory the same limit is refused, as before
    with pytest.raises(_lib.SvxError) as e:
        harness.sort_bam(src, out + ".refused", 0, max_bytes=max_bytes)
    assert G._code(e) == _abi.SVX_E_CAPACITY and not os.path.exists(out + ".refused")


def test_spilled_sam_to_bam(tmp_path, monkeypatch, spill_dir):
    """SAM text in slices of 16 KiB, a quarter of the records resident at a time: the file and the index of the sort's definition on the definition's records"""
    text, _ = sam_cases.seeded_file(22, 1200)
    header, recs = samdef.convert(text)
    src, plain, out = str(tmp_path / "seeded.sam"), str(tmp_path / "in_memory.bam"), str(tmp_path / "spilled.bam")
    with open(src, "wb") as fh:
        fh.write(text)
    monkeypatch.setenv("SVX_SAM_DEV_CHUNK_BYTES", "16384")
    st0 = harness.sam_to_bam(src, plain)
    max_bytes = max(st0["spill"]["max_chunk_bytes"], st0["arena_bytes"] // 4)
    st = harness.sam_to_bam(src, out, max_bytes=max_bytes, spill_dir=spill_dir)
    assert st["spill"]["n_runs"] >= 3 and st["n_records"] == st0["n_records"] == 1200 and os.listdir(spill_dir) == []
    stream, _ = SC.definition(dict(records=recs, header=header, n_ref=len(sam_cases.REFS)))
    assert open(out, "rb").read() == _lib.text_gz_host(stream) == open(plain, "rb").read()
    assert open(out + ".bai", "rb").read() == bai.build_index(*bai.rows_of_bam(out)) == open(plain + ".bai", "rb").read()
    dev, host = G._open(out), NativeBam(out, threads=2)                     # read back by both readers
    try:
        a, b = G._batches(dev, 500), G._batches(host, 500)
        assert host.sort_order == "coordinate" and sum(len(p["tid"]) for p in a) == 1200
        for p, q in zip(a, b):
            for key in ("tid", "pos", "flag"):
                assert np.array_equal(p[key], q[key]), key
    finally:
        dev.close()
        host.close()


def test_spilled_sort_state_rules(corner, monkeypatch, tmp_path, spill_dir):
    G._set_chunk_blocks(monkeypatch, "1")
    good = corner["blocks_cut_records_anywhere"]
    n_all = len(good["records"])
    arena, max_chunk, n_slabs = _sizes(good)
    assert n_slabs >= 4
    bam = G._open(good["path"])
    try:
        # a spill directory that does not exist, is a file, or cannot be written to
        missing, a_file, locked = str(tmp_path / "missing"), str(tmp_path / "a_file"), str(tmp_path / "locked")
        open(a_file, "w").close()
        os.mkdir(locked)
        os.chmod(locked, stat.S_IRUSR | stat.S_IXUSR)
        for d in (missing, a_file, "") + ((locked,) if os.geteuid() != 0 else ()):
            with pytest.raises(bamsort.BamSortError) as e:
                bam.sort_begin(max_chunk, d)
            assert G._code(e) == _abi.SVX_E_ARG, d
        os.chmod(locked, stat.S_IRWXU)
        # max_bytes below one chunk: SVX_E_CAPACITY, the sort is dropped, a clean rewind and a good sort
        bam.sort_begin(max_chunk - 1, spill_dir)
        with pytest.raises(_lib.SvxError) as e:
            G._pass(bam, 50)
        assert G._code(e) == _abi.SVX_E_CAPACITY and os.listdir(spill_dir) == []
        with pytest.raises(bamsort.BamSortError) as e:
            bam.sort_finish()
        assert G._code(e) == _abi.SVX_E_STATE
        bam.rewind()
        bam.sort_begin(max_chunk, spill_dir)
        assert G._pass(bam, 50) == n_all
        _, _, n_blocks = bam.sort_finish()
        assert bam.sort_spill_stats()["n_runs"] > 1 and bam.sort_encode(0, n_blocks) == good["file"]
        bam.sort_abort()
        assert os.listdir(spill_dir) == []
        # abort in the middle of the pass, after the first run was closed; the handle reads on, then reads the whole file plainly
        bam.rewind()
        bam.sort_begin(max_chunk, spill_dir)
        n = 0
        while bam.sort_spill_stats()["n_runs"] < 1:
            k = bam.read_batch(20, 20)[1]
            assert k > 0
            n += k
        assert 0 < n < n_all and bam.sort_spill_stats()["spilled_bytes"] > 0 and os.listdir(spill_dir) == []
        bam.sort_abort()
        assert os.listdir(spill_dir) == []
        assert n + G._pass(bam, 77) == n_all
        bam.rewind()
        assert G._pass(bam, 500) == n_all
        # without a spill directory the limit is what it was: SVX_E_CAPACITY
        bam.rewind()
        bam.sort_begin(arena - 1)
        with pytest.raises(_lib.SvxError) as e:
            G._pass(bam, 50)
        assert G._code(e) == _abi.SVX_E_CAPACITY
        # a sort that spills nothing: one run, no file, the same bytes
        bam.rewind()
        bam.sort_begin(arena, spill_dir)
        assert G._pass(bam, 50) == n_all
        _, _, n_blocks = bam.sort_finish()
        sp = bam.sort_spill_stats()
        assert sp["n_runs"] == 1 and sp["spilled_bytes"] == 0 and sp["max_run_bytes"] == arena and bam.sort_encode(0, n_blocks) == good["file"]
        # a second spilled sort on the same handle, and the handle closed while the spill file is open
        bam.rewind()
        bam.sort_begin(max_chunk, spill_dir)
        assert G._pass(bam, 1000) == n_all
        bam.sort_finish()
        assert bam.sort_spill_stats()["n_runs"] > 1
    finally:
        bam.close()
    assert os.listdir(spill_dir) == []
