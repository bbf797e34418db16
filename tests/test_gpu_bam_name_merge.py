"""A merge session in query-name order on the device (svx_bam_merge_open_order; csrc/bamsort.hip: runs closed in name order, k_ns_pack, k_ns_keys_tab): the
stream, the compressed file and the permutation equal, byte for byte, what the definition says (svim_amd/bammerge.py, order="queryname";
tests/test_bam_name_merge.py holds it and the host build to each other) - in memory, and spilled at arenas of a half, a third and a seventh of the records,
always held to the IN-MEMORY path's expectations (definition and host build), never to the spilled path itself.  A test that means to spill asserts the runs
from the spill stats: one that meant to spill and did not fails.  Every refusal here is a status returned by host code."""
import os
import types
import zlib

import numpy as np
import pytest

import bam_name_merge_cases as NM
import bam_name_sort_cases as NC
import foreign_bam as FB
from svim_amd import _abi, _lib, bammerge, bamsort, harness, records, synth
from svim_amd.bamio import BamMerge, NativeBam

pytestmark = pytest.mark.gpu
MAX_ROUNDS = 64


def _expect(c):
    """the definition's stream, file and permutation of a case (or its refusal) and the host build's agreement"""
    if "error" in c:
        return c
    c["stream"], perm = NM.definition(c)
    c["perm"] = np.asarray(perm, dtype=np.uint32)
    c["file"] = _lib.text_gz_host(c["stream"])
    hdr, maps = _lib.bam_merge_header_host([x["header"] for x in c["inputs"]], "queryname")
    n_ref = len(bammerge.parse_header(hdr)[1])
    body, host_perm = _lib.bam_merge_host([(b"".join(x["records"]), x["n_ref"], m) for x, m in zip(c["inputs"], maps)], n_ref, "queryname")
    assert hdr + body == c["stream"] and (host_perm == c["perm"]).all()
    c["bytes"] = sum(len(r) for x in c["inputs"] for r in x["records"])
    return c


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_name_merge_cases_gpu"))
    return {name: _expect(c) for name, c in NM.build_all(d).items()}


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


@pytest.fixture()
def spill(tmp_path):
    d = str(tmp_path / "spill")
    os.mkdir(d)
    return d


def _open(path):
    bam = NativeBam(path, threads=2)
    bam.set_device_decode(0)
    return bam


def _set_chunk_blocks(monkeypatch, chunk_blocks):
    if chunk_blocks:
        monkeypatch.setenv("SVX_BAM_DEV_CHUNK_BLOCKS", chunk_blocks)          # (read when the handle switches device decode on)
    else:
        monkeypatch.delenv("SVX_BAM_DEV_CHUNK_BLOCKS", raising=False)


def _code(excinfo):
    return getattr(excinfo.value, "code", None)


def _encode_all(m, n_blocks, piece_blocks=4096):
    comp, raw = [], []
    for first in range(0, n_blocks, piece_blocks):
        c, r = m.encode(first, min(piece_blocks, n_blocks - first), stream=True)
        comp.append(c), raw.append(r)
    return b"".join(comp), b"".join(raw)


def _device_merge(paths, piece_blocks=4096, order="queryname", watch=None, **kw):
    """-> (stream, file, permutation, stats, name stats); the readers are closed as soon as they have fed.  watch: a directory that must stay empty all along"""
    readers = [_open(p) for p in paths]
    m = None
    try:
        m = BamMerge.open(readers, device=0, order=order, **kw)
        for r in readers:
            m.add(r)
            r.close()
            assert watch is None or os.listdir(watch) == []
        n_rec, n_bytes, n_blocks = m.finish()
        assert n_blocks == bamsort.n_blocks(n_bytes) and (watch is None or os.listdir(watch) == [])
        comp, raw = _encode_all(m, n_blocks, piece_blocks)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.index()                                                      # every block encoded: still no index of a query-name-sorted file
        assert _code(e) == _abi.SVX_E_STATE
        st, ns = m.stats(), m.name_stats()
        assert st["n_records"] == n_rec == ns["n_records"] and st["key_bits"] == 0
        return raw, comp, m.permutation(), st, ns
    finally:
        if m is not None:
            m.close()
        for r in readers:
            r.close()
        assert watch is None or os.listdir(watch) == []


def _check(c, got, what):
    raw, comp, perm, st, ns = got
    assert raw == c["stream"], (what, len(raw), len(c["stream"]))
    assert comp == c["file"], (what, len(comp), len(c["file"]))
    assert (perm == c["perm"]).all(), (what, np.flatnonzero(perm != c["perm"])[:5])
    assert st["arena_bytes"] == c["bytes"] and st["merge"]["n_added"] == len(c["inputs"]), what
    assert ns["rounds"] <= MAX_ROUNDS and ns["active_total"] == sum(ns["active_rows"]), what


def _spilling(cases):
    return [(name, c) for name, c in cases.items() if "error" not in c and name.split(":")[0] in ("split", "ties", "dict")]


@pytest.mark.parametrize("chunk_blocks, piece_blocks", [("1", 1), (None, 4096)])
def test_name_merge_in_memory_equals_the_definition(cases, monkeypatch, chunk_blocks, piece_blocks):
    """every split, ties and dictionaries case and the accepted header cases: session stream, compressed file and permutation are the definition's and the host
    build's; the refused header cases leave at open; nothing is spilled, no table is made"""
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    n_translated = 0
    for name, c in cases.items():
        paths = [x["path"] for x in c["inputs"]]
        if name.startswith("header:") and "error" in c:
            with pytest.raises(bammerge.BamMergeError) as e:
                _device_merge(paths)
            assert _code(e) == _abi.SVX_E_ARG, name
            continue
        if "error" in c or name.startswith("edge:"):
            continue
        got = _device_merge(paths, piece_blocks)
        _check(c, got, (name, chunk_blocks))
        st, ns = got[3], got[4]
        assert st["spill"]["spilled_bytes"] == 0 and st["spill"]["n_runs"] <= 1, name
        assert ns["spill"] == dict(n_runs=0, run_rounds=0, run_active_rows=0, table_bytes=0, t_run_sort_ms=0.0, t_pack_ms=0.0), name
        n_translated += st["merge"]["n_translated_records"]
    assert n_translated > 500


@pytest.mark.parametrize("k", [2, 3, 7])
def test_name_merge_spilled_equals_the_in_memory_expectations(cases, monkeypatch, spill, k):
    """the same cases at max_bytes = max(max_chunk_bytes, arena_bytes // k), read a block at a time: a run wherever two chunks do not fit together"""
    _set_chunk_blocks(monkeypatch, "1")
    n_spilled = 0
    for name, c in _spilling(cases):
        paths = [x["path"] for x in c["inputs"]]
        if c["bytes"] == 0:
            continue
        if "max_chunk_bytes" not in c:
            c["max_chunk_bytes"] = _device_merge(paths)[3]["spill"]["max_chunk_bytes"]
        max_bytes = max(c["max_chunk_bytes"], c["bytes"] // k)
        got = _device_merge(paths, 4096 if k != 3 else 1, max_bytes=max_bytes, spill_dir=spill, watch=spill)
        _check(c, got, (name, k))
        sp, nsp = got[3]["spill"], got[4]["spill"]
        if max_bytes < c["bytes"]:                                         # (a file of one chunk cannot spill)
            assert sp["n_runs"] >= 2 and sp["spilled_bytes"] == c["bytes"] and sp["max_run_bytes"] <= max_bytes, (name, sp)
            assert nsp["n_runs"] == sp["n_runs"] and nsp["table_bytes"] >= 4 * got[3]["n_records"], (name, nsp)
            n_spilled += 1
        else:
            assert sp["n_runs"] <= 1 and nsp["table_bytes"] == 0, name
    assert n_spilled >= len(_spilling(cases)) - 8                          # (no_records and one_record, dealt into 2 and 3 files, are the cases of one chunk)


def test_name_merge_run_edges_inside_a_file_and_on_a_file_boundary(cases, monkeypatch, spill):
    c = cases["dict:reversed_dictionary"]
    paths = [x["path"] for x in c["inputs"]]
    size = [sum(len(r) for r in x["records"]) for x in c["inputs"]]
    _set_chunk_blocks(monkeypatch, "1")
    got = _device_merge(paths, max_bytes=size[0] + size[1] // 2, spill_dir=spill, watch=spill)
    _check(c, got, "a run ends inside the second file")
    sp = got[3]["spill"]
    assert sp["n_runs"] == 2 and size[0] < sp["max_run_bytes"] <= size[0] + size[1] // 2 and sp["spilled_bytes"] == sum(size), sp
    _set_chunk_blocks(monkeypatch, None)
    assert max(size) < sum(size)
    got = _device_merge(paths, max_bytes=max(size), spill_dir=spill, watch=spill)
    _check(c, got, "a run ends on the file boundary")
    sp = got[3]["spill"]
    assert sp["n_runs"] == 2 and sp["max_run_bytes"] == max(size) and sp["spilled_bytes"] == sum(size), sp
    assert got[4]["spill"]["n_runs"] == 2 and got[4]["spill"]["table_bytes"] > 0


def test_name_merge_directed_run_edge_files(cases, monkeypatch, spill):
    """every run-edge file of bam_name_merge_cases, a BGZF block per group and an arena of one group: the neighbours the case names sit in different runs"""
    _set_chunk_blocks(monkeypatch, "1")
    seen = 0
    for name, c in cases.items():
        if not name.startswith("edge:"):
            continue
        got = _device_merge([c["inputs"][0]["path"]], 1 if seen & 1 else 4096, max_bytes=c["max_bytes"], spill_dir=spill, watch=spill)
        _check(c, got, name)
        sp, nsp = got[3]["spill"], got[4]["spill"]
        assert sp["n_runs"] >= c["min_runs"] >= 2 and sp["spilled_bytes"] == c["bytes"], (name, sp, c["min_runs"])
        assert nsp["n_runs"] == sp["n_runs"] and nsp["table_bytes"] >= 4 * got[3]["n_records"], (name, nsp)
        if name == "edge:run_edge_64_rounds":
            assert got[4]["rounds"] == MAX_ROUNDS and got[4]["active_rows"][-1] == 4, got[4]      # the merge's rounds: both pairs open to the last word
        if name == "edge:run_edge_257_runs":
            assert sp["n_runs"] >= 257
        seen += 1
    assert seen == 10


def test_name_merge_of_the_large_shuffled_file_in_eight_runs(tmp_path, monkeypatch, spill):
    """150 500 short records dealt into 2 files, read in chunks of 40 blocks, an arena of an eighth: the rank pass and the rounds of the merge over many tiles,
    the table over many runs"""
    x = NC.large_shuffled_file(str(tmp_path / "large_shuffled.bam"))
    recs = list(x["records"])
    parts = [recs[0::2], recs[1::2]]
    paths = [str(tmp_path / ("large_%d.bam" % f)) for f in range(2)]
    for p, part in zip(paths, parts):
        raw = x["header"] + b"".join(part)
        with open(p, "wb") as fh:
            for lo in range(0, len(raw), 0xff00):
                fh.write(FB.bgzf_block(raw[lo:lo + 0xff00], 1, zlib.Z_DEFAULT_STRATEGY))
            fh.write(FB.EOF_BLOCK)
    n_ref = x["n_ref"]
    body, perm = _lib.bam_merge_host([(b"".join(part), n_ref, list(range(n_ref))) for part in parts], n_ref, "queryname")      # (held to the definition in tests/test_bam_name_merge.py)
    stream = bammerge.merged_header([x["header"]] * 2, "queryname") + body
    total = len(body)
    _set_chunk_blocks(monkeypatch, "40")
    first = _device_merge(paths)
    assert first[0] == stream and (first[2] == perm).all()
    max_bytes = max(first[3]["spill"]["max_chunk_bytes"], total // 8)
    raw, comp, got_perm, st, ns = _device_merge(paths, 64, max_bytes=max_bytes, spill_dir=spill, watch=spill)
    assert (got_perm == perm).all(), np.flatnonzero(got_perm != perm)[:5]
    assert raw == stream and comp == _lib.text_gz_host(stream)
    assert st["spill"]["n_runs"] >= 2 and st["spill"]["spilled_bytes"] == total and ns["spill"]["n_runs"] == st["spill"]["n_runs"], st["spill"]
    assert ns["active_rows"][0] == 150500 and ns["rounds"] == first[4]["rounds"] and ns["active_rows"] == first[4]["active_rows"]


def test_name_merge_of_one_file_is_the_name_sort_spilled_too(cases, tmp_path, monkeypatch, spill):
    """a session over one file is sort_bam(order="queryname") of that file byte for byte - in memory with the same rounds, and with a spill directory beyond
    the arena, which sort_bam refuses"""
    x = cases["split:long_shared_prefix/2"]["one"]
    need = sum(len(r) for r in x["records"])
    out, merged, spilled = (str(tmp_path / n) for n in ("sorted.bam", "merged.bam", "spilled.bam"))
    st0 = harness.sort_bam(x["path"], out, 0, order="queryname")
    st1 = harness.merge_bam([x["path"]], merged, 0, order="queryname")
    assert open(out, "rb").read() == open(merged, "rb").read() and not os.path.exists(merged + ".bai") and not os.path.exists(merged + ".csi")
    for key in ("n_records", "word_bytes", "rounds", "active_total", "active_max", "active_rows"):
        assert st1["name"][key] == st0["name"][key], key
    assert st1["name_spill"]["n_runs"] == 0 and st1["name_spill"]["table_bytes"] == 0 and st1["merge"]["n_files"] == 1
    _set_chunk_blocks(monkeypatch, "1")
    with pytest.raises(ValueError):
        harness.sort_bam(x["path"], spilled, 0, order="queryname", spill_dir=spill)
    st2 = harness.merge_bam([x["path"]], spilled, 0, order="queryname", spill_dir=spill, max_bytes=need // 4)
    assert st2["spill"]["n_runs"] >= 2 and st2["name_spill"]["n_runs"] == st2["spill"]["n_runs"] and st2["name_spill"]["table_bytes"] > 0, st2["spill"]
    assert open(out, "rb").read() == open(spilled, "rb").read() and os.listdir(spill) == []
    assert st2["name"]["rounds"] == st0["name"]["rounds"] and st2["name"]["active_rows"] == st0["name"]["active_rows"]
    for kw in (dict(index=True), dict(index_format="bai"), dict(index_format="csi")):
        with pytest.raises(ValueError):
            harness.merge_bam([x["path"]], merged + ".no", 0, order="queryname", **kw)
        assert not os.path.exists(merged + ".no")
    with pytest.raises(ValueError):
        harness.merge_bam([x["path"]], merged + ".no", 0, order="natural")


def test_name_merge_refusals_in_memory_and_long_after_the_run_was_closed(cases, monkeypatch, spill):
    """the refused cases with their codes and precedence: in memory at finish; with an arena of 1 000 bytes over blocks of 600 the bad record's run is closed - and refused,
    by the host, from the status word - many runs before finish, a position below -1 waits for finish and stays behind every SVX_E_ARG.  A failed add
    breaks the session; the reader works after rewind"""
    _set_chunk_blocks(monkeypatch, "1")
    seen = 0
    for name, c in cases.items():
        if not name.startswith("refused:"):
            continue
        paths = [x["path"] for x in c["inputs"]]
        with pytest.raises(bammerge.BamMergeError) as e:
            _device_merge(paths)
        assert _code(e) == c["error"], name
        with pytest.raises(bammerge.BamMergeError) as e:
            _device_merge(paths, max_bytes=1000, spill_dir=spill, watch=spill)
        assert _code(e) == c["error"], name
        seen += 1
    assert seen == 3
    c = cases["refused:no_name_in_the_second_file_and_pos_below_in_the_first"]
    ra, rb = (_open(x["path"]) for x in c["inputs"])
    m = BamMerge.open([ra, rb], device=0, order="queryname", max_bytes=1000, spill_dir=spill)
    try:
        m.add(ra)                                                          # pos < -1 in closed runs: not yet
        assert m.stats()["spill"]["n_runs"] >= 2
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(rb)                                                      # the run that holds the record without a name closes inside this add
        assert _code(e) == _abi.SVX_E_ARG
        for call in (lambda: m.add(rb), m.finish, m.count, lambda: m.encode(0, 1), m.index, m.permutation):
            with pytest.raises(bammerge.BamMergeError) as e:
                call()
            assert _code(e) == _abi.SVX_E_STATE
        rb.rewind()
        n = 0
        while True:
            got = rb.read_batch(500, 20)[1]
            if not got:
                break
            n += got
        assert n == len(c["inputs"][1]["records"]) and os.listdir(spill) == []
    finally:
        m.close()
        ra.close()
        rb.close()
    assert os.listdir(spill) == []


def _sorted_alone(bam, order):
    bam.rewind()
    bam.sort_begin(order=order)
    while bam.read_batch(5000, 20)[1]:
        pass
    _, _, n_blocks = bam.sort_finish()
    return bam.sort_encode(0, n_blocks)


def test_name_merge_state_and_life_cycle(cases, monkeypatch, spill):
    """open refuses any other order; readers that fed sort alone and are closed before and after the session; a coordinate session on the same readers after
    rewind gives the coordinate merge"""
    c = cases["dict:reversed_dictionary"]
    a, b = (x["path"] for x in c["inputs"])
    want_a = bamsort.file(a, "queryname")
    want_b = bamsort.file(b)
    coordinate = bammerge.stream_of(NM.raws(c))[0]
    size = [sum(len(r) for r in x["records"]) for x in c["inputs"]]
    _set_chunk_blocks(monkeypatch, "1")
    ra, rb = _open(a), _open(b)
    m = m2 = None
    try:
        with pytest.raises(ValueError):
            BamMerge.open([ra, rb], device=0, order="natural")
        import ctypes as C
        arr, h = (C.c_void_p * 2)(ra.h, rb.h), C.c_void_p()
        assert ra.L.svx_bam_merge_open_order(arr, C.c_int64(2), C.c_int(0), C.c_int64(0), None, C.c_int(2), C.byref(h)) == _abi.SVX_E_ARG
        m = BamMerge.open([ra, rb], device=0, order="queryname", max_bytes=size[0] // 2 + 1, spill_dir=spill)
        assert m.name_stats()["rounds"] == 0
        m.add(ra)
        assert _sorted_alone(ra, "queryname") == want_a                    # fed, then sorts alone in name order while the session holds runs of it
        m.add(rb)
        assert _sorted_alone(rb, "coordinate") == want_b
        rb.close()                                                         # closed before the session finishes
        _, _, n_blocks = m.finish()
        comp, raw = _encode_all(m, n_blocks)
        assert raw == c["stream"] and comp == c["file"] and (m.permutation() == c["perm"]).all() and m.stats()["spill"]["n_runs"] >= 3
        for fmt in ("bai", "csi"):
            with pytest.raises(bammerge.BamMergeError) as e:
                m.index(fmt)
            assert _code(e) == _abi.SVX_E_STATE
        m.close()                                                          # the session first, the reader that fed it after it
        assert os.listdir(spill) == []
        assert _sorted_alone(ra, "queryname") == want_a
        ra.rewind()
        rb = _open(b)
        m2 = BamMerge.open([ra, rb], device=0)                             # a coordinate session on the same readers
        m2.add(ra)
        m2.add(rb)
        _, _, n_blocks = m2.finish()
        comp, raw = _encode_all(m2, n_blocks)
        assert raw == coordinate and len(m2.index()) > 8 and m2.name_stats()["rounds"] == 0 and m2.name_stats()["spill"]["n_runs"] == 0
    finally:
        for s in (m, m2):
            if s is not None:
                s.close()
        ra.close()
        rb.close()


def _query_batches(bam, batch_records):
    rows = []
    while True:
        b, n = bam.read_batch(batch_records, 20, "queryname")
        if n == 0:
            return rows
        A, names = bam.batch_arrays(b), bam.read_names()
        for i in range(n):
            s0, s1 = int(A["seg_off"][i]), int(A["seg_off"][i + 1])
            rows.append((names[int(A["read_id"][i])], int(A["flag"][i]), int(A["tid"][i]), int(A["pos"][i]), int(A["order"][i]) if not A["flag"][i] & 0x8000 else -1,
                         tuple(zip(A["seg_tid"][s0:s1].tolist(), A["seg_pos"][s0:s1].tolist()))))


def test_name_merged_file_round_trip_in_query_name_mode(cases, tmp_path, monkeypatch, spill):
    """the session's file of the duplicated reads dealt round-robin into three files, spilled: read back in query-name mode by the device reader it gives the
    groups of the definition's file read through the host reader - every read once, its primary with its supplementary record"""
    c = cases["ties:duplicated_reads/3"]
    paths = [x["path"] for x in c["inputs"]]
    dev_out, def_out = str(tmp_path / "device.bam"), str(tmp_path / "definition.bam")
    _set_chunk_blocks(monkeypatch, "1")
    st = harness.merge_bam(paths, dev_out, 0, order="queryname", spill_dir=spill, max_bytes=c["bytes"] // 3, piece_blocks=1)
    assert st["n_records"] == 120 and st["spill"]["n_runs"] >= 2 and not os.path.exists(dev_out + ".bai") and not os.path.exists(dev_out + ".csi")
    with open(def_out, "wb") as fh:
        fh.write(bammerge.file(paths, "queryname"))
    assert open(dev_out, "rb").read() == open(def_out, "rb").read() == c["file"]
    _set_chunk_blocks(monkeypatch, None)
    dev, host = _open(dev_out), NativeBam(def_out, threads=2)
    try:
        assert dev.sort_order == host.sort_order == "queryname"
        a, b = _query_batches(dev, 11), _query_batches(host, 11)
    finally:
        dev.close()
        host.close()
    assert a == b and len(a) == 120 and [r[0] for r in a] == ["name%02d" % (k // 3) for k in range(120)]
    live = [r for r in a if not r[1] & 0x8000]
    assert len(live) > 50 and sum(len(r[5]) for r in a) == len(live) // 2 > 25


OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False)


def test_pipeline_on_a_list_in_query_name_mode_merges_by_name(eng, tmp_path):
    """BamPipeline(parts, merged_out=..., mode="queryname") merges in query-name order: the merged file is the definition's, and the signatures and clusters
    are those of BamPipeline(definition's file, mode="queryname") - the groups of a read whose records lie in different files are whole"""
    from svim_amd import convert
    contigs = [("chr1", 120000), ("chr2", 50000)]
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 300, refs, references, lengths, n_sites=20, types=("DEL", "INS", "INV"))
    recs += synth.fuzz_split_reads(6, 80, references, lengths)
    parts = [str(tmp_path / ("part_%d.bam" % f)) for f in range(3)]
    for f, p in enumerate(parts):
        records.write_bam(p, references, lengths, synth.coordinate_sort(recs[f::3]))      # a read's records are dealt over the files
    merged_def, merged_pipe = str(tmp_path / "merged_definition.bam"), str(tmp_path / "merged_pipeline.bam")
    with open(merged_def, "wb") as fh:
        fh.write(bammerge.file(parts, "queryname"))
    o = types.SimpleNamespace(**OPTS)
    off, codes = convert.genome_arrays(refs, references)
    tables = []
    for path, kw in ((merged_def, {}), (parts, dict(merged_out=merged_pipe))):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=211, device_decode=True, mode="queryname", **kw)
        try:
            assert pipe.run() == len(recs)
            names, sig = pipe.bam.read_names(), eng.fetch_signatures(0)
            rows = sorted((int(sig.type[i]), int(sig.contig[i]), int(sig.start[i]), int(sig.end[i]), int(sig.contig2[i]), int(sig.pos2[i]), names[int(sig.read_id[i])], sig.sequence(i))
                          for i in range(sig.n))
            pipe.cluster(genome=(off, codes))
            tables.append((rows, eng.fetch_clusters()))
        finally:
            pipe.close()
    assert open(merged_pipe, "rb").read() == open(merged_def, "rb").read() and not os.path.exists(merged_pipe + ".bai")
    assert tables[0][0] == tables[1][0] and len(tables[0][0]) > 50
    assert tables[0][1].n == tables[1][1].n > 5 and not tables[0][1].first_difference(tables[1][1], rtol=1e-12)
    with pytest.raises(ValueError):
        harness.BamPipeline(parts, o, eng, mode="queryname")               # a list needs merged_out
