"""Several BAM files merged on the device (svx_bam_merge_*: the session of csrc/bamio.cpp and csrc/bammerge.hip, k_bs_translate in csrc/bamsort.hip): the stream,
the compressed file, the .bai, the .csi and the permutation equal, byte for byte, what the definition says (svim_amd/bammerge.py; tests/test_bam_merge.py holds it
and the host build to each other) on every case of tests/bam_merge_cases.py, at reader chunks of one BGZF block and at the default; the key over the merged
dictionary and the range checks over the file's own; runs that end inside a file and on a file boundary; one file = sort_bam; the state rules; the life cycle
of readers that feed a session and then sort on their own or are closed, each order once; a SAM text reader in a session; merge_bam, BamPipeline and run_bam on a list; a reader that never
feeds is untouched."""
import os
import struct
import types

import numpy as np
import pytest

import bam_merge_cases as MC
import bam_sort_cases as SC
import sam_cases as SAMC
from svim_amd import _abi, _lib, bai, bammerge, bamsort, csi, harness, records, sam, synth
from svim_amd.bamio import BamMerge, NativeBam

pytestmark = pytest.mark.gpu


def _expect(c, tag):
    """the definition's stream, file, indexes and permutation of a case (or its refusal), and the host build's agreement"""
    if "error" in c:
        with pytest.raises(bammerge.BamMergeError) as e:
            MC.definition(c)
        assert e.value.code == c["error"]
        return c
    c["stream"], perm = MC.definition(c)
    c["perm"] = np.asarray(perm, dtype=np.uint32)
    c["file"] = _lib.text_gz_host(c["stream"])
    tmp = c["inputs"][0]["path"] + "." + tag + ".definition"
    with open(tmp, "wb") as fh:
        fh.write(c["file"])
    n_ref, rows, v_end = bai.rows_of_bam(tmp)
    os.remove(tmp)
    c["bai"], c["csi"] = bai.build_index(n_ref, rows, v_end), csi.build_bam_index(n_ref, rows, v_end)
    headers = [x["header"] for x in c["inputs"]]
    hdr, maps = _lib.bam_merge_header_host(headers)
    body, host_perm = _lib.bam_merge_host([(b"".join(x["records"]), x["n_ref"], m) for x, m in zip(c["inputs"], maps)], n_ref)
    assert hdr + body == c["stream"] and (host_perm == c["perm"]).all()
    return c


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam_merge_cases_gpu"))
    return {name: _expect(c, "k%d" % k) for k, (name, c) in enumerate(MC.build_all(d).items())}


@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


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


def _device_merge(paths, piece_blocks=4096, fmt="bai", both_indexes=False, **kw):
    """-> (stream, file, index or (.bai, .csi), permutation, stats); the readers are closed as soon as they have fed"""
    readers = [_open(p) for p in paths]
    m = None
    try:
        m = BamMerge.open(readers, device=0, **kw)
        for r in readers:
            m.add(r)
            r.close()
        n_rec, n_bytes, n_blocks = m.finish()
        assert n_blocks == bamsort.n_blocks(n_bytes)
        comp, raw = _encode_all(m, n_blocks, piece_blocks)
        index = (m.index("bai"), m.index("csi")) if both_indexes else m.index(fmt)
        st = m.stats()
        assert st["n_records"] == n_rec
        return raw, comp, index, m.permutation(), st
    finally:
        if m is not None:
            m.close()
        for r in readers:
            r.close()


def _check(c, got, what):
    raw, comp, (index_bai, index_csi), perm, st = got
    assert raw == c["stream"], (what, len(raw), len(c["stream"]))
    assert comp == c["file"], (what, len(comp), len(c["file"]))
    assert index_bai == c["bai"] and index_csi == c["csi"], what
    assert (perm == c["perm"]).all(), what
    assert st["arena_bytes"] == sum(len(r) for x in c["inputs"] for r in x["records"]) and st["merge"]["n_added"] == len(c["inputs"]), what


@pytest.mark.parametrize("chunk_blocks", ["1", None])
def test_bam_merge_equals_the_definition_on_every_case(cases, monkeypatch, chunk_blocks):
    """every case of bam_merge_cases: files dealt from one file (tie-safe and round-robin: ties across files), the reversed dictionary, two appended contigs, a
    file with n_ref = 0, a file without records first / in the middle / last, the 700 records of 36 to 40 bytes per file at every alignment (neighbours share an
    aligned word: the patch is made of byte stores), mate ids of every kind (refused in a translated file, verbatim in an identity one), the 225 kB record, the
    accepted header cases; the refused ones leave with their code - the twelve header cases at open, the record cases at finish"""
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    n_translated = 0
    for name, c in cases.items():
        paths = [x["path"] for x in c["inputs"]]
        if "error" in c:
            with pytest.raises(bammerge.BamMergeError) as e:
                _device_merge(paths)
            assert _code(e) == c["error"], name
            continue
        got = _device_merge(paths, both_indexes=True)
        _check(c, got, (name, chunk_blocks))
        n_translated += got[4]["merge"]["n_translated_records"]
        if name == "directed:tiny_records":
            assert got[4]["merge"]["n_translated_files"] == 2 and got[4]["merge"]["n_translated_records"] == 1400
            if chunk_blocks == "1":
                assert got[4]["merge"]["n_translated_chunks"] > 20, got[4]["merge"]
    assert n_translated > 2000


def test_bam_merge_header_refusals_leave_at_open(cases):
    """the header cases the definition refuses never reach the device: open raises, with handles that have not even switched device decode on"""
    seen = 0
    for name, c in cases.items():
        if name.startswith("header:") and "error" in c:
            readers = [NativeBam(x["path"], threads=1) for x in c["inputs"]]
            try:
                with pytest.raises(bammerge.BamMergeError) as e:
                    BamMerge.open(readers, device=0)
                assert _code(e) == _abi.SVX_E_ARG, name
            finally:
                for r in readers:
                    r.close()
            seen += 1
    assert seen == 3 and sum(1 for name in cases if name.startswith("header:")) == 12


def _tiny(tag, tid, pos, flag=0, mate=-1):
    return MC.with_ids(SC.tiny_record(tag, tid, pos, flag), mate=mate)


def _made(tmp_path, name, inputs, **extra):
    """a case built here from the builders of bam_merge_cases: inputs = [(refs, lens, records)]"""
    c = dict(inputs=[MC._input(str(tmp_path), "%s_%d" % (name, f), MC.header_of(refs, lens), recs, len(refs), cuts=900 + 70 * f) for f, (refs, lens, recs) in enumerate(inputs)], **extra)
    return _expect(c, name)


def test_bam_merge_key_is_built_over_the_merged_dictionary(tmp_path, monkeypatch):
    """the first file has 3 references, the second adds 2: the key is that of 5 references (tid_bits 3), not of either file (tid_bits 2).  Unplaced records of the
    first file, keyed over its own n_ref = 3, would sort in front of the records the second file places on merged ids 3 and 4"""
    assert bamsort_bits(3) == 2 and bamsort_bits(5) == 3
    refs_a, lens_a = ["k0", "k1", "k2"], [5000, 6000, 7000]
    refs_b, lens_b = ["k1", "k3", "k4"], [6000, 8000, 9000]
    a = [_tiny("a%d" % k, (0, 1, 2, -1)[k % 4], -1 if k % 4 == 3 else 10 * k, 16 * (k & 1), mate=(k % 4) - 1) for k in range(120)]
    b = [_tiny("b%d" % k, (0, 1, 2, 1, -1)[k % 5], -1 if k % 5 == 4 else 7 * k, 16 * (k & 1), mate=(k % 4) - 1) for k in range(150)]
    c = _made(tmp_path, "five_references", [(refs_a, lens_a, a), (refs_b, lens_b, b)])
    merged_ids = [struct.unpack_from("<i", c["stream"], at + 4)[0] for at in _record_starts(c["stream"])]
    assert {3, 4} <= set(merged_ids) and merged_ids.index(-1) > max(i for i, t in enumerate(merged_ids) if t >= 3)
    for chunk_blocks in ("1", None):
        _set_chunk_blocks(monkeypatch, chunk_blocks)
        got = _device_merge([x["path"] for x in c["inputs"]], both_indexes=True)
        _check(c, got, chunk_blocks)
        assert got[4]["key_bits"] == 33 + 3


def bamsort_bits(n_ref):
    b = 1
    while b < 31 and (1 << b) <= n_ref:
        b += 1
    return b


def _record_starts(stream):
    _, _, at = bamsort.split_header(stream)
    out = []
    while at < len(stream):
        out.append(at)
        at += 4 + struct.unpack_from("<I", stream, at)[0]
    return out


def test_bam_merge_identity_file_is_checked_against_its_own_dictionary(tmp_path):
    """an identity file with fewer references than the merged dictionary: a refID beyond its OWN n_ref but inside the merged one is refused (SVX_E_ARG); the same
    file without that record merges, its out-of-range mate id verbatim"""
    refs_a, lens_a = ["k0", "k1"], [5000, 6000]
    refs_b, lens_b = ["k1", "k0", "k2", "k3"], [6000, 5000, 7000, 8000]
    good_a = [_tiny("a%d" % k, k % 2, 10 * k, mate=(-1, 0, 1, 3, 9)[k % 5]) for k in range(60)]
    b = [_tiny("b%d" % k, k % 4, 5 * k, mate=(k % 5) - 1) for k in range(80)]
    c = _made(tmp_path, "identity_fewer", [(refs_a, lens_a, good_a), (refs_b, lens_b, b)])
    _check(c, _device_merge([x["path"] for x in c["inputs"]], both_indexes=True), "identity with fewer references")
    bad_a = good_a[:30] + [_tiny("bad", 2, 77)] + good_a[30:]
    bad = _made(tmp_path, "identity_beyond", [(refs_a, lens_a, bad_a), (refs_b, lens_b, b)], error=bamsort.E_ARG)
    with pytest.raises(bammerge.BamMergeError) as e:
        _device_merge([x["path"] for x in bad["inputs"]])
    assert _code(e) == _abi.SVX_E_ARG


def test_bam_merge_spilled_runs_inside_a_file_and_on_a_file_boundary(cases, tmp_path, monkeypatch):
    """max_bytes from the case's byte counts: with chunks of one block, a limit of the first file's bytes plus half of the second's closes a run INSIDE the second
    file; with whole files as chunks, a limit of the larger file's bytes - each file fits, the two together do not - closes a run exactly ON the boundary.  The bytes are those of the in-memory merge"""
    c = cases["directed:reversed_dictionary"]
    paths = [x["path"] for x in c["inputs"]]
    size = [sum(len(r) for r in x["records"]) for x in c["inputs"]]
    spill = str(tmp_path / "spill")
    os.mkdir(spill)
    _set_chunk_blocks(monkeypatch, "1")
    got = _device_merge(paths, both_indexes=True, max_bytes=size[0] + size[1] // 2, spill_dir=spill)
    _check(c, got, "a run ends inside the second file")
    sp = got[4]["spill"]
    assert sp["n_runs"] == 2 and size[0] < sp["max_run_bytes"] <= size[0] + size[1] // 2 and sp["spilled_bytes"] == sum(size), sp
    _set_chunk_blocks(monkeypatch, None)
    assert max(size) < sum(size)                                           # (each file fits alone, both together do not: the run closes between them)
    got = _device_merge(paths, both_indexes=True, max_bytes=max(size), spill_dir=spill)
    _check(c, got, "a run ends on the file boundary")
    sp = got[4]["spill"]
    assert sp["n_runs"] == 2 and sp["max_run_bytes"] == max(size) and sp["max_chunk_bytes"] == max(size) and sp["spilled_bytes"] == sum(size), sp
    assert os.listdir(spill) == []


def test_bam_merge_of_one_file_is_sort_bam(cases, tmp_path):
    x = cases["split:blocks_cut_records_anywhere/2"]["one"]
    out, merged = str(tmp_path / "sorted.bam"), str(tmp_path / "merged.bam")
    harness.sort_bam(x["path"], out, 0)
    st = harness.merge_bam([x["path"]], merged, 0)
    assert open(out, "rb").read() == open(merged, "rb").read() and open(out + ".bai", "rb").read() == open(merged + ".bai", "rb").read()
    assert st["merge"]["n_files"] == 1 and st["merge"]["n_translated_records"] == 0 and st["n_records"] == len(x["records"])


def test_bam_merge_takes_a_sam_text_reader(cases, tmp_path, monkeypatch):
    """a BAM file and a SAM text (svx_sam_open) through one session, the text second and third under dictionaries that are not the merged one, in slices of 4 KiB:
    the header of the text at open, the dictionary check in add and the text loader's feed; the bytes are the definition's over sam.py's records"""
    text, _ = SAMC.seeded_file(23, 400)
    header, recs = sam.convert(text)
    src = str(tmp_path / "seeded.sam")
    with open(src, "wb") as fh:
        fh.write(text)
    first = cases["directed:reversed_dictionary"]["inputs"][0]
    c = _expect(dict(inputs=[first, dict(path=src, header=header, records=recs, n_ref=len(SAMC.REFS)), dict(path=src, header=header, records=recs, n_ref=len(SAMC.REFS))]), "sam")
    monkeypatch.setenv("SVX_SAM_DEV_CHUNK_BYTES", "4096")
    got = _device_merge([x["path"] for x in c["inputs"]], both_indexes=True)
    _check(c, got, "a SAM text in a session")
    assert got[4]["merge"]["n_translated_files"] == 2 and got[4]["merge"]["n_translated_records"] == 800 and got[4]["merge"]["n_translated_chunks"] > 4


def test_bam_merge_state_rules(cases, monkeypatch):
    c = cases["directed:reversed_dictionary"]
    a, b = (x["path"] for x in c["inputs"])
    ra, rb = _open(a), _open(b)
    m = BamMerge.open([ra, rb], device=0)
    try:
        for call in (m.finish, m.count, lambda: m.encode(0, 1), m.index, m.permutation):
            with pytest.raises(bammerge.BamMergeError) as e:
                call()                                                     # nothing added yet
            assert _code(e) == _abi.SVX_E_STATE
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(rb)                                                      # out of order: the dictionary is not file 0's
        assert _code(e) == _abi.SVX_E_ARG
        ra.sort_begin()
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(ra)                                                      # in a sort pass of its own
        assert _code(e) == _abi.SVX_E_STATE
        ra.sort_abort()
        ra.index_begin()
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(ra)                                                      # in an index pass
        assert _code(e) == _abi.SVX_E_STATE
        ra.index_abort()
        assert ra.read_batch(10, 20)[1] == 10
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(ra)                                                      # not at its first record
        assert _code(e) == _abi.SVX_E_STATE
        ra.rewind()
        ra.seek_region(0, 0, 0, 100)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(ra)                                                      # on a region read
        assert _code(e) == _abi.SVX_E_STATE and "region read" in str(e.value)
        ra.rewind()
        ra.seek(0, 1)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(ra)                                                      # on a contig range: the pass would end in front of the end of the file
        assert _code(e) == _abi.SVX_E_STATE and "contig range" in str(e.value)
        ra.rewind()
        host = NativeBam(a, threads=1)
        try:
            with pytest.raises(bammerge.BamMergeError) as e:
                m.add(host)                                                # no device decode
            assert _code(e) == _abi.SVX_E_STATE
        finally:
            host.close()
        m.add(ra)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.finish()                                                     # before k adds
        assert _code(e) == _abi.SVX_E_STATE
        with pytest.raises(bammerge.BamMergeError) as e:
            m.encode(0, 1)                                                 # before finish
        assert _code(e) == _abi.SVX_E_STATE
        m.add(rb)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(rb)                                                      # every file has been added
        assert _code(e) == _abi.SVX_E_STATE
        with pytest.raises(bammerge.BamMergeError) as e:
            m.encode(0, 1)
        assert _code(e) == _abi.SVX_E_STATE
        _, n_bytes, n_blocks = m.finish()
        with pytest.raises(bammerge.BamMergeError) as e:
            m.index()                                                      # nothing encoded yet
        assert _code(e) == _abi.SVX_E_STATE
        comp, raw = _encode_all(m, n_blocks, 1)
        assert raw == c["stream"] and comp == c["file"] and m.index() == c["bai"] and (m.permutation() == c["perm"]).all()
    finally:
        m.close()
        ra.close()
        rb.close()


def test_bam_merge_capacity_failure_breaks_the_session_and_the_reader_rewinds(cases, monkeypatch):
    c = cases["directed:reversed_dictionary"]
    a, b = (x["path"] for x in c["inputs"])
    size = [sum(len(r) for r in x["records"]) for x in c["inputs"]]
    _set_chunk_blocks(monkeypatch, "1")
    ra, rb = _open(a), _open(b)
    m = BamMerge.open([ra, rb], device=0, max_bytes=size[0] + size[1] // 2)
    try:
        m.add(ra)
        with pytest.raises(bammerge.BamMergeError) as e:
            m.add(rb)                                                      # the arena fills inside the second file
        assert _code(e) == _abi.SVX_E_CAPACITY
        for call in (lambda: m.add(rb), m.finish, m.count, lambda: m.encode(0, 1), m.index, m.permutation):
            with pytest.raises(bammerge.BamMergeError) as e:
                call()
            assert _code(e) == _abi.SVX_E_STATE
        rb.rewind()
        n = 0
        while True:
            k = rb.read_batch(500, 20)[1]
            if not k:
                break
            n += k
        assert n == len(c["inputs"][1]["records"])
    finally:
        m.close()
        ra.close()
        rb.close()
    out = a + ".refused.bam"
    with pytest.raises(bammerge.BamMergeError) as e:
        harness.merge_bam([a, b], out, 0, max_bytes=size[0] + size[1] // 2)
    assert _code(e) == _abi.SVX_E_CAPACITY and not os.path.exists(out) and not os.path.exists(out + ".bai")


def _sorted_alone(bam, x_path, tmp):
    """the reader sorts its own file through sort_begin .. sort_finish -> (file bytes, .bai)"""
    bam.rewind()
    bam.sort_begin()
    while bam.read_batch(5000, 20)[1]:
        pass
    _, _, n_blocks = bam.sort_finish()
    return bam.sort_encode(0, n_blocks), bam.sort_index()


def _sort_bam_bytes(path, out):
    harness.sort_bam(path, out, 0)
    return open(out, "rb").read(), open(out + ".bai", "rb").read()


def test_bam_merge_reader_sorts_alone_and_is_closed_before_the_session(cases, tmp_path):
    """life cycle, once: a reader feeds, then sorts the same file on its own (the bytes sort_bam gives), is closed with its finished sort inside - BEFORE the
    session is finished and closed; the session's output is fetched after every reader is closed"""
    c = cases["directed:reversed_dictionary"]
    a, b = (x["path"] for x in c["inputs"])
    want_b = _sort_bam_bytes(b, str(tmp_path / "b_sorted.bam"))
    ra, rb = _open(a), _open(b)
    m = BamMerge.open([ra, rb], device=0)
    try:
        m.add(ra)
        ra.close()
        m.add(rb)
        assert _sorted_alone(rb, b, tmp_path) == want_b
        rb.close()                                                         # the reader that fed and then sorted alone: closed first
        _, _, n_blocks = m.finish()
        comp, raw = _encode_all(m, n_blocks)
        assert raw == c["stream"] and comp == c["file"] and m.index() == c["bai"] and (m.permutation() == c["perm"]).all()
    finally:
        m.close()
        ra.close()
        rb.close()


def test_bam_merge_reader_sorts_alone_and_is_closed_after_the_session(cases, tmp_path):
    """life cycle, once: the other order - the session is finished, read and closed first; the reader that fed it then sorts alone and is closed last"""
    c = cases["directed:reversed_dictionary"]
    a, b = (x["path"] for x in c["inputs"])
    want_a = _sort_bam_bytes(a, str(tmp_path / "a_sorted.bam"))
    ra, rb = _open(a), _open(b)
    m = BamMerge.open([ra, rb], device=0)
    try:
        m.add(ra)
        m.add(rb)
        rb.close()
        _, _, n_blocks = m.finish()
        comp, raw = _encode_all(m, n_blocks)
        assert raw == c["stream"] and comp == c["file"] and m.index("csi") == c["csi"]
        m.close()                                                          # the session first
        assert _sorted_alone(ra, a, tmp_path) == want_a
    finally:
        m.close()
        ra.close()
        rb.close()


OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
            del_ins_dup_max_distance=1.0, skip_consensus=True, minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2,
            symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
            interspersed_duplications_as_insertions=False, sample="Sample", genome=None, types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")


def _body(path):
    return b"".join(l for l in open(path, "rb").read().splitlines(True) if not l.startswith(b"#"))


def test_bam_merge_of_three_split_files_feeds_the_pipeline(eng, tmp_path):
    """merge_bam on three files dealt from one, then BamPipeline on the merged file: the VCF body and the genotype columns of the pipeline on the definition's
    file; BamPipeline and run_bam given the list do the same merge first"""
    from svim_amd import convert
    contigs = [("chr1", 120000), ("chrE", 30000), ("chr2", 50000), ("chrN", 9000)]
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 400, refs, references, lengths, n_sites=24, types=("DEL", "INS", "INV"))
    recs += synth.planted_reads(9, 100, refs, references, lengths, n_sites=6, types=("DEL", "INS"), tid=2)
    recs += synth.fuzz_split_reads(6, 60, references, lengths)
    rows = [r for r in synth.genotype_rows(31, lengths, n_reads=900, hot=((0, 60000, 300), (2, 300, 100))) if r[2] != 1]
    recs += list(records.AlignmentFile(text=synth.genotype_sam_text(references, lengths, rows)).fetch(until_eof=True))
    recs = sorted(recs, key=lambda r: r.query_name)
    parts = [str(tmp_path / ("part_%d.bam" % f)) for f in range(3)]
    for f, p in enumerate(parts):
        records.write_bam(p, references, lengths, recs[f::3], sort_order="queryname")
    merged_dev, merged_def, merged_pipe, merged_run = (str(tmp_path / n) for n in ("merged_device.bam", "merged_definition.bam", "merged_pipeline.bam", "merged_run.bam"))
    st = harness.merge_bam(parts, merged_dev, 0)
    assert st["n_records"] == len(recs) and st["merge"]["n_files"] == 3 and os.path.exists(merged_dev + ".bai")
    with open(merged_def, "wb") as fh:
        fh.write(bammerge.file(parts))
    assert open(merged_dev, "rb").read() == open(merged_def, "rb").read()
    o = types.SimpleNamespace(**OPTS)
    off, codes = convert.genome_arrays(refs, references)
    bodies = []
    for path, kw in ((merged_dev, {}), (merged_def, {}), (parts, dict(merged_out=merged_pipe))):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=211, device_decode=True, keep_alignments=True, **kw)
        try:
            assert pipe.run() == len(recs)
            pipe.cluster(genome=(off, codes))
            pipe.combine()
            pipe.genotype()
            out = str(tmp_path / ("out_%d.vcf" % len(bodies)))
            pipe.write_vcf(out)
            bodies.append(_body(out))
        finally:
            pipe.close()
    assert bodies[0] == bodies[1] == bodies[2] and bodies[0].count(b"\n") > 10
    calls = [l.split(b"\t")[9].split(b":")[0] for l in bodies[0].splitlines()]
    assert sum(1 for c in calls if c in (b"0/1", b"1/1", b"0/0")) > 3
    assert open(merged_pipe, "rb").read() == open(merged_def, "rb").read()
    fasta = str(tmp_path / "ref.fa")
    with open(fasta, "w") as fh:
        for name in references:
            fh.write(">%s\n%s\n" % (name, refs[name]))
    one = harness.run_bam(merged_def, fasta, o, device=0)
    many = harness.run_bam(parts, fasta, o, device=0, merged_out=merged_run)
    assert many["counts"] == one["counts"] and one["counts"]["records"] == len(recs) and open(merged_run, "rb").read() == open(merged_def, "rb").read()
    with pytest.raises(ValueError):
        harness.run_bam(parts, fasta, o, device=0)                          # a list needs merged_out


def test_bam_reader_and_sort_beside_a_session_are_untouched(cases, tmp_path):
    """a plain sort_bam and a plain reading pass of one corner file, with a session open on the same file beside them: the same bytes, and the reader's own
    svx_bam_sort_get_stats is what it is without any session (the session's records are not counted there)"""
    x = cases["split:blocks_cut_records_anywhere/2"]["one"]
    want = _sort_bam_bytes(x["path"], str(tmp_path / "before.bam"))
    plain = _open(x["path"])
    fed = _open(x["path"])
    m = BamMerge.open([fed], device=0)
    try:
        st0 = plain.sort_stats()
        assert st0["n_records"] == 0 and st0["arena_bytes"] == 0 and st0["n_slabs"] == 0
        m.add(fed)
        st1 = fed.sort_stats()
        assert st1["n_records"] == 0 and st1["arena_bytes"] == 0 and st1["n_slabs"] == 0      # feeding left the reader's own sort alone
        n = 0
        while True:
            k = plain.read_batch(500, 20)[1]
            if not k:
                break
            n += k
        assert n == len(x["records"]) and plain.sort_stats() == st0
        assert _sort_bam_bytes(x["path"], str(tmp_path / "beside.bam")) == want
        assert _sorted_alone(fed, x["path"], tmp_path) == want
        assert fed.sort_stats()["n_records"] == len(x["records"])
    finally:
        m.close()
        plain.close()
        fed.close()
