"""SAM text through the device reader (svx_sam_open, svim_amd/csrc/sam.hip in front of csrc/bamdev.hip): the record stream the kernels build equals, byte for
byte, the host build and the definition (svim_amd/sam.py; tests/test_sam.py holds those two to each other) on every corner line of tests/sam_cases.py, whatever
the slices; the batches equal those of the same records read from a BAM file, array by array, in both modes; COLLECT gives the same signatures; sam_to_bam
writes the file and the index the sort's definition gives on the definition's records; the state rules; a refused line fails the read that would hand out its
slice and the handle recovers; the count of floats left to the host; a BAM path never touches any of it."""
import os
import types

import numpy as np
import pytest

import bam_sort_cases as SC
import foreign_bam as FB
import sam_cases as SAMC
from svim_amd import _abi, _lib, bai, bamsort, harness, records, sam, synth
from svim_amd.bamio import NativeBam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the corner lines as a SAM file (last line without its newline) and as a BAM file of the definition's records; the definition's sorted stream"""
    d = str(tmp_path_factory.mktemp("sam_cases_gpu"))
    ls = SAMC.lines()
    recs = [sam.record_bytes(l, SAMC.TID) for _, l in ls]
    text = SAMC.text(ls, last_newline=False)
    host, n = _lib.sam_convert_host(text, SAMC.REFS)
    assert n == len(recs) and host == b"".join(recs)
    x = dict(lines=ls, records=recs, text=text, sam=os.path.join(d, "cases.sam"), bam=os.path.join(d, "cases.bam"), header=sam.header_bytes(SAMC.HEADER), n_ref=len(SAMC.REFS))
    with open(x["sam"], "wb") as fh:
        fh.write(text)
    FB.write(x["bam"], SAMC.REFS, SAMC.LENS, recs, sort_order="unsorted", index=False)
    x["stream"], x["perm"] = SC.definition(x)
    return x


def _set_chunk(monkeypatch, chunk_bytes):
    if chunk_bytes:
        monkeypatch.setenv("SVX_SAM_DEV_CHUNK_BYTES", chunk_bytes)          # (read when the handle switches device decode on)
    else:
        monkeypatch.delenv("SVX_SAM_DEV_CHUNK_BYTES", raising=False)


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


def _sorted_stream(path, **kw):
    """-> (the uncompressed bytes of the sorted file, the permutation, records read, the front end's stats)"""
    bam = _open(path)
    try:
        bam.sort_begin()
        n = _pass(bam, **kw)
        n_rec, n_bytes, n_blocks = bam.sort_finish()
        assert n_rec == n
        raw = b"".join(bam.sort_encode(first, min(64, n_blocks - first), stream=True)[1] for first in range(0, n_blocks, 64))
        return raw, bam.sort_permutation(), n, bam.sam_stats()
    finally:
        bam.close()


@pytest.mark.parametrize("chunk_bytes", ["4096", "1", None])
def test_sam_stream_equals_host_build_and_definition(cases, monkeypatch, chunk_bytes):
    """the device's records, fetched through the sort pass's uncompressed bytes.  Slices of 4096 bytes: lines lie across the budget's reach, and the lines longer
    than a slice (SEQ of 4097, the SA tag, both long CIGARs) make it grow; "1": every slice grows until it holds one line"""
    _set_chunk(monkeypatch, chunk_bytes)
    raw, perm, n, st = _sorted_stream(cases["sam"])
    assert n == len(cases["records"])
    assert raw == cases["stream"], (len(raw), len(cases["stream"]))
    assert (perm == np.asarray(cases["perm"], dtype=np.uint32)).all()
    assert st["n_lines"] == n and st["n_long_cigars"] == 1 and st["stream_bytes"] == sum(len(r) for r in cases["records"])
    assert st["text_bytes"] == len(cases["text"]) - len(SAMC.HEADER)
    if chunk_bytes == "1":
        assert st["n_chunks"] == n
    elif chunk_bytes == "4096":
        assert 1 < st["n_chunks"] < n


def _batches(path, mode, batch_records, min_mapq=20):
    bam = _open(path)
    try:
        out = []
        while True:
            b, k = bam.read_batch(batch_records, min_mapq, mode)
            if k == 0:
                break
            out.append(bam.batch_arrays(b))
        return out, bam.read_names()
    finally:
        bam.close()


def _flat(batches):
    """the batches of a pass as one table: per-record and per-segment arrays concatenated, offsets as lengths (a batch never spans two slices, so where the batches
    are cut depends on the slices; order / seg_order number the slots of ONE batch and are left out)"""
    cat = lambda k, dt: np.concatenate([a[k] for a in batches]) if batches else np.zeros(0, dt)          # noqa: E731
    out = {k: cat(k, object if k == "read_id" else _abi.BATCH_DTYPES[k]) for k in ("flag", "tid", "pos", "mapq", "lseq", "read_id", "seg_tid", "seg_pos", "seg_rev", "seg_mapq", "seg_lseq")}
    for k, dt in (("cigar", np.uint32), ("seq", np.uint8), ("seg_cigar", np.uint32)):
        out[k] = cat(k, dt)
    for k in ("cigar_off", "seq_off", "seg_off", "seg_cigar_off"):
        out[k + "_lengths"] = np.concatenate([np.diff(a[k].astype(np.int64)) for a in batches]) if batches else np.zeros(0, np.int64)
    return out


@pytest.mark.parametrize("mode", ["coordinate", "queryname"])
def test_sam_batches_equal_bam_batches(cases, monkeypatch, mode):
    """the same records as SAM text and as a BAM file (foreign_bam.write of sam.record_bytes of the same lines): every array of every batch where both files are
    one chunk; with slices of 4096 bytes the batches end where the slices end, and the arrays are compared as one table"""
    for chunk_bytes, batch_records in (("4096", 7), (None, 7), (None, 100000)):
        _set_chunk(monkeypatch, chunk_bytes)
        got, names = _batches(cases["sam"], mode, batch_records)
        monkeypatch.delenv("SVX_SAM_DEV_CHUNK_BYTES", raising=False)
        exp, exp_names = _batches(cases["bam"], mode, batch_records)
        # read ids number the names in the order the device interned them, which is not the file's within a chunk: a record's read is its NAME
        assert sorted(names) == sorted(exp_names), (chunk_bytes, batch_records)
        for arrays, nm in ((got, names), (exp, exp_names)):
            for a in arrays:
                a["read_id"] = np.array([nm[int(r)] for r in a["read_id"]], dtype=object)
        if chunk_bytes:
            assert len(got) > len(exp)
            got, exp = [_flat(got)], [_flat(exp)]
        assert len(got) == len(exp), (chunk_bytes, batch_records)
        for k, (a, b) in enumerate(zip(got, exp)):
            assert sorted(a) == sorted(b)
            for key in a:
                assert np.array_equal(a[key], b[key]), (chunk_bytes, batch_records, k, key)


def test_sam_collect_equals_bam_collect(tmp_path):
    """a seeded synth file written as SAM text and as BAM: the same signature table from either"""
    contigs = [("chr1", 120000), ("chr2", 50000)]
    refs = synth.make_reference(3, contigs)
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.planted_reads(5, 400, refs, references, lengths, n_sites=25, types=("DEL", "INS", "INV"))
    recs += synth.fuzz_split_reads(6, 60, references, lengths)
    recs = synth.coordinate_sort(recs)
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                              position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False)
    sam_path, bam_path = str(tmp_path / "synth.sam"), str(tmp_path / "synth.bam")
    with open(sam_path, "w") as fh:
        fh.write(synth.sam_text(references, lengths, recs))
    records.write_bam(bam_path, references, lengths, recs)
    eng = _lib.engine()

    def rows(path):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True)
        n = pipe.run()
        names = pipe.bam.read_names()
        t = eng.fetch_signatures(0)
        pipe.close()
        return n, [(int(t.type[i]), int(t.contig[i]), int(t.start[i]), int(t.end[i]), int(t.contig2[i]), int(t.pos2[i]), names[int(t.read_id[i])], t.sequence(i)) for i in range(t.n)]
    n_sam, sig_sam = rows(sam_path)
    n_bam, sig_bam = rows(bam_path)
    assert n_sam == n_bam == len(recs) and len(sig_bam) > 50 and sig_sam == sig_bam


def test_sam_to_bam_sorted_file_and_index(tmp_path, monkeypatch):
    """sam_to_bam(sort=True, index=True) on a seeded file of everyday lines, in slices of 64 KiB: the file is the encoder's bytes of the stream bamsort.py defines on
    the definition's records, the .bai the bytes bai.py defines for that file; the file reads back through the device reader"""
    text, ls = SAMC.seeded_file(21, 3000)
    header, recs = sam.convert(text)
    src, out = str(tmp_path / "seeded.sam"), str(tmp_path / "sorted.bam")
    with open(src, "wb") as fh:
        fh.write(text)
    _set_chunk(monkeypatch, "65536")
    st = harness.sam_to_bam(src, out, sort=True, index=True)
    stream, perm = SC.definition(dict(records=recs, header=header, n_ref=len(SAMC.REFS)))
    want = _lib.text_gz_host(stream)
    assert open(out, "rb").read() == want and st["n_records"] == 3000
    assert open(out + ".bai", "rb").read() == bai.build_index(*bai.rows_of_bam(out))
    back = _open(out)
    try:
        assert not back.is_sam and back.sort_order == "coordinate" and _pass(back) == 3000
    finally:
        back.close()
    assert st["sam"]["n_records"] == 3000 and st["sam"]["n_chunks"] > 1 and st["sam"]["text_bytes"] == len(text) - len(SAMC.HEADER)
    # harness.sort_bam takes the SAM path as it takes a BAM path
    again = str(tmp_path / "again.bam")
    harness.sort_bam(src, again, index=False)
    assert open(again, "rb").read() == want


def test_sam_state_rules_and_rewind(cases, monkeypatch):
    _set_chunk(monkeypatch, "4096")
    bam = NativeBam(cases["sam"], threads=2)
    try:
        assert bam.is_sam and bam.references == SAMC.REFS and bam.lengths == SAMC.LENS and bam.sort_order == "unsorted"
        with pytest.raises(_lib.SvxError) as e:
            bam.read_batch(10, 20, "coordinate")
        assert e.value.code == _abi.SVX_E_STATE
        bam.set_device_decode(0)
        for call in (lambda: bam.seek(0), bam.index_begin, lambda: bam.set_gpu_inflate(0)):
            with pytest.raises(_lib.SvxError) as e:
                call()
            assert e.value.code == _abi.SVX_E_STATE
        first = []
        while True:
            b, k = bam.read_batch(13, 20, "coordinate")
            if k == 0:
                break
            first.append(bam.batch_arrays(b))
        names = bam.read_names()
        bam.rewind()
        k_batch = 0
        while True:
            b, k = bam.read_batch(13, 20, "coordinate")
            if k == 0:
                break
            a = bam.batch_arrays(b)
            for key in a:
                assert np.array_equal(a[key], first[k_batch][key]), (k_batch, key)
            k_batch += 1
        assert k_batch == len(first) and bam.read_names() == names and sum(int(a["flag"].size) for a in first) == len(cases["records"])
    finally:
        bam.close()


def _slices(text, header_len, chunk):
    """the slices the reader cuts (ends of the text ranges): behind the last newline within `chunk` bytes, growing while there is none"""
    ends, start = [], header_len
    while start < len(text):
        reach = chunk
        while True:
            end = min(len(text), start + reach)
            if end == len(text):
                break
            nl = text.rfind(b"\n", start, end)
            if nl >= 0:
                end = nl + 1
                break
            reach *= 2
        ends.append(end)
        start = end
    return ends


@pytest.mark.parametrize("which", ["flag_out_of_range", "unknown_rname", "aux_float_not_a_number", "cigar_bad_letter"])
def test_sam_bad_line_in_the_third_slice(tmp_path, monkeypatch, which):
    """the refused line lies in the third slice: the records of the first two are handed out, the read that needs the third fails with the definition's status and
    the line's number in the file; after rewind the handle reads the same records again"""
    bad, code = [(l, c) for n, l, c in SAMC.refusals() if n == which][0]
    text, ls = SAMC.seeded_file(31, 120)
    chunk = 8192
    ends = _slices(text, len(SAMC.HEADER), chunk)
    assert len(ends) > 4
    at = ends[1] + text[ends[1]:ends[2]].find(b"\n") + 1          # the second line of the third slice
    text = text[:at] + bad + b"\n" + text[at:]
    want_line = text[:at].count(b"\n") + 1
    n_before = text[len(SAMC.HEADER):ends[1]].count(b"\n")
    path = str(tmp_path / "bad.sam")
    with open(path, "wb") as fh:
        fh.write(text)
    _set_chunk(monkeypatch, str(chunk))
    bam = _open(path)
    try:
        for _ in range(2):
            n = 0
            with pytest.raises(_lib.SvxError) as e:
                while True:
                    k = bam.read_batch(17, 20, "coordinate")[1]
                    assert k > 0
                    n += k
            assert n == n_before and e.value.code == code and ("SAM line %d:" % want_line) in str(e.value), (n, n_before, str(e.value))
            bam.rewind()
    finally:
        bam.close()


def test_sam_several_faults_in_one_slice(tmp_path, monkeypatch):
    """more than one fault in one slice, or in one line: the reader reports the line and the status the host build and the definition report, whichever kernel
    finds which fault"""
    _set_chunk(monkeypatch, None)
    n_head = SAMC.HEADER.count(b"\n")
    for name, ls, k, code in SAMC.several_faults():
        path = str(tmp_path / (name + ".sam"))
        with open(path, "wb") as fh:
            fh.write(SAMC.HEADER + b"\n".join(ls) + b"\n")
        bam = _open(path)
        try:
            with pytest.raises(_lib.SvxError) as e:
                bam.read_batch(100, 20, "coordinate")
            assert e.value.code == code and ("SAM line %d:" % (n_head + k + 1)) in str(e.value), (name, str(e.value))
            assert bam.sam_stats()["n_chunks"] == 0
        finally:
            bam.close()


def test_sam_patched_floats_are_counted(cases, monkeypatch):
    _set_chunk(monkeypatch, None)
    bam = _open(cases["sam"])
    try:
        assert _pass(bam) == len(cases["records"])
        st = bam.sam_stats()
    finally:
        bam.close()
    want = SAMC.n_slow_floats(cases["lines"])
    assert want == len(SAMC.SLOW_FLOATS) + 3 and st["n_patched_floats"] == want and st["n_chunks"] == 1


def test_bam_paths_never_touch_the_sam_front_end(cases):
    bam = _open(cases["bam"])
    try:
        assert not bam.is_sam and _pass(bam) == len(cases["records"])
        assert all(v == 0 for v in bam.sam_stats().values())
    finally:
        bam.close()
