"""The merge of several BAM files by its definition (svim_amd/bammerge.py) and by the host build (svx_bam_merge_header_host, svx_bam_merge_host in
csrc/bamsort_host.cpp, the rule of csrc/bamsort_core.hpp: bsort_translate), on the cases of tests/bam_merge_cases.py: one file is the
sort of that file; files dealt from one file give that file's sorted bytes, which the existing definition says without knowing of the merge; translation
against a brute force that resolves every id to its NAME; the header rule line for line; the refusals with their codes; the host build under the
sanitizers.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_merge_cases as MC
import bam_sort_cases as SC
from svim_amd import _abi, _lib, bammerge, bamsort

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return MC.build_all(str(tmp_path_factory.mktemp("bam_merge_cases")))


def _accepted(cases):
    return {name: c for name, c in cases.items() if "error" not in c}


def test_one_file_is_the_sort_of_that_file(cases):
    seen = 0
    for name, c in cases.items():
        if name.startswith("split:") and name.endswith("/2"):
            one = c["one"]
            raw = one["header"] + b"".join(one["records"])
            stream, perm = bammerge.stream_of([raw])
            body, want = bamsort.sort_records(b"".join(one["records"]), one["n_ref"])
            assert stream == bamsort.sorted_header(one["header"]) + body and list(perm) == list(want), name
            assert bammerge.merged_header([one["header"]]) == bamsort.sorted_header(one["header"]) == _lib.bam_merge_header_host([one["header"]])[0], name
            assert bammerge.merge([(b"".join(one["records"]), one["n_ref"], range(one["n_ref"]))]) == (body, want), name
            seen += 1
    assert seen >= 20


def test_split_files_give_the_sorted_bytes_of_the_one_file(cases):
    """the expectation is bamsort's, of the file the inputs were dealt from: independent of everything the merge adds"""
    seen = 0
    for name, c in cases.items():
        if not name.startswith("split:"):
            continue
        want_stream, want_perm = SC.definition(c["one"])
        stream, perm = MC.definition(c)
        assert stream == want_stream, name
        assert [c["origin"][g] for g in perm] == list(want_perm), name
        assert sorted(c["origin"]) == list(range(len(c["one"]["records"]))), name
        seen += 1
    assert seen >= 40


def test_ties_leave_in_file_order_then_in_file_order(cases):
    for name, c in cases.items():
        if not name.startswith("ties:"):
            continue
        stream, perm = MC.definition(c)
        recs = [r for x in c["inputs"] for r in x["records"]]
        keys = [bamsort.sort_key(recs[g][4:]) for g in perm]
        assert keys == sorted(keys), name
        groups = {}
        for g in perm:
            groups.setdefault(bamsort.sort_key(recs[g][4:]), []).append(g)
        assert all(members == sorted(members) for members in groups.values()), name          # global numbers: file order, then in-file order
        first_file = len(c["inputs"][0]["records"])
        assert any(members[0] < first_file <= members[-1] for members in groups.values()), name         # a key's records do sit in different files
        one_perm = SC.definition(c["one"])[1]
        assert [c["origin"][g] for g in perm] != list(one_perm), name                           # (and that is NOT the order of the one file)


def _resolved(rec, names):
    """(reference name, pos, mate's reference name, every byte that is not an id) of a record under a dictionary"""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    mate, = struct.unpack_from("<i", rec, 24)
    name_of = lambda t: None if t < 0 else names[t]             # noqa: E731
    return name_of(tid), pos, name_of(mate), rec[:4] + rec[8:24] + rec[28:]


def test_translation_against_a_brute_force_over_names(cases):
    """every output record resolved to names through the merged dictionary equals the input record resolved through its own; the order is that of a plain sort
    of the inputs by (place of the name in the merged dictionary, pos, strand), stable"""
    seen_translated = 0
    for name, c in _accepted(cases).items():
        if not name.startswith(("directed:", "header:")):
            continue
        dicts = [bammerge.parse_header(x["header"])[1] for x in c["inputs"]]
        merged = [n for n, _ in bammerge.merged_dictionary(dicts)]
        rank = {n: i for i, n in enumerate(merged)}
        identity = [[n for n, _ in d] == merged[:len(d)] for d in dicts]
        rows = []
        for f, (x, d) in enumerate(zip(c["inputs"], dicts)):
            own = [n for n, _ in d]
            for r in x["records"]:
                if identity[f]:                                            # verbatim: a mate id may name nothing at all
                    tid, pos = struct.unpack_from("<ii", r, 4)
                    rows.append((None if tid < 0 else own[tid], pos, ("raw", struct.unpack_from("<i", r, 24)[0]), r[:4] + r[8:24] + r[28:]))
                else:
                    rows.append(_resolved(r, own))
                    seen_translated += 1
        flag = lambda row: struct.unpack_from("<H", row[3], 14)[0] & 16          # noqa: E731  (rec[18:20] of the record = [14:16] once the refID is cut out)
        order = sorted(range(len(rows)), key=lambda g: (rank[rows[g][0]] if rows[g][0] is not None else 1 << 32, (rows[g][1] + 1) & 0xffffffff, flag(rows[g])))
        stream, perm = MC.definition(c)
        assert list(perm) == order, name
        hdr, n_ref, at = bamsort.split_header(stream)
        assert [n for n, _ in bammerge.parse_header(hdr)[1]] == merged and n_ref == len(merged), name
        out = bamsort.split_records(stream[at:], n_ref)
        assert len(out) == len(rows), name
        for g, r in zip(perm, out):
            f = next(i for i, x in enumerate(c["inputs"]) if g < sum(len(y["records"]) for y in c["inputs"][:i + 1]))
            if identity[f]:
                tid, pos = struct.unpack_from("<ii", r, 4)
                got = (None if tid < 0 else merged[tid], pos, ("raw", struct.unpack_from("<i", r, 24)[0]), r[:4] + r[8:24] + r[28:])
            else:
                got = _resolved(r, merged)
            assert got == rows[g], (name, g)
    assert seen_translated > 3000


def test_maps_of_the_dictionary_cases(cases):
    c = cases["directed:reversed_dictionary"]
    dicts = [bammerge.parse_header(x["header"])[1] for x in c["inputs"]]
    assert bammerge.tid_maps(dicts) == [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]]
    c = cases["directed:appends_two_contigs"]
    dicts = [bammerge.parse_header(x["header"])[1] for x in c["inputs"]]
    assert bammerge.tid_maps(dicts)[1] == [2, 0, 6, 7] and [n for n, _ in bammerge.merged_dictionary(dicts)][6:] == [b"x0", b"x1"]
    c = cases["directed:empty_file_first"]
    dicts = [bammerge.parse_header(x["header"])[1] for x in c["inputs"]]
    assert bammerge.tid_maps(dicts) == [[0, 1, 2], [3, 4, 5, 6, 1, 0], [0, 1, 6, 5, 4, 3]]
    c = cases["directed:no_references_only_unplaced"]
    dicts = [bammerge.parse_header(x["header"])[1] for x in c["inputs"]]
    assert bammerge.tid_maps(dicts)[1] == []
    # the reversed case: the second input is in coordinate order by its own ids and is not once translated
    x = cases["directed:reversed_dictionary"]["inputs"][1]
    own = [bamsort.sort_key(r[4:]) for r in x["records"]]
    tr = [bamsort.sort_key(bammerge.translate_record(r, [5, 4, 3, 2, 1, 0])[4:]) for r in x["records"]]
    assert own == sorted(own) and tr != sorted(tr)


def test_header_rule_line_for_line(cases):
    seen = 0
    for name, (files, want) in MC.HEADER_CASES.items():
        c = cases["header:" + name]
        headers = [x["header"] for x in c["inputs"]]
        if isinstance(want, int):
            with pytest.raises(bammerge.BamMergeError) as e:
                bammerge.merged_header(headers)
            assert e.value.code == want, name
            with pytest.raises(bammerge.BamMergeError) as e:
                _lib.bam_merge_header_host(headers)
            assert e.value.code == want, name
            continue
        made = bammerge.merged_header(headers)
        text, refs = bammerge.parse_header(made)
        assert text.decode("ascii").split("\n") == want + [""], name
        assert struct.unpack_from("<i", made, 4)[0] == len(text) and b"\0" not in text, name
        dicts = [bammerge.parse_header(h)[1] for h in headers]
        assert refs == bammerge.merged_dictionary(dicts), name
        host, maps = _lib.bam_merge_header_host(headers)
        assert host == made and maps == bammerge.tid_maps(dicts), name
        seen += 1
    assert seen == 9


def test_host_build_equals_the_definition_on_every_case(cases):
    for name, c in cases.items():
        headers = [x["header"] for x in c["inputs"]]
        dicts = [bammerge.parse_header(h)[1] for h in headers]
        try:
            want_header = bammerge.merged_header(headers)
        except bammerge.BamMergeError as err:
            with pytest.raises(bammerge.BamMergeError) as e:
                _lib.bam_merge_header_host(headers)
            assert e.value.code == err.code == c["error"], name
            continue
        header, maps = _lib.bam_merge_header_host(headers)
        assert header == want_header, name
        assert maps == (bammerge.tid_maps(dicts) if len(headers) > 1 else [list(range(len(dicts[0])))]), name
        files = [(b"".join(x["records"]), x["n_ref"], m) for x, m in zip(c["inputs"], maps)]
        n_merged = len(bammerge.parse_header(header)[1])
        if "error" in c:
            for fn in (bammerge.merge, lambda fs: _lib.bam_merge_host(fs, n_merged), lambda fs: MC.definition(c)):
                with pytest.raises(bammerge.BamMergeError) as e:
                    fn(files)
                assert e.value.code == c["error"], name
            continue
        stream, perm = MC.definition(c)
        body, host_perm = _lib.bam_merge_host(files, n_merged)
        assert header + body == stream and host_perm.tolist() == list(perm), name
        assert bammerge.merge(files) == (body, list(perm)), name


def test_refusals_of_the_host_build_and_the_definition():
    rec = SC.tiny_record("abc", 0, 5, 0)
    for files, n_merged, code in (([(rec, 1, [1])], 1, _abi.SVX_E_ARG),                       # a map entry beyond the merged dictionary
                                  ([(rec, 1, [-1])], 1, _abi.SVX_E_ARG),
                                  ([(rec[:-1], 1, [0])], 1, _abi.SVX_E_ARG),                   # the stream ends inside a record
                                  ([(rec, 1, [0]), (struct.pack("<i", 31) + bytes(31), 1, [0])], 1, _abi.SVX_E_ARG)):
        with pytest.raises(bammerge.BamMergeError) as e:
            _lib.bam_merge_host(files, n_merged)
        assert e.value.code == code
    with pytest.raises(bammerge.BamMergeError) as e:
        bammerge.merge([(rec[:-1], 1, [0])])
    assert e.value.code == bammerge.E_ARG
    with pytest.raises(bammerge.BamMergeError) as e:
        bammerge.merge([(rec, 1, [0, 1])])
    assert e.value.code == bammerge.E_ARG
    for bad in (b"", b"BAM\1" + struct.pack("<i", 50) + b"@HD\n", b"SAM\1" + bytes(8)):
        with pytest.raises(bammerge.BamMergeError):
            _lib.bam_merge_header_host([SC.header(), bad])
    assert issubclass(bammerge.BamMergeError, bamsort.BamSortError)


def test_merge_abi_surface():
    L = _lib.lib()
    for name in ("svx_bam_merge_header_host", "svx_bam_merge_host"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.svx_version() >= 106


def test_header_of_reads_only_the_header(cases, tmp_path):
    for name in ("directed:reversed_dictionary", "header:nul_tail", "directed:no_references_only_unplaced"):
        for x in cases[name]["inputs"]:
            assert bammerge.header_of(x["path"]) == x["header"], name
    # a header that spans several BGZF blocks
    refs = ["contig_with_a_long_name_%05d" % k for k in range(3000)]
    hdr = SC.header("@HD\tVN:1.6\n", refs, [1000 + k for k in range(3000)])
    path = str(tmp_path / "many.bam")
    SC.write_raw(path, hdr, [SC.tiny_record("abc", 2999, 5, 0)], cuts=7000)
    assert len(hdr) > 3 * 7000 and bammerge.header_of(path) == hdr
    paths = [x["path"] for x in cases["directed:appends_two_contigs"]["inputs"]]
    assert bammerge.file(paths) == _lib.text_gz_host(MC.definition(cases["directed:appends_two_contigs"])[0])


def test_merge_host_build_under_the_sanitizers(tmp_path):
    """tools/bam_merge_host_test.cpp with bamsort_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, a stand-alone program: a seeded fuzz over
    headers, maps and streams against a plain reimplementation; every call equals it or ends in the refusal it must, no report"""
    out = str(tmp_path / "bam_merge_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "bam_merge_host_test.cpp"), os.path.join(CSRC, "bamsort_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "11", "2000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "2000 merges" in run.stdout and " 0 different" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    n_equal, n_refused, n_headers = (int(run.stdout.split(w)[0].split()[-1]) for w in (" equal", " refused", " headers"))
    assert n_equal > 800 and n_refused > 200 and n_headers > 1500, run.stdout[-300:]
