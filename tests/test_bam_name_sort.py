"""Query-name order of the BAM sort by its definition (svim_amd/bamsort.py: name_key, order="queryname") and by the host build of csrc/bamsort_core.hpp
(svx_bam_sort_host_order, svx_bam_sort_header_host_order; the kernels write the same bytes, tests/test_gpu_bam_name_sort.py holds them to that): the definition
against a brute force written here, one run per name in every output, the header rule line for line, the host build equal to the definition byte for byte
and permutation for permutation on every case of tests/bam_name_sort_cases.py, the refusals and their codes, the coordinate case of the new entry points equal
to the old ones, the definition's file through the Python reader's query-name batcher, the host build under the sanitizers.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

import bam_name_sort_cases as NC
import bam_sort_cases as SC
from svim_amd import _abi, _lib, bamsort, batch, records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    """every corner file with the definition's stream and permutation, computed once"""
    d = str(tmp_path_factory.mktemp("bam_name_sort_cases"))
    out = NC.build_all(d)
    for x in out.values():
        x["stream"], x["perm"] = NC.definition(x)
    return out


def _text(hdr):
    return hdr[8:8 + struct.unpack_from("<i", hdr, 4)[0]]


def test_definition_equals_a_brute_force(corner):
    for name, x in corner.items():
        recs = x["records"]
        keys = [NC.parsed(r) for r in recs]
        want = sorted(range(len(recs)), key=lambda k: (keys[k][0], keys[k][1], k))
        assert x["perm"] == want, name
        assert x["stream"] == bamsort.sorted_header(x["header"], "queryname") + b"".join(recs[k] for k in want), name
        assert [bamsort.name_key(r[4:]) for r in recs] == keys, name
        assert bamsort.sorted_stream(x["path"], "queryname") == x["stream"], name
        assert bamsort.permutation(recs, "queryname") == want and bamsort.permutation(recs) == bamsort.permutation(recs, "coordinate"), name
    assert [bamsort.name_rank(f) for f in NC.RANK_FLAGS] == list(range(16))
    assert bamsort.name_rank(64) < bamsort.name_rank(128) and bamsort.name_rank(0) < bamsort.name_rank(256) < bamsort.name_rank(2048) < bamsort.name_rank(64)
    with pytest.raises(ValueError):
        bamsort.permutation([], "natural")
    # the files hold the corners they are named for
    c = corner
    names = lambda x: [NC.parsed(x["records"][k])[0] for k in x["perm"]]      # noqa: E731
    assert sorted({len(n) for n in names(c["name_lengths"])}) == list(NC.LENGTHS) and names(c["name_lengths"])[0][-1:] == b"y"
    chain = [n for n in names(c["prefix_chains"]) if b"!" not in n]
    assert chain[:3] == [b"a", b"ab", b"ab"] and all(b.startswith(a) for a, b in zip(chain, chain[1:])) and len(chain) == 19
    assert names(c["high_bytes"])[-1] == b"\xff\x01" and names(c["high_bytes"])[0] == b"r" and names(c["high_bytes"]).index(b"r\x7f") < names(c["high_bytes"]).index(b"r\x80")
    assert names(c["padded_names"]).count(b"pad") == 4 and b"no_nul_in_the_field" in names(c["padded_names"]) and names(c["padded_names"])[0] == b"Z" * 254 and len(names(c["padded_names"])[1]) == 255
    x = c["rank_order"]
    ranks = [NC.parsed(x["records"][k])[1] for k in x["perm"]]
    assert ranks == [r for r in range(16) for _ in (0, 1)] and all(a < b for a, b in zip(x["perm"][::2], x["perm"][1::2]))
    assert c["stable_ties"]["perm"] == list(range(5000))
    assert len({n[:24] for n in names(c["long_shared_prefix"])}) == 1 and len(set(names(c["long_shared_prefix"]))) > 2900
    assert len({n[:4] for n in names(c["distinct_first_word"])}) == 3000
    assert c["no_records"]["perm"] == [] and c["one_record"]["perm"] == [0]
    starts = np.cumsum([0] + [len(r) for r in c["every_alignment"]["records"]])[:-1]
    assert set((starts % 16).tolist()) == set(range(16))


def test_every_name_is_one_run(corner):
    """what bam_iterator needs: the records of a read lie next to each other"""
    for name, x in corner.items():
        seen, last = set(), None
        for k in x["perm"]:
            nm = NC.parsed(x["records"][k])[0]
            if nm != last:
                assert nm not in seen, (name, nm)
                seen.add(nm)
                last = nm


def test_header_rule_line_for_line(corner):
    for name in NC.HEADER_TEXTS:
        old, new = corner[name]["header"], bamsort.sorted_header(corner[name]["header"], "queryname")
        text = NC.header_text(name)
        assert _text(new) == text and len(new) == 8 + len(text) + len(old) - 8 - len(_text(old)), name
        assert new[8 + len(text):] == old[8 + len(_text(old)):], name                                  # the reference dictionary, unchanged
        assert bamsort.sorted_header(new, "queryname") == new, name
        assert _lib.bam_sort_header_host(old, "queryname") == new, name
        assert bamsort.sorted_header(bamsort.sorted_header(old, "queryname")) == bamsort.sorted_header(old), name      # (and back: SS: goes with coordinate order)
    for text in (b"@HD", b"@HD\t", b"@HD\tSO:x", b"@HD\tGO:q\tSO:a\tSO:b\tSS:c\t\tXY:z", b"@HD\tVN:1\r\n@SQ\tSN:a\tLN:1\n", b"@hd\tVN:1\n", b"\0@HD\tVN:1\n", b"@HD\tSS:a\tSS:b"):
        old = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
        new = bamsort.sorted_header(old, "queryname")
        assert _lib.bam_sort_header_host(old, "queryname") == new, text
        fields = _text(new).split(b"\n")[0].split(b"\t")
        assert fields[0] == b"@HD" and fields.count(b"SS:queryname:lexicographical") == 1 and fields[fields.index(b"SO:queryname") + 1] == b"SS:queryname:lexicographical", text
        assert not any(f[:3] == b"GO:" or (f[:3] == b"SS:" and f != b"SS:queryname:lexicographical") for f in fields), text
    text = b"@HD\tGO:q\tSO:a\tSO:b\tSS:c\t\tXY:z"
    assert _text(bamsort.sorted_header(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0), "queryname")) == \
        b"@HD\tSO:queryname\tSS:queryname:lexicographical\tSO:queryname\t\tXY:z"
    with pytest.raises(ValueError):
        bamsort.sorted_header(corner["one_record"]["header"], "name")


def test_host_build_equals_the_definition(corner):
    for name, x in corner.items():
        body, perm = _lib.bam_sort_host(b"".join(x["records"]), x["n_ref"], "queryname")
        assert perm.tolist() == x["perm"], name
        hdr = _lib.bam_sort_header_host(x["header"], "queryname")
        assert hdr + body == x["stream"], name


def test_host_build_equals_the_definition_on_the_large_file(tmp_path):
    x = NC.large_shuffled_file(str(tmp_path / "large.bam"))
    stream = b"".join(x["records"])
    want_body, want_perm = bamsort.sort_records(stream, x["n_ref"], "queryname")
    body, perm = _lib.bam_sort_host(stream, x["n_ref"], "queryname")
    assert perm.tolist() == want_perm and body == want_body and len(want_perm) == 150500
    assert len({NC.parsed(r)[0] for r in x["records"][:2000]}) > 1000                   # (names that make the rounds work, not one name)


def test_refusals():
    n_ref = len(NC.REFS)
    for name, recs, code in NC.refused():
        stream = b"".join(recs)
        with pytest.raises(bamsort.BamSortError) as e:
            bamsort.sort_records(stream, n_ref, "queryname")
        assert e.value.code == code, name
        with pytest.raises(bamsort.BamSortError) as e:
            _lib.bam_sort_host(stream, n_ref, "queryname")
        assert e.value.code == code, name
        if "pos_below" not in name:                                                    # a name the coordinate order never looks at
            assert bamsort.sort_records(stream, n_ref)[1] == _lib.bam_sort_host(stream, n_ref)[1].tolist(), name
    good = b"".join(NC.refused()[0][1][:6])
    for stream in (good[:-1], good + b"\x20\0", good[:3]):                              # the refusals of split_records stand
        with pytest.raises(bamsort.BamSortError) as e:
            bamsort.sort_records(stream, n_ref, "queryname")
        assert e.value.code == bamsort.E_ARG
        with pytest.raises(bamsort.BamSortError) as e:
            _lib.bam_sort_host(stream, n_ref, "queryname")
        assert e.value.code == bamsort.E_ARG
    bad_tid = bytearray(good)
    bad_tid[4:8] = struct.pack("<i", n_ref)
    with pytest.raises(bamsort.BamSortError) as e:
        _lib.bam_sort_host(bytes(bad_tid), n_ref, "queryname")
    assert e.value.code == bamsort.E_ARG
    assert bamsort.sort_records(b"", 0, "queryname") == (b"", []) and _lib.bam_sort_host(b"", 0, "queryname")[0] == b""
    with pytest.raises(ValueError):
        _lib.bam_sort_host(good, n_ref, "natural")
    # an order the library does not know, and a permutation buffer that is too small: the count comes back, nothing is written
    src, n = np.frombuffer(good, dtype=np.uint8), C.c_int64(-1)
    perm = np.full(4, 0xabababab, dtype=np.uint32)
    L = _lib.lib()
    assert L.svx_bam_sort_host_order(_abi.ptr(src), C.c_int64(len(good)), C.c_int32(n_ref), C.c_int(2), None, _abi.ptr(perm), C.c_int64(4), C.byref(n)) == _abi.SVX_E_ARG
    rc = L.svx_bam_sort_host_order(_abi.ptr(src), C.c_int64(len(good)), C.c_int32(n_ref), C.c_int(1), None, _abi.ptr(perm), C.c_int64(4), C.byref(n))
    assert rc == _abi.SVX_E_CAPACITY and n.value == 6 and (perm == 0xabababab).all()


def test_coordinate_order_through_the_new_entry_points_is_the_old_one(tmp_path):
    cases = SC.build_all(str(tmp_path))
    for name in ("five_keys_forty_names", "unplaced_scattered", "records_of_36_to_40_bytes", "header_so_unsorted_go_query", "header_without_hd", "no_records"):
        x = cases[name]
        stream = b"".join(x["records"])
        old_body, old_perm = bamsort.sort_records(stream, x["n_ref"])
        assert bamsort.sort_records(stream, x["n_ref"], "coordinate") == (old_body, old_perm), name
        body, perm = _lib.bam_sort_host(stream, x["n_ref"])
        body2, perm2 = _lib.bam_sort_host(stream, x["n_ref"], "coordinate")
        assert body == body2 == old_body and perm.tolist() == perm2.tolist() == old_perm, name
        assert _lib.bam_sort_header_host(x["header"]) == _lib.bam_sort_header_host(x["header"], "coordinate") == bamsort.sorted_header(x["header"]) == \
            bamsort.sorted_header(x["header"], "coordinate"), name
        # the old C entry points themselves
        L, src, n = _lib.lib(), np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8), C.c_int64()
        out, p = np.zeros(max(1, len(stream)), np.uint8), np.zeros(len(stream) // 36 + 1, np.uint32)
        assert L.svx_bam_sort_host(_abi.ptr(src), C.c_int64(len(stream)), C.c_int32(x["n_ref"]), _abi.ptr(out), _abi.ptr(p), C.c_int64(p.size), C.byref(n)) == 0
        assert out[:len(stream)].tobytes() == old_body and p[:n.value].tolist() == old_perm, name


def test_definition_file_groups_reads_for_the_query_name_batcher(corner, tmp_path):
    """the definition's file of the duplicated-reads case through the Python reader and batch.build_batch(mode="queryname"): a group is exactly the records
    that share a name - every name once, its primary analysed with its supplementary record as the one segment row"""
    x = corner["duplicated_reads"]
    path = str(tmp_path / "duplicated_reads.queryname.bam")
    with open(path, "wb") as fh:
        fh.write(_lib.text_gz_host(x["stream"]))
    assert bamsort.file(x["path"], "queryname") == open(path, "rb").read()
    bam = records.AlignmentFile(path)
    assert bam.header["HD"]["SO"] == "queryname" and bam.header["HD"]["SS"] == "queryname:lexicographical"
    recs = list(bam.fetch(until_eof=True))
    assert len(recs) == 120 and [r.query_name for r in recs] == ["name%02d" % (k // 3) for k in range(120)]
    assert [r.flag & (256 | 2048) for r in recs] == [0, 256, 2048] * 40                 # primary < secondary < supplementary inside a read
    hb = batch.build_batch(records.AlignmentFile(path), types.SimpleNamespace(min_mapq=0), mode="queryname")
    assert hb.n_rec == 120 and len(hb.read_names) == 40 and hb.read_names == ["name%02d" % k for k in range(40)]
    assert hb.arrays["read_id"].tolist() == [k // 3 for k in range(120)]
    live = [k for k in range(120) if not hb.arrays["flag"][k] & batch.SVX_FLAG_SKIP]
    placed = [k for k in range(40) if not recs[3 * k].flag & 4]
    assert live == sorted([3 * k for k in placed] + [3 * k + 2 for k in placed]) and len(placed) > 25      # the primary and the supplementary record of every placed read
    assert int(hb.n_seg) == len(placed) and hb.arrays["seg_off"].tolist() == np.cumsum([0] + [1 if (k % 3 == 0 and k // 3 in placed) else 0 for k in range(120)]).tolist()
    # the same records in file order: a name is scattered, the batcher sees 120 groups' worth of fragments
    assert len({r[36:42] for r in x["records"]}) == 40 and [NC.parsed(r)[0] for r in x["records"]] != sorted(NC.parsed(r)[0] for r in x["records"])


def test_host_build_under_the_sanitizers(tmp_path):
    """tools/bam_name_sort_host_test.cpp with bamsort_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer over 2 000 seeded streams (bad names and cut
    ends included) and 2 000 headers, against a plain reimplementation in that program: the same status, permutation and bytes every time, no report"""
    out = str(tmp_path / "bam_name_sort_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "bam_name_sort_host_test.cpp"), os.path.join(CSRC, "bamsort_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "2000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "2000 streams" in run.stdout and " 0 malformed" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    n_sorted, n_arg, n_range, n_headers, n_bad, n_cut = (int(run.stdout.split(w)[0].split()[-1]) for w in (" sorted", " bad argument", " bad range", " headers", " with a bad name", " cut short"))
    assert n_sorted > 1000 and n_arg > 300 and n_range > 20 and n_headers == 2000 and n_bad > 100 and n_cut > 100, run.stdout[-300:]


def test_symbols_declared_and_exported():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_bam_sort_begin_order", "svx_bam_sort_get_name_stats", "svx_bam_sort_host_order", "svx_bam_sort_header_host_order"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert re.search(r"#define SVX_SORT_COORDINATE\s+0\b", hdr) and re.search(r"#define SVX_SORT_QUERYNAME\s+1\b", hdr)
    assert _abi.SORT_ORDERS == {"coordinate": 0, "queryname": 1}
    assert L.svx_version() >= 108
    assert C.sizeof(_abi.BamNameSortStats) == 8 * (4 + 5 + 64) and C.sizeof(_abi.BamSortStats) == 8 * 25      # (the sort's own stats keep their layout)
