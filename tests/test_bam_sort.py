"""The coordinate sort by its definition (svim_amd/bamsort.py) and by the host build of csrc/bamsort_core.hpp (svx_bam_sort_host, svx_bam_sort_header_host; the
kernels write the same bytes, tests/test_gpu_bam_sort.py holds them to that): key order, stability and the header rules on every corner file of
tests/bam_sort_cases.py, the sorted file read back by both Python readers, the host build equal to the definition byte for byte and permutation for
permutation, the refusals, the host build under the sanitizers, the block layout of the file.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bam_sort_cases as SC
from svim_amd import _abi, _lib, bai, bamsort, records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    """every corner file with the definition's stream and permutation, computed once"""
    d = str(tmp_path_factory.mktemp("bam_sort_cases"))
    out = SC.build_all(d)
    for x in out.values():
        x["stream"], x["perm"] = SC.definition(x)
    return out


def _text(hdr):
    return hdr[8:8 + struct.unpack_from("<i", hdr, 4)[0]]


def test_definition_orders_by_key_and_keeps_equal_keys_in_file_order(corner):
    for name, x in corner.items():
        recs, perm = x["records"], x["perm"]
        assert sorted(perm) == list(range(len(recs))), name
        keys = [bamsort.sort_key(recs[k][4:]) for k in perm]
        assert keys == sorted(keys), name
        assert all(a < b for a, b, ka, kb in zip(perm, perm[1:], keys, keys[1:]) if ka == kb), name
        hdr = bamsort.sorted_header(x["header"])
        assert x["stream"] == hdr + b"".join(recs[k] for k in perm), name
        assert bamsort.sorted_stream(x["path"]) == x["stream"], name
    # the files hold the corners they are named for
    c = corner
    assert c["no_records"]["perm"] == [] and c["one_record"]["perm"] == [0]
    assert c["already_in_order"]["perm"] == list(range(306)) and c["reverse_order"]["perm"] != list(range(305, -1, -1))      # (equal keys keep their file order)
    x = c["five_keys_forty_names"]
    assert len({bamsort.sort_key(r[4:]) for r in x["records"]}) == 5 and len({r[36:42] for r in x["records"]}) == 40
    x = c["forward_and_reverse_at_one_position"]
    flags = [struct.unpack_from("<H", x["records"][k], 18)[0] for k in x["perm"]]
    assert [f & 16 for f in flags] == [0] * 4 + [16] * 5 and x["perm"] == [1, 4, 5, 8, 0, 2, 3, 6, 7]
    x = c["pos_minus_one_on_a_placed_reference"]
    first_of_2 = [struct.unpack_from("<ii", x["records"][k], 4) for k in x["perm"] if struct.unpack_from("<i", x["records"][k], 4)[0] == 2]
    assert [p for _, p in first_of_2][:3] == [-1, -1, -1] and struct.unpack_from("<i", x["records"][x["perm"][-1]], 4)[0] == -1
    x = c["unplaced_scattered"]
    tail = [struct.unpack_from("<ii", x["records"][k], 4) for k in x["perm"]][-27:]
    assert all(t == -1 for t, _ in tail) and [p for _, p in tail] == sorted(p for _, p in tail) and {p for _, p in tail} >= {-1, 100, 121}
    ends = lambda x: set(np.cumsum([len(bamsort.sorted_header(x["header"]))] + [len(x["records"][k]) for k in x["perm"]]).tolist())      # noqa: E731
    assert bamsort.BLOCK in ends(c["record_ends_at_the_block_edge"]) and bamsort.BLOCK - 2 in ends(c["length_field_straddles_the_block_edge"])
    assert max(len(r) for r in c["record_longer_than_two_blocks"]["records"]) > 2 * bamsort.BLOCK
    assert {len(r) - 4 for r in c["records_of_36_to_40_bytes"]["records"]} == {36, 37, 38, 39, 40}
    ops = sorted(struct.unpack_from("<H", r, 16)[0] for r in c["long_cigars_and_a_cg_tag"]["records"])
    assert ops[-4:] == [4096, 4097, 65535, 65535] or ops[-3:] == [4096, 4097, 65535]
    assert any(b"CGB" in r for r in c["long_cigars_and_a_cg_tag"]["records"])


def test_definition_header_rules(corner):
    sq = SC.sq_lines().encode()
    want = {"header_so_queryname": b"@HD\tVN:1.6\tSO:coordinate\n" + sq,
            "header_so_unsorted_go_query": b"@HD\tVN:1.6\tSO:coordinate\n" + sq + b"@CO\tSO:queryname stays here\n",
            "header_hd_without_so": b"@HD\tVN:1.5\tSO:coordinate\n" + sq,
            "header_without_hd": b"@HD\tVN:1.6\tSO:coordinate\n" + sq + b"@PG\tID:x\n",
            "header_nul_padded": b"@HD\tVN:1.6\tSO:coordinate\n" + sq,
            "header_without_text": b"@HD\tVN:1.6\tSO:coordinate\n"}
    for name, text in want.items():
        old, new = corner[name]["header"], bamsort.sorted_header(corner[name]["header"])
        assert _text(new) == text and len(new) == 8 + len(text) + len(old) - 8 - len(_text(old)), name
        assert new[8 + len(text):] == old[8 + len(_text(old)):], name                                  # the reference dictionary, unchanged
        assert bamsort.sorted_header(new) == new, name
        assert _lib.bam_sort_header_host(old) == new, name
    assert len(_text(corner["header_nul_padded"]["header"])) - len(_text(corner["header_nul_padded"]["header"]).rstrip(b"\0")) == 37
    for text in (b"@HD", b"@HD\t", b"@HD\tSO:x", b"@HD\tGO:q\tSO:a\tSO:b\tSS:c\t\tXY:z", b"@HD\tVN:1\r\n@SQ\tSN:a\tLN:1\n", b"@hd\tVN:1\n", b"\0@HD\tVN:1\n"):
        old = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
        new = bamsort.sorted_header(old)
        assert _lib.bam_sort_header_host(old) == new, text
        line = _text(new).split(b"\n")[0]
        assert line.startswith(b"@HD\t") and b"SO:coordinate" in line.split(b"\t") and not any(f[:3] in (b"GO:", b"SS:") for f in line.split(b"\t")), text
    text = b"@HD\tGO:q\tSO:a\tSO:b\tSS:c\t\tXY:z"
    assert _text(bamsort.sorted_header(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0))) == b"@HD\tSO:coordinate\tSO:coordinate\t\tXY:z"


def _write_definition_file(x, path):
    data = _lib.text_gz_host(x["stream"])
    with open(path, "wb") as fh:
        fh.write(data)
    return data


def test_definition_file_reads_back_and_is_in_order(corner, tmp_path):
    for name, x in corner.items():
        path = str(tmp_path / (name + ".sorted.bam"))
        _write_definition_file(x, path)
        n_ref, rows, v_end = bai.rows_of_bam(path)
        assert n_ref == x["n_ref"] and bai.check_order(rows) == 0, name
        rows_in = bai.rows_of_bam(x["path"])[1]
        assert sorted(r[:4] for r in rows) == sorted(r[:4] for r in rows_in), name
        assert [r[:4] for r in rows] == [rows_in[k][:4] for k in x["perm"]], name
        hdr_len = len(bamsort.sorted_header(x["header"]))
        starts = np.cumsum([hdr_len] + [len(x["records"][k]) for k in x["perm"]])[:-1].tolist()
        coff = [b[0] for b in bai.bgzf_blocks(open(path, "rb").read())]
        assert [r[4] for r in rows] == [(coff[u // bamsort.BLOCK] << 16) | (u % bamsort.BLOCK) for u in starts], name
        assert len(bai.build_index(n_ref, rows, v_end)) >= 16 + 8 * n_ref, name
        if name in ("already_in_order", "long_cigars_and_a_cg_tag", "unplaced_scattered", "header_without_hd"):
            # the Python reader: the same multiset of records as the input file gives it
            key = lambda a: (a.query_name, a.flag, a.reference_id, a.reference_start, tuple(a.cigartuples or ()), a.query_sequence)      # noqa: E731
            got, src = records.AlignmentFile(path), records.AlignmentFile(x["path"])
            assert got.header["HD"]["SO"] == "coordinate"
            a, b = [key(r) for r in got.fetch(until_eof=True)], [key(r) for r in src.fetch(until_eof=True)]
            assert sorted(a) == sorted(b) and len(a) == len(x["records"]) and [b[k] for k in x["perm"]] == a, name


def test_host_build_equals_the_definition(corner):
    for name, x in corner.items():
        body, perm = _lib.bam_sort_host(b"".join(x["records"]), x["n_ref"])
        assert perm.tolist() == x["perm"], name
        assert body == x["stream"][len(bamsort.sorted_header(x["header"])):], name


@pytest.mark.parametrize("seed", [81, 82])
def test_host_build_equals_the_definition_on_100000_records(seed):
    rng = np.random.default_rng(seed)
    n, n_ref = 100000, 24
    rec = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                    ("l_seq", "<i4"), ("next_tid", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S8")])
    a = np.zeros(n, dtype=rec)
    a["block_size"], a["l_read_name"], a["next_tid"], a["next_pos"] = rec.itemsize - 4, 8, -1, -1
    a["tid"] = rng.integers(-1, n_ref, n)
    a["pos"] = np.where(rng.random(n) < 0.3, rng.integers(-1, 40, n), rng.integers(-1, 1 << 28, n))          # many equal keys, and wide ones
    a["flag"] = rng.choice(np.array([0, 16, 4, 20, 256, 272], dtype=np.uint16), n)
    a["name"] = np.char.zfill(np.arange(n).astype("S7"), 7)
    stream = a.tobytes()
    want_body, want_perm = bamsort.sort_records(stream, n_ref)
    body, perm = _lib.bam_sort_host(stream, n_ref)
    assert perm.tolist() == want_perm and body == want_body
    order = np.lexsort((np.arange(n), a["flag"] & 16, (a["pos"].astype(np.int64) + 1) & 0xffffffff, a["tid"].astype(np.int64) & 0xffffffff))
    assert perm.tolist() == order.tolist()


def test_refusals(corner):
    recs = corner["already_in_order"]["records"]
    good, n_ref = b"".join(recs[:20]), 6

    def patched(k, at, value):
        b = bytearray(good)
        p = sum(len(r) for r in recs[:k])
        b[p + at:p + at + 4] = struct.pack("<i", value)
        return bytes(b)
    cases = [(patched(3, 4, -2), bamsort.E_ARG), (patched(3, 4, n_ref), bamsort.E_ARG), (patched(7, 8, -2), bamsort.E_RANGE), (patched(0, 0, 31), bamsort.E_ARG),
             (good[:-1], bamsort.E_ARG), (good + b"\x20\0", bamsort.E_ARG), (patched(9, 4, -7), bamsort.E_ARG)]
    both = bytearray(patched(7, 8, -2))
    p = sum(len(r) for r in recs[:12]) + 4
    both[p:p + 4] = struct.pack("<i", 99)
    cases.append((bytes(both), bamsort.E_ARG))                                    # both kinds in one stream: E_ARG
    for stream, code in cases:
        with pytest.raises(bamsort.BamSortError) as e:
            bamsort.sort_records(stream, n_ref)
        assert e.value.code == code
        with pytest.raises(bamsort.BamSortError) as e:
            _lib.bam_sort_host(stream, n_ref)
        assert e.value.code == code
    assert bamsort.E_ARG == _abi.SVX_E_ARG and bamsort.E_RANGE == _abi.SVX_E_RANGE
    assert bamsort.sort_records(b"", 0) == (b"", []) and _lib.bam_sort_host(b"", 0)[0] == b""
    # a permutation buffer that is too small: the count comes back, nothing is written
    perm, n = np.full(8, 0xabababab, dtype=np.uint32), C.c_int64(-1)
    src = np.frombuffer(good, dtype=np.uint8)
    rc = _lib.lib().svx_bam_sort_host(_abi.ptr(src), C.c_int64(len(good)), C.c_int32(n_ref), None, _abi.ptr(perm), C.c_int64(8), C.byref(n))
    assert rc == _abi.SVX_E_CAPACITY and n.value == 20 and (perm == 0xabababab).all()


def test_host_build_under_the_sanitizers(tmp_path):
    """tools/bam_sort_host_test.cpp with bamsort_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer over a seeded fuzz of sorted, shuffled, refused,
    truncated and garbage record streams and of headers: every call ends in a stream that is checked record by record or in one of the refusals, no report"""
    out = str(tmp_path / "bam_sort_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "bam_sort_host_test.cpp"), os.path.join(CSRC, "bamsort_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "4000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "4000 streams" in run.stdout and " 0 malformed" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    n_sorted, n_arg, n_range, n_headers = (int(run.stdout.split(w)[0].split()[-1]) for w in (" sorted", " bad argument", " bad range", " headers"))
    assert n_sorted > 2000 and n_arg > 500 and n_range > 50 and n_headers == 4000, run.stdout[-300:]


def test_blocks_of_the_file(corner, tmp_path):
    """blocks of exactly 65 280 stream bytes (the last one shorter), the end-of-file block, every block at most 65 536 bytes and sound for zlib down to its CRC"""
    for name in ("no_records", "record_ends_at_the_block_edge", "record_longer_than_two_blocks", "long_cigars_and_a_cg_tag", "unplaced_scattered"):
        x = corner[name]
        data = _write_definition_file(x, str(tmp_path / (name + ".bam")))
        assert data == bamsort.file(x["path"]) and data.endswith(_abi.TEXT_GZ_EOF), name
        at, sizes = 0, []
        while at < len(data):
            bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
            assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and bsize <= 65536, name
            payload = zlib.decompress(data[at + 18:at + bsize - 8], -15)
            crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
            assert isize == len(payload) and crc == zlib.crc32(payload) & 0xffffffff, name
            assert payload == x["stream"][sum(sizes):sum(sizes) + isize], name
            sizes.append(isize)
            at += bsize
        n = len(x["stream"])
        assert sizes == [bamsort.BLOCK] * (n // bamsort.BLOCK) + ([n % bamsort.BLOCK] if n % bamsort.BLOCK else []) + [0], name
        assert len(sizes) == bamsort.n_blocks(n), name


def test_symbols_declared_and_exported():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_bam_sort_begin", "svx_bam_sort_finish", "svx_bam_sort_abort", "svx_bam_sort_count", "svx_bam_sort_encode", "svx_bam_sort_fetch", "svx_bam_sort_index",
                 "svx_bam_sort_permutation", "svx_bam_sort_get_stats", "svx_bam_sort_host", "svx_bam_sort_header_host"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert L.svx_version() >= 103
    assert C.sizeof(_abi.BamSortStats) == 8 * 25
