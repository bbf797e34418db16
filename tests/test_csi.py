"""The CSI index by its definition (svim_amd/csi.py) and by the host builds (svx_bam_index_csi_host, svx_text_index_csi_host; the kernels write the same
bytes, tests/test_gpu_csi.py holds them to that): the bin functions, the index against the trusted .bai / .tbi definitions where both exist, the two forms of
a bin's loffset, files and texts beyond 2^29, region queries against a scan, the host builds byte for byte, the refusals, the framed file.  No GPU."""
import bisect
import os
import random
import re
import struct
import subprocess
import tracemalloc

import numpy as np
import pytest

import bai_cases as BC
import csi_cases as CC
import text_index_cases as TIC
from svim_amd import _abi, _lib, bai, csi, records, tabix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """every corner file of bai_cases, large_file and the files beyond 2^29 with their rows and the definition's bytes, computed once"""
    d = str(tmp_path_factory.mktemp("csi_cases"))
    paths = BC.build_all(d) + [BC.many_references_file(d)]
    for name, make in (("large", BC.large_file), ("beyond_range", BC.beyond_range_file), ("near_2_31", CC.near_2_31_file)):
        path = os.path.join(d, name + ".bam")
        make(path)
        paths.append((name, path))
    out = {}
    for name, path in paths:
        n_ref, rows, v_end = bai.rows_of_bam(path)
        out[name] = dict(path=path, n_ref=n_ref, rows=rows, v_end=v_end, bytes=csi.build_bam_index(n_ref, rows, v_end))
    return out


@pytest.fixture(scope="module")
def texts():
    """the texts of text_index_cases (all within 2^29) and the texts beyond, with their block tables and the definition's bytes"""
    out = {}
    for name, preset, text in TIC.corner_texts() + [("seeded_bed", TIC.BED, TIC.seeded_bed_text())]:
        out[name] = dict(preset=preset, text=text, depth=5)
    for name, preset, text, depth in CC.beyond_texts():
        out[name] = dict(preset=preset, text=text, depth=depth)
    for x in out.values():
        x["stream"], x["coff"], x["uoff"] = TIC.tables(x["text"])
        x["bytes"] = csi.build_text_index(x["text"], x["coff"], x["uoff"], x["preset"])
    return out


def test_bin_functions():
    rng = random.Random(3)
    for _ in range(20000):
        beg = rng.randrange(1 << 29)
        end = min(beg + 1 + rng.randrange(1 << rng.randrange(1, 29)), 1 << 29)
        assert csi.reg2bin(beg, end, 14, 5) == tabix.reg2bin(beg, end)
    for max_end, depth in ((0, 5), (1 << 29, 5), ((1 << 29) + 1, 6), (1 << 32, 6), ((1 << 32) + 1, 7), (1 << 41, 9)):
        assert csi.depth_for(max_end) == depth, max_end
    assert csi.depth_for((1 << 31) - 1 + (1 << 32)) == 7 and csi.depth_for((1 << 40) + 65280) == 9      # the most a BAM and a text can need
    assert csi.depth_for((1 << 41) + 1) == csi.depth_for(6 << 40) == csi.MAX_DEPTH == 9 and csi.reg2bin(5, 6 << 40, 14, 9) == 0      # the depth stops at 9: bin 0
    for depth in (5, 6, 7, 9):
        top = 1 << (14 + 3 * depth)
        for _ in range(2000):
            beg = rng.randrange(top)
            b = csi.reg2bin(beg, beg + 1, 14, depth)
            assert csi.bin_start(b, depth) == (beg >> 14) << 14 and csi.bin_level(b, depth)[0] == depth
            lvl = rng.randrange(depth + 1)
            s = 14 + 3 * (depth - lvl)
            wide = csi.reg2bin((beg >> s) << s, ((beg >> s) + 1) << s, 14, depth)
            assert csi.bin_level(wide, depth)[0] == lvl and csi.bin_start(wide, depth) == (beg >> s) << s
            assert wide in csi.reg2bins(beg, beg + 1, 14, depth) and b in csi.reg2bins(beg, beg + 1, 14, depth)
        assert csi.reg2bin(0, top, 14, depth) == 0 and csi.reg2bin(top - 1, top, 14, depth) == csi.pseudo_bin(depth) - 2
    assert csi.pseudo_bin(5) == tabix.PSEUDO_BIN == 37450
    assert csi.reg2bin((1 << 32) - 1, 1 << 32, 14, 6) == 299592 and csi.reg2bin((1 << 41) - 1, 1 << 41, 14, 9) == 153391688
    assert csi.reg2bins(100, 200) == tabix.reg2bins(100, 200) and sorted(csi.reg2bins(5 << 14, 900 << 14)) == sorted(tabix.reg2bins(5 << 14, 900 << 14))


def test_tile_size_mirrors_the_header():
    src = open(os.path.join(CSRC, "binidx_kernels.hpp")).read()
    t = int(re.search(r"#define BINIDX_T (\d+)", src).group(1))
    items = int(re.search(r"#define BINIDX_RMAX_ITEMS (\d+)", src).group(1))
    assert re.search(r"#define BINIDX_RMAX_TILE \(BINIDX_T \* BINIDX_RMAX_ITEMS\)", src) and t * items == CC.RMAX_TILE


def _same_as_classic(ix, classic, what):
    assert ix["depth"] == 5 and ix["n_no_coor"] == classic["n_no_coor"], what
    assert ix["bins"] == classic["bins"] and ix["pseudo"] == classic["pseudo"], what
    for t, lo in enumerate(ix["loffset"]):
        assert set(lo) == set(classic["bins"][t]), (what, t)
        for b, v in lo.items():
            assert v == classic["linear"][t][csi.bin_start(b, 5) >> 14], (what, t, b)


def test_within_2_29_the_index_says_what_the_classic_one_says(files, texts):
    n = 0
    for name, x in files.items():
        if name in ("beyond_range", "near_2_31"):
            continue
        _same_as_classic(csi.parse_index(x["bytes"]), bai.parse_index(bai.build_index(x["n_ref"], x["rows"], x["v_end"])), name)
        n += 1
    assert n >= 16
    for name, x in texts.items():
        if x["depth"] != 5:
            continue
        ix = csi.parse_index(x["bytes"])
        classic = tabix.parse_index(tabix.build_index(x["text"], x["coff"], x["uoff"], x["preset"]))
        _same_as_classic(ix, classic, name)
        assert ix["names"] == classic["names"] and all(ix[k] == classic[k] for k in ("format", "col_seq", "col_beg", "col_end", "meta", "skip")), name
    assert len(csi.build_bam_index(3, [], 0)) == 20 + 3 * 4 + 8 and struct.unpack_from("<4siiii", csi.build_bam_index(3, [], 0)) == (b"CSI\1", 14, 5, 0, 3)


def test_the_two_forms_of_loffset_agree():
    checked = 0
    for seed in range(60):
        rows = CC.group_rows(seed, 5 + seed * 3, top=(1 << 27) if seed % 3 else 1 << 24, span=1 << 22, first_is_largest=seed % 5 == 0)
        depth = csi.depth_for(max(r[1] for r in rows))
        starts = {csi.bin_start(csi.reg2bin(r[0], r[1], 14, depth), depth) for r in rows} | {0}
        lin = tabix.parse_part(tabix.contig_part(rows, len(rows), 0), 0, "part")[2]
        assert csi.loffset_by_linear(rows, max(starts)) == lin[max(starts) >> 14]
        for s in starts:
            assert lin[s >> 14] == csi.loffset_by_running_max(rows, s), (seed, s)
            checked += 1
        if seed % 5 == 0:
            assert {csi.loffset_by_running_max(rows, s) for s in starts} == {rows[0][2]}            # the first row reaches behind every bin's start
    # ends beyond 2^31 and coordinates to 2^33: the linear index is too long to build - the form by windows, worked out per bin
    for seed in range(60, 100):
        rows = CC.group_rows(seed, 40, first_is_largest=seed % 4 == 0)
        depth = csi.depth_for(max(r[1] for r in rows))
        assert depth >= 7 and max(r[1] for r in rows) > 1 << 31
        part = csi.group_part(rows, len(rows), 0, depth)
        n_bin, at = struct.unpack_from("<i", part, 0)[0], 4
        for _ in range(n_bin - 1):
            b, loff, n_chunk = struct.unpack_from("<IQi", part, at)
            at += 16 + 16 * n_chunk
            w = csi.bin_start(b, depth) >> 14
            by_window = next(r[2] for r in rows if (r[1] - 1) >> 14 >= w)          # the first row that overlaps window w or a later one: begs ascend, so do vbegs
            assert loff == by_window == csi.loffset_by_running_max(rows, csi.bin_start(b, depth)), (seed, b)
            checked += 1
    assert checked > 3000


def test_beyond_2_29(files, texts):
    x = files["beyond_range"]
    with pytest.raises(bai.BaiError) as e:
        bai.build_index(x["n_ref"], x["rows"], x["v_end"])
    assert e.value.code == bai.E_RANGE
    ix = csi.parse_index(x["bytes"])
    assert ix["depth"] == 6 and ix["aux"] == b"" and ix["n_ref"] == 2 and sum(len(c) for c in ix["bins"][1].values()) >= 3
    near = csi.parse_index(files["near_2_31"]["bytes"])
    assert near["depth"] == 6 and max(near["bins"][1]) >= 37449 + 65536 and near["pseudo"][2] is None and near["n_no_coor"] == 1
    assert max(r[2] for r in files["near_2_31"]["rows"]) > 1 << 31
    for name, x in texts.items():
        ix = csi.parse_index(x["bytes"])
        assert ix["depth"] == x["depth"], name
        if x["depth"] > 5:
            with pytest.raises(tabix.TabixError) as e:
                tabix.build_index(x["text"], x["coff"], x["uoff"], x["preset"])
            assert e.value.code == tabix.E_RANGE, name
    x = texts["bed_end_2_40"]
    assert len(x["bytes"]) < 600 and max(csi.parse_index(x["bytes"])["bins"][0]) > 1 << 24
    tracemalloc.start()
    csi.build_text_index(x["text"], x["coff"], x["uoff"], x["preset"])
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 1 << 20, peak                                   # five rows: no linear index of 2^26 windows (512 MB) is materialised


def _fast_scan(rows):
    """csi.brute_force with the rows grouped per reference once and their intervals as arrays: region -> the same rows, in file order"""
    by_tid = {}
    for r in rows:
        if r[0] >= 0:
            by_tid.setdefault(r[0], []).append(r)
    cols = {t: (np.array([bai.interval(r)[0] for r in rs], dtype=np.int64), np.array([bai.interval(r)[1] for r in rs], dtype=np.int64)) for t, rs in by_tid.items()}

    def scan(tid, beg, end):
        if tid not in cols or end <= beg:
            return []
        begs, ends = cols[tid]
        return [by_tid[tid][k] for k in np.nonzero((begs < end) & (ends > beg))[0].tolist()]
    return scan


def _covered(ix, rows, regions, what):
    hits, scan = 0, _fast_scan(rows)
    for k, (tid, beg, end) in enumerate(regions):
        want = scan(tid, beg, end)
        if k % 100 == 0:
            assert want == csi.brute_force(rows, tid, beg, end), (what, tid, beg, end)          # (the fast scan is the slow one)
        chunks, low = csi.query(ix, tid, beg, end)
        if not want:
            continue
        assert low is not None, (what, tid, beg, end)
        begs = [c[0] for c in chunks]
        for r in want:
            k = bisect.bisect_right(begs, r[4]) - 1
            assert k >= 0 and chunks[k][0] <= r[4] < chunks[k][1], (what, tid, beg, end, r)
            assert r[4] >= low, (what, tid, beg, end, r)
        hits += len(want)
    return hits


def _fast_text_scan(text, preset):
    """tabix.brute_force with the text parsed once: region -> the same lines"""
    per = {}
    for line in bytes(text).split(b"\n"):
        r = tabix.parse_line(line, preset)
        if r is not None:
            per.setdefault(r[0], []).append((r[1], r[2], line))
    return lambda name, beg, end: [l for b, e, l in per.get(name, ()) if end > beg and b < end and e > beg]


def test_region_queries_cover_what_a_scan_finds(files, texts):
    for name, x in files.items():
        ix = csi.parse_index(x["bytes"])
        hits = _covered(ix, x["rows"], CC.regions(5, x["rows"], x["n_ref"], 1000), name)
        assert hits >= min(400, sum(1 for r in x["rows"] if r[0] >= 0)), (name, hits)
    rows, v_end = CC.random_rows(9, 3000, 3)
    ix = csi.parse_index(csi.build_bam_index(3, rows, v_end))
    assert ix["depth"] == 6 and _covered(ix, rows, CC.regions(6, rows, 3, 1000), "seeded") > 700
    ix9 = csi.parse_index(texts["bed_end_2_40"]["bytes"])
    for beg, end in ((0, 1 << 30), ((1 << 33) - 5, (1 << 33) + 70000), (1 << 35, (1 << 35) + 1), (3, 4), ((1 << 40) - 20, 1 << 41)):
        # (a wide region is answered from the bins the group has, a narrow one from reg2bins: one set)
        assert sorted(csi.candidate_bins(ix9, 0, beg, end)) == sorted(set(csi.reg2bins(beg, end, 14, 9)) & set(ix9["bins"][0])), (beg, end)
    for name, x in texts.items():
        ix = csi.parse_index(x["bytes"])
        hits, scan = 0, _fast_text_scan(x["text"], x["preset"])
        for k, (contig, beg, end) in enumerate(CC.text_regions(7, x["text"], x["preset"], 1000)):
            want = scan(contig, beg, end)
            if k % 100 == 0:
                assert want == tabix.brute_force(x["text"], x["preset"], contig, beg, end), (name, contig, beg, end)      # (the fast scan is the slow one)
            assert csi.query_text(ix, x["stream"], contig, beg, end) == want, (name, contig, beg, end)
            hits += len(want)
        assert hits > 0 or not ix["names"], name


def test_host_builds_equal_the_definition(files, texts):
    for name, x in files.items():
        assert _lib.bam_index_host(x["n_ref"], x["rows"], x["v_end"], fmt="csi") == x["bytes"], name
    for name, x in texts.items():
        for base in (0, 4242):
            want = x["bytes"] if base == 0 else csi.build_text_index(x["text"], x["coff"], x["uoff"], x["preset"], base)
            assert _lib.text_index_host(x["text"], x["coff"], x["uoff"], x["preset"], base, fmt="csi") == want, (name, base)
    # a hand-made table with ends beyond every depth (no reader makes one): depth 9 and bin 0, in the definition as in the host build
    rows = [(0, 5, 900, 0, 1 << 16), (0, 70000, 6 << 40, 0, 2 << 16), (0, 70001, (1 << 41) + 1, 16, 3 << 16), (0, 1 << 30, (1 << 30) + 7, 0, 4 << 16), (1, 3, 1 << 41, 0, 5 << 16)]
    data = csi.build_bam_index(2, rows, 6 << 16)
    ix = csi.parse_index(data)
    assert _lib.bam_index_host(2, rows, 6 << 16, fmt="csi") == data and ix["depth"] == 9 and len(ix["bins"][0][0]) == 1 and list(ix["bins"][1]) == [0]
    for seed, n_ref, rows_v in ((1, 25, BC.random_rows(1, 100000, 25)), (2, 3, CC.random_rows(2, 100000, 3, span_bits=31))):
        rows, v_end = rows_v
        data = csi.build_bam_index(n_ref + 2, rows, v_end)
        assert _lib.bam_index_host(n_ref + 2, rows, v_end, fmt="csi") == data, seed
        assert csi.parse_index(data)["depth"] == (5 if seed == 1 else 6)
        assert _covered(csi.parse_index(data), rows, CC.regions(seed, rows, n_ref, 1000), seed) > 700


def test_refusals_and_capacity(tmp_path, files):
    import ctypes as C
    path = str(tmp_path / "swapped.bam")
    BC.swapped_file(path)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    for build in (csi.build_bam_index, lambda *a: _lib.bam_index_host(*a, fmt="csi")):
        with pytest.raises(bai.BaiError) as e:
            build(n_ref, rows, v_end)
        assert e.value.code == bai.E_ORDER
    x = files["beyond_range"]
    with pytest.raises(ValueError):
        csi.build_bam_index(1, x["rows"], x["v_end"])
    with pytest.raises(_lib.SvxError) as e:
        _lib.bam_index_host(1, x["rows"], x["v_end"], fmt="csi")
    assert not isinstance(e.value, bai.BaiError)
    for name, preset, text, code in TIC.refused_texts():
        _, coff, uoff = TIC.tables(text)
        for build in (csi.build_text_index, lambda *a: _lib.text_index_host(*a, fmt="csi")):
            if code == tabix.E_ORDER:
                with pytest.raises(tabix.TabixError) as e:
                    build(text, coff, uoff, preset)
                assert e.value.code == tabix.E_ORDER, name
            else:
                assert csi.parse_index(build(text, coff, uoff, preset))["depth"] == 6, name          # out of range for a .tbi only
    cols = [np.ascontiguousarray([r[k] for r in x["rows"]], dtype=dt) for k, dt in enumerate((np.int32, np.int32, np.int64, np.uint16, np.uint64))]
    want = len(x["bytes"])
    for cap in (0, 1, want - 1):
        out, n = np.full(max(1, cap) + 8, 0xab, dtype=np.uint8), C.c_int64(-1)
        rc = _lib.lib().svx_bam_index_csi_host(C.c_int32(x["n_ref"]), C.c_int64(len(x["rows"])), *[_abi.ptr(c) for c in cols], C.c_uint64(x["v_end"]), _abi.ptr(out), C.c_int64(cap),
                                               C.byref(n))
        assert rc == _abi.SVX_E_CAPACITY and n.value == want and (out == 0xab).all(), cap
    text = np.frombuffer(b"chr1\t5\t536870913\n", dtype=np.uint8)
    _, coff, uoff = TIC.tables(text.tobytes())
    co, uo, n = np.asarray(coff, dtype=np.int64), np.asarray(uoff, dtype=np.int64), C.c_int64(-1)
    rc = _lib.lib().svx_text_index_csi_host(_abi.ptr(text), C.c_int64(text.size), _abi.ptr(co), _abi.ptr(uo), C.c_int64(co.size - 1), C.c_int(TIC.BED), C.c_int64(0), None, C.c_int64(0), C.byref(n))
    assert rc == _abi.SVX_E_CAPACITY and n.value == len(csi.build_text_index(text.tobytes(), coff, uoff, TIC.BED))


def test_index_file_round_trip(tmp_path, files):
    for name in ("straddle_two_and_three_blocks", "references_without_records", "near_2_31", "large"):
        x = files[name]
        path = str(tmp_path / (name + ".csi"))
        with open(path, "wb") as fh:
            fh.write(csi.frame(x["bytes"]))
        assert csi.read_file(path) == x["bytes"], name
        with open(path, "rb") as fh:
            assert fh.read(4) == b"\x1f\x8b\x08\x04"
        pairs = records.read_index(path)
        if name != "near_2_31":
            bai_path = str(tmp_path / (name + ".bai"))
            with open(bai_path, "wb") as fh:
                fh.write(bai.build_index(x["n_ref"], x["rows"], x["v_end"]))
            assert records.read_index(bai_path) == records.read_bai(bai_path) == pairs, name
        placed = [r for r in x["rows"] if r[0] >= 0]
        vend = {r[4]: v for r, v in zip(x["rows"], [r[4] for r in x["rows"][1:]] + [x["v_end"]])}
        for t in range(x["n_ref"]):
            mine = [r for r in placed if r[0] == t]
            assert pairs[t] == ((mine[0][4], vend[mine[-1][4]]) if mine else None), (name, t)
    assert len(files["large"]["bytes"]) > 2 * 65280                 # a framed file of several blocks


def test_host_builds_under_the_sanitizers(tmp_path):
    """tools/csi_host_test.cpp with the two host builds under AddressSanitizer + UndefinedBehaviorSanitizer over a seeded fuzz of row tables and texts, sorted,
    unsorted, huge and garbage: every call ends in an index that walks back to its size or in a refusal that is not SVX_E_RANGE, no report"""
    out = str(tmp_path / "csi_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(REPO, "tools", "csi_host_test.cpp"),
                            os.path.join(CSRC, "bamindex_host.cpp"), os.path.join(CSRC, "textindex_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "6000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "6000 inputs" in run.stdout and " 0 malformed" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    indexed, order, tid, deep = (int(run.stdout.split(w)[0].split()[-1]) for w in (" indexed", " out of order", " bad tid", " deeper than 5"))
    assert indexed > 2000 and order > 500 and tid > 20 and deep > 500, run.stdout[-300:]


def test_symbols_declared_and_exported():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_bam_index_finish_fmt", "svx_bam_sort_index_fmt", "svx_text_index_fmt", "svx_bam_index_csi_host", "svx_text_index_csi_host"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"SVX_INDEX_CLASSIC = 0, SVX_INDEX_CSI = 1", header) and (_abi.INDEX_CLASSIC, _abi.INDEX_CSI) == (0, 1)
    assert _abi.auto_index_format([1 << 29, 5], "bai") == "bai" and _abi.auto_index_format([5, (1 << 29) + 1], "tbi") == "csi"
    # a format is named by its kind of file: a BAM has no .tbi, a text no .bai
    assert (_abi.index_format("bai", "bai"), _abi.index_format("tbi", "tbi"), _abi.index_format("csi", "bai"), _abi.index_format(7, "tbi")) == (0, 0, 1, 7)
    for call in (lambda: _abi.index_format("tbi", "bai"), lambda: _abi.index_format("bai", "tbi"), lambda: _abi.index_format("auto", "bai"),
                 lambda: _lib.bam_index_host(1, [], 0, fmt="tbi"), lambda: _lib.text_index_host(b"", [0, 28], [0, 0], 1, 0, fmt="bai")):
        with pytest.raises(ValueError):
            call()
