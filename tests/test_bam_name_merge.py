"""The merge of several BAM files in query-name order by its definition (svim_amd/bammerge.py, order="queryname"; the runs: svim_amd/bamsort.py: runs_of) and
by the host build (svx_bam_merge_header_host_order, svx_bam_merge_host_order in csrc/bamsort_host.cpp), on the CPU: the definition against a brute force over
fields parsed here, the split cases against the EXISTING one-file definition, the header line for line, the default order through every new signature equal
to the old call, runs + merge_runs + piece_cuts in this order, the host build byte for byte, the refusals with their codes and precedence, the name table's
word against the name's own (csrc/bamsort_core.hpp), and tools/bam_name_merge_host_test.cpp under the sanitizers.  The session on the device:
tests/test_gpu_bam_name_merge.py."""
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

import bam_merge_cases as MC
import bam_name_merge_cases as NM
import bam_name_sort_cases as NC
from svim_amd import _abi, _lib, bammerge, bamsort

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return NM.build_all(str(tmp_path_factory.mktemp("bam_name_merge_cases")))


def _accepted(cases, *prefixes):
    return [(name, c) for name, c in cases.items() if "error" not in c and (not prefixes or name.split(":")[0] in prefixes)]


def _translated(c):
    """every record of the case as the merged file holds it, in global order, by bammerge.translate_record alone"""
    headers = [x["header"] for x in c["inputs"]]
    maps = [list(range(c["inputs"][0]["n_ref"]))] if len(headers) == 1 else bammerge.tid_maps([bammerge.parse_header(h)[1] for h in headers])
    out = []
    for x, m in zip(c["inputs"], maps):
        out += [r if m == list(range(x["n_ref"])) else bammerge.translate_record(r, m) for r in x["records"]]
    return out, maps


def test_definition_equals_a_brute_force(cases):
    """sorted(range(n), key=(name, rank, global number)) over fields parsed in the test; the stream is the translated records in that order behind the header"""
    n_seen = 0
    for name, c in _accepted(cases):
        recs, _ = _translated(c)
        want = sorted(range(len(recs)), key=lambda k: NM.parsed(recs[k]) + (k,))
        stream, perm = NM.definition(c)
        assert list(perm) == want, name
        header = bammerge.merged_header([x["header"] for x in c["inputs"]], "queryname")
        assert stream == header + b"".join(recs[k] for k in want), name
        n_seen += len(recs)
    assert n_seen > 30000


def test_split_cases_equal_the_one_file_name_sort(cases):
    """the expectation knows nothing of the new code: bamsort.sort_records(order="queryname") of the ONE file, its stream and - through origin - its permutation"""
    for name, c in _accepted(cases, "split"):
        one = c["one"]
        body, perm_one = bamsort.sort_records(b"".join(one["records"]), one["n_ref"], "queryname")
        stream, perm = NM.definition(c)
        _, _, at = bamsort.split_header(stream)
        assert stream[at:] == body, name
        assert [c["origin"][g] for g in perm] == list(perm_one), name
    # dealt round-robin, equal keys sit in different files and leave in file order, then in-file order - not in the one file's order
    c = cases["ties:stable_ties/3"]
    assert len(c["one"]["records"]) == 5000 and list(NM.definition(c)[1]) == list(range(5000)) and c["origin"][:3] == [0, 3, 6]
    for name, c in _accepted(cases, "ties"):
        stream, perm = NM.definition(c)
        keys = [NM.parsed(c["one"]["records"][c["origin"][g]]) for g in perm]
        assert keys == sorted(keys) and all(a < b for a, b, ka, kb in zip(perm, perm[1:], keys, keys[1:]) if ka == kb), name


def test_one_input_is_the_name_sort_byte_for_byte(cases):
    for name, c in _accepted(cases, "split"):
        one = c["one"]
        raw = one["header"] + b"".join(one["records"])
        stream, perm = bammerge.stream_of([raw], "queryname")
        body, perm_one = bamsort.sort_records(b"".join(one["records"]), one["n_ref"], "queryname")
        assert stream == bamsort.sorted_header(one["header"], "queryname") + body and list(perm) == list(perm_one), name
        assert bammerge.merged_header([one["header"]], "queryname") == bamsort.sorted_header(one["header"], "queryname"), name


def test_header_line_for_line(cases):
    seen = 0
    for name, c in cases.items():
        if not name.startswith("header:"):
            continue
        headers = [x["header"] for x in c["inputs"]]
        if "error" in c:
            with pytest.raises(bammerge.BamMergeError) as e:
                bammerge.merged_header(headers, "queryname")
            assert e.value.code == c["error"], name
            with pytest.raises(bammerge.BamMergeError) as e:
                _lib.bam_merge_header_host(headers, "queryname")
            assert e.value.code == c["error"], name
            continue
        made = bammerge.merged_header(headers, "queryname")
        text, refs = bammerge.parse_header(made)
        lines = text.decode().split("\n")
        assert lines[-1] == "" and lines[:-1] == c["lines"], name
        assert lines[0].split("\t")[2:4] == ["SO:queryname", "SS:queryname:lexicographical"], name
        # every line behind the first is the coordinate merge's, and so is the dictionary
        old_text, old_refs = bammerge.parse_header(bammerge.merged_header(headers))
        assert old_text.split(b"\n")[1:] == text.split(b"\n")[1:] and old_refs == refs, name
        seen += 1
    assert seen == 9 and set(NM.QN_FIRST_LINE) == {n for n, (_, want) in MC.HEADER_CASES.items() if not isinstance(want, int)}


def test_coordinate_order_through_every_new_signature_is_the_old_call(tmp_path):
    """order="coordinate", given or left out, changes no byte: merged_text, merged_header, merge, stream_of, file, runs_of, and the host builds"""
    for fn in (bammerge.merged_text, bammerge.merged_header, bammerge.merge, bammerge.stream_of, bammerge.file, bamsort.runs_of, _lib.bam_merge_header_host, _lib.bam_merge_host):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "order" and last.default == "coordinate", fn.__name__
    old = MC.build_all(str(tmp_path))
    for name in ("ties:five_keys_forty_names/3", "directed:reversed_dictionary", "directed:appends_two_contigs", "header:pg_same_id_three_files", "header:no_hd_line"):
        c = old[name]
        headers = [x["header"] for x in c["inputs"]]
        assert bammerge.merged_header(headers, "coordinate") == bammerge.merged_header(headers) == bammerge.merged_header(headers, order="coordinate"), name
        parsed = [bammerge.parse_header(h) for h in headers]
        refs = bammerge.merged_dictionary([p[1] for p in parsed])
        assert bammerge.merged_text([p[0] for p in parsed], refs, "coordinate") == bammerge.merged_text([p[0] for p in parsed], refs), name
        stream, perm = bammerge.stream_of(MC.raws(c), "coordinate")
        assert (stream, perm) == bammerge.stream_of(MC.raws(c)), name
        maps = bammerge.tid_maps([p[1] for p in parsed])
        files = [(b"".join(x["records"]), x["n_ref"], m) for x, m in zip(c["inputs"], maps)]
        assert bammerge.merge(files, "coordinate") == bammerge.merge(files), name
        paths = [x["path"] for x in c["inputs"]]
        assert bammerge.file(paths, "coordinate") == bammerge.file(paths), name
        hdr, hmaps = _lib.bam_merge_header_host(headers, "coordinate")
        assert (hdr, hmaps) == _lib.bam_merge_header_host(headers) and hdr == bammerge.merged_header(headers), name
        body, hperm = _lib.bam_merge_host(files, len(refs), "coordinate")
        body0, hperm0 = _lib.bam_merge_host(files, len(refs))
        assert body == body0 and (hperm == hperm0).all() and hdr + body == stream, name
        x = c["inputs"][0]
        ends = [len(x["records"]) // 2, len(x["records"])]
        assert bamsort.runs_of(b"".join(x["records"]), x["n_ref"], ends, "coordinate") == bamsort.runs_of(b"".join(x["records"]), x["n_ref"], ends), name
    with pytest.raises(ValueError):
        bammerge.merged_header([old["header:no_hd_line"]["inputs"][0]["header"]], "natural")
    with pytest.raises(ValueError):
        bamsort.runs_of(b"", 1, [0], "natural")


def _global_records(c):
    recs, _ = _translated(c)
    return recs


def test_runs_in_name_order_merge_to_the_sort(cases):
    """runs_of(order="queryname") + merge_runs = sort_records over the translated records: at every single cut point, at seeded sets of 2, 3 and n runs, with
    empty runs - and every run contributes a contiguous in-run range to any contiguous range of the global order"""
    rng = random.Random(401)
    n_cuts = 0
    for name, c in _accepted(cases, "split", "ties", "dict", "edge"):
        if name.split(":")[1].split("/")[0] in ("stable_ties", "long_shared_prefix", "distinct_first_word", "every_alignment") and not name.endswith("/2"):
            continue                                                      # (the large files once)
        recs = _global_records(c)
        n = len(recs)
        body, perm = bamsort.sort_records(b"".join(recs), 1 << 30, "queryname") if n else (b"", [])
        singles = range(n + 1) if n <= 150 else sorted(rng.sample(range(n + 1), 12) + [0, 1, n - 1, n])
        sets = [[cut, n] for cut in singles]
        if n:
            sets += [sorted(rng.randrange(n + 1) for _ in range(k)) + [n] for k in (2, 3)] + [list(range(1, n + 1)) if n <= 600 else sorted(rng.sample(range(n + 1), 300)) + [n]]
            sets += [[0, 0, n // 2, n // 2, n, n], [0, n], [n, n]]
        for ends in sets:
            runs = bamsort.runs_of(recs, 1 << 30, ends, "queryname")
            assert [len(r) for r in runs] == [b - a for a, b in zip([0] + ends, ends)]
            got = bamsort.merge_runs(runs)
            assert got[0] == body and got[1] == list(perm), (name, ends[:5])
            n_cuts += 1
        if n and n <= 600:                                                # the property piece_cuts rests on, stated directly
            runs = bamsort.runs_of(recs, 1 << 30, sets[-4], "queryname")
            where = {k: (r, i) for r, run in enumerate(runs) for i, (_, k, _) in enumerate(run)}
            for _ in range(20):
                p0 = rng.randrange(n + 1)
                p1 = rng.randrange(p0, n + 1)
                for r in range(len(runs)):
                    idx = [where[k][1] for k in perm[p0:p1] if where[k][0] == r]
                    assert idx == list(range(idx[0], idx[0] + len(idx))) if idx else True, name
    assert n_cuts > 1000                                                  # (the loop ran: a dozen small files at every cut point alone)


def test_piece_cuts_give_contiguous_ranges_whose_merge_is_the_piece(cases):
    for name in ("dict:three_dictionaries", "ties:duplicated_reads/3", "edge:run_edge_lengths", "edge:run_edge_64_rounds", "split:padded_names/2"):
        recs = _global_records(cases[name])
        n = len(recs)
        body, perm = bamsort.sort_records(b"".join(recs), 1 << 30, "queryname")
        first_byte = 137
        for ends in ([n // 3, 2 * n // 3, n], [1, 1, n - 1, n], [n]):
            runs = bamsort.runs_of(recs, 1 << 30, ends, "queryname")
            stream = b"\0" * first_byte + body
            for step in (1 * bamsort.BLOCK, 3 * bamsort.BLOCK, 4096 * bamsort.BLOCK, 64, 997):      # pieces of 1, 3 and 4096 blocks; small ones, so that these files have many
                at = 0
                for p0, p1, cuts in bamsort.piece_cuts(runs, perm, first_byte, step):
                    assert all(0 <= a <= b <= len(run) for run, (a, b) in zip(runs, cuts))
                    merged, mperm = bamsort.merge_runs([run[a:b] for run, (a, b) in zip(runs, cuts)])
                    assert mperm == list(perm[p0:p1]), (name, ends, step)
                    lo = first_byte + sum(len(recs[k]) for k in perm[:p0])
                    assert stream[lo:lo + len(merged)] == merged, (name, ends, step)
                    if at + step > first_byte:                            # the piece's record bytes lie inside its records
                        assert lo <= max(at, first_byte) and lo + len(merged) >= min(at + step, len(stream)), (name, ends, step)
                    at += step
                assert at >= len(stream)


def _host(c, order="queryname"):
    headers = [x["header"] for x in c["inputs"]]
    hdr, maps = _lib.bam_merge_header_host(headers, order)
    n_ref = len(bammerge.parse_header(hdr)[1])
    body, perm = _lib.bam_merge_host([(b"".join(x["records"]), x["n_ref"], m) for x, m in zip(c["inputs"], maps)], n_ref, order)
    return hdr, maps, body, perm


def test_host_build_equals_the_definition(cases):
    for name, c in _accepted(cases):
        stream, perm = NM.definition(c)
        hdr, maps, body, hperm = _host(c)
        assert hdr == bammerge.merged_header([x["header"] for x in c["inputs"]], "queryname"), name
        assert maps == _translated(c)[1], name
        assert hdr + body == stream and (hperm == np.asarray(perm, dtype=np.uint32)).all(), name


def test_refusals_with_their_codes_and_precedence(cases):
    seen = []
    for name, c in cases.items():
        if not name.startswith("refused:"):
            continue
        with pytest.raises(bammerge.BamMergeError) as e:
            NM.definition(c)
        assert e.value.code == c["error"], name
        with pytest.raises(bammerge.BamMergeError) as e:
            _host(c)
        assert e.value.code == c["error"], name
        seen.append(c["error"])
    assert sorted(seen) == [bamsort.E_RANGE, bamsort.E_ARG, bamsort.E_ARG]
    # the second name refusal, and both of them in coordinate order: no refusal there
    good = [NC.name_record(b"g%02d" % k) for k in range(8)]
    hdr = cases["refused:pos_below_minus_one_alone"]["inputs"][0]["header"]
    n_ref = cases["refused:pos_below_minus_one_alone"]["inputs"][0]["n_ref"]
    for rname, recs, code in NC.refused():
        raws = [hdr + b"".join(good), hdr + b"".join(recs)]
        files = [(b"".join(good), n_ref, list(range(n_ref))), (b"".join(recs), n_ref, list(range(n_ref)))]
        for call in (lambda: bammerge.stream_of(raws, "queryname"), lambda: _lib.bam_merge_host(files, n_ref, "queryname")):
            with pytest.raises(bammerge.BamMergeError) as e:
                call()
            assert e.value.code == code, rname
        if "pos_below" not in rname:
            assert bammerge.stream_of(raws)[0][len(bammerge.merged_header([hdr, hdr])):] == _lib.bam_merge_host(files, n_ref)[0], rname
    # E_ARG in a LATER file goes before E_RANGE in an earlier one, also for a bad mate id of a translated file
    c = cases["dict:reversed_dictionary"]
    low = MC.with_ids(NC.name_record(b"low", 1, -2))
    bad_mate = MC.with_ids(c["inputs"][1]["records"][3], mate=99)
    raws = [c["inputs"][0]["header"] + b"".join(c["inputs"][0]["records"] + [low]), c["inputs"][1]["header"] + b"".join(c["inputs"][1]["records"] + [bad_mate])]
    with pytest.raises(bammerge.BamMergeError) as e:
        bammerge.stream_of(raws, "queryname")
    assert e.value.code == bamsort.E_ARG
    with pytest.raises(bammerge.BamMergeError) as e:
        bammerge.stream_of([raws[0], MC.raws(c)[1]], "queryname")
    assert e.value.code == bamsort.E_RANGE


def test_name_table_word_is_the_names_word():
    """bsort_name_tab_word == bsort_name_word (csrc/bamsort_core.hpp) through svx_bam_name_tab_check_host: every length 1..255, every round 0..63 (the helper
    runs them all), at offsets that put the name at the table's first and at its last word; nothing outside the name's words is written"""
    rng = random.Random(402)
    for n in range(1, 256):
        name = bytes(rng.randrange(1, 256) for _ in range(n))
        words = (n + 3) // 4
        tab = 64 + rng.randrange(4)
        for off in (0, tab - words, rng.randrange(tab - words + 1)):
            assert _lib.bam_name_tab_check_host(name, off, tab) == 0, (n, off, tab)
    assert _lib.bam_name_tab_check_host(b"\xff\x80\x7f\x01\xfe", 0, 2) == 0 and _lib.bam_name_tab_check_host(b"a", 0, 1) == 0
    for bad in ((b"abcde", 0, 1), (b"abcde", 1, 2), (b"", 0, 4), (b"a" * 256, 0, 80), (b"a", -1, 4)):
        with pytest.raises(_lib.SvxError):
            _lib.bam_name_tab_check_host(*bad)


def test_host_build_under_the_sanitizers(tmp_path):
    """tools/bam_name_merge_host_test.cpp with bamsort_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer: 2 000 seeded multi-file streams against a
    plain reimplementation in that program - the same status, permutation and bytes every time - and the name table's pack / word functions over every length
    and round, no report"""
    out = str(tmp_path / "bam_name_merge_host_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "bam_name_merge_host_test.cpp"), os.path.join(CSRC, "bamsort_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "2000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "2000 streams" in run.stdout and " 0 malformed" in run.stdout and " 0 wrong" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    n_merged, n_arg, n_range, n_bad, n_cut, n_both, n_words = (int(run.stdout.split(w)[0].split()[-1]) for w in
                                                                (" merged", " bad argument", " bad range", " with a bad name", " cut short", " with both kinds", " table words"))
    assert n_merged > 1000 and n_arg > 200 and n_range > 50 and n_bad > 50 and n_cut > 50 and n_both > 50 and n_words == 255 * 4 * 64
    assert n_merged + n_arg + n_range == 2000


def test_symbols_declared_and_exported():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_bam_merge_header_host_order", "svx_bam_merge_host_order", "svx_bam_merge_open_order", "svx_bam_merge_get_name_stats", "svx_bam_merge_get_name_spill_stats",
                 "svx_bam_name_tab_check_host"):
        assert hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
    assert "typedef struct svx_bam_name_spill_stats" in hdr and L.svx_version() >= 109
    fields = re.search(r"typedef struct svx_bam_name_spill_stats \{(.*?)\} svx_bam_name_spill_stats;", hdr, re.S).group(1)
    declared = re.findall(r"\b([a-z_]+)(?=\s*(?:/\*.*?\*/)?\s*[,;])", re.sub(r"/\*.*?\*/", "", fields))
    assert declared == [n for n, _ in _abi.BamNameSpillStats._fields_]
    core = open(os.path.join(CSRC, "bamsort_core.hpp")).read()
    for fn in ("bsort_name_tab_words", "bsort_name_tab_pack", "bsort_name_tab_word"):
        assert re.search(r"BSORT_FN \w+ %s\(" % fn, core), fn
    # the old refusals stand: the door to query-name order beyond device memory is the session
    import ctypes as C
    h = C.c_void_p()
    assert L.svx_bam_merge_open_order(None, C.c_int64(0), C.c_int(0), C.c_int64(0), None, C.c_int(1), C.byref(h)) == _abi.SVX_E_ARG
