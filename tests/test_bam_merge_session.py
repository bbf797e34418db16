"""The merge session (svx_bam_merge_*: svim_amd/csrc/bamio.cpp) on the CPU: its ABI, and its life cycle walked by tools/bam_merge_session_test.cpp - the
session's host logic and the reader of bamio.cpp over a CPU model of the decoder and of the sort that poisons what it frees and counts owners - under
AddressSanitizer + UndefinedBehaviorSanitizer (LeakSanitizer on) and, in a second build, under ThreadSanitizer.  Both are stand-alone programs with their own
main; nothing is loaded into python under a sanitizer."""
import os
import re
import subprocess

import pytest

from svim_amd import _abi, _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(REPO, "svim_amd", "csrc", "bamio.cpp"), os.path.join(REPO, "svim_amd", "csrc", "bamsort_host.cpp"), os.path.join(REPO, "tools", "bam_merge_session_test.cpp")]
SESSION = ("svx_bam_merge_open", "svx_bam_merge_add", "svx_bam_merge_finish", "svx_bam_merge_count", "svx_bam_merge_encode", "svx_bam_merge_fetch", "svx_bam_merge_index_fmt",
           "svx_bam_merge_index_count", "svx_bam_merge_index_fetch", "svx_bam_merge_permutation", "svx_bam_merge_get_stats", "svx_bam_merge_get_spill_stats",
           "svx_bam_merge_get_merge_stats", "svx_bam_merge_close")


def test_abi_has_the_merge_session():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in SESSION:
        assert hasattr(L, name) and name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.svx_version() >= 107
    # svx_bam_merge_stats as the header declares it: eight counts, three times
    body = re.search(r"typedef struct svx_bam_merge_stats \{(.*?)\} svx_bam_merge_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for kind in ("int64_t", "double") for decl in re.findall(kind + r"\s+([^;]*);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _abi.BamMergeStats._fields_]


def test_merge_session_refuses_without_a_device_or_readers(tmp_path):
    """the checks that need no GPU: no readers, a null reader; a header clash leaves at open before any device work (SVX_E_ARG, not SVX_E_NODEVICE)"""
    import ctypes as C
    import bam_merge_cases as MC
    from svim_amd import bammerge
    from svim_amd.bamio import BamMerge, NativeBam
    L = _lib.lib()
    h = C.c_void_p()
    assert L.svx_bam_merge_open(None, C.c_int64(0), C.c_int(0), C.c_int64(0), None, C.byref(h)) == _abi.SVX_E_ARG
    arr = (C.c_void_p * 1)(None)
    assert L.svx_bam_merge_open(arr, C.c_int64(1), C.c_int(0), C.c_int64(0), None, C.byref(h)) == _abi.SVX_E_ARG
    L.svx_bam_merge_close(None)
    cases = MC.build_headers(str(tmp_path))
    for name in ("conflicting_rg", "same_name_two_lengths", "name_twice_in_one_dictionary"):
        readers = [NativeBam(x["path"], threads=1) for x in cases[name]["inputs"]]
        try:
            with pytest.raises(bammerge.BamMergeError) as e:
                BamMerge.open(readers, device=0)
            assert e.value.code == _abi.SVX_E_ARG, name
        finally:
            for r in readers:
                r.close()


def _sanitizer_build(tmp_path, tag, flags):
    out = str(tmp_path / ("bam_merge_session_test_" + tag))
    probe = str(tmp_path / ("probe_%s.cpp" % tag))
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *flags, probe, "-o", str(tmp_path / ("probe_" + tag))], capture_output=True).returncode != 0:
        pytest.skip("no %s runtime in this toolchain" % tag)
    return out, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", *flags, "-fno-omit-frame-pointer", *SOURCES, "-lz", "-lpthread", "-o", out], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True)


def test_merge_session_life_cycle_under_the_sanitizers(tmp_path):
    """every order of open, add, a reader closed before, between and after the adds, a reader that fed and then sorts on its own (finish, abort in the middle,
    abort after finish), finish / encode / index, the session closed first and last, over 1 to 3 files and chunks of one block and of whole files, with an
    append that fails at every chunk index: merged bytes and permutation equal a plain merge, the ownership rules of the model hold, and neither build's
    sanitizer has anything to report.  The AddressSanitizer build walks all of it (more than 5000 scenarios, about a minute); the ThreadSanitizer build, several
    times slower per scenario, runs beside it with `light`: every plan of one and two files, one in nine of the plans of three."""
    builds = [_sanitizer_build(tmp_path, "asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), _sanitizer_build(tmp_path, "tsan", ["-fsanitize=thread"])]
    for out, p in builds:
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-2000:]
    runs = []
    for k, (out, _) in enumerate(builds):
        d = tmp_path / ("files_%d" % k)
        d.mkdir()
        runs.append(subprocess.Popen([out, str(d)] + (["light"] if k else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for k, p in enumerate(runs):
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0 and " 0 wrong" in so and "Sanitizer" not in se and "OWNERSHIP" not in se, (so[-500:], se[-3000:])
        n_scen, n_adds, n_fail, n_sorts = (int(x) for x in re.match(r"(\d+) scenarios, (\d+) adds, (\d+) injected failures, (\d+) reader sorts", so.splitlines()[-1]).groups())
        assert n_fail >= 30 and ((n_scen > 1000 and n_adds > 2000 and n_sorts > 1000) if k else (n_scen > 5000 and n_adds > 14000 and n_sorts > 5000)), so[-300:]
