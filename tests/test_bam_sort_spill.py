"""The spilled coordinate sort by its definition (svim_amd/bamsort.py: runs_of, merge_runs, piece_cuts) and by the host build (svx_bam_sort_spill_host, the cut
rule of csrc/bamsort_core.hpp that the kernels share): whatever the runs, merging them gives the stream and the permutation of the in-memory sort; every piece
reads one contiguous range per run and the ranges are exactly the piece's records; the host build equals svx_bam_sort_host byte for byte; a short write or
read of the run file is SVX_E_IO; the host build under the sanitizers.  tests/test_gpu_bam_sort_spill.py holds the device build to the same bytes.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_sort_cases as SC
import bam_sort_spill_cases as PC
from svim_amd import _abi, _lib, bamsort

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "svim_amd", "csrc")


@pytest.fixture(scope="module")
def corner(tmp_path_factory):
    """every corner file with the definition's stream and permutation, computed once"""
    d = str(tmp_path_factory.mktemp("bam_sort_spill_cases"))
    out = SC.build_all(d)
    for x in out.values():
        x["stream"], x["perm"] = SC.definition(x)
        x["body"] = x["stream"][len(bamsort.sorted_header(x["header"])):]
    return out


def test_merged_runs_equal_the_definition_at_every_cut(corner):
    for name, x in corner.items():
        recs = x["records"]
        for ends in PC.cut_sets(len(recs), 301):
            runs = bamsort.runs_of(recs, x["n_ref"], ends)
            assert [len(r) for r in runs] == [b - a for a, b in zip([0] + ends, ends)], (name, ends)
            body, perm = bamsort.merge_runs(runs)
            assert perm == x["perm"], (name, ends)
            assert body == x["body"], (name, ends)
    # the stream form: split and checked as sort_records does
    x = corner["unplaced_scattered"]
    assert bamsort.merge_runs(bamsort.runs_of(b"".join(x["records"]), x["n_ref"], [17, 60, len(x["records"])])) == (x["body"], x["perm"])
    with pytest.raises(ValueError):
        bamsort.runs_of(x["records"], x["n_ref"], [5, 3, len(x["records"])])
    with pytest.raises(ValueError):
        bamsort.runs_of(x["records"], x["n_ref"], [5])


@pytest.mark.parametrize("piece_blocks", [1, 3, 4096])
def test_piece_cuts_are_contiguous_and_hold_exactly_the_pieces_records(corner, piece_blocks):
    for name, x in corner.items():
        recs, hdr_len = x["records"], len(bamsort.sorted_header(x["header"]))
        n = len(recs)
        starts = np.cumsum([hdr_len] + [len(recs[k]) for k in x["perm"]])
        for ends in PC.few_cut_sets(n, 302):
            runs = bamsort.runs_of(recs, x["n_ref"], ends)
            pieces = bamsort.piece_cuts(runs, x["perm"], hdr_len, piece_blocks * bamsort.BLOCK)
            assert len(pieces) == -(-len(x["stream"]) // (piece_blocks * bamsort.BLOCK)), (name, ends)
            for p, (p0, p1, cuts) in enumerate(pieces):
                lo, hi = p * piece_blocks * bamsort.BLOCK, min((p + 1) * piece_blocks * bamsort.BLOCK, len(x["stream"]))
                want = [j for j in range(n) if starts[j] < hi and starts[j + 1] > lo]          # the records with a byte in the piece
                assert list(range(p0, p1)) == want, (name, ends, p)
                assert len(cuts) == len(runs) and all(0 <= a <= b <= len(run) for (a, b), run in zip(cuts, runs)), (name, ends, p)
                # the ranges, merged again, are the piece's records in order: nothing missing, nothing foreign
                got = bamsort.merge_runs([run[a:b] for (a, b), run in zip(cuts, runs)])[1]
                assert got == [x["perm"][j] for j in want], (name, ends, p)


def test_spill_host_build_equals_the_in_memory_host_build(corner):
    for name, x in corner.items():
        stream = b"".join(x["records"])
        want_body, want_perm = _lib.bam_sort_host(stream, x["n_ref"])
        assert want_body == x["body"]
        sets = PC.cut_sets(len(x["records"]), 303) if len(x["records"]) <= 310 else PC.few_cut_sets(len(x["records"]), 303)
        for ends in sets:
            for piece_blocks in (1, 3, 4096):
                body, perm = _lib.bam_sort_spill_host(stream, x["n_ref"], ends, piece_blocks)
                assert perm.tolist() == want_perm.tolist(), (name, ends, piece_blocks)
                assert body == want_body, (name, ends, piece_blocks)


def _stream_100000(seed=83):
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
    return a.tobytes(), n, n_ref


def test_spill_host_build_on_100000_records_in_1_8_and_300_runs():
    stream, n, n_ref = _stream_100000()
    want_body, want_perm = _lib.bam_sort_host(stream, n_ref)
    rng = np.random.default_rng(84)
    for n_runs in (1, 8, 300):
        ends = sorted(rng.integers(0, n + 1, n_runs - 1).tolist()) + [n]
        body, perm = _lib.bam_sort_spill_host(stream, n_ref, ends, 7)
        assert (perm == want_perm).all() and body == want_body, n_runs


def test_spill_host_build_refusals_and_short_io(corner):
    x = corner["blocks_cut_records_anywhere"]
    stream, n = b"".join(x["records"]), len(x["records"])
    for ends in ([], [n - 1], [n + 1], [5, 3, n], [-1, n]):
        with pytest.raises(bamsort.BamSortError) as e:
            _lib.bam_sort_spill_host(stream, x["n_ref"], ends)
        assert e.value.code == bamsort.E_ARG, ends
    with pytest.raises(bamsort.BamSortError) as e:
        _lib.bam_sort_spill_host(stream, x["n_ref"], [n], piece_blocks=0)
    assert e.value.code == bamsort.E_ARG
    with pytest.raises(bamsort.BamSortError) as e:
        _lib.bam_sort_spill_host(stream[:-1], x["n_ref"], [n])
    assert e.value.code == bamsort.E_ARG
    assert _lib.bam_sort_spill_host(b"", 0, [])[0] == b"" and _lib.bam_sort_spill_host(b"", 3, [0, 0])[0] == b""
    # the caller's run file: whole transfers give the sorted stream, and the file holds every record once; a short write or read is SVX_E_IO
    ends = [40, 41, 200, n]
    store = bytearray()

    def write(offset, data, short=0):
        assert offset == len(store)
        store.extend(data[:len(data) - short])
        return len(data) - short

    def read(offset, n_bytes, short=0):
        assert 0 <= offset and offset + n_bytes <= len(store)
        return bytes(store[offset:offset + n_bytes - short])
    body, perm = _lib.bam_sort_spill_host(stream, x["n_ref"], ends, 1, write, read)
    assert body == x["body"] and perm.tolist() == x["perm"] and len(store) == len(stream)
    runs = bamsort.runs_of(x["records"], x["n_ref"], ends)
    assert bytes(store) == b"".join(r[2] for run in runs for r in run)                     # the run file: every run's sorted stream, back to back
    calls = [0]

    def counted(fn, fail_at):
        def g(offset, arg):
            calls[0] += 1
            return fn(offset, arg, short=1 if calls[0] == fail_at else 0)
        return g
    for fail_write, fail_read in ((2, 0), (0, 1), (0, 3)):
        del store[:]
        calls[0] = 0
        w = counted(write, fail_write)
        calls_before_reads = len(ends)
        r = counted(read, calls_before_reads + fail_read if fail_read else 0)
        with pytest.raises(_lib.SvxError) as e:
            _lib.bam_sort_spill_host(stream, x["n_ref"], ends, 1, w, r)
        assert e.value.code == _abi.SVX_E_IO, (fail_write, fail_read)
    assert _abi.ERRORS[_abi.SVX_E_IO] == "SVX_E_IO" and _abi.SVX_E_IO == -11


def test_spill_host_build_under_the_sanitizers(tmp_path):
    """tools/bam_sort_spill_host_test.cpp with bamsort_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, a stand-alone program: a seeded fuzz of
    streams, run ends, piece sizes and run-file callbacks that come back short; every call equals svx_bam_sort_host or ends in the refusal it must, no report"""
    out = str(tmp_path / "bam_sort_spill_host_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", "-I", CSRC,
                            os.path.join(REPO, "tools", "bam_sort_spill_host_test.cpp"), os.path.join(CSRC, "bamsort_host.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "3000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "3000 streams" in run.stdout and " 0 malformed" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    n_equal, n_refused, n_io, n_bad_runs = (int(run.stdout.split(w)[0].split()[-1]) for w in (" equal", " refused", " short io", " bad runs"))
    assert n_equal > 1200 and n_refused > 500 and n_io > 50 and n_bad_runs > 30, run.stdout[-300:]


def test_spill_symbols_declared_and_exported():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "svx.h")).read()
    for name in ("svx_bam_sort_begin_spill", "svx_bam_sort_get_spill_stats", "svx_bam_sort_spill_host"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert re.search(r"#define\s+SVX_E_IO\s+\(-11\)", hdr)
    assert C.sizeof(_abi.BamSortSpillStats) == 8 * 9 and C.sizeof(_abi.BamSortStats) == 8 * 25
