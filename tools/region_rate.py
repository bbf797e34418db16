#!/usr/bin/env python3
"""What a region read costs beside the index's own chunks and beside the whole file (svx_bam_seek_region with the device reader):

    python tools/region_rate.py [--reps 5] [--rows 2000000] [--out profiles/region_rates.jsonl] [--box NAME]

One seeded file (tests/bai_cases.large_file with --rows records: three references of 2^27 bases, one record in ten skips up to 100 000 bases) and its .bai
built on the device.  For regions of several widths on its first reference, under the overlap rule: the bytes the reader inflated (svx_bam_region_stats)
against the inflated bytes of the blocks the index's chunks touch (bai.query: what a reader that hops between chunks would inflate) and against the whole
file's; the wall time of the region pass (seek_region to end-of-file, median of --reps warm passes) against a whole-file pass of the same handle.  The reader
reads contiguously from the plan's offset to the stop, so the first ratio says what not hopping costs.  One JSON line per run is appended to --out."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bai_cases as BC                                     # noqa: E402
from svim_amd import bai, harness, regions as RG            # noqa: E402
from svim_amd.bamio import NativeBam                       # noqa: E402


def block_table(path):
    """[(file offset, inflated bytes)] of every BGZF block, from the headers and trailers alone"""
    out = []
    with open(path, "rb") as fh:
        data = fh.read()
    at = 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((at, struct.unpack_from("<I", data, at + size - 4)[0]))
        at += size
    return out, len(data)


def read_to_end(nb):
    n = 0
    while True:
        _, m = nb.read_batch(200000, 0, "coordinate")
        if m == 0:
            return n
        n += m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--box", default="MI355X")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "region_rates.jsonl"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="svx_region_rate_") as d:
        path = os.path.join(d, "regions.bam")
        n_records = BC.large_file(path, n=a.rows)
        index = bai.parse_index(harness.index_bam(path, device=0))
        blocks, file_bytes = block_table(path)
        starts = [b[0] for b in blocks]
        whole_inflated = sum(b[1] for b in blocks)
        nb = NativeBam(path, threads=8)
        nb.set_device_decode(0)
        read_to_end(nb)                                     # warm-up: code objects, buffers, the page cache
        whole = []
        for _ in range(a.reps):
            nb.rewind()
            t = time.perf_counter()
            assert read_to_end(nb) == n_records
            whole.append((time.perf_counter() - t) * 1e3)
        line = {"tool": "region_rate", "box": a.box, "commit": commit, "records": n_records, "file_bytes": file_bytes, "file_inflated_bytes": whole_inflated,
                "reps": a.reps, "whole_file_pass_ms": whole, "whole_file_pass_ms_median": statistics.median(whole), "regions": []}
        import bisect
        for width in (10_000, 100_000, 1_000_000, 10_000_000, 1 << 26):
            g = (0, 1 << 25, (1 << 25) + width)
            (voff, tid, beg, end), = RG.plan(index, [g])
            chunks, _low = bai.query(index, tid, beg, end)
            touched = set()
            for vb, ve in chunks:
                lo = bisect.bisect_right(starts, vb >> 16) - 1
                hi = bisect.bisect_right(starts, ve >> 16) - 1 - (0 if ve & 0xffff else 1)
                touched.update(range(lo, hi + 1))
            chunk_inflated = sum(blocks[k][1] for k in touched)
            ms, st, n_run = [], None, 0
            for rep in range(a.reps + 1):
                t = time.perf_counter()
                nb.seek_region(voff, tid, beg, end)
                n_run = read_to_end(nb)
                if rep:                                    # (the first pass of a width is its warm-up)
                    ms.append((time.perf_counter() - t) * 1e3)
                st = nb.region_stats()
            line["regions"].append({"width": width, "records_kept": st["n_kept"], "records_marked": st["n_marked"], "records_seen": st["n_seen"], "run": n_run,
                                    "index_chunks": len(chunks), "bytes_inflated": st["bytes_inflated"], "chunk_bytes_inflated": chunk_inflated,
                                    "inflated_over_chunks": st["bytes_inflated"] / max(1, chunk_inflated), "inflated_over_file": st["bytes_inflated"] / whole_inflated,
                                    "pass_ms": ms, "pass_ms_median": statistics.median(ms), "pass_over_whole_file_pass": statistics.median(ms) / statistics.median(whole)})
        nb.close()
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
