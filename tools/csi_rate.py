#!/usr/bin/env python3
"""The CSI build beside the .bai build of the same file, in the same process (svx_bam_index_finish_fmt with SVX_INDEX_CSI / SVX_INDEX_CLASSIC):

    python tools/csi_rate.py [--reps 5] [--rows 5000000] [--out profiles/csi_rates.jsonl] [--box NAME]

Two inputs: the large file of the index tests (tests/bai_cases.large_file: 150 500 records) and a synthetic table of --rows records laid out the same way.
Per input one handle, one warm-up pass of each format, then --reps indexing passes of each format interleaved (bai, csi, bai, csi ...); only finish() is
timed - the passes in front of it append the same rows whatever the format.  Reported per input: the library's own time of finish (t_total_ms) per format as
the median of the warm runs, the run-to-run spread (max - min) of the .bai figure, the phases of the median runs, the sizes of the two indexes, and whether
both equal the host builds' bytes (the rows come from svim_amd.bai.rows_of_bam, in Python: only for inputs up to --check-rows records).  One JSON line
per input, stating box and commit, is appended to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bai_cases as BC                                     # noqa: E402
from svim_amd import _lib, bai                             # noqa: E402
from svim_amd.bamio import NativeBam                       # noqa: E402


def finish_after_a_pass(nb, fmt, first=False):
    if not first:
        nb.rewind()
    nb.index_begin()
    tot = 0
    while True:
        _, m = nb.read_batch(200000, 0, "coordinate")
        if m == 0:
            break
        tot += m
    t = time.perf_counter()
    data = nb.index_finish(fmt)
    return tot, time.perf_counter() - t, data, nb.index_stats()


def measure(path, n_records, reps, check):
    nb = NativeBam(path, threads=8)
    nb.set_device_decode(0)
    finish_after_a_pass(nb, "bai", first=True)             # warm-up: code objects, buffers, the page cache
    finish_after_a_pass(nb, "csi")
    runs = {"bai": [], "csi": []}
    data = {}
    for _ in range(reps):
        for fmt in ("bai", "csi"):
            tot, wall, data[fmt], st = finish_after_a_pass(nb, fmt)
            assert tot == n_records
            runs[fmt].append((st["t_total_ms"], wall * 1e3, st))
    nb.close()
    out = {"records": n_records, "reps": reps, "index_bytes": {k: len(v) for k, v in data.items()}}
    for fmt in ("bai", "csi"):
        ts = [r[0] for r in runs[fmt]]
        med = sorted(runs[fmt], key=lambda r: r[0])[len(ts) // 2]
        out[fmt] = {"finish_ms": ts, "finish_ms_median": statistics.median(ts), "finish_ms_spread": max(ts) - min(ts), "finish_wall_ms_median": statistics.median(r[1] for r in runs[fmt]),
                    "phases_of_the_median_run": {k: v for k, v in med[2].items() if k.startswith("t_") or k in ("n_chunks", "n_bins", "n_slots")}}
    out["csi_over_bai"] = out["csi"]["finish_ms_median"] / out["bai"]["finish_ms_median"]
    out["csi_minus_bai_ms"] = out["csi"]["finish_ms_median"] - out["bai"]["finish_ms_median"]
    if check:
        n_ref, rows, v_end = bai.rows_of_bam(path)
        out["csi_equals_host_build"] = bool(_lib.bam_index_host(n_ref, rows, v_end, fmt="csi") == data["csi"])
        out["bai_equals_host_build"] = bool(_lib.bam_index_host(n_ref, rows, v_end) == data["bai"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--check-rows", type=int, default=200_000)
    ap.add_argument("--box", default="MI355X")
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git's HEAD, when the tree is a checkout)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csi_rates.jsonl"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="svx_csi_rate_") as d:
        for name, n in (("large_file", 150000), ("synthetic_%d" % a.rows, a.rows)):
            path = os.path.join(d, name + ".bam")
            m = BC.large_file(path, n=n)
            line = {"tool": "csi_rate", "box": a.box, "commit": commit, "input": name}
            line.update(measure(path, m, a.reps, m <= a.check_rows))
            os.remove(path)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
