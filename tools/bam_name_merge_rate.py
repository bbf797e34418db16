#!/usr/bin/env python3
"""A merge session in query-name order (svx_bam_merge_open_order; csrc/bamsort.hip: runs in name order, k_ns_pack, k_ns_keys_tab) beside a coordinate session
over the same files:

    python tools/bam_name_merge_rate.py [--records 1000000] [--files 3] [--runs 8] [--passes 3] [--check] [--out profiles/bam_name_merge_rates.jsonl]

One shuffled set of --records short records per name shape of tools/bam_name_sort_rate.py ("uuid", "zmw", "long"), dealt round-robin into --files files.  One
process; per shape a warm-up of each route, then --passes times the three routes interleaved:
    coordinate   a coordinate session: the yardstick, and the code path of the commit before query-name sessions
    queryname    a query-name session in memory
    spilled      a query-name session whose arena holds an eighth (--runs) of the record bytes, with a spill directory, its readers loading a sixteenth of
                 that at a time (the other routes read in the default chunks): the runs are sorted by name as they close, their names packed into the
                 table, and finish merges them by the rank pass and the rounds over the table
Reported per shape and route, medians: the passes (open + every add; for the spilled route the runs close in here), finish alone, and their sum; for the
query-name routes the rounds and the phases of finish; for the spilled route the phases of svx_bam_name_spill_stats (the runs' own name sorts, the packing),
the table's bytes, and the spill's own times.  --check: every route's permutation against the host build (svx_bam_merge_host_order).  One JSON line is
appended to --out.  Recorded figures of single sessions, no thresholds."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                                        # noqa: E402
from bam_name_sort_rate import EOF_BLOCK, LENS, REFS, names_of      # noqa: E402
from svim_amd import _lib, harness                        # noqa: E402
from svim_amd.bamio import BamMerge, NativeBam            # noqa: E402

ROUTES = ("coordinate", "queryname", "spilled")


def write_files(paths, shape, n, seed):
    """n records as tools/bam_name_sort_rate.py writes them, in random order, dealt round-robin over the files -> (record bytes per file, their sum)"""
    rng = np.random.default_rng(seed)
    names = names_of(shape, n, rng)
    tid, pos = rng.integers(0, len(REFS), n).tolist(), rng.integers(0, 90_000_000, n).tolist()
    flag = rng.choice(np.array([0, 16, 2048, 2064, 256], dtype=np.uint16), n, p=[0.4, 0.4, 0.08, 0.08, 0.04]).tolist()
    text = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % z for z in zip(REFS, LENS))).encode()
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REFS))
    for r, l in zip(REFS, LENS):
        hdr += struct.pack("<i", len(r) + 1) + r.encode() + b"\0" + struct.pack("<i", l)
    bodies = []
    for f, path in enumerate(paths):
        recs = []
        for k in range(f, n, len(paths)):
            nb = names[k] + b"\0"
            recs.append(struct.pack("<iiiBBHHHiiii", 32 + len(nb), tid[k], pos[k], len(nb), 60, 4680, 0, flag[k], 0, -1, -1, 0) + nb)
        body = b"".join(recs)
        raw = hdr + body
        with open(path, "wb") as fh:
            for lo in range(0, len(raw), 0xff00):
                fh.write(harness._bgzf_block(raw[lo:lo + 0xff00], 1))
            fh.write(EOF_BLOCK)
        bodies.append(body)
    return bodies, sum(map(len, bodies))


def session(paths, route, max_bytes, spill_dir, want=None, chunk_blocks=None):
    """open, every add, finish -> (seconds of the passes, seconds of finish, stats, name stats, the permutation equals `want` or None).  chunk_blocks: the
    BGZF blocks the readers of this session load at a time (SVX_BAM_DEV_CHUNK_BLOCKS, read when a handle switches device decode on; None: the default)"""
    readers = [NativeBam(p) for p in paths]
    if chunk_blocks:
        os.environ["SVX_BAM_DEV_CHUNK_BLOCKS"] = str(chunk_blocks)
    try:
        for r in readers:
            r.set_device_decode(0)
    finally:
        os.environ.pop("SVX_BAM_DEV_CHUNK_BLOCKS", None)
    t0 = time.perf_counter()
    kw = dict(order="queryname", max_bytes=max_bytes, spill_dir=spill_dir) if route == "spilled" else dict(order=route)
    m = BamMerge.open(readers, device=0, **kw)
    try:
        for r in readers:
            m.add(r)
            r.close()
        t1 = time.perf_counter()
        m.finish()
        t2 = time.perf_counter()
        same = None if want is None else bool((m.permutation() == want).all())
        return t1 - t0, t2 - t1, m.stats(), m.name_stats(), same
    finally:
        m.close()
        for r in readers:
            r.close()


def measure(shape, a, workdir):
    paths = [os.path.join(workdir, "name_merge_rate.%s.%d.bam" % (shape, f)) for f in range(a.files)]
    bodies, total = write_files(paths, shape, a.records, a.seed)
    want = {}
    if a.check:
        files = [(b, len(REFS), list(range(len(REFS)))) for b in bodies]
        want = {"coordinate": _lib.bam_merge_host(files, len(REFS))[1], "queryname": _lib.bam_merge_host(files, len(REFS), "queryname")[1]}
        want["spilled"] = want["queryname"]
    del bodies
    # the spilled route reads in chunks of a sixteenth of what its arena is to hold, so that the arena - an a.runs-th of the record bytes - decides where a run ends
    chunk_blocks = max(1, total // a.runs // 16 // 0xff00)
    session(paths, "coordinate", 0, None)                     # (the warm-up of the coordinate route)
    max_chunk = session(paths, "coordinate", 0, None, chunk_blocks=chunk_blocks)[2]["spill"]["max_chunk_bytes"]
    max_bytes = max(max_chunk, total // a.runs)
    session(paths, "queryname", 0, None)
    session(paths, "spilled", max_bytes, workdir, chunk_blocks=chunk_blocks)
    t = {route: [] for route in ROUTES}
    last = {}
    for _ in range(a.passes):
        for route in ROUTES:
            t_pass, t_finish, st, ns, same = session(paths, route, max_bytes, workdir, want.get(route), chunk_blocks if route == "spilled" else None)
            t[route].append((t_pass, t_finish))
            last[route] = (st, ns, same)
    out = {"shape": shape, "records": a.records, "files": a.files, "record_bytes": total, "name_bytes": total // a.records - 37, "chunk_blocks_spilled": chunk_blocks, "max_chunk_bytes_spilled": max_chunk,
           "max_bytes_spilled": max_bytes}
    med = {}
    for route in ROUTES:
        st, ns, same = last[route]
        p, f = statistics.median(x[0] for x in t[route]), statistics.median(x[1] for x in t[route])
        med[route] = (p, f)
        o = {"passes_s": [x[0] for x in t[route]], "finish_s": [x[1] for x in t[route]], "passes_s_median": p, "finish_s_median": f, "records_per_s": a.records / (p + f),
             "finish_ms": {k: st[k] for k in ("t_finish_ms", "t_sort_ms", "t_layout_ms")}, "n_runs": st["spill"]["n_runs"]}
        if route != "coordinate":
            o["rounds"], o["active_total"] = ns["rounds"], ns["active_total"]
            o["finish_phases_ms"] = {"names": ns["t_names_ms"], "rank_pass": ns["t_rank_ms"], "rounds": ns["t_rounds_ms"], "layout": ns["t_layout_ms"]}
        if route == "spilled":
            o["name_spill"] = ns["spill"]
            o["spill"] = {k: st["spill"][k] for k in ("spilled_bytes", "max_run_bytes", "t_spill_ms", "t_merge_ms")}
        if same is not None:
            o["permutation_equals_host_build"] = same
        out[route] = o
    for route in ROUTES[1:]:
        out[route + "_over_coordinate_finish"] = med[route][1] / med["coordinate"][1]
        out[route + "_over_coordinate"] = sum(med[route]) / sum(med["coordinate"])
    for p in paths:
        os.remove(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--files", type=int, default=3)
    ap.add_argument("--runs", type=int, default=8, help="the spilled route's arena holds one part in this many of the record bytes")
    ap.add_argument("--passes", type=int, default=3, help="timed sessions of each route and shape, after one warm-up of each")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--shapes", default="uuid,zmw,long")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bam_name_merge_rates.jsonl"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="svx_name_merge_rate_") as workdir:
        line = {"tool": "bam_name_merge_rate", "records": a.records, "files": a.files, "runs_asked": a.runs, "passes": a.passes, "word_bytes": 4,
                "shapes": [measure(s, a, workdir) for s in a.shapes.split(",")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
