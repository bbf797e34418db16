#!/usr/bin/env python3
"""The query-name sort on the device (svx_bam_sort_begin_order, csrc/bamsort.hip: the k_ns_* kernels) beside the coordinate sort of the same file:

    python tools/bam_name_sort_rate.py [--records 1000000] [--passes 3] [--check] [--out profiles/bam_name_sort_rates.jsonl]

One shuffled file of --records short records per name shape - "uuid": 36-byte UUIDs (names differ in their first word: one round and a short tail),
"zmw": movie/zmw/ccs names behind a 24-byte shared prefix (six rounds without a split, the whole file active), "long": 254-byte names that differ in their
last bytes (every round over every row: the worst case) - each read by one handle: a warm-up pass of each order, then --passes times a coordinate sort and
a query-name sort interleaved (the clock of a pass starts before rewind(); sort_finish() is timed on its own).  Reported per shape, medians: records per
second of pass + finish in both orders and their ratio, finish alone in both orders and its ratio, the phases of the query-name finish (names, rank pass,
rounds, layout), the rounds and the rows active in each.  --check: the permutation against the host build (svx_bam_sort_host_order).  One JSON line is
appended to --out.  Recorded figures, no thresholds."""
import argparse
import json
import os
import statistics
import struct
import sys
import time
import uuid

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                        # noqa: E402
from svim_amd import _lib, harness                        # noqa: E402
from svim_amd.bamio import NativeBam                      # noqa: E402

REFS, LENS = ["chr1", "chr2", "chr3"], [200_000_000, 150_000_000, 100_000_000]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def names_of(shape, n, rng):
    if shape == "uuid":
        return [str(uuid.UUID(int=int.from_bytes(rng.bytes(16), "little"))).encode() for _ in range(n)]
    if shape == "zmw":
        return [b"m64011_190830_220126/zmw%d/ccs" % z for z in rng.integers(1, 180_000_000, n).tolist()]      # (reads of one movie: some names twice)
    stem = b"@long_read_name_of_a_pipeline_that_concatenates_its_whole_provenance/" * 4
    return [stem[:244] + b"%010d" % z for z in rng.integers(0, 10 ** 10, n).tolist()]


def write_file(path, shape, n, seed):
    """n records without CIGAR, bases and tags under names of that shape, flags of a query-name file (primary, supplementary, secondary), in random order"""
    rng = np.random.default_rng(seed)
    names = names_of(shape, n, rng)
    tid, pos = rng.integers(0, len(REFS), n).tolist(), rng.integers(0, 90_000_000, n).tolist()
    flag = rng.choice(np.array([0, 16, 2048, 2064, 256], dtype=np.uint16), n, p=[0.4, 0.4, 0.08, 0.08, 0.04]).tolist()
    text = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % z for z in zip(REFS, LENS))).encode()
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(REFS))
    for r, l in zip(REFS, LENS):
        hdr += struct.pack("<i", len(r) + 1) + r.encode() + b"\0" + struct.pack("<i", l)
    recs = []
    for k in range(n):
        nb = names[k] + b"\0"
        recs.append(struct.pack("<iiiBBHHHiiii", 32 + len(nb), tid[k], pos[k], len(nb), 60, 4680, 0, flag[k], 0, -1, -1, 0) + nb)
    body = b"".join(recs)
    raw = hdr + body
    with open(path, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(harness._bgzf_block(raw[lo:lo + 0xff00], 1))
        fh.write(EOF_BLOCK)
    return body, len(raw), len(set(names))


def one_sort(nb, order):
    t = time.perf_counter()
    nb.rewind()
    nb.sort_begin(order=order)
    tot = 0
    while True:
        m = nb.read_batch(200_000, 0, "coordinate")[1]
        if m == 0:
            break
        tot += m
    t_pass = time.perf_counter() - t
    t = time.perf_counter()
    nb.sort_finish()
    t_finish = time.perf_counter() - t
    return tot, t_pass, t_finish


def measure(path, shape, a):
    body, raw, distinct = write_file(path, shape, a.records, a.seed)
    nb = NativeBam(path)
    nb.set_device_decode(0)
    while nb.read_batch(200_000, 0, "coordinate")[1]:      # warm-up: code objects, buffers, the page cache
        pass
    for order in ("coordinate", "queryname"):
        one_sort(nb, order)
    t = {"coordinate": [], "queryname": []}
    for _ in range(a.passes):
        for order in ("coordinate", "queryname"):
            tot, t_pass, t_finish = one_sort(nb, order)
            assert tot == a.records
            t[order].append((t_pass, t_finish))
            if order == "coordinate":
                st_c = nb.sort_stats()
    st, ns = nb.sort_stats(), nb.sort_name_stats()          # (the last sort was a query-name sort)
    out = {"shape": shape, "records": a.records, "distinct_names": distinct, "inflated_bytes": raw, "name_bytes": len(body) // a.records - 37}
    med = {o: (statistics.median(x[0] for x in t[o]), statistics.median(x[1] for x in t[o])) for o in t}
    for o, (p, f) in med.items():
        out[o] = {"pass_s": [x[0] for x in t[o]], "finish_s": [x[1] for x in t[o]], "pass_s_median": p, "finish_s_median": f, "records_per_s": a.records / (p + f),
                  "finish_records_per_s": a.records / f}
    out["queryname_over_coordinate"] = (med["queryname"][0] + med["queryname"][1]) / (med["coordinate"][0] + med["coordinate"][1])
    out["queryname_over_coordinate_finish"] = med["queryname"][1] / med["coordinate"][1]
    out["coordinate_finish_sort_ms"], out["coordinate_key_bits"] = st_c["t_sort_ms"], st_c["key_bits"]
    out["finish_phases_ms"] = {"names": ns["t_names_ms"], "rank_pass": ns["t_rank_ms"], "rounds": ns["t_rounds_ms"], "layout": ns["t_layout_ms"], "sort_total": st["t_sort_ms"]}
    out["rounds"], out["active_rows"], out["active_total"] = ns["rounds"], ns["active_rows"], ns["active_total"]
    if a.check:
        want = _lib.bam_sort_host(body, len(REFS), "queryname")[1]
        out["permutation_equals_host_build"] = bool((nb.sort_permutation() == want).all())
    nb.sort_abort()
    nb.close()
    os.remove(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3, help="timed sorts of each order and shape, after one warm-up of each")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--shapes", default="uuid,zmw,long")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--path", default="/tmp/bam_name_sort_rate.bam")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bam_name_sort_rates.jsonl"))
    a = ap.parse_args()
    line = {"tool": "bam_name_sort_rate", "records": a.records, "passes": a.passes, "word_bytes": 4, "shapes": [measure(a.path, s, a) for s in a.shapes.split(",")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
