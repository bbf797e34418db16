#!/usr/bin/env python3
"""COMBINE on the device against the Python route of today, on a seeded whole-genome-like cluster set.

    python tools/combine_rate.py [--scale 1.0] [--python-scale 0.1] [--out profiles/combine_rates.jsonl]

The cluster set has the contig names of workloads.py's configs[3] stand-in (hg38 header order, so tid order != name order) and, at scale 1, 60 000
deletion, 40 000 insertion, 4 000 insertion-from, 3 000 tandem-duplication and 6 000 breakend clusters.  Timed: (a) Engine.combine on the table (device
events inside the library + wall clock around the call, after a warm-up call), (b) combine_clusters on lists (table build + device + lazy result),
(c) tests/combine_consumer.consume on materialised lists at --python-scale (the interpreter route every caller of the drop-in takes today).  One JSON line
per run is appended to --out; the stage-3 kernel's pair rate comes from svx_combine_stats.
"""
import argparse
import json
import os
import random
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def cluster_case(seed, scale):
    from svim_amd import workloads
    rng = random.Random(seed)
    names = [c[0] for c in workloads.profile("c3")["contigs"]]
    span = 5000000
    case = {"signatures_fully_covered": [], "clusters": [[] for _ in range(6)]}

    def mem(n, fc=False):
        k = len(case["signatures_fully_covered"])
        case["signatures_fully_covered"].extend([fc] * n)
        return list(range(k, k + n))

    def std():
        return rng.choice([None, rng.random() * 20])
    n_del, n_ins, n_dup, n_tan, n_pairs = (int(x * scale) for x in (60000, 40000, 4000, 3000, 2000))
    for _ in range(n_del):
        s = rng.randrange(0, span)
        case["clusters"][0].append([rng.choice(names), s, s + rng.randrange(40, 4000), rng.choice([0.0, 3.0, 12.5]), std(), std(), mem(rng.randrange(1, 6))])
    ins = []
    for _ in range(n_ins):
        s = rng.randrange(0, span)
        ins.append([rng.choice(names), s, s + rng.randrange(40, 900), rng.choice([0.0, 2.0, 9.5]), std(), std(), mem(rng.randrange(1, 6))])
    ins.sort(key=lambda r: (r[0], (r[1] + r[2]) // 2))
    case["clusters"][1] = ins
    for _ in range(n_tan):
        c, s, ln = rng.choice(names), rng.randrange(0, span), rng.randrange(50, 800)
        case["clusters"][3].append([c, s, s + ln, c, s + ln, s + ln + rng.randrange(1, 6) * ln // 2, 8.0, std(), std(), mem(2, rng.random() < 0.5)])
    for k in range(n_dup):
        c = rng.choice(names[:3])
        s = rng.randrange(0, 60000) if k % 4 == 0 else rng.randrange(0, span)
        ln, d = rng.randrange(100, 1200), rng.randrange(0, span)
        case["clusters"][4].append([c, s, s + ln, rng.choice(names), d, d + ln, float(rng.randrange(1, 40)), std(), std(), mem(rng.randrange(1, 4))])
    for k in range(n_pairs):
        r = ins[rng.randrange(len(ins))]
        ln, dc, d, j = r[2] - r[1], rng.choice(names), rng.randrange(0, span), rng.randrange(-30, 30)
        case["clusters"][5].append([r[0], r[1] + j, r[1] + j + 1, dc, d, d + 1, 5.0, std(), std(), mem(2), "fwd", "fwd"])
        case["clusters"][5].append([r[0], r[1] - j, r[1] - j + 1, dc, d + ln + rng.randrange(-3, 3), d + ln + 1, 5.0, std(), std(), mem(2), "rev", "rev"])
        case["clusters"][5].append([rng.choice(names), rng.randrange(0, span), 7, rng.choice(names), rng.randrange(0, span), 9, 4.0, std(), std(), mem(1),
                                    rng.choice(["fwd", "rev"]), rng.choice(["fwd", "rev"])])
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--python-scale", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "combine_rates.jsonl"))
    a = ap.parse_args()
    import combine_cases as CC
    import combine_consumer as cc
    import svim_amd
    from svim_amd import SVIM_COMBINE, _abi, _lib, batch
    o = types.SimpleNamespace(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
                              cluster_max_distance=0.5, skip_consensus=True)
    eng = _lib.engine()
    cp = _abi.CombineParams.from_options(o)
    line = {"tool": "combine_rate", "scale": a.scale, "python_scale": a.python_scale}
    case = cluster_case(11, a.scale)
    lists6, idx = CC.case_objects(case)
    ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)
    rank = batch.contig_ranks(names)
    eng.combine(cp, rank, table=ct, sig_aux=aux)                         # warm-up: code objects, buffers
    t0 = time.perf_counter()
    table = eng.combine(cp, rank, table=ct, sig_aux=aux, fetch=False)
    t1 = time.perf_counter()
    table = eng.fetch_candidates()
    t2 = time.perf_counter()
    st = eng.combine_stats()
    line.update({"clusters": int(ct.n), "cluster_members": int(ct.n_members), "candidates": int(table.n), "combine_tables_wall_s": t1 - t0, "fetch_wall_s": t2 - t1,
                 "t_combine_ms": st["t_combine_ms"], "t_cutpaste_ms": st["t_cutpaste_ms"], "cutpaste_pairs": st["n_cutpaste_pairs"],
                 "cutpaste_pairs_per_s": st["n_cutpaste_pairs"] / (st["t_cutpaste_ms"] * 1e-3) if st["t_cutpaste_ms"] > 0 else None,
                 "stats": st})
    t0 = time.perf_counter()
    out = svim_amd.combine_clusters(lists6, o)
    line["combine_clusters_lists_wall_s"] = time.perf_counter() - t0
    line["candidates_by_class"] = [len(x) for x in out]
    small = cluster_case(11, a.python_scale)
    l2, idx2 = CC.case_objects(small)
    t0 = time.perf_counter()
    want = cc.consume([list(x) for x in l2], o, idx2)
    line["python_route_wall_s"] = time.perf_counter() - t0
    line["python_route_clusters"] = sum(len(x) for x in small["clusters"])
    ct2, names2, sigs2, aux2 = SVIM_COMBINE.cluster_table_from_lists(l2)
    eng.combine(cp, batch.contig_ranks(names2), table=ct2, sig_aux=aux2)
    t0 = time.perf_counter()
    t_small = eng.combine(cp, batch.contig_ranks(names2), table=ct2, sig_aux=aux2)
    line["device_same_size_wall_s"] = time.perf_counter() - t0
    line["device_same_size_t_combine_ms"] = eng.combine_stats()["t_combine_ms"]
    line["same_size_candidates_equal"] = [len(x) for x in want["combine"]] == list(t_small.class_count)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
