#!/usr/bin/env python3
"""The BED / signature-VCF text on the device (svx_bed) against the Python definition of a line, on the clusters and candidates of the seeded combine_rate workload.

    python tools/bed_rate.py [--scale 1.0] [--no-python] [--out profiles/bed_rates.jsonl]

The cluster table is tools/combine_rate.py's cluster set (scale 1: 113 000 clusters), the candidate table what Engine.combine makes of it.  The signatures
their members index get seeded columns of all six types (a breakend's second end lies behind its first on the same contig, so the constructor keeps the order),
seeded read ids and PacBio-style names.  Three products: the seven signature BED files, the body of all.vcf, the eight candidate BED files.  Timed per product,
after a warm-up call: the svx_bed call with the read names already resident and with their upload (wall clock, and the library's HIP-event times per phase),
the device -> host fetch of the text in 64 MiB pieces (apart), and - unless --no-python - the *_python definition over the materialised objects of the same
tables in the same run (the object build - signatures, clusters, candidates - is timed apart).  One JSON line per run is appended to --out.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)


def seeded_signatures(n_sig, n_contig, n_reads, seed):
    from svim_amd import _abi
    rng = np.random.default_rng(seed)
    t = _abi.SigTable(n_sig)
    t.key[:] = np.arange(n_sig, dtype=np.uint64)
    t.type[:] = rng.integers(0, 6, n_sig)
    t.src[:] = rng.integers(0, 2, n_sig)
    t.contig[:] = rng.integers(0, n_contig, n_sig)
    t.start[:] = rng.integers(0, 5_000_000, n_sig)
    t.end[:] = t.start + rng.integers(40, 4000, n_sig)
    typ = t.type[:n_sig]
    bnd, dint, tan, inv = typ == _abi.SVX_BND, typ == _abi.SVX_DUP_INT, typ == _abi.SVX_DUP_TAN, typ == _abi.SVX_INV
    t.end[bnd] = t.start[bnd] + 1
    t.contig2[:] = np.where(bnd, t.contig[:n_sig], np.where(dint, rng.integers(0, n_contig, n_sig), -1))
    t.pos2[:] = np.where(bnd, t.start[:n_sig] + rng.integers(1, 100_000, n_sig), np.where(dint, rng.integers(0, 5_000_000, n_sig), np.where(tan, rng.integers(1, 9, n_sig), 0)))
    t.aux[:] = np.where(bnd, rng.integers(0, 4, n_sig), np.where(inv, rng.integers(0, 5, n_sig), np.where(tan, rng.integers(0, 2, n_sig), 0)))
    t.read_id[:] = rng.integers(0, n_reads, n_sig)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bed_rates.jsonl"))
    a = ap.parse_args()
    import combine_cases as CC
    import combine_rate
    from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, _abi, _lib, batch, convert
    o = types.SimpleNamespace(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
                              cluster_max_distance=0.5, skip_consensus=True)
    eng = _lib.engine()
    case = combine_rate.cluster_case(11, a.scale)
    lists6, _ = CC.case_objects(case)
    ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)
    table = eng.combine(_abi.CombineParams.from_options(o), batch.contig_ranks(names), table=ct, sig_aux=aux)
    n_sig, n_reads = len(sigs), max(1, len(sigs) // 3)
    sig = seeded_signatures(n_sig, len(names), n_reads, 5)
    read_names = ["m64011_190830_220126/%d/%d_%d" % (4000 + 3 * (k // 2), 100 * k, 100 * k + 9000) for k in range(n_reads)]
    line = {"tool": "bed_rate", "scale": a.scale, "clusters": int(ct.n), "cluster_members": int(ct.n_members), "candidates": int(table.n),
            "candidate_members": int(table.n_members), "signatures": n_sig, "reads": n_reads, "read_name_bytes": sum(len(r) for r in read_names), "runs": []}
    cl_objs = ca_objs = None
    if not a.no_python:
        t0 = time.perf_counter()
        sig_objs = convert.objects_from_sigtable(sig, names, read_names)
        t1 = time.perf_counter()
        cl_objs = tuple(list(x) for x in convert.cluster_objects(ct, sig_objs, names))
        for lst in cl_objs:
            for c in lst:
                c.members                                            # (members resolve on first read: part of the materialisation)
        t2 = time.perf_counter()
        d, i, di, t, n, b = convert.candidate_lists(table, sig_objs, names)
        ca_objs = tuple(list(x) for x in (di, i, t, d, n, b))
        for lst in ca_objs:
            for c in lst:
                c.members
        t3 = time.perf_counter()
        line["objects_wall_s"] = {"signatures": t1 - t0, "clusters": t2 - t1, "candidates": t3 - t2}
    products = (("signature_beds", _abi.BED_SIGNATURE_BEDS, ct, lambda: SVIM_CLUSTER.signature_bed_texts_python(cl_objs)),
                ("signature_vcf", _abi.BED_SIGNATURE_VCF, ct, lambda: [SVIM_CLUSTER.signature_vcf_body_python(cl_objs)]),
                ("candidate_beds", _abi.BED_CANDIDATE_BEDS, table, lambda: SVIM_COMBINE.candidate_bed_texts_python(ca_objs)))
    for label, product, tab, python in products:
        call = lambda rn: eng.bed(product, names, table=tab, sigs=sig, read_names=rn)      # noqa: E731
        call(read_names)                                               # warm-up: code objects, buffers, names
        t0 = time.perf_counter()
        n_files, n_lines, n_bytes = call(read_names)
        t1 = time.perf_counter()
        st = eng.bed_stats()
        pieces = [eng.bed_fetch(at, min(64 << 20, n_bytes - at)) for at in range(0, n_bytes, 64 << 20)]
        t2 = time.perf_counter()
        fresh = list(read_names)
        call(fresh)                                                    # the same call with the upload of the names
        t3 = time.perf_counter()
        read_names = fresh
        kernels_ms = st["t_total_ms"] - st["t_upload_ms"]
        run = {"product": label, "files": n_files, "lines": n_lines, "bytes": n_bytes, "call_wall_s": t1 - t0, "call_with_name_upload_wall_s": t3 - t2,
               "fetch_wall_s": t2 - t1, "stats": st, "device_ms_without_upload": kernels_ms,
               "bytes_per_s_device": n_bytes / (kernels_ms * 1e-3) if kernels_ms > 0 else None, "bytes_per_s_call": n_bytes / (t1 - t0),
               "payload_bytes_per_s": st["bytes_members"] / (st["t_payload_ms"] * 1e-3) if st["t_payload_ms"] > 0 else None,
               "fetch_bytes_per_s": n_bytes / (t2 - t1) if t2 > t1 else None}
        if cl_objs is not None:
            t0 = time.perf_counter()
            texts = python()
            text = "".join(texts).encode("utf-8")
            run["python_wall_s"] = time.perf_counter() - t0
            run["python_equal"] = text == b"".join(pieces)
        line["runs"].append(run)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
