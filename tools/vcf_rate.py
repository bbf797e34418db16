#!/usr/bin/env python3
"""The VCF text on the device (svx_vcf) against the Python definition of a line, on the candidates of the seeded combine_rate workload.

    python tools/vcf_rate.py [--scale 1.0] [--no-python] [--out profiles/vcf_rates.jsonl]

The candidate table is what Engine.combine makes of tools/combine_rate.py's cluster set (scale 1: 113 000 clusters -> 78 774 candidates).  Its member
signatures get seeded read ids, PacBio-style names and inserted sequences of 40 .. 300 bases; the genome is seeded random bases over the contigs the clusters
use.  Three switch sets: symbolic alleles; sequence alleles; sequence alleles + SEQS + READS (+ ZMWS).  Timed per set, after a warm-up call: the svx_vcf call
(wall clock and the library's HIP-event times per phase), the device -> host fetch of the text in 64 MiB pieces (apart), and - unless --no-python -
SVIM_COMBINE.vcf_body_python over the materialised objects of the same candidates (the object build is timed apart).  One JSON line per run is appended
to --out.
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

SPAN = 5_004_200      # combine_rate places clusters below 5 000 000 and lets them reach ~4 000 further


class Sig(object):
    __slots__ = ("read", "sequence")

    def __init__(self, read, sequence):
        self.read, self.sequence = read, sequence


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vcf_rates.jsonl"))
    a = ap.parse_args()
    import combine_cases as CC
    import combine_rate
    from svim_amd import SVIM_COMBINE, _abi, _lib, batch, convert
    o = types.SimpleNamespace(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
                              cluster_max_distance=0.5, skip_consensus=True)
    eng = _lib.engine()
    case = combine_rate.cluster_case(11, a.scale)
    lists6, _ = CC.case_objects(case)
    ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)
    table = eng.combine(_abi.CombineParams.from_options(o), batch.contig_ranks(names), table=ct, sig_aux=aux)
    rng = np.random.default_rng(5)
    n_sig, n_reads = len(sigs), max(1, len(sigs) // 3)
    read_id = rng.integers(0, n_reads, n_sig).astype(np.int32)
    read_names = ["m64011_190830_220126/%d/%d_%d" % (4000 + 3 * (k // 2), 100 * k, 100 * k + 9000) for k in range(n_reads)]      # two reads per ZMW
    seq_len = rng.integers(40, 301, n_sig)
    seq_off = np.zeros(n_sig + 1, dtype=np.int64)
    np.cumsum(seq_len, out=seq_off[1:])
    letters = np.array([1, 2, 4, 8], dtype=np.uint8)
    seq = letters[rng.integers(0, 4, int(seq_off[-1]))]
    off = np.arange(len(names) + 1, dtype=np.int64) * SPAN
    codes = letters[rng.integers(0, 4, int(off[-1]))]
    eng.set_genome(off, codes)
    line = {"tool": "vcf_rate", "scale": a.scale, "clusters": int(ct.n), "candidates": int(table.n), "candidate_members": int(table.n_members),
            "genome_bases": int(off[-1]), "runs": []}
    base = dict(symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
                interspersed_duplications_as_insertions=False)
    sets = (("symbolic", dict()), ("sequence", dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True)),
            ("sequence_seqs_reads", dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True,
                                         insertion_sequences=True, read_names=True, zmws=True)))
    objs = None
    if not a.no_python:
        t0 = time.perf_counter()
        sig_objs = [Sig(read_names[int(r)], _abi.decode_bases(seq[seq_off[k]:seq_off[k + 1]])) for k, r in enumerate(read_id)]
        d, i, di, t, n, b = convert.candidate_lists(table, sig_objs, names)
        objs = tuple(list(x) for x in (di, i, t, d, n, b))
        line["objects_wall_s"] = time.perf_counter() - t0
        genome_text = SVIM_COMBINE.GenomeText({nm: _abi.decode_bases(codes[off[k]:off[k + 1]]) for k, nm in enumerate(names)})
    for label, sw in sets:
        ov = types.SimpleNamespace(**dict(base, **sw))
        vp = _abi.VcfParams.from_options(ov)
        call = lambda: eng.vcf(vp, names, table=table, sig_read_id=read_id, sig_seq_off=seq_off, sig_seq=seq, read_names=read_names)      # noqa: E731
        call()                                                     # warm-up: code objects, buffers
        t0 = time.perf_counter()
        n_lines, n_bytes = call()
        t1 = time.perf_counter()
        st = eng.vcf_stats()
        pieces = [eng.vcf_fetch(at, min(64 << 20, n_bytes - at)) for at in range(0, n_bytes, 64 << 20)]
        t2 = time.perf_counter()
        kernels_ms = st["t_total_ms"] - st["t_upload_ms"]
        run = {"switches": label, "lines": n_lines, "bytes": n_bytes, "call_wall_s": t1 - t0, "fetch_wall_s": t2 - t1, "stats": st,
               "device_ms_without_upload": kernels_ms, "lines_per_s_device": n_lines / (kernels_ms * 1e-3) if kernels_ms > 0 else None,
               "bytes_per_s_device": n_bytes / (kernels_ms * 1e-3) if kernels_ms > 0 else None, "lines_per_s_call": n_lines / (t1 - t0),
               "bytes_per_s_call": n_bytes / (t1 - t0), "fetch_bytes_per_s": n_bytes / (t2 - t1) if t2 > t1 else None}
        if objs is not None:
            t0 = time.perf_counter()
            lines = SVIM_COMBINE.vcf_body_python(*objs, list(_abi.VCF_LABELS), ov, not ov.symbolic_alleles, genome_text)
            text = "".join(l + "\n" for l in lines).encode("utf-8")
            run["python_wall_s"] = time.perf_counter() - t0
            run["python_lines_per_s"] = len(lines) / run["python_wall_s"]
            run["python_equal"] = text == b"".join(pieces)
        line["runs"].append(run)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
