#!/usr/bin/env python3
"""The tabix index on the device (svx_text_index) on the texts of the seeded combine_rate workload: the three switch sets of tools/vcf_rate.py in position
order and the three products of tools/bed_rate.py (whose files keep the reference's order: most of them are refused, which costs the same phases).

    python tools/text_index_rate.py [--scale 1.0] [--reps 5] [--python-limit 67108864] [--out profiles/text_index_rates.jsonl]

Per text, after a warm-up call: the HIP-event time of svx_text_index per phase, beside the time of svx_text_gz on the same text, beside the host build of
the same header (svx_text_index_host, one thread) and - for texts up to --python-limit bytes - the definition (svim_amd.tabix.build_index) on the fetched text.
Every file's device index is checked against the host build.  One JSON line per run is appended to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

PIECE = 64 << 20


def measure(eng, label, source, preset, fetch_text, n_files, reps, python_limit):
    from svim_amd import _lib, tabix
    eng.text_gz(source)
    gz = eng.text_gz_stats()
    eng.text_index(preset)                                              # warm-up: code objects, buffers
    walls, stats = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.text_index(preset)
        walls.append(time.perf_counter() - t0)
        stats.append(eng.text_index_stats())
    blobs, status = eng.text_index_fetch()
    text = fetch_text()
    fo, co, uo = (x.tolist() for x in eng.text_gz_tables())
    off = [int(x) for x in eng.bed_file_offsets()[0]] if source == 1 else [0, len(text)]
    t_host = t_py = 0.0
    equal, py_equal = True, None
    for k in range(n_files):
        part = text[off[k]:off[k + 1]]
        b0, b1 = co.index(fo[k]), co.index(fo[k + 1])
        coff, uoff = [c - co[b0] for c in co[b0:b1 + 1]], [u - off[k] for u in uo[b0:b1]] + [len(part)]
        t0 = time.perf_counter()
        try:
            want, code = _lib.text_index_host(part, coff, uoff, preset, 0), 0
        except tabix.TabixError as e:
            want, code = b"", e.code
        t_host += time.perf_counter() - t0
        equal = bool(equal and want == blobs[k] and code == int(status[k]))
        if len(text) <= python_limit:
            t0 = time.perf_counter()
            try:
                py = tabix.build_index(part, coff, uoff, preset, 0)
            except tabix.TabixError:
                py = b""
            t_py += time.perf_counter() - t0
            py_equal = bool((py_equal is None or py_equal) and py == blobs[k])
    med = {k: statistics.median(s[k] for s in stats) for k in stats[0] if k.startswith("t_")}
    return {"text": label, "files": n_files, "status": [int(s) for s in status], "bytes_text": len(text), "bytes_index": sum(len(b) for b in blobs), "stats": stats[-1],
            "median_ms": med, "median_call_wall_s": statistics.median(walls), "all_call_wall_s": walls, "text_gz_total_ms": gz["t_total_ms"],
            "index_over_text_gz": med["t_total_ms"] / gz["t_total_ms"] if gz["t_total_ms"] > 0 else None,
            "text_bytes_per_s_device": len(text) / (med["t_total_ms"] * 1e-3) if med["t_total_ms"] > 0 else None,
            "host_build_s": t_host, "python_definition_s": t_py if len(text) <= python_limit else None, "equals_host_build": equal, "equals_definition": py_equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-limit", type=int, default=64 << 20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "text_index_rates.jsonl"))
    a = ap.parse_args()
    import bed_rate
    import combine_cases as CC
    import combine_rate
    import vcf_rate
    from svim_amd import SVIM_COMBINE, _abi, _lib, batch
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
    read_names = ["m64011_190830_220126/%d/%d_%d" % (4000 + 3 * (k // 2), 100 * k, 100 * k + 9000) for k in range(n_reads)]
    seq_off = np.zeros(n_sig + 1, dtype=np.int64)
    np.cumsum(rng.integers(40, 301, n_sig), out=seq_off[1:])
    letters = np.array([1, 2, 4, 8], dtype=np.uint8)
    seq = letters[rng.integers(0, 4, int(seq_off[-1]))]
    off = np.arange(len(names) + 1, dtype=np.int64) * vcf_rate.SPAN
    eng.set_genome(off, letters[rng.integers(0, 4, int(off[-1]))])
    line = {"tool": "text_index_rate", "scale": a.scale, "reps": a.reps, "clusters": int(ct.n), "candidates": int(table.n), "runs": []}
    base = dict(symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
                interspersed_duplications_as_insertions=False)
    seq_sw = dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True)
    for label, sw in (("vcf_symbolic", dict()), ("vcf_sequence", seq_sw), ("vcf_sequence_seqs_reads", dict(seq_sw, insertion_sequences=True, read_names=True, zmws=True))):
        vp = _abi.VcfParams.from_options(types.SimpleNamespace(**dict(base, **sw)))
        vcf = lambda po: eng.vcf(vp, names, table=table, sig_read_id=read_id, sig_seq_off=seq_off, sig_seq=seq, read_names=read_names, position_order=po)      # noqa: E731
        vcf(False)
        t_plain = eng.vcf_stats()["t_entries_ms"]
        _, n_bytes = vcf(True)
        t_ordered = eng.vcf_stats()["t_entries_ms"]
        fetch = lambda n=n_bytes: b"".join(eng.vcf_fetch(at, min(PIECE, n - at)) for at in range(0, n, PIECE))      # noqa: E731
        run = measure(eng, label, _abi.TEXT_GZ_VCF, _abi.INDEX_VCF, fetch, 1, a.reps, a.python_limit)
        run["vcf_entries_ms_reference_order"], run["vcf_entries_ms_position_order"] = t_plain, t_ordered
        line["runs"].append(run)
    sig = bed_rate.seeded_signatures(n_sig, len(names), n_reads, 5)
    for label, product, tab, preset in (("signature_beds", _abi.BED_SIGNATURE_BEDS, ct, _abi.INDEX_BED), ("signature_vcf", _abi.BED_SIGNATURE_VCF, ct, _abi.INDEX_VCF),
                                        ("candidate_beds", _abi.BED_CANDIDATE_BEDS, table, _abi.INDEX_BED)):
        n_files, _, n_bytes = eng.bed(product, names, table=tab, sigs=sig, read_names=read_names)
        fetch = lambda n=n_bytes: b"".join(eng.bed_fetch(at, min(PIECE, n - at)) for at in range(0, n, PIECE))      # noqa: E731
        line["runs"].append(measure(eng, label, _abi.TEXT_GZ_BED, preset, fetch, n_files, a.reps, a.python_limit))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
