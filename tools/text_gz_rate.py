#!/usr/bin/env python3
"""BGZF output on the device (svx_text_gz) on the texts of the seeded combine_rate workload: the three switch sets of tools/vcf_rate.py and the three
products of tools/bed_rate.py.

    python tools/text_gz_rate.py [--scale 1.0] [--reps 5] [--out profiles/text_gz_rates.jsonl]

Per text, after a warm-up call: the svx_text_gz call (wall clock and the library's HIP-event times per phase), GB/s of text consumed, the compressed bytes
and their quotient against zlib level 1 of the same text in the same 65 280-byte blocks (framed as BGZF).  Then, alternated in the same process, the median
of --reps runs each of
    (a) compress + fetch of the compressed stream,
    (b) the fetch of the plain text (the only way to get the text off the device before this stage existed),
    (c) zlib level 1 of the fetched text on the host's cores (one block per task, 16 threads: what a user does today, bgzip -@16 -l 1),
and the stream is checked against the host build of the encoder (svx_text_gz_host) and against gzip.  One JSON line per run is appended to --out.
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time
import types
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

BLOCK = 65280
PIECE = 64 << 20


def _zlib1_block(b):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return len(c.compress(b) + c.flush()) + 26


def host_zlib1(text, pool):
    """-> (seconds, BGZF bytes) of zlib level 1 over the blocks of text on the pool's threads (zlib releases the interpreter lock)"""
    t0 = time.perf_counter()
    view = memoryview(text)
    size = sum(pool.map(_zlib1_block, (view[at:at + BLOCK] for at in range(0, len(text), BLOCK)))) + 28
    return time.perf_counter() - t0, size


def measure(eng, label, source, fetch_text, n_files, reps, pool):
    from svim_amd import _lib
    eng.text_gz(source)                                                 # warm-up: code objects, buffers
    t0 = time.perf_counter()
    _, n_blocks, n_out = eng.text_gz(source)
    t1 = time.perf_counter()
    st = eng.text_gz_stats()
    kernels_ms = st["t_total_ms"] - st["t_upload_ms"]
    fetch_gz = lambda: b"".join(eng.text_gz_fetch(at, min(PIECE, n_out - at)) for at in range(0, n_out, PIECE))      # noqa: E731
    t_gz, t_plain, t_host = [], [], []
    text = stream = None
    z_size = 0
    for _ in range(reps):
        a = time.perf_counter()
        eng.text_gz(source)
        stream = fetch_gz()
        b = time.perf_counter()
        text = fetch_text()
        c = time.perf_counter()
        dt, z_size = host_zlib1(text, pool)
        t_gz.append(b - a), t_plain.append(c - b), t_host.append(dt)
    fo = eng.text_gz_tables()[0]
    if n_files > 1:
        off = [int(x) for x in eng.bed_file_offsets()[0]]
    else:
        off = [0, len(text)]
    equal = all(stream[int(fo[k]):int(fo[k + 1])] == _lib.text_gz_host(text[off[k]:off[k + 1]]) for k in range(n_files))
    inflates = all(gzip.decompress(stream[int(fo[k]):int(fo[k + 1])]) == text[off[k]:off[k + 1]] for k in range(n_files))
    z_total = sum(host_zlib1(text[off[k]:off[k + 1]], pool)[1] for k in range(n_files)) if n_files > 1 else z_size
    return {"text": label, "files": n_files, "blocks": n_blocks, "bytes_in": len(text), "bytes_out": n_out, "out_over_in": n_out / max(1, len(text)),
            "zlib1_bgzf_bytes": z_total, "ours_over_zlib1": n_out / max(1, z_total), "call_wall_s": t1 - t0, "stats": st, "device_ms_without_upload": kernels_ms,
            "text_bytes_per_s_device": len(text) / (kernels_ms * 1e-3) if kernels_ms > 0 else None,
            "median_compress_and_fetch_s": statistics.median(t_gz), "median_fetch_plain_s": statistics.median(t_plain), "median_host_zlib1_16_threads_s": statistics.median(t_host),
            "all_compress_and_fetch_s": t_gz, "all_fetch_plain_s": t_plain, "all_host_zlib1_s": t_host, "equals_host_build": equal, "inflates_to_text": inflates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "text_gz_rates.jsonl"))
    a = ap.parse_args()
    import bed_rate
    import combine_cases as CC
    import combine_rate
    import vcf_rate
    from svim_amd import SVIM_COMBINE, _abi, _lib, batch
    o = types.SimpleNamespace(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
                              cluster_max_distance=0.5, skip_consensus=True)
    eng = _lib.engine()
    pool = ThreadPoolExecutor(16)
    case = combine_rate.cluster_case(11, a.scale)
    lists6, _ = CC.case_objects(case)
    ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)
    table = eng.combine(_abi.CombineParams.from_options(o), batch.contig_ranks(names), table=ct, sig_aux=aux)
    rng = np.random.default_rng(5)
    n_sig, n_reads = len(sigs), max(1, len(sigs) // 3)
    read_id = rng.integers(0, n_reads, n_sig).astype(np.int32)
    read_names = ["m64011_190830_220126/%d/%d_%d" % (4000 + 3 * (k // 2), 100 * k, 100 * k + 9000) for k in range(n_reads)]
    seq_len = rng.integers(40, 301, n_sig)
    seq_off = np.zeros(n_sig + 1, dtype=np.int64)
    np.cumsum(seq_len, out=seq_off[1:])
    letters = np.array([1, 2, 4, 8], dtype=np.uint8)
    seq = letters[rng.integers(0, 4, int(seq_off[-1]))]
    off = np.arange(len(names) + 1, dtype=np.int64) * vcf_rate.SPAN
    eng.set_genome(off, letters[rng.integers(0, 4, int(off[-1]))])
    line = {"tool": "text_gz_rate", "scale": a.scale, "reps": a.reps, "clusters": int(ct.n), "candidates": int(table.n), "runs": []}
    base = dict(symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
                interspersed_duplications_as_insertions=False)
    seq_sw = dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True)
    for label, sw in (("vcf_symbolic", dict()), ("vcf_sequence", seq_sw), ("vcf_sequence_seqs_reads", dict(seq_sw, insertion_sequences=True, read_names=True, zmws=True))):
        vp = _abi.VcfParams.from_options(types.SimpleNamespace(**dict(base, **sw)))
        _, n_bytes = eng.vcf(vp, names, table=table, sig_read_id=read_id, sig_seq_off=seq_off, sig_seq=seq, read_names=read_names)
        fetch = lambda n=n_bytes: b"".join(eng.vcf_fetch(at, min(PIECE, n - at)) for at in range(0, n, PIECE))      # noqa: E731
        line["runs"].append(measure(eng, label, _abi.TEXT_GZ_VCF, fetch, 1, a.reps, pool))
    sig = bed_rate.seeded_signatures(n_sig, len(names), n_reads, 5)
    for label, product, tab in (("signature_beds", _abi.BED_SIGNATURE_BEDS, ct), ("signature_vcf", _abi.BED_SIGNATURE_VCF, ct), ("candidate_beds", _abi.BED_CANDIDATE_BEDS, table)):
        n_files, _, n_bytes = eng.bed(product, names, table=tab, sigs=sig, read_names=read_names)
        fetch = lambda n=n_bytes: b"".join(eng.bed_fetch(at, min(PIECE, n - at)) for at in range(0, n, PIECE))      # noqa: E731
        line["runs"].append(measure(eng, label, _abi.TEXT_GZ_BED, fetch, n_files, a.reps, pool))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
