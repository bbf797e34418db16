#!/usr/bin/env python3
"""The coordinate sort on the device (svx_bam_sort_*), on the file tools/device_reader_rate.py reads with its records shuffled:

    python tools/bam_sort_rate.py [--records 20000] [--passes 5] [--chunk-mb 2048] [--piece-blocks 4096] [--qual] [--check] [--out profiles/bam_sort_rates.jsonl]

One handle, one warm-up pass of each kind, then plain reading passes and sorting passes (append on) interleaved (plain, sort, plain, sort ...): the clock of a
pass starts BEFORE rewind(), a sorting pass ends before sort_finish(), which is timed on its own.  After the last sorting pass the file is encoded piece by
piece.  Reported: the reader's rate with the sort off and on (median of the warm passes of each kind), the phases of finish, the gather's bytes per second
against twice its bytes over the rate of a plain device-to-device copy of the same size measured here, the encoder's phases and rate, the share of stored
blocks, and the compressed size against zlib level 1 over the same 65 280-byte blocks (on the first --zlib-blocks blocks).  --qual: the file carries seeded
base qualities (the encoder's hard case) instead of none.  --check: the stream and the file against the definition (svim_amd.bamsort, in Python: slow on a
large file).  One JSON line is appended to --out.

    python tools/bam_sort_rate.py --spill-dir DIR [--spill-split 64] [--records ...] [--qual]

The spilled sort (svx_bam_sort_begin_spill) instead: the same file, read in at least --spill-split chunks, sorted whole - pass, finish, every piece encoded,
index - three ways: in memory, with max_bytes = arena / 4 and with max_bytes = arena / 16 (never below the largest chunk), runs written to a spill file in DIR.
One warm-up of each, then the three interleaved --passes times; the median of each.  The line holds the three rates, t_spill_ms, t_readback_ms, t_merge_ms,
the spill file's write and read bytes per second (bytes over the time spent in the phase that moves them: gather and copy out included in the write, copy in
included in the read), max_stage_bytes, and whether the three files are the same bytes.  Disk speed belongs to the box: recorded figures, no thresholds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from svim_amd import _lib, bamsort, devsynth, harness     # noqa: E402
from svim_amd.bamio import NativeBam                      # noqa: E402


def shuffle_file(src, dst, seed):
    """the records of `src` in a seeded random order -> `dst` (zlib level 1 blocks of 65 280 bytes)"""
    raw = bamsort.inflate(src)
    hdr, n_ref, at = bamsort.split_header(raw)
    recs = bamsort.split_records(raw[at:], n_ref)
    order = np.random.default_rng(seed).permutation(len(recs))
    raw = hdr + b"".join(recs[k] for k in order)
    with open(dst, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(harness._bgzf_block(raw[lo:lo + 0xff00], 1))
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return len(recs), len(raw)


def one_pass(nb, first, sort):
    t = time.perf_counter()
    if not first:
        nb.rewind()
    if sort:
        nb.sort_begin()
    tot = 0
    while True:
        _, m = nb.read_batch(30000, 20, "coordinate")
        if m == 0:
            break
        tot += m
    dt = time.perf_counter() - t
    t_finish = 0.0
    if sort:
        t = time.perf_counter()
        nb.sort_finish()
        t_finish = time.perf_counter() - t
    return tot, dt, t_finish


def copy_rate(n_bytes, reps=5):
    """bytes per second of a plain device-to-device copy of n_bytes (read once, written once), the median of `reps` after a warm-up"""
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0").fill_(7)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    del a, b
    torch.cuda.empty_cache()
    return n_bytes / statistics.median(times)


def full_sort(nb, max_bytes, spill_dir, piece_blocks):
    """rewind, pass, finish, encode every piece, index -> (seconds, sha of the file and the index, stats, spill stats)"""
    import hashlib
    t = time.perf_counter()
    nb.rewind()
    nb.sort_begin(max_bytes, spill_dir)
    while nb.read_batch(30000, 20, "coordinate")[1]:
        pass
    _, _, n_blocks = nb.sort_finish()
    h = hashlib.sha256()
    for first in range(0, n_blocks, piece_blocks):
        h.update(nb.sort_encode(first, min(piece_blocks, n_blocks - first)))
    h.update(nb.sort_index())
    dt = time.perf_counter() - t
    st, sp = nb.sort_stats(), nb.sort_spill_stats()
    nb.sort_abort()
    return dt, h.hexdigest(), st, sp


def spill_main(a, shuffled, nrec, raw):
    n_file_blocks = -(-raw // 0xff00)
    os.environ["SVX_BAM_DEV_CHUNK_BLOCKS"] = str(max(1, n_file_blocks // a.spill_split))
    nb = NativeBam(shuffled)
    nb.set_device_decode(0)
    while nb.read_batch(30000, 20, "coordinate")[1]:
        pass
    _, _, st, sp = full_sort(nb, 0, None, a.piece_blocks)
    arena, max_chunk = st["arena_bytes"], sp["max_chunk_bytes"]
    ways = [("in_memory", 0, None), ("arena_4", max(max_chunk, arena // 4), a.spill_dir), ("arena_16", max(max_chunk, arena // 16), a.spill_dir)]
    for _, mb, d in ways:
        full_sort(nb, mb, d, a.piece_blocks)                                   # warm-up of each way
    times, last, shas = {w[0]: [] for w in ways}, {}, {}
    for _ in range(a.passes):
        for name, mb, d in ways:
            dt, sha, st, sp = full_sort(nb, mb, d, a.piece_blocks)
            times[name].append(dt)
            last[name], shas[name] = (st, sp), sha
    nb.close()
    line = {"tool": "bam_sort_rate", "mode": "spill", "records": nrec, "inflated_bytes": raw, "qualities": bool(a.qual), "passes": a.passes, "piece_blocks": a.piece_blocks,
            "spill_split": a.spill_split, "arena_bytes": arena, "max_chunk_bytes": max_chunk, "same_bytes_three_ways": len(set(shas.values())) == 1}
    for name, mb, _ in ways:
        st, sp = last[name]
        m = statistics.median(times[name])
        line[name] = {"max_bytes": mb, "sort_s": times[name], "sort_s_median": m, "records_per_s": nrec / m, "stream_bytes_per_s": st["stream_bytes"] / m, "n_runs": sp["n_runs"],
                      "t_spill_ms": sp["t_spill_ms"], "t_readback_ms": sp["t_readback_ms"], "t_merge_ms": sp["t_merge_ms"], "max_stage_bytes": sp["max_stage_bytes"],
                      "spilled_bytes": sp["spilled_bytes"], "readback_bytes": sp["readback_bytes"],
                      "spill_write_bytes_per_s": sp["spilled_bytes"] / (sp["t_spill_ms"] * 1e-3) if sp["t_spill_ms"] else None,
                      "spill_read_bytes_per_s": sp["readback_bytes"] / (sp["t_readback_ms"] * 1e-3) if sp["t_readback_ms"] else None,
                      "t_append_ms": st["t_append_ms"], "t_finish_ms": st["t_finish_ms"], "t_encode_ms": st["t_encode_ms"], "t_gather_ms": st["t_gather_ms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    os.remove(shuffled)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--passes", type=int, default=5, help="warm passes of each kind")
    ap.add_argument("--chunk-mb", type=int, default=2048)
    ap.add_argument("--piece-blocks", type=int, default=4096)
    ap.add_argument("--zlib-blocks", type=int, default=2000)
    ap.add_argument("--qual", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--spill-dir", default=None, help="measure the spilled sort instead, its spill file in this directory")
    ap.add_argument("--spill-split", type=int, default=64, help="with --spill-dir: the file is read in at least this many chunks")
    ap.add_argument("--path", default="/tmp/device_reader.bam")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bam_sort_rates.jsonl"))
    a = ap.parse_args()
    n = a.records
    b, genome, _ = devsynth.make_batch(n_reads=max(n, 1000), n50=20000, contig_len=max(3_000_000, 250 * n), seed=2, device="cuda:0")
    hb = b.slice_records(0, min(n, b.n_rec))
    harness.write_bam_from_batch(a.path, hb, ["chr1"], [int(genome.numel())], qual_seed=5 if a.qual else None)
    del b, hb
    torch.cuda.empty_cache()
    shuffled = a.path + ".shuffled.bam"
    nrec, raw = shuffle_file(a.path, shuffled, 3)
    size = os.path.getsize(shuffled)
    if a.spill_dir:
        return spill_main(a, shuffled, nrec, raw)
    os.environ["SVX_BAM_DEV_CHUNK_MB"] = str(a.chunk_mb)
    nb = NativeBam(shuffled)
    nb.set_device_decode(0)
    one_pass(nb, True, False)                              # warm-up: code objects, buffers, the page cache
    one_pass(nb, False, True)
    off, on, fin = [], [], []
    for _ in range(a.passes):
        tot, dt, _ = one_pass(nb, False, False)
        assert tot == nrec
        off.append(dt)
        tot, dt, tf = one_pass(nb, False, True)
        assert tot == nrec
        on.append(dt)
        fin.append(tf)
    n_rec, n_bytes, n_blocks = nb.sort_count()
    st_finish = nb.sort_stats()
    out_path = a.path + ".sorted.bam"
    t = time.perf_counter()
    z1, z_in, got_stream = 0, 0, []
    with open(out_path, "wb") as fh:
        for first in range(0, n_blocks, a.piece_blocks):
            comp, stream = nb.sort_encode(first, min(a.piece_blocks, n_blocks - first), stream=True)
            fh.write(comp)
            if a.check:
                got_stream.append(stream)
            for lo in range(0, len(stream), bamsort.BLOCK):
                if first + lo // bamsort.BLOCK >= a.zlib_blocks:
                    break
                blk = stream[lo:lo + bamsort.BLOCK]
                z1 += len(harness._bgzf_block(blk, 1))
                z_in += len(blk)
    t_write = time.perf_counter() - t
    t = time.perf_counter()
    index = nb.sort_index()
    t_index = time.perf_counter() - t
    st = nb.sort_stats()
    nb.sort_abort()
    nb.close()
    with open(out_path + ".bai", "wb") as fh:
        fh.write(index)
    d2d = copy_rate(n_bytes)
    gather_rate = st["gather_bytes"] / (st["t_gather_ms"] * 1e-3)
    ours_in = sum(min(bamsort.BLOCK, n_bytes - k * bamsort.BLOCK) for k in range(min(a.zlib_blocks, n_blocks - 1)))
    with open(out_path, "rb") as fh:
        head = fh.read()
    ours = 0
    at = 0
    for _ in range(min(a.zlib_blocks, n_blocks - 1)):
        bs = int.from_bytes(head[at + 16:at + 18], "little") + 1
        ours += bs
        at += bs
    assert ours_in == z_in
    m_off, m_on, m_fin = statistics.median(off), statistics.median(on), statistics.median(fin)
    line = {"tool": "bam_sort_rate", "records": nrec, "bam_bytes": size, "inflated_bytes": raw, "qualities": bool(a.qual), "chunk_mb": a.chunk_mb, "passes": a.passes,
            "piece_blocks": a.piece_blocks, "pass_s_plain": off, "pass_s_sorting": on, "finish_s": fin,
            "records_per_s_plain": nrec / m_off, "records_per_s_sorting": nrec / m_on, "sorting_over_plain": m_on / m_off, "finish_s_median": m_fin,
            "finish_sort_ms": st_finish["t_sort_ms"], "finish_layout_ms": st_finish["t_layout_ms"],
            "stream_bytes": n_bytes, "n_blocks": n_blocks, "gather_bytes_per_s": gather_rate, "d2d_copy_bytes_per_s": d2d,
            "gather_fraction_of_copy_rate": gather_rate / d2d,
            "encode_bytes_per_s": st["gather_bytes"] / (st["t_encode_ms"] * 1e-3), "encode_and_write_s": t_write, "index_s": t_index,
            "stored_block_share": st["blocks_stored"] / max(1, n_blocks - 1), "bytes_out": st["bytes_out"], "compression_ratio": st["bytes_out"] / n_bytes,
            "size_over_zlib_level_1": ours / max(1, z1), "zlib_blocks_compared": min(a.zlib_blocks, n_blocks - 1), "stats": st}
    if a.check:
        print("checking the stream and the file against the definition ...", flush=True)
        want = bamsort.sorted_stream(shuffled)
        line["stream_equals_definition"] = bool(b"".join(got_stream) == want)
        line["file_equals_host_build"] = bool(head == _lib.text_gz_host(want))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    for f in (shuffled, out_path, out_path + ".bai"):
        os.remove(f)


if __name__ == "__main__":
    main()
