#!/usr/bin/env python3
"""The merge of several BAM files on the device (svx_bam_merge_*), on the file tools/device_reader_rate.py reads, its records shuffled and dealt into k files,
every file but the first under a rotated dictionary (so that its records are translated):

    python tools/bam_merge_rate.py [--records 20000] [--files 3] [--passes 5] [--piece-blocks 4096] [--qual] [--out profiles/bam_merge_rates.jsonl]

One process.  Per file: plain reading passes against passes that feed a session (a fresh session per pass; the clock of a feeding pass is that of
BamMerge.add, of a plain pass that of the same reads after rewind), one warm-up of each kind, then interleaved; the median of each.  k_bs_translate: its bytes
and its time between events (the session's stats), against the append of the same files merged under ONE dictionary, where no file is translated.  The phases of
finish.  The merge of the k shuffled files - open, adds, finish, every piece encoded, index - against harness-style sort_bam of their concatenation (one file,
the same records, the first dictionary), interleaved, the median of each.  The merged file and the sorted concatenation have different dictionaries and so
different bytes: only their record counts are compared.  Recorded figures, no thresholds.  One JSON line is appended to --out; the working files are written
beside --path (default: the system's temporary directory) and removed at the end."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from svim_amd import bamsort, devsynth, harness           # noqa: E402
from svim_amd.bamio import BamMerge, NativeBam            # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_raw(path, raw):
    with open(path, "wb") as fh:
        for lo in range(0, len(raw), 0xff00):
            fh.write(harness._bgzf_block(raw[lo:lo + 0xff00], 1))
        fh.write(EOF_BLOCK)


def header(text, refs, lens):
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for r, n in zip(refs, lens):
        out += struct.pack("<i", len(r) + 1) + r.encode() + b"\0" + struct.pack("<i", n)
    return out


def deal(src, paths, seed, rotate):
    """the records of `src`, shuffled, dealt round-robin into len(paths) files over a dictionary of the file's reference plus two more; with `rotate`, file f
    lists the dictionary rotated by f, its ids renumbered to match -> (records per file, the concatenation's path)"""
    raw = bamsort.inflate(src)
    hdr, n_ref, at = bamsort.split_header(raw)
    recs = bamsort.split_records(raw[at:], n_ref)
    order = np.random.default_rng(seed).permutation(len(recs))
    l_text = struct.unpack_from("<i", hdr, 4)[0]
    p = 12 + l_text
    l_name = struct.unpack_from("<i", hdr, p)[0]
    name, length = hdr[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", hdr, p + 4 + l_name)[0]
    refs, lens = [name, "extra_a", "extra_b"], [length, 1000, 1000]
    text = lambda rr, ll: "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in zip(rr, ll))      # noqa: E731
    counts = []
    for f, path in enumerate(paths):
        k = f % len(refs) if rotate else 0
        rr, ll = refs[k:] + refs[:k], lens[k:] + lens[:k]
        new_of_old = {t: rr.index(refs[t]) for t in range(len(refs))}
        mine = []
        for g in order[f::len(paths)]:
            r = bytearray(recs[g])
            for off in (4, 24):
                t = struct.unpack_from("<i", r, off)[0]
                if t >= 0:
                    struct.pack_into("<i", r, off, new_of_old[t])
            mine.append(bytes(r))
        write_raw(path, header(text(rr, ll), rr, ll) + b"".join(mine))
        counts.append(len(mine))
    whole = paths[0] + ".whole.bam"
    write_raw(whole, header(text(refs, lens), refs, lens) + b"".join(recs[g] for g in order))
    return counts, whole


def read_pass(nb):
    t = time.perf_counter()
    nb.rewind()
    n = 0
    while True:
        m = nb.read_batch(200000, 0, "coordinate")[1]
        if not m:
            return n, time.perf_counter() - t
        n += m


def merge_once(paths, piece_blocks, encode=True):
    """open, adds, finish, every piece, index -> (seconds, seconds per add, stats)"""
    t0 = time.perf_counter()
    readers = [NativeBam(p) for p in paths]
    for r in readers:
        r.set_device_decode(0)
    m = BamMerge.open(readers, device=0)
    adds = []
    try:
        for r in readers:
            t = time.perf_counter()
            m.add(r)
            adds.append(time.perf_counter() - t)
            r.close()
        _, _, n_blocks = m.finish()
        if encode:
            for first in range(0, n_blocks, piece_blocks):
                m.encode(first, min(piece_blocks, n_blocks - first))
            m.index()
        return time.perf_counter() - t0, adds, m.stats()
    finally:
        m.close()
        for r in readers:
            r.close()


def sort_once(path, piece_blocks):
    t0 = time.perf_counter()
    nb = NativeBam(path)
    nb.set_device_decode(0)
    try:
        nb.sort_begin()
        while nb.read_batch(200000, 0, "coordinate")[1]:
            pass
        _, _, n_blocks = nb.sort_finish()
        for first in range(0, n_blocks, piece_blocks):
            nb.sort_encode(first, min(piece_blocks, n_blocks - first))
        nb.sort_index()
        return time.perf_counter() - t0, nb.sort_stats()
    finally:
        nb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--files", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--piece-blocks", type=int, default=4096)
    ap.add_argument("--qual", action="store_true")
    ap.add_argument("--path", default=os.path.join(tempfile.gettempdir(), "device_reader_merge.bam"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bam_merge_rates.jsonl"))
    a = ap.parse_args()
    n = a.records
    b, genome, _ = devsynth.make_batch(n_reads=max(n, 1000), n50=20000, contig_len=max(3_000_000, 250 * n), seed=2, device="cuda:0")
    hb = b.slice_records(0, min(n, b.n_rec))
    harness.write_bam_from_batch(a.path, hb, ["chr1"], [int(genome.numel())], qual_seed=5 if a.qual else None)
    del b, hb
    torch.cuda.empty_cache()
    rotated = ["%s.rot%d.bam" % (a.path, f) for f in range(a.files)]
    same = ["%s.same%d.bam" % (a.path, f) for f in range(a.files)]
    counts, whole = deal(a.path, rotated, 3, True)
    deal(a.path, same, 3, False)
    # per file: the reading pass plain against feeding
    plain, feeding = [[] for _ in rotated], [[] for _ in rotated]
    readers = [NativeBam(p) for p in rotated]
    for r in readers:
        r.set_device_decode(0)
        read_pass(r)
    merge_once(rotated, a.piece_blocks, encode=False)
    for _ in range(a.passes):
        for f, r in enumerate(readers):
            plain[f].append(read_pass(r)[1])
        _, adds, _ = merge_once(rotated, a.piece_blocks, encode=False)
        for f, dt in enumerate(adds):
            feeding[f].append(dt)
    for r in readers:
        r.close()
    # the translation against the append without it; the merge against the sort of the concatenation
    merge_once(same, a.piece_blocks)
    sort_once(whole, a.piece_blocks)
    t_rot, t_same, t_sort, st_rot, st_same, st_sort = [], [], [], None, None, None
    for _ in range(a.passes):
        dt, _, st_rot = merge_once(rotated, a.piece_blocks)
        t_rot.append(dt)
        dt, _, st_same = merge_once(same, a.piece_blocks)
        t_same.append(dt)
        dt, st_sort = sort_once(whole, a.piece_blocks)
        t_sort.append(dt)
    mg = st_rot["merge"]
    line = {"tool": "bam_merge_rate", "records": sum(counts), "files": a.files, "records_per_file": counts, "qualities": bool(a.qual), "passes": a.passes, "piece_blocks": a.piece_blocks,
            "pass_s_plain": plain, "pass_s_feeding": feeding,
            "feeding_over_plain": [statistics.median(x) / statistics.median(y) for x, y in zip(feeding, plain)],
            "translate": {"files": mg["n_translated_files"], "chunks": mg["n_translated_chunks"], "records": mg["n_translated_records"], "bytes": mg["translate_bytes"], "ms": mg["t_translate_ms"],
                          "bytes_per_s": mg["translate_bytes"] / (mg["t_translate_ms"] * 1e-3) if mg["t_translate_ms"] else None,
                          "append_ms_translated": st_rot["t_append_ms"], "append_ms_identity": st_same["t_append_ms"]},
            "finish": {k: st_rot[k] for k in ("t_finish_ms", "t_sort_ms", "t_layout_ms", "key_bits")},
            "merge_s": t_rot, "merge_identity_s": t_same, "sort_of_concatenation_s": t_sort,
            "merge_over_sort": statistics.median(t_rot) / statistics.median(t_sort),
            "records_equal": st_rot["n_records"] == st_same["n_records"] == st_sort["n_records"],
            "stats_merge": st_rot, "stats_sort": st_sort}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    for f in rotated + same + [whole, a.path]:
        if os.path.exists(f):
            os.remove(f)


if __name__ == "__main__":
    main()
