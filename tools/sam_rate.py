#!/usr/bin/env python3
"""SAM text through the device reader (svx_sam_open; csrc/sam.hip), on the file tools/device_reader_rate.py reads, written as SAM text with seeded qualities:

    python tools/sam_rate.py [--records 6000] [--passes 5] [--out profiles/sam_rates.jsonl]

Two figures, each beside its yardstick from the same run:
  kernels   text GB/s of k_sam_measure and of k_sam_emit alone (svx_sam_get_stats: t_measure_kernel_ms / t_emit_kernel_ms, between events on the stream; median
            over the warm passes) beside a device-to-device copy of the same text-plus-stream byte count - the streaming bound they are judged against.  The
            host-clock phases (which hold the scans, the line ends and the read-backs too) are recorded beside them.
  pipeline  records/s from the SAM file to COLLECT beside the same records from their BAM file (BamPipeline; the clock of a pass starts before it opens the file).
One warm-up pass of each kind first; medians of the warm passes.  One JSON line is appended to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                              # noqa: E402
from svim_amd import _lib, bamsort, devsynth, harness, sam  # noqa: E402
from svim_amd.bamio import NativeBam                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=6000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="sam_rate_")
    bam_path, sam_path = os.path.join(d, "reads.bam"), os.path.join(d, "reads.sam")
    b, genome, meta = devsynth.make_batch(n_reads=max(a.records, 1000), n50=20000, contig_len=max(3_000_000, 250 * a.records), seed=2, device="cuda:0")
    hb = b.slice_records(0, min(a.records, b.n_rec))
    refs, lens = ["chr1"], [int(genome.numel())]
    n_rec, raw_bytes = harness.write_bam_from_batch(bam_path, hb, refs, lens, qual_seed=7)
    del b, hb
    torch.cuda.empty_cache()
    raw = bamsort.inflate(bam_path)
    hdr, n_ref, at = bamsort.split_header(raw)
    recs = bamsort.split_records(raw[at:], n_ref)
    with open(sam_path, "wb") as fh:
        fh.write(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % lens[0])
        for r in recs:
            fh.write(sam.line_of_record(r, refs) + b"\n")
    text_bytes, stream_bytes = os.path.getsize(sam_path), len(raw) - at
    del raw, recs

    # ---- the kernels: phases of the front end over warm passes of the reader alone ----
    nb = NativeBam(sam_path)
    nb.set_device_decode(0)
    per_pass, last = [], None
    for it in range(a.passes + 1):
        t = time.perf_counter()
        if it:
            nb.rewind()
        tot = 0
        while True:
            _, m = nb.read_batch(30000, 20, "coordinate")
            if m == 0:
                break
            tot += m
        dt = time.perf_counter() - t
        st = nb.sam_stats()
        if last is not None:
            per_pass.append({k: st[k] - last[k] for k in ("t_stage_ms", "t_lines_ms", "t_measure_ms", "t_emit_ms", "t_patch_ms", "t_measure_kernel_ms", "t_emit_kernel_ms")} | {"t_pass_s": dt})
        last = st
        assert tot == n_rec
    nb.close()
    med = {k: statistics.median(p[k] for p in per_pass) for k in per_pass[0]}
    # ---- the yardstick: a device-to-device copy of text + stream bytes ----
    n_copy = text_bytes + stream_bytes
    src = torch.empty(n_copy, dtype=torch.uint8, device="cuda:0").random_(0, 255)
    dst = torch.empty_like(src)
    times = []
    for it in range(a.passes + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    t_copy = statistics.median(times[1:])
    del src, dst
    # ---- the pipeline: file -> COLLECT, SAM beside BAM ----
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                              position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False)
    eng = _lib.engine()

    def collect(path):
        ts = []
        for it in range(a.passes + 1):
            t = time.perf_counter()
            pipe = harness.BamPipeline(path, o, eng, device_decode=True)
            n = pipe.run()
            pipe.close()
            ts.append(time.perf_counter() - t)
            assert n == n_rec
        return statistics.median(ts[1:])
    t_sam, t_bam = collect(sam_path), collect(bam_path)
    res = {"tool": "sam_rate", "records": n_rec, "text_bytes": text_bytes, "stream_bytes": stream_bytes, "passes": a.passes,
           "measure_kernel_ms": med["t_measure_kernel_ms"], "emit_kernel_ms": med["t_emit_kernel_ms"],
           "measure_phase_ms": med["t_measure_ms"], "emit_phase_ms": med["t_emit_ms"], "lines_phase_ms": med["t_lines_ms"], "stage_ms": med["t_stage_ms"], "patch_ms": med["t_patch_ms"],
           "reader_pass_s": med["t_pass_s"], "measure_text_gbps": text_bytes / med["t_measure_kernel_ms"] / 1e6, "emit_text_gbps": text_bytes / med["t_emit_kernel_ms"] / 1e6,
           "copy_bytes": n_copy, "copy_ms": t_copy * 1e3, "copy_gbps_read_plus_write_counted_once": n_copy / t_copy / 1e9,
           "emit_over_copy": (t_copy * 1e3) / med["t_emit_kernel_ms"], "measure_over_copy": (t_copy * 1e3) / med["t_measure_kernel_ms"],
           "collect_records_per_s_sam": n_rec / t_sam, "collect_records_per_s_bam": n_rec / t_bam, "sam_over_bam": t_bam / t_sam}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    for f in (bam_path, bam_path + ".bai", sam_path):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(d)


if __name__ == "__main__":
    main()
