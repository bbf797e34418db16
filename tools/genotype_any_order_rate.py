#!/usr/bin/env python
"""The alignment table in any record order, timed.  Two sets of figures, one JSON line each, appended to profiles/genotype_any_order_rates.jsonl:

  finalisation   rows handed over as record batches in shuffled and in sorted order under svx_collect_keep_alignments_mode(SVX_ALN_SORT): the finalisation's ms
                 with and without the sort (svx_alignments_get_stats), its key / sort / gather split (svx_alignments_get_sort_stats), the bytes the gather
                 moves and their share of the HBM peak
  end_to_end     wall time from a file in query-name order (SAM text without qualities, and a BAM file) to a genotyped VCF: one pass
                 (BamPipeline(mode="queryname", alignment_order="sort")) against sam_to_bam / sort_bam followed by the coordinate pipeline

    python tools/genotype_any_order_rate.py [--rows 20000,2000000,8000000] [--reads 20000] [--sites 1500] [--out profiles/genotype_any_order_rates.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12            # bytes / s, MI355X
# per row: the source row number read (4), seven columns read at it and written in order (23 + 23), the copy back over the table (23 + 23)
GATHER_BYTES_PER_ROW = 4 + 4 * 23

OPTS = dict(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
            position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
            del_ins_dup_max_distance=1.0, skip_consensus=True, minimum_score=3, minimum_depth=4, homozygous_threshold=0.8, heterozygous_threshold=0.2,
            symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False, tandem_duplications_as_insertions=False,
            interspersed_duplications_as_insertions=False, sample="Sample", genome=None, types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")


def rows_batch(references, tid, pos, flag, mapq, span, read_id):
    """rows of one M operation each as the record batch of the Python batcher (batch.build_batch, coordinate mode)"""
    from svim_amd.batch import HostBatch, contig_ranks
    n = tid.size
    hb = HostBatch()
    hb.n_rec, hb.n_seg, hb.references = n, 0, list(references)
    A = hb.arrays
    A["flag"], A["tid"], A["pos"], A["mapq"], A["read_id"] = flag, tid, pos, mapq, read_id
    A["lseq"] = np.zeros(n, np.int32)
    A["order"], A["seg_order"] = (2 * np.arange(n)).astype(np.uint32), (2 * np.arange(n) + 1).astype(np.uint32)
    A["cigar_off"], A["seq_off"], A["seg_off"] = np.arange(n + 1, dtype=np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    A["cigar"] = np.concatenate([span.astype(np.uint32) << 4, np.zeros(1, np.uint32)])
    A["seq"], A["seg_rev"], A["seg_mapq"] = np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    A["seg_tid"], A["seg_pos"], A["seg_lseq"] = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    A["seg_cigar_off"], A["seg_cigar"] = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    A["contig_rank"] = contig_ranks(hb.references)
    return hb


def finalisation(eng, n, batch_rows=1_000_000):
    from svim_amd import _abi
    o = types.SimpleNamespace(**OPTS)
    p = _abi.Params.from_options(o)
    references, lengths = ["c0", "c1", "c2"], [250_000_000] * 3
    rng = np.random.RandomState(7)
    cols = dict(tid=rng.randint(0, 3, n).astype(np.int32), pos=rng.randint(0, 240_000_000, n).astype(np.int32),
                flag=rng.choice(np.array([0, 16], np.uint16), n).astype(np.uint16), mapq=np.full(n, 60, np.uint8), span=rng.randint(500, 20000, n).astype(np.int32),
                read_id=np.arange(n, dtype=np.int32))
    key = (cols["tid"].astype(np.uint64) << np.uint64(33)) | ((cols["pos"].astype(np.uint64) + np.uint64(1)) << np.uint64(1)) | (cols["flag"].astype(np.uint64) >> np.uint64(4))
    order = np.argsort(key, kind="stable")
    t = _abi.CandidateTable(1, 0)
    t.cls[0], t.contig[0], t.start[0], t.end[0], t.contig2[0], t.score[0] = _abi.CAND_DEL, 0, 10, 90, -1, 5
    v = t.view()
    v.class_count[_abi.CAND_DEL] = 1
    t.finish(v)
    res = {}
    for label, idx in (("shuffled", None), ("sorted", order)):
        c = cols if idx is None else {k: a[idx] for k, a in cols.items()}
        for rep in range(2):                               # the second pass is the steady state
            eng.keep_alignments(True, order="sort")
            eng.accumulate(True)
            base = 0
            for lo in range(0, n, batch_rows):
                hi = min(n, lo + batch_rows)
                eng.set_slot_base(base)
                eng.collect(rows_batch(references, *[np.ascontiguousarray(c[k][lo:hi]) for k in ("tid", "pos", "flag", "mapq", "span", "read_id")]), p, fetch=False)
                base += 2 * (hi - lo) + 2
            eng.keep_alignments(False, order="sort")
            eng.genotype_resident(o, lengths, table=t, sig_read_id=np.zeros(1, np.int32))
            st, ss = eng.alignments_stats(), eng.alignment_sort_stats()
            eng.accumulate(False)
        res[label] = dict(t_finalise_ms=st["t_finalise_ms"], t_append_ms=st["t_append_ms"], **ss)
    g = res["shuffled"]["t_gather_ms"]
    gather_bytes = GATHER_BYTES_PER_ROW * n
    res["gather_bytes"] = gather_bytes
    res["gather_fraction_of_hbm_peak"] = (gather_bytes / (g * 1e-3) / HBM_PEAK) if g > 0 else None
    res["sort_pair_bytes"] = 2 * 12 * n * ((res["shuffled"]["key_bits"] + 7) // 8)
    return dict(kind="finalisation", rows=n, **res)


def end_to_end(eng, a):
    from svim_amd import convert, harness, records, synth, bamsort
    o = types.SimpleNamespace(**OPTS)
    contigs = [("chr1", a.contig_len)]
    references, lengths = ["chr1"], [a.contig_len]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, a.reads, refs, references, lengths, n_sites=a.sites, types=("DEL", "INS", "INV"))
    recs = sorted(recs, key=lambda r: (r.query_name.encode(), bamsort.name_rank(r.flag)))
    genome = convert.genome_arrays(refs, references)
    d = tempfile.mkdtemp(prefix="svx_any_order_")
    sam, qbam = os.path.join(d, "reads.sam"), os.path.join(d, "reads.queryname.bam")
    with open(sam, "w") as fh:
        fh.write(synth.sam_text(references, lengths, recs, sort_order="queryname"))
    records.write_bam(qbam, references, lengths, recs, sort_order="queryname")

    def to_vcf(path, out, **kw):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=a.batch_records, keep_alignments=True, **kw)
        try:
            pipe.run()
            pipe.cluster(genome=genome)
            pipe.combine()
            pipe.genotype()
            pipe.write_vcf(out)
            return eng.fetch_candidates().n
        finally:
            pipe.close()

    res = dict(kind="end_to_end", records=len(recs), sam_bytes=os.path.getsize(sam), bam_bytes=os.path.getsize(qbam))
    for label, path in (("sam_text", sam), ("queryname_bam", qbam)):
        one, two = [], []
        for rep in range(3):
            t0 = time.perf_counter()
            n1 = to_vcf(path, os.path.join(d, "one.vcf"), mode="queryname", alignment_order="sort")
            t1 = time.perf_counter()
            tmp = os.path.join(d, "sorted.bam")
            if label == "sam_text":
                harness.sam_to_bam(path, tmp, index=False)
            else:
                harness.sort_bam(path, tmp, index=False)
            t2 = time.perf_counter()
            n2 = to_vcf(tmp, os.path.join(d, "two.vcf"))
            t3 = time.perf_counter()
            one.append(1e3 * (t1 - t0))
            two.append(dict(total_ms=1e3 * (t3 - t1), sort_ms=1e3 * (t2 - t1), pipeline_ms=1e3 * (t3 - t2)))
        res[label] = dict(one_pass_ms=one, sort_then_coordinate=two, candidates_one_pass=n1, candidates_coordinate=n2,
                          note="wall clock, three repetitions in order; the first includes allocations")
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    os.rmdir(d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="20000,2000000,8000000")
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1500)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--batch-records", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "genotype_any_order_rates.jsonl"))
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    from svim_amd import _lib
    eng = _lib.Engine(0)
    lines = [finalisation(eng, int(n)) for n in a.rows.split(",") if n]
    if not a.skip_end_to_end:
        lines.append(end_to_end(eng, a))
    eng.close()
    with open(a.out, "a") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
