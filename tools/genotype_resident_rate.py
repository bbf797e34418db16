#!/usr/bin/env python
"""GENOTYPE from resident tables, timed: a seeded BAM file -> alignment table (kept while COLLECT runs) -> CLUSTER -> COMBINE -> svx_genotype_resident -> VCF text,
device time per phase by the HIP events of the library (svx_alignments_get_stats, svx_genotype_get_stats, svx_vcf_get_stats), against the object route on the same
candidates (objects of the candidate table, SVIM_genotyping.genotype per type, write_final_vcf's table rebuild).  One JSON line.

    python tools/genotype_resident_rate.py [--reads 20000] [--sites 1500] [--batch-records 50000] [--no-object-route]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1500)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--batch-records", type=int, default=50000)
    ap.add_argument("--no-object-route", action="store_true")
    a = ap.parse_args()
    from svim_amd import SVIM_COMBINE, SVIM_genotyping, _lib, convert, harness, records, synth
    from svim_amd.lazy import SignatureList
    contigs = [("chr1", a.contig_len)]
    references, lengths = ["chr1"], [a.contig_len]
    refs = synth.make_reference(3, contigs)
    recs = synth.coordinate_sort(synth.planted_reads(5, a.reads, refs, references, lengths, n_sites=a.sites, types=("DEL", "INS", "INV")))
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                              position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False, trans_sv_max_distance=500,
                              del_ins_dup_max_distance=1.0, skip_consensus=True, minimum_score=3, minimum_depth=4, homozygous_threshold=0.8,
                              heterozygous_threshold=0.2, symbolic_alleles=True, insertion_sequences=False, read_names=False, zmws=False,
                              tandem_duplications_as_insertions=False, interspersed_duplications_as_insertions=False, sample="Sample", genome=None,
                              types="DEL,INS,INV,DUP:TANDEM,DUP:INT,BND")
    d = tempfile.mkdtemp(prefix="svx_geno_")
    path = os.path.join(d, "reads.bam")
    records.write_bam(path, references, lengths, recs)
    eng = _lib.Engine(0)
    off, codes = convert.genome_arrays(refs, references)
    out = dict(records=len(recs), cigar_ops=sum(len(r.cigartuples) for r in recs))
    for rep in range(2):                                   # the second pass is the steady state (buffers allocated, code objects loaded)
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=a.batch_records, keep_alignments=True)
        try:
            pipe.run()
            pipe.cluster(genome=(off, codes))
            pipe.combine()
            t0 = time.perf_counter()
            pipe.genotype()
            t_geno = time.perf_counter() - t0
            pipe.write_vcf(os.path.join(d, "variants.vcf"))
            res = dict(aln=eng.alignments_stats(), genotype=eng.genotype_stats(), vcf_total_ms=eng.vcf_stats()["t_total_ms"], genotype_wall_ms=1e3 * t_geno,
                       combine_ms=eng.combine_stats()["t_combine_ms"])
            names, table, sig = pipe.bam.read_names(), eng.fetch_candidates(), eng.fetch_signatures(0)
        finally:
            pipe.close()
    out["resident"] = res
    out["candidates"] = table.n
    if not a.no_object_route:
        t0 = time.perf_counter()
        bam = records.AlignmentFile(text=synth.sam_text(references, lengths, recs))
        t1 = time.perf_counter()
        lists = [list(x) for x in convert.candidate_lists(table, SignatureList(sig, references, names), references)]
        t2 = time.perf_counter()
        for lst, typ in ((lists[0], "DEL"), (lists[1], "INV"), (lists[4], "INS"), (lists[2], "DUP_INT")):
            SVIM_genotyping.genotype(lst, bam, typ, o, engine=eng)
        t3 = time.perf_counter()
        built = SVIM_COMBINE.candidate_table_from_lists((lists[2], lists[1], lists[3], lists[0], lists[4], lists[5]), references)
        t4 = time.perf_counter()
        out["object_route"] = dict(parse_records_ms=1e3 * (t1 - t0), build_objects_ms=1e3 * (t2 - t1), index_and_genotype_ms=1e3 * (t3 - t2),
                                   table_from_objects_ms=1e3 * (t4 - t3), note="host wall clock; parse_records stands for the second pass over the file",
                                   rebuilt=built is not None)
    eng.close()
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    os.rmdir(d)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
