"""World 3 over gloo on the CPU (host reader, the oracle standing in for the engine): the indexed four-contig file of
tests/test_multigpu_gloo.py::test_two_ranks_indexed_bam_contig_runs read under coordinate-window ownership (harness.collect_cluster_bam_sharded with
ownership="windows": every rank reads the records that START in its windows, svx_bam_seek_region under the start rule).  The merged result, the read names of
the gathered signatures and the emission order equal the single-process run."""
import os
import socket
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

import test_multigpu_gloo as G

HERE = os.path.dirname(os.path.abspath(__file__))


def _worker_bam_windows(rank, world, port, ret, bam_path, fasta_path):
    G._setup(rank, world, port)
    try:
        import helpers as H
        from oracle import oracle as om
        from svim_amd import _abi, batch, convert, harness, multigpu, records
        o = H.options({"min_mapq": 20, "min_sv_size": 40, "max_sv_size": 20000, "segment_gap_tolerance": 10, "segment_overlap_tolerance": 5,
                       "partition_max_distance": 1000, "position_distance_normalizer": 900, "edit_distance_normalizer": 1.0,
                       "cluster_max_distance": 0.5, "all_bnds": False})
        o.genome = fasta_path
        p = _abi.Params.from_options(o)
        bam = records.AlignmentFile(bam_path)
        refs, lens = list(bam.references), list(bam.lengths)
        orc = om.Oracle()
        off, codes = convert.genome_arrays(fasta_path, refs)
        orc.set_genome(off, codes)
        hb_all = batch.build_batch(bam, o, mode="coordinate")
        sig_all, _ = orc.collect(hb_all, p)
        full = orc.cluster(p, hb_all.contig_rank, table=sig_all)
        eng = G._HostAccum(orc)

        class Adapter(multigpu.HostAdapter):
            def __init__(self):
                multigpu.HostAdapter.__init__(self, orc, None)

            def collect_counts(self):
                self.sig = eng.table()
                return multigpu.HostAdapter.collect_counts(self)
        windows = multigpu.assign_windows(refs, lens, world)
        res, pipe, names = harness.collect_cluster_bam_sharded(bam_path, o, eng, Adapter(), rank, world, threads=2, batch_records=60, ownership="windows",
                                                               windows=windows)
        ret["kept%d" % rank] = pipe.stats.get("region_records_kept", 0)
        ret["marked%d" % rank] = pipe.stats.get("region_records_marked", 0)
        pipe.bam.close()
        if rank == 0:
            # what the windows do to this file: cuts inside a contig with records on both sides, reads whose records start on two ranks
            placed = [(a.reference_id, a.reference_start, a.query_name) for a in records.AlignmentFile(bam_path).fetch(until_eof=True) if a.reference_id >= 0]
            tid = np.array([t for t, _, _ in placed]); pos = np.array([q for _, q, _ in placed])
            owner = windows.owner_of_positions(tid, pos)
            inside = 0
            for c, x in zip(windows.cut_contig, windows.cut_pos):
                inside += int(x >= 0 and ((tid == c) & (pos < x)).any() and ((tid == c) & (pos >= x)).any())
            by_read = {}
            for (_, _, nm), r in zip(placed, owner):
                by_read.setdefault(nm, set()).add(int(r))
            ret["cuts_inside"] = inside
            ret["reads_on_two_ranks"] = sum(1 for s in by_read.values() if len(s) > 1)
            ret["owned"] = [int((owner == r).sum()) for r in range(world)]
            verdict = G._compare(res, full, None)
            if verdict == "ok":
                keys = res.sig_cols["key"].numpy()
                order = np.argsort(keys, kind="stable")                                   # the emission order of the merged run is the file's
                got = [res.read_name(i) for i in res.sig_cols["read_id"].numpy()[order]]
                want = [hb_all.read_names[i] for i in sig_all.read_id[:sig_all.n]]
                if got != want:
                    verdict = "read names of the gathered signatures differ"
            ret[0] = verdict
        else:
            ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_three_ranks_indexed_bam_window_ownership(tmp_path):
    """the file as test_two_ranks_indexed_bam_contig_runs builds it (same seeds, same record counts: it meets the conditions below as it stands)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from svim_amd import bai, records, synth
    refs, lens = ["chr1", "chr2", "chr10", "chr3"], [100000, 80000, 80000, 60000]
    ref = synth.make_reference(61, list(zip(refs, lens)))
    recs = synth.coordinate_sort(synth.fuzz_split_reads(62, 260, refs, lens, max_sv_size=20000) +
                                 synth.planted_reads(63, 300, ref, refs, lens, n_sites=25, types=("DEL", "INS", "INV")))
    bam_path, fa = str(tmp_path / "m.bam"), str(tmp_path / "m.fa")
    records.write_bam(bam_path, refs, lens, recs)
    with open(bam_path + ".bai", "wb") as fh:                      # (write_bam leaves a minimal index: where contigs start.  Windows need the full one)
        fh.write(bai.build_index(*bai.rows_of_bam(bam_path)))
    synth.write_fasta(fa, ref)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker_bam_windows, args=(3, port, ret, bam_path, fa), nprocs=3, join=True)
    ret = dict(ret)
    assert [ret[r] for r in range(3)] == ["ok"] * 3, ret
    assert ret["cuts_inside"] >= 1 and ret["reads_on_two_ranks"] >= 1, ret
    assert [ret["kept%d" % r] for r in range(3)] == ret["owned"] and min(ret["owned"]) > 0, ret          # every placed record read by exactly its owner
