"""Worker of tests/test_gpu_regions.py::test_device_window_ownership_three_ranks_on_one_gpu (run under torch.distributed.run, all ranks on cuda:0, backend gloo):
the whole-genome-like file of tests/mp_c3_ranks_one_gpu.py (svim_amd/workloads.py profile c3 at a small scale) read under coordinate-window ownership - every
rank the records that START in its windows (harness.collect_cluster_bam_sharded with ownership="windows": svx_bam_seek_region under the start rule, device
reader) -, collected, clustered over the process group, gathered on rank 0.  Rank 0 compares the merged result with a single-rank run over the whole file and
with the oracle.  Prints one line: WINDOW_RANKS_OK <clusters> <cuts inside contigs with records on both sides> <reads with records on two ranks> <device reader>
<records kept by all ranks> <placed records of the file> - or the first difference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    bam_path, scale, seed = sys.argv[1], float(sys.argv[2]), int(sys.argv[3])
    torch.cuda.set_device(0)
    dev = "cuda:0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import types
    from mp_c3_ranks_one_gpu import _compare
    from svim_amd import _abi, _lib, bai, harness, multigpu as MG, workloads
    from svim_amd.batch import contig_ranks
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5,
                              partition_max_distance=1000, position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5,
                              all_bnds=False)
    p = _abi.Params.from_options(o)
    prof = workloads.profile("c3", scale)
    b, genome, g_off, meta = workloads.make_batch_full(prof, seed=seed, device=dev)          # every rank: the same batch (for the genome)
    refs = [c[0] for c in prof["contigs"]]
    lens = [int(x) for x in (g_off[1:] - g_off[:-1]).tolist()]
    if rank == 0:
        harness.write_bam_from_device_batch(bam_path, b, refs, lens, index=False, slab_bytes=64 << 20, threads=4)
        harness.index_bam(bam_path, device=0, out=bam_path + ".bai", threads=2)               # the full index: bins and linear index, built on the device
    dist.barrier()
    eng = _lib.Engine(0)
    eng.set_genome(g_off, genome, on_device=True)
    ad = MG.SvxAdapter(eng, dev)
    windows = MG.assign_windows(refs, lens, world)
    res, pipe, names = harness.collect_cluster_bam_sharded(bam_path, o, eng, ad, rank, world, threads=2, batch_records=4000, ownership="windows", windows=windows)
    device_reader = bool(pipe.device_decode)
    kept = [None] * world
    dist.all_gather_object(kept, int(pipe.stats.get("region_records_kept", 0)))
    pipe.close()
    if rank == 0:
        from oracle import oracle as om
        from helpers import granted_cpus
        e1 = _lib.Engine(0)
        e1.set_genome(g_off, genome, on_device=True)
        p1 = harness.BamPipeline(bam_path, o, e1, threads=2, batch_records=4000)
        p1.run()
        p1.cluster()
        one = e1.fetch_clusters()
        one_sig = e1.fetch_signatures(0)
        one_names = p1.bam.read_names()
        p1.close()
        e1.close()
        orc = om.Oracle()
        orc.set_threads(granted_cpus())
        orc.set_genome(g_off.cpu().numpy().astype(np.int64), genome.cpu().numpy())
        hb = b.slice_records(0, b.n_rec)
        osig, _ = orc.collect(hb, p)
        full = orc.cluster(p, contig_ranks(refs), source=0)
        if one.first_difference(full, rtol=1e-12) is not None:
            verdict = "single rank vs oracle: %s" % (one.first_difference(full, rtol=1e-12),)
        else:
            verdict = _compare(res, full)
        if verdict == "ok":
            keys = res.sig_cols["key"].cpu().numpy()
            order = np.argsort(keys, kind="stable")
            got = [res.read_name(int(i)) for i in res.sig_cols["read_id"].cpu().numpy()[order]]
            want = [one_names[int(i)] for i in one_sig.read_id[:one_sig.n]]
            if got != want:
                verdict = "read names of the gathered signatures differ"
        # what the windows do to this file
        tid, pos, rid = hb.arrays["tid"], hb.arrays["pos"], hb.arrays["read_id"]
        placed = tid >= 0
        owner = windows.owner_of_positions(tid[placed].astype(np.int64), pos[placed].astype(np.int64))
        inside = sum(int(x >= 0 and ((tid == c) & (pos < x)).any() and ((tid == c) & (pos >= x)).any()) for c, x in zip(windows.cut_contig, windows.cut_pos))
        lo = np.full(int(rid.max()) + 1, world, dtype=np.int64); hi = np.full(int(rid.max()) + 1, -1, dtype=np.int64)
        np.minimum.at(lo, rid[placed], owner); np.maximum.at(hi, rid[placed], owner)
        two = int((hi > lo).sum())
        print(("WINDOW_RANKS_OK %d %d %d %d %d %d" % (full.n, inside, two, int(device_reader), sum(kept), int(placed.sum()))) if verdict == "ok" else "WINDOW_RANKS_FAIL " + verdict,
              flush=True)
    dist.barrier()
    eng.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
