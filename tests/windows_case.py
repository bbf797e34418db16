"""Records for the table-level tests of coordinate-window ownership (svim_amd/multigpu.py) through the whole step: tests/test_multigpu_gloo.py drives it
with the oracle as engine on CPU tensors, tests/mp_two_ranks_one_gpu.py and tests/mp_c3_ranks_one_gpu.py (their windows mode) with the device engine.

Three contigs (name order w1 < w2 < w3), partition_max_distance 1000, so cluster_step looks 100 kb to each side of a proposed cut:
  w1  sites 50 kb apart - corridors everywhere between them.  Every site carries > 100 DEL and > 100 INS signatures (random.sample runs on every one of its
      partitions), the site at 150 kb 1100 deletions (beyond the sampler's method switch at 1045 members).  The proposals by record density at 1/2 and at 1/3
      of the records fall into sites of this contig: the refined cut lies inside w1 with sampled DEL and INS partitions of the SAME contig on both of its
      sides - the stream of the rank above the cut starts where the partitions below it stop.
  w2  a signature every <= 900 bases from 5 kb to 320 kb: one partition per type, no corridor within reach of a proposal in its middle (2/3 of the records by
      density; half of the bases by length, w2:125 000) - that cut has to fall back to the contig's first base; three sites behind the run.
  w3  the far ends of split reads.
Split reads join places on both sides of the cuts (BND rows whose owner is the other window) and other contigs; a few random split reads on top."""
import random
import types

import numpy as np

REFS, LENS = ["w1", "w2", "w3"], [500000, 700000, 50000]
SITES_W1 = [(100000, 130, 130), (150000, 1100, 0), (200000, 130, 130), (250000, 130, 130), (400000, 130, 130)]          # (position, DEL reads, INS reads)
SITES_W2 = [(450000, 150, 145), (500000, 150, 145), (550000, 150, 145)]
DENSE_W2 = (5000, 320000)
BINS = 10000


def options():
    return types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=3000, segment_gap_tolerance=10, segment_overlap_tolerance=5,
                                 partition_max_distance=1000, position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5,
                                 all_bnds=False)


def build(seed=5):
    """-> (genome dict, records in coordinate order, header-only AlignmentFile)"""
    from svim_amd import records, synth
    rng = random.Random(seed)
    ref = synth.make_reference(seed, list(zip(REFS, LENS)))
    recs = []

    def cigar_read(name, tid, pos, op, size):
        """one record: 300 matching bases, a deletion / insertion of `size`, 300 matching bases"""
        left = ref[REFS[tid]][pos:pos + 300].replace("N", "A")
        skip = size if op == 2 else 0
        right = ref[REFS[tid]][pos + 300 + skip:pos + 600 + skip].replace("N", "A")
        seq = left + (synth.random_seq(rng, size) if op == 1 else "") + right
        seg = synth.Segment(0, len(seq), tid, pos, False, [(0, 300), (op, size), (0, 300)], 60)
        recs.extend(synth.records_for_read(name, seq, [seg], REFS))

    def site(tid, at, n_del, n_ins):
        for k in range(n_del):
            cigar_read("d%d_%d_%d" % (tid, at, k), tid, at - 300 + rng.randint(-40, 40), 2, 100 + rng.randint(-8, 8) + 60 * (k % 3))
        for k in range(n_ins):
            cigar_read("i%d_%d_%d" % (tid, at, k), tid, at - 300 + rng.randint(-40, 40), 1, 90 + rng.randint(-8, 8) + 50 * (k % 2))

    for at, n_del, n_ins in SITES_W1:
        site(0, at, n_del, n_ins)
    for at, n_del, n_ins in SITES_W2:
        site(1, at, n_del, n_ins)
    for k, at in enumerate(range(DENSE_W2[0], DENSE_W2[1], 800)):
        cigar_read("dd%d" % k, 1, at + rng.randint(0, 60), 2, 80 + rng.randint(0, 60))
    for k, at in enumerate(range(DENSE_W2[0] + 350, DENSE_W2[1], 900)):
        cigar_read("di%d" % k, 1, at + rng.randint(0, 60), 1, 70 + rng.randint(0, 60))

    def split_read(name, a, b):
        """two segments (tid, position, reverse) of 400 bases each, adjacent on the read"""
        seq = synth.random_seq(rng, 800)
        segs = [synth.Segment(0, 400, a[0], a[1], a[2], [(0, 400)], 60), synth.Segment(400, 800, b[0], b[1], b[2], [(0, 400)], 60)]
        recs.extend(synth.records_for_read(name, seq, segs, REFS, hard_clip_suppl=False))

    for k in range(24):
        j = 37 * k
        split_read("x%d" % k, (0, 60000 + j, False), (0, 470000 + j, False))              # both windows of w1
        split_read("y%d" % k, (0, 480000 + j, False), (0, 70000 + j, k % 2 == 1))         # ... the other way round
        split_read("z%d" % k, (1, 600000 + j, False), (0, 30000 + j, False))              # w2 -> w1
        split_read("v%d" % k, (2, 20000 + j, False), (1, 620000 + j, k % 2 == 0))         # w3 -> w2
    recs.extend(synth.fuzz_split_reads(seed + 1, 60, REFS, LENS, max_sv_size=3000))
    recs = synth.coordinate_sort(recs)
    header = records.AlignmentFile(text=synth.sam_text(REFS, LENS, []))
    return ref, recs, header


def proposals(recs, world, by="records"):
    """assign_windows from what a driver knows before COLLECT: a histogram of the record starts per 10 kb, or (by = "length") the contig lengths alone"""
    from svim_amd import multigpu
    if by == "length":
        return multigpu.assign_windows(REFS, LENS, world)
    dens = [np.bincount([a.reference_start // BINS for a in recs if a.reference_id == k], minlength=-(-LENS[k] // BINS)).astype(np.float64) for k in range(len(REFS))]
    return multigpu.assign_windows(REFS, LENS, world, weights=dens, bin_size=BINS)


def deal(recs, owner, rank, world):
    """indices of the records rank `rank` reads: those whose start lies in its proposed window (unplaced records go to the last rank, like a file's tail)"""
    rec_owner = owner.owner_of_positions(np.asarray([max(a.reference_id, 0) for a in recs], dtype=np.int64), np.asarray([a.reference_start for a in recs], dtype=np.int64))
    return [i for i, a in enumerate(recs) if (rec_owner[i] if a.reference_id >= 0 else world - 1) == rank]


def local_batch(header, o, recs, mine):
    """this rank's records as a batch whose emission slots are the FILE's (2 x global record index), with its read names and the two callbacks cluster_step takes
    for rows that change ranks"""
    from svim_amd import batch
    hb = batch.build_batch(header, o, mode="coordinate", records=[recs[i] for i in mine])
    gi = np.asarray(mine, dtype=np.int64)
    hb.arrays["order"] = (2 * gi).astype(np.uint32)
    hb.arrays["seg_order"] = (2 * gi + 1).astype(np.uint32)
    names = list(hb.read_names)
    index = {nm: i for i, nm in enumerate(names)}

    def names_of(ids):
        return [names[int(i)] for i in ids]

    def ids_of(nms):
        out = []
        for nm in nms:
            if nm not in index:
                index[nm] = len(names)
                names.append(nm)
            out.append(index[nm])
        return out
    return hb, names, names_of, ids_of


def runs(pid):
    cut = np.nonzero(np.diff(pid))[0] + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(pid)]])


def layout_report(W, sig, orc, crank, max_distance, collected_by=None):
    """What the refined cuts W did to the single-run signature table `sig` (host SigTable): cuts, rows per rank, partitions with two owners, and per cut that lies
    inside a contig the sizes of the largest sampled (> 100 members) DEL and INS partitions of THAT contig below and above it"""
    from svim_amd import _abi
    n = sig.n
    own = W.owner_of_signatures(sig.type[:n], sig.contig[:n], sig.contig2[:n], sig.start[:n], sig.end[:n], sig.pos2[:n])
    sidx, pid = orc.form_partitions(sig, crank, max_distance)
    po, pt, pc = own[sidx], sig.type[:n][sidx], sig.contig[:n][sidx]
    straddling, parts = 0, []
    for a, b in zip(*runs(pid)):
        straddling += po[a:b].min() != po[a:b].max()
        parts.append((int(pt[a]), int(pc[a]), int(po[a]), int(b - a)))
    inside = []
    for k, (c, x) in enumerate(zip(W.cut_contig, W.cut_pos)):
        if x <= 0:
            continue
        sides = {}
        for t in (_abi.SVX_DEL, _abi.SVX_INS):
            sides[t] = (max([m for tt, cc, oo, m in parts if tt == t and cc == c and oo <= k] + [0]), max([m for tt, cc, oo, m in parts if tt == t and cc == c and oo > k] + [0]))
        inside.append((REFS[int(c)], int(x), sides[_abi.SVX_DEL], sides[_abi.SVX_INS]))
    rep = {"cuts": [(REFS[int(c)], int(x)) for c, x in zip(W.cut_contig, W.cut_pos)], "rows_per_rank": [int((own == r).sum()) for r in range(W.world)],
           "straddling_partitions": int(straddling), "inside": inside, "largest_partition": max(m for _, _, _, m in parts)}
    if collected_by is not None:
        moved = own != collected_by
        rep["foreign_rows"] = int(moved.sum())
        rep["foreign_types"] = sorted({int(t) for t in sig.type[:n][moved]})
    return rep


def _compare_tables(res, full, names_by_rank, sig_one, names_one, world):
    """rank 0: the merged StepResult (device tensors) against a single-rank ClusterTable `full` and the single-rank signature table `sig_one` (host SigTable,
    emission order) with its read names -> "ok" or the first difference"""
    from mp_c3_ranks_one_gpu import _compare
    verdict = _compare(res, full)                                      # cluster columns, member_off, members through their position in emission order
    if verdict != "ok":
        return verdict
    order = np.argsort(res.sig_cols["key"].cpu().numpy(), kind="stable")
    for col in ("key", "type", "src", "aux", "contig", "start", "end", "contig2", "pos2"):
        a = res.sig_cols[col].cpu().numpy()[order]
        b = getattr(sig_one, col)[:sig_one.n]
        if a.shape != b.shape or not np.array_equal(a, b.view(np.int64) if b.dtype == np.uint64 else b):
            return "signature column %s differs" % col
    row_rank = np.repeat(np.arange(world), res.sig_counts)
    got = [names_by_rank[r][i] for r, i in zip(row_rank[order], res.sig_cols["read_id"].cpu().numpy()[order])]
    if got != [names_one[i] for i in sig_one.read_id[:sig_one.n]]:
        return "read names of the gathered signatures differ"
    return "ok"


def expected_stream_starts(W, sig, orc, crank, max_distance, world):
    """per rank and type: the 32-bit words of the seed(1524) stream the > 100-member partitions of the ranks below it consume (CPython's own generator replayed:
    multigpu.stream_words_after) - where svx_cluster has to start that rank's stream"""
    from svim_amd import multigpu as MG
    n = sig.n
    own = W.owner_of_signatures(sig.type[:n], sig.contig[:n], sig.contig2[:n], sig.start[:n], sig.end[:n], sig.pos2[:n])
    sidx, pid = orc.form_partitions(sig, crank, max_distance)
    sizes = [[[] for _ in range(6)] for _ in range(world)]
    for a, b in zip(*runs(pid)):
        if b - a > 100:
            sizes[int(own[sidx[a]])][int(sig.type[sidx[a]])].append(int(b - a))
    return [[MG.stream_words_after([m for q in range(r) for m in sizes[q][t]]) for t in range(6)] for r in range(world)]


def main_device(tag):
    """The windows mode of tests/mp_two_ranks_one_gpu.py and tests/mp_c3_ranks_one_gpu.py (under torch.distributed.run, every rank on cuda:0, backend gloo): the
    records above dealt out by assign_windows with record-density weights, COLLECT and the windowed cluster_step on the DEVICE engine, twice (the second step on
    warm buffers); with two ranks once more with the cuts proposed by length, whose only cut has no corridor within reach.  Rank 0 compares every merged table with
    a single-rank run of the same records on the device engine and with the oracle, and every rank's stream start positions with CPython's generator.
    Prints <tag>_OK <clusters> <rows that changed ranks> <largest partition> <steps compared> - or <tag>_FAIL and the first difference."""
    import os
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = "cuda:0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from svim_amd import _abi, _lib, batch, convert, multigpu as MG
    ref, recs, header = build()
    o = options()
    p = _abi.Params.from_options(o)
    max_d = int(p.partition_max_distance)
    off, codes = convert.genome_arrays(ref, REFS)
    crank = batch.contig_ranks(REFS)
    gid = np.arange(len(REFS), dtype=np.int64)
    eng = _lib.Engine(0)
    eng.set_genome(off, codes)
    ad = MG.SvxAdapter(eng, dev)
    verdict, done, n_foreign, largest = "ok", 0, 0, 0
    full = one = sig_one = names_one = orc = None
    if rank == 0:
        # the references: one rank, all records - on the device engine and on the oracle
        from oracle import oracle as om
        hb_all = batch.build_batch(header, o, mode="coordinate", records=recs)
        e1 = _lib.Engine(0)
        e1.set_genome(off, codes)
        e1.collect(hb_all, p, fetch=False)
        sig_one = e1.fetch_signatures(0)
        one = e1.cluster(p, crank, source=0)
        names_one = list(hb_all.read_names)
        e1.close()
        orc = om.Oracle()
        orc.set_genome(off, codes)
        osig, _ = orc.collect(hb_all, p)
        full = orc.cluster(p, crank, table=osig)
        if sig_one.first_difference(osig) is not None:
            verdict = "single rank signatures vs oracle: %s" % (sig_one.first_difference(osig),)
        elif one.first_difference(full, rtol=1e-12) is not None:
            verdict = "single rank clusters vs oracle: %s" % (one.first_difference(full, rtol=1e-12),)
    for by, steps in [("records", 2)] + ([("length", 1)] if world == 2 else []):
        owner = proposals(recs, world, by)
        hb, names, names_of, ids_of = local_batch(header, o, recs, deal(recs, owner, rank, world))
        for it in range(steps):
            eng.collect(hb, p, fetch=False)
            res = MG.cluster_step(ad, p, rank, world, gid, crank, owner, names_of=names_of, ids_of=ids_of)
            everyone = [None] * world
            dist.all_gather_object(everyone, (names, eng.stream_positions()[0]))
            if rank != 0 or verdict != "ok":
                continue
            where = "windows by %s, step %d: " % (by, it)
            W = res.windows
            collected_by = owner.owner_of_positions(hb_all.arrays["tid"].clip(0).astype(np.int64), hb_all.arrays["pos"].astype(np.int64))[(osig.key[:osig.n] >> np.uint64(33)).astype(np.int64)]
            rep = layout_report(W, osig, orc, crank, max_d, collected_by)
            # the layout proves something: no partition has two owners; by record density a cut lies strictly inside a contig with sampled DEL and INS partitions of that
            # contig on both sides, one of them beyond the sampler's method switch, and rows changed ranks across it; the cut in the dense run fell back
            if rep["straddling_partitions"]:
                verdict = where + "%d partitions have two owners, cuts %r" % (rep["straddling_partitions"], rep["cuts"])
            elif by == "records" and not any(min(d) > 100 and min(i) > 100 and max(d) > 1045 for _, _, d, i in rep["inside"]):
                verdict = where + "no cut inside a contig with sampled DEL and INS partitions on both sides: %r" % (rep,)
            elif by == "records" and not (rep["foreign_rows"] > 0 and _abi.SVX_BND in rep["foreign_types"]):
                verdict = where + "no BND row changed ranks: %r" % (rep,)
            elif (by == "length" or world > 2) and ("w2", -1) not in rep["cuts"]:
                verdict = where + "the cut in the dense run of w2 did not fall back: %r" % (rep["cuts"],)
            else:
                want = expected_stream_starts(W, osig, orc, crank, max_d, world)
                got = [list(e[1]) for e in everyone]
                if by == "records" and not (want[world - 1][_abi.SVX_DEL] > 0 and want[world - 1][_abi.SVX_INS] > 0):
                    verdict = where + "the last rank's DEL / INS streams would start at 0: %r" % (want,)
                elif got != want:
                    verdict = where + "stream start positions per rank and type %r, CPython's generator says %r" % (got, want)
            if verdict == "ok":
                for ref_name, ref_ct in (("single rank on the device", one), ("oracle", full)):
                    v = _compare_tables(res, ref_ct, [e[0] for e in everyone], sig_one, names_one, world)
                    if v != "ok":
                        verdict = where + "merged vs %s: %s" % (ref_name, v)
                        break
            if verdict == "ok":
                done += 1
                n_foreign, largest = max(n_foreign, rep["foreign_rows"]), rep["largest_partition"]
    if rank == 0:
        print(("%s_OK %d %d %d %d" % (tag, full.n, n_foreign, largest, done)) if verdict == "ok" else "%s_FAIL %s" % (tag, verdict), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()
