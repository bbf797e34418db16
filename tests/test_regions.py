"""Region reads on the CPU (svim_amd/regions.py, csrc/region_core.hpp, the host reader of csrc/bamio.cpp): the grammar; the plan, the stop rule and select
reproduce bai.brute_force on every case of tests/region_cases.py from the .bai and from the .csi; the host reader hands out exactly the stated run under both
rules whatever its chunks; window ownership partitions a file's records; BamPipeline(regions=...) equals the pipeline over the sub-file; the state rules."""
import os
import subprocess

import numpy as np
import pytest

import region_cases as RC
from svim_amd import _abi, bai, multigpu, regions as RG
from svim_amd._lib import SvxError
from svim_amd.bamio import NativeBam

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return RC.build_all(str(tmp_path_factory.mktemp("region_cases")))


def _host(path):
    return NativeBam(path, threads=2)


@pytest.fixture(scope="module")
def whole(cases):
    """a pass over every whole file by the host reader, once"""
    out = {}
    for c in cases:
        bam = _host(c.path)
        try:
            out[c.name] = RC.read_table(bam)
        finally:
            bam.close()
        assert len(out[c.name]["tid"]) == len(c.rows), c.name
    return out


# ---- the grammar ------------------------------------------------------------------------------------------------------------------------------------------
REFS, LENS = ["chr1", "chr2", "HLA:A*01", "chr1:100-200"], [1000000, 5000, 3000, 700]


@pytest.mark.parametrize("text, want", [
    ("chr1", (0, 0, 1000000)), ("chr1:100", (0, 99, 1000000)), ("chr1:100-", (0, 99, 1000000)), ("chr1:100-200", (3, 0, 700)), ("chr1:1,000-2,000", (0, 999, 2000)),
    ("chr2:5-5", (1, 4, 5)), ("chr2:1-5000", (1, 0, 5000)), ("HLA:A*01", (2, 0, 3000)), ("HLA:A*01:10-20", (2, 9, 20)), ("chr1:100-200:7-9", (3, 6, 9)),
    ("chr1:0-10", (0, 0, 10)), (" chr2:2-3 ", (1, 1, 3)), ("chr1:10,000,000-12,000,000", (0, 9999999, 12000000))])
def test_parse_region_follows_the_samtools_grammar(text, want):
    assert RG.parse_region(text, REFS, LENS) == want


@pytest.mark.parametrize("text", ["chr3", "chr3:1-2", "chr1:200-100", "chr1:abc", "chr1:1-x", "chr1:", "chr1:-5", "chr1:1-2-3", "", ":1-2", "chr2:6000"])
def test_parse_region_refusals(text):
    with pytest.raises(ValueError):
        RG.parse_region(text, REFS, LENS)


def test_normalise_sorts_and_merges_like_samtools_view_M():
    assert RG.normalise([(1, 50, 60), (0, 10, 20), (0, 20, 30), (0, 5, 12), (0, 31, 40), (1, 55, 56), (1, 0, 5)]) == [(0, 5, 30), (0, 31, 40), (1, 0, 5), (1, 50, 60)]
    assert RG.normalise([]) == []
    with pytest.raises(ValueError):
        RG.normalise([(0, 5, 5)])
    rows = [(0, 8, 15, 0, 1), (0, 20, 25, 0, 2), (0, 30, 31, 0, 3), (1, 2, 3, 0, 4)]
    assert RG.select(rows, [(0, 10, 21), (0, 12, 14)], RG.RULE_OVERLAP) == rows[:2] and RG.select(rows, [(0, 10, 21), (0, 0, 9)], RG.RULE_START) == rows[:2]
    assert RG.as_region(("chr2", 3, 9), REFS, LENS) == (1, 3, 9) and RG.as_region((0, 3, 9), REFS, LENS) == (0, 3, 9) and RG.as_region("chr2:4-9", REFS, LENS) == (1, 3, 9)
    for bad in (("chr9", 1, 2), (0, 5, 5), (7, 0, 5), (0, -1, 5)):
        with pytest.raises(ValueError):
            RG.as_region(bad, REFS, LENS)


# ---- the definition against the index's own brute force ------------------------------------------------------------------------------------------------------
def test_cases_are_not_empty(cases):
    assert len(cases) == 14
    census = {c.name: RC.census(c) for c in cases}
    assert sum(1 for k, m, d in census.values() if k) >= 10, census
    assert sum(1 for k, m, d in census.values() if m) >= 3, census
    assert sum(1 for k, m, d in census.values() if d) >= 3, census


@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_plan_stop_and_select_reproduce_brute_force(cases, kind):
    n_kept = 0
    for c in cases:
        index = c.bai if kind == "bai" else c.csi
        for rs in c.region_sets:
            norm = RG.normalise(rs)
            planned = {(t, b, e): v for v, t, b, e in RG.plan(index, rs)}
            assert list(planned) == [g for g in norm if g in planned]                   # file order
            got = []
            for g in norm:
                want = bai.brute_force(c.rows, *g)
                if g not in planned:
                    assert want == [], (c.name, g, kind)                                  # the index proves it empty
                    continue
                start = c.row_of_vbeg[planned[g]]                                         # the plan's offset is a record's, and no kept record lies in front of it
                (first, stop), kept = RG.run(c.rows, g, RG.RULE_OVERLAP, start)
                assert [c.rows[first + k] for k, f in enumerate(kept) if f] == want, (c.name, g, kind)
                (f2, s2), kept2 = RG.run(c.rows, g, RG.RULE_START, start)
                assert [c.rows[f2 + k] for k, f in enumerate(kept2) if f] == [r for r in c.rows if r[0] == g[0] and g[1] <= r[1] < g[2]], (c.name, g, kind)
                got += want
                n_kept += len(want)
            assert sorted(got, key=lambda r: r[4]) == RG.select(c.rows, rs), (c.name, rs)
    assert n_kept > 1000


# ---- the host reader ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_blocks", ["1", "3", None])
def test_host_reader_hands_out_the_run_of_select(cases, whole, monkeypatch, chunk_blocks):
    if chunk_blocks:
        monkeypatch.setenv("SVX_BAM_CHUNK_BLOCKS", chunk_blocks)                          # (read when the handle is opened)
    else:
        monkeypatch.delenv("SVX_BAM_CHUNK_BLOCKS", raising=False)
    runs = marked = 0
    for c in cases:
        for rule in RG.RULES:
            r, m = RC.check_reader(c, whole[c.name], _host, rule)
            runs, marked = runs + r, marked + m
    assert runs > 500 and marked > 30


def test_host_reader_without_skip_flags_is_select(cases, whole):
    """the records a region read hands out without SVX_FLAG_SKIP are select's, for a set of several regions read in the plan's order"""
    c = next(x for x in cases if x.name == "straddle_two_and_three_blocks")
    rs = [(1, 1000, 90000), (3, 0, 5000), (1, 80000, 120000), (4, 200000, 200001), (3, 100000, 180000)]
    for rule in RG.RULES:
        bam = _host(c.path)
        got = []
        try:
            for voff, tid, beg, end in RG.plan(c.bai, rs, rule):
                bam.seek_region(voff, tid, beg, end, rule)
                T = RC.read_table(bam)
                got += [(int(t), int(p)) for t, p, f in zip(T["tid"], T["pos"], T["flag"]) if not f & RC.SKIP]
        finally:
            bam.close()
        want = RG.select(c.rows, rs, rule)
        assert got == [(r[0], r[1]) for r in want] and len(want) > 50, rule


def test_rewind_and_seek_lift_the_bound(cases, whole):
    c = next(x for x in cases if x.name == "bin_edges")
    bam = _host(c.path)
    try:
        voff, tid, beg, end = RG.plan(c.bai, [(1, 1 << 14, (1 << 14) + 10)])[0]
        bam.seek_region(voff, tid, beg, end)
        assert 0 < len(RC.read_table(bam)["tid"]) < len(c.rows)
        bam.rewind()
        assert RC.first_difference(RC.read_table(bam), whole[c.name]) is None
        bam.seek_region(voff, tid, beg, end, "start")
        bam.seek(c.rows[3][4])
        assert RC.first_difference(RC.read_table(bam), RC.table_slice(whole[c.name], 3, len(c.rows))) is None
    finally:
        bam.close()


def test_refusals(cases, tmp_path):
    c = next(x for x in cases if x.name == "one_record")
    bam = _host(c.path)
    try:
        for args in ((0, 9, 0, 10), (0, -1, 0, 10), (0, 0, 10, 10), (0, 0, 10, 5), (0, 0, -1, 5), (1 << 60, 0, 0, 5)):
            with pytest.raises(SvxError) as e:
                bam.seek_region(*args)
            assert e.value.code == _abi.SVX_E_ARG, args
        with pytest.raises(ValueError):
            bam.seek_region(0, 0, 0, 10, rule="inside")
        assert bam.L.svx_bam_seek_region(bam.h, 0, 0, 0, 10, 2) == _abi.SVX_E_ARG                 # an unknown rule at the C interface
        voff = RG.plan(c.bai, [(4, 0, 1 << 20)])[0][0]
        bam.seek_region(voff, 4, 0, 1 << 20)
        with pytest.raises(SvxError) as e:
            bam.read_batch(10, 20, "queryname")
        assert e.value.code == _abi.SVX_E_STATE
        assert bam.read_batch(10, 20)[1] == 1                                                      # the handle is where it was
    finally:
        bam.close()
    sam = str(tmp_path / "t.sam")
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c0\tLN:1000\nr\t0\tc0\t5\t60\t4M\t*\t0\t0\tACGT\t*\n")
    bam = NativeBam(sam, threads=1)
    try:
        with pytest.raises(SvxError) as e:
            bam.seek_region(0, 0, 0, 10)
        assert e.value.code == _abi.SVX_E_STATE
    finally:
        bam.close()


# ---- window ownership ---------------------------------------------------------------------------------------------------------------------------------------
def test_rank_intervals_state_the_rule_of_owner_of_positions():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n, world = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        names = ["c%d" % k for k in rng.permutation(20)[:n]]
        lens = [int(x) for x in rng.integers(1, 5000, n)]
        if trial % 3 == 0:
            win = multigpu.assign_windows(names, lens, world, bin_size=int(rng.integers(50, 900)))
        else:                                                   # seeded cuts: whole contigs (-1), inside contigs, at a contig's last base
            order = sorted(range(n), key=lambda i: names[i])
            crank = np.zeros(n, dtype=np.int64)
            crank[order] = np.arange(n)
            cuts = sorted((int(crank[c]), int(x)) for c, x in zip(rng.integers(0, n, world - 1), rng.integers(-1, 5200, world - 1)))
            win = multigpu.Windows(world, crank, [order[c] for c, _ in cuts], [min(x, lens[order[c]] - 1) if x >= 0 else -1 for c, x in cuts])
        got = {r: win.rank_intervals(r, lens) for r in range(world)}
        for c in range(n):
            pos = np.arange(lens[c])
            owner = win.owner_of_positions(np.full(lens[c], c), pos)
            for r in range(world):
                mine = [(b, e) for cc, b, e in got[r] if cc == c]
                assert len(mine) <= 1
                want = pos[owner == r]
                assert (list(range(*mine[0])) if mine else []) == list(want), (trial, c, r, mine)
        for r in range(world):
            assert [c for c, _, _ in got[r]] == sorted(c for c, _, _ in got[r])               # reference-id order
    whole = multigpu.Windows(2, [0, 1], [1], [-1])                                            # cut_pos = -1: the whole contig to the rank above
    assert whole.rank_intervals(0, [100, 50]) == [(0, 0, 100)] and whole.rank_intervals(1, [100, 50]) == [(1, 0, 50)]


@pytest.mark.parametrize("world", [2, 3, 8])
def test_window_regions_partition_the_placed_records(cases, whole, world):
    from svim_amd import harness
    import bai_cases as BC
    c = next(x for x in cases if x.name == "straddle_two_and_three_blocks")
    win = multigpu.assign_windows(BC.REFS, BC.LENS, world)
    seen = []
    for rank in range(world):
        plan = harness.window_plan(win, rank, BC.REFS, BC.LENS, c.bai)
        assert plan == sorted(plan, key=lambda g: (g[1], g[2]))
        bam = _host(c.path)
        try:
            for voff, tid, beg, end in plan:
                bam.seek_region(voff, tid, beg, end, RG.RULE_START)
                T = RC.read_table(bam)
                mine = [(int(t), int(p), nm) for t, p, f, nm in zip(T["tid"], T["pos"], T["flag"], T["name"]) if not f & RC.SKIP]
                assert all(win.owner_of_positions(np.array([t]), np.array([p]))[0] == rank for t, p, _ in mine)
                seen += [(rank,) + m for m in mine]
        finally:
            bam.close()
    placed = [(int(t), int(p), nm) for t, p, nm in zip(whole[c.name]["tid"], whole[c.name]["pos"], whole[c.name]["name"]) if t >= 0]
    assert sorted(m[1:] for m in seen) == sorted(placed) and len(seen) == len(placed)         # every placed record exactly once
    assert len({m[0] for m in seen}) >= 2


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def called_file(tmp_path_factory):
    """a file SVs are called on (four contigs, header order != name order), its records, its full index beside it"""
    from svim_amd import records, synth
    d = tmp_path_factory.mktemp("region_pipeline")
    refs, lens = ["chr1", "chr2", "chr10", "chr3"], [100000, 80000, 80000, 60000]
    ref = synth.make_reference(61, list(zip(refs, lens)))
    recs = synth.coordinate_sort(synth.fuzz_split_reads(62, 260, refs, lens, max_sv_size=20000) +
                                 synth.planted_reads(63, 300, ref, refs, lens, n_sites=25, types=("DEL", "INS", "INV")))
    path, fa = str(d / "m.bam"), str(d / "m.fa")
    records.write_bam(path, refs, lens, recs)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    with open(path + ".bai", "wb") as fh:
        fh.write(bai.build_index(n_ref, rows, v_end))
    synth.write_fasta(fa, ref)
    return dict(path=path, fasta=fa, refs=refs, lens=lens, recs=recs, rows=rows, dir=str(d))


PIPELINE_REGIONS = [["chr1:20,001-60,000"], ["chr10:1-30,000", ("chr1", 55000, 70000), "chr1:20,001-60,000", ("chr3", 100, 59000)]]


def _sig_rows(t, names):
    return [(int(t.type[i]), int(t.contig[i]), int(t.start[i]), int(t.end[i]), int(t.contig2[i]), int(t.pos2[i]), names[int(t.read_id[i])], t.sequence(i)) for i in range(t.n)]


@pytest.mark.parametrize("regions", PIPELINE_REGIONS)
def test_pipeline_over_regions_equals_pipeline_over_the_sub_file(called_file, oracle, regions, tmp_path):
    import helpers as H
    import test_multigpu_gloo as G
    from svim_amd import batch, convert, harness, records
    f = called_file
    o = H.options({"min_mapq": 20, "min_sv_size": 40, "max_sv_size": 20000, "segment_gap_tolerance": 10, "segment_overlap_tolerance": 5,
                   "partition_max_distance": 1000, "position_distance_normalizer": 900, "edit_distance_normalizer": 1.0, "cluster_max_distance": 0.5, "all_bnds": False})
    off, codes = convert.genome_arrays(f["fasta"], f["refs"])
    oracle.set_genome(off, codes)
    parsed = [RG.as_region(r, f["refs"], f["lens"]) for r in regions]
    keep = [any(RG.keeps(row, g) for g in RG.normalise(parsed)) for row in f["rows"]]
    assert 20 < sum(keep) < len(keep)
    sub = str(tmp_path / "sub.bam")
    records.write_bam(sub, f["refs"], f["lens"], [a for a, k in zip(f["recs"], keep) if k])

    def run(path, **kw):
        eng = G._HostAccum(oracle)
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=37, device_decode=False, gpu_inflate=False, **kw)
        n = pipe.run()
        names, stats = pipe.bam.read_names(), dict(pipe.stats)
        pipe.close()
        sig = eng.table()
        clu = oracle.cluster(pipe.params, batch.contig_ranks(f["refs"]), table=sig)
        return n, sig, names, clu, stats
    n, sig, names, clu, stats = run(f["path"], regions=regions)
    n2, sig2, names2, clu2, _ = run(sub)
    assert stats["region_records_kept"] == sum(keep) == n2 and n == stats["region_records_kept"] + stats["region_records_marked"] and stats["region_bytes_inflated"] > 0
    assert _sig_rows(sig, names) == _sig_rows(sig2, names2) and sig.n > 10
    assert clu.first_difference(clu2, rtol=0) is None and clu.n > 3


def test_pipeline_region_refusals(called_file, oracle, tmp_path):
    import shutil
    import helpers as H
    import test_multigpu_gloo as G
    from svim_amd import harness
    o = H.options({"min_mapq": 20, "min_sv_size": 40})
    eng = G._HostAccum(oracle)
    bare = str(tmp_path / "bare.bam")
    shutil.copy(called_file["path"], bare)
    kw = dict(threads=1, device_decode=False, gpu_inflate=False)
    with pytest.raises(ValueError, match="index_bam"):
        harness.BamPipeline(bare, o, eng, regions=["chr1:1-100"], **kw)
    with pytest.raises(ValueError, match="index_bam"):
        harness.BamPipeline(bare, o, eng, regions=["chr1:1-100"], index=bare + ".nope", **kw)
    for bad in (["chr9:1-5"], ["chr1:9-5"], [("chr1", 5, 5)], ["chr1:1-100", (0, 1)]):
        with pytest.raises(ValueError):
            harness.BamPipeline(called_file["path"], o, eng, regions=bad, **kw)
    with pytest.raises(ValueError):
        harness.BamPipeline(called_file["path"], o, eng, regions=["chr1:1-100"], build_index=True, **kw)
    with pytest.raises(ValueError):
        harness.BamPipeline(called_file["path"], o, eng, regions=["chr1:1-100"], mode="queryname", **kw)
    with pytest.raises(ValueError):
        harness.BamPipeline(called_file["path"], o, eng, regions=[(0, 1)], keep_alignments=True, **kw)
    with open(called_file["path"] + ".bai", "rb") as fh:
        data = fh.read()
    pipe = harness.BamPipeline(bare, o, eng, regions=["chr1:1-100"], index=data, **kw)          # the index as bytes
    assert pipe.regions == RG.plan(data, [(0, 0, 100)])
    pipe.close()


# ---- the host reader and region_core.hpp under the sanitizers --------------------------------------------------------------------------------------------------
def test_region_reads_under_the_sanitizers(tmp_path):
    """tools/region_host_test.cpp with bamio.cpp under AddressSanitizer + UndefinedBehaviorSanitizer: seeded regions over seeded record streams against a scan,
    through the host reader and through the chunk loader of the device reader over a CPU stand-in; a stand-alone child program with its own main"""
    out = str(tmp_path / "region_host_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    # asked BEFORE the build: a toolchain without the sanitizer runtime cannot link the smallest program; a failure of the real build is then a failure
    if subprocess.run(["g++", *san, probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *san, "-fno-omit-frame-pointer", os.path.join(REPO, "svim_amd", "csrc", "bamio.cpp"),
                            os.path.join(REPO, "tools", "region_host_test.cpp"), "-lz", "-lpthread", "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([out, "fuzz", "7", "200", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "200 files" in run.stdout and " 0 wrong" in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    reads, kept, marked = (int(run.stdout.split(w)[0].split()[-1]) for w in (" region reads", " kept records", " marked records"))
    assert reads == 4800 and kept > 5000 and marked > 1000, run.stdout[-300:]
