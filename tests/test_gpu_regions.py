"""Region reads on the device (svx_bam_seek_region with device decode: csrc/bamdev.hip k_region_*, the loader of csrc/bamio.cpp): device reader == host reader ==
regions.select on every case of tests/region_cases.py under both rules, whatever the chunks; the tiled span path decides a keep; BamPipeline(regions=...) with
the device reader equals the same pipeline over the sub-file; the state rules; a pass without regions is what it was; window ownership over three ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import region_cases as RC
from svim_amd import _abi, _lib, bai, harness, records, regions as RG
from svim_amd._lib import SvxError
from svim_amd.bamio import NativeBam

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return RC.build_all(str(tmp_path_factory.mktemp("region_cases_gpu")))


def _host(path):
    return NativeBam(path, threads=2)


def _device(path):
    bam = NativeBam(path, threads=2)
    bam.set_device_decode(0)
    return bam


@pytest.fixture(scope="module")
def whole(cases):
    """a pass over every whole file by the host reader, once: what both readers' runs are slices of"""
    out = {}
    for c in cases:
        bam = _host(c.path)
        try:
            out[c.name] = RC.read_table(bam)
        finally:
            bam.close()
    return out


def _set_chunk_blocks(monkeypatch, chunk_blocks):
    for var in ("SVX_BAM_DEV_CHUNK_BLOCKS", "SVX_BAM_CHUNK_BLOCKS"):
        if chunk_blocks:
            monkeypatch.setenv(var, chunk_blocks)          # (read when the handle is opened / switches device decode on)
        else:
            monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("files", ["straddle_two_and_three_blocks", "the_other_thirteen"])
@pytest.mark.parametrize("rule", RG.RULES)
@pytest.mark.parametrize("chunk_blocks", ["1", "3", None])
def test_device_region_reader_equals_host_reader_and_select(cases, whole, monkeypatch, chunk_blocks, rule, files):
    """every run the device reader hands out is the slice of the host reader's pass that regions.select and the stop rule name, marked records flagged, and
    region_stats counts it (the host reader's own runs are held to the same slices, with the same chunk sizes, in tests/test_regions.py).  Chunks of 1 and
    3 blocks: chunks in front of the first kept record are dropped, runs and stops straddle chunk edges"""
    _set_chunk_blocks(monkeypatch, chunk_blocks)
    runs = marked = 0
    for c in [c for c in cases if (c.name == files) == (files == "straddle_two_and_three_blocks")]:      # (the largest file on its own: a case stays a few seconds)
        if rule == RG.RULE_OVERLAP:
            bam = _device(c.path)
            try:
                assert RC.first_difference(RC.read_table(bam), whole[c.name]) is None, c.name      # the whole file: device == host
            finally:
                bam.close()
        r, m = RC.check_reader(c, whole[c.name], _device, rule)
        runs, marked = runs + r, marked + m
    # (under the start rule no record of a run is marked: between the first record with beg <= pos and the first with pos >= end every pos lies inside)
    # (tests/region_cases.census: 37 region sets of the largest file keep records and 16 hold a marked record between kept ones; the other files 309 and 18)
    assert runs >= (37 if files == "straddle_two_and_three_blocks" else 250) and (marked >= 10 if rule == RG.RULE_OVERLAP else marked == 0)


def test_device_region_first_kept_record_is_the_cg_record(cases, whole):
    """a region that only the CG record beyond 65 536 operations reaches from the left: the tiled span path decides that it is kept"""
    c = next(x for x in cases if x.name == "cg_tag_long_cigar")
    k = max(range(len(c.rows)), key=lambda i: whole[c.name]["n_cigar"][i])
    assert whole[c.name]["n_cigar"][k] > 65536
    lo, hi = bai.interval(c.rows[k])
    others = max(bai.interval(r)[1] for i, r in enumerate(c.rows) if i != k and r[0] == c.rows[k][0])
    assert hi - 5 > others                                                                  # nothing else reaches the region
    g = (c.rows[k][0], hi - 5, hi + 100)
    (voff, tid, beg, end), = RG.plan(c.bai, [g])
    bam = _device(c.path)
    try:
        bam.seek_region(voff, tid, beg, end)
        T = RC.read_table(bam)
        kept = [i for i, f in enumerate(T["flag"]) if not f & RC.SKIP]
        assert len(kept) == 1 and T["n_cigar"][kept[0]] > 65536 and kept[0] == 0 and bam.region_stats()["n_kept"] == 1
        bam.seek_region(voff, tid, hi, hi + 100)                                           # one base further: the record ends in front of it
        assert len(RC.read_table(bam)["tid"]) == 0 and bam.region_stats()["n_kept"] == 0
    finally:
        bam.close()


def test_device_region_state_rules(cases, tmp_path):
    c = next(x for x in cases if x.name == "bin_edges")
    voff, tid, beg, end = RG.plan(c.bai, [(1, 1 << 14, (1 << 14) + 10)])[0]
    bam = _device(c.path)
    try:
        bam.seek_region(voff, tid, beg, end)
        with pytest.raises(SvxError) as e:
            bam.read_batch(10, 20, "queryname")
        assert e.value.code == _abi.SVX_E_STATE
        n_region = len(RC.read_table(bam)["tid"])
        assert 0 < n_region < len(c.rows)
        bam.rewind()
        bam.index_begin()
        with pytest.raises(SvxError) as e:
            bam.seek_region(voff, tid, beg, end)
        assert e.value.code == _abi.SVX_E_STATE
        bam.index_abort()
        bam.rewind()
        bam.sort_begin()
        with pytest.raises(SvxError) as e:
            bam.seek_region(voff, tid, beg, end)
        assert e.value.code == _abi.SVX_E_STATE
        bam.sort_abort()
        # a region read from the file's first record leaves the handle where a rewind does: an index build or a sort pass over it is still refused
        bam.seek_region(c.rows[0][4], c.rows[0][0], 0, 10)
        from svim_amd.bamsort import BamSortError
        for begin, error in ((bam.index_begin, SvxError), (bam.sort_begin, BamSortError)):
            with pytest.raises(error) as e:
                begin()
            assert e.value.code == _abi.SVX_E_STATE and "region read" in str(e.value)
        bam.rewind()
        bam.index_begin()                                                                   # (the rewind has lifted the bound)
        bam.index_abort()
        bam.seek_region(voff, tid, beg, end)
        bam.rewind()                                                                        # lifts the bound
        assert len(RC.read_table(bam)["tid"]) == len(c.rows)
        for args in ((voff, 9, 0, 10), (voff, 0, 10, 10), (voff, 0, -1, 5)):
            with pytest.raises(SvxError) as e:
                bam.seek_region(*args)
            assert e.value.code == _abi.SVX_E_ARG
    finally:
        bam.close()
    sam = str(tmp_path / "t.sam")
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c0\tLN:1000\nr\t0\tc0\t5\t60\t4M\t*\t0\t0\tACGT\t*\n")
    bam = _device(sam)
    try:
        with pytest.raises(SvxError) as e:
            bam.seek_region(0, 0, 0, 10)
        assert e.value.code == _abi.SVX_E_STATE
    finally:
        bam.close()


def test_device_region_counts_only_the_run_in_an_unsorted_file(tmp_path):
    """a file that is not sorted: 300 records of the first reference, 50 of the second, the same 300 again.  The read ends at the first stop, inside the first 300;
    the records behind it that the rule would keep are neither handed out nor counted, by the device reader as by the host reader"""
    recs = []
    for k, (t, i) in enumerate([(0, i) for i in range(300)] + [(1, i) for i in range(50)] + [(0, i) for i in range(300)]):
        a = records.AlignedSegment()
        a.query_name, a.flag, a.reference_id, a.reference_start, a.mapping_quality = "r%d" % k, 0, t, 100 + 10 * i, 60
        a.cigartuples, a.query_sequence = [(0, 50)], "A" * 50
        recs.append(a)
    path = str(tmp_path / "unsorted.bam")
    records.write_bam(path, ["c0", "c1"], [10000, 10000], recs, sort_order="unsorted")
    _, rows, _ = bai.rows_of_bam(path)
    assert len(rows) == 650
    # [1000, 2500): pos = 100 + 10 i; the start rule keeps i in [90, 240), the overlap rule (50 bases each) i in [86, 240); the stop is record 240
    for rule, n_want in ((RG.RULE_START, 150), (RG.RULE_OVERLAP, 154)):
        got = {}
        for kind, opener in (("host", _host), ("device", _device)):
            bam = opener(path)
            try:
                bam.seek_region(rows[0][4], 0, 1000, 2500, rule)
                got[kind] = (RC.read_table(bam), bam.region_stats())
            finally:
                bam.close()
        for kind in got:
            T, st = got[kind]
            assert len(T["tid"]) == n_want and not (T["flag"] & RC.SKIP).any() and list(T["pos"]) == [100 + 10 * i for i in range(240 - n_want, 240)], (kind, rule)
            assert st["n_kept"] == n_want and st["n_marked"] == 0 and st["n_seen"] == 240, (kind, rule, st)
        assert RC.first_difference(got["device"][0], got["host"][0]) is None


def test_device_whole_file_pass_untouched_by_a_region_pass(cases, whole):
    c = next(x for x in cases if x.name == "straddle_two_and_three_blocks")
    bam = _device(c.path)
    try:
        before = RC.read_table(bam)
        for voff, tid, beg, end in RG.plan(c.bai, [(1, 1000, 90000), (3, 100000, 180000)]):
            bam.seek_region(voff, tid, beg, end)
            assert len(RC.read_table(bam)["tid"]) > 0
        bam.rewind()
        after = RC.read_table(bam)
        assert RC.first_difference(after, before) is None and RC.first_difference(after, whole[c.name]) is None
        assert not (after["flag"] & RC.SKIP).any()
    finally:
        bam.close()


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    return _lib.engine()


@pytest.fixture(scope="module")
def called_file(tmp_path_factory):
    """the seeded file of tests/test_gpu_genotype_resident.py (three contigs; planted SVs, split reads, piles for the reference allele), indexed on the device"""
    import test_gpu_genotype_resident as GR
    from svim_amd import convert
    d = tmp_path_factory.mktemp("region_pipeline_gpu")
    references, lengths, refs, recs = GR._seeded_records()
    path = str(d / "seeded.bam")
    records.write_bam(path, references, lengths, recs)
    harness.index_bam(path, out=path + ".bai")                      # (write_bam leaves a minimal index: regions need the full one)
    n_ref, rows, v_end = bai.rows_of_bam(path)
    assert open(path + ".bai", "rb").read() == bai.build_index(n_ref, rows, v_end)
    return dict(path=path, refs=references, lens=lengths, recs=recs, rows=rows, genome=convert.genome_arrays(refs, references), options=GR._options(), body=GR._body)


def _sig_rows(t, names):
    return [(int(t.type[i]), int(t.contig[i]), int(t.start[i]), int(t.end[i]), int(t.contig2[i]), int(t.pos2[i]), names[int(t.read_id[i])], t.sequence(i)) for i in range(t.n)]


@pytest.mark.parametrize("regions", [["chr1:30,001-90,000"], ["chr2:1-20,000", ("chr1", 70000, 100000), "chr1:10,001-40,000"]])
def test_device_pipeline_over_regions_equals_pipeline_over_the_sub_file(called_file, eng, regions, tmp_path):
    import genotype_cases as GC
    f = called_file
    o = f["options"]
    parsed = RG.normalise([RG.as_region(r, f["refs"], f["lens"]) for r in regions])
    keep = [any(RG.keeps(row, g) for g in parsed) for row in f["rows"]]
    assert 200 < sum(keep) < len(keep) - 200
    sub = str(tmp_path / "sub.bam")
    records.write_bam(sub, f["refs"], f["lens"], [a for a, k in zip(f["recs"], keep) if k])

    def run(path, label, **kw):
        pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=211, device_decode=True, keep_alignments=True, **kw)
        try:
            n = pipe.run()
            pipe.cluster(genome=f["genome"])
            pipe.combine()
            pipe.genotype()
            out = str(tmp_path / ("variants_%s.vcf" % label))
            pipe.write_vcf(out)
            return dict(n=n, body=f["body"](out), g=GC.columns_as_fields(eng.fetch_genotypes()), sig=_sig_rows(eng.fetch_signatures(0), pipe.bam.read_names()),
                        clusters=eng.fetch_clusters(), stats=dict(pipe.stats))
        finally:
            pipe.close()
    a = run(f["path"], "regions", regions=regions)
    b = run(sub, "sub")
    st = a["stats"]
    assert st["region_records_kept"] == sum(keep) == b["n"] and a["n"] == st["region_records_kept"] + st["region_records_marked"] and st["region_bytes_inflated"] > 0
    assert a["sig"] == b["sig"] and len(a["sig"]) > 20
    assert a["clusters"].first_difference(b["clusters"], rtol=0) is None and a["clusters"].n > 5
    assert a["body"] == b["body"] and len(a["body"].splitlines()) > 3
    assert a["g"] == b["g"] and any(x[1] not in ("./.", None) for x in a["g"])


def test_device_window_ownership_three_ranks_on_one_gpu(tmp_path):
    """three processes share cuda:0 over gloo; each reads the records that start in its coordinate windows of one indexed 47-contig file with the device reader
    (ownership="windows"), collects and clusters; merged == single rank over the whole file == oracle, read names resolve (tests/mp_window_ranks_one_gpu.py)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(REPO, "tests", "mp_window_ranks_one_gpu.py"), str(tmp_path / "wg.bam"), "0.003", "3"],
                         capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    ok = [l for l in out.stdout.splitlines() if l.startswith("WINDOW_RANKS_")]
    assert ok and ok[0].startswith("WINDOW_RANKS_OK"), (out.stdout[-2000:], out.stderr[-2000:])
    _, n_clusters, cuts_inside, reads_on_two, dev_reader, kept, placed = ok[0].split()
    assert int(n_clusters) > 500 and int(cuts_inside) >= 1 and int(dev_reader) == 1 and int(kept) == int(placed) > 1000
