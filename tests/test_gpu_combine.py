"""COMBINE on the device (svx_combine, svim_amd/csrc/combine.hip) against the reference's rows (tests/golden/g_combine.json.gz, g_combine_cases.json.gz)
and against the Python replay of the reference's COMBINE (tests/combine_consumer.py)."""
import copy
import random
import types

import numpy as np
import pytest

import combine_cases as CC
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


def _expected_state(lists6, exp):
    dele, insr, inv, tan, dint, bnd = lists6
    assert len(insr) == exp["n_ins_after"] and len(dint) == exp["n_dup_int_after"]
    assert len(bnd) == exp.get("n_bnd_after", exp.get("n_bnd_after_merge"))


def test_golden_through_cluster_and_combine(eng):
    """g_combine.json.gz: signatures -> cluster_sv_signatures -> combine_clusters, both on the device, nothing materialised on the resident route"""
    import svim_amd
    from svim_amd.lazy import CandidateList, ClusterList
    g = H.load("g_combine.json.gz")
    o = H.options(g["options"])
    sigs = [H.row_sig(r) for r in g["signatures"]]
    idx = {id(s): i for i, s in enumerate(sigs)}
    clusters = svim_amd.cluster_sv_signatures(sigs, o)
    before = eng.fetch_clusters()
    out = svim_amd.combine_clusters(clusters, o)
    assert all(isinstance(c, ClusterList) and c._objs is None for c in clusters) and all(isinstance(c, CandidateList) and c._objs is None for c in out)
    exp = g["expected"]
    _expected_state(clusters, exp)
    got = [[CC.cand_row(c, idx) for c in lst] for lst in out]
    d = H.first_json_difference(got, exp["combine"])
    assert d is None, d
    st = CC.check_stages(eng, exp, sigs, clusters[0].references, idx)
    assert sorted(set(st["remove_1"].tolist()) | set(st["remove_2"].tolist())) and exp["n_ins_before"] - exp["n_ins_after"] == len(set(st["remove_1"].tolist()) | set(st["remove_2"].tolist()))
    # the resident cluster tables are only read
    assert before.first_difference(eng.fetch_clusters()) is None
    # the lists now hold what the reference leaves in them
    assert [c.type for c in clusters[4]][-len(exp["merged_insertion_from_clusters"]):] == ["DUP_INT"] * len(exp["merged_insertion_from_clusters"])
    assert len(list(clusters[5])) == exp["n_bnd_after_merge"] and len(list(clusters[1])) == exp["n_ins_after"]
    # a second combine of the same resident clusters: the same table
    t1 = svim_amd.combine_tables(eng, o, references=clusters[0].references)
    t2 = svim_amd.combine_tables(eng, o, references=clusters[0].references)
    assert t1.first_difference(t2) is None and t1.n == sum(len(x) for x in out)
    # the drop-in functions of SVIM_merging, served from the stage hook
    fresh = svim_amd.cluster_sv_signatures(sigs, o)
    b2, i2 = copy.copy(fresh[5]), copy.copy(fresh[1])
    new_from, to_remove = svim_amd.merge_translocations_at_insertions(b2, i2, o)
    assert to_remove == exp["inserted_regions_to_remove"] and len(b2) == exp["n_bnd_after_merge"]
    assert H.first_json_difference(CC.merged_rows(new_from, idx), exp["merged_insertion_from_clusters"]) is None
    flagged = svim_amd.flag_cutpaste_candidates(list(fresh[4]) + new_from, fresh[0], o)
    d = H.first_json_difference([CC.cand_row(c, idx) for c in flagged], exp["flag_cutpaste"])
    assert d is None, d


def test_golden_cases_from_cluster_lists(eng):
    """g_combine_cases.json.gz: hand-built cluster lists (plain lists -> source 2) against the reference's rows, intermediates and exceptions"""
    import svim_amd
    g = H.load("g_combine_cases.json.gz")
    for case in g["cases"]:
        o = types.SimpleNamespace(**case["options"])
        lists6, idx = CC.case_objects(case)
        exp = case["expected"]
        if "raises" in exp:
            with pytest.raises(IndexError):
                svim_amd.combine_clusters(lists6, o)
            _expected_state(lists6, exp)
            continue
        out = svim_amd.combine_clusters(lists6, o)
        got = [[CC.cand_row(c, idx) for c in lst] for lst in out]
        d = H.first_json_difference(got, exp["combine"])
        assert d is None, (case["name"], d)
        _expected_state(lists6, exp)
        sigs = [None] * len(idx)
        for lst in CC.case_objects(case)[0]:
            pass
        st = eng.combine_stages()
        assert st["remove_1"].tolist() == exp["inserted_regions_to_remove"], case["name"]
        assert st["merged"].n == len(exp["merged_insertion_from_clusters"]) and st["flagged"].n == len(exp["flag_cutpaste"]), case["name"]
        assert [bool(a & 1) for a in st["flagged"].aux.tolist()] == [r["cutpaste"] for r in exp["flag_cutpaste"]], case["name"]
        assert np.allclose(st["merged"].score, [r[6] for r in exp["merged_insertion_from_clusters"]], rtol=1e-12, atol=0), case["name"]


def _seeded_clusters(seed, n_del, n_ins, n_dup, n_tan, n_bnd_pairs):
    """a multi-contig cluster set: many deletions (stage 3 spans many tiles), interspersed duplications dense enough for sampled partitions (stage 5)"""
    rng = random.Random(seed)
    R = ["chr1", "chr2", "chr10", "chrX", "chr3_alt"]
    case = {"signatures_fully_covered": [], "clusters": [[] for _ in range(6)]}

    def mem(n, fc=False):
        k = len(case["signatures_fully_covered"])
        case["signatures_fully_covered"].extend([fc] * n)
        return list(range(k, k + n))

    def std():
        return rng.choice([None, rng.random() * 20])
    for _ in range(n_del):
        s = rng.randrange(0, 3000000)
        case["clusters"][0].append([rng.choice(R), s, s + rng.randrange(40, 4000), rng.choice([0.0, 3.0, 12.5]), std(), std(), mem(rng.randrange(1, 4))])
    ins = []
    for _ in range(n_ins):
        s = rng.randrange(0, 3000000)
        ins.append([rng.choice(R), s, s + rng.randrange(40, 900), rng.choice([0.0, 2.0, 9.5]), std(), std(), mem(rng.randrange(1, 4))])
    ins.sort(key=lambda r: (r[0], (r[1] + r[2]) // 2))
    case["clusters"][1] = ins
    for _ in range(n_tan):
        c, s, ln = rng.choice(R), rng.randrange(0, 3000000), rng.randrange(50, 800)
        case["clusters"][3].append([c, s, s + ln, c, s + ln, s + ln + rng.randrange(1, 6) * ln // 2, 8.0, std(), std(), mem(2, rng.random() < 0.5)])
    for k in range(n_dup):
        c = rng.choice(R[:2])
        s = rng.randrange(0, 40000) if k % 3 else rng.randrange(0, 3000000)
        ln = rng.randrange(100, 1200)
        d = rng.randrange(0, 3000000)
        case["clusters"][4].append([c, s, s + ln, rng.choice(R), d, d + ln, float(rng.randrange(1, 40)), std(), std(), mem(rng.randrange(1, 3))])
    for k in range(n_bnd_pairs):
        r = ins[rng.randrange(len(ins))]
        ln = r[2] - r[1]
        dc, d = rng.choice(R), rng.randrange(0, 3000000)
        j = rng.randrange(-30, 30)
        case["clusters"][5].append([r[0], r[1] + j, r[1] + j + 1, dc, d, d + 1, 5.0, std(), std(), mem(2), "fwd", "fwd"])
        case["clusters"][5].append([r[0], r[1] - j, r[1] - j + 1, dc, d + ln + rng.randrange(-3, 3), d + ln + 1, 5.0, std(), std(), mem(2), "rev", "rev"])
        case["clusters"][5].append([rng.choice(R), rng.randrange(0, 3000000), 7, rng.choice(R), rng.randrange(0, 3000000), 9, 4.0, std(), std(), mem(1),
                                    rng.choice(["fwd", "rev"]), rng.choice(["fwd", "rev"])])
    return case


def test_seeded_workload_three_routes_agree(eng):
    """resident route (clusters in the context) == source 2 (table handed in) == the Python replay of the reference's COMBINE"""
    import combine_consumer as cc
    import svim_amd
    from svim_amd import SVIM_COMBINE, _abi, batch
    o = types.SimpleNamespace(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
                              cluster_max_distance=0.5, skip_consensus=True)
    case = _seeded_clusters(7, n_del=6000, n_ins=1500, n_dup=700, n_tan=300, n_bnd_pairs=400)
    lists6, idx = CC.case_objects(case)
    ref_lists = [list(x) for x in lists6]
    want = cc.consume(ref_lists, o, idx)
    assert len(want["merged_insertion_from_clusters"]) > 20 and want["n_ins_before"] - want["n_ins_after"] > len(want["inserted_regions_to_remove"])
    out = svim_amd.combine_clusters(lists6, o)
    got = [[CC.cand_row(c, idx) for c in lst] for lst in out]
    for r in want["combine"]:
        for row in r:
            row.pop("type", None)
    for r in got:
        for row in r:
            row.pop("type", None)
    d = H.first_json_difference(got, want["combine"])
    assert d is None, d
    stats = eng.combine_stats()
    assert stats["n_dup_large_partitions"] >= 1 and stats["n_cutpaste_pairs"] > 256 * 8 * 100
    assert [len(x) for x in lists6] == [len(x) for x in ref_lists]
    # the same cluster table handed in as a table (source 2) and on device pointers nothing else: equal candidate tables
    ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(CC.case_objects(case)[0])
    cp = _abi.CombineParams.from_options(o)
    t2 = eng.combine(cp, batch.contig_ranks(names), table=ct, sig_aux=aux)
    t3 = eng.combine(cp, batch.contig_ranks(names), table=ct, sig_aux=aux)
    assert t2.first_difference(t3) is None and t2.n == sum(len(x) for x in out)


def test_resident_route_from_collect(eng):
    """COLLECT -> CLUSTER -> COMBINE with nothing fetched in between == the same clusters fetched and handed in as a table"""
    from svim_amd import _abi, batch, convert, records, synth
    contigs = [("chr1", 120000), ("chr2", 50000), ("chr10", 40000)]
    refs = synth.make_reference(3, contigs)
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.planted_reads(5, 600, refs, references, lengths, n_sites=40, types=("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND"))
    recs += synth.fuzz_split_reads(6, 200, references, lengths)
    bam = records.AlignmentFile(text=synth.sam_text(references, lengths, synth.coordinate_sort(recs)))
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                              position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False,
                              trans_sv_max_distance=500, del_ins_dup_max_distance=1.0)
    hb = batch.build_batch(bam, o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    off, codes = convert.genome_arrays(refs, references)
    eng.set_genome(off, codes)
    eng.collect(hb, p, fetch=False)
    eng.cluster(p, hb.contig_rank, source=0, fetch=False)
    try:
        resident = eng.combine(cp, hb.contig_rank)
    except Exception as e:                             # a workload without deletion clusters would say so; this one has them
        raise AssertionError(e)
    ct = eng.fetch_clusters()
    sig = eng.fetch_signatures(0)
    handed = eng.combine(cp, hb.contig_rank, table=ct, sig_aux=sig.aux[:sig.n])
    assert resident.n > 0 and resident.first_difference(handed) is None
    assert ct.first_difference(eng.fetch_clusters()) is None


def test_combine_without_cluster_is_a_state_error():
    from svim_amd import _abi, _lib
    e = _lib.Engine(0)
    try:
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.combine(_abi.CombineParams.from_options(types.SimpleNamespace()), np.zeros(1, np.int32))
    finally:
        e.close()


def test_file_again_under_alloc_guard():
    """every buffer of the stage in a mapping of its own with unmapped pages behind it: an overrun is a fault, not a silent read"""
    import os
    import subprocess
    import sys
    if os.environ.get("SVX_ALLOC_GUARD") == "1":
        pytest.skip("already the guarded run")
    env = dict(os.environ, SVX_ALLOC_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "golden or seeded or resident"], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True,
                       timeout=840)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
