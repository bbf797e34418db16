"""The BED / signature-VCF text on the device (svx_bed, svim_amd/csrc/bed.hip) against what the reference wrote (tests/golden/g_bed_cases.json.gz) and against the
Python definition of a line (svim_amd.signatures, svim_amd.candidates, the *_python writers) over materialised objects; repr(float) by the device build of
csrc/fmt_repr.hpp against CPython."""
import math
import os
import random
import types

import numpy as np
import pytest

import bed_cases as BC

pytestmark = pytest.mark.gpu
TILE = 1024


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


_FRESH = []


def _fresh_engine():
    from svim_amd import _lib
    if not _FRESH:
        _FRESH.append(_lib.Engine(0))
    return _FRESH[0]


def _files(eng):
    """the text of the engine's last bed() call, fetched in 50 000-byte pieces, with its offsets checked -> (list of bytes per file, whole text, line offsets)"""
    n_files, n_lines, n_bytes = eng.bed_count()
    text = b"".join(eng.bed_fetch(at, min(50_000, n_bytes - at)) for at in range(0, n_bytes, 50_000))
    off, first = eng.bed_file_offsets()
    lines = eng.bed_line_offsets()
    assert len(text) == n_bytes and len(off) == len(first) == n_files + 1 and off[0] == 0 and off[-1] == n_bytes and first[0] == 0 and first[-1] == n_lines
    assert len(lines) == n_lines + 1 and lines[0] == 0 and lines[-1] == n_bytes and bool(np.all(np.diff(lines) > 0))
    assert all(text[int(e) - 1:int(e)] == b"\n" for e in lines[1:]) and text.count(b"\n") == n_lines
    assert [int(lines[int(k)]) for k in first] == [int(x) for x in off]
    st = eng.bed_stats()
    assert st["n_lines"] == n_lines and st["n_bytes"] == n_bytes and st["lines_per_file"] == np.diff(first).tolist()
    return [text[int(off[k]):int(off[k + 1])] for k in range(n_files)], text, lines


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        w = w.encode("utf-8") if isinstance(w, str) else w
        d = BC.first_difference(g, w)
        assert d is None, "%s, file %d: %s" % (what, k, d)


def _three_products(eng, clusters, cands, want_route):
    """the three products of the lists through the routes of svim_amd.bed -> (7 files, 1 file, 8 files)"""
    from svim_amd import _abi, bed
    out = []
    for run in (lambda: bed.signature_text(_abi.BED_SIGNATURE_BEDS, clusters, engine=eng), lambda: bed.signature_text(_abi.BED_SIGNATURE_VCF, clusters, engine=eng),
                lambda: bed.candidate_text(cands, engine=eng)):
        done = run()
        assert (None if done is None else done[1]) == want_route
        out.append(None if done is None else _files(eng)[0])
    return out


def test_golden_cases_are_the_reference_bytes(eng):
    G = BC.load()
    sigs = BC.signatures(G)
    for case in G["cases"]:
        clusters, cands = BC.cluster_lists(G, case, sigs), BC.candidate_lists(G, case, sigs)
        beds, vcf, cbeds = _three_products(eng, clusters, cands, None if case["python_only"] else "table")
        if case["python_only"]:
            assert beds is None and vcf is None and cbeds is None
            continue
        _same(beds, case["sig_beds"], case["name"] + " signature beds")
        _same(vcf, [BC.vcf_body(G, case)], case["name"] + " all.vcf")
        _same(cbeds, case["cand_beds"], case["name"] + " candidate beds")


def _repr_sample(n, seed):
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, 2 ** 64, size=n * 6 // 10, dtype=np.uint64).view(np.float64)]
    for bound in (1e-5, 1e-4, 1e15, 1e16, 1e17, 1e21, 1e22, 1e23):
        parts.append(bound * rng.uniform(0.05, 20.0, size=n // 40))
    pw = [math.ldexp(1.0, e) for e in range(-1074, 1024)] + [float("1e%d" % e) for e in range(-323, 309)]
    parts.append(np.asarray([v for p in pw for v in (p, math.nextafter(p, math.inf), math.nextafter(p, 0.0))]))
    parts.append(np.asarray([5e-324, 1.7976931348623157e308, 0.0, -0.0, float("inf"), -float("inf"), float("nan"), 2.2250738585072014e-308, 9999999999999998.0, 1e16]))
    parts.append(np.arange(50_000) / 100.0)
    parts.append(np.arange(50_000) / 8.0)
    parts.append(rng.uniform(0, 1, size=20_000) * 5e-310)                     # subnormals
    x = np.concatenate(parts)
    rest = n - x.size
    assert rest > 0
    return np.concatenate([x, rng.normal(0, 1000, size=rest)])


def test_device_repr_equals_cpython_repr(eng):
    x = _repr_sample(1_000_000, 99)
    assert x.size == 1_000_000
    got = eng.format_repr(x)
    want = [repr(v) for v in x.tolist()]
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, "%d of %d differ, first: repr %s, device %s" % (len(bad), len(want), bad[0][0], bad[0][1])
    from svim_amd import _lib
    assert _lib.format_repr_many(x[:100_000]) == got[:100_000]                # the host build of the same header


def _options():
    return types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                                 position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False,
                                 trans_sv_max_distance=500, del_ins_dup_max_distance=1.0)


def _seeded(n_reads=900, n_sites=60, n_fuzz=300):
    from svim_amd import synth
    contigs = [("chr1", 120000), ("chr2", 50000), ("chr10", 40000)]
    refs = synth.make_reference(3, contigs)
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.planted_reads(5, n_reads, refs, references, lengths, n_sites=n_sites, types=("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND"))
    recs += synth.fuzz_split_reads(6, n_fuzz, references, lengths)
    return refs, references, lengths, synth.coordinate_sort(recs)


def test_seeded_pipeline_three_routes_agree(eng):
    """COLLECT -> CLUSTER -> COMBINE resident: source 0 == the Python definition over the materialised objects == source 2 built from those objects"""
    from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, _abi, batch, bed, convert, lazy, records, synth
    refs, references, lengths, recs = _seeded()
    bam = records.AlignmentFile(text=synth.sam_text(references, lengths, recs))
    o = _options()
    hb = batch.build_batch(bam, o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    eng.set_genome(*convert.genome_arrays(refs, references))
    sig, _ = eng.collect(hb, p)
    ct = eng.cluster(p, hb.contig_rank, source=0)
    sigs = lazy.SignatureList(sig, references, hb.read_names, origin=(eng, eng.collect_generation, 0))
    assert ct.n > 20 and sum(1 for c in ct.type_count if c) >= 4
    # clusters
    for product, python in ((_abi.BED_SIGNATURE_BEDS, SVIM_CLUSTER.signature_bed_texts_python), (_abi.BED_SIGNATURE_VCF, lambda c: [SVIM_CLUSTER.signature_vcf_body_python(c)])):
        views = convert.cluster_objects(ct, sigs, references)
        done = bed.signature_text(product, views, engine=eng)
        assert done[1] == "resident" and all(x.untouched() for x in views) and sigs._objs is None
        resident = _files(eng)[0]
        objs = tuple(list(x) for x in convert.cluster_objects(ct, sigs, references))
        want = python(objs)
        _same(resident, want, "resident, product %d" % product)
        done = bed.signature_text(product, objs, engine=eng)
        assert done[1] == "table"
        _same(_files(eng)[0], want, "table, product %d" % product)
        sigs2 = lazy.SignatureList(sig, references, hb.read_names)              # the same table, not known to be the engine's: its columns are uploaded
        done = bed.signature_text(product, convert.cluster_objects(ct, sigs2, references), engine=eng)
        assert done[1] == "table" and sigs2._objs is None
        _same(_files(eng)[0], want, "table of views, product %d" % product)
    st = eng.bed_stats()
    assert st["t_total_ms"] > 0 and st["n_files"] == 1
    # candidates
    table = eng.combine(cp, hb.contig_rank)
    assert table.n > 20 and len(set(table.cls.tolist())) >= 4

    def views():
        d, i, di, t, n, b = convert.candidate_lists(table, sigs, references)
        return (di, i, t, d, n, b)
    v = views()
    done = bed.candidate_text(v, engine=eng)
    assert done[1] == "resident" and all(x._objs is None for x in v)
    resident = _files(eng)[0]
    objs = tuple(list(x) for x in views())
    want = SVIM_COMBINE.candidate_bed_texts_python(objs)
    _same(resident, want, "resident candidates")
    assert bed.candidate_text(objs, engine=eng)[1] == "table"
    _same(_files(eng)[0], want, "table candidates")
    st = eng.bed_stats()
    assert st["n_files"] == 8 and st["bytes_members"] > 0 and st["n_tiles"] > 0


def _del_sig(name, contig="c"):
    from svim_amd import signatures as S
    return S.SignatureDeletion(contig, 1, 2, "cigar", name)


def _members_of_length(total):
    """DEL signatures on contig `c` whose pieces '[c|1|2|DEL;cigar|NAME]' (18 bytes + the name) add up to `total` bytes; names of 250 bytes and one of length 1"""
    out = [_del_sig("n" * 250) for _ in range((total - 19 - 40) // 268)]
    rest = total - 268 * len(out) - 19
    out.append(_del_sig("r"))
    assert rest >= 19
    out.append(_del_sig("m" * (rest - 18)))
    assert sum(len(m.as_string("|")) + 2 for m in out) == total
    return out


def test_member_payloads_at_every_alignment_and_tile_edge(eng):
    from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, candidates as K, signatures as S
    clusters, dele, tan = [], [], []
    for total in (TILE - 17, TILE - 16, TILE - 15, TILE - 1, TILE, TILE + 1, TILE + 15, TILE + 16, TILE + 17, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 5 * TILE + 7):
        for k in range(16):
            contig = "c" + "x" * k
            m = _members_of_length(total)
            clusters.append(S.SignatureClusterUniLocal(contig, 5, 50, 1.5, len(m), m, "DEL", None, 2.5))
            dele.append(K.CandidateDeletion(contig, 5, 50, m, 1.5, None, 2.5))
            tan.append(K.CandidateDuplicationTandem(contig, 5, 50, 2, True, m, 1.5, None, 2.5))
    lists6 = (clusters, [], [], [], [], [])
    beds, vcf, cbeds = _three_products(eng, lists6, ([], [], tan, dele, [], []), "table")
    _same(beds, SVIM_CLUSTER.signature_bed_texts_python(lists6), "tile edges, clusters")
    _same(cbeds, SVIM_COMBINE.candidate_bed_texts_python(([], [], tan, dele, [], [])), "tile edges, candidates")
    _same(vcf, [SVIM_CLUSTER.signature_vcf_body_python(lists6)], "tile edges, all.vcf")
    starts = set()
    for files in (beds, cbeds):
        at = 0
        for f in files:
            for line in f.split(b"\n")[:-1]:
                starts.add((at + line.rindex(b"\t[") + 1) % 16)
                at += len(line) + 1
    assert starts == set(range(16))


def test_cluster_and_candidate_with_5000_members(eng):
    from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, candidates as K, signatures as S
    rng = random.Random(21)
    names = ["m%d/%d/%d_%d" % (rng.randrange(3), rng.randrange(400), k, k + 9) for k in range(1700)] + ["q" * 250, "z"]
    contigs = ["chr1", "chr10", "chr2"]
    pool = []
    for k in range(3000):
        c, c2, r = rng.choice(contigs), rng.choice(contigs), rng.choice(names)
        a = rng.randrange(0, 2_000_000_000)
        b = a + rng.randrange(0, 100_000)
        src = rng.choice(("cigar", "suppl"))
        pool.append([S.SignatureDeletion(c, a, b, src, r), S.SignatureInsertion(c, a, b, src, r, "ACGT"), S.SignatureInversion(c, a, b, src, r, rng.choice(("left_fwd", "left_rev", "right_fwd", "right_rev", "all"))),
                     S.SignatureInsertionFrom(c, a, b, c2, rng.randrange(0, 10 ** 9), src, r), S.SignatureDuplicationTandem(c, a, b, rng.randrange(0, 30), bool(k & 1), src, r),
                     S.SignatureTranslocation(c, a, rng.choice(("fwd", "rev")), c2, rng.randrange(0, 10 ** 9), rng.choice(("fwd", "rev")), src, r)][k % 6])
    big = [rng.choice(pool) for _ in range(5000)]
    clusters = ([S.SignatureClusterUniLocal("chr1", 500, 560, 80.0, 5000, big, "DEL", 3.5, 4.25), S.SignatureClusterUniLocal("chr2", 5, 9, 1.125, 1, pool[:1], "DEL", None, None)], [], [],
                [S.SignatureClusterBiLocal("chr2", 100, 200, "chr2", 200, 300, 17.5, 2500, big[:2500], "DUP_TAN", 0.5, None)],
                [S.SignatureClusterBiLocal("chr2", 100, 200, "chr10", 200, 300, 17.5, 5000, big, "DUP_INT", 0.5, 1e-7)], [])
    cands = ([K.CandidateDuplicationInterspersed("chr1", 5, 105, "chr2", 100, 200, big, 6.5, None, 0.0, True)], [], [],
             [K.CandidateDeletion("chr2", 40, 90, big[:2500], 8.0, 0.5, 0.25), K.CandidateDeletion("chr2", 40, 90, pool[7:8], 8.0, 0.5, 0.25)], [],
             [K.CandidateBreakend("chr1", 10 * k, "fwd", "chr2", 7 * k, "rev", pool[k:k + 1 + k % 40], 9.0, 1.0, None) for k in range(250)])
    beds, vcf, cbeds = _three_products(eng, clusters, cands, "table")
    _same(beds, SVIM_CLUSTER.signature_bed_texts_python(clusters), "5000 members, clusters")
    _same(vcf, [SVIM_CLUSTER.signature_vcf_body_python(clusters)], "5000 members, all.vcf")
    _same(cbeds, SVIM_COMBINE.candidate_bed_texts_python(cands), "5000 members, candidates")
    again = _three_products(eng, clusters, cands, "table")
    assert again[0] == beds and again[2] == cbeds                         # two calls give the same bytes
    small = ([], [], [], [], [], cands[5][:1])
    _, _, text = _three_products(eng, ([], [], [], [], [], []), small, "table")      # a smaller call afterwards does not show the first one's tail
    _same(text, SVIM_COMBINE.candidate_bed_texts_python(small), "small call")
    assert eng.bed_count() == (8, 2, sum(len(t) for t in text))
    with pytest.raises(Exception):
        eng.bed_fetch(0, sum(len(t) for t in text) + 1)


def test_state_and_argument_errors_leave_the_context_usable():
    from svim_amd import _abi, _lib, batch, bed, convert, records, synth
    e = _fresh_engine()
    for product in (_abi.BED_SIGNATURE_BEDS, _abi.BED_SIGNATURE_VCF, _abi.BED_CANDIDATE_BEDS):
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.bed(product, ["chr1"], read_names=["r"])
    G = BC.load()
    sigs = BC.signatures(G)
    case = G["cases"][0]
    clusters, cands = BC.cluster_lists(G, case, sigs), BC.candidate_lists(G, case, sigs)
    ct, names, st, reads = bed.cluster_table_from_lists(clusters)
    good = e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads)
    want = _files(e)[0]
    with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):                  # a read id outside the name table
        e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads[:-3])
    with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):                  # a contig id outside the names
        e.bed(_abi.BED_SIGNATURE_BEDS, names[:1], table=ct, sigs=st, read_names=reads)
    for line in (1, 2, good[1]):                                           # a line counted one byte short: the skeleton refuses to leave it
        with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
            e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads, debug_short_line=line)
    with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
        e.bed_count()
    assert e.bed(_abi.BED_SIGNATURE_BEDS, names, table=ct, sigs=st, read_names=reads) == good and _files(e)[0] == want
    # product 2 of resident candidates after a later cluster(): gone
    refs, references, lengths, recs = _seeded(300, 20, 60)
    o = _options()
    hb = batch.build_batch(records.AlignmentFile(text=synth.sam_text(references, lengths, recs)), o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    e.set_genome(*convert.genome_arrays(refs, references))
    e.collect(hb, p)
    e.cluster(p, hb.contig_rank, source=0, fetch=False)
    e.combine(cp, hb.contig_rank, fetch=False)
    n_files, n_lines, _ = e.bed(_abi.BED_CANDIDATE_BEDS, references, read_names=hb.read_names)
    assert n_files == 8 and n_lines > 0
    e.cluster(p, hb.contig_rank, source=0, fetch=False)
    with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
        e.bed(_abi.BED_CANDIDATE_BEDS, references, read_names=hb.read_names)
    assert e.bed(_abi.BED_SIGNATURE_BEDS, references, read_names=hb.read_names)[0] == 7
    assert e.bed(_abi.BED_SIGNATURE_VCF, references)[0] == 1


def test_bam_pipeline_writes_the_sixteen_files(eng, tmp_path):
    from svim_amd import SVIM_CLUSTER, SVIM_COMBINE, convert, harness, lazy, records
    refs, references, lengths, recs = _seeded(400, 25, 60)
    o = _options()
    path = str(tmp_path / "small.bam")
    records.write_bam(path, references, lengths, recs)
    eng.set_genome(*convert.genome_arrays(refs, references))
    pipe = harness.BamPipeline(path, o, eng, threads=2, batch_records=97, device_decode=True)
    try:
        assert pipe.run() > 0
        pipe.cluster()
        dev, py = str(tmp_path / "device"), str(tmp_path / "python")
        os.makedirs(dev), os.makedirs(py)
        assert pipe.write_signature_files(dev, "2.0.0") > 0
        ct = eng.fetch_clusters()
        pipe.combine()
        assert pipe.write_candidate_files(dev) > 0
        table = eng.fetch_candidates()
        sigs = lazy.SignatureList(eng.fetch_signatures(0), references, pipe.bam.read_names())
    finally:
        pipe.close()
    clusters = tuple(list(x) for x in convert.cluster_objects(ct, sigs, references))
    d, i, di, t, n, b = (list(x) for x in convert.candidate_lists(table, sigs, references))
    assert sum(len(x) for x in clusters) > 10 and len(d) + len(i) + len(di) + len(t) + len(n) + len(b) > 10
    SVIM_CLUSTER.write_signature_clusters_bed_python(py, clusters)
    SVIM_CLUSTER.write_signature_clusters_vcf_python(py, clusters, "2.0.0")
    SVIM_COMBINE.write_candidates_python(py, (di, i, t, d, n, b))
    files = sorted(os.path.join(sub, f) for sub in ("signatures", "candidates") for f in os.listdir(os.path.join(py, sub)))
    assert len(files) == 16 and files == sorted(os.path.join(sub, f) for sub in ("signatures", "candidates") for f in os.listdir(os.path.join(dev, sub)))
    some = 0
    for f in files:
        with open(os.path.join(dev, f), "rb") as a, open(os.path.join(py, f), "rb") as b_:
            got, want = a.read(), b_.read()
        assert BC.first_difference(got, want) is None, (f, BC.first_difference(got, want))
        some += 1 if got else 0
    assert some >= 8
