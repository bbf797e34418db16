"""The VCF text on the device (svx_vcf, svim_amd/csrc/vcf.hip) against what the reference wrote (tests/golden/g_vcf_cases.json.gz) and against the Python
definition of a line (svim_amd.candidates, SVIM_COMBINE.vcf_body_python) over materialised objects."""
import os
import random
import types

import numpy as np
import pytest

import vcf_cases as VC

pytestmark = pytest.mark.gpu
TILE = 1024


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


def _text(lines):
    return "".join(l + "\n" for l in lines).encode("utf-8")


def _device_text(eng, lists6, contig_names, types_to_output, o, sequence_alleles):
    """svx_vcf through SVIM_COMBINE.vcf_body_device -> (bytes, line offsets, route taken)"""
    from svim_amd import SVIM_COMBINE
    route = "resident" if SVIM_COMBINE._resident_candidates(lists6, eng) else "table"
    done = SVIM_COMBINE.vcf_body_device(*lists6, contig_names, types_to_output, o, sequence_alleles, engine=eng)
    assert done is not None
    _, n_lines, n_bytes = done
    text = b"".join(eng.vcf_fetch(at, min(50_000, n_bytes - at)) for at in range(0, n_bytes, 50_000))      # in pieces, as the drop-in fetches it
    off = eng.vcf_line_offsets()
    assert len(off) == n_lines + 1 and off[0] == 0 and off[-1] == n_bytes == len(text)
    assert all(text[int(e) - 1:int(e)] == b"\n" for e in off[1:]) and text.count(b"\n") == n_lines
    return text, off, route


def _check(eng, lists6, contig_names, types_to_output, o, sequence_alleles, reference):
    from svim_amd import SVIM_COMBINE
    want = _text(SVIM_COMBINE.vcf_body_python(*[list(x) for x in lists6], types_to_output, o, sequence_alleles, reference))
    got, off, _ = _device_text(eng, lists6, contig_names, types_to_output, o, sequence_alleles)
    if got != want:
        gl, wl = got.split(b"\n"), want.split(b"\n")
        for k, (a, b) in enumerate(zip(gl, wl)):
            if a != b:
                j = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                raise AssertionError("line %d differs at byte %d: %r != %r" % (k, j, a[max(0, j - 40):j + 40], b[max(0, j - 40):j + 40]))
        raise AssertionError("%d lines != %d lines" % (len(gl), len(wl)))
    return got, off


def test_golden_cases_are_the_reference_bytes(eng, tmp_path):
    G = VC.load()
    fasta = VC.write_fasta(str(tmp_path / "genome.fa"), {c: G["genome"][c] for c in G["contigs"]})
    for case in G["cases"]:
        o = VC.options(case, genome=fasta)
        objs = VC.objects(VC.case_rows(G, case), G["sigs"])
        got, _, route = _device_text(eng, VC.lists6(objs), G["contigs"], case["types"], o, not o.symbolic_alleles)
        assert route == "table"
        assert got == _text(case["body"]), case["name"]
    st = eng.vcf_stats()
    assert st["n_lines"] == 0 and st["n_bytes"] == 0              # the last case is the empty call


def _options(**kw):
    d = dict(symbolic_alleles=True, tandem_duplications_as_insertions=False, interspersed_duplications_as_insertions=False, insertion_sequences=False,
             read_names=False, zmws=False, sample="Sample", genome=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_seeded_pipeline_three_routes_agree(eng, tmp_path):
    """COLLECT -> CLUSTER -> COMBINE resident: source 0 == the Python definition over the materialised objects == source 2 built from those objects"""
    from svim_amd import SVIM_COMBINE, _abi, batch, convert, lazy, records, synth
    contigs = [("chr1", 120000), ("chr2", 50000), ("chr10", 40000)]
    refs = synth.make_reference(3, contigs)
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    recs = synth.planted_reads(5, 900, refs, references, lengths, n_sites=60, types=("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND"))
    recs += synth.fuzz_split_reads(6, 300, references, lengths)
    bam = records.AlignmentFile(text=synth.sam_text(references, lengths, synth.coordinate_sort(recs)))
    o = types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5, partition_max_distance=1000,
                              position_distance_normalizer=900, edit_distance_normalizer=1.0, cluster_max_distance=0.5, all_bnds=False,
                              trans_sv_max_distance=500, del_ins_dup_max_distance=1.0)
    hb = batch.build_batch(bam, o, mode="coordinate")
    p, cp = _abi.Params.from_options(o), _abi.CombineParams.from_options(o)
    eng.set_genome(*convert.genome_arrays(refs, references))
    sig, _ = eng.collect(hb, p)
    eng.cluster(p, hb.contig_rank, source=0, fetch=False)
    table = eng.combine(cp, hb.contig_rank)
    assert table.n > 20 and len(set(table.cls.tolist())) >= 4
    fasta = VC.write_fasta(str(tmp_path / "genome.fa"), refs)
    reference = SVIM_COMBINE.GenomeText(refs)
    sigs = lazy.SignatureList(sig, references, hb.read_names)

    def views():
        d, i, di, t, n, b = convert.candidate_lists(table, sigs, references)
        return (di, i, t, d, n, b)
    rng = random.Random(4)
    for sw in (dict(), dict(symbolic_alleles=False), dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True),
               dict(insertion_sequences=True, read_names=True, zmws=True),
               dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, insertion_sequences=True, read_names=True, zmws=True)):
        ov = _options(genome=fasta, **sw)
        seq = not ov.symbolic_alleles
        lists6 = views()
        assert SVIM_COMBINE._resident_candidates(lists6, eng)
        resident, off, route = _device_text(eng, lists6, references, VC.ALL_TYPES, ov, seq)
        assert route == "resident" and all(x._objs is None for x in lists6)
        objs = tuple(list(x) for x in views())
        want = _text(SVIM_COMBINE.vcf_body_python(*objs, VC.ALL_TYPES, ov, seq, reference))
        assert resident == want
        handed, _, route = _device_text(eng, objs, references, VC.ALL_TYPES, ov, seq)
        assert route == "table" and handed == want
        # random genotype columns: only objects can carry them
        for lst in objs:
            for c in lst:
                c.genotype = rng.choice(["./.", "0/0", "0/1", "1/1"])
                c.ref_reads, c.alt_reads = rng.choice([None, rng.randrange(60)]), rng.choice([None, rng.randrange(60)])
        _check(eng, objs, references, rng.sample(VC.ALL_TYPES, 4), ov, seq, reference)
    st = eng.vcf_stats()
    assert st["n_lines"] > 0 and st["bytes_seqs"] > 0 and st["bytes_reads"] > 0 and st["t_total_ms"] > 0


def test_drop_in_writes_the_file_on_both_routes(eng, tmp_path):
    import svim_amd
    from svim_amd import SVIM_COMBINE
    G = VC.load()
    fasta = VC.write_fasta(str(tmp_path / "genome.fa"), {c: G["genome"][c] for c in G["contigs"]})
    case = [c for c in G["cases"] if c["name"] == "all_010_111"][0]
    lengths = [len(G["genome"][c]) for c in G["contigs"]]
    for sub in ("table", "python"):
        d = tmp_path / sub
        d.mkdir()
        o = VC.options(case, genome=fasta, working_dir=str(d))
        objs = VC.objects(G["rows"], G["sigs"])
        if sub == "python":
            objs["INS"][0].sequence = "ACGTTT"             # a consensus sequence: the Python definition writes this call
        SVIM_COMBINE.write_final_vcf(*VC.lists6(objs), "2.0.0", G["contigs"], lengths, case["types"], o, engine=eng)
        lines = open(str(d / "variants.vcf")).read().split("\n")
        assert lines[-1] == "" and [l for l in lines if l.startswith("#") and not l.startswith("##fileDate=")] == case["header"]
        body = [l for l in lines[:-1] if not l.startswith("#")]
        if sub == "table":
            assert body == case["body"]
        else:
            assert len(body) == len(case["body"]) and len(set(body) ^ set(case["body"])) == 2
    assert svim_amd.SVIM_COMBINE.write_final_vcf is SVIM_COMBINE.write_final_vcf


def _directed_genome(n_contig, length, seed):
    rng = random.Random(seed)
    letters = "ACMGRSVTWYHKDBN"
    base = "".join(rng.choice("ACGT") for _ in range(length + 40))
    g = {}
    for k in range(n_contig):
        s = base[k:k + length]
        g["c" + "x" * k] = (letters + s[len(letters):]) if length >= len(letters) else s
    return g


@pytest.mark.parametrize("length", [0, 1, TILE - 1, TILE, TILE + 1, 100000])
def test_payload_lengths_at_every_destination_alignment(eng, tmp_path, length):
    """forward, reverse-complemented and repeated reference ranges of one length at every alignment of the destination (the contig names grow by one byte)"""
    from svim_amd import SVIM_COMBINE, candidates as K
    n = 24
    genome = _directed_genome(n, max(1, length) + 3, 9)
    names = list(genome)
    fasta = VC.write_fasta(str(tmp_path / "genome.fa"), genome)
    m = [VC.Sig("r1", ""), VC.Sig("r2", "")]
    dele = [K.CandidateDeletion(c, 1, 1 + length, m, 5.0, 1.5, None) for c in names] if length else [K.CandidateDeletion(c, 0, 0, m, 5.0, 1.5, None) for c in names]
    inv = [K.CandidateInversion(c, 2, 2 + length, m, 5.0, None, 2.25) for c in names]
    tan = [K.CandidateDuplicationTandem(c, 1, 1 + length, 2 if length > 5000 else 7, True, m, 5.0, None, None) for c in names]
    dint = [K.CandidateDuplicationInterspersed(names[k], 0, length, names[-1 - k], 1, 1 + length, m, 5.0, None, None) for k in range(n)]
    o = _options(symbolic_alleles=False, genome=fasta, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True)
    got, off = _check(eng, (dint, inv, tan, dele, [], []), names, VC.ALL_TYPES, o, True, SVIM_COMBINE.GenomeText(genome))
    if length:
        starts = set()
        for a, line in zip(off[:-1].tolist(), got.split(b"\n")):
            f = line.split(b"\t")
            starts.add((a + sum(len(x) + 1 for x in f[:3])) % 16)
        assert starts == set(range(16))
        st = eng.vcf_stats()
        assert st["bytes_ref_forward"] > 0 and st["bytes_ref_revcomp"] == n * length and st["bytes_ref_repeat"] > 0


def test_inversion_over_every_letter_and_clipped_ranges(eng, tmp_path):
    from svim_amd import SVIM_COMBINE, candidates as K
    genome = {"chrA": "ACMGRSVTWYHKDBN" * 5 + "acgtn" * 4, "chrB": "GATTACA" * 30}
    names = ["chrA", "chrB", "ghost"]                        # the genome lacks `ghost`: its ranges read as empty
    fasta = VC.write_fasta(str(tmp_path / "genome.fa"), genome)
    m = [VC.Sig("r1", "")]
    la, lb = len(genome["chrA"]), len(genome["chrB"])
    inv = [K.CandidateInversion("chrA", 0, la, m, 1.0, None, None), K.CandidateInversion("chrA", la - 7, la + 50, m, 1.0, None, None),
           K.CandidateInversion("chrB", lb + 5, lb + 90, m, 1.0, None, None), K.CandidateInversion("ghost", 10, 90, m, 1.0, None, None)]
    dele = [K.CandidateDeletion("chrB", lb - 3, lb + 40, m, 1.0, None, None), K.CandidateDeletion("chrB", lb + 1, lb + 40, m, 1.0, None, None),
            K.CandidateDeletion("ghost", 5, 50, m, 1.0, None, None), K.CandidateDeletion("chrA", 0, 10, m, 1.0, None, None)]
    dint = [K.CandidateDuplicationInterspersed("chrA", 3, 30, "chrB", lb + 9, lb + 36, m, 1.0, None, None), K.CandidateDuplicationInterspersed("ghost", 3, 30, "chrA", 0, 27, m, 1.0, None, None),
            K.CandidateDuplicationInterspersed("chrB", lb - 2, lb + 30, "ghost", 4, 36, m, 1.0, None, None, True)]
    tan = [K.CandidateDuplicationTandem("chrB", lb - 5, lb + 5, 3, False, m, 1.0, None, None), K.CandidateDuplicationTandem("chrA", 0, 16, -1, True, m, 1.0, None, None),
           K.CandidateDuplicationTandem("chrA", 0, 16, -4, True, m, 1.0, None, None)]
    o = _options(symbolic_alleles=False, genome=fasta, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=True)
    got, _ = _check(eng, (dint, inv, tan, dele, [], []), names, VC.ALL_TYPES, o, True, SVIM_COMBINE.GenomeText(genome))
    assert b"NVHDMRWASBYCKGT"[::-1] not in got and b"ACMGRSVTWYHKDBN" in got


def test_candidate_with_5000_members(eng):
    from svim_amd import SVIM_COMBINE, candidates as K
    rng = random.Random(21)
    names = ["m%d/%d/%d_%d" % (rng.randrange(3), rng.randrange(400), k, k + 9) for k in range(1700)] + ["plain%d" % k for k in range(40)]
    big = [VC.Sig(rng.choice(names[:1700]), "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 41)))) for _ in range(5000)]
    other = [VC.Sig(rng.choice(names), "".join(rng.choice("ACGTN") for _ in range(rng.randrange(0, 9)))) for _ in range(300)]
    ins = [K.CandidateNovelInsertion("chr1", 500, 560, "", big, 50.0, 3.5, 4.25), K.CandidateNovelInsertion("chr1", 100, 140, "", other[:7], 5.0, None, 1.0),
           K.CandidateNovelInsertion("chr2", 100, 140, "", [other[9]], 5.0, None, 1.0), K.CandidateNovelInsertion("chr2", 10, 14, "", [VC.Sig("e", ""), VC.Sig("f", "")], 5.0, None, 1.0)]
    bnd = [K.CandidateBreakend("chr1", 10 * k, "fwd", "chr2", 7 * k, "rev", other[k:k + 1 + k % 40], 9.0, 1.0, None) for k in range(250)]
    dele = [K.CandidateDeletion("chr2", 40, 90, big[:2500], 8.0, 0.5, 0.25)]
    o = _options(insertion_sequences=True, read_names=True, zmws=True)
    got, _ = _check(eng, ([], [], [], dele, ins, bnd), ["chr1", "chr2"], VC.ALL_TYPES, o, False, None)
    assert b";ZMWS=" in got and len(got.split(b"\n")[0]) > 0
    again, _, _ = _device_text(eng, ([], [], [], dele, ins, bnd), ["chr1", "chr2"], VC.ALL_TYPES, o, False)
    assert again == got                                       # two calls give the same bytes
    small = ([], [], [], [], ins[2:3], [])
    text, _ = _check(eng, small, ["chr1", "chr2"], VC.ALL_TYPES, o, False, None)      # a smaller call afterwards does not show the first one's tail
    assert len(text) < 400 and eng.vcf_count() == (1, len(text))
    with pytest.raises(Exception):
        eng.vcf_fetch(0, len(text) + 1)


def test_errors_are_said_not_printed(eng):
    from svim_amd import _abi, _lib, SVIM_COMBINE, candidates as K
    m = [VC.Sig("r1", "")]
    o = _options()
    with pytest.raises(_lib.SvxError, match="SVX_E_ARG"):
        SVIM_COMBINE.vcf_body_device([], [], [], [K.CandidateDeletion("chr1", 5, 50, m, 1.0, 1e10, None)], [], [], ["chr1"], VC.ALL_TYPES, o, False, engine=eng)
    with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
        SVIM_COMBINE.vcf_body_device([], [], [], [K.CandidateDeletion("chr1", 5, 50, m, 1.0, None, None)], [], [], ["chr1"], VC.ALL_TYPES, _options(symbolic_alleles=False),
                                     True, engine=_fresh_engine())
    with pytest.raises(_lib.SvxError, match="SVX_E_STATE"):
        _fresh_engine().vcf(_abi.VcfParams.from_options(o), ["chr1"])


_FRESH = []


def _fresh_engine():
    from svim_amd import _lib
    if not _FRESH:
        _FRESH.append(_lib.Engine(0))
    return _FRESH[0]
