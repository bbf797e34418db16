#!/usr/bin/env python3
"""Generate tests/golden/g_bed_cases.json.gz by RUNNING THE REFERENCE's three BED / signature-VCF writers on hand-built objects.

Build container only (needs the reference checkout make_golden.py reads; this module imports make_golden for its stubs).  The member signatures are the
reference's real Signature* objects of all six classes - the text of a member depends on ITS class, not on the line's - and the golden stores their
constructor arguments.  Every case is cluster rows and candidate rows (constructor arguments with the members slot holding signature indices) and what the
reference made of them: the seven files of write_signature_clusters_bed, the file of write_signature_clusters_vcf, the eight files of write_candidates, and
every get_bed_entry / get_bed_entries / get_vcf_entry / as_string string.  Cases marked python_only hold something a table cannot say (an int score).
DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bed.py
"""
import gzip
import itertools
import json
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG    # noqa: E402  (stubs pysam / edlib, puts the reference on the path)

for _name in ("spoa", "cpuinfo"):
    _stub = types.ModuleType(_name)
    _stub.poa = _stub.get_cpu_info = None
    sys.modules.setdefault(_name, _stub)
from svim import SVIM_CLUSTER, SVIM_COMBINE, SVCandidate, SVSignature    # noqa: E402
from svim.SVIM_clustering import calculate_score                         # noqa: E402

SIG_CLASSES = {"DEL": SVSignature.SignatureDeletion, "INS": SVSignature.SignatureInsertion, "INV": SVSignature.SignatureInversion,
               "DUP_INT": SVSignature.SignatureInsertionFrom, "DUP_TAN": SVSignature.SignatureDuplicationTandem, "BND": SVSignature.SignatureTranslocation}
CAND_CLASSES = {"DEL": SVCandidate.CandidateDeletion, "INV": SVCandidate.CandidateInversion, "INS": SVCandidate.CandidateNovelInsertion,
                "DUP_TAN": SVCandidate.CandidateDuplicationTandem, "DUP_INT": SVCandidate.CandidateDuplicationInterspersed, "BND": SVCandidate.CandidateBreakend}
CLUSTER_SLOTS = ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")            # cluster_sv_signatures' tuple order
CANDIDATE_SLOTS = ("DUP_INT", "INV", "DUP_TAN", "DEL", "INS", "BND")          # write_candidates' tuple order
CAND_MEMBER_SLOT = {"DEL": 3, "INV": 3, "INS": 4, "DUP_TAN": 5, "DUP_INT": 6, "BND": 6}
CONTIGS = ["chr1", "chr10", "chr2", "chr01"]
READS = ["r", "m1/100/0_500", "m1/100/600_900", "readA", "plain_read_8", "q" * 250, "m2/7/ccs", "a/b/c/d", "x1", "read-with-dash.2"]
INV_DIRECTIONS = ["left_fwd", "left_rev", "right_fwd", "right_rev", "all"]
# None, 0.0, and values whose repr has 1, 2, 16 and 17 significant digits (and some in between, an exponent form, a value rounding at the second digit)
STD = [None, 0.0, 0.5, 0.25, 7.0, 12.0, 0.1 + 0.2, 2.0 / 3.0, 1.0 / 3.0, 2.675, 0.005, 123456.785, 1e-05, 5.551115123125783e-17, 1234567.8901234567, 99.995,
       0.7071067811865476, 1e16 / 3.0]


def make_sigs():
    rng = random.Random(21)
    sigs = []
    src = itertools.cycle(["cigar", "suppl", "suppl", "cigar", "cigar"])
    rd = itertools.cycle(READS)
    for contig in CONTIGS:
        sigs.append(["DEL", [contig, 100, 200, next(src), next(rd)]])
        sigs.append(["DEL", [contig, rng.randrange(0, 10 ** 9), 2 * 10 ** 9, next(src), next(rd)]])
        sigs.append(["INS", [contig, 100, 200, next(src), next(rd), "ACGT" * rng.randrange(0, 4)]])
        sigs.append(["INS", [contig, 0, 7, next(src), next(rd), ""]])
    for k, d in enumerate(INV_DIRECTIONS):
        sigs.append(["INV", [CONTIGS[k % 4], 100 + k, 200 + 10 * k, next(src), next(rd), d]])
    for k in range(5):
        sigs.append(["DUP_INT", [CONTIGS[k % 4], 1000 * k, 1000 * k + 350, CONTIGS[(k + 1) % 4], 99 + k, next(src), next(rd)]])
    for k, copies in enumerate((0, 1, 2, 17, 3)):
        sigs.append(["DUP_TAN", [CONTIGS[k % 4], 5000 + k, 5400 + 3 * k, copies, bool(k % 2), next(src), next(rd)]])
    sigs.append(["DUP_TAN", ["chr2", 1500000000, 2000000000, 3, True, "suppl", "far"]])
    for k, (d1, d2) in enumerate(itertools.product(("fwd", "rev"), repeat=2)):
        sigs.append(["BND", [CONTIGS[k % 4], 700 + k, d1, CONTIGS[(k + 2) % 4], 10 + k, d2, next(src), next(rd)]])
    sigs.append(["BND", ["chr2", 5, "fwd", "chr1", 900, "rev", "suppl", "swapped_by_the_constructor"]])
    sigs.append(["BND", ["chr1", 900, "rev", "chr1", 5, "fwd", "cigar", "swapped_same_contig"]])
    return sigs


def by_type(sig_rows):
    out = {}
    for k, (t, _) in enumerate(sig_rows):
        out.setdefault(t, []).append(k)
    return out


def main_case(sig_rows):
    T = by_type(sig_rows)
    std = itertools.cycle(STD)
    score = itertools.cycle([1.0, 2.25, 3.5, 12.9, 80.0, 17.123456789012345, 0.30000000000000004, 1e-07, 100.0, 4.625])
    clusters = {k: [] for k in CLUSTER_SLOTS}
    pick = lambda t, n, at=0: [T[t][(at + j) % len(T[t])] for j in range(n)]      # noqa: E731
    # equal source tuples in different classes (the sort of all.vcf is stable over DEL, INS, INV, DUP_TAN), every contig, string order != natural order
    for k, contig in enumerate(["chr2", "chr10", "chr1", "chr01", "chr1", "chr10"]):
        for t in ("DEL", "INS", "INV"):
            clusters[t].append(["uni", [contig, 100, 200, next(score), 1 + k, pick(t, 1 + k, k), t, next(std), next(std)]])
        clusters["DEL"].append(["uni", [contig, 100, 150 + k, next(score), 2, pick("DEL", 2, k), "DEL", next(std), next(std)]])
        clusters["DUP_TAN"].append(["bi", [contig, 100, 200, contig, 200, 200 + 100 * k, next(score), 2, pick("DUP_TAN", 2, k), "DUP_TAN", next(std), next(std)]])
        clusters["DUP_INT"].append(["bi", [contig, 10 * k, 10 * k + 300, CONTIGS[k % 4], 77, 377, next(score), 3, pick("DUP_INT", 3, k), "DUP_INT", next(std), next(std)]])
        clusters["BND"].append(["bi", [contig, 40 + k, 41 + k, CONTIGS[(k + 1) % 4], 9, 10, next(score), 2, pick("BND", 2, k), "BND", next(std), next(std)]])
    clusters["INS"].append(["uni", ["chr1", 0, 2000000000, 5.0, 1, pick("INS", 1), "INS", None, None]])
    # the merged interspersed duplications of COMBINE: insertion and breakend members
    clusters["DUP_INT"].append(["bi", ["chr1", 5, 105, "chr2", 100, 200, 6.5, 3, [T["INS"][0], T["BND"][0], T["BND"][4]], "DUP_INT", None, 0.0]])
    clusters["DUP_TAN"].append(["bi", ["chr2", 1500000000, 2000000000, "chr2", 2000000000, 2147483647, 9.0, 1, [T["DUP_TAN"][-1]], "DUP_TAN", None, None]])
    cands = {k: [] for k in CANDIDATE_SLOTS}
    std = itertools.cycle([x for x in STD if x is None or x < 1e10])      # candidate deviations are printed rounded to two digits: the device does that below 1e10
    for k, contig in enumerate(["chr2", "chr10", "chr1", "chr01", "chr1"]):
        cands["DEL"].append([contig, 100 - 30 * k, 200, pick("DEL", 1 + k, k), next(score), next(std), next(std)])
        cands["INV"].append([contig, 100 + k, 200, pick("INV", 5, k), next(score), next(std), next(std)])
        cands["INS"].append([contig, 100, 200 + k, "", pick("INS", 2, k), next(score), next(std), next(std)])
        cands["DUP_TAN"].append([contig, 100, 200, k, bool(k % 2), pick("DUP_TAN", 2, k), next(score), next(std), next(std)])
        cands["DUP_INT"].append([contig, 10 * k, 10 * k + 300, CONTIGS[k % 4], 77 - 20 * k, 377, pick("DUP_INT", 3, k), next(score), next(std), next(std), bool(k % 2)])
        d = ("fwd", "rev")
        cands["BND"].append([contig, 40 + k - 41 * (k == 4), d[k % 2], CONTIGS[(k + 1) % 4], 9, d[(k // 2) % 2], pick("BND", 2, k), next(score), next(std), next(std)])
    # members of another type than the line; the destination end of a tandem duplication that leaves int32
    cands["DUP_INT"].append(["chr1", 5, 105, "chr2", 100, 200, [T["INS"][0], T["BND"][0], T["BND"][5], T["DEL"][1]], 6.5, None, 0.0, True])
    cands["DUP_INT"].append(["chr1", 5, 105, "chr2", 100, 200, [T["INS"][1]], 6.5, 0.004999, 0.005, False])
    cands["DUP_TAN"].append(["chr2", 1500000000, 2000000000, 3, True, [T["DUP_TAN"][-1]], 9.0, None, None])
    return clusters, cands


def score_case(sig_rows):
    """DEL clusters and candidates of 1..85 members whose scores are the reference's calculate_score of that many members"""
    T = by_type(sig_rows)
    std = itertools.cycle([(None, None), (0.0, 0.0), (1.5, 2.5), (10.0 / 3.0, 7.0), (99.0, 0.1), (250.0, 3.0)])
    clusters = {k: [] for k in CLUSTER_SLOTS}
    cands = {k: [] for k in CANDIDATE_SLOTS}
    for n in range(1, 86):
        sp, po = next(std)
        members = [T["DEL"][j % len(T["DEL"])] for j in range(n)]
        sc = calculate_score([None] * n, sp, po, 100 + n, "DEL")
        assert isinstance(sc, float)
        clusters["DEL"].append(["uni", ["chr1", 1000 * n, 1000 * n + 100 + n, sc, n, members, "DEL", sp, po]])
        cands["DEL"].append(["chr1", 1000 * n, 1000 * n + 100 + n, members, sc, sp, po])
        members = [T["INV"][j % len(T["INV"])] for j in range(n)]
        sc = calculate_score([types.SimpleNamespace(direction=sig_rows[m][1][5]) for m in members], sp, po, 100 + n, "INV")
        clusters["INV"].append(["uni", ["chr10", 1000 * n, 1000 * n + 100 + n, sc, n, members, "INV", sp, po]])
    return clusters, cands


def python_only_case(sig_rows):
    T = by_type(sig_rows)
    clusters = {k: [] for k in CLUSTER_SLOTS}
    cands = {k: [] for k in CANDIDATE_SLOTS}
    clusters["DEL"].append(["uni", ["chr1", 100, 200, 5, 1, [T["DEL"][0]], "DEL", 1.5, 2.5]])
    clusters["INS"].append(["uni", ["chr1", 100, 200, 5.0, 1, [T["INS"][0]], "INS", 1.5, 2.5]])
    cands["DEL"].append(["chr1", 100, 200, [T["DEL"][0]], 5, 1.5, 2.5])
    cands["INV"].append(["chr1", 100, 200, [T["INV"][0]], 5.0, 1.5, 2.5])
    return clusters, cands


def read_files(directory, names):
    out = []
    for n in names:
        with open(os.path.join(directory, n)) as fh:
            out.append(fh.read())
    return out


SIG_BED_FILES = ["del.bed", "ins.bed", "inv.bed", "dup_tan_source.bed", "dup_tan_dest.bed", "trans.bed", "dup_int.bed"]
CAND_BED_FILES = ["candidates_deletions.bed", "candidates_inversions.bed", "candidates_tan_duplications_source.bed", "candidates_tan_duplications_dest.bed",
                  "candidates_int_duplications_source.bed", "candidates_int_duplications_dest.bed", "candidates_novel_insertions.bed", "candidates_breakends.bed"]


def run_case(name, sig_rows, clusters, cands, python_only=False):
    sigs = [SIG_CLASSES[t](*args) for t, args in sig_rows]
    cl_objs, cl_entries = [], {}
    for slot in CLUSTER_SLOTS:
        objs = []
        for kind, args in clusters[slot]:
            a = list(args)
            k = 5 if kind == "uni" else 8
            a[k] = [sigs[j] for j in a[k]]
            objs.append((SVSignature.SignatureClusterUniLocal if kind == "uni" else SVSignature.SignatureClusterBiLocal)(*a))
        cl_objs.append(objs)
        cl_entries[slot] = [{"bed": [o.get_bed_entry()] if kind == "uni" else list(o.get_bed_entries()), "vcf": o.get_vcf_entry()}
                            for o, (kind, _) in zip(objs, clusters[slot])]
    ca_objs, ca_entries = [], {}
    for slot in CANDIDATE_SLOTS:
        objs = []
        for args in cands[slot]:
            a = list(args)
            k = CAND_MEMBER_SLOT[slot]
            a[k] = [sigs[j] for j in a[k]]
            objs.append(CAND_CLASSES[slot](*a))
        ca_objs.append(objs)
        ca_entries[slot] = [[o.get_bed_entry()] if slot in ("DEL", "INV", "INS") else list(o.get_bed_entries()) for o in objs]
    with tempfile.TemporaryDirectory() as d:
        SVIM_CLUSTER.write_signature_clusters_bed(d, tuple(cl_objs))
        SVIM_CLUSTER.write_signature_clusters_vcf(d, tuple(cl_objs), "2.0.0")
        SVIM_COMBINE.write_candidates(d, tuple(ca_objs))
        sig_beds = read_files(os.path.join(d, "signatures"), SIG_BED_FILES)
        sig_vcf = read_files(os.path.join(d, "signatures"), ["all.vcf"])[0]
        cand_beds = read_files(os.path.join(d, "candidates"), CAND_BED_FILES)
    return {"name": name, "python_only": python_only, "clusters": clusters, "candidates": cands, "cluster_entries": cl_entries, "candidate_entries": ca_entries,
            "sig_beds": sig_beds, "sig_vcf": sig_vcf, "cand_beds": cand_beds}


def main():
    sig_rows = make_sigs()
    sigs = [SIG_CLASSES[t](*args) for t, args in sig_rows]
    cases = [run_case("main", sig_rows, *main_case(sig_rows)), run_case("scores", sig_rows, *score_case(sig_rows)),
             run_case("empty", sig_rows, {k: [] for k in CLUSTER_SLOTS}, {k: [] for k in CANDIDATE_SLOTS}),
             run_case("int_score", sig_rows, *python_only_case(sig_rows), python_only=True)]
    out = {"versions": MG.VERSIONS, "contigs": CONTIGS, "sigs": sig_rows, "as_string": [[s.as_string("|"), s.as_string()] for s in sigs],
           "cluster_slots": CLUSTER_SLOTS, "candidate_slots": CANDIDATE_SLOTS, "sig_bed_files": SIG_BED_FILES, "cand_bed_files": CAND_BED_FILES, "version": "2.0.0",
           "cases": cases}
    path = os.path.join(HERE, "g_bed_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(out, sort_keys=True).encode("utf-8"))
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
