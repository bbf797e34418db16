#!/usr/bin/env python3
"""Generate tests/golden/g_vcf_cases.json.gz by RUNNING THE REFERENCE's VCF writer on hand-built candidate objects.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them - its FastaFile stand-in
slices a FASTA file with end clipping, so a case's genome is written to a temporary file whose path is options.genome).  Every case is candidate rows
(constructor arguments of the reference's six candidate classes, genotype fields, member indices into stand-in signatures with `read` and `sequence`),
a set of switches, and what the reference made of them: write_final_vcf's file (header lines apart, fileDate dropped) and every get_vcf_entry* string.
DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vcf.py
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
from svim import SVIM_COMBINE, SVCandidate    # noqa: E402



class FastaFile(MG.FastaFile):
    """the stand-in of make_golden with the close() the writer calls"""

    def close(self):
        pass


SVIM_COMBINE.FastaFile = FastaFile
CLASSES = {"DEL": SVCandidate.CandidateDeletion, "INV": SVCandidate.CandidateInversion, "INS": SVCandidate.CandidateNovelInsertion,
           "DUP_TAN": SVCandidate.CandidateDuplicationTandem, "DUP_INT": SVCandidate.CandidateDuplicationInterspersed, "BND": SVCandidate.CandidateBreakend}
ALL_TYPES = ["DEL", "INS", "INV", "DUP:TANDEM", "DUP:INT", "BND"]
CONTIGS = ["chr1", "chr2", "chr10", "chrX", "chr01", "1", "MT", "scaffold_12_3"]
STD = [None, 0.0, 0.004999, 0.005, 0.015, 2.675, 1.0, 99.995, 123456.785]
READS = ["m1/100/0_500", "m1/100/600_900", "m1/1000/ccs", "m1/10/ccs", "m2/100/ccs", "readA", "a/b/c/d", "m3/7/0_9", "plain_read_8", "m1/100/0_500x"]


class Sig(object):
    def __init__(self, read, sequence):
        self.read, self.sequence = read, sequence


def make_genome(seed):
    rng = random.Random(seed)
    g = {}
    for k, name in enumerate(CONTIGS):
        n = 260 + 37 * k
        s = "".join(rng.choice("ACGT") for _ in range(n))
        s = s[:40] + "ACMGRSVTWYHKDBNacgtn" + s[60:]                  # every letter of the alphabet, and lower case the writer upper-cases
        g[name] = s
    return g


def make_sigs(seed, n=40):
    rng = random.Random(seed)
    return [[READS[rng.randrange(len(READS))] if k % 3 else READS[k % len(READS)], "".join(rng.choice("ACGTN") for _ in range(rng.randrange(0, 30)))] for k in range(n)]


def base_rows():
    """candidate rows per class: [constructor arguments with the members slot holding signature indices, genotype fields]"""
    std = itertools.cycle(STD)
    gts = itertools.cycle([[], ["0.5", "0/1", 3, 4], ["0.0", "0/0", 9, 0], ["1.0", "1/1", 0, 12], [".", "./.", None, 3], [".", "./.", 4, None], [".", "0/0", None, None]])
    R = {k: [] for k in CLASSES}
    m = lambda *idx: list(idx)      # noqa: E731
    for contig, start, end in (("chr1", 0, 50), ("chr1", 1, 80), ("chr1", 100, 200), ("chr01", 100, 200), ("chr10", 5, 45), ("chr2", 100, 200), ("1", 30, 31),
                               ("MT", 250, 300), ("scaffold_12_3", 3, 500), ("chrX", 100, 200)):
        R["DEL"].append([[contig, start, end, m(0, 1, 2, 1), 12.9, next(std), next(std)], next(gts)])
    for contig, start, end in (("chr1", 100, 200), ("chr2", 0, 75), ("chr1", 30, 70), ("chrX", 35, 65), ("chr01", 100, 200)):
        R["INV"].append([[contig, start, end, m(3, 4), 7.0, next(std), next(std)], next(gts)])
    for contig, start, end, mem in (("chr1", 100, 200, m(5, 6, 7)), ("chr1", 0, 30, m(8)), ("chr1", 1, 31, m(9, 9, 10)), ("chr10", 100, 200, m(0, 1, 4)),
                                    ("MT", 100, 140, m(11, 12, 13, 14, 15, 16)), ("1", 100, 200, m(7, 3))):
        R["INS"].append([[contig, start, end, "", mem, 3.99, next(std), next(std)], next(gts)])
    for contig, start, end, copies, covered in (("chr1", 100, 200, 1, True), ("chr1", 10, 40, 0, False), ("chr2", 50, 90, 7, True), ("chrX", 0, 20, 2, False),
                                                ("chr1", 150, 200, 1, False), ("chr01", 150, 200, 3, True)):
        R["DUP_TAN"].append([[contig, start, end, copies, covered, m(17, 18, 17), 20.5, next(std), next(std)], next(gts)])
    for sc, ss, se, dc, ds, de, cut in (("chr1", 100, 200, "chr2", 100, 200, False), ("chr2", 10, 60, "chr1", 0, 50, True), ("chr10", 20, 50, "chrX", 1, 31, False),
                                        ("chr1", 100, 200, "chr1", 100, 200, True), ("MT", 0, 40, "1", 200, 240, False)):
        R["DUP_INT"].append([[sc, ss, se, dc, ds, de, m(19, 20, 21, 22), 5.0, next(std), next(std), cut], next(gts)])
    for sc, ss, sd, dc, ds, dd in (("chr1", 100, "fwd", "chr2", 100, "fwd"), ("chr1", 100, "fwd", "chr10", 7, "rev"), ("chr2", 0, "rev", "chr2", 199, "rev"),
                                   ("chrX", 99, "rev", "chr1", 100, "fwd"), ("chr01", 100, "fwd", "scaffold_12_3", 12, "rev")):
        R["BND"].append([[sc, ss, sd, dc, ds, dd, m(23, 24, 25, 24), 9.5, next(std), next(std)], next(gts)])
    return R


def objects(rows, sigs):
    out = {}
    for name, cls in CLASSES.items():
        objs = []
        slot = {"INS": 4, "DUP_TAN": 5, "DUP_INT": 6, "BND": 6}.get(name, 3)
        for args, geno in rows[name]:
            a = list(args)
            a[slot] = [sigs[k] for k in a[slot]]
            kw = dict(zip(("support_fraction", "genotype", "ref_reads", "alt_reads"), geno))
            objs.append(cls(*a, **kw))
        out[name] = objs
    return out


def run_case(name, genome, sig_rows, rows, switches, types_to_output):
    sigs = [Sig(r, s) for r, s in sig_rows]
    objs = objects(rows, sigs)
    with tempfile.TemporaryDirectory() as d:
        fasta = os.path.join(d, "genome.fa")
        with open(fasta, "w") as fh:
            for k, v in genome.items():
                fh.write(">%s\n" % k)
                for at in range(0, len(v), 60):
                    fh.write(v[at:at + 60] + "\n")
        o = types.SimpleNamespace(working_dir=d, genome=fasta, sample="Sample", **switches)
        SVIM_COMBINE.write_final_vcf(objs["DUP_INT"], objs["INV"], objs["DUP_TAN"], objs["DEL"], objs["INS"], objs["BND"], "2.0.0", list(genome),
                                     [len(v) for v in genome.values()], types_to_output, o)
        with open(os.path.join(d, "variants.vcf")) as fh:
            lines = fh.read().split("\n")
        assert lines[-1] == ""
        lines = lines[:-1]
        reference = FastaFile(fasta)
        seq = not o.symbolic_alleles
        sw = (o.read_names, o.zmws)
        entries = {
            "DEL": [{"get_vcf_entry": c.get_vcf_entry(seq, reference, *sw)} for c in objs["DEL"]],
            "INV": [{"get_vcf_entry": c.get_vcf_entry(seq, reference, *sw)} for c in objs["INV"]],
            "INS": [{"get_vcf_entry": c.get_vcf_entry(seq, reference, o.insertion_sequences, *sw)} for c in objs["INS"]],
            "DUP_TAN": [{"get_vcf_entry_as_ins": c.get_vcf_entry_as_ins(seq, reference, *sw), "get_vcf_entry_as_dup": c.get_vcf_entry_as_dup(*sw)} for c in objs["DUP_TAN"]],
            "DUP_INT": [{"get_vcf_entry_as_ins": c.get_vcf_entry_as_ins(seq, reference, *sw), "get_vcf_entry_as_dup": c.get_vcf_entry_as_dup(*sw)} for c in objs["DUP_INT"]],
            "BND": [{"get_vcf_entry": c.get_vcf_entry(*sw), "get_vcf_entry_reverse": c.get_vcf_entry_reverse(*sw)} for c in objs["BND"]],
        }
    header = [l for l in lines if l.startswith("#") and not l.startswith("##fileDate=")]
    body = [l for l in lines if not l.startswith("#")]
    return {"name": name, "switches": switches, "types": types_to_output, "header": header, "body": body, "entries": entries}


def main():
    genome, sig_rows, rows = make_genome(11), make_sigs(12), base_rows()
    cases = []
    names = ("symbolic_alleles", "tandem_duplications_as_insertions", "interspersed_duplications_as_insertions")
    extras = ((False, False, False), (True, True, True), (False, True, False), (False, False, True), (True, False, False))
    for flags in itertools.product((False, True), repeat=3):
        for seqs, reads, zmws in extras:
            sw = dict(zip(names, flags), insertion_sequences=seqs, read_names=reads, zmws=zmws)
            cases.append(run_case("all_%d%d%d_%d%d%d" % (tuple(map(int, flags)) + (int(seqs), int(reads), int(zmws))), genome, sig_rows, rows, sw, ALL_TYPES))
    plain = dict(symbolic_alleles=False, tandem_duplications_as_insertions=True, interspersed_duplications_as_insertions=False, insertion_sequences=True,
                 read_names=True, zmws=True)
    for label, tt in (("none", []), ("bnd_only", ["BND"]), ("del_ins", ["DEL", "INS"]), ("dups", ["DUP:TANDEM", "DUP:INT"]), ("ins_only", ["INS"])):
        cases.append(run_case("mask_" + label, genome, sig_rows, rows, plain, tt))
    cases.append(run_case("empty", genome, sig_rows, {k: [] for k in CLASSES}, plain, ALL_TYPES))
    std = [[x, str(round(x, 2)) if x else "."] for x in STD[1:]]
    nat_names = CONTIGS + ["chr1_random", "chr001", "chrUn_12", "10", "2", "chr1a2", "chrM", "", "chr"]
    nat_sorted = [e[0][0] for e in SVIM_COMBINE.sorted_nicely([((n, 0, 0), "", "DEL") for n in nat_names])]
    out = {"versions": MG.VERSIONS, "contigs": CONTIGS, "genome": genome, "sigs": sig_rows, "rows": rows, "std": std,
           "natural": {"names": nat_names, "sorted": nat_sorted}, "cases": cases}
    path = os.path.join(HERE, "g_vcf_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps(out, sort_keys=True).encode("utf-8"))
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
