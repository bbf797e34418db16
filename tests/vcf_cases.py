"""Shared by tests/test_vcf.py and tests/test_gpu_vcf.py: the cases of tests/golden/g_vcf_cases.json.gz as svim_amd candidate objects."""
import gzip
import json
import os
import types

from svim_amd import candidates as K

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = {"DEL": K.CandidateDeletion, "INV": K.CandidateInversion, "INS": K.CandidateNovelInsertion, "DUP_TAN": K.CandidateDuplicationTandem,
           "DUP_INT": K.CandidateDuplicationInterspersed, "BND": K.CandidateBreakend}
_MEMBER_SLOT = {"INS": 4, "DUP_TAN": 5, "DUP_INT": 6, "BND": 6}
ALL_TYPES = ["DEL", "INS", "INV", "DUP:TANDEM", "DUP:INT", "BND"]


def load():
    with gzip.open(os.path.join(HERE, "golden", "g_vcf_cases.json.gz"), "rt") as fh:
        return json.load(fh)


class Sig(object):
    def __init__(self, read, sequence):
        self.read, self.sequence = read, sequence


def objects(rows, sig_rows):
    """candidate rows of the golden file -> {class name: list of svim_amd candidate objects} over fresh stand-in signatures"""
    sigs = [Sig(r, s) for r, s in sig_rows]
    out = {}
    for name, cls in CLASSES.items():
        objs = []
        for args, geno in rows.get(name, []):
            a = list(args)
            slot = _MEMBER_SLOT.get(name, 3)
            a[slot] = [sigs[k] for k in a[slot]]
            objs.append(cls(*a, **dict(zip(("support_fraction", "genotype", "ref_reads", "alt_reads"), geno))))
        out[name] = objs
    return out


def case_rows(G, case):
    return {k: [] for k in CLASSES} if case["name"] == "empty" else G["rows"]


def lists6(objs):
    """write_final_vcf's argument order"""
    return (objs["DUP_INT"], objs["INV"], objs["DUP_TAN"], objs["DEL"], objs["INS"], objs["BND"])


def options(case, **kw):
    return types.SimpleNamespace(sample="Sample", **dict(case["switches"], **kw))


def write_fasta(path, genome, width=60):
    with open(path, "w") as fh:
        for k, v in genome.items():
            fh.write(">%s\n" % k)
            for at in range(0, len(v), width):
                fh.write(v[at:at + width] + "\n")
    return path
