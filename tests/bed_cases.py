"""tests/golden/g_bed_cases.json.gz (made by tests/golden/make_golden_bed.py from the reference's writers) as objects of this package's classes."""
import helpers as H
from svim_amd import candidates as K, signatures as S

SIG_CLASSES = {"DEL": S.SignatureDeletion, "INS": S.SignatureInsertion, "INV": S.SignatureInversion, "DUP_INT": S.SignatureInsertionFrom,
               "DUP_TAN": S.SignatureDuplicationTandem, "BND": S.SignatureTranslocation}
CAND_CLASSES = {"DEL": K.CandidateDeletion, "INV": K.CandidateInversion, "INS": K.CandidateNovelInsertion, "DUP_TAN": K.CandidateDuplicationTandem,
                "DUP_INT": K.CandidateDuplicationInterspersed, "BND": K.CandidateBreakend}
CAND_MEMBER_SLOT = {"DEL": 3, "INV": 3, "INS": 4, "DUP_TAN": 5, "DUP_INT": 6, "BND": 6}


def load():
    return H.load("g_bed_cases.json.gz")


def signatures(G):
    return [SIG_CLASSES[t](*args) for t, args in G["sigs"]]


def cluster_lists(G, case, sigs):
    """the six lists in cluster_sv_signatures' order"""
    out = []
    for slot in G["cluster_slots"]:
        objs = []
        for kind, args in case["clusters"][slot]:
            a = list(args)
            k = 5 if kind == "uni" else 8
            a[k] = [sigs[j] for j in a[k]]
            objs.append((S.SignatureClusterUniLocal if kind == "uni" else S.SignatureClusterBiLocal)(*a))
        out.append(objs)
    return tuple(out)


def candidate_lists(G, case, sigs):
    """the six lists in write_candidates' order"""
    out = []
    for slot in G["candidate_slots"]:
        objs = []
        for args in case["candidates"][slot]:
            a = list(args)
            k = CAND_MEMBER_SLOT[slot]
            a[k] = [sigs[j] for j in a[k]]
            objs.append(CAND_CLASSES[slot](*a))
        out.append(objs)
    return tuple(out)


def vcf_body(G, case):
    """the lines of the golden's all.vcf behind its header"""
    return "".join(l + "\n" for l in case["sig_vcf"].split("\n")[:-1] if not l.startswith("#"))


def first_difference(got, want):
    if got == want:
        return None
    gl, wl = got.split(b"\n"), want.split(b"\n")
    for k, (a, b) in enumerate(zip(gl, wl)):
        if a != b:
            j = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "line %d differs at byte %d: %r != %r" % (k, j, a[max(0, j - 40):j + 40], b[max(0, j - 40):j + 40])
    return "%d lines != %d lines" % (len(gl), len(wl))
