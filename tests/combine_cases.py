"""Shared by tests/test_combine.py, tests/test_gpu_combine.py and the two modules of the threshold cases: the cases of tests/golden/g_combine_cases.json.gz and
g_combine_threshold_cases.json.gz as svim_amd cluster objects, candidate objects as the rows the goldens hold, and the stage tables of the device against them."""
from svim_amd.signatures import SignatureClusterBiLocal, SignatureClusterUniLocal

TYPES = ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")


class Sig(object):
    """stand-in signature: COMBINE reads nothing of a member but `fully_covered` (tandem duplications)"""

    def __init__(self, k, fully_covered):
        self.k, self.fully_covered, self.type = k, fully_covered, "DUP_TAN" if fully_covered else "DEL"


def case_objects(case):
    """-> (six plain lists of cluster objects in cluster_sv_signatures' order, {id(signature): index})"""
    sigs = [Sig(k, fc) for k, fc in enumerate(case["signatures_fully_covered"])]
    out = []
    for t, rows in zip(TYPES, case["clusters"]):
        lst = []
        for r in rows:
            if t in ("DEL", "INS", "INV"):
                lst.append(SignatureClusterUniLocal(r[0], r[1], r[2], r[3], len(r[6]), [sigs[k] for k in r[6]], t, r[4], r[5]))
            else:
                c = SignatureClusterBiLocal(r[0], r[1], r[2], r[3], r[4], r[5], r[6], len(r[9]), [sigs[k] for k in r[9]], t, r[7], r[8])
                if t == "BND":
                    c.direction1, c.direction2 = r[10], r[11]
                lst.append(c)
        out.append(lst)
    return out, {id(s): s.k for s in sigs}


def cand_row(c, idx):
    """Candidate object -> the row make_golden.py's cand_row writes: every data attribute by name, members as signature indices"""
    d = {k: v for k, v in vars(c).items() if k not in ("members", "_members", "complement")}
    d["members"] = [idx[id(m)] for m in c.members]
    d["class"] = type(c).__name__
    return d


def merged_rows(clusters, idx):
    return [[c.source_contig, c.source_start, c.source_end, c.dest_contig, c.dest_start, c.dest_end, c.score, c.size, [idx[id(m)] for m in c.members], c.type,
             c.std_span, c.std_pos] for c in clusters]


def check_stages(eng, exp, sigs, references, idx, what=None):
    """the stage tables of the engine's last combine() against the golden's intermediates, ROW FOR ROW: the merged clusters, stage 2's removal list, the flagged
    candidates and - where the golden holds it - the walk's removal list"""
    import helpers as H
    from svim_amd import SVIM_COMBINE, convert
    st = eng.combine_stages()
    merged = merged_rows(SVIM_COMBINE.merged_cluster_objects(st["merged"], sigs, references), idx)
    d = H.first_json_difference(merged, exp["merged_insertion_from_clusters"])
    assert d is None, (what, d)
    assert st["remove_1"].tolist() == exp["inserted_regions_to_remove"], what
    flagged = [cand_row(c, idx) for c in convert.candidate_objects_range(st["flagged"], 0, st["flagged"].n, sigs, references)]
    d = H.first_json_difference(flagged, exp["flag_cutpaste"])
    assert d is None, (what, d)
    if "inserted_regions_to_remove_2" in exp:
        assert st["remove_2"].tolist() == exp["inserted_regions_to_remove_2"], what
    return st
