#!/usr/bin/env python3
"""Generate tests/golden/g_combine_cases.json.gz by RUNNING THE REFERENCE's COMBINE step on hand-built cluster lists.

Build container only (needs the reference checkout make_golden.py reads; the same stubs: this module imports make_golden for them).  Every case is six
lists of cluster rows (cluster_sv_signatures' order) over stand-in signatures (only `fully_covered` of a member is ever read by COMBINE) and the rows
the reference's merge_translocations_at_insertions, flag_cutpaste_candidates and combine_clusters (--skip_consensus) made of them - or the exception it
raised.  DATA ONLY: no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_combine.py
"""
import copy
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG    # noqa: E402  (stubs pysam / edlib, puts the reference on the path)

for _name in ("spoa", "cpuinfo"):
    _stub = types.ModuleType(_name)
    _stub.poa = _stub.get_cpu_info = None
    sys.modules.setdefault(_name, _stub)
from svim import SVIM_COMBINE, SVIM_merging                                        # noqa: E402
from svim.SVSignature import SignatureClusterBiLocal, SignatureClusterUniLocal    # noqa: E402

OPT = dict(trans_sv_max_distance=500, del_ins_dup_max_distance=1.0, position_distance_normalizer=900, partition_max_distance=1000,
           cluster_max_distance=0.5, skip_consensus=True)


class Sig(object):
    def __init__(self, k, fully_covered):
        self.k, self.fully_covered = k, fully_covered


class Case(object):
    """rows: uni [contig, start, end, score, std_span, std_pos, members]; bi [sc, ss, se, dc, ds, de, score, std_span, std_pos, members(, d1, d2)]"""

    def __init__(self, name, references, **opt):
        self.name, self.references, self.opt = name, references, dict(OPT, **opt)
        self.sigs = []
        self.lists = {k: [] for k in ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")}

    def mem(self, n, fully_covered=False):
        out = []
        for _ in range(n):
            self.sigs.append(bool(fully_covered))
            out.append(len(self.sigs) - 1)
        return out

    def uni(self, t, contig, start, end, score=10.0, std_span=1.5, std_pos=2.5, n=2):
        self.lists[t].append([contig, start, end, score, std_span, std_pos, self.mem(n)])

    def bi(self, t, sc, ss, se, dc, ds, de, score=10.0, std_span=1.5, std_pos=2.5, n=2, dirs=None, fully_covered=False, members=None):
        row = [sc, ss, se, dc, ds, de, score, std_span, std_pos, members if members is not None else self.mem(n, fully_covered)]
        self.lists[t].append(row + (list(dirs) if dirs else []))

    def flank(self, contig, pos, dest_contig, d1, d2, **kw):
        """fwd/fwd breakend at pos -> (dest_contig, d1) and rev/rev breakend at pos -> (dest_contig, d2)"""
        self.bi("BND", contig, pos, pos + 1, dest_contig, d1, d1 + 1, dirs=("fwd", "fwd"), **kw)
        self.bi("BND", contig, pos, pos + 1, dest_contig, d2, d2 + 1, dirs=("rev", "rev"), **kw)


def objects(case):
    sigs = [Sig(k, fc) for k, fc in enumerate(case.sigs)]
    out = []
    for t in ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND"):
        lst = []
        for r in case.lists[t]:
            if t in ("DEL", "INS", "INV"):
                lst.append(SignatureClusterUniLocal(r[0], r[1], r[2], r[3], len(r[6]), [sigs[k] for k in r[6]], t, r[4], r[5]))
            else:
                c = SignatureClusterBiLocal(r[0], r[1], r[2], r[3], r[4], r[5], r[6], len(r[9]), [sigs[k] for k in r[9]], t, r[7], r[8])
                if t == "BND":
                    c.direction1, c.direction2 = r[10], r[11]
                lst.append(c)
        out.append(lst)
    return out, {id(s): s.k for s in sigs}


def run(case):
    o = types.SimpleNamespace(**case.opt)
    c6, idx = objects(case)
    dele, insr, inv, tan, dint, bnd = c6
    b2, i2 = list(bnd), list(insr)
    new_from, to_remove = SVIM_merging.merge_translocations_at_insertions(b2, i2, o)
    merged = [[c.source_contig, c.source_start, c.source_end, c.dest_contig, c.dest_start, c.dest_end, c.score, c.size, [idx[id(m)] for m in c.members], c.type,
               c.std_span, c.std_pos] for c in new_from]
    n_ins_before = len(insr)
    try:
        flagged = [MG.cand_row(c, idx) for c in SVIM_merging.flag_cutpaste_candidates(list(dint) + new_from, dele, o)]
        out = SVIM_COMBINE.combine_clusters((dele, insr, inv, tan, dint, bnd), o)
    except IndexError:
        try:
            SVIM_COMBINE.combine_clusters((dele, insr, inv, tan, dint, bnd), o)       # the state combine_clusters itself leaves its lists in when it raises
            raise AssertionError("expected IndexError")
        except IndexError:
            pass
        return {"raises": "IndexError", "merged_insertion_from_clusters": merged, "inserted_regions_to_remove": to_remove, "n_bnd_after": len(bnd),
                "n_dup_int_after": len(dint), "n_ins_after": len(insr)}
    return {"merged_insertion_from_clusters": merged, "inserted_regions_to_remove": to_remove, "n_bnd_after_merge": len(b2), "flag_cutpaste": flagged,
            "n_ins_before": n_ins_before, "n_ins_after": len(insr), "n_dup_int_after": len(dint), "n_bnd_after": len(bnd),
            "combine": [[MG.cand_row(c, idx) for c in lst] for lst in out]}


def cases():
    out = []
    R = ["chr1", "chr2", "chr10"]                       # tid order != name order ("chr10" < "chr2")

    c = Case("empty_everything", R)
    out.append(c)

    for k, only in enumerate(("DEL", "INS", "INV", "DUP_TAN", "BND")):
        c = Case("only_" + only.lower(), R)
        if only in ("DEL", "INS", "INV"):
            c.uni(only, "chr2", 1000 + k, 1400 + k)
            c.uni(only, "chr10", 50, 700, score=0.0)
            c.uni(only, "chr10", -3, 400, score=7.0, std_span=None, std_pos=None)         # start clamps to 0
        elif only == "DUP_TAN":
            c.bi(only, "chr1", 1000, 1100, "chr1", 1100, 1350, fully_covered=True)         # 2.5 -> 2
            c.bi(only, "chr1", 2000, 2100, "chr1", 2100, 2450)                             # 3.5 -> 4
            c.bi(only, "chr2", -5, 95, "chr2", 95, 245, std_span=None, std_pos=None)       # 1.5 -> 2, start clamps
            c.bi(only, "chr2", 500, 700, "chr2", 700, 1000)                                # 1.5 -> 2
            c.bi(only, "chr2", 900, 1100, "chr2", 1100, 1200)                              # 0.5 -> 0
        else:
            c.bi(only, "chr1", 100, 101, "chr2", -2, -1, dirs=("fwd", "rev"))
            c.bi(only, "chr10", 5, 6, "chr2", 77, 78, dirs=("rev", "rev"), std_span=None)
        out.append(c)

    c = Case("no_deletion_index_error", R)
    c.uni("INS", "chr1", 1000, 1300)
    c.flank("chr1", 1000, "chr2", 5000, 5300)
    c.bi("DUP_INT", "chr2", 100, 400, "chr1", 9000, 9300)
    out.append(c)

    c = Case("dup_int_without_deletions", R)
    c.bi("DUP_INT", "chr2", 100, 400, "chr1", 9000, 9300)
    out.append(c)

    # stage 2: bounds of the length ratio hit exactly, ties, duplicates, one-sided contigs, None stds, different destination contigs
    c = Case("merge_bounds_and_ties", R)
    c.uni("DEL", "chr2", 5000, 5210)
    c.uni("DEL", "chr1", 100, 300, score=-1.0)
    c.uni("INS", "chr1", 1000, 1208)                    # (208 + 1) / (189 + 1) = 1.1 exactly
    c.flank("chr1", 1000, "chr2", 5000, 5189, std_span=None, std_pos=None)
    c.uni("INS", "chr1", 3000, 3189)                    # (189 + 1) / (199 + 1) = 0.95
    c.flank("chr1", 3010, "chr2", 7000, 7199)
    c.uni("INS", "chr1", 6000, 6300)                    # ratio 301 / 274 = 1.0985...: inside; ratio just outside below
    c.flank("chr1", 5990, "chr2", 9000, 9273, std_pos=None)
    c.uni("INS", "chr1", 8000, 8300)                    # 301 / 273 > 1.1
    c.flank("chr1", 8000, "chr2", 12000, 12272)
    c.uni("INS", "chr1", 10000, 10300, score=0.0)       # tie: breakends at 9900 and 10100 -> the lower one; merged although its score is 0
    c.flank("chr1", 9900, "chr2", 20000, 20300)
    c.flank("chr1", 10100, "chr2", 30000, 30300)
    c.uni("INS", "chr1", 12000, 12300)                  # duplicates at the same position: bisect_left lands on the first
    c.flank("chr1", 12000, "chr2", 40000, 40300)
    c.flank("chr1", 12000, "chr2", 45000, 45300)
    c.uni("INS", "chr10", 2000, 2300)                   # fwd/fwd only on chr10: KeyError -> continue
    c.bi("BND", "chr10", 2000, 2001, "chr2", 50000, 50001, dirs=("fwd", "fwd"))
    c.uni("INS", "chr2", 60000, 60300)                  # matched only through MIRRORED clusters (chr1 -> chr2 breakends seen from chr2)
    c.bi("BND", "chr1", 70000, 70001, "chr2", 60000, 60001, dirs=("rev", "rev"))     # mirrored: chr2:60000 fwd/fwd -> chr1:70000
    c.bi("BND", "chr1", 70300, 70301, "chr2", 60000, 60001, dirs=("fwd", "fwd"))     # mirrored: rev/rev
    c.uni("INS", "chr1", 15000, 15300)                  # destinations on different contigs
    c.bi("BND", "chr1", 15000, 15001, "chr2", 100, 101, dirs=("fwd", "fwd"))
    c.bi("BND", "chr1", 15000, 15001, "chr10", 400, 401, dirs=("rev", "rev"))
    c.uni("INS", "chr1", 17000, 17300)                  # too far: 501 > trans_sv_max_distance
    c.flank("chr1", 17501, "chr2", 200, 500)
    c.uni("INS", "chr1", 19000, 19300)                  # exactly 500 away, std 100 and beyond -> factor 0
    c.flank("chr1", 19500, "chr2", 300, 600, std_span=120.0, std_pos=100.0)
    c.bi("BND", "chr1", 500, 502, "chr2", 900, 900, dirs=("fwd", "rev"))              # end - start of 2 and 0: rounding of x and x + 1
    c.bi("DUP_INT", "chr2", 5005, 5205, "chr1", 30000, 30200)                          # near the chr2 deletion: cutpaste
    c.bi("DUP_INT", "chr2", -4, 300, "chr1", -7, 297, std_span=None, std_pos=None)     # clamps
    out.append(c)

    # stage 4: the interspersed list runs out mid-walk and the tandem list takes over / never runs out although a tandem overlap exists
    c = Case("walk_runs_out", R)
    c.uni("DEL", "chr1", 100, 300)
    c.bi("DUP_INT", "chr2", 100, 400, "chr1", 1000, 1300)
    c.bi("DUP_INT", "chr2", 900, 1200, "chr10", 500, 800)
    c.uni("INS", "chr1", 1000, 1290)                    # overlaps the first duplication's destination
    c.uni("INS", "chr1", 5000, 5200)                    # moves the pointer on; chr10 < chr1, so the list runs out HERE: tandem consulted, overlap found
    c.uni("INS", "chr1", 7000, 7100)                    # tandem list: pointer moves
    c.uni("INS", "chr2", 300, 420)                      # tandem destination chr2:300-400... (below)
    c.uni("INS", "chr2", 300, 1000, score=5.0)          # too long for the tandem destination: (700 - 100) / 700 >= 0.2
    c.bi("DUP_TAN", "chr1", 4800, 5000, "chr1", 5000, 5200)          # destination chr1:5000-5200
    c.bi("DUP_TAN", "chr2", 200, 300, "chr2", 300, 400)              # destination chr2:300-400
    out.append(c)
    c = Case("walk_never_runs_out", R)
    c.uni("DEL", "chr1", 100, 300)
    c.bi("DUP_INT", "chr2", 100, 400, "chr1", 1000, 1300)
    c.bi("DUP_INT", "chr2", 900, 1200, "chr2", 90000, 90300)          # stays in front of every insertion: the tandem list is never consulted
    c.bi("DUP_INT", "chr2", 2000, 2300, "chr1", 900, 5000)            # end not monotone in the sort order
    c.uni("INS", "chr1", 950, 1250)
    c.uni("INS", "chr1", 5000, 5200)                    # a tandem duplication ends up exactly here, but the insertion stays
    c.uni("INS", "chr1", 5100, 5300, score=0.0)         # dropped for its score, not removed
    c.bi("DUP_TAN", "chr1", 4800, 5000, "chr1", 5000, 5200)
    out.append(c)

    # stage 5: partitions of exactly 100 and of more than 100 candidates, seeded sampling carried across partitions, a chain across the distance limit
    rng = random.Random(99)
    c = Case("recluster_large_partitions", R)
    c.uni("DEL", "chr2", 1000, 1300)
    for part, (contig, n, base) in enumerate((("chr2", 100, 1000), ("chr10", 137, 50000), ("chr1", 1100, 200000), ("chr1", 3, 900000), ("chr2", 1, 500000))):
        for k in range(n):
            s = base + rng.randrange(0, 40) * 7
            ln = 300 + rng.randrange(0, 4) * 150
            d = 10000 + rng.randrange(0, 6) * 400
            c.bi("DUP_INT", contig, s, s + ln, R[(part + k) % 3], d, d + ln, score=float(rng.randrange(1, 30)), std_span=rng.choice([None, 0.5, 3.25]),
                 std_pos=rng.choice([None, 1.0, 7.125]), n=1 + k % 3)
    out.append(c)

    c = Case("recluster_chain", R, partition_max_distance=50)
    c.uni("DEL", "chr1", 100, 300)
    for k in range(12):
        c.bi("DUP_INT", "chr1", 1000 + 330 * k, 1300 + 330 * k, "chr2", 500 + 5 * k, 800 + 5 * k, score=float(k))
    c.bi("DUP_INT", "chr1", 1000 + 330 * 12 + 51, 9000, "chr2", 1, 2)
    out.append(c)
    return out


def main():
    res = []
    for c in cases():
        exp = run(c)
        res.append({"name": c.name, "references": c.references, "signatures_fully_covered": c.sigs, "options": c.opt, "clusters": [c.lists[t] for t in
                    ("DEL", "INS", "INV", "DUP_TAN", "DUP_INT", "BND")], "expected": exp})
        print(c.name, "raises" if "raises" in exp else [len(x) for x in exp["combine"]], exp.get("inserted_regions_to_remove"))
    by = {r["name"]: r["expected"] for r in res}
    assert by["no_deletion_index_error"].get("raises") and by["dup_int_without_deletions"].get("raises")
    assert len(by["merge_bounds_and_ties"]["merged_insertion_from_clusters"]) >= 5
    assert by["walk_runs_out"]["n_ins_after"] < by["walk_runs_out"]["n_ins_before"]
    MG.dump("g_combine_cases.json.gz", {"cases": res, "source": "svim.SVIM_merging.merge_translocations_at_insertions / flag_cutpaste_candidates and "
                                        "svim.SVIM_COMBINE.combine_clusters (skip_consensus) on hand-built cluster lists"})


if __name__ == "__main__":
    main()
