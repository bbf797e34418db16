"""Shared by the GENOTYPE table-route tests: the golden's hand-made candidates as a candidate table (svx_candidate_view) plus the read ids of the signatures its
members index, the table route stated in Python over an interval join (the C oracle's or the HIP one's), the object route the results are compared with, and
the check of the resident alignment table against AlignmentIndex."""
import numpy as np

from svim_amd import SVIM_genotyping, _abi

CLS = {"DEL": _abi.CAND_DEL, "INV": _abi.CAND_INV, "INS": _abi.CAND_INS, "DUP_INT": _abi.CAND_DUP_INT}


class Sig(object):
    def __init__(self, read):
        self.read = read


class Candidate(object):
    """Quacks like the reference's candidates (src/svim/SVCandidate.py) as far as genotype() looks: get_source / get_destination, score, members."""

    def __init__(self, typ, contig, start, end, members, score):
        self.type, self.locus, self.members, self.score = typ, (contig, start, end), [Sig(m) for m in members], score
        self.support_fraction, self.genotype, self.ref_reads, self.alt_reads = ".", "./.", None, None

    def get_source(self):
        return self.locus if self.type in ("DEL", "INV") else ("chr1", 100, 100 + self.locus[2] - self.locus[1])

    def get_destination(self):
        return self.locus

    def fields(self):
        return [self.support_fraction, self.genotype, self.ref_reads, self.alt_reads]


def table_from_candidates(cands, references, read_id):
    """[(type name, contig, start, end, member read names, score)] -> (CandidateTable grouped by class, sig_read_id int32, row of every input candidate).
    One signature per member; read_id(name) interns a read name.  DEL / INV rows use the source columns, INS / DUP_INT rows the destination columns."""
    order = sorted(range(len(cands)), key=lambda k: (CLS[cands[k][0]], k))
    row_of = {k: r for r, k in enumerate(order)}
    n_members = sum(len(c[4]) for c in cands)
    t = _abi.CandidateTable(len(cands), n_members)
    t.std_span[:] = np.nan
    t.std_pos[:] = np.nan
    rid, at = [], 0
    for r, k in enumerate(order):
        typ, contig, start, end, members, score = cands[k]
        cls = CLS[typ]
        t.cls[r], t.score[r] = cls, score
        if cls in (_abi.CAND_DEL, _abi.CAND_INV):
            t.contig[r], t.start[r], t.end[r], t.contig2[r] = references.index(contig), start, end, -1
        else:
            t.contig[r] = -1 if cls == _abi.CAND_INS else 0
            t.contig2[r], t.start2[r], t.end2[r] = references.index(contig), start, end
        for m in members:
            t.members[at] = at
            rid.append(read_id(m))
            at += 1
        t.member_off[r + 1] = at
    v = t.view()
    for cls in range(6):
        v.class_count[cls] = sum(1 for c in cands if CLS[c[0]] == cls)
    t.finish(v)
    return t, np.asarray(rid, dtype=np.int32), [row_of[k] for k in range(len(cands))]


def golden_candidates(g):
    return [(case["type"], r[0], r[1], r[2], r[3], r[4]) for case in g["cases"] for r in case["candidates"]]


def golden_expected(g):
    return [e for case in g["cases"] for e in case["expected"]]


def table_route_python(table, sig_read_id, join, options):
    """The table route stated in Python: class and score select, the distinct read ids of the members, the interval join `join` (an engine or the oracle with
    the alignment index set, whose name ids are the read ids), the call from the two counts -> [support_fraction, genotype, ref_reads, alt_reads] per row."""
    sel, mode, tid, start, end = SVIM_genotyping.candidate_loci(table, options.minimum_score)
    ids = [np.unique(sig_read_id[table.members[table.member_off[r]:table.member_off[r + 1]]]) for r in range(table.n)]
    ref = np.zeros(table.n, dtype=np.int64)
    for m in (0, 1):
        rows = [r for r in range(table.n) if sel[r] and mode[r] == m]
        if rows:
            moff = np.concatenate([[0], np.cumsum([len(ids[r]) for r in rows])]).astype(np.int64)
            names = np.concatenate([ids[r] for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
            ref[rows] = join.genotype(m, tid[rows], start[rows], end[rows], moff, names, int(options.min_mapq))
    out = []
    for r in range(table.n):
        if not sel[r]:
            out.append([".", "./.", None, None])
            continue
        code, f = SVIM_genotyping.genotype_calls(len(ids[r]), int(ref[r]), options)
        out.append([f, _abi.GT_NAMES[code], int(ref[r]), len(ids[r])])
    return out


def columns_as_fields(g):
    """Engine.fetch_genotypes() -> the same per-row lists"""
    out = []
    for gt, rr, ar, sf in zip(g["gt"].tolist(), g["ref_reads"].tolist(), g["alt_reads"].tolist(), g["support_fraction"].tolist()):
        out.append([".", "./.", None, None] if rr < 0 else ["." if sf != sf else sf, _abi.GT_NAMES[gt], rr, ar])
    return out


def check_table_against_index(eng, pipe, index):
    """the resident table = AlignmentIndex of the same records, column by column; names up to the id relabelling; end only where it is defined"""
    a, names = eng.alignments(), pipe.bam.read_names()
    keep = np.flatnonzero(a["tid"] >= 0)                    # (AlignmentIndex leaves records without a position out; the table keeps them, behind the contigs)
    assert keep.size == index.n and (keep == np.arange(keep.size)).all()
    for col, exp in (("pos", index.pos), ("flag", index.flag), ("mapq", index.mapq)):
        assert (a[col][keep] == exp).all(), col
    assert (np.searchsorted(a["tid"][keep], np.arange(index.n_contig + 1)) == index.contig_first).all()
    counts = (a["flag"][keep] & (4 | 256)) == 0
    assert (a["end"][keep][counts] == index.end[counts]).all() and (a["end"][keep][~counts] == a["pos"][keep][~counts]).all()
    by_id = {v: k for k, v in index.name_ids.items()}
    assert [names[r] for r in a["read_id"][keep].tolist()] == [by_id[i] for i in index.name_id.tolist()]
    return a, names
