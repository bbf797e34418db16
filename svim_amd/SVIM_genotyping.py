"""GENOTYPE on the GPU: drop-in for svim.SVIM_genotyping (src/svim/SVIM_genotyping.py) - same entry points, same results.

    genotype(candidates, bam, type, options)          mutates the candidates like the reference (:79-93)
    genotype_resident(engine, options, lengths)       the same for all four types at once, from the tables resident in the engine: no object is made
    span_position_distance(candidate, signature, n)   (:9-31)

The reference re-fetches the BAM around every candidate (:48).  Here the alignment records are indexed once per file
(`AlignmentIndex`: reference_start / reference_end / flag / mapq / interned query name, file order) and the per-candidate walk is
an interval join on the device (`svx_genotype`, svim_amd/csrc/genotype.hip).  The candidates only have to quack like the
reference's: get_source() / get_destination(), .score, .members (signatures with .read), and receive support_fraction, genotype,
ref_reads, alt_reads.
"""
import numpy as np

from . import _abi
from ._abi import ptr


class AlignmentIndex(object):
    """Structure-of-arrays view of every alignment record of a coordinate-sorted file, in file order.
    order="sort": the file may be in any order; the index is that of its records in the coordinate order of svim_amd/bamsort.py - key (uint32(refID),
    uint32(pos + 1), flag & 16), stable, so ties keep file order - which is the index of sort_bam(file).  src_row[i] is then the place in the file of row i,
    counted over all records (those without a position, which the index leaves out, sort last)."""

    def __init__(self, bam, order="file"):
        if order not in ("file", "sort"):
            raise ValueError("order: 'file' or 'sort'")
        self.references = list(bam.references)
        self.lengths = [int(x) for x in bam.lengths]
        tid, pos, end, flag, mapq, name = [], [], [], [], [], []
        self.name_ids = {}
        recs = list(enumerate(bam.fetch(until_eof=True)))
        if order == "sort":
            from .bamsort import coordinate_key
            recs.sort(key=lambda ka: coordinate_key(-1 if ka[1].reference_id is None else ka[1].reference_id, ka[1].reference_start, ka[1].flag))
        self.src_row = np.asarray([k for k, a in recs if a.reference_id is not None and a.reference_id >= 0], dtype=np.uint32)
        for _, a in recs:
            if a.reference_id is None or a.reference_id < 0:
                continue                                    # records without a position are never returned by a region fetch
            tid.append(a.reference_id)
            pos.append(a.reference_start)
            # end = pos + reference span, as the resident table has it (csrc/alnindex.hip): pos itself for an unmapped-but-placed record and for a mapped record
            # without reference span (30S), for which reference_end is bam_endpos = pos + 1; the join derives bam_endpos from the two columns where it needs it
            re = a.reference_end
            spans = re is not None and any(l and op in (0, 2, 3, 7, 8) for op, l in a.cigartuples)
            end.append(re if spans else a.reference_start)
            flag.append(a.flag)
            mapq.append(a.mapping_quality)
            name.append(self.name_ids.setdefault(a.query_name, len(self.name_ids)))
        tid = np.asarray(tid, dtype=np.int32)
        pos = np.asarray(pos, dtype=np.int32)
        if tid.size and ((np.diff(tid) < 0).any() or ((np.diff(tid) == 0) & (np.diff(pos) < 0)).any()):
            raise ValueError("genotyping needs a coordinate-sorted alignment file")
        n_contig = len(self.references)
        self.n, self.n_contig = int(tid.size), n_contig
        self.contig_first = np.searchsorted(tid, np.arange(n_contig + 1), side="left").astype(np.int64)
        self.contig_len = np.asarray(self.lengths, dtype=np.int64)
        self.pos = pos
        self.end = np.asarray(end, dtype=np.int32)
        self.flag = np.asarray(flag, dtype=np.uint16)
        self.mapq = np.asarray(mapq, dtype=np.uint8)
        self.name_id = np.asarray(name, dtype=np.int32)

    def view(self):
        v = _abi.AlnIndex()
        v.n, v.n_contig = self.n, self.n_contig
        pad = lambda a, dt: a if a.size else np.zeros(1, dtype=dt)      # noqa: E731
        self._keep = [self.contig_first, pad(self.contig_len, np.int64), pad(self.pos, np.int32), pad(self.end, np.int32),
                      pad(self.flag, np.uint16), pad(self.mapq, np.uint8), pad(self.name_id, np.int32)]
        v.contig_first, v.contig_len, v.pos, v.end, v.flag, v.mapq, v.name_id = [ptr(a) for a in self._keep]
        return v


_INDEX_ATTR = "_svx_alignment_index"


def alignment_index(bam, order="file"):
    """The index of `bam` in that order, built on first use and kept on the object."""
    attr = _INDEX_ATTR if order == "file" else _INDEX_ATTR + "_" + str(order)
    ix = getattr(bam, attr, None)
    if ix is None:
        ix = AlignmentIndex(bam, order=order)
        try:
            setattr(bam, attr, ix)
        except AttributeError:
            pass
    return ix


def span_position_distance(candidate, signature, position_distance_normalizer):
    """src/svim/SVIM_genotyping.py:9-31."""
    c_contig, c_start, c_end = candidate.get_destination() if candidate.type in ("INS", "DUP_INT") else candidate.get_source()
    s_contig, s_start, s_end = signature.get_destination() if signature.type == "DUP_INT" else signature.get_source()
    compatible = candidate.type == signature.type or {candidate.type, signature.type} == {"INS", "DUP_INT"}
    if not compatible or c_contig != s_contig:
        return float("inf")
    span1, span2 = c_end - c_start, s_end - s_start
    center1, center2 = (c_start + c_end) // 2, (s_start + s_end) // 2
    position_distance = min(abs(c_start - s_start), abs(c_end - s_end), abs(center1 - center2)) / position_distance_normalizer
    return position_distance + abs(span1 - span2) / max(span1, span2)


def _engine(engine):
    if engine is not None:
        return engine
    from ._lib import engine as default_engine
    return default_engine()


def genotype(candidates, bam, type, options, engine=None, alignment_order="file"):
    """src/svim/SVIM_genotyping.py:34-93.  `type` is "DEL", "INV", "INS" or "DUP_INT" as at src/svim/svim:164-170.
    alignment_order="sort": `bam` may be in any record order (AlignmentIndex(order="sort")): the result is that of the coordinate-sorted file."""
    eng = _engine(engine)
    index = alignment_index(bam, alignment_order)
    if getattr(eng, "_svx_index_id", None) != id(index):
        eng.set_alignment_index(index)
        eng._svx_index_id = id(index)
    point = type in ("INS", "DUP_INT")
    todo = [c for c in candidates if not c.score < options.minimum_score]              # :38-39
    tid, start, end, moff, mnames, alt = [], [], [], [0], [], []
    name_ids = index.name_ids
    for c in todo:
        contig, s, e = c.get_destination() if point else c.get_source()               # :41-46
        if point:
            e = s
        tid.append(index.references.index(contig) if contig in index.references else -1)
        start.append(s)
        end.append(e)
        reads = set(sig.read for sig in c.members)                                     # :50
        alt.append(len(reads))
        ids = sorted(name_ids[r] for r in reads if r in name_ids)
        mnames.extend(ids)
        moff.append(len(mnames))
    ref = eng.genotype(1 if point else 0, tid, start, end, moff, np.asarray(mnames, dtype=np.int32), int(options.min_mapq)) if todo else []
    for c, n_alt, n_ref in zip(todo, alt, ref):
        n_ref = int(n_ref)
        total = n_alt + n_ref
        if total >= options.minimum_depth:                                             # :79-88
            c.support_fraction = n_alt / total
            if c.support_fraction >= options.homozygous_threshold:
                c.genotype = "1/1"
            elif c.support_fraction >= options.heterozygous_threshold:
                c.genotype = "0/1"
            elif c.support_fraction < options.heterozygous_threshold:
                c.genotype = "0/0"
            else:
                c.genotype = "./."
        elif total > 0:                                                                # :89-91
            c.support_fraction = n_alt / total
            c.genotype = "./."
        else:
            c.support_fraction = "."
            c.genotype = "./."
        c.ref_reads = n_ref
        c.alt_reads = n_alt


def genotype_calls(alt_reads, ref_reads, options):
    """The call of :77-93 from the two counts, as the table route states it: -> (genotype code of _abi.GT_NAMES, support_fraction or ".")."""
    total = alt_reads + ref_reads
    if total >= options.minimum_depth and total > 0:
        f = alt_reads / total
        return (3 if f >= options.homozygous_threshold else 2 if f >= options.heterozygous_threshold else 1 if f < options.heterozygous_threshold else 0), f
    if total > 0:
        return 0, alt_reads / total
    return 0, "."


def candidate_loci(table, minimum_score):
    """Class and score select of the table route (:38-46): -> (selected bool[n], mode int8[n] (0 = DEL / INV, 1 = INS / DUP_INT), tid, start, end int32[n]);
    rows that are not selected have tid -1."""
    from ._abi import CAND_DEL, CAND_INV, CAND_DUP_INT, CAND_INS
    cls = np.asarray(table.cls[:table.n])
    point = (cls == CAND_INS) | (cls == CAND_DUP_INT)
    sel = (point | (cls == CAND_DEL) | (cls == CAND_INV)) & ~(np.asarray(table.score[:table.n]) < minimum_score)
    tid = np.where(sel, np.where(point, table.contig2[:table.n], table.contig[:table.n]), -1).astype(np.int32)
    start = np.where(sel, np.where(point, table.start2[:table.n], table.start[:table.n]), 0).astype(np.int32)
    end = np.where(sel, np.where(point, start, table.end[:table.n]), 0).astype(np.int32)
    return sel, point.astype(np.int8), tid, start, end


def genotype_resident(engine, options, lengths):
    """genotype() for the deletion, inversion, novel insertion and interspersed duplication candidates resident in `engine` (its last combine() of resident
    clusters) against the alignment table it kept while the file was collected (Engine.keep_alignments / harness.BamPipeline(keep_alignments=True)).
    Nothing leaves the device but the four columns, which are returned (Engine.fetch_genotypes) and attached to the CandidateTable the engine handed out for
    that combine(): CandidateList objects built afterwards carry them, and write_final_vcf prints them from the device."""
    engine.genotype_resident(options, lengths)
    g = engine.fetch_genotypes()
    t = getattr(engine, "_resident_cand", None)
    if t is not None:
        t.genotypes = g
    return g
