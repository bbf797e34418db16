"""Shared by the tests of the alignment table in any record order (tests/test_aln_order.py, tests/test_gpu_aln_order.py): the builders of the cases, the
definition's permutation taken from svim_amd/bamsort.py itself, and rows handed to the engine as record batches without a file in between.

The order under test is bamsort.py's coordinate order - key (uint32(refID), uint32(pos + 1), flag & 16), stable - so the alignment table of a file in any
order is by definition that of sort_bam(file)."""
import random
import struct

import numpy as np

from svim_amd import _abi, bamsort, records, synth
from svim_amd.batch import HostBatch, contig_ranks

# the sort's own edges: RADIX_TILE 2048, the one-workgroup form up to 16 384 pairs, PM_TILE 2048; 150 500: many tiles
SIZES = (0, 1, 2, 2047, 2048, 2049, 16384, 16385, 150500)
KINDS = ("one_key", "sorted", "reversed", "one_contig", "contigs300", "unplaced", "pos0", "placed_unmapped")


def definition_permutation(tid, pos, flag):
    """bamsort.permutation over records that hold nothing but the three fields: the file index of every row of the sorted order"""
    recs = [struct.pack("<Iii6xH16x", 32, int(t), int(p), int(f)) for t, p, f in zip(tid, pos, flag)]
    return np.asarray(bamsort.permutation(recs), dtype=np.int64)


def rows(n, kind="random", seed=0):
    """n alignment rows in append order -> dict(references, lengths, tid, pos, flag, mapq, span, read_id); every row is one M operation of `span` bases.
    Positions are dense, so equal keys are everywhere and only a stable sort by the full key gives the definition's order."""
    rng = np.random.RandomState(1000 + seed)
    n_contig = {"one_contig": 1, "contigs300": 300}.get(kind, 3)
    tid = rng.randint(0, n_contig, n).astype(np.int32)
    pos = rng.randint(0, 3 if kind == "pos0" else 4000, n).astype(np.int32)
    flag = rng.choice(np.array([0, 16, 0, 16, 256, 4, 2048, 2064], dtype=np.uint16), n).astype(np.uint16)
    mapq = rng.choice(np.array([60, 60, 60, 20, 19, 0], dtype=np.uint8), n).astype(np.uint8)
    span = rng.randint(1, 5000, n).astype(np.int32)
    read_id = rng.randint(0, max(1, n // 2), n).astype(np.int32)
    if kind == "one_key":
        tid[:], pos[:], flag[:] = 1, 777, rng.choice(np.array([0, 256, 2048], dtype=np.uint16), n)
    if kind == "placed_unmapped":
        flag[rng.rand(n) < 0.4] |= 4
    if kind == "unplaced":                                     # records without a reference, interleaved: they sort behind every contig
        u = rng.rand(n) < 0.3
        tid[u], pos[u] = -1, np.where(rng.rand(int(u.sum())) < 0.5, -1, 5)
        flag[u] |= 4
    if kind in ("sorted", "reversed"):
        p = definition_permutation(tid, pos, flag)
        if kind == "reversed":
            p = p[::-1]
        tid, pos, flag, mapq, span, read_id = tid[p], pos[p], flag[p], mapq[p], span[p], read_id[p]
    return dict(references=["c%d" % k for k in range(n_contig)], lengths=[200000] * n_contig, tid=tid, pos=pos, flag=flag, mapq=mapq, span=span, read_id=read_id)


class Row(object):
    """what SVIM_genotyping.AlignmentIndex reads of a record"""
    __slots__ = ("reference_id", "reference_start", "flag", "mapping_quality", "query_name", "span")

    def __init__(self, *a):
        self.reference_id, self.reference_start, self.flag, self.mapping_quality, self.query_name, self.span = a

    @property
    def cigartuples(self):
        return [(0, self.span)]

    @property
    def reference_end(self):
        return self.reference_start + self.span


class RowFile(object):
    def __init__(self, r, order=None):
        self.references, self.lengths = r["references"], r["lengths"]
        idx = range(len(r["tid"])) if order is None else order
        cols = [r[k].tolist() for k in ("tid", "pos", "flag", "mapq", "read_id", "span")]
        self.rows = [Row(cols[0][i], cols[1][i], cols[2][i], cols[3][i], "r%d" % cols[4][i], cols[5][i]) for i in idx]

    def fetch(self, until_eof=True):
        return iter(self.rows)


def rows_batch(r, lo, hi):
    """rows [lo, hi) as the record batch the Python batcher makes of such records in coordinate mode (batch.build_batch): no SEQ, no segments"""
    n = hi - lo
    hb = HostBatch()
    hb.n_rec, hb.n_seg, hb.references = n, 0, list(r["references"])
    A = hb.arrays
    A["flag"], A["tid"], A["pos"], A["mapq"] = [np.ascontiguousarray(r[k][lo:hi]) for k in ("flag", "tid", "pos", "mapq")]
    A["lseq"], A["read_id"] = np.zeros(max(1, n), np.int32), np.ascontiguousarray(r["read_id"][lo:hi])
    A["order"], A["seg_order"] = (2 * np.arange(max(1, n))).astype(np.uint32), (2 * np.arange(max(1, n)) + 1).astype(np.uint32)
    A["cigar_off"], A["seq_off"], A["seg_off"] = np.arange(n + 1, dtype=np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    A["cigar"] = np.concatenate([(r["span"][lo:hi].astype(np.uint32) << 4), np.zeros(1, np.uint32)])
    A["seq"] = np.zeros(1, np.uint8)
    for k in ("seg_tid", "seg_pos", "seg_lseq"):
        A[k] = np.zeros(1, np.int32)
    A["seg_rev"], A["seg_mapq"] = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    A["seg_cigar_off"], A["seg_cigar"] = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    A["contig_rank"] = contig_ranks(hb.references)
    for k, dt in _abi.BATCH_DTYPES.items():
        assert A[k].dtype == dt, (k, A[k].dtype, dt)
    return hb


def text_file(references, lengths, rws, sort_order="unsorted"):
    """rows [name, flag, tid, pos, mapq, ref_len] -> records.AlignmentFile over SAM text, in the rows' order"""
    text = synth.genotype_sam_text(references, lengths, rws).replace("SO:coordinate", "SO:%s" % sort_order, 1)
    return records.AlignmentFile(text=text)


# ---- the tie pile at the 500-alignment cap ----------------------------------------------------------------------------------------------------------------
def tie_pile():
    """One INS candidate at chr1:50000.  499 eligible records at 49000 .. 49498 (50M: they count, none supports the reference), then three at 49600 in
    append order B (reverse, 1500M: spans the locus), A (forward, 100M), C (forward, 1500M), then three more.  The coordinate order puts forward records
    first: A, C, B - A is the 500th alignment and the walk ends: ref_reads 0.  With ties in append order (or a key of (tid, pos) alone) B is the 500th:
    ref_reads 1.  -> (references, lengths, rows in append order, candidate)"""
    rws = [["pile%03d" % k, 0, 0, 49000 + k, 60, 50] for k in range(499)]
    rws += [["B", 16, 0, 49600, 60, 1500], ["A", 0, 0, 49600, 60, 100], ["C", 0, 0, 49600, 60, 1500]]
    rws += [["after%d" % k, 0, 0, 49700 + k, 60, 50] for k in range(3)]
    return ["chr1"], [120000], rws, ("INS", "chr1", 50000, 50040, ["alt1", "alt2", "alt3"], 10)


# ---- the golden's rows, shuffled --------------------------------------------------------------------------------------------------------------------------
SHUFFLE_SEEDS = (0, 1, 2, 3, 4)


def shuffled(rws, seed):
    out = list(rws)
    random.Random(seed).shuffle(out)
    return out


# ---- records of whole reads: COLLECT finds signatures in them (test_gpu_genotype_resident._seeded_records, rebuilt) -------------------------------------
def seeded_records():
    """-> (references, lengths, reference sequences, records in coordinate order (synth.coordinate_sort))"""
    contigs = [("chr1", 120000), ("chrE", 30000), ("chr2", 50000)]
    references, lengths = [c[0] for c in contigs], [c[1] for c in contigs]
    refs = synth.make_reference(3, contigs)
    recs = synth.planted_reads(5, 500, refs, references, lengths, n_sites=30, types=("DEL", "INS", "INV"))
    recs += synth.planted_reads(9, 120, refs, references, lengths, n_sites=8, types=("DEL", "INS"), tid=2)
    recs += synth.fuzz_split_reads(6, 80, references, lengths)
    rws = [r for r in synth.genotype_rows(31, lengths, n_reads=1800, hot=((0, 60000, 900), (2, 300, 300), (2, 49700, 300))) if r[2] != 1]
    recs += list(records.AlignmentFile(text=synth.genotype_sam_text(references, lengths, rws)).fetch(until_eof=True))
    return references, lengths, refs, synth.coordinate_sort(recs)


def name_order(recs):
    """records in query-name order (svim_amd/bamsort.py: name, then READ1 / READ2, primary < secondary < supplementary; stable)"""
    return sorted(recs, key=lambda a: (a.query_name.encode(), bamsort.name_rank(a.flag)))


def shuffled_records(recs, seed=7):
    out = list(recs)
    random.Random(seed).shuffle(out)
    return out


# ---- directed groups for the flag rule --------------------------------------------------------------------------------------------------------------------
def flag_groups():
    """One DEL candidate chr1:10000-10400 and read groups in query-name order.  Five plain reads span it.  Three groups the query-name front end does not
    analyse - every record of them leaves it with SVX_FLAG_SKIP - hold records genotype() counts all the same (src/svim/SVIM_genotyping.py:64-65 looks at
    the record alone):
      g1  a primary at mapq 5 and its supplementary at mapq 60, which spans the candidate
      g2  two primaries, both spanning
      g3  a good primary elsewhere and a supplementary at mapq 15 that spans: below COLLECT's min_mapq 20, above a genotype call's min_mapq 10
    -> (references, lengths, rows in name order, candidate, {min_mapq: ref_reads})"""
    span = lambda name, flag, mapq, pos=9000: [name, flag, 0, pos, mapq, 3000]      # noqa: E731
    rws = [span("a_plain%d" % k, 16 * (k & 1), 60, 9000 + 10 * k) for k in range(5)]
    rws += [["g1", 0, 0, 30000, 5, 500], span("g1", 2048, 60)]
    rws += [span("g2", 0, 60, 9100), span("g2", 16, 60, 9200)]
    rws += [["g3", 0, 0, 40000, 60, 500], span("g3", 2048, 15, 9300)]
    rws += [["z_far", 0, 0, 70000, 60, 500]]
    # reads, not records, are counted: g2's two primaries are one read
    return ["chr1"], [120000], rws, ("DEL", "chr1", 10000, 10400, ["alt1", "alt2"], 10), {20: 5 + 2, 10: 5 + 3}
