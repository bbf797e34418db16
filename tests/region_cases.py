"""Cases for region reads (svim_amd/regions.py, csrc/region_core.hpp, the readers of csrc/bamio.cpp and csrc/bamdev.hip): the fourteen corner files of
tests/bai_cases.py, each with sixty seeded regions, and directed regions on bin_edges and cg_tag_long_cigar.  tests/test_regions.py holds the definition and
the host reader to them on the CPU, tests/test_gpu_regions.py the device reader on the GPU.

    seeded     bai_cases.regions(5, rows, n_ref, 60) per file: most around the rows' own intervals, some anywhere, some on the 16 kb window edges
    directed   beg or end equal to a record's pos, pos + 1, interval end and interval end +- 1; a region inside the N skip of the thousand-window record;
               beg = 0; end = the contig's length; two regions that abut; two that overlap; one on a reference without records; one behind the last record

Test infrastructure only."""
import bai_cases as BC
from svim_amd import bai, regions as RG

N_SEEDED = 60
DIRECTED_FILES = ("bin_edges", "cg_tag_long_cigar")


class Case(object):
    """one corner file: its rows (bai.rows_of_bam), the bytes of its .bai and .csi by the definition, and its region sets (each a list of (tid, beg, end))"""

    def __init__(self, name, path):
        from svim_amd import csi
        self.name, self.path = name, path
        self.n_ref, self.rows, self.v_end = bai.rows_of_bam(path)
        self.bai = bai.build_index(self.n_ref, self.rows, self.v_end)
        self.csi = csi.build_bam_index(self.n_ref, self.rows, self.v_end)
        self.row_of_vbeg = {r[4]: k for k, r in enumerate(self.rows)}
        self.region_sets = [[g] for g in BC.regions(5, self.rows, self.n_ref, N_SEEDED) if g[0] < self.n_ref]
        if name in DIRECTED_FILES:
            self.region_sets += directed(self.rows, self.n_ref)


def directed(rows, n_ref):
    """the directed region sets of a file whose header is bai_cases.REFS / LENS"""
    placed = [r for r in rows if r[0] >= 0]
    out = []
    picks = placed[:6] + placed[-4:] + [r for r in placed if bai.interval(r)[1] - bai.interval(r)[0] > (500 << 14)]
    for r in picks:
        tid, (lo, hi) = r[0], bai.interval(r)
        for edge in (lo, lo + 1, hi - 1, hi, hi + 1):
            if edge > 0:
                out.append([(tid, max(0, edge - 300), edge)])              # end on the edge
            out.append([(tid, edge, edge + 300)])                           # beg on the edge
            out.append([(tid, edge, edge + 1)])
    for r in placed:                                                        # inside the N skip of the record over a thousand windows
        lo, hi = bai.interval(r)
        if hi - lo > (500 << 14):
            mid = lo + (hi - lo) // 2
            out.append([(r[0], mid, mid + 10)])
            out.append([(r[0], mid, mid + (3 << 14))])
    used = sorted({r[0] for r in placed})
    last = placed[-1]
    t = last[0]
    out.append([(t, 0, 1)])                                                 # beg = 0
    out.append([(t, 0, BC.LENS[t])])                                        # the whole contig
    out.append([(t, max(0, last[1] - 50), BC.LENS[t])])                     # end = the contig's length
    first = placed[0]
    a = max(first[1], 0)
    out.append([(first[0], max(0, a - 10), a + 1), (first[0], a + 1, a + 500)])              # two that abut
    out.append([(first[0], max(0, a - 10), a + 200), (first[0], a + 100, a + 5000)])         # two that overlap
    out.append([(t, bai.interval(last)[1] + 1000, bai.interval(last)[1] + 2000)])           # behind the last record
    empty = [k for k in range(n_ref) if k not in used]
    if empty:
        out.append([(empty[0], 0, BC.LENS[empty[0]])])                      # a reference without records
        out.append([(empty[-1], 100, 200)])
    out.append([(first[0], max(0, a - 10), a + 200), (t, 0, BC.LENS[t])] if first[0] != t else [(t, 0, 5), (t, max(last[1], 6), BC.LENS[t])])
    return out


def build_all(dirpath):
    """-> [Case] for the fourteen corner files, written into dirpath"""
    return [Case(name, path) for name, path in BC.build_all(dirpath)]


def expected(case, region_set, rule):
    """per normalised region of the set, what a reader hands out when it follows regions.plan: [(region, voff or None, first row, stop row, kept flags)] - the
    run of rows [first, stop) and which of them the rule keeps; voff None: the index proves the region empty (nothing is read)"""
    out = []
    planned = {(t, b, e): v for v, t, b, e in RG.plan(case.bai, region_set, rule)}
    for g in RG.normalise(region_set):
        voff = planned.get(g)
        if voff is None:
            out.append((g, None, 0, 0, []))
            continue
        (first, stop), kept = RG.run(case.rows, g, rule, case.row_of_vbeg[voff])
        out.append((g, voff, first, stop, kept))
    return out


def census(case):
    """-> (region sets that keep a record, sets with a marked record between kept ones, sets where the two rules keep different records)"""
    keep = marked = differ = 0
    for rs in case.region_sets:
        ov, st = RG.select(case.rows, rs, RG.RULE_OVERLAP), RG.select(case.rows, rs, RG.RULE_START)
        keep += bool(ov)
        differ += ov != st
        hit = False
        for rule in RG.RULES:
            for _g, voff, _first, _stop, kept in expected(case, rs, rule):
                if voff is not None and kept and not all(kept[:len(kept) - kept[::-1].index(True)]):
                    hit = True
        marked += hit
    return keep, marked, differ


# ---- what a reader handed out, as one table ---------------------------------------------------------------------------------------------------------------
SKIP = 0x8000


def read_table(bam, batch_records=1 << 22, min_mapq=20):
    """every batch the handle gives from where it stands to its end-of-file, as one table (the columns of the batches concatenated, offsets turned into
    per-record lengths, read ids into names)"""
    import numpy as np
    parts = []
    while True:
        b, n = bam.read_batch(batch_records, min_mapq)
        if n == 0:
            break
        parts.append(bam.batch_arrays(b))
    names = bam.read_names()

    def cat(k, dt):
        return np.concatenate([A[k] for A in parts]) if parts else np.zeros(0, dt)
    T = {k: cat(k, np.int64) for k in ("flag", "tid", "pos", "mapq", "lseq", "cigar", "seq", "seg_tid", "seg_pos", "seg_rev", "seg_mapq", "seg_lseq", "seg_cigar")}
    for k, off in (("n_cigar", "cigar_off"), ("n_seq", "seq_off"), ("n_seg", "seg_off"), ("n_seg_cigar", "seg_cigar_off")):
        T[k] = np.concatenate([np.diff(A[off].astype(np.int64)) for A in parts]) if parts else np.zeros(0, np.int64)
    T["name"] = [names[i] for A in parts for i in A["read_id"]]
    return T


def _take(values, counts, a, b):
    import numpy as np
    off = np.concatenate([[0], np.cumsum(counts)])
    return values[int(off[a]):int(off[b])]


def table_slice(T, a, b, kept=None):
    """records [a, b) of a table; kept: per record of the slice whether the rule keeps it (SVX_FLAG_SKIP is or-ed into the others)"""
    import numpy as np
    S = {k: T[k][a:b].copy() for k in ("flag", "tid", "pos", "mapq", "lseq", "n_cigar", "n_seq", "n_seg")}
    S["name"] = T["name"][a:b]
    S["cigar"], S["seq"] = _take(T["cigar"], T["n_cigar"], a, b), _take(T["seq"], T["n_seq"], a, b)
    seg_off = np.concatenate([[0], np.cumsum(T["n_seg"])])
    s0, s1 = int(seg_off[a]), int(seg_off[b])
    for k in ("seg_tid", "seg_pos", "seg_rev", "seg_mapq", "seg_lseq"):
        S[k] = T[k][s0:s1]
    S["n_seg_cigar"] = T["n_seg_cigar"][s0:s1]
    S["seg_cigar"] = _take(T["seg_cigar"], T["n_seg_cigar"], s0, s1)
    if kept is not None:
        S["flag"] = (S["flag"] | np.where(np.asarray(kept, dtype=bool), 0, SKIP).astype(S["flag"].dtype))
    return S


def first_difference(got, want):
    """None, or the name of the first column in which two tables differ"""
    import numpy as np
    for k in sorted(want):
        if k == "name":
            if list(got[k]) != list(want[k]):
                return k
        elif not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return k
    return None


def check_reader(case, whole, open_reader, rule):
    """every region set of the case through seek_region on a handle from open_reader(path): per planned region the handle gives exactly the run of
    expected(), the marked records flagged, and region_stats counts it.  whole: read_table of a pass over the whole file by the same kind of reader.
    -> (runs read, runs that held a marked record)"""
    bam = open_reader(case.path)
    n_runs = n_marked = 0
    try:
        for rs in case.region_sets:
            for g, voff, first, stop, kept in expected(case, rs, rule):
                if voff is None:
                    continue
                bam.seek_region(voff, g[0], g[1], g[2], rule)
                got = read_table(bam)
                want = table_slice(whole, first, stop, kept)
                d = first_difference(got, want)
                assert d is None, (case.name, g, rule, d, len(got["tid"]), stop - first)
                st = bam.region_stats()
                assert st["n_kept"] == sum(kept) and st["n_marked"] == len(kept) - sum(kept), (case.name, g, rule, st)
                start = case.row_of_vbeg[voff]
                assert st["n_seen"] == next((k for k in range(start, len(case.rows)) if RG.stops(case.rows[k], g)), len(case.rows)) - start, (case.name, g, rule, st)
                assert bam.read_batch(100, 20)[1] == 0                      # the end of a region stays its end
                n_runs += 1
                n_marked += bool(kept) and not all(kept)
    finally:
        bam.close()
    return n_runs, n_marked
