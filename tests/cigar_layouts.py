"""Directed layouts for the CIGAR scan (k_scan_prepare / k_cigar_scan / k_emit_indels / k_gather_seq, svim_amd/csrc/collect.hip) and the plain expectation
they are held to.  No GPU needed: tests/test_cigar_layouts.py pins generator, expectation and the oracle's multi-record walk against each other on the CPU,
tests/test_gpu_cigar_layouts.py runs the same batches through Engine.collect.

A batch is described by a list of records (rec(...)); build() writes the arrays of a HostBatch directly - offsets, flags and operation words are exactly what
the case says, nothing goes through SAM text.  Every record gets a seeded SEQ, by default of the length its CIGAR consumes, so the bases of every reported
insertion are part of the expectation.

The expectation is the definition, with Python integers: walk() is analyze_cigar_indel (src/svim/SVIM_intra.py:8-30), geometry() the five numbers pysam
derives from a CIGAR (reference_length, query_alignment_start, query_alignment_end, infer_read_length, hard-clipped bases).
"""
import numpy as np

from svim_amd import _abi
from svim_amd.batch import HostBatch, SVX_FLAG_SA

M, I, D, N, S, H, P, EQ, X, B = range(10)
MIN_MAPQ = 20
L28 = (1 << 28) - 1                      # the longest operation a packed CIGAR word holds
WAVE_STRIDE_ONE_BLOCK_PER_CU = 1024      # waves of the scan's grid under SVX_SCAN_BLOCKS=1 on a 256-CU device
WAVE_STRIDE_DEFAULT = 8192               # the most waves the scan's grid ever has (RAW_SHARDS)


def w(op, length):
    return (length << 4) | op


def params(min_sv_size=40, all_bnds=False):
    return _abi.Params(MIN_MAPQ, int(min_sv_size), 100000, 10, 5, 1 if all_bnds else 0, 1000, 900.0, 1.0, 0.5)


# ---- the plain expectation ---------------------------------------------------------------------------------------------------------------------------------
def walk(ops, min_len):
    """analyze_cigar_indel: (op index, pos_ref, pos_read, length, is_del) of every I / D of at least min_len"""
    pr = pq = 0
    for k, word in enumerate(ops):
        op, l = word & 15, word >> 4
        if op in (M, EQ, X):
            pr += l
            pq += l
        elif op == I:
            if l >= min_len:
                yield (k, pr, pq, l, False)
            pq += l
        elif op == D:
            if l >= min_len:
                yield (k, pr, pq, l, True)
            pr += l
        elif op == S:
            pq += l


def geometry(ops, lseq):
    """(reference_length, query_alignment_start, query_alignment_end, infer_read_length or 0, hard-clipped bases) as pysam gives them"""
    pairs = [(word & 15, word >> 4) for word in ops]
    ref = sum(l for op, l in pairs if op in (M, D, N, EQ, X))
    read = sum(l for op, l in pairs if op in (M, I, S, H, EQ, X))
    hard = sum(l for op, l in pairs if op == H)
    qstart = 0
    for op, l in pairs:
        if op == H:
            continue
        if op != S:
            break
        qstart += l
    if lseq == 0:
        qend = 0
        for op, l in pairs:
            if op in (M, I, EQ, X) or (op == S and qend == 0):
                qend += l
    else:
        qend = lseq
        for op, l in reversed(pairs[1:]):
            if op == H:
                continue
            if op != S:
                break
            qend -= l
    return (ref if ref else 1, qstart, qend, read if pairs else 0, hard)


def consumed(ops):
    return sum(word >> 4 for word in ops if (word & 15) in (M, I, S, EQ, X))


def py_slice(a, b, n):
    return range(n)[a:b]


# ---- records and batches -------------------------------------------------------------------------------------------------------------------------------------
def rec(ops, flag=0, mapq=60, pos=1000, tid=0, lseq=None, rows=(), sa=True):
    """one BAM record; lseq None: a SEQ of the length the CIGAR consumes; rows: segment-table rows made by row(); sa: the rows were rebuilt from an SA tag"""
    return dict(ops=[int(x) for x in ops], flag=flag, mapq=mapq, pos=pos, tid=tid, lseq=lseq, rows=list(rows), sa=sa)


def row(ops, tid=0, pos=5000, rev=0, mapq=60, lseq=0):
    return dict(ops=[int(x) for x in ops], tid=tid, pos=pos, rev=rev, mapq=mapq, lseq=lseq)


def used(r):
    return not (r["flag"] & (_abi.SVX_FLAG_SKIP | 4 | 256)) and r["mapq"] >= MIN_MAPQ


def filtered(ops, k=0):
    """the same CIGAR on a record that COLLECT must not look at: by flag (unmapped, secondary, not the group's) or by mapping quality, in turn"""
    return rec(ops, **[dict(flag=4), dict(flag=256), dict(mapq=MIN_MAPQ - 1), dict(flag=_abi.SVX_FLAG_SKIP)][k % 4])


class Case(object):
    def __init__(self, name, recs, min_sv_size=40, seed=1, permute_order=False):
        self.name, self.recs, self.min_sv_size = name, recs, min_sv_size
        n = len(recs)
        rng = np.random.default_rng(seed)
        self.lseq = [consumed(r["ops"]) if r["lseq"] is None else r["lseq"] for r in recs]
        self.order = [2 * int(x) for x in (rng.permutation(n) if permute_order else range(n))]
        self.seq_off = [0]
        for l in self.lseq:
            self.seq_off.append(self.seq_off[-1] + (l + 1) // 2)
        self.seq = rng.integers(0, 256, size=max(1, self.seq_off[-1]), dtype=np.uint8)      # every code of the BAM alphabet; the spare nibble of an odd length is noise
        self._text = _abi.decode_bases(np.stack([self.seq >> 4, self.seq & 15], axis=1).reshape(-1))      # two symbols per byte, high nibble first

    def bases(self, r, a, b):
        """query_sequence[a:b] of record r"""
        sl = py_slice(a, b, self.lseq[r])
        return self._text[2 * self.seq_off[r] + sl.start:2 * self.seq_off[r] + sl.stop]

    def host_batch(self):
        recs, n = self.recs, len(self.recs)
        hb = HostBatch()
        hb.n_rec = n
        hb.references = ["chr1", "chr2"]
        hb.read_names = ["r%d" % i for i in range(n)]
        A = hb.arrays
        A["flag"] = np.array([r["flag"] for r in recs], dtype=np.uint16)
        for i, r in enumerate(recs):
            if r["rows"] and used(r) and not (r["flag"] & 2048) and r["sa"]:
                A["flag"][i] |= SVX_FLAG_SA
        A["tid"] = np.array([r["tid"] for r in recs], dtype=np.int32)
        A["pos"] = np.array([r["pos"] for r in recs], dtype=np.int32)
        A["mapq"] = np.array([r["mapq"] for r in recs], dtype=np.uint8)
        A["lseq"] = np.array(self.lseq, dtype=np.int32)
        A["read_id"] = np.arange(n, dtype=np.int32)
        A["order"] = np.array(self.order, dtype=np.uint32)
        A["seg_order"] = A["order"] + np.uint32(1)
        A["cigar_off"] = np.cumsum([0] + [len(r["ops"]) for r in recs]).astype(np.uint64)
        flat = [x for r in recs for x in r["ops"]]
        A["cigar"] = np.array(flat if flat else [0], dtype=np.uint32)
        A["seq_off"] = np.array(self.seq_off, dtype=np.uint64)
        A["seq"] = self.seq
        rows = [s for r in recs for s in r["rows"]]
        hb.n_seg = len(rows)
        A["seg_off"] = np.cumsum([0] + [len(r["rows"]) for r in recs]).astype(np.uint32)
        for k, dt in (("tid", np.int32), ("pos", np.int32), ("rev", np.uint8), ("mapq", np.uint8), ("lseq", np.int32)):
            A["seg_" + k] = np.array([s[k] for s in rows] or [0], dtype=dt)
        A["seg_cigar_off"] = np.cumsum([0] + [len(s["ops"]) for s in rows]).astype(np.uint64)
        sflat = [x for s in rows for x in s["ops"]]
        A["seg_cigar"] = np.array(sflat if sflat else [0], dtype=np.uint32)
        A["contig_rank"] = np.array([0, 1], dtype=np.int32)
        return hb

    # the tables of the definition: CIGAR-sourced rows only (what the split-read analysis adds is held to the reference by tests/segment_cases.py and its golden)
    def expect_rows(self, min_sv_size=None, all_bnds=False):
        """(main list, side list) as rows (key, type, contig, start, end, contig2, pos2, read_id, inserted bases), in key order"""
        m = self.min_sv_size if min_sv_size is None else min_sv_size
        main, side = [], []
        for r, rc in enumerate(self.recs):
            if not used(rc):
                continue
            for k, pr, pq, l, is_del in walk(rc["ops"], m):
                key = (self.order[r] << 32) | k
                s = rc["pos"] + pr
                if is_del:
                    main.append((key, _abi.SVX_DEL, rc["tid"], s, s + l, -1, 0, r, ""))
                    if all_bnds:
                        side.append((key, _abi.SVX_BND, rc["tid"], s, s + 1, rc["tid"], s + l, r, ""))
                else:
                    main.append((key, _abi.SVX_INS, rc["tid"], s, s + l, -1, 0, r, self.bases(r, pq, pq + l)))
        return sorted(main), sorted(side)

    def expect_geometry(self):
        """{item: five numbers} for the items COLLECT computes geometry for: records that are used, not supplementary and own rows; every row (item n_rec + s)"""
        out, s = {}, len(self.recs)
        for r, rc in enumerate(self.recs):
            if rc["rows"] and used(rc) and not (rc["flag"] & 2048):
                out[r] = geometry(rc["ops"], self.lseq[r])
            for sr in rc["rows"]:
                out[s] = geometry(sr["ops"], sr["lseq"])
                s += 1
        return out


def table_rows(t, cigar_only=True):
    """a SigTable as rows like Case.expect_rows (cigar_only: without the rows of the split-read analysis)"""
    seq = _abi.decode_bases(t.seq[:int(t.seq_off[t.n])])
    off = t.seq_off.tolist()
    cols = [getattr(t, k).tolist() for k in ("key", "type", "contig", "start", "end", "contig2", "pos2", "read_id")]
    src = t.src.tolist()
    return [row_ + (seq[off[i]:off[i + 1]],) for i, row_ in enumerate(zip(*cols)) if not cigar_only or src[i] == 0]


def first_row_difference(got, exp):
    if len(got) != len(exp):
        head = "%d rows, expected %d; " % (len(got), len(exp))
    else:
        head = ""
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:
            return head + "row %d: got %r, expected %r" % (i, a, b)
    if head:
        extra = got[len(exp):len(exp) + 1] or exp[len(got):len(got) + 1]
        return head + "first row without a partner: %r" % (extra[0],)
    return None


def geometry_difference(case, rec_geom, seg_geom):
    n = len(case.recs)
    for item, exp in sorted(case.expect_geometry().items()):
        got = tuple(int(x) for x in (rec_geom[item] if item < n else seg_geom[item - n]))
        if got != exp:
            return "%s %d: got %r, expected %r" % ("record" if item < n else "segment row", item if item < n else item - n, got, exp)
    return None


# ---- on the device, inside poisoned surroundings ---------------------------------------------------------------------------------------------------------
POISON_WORDS = 64                        # a multiple of four: the slice keeps the 16-byte alignment of the allocation


def poison(i):
    """a reportable operation nobody wrote into a case: an I or D of 0xBAD00 + i bases"""
    return w(I if i & 1 else D, 0xBAD00 + i)


def device_batch(hb, device="cuda"):
    """the same batch as torch tensors on the device (on_device = 1); the two CIGAR arrays are slices of larger tensors whose words before and behind are
    reportable operations: a read outside the arrays that leaks into a result shows as a signature no case expects"""
    import torch
    from svim_amd.devsynth import DeviceBatch
    db = DeviceBatch()
    db.n_rec, db.n_seg, db.n_contig = hb.n_rec, hb.n_seg, len(hb.references)
    db.references = hb.references
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    for k, a in hb.arrays.items():
        if k in ("cigar", "seg_cigar"):
            n_ops = int(hb.arrays[k + "_off"][-1])
            a = np.concatenate([np.array([poison(i) for i in range(POISON_WORDS)], dtype=np.uint32), a[:n_ops],
                                np.array([poison(POISON_WORDS + i) for i in range(POISON_WORDS)], dtype=np.uint32)])
            t = torch.from_numpy(a.view(np.int32)).to(device)
            db.t[k] = t[POISON_WORDS:POISON_WORDS + max(1, n_ops)] if n_ops else t[POISON_WORDS:POISON_WORDS + 1]
            db.t["_whole_" + k] = t
        else:
            a = np.ascontiguousarray(a)
            db.t[k] = torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).to(device)
    return db


# ---- families ------------------------------------------------------------------------------------------------------------------------------------------------
def _fill(n, seed, id_len=None, at=()):
    """n operations that advance both cursors by small odd amounts, with reportable operations of length id_len + position at the positions `at`"""
    rng = np.random.default_rng(seed)
    ops = [w((M, EQ, X, S, M, I, D, M)[int(c)], int(l)) for c, l in zip(rng.integers(0, 8, n), rng.integers(1, 9, n))]
    for j, k in enumerate(at):
        if 0 <= k < n:
            ops[k] = w(I if (k + j) & 1 else D, id_len + (k % 1000))
    return ops


def g1_cases():
    import helpers as Hh
    return Hh.load("g1_cigar_indel.json.gz")["cases"]


def g1_packed(lead, repeat=1, filter_every_third=False, seed=11):
    """all cases of the reference's analyze_cigar_indel golden as the records of ONE batch, behind a dummy record of `lead` operations: over lead 0-3 every
    case starts at every residue of its 16-byte word.  The list is rotated so that a short case (1-7 operations) is the last record of the array (the load
    that is moved back and shifted down, by another amount for every lead).  -> (Case, golden case index per record or None)"""
    cases = g1_cases()
    short = [i for i, c in enumerate(cases) if 1 <= len(c["tuples"]) <= 7]
    last = short[(11 * repeat + 3) % len(short)]
    idx = list(range(last + 1, len(cases))) + list(range(0, last + 1))
    recs, which = [rec([w(M, 5)] * lead, pos=77)], [None]
    for rep in range(repeat):
        for j, i in enumerate(idx):
            ops = [w(op, l) for op, l in cases[i]["tuples"]]
            pos = 1000 + 37 * ((rep * len(idx) + j) % 5003)
            if filter_every_third and (len(recs) % 3 == 0) and not (rep == repeat - 1 and j == len(idx) - 1):
                recs.append(filtered(ops, len(recs) // 3))
                recs[-1]["pos"] = pos
                which.append(None)
            else:
                recs.append(rec(ops, pos=pos))
                which.append(i)
    return Case("g1 packed lead %d x%d" % (lead, repeat), recs, seed=seed + lead, permute_order=bool(lead & 1)), which


def golden_rows_difference(case, which, got_rows, min_sv_size):
    """the rows of the records whose golden case was made with this min_length against the golden's own tuples moved by the record's pos"""
    cases = g1_cases()
    by_rec = {}
    for rw in got_rows:
        by_rec.setdefault(rw[7], []).append(rw)
    n_checked = 0
    for r, i in enumerate(which):
        if i is None or cases[i]["min_length"] != min_sv_size:
            continue
        pos = case.recs[r]["pos"]
        exp = [(_abi.SVX_DEL if t == "DEL" else _abi.SVX_INS, pos + pr, pos + pr + l, "" if t == "DEL" else case.bases(r, pq, pq + l)) for pr, pq, l, t in cases[i]["expect"]]
        got = [(rw[1], rw[3], rw[4], rw[8]) for rw in by_rec.get(r, [])]
        if got != exp:
            return "record %d (golden case %d): got %r, golden %r" % (r, i, got[:4], exp[:4])
        n_checked += 1
    assert n_checked > 0
    return None


GRID_LENGTHS = [n for c in (0, 252, 508, 764, 1020, 1532) for n in range(c, c + 9)]


def grid_cases(lengths=GRID_LENGTHS):
    """item length x lead x place in the array.  The item under test has reportable I / D at operations 0, 1, 255, 256, 257, 511, 512, 513, n-2, n-1 whose
    lengths (40000 + position) name it; the neighbours' border operations are reportable too, with lengths that name THEM (50000 + / 60000 +)."""
    out = []
    for n in lengths:
        at = (0, 1, 255, 256, 257, 511, 512, 513, n - 2, n - 1)
        item = _fill(n, 100 + n, 40000, at)
        for lead in range(4):
            before = _fill(4 + lead, 7 * n + lead, 50000, (0, 2 + lead, 3 + lead))           # 4 + lead operations: the next record starts at residue `lead`
            behind = _fill(6, 9 * n + lead, 60000, (0, 1, 5))
            for place in ("first", "middle", "last"):
                if place == "first":
                    if lead:
                        continue                                                                # the first record of an array starts at residue 0
                    recs = [rec(item, pos=3000), rec(behind, pos=9000)]
                elif place == "middle":
                    recs = [rec(before, pos=100), rec(item, pos=3000), rec(behind, pos=9000)]
                else:
                    recs = [rec(before, pos=100), rec(item, pos=3000)]
                out.append(Case("grid n=%d lead=%d %s" % (n, lead, place), recs, seed=n * 16 + lead))
    return out


def grid_batch(lengths=GRID_LENGTHS, repeat=3):
    """the grid once more as ONE batch of more items than a grid of one block per CU has waves: every (length, lead) item between two neighbours, each at
    some other place of a long array, several items to a wave"""
    recs, total = [], 0
    for rep_ in range(repeat):
        for n in lengths:
            for lead in range(4):
                at = (0, 1, 255, 256, 257, 511, 512, 513, n - 2, n - 1)
                pad = (lead - total) % 4
                recs.append(rec(_fill(4 + pad, 5 * n + lead + rep_, 50000, (0, 3 + pad)), pos=100))
                recs.append(rec(_fill(n, 300 + n + lead + 7 * rep_, 40000, at), pos=3000))
                total += 4 + pad + n
    return Case("grid as one batch", recs, seed=5)


def skip_cases():
    dense = [w(M, 3), w(I, 41), w(D, 42), w(I, 43)] * 3
    live = lambda k: rec(_fill(20 + k % 7, k, 40000, (0, 5, 19 + k % 7)), pos=1000 + k)      # noqa: E731
    out = []
    for stride in (WAVE_STRIDE_ONE_BLOCK_PER_CU, WAVE_STRIDE_DEFAULT):
        n = 3 * stride + 5
        # runs of filtered items longer than the wave stride: a wave's next, and next but one, item is filtered
        recs = [live(k) if (k < stride or k >= 3 * stride) else filtered(dense, k) for k in range(n)]
        out.append(Case("skips: run of %d filtered in the middle" % (2 * stride), recs, seed=stride))
        recs = [filtered(dense, k) if k < 2 * stride + 3 else live(k) for k in range(n)]
        out.append(Case("skips: the first %d filtered" % (2 * stride + 3), recs, seed=stride + 1))
        recs = [live(k) if k < stride - 3 else filtered(dense, k) for k in range(n)]
        out.append(Case("skips: all behind the first %d filtered" % (stride - 3), recs, seed=stride + 2))
    out.append(Case("skips: every item filtered", [filtered(dense, k) for k in range(2 * WAVE_STRIDE_ONE_BLOCK_PER_CU + 7)], seed=3))
    # empty CIGARs at the start, in the middle and at the very end (the last one at every residue of the array end)
    for lead in range(4):
        body = _fill(8 + lead, 40 + lead, 40000, (0, 7 + lead))
        recs = [rec([]), rec([]), rec(body), rec([]), rec(_fill(4, 50 + lead, 40000, (3,))), rec([]), rec([])]
        out.append(Case("skips: empty CIGARs, array of %d operations" % (12 + lead), recs, seed=60 + lead))
    return out


def tiny_cases():
    out = []
    shapes = [[0], [1], [2], [3], [0, 0], [1, 0], [0, 1], [1, 1], [2, 1], [1, 2], [0, 3], [3, 0], [0, 0, 0], [1, 1, 1], [1, 0, 2], [0, 2, 0], [2, 0, 1]]
    for sh in shapes:
        recs = [rec([w((I, D, I)[j], 41 + 10 * k + j) for j in range(n)], pos=500 * (k + 1)) for k, n in enumerate(sh)]
        out.append(Case("tiny %s" % "+".join(map(str, sh)), recs, seed=sum(sh) * 8 + len(sh)))
    return out


def opcode_cases(repeat=1):
    """(Case, min_sv_size) pairs: N, P, B, the undefined codes 10-15 and zero-length operations beside reportable ones; I / D one below, at and far above the
    threshold; thresholds 0, 1, 40, 2^28 and 2^28 + 1"""
    quiet = [w(op, l) for op in (N, P, B, 10, 11, 12, 13, 14, 15, H) for l in (0, 1, 39, 40, 41, 5000)]
    recs = []
    for lead in range(4 * repeat):
        recs.append(rec([w(M, 7)] * ((lead - sum(len(r["ops"]) for r in recs)) % 4 + 4), pos=50))
        ops = []
        for j, q in enumerate(quiet):
            ops += [q, w((I, D)[j & 1], 39 + j % 3), w(M, 0), w(I, 0), w(D, 0), w(S, 0), w(EQ, 3), q]
        recs.append(rec(ops, pos=2000))
        recs.append(rec(quiet * 5, pos=2500))                                              # several chunks of nothing to report
        recs.append(rec([w(I, 0)] * 3 + [w(D, 0)] * 3 + [w(N, 41)] * 3, pos=2600))
    # the longest lengths: one per record (sums stay below 2^31), the insertion with a SEQ far shorter than it claims
    recs.append(rec([w(M, 9), w(D, L28), w(M, 5), w(I, 44), w(D, 39)], pos=10))
    recs.append(rec([w(S, 3), w(I, L28), w(M, 5), w(D, 45)], pos=20, lseq=50))
    recs.append(rec([w(EQ, L28), w(X, 11), w(I, 40), w(D, 40)], pos=30, lseq=0))
    recs.append(rec([w(S, L28), w(I, 41), w(M, 2)], pos=40, lseq=7))
    recs.append(rec([w(N, L28), w(B, L28), w(P, L28), w(15, L28), w(D, 40), w(I, 39)], pos=60))
    return [(Case("operation codes and lengths", recs, seed=21), m) for m in (0, 1, 40, 1 << 28, (1 << 28) + 1)]


def insertion_case():
    """k_gather_seq: insertions of 1, 7, 8, 15, 16, 17, 127, 128, 129 bases at odd and even read positions, the last of each record ending at the read's
    last base; with SEQ absent and shorter than the CIGAR says"""
    recs = []
    lens = (1, 7, 8, 15, 16, 17, 127, 128, 129)
    for start in (0, 1, 2, 5):
        ops = [w(S, start)] if start else []
        for j, l in enumerate(lens):
            ops += [w(I, l), w(M, 1 + (j & 1))]
        for l in lens:
            recs.append(rec(ops + [w(I, l)], pos=100 * start + l))
    recs.append(rec([w(M, 5), w(I, 9), w(M, 5)], lseq=0))
    recs.append(rec([w(M, 5), w(I, 9), w(M, 5)], lseq=10))
    recs.append(rec([w(M, 5), w(I, 9), w(M, 5)], lseq=3))
    return Case("inserted bases", recs, min_sv_size=1, seed=31)


def segment_cases():
    """rows of 1 .. 514 operations at every residue, every combination of leading / trailing H and S, N inside, stored length 0 and not; primaries that own
    rows (their geometry comes from the scan) next to primaries that do not.  min_sv_size is large: the tables hold what the split-read analysis decides
    from the geometry - compared with the oracle here; the decision tree itself is held to the reference's outputs by tests/segment_cases.py - and the CIGAR-sourced
    rows of the definition."""
    clips = [[], [w(H, 3)], [w(S, 4)], [w(H, 3), w(S, 4)], [w(S, 4), w(H, 3)], [w(H, 0), w(S, 0)], [w(H, 2), w(H, 1), w(S, 2), w(S, 5)]]
    sizes = (1, 2, 31, 32, 33, 34, 255, 256, 257, 258, 511, 512, 513, 514)

    def body(n, seed):
        rng = np.random.default_rng(seed)
        ops = [w((M, I, D, N, EQ, X, M, P)[int(c)], int(l)) for c, l in zip(rng.integers(0, 8, n), rng.integers(0, 30, n))]
        return ops

    def shaped(n, a, b, seed):
        """n operations: clips `a`, a body, clips `b` reversed (as many clip operations as fit)"""
        a, b = a[:n], list(reversed(b))
        b = b[:max(0, n - len(a))]
        return a + body(n - len(a) - len(b), seed) + b

    cases = []
    for lead in range(4):
        recs, k = [], 0
        for n in sizes:
            rows = []
            for ia, a in enumerate(clips):
                for ib, b_ in enumerate(clips):
                    if n > 34 and (ia + ib + n) % 3:                                            # the long rows: a third of the combinations each
                        continue
                    ops = shaped(n, a, b_, 1000 * n + 10 * ia + ib)
                    rows.append(row(ops, tid=(ia + ib) & 1, pos=4000 + 13 * len(rows), rev=(ia ^ ib) & 1, mapq=(60, 60, 5)[(ia + ib) % 3],
                                    lseq=0 if (ia + ib + n) & 1 else max(1, consumed(ops))))
            # pad the row array so that this record's rows start at residue (lead + k) % 4
            prim = shaped(40 + n % 5, clips[k % 7], clips[(k + 3) % 7], n) if k % 2 == 0 else shaped(300 + n, clips[(k + 1) % 7], clips[k % 7], n + 1)
            recs.append(rec(prim, pos=2000 + n, flag=16 * (k & 1), rows=rows, lseq=0 if k % 4 == 3 else None, sa=k % 3 != 0))
            recs.append(rec(body(5 + (lead + k) % 4, n + 7), pos=2500 + n))                     # a primary without rows: its geometry is never asked for
            k += 1
        # clips only, a single operation, an empty CIGAR, a supplementary record (rows are not its to own), a filtered primary that owns rows
        odd = [row([w(S, 5)]), row([w(H, 5)]), row([w(S, 5), w(H, 2)], rev=1), row([w(H, 1), w(S, 2), w(S, 3), w(H, 4)], lseq=5), row([]), row([], rev=1),
               row([w(M, 50)], rev=1, lseq=50), row([w(N, 9)]), row([w(D, 9)], rev=1), row([w(M, 0)], rev=1), row([w(S, 0), w(M, 9), w(S, 7)], lseq=0),
               row([w(M, 0), w(S, 6), w(I, 4), w(S, 2)], lseq=0, rev=1)]
        recs.insert(0, rec([w(S, 7)] * lead, pos=10))                                           # the records' CIGAR array: everything behind starts at residue lead
        recs.append(rec([w(S, 10), w(M, 100), w(S, 20)], pos=7000, rows=odd))
        recs.append(rec([w(S, 30), w(S, 30)], pos=7100, rows=odd[:3], lseq=0))
        recs.append(rec([w(M, 30)], pos=7200, rows=odd[3:5]))
        recs.append(rec([], pos=7300, rows=odd[5:8]))
        recs.append(rec([w(H, 10), w(M, 100)], pos=7400, rows=odd[8:10]))                       # hard-clipped primary with an SA tag: the rebuild is void
        recs.append(rec([w(M, 100), w(S, 9)], pos=7500, flag=2048, rows=[]))
        recs.append(filtered([w(M, 100), w(S, 9)], 2))
        recs[-1]["rows"] = odd[10:]
        # the segment-row array too starts its rows at every residue: a leading row of `lead` operations on the first primary that owns rows
        recs[1]["rows"].insert(0, row([w(M, 11)] * lead, pos=4500))
        cases.append(Case("segment rows lead %d" % lead, recs, min_sv_size=40, seed=70 + lead))
    return cases


def segment_cases_combined():
    """the four batches as one: more items than a grid of one block per CU has waves"""
    return Case("segment rows, all leads in one batch", [r for c in segment_cases() for r in c.recs], min_sv_size=40, seed=75)


def dense_read(k, seed=0):
    """a CIGAR with k reportable operations (every other operation; I and D by turns) """
    ops = []
    for j in range(k):
        ops += [w(M, 3 + (j + seed) % 5), w((I, D)[(j + seed) & 1], 40 + (j % 9))]
    return ops + [w(M, 6)]


CAPACITY_K = (16, 17, 18, 64, 65, 66, 256, 257, 258, 1000, 5000)


def capacity_case(k):
    return Case("capacity: one read with %d reportable operations" % k, [rec(dense_read(k), pos=123)], seed=k)


def capacity_limit_case(k=53000):
    """a batch that fills the scan's largest grid, one of its reads with more reportable operations than the regions of that grid may grow to hold"""
    recs = [rec([w(M, 50)], pos=10 * j) for j in range(WAVE_STRIDE_DEFAULT + 8)]
    recs[77] = rec(dense_read(k), pos=50)
    return Case("capacity: %d reportable operations in one read of a full grid" % k, recs, seed=9)


def capacity_pair_case(k=300, stride=WAVE_STRIDE_ONE_BLOCK_PER_CU):
    """two dense reads `stride` items apart - the same wave takes both when the grid has that many waves - among records with little to report"""
    recs = [rec([w(M, 50), w(D, 40 + j % 3), w(M, 50)], pos=10 * j) for j in range(2 * stride + 1)]
    recs[5] = rec(dense_read(k, 1), pos=50)
    recs[5 + stride] = rec(dense_read(k + 7, 2), pos=51)
    return Case("capacity: two reads with %d and %d reportable operations, %d items apart" % (k, k + 7, stride), recs, seed=k + 1)
