"""Directed cases for the insertion haplotypes of CLUSTER (csrc/edit.hip: record_hap / k_hap_pack / PairSource::views / k_edit_prep, csrc/cluster.hip:
ins_needs_edit) and the definition they are held to, in plain words.  tests/golden/make_golden_hap.py runs the reference on them
(tests/golden/g_hap_cases.json.gz), tests/test_hap_cases.py holds the oracle and the definition to that file on the CPU, tests/test_gpu_hap_cases.py the device.

THE DEFINITION (compute_haplotype_edit_distance and the INS branch of span_position_distance, SVIM_clustering.py:32-45 and :64-77).  Two insertion signatures
s1, s2 (contig, start, end, inserted sequence).  The window is [min(start) - 100, max(start) + 100).  The haplotype of a signature is the contig from the window's
start to the signature's start, the inserted sequence, and the contig from the signature's start to the window's end - every bound first raised to 0, the slice
then cut at the contig's end the way a Python slice is, everything upper-cased; each signature reads ITS OWN contig.  span = end - start (not the sequence's
length).  position distance = |start1 - start2| / normalizer.  When that is > 2 * cluster_max_distance the result is position distance + |span1 - span2| /
max(span); otherwise it is position distance + edit distance of the two haplotypes / max(span) / edit_distance_normalizer.  Every `/` is one FP64 division.

THE GENOME (seeded, ~65 kb): `big` (20 kb: the large shifts), `far` (40.3 kb: only the normalizer-40000 threshold needs it), contigs of 1, 5, 7, 8, 9, 99, 100,
101, 199, 200, 201 and 300 bases, `lower` (lower-case stretches), `nrun` (an N run of 150 and of 1, a few IUPAC codes) and `absent`, a name the references list
and the genome does not hold (length 0: every fetch is empty).

THE FAMILIES: one table of signature rows (golden row layout; a DEL, INV or BND row between every few insertions - the haplotype store skips them and its word
offsets must survive that) and the pairs to ask for, each (i, j, tag, (normalizer, edit_normalizer, cluster_max_distance)).

    start_edge  starts 0, 1, 7, 8, 9, 50, 99, 100, 101, 150 among each other and with starts up to 250 further right, both orders; on `big` and on L300 (both clips)
    end_edge    on every contig length: starts clen, clen-1, clen-7..clen-9, clen-99..clen-101 among each other, both orders, and with starts up to 250 further left
    tiny        contigs of <= 9 bases and the absent one, inserted lengths 0, 1, 2, 7, 8, 9: haplotypes of 0..8 symbols and longer, both empty, span != len(sequence)
    nibble      every (start mod 8, start difference 0..8): a related pair and an identical inserted sequence - every nibble offset of both cores; common prefix /
                suffix ending at a piece border and at 128 and 256 symbols; one core a prefix / suffix of the other; equal haplotypes
    shift       related insertions 1 .. 16500 bases apart (2047 / 2048: the clamp of the shift in the class word; 15898..16000: the prepack limit), either one
                first in the table, either one the shorter; long insertions at 2046..2049 (the cheap alignment really runs 2 * shift off the diagonal)
    threshold   seven (normalizer, cluster_max_distance) settings, start differences floor(2 * cmd * normalizer) + {-1, 0, 1, 2}
    alphabet    clean insertions beside the N run (left flank only, right flank only, outside the window but inside the record's radius), N and = inside the
                inserted sequence, lower-case flank and lower-case inserted bases, IUPAC codes in the flank
    cross_contig  two contigs in one pair: the only pairs whose distance depends on the window padding (see cross_contig)
    cluster     partitions of 3..60 insertions across a contig start or end, on the short contigs, beside the N run (for the CLUSTER route)

Test infrastructure only; imports no GPU code."""
import hashlib
import json
import math
import random

PAD = 100
DEFAULT = (900, 1.0, 0.5)
SHORT = (1, 5, 7, 8, 9, 99, 100, 101, 199, 200, 201, 300)
START_EDGE = (0, 1, 7, 8, 9, 50, 99, 100, 101, 150)
SHIFTS = (1, 31, 32, 33, 99, 100, 101, 500, 2046, 2047, 2048, 2049, 3000, 15897, 15898, 15899, 15999, 16000, 16500)
THRESHOLDS = ((900, 0.5), (900, 0.3), (900, 0.7), (1, 0.5), (3, 0.35), (7, 0.45), (40000, 0.5))
N_RUN = (400, 550)            # the long N run of `nrun`
OPTIONS = {"min_mapq": 20, "min_sv_size": 40, "max_sv_size": 100000, "segment_gap_tolerance": 10, "segment_overlap_tolerance": 5, "partition_max_distance": 1000,
           "position_distance_normalizer": 900, "edit_distance_normalizer": 1.0, "cluster_max_distance": 0.5, "all_bnds": False}


def rseq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def noisy(rng, s, rate=0.04):
    """a copy with `rate` substitutions, insertions and deletions (a third each)"""
    out = []
    for ch in s:
        r = rng.random()
        if r >= rate:
            out.append(ch)
        elif r < rate / 3:
            out.append(rng.choice("ACGT"))
        elif r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
            out.append(ch)
    return "".join(out)


def other(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


def make_genome(n_run=N_RUN):
    rng = random.Random(20240917)
    g = {"big": rseq(rng, 20000), "far": rseq(rng, 40300)}
    for n in SHORT:
        g["L%d" % n] = rseq(rng, n)
    low = list(rseq(rng, 700))
    for a, b in ((0, 40), (95, 130), (300, 301), (420, 700)):
        low[a:b] = [c.lower() for c in low[a:b]]
    g["lower"] = "".join(low)
    nr = list(rseq(rng, 1200))
    nr[n_run[0]:n_run[1]] = "N" * (n_run[1] - n_run[0])
    nr[700] = "N"
    for p, c in ((900, "R"), (905, "y"), (910, "K"), (1100, "M"), (1199, "n")):
        nr[p] = c
    g["nrun"] = "".join(nr)
    return g


REFERENCES = ["far", "big", "L300", "absent", "L1", "L5", "L7", "L8", "L9", "nrun", "L99", "L100", "L101", "L199", "L200", "L201", "lower"]      # not in string order
GENOME = make_genome()
assert set(REFERENCES) - set(GENOME) == {"absent"}


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------------------
def haplotypes(genome, s1, s2):
    """s = (contig, start, end, sequence) -> the two strings compute_haplotype_edit_distance aligns"""
    ws = min(s1[1], s2[1]) - PAD
    we = max(s1[1], s2[1]) + PAD
    out = []
    for contig, start, _, seq in (s1, s2):
        ref = genome.get(contig, "")
        left = ref[max(0, ws):max(0, start)].upper()
        right = ref[max(0, start):max(0, we)].upper()
        out.append(left + seq.upper() + right)
    return out[0], out[1]


def needs_edit(s1, s2, params):
    return not (abs(s1[1] - s2[1]) / params[0] > 2 * params[2])


def distance(genome, s1, s2, params, ed):
    """INS branch of span_position_distance in Python floats; ed = edit distance of haplotypes(genome, s1, s2), used only when needs_edit"""
    normalizer, edit_normalizer, cmd = params
    span1, span2 = s1[2] - s1[1], s2[2] - s2[1]
    pd = abs(s1[1] - s2[1]) / normalizer
    if pd > 2 * cmd:
        return pd + abs(span1 - span2) / max(span1, span2)
    return pd + ed / max(span1, span2) / edit_normalizer


def sig(row):
    assert row[0] == "INS"
    return (row[1], row[2], row[3], row[6])


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------------------------
class Table(object):
    """rows in the golden layout with a non-insertion row after every third insertion"""

    def __init__(self, name, seed):
        self.name, self.rows, self.pairs, self.rng, self.n_ins = name, [], [], random.Random(seed), 0

    def ins(self, contig, start, seq, span=None):
        assert 0 <= start <= len(GENOME.get(contig, "")), (self.name, contig, start)
        span = len(seq) if span is None else span
        k = len(self.rows)
        self.rows.append(["INS", contig, start, start + span, "cigar" if k % 2 else "suppl", "%s_r%d" % (self.name, k), seq])
        self.n_ins += 1
        if self.n_ins % 3 == 0:
            self.other_row(contig, start)
        return k

    def other_row(self, contig, start):
        k = len(self.rows)
        rd = "%s_r%d" % (self.name, k)
        which = self.n_ins // 3 % 3
        if which == 0:
            self.rows.append(["DEL", contig, start, start + 60 + k % 7, "cigar", rd])
        elif which == 1:
            self.rows.append(["INV", contig, start, start + 500, "suppl", rd, ("left_fwd", "right_rev")[k % 2]])
        else:
            self.rows.append(["BND", contig, start, "fwd", "big", 12000 + k, "rev", "suppl", rd])

    def pair(self, i, j, tag, params=DEFAULT, both=True):
        self.pairs.append((i, j, tag, tuple(params)))
        if both:
            self.pairs.append((j, i, tag + " swapped", tuple(params)))

    def digest(self):
        return hashlib.sha256(json.dumps([self.rows, [list(p[:3]) + [list(p[3])] for p in self.pairs]], separators=(",", ":")).encode()).hexdigest()


def rows_digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


def allele(rng, n):
    return rseq(rng, n)


def start_edge():
    t = Table("start_edge", 1)
    for contig in ("big", "L300"):
        base = allele(t.rng, 90)
        clen = len(GENOME[contig])
        near = [t.ins(contig, s, noisy(t.rng, base)[:60 + s % 13]) for s in START_EDGE]
        for a in range(len(near)):
            for b in range(a + 1, len(near)):
                t.pair(near[a], near[b], "%s %d/%d" % (contig, START_EDGE[a], START_EDGE[b]))
        for a, s in enumerate(START_EDGE):
            for d in (0, 1, 57, 100, 199, 250):
                if s + d <= clen:
                    k = t.ins(contig, s + d, noisy(t.rng, base)[:70])
                    t.pair(near[a], k, "%s %d/+%d" % (contig, s, d))
    return t


def end_edge():
    t = Table("end_edge", 2)
    for contig in ["L%d" % n for n in SHORT] + ["big", "lower", "far"]:
        clen = len(GENOME[contig])
        base = allele(t.rng, 80)
        starts = sorted({clen - d for d in (0, 1, 7, 8, 9, 99, 100, 101) if clen - d >= 0})
        near = [t.ins(contig, s, noisy(t.rng, base)[:50 + (clen - s) % 11]) for s in starts]
        for a in range(len(near)):
            for b in range(a + 1, len(near)):
                t.pair(near[a], near[b], "%s clen-%d/clen-%d" % (contig, clen - starts[a], clen - starts[b]))
        for a, s in enumerate(starts):
            for d in (0, 63, 250):
                if s - d >= 0 and clen > 9:
                    k = t.ins(contig, s - d, noisy(t.rng, base)[:64])
                    t.pair(near[a], k, "%s clen-%d/-%d" % (contig, clen - s, d), both=(d != 63))
    return t


def tiny():
    t = Table("tiny", 3)
    for contig in ("L1", "L5", "L7", "L8", "L9", "absent"):
        clen = len(GENOME.get(contig, ""))
        ids = []
        for s in sorted({0, clen // 2, clen}):
            for n, ln in enumerate((0, 1, 2, 7, 8, 9)):
                span = ln + (0, 1, 3)[(n + s) % 3]
                ids.append(t.ins(contig, s, rseq(t.rng, ln, "ACGTAC"), span=max(1, span)))
        for a in range(len(ids)):
            for b in range(a + 1, len(ids)):
                t.pair(ids[a], ids[b], "%s %d+%d/%d+%d" % (contig, t.rows[ids[a]][2], len(t.rows[ids[a]][6]), t.rows[ids[b]][2], len(t.rows[ids[b]][6])), both=((a + b) % 3 == 0))
    # each signature reads its own contig: two contigs in one pair (never formed by CLUSTER, answered all the same)
    a, b = t.ins("L9", 4, "ACGTACG"), t.ins("L5", 3, "ACGTAC")
    t.pair(a, b, "L9/L5")
    more = [t.ins("absent", 0, rseq(t.rng, ln)) for ln in (3, 4, 5, 6)]          # with the lengths above: every haplotype length 0..10 without a flank
    for x in range(4):
        for y in range(x + 1, 4):
            t.pair(more[x], more[y], "absent 0+%d/0+%d" % (3 + x, 3 + y), both=(x == 0))
    a = t.ins("absent", 0, "")
    t.pair(a, t.ins("absent", 0, "", span=2), "absent empty/empty")
    return t


ZERO_SPAN = [["INS", "L9", 3, 3, "cigar", "z0", ""], ["INS", "L9", 4, 4, "cigar", "z1", "ACG"]]      # max(span) = 0: the reference divides by it
EXPECTED_RAISES = {"zero_span 0/1": "ZeroDivisionError"}


def nibble():
    t = Table("nibble", 4)
    for origin in (1000, 0):
        for r in range(8):
            base = allele(t.rng, 280 + 3 * r)
            s1 = origin + r
            a = t.ins("big", s1, base)
            for d in range(9):
                b = t.ins("big", s1 + d, noisy(t.rng, base))
                t.pair(a, b, "related start %d +%d" % (s1, d))
                c = t.ins("big", s1 + d, base)
                t.pair(a, c, "identical start %d +%d" % (s1, d), both=(d % 2 == 0))
    # common prefix / suffix of a given length: same start 1003 (left flank 100, right flank 100), the inserted sequences agree on `keep` symbols from one end
    for keep in (0, 1, 27, 28, 29, 155, 156, 157):
        for end in ("prefix", "suffix"):
            base = allele(t.rng, 300)
            cut = keep if end == "prefix" else len(base) - keep - 1
            var = base[:cut] + other(base[cut]) + base[cut + 1:]
            # and a second difference in the middle, so that prefix and suffix do not meet
            mid = 200 if end == "prefix" else 100
            var = var[:mid] + other(var[mid]) + var[mid + 1:]
            a, b = t.ins("big", 1003, base), t.ins("big", 1003, var)
            t.pair(a, b, "%s %d" % (end, 100 + keep))
    base = allele(t.rng, 200)
    a = t.ins("big", 1500, base)
    t.pair(a, t.ins("big", 1500, base[:120]), "one a prefix of the other")
    t.pair(a, t.ins("big", 1500, base[77:]), "one a suffix of the other")
    t.pair(a, t.ins("big", 1500, base), "equal haplotypes")
    t.pair(a, t.ins("big", 1500, ""), "against the bare window")
    return t


def shift():
    t = Table("shift", 5)
    k = 0
    for d in SHIFTS:
        params = [DEFAULT] if d <= 900 else []
        params.append((d + 37, 1.0, 0.5))
        if d > 900:
            params.append((40000, 1.5, 0.5))
        for variant in range(4):
            base = allele(t.rng, 260 + 5 * variant)
            short = noisy(t.rng, base)[:len(base) - 31]
            early, late = (base, short) if variant & 1 else (short, base)          # which one is the shorter core
            s1 = (1500, 40, 1203, 20000 - d)[variant]                                # (variant 1: the left flank is clipped; 3: the later one AT the contig end)
            s2 = s1 + d
            if variant & 2:                                                         # the later insertion first in the table
                b = t.ins("big", s2, late); a = t.ins("big", s1, early)
            else:
                a = t.ins("big", s1, early); b = t.ins("big", s2, late)
            t.pair(a, b, "shift %d variant %d" % (d, variant), params[k % len(params)], both=(d < 3000 or variant == 0))
            k += 1
    for d in (2046, 2047, 2048, 2049):
        base = allele(t.rng, 4400)
        a, b = t.ins("big", 700, base), t.ins("big", 700 + d, noisy(t.rng, base, 0.02))
        t.pair(a, b, "long insertion shift %d" % d, (d + 37, 1.0, 0.5) if d % 2 else (40000, 1.0, 0.5))
    return t


def threshold():
    t = Table("threshold", 6)
    for normalizer, cmd in THRESHOLDS:
        contig = "far" if normalizer == 40000 else "big"
        edge = int(math.floor(2 * cmd * normalizer))
        base = allele(t.rng, 120)
        s1 = 150 if normalizer == 40000 else 3000
        a = t.ins(contig, s1, base)
        for d in sorted({max(0, edge + x) for x in (-1, 0, 1, 2)}):
            b = t.ins(contig, s1 + d, noisy(t.rng, base)[:100 + d % 17])
            t.pair(a, b, "normalizer %r cmd %r delta %d" % (normalizer, cmd, d), (normalizer, 1.0, cmd))
    return t


def alphabet():
    t = Table("alphabet", 7)
    n0, n1 = N_RUN
    base = allele(t.rng, 90)
    for tag, s1, s2 in (("N run in the left flank only", n1 + 10, n1 + 20), ("N run in the right flank only", n0 - 20, n0 - 10),
                        ("N run outside the window, inside the record radius", n0 - 200, n0 - 190), ("N run inside the window of one pair of the call", n0 - 200, n0 - 1),
                        ("single N and IUPAC codes", 690, 905), ("contig end with n", 1150, 1199)):
        a, b = t.ins("nrun", s1, base), t.ins("nrun", s2, noisy(t.rng, base))
        t.pair(a, b, tag)
    for tag, mut in (("N inside the inserted sequence", lambda s: s[:40] + "N" + s[41:]), ("= inside the inserted sequence", lambda s: s[:17] + "=" + s[17:]),
                     ("lower-case inserted bases", lambda s: s[:30].lower() + s[30:]), ("IUPAC inside the inserted sequence", lambda s: s[:8] + "RYKMSW" + s[8:])):
        a, b = t.ins("big", 5000, mut(base)), t.ins("big", 5003, noisy(t.rng, base))
        t.pair(a, b, tag)
        a, b = t.ins("big", 5000, mut(base)), t.ins("big", 5000, mut(base))
        t.pair(a, b, tag + ", twice")
    for s1, s2 in ((10, 30), (100, 128), (295, 310), (415, 425), (600, 700)):
        a, b = t.ins("lower", s1, base.lower()), t.ins("lower", s2, noisy(t.rng, base))
        t.pair(a, b, "lower-case flank %d/%d" % (s1, s2))
    return t


def alphabet_routing():
    """A clean pair table on `nrun` ([start 150 and 160] + [150 and 250]: record radius 200 in a call of its own) and three genomes: the N run just OUTSIDE the
    radius of every record (no record is flagged: the A,C,G,T kernels), just INSIDE the radius of the last record but outside every window (flagged: the generic
    kernels, the same strings), and far away.  -> (table, {name: genome})"""
    t = Table("alphabet_routing", 8)
    base = allele(t.rng, 150)
    a, b, c = t.ins("nrun", 150, base), t.ins("nrun", 160, noisy(t.rng, base)), t.ins("nrun", 250, noisy(t.rng, base))
    t.pair(a, b, "near")
    t.pair(a, c, "radius 200")
    t.pair(b, c, "90 apart")
    genomes = {}
    for name, at in (("outside", 450), ("inside", 449), ("far", 800)):      # records reach to start + 200 = 450 (exclusive); the windows to 350
        g = make_genome((at, at + 150))
        nr = list(g["nrun"])
        for p in range(0, 449):
            if nr[p] not in "ACGT":
                nr[p] = "A"
        nr[700] = "A" if at == 450 else nr[700]
        g["nrun"] = "".join(nr)
        genomes[name] = g
    assert genomes["outside"]["nrun"][:449] == genomes["inside"]["nrun"][:449] and genomes["inside"]["nrun"][449] == "N" and genomes["outside"]["nrun"][449] in "ACGT"
    return t, genomes


def cross_contig():
    """Two contigs in one pair.  CLUSTER never forms such a pair, the distance function answers it all the same (each signature reads its own contig) - and it is
    the only kind of pair that can see the window padding: on ONE contig both haplotypes begin with the same symbol ref[window start] and end with the same
    symbol ref[window end - 1], and a symbol that both strings begin or end with never changes their edit distance."""
    t = Table("cross_contig", 9)
    base = allele(t.rng, 70)
    for (c1, s1), (c2, s2) in ((("big", 1000), ("far", 1000)), (("big", 1000), ("far", 1007)), (("far", 2000), ("big", 1990)), (("L300", 150), ("big", 160)),
                               (("nrun", 300), ("lower", 310)), (("L99", 50), ("L101", 60)), (("big", 5), ("far", 3)), (("far", 40290), ("L300", 295)),
                               (("L200", 100), ("L201", 100)), (("absent", 0), ("L9", 4))):
        a, b = t.ins(c1, s1, base), t.ins(c2, s2, noisy(t.rng, base))
        t.pair(a, b, "%s %d/%s %d" % (c1, s1, c2, s2))
    return t


def families():
    return [start_edge(), end_edge(), tiny(), nibble(), shift(), threshold(), alphabet(), cross_contig()]


# ---- CLUSTER route ----------------------------------------------------------------------------------------------------------------------------------------------
def cluster_cases():
    """[(name, rows, options)]: one partition's worth of insertions each (plus the non-insertion rows), two or three alleles so that clusters form and split"""
    out = []

    def case(name, contig, starts, n, seed, opts=None, n_alleles=2, length=80, same_read_every=0):
        t = Table(name, seed)
        alleles = [allele(t.rng, length + 9 * k) for k in range(n_alleles)]
        for m in range(n):
            s = t.rng.choice(starts) if not isinstance(starts, range) else t.rng.randrange(starts.start, starts.stop)
            k = t.ins(contig, s, noisy(t.rng, alleles[m % n_alleles]))
            if same_read_every and m % same_read_every == same_read_every - 1:
                t.rows[k][5] = t.rows[k - 1][5] if t.rows[k - 1][0] == "INS" else t.rows[k][5]
        out.append((name, t.rows, dict(OPTIONS, **(opts or {}))))

    big = len(GENOME["big"])
    case("three at the start", "big", (0, 7, 40), 3, 11)
    case("sixty across the start", "big", range(0, 151), 60, 12, same_read_every=7)
    case("twenty at the end", "big", range(big - 120, big + 1), 20, 13)
    case("forty at the end, three alleles", "big", range(big - 101, big + 1), 40, 14, n_alleles=3, opts={"cluster_max_distance": 0.3})
    case("both clips", "L300", range(0, 301), 25, 15)
    case("contig of 100", "L100", range(0, 101), 12, 16, opts={"position_distance_normalizer": 450, "edit_distance_normalizer": 1.5, "cluster_max_distance": 0.7})
    case("contig of 9", "L9", range(0, 10), 6, 17, length=8)
    case("contig of 1", "L1", (0, 1), 4, 18, length=5)
    case("beside the N run", "nrun", range(N_RUN[0] - 120, N_RUN[1] + 120), 30, 19)
    case("lower-case contig end", "lower", range(560, 701), 15, 20)
    case("small normalizer at the start", "big", range(0, 12), 10, 21, opts={"position_distance_normalizer": 7, "cluster_max_distance": 0.45})
    return out


def absent_cluster_case():
    t = Table("absent", 22)
    alleles = [allele(t.rng, 70), allele(t.rng, 75)]
    for m in range(9):
        t.ins("absent", t.rng.randrange(0, 1), noisy(t.rng, alleles[m % 2]))
    return ("absent contig", t.rows, dict(OPTIONS))


def all_insertions_table():
    """every family's rows in one table (the cluster cases' too), read names made unique"""
    rows = []
    for t in families():
        rows += t.rows
    for name, r, _ in cluster_cases():
        rows += r
    return [list(r) for r in rows]
