"""k_edit_prep's bound pass in deep trips (csrc/edit.hip: bound_at, SVX_EDIT_PREP_DEPTH) on a real MI355X (`-m gpu`): distances against the oracle, and the
same call with depth 1 (the loop of rounds 1-6) - equal distances AND equal routing (word-columns issued, band word-columns, the per-call guess): a changed
upper bound or core boundary sends a pair to another class and shows there.

The pairs: cores (what is left behind the common prefix and suffix) of every length around the trip edges - 8 symbols per lane, 128 per first trip, 512 per deep
trip of depth 4 - first trips with 32 and 33 mismatches (the give-up threshold), one long pair among three short ones in a wave of four and the reverse, every
nibble offset of both cores, and for signature pairs position shifts that send the pass through bound_at(0, shift) / bound_at(shift, 0).  Calls of more than
4096 pairs: the pilot and the band route are in play."""
import random

import numpy as np
import pytest

import helpers as H
from svim_amd import _abi, batch, convert

pytestmark = pytest.mark.gpu

CORES = (1, 7, 8, 127, 128, 129, 511, 512, 513, 640, 1023, 1024, 1025, 2049)
SHIFTS = (0, 1, 7, 8, 99, 700)           # 700: larger than the shorter core of the pairs it is used with
DEPTHS = ("1", "2", "4", "8")
STATS = ("n_edit_wordcols_issued", "n_edit_wordcols_band", "edit_guess")
FLOOR = 4096


def rseq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(ch, alphabet="ACGT"):
    return alphabet[(alphabet.index(ch) + 1) % len(alphabet)] if ch in alphabet else "A"


def related(rng, core, n_first, n_rest, alphabet):
    """a copy of `core` with exactly n_first substitutions among its first 128 symbols and n_rest behind them; the first and the last symbol always differ
    (they end the common prefix and suffix), counted in n_first / n_rest where they fall"""
    c = list(core)
    n = len(c)
    head = min(n, 128)
    must = {0} | ({n - 1} if n - 1 < head else set())
    first = set(must)
    while len(first) < min(max(n_first, len(must)), head):
        first.add(rng.randrange(head))
    rest = set()
    if n > head:
        rest.add(n - 1)
        while len(rest) < min(max(n_rest, 1), n - head):
            rest.add(rng.randrange(head, n))
    for p in first | rest:
        c[p] = other(c[p]) if alphabet == "ACGT" or rng.random() < 0.8 else "N"
        if c[p] == core[p]:
            c[p] = other(core[p])
    return "".join(c)


def trimmed(a, b):
    """(prefix, core of a, core of b) as k_edit_prep trims: the common prefix first, then the common suffix of what is left"""
    mn = min(len(a), len(b))
    pre = 0
    while pre < mn and a[pre] == b[pre]:
        pre += 1
    suf = 0
    while suf < mn - pre and a[len(a) - 1 - suf] == b[len(b) - 1 - suf]:
        suf += 1
    return pre, len(a) - pre - suf, len(b) - pre - suf


def plain_pairs(alphabet):
    rng = random.Random(41 if alphabet == "ACGT" else 43)
    groups = []                                   # waves of four work items

    def pair(core_len, n_first, n_rest, prefix, gap=0):
        p, s = rseq(rng, prefix), rseq(rng, rng.choice((0, 3, 40)))
        core = rseq(rng, core_len, alphabet if alphabet == "ACGT" else "ACGTACGTACGTN")
        twin = related(rng, core, n_first, n_rest, alphabet)
        if gap:                                   # the longer core: `gap` more symbols in front of its last one
            twin = twin[:-1] + rseq(rng, gap) + twin[-1]
        a, b = p + core + s, p + twin + s
        return (a, b) if rng.random() < 0.5 else (b, a)

    singles = []
    for k, c in enumerate(CORES):
        for prefix in range(8):                   # the core starts at nibble `prefix` of its word
            singles.append(pair(c, 1 + (k + prefix) % 20, (k * 3 + prefix) % 9, prefix + 8 * (prefix % 3)))
        singles.append(pair(c, 5, 3, 2, gap=rng.choice((1, 9, 130))))
    for c in (129, 513, 1025, 2049):              # both sides of the give-up threshold: more than 32 mismatches among the first 128 symbols
        for n_first in (31, 32, 33, 34, 90):
            singles.append(pair(c, n_first, 4, 5))
    while len(singles) % 4:
        singles.append(pair(60, 3, 0, 1))
    groups += [singles[i:i + 4] for i in range(0, len(singles), 4)]
    for long_len in (513, 640, 1025, 2049):       # one long pair among three short ones, at every place of the wave; and the reverse
        for place in range(4):
            groups.append([pair(long_len, 6, 9, 3) if q == place else pair(rng.choice((7, 40, 120)), 2, 0, q) for q in range(4)])
            groups.append([pair(rng.choice((1, 100, 128)), 2, 0, q) if q == place else pair(long_len + q, 7, 11, 4) for q in range(4)])
    pairs = [p for g in groups for p in g]
    assert all(len(g) == 4 for g in groups)
    short = [pair(rng.choice((30, 64, 100)), rng.choice((1, 2, 5)), 0, rng.randrange(8)) for _ in range(64)]
    k = 0
    while len(pairs) < FLOOR + 40:                # the floor: copies of short pairs (the oracle sees each once)
        pairs.append(short[k % len(short)])
        k += 1
    pairs.append(pair(1025, 6, 9, 3))             # its second string is the last record of the store: the deep trips end where the store does
    return pairs


CONTIG = "chrP"
CONTIG_LEN = 9000


def signature_case(alphabet):
    """insertions on one contig and the pairs to ask for: cores seq1 + ref[s1:s2] and ref[s1:s2] + seq2 behind the trimming"""
    rng = random.Random(47 if alphabet == "ACGT" else 53)
    ref = rseq(rng, CONTIG_LEN)
    rows, pairs = [], []

    def ins(start, seq):
        rows.append(["INS", CONTIG, start, start + len(seq), "cigar", "r%d" % len(rows), seq])
        return len(rows) - 1

    def pair(core_len, shift, n_first, n_rest, extend, start):
        s1, s2 = start, start + shift
        between = ref[s1:s2]
        seq_len = max(1, core_len + extend - shift)       # `extend` symbols go to the prefix: the cores keep core_len
        seq2 = rseq(rng, seq_len)
        want = between + seq2                       # the later insertion's core; the earlier one's is seq1 + between
        n = len(want)
        # seq1 + between related to want, the first `extend` symbols equal (the prefix grows by them: every nibble offset), then a difference
        twin = list(related(rng, want[extend:], n_first, n_rest, alphabet)) if n > extend else []
        cand = list(want[:extend]) + twin
        seq1 = "".join(cand[:seq_len])
        if seq1 and want and len(seq1) > extend and seq1[extend] == want[extend]:
            seq1 = seq1[:extend] + other(want[extend]) + seq1[extend + 1:]
        if seq2[-1] == ref[s2 - 1]:
            seq2 = seq2[:-1] + other(seq2[-1])
        i, j = ins(s1, seq1), ins(s2, seq2)
        pairs.append((i, j) if rng.random() < 0.5 else (j, i))

    groups = 0
    for k, c in enumerate(CORES):
        for shift in SHIFTS:
            if shift >= c and shift != 700:
                continue
            for extend in ((k + shift) % 8, (k + shift + 3) % 8):
                pair(c if shift != 700 else max(c, 701), shift, 2 + k % 12, k % 7, extend, 1000 + 13 * k + 8 * groups % 64)
                groups += 1
    for j in range(8):                              # nibble offsets of the two cores: (R + j) and (R - shift + j) mod 8 with the records' radius R
        for shift in range(8):
            pair(300, shift, 4, 3, j, 3000 + 16 * j)
    for shift, short_len in ((700, 50), (99, 40), (8, 7)):      # a shift larger than the shorter core: the earlier insertion repeats the bases between the two starts
        s1 = 4000 + shift
        i = ins(s1, ref[s1:s1 + shift] + rseq(rng, 300))
        tail = rseq(rng, short_len)
        j = ins(s1 + shift, other(ref[s1 + shift]) + tail[1:-1] + other(ref[s1 + shift - 1]))
        pairs += [(i, j), (j, i)]
    for c in (513, 1025):                           # the give-up threshold through the shifted bound
        for n_first in (32, 33, 34):
            pair(c, 99, n_first, 4, 0, 5000)
    for long_len in (640, 2049):                    # one long pair among three short ones and the reverse
        while len(pairs) % 4:
            pair(50, 1, 2, 0, 0, 6000)
        for place in range(4):
            for q in range(4):
                pair(long_len if q == place else 60, 7, 5, 6 if q == place else 0, q, 6000 + 40 * q)
        for place in range(4):
            for q in range(4):
                pair(40 if q == place else long_len + q, 8, 5, 6, q, 7000 + 40 * q)
    pair(600, 50, 3, 2, 0, CONTIG_LEN - 60)         # ends in the last record of the store (the last row of the table), 10 bases before the contig's end
    designed = len(pairs)
    short = list(pairs[-17:-1]) + [(0, 1), (2, 3)]
    k = 0
    while len(pairs) < FLOOR + 40:
        pairs.append(short[k % len(short)])
        k += 1
    return ref, rows, pairs, designed


def haplotypes(ref, r1, r2):
    """the two strings compute_haplotype_edit_distance aligns for two insertion rows on the contig `ref` (window: the starts -+ 100)"""
    ws, we = max(0, min(r1[2], r2[2]) - 100), max(r1[2], r2[2]) + 100
    return ref[ws:r1[2]] + r1[6] + ref[r1[2]:we], ref[ws:r2[2]] + r2[6] + ref[r2[2]:we]


def deltas(eng, before):
    st = eng.stats()
    return tuple(st[k] - before[k] if k != "edit_guess" else st[k] for k in STATS), st


@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTN"])
def test_plain_pairs_at_every_depth_vs_oracle(oracle, monkeypatch, alphabet):
    from svim_amd._lib import Engine
    pairs = plain_pairs(alphabet)
    cores = {min(trimmed(a, b)[1:]) for a, b in pairs}
    assert set(CORES) <= cores, sorted(set(CORES) - cores)
    assert {trimmed(a, b)[0] & 7 for a, b in pairs} == set(range(8))          # (plain strings start their records: both cores sit at the nibble of the prefix)
    assert min(trimmed(*pairs[-1])[1:]) == 1025
    memo = {}
    exp = [memo.setdefault(p, oracle.edit_distance(*p)) if p not in memo else memo[p] for p in pairs]
    eng = Engine(0)
    try:
        seen = {}
        for depth in DEPTHS:
            monkeypatch.setenv("SVX_EDIT_PREP_DEPTH", depth)
            before = eng.stats()
            got = eng.edit_distances(pairs)
            seen[depth], _ = deltas(eng, before)
            bad = [(i, g, e, trimmed(*pairs[i])) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
            assert not bad, (depth, bad[:5])
        print("routing per depth:", seen)
        assert all(seen[d] == seen["1"] for d in DEPTHS), seen
        assert seen["1"][0] > 0
    finally:
        eng.close()


@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTN"])
def test_signature_pairs_with_shifts_at_every_depth_vs_oracle(oracle, monkeypatch, alphabet):
    from svim_amd._lib import Engine
    import types
    ref, rows, pairs, designed = signature_case(alphabet)
    tab, contigs, reads = convert.sigtable_from_objects([H.row_sig(r) for r in rows], convert.Interner([CONTIG]))
    off, codes = convert.genome_arrays({CONTIG: ref.encode("ascii")}, [CONTIG])
    # normalizer 40000: every pair's position distance is far below 2 * cluster_max_distance, so every pair takes the edit distance
    p = _abi.Params.from_options(types.SimpleNamespace(position_distance_normalizer=40000, edit_distance_normalizer=1.0, cluster_max_distance=0.5))
    shifts = {abs(int(tab.start[i]) - int(tab.start[j])) for i, j in pairs[:designed]}
    assert set(SHIFTS) <= shifts
    assert max(max(i, j) for i, j in pairs[:designed]) == tab.n - 1          # a pair ends in the last record of the store
    shape = [(abs(rows[i][2] - rows[j][2]), min(trimmed(*haplotypes(ref, rows[i], rows[j]))[1:])) for i, j in pairs[:designed]]
    assert set(CORES) <= {m for _, m in shape} and any(shift > m > 0 for shift, m in shape)
    # nibble offsets of the two cores: every record of an insertion inside the contig carries the same number of bases in front of its start, so behind a common
    # prefix of `pre` symbols the earlier insertion's core sits at (constant + pre) and the later one's at (constant + pre - shift) - every pair of offsets 0..7
    offsets = {(trimmed(*haplotypes(ref, rows[i], rows[j]))[0] & 7, abs(rows[i][2] - rows[j][2]) & 7) for i, j in pairs[:designed]}
    assert offsets == {(a, b) for a in range(8) for b in range(8)}, sorted({(a, b) for a in range(8) for b in range(8)} - offsets)
    oracle.set_genome(off, codes)
    memo = {}
    exp = []
    for i, j in pairs:
        if (i, j) not in memo:
            memo[(i, j)] = oracle.span_position_distance(tab, i, j, p)
        exp.append(memo[(i, j)])
    eng = Engine(0)
    try:
        eng.set_genome(off, codes)
        seen, dist = {}, {}
        for depth in DEPTHS:
            monkeypatch.setenv("SVX_EDIT_PREP_DEPTH", depth)
            before = eng.stats()
            dist[depth] = np.array(eng.pair_distances(tab, pairs, p))
            seen[depth], _ = deltas(eng, before)
            bad = [(k, pairs[k], float(g), e) for k, (g, e) in enumerate(zip(dist[depth], exp)) if float(g) != e]
            assert not bad, (depth, bad[:5])
        print("routing per depth:", seen)
        assert all(seen[d] == seen["1"] for d in DEPTHS), seen
        assert all(np.array_equal(dist[d], dist["1"]) for d in DEPTHS)
        assert seen["1"][0] > 0
    finally:
        eng.close()
