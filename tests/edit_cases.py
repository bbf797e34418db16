"""Directed cases for the edit-distance kernels (svim_amd/csrc/edit.hip), the plain DP they are held to, and an integer model of one window attempt.

THE TRUTH.  levenshtein_rows(a, b) is the Wagner-Fischer recurrence, one row at a time in integer numpy: substitution and deletion are element-wise minima, the
insertion chain D[i][j] = min_k (t[k] + (j - k)) is np.minimum.accumulate(t - idx) + idx.  No bit-vectors, no bands, no cut-offs: nothing it could share with a
Myers kernel or with oracle/svx_oracle.c (svo_edit_distance is a Myers/Hyyro bit-vector too).  tests/test_edit_cases.py holds it to the pure-Python
levenshtein_dp of tests/golden/make_golden.py.

THE CASES.  Deterministic (seeded by family and case name), at the smallest shapes that still reach a kernel: the lane short-cut of k_edit_classify sends a
pattern of m <= 512 rows to the one-lane full matrix as soon as that needs no more words than the band, so a staircase class of 3 / 4 / 6 / 8..14 / 16 words is
reached only for m above 64 / 128 / 128 / 256 / 512.  Every case names the route it is aimed at; first_class() below restates how the device picks it (trim,
upper bound, classes), and tests/test_edit_cases.py prints the table of what the cases reach.

THE MODEL.  window_model() computes, in plain integers over the cells of the window only, what one band or staircase attempt returns and whether the kernel
accepts it.  It proves on the CPU that the margin cases sit where they claim (accepted below and on the margin, rejected above), and its one-step mutants show
which of them would report a wrong distance if an acceptance rule were off by one.
"""
import hashlib
import random

import numpy as np

# ---- constants of svim_amd/csrc/edit.hip, restated (one block: a change there must be repeated here, and the coverage tests say so) ----------------------
NIBBLE = "=ACMGRSVTWYHKDBN"
NBAND = 9
FIRST_STAIR_CLS = 1
CLS_FULL, CLS_LANE0, CLS_WIDE0, CLS_WIDE12, CLS_WIDE14, CLS_WIDE10 = 9, 10, 15, 19, 23, 27
MIN_MARGIN = 16
STAIR_QMIN = 3
PREP_LANES = 16                 # k_edit_prep: 16 lanes x 8 symbols = 128 symbols per trip
FEW_PAIRS = 2048                # SVX_EDIT_FEW_PAIRS default
PILOT_PAIRS = 4096              # calls from this size on run the pilot
BIG_ROWS = 16384                # a shorter core beyond this: k_edit_full_big
SLACK_SLIDE, SLACK_STAIR = 14, 46


def band_words(b):
    return 1 if b == 0 else 3 if b == 1 else 4 if b == 2 else 2 * b          # 1 | 3 4 6 8 10 12 14 16


def band_class_for(need_w, slack=(SLACK_SLIDE, SLACK_STAIR)):
    for b in range(NBAND):
        if need_w + (slack[0] if b < FIRST_STAIR_CLS else slack[1]) <= 32 * band_words(b):
            return b
    return CLS_FULL


def band_class_with_words(words):
    for b in range(NBAND):
        if band_words(b) >= words:
            return b
    return CLS_FULL


def need_window(m, n, ub):
    x = max(0, (ub - (n - m)) // 2) if ub - (n - m) >= 0 else 0
    return (n - m) + 2 * x + 1


def lane_class_for(m):
    return 0 if m <= 32 else 1 if m <= 64 else 2 if m <= 128 else 3 if m <= 256 else 4


def full_class_for(m):
    if m <= 512:
        return CLS_LANE0 + lane_class_for(m)
    for k in range(4):
        if m <= (640 << k):
            return CLS_WIDE10 + k
        if m <= (768 << k):
            return CLS_WIDE12 + k
        if m <= (896 << k):
            return CLS_WIDE14 + k
        if m <= (1024 << k):
            return CLS_WIDE0 + k
    return CLS_FULL


def lane_shortcut(cls, m):
    """k_edit_classify / band_retry: a band class whose window is no narrower than the whole pattern in one lane goes to that lane class"""
    if 0 < cls < NBAND and m <= 512 and (1 << lane_class_for(m)) <= band_words(cls):
        return CLS_LANE0 + lane_class_for(m)
    return full_class_for(m) if cls == CLS_FULL else cls


def slide_geometry(m, n, words=1):
    """band_core: (dmax, margin) of the sliding window"""
    W, delta = 32 * words, n - m
    a0 = (W - 1 - delta) // 2 if W - 1 - delta >= 0 else -((delta - W + 1) // 2)          # C division truncates toward zero
    dmax = delta + a0
    dmax -= (dmax - 7) & 7
    return dmax, dmax - delta


def stair_geometry(m, n, words, align=True):
    """d_edit_stair: (off, margin) - the window starts at row -off, holds 32 * words rows and drops 32 rows per 32 columns"""
    W0, delta = 32 * words, n - m
    off = max(7, (W0 - 34 + delta) // 2)
    if align:
        off -= (off - 7) & 7
    return off, min(W0 - off - 33, off + 1 - delta)


def class_margin(cls, m, n):
    return slide_geometry(m, n)[1] if cls < FIRST_STAIR_CLS else stair_geometry(m, n, band_words(cls))[1]


def encode(s):
    return np.array([NIBBLE.index(c) for c in s], dtype=np.uint8) if s else np.zeros(0, np.uint8)


def trim(ca, cb):
    """k_edit_prep: common prefix first, then the common suffix of what is left of the SHORTER string -> (pre, suf)"""
    mn = min(ca.size, cb.size)
    ne = np.nonzero(ca[:mn] != cb[:mn])[0]
    pre = int(ne[0]) if ne.size else mn
    lim = mn - pre
    if lim == 0:
        return pre, 0
    ne = np.nonzero(ca[ca.size - lim:][::-1] != cb[cb.size - lim:][::-1])[0]
    return pre, int(ne[0]) if ne.size else lim


def cores(a, b):
    """(pattern core, text core) as code arrays, m <= n; A is the pattern on a tie, as on the device"""
    ca, cb = encode(a), encode(b)
    pre, suf = trim(ca, cb)
    xa, xb = ca[pre:ca.size - suf], cb[pre:cb.size - suf]
    return (xa, xb) if xa.size <= xb.size else (xb, xa)


def upper_bound(p, t):
    """the left-justified substitution-only bound of k_edit_prep (bound_at(0, 0)); given up when more than a quarter of the first 128 symbols mismatch"""
    m, n = p.size, t.size
    if m > 8 * PREP_LANES and int(np.count_nonzero(p[:8 * PREP_LANES] != t[:8 * PREP_LANES])) > 2 * PREP_LANES:
        return n
    return min(n, int(np.count_nonzero(p != t[:m])) + (n - m))


def flags(a, b):
    """(generic, zero): a symbol that is not one of A, C, G, T anywhere in either STRING (not only in the cores) / a code 0 anywhere"""
    s = a + b
    return int(any(c not in "ACGT" for c in s)), int("=" in s)


def first_class(a, b, guess=None, few=False, force_full=False, slack_cut=0):
    """the class the device gives the pair in round 0 -> (cls or -1 when k_edit_prep answers, generic, m, n, ub).  guess = SVX_EDIT_GUESS (a fraction)"""
    p, t = cores(a, b)
    m, n = p.size, t.size
    generic, zero = flags(a, b)
    if m == 0:
        return -1, generic, m, n, n
    ub = upper_bound(p, t)
    if force_full:
        return CLS_FULL, generic, m, n, ub
    if zero:
        cls = full_class_for(m)
    else:
        slack = (SLACK_SLIDE - slack_cut, SLACK_STAIR - slack_cut)
        guaranteed = band_class_for(need_window(m, n, ub), slack)
        g = 2 * MIN_MARGIN
        if guess is not None:
            g = max(g, int(np.ceil(np.float32(guess) * np.float32(m))))
        spec = band_class_for((n - m) + g + 1, slack)
        if spec == CLS_FULL and band_class_for((n - m) + 2 * MIN_MARGIN + 1, slack) != CLS_FULL:
            spec = NBAND - 1
        cls = lane_shortcut(min(guaranteed, spec), m)
    if few and m > 64 and not (cls < NBAND and m <= 512):
        cls = CLS_WIDE0 + 2 if m <= 4096 else CLS_WIDE12 + 3 if m <= 6144 else CLS_WIDE0 + 3 if m <= 8192 else CLS_FULL
    return cls, generic, m, n, ub


def retry_class(cur, m, n, ub, d, swap=False, slack_cut=0):
    """band_retry: the class a pair that failed class `cur` with the upper bound d goes to"""
    ub = min(ub, d)
    cls = band_class_for(need_window(m, n, ub), (SLACK_SLIDE - slack_cut, SLACK_STAIR - slack_cut))
    lo, hi = band_class_with_words(2 * band_words(cur)), band_class_with_words(4 * band_words(cur))
    if swap:
        lo, hi = hi, lo
    if cls > hi:
        cls = hi
    if cls < lo:
        cls = lo
    if cls >= NBAND:
        cls = CLS_FULL
    return lane_shortcut(cls, m), ub


# ---- the truth ----------------------------------------------------------------------------------------------------------------------------------------------
def _codes(s):
    return np.frombuffer(s.encode("ascii"), np.uint8) if isinstance(s, str) else np.asarray(s)


def levenshtein_rows(a, b):
    """unit-cost global edit distance, Wagner-Fischer row by row (the shorter string along the row)"""
    a, b = _codes(a), _codes(b)
    if a.size < b.size:
        a, b = b, a
    n = b.size
    idx = np.arange(n + 1, dtype=np.int64)
    prev = idx.copy()
    t = np.empty(n + 1, np.int64)
    for i in range(a.size):
        t[0] = i + 1
        np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i]), out=t[1:])
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[n])


def levenshtein_matrix(a, b):
    """the whole (len(a) + 1) x (len(b) + 1) matrix of the same recurrence (small cases only)"""
    a, b = _codes(a), _codes(b)
    n = b.size
    idx = np.arange(n + 1, dtype=np.int64)
    D = np.empty((a.size + 1, n + 1), np.int64)
    D[0] = idx
    t = np.empty(n + 1, np.int64)
    for i in range(a.size):
        t[0] = i + 1
        np.minimum(D[i, 1:] + 1, D[i, :-1] + (b != a[i]), out=t[1:])
        D[i + 1] = np.minimum.accumulate(t - idx) + idx
    return D


# ---- the window model ---------------------------------------------------------------------------------------------------------------------------------------
class Mutant:
    """one-step changes of the rules below; every field 0 / False is the kernel as it stands"""
    def __init__(self, margin=0, kcap=0, top_eager=0, bot_eager=0, oc_t=0, oc_b=0, unaligned=False, slack=0, swap=False):
        self.margin, self.kcap, self.top_eager, self.bot_eager, self.oc_t, self.oc_b = margin, kcap, top_eager, bot_eager, oc_t, oc_b
        self.unaligned, self.slack, self.swap = unaligned, slack, swap


KERNEL = Mutant()


def _window_columns(D, r0, p, t, j_from, j_to, top):
    """columns j_from + 1 .. j_to over the window rows r0 .. r0 + len(D) - 1; D = the window's cells at column j_from, top = D[r0 - 1][j_from].
    The row above the window steps +1 per column; a row <= 0 or > m holds the never-matching filler.  Returns (D at j_to, top at j_to)."""
    rows = np.arange(r0, r0 + D.size)
    real = (rows >= 1) & (rows <= p.size)
    sym = np.where(real, p[np.clip(rows - 1, 0, max(0, p.size - 1))] if p.size else 0, 255).astype(np.int64)
    idx = np.arange(D.size, dtype=np.int64)
    for j in range(j_from + 1, j_to + 1):
        up = np.empty(D.size, np.int64)                      # D[i - 1][j - 1]
        up[0] = top
        up[1:] = D[:-1]
        top += 1
        x = np.minimum(D + 1, up + (sym != int(t[j - 1])))
        x[0] = min(x[0], top + 1)
        D = np.minimum.accumulate(x - idx) + idx
    return D, top


def window_model(a_core, b_core, cls, ub, narrow=True, mut=KERNEL):
    """One attempt of band class `cls` on a pair of cores (code arrays, len(a_core) <= len(b_core)) whose known upper bound is ub ->
    {"d": the cost the attempt returns, "accepted": whether the kernel writes it as the distance, "margin", "kcap", "events": what stair_block decided at every
    block boundary as (block, words before, top quantity - kcap or None, bottom quantity - kcap or None, cut top, cut bottom)}.
    A DP over the window's cells only, with the kernel's boundary rules; a wave is taken to hold copies of this pair (its __all votes are the pair's own)."""
    p, t = np.asarray(a_core), np.asarray(b_core)
    m, n = p.size, t.size
    delta = n - m
    ev = []
    if cls < FIRST_STAIR_CLS:
        # sliding window (band_core): bit b of column j is row j - dmax + b; rows above it step +1 per column.  The same cells as a fixed diagonal band.
        W = 32 * band_words(cls)
        dmax, margin = slide_geometry(m, n, band_words(cls))
        if mut.unaligned:
            dmax, margin = delta + (W - 1 - delta) // 2, (W - 1 - delta) // 2
        INF = 1 << 40
        col = np.full(m + 2, INF, np.int64)                  # D[i][j], diagonals j - i in [dmax - W + 1, dmax]; index m + 1 is a guard
        for i in range(0, m + 1):
            if -i >= dmax - W + 1:
                col[i] = i
        idx = np.arange(m + 1, dtype=np.int64)
        for j in range(1, n + 1):
            lo, hi = max(0, j - dmax), min(m, j - (dmax - W + 1))
            new = np.full(m + 2, INF, np.int64)
            if lo <= hi:
                x = np.full(m + 1, INF, np.int64)
                rows = np.arange(max(lo, 1), hi + 1)
                if rows.size:
                    x[rows] = np.minimum(col[rows] + 1, col[rows - 1] + (p[rows - 1] != t[j - 1]))
                if lo == 0:
                    x[0] = j
                # (the row that leaves at the top hands D + 1 down and the row that enters at the bottom starts from D of the row above + 1: neither can beat the
                # diagonal step into the same cell, so both edges are walls)
                y = np.minimum.accumulate(x - idx) + idx
                new[lo:hi + 1] = y[lo:hi + 1]
            col = new
        d = int(col[m]) if col[m] < INF else -1
        x = (d - delta) >> 1
        acc = d >= 0 and margin >= 0 and 0 <= x <= margin + mut.margin
        return {"d": d, "accepted": bool(acc), "margin": margin, "kcap": delta + 2 * margin + 1, "events": ev}
    Q = band_words(cls)
    off, margin = stair_geometry(m, n, Q, align=not mut.unaligned)
    kcap = delta + 2 * (margin + mut.margin) + 1 if margin >= 0 else -1
    if ub < kcap:
        kcap = ub
    kcap += mut.kcap
    trow, top = -off, off + 1
    rows = np.arange(trow, trow + 32 * Q)
    D = np.where(rows <= 0, -rows, rows).astype(np.int64)    # column 0: rows <= 0 step -1 down to D[0][0] = 0, real rows step +1
    d = -1
    n_blocks = (n + 31) >> 5
    for kb in range(n_blocks):
        j1 = 32 * (kb + 1)
        D, top_new = _window_columns(D, trow, p, t, 32 * kb, min(j1, n), top)
        if n <= j1:
            bm = m - trow
            d = int(D[bm]) if 0 <= bm < 32 * Q else -1
            break
        top = top_new
        t1 = int(D[31])
        et = eb = False
        qt = qb = None
        if narrow and Q > STAIR_QMIN:
            t2 = int(D[63])
            oc_t = j1 - (trow + 63) + mut.oc_t
            qt = t2 + (oc_t - delta) - kcap if oc_t >= delta else None
            ok_t = qt is not None and qt > -mut.top_eager
            sb = int(D[32 * (Q - 1) - 1])
            bot = trow + 32 * Q
            oc_b = j1 - (bot - 33) + mut.oc_b
            qb = sb + (delta - oc_b) - kcap if bot <= m and oc_b <= delta else None
            ok_b = bot > m or (qb is not None and qb > -mut.bot_eager)
            et, eb = bool(ok_t), bool(ok_b)
            if et and eb and Q - 2 < STAIR_QMIN:
                eb = False
        ev.append((kb, Q, qt, qb, et, eb))
        drop = 64 if et else 32
        keep = D[drop:]
        top = int(D[drop - 1])
        trow += drop
        if not eb:
            keep = np.concatenate([keep, keep[-1] + np.arange(1, 33, dtype=np.int64)])        # a word that enters steps +1 per row
        D = keep
        Q = Q - (1 if et else 0) - (1 if eb else 0)
    acc = margin >= 0 and d >= 0 and d <= kcap
    return {"d": d, "accepted": bool(acc), "margin": margin, "kcap": kcap, "events": ev}


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------------------
# SVX_EDIT_GUESS of the band families.  A pair whose trivial bound says nothing starts in the class that holds n - m + max(32, ceil(guess * m)) + 1 diagonals
# (k_edit_classify), so with the guess pinned the LENGTH of a pair picks its class.  A detour of `margin` diagonals costs 2 * margin; it is the cheapest alignment
# only while that is well below what unrelated text costs (about m / 2), so m is about 7 margins: the largest m that still starts in the class.
GUESS = "0.25"
GUESS_MID = "0.1"
GUESS_CHAIN = "0.05"            # the retry chains: long pairs (whose distance defeats 12 and 16 words) that still START in 3 and 4 words
LANE_FLOOR = {1: 64, 2: 128, 3: 128, 4: 256, 5: 256, 6: 256, 7: 256, 8: 512}          # the lane short-cut takes a class's pairs up to this m


def m_for(cls, delta, guess=GUESS):
    """largest pattern length that starts in band class cls (1..8) at n - m = delta when its bound is useless; None where the class cannot be reached that way"""
    lim = 32 * band_words(cls) - SLACK_STAIR - 1 - delta          # ceil(guess * m) <= lim
    if lim < 2 * MIN_MARGIN:
        return None
    m = int((lim - 0.001) / float(guess))
    while first_guess_class(m, m + delta, guess) != cls and m > LANE_FLOOR[cls]:
        m -= 1
    return m if m > LANE_FLOOR[cls] and first_guess_class(m, m + delta, guess) == cls else None


def first_guess_class(m, n, guess):
    g = max(2 * MIN_MARGIN, int(np.ceil(np.float32(float(guess)) * np.float32(m))))
    spec = band_class_for((n - m) + g + 1)
    if spec == CLS_FULL and band_class_for((n - m) + 2 * MIN_MARGIN + 1) != CLS_FULL:
        spec = NBAND - 1
    return spec


class Case:
    """one pair.  route: what it is aimed at; copies: how often the pair stands in its call; guess: the SVX_EDIT_GUESS of its engine; wave: cases that share a
    `wave` form one call of their own (the cut family: a wave of 64 lanes votes on every cut)"""
    __slots__ = ("family", "name", "a", "b", "route", "copies", "guess", "wave")

    def __init__(self, family, name, a, b, route, copies=1, guess=GUESS, wave=None):
        self.family, self.name, self.a, self.b, self.route, self.copies, self.guess, self.wave = family, name, a, b, route, copies, guess, wave

    def first_class(self, **kw):
        return first_class(self.a, self.b, guess=float(self.guess), **kw)

    @property
    def generic(self):
        return flags(self.a, self.b)[0]

    def sha1(self):
        return hashlib.sha1((self.a + "|" + self.b).encode("ascii")).hexdigest()


def _rng(*key):
    return random.Random("edit_cases/" + "/".join(str(k) for k in key))


def seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(c, rng=None):
    """a base that differs from c"""
    s = [x for x in "ACGT" if x != c]
    return s[0] if rng is None else rng.choice(s)


def unrelated_ends(a, b):
    """first and last symbols made to differ, so that nothing is trimmed and the cores are the strings"""
    if a and b:
        if a[0] == b[0]:
            b = other(a[0]) + b[1:]
        if len(a) > 1 and len(b) > 1 and a[-1] == b[-1]:
            b = b[:-1] + other(a[-1])
    return a, b


def detour(rng, base, k, delta, side, e=0, head=3, tail=3):
    """the pair of the margin family: the text lacks a block of k symbols of `base` near one end and holds k (+ delta) random ones near the other, so its only
    cheap alignment runs k diagonals off the corridor 0..delta for nearly the whole length: below it (side 0: the missing block comes first) or above it (side 1).
    Distance = 2 k + delta + e for random `base` (e substitutions in the middle); the first and last symbols are made to differ so that nothing is trimmed."""
    m = len(base)
    b = list(base)
    for q in range(e):
        pos = m // 2 + 7 * q
        b[pos] = other(b[pos])
    b = "".join(b)
    ins = seq(rng, k + delta)
    if side == 0:
        b = b[:head] + b[head + k:]
        b = b[:len(b) - tail] + ins + b[len(b) - tail:]
    else:
        b = b[:head] + ins + b[head:]
        b = b[:len(b) - tail - k] + b[len(b) - tail:]
    return base, b


def diverged(rng, s, rate):
    """s with an edit at about `rate` of its positions: substitutions, deletions and insertions in equal parts, the length kept"""
    out = []
    for ch in s:
        r = rng.random()
        if r >= rate:
            out.append(ch)
        elif r < rate / 3:
            out.append(other(ch, rng))
        elif r < 2 * rate / 3:
            out.append(ch + rng.choice("ACGT"))
    t = "".join(out)
    return (t + seq(rng, len(s)))[:len(s)]


def with_n(a, b):
    """the same cores in the other alphabet: one shared N in front of both strings (trimmed by k_edit_prep; the flag is taken from the whole records)"""
    return "N" + a, "N" + b


def fam_trim():
    out = []
    edges = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257)
    rng = _rng("trim")
    for pre in edges:
        for suf in edges:
            if pre and suf and pre != suf:
                continue                                     # each alone, and both together at the same edge
            ca, cb = unrelated_ends(seq(rng, 9), seq(rng, 12))
            P, S = seq(rng, pre), seq(rng, suf)
            out.append(Case("trim", "pre%d suf%d" % (pre, suf), P + ca + S, P + cb + S, "lane"))
    for k in (1, 7, 8, 9, 127, 128, 129, 257):
        for j in (1, 8, 130):
            out.append(Case("trim", "A*%d vs A*%d" % (k, k + j), "A" * k, "A" * (k + j), "prep"))
        for unit in ("AC", "ACG", seq(rng, 31), seq(rng, 33)):
            if len(unit) * k <= 4000:
                out.append(Case("trim", "unit%d*%d vs *%d" % (len(unit), k, k + 1), unit * k, unit * (k + 1), "prep"))
                out.append(Case("trim", "unit%d*%d vs *%d, one change" % (len(unit), k, k + 1), unit * k, (unit * (k + 1))[:-1] + other(unit[-1]), "lane"))
    s = seq(rng, 300)
    out += [Case("trim", "both empty", "", "", "prep"), Case("trim", "one empty", "", s[:70], "prep"), Case("trim", "other empty", s[:5], "", "prep"),
            Case("trim", "equal", s, s, "prep"), Case("trim", "one symbol equal", "A", "A", "prep"), Case("trim", "one symbol differs", "A", "C", "lane"),
            Case("trim", "core empty: head", s, s[:200] + s[230:], "prep"), Case("trim", "core empty: tail", s[:250], s, "prep"),
            Case("trim", "core empty: front", s[50:], s, "prep")]
    return out


def fam_alphabet():
    out = []
    rng = _rng("alphabet")
    prefixes = [seq(rng, ph) for ph in range(8)]
    for x in NIBBLE:
        for y in NIBBLE:
            for ph in range(8):                              # one-symbol cores behind every nibble phase (equal codes: nothing is left of the cores)
                out.append(Case("alphabet", "%s/%s behind %d" % (x, y, ph), prefixes[ph] + x, prefixes[ph] + y, "prep" if x == y else "lane"))
            body = seq(rng, 31)
            out.append(Case("alphabet", "%s/%s first of 33" % (x, y), "A" + x + body + "C" + "T", "C" + y + body + "G" + "T", "lane"))
            out.append(Case("alphabet", "%s/%s last of 33" % (x, y), "T" + "A" + body + x + "C", "T" + "C" + body + y + "G", "lane"))
    for ph in range(8):
        P = seq(rng, ph)
        for x in NIBBLE:
            out.append(Case("alphabet", "%s alone behind %d" % (x, ph), P + x, P + "", "prep"))
            out.append(Case("alphabet", "%s/%s phase %d" % (x, x, ph), P + "A" + x + "A", P + "C" + x + "C", "lane"))
    return out


def fam_margin():
    out = []
    for cls in range(1, NBAND):
        for delta in (0, 1, 7, 8, 9, 31, 32, 33):
            m = m_for(cls, delta)
            if m is None:
                continue                                     # 3 words hold n - m + 33 + 46 <= 96 diagonals: no pair with n - m > 17 starts there
            n = m + delta
            margin = class_margin(cls, m, n)
            for side in (0, 1):
                for dk in (-2, -1, 0, 1, 2):
                    for e in ((0, 1) if dk in (0, 1) else (0,)):
                        k = margin + dk
                        if k < 1:
                            continue
                        rng = _rng("margin", cls, delta, side, dk, e)
                        a, b = detour(rng, seq(rng, m), k, delta, side, e)
                        out.append(Case("margin", "c%d delta%d side%d k=margin%+d e%d" % (cls, delta, side, dk, e), a, b, "band%d" % cls))
    # substitutions only: ub = the distance = kcap; and the same with one indel (the distance is ub - 1 or less)
    # The bound picks the class (guaranteed <= spec) and is the kcap the window narrows against: the widest class that still holds ub + 1 diagonals, every start width.
    for cls in range(1, NBAND):
        m = m_for(cls, 0)
        rng = _rng("margin", "subst", cls)
        base = seq(rng, m)
        w_prev = band_words(cls - 1) if cls > 1 else 0
        lo_ub = max(18, 32 * w_prev - SLACK_STAIR) if cls > 1 else 18          # need_window = ub + 1 must not fit the class before
        hi_ub = 32 * band_words(cls) - SLACK_STAIR - 1
        for ub in sorted({lo_ub, (lo_ub + hi_ub) // 2, hi_ub}):
            b = list(base)
            step = (m - 130) / float(ub)
            for q in range(ub):                              # behind the first 128 symbols, or the bound pass gives up
                pos = min(m - 1, 129 + int(q * step)) if m > 260 else int(q * (m - 1) / max(1, ub - 1))
                b[pos] = other(b[pos])
            b = "".join(b)
            b = b[:-1] + other(base[-1]) if b[-1] == base[-1] else b
            out.append(Case("margin", "c%d ub%d substitutions" % (cls, ub), base, b, "tight"))
            q = m // 2
            while b[q] != base[q] or b[q + 1] != base[q + 1]:
                q += 1
            b2 = b[:q] + b[q + 1:q + 40] + other(b[q + 40]) + b[q + 40:]       # one symbol out, another in 40 further on: a short excursion below the corridor
            out.append(Case("margin", "c%d ub%d substitutions, a short detour" % (cls, ub), base, b2, "tight"))
    # class 0 through a tight bound: need_window <= 18, the widest x its rule admits at every delta
    rng = _rng("margin", "class0")
    for delta in range(0, 18):
        for m in (70, 200):
            x_max = (18 - 1 - delta) // 2
            for x in sorted({0, max(0, x_max - 1), x_max, x_max + 1}):
                base = seq(rng, m)
                b = list(base)
                pos = sorted({(q * (m - 1)) // (2 * x) if x else 0 for q in range(2 * x + 1)})       # 2 x + 1 mismatches, the first symbol among them: ub = delta + 2 x + 1
                for q in pos:
                    b[q] = other(b[q])
                b = "".join(b)
                if delta:
                    b = b + seq(rng, delta - 1) + other(base[-1])
                out.append(Case("margin", "class0 m%d delta%d x%d" % (m, delta, x), base, b, "band0" if x <= x_max else "tight"))
    return out


def fam_full():
    out = []
    rng = _rng("full")
    for edge in (32, 64, 128, 256, 512, 640, 768, 896, 1024):
        for dm in (-1, 0, 1):
            m = edge + dm
            for gap in range(0, 9):
                a, b = unrelated_ends(seq(rng, m), seq(rng, m + gap))
                out.append(Case("full", "m%d gap%d" % (m, gap), a, b, "full"))
            # (a gap no band holds: the only way an A/C/G/T pair of more than 512 rows enters its full-matrix class in round 0 - with a small gap it tries 16 words first)
            a, b = unrelated_ends(seq(rng, m), seq(rng, m + 450))
            out.append(Case("full", "m%d gap450" % m, a, b, "full"))
            a = seq(rng, m)
            z = a[:m // 2] + "=" + a[m // 2 + 1:]
            b = other(a[0]) + a[1:m - 1] + seq(rng, 4) + other(a[-1])
            out.append(Case("full", "m%d with = in the pattern" % m, z, b, "full"))
            out.append(Case("full", "m%d with = in the text" % m, a, b[:m // 3] + "=" + b[m // 3 + 1:], "full"))
    return out


def fam_full_long():
    """8192, 8193, 16384 and 16385 rows once each with a related text (the systolic kernel, and the big-pair kernel above 16384)"""
    out = []
    rng = _rng("full_long")
    for m in (BIG_ROWS // 2, BIG_ROWS // 2 + 1, BIG_ROWS, BIG_ROWS + 1):
        a = seq(rng, m)
        b = list(a)
        for _ in range(m // 40):
            q = rng.randrange(len(b))
            r = rng.random()
            if r < 0.4:
                b[q] = rng.choice("ACGT")
            elif r < 0.7:
                del b[q]
            else:
                b.insert(q, rng.choice("ACGT"))
        b = "".join(b)
        b += seq(rng, max(15, m + 15 - len(b)))              # the pattern stays the shorter string: m rows exactly
        a, b = unrelated_ends(a, b)
        out.append(Case("full_long", "m%d related" % m, a, b, "full"))
        if m & 1:                                            # code 0 in the pattern: the 4-plane systolic and big-pair kernels
            out.append(Case("full_long", "m%d related, = in one string" % m, a[:m // 2] + "=" + a[m // 2 + 1:], b, "full"))
    return out


def fam_few():
    """the low-latency forms of a call with few pairs (default SVX_EDIT_FEW_PAIRS): m on either side of 64 and 512"""
    out = []
    rng = _rng("few")
    for m in (64, 65, 512, 513):
        for gap in (0, 5, 300):
            a, b = unrelated_ends(seq(rng, m), seq(rng, m + gap))
            out.append(Case("few", "m%d gap%d unrelated" % (m, gap), a, b, "few"))
        base = seq(rng, m)
        a, b = detour(rng, base, 20, 3, 0, 1)
        out.append(Case("few", "m%d detour" % m, a, b, "few"))
        out.append(Case("few", "m%d detour, = in the pattern" % m, a[:m // 2] + "=" + a[m // 2 + 1:], b, "few"))
        out.append(Case("few", "m%d detour, = in the text" % m, a, b[:m // 3] + "=" + b[m // 3 + 1:], "few"))
    return out


def _repeat_base(rng, kind, m):
    if kind == "homopolymer":
        return "A" * m
    if kind == "interrupted":
        return "A" * (m // 2) + "C" + "A" * (m - m // 2 - 1)
    if kind == "polyA flanks":
        return "A" * 70 + seq(rng, m - 140) + "A" * 70
    unit = seq(rng, int(kind[4:]))
    return (unit * (m // len(unit) + 1))[:m]


REPEAT_KINDS = ("homopolymer", "interrupted", "polyA flanks", "unit2", "unit3", "unit31", "unit32", "unit33", "unit64")


def fam_repeats():
    out = []
    for cls in range(1, NBAND):
        m = m_for(cls, 1)
        margin = class_margin(cls, m, m + 1)
        for kind in REPEAT_KINDS:
            rng = _rng("repeats", cls, kind)
            base = _repeat_base(rng, kind, m)
            # copy-number change: the unit deleted j times at one place (a plateau of co-optimal paths), ends pinned by a flank that differs
            u = 1 if kind in ("homopolymer", "interrupted", "polyA flanks") else int(kind[4:])
            for j in (1, 2):
                if u * j < m // 3:
                    a, b = "C" + base + "G", "T" + base[u * j:] + "T"
                    out.append(Case("repeats", "c%d %s minus %d units" % (cls, kind, j), a, b, "band%d" % cls))
            # the margin pair on low-complexity text: a detour of margin - 1, margin, margin + 1 diagonals, where a shifted alignment is nearly free
            for dk in (-1, 0, 1):
                for side in (0, 1):
                    a, b = detour(rng, base, margin + dk, 1, side, 0)
                    a, b = "C" + a + "G", "T" + b + "T"
                    out.append(Case("repeats", "c%d %s detour margin%+d side%d" % (cls, kind, dk, side), a, b, "band%d" % cls))
    # plateaus: a = X S, b = S Z with |X| = |Z| = k and S = A..AC..CG..G.  Dropping X and adding Z costs 2 k and runs k diagonals off the corridor; the path that
    # stays one diagonal closer pays one more per change of letter in S.  So with k = margin + 1 the window holds a path one or two above the distance it cannot
    # hold - what an acceptance rule that is off by one would report - and with k = margin a cut that is too eager by two leaves exactly such a path behind.
    for cls in range(1, NBAND):
        m = m_for(cls, 0)
        margin = class_margin(cls, m, m)
        for changes in (0, 1, 2):
            for dk in (-1, 0, 1, 2):
                for side in (0, 1):
                    k = margin + dk
                    L = m - k
                    S = ("A" * L, "A" * (L // 2) + "C" * (L - L // 2), "A" * (L // 3) + "C" * (L // 3) + "G" * (L - 2 * (L // 3)))[changes]
                    X, Z = "T" * k, "GT" * (k // 2) + "T" * (k % 2)
                    a, b = (X + S, S + Z) if side == 0 else (S + X, Z + S)
                    out.append(Case("repeats", "c%d plateau %d changes, k=margin%+d side%d" % (cls, changes, dk, side), a, b, "band%d" % cls))
    # the full-matrix classes on the same content
    for m in (33, 65, 129, 257, 513, 641, 769, 897):
        for kind in REPEAT_KINDS:
            if kind == "polyA flanks" and m < 200:
                continue
            rng = _rng("repeats", "full", m, kind)
            base = _repeat_base(rng, kind, m)
            out.append(Case("repeats", "full m%d %s vs shifted" % (m, kind), "C" + base + "G", "T" + base[m // 3:] + base[:m // 3] + seq(rng, 40) + "T", "full"))
    return out




def route_chain(a, b, guess, narrow=True, mut=KERNEL):
    """the classes a pair walks through, by the model: ([first class, retry class, ...], the value a band attempt was accepted with or None when a full matrix ends it)"""
    cls, _, m, n, ub = first_class(a, b, guess=float(guess), slack_cut=mut.slack)
    p, t = cores(a, b)
    chain = [cls]
    while 0 <= cls < NBAND:
        r = window_model(p, t, cls, ub, narrow, mut)
        if r["accepted"]:
            return chain, r["d"]
        cls, ub = retry_class(cls, m, n, ub, r["d"] if r["d"] >= 0 else ub, swap=mut.swap, slack_cut=mut.slack)
        chain.append(cls)
    return chain, None


def fam_retry():
    """Pairs that fail their first class into every class band_retry's clamps allow.  Found by search: detours just beyond the margin, related text of graded
    divergence (15 to 40 %) and unrelated text are replayed through the model, and for every (class, next class) the first pair of each kind that walks it is kept.
    band_retry at least doubles the words, so 10 words and more can only fail into the full matrix, and a retry class that is not clamped to 4 x holds the window of
    the cost it was computed from: a pair sees at most two band rounds, and the longest chains are 3 -> 12 words -> full matrix and 4 -> 16 words -> full matrix; a pair
    long enough to defeat 12 and 16 words starts in 3 or 4 words only under a small guess (GUESS_CHAIN)."""
    out = []
    seen = set()
    for guess in (GUESS, GUESS_MID, GUESS_CHAIN):
        for cls in range(1, NBAND):
            m_hi = m_for(cls, 0, guess)
            if m_hi is None:
                continue
            for m in sorted({min(m_hi, 1900), min(m_hi, 1900) * 3 // 4, min(m_hi, 1900) * 5 // 8}):
                if first_guess_class(m, m, guess) != cls or m <= LANE_FLOOR[cls]:
                    continue
                margin = class_margin(cls, m, m)
                for kind in ("detour side0", "detour side1", "unrelated") + tuple("related %d%%" % r for r in (15, 20, 25, 30, 35, 40)):
                    rng = _rng("retry", guess, cls, m, kind)
                    if kind == "unrelated":
                        a, b = unrelated_ends(seq(rng, m), seq(rng, m))
                    elif kind.startswith("related"):
                        a = seq(rng, m)
                        a, b = unrelated_ends(a, diverged(rng, a, int(kind[8:10]) / 100.0))
                    else:
                        a, b = detour(rng, seq(rng, m), margin + 1, 0, int(kind[-1]), 1)
                    chain, _ = route_chain(a, b, guess)
                    key = (cls, chain[1] if len(chain) > 1 else None, kind.split()[0] if kind.startswith("related") else kind)
                    if chain[0] != cls or len(chain) < 2 or key in seen:
                        continue
                    seen.add(key)
                    out.append(Case("retry", "c%d fails into %d: m%d %s, guess %s, walks %s" % (cls, chain[1], m, kind, guess, "-".join(str(x) for x in chain)),
                                    a, b, "band%d" % cls, guess=guess))
    # the longest chains: unrelated text long enough to defeat 12 and 16 words, under the guess that still starts it in 3 and 4 words
    for name, m in (("chain from 3 words", 760), ("chain from 4 words", 1200)):
        rng = _rng("retry", name)
        a, b = unrelated_ends(seq(rng, m), seq(rng, m))
        out.append(Case("retry", name, a, b, "chain", guess=GUESS_CHAIN))
    # one pair 130 times in a call of its own: every pair of the round fails one class into one other, and that list fills to its capacity
    c = next(c for c in out if c.name.startswith("c4 fails into 8") and c.guess == GUESS)
    out.append(Case("retry", "fill: " + c.name, c.a, c.b, c.route, copies=130, guess=c.guess, wave="fill"))
    return out


def _cut_candidates(cls, source, rng):
    """pairs of the margin kind plus clustered noise that start in class cls; source 'window': the bound says nothing, kcap is the window's own;
    source 'ub': substitutions behind the first 128 symbols and a short excursion, so that the bound is tight enough to be kcap and still picks this class"""
    m = m_for(cls, 0)
    margin = class_margin(cls, m, m)
    base = seq(rng, m)
    if source == "window":
        nburst, e = rng.choice((0, 3, 8)), rng.choice((0, 1, 2, 3))
        delta = rng.choice((0, 0, 1, 2))
        k = margin - (nburst + e + 1) // 2 - rng.choice((0, 0, 1, 2, 4))          # 2 k + delta + e + burst stays within delta + 2 margin + 1: the attempt is accepted
        head = rng.choice((31, 32, 33, 63, 64, 65, 95, 96, 97))
        tail = rng.choice((3, 31, 32, 33, 64, 150))
        a, b = detour(rng, base, k, delta, rng.choice((0, 1)), e, head, tail)
        if nburst == 0 or m - tail - k - 60 <= head + k + 10:
            return a, b, head
        lo = rng.randrange(head + k + 10, m - tail - k - 60)
        b = list(b)
        for q in rng.sample(range(lo, lo + 40), nburst):     # a burst of substitutions somewhere on the detour
            b[q] = other(b[q], rng)
        return a, "".join(b), head
    w_prev = band_words(cls - 1)
    ub = rng.randrange(32 * w_prev - SLACK_STAIR, 32 * band_words(cls) - SLACK_STAIR - 1)
    b = list(base)
    for pos in rng.sample(range(129, m - 1), ub - 2):
        b[pos] = other(b[pos], rng)
    b[0], b[m - 1] = other(base[0]), other(base[m - 1])
    b = "".join(b)
    k, at, ln = rng.choice((2, 4, 8, 12, 20)), rng.choice((159, 160, 161, 191, 192, 193, 255, 256, 257)), rng.choice((30, 64, 100, 200))
    if at + ln + k + 2 < m:                                  # k symbols out, k others in `ln` further on: the excursion pays while it is short
        b = b[:at] + b[at + k:at + ln] + seq(rng, k) + b[at + ln:]
    return base, b, at


def fam_cut():
    """Pairs at which a quantity of stair_block lands on its threshold (a cut just refused: 0) or one above it (just allowed: 1) at some block boundary, found by
    replaying candidates through the model and keeping, of those the attempt ACCEPTS, the ones whose distance is nearest kcap (a wrong cut shows only where the
    second-best path still costs <= kcap); the excursion leaves the corridor at a column 32 k - 1, 32 k or 32 k + 1; every start width of 4 to 16 words, kcap once from the window and once from the bound.  Each pair stands 64 times in a
    call of its own (one wave: the vote is the pair's), then with one lane that vetoes, in populations around one and two waves, and with ragged text lengths."""
    out = []
    for cls in range(2, NBAND):
        for source in ("window", "ub"):
            rng = _rng("cut", cls, source)
            kept = {}
            for _ in range(64):
                a, b, leaves = _cut_candidates(cls, source, rng)
                c0, _, m, n, ub = first_class(a, b, guess=float(GUESS))
                if c0 != cls:
                    continue
                p, t = cores(a, b)
                r = window_model(p, t, cls, ub, True)
                if not r["accepted"] or (source == "ub") != (r["kcap"] == ub):
                    continue                                 # only an accepted attempt can report a wrong cut's second-best path
                for kb, Q, qt, qb, et, eb in r["events"]:
                    for which, q in (("top", qt), ("bottom", qb)):
                        if q in (0, 1) and ((which, q) not in kept or r["kcap"] - r["d"] < kept[(which, q)][0]):
                            kept[(which, q)] = (r["kcap"] - r["d"], a, b, kb, Q, leaves)
            for (which, q), (room, a, b, kb, Q, leaves) in sorted(kept.items()):
                name = "c%d kcap from %s, %s at %+d in block %d with %d words, leaves at %d, d = kcap - %d" % (cls, source, which, q, kb, Q, leaves, room)
                out.append(Case("cut", name, a, b, "band%d" % cls, copies=64, wave=name))
    # one lane that vetoes: 63 copies of a pair whose top cut is just allowed, and one pair of the same class whose path runs `margin` diagonals above the corridor
    allowed = [c for c in out if ", top at +1" in c.name and "from window" in c.name]
    for c in allowed[:3]:
        cls = int(c.route[4:])
        m = m_for(cls, 0)
        rng = _rng("cut", "veto", cls)
        va, vb = detour(rng, seq(rng, m), class_margin(cls, m, m), 0, 1, 0)
        w = "veto: " + c.name
        out.append(Case("cut", w + " (63)", c.a, c.b, c.route, copies=63, wave=w))
        out.append(Case("cut", w + " (the veto)", va, vb, c.route, copies=1, wave=w))
    # populations around one and two waves
    if out:
        c = out[0]
        for pop in (1, 63, 65, 129):
            w = "population %d: %s" % (pop, c.name)
            out.append(Case("cut", w, c.a, c.b, c.route, copies=pop, wave=w))
    # ragged text lengths inside a wave: detours of one class whose texts end in different blocks (n - m = 0 .. 58: a class is 64 diagonals wide), four of each
    for cls in (3, 6):
        m = m_for(cls, 58)
        w = "ragged c%d" % cls
        for r in range(0, 16):
            delta = (58 * r) // 15
            rng = _rng("cut", "ragged", cls, r)
            a, b = detour(rng, seq(rng, m), class_margin(cls, m, m + delta) - 2 - r % 3, delta, r & 1, r % 2)
            out.append(Case("cut", "%s delta%d" % (w, delta), a, b, "band%d" % cls, copies=4, wave=w))
    return out


def fam_call_short(n):
    """n short pairs (the filler of the call family): 20..44 symbols, a third related"""
    rng = _rng("call", "short")
    out = []
    for i in range(n):
        a = seq(rng, 20 + rng.randrange(20))
        if i % 3 == 0:
            q = rng.randrange(len(a))
            b = a[:q] + other(a[q]) + a[q + 1:] + seq(rng, rng.randrange(4))
        else:
            b = seq(rng, len(a) + rng.randrange(5))
        out.append(Case("call", "short %d" % i, a, b, "lane"))
    return out


def fam_call():
    """the long related pair first, then the short ones: a call of size s is the first s - 1 short pairs around the long one"""
    rng = _rng("call", "long")
    a, b = detour(rng, seq(rng, 700), 30, 2, 0, 1)
    return [Case("call", "long", a, b, "band")] + fam_call_short(max(CALL_SIZES))


CALL_SIZES = (FEW_PAIRS - 1, FEW_PAIRS, FEW_PAIRS + 1, PILOT_PAIRS - 1, PILOT_PAIRS, PILOT_PAIRS + 1)
TRIM_CALL_SIZES = (1, 15, 16, 17)
BAND_FAMILIES = ("margin", "repeats", "retry", "cut")
FAMILIES = {"trim": fam_trim, "alphabet": fam_alphabet, "margin": fam_margin, "full": fam_full, "full_long": fam_full_long, "few": fam_few,
            "repeats": fam_repeats, "retry": fam_retry, "cut": fam_cut, "call": fam_call}
_CACHE = {}


def family(name):
    """the cases of one family; the band families come in both alphabets (the second half: the same pairs behind one shared N)"""
    if name not in _CACHE:
        cs = FAMILIES[name]()
        if name in BAND_FAMILIES:
            cs = cs + [Case(c.family, c.name + " [N]", *with_n(c.a, c.b), c.route, c.copies, c.guess, None if c.wave is None else c.wave + " [N]") for c in cs]
        names = [c.name for c in cs]
        assert len(set(names)) == len(names), "duplicate case names in " + name
        _CACHE[name] = cs
    return _CACHE[name]


def all_cases():
    return [c for name in FAMILIES for c in family(name)]


def golden_rows(distance=levenshtein_rows):
    """[family, name, len(a), len(b), SHA-1 of both strings, distance] per case"""
    memo = {}
    rows = []
    for c in all_cases():
        key = (c.a, c.b)
        if key not in memo:
            ka, kb = (c.a[1:], c.b[1:]) if c.a[:1] == "N" and c.b[:1] == "N" else key           # a shared first symbol costs nothing
            if (ka, kb) not in memo:
                memo[(ka, kb)] = distance(ka, kb)
            memo[key] = memo[(ka, kb)]
        rows.append([c.family, c.name, len(c.a), len(c.b), c.sha1(), memo[key]])
    return rows


# ---- mutants of the model -----------------------------------------------------------------------------------------------------------------------------------
MUTANTS = [("slide: margin + 1", Mutant(margin=1), "slide"), ("stair: margin + 1", Mutant(margin=1), "stair"), ("stair: kcap + 1", Mutant(kcap=1), "stair"),
           ("top cut eager by 1", Mutant(top_eager=1), "stair"), ("top cut eager by 2", Mutant(top_eager=2), "stair"),
           ("bottom cut eager by 1", Mutant(bot_eager=1), "stair"), ("bottom cut eager by 2", Mutant(bot_eager=2), "stair"),
           ("oc_t + 1", Mutant(oc_t=1), "stair"), ("oc_t - 1", Mutant(oc_t=-1), "stair"), ("oc_b + 1", Mutant(oc_b=1), "stair"), ("oc_b - 1", Mutant(oc_b=-1), "stair"),
           ("off not aligned to 7 mod 8", Mutant(unaligned=True), "both"), ("slack 14 / 46 reduced by 2", Mutant(slack=2), "route"),
           ("lo / hi swapped", Mutant(swap=True), "route")]

# why a mutant that no case catches cannot be caught: an argument, not a shrug (tests/test_edit_cases.py fails on a survivor that has none)
EQUIVALENT = {
    "slide: margin + 1": "the 1-word class is entered only through a bound that fits its margin (need_window <= 18; no retry leads there), and the bound's own "
                         "left-justified path lies inside the window: the attempt never returns more than the bound, so floor((d - delta) / 2) never exceeds the margin.",
    "top cut eager by 1": "it cuts cells through which the best path costs kcap exactly.  If the distance is below kcap no cell of an optimal path is cut; if it is kcap "
                          "every other path costs more than kcap and the attempt is rejected (a needless retry, not a wrong value).",
    "bottom cut eager by 1": "as for the top cut: only a path of cost exactly kcap can be lost, and what is left costs more than kcap.",
    "oc_t + 1": "adds one to the top quantity: the top cut eager by 1; and where it lets a cell one diagonal below delta pass the diagonal test, its quantity is D itself, "
                "which is no more than the true cost through the cell.",
    "oc_t - 1": "takes one off the top quantity and tightens the diagonal test: cuts come later, none comes earlier.",
    "oc_b + 1": "takes one off the bottom quantity and tightens the diagonal test: cuts come later, none comes earlier.",
    "oc_b - 1": "adds one to the bottom quantity: the bottom cut eager by 1; the cell it newly lets pass the diagonal test is tested with D alone.",
    "stair: kcap + 1": "the window holds every path of cost <= kcap, so an attempt that returns kcap + 1 has found the distance itself (a cheaper path would lie inside the "
                       "window and be returned); with kcap taken from the bound, the bound's own left-justified path lies inside the window, so the attempt never "
                       "returns more than the bound.  The larger kcap only makes the cuts later.",
    "off not aligned to 7 mod 8": "the alignment puts the window's first row at the nibble phase of the packed words; the integers of the DP do not know about "
                                  "words.  An unaligned window is a window with other margins, and the acceptance uses the margins of the window it has.",
    "slack 14 / 46 reduced by 2": "the slack only picks the class a pair starts in; whatever the class, the attempt is accepted by its own margin and retried otherwise.",
    "lo / hi swapped": "the clamps only pick the class of the retry; the retry is accepted by its own margin or fails on into a full matrix.",
}


def mutant_cases():
    """the cases the mutants are tried on, the plateaus of the three narrowest classes (the killers), every cut case, the short retries, the margin family of 3 and 4 words from the margin on, class 0"""
    rep = [c for c in family("repeats") if "plateau" in c.name and not c.generic and c.name[:2] in ("c1", "c2", "c3")]
    cut = [c for c in family("cut") if not c.generic and c.copies == 64]
    ret = [c for c in family("retry") if not c.generic and c.copies == 1 and len(c.a) < 700]
    mar = [c for c in family("margin") if not c.generic and c.name[:2] in ("c1", "c2") and ("k=margin+" in c.name or "substitutions" in c.name)]
    mar += [c for c in family("margin") if not c.generic and "class0" in c.name]
    return rep + cut + ret + mar


def mutant_table(golden, narrow=True, limit=None):
    """[(mutant, (the first case whose accepted value differs from the DP, that value, the DP's) or None, cases tried)]; at most `limit` cases per mutant"""
    cases = mutant_cases()
    rows = []
    for name, mut, scope in MUTANTS:
        hit, tried = None, 0
        for c in cases:
            c0 = first_class(c.a, c.b, guess=float(c.guess), slack_cut=mut.slack)[0]
            if not 0 <= c0 < NBAND or (scope == "slide") != (c0 == 0) and scope in ("slide", "stair"):
                continue
            if limit is not None and tried >= limit:
                break
            tried += 1
            chain, val = route_chain(c.a, c.b, c.guess, narrow, mut)
            if val is not None and val != golden[(c.family, c.name)]:
                hit = (c.name, val, golden[(c.family, c.name)])
                break
        rows.append((name, hit, tried))
    return rows
