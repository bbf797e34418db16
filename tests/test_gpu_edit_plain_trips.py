"""The plain 8-column trips of the multi-lane full-matrix edit-distance form (svim_amd/csrc/edit.hip: d_edit_wide) on a real MI355X (`-m gpu`): every distance
equals the plain DP (edit_cases.levenshtein_rows), with the switch on and off (SVX_EDIT_WIDE_PLAIN; a fresh Engine per setting), and the classes the pairs are aimed
at are read back from the edit_profile lines of SVX_EDIT_PROFILE=1.

HOW A PAIR REACHES ITS CLASS.  A pair that holds '=' (code 0) goes straight to full_class_for(m) in the 4-plane kernels, whatever its text length n >= m.  An
A/C/G/T pair reaches the same class in round 0 (2-plane kernels) when its length gap alone is beyond every band: n - m >= REACH = 466, where need_window >=
n - m + 1 no longer fits the 16-word class (band_class_for, restated in edit_cases).  The pattern is the shorter core, so n >= m (>= m + 466): the text lengths are
n = 8 k - 1, 8 k, 8 k + 1 for the SMALLEST k the route admits, not the first trip behind the prologue (unreachable: a wide class has m > 512), and one n some
300 columns further on.  With the classes of a throughput call (SVX_EDIT_FEW_PAIRS=0) a group of G lanes is always full (m > (G - 1) 32 Q in every class), so the
idle lane of a group is reached through the few-pairs route, which sends any m <= 4096 to the 8-lane form of 16 words (SVX_EDIT_NO_LL=1) or to the 64-lane forms.

SHAPES.  The smallest m of each class (513, 641, 769, 897 rows: 10, 12, 14, 16 words in 2 lanes; 1025: 4 lanes; 2049: 8 lanes); calls of one wave or two, so that
a case takes a second or two on the device; the DP of every distinct pair is computed once per process and shared."""
import collections
import json
import random

import numpy as np
import pytest

import edit_cases as EC

SWITCHES = ("SVX_EDIT_GUESS", "SVX_EDIT_FORCE_FULL", "SVX_EDIT_NARROW", "SVX_EDIT_FEW_PAIRS", "SVX_EDIT_RETRY_FULL", "SVX_EDIT_NO_EARLY", "SVX_EDIT_NO_LL",
            "SVX_EDIT_PROFILE", "SVX_EDIT_SERIAL", "SVX_EDIT_SHIFT_BOUNDS", "SVX_EDIT_PREP_DEPTH", "SVX_EDIT_WIDE_PLAIN")
# the widest need_window a band holds (16 words, staircase slack): a gap of REACH and more is beyond every band whatever the bound
REACH = 32 * EC.band_words(EC.NBAND - 1) - EC.SLACK_STAIR
THROUGHPUT = {"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": EC.GUESS}
# (class, lanes per pair G, words per lane Q, smallest m that enters it)
WIDE = [(EC.CLS_WIDE10, 2, 10, 513), (EC.CLS_WIDE12, 2, 12, 641), (EC.CLS_WIDE14, 2, 14, 769), (EC.CLS_WIDE0, 2, 16, 897),
        (EC.CLS_WIDE10 + 1, 4, 10, 1025), (EC.CLS_WIDE10 + 2, 8, 10, 2049)]
_DP = {}


def dist(a, b):
    if (a, b) not in _DP:
        _DP[(a, b)] = EC.levenshtein_rows(a, b)
    return _DP[(a, b)]


def make_pair(key, m, n, generic, related=False):
    """pattern of m rows, text of n >= m columns, nothing trimmed; related: the text is the pattern with 3 % substitutions, then random symbols"""
    rng = random.Random("plain_trips/%s/%d/%d/%d/%d" % (key, m, n, generic, related))
    a = EC.seq(rng, m)
    if related:
        b = "".join(EC.other(c, rng) if rng.random() < 0.03 else c for c in a) + EC.seq(rng, n - m)
    else:
        b = EC.seq(rng, n)
    a, b = EC.unrelated_ends(a, b)
    if generic:
        a = a[:m // 2] + "=" + a[m // 2 + 1:]
    assert EC.first_class(a, b, guess=float(EC.GUESS))[2:4] == (m, n), "the cores are the strings"
    return a, b


def text_lengths(m, generic):
    """8 k - 1, 8 k, 8 k + 1 for the smallest k the route admits, and one some 300 columns further"""
    n0 = m if generic else m + REACH
    k = (n0 + 1 + 7) // 8
    return [8 * k - 1, 8 * k, 8 * k + 1, 8 * k + 301]


def ragged(key, m, n, generic):
    """texts of n, n - 1, n - 7, n - 8, n - 9 and n - 64 columns: the plain loop ends while some pairs still have columns"""
    return [make_pair(key, m, n - d, generic) for d in (0, 1, 7, 8, 9, 64)]


def cycle(pairs, count):
    return [pairs[i % len(pairs)] for i in range(count)]


class Session:
    """a fresh Engine under one switch setting"""
    def __init__(self, monkeypatch, env):
        from svim_amd._lib import Engine
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.env = env
        self.e = Engine()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.e.close()

    def check(self, pairs, what):
        got = self.e.edit_distances(pairs)
        bad = [(i, len(a), len(b), got[i], dist(a, b)) for i, (a, b) in enumerate(pairs) if got[i] != dist(a, b)]
        assert not bad, "%s %r: %d of %d pairs differ from the DP, first (index, len a, len b, device, DP): %s" % (what, self.env, len(bad), len(pairs), bad[:8])


def profile_rows(err):
    """{(round, cls, generic): pairs} from the edit_profile lines"""
    tab = collections.Counter()
    for line in err.splitlines():
        if line.startswith('{"edit_profile"'):
            r = json.loads(line)["edit_profile"]
            tab[(r["round"], r["cls"], r["generic"])] += r["pairs"]
    return tab


def classes_of(monkeypatch, capfd, env, pairs, what):
    """the call under SVX_EDIT_PROFILE=1 -> {(round, class, alphabet): pairs}; distances checked as well"""
    with Session(monkeypatch, dict(env, SVX_EDIT_PROFILE="1")) as s:
        capfd.readouterr()
        s.check(pairs, what + " (profiled)")
        return profile_rows(capfd.readouterr().err)


# ---- the hand-off bits at a lane boundary, from the DP alone ------------------------------------------------------------------------------------------------
def handoff_states(a, b, row):
    """what the lane that ends at pattern row `row` hands down in the columns 1..n, from the plain DP's matrix: the horizontal delta of that row (plus: +1,
    minus: -1) and the carry of the adder chain (eq & pv) + pv out of it - a row i <= `row` whose symbol matches the column's and whose vertical delta in the
    column before is +1, with vertical deltas +1 from there down to `row` -> ({plus values}, {minus values}, {carry values})"""
    D = EC.levenshtein_matrix(a, b)                          # pattern along the rows
    pa, tb = EC._codes(a), EC._codes(b)
    h = D[row, 1:] - D[row, :-1]
    plus, minus = set((h == 1).tolist()), set((h == -1).tolist())
    carry = set()
    for j in range(1, tb.size + 1):
        pv = (D[1:row + 1, j - 1] - D[:row, j - 1]) == 1     # rows 1..row
        zeros = np.nonzero(~pv)[0]
        first = int(zeros[-1]) + 1 if zeros.size else 0      # the run of +1 deltas that ends at `row` starts here
        carry.add(bool(np.any(pa[first:row] == tb[j - 1])))
        if len(carry) == 2:
            break
    return plus, minus, carry


@pytest.mark.parametrize("cls,G,Q,m", [w for w in WIDE if w[1] <= 4])
def test_handoff_bits_take_both_states(cls, G, Q, m):
    """unrelated and related text together put each of the three hand-off bits into both states at the first lane boundary (CPU only)"""
    assert EC.full_class_for(m) == cls and EC.full_class_for(m - 1) != cls
    n = text_lengths(m, 0)[3]
    pad = G * 32 * Q - m
    row = 32 * Q - pad                                       # last pattern row of lane 0
    assert 0 < row < m
    got = [set(), set(), set()]
    for related in (False, True):
        a, b = make_pair("wide%d" % cls, m, n, 0, related)
        for s, t in zip(got, handoff_states(a, b, row)):
            s |= t
    assert got == [{False, True}] * 3, got


# ---- the multi-lane forms -----------------------------------------------------------------------------------------------------------------------------------
def wide_calls(cls, G, m, generic):
    """[(what, pairs)]: one call each"""
    per_wave = 64 // G
    key = "wide%d" % cls
    ns = text_lengths(m, generic)
    calls = [("every pair n = %d" % n, [make_pair(key, m, n, generic)] * per_wave) for n in ns]
    rag = ragged(key, m, ns[3], generic)
    calls.append(("a wave of ragged texts", cycle(rag, per_wave)))
    calls.append(("one pair", rag[:1]))
    for count in (per_wave - 1, per_wave, per_wave + 1):
        calls.append(("%d pairs" % count, cycle(rag[:3], count)))
    rel = make_pair(key, m, ns[3], generic, related=True)
    calls.append(("related text", [rel] * 2 + rag[:2]))
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("cls,G,Q,m", WIDE)
def test_wide_plain_trips(monkeypatch, capfd, cls, G, Q, m):
    for generic in (0, 1):
        calls = wide_calls(cls, G, m, generic)
        tab = collections.Counter()
        for what, pairs in calls[3:5]:
            tab.update(classes_of(monkeypatch, capfd, THROUGHPUT, pairs, "class %d alphabet %d, %s" % (cls, generic, what)))
        assert set(tab) == {(0, cls, generic)}, "aimed at class %d alphabet %d in round 0, the profile {(round, class, alphabet): pairs}: %s" % (cls, generic, dict(tab))
        for plain in ("1", "0"):
            with Session(monkeypatch, dict(THROUGHPUT, SVX_EDIT_WIDE_PLAIN=plain)) as s:
                for what, pairs in calls:
                    s.check(pairs, "class %d alphabet %d, %s" % (cls, generic, what))


@pytest.mark.gpu
@pytest.mark.parametrize("no_ll", ["1", "0"])
def test_wide_idle_lanes(monkeypatch, capfd, no_ll):
    """a call of few pairs: any m <= 4096 takes the 8-lane form of 16 words (SVX_EDIT_NO_LL=1) or the 64-lane form of 2 words - m = 3073 fills 7 of 8 lanes and 49
    of 64, m = 65 one lane and two; with the pairs of a full group beside them and alone"""
    env = {"SVX_EDIT_NO_LL": "1"} if no_ll == "1" else {}
    for generic in (0, 1):
        calls = []
        for m in (3073, 65):
            ns = text_lengths(m, generic)
            rag = ragged("idle", m, ns[3], generic)
            calls += [("m %d, n = %d" % (m, n), [make_pair("idle", m, n, generic)] * 2) for n in ns[:3]]
            calls += [("m %d, ragged" % m, rag), ("m %d, one pair" % m, rag[:1]), ("m %d, related" % m, [make_pair("idle", m, ns[3], generic, related=True)])]
            calls += [("m %d, %d pairs" % (m, count), cycle(rag[:3], count)) for count in (7, 8, 9)]        # around one wave of the 8-lane form
        calls.append(("full and partly idle groups", ragged("idle", 3073, 3600, generic)[:2] + ragged("idle", 4096, 4600, generic)[:2] + ragged("idle", 65, 700, generic)[:2]))
        tab = classes_of(monkeypatch, capfd, env, calls[3][1], "few pairs, alphabet %d" % generic)
        assert set(tab) == {(0, EC.CLS_WIDE0 + 2, generic)}, dict(tab)
        for plain in ("1", "0"):
            with Session(monkeypatch, dict(env, SVX_EDIT_WIDE_PLAIN=plain)) as s:
                for what, pairs in calls:
                    s.check(pairs, "few pairs, alphabet %d, %s" % (generic, what))
