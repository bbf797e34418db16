"""The edit-distance kernels (svim_amd/csrc/edit.hip) on a real MI355X (`-m gpu`) against the plain DP of tests/edit_cases.py, at every window edge.

Every family of tests/edit_cases.py runs on the route it is aimed at and once more as systolic full matrices (SVX_EDIT_FORCE_FULL=1); the band families also with
static windows (SVX_EDIT_NARROW=0), the retries with band retries instead of full matrices (SVX_EDIT_RETRY_FULL=0) and without round 0's early part
(SVX_EDIT_NO_EARLY).  The expected value of every pair is the DP's, from tests/golden/g_edit_cases.json.gz (tests/test_edit_cases.py holds the generator to the
file's hashes): exact equality, no pair skipped or sampled.  One run per family under SVX_EDIT_PROFILE=1 reads the per-class pair counts from stderr and holds
them to what tests/edit_cases.py says the pairs should reach (at least; a routing change must fail here with the table, not lose coverage in silence)."""
import collections
import json

import pytest

import edit_cases as EC
import helpers as H

pytestmark = pytest.mark.gpu

SWITCHES = ("SVX_EDIT_GUESS", "SVX_EDIT_FORCE_FULL", "SVX_EDIT_NARROW", "SVX_EDIT_FEW_PAIRS", "SVX_EDIT_RETRY_FULL", "SVX_EDIT_NO_EARLY", "SVX_EDIT_NO_LL",
            "SVX_EDIT_PROFILE", "SVX_EDIT_SERIAL", "SVX_EDIT_SHIFT_BOUNDS", "SVX_EDIT_PREP_DEPTH")
_GOLD = {}


def gold():
    if not _GOLD:
        for fam, name, la, lb, sha, d in H.load("g_edit_cases.json.gz")["cases"]:
            _GOLD[(fam, name)] = d
    return _GOLD


class Session:
    """a fresh Engine under one switch setting (SVX_EDIT_GUESS and SVX_EDIT_FORCE_FULL are read when the context is created, the others per call)"""
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

    def check(self, cases, what=""):
        pairs, exp, names = [], [], []
        g = gold()
        for c in cases:
            pairs += [(c.a, c.b)] * c.copies
            exp += [g[(c.family, c.name)]] * c.copies
            names += [c.name] * c.copies
        got = self.e.edit_distances(pairs)
        bad = [(names[i], got[i], exp[i]) for i in range(len(pairs)) if got[i] != exp[i]]
        assert not bad, "%s %r: %d of %d pairs differ from the DP, first (case, device, DP): %s" % (what, self.env, len(bad), len(pairs), bad[:8])
        return len(pairs)


def profile_rows(err):
    """{(round, cls, generic): pairs} from the edit_profile lines of SVX_EDIT_PROFILE=1"""
    tab = collections.Counter()
    for line in err.splitlines():
        if line.startswith('{"edit_profile"'):
            r = json.loads(line)["edit_profile"]
            tab[(r["round"], r["cls"], r["generic"])] += r["pairs"]
    return tab


def profile_mean_m(err):
    """{(round, cls, generic): mean pattern rows} of the same lines"""
    out = {}
    for line in err.splitlines():
        if line.startswith('{"edit_profile"'):
            r = json.loads(line)["edit_profile"]
            out[(r["round"], r["cls"], r["generic"])] = r["mean_m"]
    return out


def profiled(monkeypatch, capfd, env, cases, what):
    """one call under SVX_EDIT_PROFILE=1 with the guess pinned: results, and round 0 holds at least what first_class() predicts for every class and alphabet
    -> ({(round, class, alphabet): pairs}, {(class, alphabet): predicted pairs}, stderr)"""
    env = dict({"SVX_EDIT_GUESS": EC.GUESS, "SVX_EDIT_PROFILE": "1"}, **env)
    with Session(monkeypatch, env) as s:
        capfd.readouterr()
        n = s.check(cases, what + " (profiled)")
        err = capfd.readouterr().err
    few = n <= int(env.get("SVX_EDIT_FEW_PAIRS", EC.FEW_PAIRS))
    want = dict(predicted(cases, few=few, force_full=env.get("SVX_EDIT_FORCE_FULL") == "1"))
    tab = profile_rows(err)
    assert_round0(tab, want, what)
    return tab, want, err


def predicted(cases, **kw):
    tab = collections.Counter()
    for c in cases:
        r = c.first_class(**kw)
        if r[0] >= 0:
            tab[(r[0], r[1])] += c.copies
    return tab


def assert_round0(tab, want, what):
    """every class the cases are said to reach holds at least that many pairs in round 0"""
    short = {k: (tab.get((0,) + k, 0), v) for k, v in want.items() if tab.get((0,) + k, 0) < v}
    assert not short, "%s: round 0 holds fewer pairs than aimed, {(class, alphabet): (held, aimed)} = %s; the whole profile {(round, class, alphabet): pairs} = %s" % (
        what, short, dict(sorted(tab.items())))


BAND = {"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": EC.GUESS}


def by_wave(cases):
    waves = collections.OrderedDict()
    for c in cases:
        waves.setdefault(c.wave, []).append(c)
    return waves


def test_edit_cases_trim(monkeypatch, capfd):
    cs = EC.family("trim")
    # the pairs k_edit_prep does not answer itself sit in the 1-word band (a tight bound) in round 0
    tab, want, _ = profiled(monkeypatch, capfd, {}, cs, "trim")
    assert set(want) == {(0, 0)} and sum(c.first_class()[0] == -1 for c in cs) >= 80, want
    long_trims = [c for c in cs if c.name.startswith("pre") and ("127" in c.name or "128" in c.name or "129" in c.name or "25" in c.name)]
    for env in ({}, {"SVX_EDIT_FEW_PAIRS": "0"}, {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            s.check(cs, "trim")
            for size in EC.TRIM_CALL_SIZES:                  # the last wave of k_edit_prep has idle sub-groups
                s.check(long_trims[:size], "trim, a call of %d" % size)
                s.check(cs[-size:], "trim, a call of the last %d" % size)


def test_edit_cases_alphabet(monkeypatch, capfd):
    cs = EC.family("alphabet")
    # one-symbol and 33-symbol cores: the 1-word band and the one-lane matrices of 32 and 64 rows, A/C/G/T pairs in the 2-plane kernels and the rest in the 4-plane ones
    tab, want, _ = profiled(monkeypatch, capfd, {}, cs, "alphabet")
    assert {(0, 0), (0, 1), (EC.CLS_LANE0, 1), (EC.CLS_LANE0 + 1, 1)} <= set(want), want
    for env in ({}, {"SVX_EDIT_FEW_PAIRS": "0"}, {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            s.check(cs, "alphabet")


@pytest.mark.parametrize("family", ["margin", "repeats"])
def test_edit_cases_windows(monkeypatch, capfd, family):
    cs = EC.family(family)
    with Session(monkeypatch, dict(BAND, SVX_EDIT_PROFILE="1")) as s:
        capfd.readouterr()
        s.check(cs, family + " (profiled)")
        tab = profile_rows(capfd.readouterr().err)
    want = {k: v for k, v in predicted(cs).items() if k[0] < EC.NBAND}
    assert {k[0] for k in want} == set(range(EC.NBAND)) and {k[1] for k in want} == {0, 1}, sorted(want)
    assert_round0(tab, want, family)
    for env in (BAND, dict(BAND, SVX_EDIT_NARROW="0"), dict(BAND, SVX_EDIT_RETRY_FULL="0"), {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            s.check(cs, family)


def test_edit_cases_cut(monkeypatch, capfd):
    waves = by_wave(EC.family("cut"))
    with Session(monkeypatch, dict(BAND, SVX_EDIT_PROFILE="1")) as s:
        capfd.readouterr()
        for w, cs in waves.items():
            s.check(cs, "cut, wave %r (profiled)" % w)
        tab = profile_rows(capfd.readouterr().err)
    want = collections.Counter()
    for w, cs in waves.items():
        want.update({k: v for k, v in predicted(cs).items() if k[0] < EC.NBAND})
    assert {k[0] for k in want} >= set(range(2, EC.NBAND)) and {k[1] for k in want} == {0, 1}, sorted(want)
    assert_round0(tab, want, "cut")
    for env in (BAND, dict(BAND, SVX_EDIT_NARROW="0"), {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            for w, cs in waves.items():
                s.check(cs, "cut, wave %r" % w)


def test_edit_cases_retry(monkeypatch, capfd):
    cs = EC.family("retry")
    groups = collections.OrderedDict()
    for c in cs:
        groups.setdefault((c.guess, c.wave), []).append(c)
    tab = collections.Counter()
    want = collections.Counter()
    for (guess, wave), g in groups.items():
        with Session(monkeypatch, {"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": guess, "SVX_EDIT_RETRY_FULL": "0", "SVX_EDIT_PROFILE": "1", "SVX_EDIT_NO_EARLY": "1"}) as s:
            capfd.readouterr()
            s.check(g, "retry (profiled)")
            tab.update(profile_rows(capfd.readouterr().err))
        want.update({k: v for k, v in predicted(g).items() if k[0] < EC.NBAND})
    assert_round0(tab, want, "retry")
    # band retries happened, in both alphabets; the list of the fill call held every pair of its round
    later = {(k[1], k[2]): v for k, v in tab.items() if k[0] >= 1 and k[1] < EC.NBAND}
    assert {g for _, g in later} == {0, 1} and len({c for c, _ in later}) >= 4, "band classes of the retry rounds {(class, alphabet): pairs}: %s" % later
    assert later.get((8, 0), 0) >= 130 and later.get((8, 1), 0) >= 130, later
    # With static windows the cost a failed attempt returns - and with it the class of the retry - is the window model's (tests/edit_cases.py: route_chain) whatever
    # pairs share a wave; with narrowing a wave-mate's veto keeps words the model of a lone pair cuts, and the returned cost can be lower.  Every later round holds at
    # least what the model sends there.
    tab, want = collections.Counter(), collections.Counter()
    for (guess, wave), g in groups.items():
        with Session(monkeypatch, {"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": guess, "SVX_EDIT_RETRY_FULL": "0", "SVX_EDIT_PROFILE": "1", "SVX_EDIT_NO_EARLY": "1",
                                   "SVX_EDIT_NARROW": "0"}) as s:
            capfd.readouterr()
            s.check(g, "retry (profiled, static windows)")
            tab.update(profile_rows(capfd.readouterr().err))
        for c in g:
            chain, _ = EC.route_chain(c.a, c.b, c.guess, narrow=False)
            for rnd, cls in enumerate(chain[1:], 1):
                want[(rnd, cls, c.generic)] += c.copies
    short = {k: (tab.get(k, 0), v) for k, v in want.items() if tab.get(k, 0) < v}
    assert not short, "retry rounds with static windows, {(round, class, alphabet): (held, the model's)} = %s; the whole profile: %s" % (short, dict(sorted(tab.items())))
    assert max(k[0] for k in want) == 2 and any(k[0] == 2 and k[1] > EC.CLS_FULL for k in want), sorted(want)      # the two longest chains end in round 2, in a full matrix
    for extra in ({}, {"SVX_EDIT_RETRY_FULL": "0"}, {"SVX_EDIT_RETRY_FULL": "0", "SVX_EDIT_NO_EARLY": "1"}, {"SVX_EDIT_RETRY_FULL": "0", "SVX_EDIT_NARROW": "0"},
                  {"SVX_EDIT_FORCE_FULL": "1"}):
        for (guess, wave), g in groups.items():
            with Session(monkeypatch, dict({"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": guess}, **extra)) as s:
                s.check(g, "retry")
        with Session(monkeypatch, dict({"SVX_EDIT_FEW_PAIRS": "0", "SVX_EDIT_GUESS": EC.GUESS}, **extra)) as s:
            s.check([c for c in cs if c.guess == EC.GUESS], "retry, one call")           # failures of every class in one round: both parts of round 0's split launch


def test_edit_cases_full(monkeypatch, capfd):
    cs = EC.family("full") + [c for c in EC.family("repeats") if c.name.startswith("full ")]
    # (SVX_EDIT_NO_EARLY: what round 0's early part fails is launched at once and stands in no round's table)
    with Session(monkeypatch, dict(BAND, SVX_EDIT_PROFILE="1", SVX_EDIT_NO_EARLY="1")) as s:
        capfd.readouterr()
        s.check(cs, "full (profiled)")
        tab = profile_rows(capfd.readouterr().err)
    # A pair that holds '=' goes straight to its full-matrix class (4-plane kernels); an unrelated pair without it tries a band first (3 to 10 words under this guess,
    # unless the one-lane matrix is no wider) and reaches its full-matrix class as a retry.  Round 0 as predicted; over all rounds every one-lane class, the 2-lane
    # forms of 10, 12, 14 and 16 words and the first 4-lane form, in both alphabets.
    want = {k: v for k, v in predicted(cs).items() if k[0] > EC.CLS_FULL}
    assert_round0(tab, want, "full")
    reached = {(k[1], k[2]) for k in tab}
    missing = [(cls, g) for cls in list(range(EC.CLS_LANE0, EC.CLS_LANE0 + 5)) + [EC.CLS_WIDE10, EC.CLS_WIDE12, EC.CLS_WIDE14, EC.CLS_WIDE0, EC.CLS_WIDE10 + 1]
               for g in (0, 1) if (cls, g) not in reached]
    assert not missing, "full-matrix classes no pair reached in any round: %s; the whole profile {(round, class, alphabet): pairs}: %s" % (missing, dict(sorted(tab.items())))
    # the few-pairs route (default SVX_EDIT_FEW_PAIRS): 64 rows stay in their lane class, 65 and 513 rows go to the 64-lane form, a band of a pattern of <= 512 rows stays
    few = EC.family("few")
    tab, want, _ = profiled(monkeypatch, capfd, {}, few, "few")
    assert {(EC.CLS_LANE0 + 1, 0), (EC.CLS_WIDE0 + 2, 0), (EC.CLS_WIDE0 + 2, 1)} <= set(want) and any(k[0] < EC.NBAND for k in want), want
    assert all(c.first_class(few=True)[0] == EC.CLS_WIDE0 + 2 for c in few if c.name.startswith("m513 gap")), "513 rows"
    assert all(c.first_class(few=True)[0] != EC.CLS_WIDE0 + 2 for c in few if c.name.startswith("m64 ")), "64 rows"
    for env in ({}, {"SVX_EDIT_FEW_PAIRS": "0"}, {"SVX_EDIT_NO_LL": "1"}, {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            s.check(cs, "full")
            s.check(few, "few")


def test_edit_cases_long_rows(monkeypatch, capfd):
    cs = EC.family("full_long")
    # a call of few pairs: 8192 rows take the last 16-lane form, 8193 and more the systolic kernel, in both alphabets (one pair of each size holds '=')
    tab, want, _ = profiled(monkeypatch, capfd, {}, cs, "long rows")
    assert {(EC.CLS_WIDE0 + 3, 0), (EC.CLS_FULL, 0), (EC.CLS_FULL, 1)} <= set(want), want
    # beyond 16384 rows the systolic class hands the pair to k_edit_full_big (no counter of it is exported: the profile shows the pair, alone in its call, in the
    # systolic class with its rows; that the rows lie beyond the limit is the restated BIG_ROWS)
    for c in cs:
        m = c.first_class(few=True)[2]
        if m > EC.BIG_ROWS or m == EC.BIG_ROWS:
            tab, want, err = profiled(monkeypatch, capfd, {}, [c], c.name)
            assert list(want) == [(EC.CLS_FULL, c.generic)] and profile_mean_m(err)[(0, EC.CLS_FULL, c.generic)] == float(m), (c.name, want)
    assert sum(c.first_class()[2] > EC.BIG_ROWS for c in cs) >= 2 and any(c.first_class()[2] == EC.BIG_ROWS for c in cs)
    for env in ({}, {"SVX_EDIT_FEW_PAIRS": "0"}, {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            s.check(cs, "8192 / 8193 / 16384 / 16385 rows")


def test_edit_cases_call_sizes(monkeypatch, capfd):
    cs = EC.family("call")

    def call(size):
        half = (size - 1) // 2
        return cs[1:1 + half] + cs[:1] + cs[1 + half:size]

    # on either side of the few-pairs switch the long pair sits in a 64-lane form / in its band class
    long_cls = {}
    for size in EC.CALL_SIZES[:3]:
        tab, want, _ = profiled(monkeypatch, capfd, {}, call(size), "a call of %d" % size)
        long_cls[size] = cs[0].first_class(few=size <= EC.FEW_PAIRS)[0]
        assert tab.get((0, long_cls[size], 0), 0) >= 1
    assert long_cls[EC.FEW_PAIRS] == EC.CLS_WIDE0 + 2 and long_cls[EC.FEW_PAIRS - 1] == EC.CLS_WIDE0 + 2 and 0 < long_cls[EC.FEW_PAIRS + 1] < EC.NBAND, long_cls
    # on either side of the pilot's switch: the pilot reports its guess from 4096 pairs on
    for size in EC.CALL_SIZES[3:]:
        with Session(monkeypatch, {"SVX_EDIT_PROFILE": "1"}) as s:
            capfd.readouterr()
            s.check(call(size), "a call of %d (profiled, no guess pinned)" % size)
            assert ('"edit_guess_pilot"' in capfd.readouterr().err) == (size >= EC.PILOT_PAIRS), size
    for env in ({}, {"SVX_EDIT_FEW_PAIRS": "0"}, {"SVX_EDIT_GUESS": EC.GUESS}, {"SVX_EDIT_FEW_PAIRS": "100000"}, {"SVX_EDIT_FORCE_FULL": "1"}):
        with Session(monkeypatch, env) as s:
            for size in EC.CALL_SIZES:
                s.check(call(size), "a call of %d" % size)
