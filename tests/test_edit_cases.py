"""The directed edit-distance cases on the CPU (tests/edit_cases.py; no GPU): the generator against the golden's hashes, the plain DP against the pure-Python one,
the oracle's bit-vector against the DP at lengths it was never held to a DP at, the window model and its mutants, and the table of what the cases reach."""
import ast
import collections
import os

import pytest

import edit_cases as EC
import helpers as H

GOLDEN = "g_edit_cases.json.gz"


@pytest.fixture(scope="module")
def gold():
    return {(r[0], r[1]): r for r in H.load(GOLDEN)["cases"]}


@pytest.fixture(scope="module")
def levenshtein_dp():
    """the pure-Python DP of tests/golden/make_golden.py, taken from its source: importing that module needs the reference checkout"""
    path = os.path.join(H.GOLDEN, "make_golden.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "levenshtein_dp"]
    assert len(fn) == 1
    ns = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["levenshtein_dp"]


def test_generator_reproduces_the_golden(gold):
    cases = EC.all_cases()
    assert len(cases) == len(gold)
    for c in cases:
        r = gold[(c.family, c.name)]
        assert (len(c.a), len(c.b), c.sha1()) == (r[2], r[3], r[4]), (c.family, c.name)
    print("cases per family:", dict(collections.Counter(c.family for c in cases)))


def test_levenshtein_rows_vs_pure_python(gold, levenshtein_dp):
    g = H.load("g_editdistance.json.gz")
    for a, b, d in g["cases"]:
        assert EC.levenshtein_rows(a, b) == d == levenshtein_dp(a, b)
        assert EC.levenshtein_rows(b, a) == d
        assert int(EC.levenshtein_matrix(a, b)[-1, -1]) == d
    seen, n = set(), 0
    for c in EC.all_cases():
        if c.name.endswith(" [N]"):
            continue                                         # the pair before it behind one shared symbol: the golden takes its value from that pair
        if len(c.a) * len(c.b) <= 250000 and (c.a, c.b) not in seen:
            seen.add((c.a, c.b))
            n += 1
            assert levenshtein_dp(c.a, c.b) == gold[(c.family, c.name)][5], (c.family, c.name)
    print("%d directed cases of at most 250 000 cells held to the pure-Python DP" % n)
    # the matrix variant: every cell, on small cases of every family that has some
    for c in [c for c in EC.all_cases() if 0 < len(c.a) * len(c.b) <= 4000][::25]:
        D = EC.levenshtein_matrix(c.a, c.b)
        assert int(D[-1, -1]) == gold[(c.family, c.name)][5]
        assert all(int(D[i, j]) == levenshtein_dp(c.a[:i], c.b[:j]) for i in (1, len(c.a) // 2, len(c.a)) for j in (1, len(c.b) // 2, len(c.b)))


def test_oracle_equals_the_dp_on_every_case(oracle, gold):
    bad, seen = [], {}
    for k, c in enumerate(EC.all_cases()):
        if (c.a, c.b) not in seen:
            seen[(c.a, c.b)] = oracle.edit_distance(c.a, c.b)
            if k % 7 == 0:
                assert oracle.edit_distance(c.b, c.a) == seen[(c.a, c.b)], (c.family, c.name)
        if seen[(c.a, c.b)] != gold[(c.family, c.name)][5]:
            bad.append((c.family, c.name, seen[(c.a, c.b)], gold[(c.family, c.name)][5]))
    assert not bad, bad[:10]


def test_restated_geometry():
    """what the restated constants imply, checked against the statements of edit.hip's comments"""
    assert [EC.band_words(b) for b in range(EC.NBAND)] == [1, 3, 4, 6, 8, 10, 12, 14, 16]
    assert [EC.band_class_for(w) for w in (18, 19, 50, 51, 82, 83, 146, 466, 467)] == [0, 1, 1, 2, 2, 3, 3, 8, EC.CLS_FULL]
    for cls in range(1, EC.NBAND):
        for delta in range(0, 40):
            off, margin = EC.stair_geometry(500, 500 + delta, EC.band_words(cls))
            assert off % 8 == 7
            # a window chosen by need_window certifies: the slack of 46 covers the alignment and the 32 columns the window stands still
            need = 32 * EC.band_words(cls) - EC.SLACK_STAIR
            x = (need - 1 - delta) // 2
            assert x < 0 or margin >= x, (cls, delta, margin, x)
    for delta in range(0, 18):                              # class 0 is entered only through a bound: need_window <= 18, and its margin holds that x with room
        x_max = (18 - 1 - delta) // 2
        assert EC.slide_geometry(100, 100 + delta)[1] >= x_max, delta
    # band_retry at least doubles the words, so 10 words and more fail into the full matrix; and the class it picks holds the returned cost's window unless it is
    # clamped to hi (4 x the words), which can only fail into the full matrix: a pair sees at most two band rounds
    for cls in range(1, EC.NBAND):
        lo, hi = EC.band_class_with_words(2 * EC.band_words(cls)), EC.band_class_with_words(4 * EC.band_words(cls))
        assert (lo == EC.CLS_FULL) == (EC.band_words(cls) > 8)
        assert hi == EC.CLS_FULL or EC.band_class_with_words(2 * EC.band_words(hi)) == EC.CLS_FULL


def test_margin_cases_sit_on_their_margin(gold):
    """every margin case starts in the class it names; the model accepts it exactly when floor((d - delta) / 2) <= margin, with the DP's value, narrowing or not"""
    n = collections.Counter()
    for c in EC.family("margin"):
        if c.generic or not c.name.startswith("c") or "k=margin" not in c.name:
            continue
        if int(c.name.split()[1][5:]) not in (0, 9, 33) and c.name[:2] not in ("c1", "c2"):
            continue                                         # (3 and 4 words at every gap, the wider classes at the edges of the gap: the GPU test runs them all)
        cls, _, m, nn, ub = c.first_class()
        assert cls == int(c.name[1]), c.name
        d = gold[(c.family, c.name)][5]
        p, t = EC.cores(c.a, c.b)
        for narrow in (True, False):
            r = EC.window_model(p, t, cls, ub, narrow)
            assert r["accepted"] == ((d - (nn - m)) // 2 <= r["margin"]), (c.name, r)
            assert not r["accepted"] or r["d"] == d, (c.name, r)
            assert r["d"] < 0 or r["d"] >= d, (c.name, r)
            n[(cls, r["accepted"])] += 1
    print("margin cases replayed {(class, accepted): attempts}:", dict(sorted(n.items())))
    for cls in range(1, EC.NBAND):
        assert n[(cls, True)] > 0 and n[(cls, False)] > 0, cls


def test_cut_cases_sit_on_their_threshold(gold):
    """every cut case has, at the block its name gives, the quantity of stair_block its name gives; its attempt is ACCEPTED with the DP's value, no more than 9 below
    kcap (a wrong cut shows only where the second-best path still costs <= kcap); its excursion leaves at a column 32 k - 1, 32 k or 32 k + 1; and the lane of
    every veto wave does refuse the cut that its 63 wave-mates allow"""
    n, residues, model = collections.Counter(), set(), {}
    for c in EC.family("cut"):
        if c.generic or c.copies != 64:
            continue
        w = c.name.replace(",", "").split()
        cls, which, q, kb, leaves, room = int(w[0][1:]), w[4], int(w[6]), int(w[9]), int(w[15]), int(w[20])
        c0, _, m, nn, ub = c.first_class()
        assert c0 == cls, c.name
        p, t = EC.cores(c.a, c.b)
        r = model[c.name] = EC.window_model(p, t, cls, ub, True)
        ev = [e for e in r["events"] if e[0] == kb][0]
        assert (ev[2] if which == "top" else ev[3]) == q, (c.name, ev)
        assert (r["kcap"] == ub) == ("from ub" in c.name), (c.name, r["kcap"], ub)
        assert r["accepted"] and r["d"] == gold[(c.family, c.name)][5] and r["kcap"] - r["d"] == room and 0 <= room <= 9, (c.name, r["d"], r["kcap"])
        assert leaves % 32 in (31, 0, 1), c.name
        residues.add(leaves % 32)
        n[(cls, "ub" in w[3])] += 1
    print("cut cases on their threshold {(class, kcap from ub): pairs}:", dict(sorted(n.items())))
    assert residues == {31, 0, 1}
    assert all(n[(cls, src)] >= 3 for cls in range(2, EC.NBAND) for src in (False, True)) and sum(n.values()) >= 54, n
    vetoes = [c for c in EC.family("cut") if c.name.endswith("(the veto)") and not c.generic]
    assert len(vetoes) == 3
    for v in vetoes:
        w = v.wave.replace(",", "").split()
        cls, kb = int(w[1][1:]), int(w[10])
        c0, _, m, nn, ub = v.first_class()
        assert c0 == cls, v.name
        ev = [e for e in EC.window_model(*EC.cores(v.a, v.b), cls, ub, True)["events"] if e[0] == kb][0]
        mates = [e for e in model[v.wave[len("veto: "):]]["events"] if e[0] == kb][0]
        assert mates[4] and not ev[4] and (ev[2] is None or ev[2] <= 0), (v.name, ev, mates)


def test_retry_cases_walk_their_chain(gold):
    walked = collections.Counter()
    for c in EC.family("retry"):
        if c.generic:
            continue
        chain, val = EC.route_chain(c.a, c.b, c.guess)
        assert val is None or val == gold[(c.family, c.name)][5], c.name
        assert len(chain) >= 2, c.name
        for x, y in zip(chain, chain[1:]):
            walked[(x, y if y < EC.NBAND else "full matrix")] += 1
        if c.name == "chain from 3 words":
            assert chain[:2] == [1, 6] and chain[2] > EC.CLS_FULL, chain
        if c.name == "chain from 4 words":
            assert chain[:2] == [2, 8] and chain[2] > EC.CLS_FULL, chain
    print("retry steps {(class, next): cases}:", dict(sorted(walked.items(), key=str)))
    # every class between the clamps of band_retry, lo (2 x the words) and hi (4 x), is walked into from every class; beyond 16 words: the full matrix
    for cls in range(1, EC.NBAND):
        lo, hi = EC.band_class_with_words(2 * EC.band_words(cls)), EC.band_class_with_words(4 * EC.band_words(cls))
        nxt = {y for (x, y) in walked if x == cls}
        for y in range(lo, min(hi, EC.NBAND - 1) + 1):
            assert y in nxt, "no retry case walks from class %d into class %d; walked: %s" % (cls, y, sorted(nxt, key=str))
        if hi >= EC.NBAND:
            assert "full matrix" in nxt, cls


def test_mutants_of_the_window_model(gold):
    """every one-step mutant either reports a wrong distance on some case (killed) or has a written reason why none can"""
    g = {k: r[5] for k, r in gold.items()}
    rows = EC.mutant_table(g)
    print("mutant | killed by (case, accepted, DP) | cases tried")
    for name, hit, tried in rows:
        print("%s | %s | %d" % (name, hit if hit else "equivalent: " + EC.EQUIVALENT.get(name, "NO REASON")[:90] + "...", tried))
    killed = {name for name, hit, _ in rows if hit}
    assert killed >= {"stair: margin + 1", "top cut eager by 2", "bottom cut eager by 2"}, killed
    unexplained = [name for name, hit, _ in rows if not hit and name not in EC.EQUIVALENT]
    assert not unexplained, unexplained
    assert not (killed & set(EC.EQUIVALENT)), killed & set(EC.EQUIVALENT)


def test_coverage_of_the_routes():
    """{family: {(first class, alphabet): pairs}} - every band class in both alphabets by the margin, repeats and retry families, 4 to 16 words by the cut family,
    the one-lane and 2-lane full-matrix classes by the full family, k_edit_prep's own answers by the trim family"""
    table = {}
    for fam in EC.FAMILIES:
        t = collections.Counter()
        for c in EC.family(fam):
            r = c.first_class(few=fam in ("few", "full_long"))           # (as a call of few pairs sends them)
            t[(r[0], r[1])] += c.copies
        table[fam] = t
        print(fam, dict(sorted(t.items())))
    bands = {(cls, g) for cls in range(EC.NBAND) for g in (0, 1)}
    for fam in ("margin", "repeats"):
        assert bands <= set(table[fam]), (fam, sorted(bands - set(table[fam])))
    assert {(cls, g) for cls in range(1, EC.NBAND) for g in (0, 1)} <= set(table["retry"])
    assert {(cls, g) for cls in range(2, EC.NBAND) for g in (0, 1)} <= set(table["cut"])
    assert {(cls, 1) for cls in list(range(EC.CLS_LANE0, EC.CLS_LANE0 + 5)) + [EC.CLS_WIDE10, EC.CLS_WIDE12, EC.CLS_WIDE14, EC.CLS_WIDE0]} <= set(table["full"])
    assert (-1, 0) in table["trim"] and (-1, 1) in table["alphabet"]
    assert {(EC.CLS_LANE0 + 1, 0), (EC.CLS_WIDE0 + 2, 0)} <= set(table["few"])
    assert {k[0] for k in table["full_long"]} == {EC.CLS_WIDE0 + 3, EC.CLS_FULL}          # 8192 rows: the last 16-lane form; beyond: the systolic kernels
    assert len({c.generic for c in EC.family("alphabet")}) == 2
