"""The insertion haplotypes on the CPU: the oracle (oracle/svx_oracle.c: fetch, haplotype_edit_distance, the INS branch of span_position_distance) and the
definition in words (tests/hap_cases.py: haplotypes, distance) against what the REFERENCE returned for the directed cases of tests/hap_cases.py
(tests/golden/g_hap_cases.json.gz, written by tests/golden/make_golden_hap.py) - contig starts and ends, contigs shorter than a flank, an absent contig, every nibble
offset, the large shifts, the threshold of the near branch, the alphabet - and a mutant table: every step of the haplotype construction changed by one, compiled
on its own and held to the same golden; the comparison must FAIL for every one of them.  tests/test_gpu_hap_cases.py holds the device to the same file.

The child process of the mutant test is tests/hap_child.py; what this module shares with the GPU module is in tests/hap_checks.py."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import hap_cases as HC
import hap_child
import helpers as H
from hap_checks import GOLDEN, bits, genome_arrays, oracle_cluster_difference, oracle_pair_difference

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ORACLE_C = os.path.join(REPO, "oracle", "svx_oracle.c")
FAMILIES = {t.name: t for t in HC.families()}
CLUSTER_CASES = HC.cluster_cases()


@pytest.fixture(scope="module")
def hap_oracle(oracle):
    oracle.set_genome(*genome_arrays())
    return oracle


def test_golden_is_the_cases_of_this_tree():
    """the rows and pairs the golden was computed from are the ones tests/hap_cases.py builds today (digests), every pair is in it or definition-only, the
    reference raised exactly where the cases say so"""
    g = H.load(GOLDEN)
    assert g["references"] == HC.REFERENCES and g["lengths"] == [len(HC.GENOME.get(r, "")) for r in HC.REFERENCES]
    assert g["raises"] == HC.EXPECTED_RAISES
    assert [f["name"] for f in g["families"]] == list(FAMILIES)
    for f in g["families"]:
        t = FAMILIES[f["name"]]
        assert f["digest"] == t.digest() and f["n_rows"] == len(t.rows), f["name"]
        assert len(f["pairs"]) + f["n_definition_only"] == len(t.pairs)
        assert {r[0] for r in t.rows} == {"INS", "DEL", "INV", "BND"}
    assert [(c["name"], c["digest"]) for c in g["cluster_cases"]] == [(n, HC.rows_digest(r)) for n, r, _ in CLUSTER_CASES]


def test_golden_covers_what_the_cases_are_for():
    """from the golden and the definition: both branches at every threshold setting, haplotypes of every length 0..8, both strings empty, a left / right flank cut
    by the contig start / end and by both, span != len(sequence), shifts on both sides of 2047 and of the prepack limit"""
    g = H.load(GOLDEN)
    fam = {f["name"]: f for f in g["families"]}
    by_setting = {}
    for i, j, tag, params, hexd, ed in fam["threshold"]["pairs"]:
        by_setting.setdefault(tuple(params), set()).add(ed is None)
    assert sorted((p[0], p[2]) for p in by_setting) == sorted(HC.THRESHOLDS) and all(v == {True, False} for v in by_setting.values()), by_setting
    t = FAMILIES["tiny"]
    lens, spans = set(), set()
    for i, j, tag, params in t.pairs:
        a, b = HC.haplotypes(HC.GENOME, HC.sig(t.rows[i]), HC.sig(t.rows[j]))
        lens |= {len(a), len(b)}
        if not a and not b:
            lens.add("both empty")
        spans.add(t.rows[i][3] - t.rows[i][2] == len(t.rows[i][6]))
    assert set(range(9)) | {"both empty"} <= lens and spans == {True, False}
    shifts = {abs(FAMILIES["shift"].rows[i][2] - FAMILIES["shift"].rows[j][2]) for i, j, _, _ in FAMILIES["shift"].pairs}
    assert set(HC.SHIFTS) <= shifts
    assert all(p[5] is not None for p in fam["shift"]["pairs"])          # every one of them below its threshold
    cut = set()
    for name in ("start_edge", "end_edge"):
        t = FAMILIES[name]
        for i, j, tag, params in t.pairs:
            (c, s1, _, _), (_, s2, _, _) = HC.sig(t.rows[i]), HC.sig(t.rows[j])
            cut.add((min(s1, s2) < HC.PAD, max(s1, s2) + HC.PAD > len(HC.GENOME[c])))
    assert cut == {(True, False), (False, True), (True, True), (False, False)}
    n_pairs = sum(len(t.pairs) for t in FAMILIES.values())
    assert 2000 < n_pairs < 5000


@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_and_definition_against_the_reference(hap_oracle, name):
    """per golden pair: the oracle's span_position_distance has the reference's bit pattern; the definition in words, fed with the oracle's edit distance of the
    definition's own strings, has it too; the reference's integer edit distance is the oracle's of those strings.  Definition-only pairs: oracle == definition."""
    g = H.load(GOLDEN)
    t = FAMILIES[name]
    d = oracle_pair_difference(hap_oracle, g, t)
    assert d is None, d
    fam = next(f for f in g["families"] if f["name"] == name)
    for i, j, tag, params, hexd, ed in fam["pairs"]:
        s1, s2 = HC.sig(t.rows[i]), HC.sig(t.rows[j])
        a, b = HC.haplotypes(HC.GENOME, s1, s2)
        near = HC.needs_edit(s1, s2, tuple(params))
        assert near == (ed is not None), (name, tag)
        mine = hap_oracle.edit_distance(a, b) if near else None
        assert mine == ed, (name, tag, mine, ed)
        assert bits(HC.distance(HC.GENOME, s1, s2, tuple(params), mine)) == hexd, (name, tag)


@pytest.mark.parametrize("idx", range(len(CLUSTER_CASES)))
def test_oracle_clusters_against_the_reference(hap_oracle, idx):
    g = H.load(GOLDEN)
    name, rows, opts = CLUSTER_CASES[idx]
    assert g["cluster_cases"][idx]["options"] == opts
    d = oracle_cluster_difference(hap_oracle, g["cluster_cases"][idx], name, rows, opts)
    assert d is None, d
    assert len(g["cluster_cases"][idx]["clusters"][1]) >= 1


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------------------
_FETCH = "static int64_t fetch(const svo_ctx* c, int32_t contig, int64_t a, int64_t b, uint8_t* out) {"
_LEN = "int64_t len = c->g_off[contig + 1] - c->g_off[contig];"
_WS, _WE = "int64_t ws = (s1->start < s2->start", "int64_t we = (s1->start > s2->start"
_L1, _R1 = "int64_t l1 = fetch(c, s1->contig, ws, s1->start, h1);", "l1 += fetch(c, s1->contig, s1->start, we, h1 + l1);"
_L2, _R2 = "int64_t l2 = fetch(c, s2->contig, ws, s2->start, h2);", "l2 += fetch(c, s2->contig, s2->start, we, h2 + l2);"
_M1, _M2 = "memcpy(h1 + l1, s1->seq, (size_t)s1->seq_len); l1 += s1->seq_len;", "memcpy(h2 + l2, s2->seq, (size_t)s2->seq_len); l2 += s2->seq_len;"

# (consecutive source lines that name the place - each stripped, a prefix is enough - , [(text inside them, its replacement), ...]): one step each of the haplotype
# construction of oracle/svx_oracle.c (fetch, haplotype_edit_distance) and the threshold of the near branch.
# NOT in the list, because no input can tell it from the original: dropping fetch's second `max(0, .)` (`if (b < 0) b = 0;`) - the first one has raised `a` to
# at least 0 by then, so a negative `b` gives `a >= b` and the empty string either way (and no bound is negative while starts are not).
MUTANTS = [
    ([_FETCH, "if (a < 0) a = 0;"], [("if (a < 0) a = 0;", "")]),                                              # drop max(0, window start)
    ([_LEN, "if (b > len) b = len;"], [("if (b > len) b = len;", "")]),                                         # drop the end clip
    ([_LEN, "if (b > len) b = len;"], [("if (b > len) b = len;", "if (b > len + 1) b = len + 1;")]),
    ([_LEN, "if (b > len) b = len;"], [("if (b > len) b = len;", "if (b > len - 1) b = len - 1;")]),
    ([_WS], [("- 100;", "- 99;")]), ([_WS], [("- 100;", "- 101;")]),                                            # window padding
    ([_WE], [("+ 100;", "+ 99;")]), ([_WE], [("+ 100;", "+ 101;")]),
    ([_WS], [("s1->start < s2->start", "s1->start > s2->start")]),                                              # min <-> max
    ([_WE], [("s1->start > s2->start", "s1->start < s2->start")]),
    ([_L1], [("ws, s1->start", "ws, s2->start")]), ([_R1], [("s1->start, we", "s2->start, we")]),               # s1 for s2 in either fetch of either haplotype
    ([_L2], [("ws, s2->start", "ws, s1->start")]), ([_R2], [("s2->start, we", "s1->start, we")]),
    ([_L1], [("s1->contig", "s2->contig")]), ([_R1], [("s1->contig", "s2->contig")]),                           # ... and the other signature's contig
    ([_L2], [("s2->contig", "s1->contig")]), ([_R2], [("s2->contig", "s1->contig")]),
    ([_L1, _M1, _R1], [("ws, s1->start, h1)", "s1->start, we, h1)"), ("s1->start, we, h1 + l1)", "ws, s1->start, h1 + l1)")]),      # flank order
    ([_L2, _M2, _R2], [("ws, s2->start, h2)", "s2->start, we, h2)"), ("s2->start, we, h2 + l2)", "ws, s2->start, h2 + l2)")]),
    (["if (pd > 2 * p->cluster_max_distance) {", "double sd = (double)llabs(span1 - span2) / (double)mx;"], [("pd > 2", "pd >= 2")]),      # > <-> >= on the threshold
]
# every build, the unchanged one too, gets haplotype buffers with room for what a mutant may write (two flanks of the whole window each)
_ROOM = ("int64_t cap1 = (we - ws) + s1->seq_len + 8, cap2 = (we - ws) + s2->seq_len + 8;",
         "int64_t cap1 = 2 * (we - ws) + s1->seq_len + 1024, cap2 = 2 * (we - ws) + s2->seq_len + 1024;")


def place(src_lines, anchors):
    """the exact source text of the consecutive lines the anchors name"""
    norm = lambda t: " ".join(t.split())          # noqa: E731
    hits = [i for i in range(len(src_lines) - len(anchors) + 1) if all(norm(src_lines[i + k]).startswith(norm(a)) for k, a in enumerate(anchors))]
    assert len(hits) == 1, "%r names %d places" % (anchors, len(hits))
    return "\n".join(src_lines[hits[0]:hits[0] + len(anchors)])


def makefile_flags():
    with open(os.path.join(REPO, "oracle", "Makefile")) as fh:
        line = next(l for l in fh if l.startswith("CFLAGS"))
    return [f for f in line.split("=", 1)[1].split() if not f.startswith("-O")] + ["-O1"]


def run_one(job):
    k, source, workdir = job
    c_path, so_path = os.path.join(workdir, "m%03d.c" % k), os.path.join(workdir, "m%03d.so" % k)
    with open(c_path, "w") as fh:
        fh.write(source)
    cc = subprocess.run([os.environ.get("CC", "gcc")] + makefile_flags() + ["-w", "-I", os.path.join(REPO, "include"), "-shared", "-o", so_path, c_path, "-lm", "-lpthread"],
                        capture_output=True, text=True)
    if cc.returncode:
        return k, "compile", cc.stderr[-2000:]
    env = dict(os.environ, SVX_ORACLE_LIB=so_path, PYTHONDONTWRITEBYTECODE="1")
    run = subprocess.run([sys.executable, os.path.abspath(hap_child.__file__)], env=env, capture_output=True, text=True)
    return k, run.returncode, (run.stdout + run.stderr)[-2000:]


def test_no_mutant_of_the_haplotype_construction_survives_the_golden(tmp_path):
    """Every entry of MUTANTS names one place of oracle/svx_oracle.c (the snippet occurs exactly once), is compiled with the Makefile's flags and loaded by a child
    process through SVX_ORACLE_LIB; the child compares the oracle with g_hap_cases.json.gz and must report a difference (exit status hap_child.DIFFERENT, which
    nothing else ends a Python process with).  The unchanged source goes the same way and must agree (exit status 0): a difference is the mutant's, not the build's."""
    with open(ORACLE_C) as fh:
        src = fh.read()
    assert src.count(_ROOM[0]) == 1
    src = src.replace(*_ROOM)
    lines = src.split("\n")
    jobs, seen = [(0, src, str(tmp_path))], set()
    for k, (anchors, edits) in enumerate(MUTANTS, 1):
        snippet = place(lines, anchors)
        assert src.count(snippet) == 1, "mutant %d: %r occurs %d times" % (k, snippet, src.count(snippet))
        changed = snippet
        for old, new in edits:
            assert changed.count(old) == 1, "mutant %d: %r occurs %d times in %r" % (k, old, changed.count(old), changed)
            changed = changed.replace(old, new)
        mutated = src.replace(snippet, changed)
        assert mutated != src and mutated not in seen, "mutant %d changes nothing new" % k
        seen.add(mutated)
        jobs.append((k, mutated, str(tmp_path)))
    with ThreadPoolExecutor(max_workers=min(8, H.granted_cpus())) as pool:
        results = sorted(pool.map(run_one, jobs))
    assert results[0][1] == 0, "the unchanged oracle against the golden: %r" % (results[0],)
    survivors = ["%d: %r at %r (exit %r) %s" % (k, MUTANTS[k - 1][1], MUTANTS[k - 1][0][-1], rc, out.strip()[-300:]) for k, rc, out in results[1:] if rc != hap_child.DIFFERENT]
    assert not survivors, "%d of %d mutants not detected:\n%s" % (len(survivors), len(MUTANTS), "\n".join(survivors))
    assert len(MUTANTS) == 21
