"""CLUSTER on the CPU: the oracle (oracle/svx_oracle.c: svo_form_partitions, svo_cluster, span_position_distance, svo_linkage_fcluster, consolidate, calc_score)
against what the REFERENCE returned for the directed cases of tests/cluster_cases.py (tests/golden/g_cluster_cases.json.gz, written by
tests/golden/make_golden_cluster.py, which also confirmed every expectation the cases' author wrote down) - family by family and case by case: partitions,
clusters (the existing 1e-9 on score and deviations, everything else exact), pair distances bit for bit - , a coverage table (every threshold has a case on each
side it needs), and a mutant table: 59 one-step changes of the oracle's clustering code, each compiled on its own and held to the same golden; the comparison
must FAIL for every one of them.  tests/test_gpu_cluster_cases.py holds the device to the same file.

The child process of the mutant test is tests/cluster_child.py, which also holds what this module shares with the GPU module."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import cluster_cases as CC
import cluster_child as K
import helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ORACLE_C = os.path.join(REPO, "oracle", "svx_oracle.c")
FAMILIES = CC.families()
NAMES = [f.name for f in FAMILIES]


@pytest.fixture(scope="module")
def cluster_oracle(oracle):
    oracle.set_genome(*K.genome_arrays())
    return oracle


def golden_family(name):
    return next(f for f in H.load(K.GOLDEN)["families"] if f["name"] == name)


def test_golden_is_the_cases_of_this_tree():
    """the rows, options, row ranges and pairs the golden was computed from are the ones tests/cluster_cases.py builds today; the reference raised exactly where the
    cases say so; the file stays well under the size of g5_cluster.json.gz"""
    g = H.load(K.GOLDEN)
    assert g["references"] == CC.REFS == H.REFS and g["raises"] == CC.EXPECTED_RAISES and sorted(g["raises"]) == sorted(n for n, _, _ in CC.REFUSED)
    assert [f["name"] for f in g["families"]] == NAMES
    for gf, f in zip(g["families"], FAMILIES):
        assert gf["signatures"] == f.rows() and gf["independent"] == f.independent, f.name
        assert {k: v for k, v in gf["options"].items() if k != "genome"} == f.options, f.name
        assert [(c["name"], c["range"]) for c in gf["cases"]] == [(c.name, list(r)) for c, r in zip(f.cases, f.ranges())], f.name
        for gc, c, (lo, hi) in zip(gf["cases"], f.cases, f.ranges()):
            assert [(i - lo, j - lo) for i, j, _ in gc["pairs"]] == c.pairs, (f.name, c.name)
        assert 0 < len(gf["signatures"]) < 5000
    assert sum(len(f.cases) for f in FAMILIES) == 205
    assert os.path.getsize(os.path.join(H.GOLDEN, K.GOLDEN)) < os.path.getsize(os.path.join(H.GOLDEN, "g5_cluster.json.gz")) // 4


def test_every_threshold_has_a_case_on_each_side():
    """The coverage table: tests/cluster_cases.py tags every case with the thresholds it sits below, on or above; every threshold of cluster_cases.REQUIRED must
    have a case on each side listed there, so a later edit of the cases cannot silently lose one.  The device-shape sides are checked on the golden's own
    partitions: the sizes 48, 49, 72, 73 and 100, more than 64 clusters in one partition, a partition of 73 or more left with 2 and with 1 members."""
    table = CC.coverage(FAMILIES)
    assert sorted(table) == sorted(CC.REQUIRED)
    for name, sides in CC.REQUIRED.items():
        for side in sides:
            assert table[name].get(side), "no case %s %r" % (side, name)
    shape = golden_family("shape")
    sizes = {t: {len(q) for q in p["partitions"]} for t, p in zip(CC.TYPES, shape["partitions"])}
    slot = {"DEL": 0, "INS": 1, "DUP_INT": 4}
    for typ in CC.SHAPE_TYPES:
        assert set(CC.SHAPE_SIZES) | {65} <= sizes[typ], (typ, sizes[typ])
        member_col = 7 if slot[typ] < 3 else 10
        per_part = []
        for q in shape["partitions"][CC.TYPES.index(typ)]["partitions"]:
            mine = [c for c in shape["clusters"][slot[typ]] if c[member_col][0] in q]
            per_part.append((len(q), len(mine), sum(len(c[member_col]) for c in mine)))
        assert {(100, 100, 100), (65, 65, 65), (100, 2, 100), (100, 50, 100), (73, 1, 2), (100, 1, 1)} <= set(per_part), (typ, sorted(set(per_part)))
    big = golden_family("sample")
    assert all({100, 101} <= {len(q) for q in p["partitions"]} for p in big["partitions"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference_family_by_family(cluster_oracle, name):
    d = K.oracle_family_difference(cluster_oracle, golden_family(name))
    assert d is None, d


def restricted(fam, lo, hi):
    """the golden of a family cut down to the rows [lo, hi) of one case, row numbers from 0"""
    clusters = []
    for k, lst in enumerate(fam["clusters"]):
        m = 7 if k < 3 else 10
        clusters.append([c[:m] + [[i - lo for i in c[m]]] + c[m + 1:] for c in lst if lo <= c[m][0] < hi])
    parts = [{"type": p["type"], "partitions": [[i - lo for i in q] for q in p["partitions"] if lo <= q[0] < hi]} for p in fam["partitions"]]
    return {"name": fam["name"], "options": fam["options"], "signatures": fam["signatures"][lo:hi], "clusters": clusters, "partitions": parts}


@pytest.mark.parametrize("name", [f.name for f in FAMILIES if f.independent])
def test_oracle_against_the_reference_case_by_case(cluster_oracle, name):
    """every case ALONE through the oracle: the partitions and clusters the reference gave it inside its family (the generator checked that they are the ones it
    gives the case alone), the pair distances bit for bit"""
    fam = golden_family(name)
    for c in fam["cases"]:
        lo, hi = c["range"]
        one = restricted(fam, lo, hi)
        one["cases"] = [{"name": c["name"], "range": [0, hi - lo], "pairs": [[i - lo, j - lo, h] for i, j, h in c["pairs"]]}]
        assert sum(len(q) for p in one["partitions"] for q in p["partitions"]) == hi - lo, c["name"]
        d = K.oracle_family_difference(cluster_oracle, one)
        assert d is None, "case %r alone: %s" % (c["name"], d)


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------------------
# The partition loop exists twice (svo_cluster, 16 blanks deep; svo_form_partitions, 12 blanks deep after a line break) and so do the sort keys (told apart by
# the line that follows the sort): each copy is mutated, the first shows in the clusters, the second in the partitions.
_C, _P = " " * 16, "\n" + " " * 12
_INS_GAP = "if (type == SVX_INS) { if (v->contig[a] != v->contig[b]) inf = 1; dist = (int64_t)v->start[b] - v->start[a]; }"
_DINT_GAP = "else if (type == SVX_DUP_INT) { if (v->contig2[a] != v->contig2[b] || v->contig[a] != v->contig[b]) inf = 1; dist = (int64_t)v->pos2[b] - v->pos2[a]; }"
_ELSE_GAP = "else { if (v->contig[a] != v->contig[b]) inf = 1; dist = (int64_t)v->start[b] - v->end[a]; }"
_CLAMP = "if (dist < 0) dist = 0;"
_KEYS = """            case SVX_INS: k.r1 = rank[v->contig[i]]; k.coord = v->start[i]; break;
            case SVX_DUP_INT: k.r1 = rank[v->contig2[i]]; k.r2 = rank[v->contig[i]]; k.coord = v->pos2[i]; break;
            case SVX_BND: k.r1 = rank[v->contig[i]]; k.coord = v->start[i]; break;
            default: k.r1 = rank[v->contig[i]]; k.coord = v->end[i]; break;
        }
        keys[i] = k;
    }
    qsort(keys, (size_t)n, sizeof(skey), cmp_skey);
"""
_KEYS_C, _KEYS_P = _KEYS + "    int64_t global_part = 0;", _KEYS + "    int64_t pid = -1;"
_BND_DEST = """v->contig2[k] = m[0].contig2; v->start2[k] = (int32_t)py_round_half_even(davg_s); v->end2[k] = (int32_t)py_round_half_even(davg_e);
        v->aux[k] = (uint8_t)m[0].aux;"""

# (a snippet of oracle/svx_oracle.c that occurs exactly once, the text inside it, its replacement)
MUTANTS = [
    # form_partitions: `> max_distance`, the max(0, .) clamp, each type's gap rule, the contig conditions, the sort keys
    ("if (inf || dist > p->partition_max_distance) break;", "dist >", "dist >="),
    ("newp = inf || dist > max_distance;", "dist >", "dist >="),
    (_C + _CLAMP, "dist = 0;", "dist = -dist;"), (_P + _CLAMP, "dist = 0;", "dist = -dist;"),
    (_C + _CLAMP, "if (dist < 0) dist = 0;", "if (dist < 1) dist = 1;"), (_P + _CLAMP, "if (dist < 0) dist = 0;", "if (dist < 1) dist = 1;"),
    (_C + _INS_GAP, "- v->start[a]", "- v->end[a]"), (_P + _INS_GAP, "- v->start[a]", "- v->end[a]"),
    (_C + _DINT_GAP, "- v->pos2[a]", "- (v->pos2[a] + v->end[a] - v->start[a])"), (_P + _DINT_GAP, "- v->pos2[a]", "- (v->pos2[a] + v->end[a] - v->start[a])"),
    (_C + _ELSE_GAP, "- v->end[a]", "- v->start[a]"), (_P + _ELSE_GAP, "- v->end[a]", "- v->start[a]"),
    (_C + _ELSE_GAP, "- v->end[a]", "- (v->end[a] - 1)"), (_P + _ELSE_GAP, "- v->end[a]", "- (v->end[a] - 1)"),
    (_C + _DINT_GAP, " || v->contig[a] != v->contig[b]", ""), (_P + _DINT_GAP, " || v->contig[a] != v->contig[b]", ""),
    (_KEYS_C, "case SVX_INS: k.r1 = rank[v->contig[i]]; k.coord = v->start[i];", "case SVX_INS: k.r1 = rank[v->contig[i]]; k.coord = v->end[i];"),
    (_KEYS_P, "case SVX_INS: k.r1 = rank[v->contig[i]]; k.coord = v->start[i];", "case SVX_INS: k.r1 = rank[v->contig[i]]; k.coord = v->end[i];"),
    (_KEYS_C, "k.coord = v->end[i];", "k.coord = v->start[i];"), (_KEYS_P, "k.coord = v->end[i];", "k.coord = v->start[i];"),
    (_KEYS_C, "k.r1 = rank[v->contig2[i]]; k.r2 = rank[v->contig[i]];", "k.r2 = rank[v->contig2[i]]; k.r1 = rank[v->contig[i]];"),
    (_KEYS_P, "k.r1 = rank[v->contig2[i]]; k.r2 = rank[v->contig[i]];", "k.r2 = rank[v->contig2[i]]; k.r1 = rank[v->contig[i]];"),
    # clusters_from_partitions: `> 100`, the seed, the INV exemption (twice), `<= cluster_max_distance`, "any earlier element, dropped or not", the 99999
    ("if (psize > 100) {", "> 100", ">= 100"),
    ("mt_seed_int(&rng, 1524u);", "1524u", "1525u"),
    ("    if (type != SVX_INV) {\n", "type != SVX_INV", "1"),
    ("if (type != SVX_INV && mm[i].read_id == mm[j].read_id) cd[q++] = 99999.0;", "type != SVX_INV && ", ""),
    ("if (d <= p->cluster_max_distance) dup[j] = 1;", "<=", "<"),
    ("            if (m[i].read_id == m[j].read_id) {", "if (m[i]", "if (!dup[i] && m[i]"),
    ("if (type != SVX_INV && mm[i].read_id == mm[j].read_id) cd[q++] = 99999.0;", "type != SVX_INV && mm[i].read_id == mm[j].read_id", "0"),
    ("if (type != SVX_INV && mm[i].read_id == mm[j].read_id) cd[q++] = 99999.0;", "99999.0", "1.0"),
    # span_position_distance
    ("int64_t mx = span1 > span2 ? span1 : span2;", "span1 > span2", "span1 < span2"),
    ("static inline int64_t floordiv2(int64_t x) { return (x >= 0) ? x / 2 :", "? x / 2 :", "? (x + 1) / 2 :"),
    ("if (a->aux == b->aux) return (double)(d1 + d2) / 3000.0;", "a->aux == b->aux", "(a->aux & 1) == (b->aux & 1)"),
    ("if (a->aux == b->aux) return (double)(d1 + d2) / 3000.0;", "a->aux == b->aux", "(a->aux & 2) == (b->aux & 2)"),
    ("if (a->aux == b->aux) return (double)(d1 + d2) / 3000.0;", "3000.0", "3001.0"),
    ("return pds + pdd + sd;", "pds + pdd + sd", "pds + sd"),
    ("if (pd > 2 * p->cluster_max_distance) {", "pd > 2", "pd >= 2"),
    # linkage and fcluster
    ("if (dist < cur) { cur = dist; y = i; }", "dist < cur", "dist <= cur"),
    ("Z[4 * ord[j] + 2] > Z[4 * v + 2]", "] > Z[", "] >= Z["),
    ("if (x > y) { int t = x; x = y; y = t; }", "x > y", "0"),
    ("if (leader == -1 && MD[root] <= cutoff) { leader = root; ncl++; }", "<= cutoff", "< cutoff"),
    # score
    ("double a = std_span / span; sds = 1 - (a < 1 ? a : 1);", "(a < 1 ? a : 1)", "a"),
    ("double b = std_pos / span;  pds = 1 - (b < 1 ? b : 1);", "(b < 1 ? b : 1)", "b"),
    ("num = valid < 80 ? valid : 80;", "valid < 80 ? valid : 80", "valid < 81 ? valid : 81"),
    ("} else num = n < 80 ? n : 80;", "n < 80 ? n : 80", "n < 81 ? n : 81"),
    ("int valid = (left < right ? left : right) + cnt[4];", "left < right", "left > right"),
    ("int valid = (left < right ? left : right) + cnt[4];", " + cnt[4]", ""),
    # consolidation
    ("static double py_round_half_even(double x) { return nearbyint(x); }", "nearbyint(x)", "floor(x + 0.5)"),
    ("    int has = n > 1;", "n > 1", "n > 2"),
    ("int64_t maxc = 0; for (int i = 0; i < n; i++) if (m[i].pos2 > maxc) maxc = m[i].pos2;", "if (m[i].pos2 > maxc)", "if (i == 0)"),
    (_BND_DEST, "m[0].contig2", "m[n - 1].contig2"),
    (_BND_DEST, "(uint8_t)m[0].aux", "(uint8_t)0"),
    ("v->score[k] = calc_score(m, n, 1, std_pos, dpo, 500.0, type);", "500.0", "501.0"),
    ("davg_e = (double)(ds + n) / (double)n;", "(ds + n)", "(ds)"),
    ("double mspan = (std_span + dsp) / 2.0, mpos = (std_pos + dpo) / 2.0;", "(std_span + dsp) / 2.0", "(std_span + dsp) / 1.0"),
    ("double mspan = (std_span + dsp) / 2.0, mpos = (std_pos + dpo) / 2.0;", "(std_pos + dpo) / 2.0", "(std_pos + dpo) / 1.0"),
    ("double span = ((avg_e - avg_s) + (davg_e - davg_s)) / 2.0;", "/ 2.0", "/ 1.0"),
    ("v->std_span[k] = std_pos; v->std_pos[k] = dpo;", "v->std_span[k] = std_pos; v->std_pos[k] = dpo;", "v->std_span[k] = dpo; v->std_pos[k] = std_pos;"),
    ("ck[k].coord = (int64_t)out->start[g] + out->end[g]; ck[k].idx = k; }", "(int64_t)out->start[g] + out->end[g]", "(int64_t)out->end[g]"),
]
# NOT in the list, because no input can tell them from the original:
# * dropping the clamp `if (dist < 0) dist = 0;`: a negative distance is never > partition_max_distance while that is >= 0 (the clamp is mutated to -dist and to 1);
# * `m[0].aux` -> another member's: a BND cluster never mixes direction pairs (unequal pairs are 99999 apart); DUP_INT's `m[0].contig2` -> another member's: a
#   DUP_INT partition has one destination contig; the `500.0` of a one-member BND cluster: the span is not used without deviations;
# * the `MD[l - n] > m` / `MD[r - n] > m` maxima of get_max_dist_for_each_cluster: average linkage never merges below the height of a child, so the maximum over a
#   subtree is the node's own height;
# * the `ss -= sd * sd / n` correction of the deviation: the sum of the residuals about the FP64 mean is a rounding error, far inside the 1e-9 of the comparison.


def makefile_flags():
    with open(os.path.join(REPO, "oracle", "Makefile")) as fh:
        line = next(l for l in fh if l.startswith("CFLAGS"))
    return [f for f in line.split("=", 1)[1].split() if not f.startswith("-O")] + ["-O0"]


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
    run = subprocess.run([sys.executable, os.path.abspath(K.__file__)], env=env, capture_output=True, text=True)
    return k, run.returncode, (run.stdout + run.stderr)[-2000:]


def test_no_mutant_of_the_clustering_survives_the_golden(tmp_path):
    """Every entry of MUTANTS (59) names one snippet of oracle/svx_oracle.c that occurs exactly once and a one-step change of it; the mutated source is compiled
    with the Makefile's flags at -O0 and loaded by a child process through SVX_ORACLE_LIB; the child (tests/cluster_child.py) compares the oracle with
    g_cluster_cases.json.gz and must report a difference (exit status cluster_child.DIFFERENT, which nothing else ends a Python process with: a child that dies of
    an exception does not count as a detection).  The unchanged source goes the same way and must agree (exit status 0): a difference is the mutant's, not the
    build's."""
    with open(ORACLE_C) as fh:
        src = fh.read()
    jobs, seen = [(0, src, str(tmp_path))], set()
    for k, (snippet, old, new) in enumerate(MUTANTS, 1):
        assert src.count(snippet) == 1, "mutant %d: %r occurs %d times" % (k, snippet, src.count(snippet))
        assert snippet.count(old) == 1, "mutant %d: %r occurs %d times in %r" % (k, old, snippet.count(old), snippet)
        mutated = src.replace(snippet, snippet.replace(old, new))
        assert mutated != src and mutated not in seen, "mutant %d changes nothing new" % k
        seen.add(mutated)
        jobs.append((k, mutated, str(tmp_path)))
    with ThreadPoolExecutor(max_workers=min(8, H.granted_cpus())) as pool:
        results = sorted(pool.map(run_one, jobs))
    assert results[0][1] == 0, "the unchanged oracle against the golden: %r" % (results[0],)
    survivors = ["%d: %r -> %r in %r (exit %r) %s" % (k, MUTANTS[k - 1][1], MUTANTS[k - 1][2], MUTANTS[k - 1][0][:80], rc, out.strip()[-300:])
                 for k, rc, out in results[1:] if rc != K.DIFFERENT]
    assert not survivors, "%d of %d mutants not detected:\n%s" % (len(survivors), len(MUTANTS), "\n".join(survivors))
    assert len(MUTANTS) == 59
