"""GENOTYPE on the CPU: the oracle (oracle/svx_oracle.c: svo_genotype) under SVIM_genotyping.genotype, and the table route stated in Python over the oracle's join,
against what the REFERENCE returned for the directed cases of tests/genotype_walk_cases.py (tests/golden/g_genotype_cases.json.gz, written by
tests/golden/make_golden_genotype.py, which also confirmed every expectation the cases' author wrote down); a coverage table (every comparison has a case on each
side it needs); the refusals; and two mutant tables: MUTANTS, one-step changes of svo_genotype, each compiled on its own and held to the same golden - the
comparison must FAIL for every one of them - and EQUIVALENT, three changes no input can tell from the original, which must PASS.
tests/test_gpu_genotype_cases.py holds the device to the same file.

The child process of the mutant test is tests/genotype_child.py, which also holds what this module shares with the GPU module."""
import os
import subprocess
import sys
import types
from concurrent.futures import ThreadPoolExecutor

import pytest

import genotype_cases as GC
import genotype_child as K
import genotype_walk_cases as W
import helpers as H
from svim_amd import SVIM_genotyping, records

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ORACLE_C = os.path.join(REPO, "oracle", "svx_oracle.c")


@pytest.fixture(scope="module")
def world():
    w = W.world()
    return w, H.load(K.GOLDEN), records.AlignmentFile(text=w.sam_text())


def test_golden_is_the_cases_of_this_tree(world):
    """the rows, candidates, options and expectations the golden was computed from are the ones tests/genotype_walk_cases.py builds today; the reference raised
    exactly where the cases say so and agreed with every author; the set stays inside the sizes the issue sets; the file holds data only and stays small"""
    w, g, _ = world
    assert g["rows_sha256"] == w.rows_sha256() and g["cases_sha256"] == w.cases_sha256() and g["n_rows"] == len(w.rows) and g["n_contigs"] == len(w.references)
    assert [c["id"] for c in g["cases"]] == [c.id for c in W.cases()] and len(W.cases()) == 104
    assert g["raises"] == W.EXPECTED_RAISES and sorted(g["raises"]) == sorted(c.id for c in W.refused())
    for c, gc in zip(W.cases(), g["cases"]):
        assert gc["expected"] == [W.expected_fields(e) for e in c.expected], c.id
        assert len(c.rows) <= 530 or c.family in ("walk", "eligible"), c.id              # a cap case stays at about 520 rows
    assert len(w.rows) < 60000 and len(w.references) > 100
    assert os.path.getsize(os.path.join(H.GOLDEN, K.GOLDEN)) < 100000


def test_every_comparison_has_a_case_on_each_side():
    """The coverage table: tests/genotype_walk_cases.py tags every case with the comparisons it sits below, on or above; every comparison of REQUIRED must have a
    case on each side listed there, so a later edit of the cases cannot silently lose one."""
    table = W.coverage(W.cases())
    assert sorted(table) == sorted(W.REQUIRED)
    for name, sides in W.REQUIRED.items():
        for side in sides:
            assert table[name].get(side), "no case %s %r" % (side, name)


def test_rows_index_is_the_alignment_index_of_the_file_and_the_file_has_the_shape_the_cases_need(world):
    """genotype_walk_cases.RowsIndex (what the mutants' child hands the oracle) = AlignmentIndex of the SAM text, column by column; contigs begin at the global
    records 2047, 2048, 2049, 4096 and 6145; a record without reference span has end == pos in the index and reference_end == pos + 1 on the record"""
    w, _, bam = world
    a, b = SVIM_genotyping.alignment_index(bam), W.RowsIndex(w)
    assert (a.n, a.n_contig, a.references, a.lengths, a.name_ids) == (b.n, b.n_contig, b.references, b.lengths, b.name_ids)
    for col in ("contig_first", "contig_len", "pos", "end", "flag", "mapq", "name_id"):
        x, y = getattr(a, col), getattr(b, col)
        assert x.dtype == y.dtype and (x == y).all(), col
    assert {2047, 2048, 2049, 4096, 6145} <= set(a.contig_first.tolist())
    nospan = [r for r in bam.fetch(until_eof=True) if r.cigarstring == "30S"]
    assert len(nospan) == 2 and all(r.reference_end == r.reference_start + 1 for r in nospan)
    assert int(((a.end == a.pos) & ((a.flag & 4) == 0)).sum()) == 2


@pytest.mark.parametrize("family", W.FAMILIES)
def test_oracle_object_route_against_the_reference(world, oracle, family):
    w, g, bam = world
    d = K.object_route_difference(w, g, bam, oracle, family=family)
    assert d is None, d


def test_table_route_over_the_oracle_join_against_the_reference(world, oracle):
    """class and score select, distinct member ids, the join, the call - stated in Python (genotype_cases.table_route_python) - on class-grouped tables of all
    candidates (one per set of options; tandem duplication and breakend rows ride along and stay untouched), on a table of DEL rows only and one of INS rows only"""
    w, g, bam = world
    index = SVIM_genotyping.alignment_index(bam)
    oracle.set_alignment_index(index)
    oracle._svx_index_id = id(index)

    def run(o, t, rid):
        return GC.table_route_python(t, rid, oracle, o)
    for kw in ({}, {"types_kept": ("DEL",)}, {"types_kept": ("INS",)}):
        d = K.table_route_difference(w, g, index.name_ids, run, **kw)
        assert d is None, d
    assert len(K.option_groups(w, g)) == 7


def test_refusals(world, oracle):
    """What the reference raises on (the golden records the exception type), and what this project answers instead.  A contig that the file does not have:
    ValueError there; here the candidate gets ref_reads 0 - a documented deviation.  minimum_depth <= 0 with no read on either side: the
    reference divides by zero; so does the object route, while the table route (genotype_calls, k_geno_call) gives the uncalled row of total 0."""
    w, g, bam = world
    a, b, c = W.refused()
    assert g["raises"][a.id] == "ValueError"
    assert K.object_route(w, a, bam, oracle) == [[1.0, "1/1", 0, 4]]
    for case in (b, c):
        assert g["raises"][case.id] == "ZeroDivisionError"
        with pytest.raises(ZeroDivisionError):
            K.object_route(w, case, bam, oracle)
        assert SVIM_genotyping.genotype_calls(0, 0, types.SimpleNamespace(**case.options)) == (0, ".")


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------------------
# Every entry: (what it changes, [(a piece of oracle/svx_oracle.c that occurs exactly once, its replacement)]).
_WINDOW = "const int64_t ws = start - 1000 > 0 ? start - 1000 : 0, we = end + 1000 < clen ? end + 1000 : clen;"
_CLAUSES = "support = ((double)rs < (double)end - minimum_overlap && re > end + 100) || (rs < start - 100 && (double)re > (double)start + minimum_overlap);"
_POINT = "support = rs < start - 100 && re > end + 100;"
_SKIP = "if ((ix->flag[i] & 0x4) || (ix->flag[i] & 0x100) || ix->mapq[i] < min_mapq) continue;"


def _in(line, old, new):
    assert line.count(old) == 1, (line, old)
    return [(line, line.replace(old, new))]


MUTANTS = [
    # the left edge of the fetch window (the right edge and the clamps: EQUIVALENT)
    ("1000 on the left edge, up", _in(_WINDOW, "start - 1000 > 0 ? start - 1000", "start - 1001 > 0 ? start - 1001")),
    ("1000 on the left edge, down", _in(_WINDOW, "start - 1000 > 0 ? start - 1000", "start - 999 > 0 ? start - 999")),
    # the four 100s, both ways
    ("end + 100, DEL / INV, up", _in(_CLAUSES, "re > end + 100", "re > end + 101")), ("end + 100, DEL / INV, down", _in(_CLAUSES, "re > end + 100", "re > end + 99")),
    ("start - 100, DEL / INV, up", _in(_CLAUSES, "rs < start - 100", "rs < start - 101")), ("start - 100, DEL / INV, down", _in(_CLAUSES, "rs < start - 100", "rs < start - 99")),
    ("start - 100, INS / DUP_INT, up", _in(_POINT, "start - 100", "start - 101")), ("start - 100, INS / DUP_INT, down", _in(_POINT, "start - 100", "start - 99")),
    ("end + 100, INS / DUP_INT, up", _in(_POINT, "end + 100", "end + 101")), ("end + 100, INS / DUP_INT, down", _in(_POINT, "end + 100", "end + 99")),
    # minimum_overlap
    ("2000, up", [("/ 2.0, 2000.0);", "/ 2.0, 2001.0);")]), ("2000, down", [("/ 2.0, 2000.0);", "/ 2.0, 1999.0);")]),
    ("/ 2.0 -> / 3.0", [("(double)(end - start) / 2.0", "(double)(end - start) / 3.0")]), ("/ 2.0 -> / 1.0", [("(double)(end - start) / 2.0", "(double)(end - start) / 1.0")]),
    ("minimum_overlap rounded up to an integer", [("(double)(end - start) / 2.0", "(double)((end - start + 1) / 2)")]),
    # the cap
    ("500, up", [("&& aln_no < 500; i++)", "&& aln_no < 501; i++)")]), ("500, down", [("&& aln_no < 500; i++)", "&& aln_no < 499; i++)")]),
    ("aln_no < 500 -> <=", [("&& aln_no < 500; i++)", "&& aln_no <= 500; i++)")]),
    # every < and > of the walk
    ("bam_endpos: re > rs -> >=", [("const int64_t endp = re > rs ? re : rs + 1;", "const int64_t endp = re >= rs ? re : rs + 1;")]),
    ("fetch: endp > ws -> >=", [("if (!(rs < we && endp > ws)) continue;", "if (!(rs < we && endp >= ws)) continue;")]),
    ("clause one: rs < -> <=", _in(_CLAUSES, "(double)rs < (double)end", "(double)rs <= (double)end")),
    ("clause one: re > -> >=", _in(_CLAUSES, "re > end + 100", "re >= end + 100")),
    ("clause two: rs < -> <=", _in(_CLAUSES, "rs < start - 100", "rs <= start - 100")),
    ("clause two: re > -> >=", _in(_CLAUSES, "(double)re > (double)start", "(double)re >= (double)start")),
    ("point: rs < -> <=", _in(_POINT, "rs < start", "rs <= start")), ("point: re > -> >=", _in(_POINT, "re > end", "re >= end")),
    ("|| -> && between the clauses", _in(_CLAUSES, "re > end + 100) || (rs", "re > end + 100) && (rs")),
    # eligibility
    ("unmapped mask 0x4 -> 0x8", _in(_SKIP, "& 0x4)", "& 0x8)")), ("unmapped mask 0x4 -> 0x10", _in(_SKIP, "& 0x4)", "& 0x10)")),
    ("unmapped mask 0x4 -> 0x400", _in(_SKIP, "& 0x4)", "& 0x400)")),
    ("secondary mask 0x100 -> 0x200", _in(_SKIP, "& 0x100)", "& 0x200)")), ("secondary mask 0x100 -> 0x800", _in(_SKIP, "& 0x100)", "& 0x800)")),
    ("mapq < -> <=", _in(_SKIP, "mapq[i] < min_mapq", "mapq[i] <= min_mapq")),
    ("the member test behind aln_no++", [("if (in_variant) continue;", ""), ("aln_no++;", "aln_no++; if (in_variant) continue;")]),
    ("aln_no++ behind the support test", [("aln_no++;", ""), ("if (!support) continue;", "if (!support) continue; aln_no++;")]),
    ("the seen test dropped", [("if (!seen) names[n_names++] = name;", "names[n_names++] = name;")]),
    ("endp -> re in the fetch test", [("if (!(rs < we && endp > ws)) continue;", "if (!(rs < we && re > ws)) continue;")]),
    ("the mode test", [("            if (mode == 0)\n                support = ((double)rs", "            if (mode != 0)\n                support = ((double)rs")]),
]
# No input that the reference accepts can tell these from the original: a record at or behind the right edge of the window sorts after every
# record that can support the reference allele (a supporter has reference_start < end), so it can neither be one nor take a place in front of one; every record
# of a contig starts inside the contig; every record has bam_endpos >= 1 > a negative window start.  They must SURVIVE; one that is detected means the argument is wrong.
EQUIVALENT = [
    ("1000 on the right edge", _in(_WINDOW, "end + 1000 < clen ? end + 1000", "end + 999 < clen ? end + 999")),
    ("the clamp to the contig length", _in(_WINDOW, "end + 1000 < clen ? end + 1000 : clen", "end + 1000")),
    ("the clamp at 0", _in(_WINDOW, "start - 1000 > 0 ? start - 1000 : 0", "start - 1000")),
]
# NOT in either list:
# * (end - start) / 2 as an integer division rounding DOWN: reference_start and reference_end are integers, and `rs < end - x.5` is `rs < end - x`, `re > start + x.5`
#   is `re > start + x`: the same answers (rounding UP is in the list);
# * `start - 1000 > 0` -> `>=`, `end + 1000 < clen` -> `<=`: both arms of the clamp are equal there; `rs < we` -> `<=`: the right edge, as above.


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


def test_no_mutant_of_the_walk_survives_the_golden_and_the_equivalent_ones_do(tmp_path):
    """Every entry of MUTANTS (38) and EQUIVALENT (3) names pieces of oracle/svx_oracle.c that occur exactly once and their replacements; the mutated source is
    compiled with the Makefile's flags at -O0 and loaded by a child process through SVX_ORACLE_LIB; the child (tests/genotype_child.py) holds the object route over
    that oracle to g_genotype_cases.json.gz.  A mutant must be reported different (exit status genotype_child.DIFFERENT, which nothing else ends a Python process
    with: a child that dies of an exception does not count as a detection); an equivalent change, and the unchanged source, must agree (exit status 0)."""
    with open(ORACLE_C) as fh:
        src = fh.read()
    jobs, seen = [(0, src, str(tmp_path))], set()
    table = MUTANTS + EQUIVALENT
    for k, (what, changes) in enumerate(table, 1):
        mutated = src
        for old, new in changes:
            assert src.count(old) == 1, "mutant %d (%s): %r occurs %d times" % (k, what, old, src.count(old))
            mutated = mutated.replace(old, new)
        assert mutated != src and mutated not in seen, "mutant %d (%s) changes nothing new" % (k, what)
        seen.add(mutated)
        jobs.append((k, mutated, str(tmp_path)))
    with ThreadPoolExecutor(max_workers=min(8, H.granted_cpus())) as pool:
        results = sorted(pool.map(run_one, jobs))
    assert results[0][1] == 0, "the unchanged oracle against the golden: %r" % (results[0],)
    survivors = ["%d: %s (exit %r) %s" % (k, table[k - 1][0], rc, out.strip()[-300:]) for k, rc, out in results[1:len(MUTANTS) + 1] if rc != K.DIFFERENT]
    assert not survivors, "%d of %d mutants not detected:\n%s" % (len(survivors), len(MUTANTS), "\n".join(survivors))
    detected = ["%d: %s (exit %r) %s" % (k, table[k - 1][0], rc, out.strip()[-300:]) for k, rc, out in results[len(MUTANTS) + 1:] if rc != 0]
    assert not detected, "changes held to be equivalent that the golden tells from the original:\n%s" % "\n".join(detected)
    assert len(MUTANTS) == 38 and len(EQUIVALENT) == 3
