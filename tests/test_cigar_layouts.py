"""The layouts of tests/cigar_layouts.py on the CPU: the oracle's multi-record walk against the plain expectation of the definition and, on the packed golden,
against the reference's own tuples - generator, expectation and oracle are pinned to each other before any of them judges the GPU."""
import numpy as np
import pytest

import cigar_layouts as CL


def check(oracle, case, min_sv_size=None, all_bnds=False):
    m = case.min_sv_size if min_sv_size is None else min_sv_size
    hb = case.host_batch()
    sig, bnd = oracle.collect(hb, CL.params(m, all_bnds))
    exp_main, exp_side = case.expect_rows(m, all_bnds)
    d = CL.first_row_difference(CL.table_rows(sig), exp_main)
    assert d is None, "%s, min_sv_size %d, main list: %s" % (case.name, m, d)
    d = CL.first_row_difference(CL.table_rows(bnd), exp_side)
    assert d is None, "%s, min_sv_size %d, side list: %s" % (case.name, m, d)
    d = CL.geometry_difference(case, *oracle.collect_geometry(hb))
    assert d is None, "%s: %s" % (case.name, d)
    return sig, bnd


def test_walk_is_the_golden_walk():
    for c in CL.g1_cases():
        ops = [CL.w(op, l) for op, l in c["tuples"]]
        assert [(pr, pq, l, "DEL" if d else "INS") for _, pr, pq, l, d in CL.walk(ops, c["min_length"])] == [tuple(x) for x in c["expect"]]


def test_geometry_examples():
    w, g = CL.w, CL.geometry
    assert g([], 0) == (1, 0, 0, 0, 0) and g([], 9) == (1, 0, 9, 0, 0)
    assert g([w(CL.H, 5), w(CL.S, 3), w(CL.M, 10), w(CL.N, 7), w(CL.D, 2), w(CL.I, 4), w(CL.S, 6), w(CL.H, 1)], 23) == (19, 3, 17, 29, 6)
    assert g([w(CL.S, 3), w(CL.M, 10), w(CL.S, 6)], 0) == (10, 3, 13, 19, 0)
    assert g([w(CL.S, 4)], 4) == (1, 4, 4, 4, 0)                       # element 0 is never taken off the end
    assert g([w(CL.S, 0), w(CL.S, 4), w(CL.S, 2), w(CL.M, 1)], 0) == (1, 6, 5, 7, 0)


@pytest.mark.parametrize("lead", range(4))
def test_g1_packed(oracle, lead):
    case, which = CL.g1_packed(lead)
    assert len(case.recs) == 1205 and 1 <= len(case.recs[-1]["ops"]) <= 7
    for m in (1, 30, 40, 41):
        sig, _ = check(oracle, case, m)
        d = CL.golden_rows_difference(case, which, CL.table_rows(sig), m)
        assert d is None, "lead %d, min_sv_size %d: %s" % (lead, m, d)


def test_g1_packed_repeated_with_every_third_record_filtered(oracle):
    case, which = CL.g1_packed(2, repeat=7, filter_every_third=True)
    assert len(case.recs) > CL.WAVE_STRIDE_DEFAULT
    sig, _ = check(oracle, case, 30)
    assert CL.golden_rows_difference(case, which, CL.table_rows(sig), 30) is None


def test_every_case_of_the_golden_meets_every_lead():
    seen = {}
    for lead in range(4):
        case, which = CL.g1_packed(lead)
        off = 0
        for r, i in zip(case.recs, which):
            if i is not None:
                seen.setdefault(i, set()).add(off & 3)
            off += len(r["ops"])
    assert len(seen) == 1204 and all(v == {0, 1, 2, 3} for v in seen.values())


def test_grid(oracle):
    cases = CL.grid_cases()
    assert len(cases) == 54 * 9
    for case in cases:
        check(oracle, case)
    check(oracle, CL.grid_batch())


def test_grid_items_lie_where_their_names_say():
    for case in CL.grid_cases([5, 256]):
        lead = int(case.name.split("lead=")[1].split()[0])
        off = np.cumsum([0] + [len(r["ops"]) for r in case.recs])
        k = 0 if "first" in case.name else 1
        assert off[k] & 3 == lead and len(case.recs[k]["ops"]) == int(case.name.split("n=")[1].split()[0])
        assert ("last" in case.name) == (k == len(case.recs) - 1)


@pytest.mark.parametrize("family", ["skips", "tiny", "inserted_bases", "segment_rows"])
def test_family(oracle, family):
    cases = {"skips": CL.skip_cases, "tiny": CL.tiny_cases, "inserted_bases": lambda: [CL.insertion_case()], "segment_rows": CL.segment_cases}[family]()
    for case in cases:
        check(oracle, case)
        check(oracle, case, all_bnds=True)


def test_operation_codes_and_lengths(oracle):
    for case, m in CL.opcode_cases():
        sig, _ = check(oracle, case, m, all_bnds=True)
        assert (sig.n == 0) == (m >= 1 << 28)


def test_segment_rows_cover_both_geometry_paths_and_every_residue():
    for case in CL.segment_cases():
        rows = [s for r in case.recs for s in r["rows"]]
        n = [len(s["ops"]) for s in rows]
        assert {1, 2, 31, 32, 33, 34, 255, 256, 257, 258, 511, 512, 513, 514} <= set(n)
        assert any(s["lseq"] == 0 for s in rows) and any(s["lseq"] > 0 for s in rows)
    starts = set()
    for case in CL.segment_cases():
        off = np.cumsum([0] + [len(s["ops"]) for r in case.recs for s in r["rows"]])
        starts |= {(int(a) & 3, int(b - a) > 32) for a, b in zip(off[:-1], off[1:])}
    assert starts == {(r, big) for r in range(4) for big in (False, True)}


@pytest.mark.parametrize("k", CL.CAPACITY_K)
def test_capacity(oracle, k):
    case = CL.capacity_case(k)
    sig, bnd = check(oracle, case, all_bnds=True)
    assert sig.n == k and bnd.n == k // 2


def test_capacity_pair(oracle):
    case = CL.capacity_pair_case()
    sig, _ = check(oracle, case)
    assert sig.n == 300 + 307 + (len(case.recs) - 2)
