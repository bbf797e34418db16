"""The CIGAR scan (k_scan_prepare, k_cigar_scan, k_shard_prefix, k_emit_indels, k_gather_seq; svim_amd/csrc/collect.hip) on the layouts of
tests/cigar_layouts.py: the signature tables of Engine.collect against the oracle's and against the plain expectation of the definition, inserted bases
included; the geometry table against both; a batch given as host arrays against the same batch given as device arrays inside poisoned surroundings.
Every family runs with the default grid and with SVX_SCAN_BLOCKS=1 (the fewest waves: several items per wave, the cross-item prefetch)."""
import pytest

import cigar_layouts as CL
from svim_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.fixture(params=["default_grid", "one_block_per_cu"])
def grid(request, monkeypatch):
    if request.param == "one_block_per_cu":
        monkeypatch.setenv("SVX_SCAN_BLOCKS", "1")
    else:
        monkeypatch.delenv("SVX_SCAN_BLOCKS", raising=False)
    return request.param


def check(eng, oracle, case, min_sv_size=None, all_bnds=False, on_device=False, expectation=True):
    m = case.min_sv_size if min_sv_size is None else min_sv_size
    what = "%s, min_sv_size %d%s" % (case.name, m, ", all_bnds" if all_bnds else "")
    p = CL.params(m, all_bnds)
    hb = case.host_batch()
    sig, bnd = eng.collect(hb, p)
    rec_geom, seg_geom = eng.collect_geometry()
    osig, obnd = oracle.collect(hb, p)
    d = sig.first_difference(osig)
    assert d is None, "%s: main list against the oracle: %s" % (what, d)
    d = bnd.first_difference(obnd)
    assert d is None, "%s: side list against the oracle: %s" % (what, d)
    if expectation:
        exp_main, exp_side = case.expect_rows(m, all_bnds)
        d = CL.first_row_difference(CL.table_rows(sig), exp_main)
        assert d is None, "%s: main list against the definition: %s" % (what, d)
        d = CL.first_row_difference(CL.table_rows(bnd), exp_side)
        assert d is None, "%s: side list against the definition: %s" % (what, d)
    assert rec_geom.shape == (hb.n_rec, 5) and seg_geom.shape == (hb.n_seg, 5)
    d = CL.geometry_difference(case, rec_geom, seg_geom)
    assert d is None, "%s: geometry against the definition: %s" % (what, d)
    og = oracle.collect_geometry(hb)
    defined = sorted(case.expect_geometry())
    for item in defined:
        got = rec_geom[item] if item < hb.n_rec else seg_geom[item - hb.n_rec]
        exp = og[0][item] if item < hb.n_rec else og[1][item - hb.n_rec]
        assert got.tolist() == exp.tolist(), "%s: geometry of item %d against the oracle" % (what, item)
    if on_device:
        db = CL.device_batch(hb)
        dsig, dbnd = eng.collect(db, p)
        d = dsig.first_difference(sig)
        assert d is None, "%s: device arrays against host arrays, main list: %s" % (what, d)
        d = dbnd.first_difference(bnd)
        assert d is None, "%s: device arrays against host arrays, side list: %s" % (what, d)
        d = CL.geometry_difference(case, *eng.collect_geometry())
        assert d is None, "%s: geometry from device arrays: %s" % (what, d)
    return sig, bnd


@pytest.mark.parametrize("lead", range(4))
def test_cigar_layout_g1_packed(eng, oracle, grid, lead):
    case, which = CL.g1_packed(lead)
    for m in (1, 30, 40, 41):
        sig, _ = check(eng, oracle, case, m, on_device=(m == 30))
        d = CL.golden_rows_difference(case, which, CL.table_rows(sig), m)
        assert d is None, "lead %d, min_sv_size %d: %s" % (lead, m, d)


def test_cigar_layout_g1_packed_repeated_with_every_third_record_filtered(eng, oracle, grid):
    case, which = CL.g1_packed(2, repeat=7, filter_every_third=True)
    sig, _ = check(eng, oracle, case, 30, all_bnds=True)
    assert CL.golden_rows_difference(case, which, CL.table_rows(sig), 30) is None


def test_cigar_layout_grid(eng, oracle):
    """(at most three items per batch: the grid is one block whatever SVX_SCAN_BLOCKS says)"""
    for case in CL.grid_cases():
        check(eng, oracle, case, on_device=True)


def test_cigar_layout_grid_as_one_batch(eng, oracle, grid):
    check(eng, oracle, CL.grid_batch(), on_device=True)


def test_cigar_layout_skips(eng, oracle, grid):
    for case in CL.skip_cases():
        check(eng, oracle, case, on_device=len(case.recs) < 100)


def test_cigar_layout_tiny_arrays(eng, oracle):
    for case in CL.tiny_cases():
        check(eng, oracle, case, on_device=True)
        check(eng, oracle, case, all_bnds=True)


def test_cigar_layout_operation_codes_and_lengths(eng, oracle, grid):
    for case, m in CL.opcode_cases(repeat=80):
        sig, _ = check(eng, oracle, case, m, all_bnds=True, on_device=(m == 40))
        assert (sig.n == 0) == (m >= 1 << 28)


def test_cigar_layout_inserted_bases(eng, oracle):
    case = CL.insertion_case()
    sig, _ = check(eng, oracle, case, on_device=True)
    assert sig.n > 300


def test_cigar_layout_segment_rows(eng, oracle, grid):
    if grid == "default_grid":
        for case in CL.segment_cases():
            check(eng, oracle, case, on_device=True)
            check(eng, oracle, case, all_bnds=True)
    check(eng, oracle, CL.segment_cases_combined(), all_bnds=True)


@pytest.mark.parametrize("k", CL.CAPACITY_K)
def test_cigar_layout_capacity(oracle, k):
    """one read with k reportable operations, each in a context of its own (capacities persist in a context); then once more in the same context"""
    case = CL.capacity_case(k)
    for all_bnds in (False, True):
        e = _lib.Engine(0)
        try:
            for _ in range(2):
                sig, bnd = check(e, oracle, case, all_bnds=all_bnds)
                assert sig.n == k and bnd.n == (k // 2 if all_bnds else 0)
        finally:
            e.close()


def test_cigar_layout_capacity_of_a_wave_with_several_dense_reads(oracle, grid):
    case = CL.capacity_pair_case()
    for all_bnds in (False, True):
        e = _lib.Engine(0)
        try:
            check(e, oracle, case, all_bnds=all_bnds)
        finally:
            e.close()


def test_cigar_layout_capacity_limit_is_a_clear_error(oracle):
    """regions for the fullest wave, times the waves of the grid, beyond the documented limit: SVX_E_CAPACITY that says so, and the context goes on working"""
    e = _lib.Engine(0)
    try:
        with pytest.raises(_lib.SvxError, match="SVX_E_CAPACITY.*53000 reportable"):
            e.collect(CL.capacity_limit_case(53000).host_batch(), CL.params())
        check(e, oracle, CL.capacity_case(300))
        check(e, oracle, CL.capacity_limit_case(5000))
    finally:
        e.close()
