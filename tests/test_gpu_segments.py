"""The split-read analysis on the device (k_segments, svim_amd/csrc/collect.hip) on the directed cases of tests/segment_cases.py: the tables of Engine.collect
against what the REFERENCE returned (tests/golden/g_segments_cases.json.gz) and against the oracle's, inserted bases included; the same reads at chosen lanes of
the kernel's 256-thread blocks under a permuted key order; reads whose per-read lists fill to their capacity; and one read whose rows outgrow the first sizing pass
of svx_collect_impl."""
import time

import pytest

import cigar_layouts as CL
import helpers as H
import segment_cases as SC
from svim_amd import _abi, _lib
from segment_checks import GOLDEN, many_rows_capacity_difference, placement_difference, placement_owners

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def against_oracle(eng, oracle, hb, p, what):
    sig, bnd = eng.collect(hb, p)
    osig, obnd = oracle.collect(hb, p)
    d = sig.first_difference(osig)
    assert d is None, "%s: main list against the oracle: %s" % (what, d)
    d = bnd.first_difference(obnd)
    assert d is None, "%s: side list against the oracle: %s" % (what, d)
    return sig, bnd


@pytest.mark.parametrize("idx", range(len(H.load(GOLDEN)["cases"])))
def test_device_against_the_reference_and_the_oracle(eng, oracle, idx):
    g = H.load(GOLDEN)
    case = g["cases"][idx]
    what = "%s / %s%s" % (case["name"], case["mode"], ", all_bnds" if case["options"]["all_bnds"] else "")
    bam, hb, o = H.sam_case_batch(case, g)
    sig, bnd = against_oracle(eng, oracle, hb, _abi.Params.from_options(o), what)
    got = H.table_rows(sig, hb.references, hb.read_names)
    assert got == case["signatures"], "%s: main list against the reference, first difference %r" % (what, next(((a, b) for a, b in zip(got, case["signatures"]) if a != b), None))
    assert H.table_rows(bnd, hb.references, hb.read_names) == case["bnds"], "%s: side list against the reference" % what


@pytest.mark.parametrize("n_rec,options", [(n, None) for n in SC.PLACEMENT_N_REC] + [(257, SC.INS_FROM_OPTIONS)])
def test_placement_in_the_block_and_permuted_keys(eng, oracle, n_rec, options):
    """one lane per primary in 256-thread blocks, workspace at ws + seg_off[r] + r: owners of rows at the first and last lane of a wave and of a block (read from
    the built batch), every other record without rows, the keys in another order than the records - per read the rows of the golden, and the oracle's tables.  One batch takes
    one set of options: the nine families with the common ones (205 reads), and the family "ins_from" in a batch of its own"""
    hb, opt, names, perm = SC.placement_batch(n_rec, options)
    assert hb.n_rec == n_rec
    assert {i for i in SC.PLACEMENT_OWNERS if i < n_rec} | {n_rec - 1} <= placement_owners(hb)
    for all_bnds in (False, True):
        sig, bnd = against_oracle(eng, oracle, hb, _abi.Params.from_options(H.options(dict(opt, all_bnds=all_bnds))), "n_rec %d" % n_rec)
        d = placement_difference(hb, names, perm, sig, bnd, all_bnds, opt)
        assert d is None, d


def test_many_rows_on_one_read(eng, oracle):
    """1, 2, 63, 64, 65 and 300 good rows on a read.  Read from seg_off of the built batch: where every row is good, the breakends of a "bnd" read (entries of
    its translocation list) and the copies of a "tan" read's DUP_TAN (entries of its tandem list) are the read's n_seg - the list fills its workspace; with a
    row below min_mapq they are n_seg - 1.  Counts in closed form, tables against the oracle"""
    case, n_main, n_side, layouts = SC.many_rows_case()
    hb = case.host_batch()
    for all_bnds in (False, True):
        sig, bnd = against_oracle(eng, oracle, hb, CL.params(40, all_bnds), case.name)
        assert (sig.n, bnd.n) == (n_main, n_side if all_bnds else 0)
        d = many_rows_capacity_difference(hb, sig, layouts)
        assert d is None, d


@pytest.mark.parametrize("all_bnds", (False, True))
def test_rows_beyond_the_first_sizing_pass(oracle, all_bnds):
    """one read whose insertions with detected origin alone are more than twice what the first pass of svx_collect_impl reserves (a fresh context: capacities
    persist in one): the second pass, sized from the first one's counters, must hold them all.  The time of the call is printed."""
    case, n_main, n_side, cap = SC.second_pass_case()
    assert n_main > 2 * cap and SC.first_pass_capacity(0, 0) == 16 * SC.RAW_SHARDS
    e = _lib.Engine(0)
    try:
        hb, p = case.host_batch(), CL.params(40, all_bnds)
        t0 = time.perf_counter()
        sig, bnd = e.collect(hb, p)
        dt = time.perf_counter() - t0
        print("%s: %d rows (first pass sized for %d) in %.3f s" % (case.name, sig.n, cap, dt))
        assert (sig.n, bnd.n) == (n_main, n_side if all_bnds else 0)
        osig, obnd = oracle.collect(hb, p)
        assert sig.first_difference(osig) is None and bnd.first_difference(obnd) is None
        sig2, _ = e.collect(hb, p)                                  # once more in the same context: the capacity is there from the start
        assert sig2.first_difference(osig) is None
    finally:
        e.close()
