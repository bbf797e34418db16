"""COMBINE on the device (svx_combine, svim_amd/csrc/combine.hip) against what the REFERENCE returned for the directed cases of tests/combine_threshold_cases.py
(tests/golden/g_combine_threshold_cases.json.gz; the Python replay is held to the same file by tests/test_combine_threshold_cases.py, which also shows that the
file notices every one-step change of the replay).

Per family: the case's six plain lists through svim_amd.combine_clusters (source 2: the cluster table handed in) - the candidate rows, the lists as the
reference leaves them -, the stage tables of that call ROW FOR ROW (the merged clusters, the flagged candidates, both removal lists), and the same table through
Engine.combine twice: equal candidate tables.

The resident route (source 0) takes the clusters a svx_cluster call left in the context; the library has no call that makes a cluster table resident from
rows (svx_combine's source 2 uploads into buffers of its own, and a svx_cluster call makes its clusters from signatures), so the shape families of stages 3 and
4 stay on the table route here.  Behind the upload both routes run the same combine_body on the same column pointers; the resident route is held by
tests/test_gpu_combine.py (test_golden_through_cluster_and_combine, test_resident_route_from_collect)."""
import types

import numpy as np
import pytest

import combine_cases as CC
import combine_threshold_cases as T
import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = "g_combine_threshold_cases.json.gz"


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


@pytest.fixture(scope="module")
def golden():
    return H.load(GOLDEN)


@pytest.mark.parametrize("family", T.FAMILIES)
def test_table_route_and_stage_tables_against_the_reference(eng, golden, family):
    import svim_amd
    from svim_amd import SVIM_COMBINE, _abi, batch
    ran = 0
    for case in golden["cases"]:
        if case["family"] != family:
            continue
        name, exp, o = case["name"], case["expected"], types.SimpleNamespace(**case["options"])
        lists6, idx = CC.case_objects(case)
        ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)       # the table combine_clusters makes of these lists, and the order of its signatures
        out = svim_amd.combine_clusters(lists6, o)
        got = [[CC.cand_row(c, idx) for c in lst] for lst in out]
        d = H.first_json_difference(got, exp["combine"])
        assert d is None, (name, d)
        assert [len(lists6[k]) for k in (1, 4, 5)] == [exp["n_ins_after"], exp["n_dup_int_after"], exp["n_bnd_after"]], name
        st = CC.check_stages(eng, exp, sigs, names, idx, what=name)
        assert np.allclose(st["merged"].score, [r[6] for r in exp["merged_insertion_from_clusters"]], rtol=1e-12, atol=0), name
        assert len(set(st["remove_1"].tolist()) | set(st["remove_2"].tolist())) == exp["n_ins_before"] - exp["n_ins_after"], name
        # the same table twice: equal candidate tables
        cp, rank = _abi.CombineParams.from_options(o), batch.contig_ranks(names)
        t1 = eng.combine(cp, rank, table=ct, sig_aux=aux)
        t2 = eng.combine(cp, rank, table=ct, sig_aux=aux)
        assert t1.first_difference(t2) is None and t1.n == sum(len(x) for x in exp["combine"]), name
        ran += 1
    assert ran


def test_refusals(eng, golden):
    """What the reference raises on (the golden records the exception type and the sizes it leaves its lists with), and what the device and the drop-in do.
    A tandem duplication cluster without source span: k_cmb_emit gives it copies = 0 and svx_combine returns; the reference divides by the span before it
    touches a list, and so does combine_clusters (SVIM_COMBINE._tandem_without_span), with the lists untouched.  A deletion cluster and an insertion-from cluster
    that both have no span: k_cutpaste_min's 0 / 0 is a NaN that no minimum takes, so the pair is left out and svx_combine returns; the reference divides by
    zero in flag_cutpaste_candidates, after the breakend and the insertion-from lists were extended, and so do combine_clusters and
    svim_amd.flag_cutpaste_candidates.  The kernels neither fault nor trap."""
    import svim_amd
    from svim_amd import SVIM_COMBINE, _abi, batch
    assert sorted(golden["refused"]) == sorted(T.EXPECTED_RAISES)
    for name, g in golden["refused"].items():
        o = types.SimpleNamespace(**g["options"])
        lists6, idx = CC.case_objects(g)
        ct, names, sigs, aux = SVIM_COMBINE.cluster_table_from_lists(lists6)
        if g["raises"] is None:
            # the reference returns a merged cluster that ends at 2 150 000 000; the table's int32 column wraps (k_merge_rows), so the drop-in refuses
            # with OverflowError before it edits a list
            with pytest.raises(OverflowError):
                svim_amd.combine_clusters(lists6, o)
            assert [len(lists6[k]) for k in (1, 4, 5)] == [1, 0, 2], name
            continue
        assert g["raises"] == "ZeroDivisionError"
        with pytest.raises(ZeroDivisionError):
            svim_amd.combine_clusters(lists6, o)
        assert [len(lists6[k]) for k in (1, 4, 5)] == g["state"], name
        # the device itself: the call returns a table
        t = eng.combine(_abi.CombineParams.from_options(o), batch.contig_ranks(names), table=ct, sig_aux=aux)
        assert t.n > 0, name
        if name.endswith("tandem_zero_span"):
            lo = int(t.bounds()[_abi.CAND_DUP_TAN])
            assert t.copies[lo] == 0
        else:
            st = eng.combine_stages()
            assert st["flagged"].n == 2 and [int(a) & 1 for a in st["flagged"].aux.tolist()] == [0, 0]      # (the span 0 / 0 pair is not a minimum)
            fresh, _ = CC.case_objects(g)
            with pytest.raises(ZeroDivisionError):
                svim_amd.flag_cutpaste_candidates(fresh[4], fresh[0], o)
