"""CLUSTER on the device (run on a real MI355X with `-m gpu`): k_part_flags, k_cluster (its three LDS capacity classes, the duplicate removal, the compaction, the
edit index of a surviving insertion pair, one lane per cluster), linkage_fcluster_lds and consolidate_one (csrc/cluster.hip) against what the REFERENCE returned
for the directed cases of tests/cluster_cases.py (tests/golden/g_cluster_cases.json.gz).  Per family ONE svx_cluster call on the family's table: the clusters
under the golden's comparison and identical to the oracle's tables up to 1e-12, the partitions the reference formed, and svx_pair_distances on the golden's pairs
with identical bit patterns.  The device-shape family again with the scheduling switches, which must not change the table.  tests/test_cluster_cases.py holds the
oracle to the same file on the CPU."""
import pytest

import cluster_cases as CC
import cluster_child as K
import helpers as H

pytestmark = pytest.mark.gpu

ENV = ("SVX_EDIT_NO_EARLY", "SVX_EDIT_NO_PREPACK")
NAMES = ["wide", "pmd0", "sample", "main", "cmd0", "int32", "shape"]
_CACHE = {}


def golden_family(name):
    if "golden" not in _CACHE:
        _CACHE["golden"] = H.load(K.GOLDEN)
        assert [f["name"] for f in _CACHE["golden"]["families"]] == NAMES
    return next(f for f in _CACHE["golden"]["families"] if f["name"] == name)


def oracle_table(oracle, fam):
    """the oracle's table of a family (computed once and left unchanged)"""
    key = "oracle " + fam["name"]
    if key not in _CACHE:
        tab, rank = K.setup(fam["signatures"])
        oracle.set_genome(*K.genome_arrays())
        _CACHE[key] = oracle.cluster(K.params_of(fam["options"]), rank, table=tab)
    return _CACHE[key]


def engine(monkeypatch, env):
    from svim_amd._lib import Engine
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Engine()
    e.set_genome(*K.genome_arrays())
    return e


@pytest.mark.parametrize("name", NAMES)
def test_cluster_cases_on_the_device(oracle, monkeypatch, name):
    from svim_amd import _abi
    fam = golden_family(name)
    tab, rank = K.setup(fam["signatures"])
    p = K.params_of(fam["options"])
    oc = oracle_table(oracle, fam)
    e = engine(monkeypatch, {})
    try:
        ct = e.cluster(p, rank, table=tab)
        parts = e.partitions()
        st = e.stats()
        dist = e.pair_distances(tab, K.pairs_of(fam), p)
    finally:
        e.close()
    d = K.clusters_difference(fam, ct)
    assert d is None, d
    d = ct.first_difference(oc, rtol=1e-12)
    assert d is None, "family %r against the oracle: %s" % (name, d)
    assert all(len({int(tab.type[i]) for i in q}) == 1 for q in parts) and sorted(i for q in parts for i in q) == list(range(tab.n))
    d = K.partitions_difference(fam, K.partition_lists_by_type(tab, parts))
    assert d is None, d
    d = K.pairs_difference(fam, [K.bits(x) for x in dist])
    assert d is None, d
    if name == "sample":
        assert st["n_large_partitions"] == 8
    if name in ("shape", "main", "sample"):
        assert ct.type_count[_abi.SVX_INS] > 0 and st["n_edit_pairs"] > 0


@pytest.mark.parametrize("switch", ENV)
def test_device_shape_family_with_the_scheduling_switches(oracle, monkeypatch, switch):
    """the partitions of 48, 49, 72, 73 and 100 members - one cluster, singletons, mixed sizes, brought down to 2 and to 1 by the duplicate removal - with the early
    full-matrix retries off and with the haplotype store packed from the pair list: the same table"""
    fam = golden_family("shape")
    tab, rank = K.setup(fam["signatures"])
    oc = oracle_table(oracle, fam)
    e = engine(monkeypatch, {switch: "1"})
    try:
        ct = e.cluster(K.params_of(fam["options"]), rank, table=tab)
        parts = e.partitions()
    finally:
        e.close()
    d = K.clusters_difference(fam, ct)
    assert d is None, "%s: %s" % (switch, d)
    d = ct.first_difference(oc, rtol=1e-12)
    assert d is None, "%s, against the oracle: %s" % (switch, d)
    d = K.partitions_difference(fam, K.partition_lists_by_type(tab, parts))
    assert d is None, "%s: %s" % (switch, d)
    assert sorted(CC.SHAPE_SIZES) == sorted({len(q) for q in parts} & set(CC.SHAPE_SIZES))
