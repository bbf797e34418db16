"""The insertion haplotypes on the device (run on a real MI355X with `-m gpu`): the signature branch of PairSource (csrc/edit.hip: record_hap, k_hap_pack,
PairSource::views, k_edit_prep at nibble offsets, the shifted bounds) and ins_needs_edit (csrc/cluster.hip) against what the REFERENCE returned for the directed
cases of tests/hap_cases.py (tests/golden/g_hap_cases.json.gz) - identical bit patterns - and, through CLUSTER, against the oracle's tables, with the haplotype
store packed ahead of the pair list (radius from the parameters) and packed from the pair list (exact radius).  tests/test_hap_cases.py holds the oracle and the
definition to the same file on the CPU."""
import pytest

import hap_cases as HC
import helpers as H
from hap_checks import GOLDEN, bits, contig_rank, expected_pairs, genome_arrays, pair_difference, params_of, table_of
from svim_amd import _abi

pytestmark = pytest.mark.gpu

ENV = ("SVX_EDIT_FEW_PAIRS", "SVX_EDIT_SHIFT_BOUNDS", "SVX_EDIT_NO_PREPACK")
_CACHE = {}


def families():
    if "families" not in _CACHE:
        _CACHE["families"] = HC.families()
    return _CACHE["families"]


def expected(oracle, t):
    """(computed once per family and left unchanged)"""
    if t.name not in _CACHE:
        _CACHE[t.name] = expected_pairs(H.load(GOLDEN), t, oracle.edit_distance)
    return _CACHE[t.name]


def engine(monkeypatch, env, genome=None):
    from svim_amd._lib import Engine
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Engine()
    e.set_genome(*genome_arrays(genome))
    return e


def by_params(exp):
    groups = {}
    for k, x in enumerate(exp):
        groups.setdefault(x[3], []).append(k)
    return groups


@pytest.mark.parametrize("route", ["few pairs", "large call", "padded beyond the pilot's limit"])
def test_hap_pair_distances_have_the_reference_bit_patterns(oracle, monkeypatch, route):
    """svx_pair_distances (the exact-radius rule: k_pair_span, then the store) on every family: the reference's bit pattern for every golden pair, the
    definition's for the pairs on the absent contig.  Routes: the low-latency forms of a call with few pairs (default), the classes of a large call
    (SVX_EDIT_FEW_PAIRS=0), and a call padded with the pairs of the `tiny` family to more than 4096 edit pairs (the per-call pilot runs).  Each with and without
    the shifted upper bounds (SVX_EDIT_SHIFT_BOUNDS=0), which must not change a bit."""
    tiny = next(t for t in families() if t.name == "tiny")
    results = []
    for shift_bounds in (None, "0"):
        env = {"SVX_EDIT_FEW_PAIRS": "0"} if route == "large call" else {}
        if shift_bounds is not None:
            env["SVX_EDIT_SHIFT_BOUNDS"] = shift_bounds
        e = engine(monkeypatch, env)
        got_all = []
        try:
            for t in families():
                exp = expected(oracle, t)
                rows, filler = t.rows, []
                if route.startswith("padded"):
                    rows = t.rows + tiny.rows
                    near = [(len(t.rows) + i, len(t.rows) + j) for i, j, _, _ in tiny.pairs]
                    filler = (near * (4500 // len(near) + 1))[:4500]
                tab = table_of(rows)
                got = [None] * len(exp)
                for params, ks in by_params(exp).items():
                    d = e.pair_distances(tab, [(exp[k][0], exp[k][1]) for k in ks] + filler, params_of(params))
                    for k, x in zip(ks, d):
                        got[k] = bits(x)
                diff = pair_difference(t, exp, got)
                assert diff is None, "%s, SVX_EDIT_SHIFT_BOUNDS %r: %s" % (route, shift_bounds, diff)
                got_all.append(got)
        finally:
            e.close()
        results.append(got_all)
    assert results[0] == results[1]


def _cluster_both(e, oracle, rows, opts):
    p = _abi.Params.from_options(H.options(opts))
    tab = table_of(rows)
    ct = e.cluster(p, contig_rank(), table=tab)
    st = e.stats()
    oc = oracle.cluster(p, contig_rank(), table=tab)
    return ct, oc, st


# 2 * cluster_max_distance * normalizer just below / just above 16000: the store's radius from the parameters (16101) / given up, from the pair list
NEAR_LIMIT = {"below the prepack limit": {"position_distance_normalizer": 15999.5, "partition_max_distance": 20000},
              "above the prepack limit": {"position_distance_normalizer": 16000.5, "partition_max_distance": 20000}}


@pytest.mark.parametrize("mode", ["prepack", "no prepack"] + list(NEAR_LIMIT))
def test_hap_cluster_cases_give_the_oracle_tables(oracle, monkeypatch, mode):
    """CLUSTER on the partitions that sit across a contig start or end, on the short contigs, beside the N run and on the absent contig: the oracle's tables
    (which tests/test_hap_cases.py holds to the reference's clusters), with the store packed ahead (default), from the pair list (SVX_EDIT_NO_PREPACK=1) and with
    parameters on either side of the prepack limit."""
    oracle.set_genome(*genome_arrays())
    oracle.set_threads(H.granted_cpus())
    e = engine(monkeypatch, {"SVX_EDIT_NO_PREPACK": "1"} if mode == "no prepack" else {})
    try:
        for name, rows, opts in HC.cluster_cases() + [HC.absent_cluster_case()]:
            ct, oc, st = _cluster_both(e, oracle, rows, dict(opts, **NEAR_LIMIT.get(mode, {})))
            assert ct.type_count[_abi.SVX_INS] > 0 and st["n_edit_pairs"] > 0, name
            d = ct.first_difference(oc, rtol=1e-12)
            assert d is None, "%s (%s): %s" % (name, mode, d)
    finally:
        e.close()
        oracle.set_threads(1)


@pytest.mark.parametrize("setting", ["defaults"] + list(NEAR_LIMIT))
def test_hap_cluster_every_insertion_in_one_table_with_both_radius_rules(oracle, monkeypatch, setting):
    """Every family's rows (the cluster cases' too) as ONE table through CLUSTER: the oracle's tables with the prepacked store and with the exact-radius store
    (SVX_EDIT_NO_PREPACK=1), at the defaults and on either side of the prepack limit (one partition per contig there: the sampled members are up to 16000 bases
    apart).  n_hap_bytes shows that both radius rules ran: the prepacked store (radius from the parameters: 1002, 16101) is larger than the exact-radius one of
    the same table; above the limit the switch changes nothing, the radius comes from the pair list either way."""
    oracle.set_genome(*genome_arrays())
    oracle.set_threads(H.granted_cpus())
    rows = HC.all_insertions_table()
    opts = dict(HC.OPTIONS, **NEAR_LIMIT.get(setting, {}))
    hap_bytes = {}
    try:
        p = _abi.Params.from_options(H.options(opts))
        oc = oracle.cluster(p, contig_rank(), table=table_of(rows))
    finally:
        oracle.set_threads(1)
    for mode, env in (("prepack", {}), ("no prepack", {"SVX_EDIT_NO_PREPACK": "1"})):
        e = engine(monkeypatch, env)
        try:
            ct = e.cluster(p, contig_rank(), table=table_of(rows))
            st = e.stats()
        finally:
            e.close()
        assert ct.type_count[_abi.SVX_INS] > 0 and st["n_edit_pairs"] > 0 and st["n_large_partitions"] > 0, mode
        d = ct.first_difference(oc, rtol=1e-12)
        assert d is None, "%s, %s: %s" % (setting, mode, d)
        hap_bytes[mode] = st["n_hap_bytes"]
    if setting == "above the prepack limit":
        assert hap_bytes["prepack"] == hap_bytes["no prepack"] > 0, hap_bytes
    else:
        assert hap_bytes["prepack"] > hap_bytes["no prepack"] > 0, hap_bytes


def test_hap_alphabet_routing_does_not_change_a_distance(oracle, monkeypatch):
    """The alphabet flags are taken over the whole record, flanks included: the same pair table on a genome whose N run lies just outside every record's radius
    (no record flagged: the A, C, G, T kernels), just inside the last record's radius but outside every window (flagged: the generic kernels on the same
    strings) and far away - identical distances, the definition's.  And the `alphabet` family itself with few pairs and as a large call: identical."""
    t, genomes = HC.alphabet_routing()
    tab = table_of(t.rows)
    want = []
    for i, j, tag, params in t.pairs:
        s1, s2 = HC.sig(t.rows[i]), HC.sig(t.rows[j])
        strings = {name: HC.haplotypes(g, s1, s2) for name, g in genomes.items()}
        assert strings["outside"] == strings["inside"] == strings["far"] and all(set(s) <= set("ACGT") for s in strings["far"])
        want.append(bits(HC.distance(genomes["far"], s1, s2, params, oracle.edit_distance(*strings["far"]))))
    for few_pairs in (None, "0"):
        for name, g in genomes.items():
            e = engine(monkeypatch, {} if few_pairs is None else {"SVX_EDIT_FEW_PAIRS": few_pairs}, genome=g)
            try:
                got = [bits(x) for x in e.pair_distances(tab, [(i, j) for i, j, _, _ in t.pairs], params_of(HC.DEFAULT))]
            finally:
                e.close()
            assert got == want, (name, few_pairs, got, want)
    fam = next(f for f in families() if f.name == "alphabet")
    exp = expected(oracle, fam)
    out = []
    for few_pairs in (None, "0"):
        e = engine(monkeypatch, {} if few_pairs is None else {"SVX_EDIT_FEW_PAIRS": few_pairs})
        try:
            out.append([bits(x) for x in e.pair_distances(table_of(fam.rows), [(x[0], x[1]) for x in exp], params_of(HC.DEFAULT))])
        finally:
            e.close()
    assert out[0] == out[1] == [x[4] for x in exp]
