"""k_sample_sweep against k_sample_tables (SVX_SAMPLE_TABLES=walk) and the oracle (run with `-m gpu`): a signature table whose large partitions have the sizes at
which the bounds of random.sample change their bit length at or near the first draw (127, 128, 129), the smallest and the largest pool-method size (101, 1045)
and one in between; 65 large partitions of one type - one more than a chase run holds (CHASE_RUN, csrc/cluster.hip) - and 3 of another, small partitions in
between.  The clusters depend on every sample drawn, the samples on every table entry the chain passes through: equal cluster tables = equal chains.
tests/test_sample_sweep.py holds the table itself, entry for entry, to the walk and to CPython on the CPU."""
import random
import threading

import numpy as np
import pytest

import helpers as H
from svim_amd import _abi, batch, convert

pytestmark = pytest.mark.gpu

DEL_SIZES = [101, 127, 128, 129, 300, 1045, 1045] + [101, 127, 128, 129] * 13 + [300, 300, 127, 129, 1045, 128]       # 65
INV_SIZES = [129, 1045, 101]
OPTS = {"partition_max_distance": 1000, "cluster_max_distance": 0.5, "position_distance_normalizer": 900, "edit_distance_normalizer": 1.0}


def _rows(extra_del=()):
    """DEL partitions 1..40 on chr1, the others and the INV partitions on chr2 (string order chr1 < chr2: the same stream order on one rank and on two);
    behind every large partition a small one that draws nothing"""
    assert len(DEL_SIZES) == 65
    rng = random.Random(17)
    rows, rid = [], 0
    at = {"chr1": 10000, "chr2": 10000}
    plan = [("DEL", "chr1" if k < 40 else "chr2", n) for k, n in enumerate(list(DEL_SIZES) + list(extra_del))] + [("INV", "chr2", n) for n in INV_SIZES]
    for typ, contig, n in plan:
        for size, pos in ((n, at[contig]), (rng.randint(2, 40), at[contig] + 2500)):
            for _ in range(size):
                rid += 1
                st = pos + rng.randint(-100, 100)
                sp = 200 + rng.randint(-20, 20)
                rows.append(["DEL", contig, st, st + sp, "cigar", "r%d" % rid] if typ == "DEL" else
                            ["INV", contig, st, st + sp, "suppl", "r%d" % rid, rng.choice(("left_fwd", "right_rev"))])
        at[contig] += 5000
    rng.shuffle(rows)
    return rows


def _table(rows):
    tab, contigs, reads = convert.sigtable_from_objects([H.row_sig(r) for r in rows], convert.Interner(H.REFS))
    return tab, batch.contig_ranks(contigs.names)


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case(oracle):
    rows = _rows()
    tab, rank = _table(rows)
    p = _abi.Params.from_options(H.options(OPTS))
    return rows, tab, rank, p, oracle.cluster(p, rank, table=tab)


def test_sweep_walk_and_oracle_agree(eng, case, monkeypatch):
    rows, tab, rank, p, oc = case
    monkeypatch.delenv("SVX_SAMPLE_TABLES", raising=False)
    sweep = eng.cluster(p, rank, table=tab)
    pos_sweep = eng.stream_positions()
    assert eng.stats()["n_large_partitions"] == 68
    monkeypatch.setenv("SVX_SAMPLE_TABLES", "walk")
    walk = eng.cluster(p, rank, table=tab)
    assert eng.stream_positions() == pos_sweep and max(pos_sweep[1]) > 65 * 100
    assert sweep.first_difference(walk) is None
    assert sweep.n == oc.n and sweep.first_difference(oc, rtol=1e-12) is None
    assert walk.first_difference(oc, rtol=1e-12) is None


def test_a_set_method_partition_leaves_the_table_path(eng, oracle, case, monkeypatch):
    """one partition of 1046 members: random.sample's set method, whose consumption depends on the values drawn - no table is built, the serial scan samples"""
    tab, rank = _table(_rows(extra_del=(1046,)))
    p = case[3]
    oc = oracle.cluster(p, rank, table=tab)
    monkeypatch.delenv("SVX_SAMPLE_TABLES", raising=False)
    got = eng.cluster(p, rank, table=tab)
    assert eng.stats()["n_large_partitions"] == 69
    monkeypatch.setenv("SVX_SAMPLE_TABLES", "walk")
    walk = eng.cluster(p, rank, table=tab)
    assert got.first_difference(walk) is None
    assert got.n == oc.n and got.first_difference(oc, rtol=1e-12) is None


def test_two_ranks_build_their_tables_under_the_exchange(eng, case, monkeypatch):
    """build_tables under svx_sampling_exchange: two contexts on cuda:0, one thread each, own chr1 and chr2 (the transport is an in-process barrier, as in
    test_rank_exchange_three_contexts_on_one_gpu; the gloo transport itself is held by the existing two-rank tests, whose helpers start processes of their own).
    Rank 1's tables stand around the EXPECTED end of rank 0's chain, so its windows are wide.  Sweep and walk: the same clusters and stream positions on either
    rank; together the single rank's count, and rank 1 stops where the single rank stops."""
    from svim_amd import _lib
    rows, tab, rank, p, oc = case
    monkeypatch.delenv("SVX_SAMPLE_TABLES", raising=False)
    eng.cluster(p, rank, table=tab, fetch=False)
    single_end = eng.stream_positions()[1]
    locals_ = [_table([r for r in rows if r[1] == c])[0] for c in ("chr1", "chr2")]
    out = {}
    for how in ("sweep", "walk"):
        if how == "walk":
            monkeypatch.setenv("SVX_SAMPLE_TABLES", "walk")
        ag = H.ThreadAllGather(2)
        results, errors = [None, None], []

        def work(r):
            try:
                e = _lib.Engine(0)
                e.set_ranks(r, 2, ag.for_rank(r))
                ct = e.cluster(p, rank, table=locals_[r])
                results[r] = (ct, e.stream_positions())
                e.set_ranks(0, 1, None)
                e.close()
            except BaseException as ex:                                    # noqa: B902
                errors.append((r, ex))
                ag.abort()
        threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(300)
        assert not errors, errors
        out[how] = results
    for r in range(2):
        assert out["sweep"][r][0].first_difference(out["walk"][r][0]) is None, r
        assert out["sweep"][r][1] == out["walk"][r][1], r
    assert out["sweep"][0][0].n + out["sweep"][1][0].n == oc.n
    assert out["sweep"][1][1][0] == out["sweep"][0][1][1] and out["sweep"][1][1][1] == single_end
