"""The ordering sorts of CLUSTER (csrc/cluster.hip: k_make_key1 / k_make_keys and the key of the final cluster order in k_finalize; SVX_CLUSTER_ONE_SORT, SVX_CLUSTER_NARROW_KEY) on a real MI355X (`-m gpu`): the partitions and the cluster
table against the oracle, and against the two-sort path of rounds 1-6, for key widths from one contig (b = 1) to 16 384 contigs (b = 14, a 63-bit key) and
16 385 (the key does not fit: the two sorts stay).  Tables of more than 16 384 rows of all six types (the tiled sort runs), a rank array that is not the
identity, DUP_INT rows whose two contigs differ, rows with equal keys (ties keep their list order) and the coordinates 0 and 2^31 - 1 (DEL ends, BND
and INS starts; a DUP_INT destination as far right as its end still fits an int32)."""
import random

import numpy as np
import pytest

from svim_amd import _abi

pytestmark = pytest.mark.gpu

CONTIG_COUNTS = (1, 2, 3, 255, 256, 16384, 16385)
N_SITES = 5600                         # three or four rows each: more than 16 384 rows
I32_MAX = 2 ** 31 - 1
CODE = _abi.TYPE_CODE
_CASES = {}


def make_case(n_contig):
    """(SigTable, rank, genome offsets, genome codes): rows scattered over the contigs in no order"""
    rng = random.Random(1000 + n_contig)
    rank = list(range(n_contig))
    rng.shuffle(rank)                                       # not the identity (one contig: nothing to shuffle)
    if rank == sorted(rank):
        rank.reverse()
    top = rank.index(n_contig - 1)                          # the contig with the largest rank: the widest key
    rows = []                                               # (type, contig, start, end, contig2, pos2, aux, sequence)

    def site(k):
        c = top if k % 97 == 0 else rng.randrange(n_contig)
        base = 2000 + 3000 * rng.randrange(1, 600000)       # < 2^31; sites of one contig either far apart or (same draw) one partition
        t = ("DEL", "DEL", "DEL", "INV", "DUP_TAN", "BND", "DUP_INT", "INS", "DEL")[k % 9]
        for m in range(3 + (k % 5 == 0)):
            st = base + rng.randrange(0, 40)
            if m == 2:
                st = base                                   # ... and rows with the same key
            if t == "DEL":
                rows.append((CODE[t], c, st, base + 300, -1, 0, 0, ""))            # key: the end - equal for the rows of the site
            elif t == "INV":
                rows.append((CODE[t], c, st, base + 500, -1, 0, rng.randrange(5), ""))
            elif t == "DUP_TAN":
                rows.append((CODE[t], c, st, base + 400, -1, 2, m & 1, ""))
            elif t == "BND":
                c2 = rng.randrange(n_contig)
                rows.append((CODE[t], c, st, st + 1, c2, 70000 + rng.randrange(30), rng.randrange(4), ""))
            elif t == "DUP_INT":
                c2 = (c + 1 + rng.randrange(max(1, n_contig - 1))) % n_contig       # destination contig: another one wherever there is one (rank2 != 0 for most)
                rows.append((CODE[t], c, st, st + 250, c2 if m else top, 90000 + (0 if m == 2 else rng.randrange(30)), 0, ""))
            else:
                rows.append((CODE[t], c, st, st + 60, -1, 0, 0, "".join(rng.choice("ACGT") for _ in range(60))))

    for k in range(N_SITES):
        site(k)
    # the ends of the coordinate range, in every field a key is made of: BND and INS starts, DEL ends, DUP_INT destinations
    for c in {0, top}:
        rows.append((CODE["BND"], c, 0, 1, top, 5, 1, ""))
        rows.append((CODE["BND"], c, 0, 1, top, 5, 1, ""))
        rows.append((CODE["BND"], c, I32_MAX - 1, I32_MAX, 0, 9, 2, ""))
        rows.append((CODE["INS"], c, 0, 50, -1, 0, 0, "ACGTTGCA" * 6))
        rows.append((CODE["INS"], c, 0, 50, -1, 0, 0, "ACGTTGCA" * 6))
        rows.append((CODE["DEL"], c, I32_MAX - 400, I32_MAX, -1, 0, 0, ""))
        rows.append((CODE["DEL"], c, I32_MAX - 380, I32_MAX, -1, 0, 0, ""))
        rows.append((CODE["DEL"], c, 0, 300, -1, 0, 0, ""))
        rows.append((CODE["DUP_INT"], 0, 700, 900, c, I32_MAX - 200, 0, ""))      # (the destination's end, pos2 + span, is still an int32)
        rows.append((CODE["DUP_INT"], top, 720, 900, c, 0, 0, ""))
    rng.shuffle(rows)
    n = len(rows)
    assert n > 16384
    tab = _abi.SigTable(n, sum(len(r[7]) for r in rows))
    at = 0
    for i, (t, c, st, en, c2, p2, aux, seq) in enumerate(rows):
        tab.type[i], tab.contig[i], tab.start[i], tab.end[i], tab.contig2[i], tab.pos2[i], tab.aux[i] = t, c, st, en, c2, p2, aux
        tab.src[i], tab.read_id[i] = i & 1, i // 2                       # two rows per read: the same-read rule of the sampling has something to do
        tab.seq_off[i] = at
        if seq:
            tab.seq[at:at + len(seq)] = _abi.encode_bases(seq)
            at += len(seq)
    tab.seq_off[n] = at
    dup = (tab.type == CODE["DUP_INT"])
    assert set(int(x) for x in tab.type) == set(range(6))
    assert n_contig == 1 or (tab.contig[dup] != tab.contig2[dup]).any()
    off = np.arange(n_contig + 1, dtype=np.int64) * 4                    # tiny contigs: every insertion lies beyond its contig's end, the flanks are empty
    codes = np.tile(np.array([1, 2, 4, 8], dtype=np.uint8), n_contig)
    return tab, np.array(rank, dtype=np.int32), off, codes


def case(n_contig, oracle):
    """the case with the oracle's partitions and cluster table (computed once and left unchanged)"""
    if n_contig not in _CASES:
        tab, rank, off, codes = make_case(n_contig)
        p = params()
        oracle.set_genome(off, codes)
        sidx, pid = oracle.form_partitions(tab, rank, p.partition_max_distance)
        parts = [[] for _ in range(int(pid.max()) + 1)]
        for s, q in zip(sidx, pid):
            parts[int(q)].append(int(s))
        _CASES[n_contig] = (tab, rank, off, codes, parts, oracle.cluster(p, rank, table=tab))
    return _CASES[n_contig]


def params():
    import types
    return _abi.Params.from_options(types.SimpleNamespace(min_mapq=20, min_sv_size=40, max_sv_size=100000, segment_gap_tolerance=10, segment_overlap_tolerance=5,
                                                          partition_max_distance=1000, position_distance_normalizer=900, edit_distance_normalizer=1.0,
                                                          cluster_max_distance=0.5, all_bnds=False))


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n_contig", CONTIG_COUNTS)
def test_partitions_and_clusters_with_one_sort_and_with_two(eng, oracle, monkeypatch, n_contig):
    tab, rank, off, codes, parts, oct_ = case(n_contig, oracle)
    assert n_contig == 1 or list(rank) != sorted(rank)
    assert any(len(q) > 1 and len({(int(tab.type[i]), int(tab.contig[i]), int(tab.end[i])) for i in q}) == 1 for q in parts)       # equal keys in a partition
    eng.set_genome(off, codes)
    got = {}
    for one_sort, narrow_key in (("1", "1"), ("0", "0"), ("1", "0"), ("0", "1")):      # the two switches are independent: every combination
        monkeypatch.setenv("SVX_CLUSTER_ONE_SORT", one_sort)
        monkeypatch.setenv("SVX_CLUSTER_NARROW_KEY", narrow_key)
        what = "SVX_CLUSTER_ONE_SORT=%s SVX_CLUSTER_NARROW_KEY=%s" % (one_sort, narrow_key)
        ct = eng.cluster(params(), rank, table=tab)
        got[what] = ct
        assert eng.partitions() == parts, "partitions, " + what
        assert ct.first_difference(oct_, rtol=1e-12) is None, "clusters, " + what
    first = next(iter(got.values()))
    assert all(ct.first_difference(first) is None for ct in got.values())            # every path: the same bits
