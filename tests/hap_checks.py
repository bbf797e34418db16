"""What tests/test_hap_cases.py (oracle, CPU), its child process tests/hap_child.py and tests/test_gpu_hap_cases.py (device) share: the tables of tests/hap_cases.py
as SigTables, the genome arrays, and the comparison of pair distances with tests/golden/g_hap_cases.json.gz."""
import struct
import types

import helpers as H
import hap_cases as HC
from svim_amd import _abi, batch, convert

GOLDEN = "g_hap_cases.json.gz"


def bits(x):
    return struct.pack("<d", float(x)).hex()


def params_of(p):
    return _abi.Params.from_options(types.SimpleNamespace(position_distance_normalizer=p[0], edit_distance_normalizer=p[1], cluster_max_distance=p[2]))


def table_of(rows):
    """rows -> SigTable with the contig ids of HC.REFERENCES"""
    tab, contigs, reads = convert.sigtable_from_objects([H.row_sig(r) for r in rows], convert.Interner(HC.REFERENCES))
    assert contigs.names == HC.REFERENCES
    return tab


def genome_arrays(genome=None):
    return convert.genome_arrays({k: v.encode("ascii") for k, v in (genome or HC.GENOME).items()}, HC.REFERENCES)


def contig_rank():
    return batch.contig_ranks(HC.REFERENCES)


def describe(t, i, j, tag):
    ri, rj = t.rows[i], t.rows[j]
    return "%s / %s: starts %d (%s, %d inserted) and %d (%s, %d inserted), contig lengths %d and %d" % (
        t.name, tag, ri[2], ri[1], len(ri[6]), rj[2], rj[1], len(rj[6]), len(HC.GENOME.get(ri[1], "")), len(HC.GENOME.get(rj[1], "")))


def expected_pairs(g, t, edit_distance):
    """every pair of the family with the bit pattern it must have: the reference's where the golden has the pair, the definition's (haplotypes by slicing,
    edit_distance(a, b) of them, Python floats) for the definition-only pairs -> [(i, j, tag, params, hex, 'reference' | 'definition')]"""
    fam = next(f for f in g["families"] if f["name"] == t.name)
    ref = {(p[0], p[1], tuple(p[3])): p for p in fam["pairs"]}
    out = []
    for i, j, tag, params in t.pairs:
        p = ref.get((i, j, params))
        if p is not None:
            out.append((i, j, tag, params, p[4], "reference"))
        else:
            s1, s2 = HC.sig(t.rows[i]), HC.sig(t.rows[j])
            ed = edit_distance(*HC.haplotypes(HC.GENOME, s1, s2)) if HC.needs_edit(s1, s2, params) else None
            out.append((i, j, tag, params, bits(HC.distance(HC.GENOME, s1, s2, params, ed)), "definition"))
    return out


def pair_difference(t, expected, got_bits):
    """first pair whose distance does not have the expected bit pattern, described; None when all agree"""
    for (i, j, tag, params, want, src), got in zip(expected, got_bits):
        if got != want:
            return "%s, parameters %r: %s (%r) != the %s's %s (%r)" % (describe(t, i, j, tag), params, got, struct.unpack("<d", bytes.fromhex(got))[0], src, want,
                                                                       struct.unpack("<d", bytes.fromhex(want))[0])
    return None


def oracle_pair_difference(oracle, g, t):
    tab = table_of(t.rows)
    exp = expected_pairs(g, t, oracle.edit_distance)
    got = [bits(oracle.span_position_distance(tab, i, j, params_of(params))) for i, j, tag, params, _, _ in exp]
    return pair_difference(t, exp, got)


def oracle_cluster_difference(oracle, case, name, rows, opts):
    ct = oracle.cluster(_abi.Params.from_options(H.options(opts)), contig_rank(), table=table_of(rows))
    try:
        H.compare_cluster_rows(H.cluster_rows(ct, HC.REFERENCES), case["clusters"])
    except AssertionError as e:
        return "cluster case %r: %s" % (name, e)
    return None
