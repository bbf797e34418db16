"""k_gather_seq16 / k_gather_seq (csrc/collect.hip, SVX_GATHER_SEQ16) on a real MI355X (`-m gpu`): the inserted bases of hand-made records (tests/cigar_layouts.py)
against the oracle's and against the records' own bases - insertions of 1 .. 300 bases at even and odd read positions, ending on the last base of their record,
in the last record of the SEQ array, in records of odd length; the same through a sparse-SEQ batch (only the ranges of the reported insertions are there, the
last one ending with the array), and the error for an insertion whose bases are not in the batch."""
import numpy as np
import pytest

import cigar_layouts as CL
from cigar_layouts import I, M, S, rec, w
from svim_amd import _abi, _lib

pytestmark = pytest.mark.gpu

LENS = (1, 7, 8, 15, 16, 17, 127, 128, 129, 300)


def insertion_case():
    recs = []
    for lead in (0, 1, 2, 5):                                 # the first insertion at read position `lead`; matches of 1 and 2 bases behind the others: both parities
        ops = [w(S, lead)] if lead else []
        for j, l in enumerate(LENS):
            ops += [w(I, l), w(M, 1 + (j & 1))]
        for l in LENS:                                        # ... and one more that ends on the record's last base
            recs.append(rec(ops + [w(I, l)], pos=100 * lead + l))
    recs.append(rec([w(M, 3), w(I, 300)], pos=7))             # 303 bases: a record of odd length whose last byte is half used
    recs.append(rec([w(M, 4), w(I, 17)], pos=9))              # the last record of the SEQ array ends with its insertion (21 bases: the array's last byte too)
    return CL.Case("inserted bases, 16 per load", recs, min_sv_size=1, seed=37)


class SparseBatch(object):
    """the batch with only the SEQ ranges of its insertions of at least min_len bases (include/svx.h: seq_rng_*), as svx_bam_set_seq_filter leaves it;
    drop: the range of that insertion (counted over the batch) is left out"""

    def __init__(self, case, min_len, drop=None):
        self.hb = case.host_batch()
        dense, off = self.hb.arrays["seq"], case.seq_off
        rng_off, q0s, lens, byts, parts, at, k = [0], [], [], [], [], 0, 0
        for r, rc in enumerate(case.recs):
            for _, _, pq, l, is_del in CL.walk(rc["ops"], min_len):
                if is_del:
                    continue
                k += 1
                if drop is not None and k - 1 == drop:
                    continue
                q0 = pq & ~1                                  # ranges start on a byte
                n = pq + l - q0
                q0s.append(q0); lens.append(n); byts.append(at)
                parts.append(dense[off[r] + q0 // 2:off[r] + q0 // 2 + (n + 1) // 2])
                at += (n + 1) // 2
            rng_off.append(len(q0s))
        self.n_ins = k
        self.seq = np.ascontiguousarray(np.concatenate(parts))              # nothing behind the last range
        self.rng = (np.array(rng_off, dtype=np.uint32), np.array(q0s, dtype=np.int32), np.array(lens, dtype=np.int32), np.array(byts, dtype=np.uint64))
        self.read_names, self.references, self.n_rec, self.n_seg = self.hb.read_names, self.hb.references, self.hb.n_rec, self.hb.n_seg

    def struct(self):
        b = self.hb.struct()
        b.seq = _abi.ptr(self.seq)
        b.seq_rng_off, b.seq_rng_q0, b.seq_rng_len, b.seq_rng_byte = (_abi.ptr(a) for a in self.rng)
        b.n_seq_rng = len(self.rng[1])
        self._keep = b
        return b


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """(case, the oracle's main list on the dense batch) - computed once and left unchanged"""
    case = insertion_case()
    osig, _ = oracle.collect(case.host_batch(), CL.params(1))
    return case, osig


@pytest.mark.parametrize("form", ["1", "0"], ids=["16 bases per load", "8 bases per load"])
def test_inserted_bases_dense_and_sparse(eng, oracle, expected, monkeypatch, form):
    monkeypatch.setenv("SVX_GATHER_SEQ16", form)
    case, osig = expected
    p = CL.params(1)
    rows, _ = case.expect_rows(1)
    ins = [r for r in rows if r[1] == _abi.SVX_INS]
    assert {len(r[8]) for r in ins} == set(LENS) and len(ins) == osig.n
    sig, _ = eng.collect(case.host_batch(), p)
    assert sig.first_difference(osig) is None
    assert CL.first_row_difference(CL.table_rows(sig), rows) is None            # the records' own bases
    sparse = SparseBatch(case, 1)
    assert sparse.n_ins == len(ins) and sparse.seq.size < case.host_batch().arrays["seq"].size
    ssig, _ = eng.collect(sparse, p)
    assert ssig.first_difference(osig) is None
    assert ssig.first_difference(oracle.collect(sparse, p)[0]) is None
    # an insertion whose range the reader did not keep: a clear error, not bases from somewhere else
    with pytest.raises(Exception, match="sparse SEQ"):
        eng.collect(SparseBatch(case, 1, drop=sparse.n_ins // 2), p)
    sig2, _ = eng.collect(case.host_batch(), p)                                 # the context is usable afterwards
    assert sig2.first_difference(osig) is None
