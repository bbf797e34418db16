"""Routes of the BED / signature-VCF text to the device writer (svx_bed, csrc/bed.hip), as SVIM_COMBINE.vcf_body_device has them for variants.vcf.

`signature_text(product, clusters)` (cluster_sv_signatures' 6-tuple) and `candidate_text(candidates)` (write_candidates' 6-tuple) leave the text of one product
resident in the engine and return (engine, route), or None when the Python definition has to write this call:

  * "resident": the six lists are untouched views of the table the engine holds from its last cluster() / combine() and the signature table their members
    index is the one the engine collected: source 0, nothing is uploaded but names, no object is made;
  * "table": untouched views of one table that is no longer resident (its columns are uploaded as they are, still no object), or anything else - plain lists,
    lists somebody changed - whose objects fit the tables: one pass over the objects builds them, source 2;
  * None, too, when no engine is given, the lists are bound to none and this process has not opened one: nothing of the run lives on a device (clusters of
    the CPU oracle, hand-made objects in a process without a GPU), and the writers keep working there as they did before the device route existed.  A call
    that names an engine, or follows any device work, never takes this exit: a missing device is then an error, not a slower route;
  * None: something a table cannot say - a score or deviation that is not a float (`"{}".format(5)` is `5`, not `5.0`) or is NaN, a `signature` string other
    than cigar / suppl, a coordinate outside int32, an object without the attributes of its slot.
"""
import logging
import os

import numpy as np

from . import _abi, _lib, convert
from ._abi import SVX_BND, SVX_DEL, SVX_DUP_INT, SVX_DUP_TAN, SVX_INS, SVX_INV

_PIECE = 64 << 20
_CLUSTER_SLOT_TYPES = (SVX_DEL, SVX_INS, SVX_INV, SVX_DUP_TAN, SVX_DUP_INT, SVX_BND)      # cluster_sv_signatures' tuple order -> type codes
_CAND_SLOTS = (_abi.CAND_DUP_INT, _abi.CAND_INV, _abi.CAND_DUP_TAN, _abi.CAND_DEL, _abi.CAND_INS, _abi.CAND_BND)      # write_candidates' tuple order
_CAND_TYPE = {_abi.CAND_DEL: "DEL", _abi.CAND_INV: "INV", _abi.CAND_DUP_INT: "DUP_INT", _abi.CAND_DUP_TAN: "DUP_TAN", _abi.CAND_INS: "INS", _abi.CAND_BND: "BND"}


class _NoTable(Exception):
    """an object says something the tables cannot"""


def _float(x):
    if not isinstance(x, float) or x != x:
        raise _NoTable("not a float: %r" % (x,))
    return float(x)


def _dev(x):
    return float("nan") if x is None else _float(x)


def _name(x):
    if type(x) is not str or "\0" in x:
        raise _NoTable("not a name: %r" % (x,))
    return x


def _int(x):
    try:
        return convert._coord(x)
    except (TypeError, OverflowError):
        raise _NoTable("not an int32: %r" % (x,))


class _Members(object):
    """the member signatures of all rows, each object once, and the member list that indexes them"""

    def __init__(self):
        self.sigs, self.index, self.off, self.members = [], {}, [0], []

    def add(self, members):
        for m in members:
            k = self.index.get(id(m))
            if k is None:
                k = self.index[id(m)] = len(self.sigs)
                self.sigs.append(m)
            self.members.append(k)
        self.off.append(len(self.members))

    def table(self, contigs):
        for s in self.sigs:
            if s.signature not in _abi.SRC_NAMES or s.type not in _abi.TYPE_CODE or (s.type == "DUP_TAN" and type(s.copies) is not int):
                raise _NoTable("signature %r" % (s,))
            _name(s.read)
            for k in ("contig", "contig1", "contig2"):
                if hasattr(s, k):
                    _name(getattr(s, k))
        try:
            t, _, reads = convert.sigtable_from_objects(self.sigs, contigs=contigs, reads=convert.Interner())
        except (TypeError, OverflowError, KeyError, AttributeError) as e:
            raise _NoTable(str(e))
        return t, reads.names


def cluster_table_from_lists(lists6):
    """six sequences of SignatureCluster objects (cluster_sv_signatures' order) -> (ClusterTable, contig names, SigTable of the members, read names); None when
    an object's text is outside what the tables can say"""
    contigs, mem = convert.Interner(), _Members()
    by_type = dict(zip(_CLUSTER_SLOT_TYPES, lists6))
    rows = []
    try:
        for t in range(6):
            for c in by_type[t]:
                if c.type != _abi.TYPE_NAMES[t] or type(c.size) is not int:
                    raise _NoTable("cluster %r" % (c,))
                if t <= SVX_INV:
                    row = (contigs(_name(c.contig)), _int(c.start), _int(c.end), -1, 0, 0)
                else:
                    row = (contigs(_name(c.source_contig)), _int(c.source_start), _int(c.source_end), contigs(_name(c.dest_contig)), _int(c.dest_start), _int(c.dest_end))
                mem.add(c.members)
                rows.append((t,) + row + (0, _float(c.score), _dev(c.std_span), _dev(c.std_pos), _int(c.size)))
        sig, read_names = mem.table(contigs)
    except (_NoTable, AttributeError):
        return None
    ct = _abi.ClusterTable(len(rows), len(mem.members))
    if rows:
        cols = list(zip(*rows))
        for k, name in enumerate(("type", "contig", "start", "end", "contig2", "start2", "end2", "aux", "score", "std_span", "std_pos", "size")):
            getattr(ct, name)[:] = np.asarray(cols[k], dtype=_abi.CLU_DTYPES[name])
    ct.member_off[:] = np.asarray(mem.off, dtype=np.int64)
    ct.members[:len(mem.members)] = np.asarray(mem.members, dtype=np.int32)
    v = ct.view()
    for t in range(6):
        v.type_count[t] = len(by_type[t])
    ct.finish(v)
    return ct, contigs.names, sig, read_names


def candidate_table_from_lists(lists6):
    """six sequences of candidate objects (write_candidates' order) -> (CandidateTable, contig names, SigTable of the members, read names); None when an object's
    text is outside what the tables can say"""
    contigs, mem = convert.Interner(), _Members()
    by_cls = dict(zip(_CAND_SLOTS, lists6))
    rows = []
    try:
        for cls in range(6):
            for c in by_cls[cls]:
                if c.type != _CAND_TYPE[cls]:
                    raise _NoTable("candidate %r" % (c,))
                if cls == _abi.CAND_INS:
                    row = (-1, 0, 0, contigs(_name(c.dest_contig)), _int(c.dest_start), _int(c.dest_end), 0, 0, _dev(c.std_span), _dev(c.std_pos))
                elif cls == _abi.CAND_DUP_INT:
                    row = (contigs(_name(c.source_contig)), _int(c.source_start), _int(c.source_end), contigs(_name(c.dest_contig)), _int(c.dest_start), _int(c.dest_end),
                           1 if c.cutpaste else 0, 0, _dev(c.std_span), _dev(c.std_pos))
                elif cls == _abi.CAND_BND:
                    row = (contigs(_name(c.source_contig)), _int(c.source_start), _int(c.source_start), contigs(_name(c.dest_contig)), _int(c.dest_start),
                           _int(c.dest_start), 0, 0, _dev(c.std_pos1), _dev(c.std_pos2))
                else:
                    tan = cls == _abi.CAND_DUP_TAN
                    row = (contigs(_name(c.source_contig)), _int(c.source_start), _int(c.source_end), -1, 0, 0, 0, _int(c.copies) if tan else 0, _dev(c.std_span),
                           _dev(c.std_pos))
                mem.add(c.members)
                rows.append((cls,) + row + (_float(c.score),))
        sig, read_names = mem.table(contigs)
    except (_NoTable, AttributeError):
        return None
    t = _abi.CandidateTable(len(rows), len(mem.members))
    if rows:
        cols = list(zip(*rows))
        for k, name in enumerate(("cls", "contig", "start", "end", "contig2", "start2", "end2", "aux", "copies", "std_span", "std_pos", "score")):
            getattr(t, name)[:] = np.asarray(cols[k], dtype=_abi.CAND_DTYPES[name])
    t.member_off[:] = np.asarray(mem.off, dtype=np.int64)
    t.members[:len(mem.members)] = np.asarray(mem.members, dtype=np.int32)
    v = t.view()
    for cls in range(6):
        v.class_count[cls] = len(by_cls[cls])
    t.finish(v)
    return t, contigs.names, sig, read_names


def _engine_for(lists6, engine):
    """the engine a call without `engine=` runs on: the one the lists' signature table came from, else the one this process has open; None: there is none"""
    if engine is not None:
        return engine
    for x in lists6:
        o = getattr(getattr(x, "signatures", None), "origin", None)
        if o is not None:
            return o[0]
    if _lib._ENGINES:
        return _lib._ENGINES.get(int(os.environ.get("LOCAL_RANK", "0"))) or next(iter(_lib._ENGINES.values()))
    return None


def _collected_by(signatures, eng):
    """`signatures` is the table the engine collected last and still holds with every column"""
    from .lazy import SignatureList
    o = getattr(signatures, "origin", None)
    return isinstance(signatures, SignatureList) and o is not None and o[0] is eng and o[1] == eng.collect_generation


def _views(lists6, slots, bounds_of):
    """the six lists are untouched views of ONE table, each of the rows of its group, over a SignatureList -> that table, else None"""
    from .lazy import CandidateList, ClusterList, SignatureList
    first = lists6[0]
    if isinstance(first, ClusterList):
        table = first.ct
        if not all(isinstance(x, ClusterList) and x.untouched() and x.ct is table for x in lists6):
            return None
    elif isinstance(first, CandidateList):
        table = first.table
        if not all(isinstance(x, CandidateList) and x._objs is None and x.table is table for x in lists6):
            return None
    else:
        return None
    b = bounds_of(table)
    if not all((x.lo, x.hi) == (b[k], b[k + 1]) for x, k in zip(lists6, slots)) or not isinstance(first.signatures, SignatureList) or \
            not all(x.signatures is first.signatures and x.references is first.references for x in lists6):
        return None
    return table


def _cluster_bounds(ct):
    b = [0]
    for c in ct.type_count:
        b.append(b[-1] + int(c))
    return b


def signature_text(product, clusters, engine=None):
    """svx_bed product BED_SIGNATURE_BEDS or BED_SIGNATURE_VCF of the six cluster lists -> (engine, route) with the text resident in the engine; None: the
    Python definition writes this call"""
    from . import SVIM_COMBINE
    lists6 = tuple(clusters)
    if len(lists6) != 6:
        raise ValueError("the 6-tuple cluster_sv_signatures returns is expected")
    eng = _engine_for(lists6, engine)
    if eng is None:
        return None
    table = _views(lists6, _CLUSTER_SLOT_TYPES, _cluster_bounds)
    if table is not None:
        first = lists6[0]
        if SVIM_COMBINE._resident(lists6, eng) and _collected_by(first.signatures, eng):
            eng.bed(product, first.references, read_names=first.signatures.read_names)
            return eng, "resident"
        eng.bed(product, first.references, table=table, sigs=first.signatures.table, read_names=first.signatures.read_names)
        return eng, "table"
    built = cluster_table_from_lists(lists6)
    if built is None:
        return None
    ct, references, sig, read_names = built
    eng.bed(product, references, table=ct, sigs=sig, read_names=read_names)
    return eng, "table"


def candidate_text(candidates, engine=None):
    """svx_bed product BED_CANDIDATE_BEDS of the six candidate lists (write_candidates' order) -> (engine, route); None: the Python definition writes this call"""
    from . import SVIM_COMBINE
    lists6 = tuple(candidates)
    if len(lists6) != 6:
        raise ValueError("the 6-tuple of write_candidates is expected")
    eng = _engine_for(lists6, engine)
    if eng is None:
        return None
    table = _views(lists6, _CAND_SLOTS, lambda t: t.bounds())
    if table is not None:
        first = lists6[0]
        if SVIM_COMBINE._resident_candidates(lists6, eng) and _collected_by(first.signatures, eng):
            eng.bed(_abi.BED_CANDIDATE_BEDS, first.references, read_names=first.signatures.read_names)
            return eng, "resident"
        eng.bed(_abi.BED_CANDIDATE_BEDS, first.references, table=table, sigs=first.signatures.table, read_names=first.signatures.read_names)
        return eng, "table"
    built = candidate_table_from_lists(lists6)
    if built is None:
        return None
    t, references, sig, read_names = built
    eng.bed(_abi.BED_CANDIDATE_BEDS, references, table=t, sigs=sig, read_names=read_names)
    return eng, "table"


def file_texts(eng, piece=_PIECE):
    """the text of the engine's last bed() call, fetched in pieces -> list of bytes, one per file"""
    _, _, n_bytes = eng.bed_count()
    text = b"".join(eng.bed_fetch(at, min(piece, n_bytes - at)) for at in range(0, n_bytes, piece))
    off, _ = eng.bed_file_offsets()
    return [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def write_files(eng, directory, names, heads=None, piece=_PIECE, compress=False, index=None, index_format="tbi"):
    """the files of the engine's last bed() call into `directory` under `names` (heads: bytes written in front of each), fetched in pieces.
    compress: every name with .gz appended, the text compressed to BGZF on the device (svx_text_gz) and only the streams fetched; a head is compressed here.
    index (_abi.INDEX_BED / INDEX_VCF, with compress): name + ".gz.tbi" for every file whose lines tabix takes as they are (svx_text_index; nothing is
    re-sorted) -> the names of the files that got none (logged once each); [] without index.  index_format="csi": name + ".gz.csi" instead (svim_amd/csi.py),
    which no coordinate is too large for"""
    off, _ = eng.bed_file_offsets()
    if len(off) - 1 != len(names):
        raise ValueError("%d files in the text, %d names" % (len(off) - 1, len(names)))
    if index is not None and not compress:
        raise ValueError("write_files: an index needs compress=True")
    if compress:
        from . import harness
        eng.text_gz(_abi.TEXT_GZ_BED)
        goff, _, _ = eng.text_gz_tables()
        zheads = [harness.bgzf_blocks(h) for h in heads] if heads is not None else [b""] * len(names)
        for k, name in enumerate(names):
            with open(os.path.join(directory, name + ".gz"), "wb") as fh:
                fh.write(zheads[k])
                harness.write_text_gz(eng, fh, goff[k], goff[k + 1], piece)
        missing = []
        if index is not None:
            from .SVIM_COMBINE import _write_tbi
            eng.text_index(index, [len(h) for h in zheads], fmt=index_format)
            blobs, status = eng.text_index_fetch()
            for k, name in enumerate(names):
                if status[k] == 0:
                    _write_tbi(os.path.join(directory, name + ".gz." + index_format), blobs[k])
                else:
                    logging.warning("%s.gz gets no tabix index: %s" % (name, _abi.ERRORS.get(int(status[k]), int(status[k]))))
                    missing.append(name)
        return missing
    for k, name in enumerate(names):
        with open(os.path.join(directory, name), "wb") as fh:
            if heads is not None:
                fh.write(heads[k])
            for at in range(int(off[k]), int(off[k + 1]), piece):
                fh.write(eng.bed_fetch(at, min(piece, int(off[k + 1]) - at)))
    return []
