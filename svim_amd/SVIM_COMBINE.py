"""GPU-backed counterpart of src/svim/SVIM_COMBINE.py: signature clusters -> SV candidates on the device (svx_combine, csrc/combine.hip).

`combine_clusters(signature_clusters, options)` has the reference's signature and return order (deletion, inversion, interspersed duplication, tandem
duplication, novel insertion, breakend candidates) and leaves its six input lists as the reference leaves them: insertion clusters that were merged or
coincide with a duplication deleted, the breakend list extended by the mirrored clusters, the insertion-from list extended by the merged ones.

  * lazy ClusterLists that are still untouched views of the cluster table the engine holds go the resident route (source 0): nothing is uploaded and no
    Python object is made - neither for the clusters nor for the candidates (CandidateList) nor for the edits of the input lists (ClusterList.defer);
  * anything else (plain lists, lists somebody changed, clusters of another call) is turned into a cluster table and goes source 2.

The insertion consensus (spoa) is not part of the device path: it implements the reference's skip_consensus branch; with options.skip_consensus false
this is logged once and the same candidates are returned ("COMBINE on the device").
"""
import logging

import numpy as np

from . import _abi, _lib, batch, convert
from ._abi import SVX_BND, SVX_DEL, SVX_DUP_INT, SVX_DUP_TAN, SVX_INS, SVX_INV, ClusterTable
from .lazy import ClusterList
from .signatures import SignatureClusterBiLocal

# cluster_sv_signatures' tuple order -> type codes of the cluster table
_SLOT_TYPES = (SVX_DEL, SVX_INS, SVX_INV, SVX_DUP_TAN, SVX_DUP_INT, SVX_BND)
_CONSENSUS_NOTE = [False]


def _nan(x):
    return float("nan") if x is None else float(x)


def cluster_table_from_lists(lists6):
    """six sequences of SignatureCluster objects (cluster_sv_signatures' order) -> (ClusterTable, contig names, signature objects, their aux column)"""
    contigs = convert.Interner()
    sigs, sig_index = [], {}
    by_type = {t: list(lst) for t, lst in zip(_SLOT_TYPES, lists6)}
    n = sum(len(v) for v in by_type.values())
    moff, members = [0], []
    rows = []
    for t in range(6):
        for c in by_type[t]:
            if t <= SVX_INV:
                row = (contigs(c.contig), c.start, c.end, -1, 0, 0, 0)
            else:
                aux = 0
                if t == SVX_BND:
                    aux = (1 if c.direction1 == "rev" else 0) | (2 if c.direction2 == "rev" else 0)
                row = (contigs(c.source_contig), c.source_start, c.source_end, contigs(c.dest_contig), c.dest_start, c.dest_end, aux)
            for m in c.members:
                k = sig_index.get(id(m))
                if k is None:
                    k = sig_index[id(m)] = len(sigs)
                    sigs.append(m)
                members.append(k)
            moff.append(len(members))
            rows.append((t,) + row + (float(c.score), _nan(c.std_span), _nan(c.std_pos), moff[-1] - moff[-2]))
    ct = ClusterTable(n, len(members))
    if n:
        cols = list(zip(*rows))
        for k, name in enumerate(("type", "contig", "start", "end", "contig2", "start2", "end2", "aux", "score", "std_span", "std_pos", "size")):
            getattr(ct, name)[:n] = np.asarray(cols[k], dtype=_abi.CLU_DTYPES[name])
    ct.member_off[:] = np.asarray(moff, dtype=np.int64)
    ct.members[:len(members)] = np.asarray(members, dtype=np.int32)
    v = ct.view()
    for t in range(6):
        v.type_count[t] = len(by_type[t])
    ct.finish(v)
    aux = np.fromiter((1 if getattr(s, "fully_covered", False) else 0 for s in sigs), dtype=np.uint8, count=len(sigs))
    return ct, contigs.names, sigs, aux


def _signature_aux(signatures):
    """aux column (bit 0 = fully_covered of tandem duplications) of the sequence cluster members index into"""
    table = getattr(signatures, "table", None)
    if table is not None:
        return table.aux[:table.n]
    return np.fromiter((1 if getattr(s, "fully_covered", False) else 0 for s in signatures), dtype=np.uint8, count=len(signatures))


def mirrored_clusters(bnd_objects):
    """the mirror image of every breakend cluster as src/svim/SVIM_merging.py:97-105 builds it (same members; that constructor call hands std_pos over
    where std_span goes and the other way round)"""
    out = []
    for c in bnd_objects:
        m = SignatureClusterBiLocal(c.dest_contig, c.dest_start, c.dest_end, c.source_contig, c.source_start, c.source_end, c.score, c.size, c.members,
                                    c.type, c.std_pos, c.std_span)
        m.direction1 = "fwd" if c.direction2 == "rev" else "rev"
        m.direction2 = "fwd" if c.direction1 == "rev" else "rev"
        out.append(m)
    return out


def merged_cluster_objects(merged, signatures, references):
    """stage 2's rows (Engine.combine_stages()["merged"]) -> SignatureClusterBiLocal objects of type DUP_INT"""
    out = []
    moff = merged.member_off.tolist()
    for k in range(merged.n):
        out.append(SignatureClusterBiLocal(references[int(merged.contig[k])], int(merged.start[k]), int(merged.end[k]), references[int(merged.contig2[k])],
                                           int(merged.start2[k]), int(merged.end2[k]), float(merged.score[k]), moff[k + 1] - moff[k],
                                           (signatures, merged.members[moff[k]:moff[k + 1]]), "DUP_INT", convert._none_if_nan(float(merged.std_span[k])),
                                           convert._none_if_nan(float(merged.std_pos[k]))))
    return out


def _resident(lists6, eng):
    """the six lists are the untouched views of the cluster table `eng` fetched from its last cluster() call"""
    ct = getattr(eng, "_resident_ct", None)
    if ct is None or not all(isinstance(x, ClusterList) and x.untouched() and x.ct is ct for x in lists6):
        return False
    bounds = [0]
    for c in ct.type_count:
        bounds.append(bounds[-1] + int(c))
    return all((x.lo, x.hi) == (bounds[t], bounds[t + 1]) for x, t in zip(lists6, _SLOT_TYPES)) and \
        all(x.signatures is lists6[0].signatures and x.references is lists6[0].references for x in lists6)


def _apply_edits(lists6, n_ins, stages, signatures, references, with_deletions=True):
    dele, insr, inv, tan, dint, bnd = lists6
    merged = stages["merged"]
    n_bnd = len(bnd)
    removed = sorted(set(stages["remove_1"].tolist()) | set(stages["remove_2"].tolist())) if with_deletions else []
    make_merged = lambda objs=None: merged_cluster_objects(merged, signatures, references)      # noqa: E731
    if n_ins > 0:
        if isinstance(bnd, ClusterList):
            bnd.defer(n_appended=n_bnd, appended=mirrored_clusters)
        else:
            bnd.extend(mirrored_clusters(list(bnd)))
    if isinstance(dint, ClusterList):
        dint.defer(n_appended=merged.n, appended=make_merged)
    else:
        dint.extend(make_merged())
    if isinstance(insr, ClusterList):
        insr.defer(deleted=removed)
    else:
        for k in reversed(removed):
            del insr[k]


def combine_clusters(signature_clusters, options, engine=None):
    """src/svim/SVIM_COMBINE.py:332-478 on the device -> (deletion, inversion, interspersed duplication, tandem duplication, novel insertion, breakend
    candidates) as lazy CandidateLists.  IndexError when there are insertion-from clusters but no deletion cluster, as in the reference."""
    lists6 = tuple(signature_clusters)
    if len(lists6) != 6:
        raise ValueError("combine_clusters expects the 6-tuple cluster_sv_signatures returns")
    if not getattr(options, "skip_consensus", True) and not _CONSENSUS_NOTE[0]:
        _CONSENSUS_NOTE[0] = True
        logging.warning("svim_amd: insertion consensus sequences are not computed on the device path; continuing as with --skip_consensus")
    eng = engine if engine is not None else _lib.engine()
    cp = _abi.CombineParams.from_options(options)
    n_ins = len(lists6[1])
    if _resident(lists6, eng):
        signatures, references = lists6[0].signatures, lists6[0].references
        run = lambda: eng.combine(cp, batch.contig_ranks(references))                              # noqa: E731
    else:
        ct, references, signatures, aux = cluster_table_from_lists(lists6) if not _same_table(lists6) else _table_of(lists6)
        run = lambda: eng.combine(cp, batch.contig_ranks(references), table=ct, sig_aux=aux)       # noqa: E731
    logging.info("Combine inserted regions with translocation breakpoints..")
    try:
        table = run()
    except _lib.NoDeletionClusters:
        _apply_edits(lists6, n_ins, eng.combine_stages(), signatures, references, with_deletions=False)
        raise IndexError("list index out of range")
    _apply_edits(lists6, n_ins, eng.combine_stages(), signatures, references)
    logging.info("Cluster interspersed duplication candidates one more time..")
    return convert.candidate_lists(table, signatures, references)


def _same_table(lists6):
    """untouched views of ONE cluster table that is no longer the engine's resident one: its columns are uploaded as they are (still no objects)"""
    first = lists6[0]
    if not all(isinstance(x, ClusterList) and x.untouched() and x.ct is getattr(first, "ct", None) for x in lists6):
        return False
    bounds = [0]
    for c in first.ct.type_count:
        bounds.append(bounds[-1] + int(c))
    return all((x.lo, x.hi) == (bounds[t], bounds[t + 1]) for x, t in zip(lists6, _SLOT_TYPES)) and \
        all(x.signatures is first.signatures and x.references is first.references for x in lists6)


def _table_of(lists6):
    first = lists6[0]
    return first.ct, first.references, first.signatures, _signature_aux(first.signatures)


def combine_tables(engine, options, references=None, contig_rank=None):
    """COMBINE of the clusters resident in `engine` (its last cluster() call) -> CandidateTable; no Python object is made.  The contig order comes from
    `references` (names), `contig_rank`, or - neither given - the ranks the cluster() call was given."""
    if contig_rank is None:
        contig_rank = batch.contig_ranks(references) if references is not None else getattr(engine, "_last_contig_rank", None)
    if contig_rank is None:
        raise ValueError("combine_tables: no contig ranks (pass references or contig_rank)")
    return engine.combine(_abi.CombineParams.from_options(options), contig_rank)
