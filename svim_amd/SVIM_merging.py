"""GPU-backed counterparts of src/svim/SVIM_merging.py: the two functions COMBINE calls, served from the stages of svx_combine (csrc/combine.hip)."""
import numpy as np   # noqa: F401

from . import _abi, _lib, batch, convert
from .SVIM_COMBINE import cluster_table_from_lists, merged_cluster_objects, mirrored_clusters


def merge_translocations_at_insertions(translocation_signature_clusters, insertion_signature_clusters, options, engine=None):
    """src/svim/SVIM_merging.py:93-159 -> (new insertion-from clusters, indices of the insertion clusters they replace); EXTENDS the breakend list by
    the mirrored clusters, as the reference does."""
    if len(insertion_signature_clusters) == 0:
        return [], []
    eng = engine if engine is not None else _lib.engine()
    ct, names, sigs, aux = cluster_table_from_lists(([], insertion_signature_clusters, [], [], [], translocation_signature_clusters))
    try:
        eng.combine(_abi.CombineParams.from_options(options), batch.contig_ranks(names), table=ct, sig_aux=aux, fetch=False)
    except _lib.NoDeletionClusters:
        pass                                    # stage 2 is complete: only the flagging needs deletion clusters
    st = eng.combine_stages()
    translocation_signature_clusters.extend(mirrored_clusters(list(translocation_signature_clusters)))
    return merged_cluster_objects(st["merged"], sigs, names), [int(k) for k in st["remove_1"]]


def flag_cutpaste_candidates(insertion_from_signature_clusters, deletion_signature_clusters, options, engine=None):
    """src/svim/SVIM_merging.py:12-29 -> CandidateDuplicationInterspersed objects, cutpaste set where a deletion cluster is close.  IndexError without a
    deletion cluster and ZeroDivisionError where a deletion cluster and an insertion-from cluster both have no span, as in the reference."""
    if len(insertion_from_signature_clusters) == 0:
        return []
    if len(deletion_signature_clusters) == 0:
        raise IndexError("list index out of range")
    if any(d.end == d.start for d in deletion_signature_clusters) and any(c.source_end == c.source_start for c in insertion_from_signature_clusters):
        raise ZeroDivisionError("division by zero")
    eng = engine if engine is not None else _lib.engine()
    ct, names, sigs, aux = cluster_table_from_lists((deletion_signature_clusters, [], [], [], insertion_from_signature_clusters, []))
    eng.combine(_abi.CombineParams.from_options(options), batch.contig_ranks(names), table=ct, sig_aux=aux, fetch=False)
    flagged = eng.combine_stages()["flagged"]
    return convert.candidate_objects_range(flagged, 0, flagged.n, sigs, names)
