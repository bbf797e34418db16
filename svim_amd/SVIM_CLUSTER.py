"""GPU-backed counterpart of src/svim/SVIM_CLUSTER.py."""
from .SVIM_clustering import cluster_signature_lists, partition_and_cluster      # noqa: F401


def cluster_sv_signatures(sv_signatures, options):
    """Split by type, partition, cluster, consolidate (src/svim/SVIM_CLUSTER.py:7-26) - one device pass for all
    six types.  Returns (DEL, INS, INV, DUP_TAN, DUP_INT, BND) lists of SignatureCluster{UniLocal,BiLocal}."""
    return cluster_signature_lists(sv_signatures, options)


# ---- writers (src/svim/SVIM_CLUSTER.py:29-106): same files, same lines ------------------------------------------------------
# (file name, slot of the 6-tuple, which bed line(s) of a cluster go into it)
_BED_FILES = (("del.bed", 0, None), ("ins.bed", 1, None), ("inv.bed", 2, None),
              ("dup_tan_source.bed", 3, (0,)), ("dup_tan_dest.bed", 3, (1,)),
              ("trans.bed", 5, (0, 1)), ("dup_int.bed", 4, (0, 1)))
_VCF_HEADER = (
    "##fileformat=VCFv4.3", "##source=SVIMV{version}",
    '##ALT=<ID=DEL,Description="Deletion">', '##ALT=<ID=INV,Description="Inversion">', '##ALT=<ID=DUP,Description="Duplication">',
    '##ALT=<ID=DUP:TANDEM,Description="Tandem Duplication">', '##ALT=<ID=INS,Description="Insertion">',
    '##INFO=<ID=END,Number=1,Type=Integer,Description="End position of the variant described in this record">',
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
    '##INFO=<ID=SVLEN,Number=.,Type=Integer,Description="Difference in length between REF and ALT alleles">',
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")


def _signature_dir(working_dir):
    import os
    d = os.path.join(working_dir, "signatures")
    os.makedirs(d, exist_ok=True)
    return d


def signature_bed_texts_python(clusters):
    """The text of the seven BED files (in _BED_FILES order) from cluster OBJECTS, as the reference's writer makes it (src/svim/SVIM_CLUSTER.py:44-61): the
    definition the device writer (svx_bed, csrc/bed.hip) is held against."""
    texts = []
    for name, slot, which in _BED_FILES:
        lines = []
        for cluster in clusters[slot]:
            if which is None:
                lines.append(cluster.get_bed_entry() + "\n")
            else:
                entries = cluster.get_bed_entries()
                lines.extend(entries[k] + "\n" for k in which)
        texts.append("".join(lines))
    return texts


def signature_vcf_body_python(clusters):
    """The lines of signatures/all.vcf behind the header from cluster OBJECTS: the DEL / INS / INV / DUP_TAN clusters in that append order, sorted stably by
    their source tuple - contig NAME as a string, start, end (src/svim/SVIM_CLUSTER.py:93-105)."""
    entries = [(c.get_source(), c.get_vcf_entry()) for slot in (0, 1, 2, 3) for c in clusters[slot]]
    return "".join("%s\n" % entry for _, entry in sorted(entries, key=lambda pair: pair[0]))


def vcf_header_text(version):
    return "".join(line.format(version=version) + "\n" for line in _VCF_HEADER)


def write_signature_clusters_bed_python(working_dir, clusters):
    """write_signature_clusters_bed over the objects (every cluster and every member signature is materialised)"""
    import os
    d = _signature_dir(working_dir)
    for (name, _, _), text in zip(_BED_FILES, signature_bed_texts_python(clusters)):
        with open(os.path.join(d, name), "w") as fh:
            fh.write(text)


def write_signature_clusters_vcf_python(working_dir, clusters, version):
    """write_signature_clusters_vcf over the objects"""
    import os
    with open(os.path.join(_signature_dir(working_dir), "all.vcf"), "w") as fh:
        fh.write(vcf_header_text(version))
        fh.write(signature_vcf_body_python(clusters))


def write_signature_clusters_bed(working_dir, clusters, engine=None):
    """<working_dir>/signatures/{del,ins,inv,dup_tan_source,dup_tan_dest,trans,dup_int}.bed (src/svim/SVIM_CLUSTER.py:29-70).  The lines are made on the
    device (svx_bed) where the clusters are, or fit, a cluster table (svim_amd.bed.signature_text says which route a call takes); the Python definition
    (write_signature_clusters_bed_python) otherwise."""
    from . import bed
    done = bed.signature_text(_abi_product("SIGNATURE_BEDS"), clusters, engine=engine)
    if done is None:
        return write_signature_clusters_bed_python(working_dir, clusters)
    bed.write_files(done[0], _signature_dir(working_dir), [name for name, _, _ in _BED_FILES])


def write_signature_clusters_vcf(working_dir, clusters, version, engine=None):
    """<working_dir>/signatures/all.vcf: header, then the DEL / INS / INV / DUP_TAN clusters sorted by source locus (src/svim/SVIM_CLUSTER.py:73-106).
    The header is written here, the lines behind it on the device where the route allows (see write_signature_clusters_bed)."""
    from . import bed
    done = bed.signature_text(_abi_product("SIGNATURE_VCF"), clusters, engine=engine)
    if done is None:
        return write_signature_clusters_vcf_python(working_dir, clusters, version)
    bed.write_files(done[0], _signature_dir(working_dir), ["all.vcf"], heads=[vcf_header_text(version).encode("utf-8")])


def _abi_product(name):
    from . import _abi
    return getattr(_abi, "BED_" + name)
