"""The six SV candidate classes COMBINE hands on (src/svim/SVCandidate.py) as a data surface.

Same constructor argument order, attributes, `get_source` / `get_destination` / `get_key` / `downstream_distance_to` and the genotype fields with the
reference's defaults (`support_fraction "."`, `genotype "./."`, `ref_reads` / `alt_reads None`), table-driven like signatures.py: one row of _SPEC per
class instead of one hand-written constructor each.  The nine `get_vcf_entry*` methods are one row of _VCF each over one formatter (`vcf_entry`): the readable
definition of a VCF line that the device writer (csrc/vcf.hip) is held against.  `get_bed_entry` / `get_bed_entries` are rows of _BED over `bed_entry` in the same
way: the definition of a line of the candidate BED files (csrc/bed.hip).
`members` may be handed over as (signature sequence, index array) and resolves to signature objects on first read, as for clusters.
"""
from .signatures import _LazyMembers

_INF = float("inf")
_GENOTYPE_DEFAULTS = (("support_fraction", "."), ("genotype", "./."), ("ref_reads", None), ("alt_reads", None))


class Candidate(_LazyMembers):
    type = None
    _args = ("source_contig", "source_start", "source_end", "members", "score", "std_span", "std_pos")
    _clamped = ()                      # arguments stored as max(0, value)

    def __init__(self, *args, **kwargs):
        names = self._args + tuple(k for k, _ in _GENOTYPE_DEFAULTS)
        if len(args) > len(names):
            raise TypeError("%s() takes at most %d arguments (%d given)" % (self.__class__.__name__, len(names), len(args)))
        values = dict(_GENOTYPE_DEFAULTS)
        values.update(getattr(self, "_defaults", {}))
        values.update(zip(names, args))
        for k, v in kwargs.items():
            if k not in names or k in names[:len(args)]:
                raise TypeError("%s() got an unexpected or repeated argument %r" % (self.__class__.__name__, k))
            values[k] = v
        missing = [k for k in self._args if k not in values]
        if missing:
            raise TypeError("%s() missing argument(s) %s" % (self.__class__.__name__, ", ".join(missing)))
        for k in names:
            v = values[k]
            setattr(self, k, max(0, v) if k in self._clamped else v)
        self.type = self.__class__.type

    def get_source(self):
        return (self.source_contig, self.source_start, self.source_end)

    def get_key(self):
        contig, start, end = self.get_source()
        return (self.type, contig, end)

    def downstream_distance_to(self, candidate2):
        this_contig, this_start, this_end = self.get_source()
        other_contig, other_start, other_end = candidate2.get_source()
        if self.type == candidate2.type and this_contig == other_contig:
            return max(0, other_start - this_end)
        return _INF

    def get_std_span(self, ndigits=2):
        return round(self.std_span, ndigits) if self.std_span else "."

    def get_std_pos(self, ndigits=2):
        return round(self.std_pos, ndigits) if self.std_pos else "."

    def __repr__(self):
        return "<%s %s>" % (self.__class__.__name__, " ".join("%s=%r" % (k, getattr(self, k)) for k in self._args if k != "members"))


class CandidateDeletion(Candidate):
    type = "DEL"
    _clamped = ("source_start",)


class CandidateInversion(Candidate):
    type = "INV"
    _clamped = ("source_start",)

    def __init__(self, *args, **kwargs):
        Candidate.__init__(self, *args, **kwargs)
        self.complement = {"A": "T", "C": "G", "G": "C", "T": "A"}


class CandidateNovelInsertion(Candidate):
    type = "INS"
    _args = ("dest_contig", "dest_start", "dest_end", "sequence", "members", "score", "std_span", "std_pos")
    _clamped = ("dest_start",)

    def get_destination(self):
        return (self.dest_contig, self.dest_start, self.dest_end)


class CandidateDuplicationTandem(Candidate):
    type = "DUP_TAN"
    _args = ("source_contig", "source_start", "source_end", "copies", "fully_covered", "members", "score", "std_span", "std_pos")
    _clamped = ("source_start",)

    def get_destination(self):
        source_contig, source_start, source_end = self.get_source()
        return (source_contig, source_end, source_end + self.copies * (source_end - source_start))


class CandidateDuplicationInterspersed(Candidate):
    type = "DUP_INT"
    _args = ("source_contig", "source_start", "source_end", "dest_contig", "dest_start", "dest_end", "members", "score", "std_span", "std_pos", "cutpaste")
    _defaults = {"cutpaste": False}
    _clamped = ("source_start", "dest_start")

    def get_destination(self):
        return (self.dest_contig, self.dest_start, self.dest_end)


class CandidateBreakend(Candidate):
    type = "BND"
    _args = ("source_contig", "source_start", "source_direction", "dest_contig", "dest_start", "dest_direction", "members", "score", "std_pos1", "std_pos2")
    _clamped = ("source_start", "dest_start")

    def get_source(self):
        return (self.source_contig, self.source_start)

    def get_destination(self):
        return (self.dest_contig, self.dest_start)

    def get_std_pos1(self, ndigits=2):
        return round(self.std_pos1, ndigits) if self.std_pos1 else "."

    def get_std_pos2(self, ndigits=2):
        return round(self.std_pos2, ndigits) if self.std_pos2 else "."


# ---- VCF text (src/svim/SVCandidate.py: get_vcf_entry / get_vcf_entry_as_ins / get_vcf_entry_as_dup / get_vcf_entry_reverse) ---------------------------------
def _fetch(reference, contig, start, end):
    return reference.fetch(contig, start, end).upper()


def _bnd_alt(n_first, opening, contig, start):
    b = "[" if opening else "]"
    return ("N" if n_first else "") + "%s%s:%d%s" % (b, contig, start + 1, b) + ("" if n_first else "N")


class _VcfRow(object):
    """One get_vcf_entry* method: where the line sits, what its INFO holds between SVTYPE and SUPPORT, its alleles.
    args: the method's parameters in the reference's order; place(c) -> (CHROM, POS); mid(c) -> text behind "SVTYPE=<svtype>;" and in front of
    "SUPPORT="; alleles(c, reference) -> (REF, ALT) with sequence alleles, None: the method has symbolic alleles only; symbolic(c) -> ALT otherwise."""

    def __init__(self, args, svtype, place, mid, symbolic, alleles=None, std=(("STD_SPAN", "get_std_span"), ("STD_POS", "get_std_pos")), tandem=False, cn=False,
                 seqs=False):
        self.args, self.svtype, self.place, self.mid, self.symbolic, self.alleles, self.std = args, svtype, place, mid, symbolic, alleles, std
        self.tandem, self.cn, self.seqs = tandem, cn, seqs


_SEQ_ARGS = ("sequence_alleles", "reference", "read_names", "zmws")
_complement = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _inv_alleles(c, reference):
    ref = _fetch(reference, c.source_contig, c.source_start, c.source_end)
    return ref, "".join(_complement.get(b, b) for b in reversed(ref))


def _del_alleles(c, reference):
    p = max(0, c.source_start - 1)
    return _fetch(reference, c.source_contig, p, c.source_end), _fetch(reference, c.source_contig, p, c.source_start)


def _ins_alleles(c, reference):
    if c.sequence == "":
        return None
    p = max(0, c.dest_start - 1)
    ref = _fetch(reference, c.dest_contig, p, p + 1)
    return ref, ref + c.sequence


def _tan_alleles(c, reference):
    ref = _fetch(reference, c.source_contig, c.source_start, c.source_end)
    return ref, ref * (c.copies + 1)


def _int_alleles(c, reference):
    p = max(0, c.dest_start - 1)
    ref = _fetch(reference, c.dest_contig, p, p + 1)
    return ref, ref + _fetch(reference, c.source_contig, c.source_start, c.source_end)


_cut = lambda c: "CUTPASTE;" if c.cutpaste else ""      # noqa: E731
_VCF = {
    ("DEL", "get_vcf_entry"): _VcfRow(_SEQ_ARGS, "DEL", lambda c: (c.source_contig, max(1, c.source_start)),
                                      lambda c: "END=%d;SVLEN=%d;" % (c.source_end, c.source_start - c.source_end), lambda c: "<DEL>", _del_alleles),
    ("INV", "get_vcf_entry"): _VcfRow(_SEQ_ARGS, "INV", lambda c: (c.source_contig, c.source_start + 1), lambda c: "END=%d;" % c.source_end, lambda c: "<INV>",
                                      _inv_alleles),
    ("INS", "get_vcf_entry"): _VcfRow(("sequence_alleles", "reference", "insertion_sequences", "read_names", "zmws"), "INS",
                                      lambda c: (c.dest_contig, max(1, c.dest_start)), lambda c: "END=%d;SVLEN=%d;" % (c.dest_start, c.dest_end - c.dest_start),
                                      lambda c: "<INS>", _ins_alleles, seqs=True),
    ("DUP_TAN", "get_vcf_entry_as_ins"): _VcfRow(_SEQ_ARGS, "INS", lambda c: (c.source_contig, c.source_start + 1),
                                                 lambda c: "END=%d;SVLEN=%d;" % (c.source_end, c.get_destination()[2] - c.get_destination()[1]),
                                                 lambda c: "<DUP_TAN>", _tan_alleles, tandem=True),
    ("DUP_TAN", "get_vcf_entry_as_dup"): _VcfRow(("read_names", "zmws"), "DUP:TANDEM", lambda c: (c.source_contig, c.source_start + 1),
                                                 lambda c: "END=%d;SVLEN=%d;" % (c.source_end, c.source_end - c.source_start), lambda c: "<DUP:TANDEM>",
                                                 tandem=True, cn=True),
    ("DUP_INT", "get_vcf_entry_as_ins"): _VcfRow(_SEQ_ARGS, "INS", lambda c: (c.dest_contig, max(1, c.dest_start)),
                                                 lambda c: "%sEND=%d;SVLEN=%d;" % (_cut(c), c.dest_start, c.dest_end - c.dest_start), lambda c: "<DUP_INT>",
                                                 _int_alleles),
    ("DUP_INT", "get_vcf_entry_as_dup"): _VcfRow(("read_names", "zmws"), "DUP:INT", lambda c: (c.source_contig, c.source_start + 1),
                                                 lambda c: "%sEND=%d;SVLEN=%d;" % (_cut(c), c.source_end, c.source_end - c.source_start), lambda c: "<DUP:INT>"),
    ("BND", "get_vcf_entry"): _VcfRow(("read_names", "zmws"), "BND", lambda c: (c.source_contig, c.source_start + 1), lambda c: "",
                                      lambda c: _bnd_alt(c.source_direction == "fwd", c.dest_direction == "fwd", c.dest_contig, c.dest_start),
                                      std=(("STD_POS1", "get_std_pos1"), ("STD_POS2", "get_std_pos2"))),
    ("BND", "get_vcf_entry_reverse"): _VcfRow(("read_names", "zmws"), "BND", lambda c: (c.dest_contig, c.dest_start + 1), lambda c: "",
                                              lambda c: _bnd_alt(c.dest_direction == "rev", c.source_direction == "rev", c.source_contig, c.source_start),
                                              std=(("STD_POS1", "get_std_pos2"), ("STD_POS2", "get_std_pos1"))),
}


def vcf_entry(c, row, sequence_alleles=False, reference=None, insertion_sequences=False, read_names=False, zmws=False):
    """The VCF line of candidate `c` under row `row` of _VCF, with PLACEHOLDERFORID where write_final_vcf puts the id."""
    chrom, pos = row.place(c)
    alleles = row.alleles(c, reference) if (sequence_alleles and row.alleles is not None) else None
    ref, alt = alleles if alleles is not None else ("N", row.symbolic(c))
    filters = (["hom_ref"] if c.genotype == "0/0" else []) + (["not_fully_covered"] if row.tandem and not c.fully_covered else [])
    reads = [m.read for m in c.members]
    info = "SVTYPE=%s;%sSUPPORT=%d;%s" % (row.svtype, row.mid(c), len(set(reads)), ";".join("%s=%s" % (k, getattr(c, g)()) for k, g in row.std))
    if row.seqs and insertion_sequences:
        info += ";SEQS=" + ",".join(m.sequence for m in c.members)
    if read_names:
        info += ";READS=" + ",".join(reads)
    if zmws:
        fields = [r.split("/") for r in reads]
        if all(len(f) == 3 for f in fields):
            info += ";ZMWS=%d" % len(set("/".join(f[0:2]) for f in fields))
    none = lambda v: "." if v is None else v      # noqa: E731
    dp = str(c.ref_reads + c.alt_reads) if c.ref_reads is not None and c.alt_reads is not None else "."
    sample = [c.genotype] + ([str(c.copies + 1)] if row.cn else []) + [dp, "%s,%s" % (none(c.ref_reads), none(c.alt_reads))]
    return "\t".join([chrom, str(pos), "PLACEHOLDERFORID", ref, alt, str(int(c.score)), ";".join(filters) or "PASS", info, "GT:CN:DP:AD" if row.cn else "GT:DP:AD",
                      ":".join(sample)])


def _vcf_method(row, name):
    defaults = dict(sequence_alleles=False, reference=None, insertion_sequences=False, read_names=False, zmws=False)

    def method(self, *args, **kwargs):
        if len(args) > len(row.args):
            raise TypeError("%s() takes at most %d arguments (%d given)" % (name, len(row.args), len(args)))
        o = dict(defaults)
        o.update(zip(row.args, args))
        for k, v in kwargs.items():
            if k not in row.args or k in row.args[:len(args)]:
                raise TypeError("%s() got an unexpected or repeated argument %r" % (name, k))
            o[k] = v
        return vcf_entry(self, row, **o)
    method.__name__ = name
    return method


CLASSES = (CandidateDeletion, CandidateInversion, CandidateDuplicationInterspersed, CandidateDuplicationTandem, CandidateNovelInsertion, CandidateBreakend)
for (_type, _name), _row in _VCF.items():
    setattr({c.type: c for c in CLASSES}[_type], _name, _vcf_method(_row, _name))


# ---- BED text (src/svim/SVCandidate.py: get_bed_entry :52, :219; get_bed_entries :302, :455, :618) -------------------------------------------------------------
class _BedRow(object):
    """One BED line of a candidate: locus(c) -> (contig, start, end); name(c) -> the 4th column; extra(c) -> the column between the score and the members
    ("." or the cut&paste note), None: the line has none (breakends).  The score and the deviations go through str.format as they are: the score is printed
    with repr's digits, the deviations as get_std_*() rounds them ("." for None and 0.0)."""

    def __init__(self, locus, name, extra=lambda c: "."):
        self.locus, self.name, self.extra = locus, name, extra


_src = lambda c: (c.source_contig, c.source_start, c.source_end)      # noqa: E731
_dst = lambda c: c.get_destination()                                  # noqa: E731
_std = lambda c: "%s;%s" % (c.get_std_span(), c.get_std_pos())        # noqa: E731
_std12 = lambda c: "%s;%s" % (c.get_std_pos1(), c.get_std_pos2())     # noqa: E731
_note = lambda c: "origin potentially deleted" if c.cutpaste else "."      # noqa: E731
_plain = lambda c: "%s;%s" % (c.type, _std(c))                        # noqa: E731
# type -> (method name, rows): one row -> get_bed_entry, two -> get_bed_entries (source entry, destination entry)
_BED = {
    "DEL": ("get_bed_entry", (_BedRow(_src, _plain),)),
    "INV": ("get_bed_entry", (_BedRow(_src, _plain),)),
    "INS": ("get_bed_entry", (_BedRow(_dst, _plain),)),
    "DUP_TAN": ("get_bed_entries", (_BedRow(_src, lambda c: "tan_dup_source;>%s:%s-%s;%s" % (_dst(c) + (_std(c),))),
                                    _BedRow(_dst, lambda c: "tan_dup_dest;<%s:%s-%s;%s" % (_src(c) + (_std(c),))))),
    "DUP_INT": ("get_bed_entries", (_BedRow(_src, lambda c: "int_dup_source;>%s:%s-%s;%s" % (_dst(c) + (_std(c),)), _note),
                                    _BedRow(_dst, lambda c: "int_dup_dest;<%s:%s-%s;%s" % (_src(c) + (_std(c),)), _note))),
    "BND": ("get_bed_entries", (_BedRow(lambda c: (c.source_contig, c.source_start, c.source_start + 1),
                                        lambda c: "bnd;>%s:%s;%s" % (c.dest_contig, c.dest_start, _std12(c)), lambda c: None),
                                _BedRow(lambda c: (c.dest_contig, c.dest_start, c.dest_start + 1),
                                        lambda c: "bnd;<%s:%s;%s" % (c.source_contig, c.source_start, _std12(c)), lambda c: None))),
}


def bed_entry(c, row, sep="\t"):
    """The BED line of candidate `c` under row `row` of _BED, without the newline."""
    extra = row.extra(c)
    members = "[" + "][".join(m.as_string("|") for m in c.members) + "]"
    cols = row.locus(c) + (row.name(c), c.score) + (() if extra is None else (extra,)) + (members,)
    return sep.join("{0}".format(x) for x in cols)


def _bed_methods():
    for cls in CLASSES:
        name, rows = _BED[cls.type]
        if len(rows) == 1:
            setattr(cls, name, lambda self, _r=rows[0]: bed_entry(self, _r))
        else:
            setattr(cls, name, lambda self, sep="\t", _r=rows: (bed_entry(self, _r[0], sep), bed_entry(self, _r[1], sep)))
        getattr(cls, name).__name__ = name


_bed_methods()
