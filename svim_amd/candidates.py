"""The six SV candidate classes COMBINE hands on (src/svim/SVCandidate.py) as a data surface.

Same constructor argument order, attributes, `get_source` / `get_destination` / `get_key` / `downstream_distance_to` and the genotype fields with the
reference's defaults (`support_fraction "."`, `genotype "./."`, `ref_reads` / `alt_reads None`), table-driven like signatures.py: one row of _SPEC per
class instead of one hand-written constructor each.  The VCF / BED text of candidates is not part of this surface ("COMBINE on the device").
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


CLASSES = (CandidateDeletion, CandidateInversion, CandidateDuplicationInterspersed, CandidateDuplicationTandem, CandidateNovelInsertion, CandidateBreakend)
