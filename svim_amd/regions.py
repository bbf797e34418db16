"""Region reads of a coordinate-sorted BAM file: the definition the host reader (csrc/bamio.cpp decode_run) and the device reader (csrc/bamdev.hip k_region_*,
both through csrc/region_core.hpp) are held against, the region grammar, and the plan that turns regions and an index into reads.  Pure Python, no GPU, no
library.

  region    (tid, beg, end): 0-based, half-open, on one reference of the header, 0 <= beg < end.
  interval  of a record: the one the index is built from - bai.record_row gives the end, bai.interval the pair: pos (a negative pos read as 0) to pos + the
            reference span of the effective CIGAR (htslib's CG rule).  A placed record without a reference span, or with flag bit 4, occupies [pos, pos + 1).
  rules     RULE_OVERLAP keeps a record of the region's reference when interval.beg < end and interval.end > beg: what `samtools view file region` prints, and
            bai.brute_force.  RULE_START keeps it when beg <= pos < end: ownership - a record belongs to exactly one of a set of abutting regions.
  stop      a read of the region ends (like the end of the file) at the first record that is unplaced, lies on a later reference, or lies on the region's
            reference with pos >= end.  Records of an earlier reference are not kept and do not stop the read.
  run       what a reader hands out: the records from the first kept one to the last one in front of the stop, one contiguous piece of the file; a record of
            the run that the rule does not keep carries SVX_FLAG_SKIP.  A region without a kept record hands out nothing.
  plan      per region the virtual offset where reading starts: max(begin of the first chunk, the linear index's lower bound) from bai.query, the equivalent
            from csi.query.  A region the index proves empty is dropped.  RULE_START uses the same offsets: a record that starts in the region overlaps it.
  several   regions are sorted by (tid, beg) and overlapping or abutting ones of a reference merged (the `samtools view -M` rule): a record appears once, in
            file order.
Reading goes on contiguously from the plan's offset to the stop; hopping between the index's chunks inside a region is not done."""
from . import bai, csi

RULE_OVERLAP, RULE_START = "overlap", "start"
RULES = (RULE_OVERLAP, RULE_START)
MAX_POS = (1 << 31) - 1


def _number(text, what):
    digits = text.replace(",", "")
    if not digits.isdigit():
        raise ValueError("region %r: %r is not a number" % (what, text))
    return int(digits)


def parse_region(text, references, lengths):
    """samtools' grammar -> (tid, beg, end), 0-based half-open: `name`, `name:beg`, `name:beg-`, `name:beg-end` with 1-based inclusive numbers that may hold
    commas.  A text that is a header contig as it stands is that contig, whatever colons it holds; otherwise it is split at its last colon.  ValueError for an
    unknown contig, beg > end, a number that is none"""
    text = text.strip()
    tid_of = {r: i for i, r in enumerate(references)}
    if text in tid_of:
        return tid_of[text], 0, int(lengths[tid_of[text]])
    name, colon, span = text.rpartition(":")
    if not colon or name not in tid_of:
        raise ValueError("region %r: no contig of that name in the header" % text)
    tid = tid_of[name]
    first, _dash, last = span.partition("-")
    beg1 = _number(first, text)
    end = _number(last, text) if last else int(lengths[tid])         # `name:beg` and `name:beg-` run to the end of the contig
    beg = max(beg1, 1) - 1
    if beg1 > end:
        raise ValueError("region %r: begins behind its end" % text)
    return tid, beg, end


def as_region(item, references, lengths):
    """a region string, a (contig name or tid, beg, end) tuple (0-based, half-open) -> (tid, beg, end), checked against the header"""
    if isinstance(item, str):
        tid, beg, end = parse_region(item, references, lengths)
    else:
        name, beg, end = item
        if isinstance(name, str):
            if name not in references:
                raise ValueError("region %r: no contig of that name in the header" % (item,))
            tid = list(references).index(name)
        else:
            tid = int(name)
        beg, end = int(beg), int(end)
    if not 0 <= tid < len(references):
        raise ValueError("region %r: no reference %d in the header" % (item, tid))
    if beg < 0 or end <= beg or end > MAX_POS:
        raise ValueError("region %r: needs 0 <= beg < end" % (item,))
    return tid, beg, end


def normalise(regions):
    """sorted by (tid, beg); overlapping and abutting regions of one reference merged"""
    out = []
    for tid, beg, end in sorted((int(t), int(b), int(e)) for t, b, e in regions):
        if end <= beg:
            raise ValueError("empty region (%d, %d, %d)" % (tid, beg, end))
        if out and out[-1][0] == tid and beg <= out[-1][2]:
            out[-1] = (tid, out[-1][1], max(out[-1][2], end))
        else:
            out.append((tid, beg, end))
    return out


def stops(row, region):
    tid, beg, end = region
    return row[0] < 0 or row[0] > tid or (row[0] == tid and row[1] >= end)


def keeps(row, region, rule=RULE_OVERLAP):
    tid, beg, end = region
    if row[0] != tid or tid < 0:
        return False
    if rule == RULE_START:
        return beg <= row[1] < end
    if rule != RULE_OVERLAP:
        raise ValueError("unknown rule %r" % (rule,))
    lo, hi = bai.interval(row)
    return lo < end and hi > beg


def select(rows, regions, rule=RULE_OVERLAP):
    """the rows (bai.rows_of_bam) kept by any of the regions, in file order, by a scan over every row: what everything else is held to"""
    regions = normalise(regions)
    return [r for r in rows if any(keeps(r, g, rule) for g in regions)]


def run(rows, region, rule=RULE_OVERLAP, start=0):
    """what a reader of one region hands out when it starts at row index `start` (at or in front of the region's first kept row): (first, stop) - the rows
    [first, stop) from the first kept one to the stop - and the kept flags of that run.  (start, start) when nothing is kept"""
    stop = next((k for k in range(start, len(rows)) if stops(rows[k], region)), len(rows))
    first = next((k for k in range(start, stop) if keeps(rows[k], region, rule)), None)
    if first is None:
        return (start, start), []
    return (first, stop), [keeps(rows[k], region, rule) for k in range(first, stop)]


def _parsed(index):
    if isinstance(index, dict):
        return index, ("depth" in index)
    data = bytes(index)
    try:
        if data[:4] == b"BAI\1":
            return bai.parse_index(data), False
        if data[:2] == b"\x1f\x8b":
            data = csi.unframe(data)
        return csi.parse_index(data), True
    except ValueError as e:
        # (records.write_bam leaves a minimal .bai - one bin per reference, no linear index - that says where a contig starts and nothing finer)
        raise ValueError("regions need a full index of the file (bins, linear index, pseudo-bins; harness.index_bam writes one): %s" % e)


def plan(index, regions, rule=RULE_OVERLAP):
    """-> [(voff, tid, beg, end)] in file order for the normalised regions: where the read of each begins.  index: the bytes of a .bai or of a .csi (BGZF-framed
    as on disk, or not), or either parser's dict.  A region the index proves empty is dropped"""
    if rule not in RULES:
        raise ValueError("unknown rule %r" % (rule,))
    ix, is_csi = _parsed(index)
    out = []
    for tid, beg, end in normalise(regions):
        chunks, low = (csi.query if is_csi else bai.query)(ix, tid, beg, end)
        if not chunks:
            continue
        out.append((max(chunks[0][0], low or 0), tid, beg, end))
    return out
