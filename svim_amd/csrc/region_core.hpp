// region_core.hpp - what a region read (svx_bam_seek_region) says about one record of a coordinate-sorted file: where the read stops, which records it keeps
// under either rule, and the interval a record occupies.  One source for the kernels of bamdev.hip (k_region_*) and for the host reader (bamio.cpp
// decode_run).  The definition in words: svim_amd/regions.py.
#pragma once
#include "bamindex_core.hpp"

struct RegionBound { int32_t tid, beg, end; int rule; };       // [beg, end) on reference tid, 0-based; rule: SVX_REGION_OVERLAP or SVX_REGION_START

// the read stops (like the end of the file) at the first record that is unplaced, lies on a later reference, or starts at or behind the region's end
BINIDX_HD bool region_stops(const RegionBound& g, int32_t tid, int32_t pos) { return tid < 0 || tid > g.tid || (tid == g.tid && pos >= g.end); }
// a record in front of the stop whose decision needs no CIGAR: it lies on an earlier reference (never kept), or it starts inside the region (kept under both
// rules: a record that starts in [beg, end) overlaps it).  Only a record of the region's reference with pos < beg needs its reference span, and only under
// SVX_REGION_OVERLAP
BINIDX_HD bool region_starts_inside(const RegionBound& g, int32_t tid, int32_t pos) { return tid == g.tid && pos >= g.beg && pos < g.end; }
BINIDX_HD bool region_needs_span(const RegionBound& g, int32_t tid, int32_t pos) { return g.rule == 0 && tid == g.tid && pos < g.beg; }
// the keep test of a record in front of the stop.  span: the reference span of its effective CIGAR (32 bits; read only where region_needs_span holds).  The
// interval is the index's own (bix_end, bix_interval): a negative pos is read as 0, a record without a span or with flag bit 4 occupies [pos, pos + 1)
BINIDX_HD bool region_keeps(const RegionBound& g, int32_t tid, int32_t pos, uint32_t span, uint32_t flag) {
    if (tid != g.tid) return false;
    if (g.rule != 0) return pos >= g.beg && pos < g.end;
    const BinIdxInterval v = bix_interval(pos, bix_end(pos, span, flag));
    return v.beg < (int64_t)g.end && v.end > (int64_t)g.beg;
}
