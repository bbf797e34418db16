// bamindex_core.hpp - what a BAM index says about one row (tid, pos, end, flag, vbeg) of a file's record table: the interval, the order and the virtual
// offset, one source for the kernels of bamindex.hip and for svx_bam_index_host (bamindex_host.cpp).  The bins and the layout of a reference's part are
// those a .tbi has as well: binidx_core.hpp.  The definition in words: svim_amd/bai.py.
#pragma once
#include "binidx_core.hpp"

#define BIX_HEADER_BYTES 8                   /* magic + n_ref */
#define BIX_CSI_HEADER_BYTES 20              /* a .csi: magic, min_shift, depth, l_aux = 0, n_ref */

// the interval the index takes for a placed row: a negative pos is read as 0, an end that is not beyond beg as beg + 1
BINIDX_HD BinIdxInterval bix_interval(int32_t pos, int64_t end) {
    BinIdxInterval v; v.beg = pos > 0 ? pos : 0; v.end = end > v.beg ? end : v.beg + 1;
    return v;
}
// end of a placed record from its reference span (32 bits) and its flag
BINIDX_HD int64_t bix_end(int32_t pos, uint32_t span, uint32_t flag) {
    const int64_t beg = pos > 0 ? pos : 0;
    return (flag & 4u) || span == 0u ? beg + 1 : beg + (int64_t)span;
}
// row b directly behind row a: is the pair out of coordinate order?  Unplaced rows (tid < 0) lie behind every placed one and are not compared with each other
BINIDX_HD bool bix_out_of_order(int32_t tid_a, int32_t pos_a, int32_t tid_b, int32_t pos_b) {
    if (tid_a < 0) return tid_b >= 0;
    if (tid_b < 0) return false;
    return tid_b < tid_a || (tid_b == tid_a && pos_b < pos_a);
}
// virtual offset of stream offset u in a table of nb > 0 blocks (start[b] ascending, start[0] <= u; vbase[b]: the virtual offset of start[b]): the last block
// that starts at or before u
BINIDX_HD uint64_t bix_voff(uint64_t u, const uint64_t* start, const uint64_t* vbase, int64_t nb) {
    int64_t lo = 0, hi = nb;                          // first block with start > u
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (start[mid] > u) hi = mid; else lo = mid + 1; }
    const int64_t b = lo > 0 ? lo - 1 : 0;
    return vbase[b] + (u - start[b]);
}
