// binidx_core.hpp - the binning index a .tbi and a .bai share, behind the point where a record has become (group, beg, end, vbeg): the five-level bins, the
// limits, the unaligned little-endian stores and the size of a group's part (a contig's in a .tbi, a reference's in a .bai).  One source for the kernels
// (binidx_kernels.hpp), for the host writer (binidx_host.hpp) and for what each index keeps to itself (textindex_core.hpp, bamindex_core.hpp).
// The definition in words: svim_amd/tabix.py (contig_part).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define BINIDX_HD __host__ __device__ __forceinline__
#else
#define BINIDX_HD inline
#endif

#define BINIDX_MAX_END (1ll << 29)           /* what the five-level binning holds */
#define BINIDX_PSEUDO_BIN 37450u
#define BINIDX_NO_SLOT 0xffffffffffffffffull
#define BINIDX_EMPTY_PART_BYTES 8            /* a group without rows: n_bin = 0, n_intv = 0 (a .bai has them, a .tbi never) */

struct BinIdxInterval { int64_t beg, end; };    // 0-based, half-open, end > beg

BINIDX_HD uint32_t binidx_reg2bin(int64_t beg, int64_t end) {
    end--;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0u;
}
// the bin of a row (one that ends beyond the limit has none: its file is refused before a bin is written)
BINIDX_HD uint32_t binidx_bin(const BinIdxInterval& v) { return v.end <= BINIDX_MAX_END ? binidx_reg2bin(v.beg, v.end) : 0u; }
// little-endian stores at any alignment
BINIDX_HD void binidx_put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
BINIDX_HD void binidx_put64(uint8_t* p, uint64_t v) { binidx_put32(p, (uint32_t)v); binidx_put32(p + 4, (uint32_t)(v >> 32)); }
// the bytes of the part of a group with rows: n_bin, its bins with their chunks, the pseudo-bin, n_intv, the linear index
BINIDX_HD int64_t binidx_part_bytes(int64_t n_bins, int64_t n_chunks, int64_t n_intv) { return 4 + 8 * n_bins + 16 * n_chunks + 40 + 4 + 8 * n_intv; }

// ---- the CSI form: the same bins at a depth chosen per file, a loffset per bin in place of the linear index (the definition in words: svim_amd/csi.py) ----
#define BINIDX_CSI_MIN_SHIFT 14              /* 16 kb leaves, as the five-level scheme has them */
#define BINIDX_CSI_MIN_DEPTH 5
#define BINIDX_CSI_MAX_DEPTH 9               /* 2^41: beyond the text parser's cap of 2^40 plus a line's REF; a BAM never needs more than 7 */
#define BINIDX_CSI_EMPTY_PART_BYTES 4        /* a group without rows: n_bin = 0 */

// the smallest depth >= 5 whose root bin covers [0, max_end)
BINIDX_HD int binidx_depth_for(int64_t max_end) {
    int d = BINIDX_CSI_MIN_DEPTH;
    while (d < BINIDX_CSI_MAX_DEPTH && max_end > (1ll << (BINIDX_CSI_MIN_SHIFT + 3 * d))) d++;
    return d;
}
// the CSI specification's reg2bin at min_shift 14 (depth 5: binidx_reg2bin)
BINIDX_HD uint32_t binidx_reg2bin_csi(int64_t beg, int64_t end, int depth) {
    int l = depth, s = BINIDX_CSI_MIN_SHIFT;
    int64_t t = ((1ll << (3 * depth)) - 1) / 7;
    for (--end; l > 0; --l, s += 3, t -= 1ll << (3 * l)) if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    return 0u;
}
// the first coordinate a bin covers
BINIDX_HD int64_t binidx_bin_start(uint32_t bin, int depth) {
    int l = 0; int64_t first = 0;                 // the level of the bin, and the first bin of that level
    while (l < depth && (int64_t)bin >= first + (1ll << (3 * l))) { first += 1ll << (3 * l); l++; }
    return ((int64_t)bin - first) << (BINIDX_CSI_MIN_SHIFT + 3 * (depth - l));
}
BINIDX_HD uint32_t binidx_csi_pseudo_bin(int depth) { return (uint32_t)(((1ll << (3 * depth + 3)) - 1) / 7 + 1); }
// sort key of a chunk in the CSI form: the bin in the low 3 * (depth + 1) bits (it is below 8^(depth + 1) / 7), the group above
BINIDX_HD int binidx_csi_key_shift(int depth) { return 3 * (depth + 1); }
BINIDX_HD uint64_t binidx_csi_key(uint64_t group, uint32_t bin, int depth) { return (group << binidx_csi_key_shift(depth)) | bin; }
// the bytes of the part of a group with rows: n_bin, its bins (bin, loffset, n_chunk) with their chunks, the pseudo-bin with its two pairs
BINIDX_HD int64_t binidx_csi_part_bytes(int64_t n_bins, int64_t n_chunks) { return 4 + 16 * n_bins + 16 * n_chunks + 48; }
