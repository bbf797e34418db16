// bamindex.hpp - internal interface between the device reader (bamdev.hip) and the BAM index it can build from its record stream (bamindex.hip).
#pragma once
#include "common.hpp"

struct BamIndex;
// what one loaded chunk hands over: the decoded arrays of its n records (device), and the chunk's block table (host): n_blk > 0 entries, blk_start[b]
// ascending stream offsets with blk_start[0] <= every rec_off, blk_vbase[b] the virtual offset of blk_start[b]
struct BamIndexChunk {
    long long n; const int32_t *tid, *pos; const uint16_t* flag; const uint64_t* cigar_off; const uint32_t* cigar; const uint64_t* rec_off;
    const uint64_t *blk_start, *blk_vbase; long long n_blk;
};
int  bamindex_begin(BamIndex** ix);                        // an empty table (the state is made on first use)
void bamindex_drop(BamIndex* ix);                          // the table's memory goes back; the bytes of a finished index stay
void bamindex_destroy(BamIndex* ix);
int  bamindex_append(BamIndex* ix, const BamIndexChunk& c, hipStream_t st);
// ready rows instead of appended ones (bamsort.hip: the index of the sorted file): row i of `ix` becomes row perm[i] of `src` - tid, pos, end, flag - with the
// virtual offset of stream offset u = rec_soff[i] in a file of blocks of block_bytes stream bytes each, (coff[u / block_bytes] << 16) | (u % block_bytes).
// perm, rec_soff (n entries) and coff (n_blk entries) are device arrays; whatever `ix` held is replaced
int  bamindex_take_rows(BamIndex* ix, const BamIndex* src, const uint32_t* perm, const int64_t* rec_soff, const int64_t* coff, int64_t n_blk, int64_t block_bytes, hipStream_t st);
int64_t bamindex_rows(const BamIndex* ix);
// the bytes of the .bai (fmt SVX_INDEX_CLASSIC) or the uncompressed .csi (SVX_INDEX_CSI) from the table, which is dropped whatever the result: SVX_OK,
// SVX_E_ORDER, SVX_E_RANGE (a .bai only)
int  bamindex_finish(BamIndex* ix, int32_t n_ref, uint64_t v_end, hipStream_t st, int fmt);
bool bamindex_bytes(const BamIndex* ix, int64_t* n_bytes);        // false: no finished index
int  bamindex_fetch(BamIndex* ix, uint8_t* host_dst, hipStream_t st);
void bamindex_stats(const BamIndex* ix, svx_bam_index_stats* out);
