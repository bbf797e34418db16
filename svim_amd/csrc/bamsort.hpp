// bamsort.hpp - internal interface between the device reader (bamdev.hip) and the sort (coordinate or query-name order) it can feed from its record stream (bamsort.hip).
#pragma once
#include "common.hpp"
#include "bamindex.hpp"

struct BamSort;
// what one loaded chunk hands over: its n records lie back to back in stream[first_byte, end_byte), record i at rec_off[i]; the decoded columns are those the
// index takes (device arrays).  A merge session (bammerge.hip) says which file of several the chunk is of: n_ref_file >= 0 is that file's dictionary size - the
// range checks run over it, the key over the sort's n_ref (the merged dictionary) - and, unless `identity`, tid_map (device, n_ref_file entries) the merged id
// of every reference of the file: the chunk's records then get refID and next_refID translated in the sort's copy (k_bs_translate).  n_ref_file < 0: one file
// sorted alone, nothing of this applies
struct BamSortChunk {
    long long n; const uint8_t* stream; uint64_t first_byte, end_byte; const uint64_t* rec_off;
    const int32_t *tid, *pos; const uint16_t* flag; const uint64_t* cigar_off; const uint32_t* cigar;
    const int32_t* tid_map = nullptr; int32_t n_ref_file = -1; bool identity = true;
};
// an empty arena (the state is made on first use); max_bytes 0: what the device has free.  spill_dir (may be null): the directory of the spill file - a chunk
// that would pass the limit then closes a run (sorted, laid out, written to the file, slabs freed) instead of failing; SVX_E_ARG: not a writable directory
// order: BSORT_COORDINATE or BSORT_QUERYNAME (bamsort_core.hpp); bamsort_index after query-name order is SVX_E_STATE.  Query-name order with a spill directory
// closes its runs in that order and keeps their names in a table (only a merge session begins such a sort; a run that closes refuses what finish refuses with
// SVX_E_ARG at once, from bamsort_append)
int  bamsort_begin(BamSort** s, int64_t max_bytes, int32_t n_ref, const char* spill_dir = nullptr, int order = 0);
void bamsort_drop(BamSort* s);                                         // arena, rows and the encoder's buffers go back
void bamsort_destroy(BamSort* s);
// SVX_E_CAPACITY: the arena would pass max_bytes (nothing of the chunk is kept); with a spill directory only for a chunk that alone passes it.  SVX_E_IO: the spill file
int  bamsort_append(BamSort* s, const BamSortChunk& c, hipStream_t st);
// header: the rewritten header (host).  SVX_E_ARG / SVX_E_RANGE: a record the definition refuses; SVX_E_CAPACITY: more than 2^32 - 1 records
int  bamsort_finish(BamSort* s, const uint8_t* header, int64_t header_bytes, hipStream_t st);
bool bamsort_finished(const BamSort* s);
void bamsort_count(const BamSort* s, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks);
int  bamsort_encode(BamSort* s, int64_t first_block, int64_t n_blocks, int64_t* n_bytes, hipStream_t st);
int  bamsort_fetch(BamSort* s, uint8_t* compressed_dst, uint8_t* stream_dst, hipStream_t st);
// the .bai of the encoded file into `ix` (SVX_E_STATE unless every block was encoded, in ascending gap-free ranges); SVX_E_RANGE as bamindex_finish
int  bamsort_index(BamSort* s, BamIndex* ix, hipStream_t st, int fmt);
int  bamsort_permutation(BamSort* s, uint32_t* host_perm, hipStream_t st);
void bamsort_stats(const BamSort* s, svx_bam_sort_stats* out);
void bamsort_spill_stats(const BamSort* s, svx_bam_sort_spill_stats* out);
void bamsort_name_stats(const BamSort* s, svx_bam_name_sort_stats* out);      // zeros unless the last finish was in query-name order (after runs: the merge's rounds)
void bamsort_name_spill_stats(const BamSort* s, svx_bam_name_spill_stats* out);      // the runs closed in query-name order since begin
// what k_bs_translate has done for the sort since begin: chunks and records it ran over, the bytes it read and wrote, its time between events on the stream
void bamsort_translate_stats(const BamSort* s, int64_t* n_chunks, int64_t* n_records, int64_t* n_bytes, double* ms);
// A sort with the stream it runs on and the slot its index goes to (devdec.hpp: sortout_*; sortout.hip).  The owner - a reader's decoder, a merge session -
// fills it in and outlives it; stream and *index are the owner's and are only borrowed here.  on: appending (the owner's begin sets it, finish and drop clear it)
struct SortOut { int device = 0; hipStream_t stream = nullptr; BamSort* sort = nullptr; BamIndex** index = nullptr; bool on = false; };
