// devdec.hpp - internal interface between the host side of the BAM reader (bamio.cpp, plain C++) and its device-resident decode path (bamdev.hip):
// BGZF blocks -> inflated stream in HBM -> record table -> svx_batch arrays on the device.  No HIP types here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/svx.h"

struct DevDecBlock { const uint8_t* comp; uint32_t clen, isize, crc; uint64_t coff; };   // one BGZF block: raw DEFLATE payload in the memory-mapped file, inflated size, CRC32 of the inflated bytes, where the block starts in the file

struct svx_devdec;
// names_blob: the reference names NUL-separated in header order (SA tags name contigs)
int  devdec_create(int device, int n_threads /* CPUs the host's share of the inflate may use */, int32_t n_ref, const int32_t* ref_len, const char* names_blob, const int32_t* contig_rank, svx_devdec** out);
void devdec_destroy(svx_devdec* d);
// Inflate `n` blocks into chunk slot `slot` (0..2) behind the unconsumed tail of slot `carry_slot` (-1: none), skip `skip_bytes` at the start of the
// stream (the BAM header, first chunk only), find every complete record and decode all of them.  final_chunk: nothing follows (a partial record at the
// end is an error).  min_mapq: primaries below it get no segment rows (src/svim/SVIM_COLLECT.py:143-161).
// mode 1 = query-name-sorted input (src/svim/SVIM_COLLECT.py:96-129): no SA tag is expanded, and unless final_chunk the last read's group of the chunk is left to the
// next load (groups never straddle loads).
int  devdec_load(svx_devdec* d, int slot, const DevDecBlock* blocks, size_t n, int carry_slot, uint64_t skip_bytes, bool final_chunk, int min_mapq, int mode);
// The same for a slice of SAM text made of whole alignment lines (sam.hip builds the record stream from it; nothing is carried over between slices).
// line_base: lines of the file in front of the slice.  *consumed: the text bytes whose records the slot holds - all of them, except in query-name mode, where the
// last read's group is left to the next slice.  A refused line: SVX_E_ARG / SVX_E_RANGE, named by its number in the file.
int  devdec_load_text(svx_devdec* d, int slot, const uint8_t* text, size_t n, bool final_chunk, int min_mapq, int mode, int64_t line_base, uint64_t* consumed, int64_t* n_lines);
void devdec_sam_stats(const svx_devdec* d, svx_sam_stats* out);
// records decoded in the slot; n_valid: those before the first record whose reference id is negative or above tid_limit (tid_limit -2: all)
int  devdec_count(svx_devdec* d, int slot, int32_t tid_limit, int64_t* n_rec, int64_t* n_valid);
// Region reads (svx_bam_seek_region; region_core.hpp): over the records of the slot, *stop = the first stopping record (n_rec: none), *first_kept = the first
// record the rule keeps (n_rec: none), *n_kept = the records it keeps; SVX_FLAG_SKIP is or-ed into the flags of the records of [first_kept - or 0 when the
// region has `started` in an earlier chunk - , stop) that the rule does not keep
int  devdec_region(svx_devdec* d, int slot, int32_t tid, int32_t beg, int32_t end, int rule, bool started, int64_t* first_kept, int64_t* stop, int64_t* n_kept);
// bytes of the slot's inflated stream behind its last complete record (what the next load would carry over)
uint64_t devdec_tail_bytes(const svx_devdec* d, int slot);
// device-resident svx_batch over records [first, first + count) of the slot (arrays stay valid until the slot is loaded again)
// mode 1: *count grows to the end of the read group it ends in; flags carry SVX_FLAG_SKIP, the segment table holds the good supplementary records of every analysed
// read and the emission slots follow the reference's per-read order (bamio.cpp svx_bam_read_batch does the same on the host)
int  devdec_batch(svx_devdec* d, int slot, int64_t first, int64_t* count, int mode, int min_mapq, svx_batch* out);
// read names interned so far, id order (host copy; grows with every load)
const std::vector<std::string>& devdec_names(svx_devdec* d);
// timing / accounting of the loads so far
struct DevDecStats { double t_stage = 0, t_inflate_wait = 0, t_discover = 0, t_decode = 0, t_names = 0; int64_t blocks = 0, gpu_blocks = 0, cpu_blocks = 0, bytes = 0, records = 0, fallbacks = 0; double inflate_kernel_ms = 0; };
void devdec_stats(svx_devdec* d, DevDecStats* out);
void devdec_reset_names(svx_devdec* d);
// BAM index from the record stream (bamindex.hip; include/svx.h: svx_bam_index*).  begin: an empty row table, every later devdec_load appends the records it
// hands to devdec_count (once per chunk, on the loader's stream).  finish: the bytes of the .bai (v_end: the virtual offset where the file's data ends) - SVX_OK,
// SVX_E_ORDER or SVX_E_RANGE; indexing is off and the table dropped afterwards, as after drop.  Never begun: devdec_load does nothing for it.
int  devdec_index_begin(svx_devdec* d);
void devdec_index_drop(svx_devdec* d);
bool devdec_index_on(const svx_devdec* d);
int  devdec_index_finish(svx_devdec* d, uint64_t v_end, int fmt);
bool devdec_index_bytes(const svx_devdec* d, int64_t* n_bytes);
int  devdec_index_fetch(svx_devdec* d, uint8_t* host_dst);
void devdec_index_stats(const svx_devdec* d, svx_bam_index_stats* out);
// Sort from the record stream (bamsort.hip; include/svx.h: svx_bam_sort*).  begin: an empty arena, every later devdec_load appends the bytes and the rows of the
// records it hands to devdec_count (once per chunk, on the loader's stream, with no synchronise of its own); a load whose records pass max_bytes fails with
// SVX_E_CAPACITY and drops the sort.  on: appending, from begin to the finish or drop of devdec_sort_out (below), which holds everything else.
int  devdec_sort_begin(svx_devdec* d, int64_t max_bytes, const char* spill_dir /* null: no spill file, SVX_E_CAPACITY at the limit */, int order = 0 /* SVX_SORT_* */);
bool devdec_sort_on(const svx_devdec* d);
// A merge session's feed (svx_bam_merge_add; bammerge.hip): while set, every devdec_load appends the records it hands to devdec_count to the SESSION's sort -
// in this decoder's loader thread but on the SESSION's stream (both are `session`'s), once the decoder's own stream has been drained - as records of a
// file with n_ref_file references whose ids dev_map (device memory of the session; unused when `identity`) takes into the merged dictionary.  Every command that
// touches the session's memory thus runs on the one stream that lives as long as that memory does, whichever readers come and go.  The decoder borrows the sort
// and never owns it: a failed append clears the feed and fails the load, nothing else.  Set and cleared only while no loader runs.
struct SortOut;
void devdec_feed_set(svx_devdec* d, SortOut* session, const int32_t* dev_map, int32_t n_ref_file, bool identity);
void devdec_feed_clear(svx_devdec* d);
bool devdec_feed_on(const svx_devdec* d);
int  devdec_device(const svx_devdec* d);
// ---- the device side of a merge session (bammerge.hip): a sort, a stream and an output index of its OWN, and the files' id maps ----
struct MergeDev;
// maps: the files' maps back to back (n_maps entries, uploaded once); spill_dir may be null
int  mergedev_create(int device, int64_t max_bytes, int32_t n_ref_merged, const char* spill_dir, int order /* SVX_SORT_* */, const int32_t* maps, int64_t n_maps, MergeDev** out);
void mergedev_destroy(MergeDev* m);
int  mergedev_device(const MergeDev* m);
void mergedev_feed(MergeDev* m, svx_devdec* d, int64_t map_at, int32_t n_ref_file, bool identity);      // devdec_feed_set with the session's sort, stream and map
// ---- a sort with the stream it runs on and the slot its index goes to (sortout.hip): what a reader's own sort and a merge session both end as ----
// The owner makes the sort (devdec_sort_begin, mergedev_create) and appends to it; everything from finish on is written once, here.  finish (header: the
// rewritten header): appending is over, the sorted order and the stream layout stay until drop or the owner's next begin; a failed finish drops the sort.
// drop: the sort's memory goes back (an abort, a failed append).  count / encode / fetch / index / permutation need a finished sort.  encode: SVX_E_IO is a
// spill file that cannot be read - nothing of the sort is of use and it is dropped.  index leaves its bytes where index_bytes / index_fetch read them: for a
// reader that is the decoder's own index slot (devdec_index_bytes / devdec_index_fetch see the same bytes), for a session its own.
SortOut* devdec_sort_out(svx_devdec* d);
SortOut* mergedev_sort_out(MergeDev* m);
int  sortout_finish(SortOut* o, const uint8_t* header, int64_t header_bytes);
void sortout_drop(SortOut* o);
bool sortout_finished(const SortOut* o);
void sortout_count(const SortOut* o, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks);
int  sortout_encode(SortOut* o, int64_t first_block, int64_t n_blocks, int64_t* n_bytes);
int  sortout_fetch(SortOut* o, uint8_t* compressed_dst, uint8_t* stream_dst);
int  sortout_index(SortOut* o, int fmt);
bool sortout_index_bytes(const SortOut* o, int64_t* n_bytes);
int  sortout_index_fetch(SortOut* o, uint8_t* host_dst);
int  sortout_permutation(SortOut* o, uint32_t* host_perm);
void sortout_stats(const SortOut* o, svx_bam_sort_stats* out);
void sortout_spill_stats(const SortOut* o, svx_bam_sort_spill_stats* out);
void sortout_name_stats(const SortOut* o, svx_bam_name_sort_stats* out);      // zeros unless the last finish was in query-name order
void sortout_name_spill_stats(const SortOut* o, svx_bam_name_spill_stats* out);      // zeros unless runs were closed in query-name order
void sortout_translate_stats(const SortOut* o, int64_t* n_chunks, int64_t* n_records, int64_t* n_bytes, double* ms);
