// sortout.hip - a finished sort on the device, written once for its two owners (devdec.hpp: sortout_*): a reader's decoder, whose own sort runs on the loader's
// stream and indexes into the decoder's index slot (bamdev.hip), and a merge session, which brings a stream and an index of its own (bammerge.hip).  No sort,
// gather, encoder or index code lives in this file: every function is bamsort_* / bamindex_* with the owner's device, stream and slot.
#include "common.hpp"
#include "devdec.hpp"
#include "bamsort.hpp"

void sortout_drop(SortOut* o) {
    (void)hipSetDevice(o->device);
    o->on = false;
    bamsort_drop(o->sort);
}
int sortout_finish(SortOut* o, const uint8_t* header, int64_t header_bytes) {
    HIPCHK(hipSetDevice(o->device));
    o->on = false;
    const int rc = bamsort_finish(o->sort, header, header_bytes, o->stream);
    if (rc != SVX_OK) bamsort_drop(o->sort);
    return rc;
}
bool sortout_finished(const SortOut* o) { return bamsort_finished(o->sort); }
void sortout_count(const SortOut* o, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks) { bamsort_count(o->sort, n_records, stream_bytes, n_blocks); }
int sortout_encode(SortOut* o, int64_t first_block, int64_t n_blocks, int64_t* n_bytes) {
    HIPCHK(hipSetDevice(o->device));
    const int rc = bamsort_encode(o->sort, first_block, n_blocks, n_bytes, o->stream);
    if (rc == SVX_E_IO) bamsort_drop(o->sort);              // (the spill file cannot be read: nothing of the sort is of use)
    return rc;
}
int sortout_fetch(SortOut* o, uint8_t* compressed_dst, uint8_t* stream_dst) {
    HIPCHK(hipSetDevice(o->device));
    return bamsort_fetch(o->sort, compressed_dst, stream_dst, o->stream);
}
int sortout_index(SortOut* o, int fmt) {
    HIPCHK(hipSetDevice(o->device));
    SVXCHK(bamindex_begin(o->index));
    const int rc = bamsort_index(o->sort, *o->index, o->stream, fmt);
    bamindex_drop(*o->index);                               // (the table's memory goes back; the bytes of a finished index stay)
    return rc;
}
bool sortout_index_bytes(const SortOut* o, int64_t* n_bytes) { return bamindex_bytes(*o->index, n_bytes); }
int sortout_index_fetch(SortOut* o, uint8_t* host_dst) {
    HIPCHK(hipSetDevice(o->device));
    return bamindex_fetch(*o->index, host_dst, o->stream);
}
int sortout_permutation(SortOut* o, uint32_t* host_perm) {
    HIPCHK(hipSetDevice(o->device));
    return bamsort_permutation(o->sort, host_perm, o->stream);
}
void sortout_stats(const SortOut* o, svx_bam_sort_stats* out) { bamsort_stats(o->sort, out); }
void sortout_spill_stats(const SortOut* o, svx_bam_sort_spill_stats* out) { bamsort_spill_stats(o->sort, out); }
void sortout_name_stats(const SortOut* o, svx_bam_name_sort_stats* out) { bamsort_name_stats(o->sort, out); }
void sortout_name_spill_stats(const SortOut* o, svx_bam_name_spill_stats* out) { bamsort_name_spill_stats(o->sort, out); }
void sortout_translate_stats(const SortOut* o, int64_t* n_chunks, int64_t* n_records, int64_t* n_bytes, double* ms) { bamsort_translate_stats(o->sort, n_chunks, n_records, n_bytes, ms); }
