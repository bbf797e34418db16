// bammerge.hip - the device side of a merge session (svx_bam_merge_*, include/svx.h; the session's host logic: bamio.cpp; what the merged file is:
// svim_amd/bammerge.py).  Replaces: samtools merge in front of the pipeline, for records the device reader has already found.
// A session owns one BamSort, one HIP stream, one output BamIndex and the files' id maps on the device, and nothing else.  Readers FEED the sort (devdec_feed_set:
// their loader thread appends to it, on the SESSION's stream, for the length of one svx_bam_merge_add) and never own any of it; a reader's own sort and index objects are not
// touched from here.  No sort, gather, encoder or index code lives in this file: every function is bamsort_* / bamindex_* with the session's stream.  The one
// kernel a merge adds, k_bs_translate, is part of the append (bamsort.hip).
#include "common.hpp"
#include "hostcopy.hpp"
#include "devdec.hpp"
#include "bamsort.hpp"

struct MergeDev {
    int device = 0;
    hipStream_t stream = nullptr;
    BamSort* sort = nullptr;
    BamIndex* index = nullptr;
    DevBuf maps;
};

int mergedev_create(int device, int64_t max_bytes, int32_t n_ref_merged, const char* spill_dir, const int32_t* maps, int64_t n_maps, MergeDev** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return svx_fail(SVX_E_NODEVICE, "svx_bam_merge_open: no such GPU", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(device));
    MergeDev* m = new MergeDev();
    m->device = device;
    int rc = SVX_OK;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { m->stream = nullptr; rc = svx_fail(SVX_E_HIP, "svx_bam_merge_open: no stream", __FILE__, __LINE__, hipSuccess); }
    if (rc == SVX_OK) rc = bamsort_begin(&m->sort, max_bytes, n_ref_merged, spill_dir);
    if (rc == SVX_OK) rc = bamindex_begin(&m->index);
    if (rc == SVX_OK) rc = m->maps.reserve((size_t)(n_maps > 0 ? n_maps : 1) * 4);
    if (rc == SVX_OK && n_maps > 0) rc = svx_h2d(m->maps.p, maps, (size_t)n_maps * 4, m->stream);
    if (rc == SVX_OK && hipStreamSynchronize(m->stream) != hipSuccess) rc = svx_fail(SVX_E_HIP, "svx_bam_merge_open: the maps did not reach the device", __FILE__, __LINE__, hipSuccess);
    if (rc != SVX_OK) { mergedev_destroy(m); return rc; }
    *out = m;
    return SVX_OK;
}
void mergedev_destroy(MergeDev* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    bamsort_destroy(m->sort); m->sort = nullptr;
    bamindex_destroy(m->index); m->index = nullptr;
    m->maps.release();
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}
int mergedev_device(const MergeDev* m) { return m->device; }
void mergedev_feed(MergeDev* m, svx_devdec* d, int64_t map_at, int32_t n_ref_file, bool identity) {
    devdec_feed_set(d, m->sort, (void*)m->stream, m->maps.as<int32_t>() + map_at, n_ref_file, identity);
}
void mergedev_drop(MergeDev* m) {
    (void)hipSetDevice(m->device);
    bamsort_drop(m->sort);
}
int mergedev_finish(MergeDev* m, const uint8_t* header, int64_t header_bytes) {
    HIPCHK(hipSetDevice(m->device));
    const int rc = bamsort_finish(m->sort, header, header_bytes, m->stream);
    if (rc != SVX_OK) bamsort_drop(m->sort);
    return rc;
}
void mergedev_count(const MergeDev* m, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks) { bamsort_count(m->sort, n_records, stream_bytes, n_blocks); }
int mergedev_encode(MergeDev* m, int64_t first_block, int64_t n_blocks, int64_t* n_bytes) {
    HIPCHK(hipSetDevice(m->device));
    return bamsort_encode(m->sort, first_block, n_blocks, n_bytes, m->stream);
}
int mergedev_fetch(MergeDev* m, uint8_t* compressed_dst, uint8_t* stream_dst) {
    HIPCHK(hipSetDevice(m->device));
    return bamsort_fetch(m->sort, compressed_dst, stream_dst, m->stream);
}
int mergedev_index(MergeDev* m, int fmt) {
    HIPCHK(hipSetDevice(m->device));
    SVXCHK(bamindex_begin(&m->index));
    const int rc = bamsort_index(m->sort, m->index, m->stream, fmt);
    bamindex_drop(m->index);                                // (the table's memory goes back; the bytes of a finished index stay)
    return rc;
}
bool mergedev_index_bytes(const MergeDev* m, int64_t* n_bytes) { return bamindex_bytes(m->index, n_bytes); }
int mergedev_index_fetch(MergeDev* m, uint8_t* host_dst) {
    HIPCHK(hipSetDevice(m->device));
    return bamindex_fetch(m->index, host_dst, m->stream);
}
int mergedev_permutation(MergeDev* m, uint32_t* host_perm) {
    HIPCHK(hipSetDevice(m->device));
    return bamsort_permutation(m->sort, host_perm, m->stream);
}
void mergedev_stats(const MergeDev* m, svx_bam_sort_stats* out, svx_bam_sort_spill_stats* spill, int64_t* tr_chunks, int64_t* tr_records, int64_t* tr_bytes, double* tr_ms) {
    bamsort_stats(m->sort, out);
    bamsort_spill_stats(m->sort, spill);
    bamsort_translate_stats(m->sort, tr_chunks, tr_records, tr_bytes, tr_ms);
}
