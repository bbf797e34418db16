// bammerge.hip - the device side of a merge session (svx_bam_merge_*, include/svx.h; the session's host logic: bamio.cpp; what the merged file is:
// svim_amd/bammerge.py).  Replaces: samtools merge in front of the pipeline, for records the device reader has already found.
// A session owns one BamSort, one HIP stream, one output BamIndex and the files' id maps on the device, and nothing else.  Readers FEED the sort (devdec_feed_set:
// their loader thread appends to it, on the SESSION's stream, for the length of one svx_bam_merge_add) and never own any of it; a reader's own sort and index objects are not
// touched from here.  What a session has alone is in this file: making and destroying those four, and the feed.  From finish on the session is a SortOut
// (mergedev_sort_out; sortout.hip), the same object a reader's own sort is.  The one kernel a merge adds, k_bs_translate, is part of the append (bamsort.hip).
#include "common.hpp"
#include "hostcopy.hpp"
#include "devdec.hpp"
#include "bamsort.hpp"

struct MergeDev {
    hipStream_t stream = nullptr;
    BamIndex* index = nullptr;
    DevBuf maps;
    SortOut out;                               // the sort, on `stream`, its index into `index`
};

int mergedev_create(int device, int64_t max_bytes, int32_t n_ref_merged, const char* spill_dir, int order, const int32_t* maps, int64_t n_maps, MergeDev** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return svx_fail(SVX_E_NODEVICE, "svx_bam_merge_open: no such GPU", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(device));
    MergeDev* m = new MergeDev();
    m->out.device = device; m->out.index = &m->index;
    int rc = SVX_OK;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { m->stream = nullptr; rc = svx_fail(SVX_E_HIP, "svx_bam_merge_open: no stream", __FILE__, __LINE__, hipSuccess); }
    m->out.stream = m->stream;
    if (rc == SVX_OK) rc = bamsort_begin(&m->out.sort, max_bytes, n_ref_merged, spill_dir, order);
    m->out.on = rc == SVX_OK;
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
    (void)hipSetDevice(m->out.device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    bamsort_destroy(m->out.sort); m->out.sort = nullptr;
    bamindex_destroy(m->index); m->index = nullptr;
    m->maps.release();
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}
int mergedev_device(const MergeDev* m) { return m->out.device; }
void mergedev_feed(MergeDev* m, svx_devdec* d, int64_t map_at, int32_t n_ref_file, bool identity) {
    devdec_feed_set(d, &m->out, m->maps.as<int32_t>() + map_at, n_ref_file, identity);
}
SortOut* mergedev_sort_out(MergeDev* m) { return &m->out; }
