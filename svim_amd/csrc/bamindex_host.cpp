// bamindex_host.cpp - svx_bam_index_host: the .bai of one file from its row table by the interval and order rules of bamindex_core.hpp, built for the host; no
// GPU involved.  The checks, the references, their empty parts and the trailer are made here; the part of a reference with rows is written by
// binidx_host.hpp.  The kernels of bamindex.hip write the same bytes for the same rows; here the references, chunks and windows are walked one row after
// the other, there they come from bisections, scans and a sort.
#include "bamindex_core.hpp"
#include "binidx_host.hpp"
#include "../../include/svx.h"
#include <cstring>
#include <vector>

// csi: the .csi of the same rows (svim_amd/csi.py) - a depth from the largest end, no range to refuse
static int bam_index_host(bool csi, int32_t n_ref, int64_t n_rows, const int32_t* tid, const int32_t* pos, const int64_t* end, const uint16_t* flag, const uint64_t* vbeg,
                          uint64_t v_end, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (n_ref < 0 || n_rows < 0 || cap < 0 || (cap && !out) || !n_out || (n_rows && (!tid || !pos || !end || !flag || !vbeg))) return SVX_E_ARG;
    *n_out = 0;
    for (int64_t k = 0; k < n_rows; k++) if (tid[k] >= n_ref) return SVX_E_ARG;
    // the order and the range
    bool bad_order = false, bad_range = false;
    int64_t max_end = 0;
    int64_t n_placed = n_rows;                                 // (in order: the placed rows are a prefix)
    for (int64_t k = 0; k < n_rows; k++) {
        if (k && bix_out_of_order(tid[k - 1], pos[k - 1], tid[k], pos[k])) bad_order = true;
        if (tid[k] >= 0) max_end = std::max(max_end, bix_interval(pos[k], end[k]).end);
        if (tid[k] < 0 && n_placed == n_rows) n_placed = k;
    }
    if (bad_order) return SVX_E_ORDER;
    bad_range = !csi && max_end > BINIDX_MAX_END;
    if (bad_range) return SVX_E_RANGE;
    const int depth = binidx_depth_for(max_end);
    std::vector<uint8_t> blob((size_t)(csi ? BIX_CSI_HEADER_BYTES : BIX_HEADER_BYTES));
    if (csi) {
        memcpy(blob.data(), "CSI\1", 4);
        binidx_put32(blob.data() + 4, BINIDX_CSI_MIN_SHIFT); binidx_put32(blob.data() + 8, (uint32_t)depth); binidx_put32(blob.data() + 12, 0u); binidx_put32(blob.data() + 16, (uint32_t)n_ref);
    } else {
        memcpy(blob.data(), "BAI\1", 4);
        binidx_put32(blob.data() + 4, (uint32_t)n_ref);
    }
    int64_t lo = 0;
    for (int32_t t = 0; t < n_ref; t++) {
        int64_t hi = lo;
        while (hi < n_placed && tid[hi] == t) hi++;
        if (hi == lo) { blob.resize(blob.size() + (csi ? BINIDX_CSI_EMPTY_PART_BYTES : BINIDX_EMPTY_PART_BYTES), 0); continue; }
        std::vector<BinIdxRow> rows;
        uint64_t n_unmapped = 0;
        for (int64_t j = lo; j < hi; j++) {
            const BinIdxInterval v = bix_interval(pos[j], end[j]);
            rows.push_back(BinIdxRow{v.beg, v.end, vbeg[j], j + 1 < n_rows ? vbeg[j + 1] : v_end});
            n_unmapped += (flag[j] & 4u) ? 1u : 0u;
        }
        if (csi) binidx_append_part_csi(blob, rows.data(), rows.size(), (uint64_t)(hi - lo) - n_unmapped, n_unmapped, depth);
        else binidx_append_part(blob, rows.data(), rows.size(), (uint64_t)(hi - lo) - n_unmapped, n_unmapped);
        lo = hi;
    }
    const size_t at = blob.size();
    blob.resize(at + 8);
    binidx_put64(blob.data() + at, (uint64_t)(n_rows - n_placed));
    *n_out = (int64_t)blob.size();
    if ((int64_t)blob.size() > cap) return SVX_E_CAPACITY;
    memcpy(out, blob.data(), blob.size());
    return SVX_OK;
}

extern "C" int svx_bam_index_host(int32_t n_ref, int64_t n_rows, const int32_t* tid, const int32_t* pos, const int64_t* end, const uint16_t* flag, const uint64_t* vbeg,
                                  uint64_t v_end, uint8_t* out, int64_t cap, int64_t* n_out) {
    return bam_index_host(false, n_ref, n_rows, tid, pos, end, flag, vbeg, v_end, out, cap, n_out);
}
extern "C" int svx_bam_index_csi_host(int32_t n_ref, int64_t n_rows, const int32_t* tid, const int32_t* pos, const int64_t* end, const uint16_t* flag, const uint64_t* vbeg,
                                      uint64_t v_end, uint8_t* out, int64_t cap, int64_t* n_out) {
    return bam_index_host(true, n_ref, n_rows, tid, pos, end, flag, vbeg, v_end, out, cap, n_out);
}
