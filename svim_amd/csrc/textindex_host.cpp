// textindex_host.cpp - svx_text_index_host: the tabix index of one file by the line parser of textindex_core.hpp, built for the host; no GPU involved.  Lines,
// records, contig runs, names and the header are made here; a contig's part is written by binidx_host.hpp.  The kernels of textindex.hip write the same
// bytes for the same text and block table; here the runs, chunks and windows are walked one record after the other, there they come from scans and a sort.
#include "textindex_core.hpp"
#include "binidx_host.hpp"
#include "../../include/svx.h"
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace {
struct Rec { int64_t at, beg, end; int32_t name_len; uint64_t vbeg, vend; };
}

// csi: the .csi of the same text (svim_amd/csi.py) - a depth from the largest end, no range to refuse
static int text_index_host(bool csi, const uint8_t* text, int64_t n, const int64_t* block_coff, const int64_t* block_uoff, int64_t n_blocks, int preset, int64_t stream_base,
                           uint8_t* out, int64_t cap, int64_t* n_out) {
    if (n < 0 || cap < 0 || (n && !text) || (cap && !out) || !n_out || !block_coff || !block_uoff || n_blocks < 1 || (preset != SVX_INDEX_VCF && preset != SVX_INDEX_BED) ||
        stream_base < 0 || block_uoff[0] != 0 || block_uoff[n_blocks - 1] != n)
        return SVX_E_ARG;
    for (int64_t b = 0; b + 1 < n_blocks; b++) if (block_uoff[b + 1] < block_uoff[b] || block_uoff[b + 1] - block_uoff[b] > 65536) return SVX_E_ARG;
    *n_out = 0;
    // lines, records
    std::vector<int64_t> starts;
    for (int64_t at = 0; at < n;) {
        starts.push_back(at);
        const void* nl = memchr(text + at, '\n', (size_t)(n - at));
        at = nl ? (int64_t)((const uint8_t*)nl - text) + 1 : n;
    }
    const uint64_t v_eof = (uint64_t)(stream_base + block_coff[n_blocks - 1]) << 16;
    std::vector<Rec> recs;
    for (size_t k = 0; k < starts.size(); k++) {
        const int64_t s = starts[k], e = k + 1 < starts.size() ? starts[k + 1] : n;
        const TixLine L = tix_parse_line(text, s, e, preset);
        if (L.skip) continue;
        Rec r; r.at = s; r.beg = L.beg; r.end = L.end; r.name_len = L.name_len;
        r.vbeg = tix_voff(s, block_coff, block_uoff, 0, n_blocks, 0, stream_base);
        r.vend = k + 1 < starts.size() ? tix_voff(e, block_coff, block_uoff, 0, n_blocks, 0, stream_base) : v_eof;
        recs.push_back(r);
    }
    // contig runs, the order and the range
    std::vector<size_t> run_first;
    std::unordered_set<std::string> seen;
    bool bad_order = false, bad_range = false;
    int64_t max_end = 0;
    for (size_t j = 0; j < recs.size(); j++) {
        const Rec& r = recs[j];
        const bool head = j == 0 || r.name_len != recs[j - 1].name_len || memcmp(text + r.at, text + recs[j - 1].at, (size_t)r.name_len) != 0;
        if (head) {
            if (!seen.insert(std::string((const char*)text + r.at, (size_t)r.name_len)).second) bad_order = true;
            run_first.push_back(j);
        } else if (r.beg < recs[j - 1].beg) bad_order = true;
        max_end = std::max(max_end, r.end);
    }
    if (bad_order) return SVX_E_ORDER;
    bad_range = !csi && max_end > BINIDX_MAX_END;
    if (bad_range) return SVX_E_RANGE;
    const int depth = binidx_depth_for(max_end);
    const size_t n_ref = run_first.size();
    run_first.push_back(recs.size());
    std::vector<uint8_t> blob((size_t)(csi ? TIX_CSI_HEADER_BYTES - 4 : TIX_HEADER_BYTES));     // (a .csi has n_ref behind the names)
    int64_t l_nm = 0;
    for (size_t t = 0; t < n_ref; t++) {
        const Rec& r = recs[run_first[t]];
        blob.insert(blob.end(), text + r.at, text + r.at + r.name_len); blob.push_back(0);
        l_nm += r.name_len + 1;
    }
    const uint32_t head[8] = {(uint32_t)n_ref, preset == SVX_INDEX_BED ? 0x10000u : 2u, 1u, 2u, preset == SVX_INDEX_BED ? 3u : 0u, (uint32_t)'#', 0u, (uint32_t)l_nm};
    if (csi) {
        memcpy(blob.data(), "CSI\1", 4);
        binidx_put32(blob.data() + 4, BINIDX_CSI_MIN_SHIFT); binidx_put32(blob.data() + 8, (uint32_t)depth); binidx_put32(blob.data() + 12, (uint32_t)(28 + l_nm));
        for (int k = 1; k < 8; k++) binidx_put32(blob.data() + 12 + 4 * k, head[k]);
        blob.resize(blob.size() + 4);
        binidx_put32(blob.data() + blob.size() - 4, (uint32_t)n_ref);
    } else {
        memcpy(blob.data(), "TBI\1", 4);
        for (int k = 0; k < 8; k++) binidx_put32(blob.data() + 4 + 4 * k, head[k]);
    }
    for (size_t t = 0; t < n_ref; t++) {
        const size_t lo = run_first[t], hi = run_first[t + 1];
        std::vector<BinIdxRow> rows;
        for (size_t j = lo; j < hi; j++) rows.push_back(BinIdxRow{recs[j].beg, recs[j].end, recs[j].vbeg, recs[j].vend});
        if (csi) binidx_append_part_csi(blob, rows.data(), rows.size(), (uint64_t)(hi - lo), 0ull, depth);
        else binidx_append_part(blob, rows.data(), rows.size(), (uint64_t)(hi - lo), 0ull);
    }
    blob.resize(blob.size() + 8, 0);
    *n_out = (int64_t)blob.size();
    if ((int64_t)blob.size() > cap) return SVX_E_CAPACITY;
    memcpy(out, blob.data(), blob.size());
    return SVX_OK;
}

extern "C" int svx_text_index_host(const uint8_t* text, int64_t n, const int64_t* block_coff, const int64_t* block_uoff, int64_t n_blocks, int preset, int64_t stream_base,
                                   uint8_t* out, int64_t cap, int64_t* n_out) {
    return text_index_host(false, text, n, block_coff, block_uoff, n_blocks, preset, stream_base, out, cap, n_out);
}
extern "C" int svx_text_index_csi_host(const uint8_t* text, int64_t n, const int64_t* block_coff, const int64_t* block_uoff, int64_t n_blocks, int preset, int64_t stream_base,
                                       uint8_t* out, int64_t cap, int64_t* n_out) {
    return text_index_host(true, text, n, block_coff, block_uoff, n_blocks, preset, stream_base, out, cap, n_out);
}
