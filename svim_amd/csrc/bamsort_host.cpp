// bamsort_host.cpp - svx_bam_sort_host and svx_bam_sort_header_host: the coordinate sort of a record stream and the header of the sorted file by the rule of
// bamsort_core.hpp and svim_amd/bamsort.py, built for the host; no GPU involved.  The kernels of bamsort.hip write the same bytes and the same permutation:
// there the keys go through the radix sort and the records through a gather, here through std::stable_sort and memcpy.
#include "bamsort_core.hpp"
#include "../../include/svx.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

static inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

extern "C" int svx_bam_sort_host(const uint8_t* records, int64_t n_bytes, int32_t n_ref, uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records) {
    if (n_bytes < 0 || n_ref < 0 || perm_cap < 0 || (n_bytes && !records) || !n_records) return SVX_E_ARG;
    *n_records = 0;
    struct Row { uint64_t key; int64_t at; uint32_t len; };
    std::vector<Row> rows;
    int bad = 0;
    for (int64_t p = 0; p < n_bytes;) {
        if (n_bytes - p < 4) return SVX_E_ARG;
        const uint32_t bs = rd32(records + p);
        if (bs < BSORT_MIN_BLOCK_SIZE || (int64_t)bs > n_bytes - p - 4) return SVX_E_ARG;          // (nothing behind a record that cannot be walked is a record)
        const int32_t tid = (int32_t)rd32(records + p + 4), pos = (int32_t)rd32(records + p + 8);
        const uint32_t flag = rd32(records + p + 16) >> 16;
        bad |= bsort_check(tid, pos, bs, n_ref);
        rows.push_back(Row{bsort_key(tid, pos, flag, n_ref), p, 4u + bs});
        p += 4 + (int64_t)bs;
    }
    if (bad) return bsort_status(bad);
    if (rows.size() > 0xffffffffull) return SVX_E_CAPACITY;
    *n_records = (int64_t)rows.size();
    if (perm && (int64_t)rows.size() > perm_cap) return SVX_E_CAPACITY;
    std::vector<uint32_t> order(rows.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[a].key < rows[b].key; });
    int64_t at = 0;
    for (size_t k = 0; k < order.size(); k++) {
        const Row& r = rows[order[k]];
        if (out) memcpy(out + at, records + r.at, r.len);
        if (perm) perm[k] = order[k];
        at += r.len;
    }
    return SVX_OK;
}

// header: magic, l_text, text, n_ref, the reference dictionary (the inflated file up to its first record)
extern "C" int svx_bam_sort_header_host(const uint8_t* header, int64_t n_bytes, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (!header || n_bytes < 12 || cap < 0 || (cap && !out) || !n_out || memcmp(header, "BAM\1", 4) != 0) return SVX_E_ARG;
    *n_out = 0;
    const uint32_t l_text = rd32(header + 4);
    if ((int64_t)l_text > n_bytes - 12) return SVX_E_ARG;
    std::string text((const char*)header + 8, l_text);
    const size_t nul = text.find('\0');
    if (nul != std::string::npos) text.resize(nul);
    if (text.compare(0, 4, "@HD\t") == 0) {
        const size_t eol = text.find('\n');
        const std::string line = text.substr(0, eol), tail = eol == std::string::npos ? std::string() : text.substr(eol);
        std::string made = "@HD";
        bool seen = false;
        for (size_t a = 4; a <= line.size();) {                                  // the fields behind "@HD\t" (an empty one between two tabs is a field)
            size_t b = line.find('\t', a);
            if (b == std::string::npos) b = line.size();
            const std::string f = line.substr(a, b - a);
            if (f.compare(0, 3, "GO:") != 0 && f.compare(0, 3, "SS:") != 0) {
                made += '\t';
                if (f.compare(0, 3, "SO:") == 0) { made += "SO:coordinate"; seen = true; } else made += f;
            }
            a = b + 1;
        }
        if (!seen) made += "\tSO:coordinate";
        text = made + tail;
    } else text = "@HD\tVN:1.6\tSO:coordinate\n" + text;
    const int64_t rest = n_bytes - 8 - (int64_t)l_text, total = 8 + (int64_t)text.size() + rest;
    *n_out = total;
    if (total > cap) return SVX_E_CAPACITY;
    memcpy(out, "BAM\1", 4);
    wr32(out + 4, (uint32_t)text.size());
    memcpy(out + 8, text.data(), text.size());
    memcpy(out + 8 + text.size(), header + 8 + l_text, (size_t)rest);
    return SVX_OK;
}
