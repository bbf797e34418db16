// binidx_host.hpp - the part of one group (a contig of a .tbi, a reference of a .bai) written on the host, row after row: what svx_text_index_host and
// svx_bam_index_host are built from and what the kernels of binidx_kernels.hpp are held against.  It shares binidx_core.hpp with them and nothing else:
// no scan, no sort of theirs, no table - chunks, bins and windows are walked one row after the other.
#pragma once
#include "binidx_core.hpp"
#include <algorithm>
#include <vector>

struct BinIdxRow { int64_t beg, end; uint64_t vbeg, vend; };      // one row of a group, in file order: its interval, where it starts and where it ends

// appends the part of a group of n > 0 rows to blob: n_bin, the bins ascending with their chunks in file order, the pseudo-bin, n_intv, the linear index
inline void binidx_append_part(std::vector<uint8_t>& blob, const BinIdxRow* rows, size_t n, uint64_t n_mapped, uint64_t n_unmapped) {
    struct Chunk { uint32_t bin; uint64_t beg, end; };
    std::vector<Chunk> chunks;
    int64_t max_end = 0;
    for (size_t j = 0; j < n; j++) {
        const uint32_t bin = binidx_bin(BinIdxInterval{rows[j].beg, rows[j].end});
        if (j > 0 && bin == chunks.back().bin) chunks.back().end = rows[j].vend; else chunks.push_back(Chunk{bin, rows[j].vbeg, rows[j].vend});
        max_end = std::max(max_end, rows[j].end);
    }
    std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk& a, const Chunk& b) { return a.bin < b.bin; });
    int64_t n_bins = 0;
    for (size_t k = 0; k < chunks.size(); k++) n_bins += k == 0 || chunks[k].bin != chunks[k - 1].bin;
    const int64_t n_intv = 1 + ((max_end - 1) >> 14);
    const size_t at = blob.size();
    blob.resize(at + (size_t)binidx_part_bytes(n_bins, (int64_t)chunks.size(), n_intv));
    uint8_t* p = blob.data() + at;
    binidx_put32(p, (uint32_t)(n_bins + 1)); p += 4;
    for (size_t k = 0; k < chunks.size();) {
        size_t m = k;
        while (m < chunks.size() && chunks[m].bin == chunks[k].bin) m++;
        binidx_put32(p, chunks[k].bin); binidx_put32(p + 4, (uint32_t)(m - k)); p += 8;
        for (; k < m; k++) { binidx_put64(p, chunks[k].beg); binidx_put64(p + 8, chunks[k].end); p += 16; }
    }
    binidx_put32(p, BINIDX_PSEUDO_BIN); binidx_put32(p + 4, 2u); binidx_put64(p + 8, rows[0].vbeg); binidx_put64(p + 16, rows[n - 1].vend);
    binidx_put64(p + 24, n_mapped); binidx_put64(p + 32, n_unmapped); p += 40;
    binidx_put32(p, (uint32_t)n_intv); p += 4;
    std::vector<uint64_t> lin((size_t)n_intv, BINIDX_NO_SLOT);
    for (size_t j = 0; j < n; j++)
        for (int64_t w = rows[j].beg >> 14; w <= (rows[j].end - 1) >> 14; w++) lin[(size_t)w] = std::min(lin[(size_t)w], rows[j].vbeg);
    for (int64_t w = n_intv - 2; w >= 0; w--) if (lin[(size_t)w] == BINIDX_NO_SLOT) lin[(size_t)w] = lin[(size_t)w + 1];
    for (int64_t w = 0; w < n_intv; w++) binidx_put64(p + 8 * w, lin[(size_t)w]);
}

// the CSI form of the same part (binidx_core.hpp; svim_amd/csi.py): the bins at `depth`, each with the loffset that the filled linear index would hold at
// the bin's first window - the vbeg of the first row whose running maximum of ends lies beyond the bin's start - and no linear index
inline void binidx_append_part_csi(std::vector<uint8_t>& blob, const BinIdxRow* rows, size_t n, uint64_t n_mapped, uint64_t n_unmapped, int depth) {
    struct Chunk { uint32_t bin; uint64_t beg, end; };
    std::vector<Chunk> chunks;
    std::vector<int64_t> run_max(n);
    for (size_t j = 0; j < n; j++) {
        const uint32_t bin = binidx_reg2bin_csi(rows[j].beg, rows[j].end, depth);
        if (j > 0 && bin == chunks.back().bin) chunks.back().end = rows[j].vend; else chunks.push_back(Chunk{bin, rows[j].vbeg, rows[j].vend});
        run_max[j] = j > 0 ? std::max(run_max[j - 1], rows[j].end) : rows[j].end;
    }
    std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk& a, const Chunk& b) { return a.bin < b.bin; });
    int64_t n_bins = 0;
    for (size_t k = 0; k < chunks.size(); k++) n_bins += k == 0 || chunks[k].bin != chunks[k - 1].bin;
    const size_t at = blob.size();
    blob.resize(at + (size_t)binidx_csi_part_bytes(n_bins, (int64_t)chunks.size()));
    uint8_t* p = blob.data() + at;
    binidx_put32(p, (uint32_t)(n_bins + 1)); p += 4;
    for (size_t k = 0; k < chunks.size();) {
        size_t m = k;
        while (m < chunks.size() && chunks[m].bin == chunks[k].bin) m++;
        const size_t j = (size_t)(std::upper_bound(run_max.begin(), run_max.end(), binidx_bin_start(chunks[k].bin, depth)) - run_max.begin());
        binidx_put32(p, chunks[k].bin); binidx_put64(p + 4, j < n ? rows[j].vbeg : 0ull); binidx_put32(p + 12, (uint32_t)(m - k)); p += 16;
        for (; k < m; k++) { binidx_put64(p, chunks[k].beg); binidx_put64(p + 8, chunks[k].end); p += 16; }
    }
    binidx_put32(p, binidx_csi_pseudo_bin(depth)); binidx_put64(p + 4, 0ull); binidx_put32(p + 12, 2u);
    binidx_put64(p + 16, rows[0].vbeg); binidx_put64(p + 24, rows[n - 1].vend); binidx_put64(p + 32, n_mapped); binidx_put64(p + 40, n_unmapped);
}
