// textindex_core.hpp - what a tabix index says about one line of a VCF or BED text: the line parser and the virtual offset of a text offset, one source for
// the kernels of textindex.hip and for svx_text_index_host (textindex_host.cpp), as deflate_core.hpp is for the encoder.  The bins and the layout of a
// contig's part: binidx_core.hpp.  The definition in words: svim_amd/tabix.py.
#pragma once
#include "binidx_core.hpp"

#define TIX_HEAD 65280                       /* bytes of a line that are parsed (one BGZF block of text) */
#define TIX_NUM_CAP (1ll << 40)
#define TIX_HEADER_BYTES 36                  /* magic + eight int32, in front of the names */
#define TIX_CSI_HEADER_BYTES 48              /* a .csi: magic, min_shift, depth, l_aux, then aux = seven int32 of the .tbi header and the names, then n_ref */

struct TixLine { int32_t skip, name_len; int64_t beg, end; };

// leading decimal digits at p (none: 0), capped; *used = how many
BINIDX_HD int64_t tix_num(const uint8_t* p, const uint8_t* e, int* used) {
    int64_t v = 0; int k = 0;
    while (p + k < e && p[k] >= '0' && p[k] <= '9') { v = v * 10 + (p[k] - '0'); if (v > TIX_NUM_CAP) v = TIX_NUM_CAP; k++; }
    if (used) *used = k;
    return v;
}
// one column: x at its first byte while `more` says the line has it (an absent column is empty) -> [*b, *e); x and more move on to the next one.
// A column ends at a tab, at the line's newline or at lim
BINIDX_HD void tix_col(const uint8_t*& x, const uint8_t* lim, bool& more, const uint8_t** b, const uint8_t** e) {
    if (!more) { *b = *e = lim; return; }
    *b = x;
    while (x < lim && *x != '\t' && *x != '\n') x++;
    *e = x;
    more = x < lim && *x == '\t';
    if (more) x++;
}
// the line text[s, e) (e: the next line's start, or the text's end); only its first TIX_HEAD bytes are read
BINIDX_HD TixLine tix_parse_line(const uint8_t* text, int64_t s, int64_t e, int preset) {
    TixLine r; r.skip = 1; r.name_len = 0; r.beg = 0; r.end = 0;
    if (e <= s || text[s] == '#' || text[s] == '\n') return r;
    r.skip = 0;
    const uint8_t* x = text + s;
    const uint8_t* lim = text + (e - s > TIX_HEAD ? s + TIX_HEAD : e);
    const uint8_t *cb, *ce; bool more = true;
    tix_col(x, lim, more, &cb, &ce); r.name_len = (int32_t)(ce - cb);
    tix_col(x, lim, more, &cb, &ce);
    const int64_t v2 = tix_num(cb, ce, nullptr);
    if (preset == 1) {
        tix_col(x, lim, more, &cb, &ce);
        r.beg = v2; r.end = tix_num(cb, ce, nullptr);
    } else {
        r.beg = v2 > 0 ? v2 - 1 : 0;
        tix_col(x, lim, more, &cb, &ce);                                  // ID
        tix_col(x, lim, more, &cb, &ce); r.end = r.beg + (int64_t)(ce - cb);   // REF
        for (int k = 0; k < 3; k++) tix_col(x, lim, more, &cb, &ce);      // ALT, QUAL, FILTER
        // INFO: the first item that starts with END= (the items are not walked to their end: a READS= list can be most of the line)
        if (more) {
            bool at_item = true;
            for (; x < lim && *x != '\t' && *x != '\n'; x++) {
                if (at_item && lim - x >= 4 && x[0] == 'E' && x[1] == 'N' && x[2] == 'D' && x[3] == '=') {
                    const int64_t v = tix_num(x + 4, lim, nullptr);
                    if (v > r.beg) r.end = v;
                    break;
                }
                at_item = *x == ';';
            }
        }
    }
    if (r.end <= r.beg) r.end = r.beg + 1;
    return r;
}
// virtual offset of text offset u: the last block of [b_lo, b_hi) that starts at or before u (uoff[b_lo] <= u is required); coff_base: where the file's
// stream starts in coff's numbering, stream_base: what lies in front of it in the file
BINIDX_HD uint64_t tix_voff(int64_t u, const int64_t* coff, const int64_t* uoff, int64_t b_lo, int64_t b_hi, int64_t coff_base, int64_t stream_base) {
    int64_t lo = b_lo, hi = b_hi;                     // first block with uoff > u
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (uoff[mid] > u) hi = mid; else lo = mid + 1; }
    const int64_t b = lo - 1;
    return ((uint64_t)(stream_base + coff[b] - coff_base) << 16) | (uint64_t)(u - uoff[b]);
}
