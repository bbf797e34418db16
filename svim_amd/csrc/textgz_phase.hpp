// textgz_phase.hpp - the argument check of the phase-level entries of the BGZF encoder (svx_text_gz_phase in textgz.hip, svx_text_gz_phase_host in
// textgz_host.cpp; include/svx.h).  The entries are test infrastructure: they hand the phases of deflate_core.hpp inputs that svx_text_gz never makes (a
// histogram, a token list, a synthetic DefBlockCodes), so everything a phase indexes with is checked here first, by plain host code, for both builds.
#pragma once
#include "deflate_core.hpp"

#define TGZ_PHASE_MATCH 0
#define TGZ_PHASE_CODES 1
#define TGZ_PHASE_BITS 2
#define TGZ_PHASE_MAXBLOCKS 2048                         /* = TGZ_CHUNK: one launch per phase */
#define TGZ_CODES_WORDS (sizeof(DefBlockCodes) / 4)

// (symbol index within its alphabet, extra bits) of a length 3 .. 258 / a distance 1 .. 32 768 by walking the tables of RFC 1951 section 3.2.5: host code, so it
// cannot call the device functions of deflate_core.hpp in the HIP build
static inline void tgz_len_class(uint32_t len, uint32_t* sym, uint32_t* extra) {
    if (len == 258u) { *sym = 28u; *extra = 0u; return; }
    uint32_t base = 3u;
    for (uint32_t s = 0;; s++) { const uint32_t e = s < 8u ? 0u : (s - 4u) >> 2; if (len < base + (1u << e)) { *sym = s; *extra = e; return; } base += 1u << e; }
}
static inline void tgz_dist_class(uint32_t dist, uint32_t* sym, uint32_t* extra) {
    uint32_t base = 1u;
    for (uint32_t s = 0;; s++) { const uint32_t e = s < 4u ? 0u : (s >> 1) - 1u; if (dist < base + (1u << e)) { *sym = s; *extra = e; return; } base += 1u << e; }
}
// nullptr when the call is in range, else what is wrong.  Layout (b = block): text[text_off[b] .. + n[b]), tok[b * DEF_BLOCK ..), nt[b], hist[b * DEF_NHIST ..),
// codes[b * TGZ_CODES_WORDS ..), slots[b * DEF_SLOT ..)
static inline const char* tgz_phase_check(int phase, int64_t nb, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, const uint32_t* tok,
                                          const uint32_t* nt, const uint32_t* hist, const uint32_t* codes, const uint8_t* slots) {
    if (phase < TGZ_PHASE_MATCH || phase > TGZ_PHASE_BITS) return "phase 0 (match), 1 (codes) or 2 (bits)";
    if (nb < 1 || nb > TGZ_PHASE_MAXBLOCKS || !n) return "1 .. 2048 blocks and their text sizes";
    for (int64_t b = 0; b < nb; b++) if (n[b] > DEF_BLOCK || (phase == TGZ_PHASE_MATCH && n[b] == 0u)) return "a block holds 1 .. 65 280 bytes of text (0: the end-of-file block, phases 1 and 2)";
    if (phase != TGZ_PHASE_CODES) {
        if (!text_off || text_off[0] != 0 || text_off[nb] < 0 || (text_off[nb] && !text)) return "the text and its nb + 1 offsets";
        for (int64_t b = 0; b < nb; b++) if (text_off[b] < 0 || text_off[b] + (int64_t)n[b] > text_off[nb]) return "a block's text lies outside the text";
    }
    if (phase == TGZ_PHASE_MATCH) return tok && nt && hist ? nullptr : "match: tok, nt and hist receive the result";
    if (phase == TGZ_PHASE_CODES) {
        if (!hist || !crc || !codes) return "codes: hist and crc go in, codes receives the result";
        for (int64_t b = 0; b < nb; b++) {
            uint64_t sl = 0, sd = 0;
            for (uint32_t s = 0; s < DEF_NL; s++) sl += hist[b * DEF_NHIST + s];
            for (uint32_t s = 0; s < DEF_ND; s++) sd += hist[b * DEF_NHIST + DEF_NL + s];
            if (sl > DEF_BLOCK + 1u || sd > DEF_BLOCK) return "codes: a histogram counts more tokens than a block has bytes";
        }
        return nullptr;
    }
    if (!tok || !nt || !codes || !slots) return "bits: tok, nt and codes go in, slots receives the result";
    for (int64_t b = 0; b < nb; b++) {
        const DefBlockCodes* bc = reinterpret_cast<const DefBlockCodes*>(codes + b * TGZ_CODES_WORDS);
        if (bc->kind > DEF_KIND_DYNAMIC || bc->n_pre > DEF_MAXPRE || bc->n_suf > 8u || nt[b] > DEF_BLOCK) return "bits: kind, n_pre, n_suf or nt out of range";
        uint64_t bits = 0;
        for (uint32_t i = 0; i < bc->n_pre; i++) { if ((bc->pre[i] >> 24) > 48u) return "bits: an item of more than 48 bits"; bits += bc->pre[i] >> 24; }
        for (uint32_t i = 0; i < bc->n_suf; i++) { if ((bc->suf[i] >> 24) > 48u) return "bits: an item of more than 48 bits"; bits += bc->suf[i] >> 24; }
        if (bc->kind == DEF_KIND_STORED) bits += 8ull * n[b];
        if (bc->kind == DEF_KIND_DYNAMIC) {
            for (uint32_t s = 0; s < DEF_NHIST; s++) if ((bc->code[s] >> 16) > 15u) return "bits: a code of more than 15 bits";
            const uint32_t* t = tok + b * (int64_t)DEF_BLOCK;
            for (uint32_t i = 0; i < nt[b]; i++) {
                if (t[i] & DEF_TOK_MATCH) {
                    if ((t[i] & 511u) > 255u || (t[i] & 0x7f000000u)) return "bits: a match token outside length 3 .. 258, distance 1 .. 32 768";
                    uint32_t ls, le, ds, de;
                    tgz_len_class((t[i] & 511u) + 3u, &ls, &le); tgz_dist_class(((t[i] >> 9) & 0x7fffu) + 1u, &ds, &de);
                    bits += (bc->code[257u + ls] >> 16) + le + (bc->code[DEF_NL + ds] >> 16) + de;
                } else {
                    if (t[i] > 255u) return "bits: a literal token above 255";
                    bits += bc->code[t[i]] >> 16;
                }
            }
        }
        if (bits > 8ull * DEF_SLOT) return "bits: the block does not fit into its slot";
    }
    return nullptr;
}

#ifdef DEF_HOST
#include <memory>
// The host twin of svx_text_gz_phase: the same phase function per block, the lanes one after another.  The scratch of a block lives on the heap for that block
// alone, so a sanitizer build sees an index past DefBitsLds::stage (its last member) or past a block's slot.  Returns nullptr, or what tgz_phase_check says.
static inline const char* tgz_phase_host(int phase, int64_t nb, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, uint32_t* tok, uint32_t* nt,
                                         uint32_t* hist, uint32_t* codes, uint8_t* slots) {
    if (const char* bad = tgz_phase_check(phase, nb, text, text_off, n, crc, tok, nt, hist, codes, slots)) return bad;
    for (int64_t b = 0; b < nb; b++) {
        DefBlockCodes* bc = codes ? reinterpret_cast<DefBlockCodes*>(codes + b * TGZ_CODES_WORDS) : nullptr;
        if (phase == TGZ_PHASE_MATCH) {
            std::unique_ptr<DefMatchLds> L(new DefMatchLds);
            std::unique_ptr<uint32_t[]> t(new uint32_t[n[b]]);
            def_match(text + text_off[b], n[b], t.get(), hist + b * DEF_NHIST, nt + b, *L);
            memset(tok + b * (int64_t)DEF_BLOCK, 0, (size_t)DEF_BLOCK * 4);
            memcpy(tok + b * (int64_t)DEF_BLOCK, t.get(), (size_t)nt[b] * 4);
        } else if (phase == TGZ_PHASE_CODES) {
            std::unique_ptr<DefCodesLds> L(new DefCodesLds);
            memset(bc, 0, sizeof *bc);
            def_codes(hist + b * DEF_NHIST, n[b], crc[b], bc, *L);
        } else {
            std::unique_ptr<DefBitsLds> L(new DefBitsLds);
            std::unique_ptr<uint32_t[]> slot(new uint32_t[DEF_SLOT / 4]());
            def_bits(text ? text + text_off[b] : nullptr, n[b], tok + b * (int64_t)DEF_BLOCK, nt[b], bc, slot.get(), *L);
            memcpy(slots + b * (int64_t)DEF_SLOT, slot.get(), DEF_SLOT);
        }
    }
    return nullptr;
}
#endif
