// deflate_core.hpp - raw DEFLATE (RFC 1951) ENCODER for one BGZF block (at most 65 280 bytes of text), written for a 64-lane wavefront (one wave per
// block, textgz.hip) and, with the lane operations emulated (DEF_HOST), for the host (textgz_host.cpp: svx_text_gz_host; tools/text_gz_host_test.cpp).
// The two builds produce the same bytes for the same input: everything is integer arithmetic, and where lanes meet in memory they meet through operations
// whose result does not depend on their order (maximum, sum, bitwise or) behind a barrier that separates them from every read.
// Replaces: bgzip / zlib's deflate() after the text has left the device (the reference writes plain text; its users compress it afterwards).
//
// Three phases per block, one function each (three kernels: their times are reported apart):
//   def_match  LZ77 within the block.  A batch is 64 consecutive positions, lane l at position base + l.  Every lane hashes its next four bytes, reads
//              the most recent EARLIER-batch position with that hash from a table in LDS (one probe) and extends it (4 bytes per step, 4..258); a second
//              candidate is the position at the distance of the block's last match (lines repeat their neighbours at a fixed distance).  Only then the
//              batch's own positions enter the table (maximum of position + 1: order-independent).  The parse is greedy and serial, but it runs on the
//              64-bit mask of lanes that have a match: literals between two matches are skipped with one count-trailing-zeros, so a step of the chain
//              is a match, not a byte.  Tokens go to global memory by rank in the mask, the histograms are LDS adds.
//              What it cannot see: a repeat whose only earlier occurrence lies inside the same batch (distance < 64 from a position of the batch), apart
//              from the last-distance candidate; a position whose table entry was overwritten by a later one with the same hash; lazy evaluation.
//   def_codes  Dynamic Huffman codes: symbols ranked by (count, symbol) by all lanes, then lane 0 alone: two-queue merge, depths, the length limit (15 / 7 bits)
//              by moving codes between lengths until the Kraft sum is exact (the rule of miniz's tdefl_huffman_enforce_max_code_size, public domain; any complete
//              set is legal), canonical codes, the run-length form of the code lengths (16 / 17 / 18), the code-length code, the exact size in bits.  An alphabet
//              with fewer than two used symbols gets two codes of one bit (what zlib's compressor does: a complete set in every case).
//              A block whose coded form would not be smaller than its bytes becomes a stored block.
//   def_bits   Everything the block consists of is an ITEM (value, number of bits <= 48): the BGZF header, the block header, the tokens, the end-of-block code, the
//              padding, CRC32 and ISIZE.  A batch of 64 items: exclusive scan of the bit counts, every lane ors its item into a staging window in LDS
//              (atomic or: no read-modify-write race, order-independent), complete words leave as aligned 4-byte stores to the block's slot.
// Format facts after RFC 1951 / RFC 1952 / the SAM specification section 4.1 (BGZF); nothing is taken from another implementation beyond the rule named above.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#define DEF_BLOCK 65280u           /* text bytes per BGZF block (what bgzip uses: a stored block of it still fits 64 KiB) */
#define DEF_SLOT 65536u            /* bytes of the slot a block is coded into */
#define DEF_HBITS 12
#define DEF_HSIZE (1u << DEF_HBITS)
#define DEF_MINLEN 4u
#define DEF_MAXLEN 258u
#define DEF_MAXDIST 32768u
#define DEF_NL 288                 /* literal/length symbols incl. the two that never occur */
#define DEF_ND 32
#define DEF_NHIST (DEF_NL + DEF_ND)
#define DEF_MAXPRE 360             /* items in front of the tokens: 9 header + 2 + 19 + at most 316 code lengths */
#define DEF_STAGE 112              /* words of the staging window: 64 items of 48 bits + the carried word + the spill of the last item */
#define DEF_KIND_EOF 0
#define DEF_KIND_STORED 1
#define DEF_KIND_DYNAMIC 2
#define DEF_TOK_MATCH 0x80000000u  /* token: literal byte, or MATCH | (distance - 1) << 9 | (length - 3) */

// per-wave scratch of the phases (LDS on the device)
struct DefMatchLds { uint32_t head[DEF_HSIZE]; uint32_t hist[DEF_NHIST]; };
struct DefCodesLds {
    uint32_t freq[DEF_NL]; uint32_t nfreq[DEF_NL];
    uint16_t sorted[DEF_NL], lpar[DEF_NL], npar[DEF_NL], ndepth[DEF_NL];
    uint16_t cl[DEF_NL + DEF_ND + 4];         // code-length sequence in run-length form: symbol | extra value << 5
    uint8_t len[DEF_NL + DEF_ND], clen[20];
    uint32_t ccode[20];
    uint32_t hist[DEF_NHIST];
    uint32_t cnt[40];
};
struct DefBitsLds { uint32_t code[DEF_NHIST]; uint32_t stage[DEF_STAGE]; };
// what def_codes leaves for def_bits, per block (global memory)
struct DefBlockCodes {
    uint32_t code[DEF_NHIST];        // Huffman code, bit-reversed (it is sent from its most significant bit) | length << 16; distance codes from DEF_NL on
    uint32_t pre[DEF_MAXPRE];        // items: value | bits << 24
    uint32_t suf[8];
    uint32_t n_pre, n_suf, size, kind;
};

#ifdef DEF_HOST
#define DEF_FN static inline
#define D_VEC(T, name) T name[64]
#define D_FOR for (int lane_ = 0; lane_ < 64; lane_++)
#define DV(name) name[lane_]
#define D_LANE lane_
#define D_LANE0
#define D_READLANE(name, idx) ((uint32_t)name[(idx)])
#define D_BALLOT(dst, expr) do { dst = 0; for (int lane_ = 0; lane_ < 64; lane_++) if (expr) dst |= 1ull << lane_; } while (0)
#define D_RANK(mask) ((uint32_t)__builtin_popcountll((mask) & ((1ull << lane_) - 1ull)))
#define D_EXCL_SCAN(dst, src, total) do { uint32_t run_ = 0; for (int lane_ = 0; lane_ < 64; lane_++) { const uint32_t v_ = src[lane_]; dst[lane_] = run_; run_ += v_; } total = run_; } while (0)
#define D_SYNC() do { } while (0)
#define D_ATOMIC_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define D_ATOMIC_ADD(p, v) do { *(p) += (v); } while (0)
#define D_ATOMIC_OR(p, v) do { *(p) |= (v); } while (0)
static inline uint32_t def_ld32(const uint8_t* p) { uint32_t x; memcpy(&x, p, 4); return x; }
#else
#define DEF_FN __device__ __forceinline__
#define D_VEC(T, name) T name
#define D_FOR
#define DV(name) name
#define D_LANE ((int)(threadIdx.x & 63))
#define D_LANE0 if ((threadIdx.x & 63) == 0)
#define D_READLANE(name, idx) ((uint32_t)__builtin_amdgcn_readlane((int)(name), (int)(idx)))
#define D_BALLOT(dst, expr) dst = __ballot(expr)
#define D_RANK(mask) ((uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)((mask) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(mask), 0u)))
#define D_EXCL_SCAN(dst, src, total) do { const int v_ = (int)(src); const int i_ = wave_incl_scan_i32(v_); dst = (uint32_t)(i_ - v_); total = (uint32_t)__builtin_amdgcn_readlane(i_, 63); } while (0)
#define D_SYNC() __syncthreads()                 /* the workgroup is one wave: this orders its LDS and global accesses for the compiler and the hardware */
#define D_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define D_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define D_ATOMIC_OR(p, v) atomicOr((p), (v))
typedef uint32_t __attribute__((aligned(1))) def_u32_unaligned;
static __device__ __forceinline__ uint32_t def_ld32(const uint8_t* p) { return *reinterpret_cast<const def_u32_unaligned*>(p); }
#endif

DEF_FN uint32_t def_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
DEF_FN uint32_t def_bitrev(uint32_t code, uint32_t len) { uint32_t r = 0; for (uint32_t i = 0; i < len; i++) { r = (r << 1) | (code & 1u); code >>= 1; } return r; }
// length 3..258 -> symbol - 257 | extra bits << 8 | extra value << 16
DEF_FN uint32_t def_len_sym(uint32_t len) {
    const uint32_t l = len - 3u;
    if (l == 255u) return 28u;
    if (l < 8u) return l;
    const uint32_t e = def_log2(l) - 2u;
    return (4u * e + 4u + ((l >> e) & 3u)) | e << 8 | (l & ((1u << e) - 1u)) << 16;
}
// distance 1..32768 -> symbol | extra bits << 8 | extra value << 16
DEF_FN uint32_t def_dist_sym(uint32_t dist) {
    const uint32_t d = dist - 1u;
    if (d < 4u) return d;
    const uint32_t nb = def_log2(d), e = nb - 1u;
    return (2u * nb + ((d >> e) & 1u)) | e << 8 | (d & ((1u << e) - 1u)) << 16;
}
// common prefix of the text at a and at p, at most maxl bytes (a < p; nothing at or behind p + maxl is read)
DEF_FN uint32_t def_extend(const uint8_t* src, uint32_t a, uint32_t p, uint32_t maxl) {
    uint32_t l = 0;
    while (l + 4u <= maxl) {
        const uint32_t y = def_ld32(src + a + l) ^ def_ld32(src + p + l);
        if (y) return l + ((uint32_t)__builtin_ctz(y) >> 3);
        l += 4u;
    }
    while (l < maxl && src[a + l] == src[p + l]) l++;
    return l;
}

// ---- phase 1: tokens and histograms of one block ----------------------------------------------------------------------------------------------------------
// src: the block's text, n bytes (1..65 280); tok: room for n tokens; hist_out: DEF_NHIST counts (literal/length, then distance; the end-of-block symbol counted once)
DEF_FN void def_match(const uint8_t* src, uint32_t n, uint32_t* tok, uint32_t* hist_out, uint32_t* nt_out, DefMatchLds& L) {
    D_FOR {
        for (uint32_t i = (uint32_t)D_LANE; i < DEF_HSIZE; i += 64u) L.head[i] = 0u;
        for (uint32_t i = (uint32_t)D_LANE; i < DEF_NHIST; i += 64u) L.hist[i] = 0u;
    }
    D_SYNC();
    uint32_t cur = 0, nt = 0, rep = 0;                    // wave-uniform: first position not yet covered, tokens so far, distance of the last match
    for (uint32_t base = 0; base < n; base += 64u) {
        D_VEC(uint32_t, len); D_VEC(uint32_t, dist); D_VEC(uint32_t, hsh);
        const bool look = cur < base + 64u;
        D_FOR {
            const uint32_t p = base + (uint32_t)D_LANE;
            uint32_t bl = 0, bd = 0, h = 0xffffffffu;
            if (p + 4u <= n) {
                const uint32_t x = def_ld32(src + p);
                h = (x * 2654435761u) >> (32 - DEF_HBITS);
                if (look && p >= cur) {
                    const uint32_t maxl = n - p < DEF_MAXLEN ? n - p : DEF_MAXLEN;
                    const uint32_t c = L.head[h];
                    if (c && p - (c - 1u) <= DEF_MAXDIST && def_ld32(src + c - 1u) == x) { bl = def_extend(src, c - 1u, p, maxl); bd = p - (c - 1u); }
                    if (rep && rep <= p && rep != bd && def_ld32(src + p - rep) == x) {
                        const uint32_t l2 = def_extend(src, p - rep, p, maxl);
                        if (l2 >= bl) { bl = l2; bd = rep; }
                    }
                    if (bl < DEF_MINLEN) { bl = 0; bd = 0; }
                }
            }
            DV(len) = bl; DV(dist) = bd; DV(hsh) = h;
        }
        D_SYNC();                                         // every look-up of the batch before any insert of the batch
        D_FOR { if (DV(hsh) != 0xffffffffu) D_ATOMIC_MAX(&L.head[DV(hsh)], base + (uint32_t)D_LANE + 1u); }
        // the parse: which positions of the batch start a token
        uint64_t M; D_BALLOT(M, DV(len) >= DEF_MINLEN);
        const uint32_t lim = n - base < 64u ? n - base : 64u;
        uint32_t r = cur - base;
        uint64_t starts = 0;
        while (r < lim) {
            const uint64_t rest = (M >> r) << r;
            const uint64_t below = (1ull << r) - 1ull;
            if (!rest) { starts |= (lim >= 64u ? ~0ull : (1ull << lim) - 1ull) & ~below; r = lim; break; }
            const uint32_t k = (uint32_t)__builtin_ctzll(rest);
            starts |= (k >= 63u ? ~0ull : (1ull << (k + 1u)) - 1ull) & ~below;
            r = k + D_READLANE(len, k);
            rep = D_READLANE(dist, k);
        }
        cur = base + r;
        D_FOR {
            if ((starts >> D_LANE) & 1ull) {
                const uint32_t at = nt + D_RANK(starts);
                if (DV(len) >= DEF_MINLEN) {
                    tok[at] = DEF_TOK_MATCH | (DV(dist) - 1u) << 9 | (DV(len) - 3u);
                    D_ATOMIC_ADD(&L.hist[257u + (def_len_sym(DV(len)) & 255u)], 1u);
                    D_ATOMIC_ADD(&L.hist[DEF_NL + (def_dist_sym(DV(dist)) & 255u)], 1u);
                } else {
                    const uint32_t b = src[base + (uint32_t)D_LANE];
                    tok[at] = b;
                    D_ATOMIC_ADD(&L.hist[b], 1u);
                }
            }
        }
        nt += (uint32_t)__builtin_popcountll(starts);
        D_SYNC();
    }
    D_FOR { for (uint32_t i = (uint32_t)D_LANE; i < DEF_NHIST; i += 64u) hist_out[i] = L.hist[i] + (i == 256u ? 1u : 0u); }
    D_LANE0 { *nt_out = nt; }
}

// ---- phase 2: codes ------------------------------------------------------------------------------------------------------------------------------------------
// code lengths of at most maxbits for the nsym counts in hist -> len[0..nsym); S.freq, S.sorted and the tree arrays are scratch
DEF_FN void def_build_lengths(const uint32_t* hist, uint32_t nsym, uint32_t maxbits, uint8_t* len, DefCodesLds& S) {
    D_FOR { for (uint32_t s = (uint32_t)D_LANE; s < nsym; s += 64u) { S.freq[s] = hist[s]; len[s] = 0; } }
    D_SYNC();
    D_LANE0 {
        uint32_t used = 0;
        for (uint32_t s = 0; s < nsym; s++) used += S.freq[s] != 0u;
        if (used < 2u && !S.freq[0]) { S.freq[0] = 1u; used++; }
        if (used < 2u) S.freq[1] = 1u;
        uint32_t m = 0;
        for (uint32_t s = 0; s < nsym; s++) m += S.freq[s] != 0u;
        S.cnt[39] = m;
    }
    D_SYNC();
    const uint32_t m = S.cnt[39];
    // rank by (count, symbol): a total order, so the sorted list is unique
    D_FOR {
        for (uint32_t s = (uint32_t)D_LANE; s < nsym; s += 64u) {
            const uint32_t f = S.freq[s];
            if (f) {
                const uint32_t key = f << 9 | s;
                uint32_t rank = 0;
                for (uint32_t t = 0; t < nsym; t++) { const uint32_t g = S.freq[t]; rank += (g != 0u && (g << 9 | t) < key) ? 1u : 0u; }
                S.sorted[rank] = (uint16_t)s;
            }
        }
    }
    D_SYNC();
    D_LANE0 {
        // two queues: leaves in ascending order, internal nodes in the order they are made (ascending too); ties take the leaf
        uint32_t li = 0, ni = 0;
        for (uint32_t k = 0; k + 1u < m; k++) {
            uint32_t f = 0;
            for (int pick = 0; pick < 2; pick++) {
                const bool leaf = li < m && (ni >= k || S.freq[S.sorted[li]] <= S.nfreq[ni]);
                if (leaf) { f += S.freq[S.sorted[li]]; S.lpar[li] = (uint16_t)k; li++; }
                else { f += S.nfreq[ni]; S.npar[ni] = (uint16_t)k; ni++; }
            }
            S.nfreq[k] = f;
        }
        for (uint32_t i = 0; i <= maxbits; i++) S.cnt[i] = 0;
        S.ndepth[m - 2u] = 0;
        for (uint32_t k = m - 2u; k-- > 0u;) S.ndepth[k] = (uint16_t)(S.ndepth[S.npar[k]] + 1u);
        for (uint32_t i = 0; i < m; i++) { const uint32_t d = S.ndepth[S.lpar[i]] + 1u; S.cnt[d < maxbits ? d : maxbits]++; }
        uint32_t total = 0;
        for (uint32_t i = 1; i <= maxbits; i++) total += S.cnt[i] << (maxbits - i);
        while (total != (1u << maxbits)) {
            S.cnt[maxbits]--;
            for (uint32_t i = maxbits - 1u; i > 0u; i--) if (S.cnt[i]) { S.cnt[i]--; S.cnt[i + 1u] += 2u; break; }
            total--;
        }
        uint32_t j = m;
        for (uint32_t i = 1; i <= maxbits; i++) for (uint32_t l = S.cnt[i]; l > 0u; l--) len[S.sorted[--j]] = (uint8_t)i;
    }
    D_SYNC();
}
// canonical codes of len[0..nsym) -> out[s] = reversed code | length << 16 (0 for an unused symbol)
DEF_FN void def_assign_codes(const uint8_t* len, uint32_t nsym, uint32_t maxbits, uint32_t* out, DefCodesLds& S) {
    D_LANE0 {
        for (uint32_t i = 0; i <= maxbits; i++) S.cnt[i] = 0;
        for (uint32_t s = 0; s < nsym; s++) S.cnt[len[s]]++;
        uint32_t code = 0; S.cnt[0] = 0;
        uint32_t prev = 0;
        for (uint32_t i = 1; i <= maxbits; i++) { code = (code + prev) << 1; prev = S.cnt[i]; S.cnt[20 + i] = code; }
        for (uint32_t s = 0; s < nsym; s++) {
            const uint32_t l = len[s];
            out[s] = l ? (def_bitrev(S.cnt[20 + l]++, l) | l << 16) : 0u;
        }
    }
    D_SYNC();
}
#define DEF_ITEM(v, bits) ((uint32_t)(v) | (uint32_t)(bits) << 24)
// hist_in: def_match's counts; n: text bytes of the block (0: the end-of-file block); crc: CRC32 of the text -> *out
DEF_FN void def_codes(const uint32_t* hist_in, uint32_t n, uint32_t crc, DefBlockCodes* out, DefCodesLds& S) {
    if (n == 0u) {
        // the BGZF end-of-file block: an empty fixed-Huffman block, as the SAM specification prints it
        D_LANE0 {
            const uint16_t w[14] = {0x8b1f, 0x0408, 0, 0, 0xff00, 0x0006, 0x4342, 0x0002, 0x001b, 0x0003, 0, 0, 0, 0};
            for (int i = 0; i < 14; i++) out->pre[i] = DEF_ITEM(w[i], 16);
            out->n_pre = 14; out->n_suf = 0; out->size = 28; out->kind = DEF_KIND_EOF;
        }
        D_SYNC();
        return;
    }
    D_FOR { for (uint32_t i = (uint32_t)D_LANE; i < DEF_NHIST; i += 64u) S.hist[i] = hist_in[i]; }
    D_SYNC();
    def_build_lengths(S.hist, 286u, 15u, S.len, S);
    def_build_lengths(S.hist + DEF_NL, 30u, 15u, S.len + DEF_NL, S);
    def_assign_codes(S.len, 286u, 15u, out->code, S);
    def_assign_codes(S.len + DEF_NL, 30u, 15u, out->code + DEF_NL, S);
    D_FOR { for (uint32_t i = 286u + (uint32_t)D_LANE; i < DEF_NL; i += 64u) out->code[i] = 0u; if (D_LANE < 2) out->code[DEF_NL + 30 + D_LANE] = 0u; }
    // the code lengths in run-length form (lane 0), their histogram
    uint32_t hlit = 286u, hdist = 30u, ncl = 0;
    D_LANE0 {
        while (hlit > 257u && !S.len[hlit - 1u]) hlit--;
        while (hdist > 1u && !S.len[DEF_NL + hdist - 1u]) hdist--;
        for (uint32_t i = 0; i < hdist; i++) S.len[hlit + i] = S.len[DEF_NL + i];         // one sequence (hlit <= 286 < DEF_NL: no overlap forwards)
        const uint32_t total = hlit + hdist;
        for (uint32_t i = 0; i < 19u; i++) S.nfreq[DEF_NL - 20 + i] = 0u;
        uint32_t* chist = S.nfreq + DEF_NL - 20;
        uint32_t i = 0;
        while (i < total) {
            const uint32_t v = S.len[i];
            uint32_t run = 1;
            while (i + run < total && S.len[i + run] == v) run++;
            i += run;
            if (v == 0u) {
                while (run >= 11u) { const uint32_t k = run < 138u ? run : 138u; S.cl[ncl++] = (uint16_t)(18u | (k - 11u) << 5); chist[18]++; run -= k; }
                if (run >= 3u) { S.cl[ncl++] = (uint16_t)(17u | (run - 3u) << 5); chist[17]++; run = 0; }
            } else {
                S.cl[ncl++] = (uint16_t)v; chist[v]++; run--;
                while (run >= 3u) { const uint32_t k = run < 6u ? run : 6u; S.cl[ncl++] = (uint16_t)(16u | (k - 3u) << 5); chist[16]++; run -= k; }
            }
            for (; run > 0u; run--) { S.cl[ncl++] = (uint16_t)v; chist[v]++; }
        }
        S.cnt[36] = hlit; S.cnt[37] = hdist; S.cnt[38] = ncl;
        for (uint32_t k = 0; k < 19u; k++) S.hist[k] = chist[k];          // (the token histograms are still needed: kept in hist_in)
    }
    D_SYNC();
    hlit = S.cnt[36]; hdist = S.cnt[37]; ncl = S.cnt[38];
    def_build_lengths(S.hist, 19u, 7u, S.clen, S);
    def_assign_codes(S.clen, 19u, 7u, S.ccode, S);
    D_LANE0 {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const uint8_t clx[19] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 7};
        uint32_t hclen = 19u;
        while (hclen > 4u && !S.clen[order[hclen - 1u]]) hclen--;
        uint64_t bits = 3u + 14u + 3u * hclen;
        for (uint32_t k = 0; k < ncl; k++) { const uint32_t s = S.cl[k] & 31u; bits += S.clen[s] + clx[s]; }
        for (uint32_t s = 0; s < 286u; s++) {
            const uint32_t f = hist_in[s];
            if (f) { uint32_t x = 0; if (s >= 265u && s < 285u) x = (s - 261u) >> 2; bits += (uint64_t)f * ((out->code[s] >> 16) + x); }
        }
        for (uint32_t s = 0; s < 30u; s++) {
            const uint32_t f = hist_in[DEF_NL + s];
            if (f) bits += (uint64_t)f * ((out->code[DEF_NL + s] >> 16) + (s >= 4u ? (s >> 1) - 1u : 0u));
        }
        const uint32_t dyn = (uint32_t)((bits + 7u) >> 3);
        const bool stored = dyn >= n;
        const uint32_t payload = stored ? n + 5u : dyn;
        const uint32_t size = 18u + payload + 8u;
        const uint16_t w[9] = {0x8b1f, 0x0408, 0, 0, 0xff00, 0x0006, 0x4342, 0x0002, (uint16_t)(size - 1u)};
        uint32_t np = 0, ns = 0;
        for (int i = 0; i < 9; i++) out->pre[np++] = DEF_ITEM(w[i], 16);
        if (stored) {
            out->pre[np++] = DEF_ITEM(1u, 8);                        // BFINAL = 1, BTYPE = 00, padding
            out->pre[np++] = DEF_ITEM(n, 16);
            out->pre[np++] = DEF_ITEM(~n & 0xffffu, 16);
        } else {
            out->pre[np++] = DEF_ITEM(1u | 2u << 1, 3);              // BFINAL = 1, BTYPE = 10
            out->pre[np++] = DEF_ITEM((hlit - 257u) | (hdist - 1u) << 5 | (hclen - 4u) << 10, 14);
            for (uint32_t k = 0; k < hclen; k++) out->pre[np++] = DEF_ITEM(S.clen[order[k]], 3);
            for (uint32_t k = 0; k < ncl; k++) {
                const uint32_t s = S.cl[k] & 31u, x = S.cl[k] >> 5, c = S.ccode[s], l = c >> 16;
                out->pre[np++] = DEF_ITEM((c & 0xffffu) | x << l, l + clx[s]);
            }
            const uint32_t eob = out->code[256];
            out->suf[ns++] = DEF_ITEM(eob & 0xffffu, eob >> 16);
            const uint32_t pad = (uint32_t)((8u - (bits & 7u)) & 7u);
            if (pad) out->suf[ns++] = DEF_ITEM(0u, pad);
        }
        out->suf[ns++] = DEF_ITEM(crc & 0xffffu, 16); out->suf[ns++] = DEF_ITEM(crc >> 16, 16);
        out->suf[ns++] = DEF_ITEM(n & 0xffffu, 16); out->suf[ns++] = DEF_ITEM(n >> 16, 16);
        out->n_pre = np; out->n_suf = ns; out->size = size; out->kind = stored ? DEF_KIND_STORED : DEF_KIND_DYNAMIC;
    }
    D_SYNC();
}

// ---- phase 3: bits ---------------------------------------------------------------------------------------------------------------------------------------------
struct DefBitPos { uint32_t bitpos, wbase; };
// one batch: lane l appends the low nb bits of v (nb <= 48; 0: nothing) behind those of the lanes before it
#define DEF_EMIT_BATCH(v, nb)                                                                                                       \
    do {                                                                                                                            \
        D_VEC(uint32_t, off_); uint32_t total_;                                                                                     \
        D_EXCL_SCAN(off_, nb, total_);                                                                                              \
        D_FOR {                                                                                                                     \
            if (DV(nb)) {                                                                                                           \
                const uint32_t pos_ = bp.bitpos + DV(off_), w_ = (pos_ >> 5) - bp.wbase, sh_ = pos_ & 31u;                          \
                const uint64_t val_ = DV(v) & ((1ull << DV(nb)) - 1ull), lo_ = val_ << sh_;                                        \
                const uint32_t hi_ = sh_ ? (uint32_t)(val_ >> (64u - sh_)) : 0u;                                                    \
                if ((uint32_t)lo_) D_ATOMIC_OR(&L.stage[w_], (uint32_t)lo_);                                                        \
                if ((uint32_t)(lo_ >> 32)) D_ATOMIC_OR(&L.stage[w_ + 1u], (uint32_t)(lo_ >> 32));                                   \
                if (hi_) D_ATOMIC_OR(&L.stage[w_ + 2u], hi_);                                                                       \
            }                                                                                                                       \
        }                                                                                                                           \
        D_SYNC();                                                                                                                   \
        bp.bitpos += total_;                                                                                                        \
        const uint32_t done_ = (bp.bitpos >> 5) - bp.wbase;                                                                         \
        if (done_) {                                                                                                                \
            D_FOR { for (uint32_t i_ = (uint32_t)D_LANE; i_ < done_; i_ += 64u) dst[bp.wbase + i_] = L.stage[i_]; }                 \
            const uint32_t carry_ = L.stage[done_];                                                                                 \
            D_SYNC();                                                                                                               \
            D_FOR { for (uint32_t i_ = (uint32_t)D_LANE; i_ < done_ + 3u && i_ < DEF_STAGE; i_ += 64u) L.stage[i_] = i_ ? 0u : carry_; } \
            D_SYNC();                                                                                                               \
            bp.wbase += done_;                                                                                                      \
        }                                                                                                                           \
    } while (0)

// src, n, tok, nt: as in def_match; bc: def_codes' result for the block; dst: the block's slot (DEF_SLOT bytes, 4-byte aligned).  bc->size bytes are the block
DEF_FN void def_bits(const uint8_t* src, uint32_t n, const uint32_t* tok, uint32_t nt, const DefBlockCodes* bc, uint32_t* dst, DefBitsLds& L) {
    D_FOR {
        for (uint32_t i = (uint32_t)D_LANE; i < DEF_NHIST; i += 64u) L.code[i] = bc->code[i];
        for (uint32_t i = (uint32_t)D_LANE; i < DEF_STAGE; i += 64u) L.stage[i] = 0u;
    }
    D_SYNC();
    DefBitPos bp; bp.bitpos = 0; bp.wbase = 0;
    const uint32_t np = bc->n_pre, ns = bc->n_suf, kind = bc->kind;
    for (uint32_t base = 0; base < np; base += 64u) {
        D_VEC(uint64_t, v); D_VEC(uint32_t, nb);
        D_FOR { const uint32_t i = base + (uint32_t)D_LANE; const uint32_t it = i < np ? bc->pre[i] : 0u; DV(v) = it & 0xffffffu; DV(nb) = it >> 24; }
        DEF_EMIT_BATCH(v, nb);
    }
    if (kind == DEF_KIND_DYNAMIC) {
        for (uint32_t base = 0; base < nt; base += 64u) {
            D_VEC(uint64_t, v); D_VEC(uint32_t, nb);
            D_FOR {
                const uint32_t i = base + (uint32_t)D_LANE;
                uint64_t val = 0; uint32_t bits = 0;
                if (i < nt) {
                    const uint32_t t = tok[i];
                    if (t & DEF_TOK_MATCH) {
                        const uint32_t ls = def_len_sym((t & 511u) + 3u), ds = def_dist_sym(((t >> 9) & 0x7fffu) + 1u);
                        const uint32_t lc = L.code[257u + (ls & 255u)], dc = L.code[DEF_NL + (ds & 255u)];
                        val = lc & 0xffffu; bits = lc >> 16;
                        val |= (uint64_t)(ls >> 16) << bits; bits += (ls >> 8) & 255u;
                        val |= (uint64_t)(dc & 0xffffu) << bits; bits += dc >> 16;
                        val |= (uint64_t)(ds >> 16) << bits; bits += (ds >> 8) & 255u;
                    } else { const uint32_t c = L.code[t]; val = c & 0xffffu; bits = c >> 16; }
                }
                DV(v) = val; DV(nb) = bits;
            }
            DEF_EMIT_BATCH(v, nb);
        }
    } else if (kind == DEF_KIND_STORED) {
        for (uint32_t base = 0; base < n; base += 256u) {
            D_VEC(uint64_t, v); D_VEC(uint32_t, nb);
            D_FOR {
                const uint32_t p = base + 4u * (uint32_t)D_LANE;
                uint64_t val = 0; uint32_t k = 0;
                for (; k < 4u && p + k < n; k++) val |= (uint64_t)src[p + k] << (8u * k);
                DV(v) = val; DV(nb) = 8u * k;
            }
            DEF_EMIT_BATCH(v, nb);
        }
    }
    {
        D_VEC(uint64_t, v); D_VEC(uint32_t, nb);
        D_FOR { const uint32_t it = (uint32_t)D_LANE < ns ? bc->suf[D_LANE] : 0u; DV(v) = it & 0xffffffu; DV(nb) = it >> 24; }
        DEF_EMIT_BATCH(v, nb);
    }
    if (bp.bitpos & 31u) { D_LANE0 { dst[bp.wbase] = L.stage[0]; } }
}

#ifdef DEF_HOST
#include <vector>
// One file of text -> its BGZF stream (blocks of DEF_BLOCK bytes, the end-of-file block behind them), by the three phases above.  crc_fn: CRC32 of a byte range
// (zlib's; the device has a kernel for it).  Returns the number of bytes, or -1 when cap is too small.  block_coff / block_uoff (may be null): the block table.
static inline int64_t def_file_host(const uint8_t* text, int64_t n, uint8_t* out, int64_t cap, uint32_t (*crc_fn)(const uint8_t*, uint32_t),
                                    std::vector<int64_t>* block_coff = nullptr, std::vector<int64_t>* block_uoff = nullptr, int64_t* kinds = nullptr) {
    static thread_local DefMatchLds ML; static thread_local DefCodesLds CL; static thread_local DefBitsLds BL;
    std::vector<uint32_t> tok(DEF_BLOCK), slot(DEF_SLOT / 4), hist(DEF_NHIST);
    DefBlockCodes bc;
    int64_t at = 0;
    for (int64_t lo = 0;; lo += DEF_BLOCK) {
        const uint32_t len = lo < n ? (uint32_t)(n - lo < (int64_t)DEF_BLOCK ? n - lo : (int64_t)DEF_BLOCK) : 0u;
        uint32_t nt = 0;
        if (len) def_match(text + lo, len, tok.data(), hist.data(), &nt, ML);
        def_codes(hist.data(), len, len ? crc_fn(text + lo, len) : 0u, &bc, CL);
        def_bits(text + lo, len, tok.data(), nt, &bc, slot.data(), BL);
        if (at + (int64_t)bc.size > cap) return -1;
        memcpy(out + at, slot.data(), bc.size);
        if (block_coff) block_coff->push_back(at);
        if (block_uoff) block_uoff->push_back(lo < n ? lo : n);
        if (kinds) kinds[bc.kind]++;
        at += bc.size;
        if (!len) break;
    }
    if (block_coff) block_coff->push_back(at);
    if (block_uoff) block_uoff->push_back(n);
    return at;
}
#endif
