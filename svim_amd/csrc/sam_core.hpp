// sam_core.hpp - one alignment line of SAM text -> the bytes of its BAM record: one source for the host build (sam_host.cpp: svx_sam_convert_host) and the
// kernels (sam.hip).  The rule in words: svim_amd/sam.py (SAM specification 1.4, 4.2, 4.2.4; htslib's sam_parse1 where the specification leaves a choice).
// Here: the field walk, the integer parser with its range checks, the size of a record from its line, the aux typing rule, the nibble table, the float fast
// path and `bin`.  Everything is byte-wise: a record starts at any byte of the stream.
#pragma once
#include <stdint.h>
#include "contig_core.hpp"

#if defined(__HIPCC__)
#define SAM_FN __host__ __device__ inline
#else
#define SAM_FN static inline
#endif

// what a line is refused for (svx_sam_convert_host / the reader report the first bad line with one of these)
enum { SAM_OK = 0, SAM_E_FIELDS = 1 /* fewer than 11 fields */, SAM_E_RANGE = 2 /* a number missing, malformed or outside its field's range */, SAM_E_AUX = 3 /* a bad aux field */,
       SAM_E_HEADER = 4 /* a header line behind the first alignment */, SAM_E_REF = 5 /* RNAME / RNEXT not in the dictionary */, SAM_E_CIGAR = 6, SAM_E_QUAL = 7 /* QUAL and SEQ differ in length */,
       SAM_E_QNAME = 8 /* QNAME empty or longer than 254 */, SAM_E_FLOAT = 9 /* an 'f' value strtod does not take whole (found by the host when it patches) */ };
#define SAM_MAX_CIG_LEN ((1u << 28) - 1u)
#define SAM_MAX_BAM_OPS 65535u                /* beyond this the record holds <l_seq>S<reflen>N and the real CIGAR in CG:B:I (SAM specification 4.2.2) */

SAM_FN const char* sam_strerror(int e) {
    return e == SAM_E_FIELDS ? "fewer than 11 fields" : e == SAM_E_RANGE ? "a value missing, malformed or out of its field's range" : e == SAM_E_AUX ? "bad aux field" :
           e == SAM_E_HEADER ? "header line after the first alignment" : e == SAM_E_REF ? "RNAME or RNEXT not in the @SQ dictionary" : e == SAM_E_CIGAR ? "bad CIGAR" :
           e == SAM_E_QUAL ? "QUAL and SEQ differ in length" : e == SAM_E_QNAME ? "QNAME empty or longer than 254 bytes" : e == SAM_E_FLOAT ? "bad float value" : "ok";
}

SAM_FN bool sam_digit(uint8_t c) { return c >= '0' && c <= '9'; }
SAM_FN void sam_w16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
SAM_FN void sam_w32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// [+-]digits, nothing else, lo <= value <= hi (|value| below 10^18: longer numbers are refused before they can overflow)
SAM_FN bool sam_parse_int(const uint8_t* s, uint32_t n, int64_t lo, int64_t hi, int64_t* v) {
    uint32_t i = 0; bool neg = false;
    if (n && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
    if (i >= n) return false;
    int64_t x = 0; uint32_t nd = 0;
    for (; i < n; i++) {
        if (!sam_digit(s[i])) return false;
        if (x || s[i] != '0') nd++;
        if (nd > 18) return false;
        x = x * 10 + (s[i] - '0');
    }
    if (neg) x = -x;
    if (x < lo || x > hi) return false;
    *v = x;
    return true;
}

// "=ACMGRSVTWYHKDBN", case ignored, every other byte 15
SAM_FN uint8_t sam_nib(uint8_t c) {
    if (c == '=') return 0;
    const uint8_t l = c | 0x20;
    if (l < 'a' || l > 'z') return 15;
    //                       p o n m l k j i h g f e d c b a                        z y x w v u t s r q
    const uint64_t lo = 0xfff3fcffb4ffd2e1ull, hi = 0xfaf97f865full;
    const uint32_t k = (uint32_t)(l - 'a');
    return (uint8_t)((k < 16 ? lo >> (4 * k) : hi >> (4 * (k - 16))) & 15u);
}
// "MIDNSHP=X" -> 0..8, anything else -1
SAM_FN int sam_cigar_op(uint8_t c) {
    return c == 'M' ? 0 : c == 'I' ? 1 : c == 'D' ? 2 : c == 'N' ? 3 : c == 'S' ? 4 : c == 'H' ? 5 : c == 'P' ? 6 : c == '=' ? 7 : c == 'X' ? 8 : -1;
}
SAM_FN bool sam_op_on_ref(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
// the operation whose letter is s[p] (digits in front of it back to `lo`): 1 to 9 digits, at most 2^28 - 1.  false: no operation
SAM_FN bool sam_cigar_at(const uint8_t* s, uint32_t lo, uint32_t p, uint32_t* word) {
    const int op = sam_cigar_op(s[p]);
    uint32_t q = p, nd = 0; uint64_t v = 0, mul = 1;
    while (q > lo && sam_digit(s[q - 1]) && nd < 10) { q--; v += mul * (uint64_t)(s[q] - '0'); mul *= 10; nd++; }
    if (op < 0 || nd == 0 || nd > 9 || v > SAM_MAX_CIG_LEN) return false;
    *word = (uint32_t)(v << 4) | (uint32_t)op;
    return true;
}

// htslib's hts_reg2bin on [beg, end) with min_shift 14 and five levels, as bam.bin holds it
SAM_FN uint32_t sam_reg2bin(int64_t beg, int64_t end) {
    end--;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
SAM_FN uint32_t sam_bin(int32_t pos, uint32_t flag, int64_t reflen) {
    const int64_t end = ((flag & 4u) || reflen == 0) ? (int64_t)pos + 1 : (int64_t)pos + reflen;
    return sam_reg2bin(pos, end) & 0xffffu;
}

// ---- floats -----------------------------------------------------------------------------------------------------------------------------------------
// The fast path: at most 15 significant digits m and a decimal exponent k of at most 22 in magnitude.  m and 10^|k| are exact doubles, so m * 10^k or
// m / 10^-k is ONE correctly rounded operation on exact operands - the double strtod returns; the cast to float follows as in htslib.  false: the value
// is left to the host's strtod (inf, nan, long mantissas, more than 400 fractional digits, large exponents, and whatever is no number at all).
SAM_FN bool sam_float_fast(const uint8_t* s, uint32_t n, float* out) {
    const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    uint32_t i = 0; bool neg = false, any = false;
    if (n && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
    uint64_t m = 0; uint32_t nd = 0; int32_t frac = 0;
    for (; i < n && sam_digit(s[i]); i++) { any = true; if (m || s[i] != '0') { nd++; if (nd <= 15) m = m * 10 + (uint64_t)(s[i] - '0'); } }
    if (i < n && s[i] == '.') {
        for (i++; i < n && sam_digit(s[i]); i++) { any = true; if (++frac > 400) return false; if (m || s[i] != '0') { nd++; if (nd <= 15) m = m * 10 + (uint64_t)(s[i] - '0'); } }
    }
    if (!any || nd > 15) return false;
    int32_t e = 0;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (s[i] == '-' || s[i] == '+')) { eneg = s[i] == '-'; i++; }
        if (i >= n) return false;
        uint32_t ed = 0;
        for (; i < n && sam_digit(s[i]); i++) { if (++ed > 6) return false; e = e * 10 + (s[i] - '0'); }
        if (ed == 0) return false;
        if (eneg) e = -e;
    }
    if (i != n) return false;
    const int32_t k = e - frac;
    if (k < -22 || k > 22) return false;
    double v = (double)m;
    v = k < 0 ? v / p10[-k] : v * p10[k];
    *out = (float)(neg ? -v : v);
    return true;
}

// ---- aux fields -------------------------------------------------------------------------------------------------------------------------------------
// 'i': the smallest type that holds the value (htslib): negative c from -128, s from -32768, then i; non-negative C to 255, S to 65535, then I
SAM_FN uint8_t sam_int_type(int64_t v, uint32_t* bytes) {
    if (v < 0) { if (v >= -128) { *bytes = 1; return 'c'; } if (v >= -32768) { *bytes = 2; return 's'; } *bytes = 4; return 'i'; }
    if (v <= 255) { *bytes = 1; return 'C'; } if (v <= 65535) { *bytes = 2; return 'S'; } *bytes = 4; return 'I';
}
SAM_FN uint32_t sam_b_elem(uint8_t sub, int64_t* lo, int64_t* hi) {
    switch (sub) {
        case 'c': *lo = -128; *hi = 127; return 1;
        case 'C': *lo = 0; *hi = 255; return 1;
        case 's': *lo = -32768; *hi = 32767; return 2;
        case 'S': *lo = 0; *hi = 65535; return 2;
        case 'i': *lo = -2147483648ll; *hi = 2147483647ll; return 4;
        case 'I': *lo = 0; *hi = 4294967295ll; return 4;
        case 'f': *lo = 0; *hi = 0; return 4;
    }
    return 0;
}
// a float the fast path leaves to the host: where its 4 bytes lie in the stream, where its text lies in the chunk
struct SamPatch { uint64_t at; uint64_t text_at; uint32_t text_len; uint32_t line; };

// one field XX:T:value of `n` bytes -> the bytes it takes in the record and the floats in it that miss the fast path; != 0: what is wrong with it
SAM_FN int sam_aux_size(const uint8_t* s, uint32_t n, uint32_t* bytes, uint32_t* n_patch) {
    *bytes = 0; *n_patch = 0;
    if (n < 5 || s[2] != ':' || s[4] != ':') return SAM_E_AUX;
    const uint8_t ty = s[3];
    const uint8_t* v = s + 5; const uint32_t m = n - 5;
    if (ty == 'A') { if (m != 1) return SAM_E_AUX; *bytes = 4; return SAM_OK; }
    if (ty == 'Z' || ty == 'H') { *bytes = 3 + m + 1; return SAM_OK; }
    if (ty == 'i') {
        int64_t x; uint32_t w;
        if (!sam_parse_int(v, m, -2147483648ll, 4294967295ll, &x)) return SAM_E_RANGE;
        (void)sam_int_type(x, &w);
        *bytes = 3 + w;
        return SAM_OK;
    }
    if (ty == 'f') { float f; if (m == 0) return SAM_E_RANGE; if (!sam_float_fast(v, m, &f)) *n_patch = 1; *bytes = 7; return SAM_OK; }
    if (ty == 'B') {
        int64_t lo = 0, hi = 0;
        if (m < 1) return SAM_E_AUX;
        const uint32_t es = sam_b_elem(v[0], &lo, &hi);
        if (!es || (m > 1 && v[1] != ',')) return SAM_E_AUX;
        uint32_t cnt = 0, np = 0;
        for (uint32_t a = 1; a < m;) {                     // v[a] == ','
            uint32_t b = a + 1;
            while (b < m && v[b] != ',') b++;
            if (b == a + 1) return SAM_E_RANGE;
            if (v[0] == 'f') { float f; if (!sam_float_fast(v + a + 1, b - a - 1, &f)) np++; }
            else { int64_t x; if (!sam_parse_int(v + a + 1, b - a - 1, lo, hi, &x)) return SAM_E_RANGE; }
            cnt++; a = b;
        }
        *bytes = 3 + 1 + 4 + es * cnt; *n_patch = np;
        return SAM_OK;
    }
    return SAM_E_AUX;
}
// the same field written at out (sam_aux_size has accepted it).  copy_payload false: the bytes of a Z / H value are left to the caller (the kernels copy them
// wave-wide), only tag, type and the closing NUL are written.  patch: *n_patch entries are filled for the floats left to the host (their 4 bytes stay 0).
SAM_FN void sam_aux_emit(const uint8_t* s, uint32_t n, uint8_t* out, bool copy_payload, uint64_t out_at, uint64_t text_at, uint32_t line, SamPatch* patch) {
    const uint8_t ty = s[3];
    const uint8_t* v = s + 5; const uint32_t m = n - 5;
    out[0] = s[0]; out[1] = s[1]; out[2] = ty;
    if (ty == 'A') { out[3] = v[0]; return; }
    if (ty == 'Z' || ty == 'H') { if (copy_payload) for (uint32_t k = 0; k < m; k++) out[3 + k] = v[k]; out[3 + m] = 0; return; }
    if (ty == 'i') {
        int64_t x = 0; uint32_t w;
        (void)sam_parse_int(v, m, -2147483648ll, 4294967295ll, &x);
        out[2] = sam_int_type(x, &w);
        const uint32_t u = (uint32_t)x;
        for (uint32_t k = 0; k < w; k++) out[3 + k] = (uint8_t)(u >> (8 * k));
        return;
    }
    uint32_t np = 0;
    if (ty == 'f') {
        float f = 0.f; uint32_t u = 0;
        if (sam_float_fast(v, m, &f)) { union { float f; uint32_t u; } c; c.f = f; u = c.u; }
        else patch[np++] = SamPatch{out_at + 3, text_at + 5, m, line};
        sam_w32(out + 3, u);
        return;
    }
    // B
    int64_t lo = 0, hi = 0;
    const uint32_t es = sam_b_elem(v[0], &lo, &hi);
    out[3] = v[0];
    uint32_t cnt = 0;
    uint8_t* w = out + 8;
    for (uint32_t a = 1; a < m;) {
        uint32_t b = a + 1;
        while (b < m && v[b] != ',') b++;
        uint32_t u = 0;
        if (v[0] == 'f') {
            float f = 0.f;
            if (sam_float_fast(v + a + 1, b - a - 1, &f)) { union { float f; uint32_t u; } c; c.f = f; u = c.u; }
            else patch[np++] = SamPatch{out_at + (uint64_t)(w - out), text_at + 5 + a + 1, b - a - 1, line};
        } else { int64_t x = 0; (void)sam_parse_int(v + a + 1, b - a - 1, lo, hi, &x); u = (uint32_t)x; }
        for (uint32_t k = 0; k < es; k++) w[k] = (uint8_t)(u >> (8 * k));
        w += es; cnt++; a = b;
    }
    sam_w32(out + 4, cnt);
}

// ---- a line ------------------------------------------------------------------------------------------------------------------------------------------
// f[k] = where field k starts (k = 0..10), f[11] = where the aux fields start (len + 1 when there are none): field k is [f[k], f[k + 1] - 1)
struct SamDesc { uint32_t f[12]; uint32_t len, n_ops, l_seq, aux_bytes, n_patch, err; };
// bytes of the record (block_size included) from what measure found
SAM_FN uint64_t sam_record_bytes(const SamDesc& d) {
    const uint32_t l_name = d.f[1] - d.f[0];            // QNAME and its NUL
    const bool lng = d.n_ops > SAM_MAX_BAM_OPS;
    return 36ull + l_name + 4ull * (lng ? 2u : d.n_ops) + ((uint64_t)d.l_seq + 1) / 2 + d.l_seq + d.aux_bytes + (lng ? 8ull + 4ull * d.n_ops : 0ull);
}
// the checks of the fields that need no neighbour: called once per line by whoever has the field starts (d.f, d.len set).  Sets l_seq and err
SAM_FN void sam_check_fields(const uint8_t* s, SamDesc& d) {
    d.err = SAM_OK;
    const uint32_t l_name = d.f[1] - 1 - d.f[0];
    if (l_name < 1 || l_name > 254) { d.err = SAM_E_QNAME; return; }
    const uint32_t ls = d.f[10] - 1 - d.f[9], lq = d.f[11] - 1 - d.f[10];
    const bool no_seq = ls == 1 && s[d.f[9]] == '*', no_qual = lq == 1 && s[d.f[10]] == '*';
    d.l_seq = no_seq ? 0u : ls;
    if (ls == 0 || lq == 0) { d.err = SAM_E_RANGE; return; }
    if (!no_qual && lq != d.l_seq) { d.err = SAM_E_QUAL; return; }
}
// the 32 bytes of fixed fields behind block_size.  reflen: reference bases of the CIGAR.  != 0: why not
SAM_FN int sam_fixed(const uint8_t* s, const SamDesc& d, const ContigTable& ct, int64_t reflen, uint8_t* out /* the record: block_size first */) {
    int64_t flag, pos, mapq, pnext, tlen;
    if (!sam_parse_int(s + d.f[1], d.f[2] - 1 - d.f[1], 0, 65535, &flag)) return SAM_E_RANGE;
    if (!sam_parse_int(s + d.f[3], d.f[4] - 1 - d.f[3], 0, 2147483647ll, &pos)) return SAM_E_RANGE;
    if (!sam_parse_int(s + d.f[4], d.f[5] - 1 - d.f[4], 0, 255, &mapq)) return SAM_E_RANGE;
    if (!sam_parse_int(s + d.f[7], d.f[8] - 1 - d.f[7], 0, 2147483647ll, &pnext)) return SAM_E_RANGE;
    if (!sam_parse_int(s + d.f[8], d.f[9] - 1 - d.f[8], -2147483648ll, 2147483647ll, &tlen)) return SAM_E_RANGE;
    int32_t tid = -1, ntid = -1;
    const uint32_t lr = d.f[3] - 1 - d.f[2], ln = d.f[7] - 1 - d.f[6];
    if (lr == 0 || ln == 0) return SAM_E_REF;
    if (!(lr == 1 && s[d.f[2]] == '*')) { tid = ctg_lookup(ct, s + d.f[2], lr); if (tid < 0) return SAM_E_REF; }
    if (ln == 1 && s[d.f[6]] == '=') ntid = tid;
    else if (!(ln == 1 && s[d.f[6]] == '*')) { ntid = ctg_lookup(ct, s + d.f[6], ln); if (ntid < 0) return SAM_E_REF; }
    const bool lng = d.n_ops > SAM_MAX_BAM_OPS;
    const uint32_t l_name = d.f[1] - d.f[0];
    sam_w32(out, (uint32_t)(sam_record_bytes(d) - 4));
    sam_w32(out + 4, (uint32_t)tid);
    sam_w32(out + 8, (uint32_t)(int32_t)(pos - 1));
    out[12] = (uint8_t)l_name; out[13] = (uint8_t)mapq;
    sam_w16(out + 14, sam_bin((int32_t)(pos - 1), (uint32_t)flag, reflen));
    sam_w16(out + 16, lng ? 2u : d.n_ops);
    sam_w16(out + 18, (uint32_t)flag);
    sam_w32(out + 20, d.l_seq);
    sam_w32(out + 24, (uint32_t)ntid);
    sam_w32(out + 28, (uint32_t)(int32_t)(pnext - 1));
    sam_w32(out + 32, (uint32_t)(int32_t)tlen);
    return SAM_OK;
}
// CG:B:I header behind the last aux field of a long-CIGAR record, and the placeholder in the CIGAR's place
SAM_FN void sam_long_cigar_frame(const SamDesc& d, int64_t reflen, uint8_t* placeholder, uint8_t* cg) {
    sam_w32(placeholder, (d.l_seq << 4) | 4u);
    sam_w32(placeholder + 4, ((uint32_t)reflen << 4) | 3u);
    cg[0] = 'C'; cg[1] = 'G'; cg[2] = 'B'; cg[3] = 'I';
    sam_w32(cg + 4, d.n_ops);
}
