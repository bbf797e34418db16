// fmt_repr.hpp - repr(float) as CPython prints it, in integer arithmetic, host and device from one source.
//
// FP64 -> the shortest decimal digit string that parses back to the same double, and among the shortest the one closest to the value (what CPython's repr
// gets from David Gay's dtoa in mode 0), in CPython's layout (Python/pystrtod.c, format_float_short with 'r'): fixed notation with at least one digit behind
// the point while the decimal point position is in (-4, 16], otherwise d[.ddd]e+XX / e-XX with at least two exponent digits; -0.0, inf, -inf, nan.
//
// The digits come from the Ryu algorithm (Ulf Adams, "Ryu: fast float-to-string conversion", PLDI 2018): the value and the two halfway points to its
// neighbours are scaled by a power of ten with ONE 64 x 128-bit multiplication each against a table of 5^i (326 entries) or 2^k / 5^i (342 entries), 125
// significant bits each, then digits are dropped while the interval still holds a shorter number.  Right for every finite double.  The tables are not
// written out: repr_build_tables() makes them with a small big-integer generator on the host (5^i by repeated multiplication, 2^k / 5^i by i divisions by 5);
// the device reads a copy the host uploads (api: svx_repr_device_tables).  No double arithmetic, no printf, no library call in repr_digits / put_repr.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

#define REPR_POW5_INV_BITCOUNT 125
#define REPR_POW5_BITCOUNT 125
#define REPR_POW5_INV_N 342
#define REPR_POW5_N 326
#define REPR_TABLE_WORDS (2 * (REPR_POW5_INV_N + REPR_POW5_N))      /* uint64 words: inv[i] = {lo, hi} first, then pow5[i] = {lo, hi} */

// ---------------------------------------------------------------------------------------------------------
// host: the table generator
// ---------------------------------------------------------------------------------------------------------
#define REPR_BIG_LIMBS 32      /* 32 x 32 bits = 1024 bits: 2^(125 + 792) is the largest number built */
struct ReprBig { uint32_t w[REPR_BIG_LIMBS]; };
inline void repr_big_set_pow2(ReprBig& a, int bit) { memset(a.w, 0, sizeof a.w); a.w[bit >> 5] = 1u << (bit & 31); }
inline void repr_big_mul_small(ReprBig& a, uint32_t m) {
    uint64_t carry = 0;
    for (int k = 0; k < REPR_BIG_LIMBS; k++) { const uint64_t t = (uint64_t)a.w[k] * m + carry; a.w[k] = (uint32_t)t; carry = t >> 32; }
}
inline void repr_big_div_small(ReprBig& a, uint32_t d) {
    uint64_t rem = 0;
    for (int k = REPR_BIG_LIMBS - 1; k >= 0; k--) { const uint64_t t = (rem << 32) | a.w[k]; a.w[k] = (uint32_t)(t / d); rem = t % d; }
}
inline int repr_big_bitlength(const ReprBig& a) {
    for (int k = REPR_BIG_LIMBS - 1; k >= 0; k--) if (a.w[k]) { int b = 32; while (!(a.w[k] >> (b - 1))) b--; return 32 * k + b; }
    return 0;
}
// bits [sh, sh + 128) of a (sh may be negative: shifted left) -> {lo, hi}
inline void repr_big_window(const ReprBig& a, int sh, uint64_t out[2]) {
    out[0] = out[1] = 0;
    for (int b = 0; b < 128; b++) {
        const int src = sh + b;
        if (src < 0 || src >= 32 * REPR_BIG_LIMBS) continue;
        if ((a.w[src >> 5] >> (src & 31)) & 1u) out[b >> 6] |= 1ull << (b & 63);
    }
}
// tab[REPR_TABLE_WORDS]
inline void repr_build_tables(uint64_t* tab) {
    ReprBig p; repr_big_set_pow2(p, 0);                       // 5^i
    for (int i = 0; i < REPR_POW5_INV_N; i++) {
        const int len = repr_big_bitlength(p);
        if (i < REPR_POW5_N) repr_big_window(p, len - REPR_POW5_BITCOUNT, tab + 2 * REPR_POW5_INV_N + 2 * i);      // the top 125 bits of 5^i
        ReprBig q; repr_big_set_pow2(q, len - 1 + REPR_POW5_INV_BITCOUNT);      // floor(2^(len - 1 + 125) / 5^i) + 1: floor(floor(x / 5) / 5) = floor(x / 25)
        for (int k = 0; k < i; k++) repr_big_div_small(q, 5);
        uint64_t v[2]; repr_big_window(q, 0, v);
        if (++v[0] == 0) v[1]++;
        tab[2 * i] = v[0]; tab[2 * i + 1] = v[1];
        repr_big_mul_small(p, 5);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host and device: digits
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline int repr_pow5bits(int e) { return (int)(((unsigned)e * 1217359u) >> 19) + 1; }      // bit length of 5^e, 0 <= e <= 3528
__host__ __device__ inline int repr_log10pow2(int e) { return (int)(((unsigned)e * 78913u) >> 18); }           // floor(log10(2^e)), 0 <= e <= 1650
__host__ __device__ inline int repr_log10pow5(int e) { return (int)(((unsigned)e * 732923u) >> 20); }          // floor(log10(5^e)), 0 <= e <= 2620

// high and low half of a 64 x 64 bit product from 32-bit pieces (the same code on both sides: no __int128, no intrinsic)
__host__ __device__ inline uint64_t repr_mul64(uint64_t a, uint64_t b, uint64_t* hi) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = p10 + (p00 >> 32) + (uint32_t)p01;
    *hi = p11 + (mid >> 32) + (p01 >> 32);
    return (mid << 32) | (uint32_t)p00;
}
// (m * mul) >> j for a 128-bit mul = {lo, hi} with at most 125 bits, m < 2^56, 64 < j < 128 + 56
__host__ __device__ inline uint64_t repr_mulshift(uint64_t m, const uint64_t* mul, int j) {
    uint64_t h0, h1;
    (void)repr_mul64(m, mul[0], &h0);
    const uint64_t l1 = repr_mul64(m, mul[1], &h1);
    const uint64_t s0 = h0 + l1, s1 = h1 + (s0 < h0 ? 1u : 0u);      // ((m * lo) >> 64) + m * hi
    const int s = j - 64;                                            // 0 < s < 64 for every double; the other two branches keep the shift defined
    return s <= 0 ? s0 : s >= 64 ? s1 >> (s - 64) : (s1 << (64 - s)) | (s0 >> s);
}
__host__ __device__ inline int repr_pow5factor(uint64_t v) { int c = 0; while (v && v % 5ull == 0) { v /= 5ull; c++; } return c; }

// finite, non-zero |x| given by its fields -> digits (an integer of 1..17 decimal digits) and the power of ten that goes with them
__host__ __device__ inline void repr_digits(uint64_t ieee_mant, int ieee_exp, const uint64_t* tab, uint64_t* digits, int* exp10) {
    int e2; uint64_t m2;
    if (ieee_exp == 0) { e2 = 1 - 1023 - 52 - 2; m2 = ieee_mant; } else { e2 = ieee_exp - 1023 - 52 - 2; m2 = (1ull << 52) | ieee_mant; }
    const bool accept = (m2 & 1ull) == 0;
    const uint64_t mv = 4ull * m2;
    const unsigned mm_shift = (ieee_mant != 0 || ieee_exp <= 1) ? 1u : 0u;
    uint64_t vr, vp, vm; int e10;
    bool vm_tz = false, vr_tz = false;
    if (e2 >= 0) {
        const int q = repr_log10pow2(e2) - (e2 > 3 ? 1 : 0);
        e10 = q;
        const int k = REPR_POW5_INV_BITCOUNT + repr_pow5bits(q) - 1, i = -e2 + q + k;
        const uint64_t* mul = tab + 2 * q;
        vr = repr_mulshift(mv, mul, i); vp = repr_mulshift(mv + 2ull, mul, i); vm = repr_mulshift(mv - 1ull - mm_shift, mul, i);
        if (q <= 21) {
            if (mv % 5ull == 0) vr_tz = repr_pow5factor(mv) >= q;
            else if (accept) vm_tz = repr_pow5factor(mv - 1ull - mm_shift) >= q;
            else vp -= repr_pow5factor(mv + 2ull) >= q ? 1ull : 0ull;
        }
    } else {
        const int q = repr_log10pow5(-e2) - (-e2 > 1 ? 1 : 0);
        e10 = q + e2;
        const int i = -e2 - q, k = repr_pow5bits(i) - REPR_POW5_BITCOUNT, j = q - k;
        const uint64_t* mul = tab + 2 * REPR_POW5_INV_N + 2 * i;
        vr = repr_mulshift(mv, mul, j); vp = repr_mulshift(mv + 2ull, mul, j); vm = repr_mulshift(mv - 1ull - mm_shift, mul, j);
        if (q <= 1) {
            vr_tz = true;
            if (accept) vm_tz = mm_shift == 1u; else --vp;
        } else if (q < 63) {
            vr_tz = (mv & ((1ull << q) - 1ull)) == 0;
        }
    }
    int removed = 0; unsigned last = 0;
    while (vp / 10ull > vm / 10ull) {
        vm_tz &= vm % 10ull == 0;
        vr_tz &= last == 0;
        last = (unsigned)(vr % 10ull);
        vr /= 10ull; vp /= 10ull; vm /= 10ull; removed++;
    }
    if (vm_tz) {
        while (vm % 10ull == 0) {
            vr_tz &= last == 0;
            last = (unsigned)(vr % 10ull);
            vr /= 10ull; vp /= 10ull; vm /= 10ull; removed++;
        }
    }
    if (vr_tz && last == 5 && vr % 2ull == 0) last = 4;      // exactly halfway: round to even
    *digits = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5) ? 1ull : 0ull);
    *exp10 = e10 + removed;
}

// ---------------------------------------------------------------------------------------------------------
// host and device: layout.  S: anything with ch(char)
// ---------------------------------------------------------------------------------------------------------
template <class S> __host__ __device__ inline void put_repr(S& s, double x, const uint64_t* tab) {
    uint64_t bits; memcpy(&bits, &x, 8);
    const uint64_t mant = bits & ((1ull << 52) - 1ull);
    const int be = (int)((bits >> 52) & 0x7ffull);
    if (be == 0x7ff && mant) { s.ch('n'); s.ch('a'); s.ch('n'); return; }
    if (bits >> 63) s.ch('-');
    if (be == 0x7ff) { s.ch('i'); s.ch('n'); s.ch('f'); return; }
    if (be == 0 && mant == 0) { s.ch('0'); s.ch('.'); s.ch('0'); return; }
    uint64_t d; int e10;
    repr_digits(mant, be, tab, &d, &e10);
    uint64_t p = 10ull; int nd = 1;
    while (nd < 17 && d >= p) { p *= 10ull; nd++; }      // p = 10^nd (10^17 fits)
    const int decpt = e10 + nd;                          // value = 0.d1d2..dn * 10^decpt
    // digit k (0 = most significant) = (d / 10^(nd - 1 - k)) % 10: walk a divisor down instead of storing the digits
    uint64_t div = p / 10ull;
    if (decpt > -4 && decpt <= 16) {
        if (decpt <= 0) { s.ch('0'); s.ch('.'); for (int k = 0; k < -decpt; k++) s.ch('0'); }
        for (int k = 0; k < nd; k++) {
            if (k == decpt && k > 0) s.ch('.');
            s.ch((char)('0' + (unsigned)((d / div) % 10ull))); div /= 10ull;
        }
        if (decpt >= nd) { for (int k = nd; k < decpt; k++) s.ch('0'); s.ch('.'); s.ch('0'); }
    } else {
        for (int k = 0; k < nd; k++) {
            if (k == 1) s.ch('.');
            s.ch((char)('0' + (unsigned)((d / div) % 10ull))); div /= 10ull;
        }
        int e = decpt - 1;
        s.ch('e');
        if (e < 0) { s.ch('-'); e = -e; } else s.ch('+');
        if (e >= 100) s.ch((char)('0' + e / 100));
        s.ch((char)('0' + (e / 10) % 10)); s.ch((char)('0' + e % 10));
    }
}
