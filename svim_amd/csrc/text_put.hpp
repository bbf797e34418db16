// text_put.hpp - the small text emitters the line writers share (vcf.hip, bed.hip), host and device: decimal integers, literal strings, and the two-digit rounding
// of get_std_span() / get_std_pos().  S is a sink: anything with ch(char).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

// round(x, 2) as CPython does it (correctly rounded, half-even on the exact binary value) -> hundredths.  |x| < 1e10: the 53-bit mantissa times 100 fits into
// 64 bits and the binary exponent is negative, so the product is shifted right and the remainder decides.  false: not representable here (inf, >= 1e10)
__host__ __device__ inline bool std_hundredths(double x, bool* neg, unsigned long long* q_out) {
    unsigned long long bits; memcpy(&bits, &x, 8);
    *neg = (bits >> 63) != 0;
    const int be = (int)((bits >> 52) & 0x7ff);
    unsigned long long m = bits & ((1ull << 52) - 1);
    if (be == 0x7ff) return false;
    int e;                                               // x = m * 2^e
    if (be == 0) e = -1074; else { m |= 1ull << 52; e = be - 1075; }
    if (e >= -18) return false;                          // |x| >= 2^52 * 2^-18 = 2^34 > 1e10 (normal numbers)
    const unsigned long long p = m * 100ull;             // < 2^60
    const int sh = -e;                                   // >= 19
    if (sh >= 62) { *q_out = 0; return true; }           // p / 2^62 < 1/4
    unsigned long long q = p >> sh;
    const unsigned long long rem = p & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (q & 1))) q++;
    if (q >= 1000000000000ull) return false;             // >= 1e10
    *q_out = q;
    return true;
}

template <class S> __host__ __device__ inline void put_str(S& s, const char* t) { for (; *t; t++) s.ch(*t); }
template <class S> __host__ __device__ inline void put_u64(S& s, unsigned long long v) {
    unsigned long long d0 = 0; unsigned d1 = 0; int n = 0;          // decimal digits as nibbles, least significant first (no array: stays in registers)
    do {
        const unsigned long long q = v / 10ull; const unsigned r = (unsigned)(v - q * 10ull);
        if (n < 16) d0 |= (unsigned long long)r << (4 * n); else d1 |= r << (4 * (n - 16));
        n++; v = q;
    } while (v);
    for (int k = n - 1; k >= 0; k--) s.ch((char)('0' + (k < 16 ? (unsigned)((d0 >> (4 * k)) & 15ull) : ((d1 >> (4 * (k - 16))) & 15u))));
}
template <class S> __host__ __device__ inline void put_i64(S& s, long long v) {
    if (v < 0) { s.ch('-'); put_u64(s, 0ull - (unsigned long long)v); } else put_u64(s, (unsigned long long)v);
}
// get_std_span() / get_std_pos() (src/svim/SVCandidate.py:39-50) as str.format prints it; false: value outside the stated bound
template <class S> __host__ __device__ inline bool put_std(S& s, double x) {
    if (x != x || x == 0.0) { s.ch('.'); return true; }
    bool neg; unsigned long long q;
    if (!std_hundredths(x, &neg, &q)) { s.ch('.'); return false; }
    if (neg) s.ch('-');
    const unsigned long long ip = q / 100ull; const unsigned fp = (unsigned)(q - ip * 100ull);
    put_u64(s, ip); s.ch('.');
    s.ch((char)('0' + fp / 10));
    if (fp % 10) s.ch((char)('0' + fp % 10));
    return true;
}
