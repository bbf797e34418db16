// crc32_wave.hpp - CRC32 (the gzip polynomial) of a byte range by one wavefront: the arithmetic of k_crc32 (bamdev.hip, which compares the result with a BGZF
// trailer) as a device function, so that the writer of BGZF blocks (textgz.hip, which stores it) runs the same code.
// 4 KiB per round: lane l runs the table-driven byte recurrence over its 64 bytes of the round from register 0 (the lanes of a wave read one contiguous 4 KiB),
// the 64 registers are combined pairwise in six levels - register(A || B) = shift(register(A), |B|) ^ register(B), the shift by 2^j zero bytes being a fixed
// 32 x 32 matrix over GF(2) - and the rounds are chained the same way.  The range is right-aligned in its rounds (leading zero bytes leave a zero register
// alone); the initial value 0xffffffff enters at the end as shift(0xffffffff, len).
#pragma once
#include "common.hpp"

#define CRC_POW 17                                  /* shift matrices for 2^0 .. 2^16 zero bytes */
typedef uint32_t __attribute__((aligned(1))) crc_u32_unaligned;
struct CrcTables { uint32_t T[256], T1[256], T2[256], T3[256]; };        // T: one byte; T1..T3: the same byte followed by 1..3 zero bytes (a word takes one round of look-ups)

__device__ __forceinline__ uint32_t crc_apply(const uint32_t* __restrict__ m, uint32_t x) {       // m: 32 words, wave-uniform address
    uint32_t o = 0;
#pragma unroll
    for (int bit = 0; bit < 32; bit++) o ^= m[bit] & (0u - ((x >> bit) & 1u));
    return o;
}
// fills the tables in LDS (one wave per workgroup; every lane calls it)
__device__ __forceinline__ void crc32_wave_tables(CrcTables& S) {
    const int lane = lane_id();
    for (int e = lane; e < 256; e += 64) {
        uint32_t c = (uint32_t)e;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        S.T[e] = c;
    }
    __syncthreads();
    for (int e = lane; e < 256; e += 64) {
        const uint32_t c1 = S.T[S.T[e] & 255u] ^ (S.T[e] >> 8), c2 = S.T[c1 & 255u] ^ (c1 >> 8), c3 = S.T[c2 & 255u] ^ (c2 >> 8);
        S.T1[e] = c1; S.T2[e] = c2; S.T3[e] = c3;
    }
    __syncthreads();
}
// CRC32 of base[0 .. len), the same value in every lane.  shift: the CRC_POW matrices of crc_shift_matrices (device memory)
__device__ __forceinline__ uint32_t crc32_wave(const uint8_t* base, long long len, const uint32_t* __restrict__ shift, const CrcTables& S) {
    const int lane = lane_id();
    const long long rounds = (len + 4095) >> 12, pad = (rounds << 12) - len;
    uint32_t acc = 0;
    for (long long r = 0; r < rounds; r++) {
        const long long off = (r << 12) + (long long)lane * 64 - pad;            // where my 64 bytes start in the range (negative: virtual zero bytes)
        uint32_t reg = 0;
        if (off >= 0) {
            const crc_u32_unaligned* w = reinterpret_cast<const crc_u32_unaligned*>(base + off);
            uint32_t x[16];
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = w[k];
#pragma unroll
            for (int k = 0; k < 16; k++) {
                reg ^= x[k];
                reg = S.T3[reg & 255u] ^ S.T2[(reg >> 8) & 255u] ^ S.T1[(reg >> 16) & 255u] ^ S.T[reg >> 24];
            }
        } else if (off > -64) {
            for (long long i = 0; i < off + 64; i++) reg = S.T[(reg ^ base[i]) & 255u] ^ (reg >> 8);
        }
        // six levels: the last lane of every group of 2, 4, ... 64 holds the register of its group's bytes
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const uint32_t left = (uint32_t)__shfl_up((int)reg, 1 << j, 64);
            const uint32_t joined = crc_apply(shift + 32 * (6 + j), left) ^ reg;
            if ((lane & ((2 << j) - 1)) == (2 << j) - 1) reg = joined;
        }
        acc = crc_apply(shift + 32 * 12, acc) ^ (uint32_t)__builtin_amdgcn_readlane((int)reg, 63);
    }
    uint32_t init = 0xffffffffu;
    for (int j = 0; j < CRC_POW; j++) if ((len >> j) & 1) init = crc_apply(shift + 32 * j, init);
    return ~(acc ^ init);
}
// the shift matrices: column `bit` of matrix j = the register that 1 << bit becomes after 2^j zero bytes
static inline void crc_shift_matrices(uint32_t (*m)[32]) {
    uint32_t T[256];
    for (uint32_t e = 0; e < 256; e++) { uint32_t c = e; for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; T[e] = c; }
    for (int bit = 0; bit < 32; bit++) { const uint32_t r = 1u << bit; m[0][bit] = T[r & 255u] ^ (r >> 8); }
    for (int j = 1; j < CRC_POW; j++)
        for (int bit = 0; bit < 32; bit++) { uint32_t o = 0; for (int k = 0; k < 32; k++) if ((m[j - 1][bit] >> k) & 1u) o ^= m[j - 1][k]; m[j][bit] = o; }
}
