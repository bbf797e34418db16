// bamsort_core.hpp - the coordinate order of BAM records and the checks a record must pass before it is sorted: one source for the host build
// (bamsort_host.cpp: svx_bam_sort_host) and the kernels (bamsort.hip).  The rule in words: svim_amd/bamsort.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSORT_FN __host__ __device__ __forceinline__
#else
#define BSORT_FN static inline
#endif

#define BSORT_BLOCK 65280                    /* stream bytes per BGZF block of the output (deflate_core.hpp: DEF_BLOCK) */
#define BSORT_MIN_BLOCK_SIZE 32u             /* the fixed fields of a record behind its block_size field */
enum { BSORT_BAD_SIZE = 1, BSORT_BAD_TID = 2, BSORT_BAD_POS = 4 };

// what is wrong with a record (0: nothing)
BSORT_FN int bsort_check(int32_t tid, int32_t pos, uint32_t block_size, int32_t n_ref) {
    return (block_size < BSORT_MIN_BLOCK_SIZE ? BSORT_BAD_SIZE : 0) | (tid < -1 || tid >= n_ref ? BSORT_BAD_TID : 0) | (pos < -1 ? BSORT_BAD_POS : 0);
}
// bits that hold every reference id and n_ref itself (the place of refID = -1: behind every reference)
BSORT_FN int bsort_tid_bits(int32_t n_ref) { int b = 1; while (b < 31 && (1ll << b) <= (long long)n_ref) b++; return b; }
// (uint32(refID), uint32(pos + 1), flag & 16) compacted into one word that compares the same way for records that passed bsort_check: refID = -1 becomes n_ref
// (the largest), pos + 1 lies in [0, 2^31], the strand bit is the lowest.  33 + bsort_tid_bits(n_ref) <= 64 bits are used.
BSORT_FN uint64_t bsort_key(int32_t tid, int32_t pos, uint32_t flag, int32_t n_ref) {
    const uint64_t t = tid < 0 ? (uint64_t)(uint32_t)n_ref : (uint64_t)(uint32_t)tid;
    return (t << 33) | ((uint64_t)(uint32_t)(pos + 1) << 1) | ((flag >> 4) & 1u);
}
BSORT_FN int bsort_key_bits(int32_t n_ref) { return 33 + bsort_tid_bits(n_ref); }
// the status of a stream whose records showed the union `bad` of bsort_check: SVX_E_ARG (-3) before SVX_E_RANGE (-10)
BSORT_FN int bsort_status(int bad) { return (bad & (BSORT_BAD_SIZE | BSORT_BAD_TID)) ? -3 : (bad & BSORT_BAD_POS) ? -10 : 0; }
