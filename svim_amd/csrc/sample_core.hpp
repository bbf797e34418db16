// sample_core.hpp - how many words of the seed(1524) stream one random.sample(range(n), 100) of the pool method (101 <= n <= 1045) consumes from a given
// start: the per-start walk and the backward sweep that gives the same number for every start of a window at once.  One source for the kernels of
// cluster.hip (k_sample_tables, k_sample_sweep) and for svx_sample_used_host (sample_host.cpp), as textindex_core.hpp is for the tabix index.
//
// Draw i = 0 .. 99 has the bound n - i and k_i = bit_length(n - i) (Random._randbelow_with_getrandbits); a word w is accepted iff (w >> (32 - k_i)) < n - i.
// Every word examined moves the position on by one, an accepted word moves the state i on by one, the walk ends in state 100.  With
//     T[s][100] = 0,    T[s][i] = 1 + T[s + 1][i + accepted(w_s, i)]    (i < 100)
// T[s][i] is the number of words a walk in state i at position s still consumes, and used(s) = T[s][0] is what the walk from s counts: the recurrence is the
// walk read backwards, one word at a time.  An entry is exact as soon as it is not SAMPLE_INVALID, whatever the sweep started from.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SAMPLE_HD __host__ __device__ __forceinline__
#else
#define SAMPLE_HD inline
#endif

#define SAMPLE_DRAWS 100
#define SAMPLE_SWEEP_C 512                   /* starts of a window one sweep covers */
#define SAMPLE_SWEEP_M 320                   /* words behind its last start a sweep begins at.  Every bound accepts with probability > 1/2; the longest walks are
                                                those of n = 2^k + 100 (all hundred bounds just above 2^k: mean 182 words, sigma 12), so 320 is 11 sigma out.
                                                A longer walk only takes the per-start walk; the table does not depend on this number */
#define SAMPLE_INVALID 0x40000000u           /* T >= this: the walk has not reached state 100 inside the swept words; stays so under the +1 of a sweep */
#define SAMPLE_NONE 0xffffu                  /* table entry of a walk that leaves the stream or uses >= 65535 words */
#define SAMPLE_NO_WORD 0xffffffffu           /* a word no state accepts: (w >> (32 - k)) = 2^k - 1 >= bound */

// (w >> (32 - k)) < bound  <=>  w < bound << (32 - k): one compare per state and word.  32 - k = clz(bound); bound < 2^k, so the shift does not overflow.
// States from 100 on accept nothing.
SAMPLE_HD uint32_t sample_threshold(int n, int state) {
    if (state >= SAMPLE_DRAWS) return 0u;
    const uint32_t bound = (uint32_t)(n - state);
    return bound << __builtin_clz(bound);
}
// T[s][i] from own = T[s + 1][i] and next = T[s + 1][i + 1]; inc: 1 for a state below 100, 0 for state 100 (and the unused ones above it)
SAMPLE_HD uint32_t sample_sweep_step(uint32_t own, uint32_t next, uint32_t word, uint32_t threshold, uint32_t inc) {
    return (word < threshold ? next : own) + inc;
}
// where the sweep of the starts [.., end) begins: `margin` words behind the last start, inside the stream
SAMPLE_HD long long sample_sweep_top(long long end, int margin, long long cap) { return end + margin < cap ? end + margin : cap; }

// the walk from `start`: word_at(pos) is only asked for pos < cap
template <class WordAt> SAMPLE_HD uint16_t sample_walk(int n, long long start, long long cap, WordAt word_at) {
    long long pos = start;
    uint32_t bound = (uint32_t)n;
    for (int i = 0; i < SAMPLE_DRAWS; i++, bound--) {
        const int k = 32 - __builtin_clz(bound);                  // Random._randbelow_with_getrandbits: k = bound.bit_length()
        for (;;) {
            if (pos >= cap) return (uint16_t)SAMPLE_NONE;
            const uint32_t word = word_at(pos);
            pos++;
            if ((word >> (32 - k)) < bound) break;
        }
    }
    const long long used = pos - start;
    return used < SAMPLE_NONE ? (uint16_t)used : (uint16_t)SAMPLE_NONE;
}

#ifndef __HIPCC__
// The table of the window [lo, lo + width) as k_sample_sweep makes it, with plain loops over the 101 states: chunks of `chunk` starts, each swept from
// `margin` words behind its end; what the sweep leaves invalid is walked.
inline void sample_sweep_host(const uint32_t* stream, long long cap, int n, long long lo, int width, int chunk, int margin, uint16_t* out) {
    uint32_t thr[SAMPLE_DRAWS + 1], T[SAMPLE_DRAWS + 2];
    for (int i = 0; i <= SAMPLE_DRAWS; i++) thr[i] = sample_threshold(n, i);
    auto word_at = [&](long long p) { return stream[p]; };
    for (int b = 0; b < width; b += chunk) {
        const int e = b + chunk < width ? b + chunk : width;
        const long long top = sample_sweep_top(lo + e, margin, cap);
        for (int i = 0; i < SAMPLE_DRAWS; i++) T[i] = SAMPLE_INVALID;
        T[SAMPLE_DRAWS] = T[SAMPLE_DRAWS + 1] = 0;
        for (int s = b; s < e; s++) out[s] = (uint16_t)SAMPLE_NONE;
        for (long long s = top - 1; s >= lo + b; s--) {
            for (int i = 0; i < SAMPLE_DRAWS; i++) T[i] = sample_sweep_step(T[i], T[i + 1], stream[s], thr[i], 1u);       // ascending: T[i + 1] is still T[s + 1][i + 1]
            if (s < lo + e && T[0] < SAMPLE_INVALID) out[s - lo] = (uint16_t)T[0];
        }
        for (int s = b; s < e; s++) if (out[s] == SAMPLE_NONE) out[s] = sample_walk(n, lo + s, cap, word_at);
    }
}
#endif
