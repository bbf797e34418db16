// binidx_kernels.hpp - the phases of a binning index (a .tbi: textindex.hip, a .bai: bamindex.hip) behind the row table, written once (gfx950).  The scheme
// and the layout: binidx_core.hpp; the same part written row after row on the host: binidx_host.hpp.
// An index instantiates every kernel with its row accessor A, a plain struct of device pointers whose members answer, for a row j (rows are in file order, a
// group's rows contiguous; a group is a contig of a .tbi, a reference of a .bai):
//   group(j)  interval(j) -> BinIdxInterval  vbeg(j)  vend(j): the virtual offset where a chunk whose last row is j ends
//   live(j): does the row's group get bytes (the status of the file in a .tbi, always in a .bai)
// and for a group t:
//   first(t), last(t): its rows [first, last)   part_off(t): where its part starts in the blob   n_mapped(t), n_unmapped(t): the counts of its pseudo-bin
//   group_live(t): live() of its rows, asked of the group (the per-group kernels ask it, as they did before they were shared)
// The template argument also keeps the kernels of the two indexes apart in a kernel trace.  What the caller has made before: chunk_rec (first row of every
// chunk in file order, n_chunks + 1 entries) and the keys binidx_key(group, bin) of the chunks with the chunk number as value, sorted stably.
//   k_binidx_bin_heads   a sorted chunk: does a bin start here (the caller scans the marks into binpos)
//   k_binidx_bins        a sorted chunk: first chunk of its bin; a group: its first bin by bisection of the sorted keys (a group without rows: an empty range)
//   k_binidx_max_end     a row: atomicMax into its group's largest end
//   k_binidx_sizes       a group: n_intv and the bytes of its part (the caller scans them into loff and toff)
//   k_binidx_linear      a row: atomicMin(vbeg) into its windows - its own lane for one window, the whole wave for a row of many
//   k_binidx_ser_chunks  a sorted chunk: bin header and (vbeg, vend) at their offsets
//   k_binidx_ser_group   one wave per group: n_bin, the pseudo-bin, n_intv, the linear index with its empty slots filled from behind (a reverse scan in tiles of 64)
// Every store into the index goes through binidx_at: a layout that disagrees with its sizes raises a flag, it does not write somewhere else.
#pragma once
#include "common.hpp"
#include "binidx_core.hpp"
#include <algorithm>

#define BINIDX_T 256
#define BINIDX_GRID(n) (unsigned)(((long long)(n) + BINIDX_T - 1) / BINIDX_T)
#define BINIDX_KEY_SHIFT 16                 /* sort key of a chunk: the bin (< 37 450 < 2^16) in the low bits, the group above: no radix pass over bits that are zero in every key */

BINIDX_HD uint64_t binidx_key(uint64_t group, uint32_t bin) { return (group << BINIDX_KEY_SHIFT) | bin; }
inline int binidx_sort_end_bit(long long n_groups) { return BINIDX_KEY_SHIFT + std::max(1, svx_ceil_log2(n_groups + 1)); }

struct BinIdxOut { uint8_t* blob; long long n_blob; int* err; int err_bit; };
__device__ __forceinline__ uint8_t* binidx_at(const BinIdxOut& o, long long off, long long len) {
    if (off < 0 || off + len > o.n_blob) { atomicOr(o.err, o.err_bit); return nullptr; }
    return o.blob + off;
}

// (A is not read here or in k_binidx_bins: it is what names the kernel after its index in a kernel trace - keep it)
template <class A> __global__ void k_binidx_bin_heads(long long n_chunks, const uint64_t* key, int32_t* bh) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_chunks) return;
    bh[p] = p < n_chunks && (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}
// two jobs of different lane ranges in one launch: lanes 0 .. n_chunks and lanes 0 .. n_groups.  Launched through binidx_launch_bins, which sizes the grid
template <class A> __global__ void k_binidx_bins(long long n_chunks, long long n_bins, long long n_groups, const uint64_t* key, const int32_t* bh, const int64_t* binpos, uint32_t* bin_first,
                                                 uint32_t* group_first_bin) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == n_chunks) bin_first[n_bins] = (uint32_t)n_chunks;
    else if (p < n_chunks && bh[p] && binpos[p] < n_bins) bin_first[binpos[p]] = (uint32_t)p;
    if (p > n_groups) return;
    long long lo = 0, hi = n_chunks;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)(key[mid] >> BINIDX_KEY_SHIFT) >= p) hi = mid; else lo = mid + 1; }
    group_first_bin[p] = (uint32_t)binpos[lo];
}
template <class A> void binidx_launch_bins(hipStream_t st, long long n_chunks, long long n_bins, long long n_groups, const uint64_t* key, const int32_t* bh, const int64_t* binpos,
                                          uint32_t* bin_first, uint32_t* group_first_bin) {
    k_binidx_bins<A><<<BINIDX_GRID(std::max(n_chunks, n_groups) + 1), BINIDX_T, 0, st>>>(n_chunks, n_bins, n_groups, key, bh, binpos, bin_first, group_first_bin);
}
template <class A> __global__ void k_binidx_max_end(A a, long long n_rows, int32_t* tmax) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_rows && a.live(j)) atomicMax(tmax + a.group(j), (int32_t)a.interval(j).end);          // (end <= 2^29 in a live group: the range check has passed)
}
template <class A> __global__ void k_binidx_sizes(A a, long long n_groups, const int32_t* tmax, const uint32_t* group_first_bin, const uint32_t* bin_first, int64_t* tsz, int64_t* nintv) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_groups) return;
    long long sz = 0, ni = 0;
    if (t < n_groups) {
        if (a.last(t) <= a.first(t)) sz = BINIDX_EMPTY_PART_BYTES;
        else if (a.group_live(t)) {
            ni = 1 + (((long long)tmax[t] - 1) >> 14);
            const uint32_t b0 = group_first_bin[t], b1 = group_first_bin[t + 1];
            sz = binidx_part_bytes((long long)b1 - b0, (long long)bin_first[b1] - bin_first[b0], ni);
        }
    }
    tsz[t] = sz; nintv[t] = ni;
}
template <class A> __global__ __launch_bounds__(BINIDX_T) void k_binidx_linear(A a, long long n_rows, const int64_t* loff, long long n_slots, unsigned long long* lin) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long w0 = 0, w1 = -1, base = 0; unsigned long long v = 0;
    if (j < n_rows && a.live(j)) {
        const long long t = a.group(j);
        const BinIdxInterval iv = a.interval(j);
        base = loff[t]; w0 = iv.beg >> 14; w1 = (iv.end - 1) >> 14; v = a.vbeg(j);
        if (base + w1 >= n_slots || base + w1 >= loff[t + 1]) w1 = w0 - 1;       // (cannot happen: the slots were sized by the largest end)
    }
    if (w1 == w0) atomicMin(lin + base + w0, v);
    unsigned long long many = __ballot(w1 > w0);
    while (many) {                                           // a row of many windows: the wave writes them, 64 at a time
        const int src = __ffsll((long long)many) - 1;
        many &= many - 1;
        const long long b = __shfl(base, src, 64), lo = __shfl(w0, src, 64), hi = __shfl(w1, src, 64);
        const unsigned long long vv = __shfl(v, src, 64);
        for (long long w = lo + lane_id(); w <= hi; w += 64) atomicMin(lin + b + w, vv);
    }
}
template <class A> __global__ void k_binidx_ser_chunks(A a, long long n_chunks, const uint64_t* key, const uint32_t* val, const int32_t* bh, const int64_t* binpos, const uint32_t* bin_first,
                                                       const uint32_t* group_first_bin, const uint32_t* chunk_rec, BinIdxOut o) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_chunks) return;
    const long long t = (long long)(key[p] >> BINIDX_KEY_SHIFT);
    if (!a.group_live(t)) return;
    const uint32_t cq = val[p];
    const long long j0 = chunk_rec[cq], j1 = (long long)chunk_rec[cq + 1] - 1;
    const long long q = binpos[p] + bh[p] - 1, fb = group_first_bin[t];
    const long long at = a.part_off(t) + 4 + 8 * (q - fb) + 16 * ((long long)bin_first[q] - bin_first[fb]);
    if (bh[p]) {
        uint8_t* d = binidx_at(o, at, 8);
        if (d) { binidx_put32(d, (uint32_t)(key[p] & ((1u << BINIDX_KEY_SHIFT) - 1u))); binidx_put32(d + 4, bin_first[q + 1] - bin_first[q]); }
    }
    uint8_t* d = binidx_at(o, at + 8 + 16 * (p - (long long)bin_first[q]), 16);
    if (d) { binidx_put64(d, a.vbeg(j0)); binidx_put64(d + 8, a.vend(j1)); }
}
template <class A> __global__ __launch_bounds__(64) void k_binidx_ser_group(A a, long long n_groups, const uint32_t* group_first_bin, const uint32_t* bin_first, const int64_t* loff,
                                                                            const unsigned long long* lin, BinIdxOut o) {
    const long long t = blockIdx.x;
    if (t >= n_groups) return;
    const long long j0 = a.first(t), j1 = a.last(t);
    if (j1 <= j0 || !a.group_live(t)) return;                     // (a group without rows keeps the eight zero bytes the index was cleared to)
    const long long base = a.part_off(t);
    const long long nb = (long long)group_first_bin[t + 1] - group_first_bin[t], nc = (long long)bin_first[group_first_bin[t + 1]] - bin_first[group_first_bin[t]];
    const long long ni = loff[t + 1] - loff[t];
    const long long ps = base + 4 + 8 * nb + 16 * nc;
    if (lane_id() == 0) {
        uint8_t* d = binidx_at(o, base, 4);
        if (d) binidx_put32(d, (uint32_t)(nb + 1));
        d = binidx_at(o, ps, 44);
        if (d) {
            binidx_put32(d, BINIDX_PSEUDO_BIN); binidx_put32(d + 4, 2u); binidx_put64(d + 8, a.vbeg(j0)); binidx_put64(d + 16, a.vend(j1 - 1));
            binidx_put64(d + 24, a.n_mapped(t)); binidx_put64(d + 32, a.n_unmapped(t)); binidx_put32(d + 40, (uint32_t)ni);
        }
    }
    unsigned long long carry = BINIDX_NO_SLOT;
    for (long long top = ni - 1; top >= 0; top -= 64) {                 // lane l holds window top - l: a prefix minimum over the lanes is a suffix minimum over the windows
        const long long w = top - lane_id();
        unsigned long long v = w >= 0 ? lin[loff[t] + w] : BINIDX_NO_SLOT;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { const unsigned long long u = __shfl_up(v, s, 64); if (lane_id() >= s && u < v) v = u; }
        if (carry < v) v = carry;
        if (w >= 0) { uint8_t* d = binidx_at(o, ps + 44 + 8 * w, 8); if (d) binidx_put64(d, v); }
        carry = __shfl(v, 63, 64);
    }
}
