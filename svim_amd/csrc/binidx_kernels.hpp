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
inline int binidx_sort_end_bit(long long n_groups, int key_shift = BINIDX_KEY_SHIFT) { return key_shift + std::max(1, svx_ceil_log2(n_groups + 1)); }

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
                                                 uint32_t* group_first_bin, int key_shift) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == n_chunks) bin_first[n_bins] = (uint32_t)n_chunks;
    else if (p < n_chunks && bh[p] && binpos[p] < n_bins) bin_first[binpos[p]] = (uint32_t)p;
    if (p > n_groups) return;
    long long lo = 0, hi = n_chunks;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)(key[mid] >> key_shift) >= p) hi = mid; else lo = mid + 1; }
    group_first_bin[p] = (uint32_t)binpos[lo];
}
template <class A> void binidx_launch_bins(hipStream_t st, long long n_chunks, long long n_bins, long long n_groups, const uint64_t* key, const int32_t* bh, const int64_t* binpos,
                                          uint32_t* bin_first, uint32_t* group_first_bin, int key_shift = BINIDX_KEY_SHIFT) {
    k_binidx_bins<A><<<BINIDX_GRID(std::max(n_chunks, n_groups) + 1), BINIDX_T, 0, st>>>(n_chunks, n_bins, n_groups, key, bh, binpos, bin_first, group_first_bin, key_shift);
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
// ---- the CSI form (binidx_core.hpp; svim_amd/csi.py): a depth per file, a loffset per bin, no linear index.  The accessor also answers depth(t), the depth
// of the file group t lies in.  The keys are binidx_csi_key at the largest depth of the call (key_shift): the bin field of a deeper file is wider than 16 bits.
//   k_binidx_run_max*    a segmented inclusive running maximum of interval(j).end over the rows, restarting at every group's first row: the (head, value)
//                        aggregate of every tile of BINIDX_RMAX_TILE rows, an exclusive scan of those aggregates by one workgroup, the tiles scanned again
//                        behind their carry (the pattern of scan.hpp).  The last entry of a group, its largest end, also goes to gmax[group]
//   k_binidx_bin_loff    a bin head of the sorted chunks: the vbeg of the group's first row whose running maximum lies beyond the bin's first coordinate,
//                        by bisection (the running maximum does not decrease inside a group)
//   k_binidx_sizes_csi, k_binidx_ser_chunks_csi, k_binidx_ser_group_csi   the part of a group in its CSI layout
// k_binidx_max_end and k_binidx_linear are not launched on this route: an end can pass 2^31 here, and a 2^40 coordinate would mean a 512 MB linear index.
#define BINIDX_RMAX_ITEMS 8
#define BINIDX_RMAX_TILE (BINIDX_T * BINIDX_RMAX_ITEMS)
#define BINIDX_SEG_NONE (-0x7fffffffffffffffll - 1)

struct BinIdxSeg { long long v; int f; };                   // a stretch of rows: does a group start in it, and the running maximum at its last row
__device__ __forceinline__ BinIdxSeg binidx_seg_join(const BinIdxSeg& a, const BinIdxSeg& b) {          // a in front of b
    BinIdxSeg r; r.v = (b.f || b.v > a.v) ? b.v : a.v; r.f = a.f | b.f;
    return r;
}
// one aggregate per thread over a workgroup of BINIDX_T threads -> what lies in front of the thread; *total: the whole workgroup.  shv, shf: BINIDX_T / 64 entries
__device__ __forceinline__ BinIdxSeg binidx_seg_block_excl(BinIdxSeg in, long long* shv, int* shf, BinIdxSeg* total) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        BinIdxSeg u; u.v = __shfl_up(in.v, s, 64); u.f = __shfl_up(in.f, s, 64);
        if (lane_id() >= s) in = binidx_seg_join(u, in);
    }
    const int w = (int)(threadIdx.x >> 6);
    __syncthreads();                                              // (the arrays may still be read from the trip before)
    if (lane_id() == 63) { shv[w] = in.v; shf[w] = in.f; }
    __syncthreads();
    BinIdxSeg ex; ex.v = __shfl_up(in.v, 1, 64); ex.f = __shfl_up(in.f, 1, 64);
    if (lane_id() == 0) { ex.v = BINIDX_SEG_NONE; ex.f = 0; }
    BinIdxSeg base{BINIDX_SEG_NONE, 0}, sum{BINIDX_SEG_NONE, 0};
#pragma unroll
    for (int k = 0; k < BINIDX_T / 64; k++) { const BinIdxSeg x{shv[k], shf[k]}; if (k < w) base = binidx_seg_join(base, x); sum = binidx_seg_join(sum, x); }
    *total = sum;
    return binidx_seg_join(base, ex);
}
// thread t owns rows lo + t * ITEMS .. + ITEMS - 1 of the tile: x[k] = the running aggregate of its own rows up to k; -> the aggregate of all of them
template <class A> __device__ __forceinline__ BinIdxSeg binidx_rmax_load(const A& a, long long lo, long long n, BinIdxSeg (&x)[BINIDX_RMAX_ITEMS]) {
    const long long j0 = lo + (long long)threadIdx.x * BINIDX_RMAX_ITEMS;
    long long gprev = (j0 > 0 && j0 < n) ? a.group(j0 - 1) : -1;
    BinIdxSeg run{BINIDX_SEG_NONE, 0};
#pragma unroll
    for (int k = 0; k < BINIDX_RMAX_ITEMS; k++) {
        const long long j = j0 + k;
        BinIdxSeg e{BINIDX_SEG_NONE, 0};
        if (j < n) { const long long g = a.group(j); e.f = (j == 0 || g != gprev) ? 1 : 0; e.v = a.interval(j).end; gprev = g; }
        run = binidx_seg_join(run, e);
        x[k] = run;
    }
    return run;
}
template <class A> __global__ __launch_bounds__(BINIDX_T) void k_binidx_run_max_tiles(A a, long long n_rows, long long* tile_v, int* tile_f) {
    __shared__ long long shv[BINIDX_T / 64]; __shared__ int shf[BINIDX_T / 64];
    BinIdxSeg x[BINIDX_RMAX_ITEMS], total;
    const BinIdxSeg mine = binidx_rmax_load(a, (long long)blockIdx.x * BINIDX_RMAX_TILE, n_rows, x);
    (void)binidx_seg_block_excl(mine, shv, shf, &total);
    if (threadIdx.x == 0) { tile_v[blockIdx.x] = total.v; tile_f[blockIdx.x] = total.f; }
}
// the tiles' aggregates -> what lies in front of every tile, in place (one workgroup walks them and carries)
template <class A> __global__ __launch_bounds__(BINIDX_T) void k_binidx_run_max_carry(long long n_tiles, long long* tile_v, int* tile_f) {
    __shared__ long long shv[BINIDX_T / 64]; __shared__ int shf[BINIDX_T / 64];
    BinIdxSeg carry{BINIDX_SEG_NONE, 0};
    for (long long lo = 0; lo < n_tiles; lo += BINIDX_T) {
        const long long i = lo + threadIdx.x;
        BinIdxSeg mine{BINIDX_SEG_NONE, 0}, total;
        if (i < n_tiles) { mine.v = tile_v[i]; mine.f = tile_f[i]; }
        const BinIdxSeg ex = binidx_seg_join(carry, binidx_seg_block_excl(mine, shv, shf, &total));
        if (i < n_tiles) { tile_v[i] = ex.v; tile_f[i] = ex.f; }
        carry = binidx_seg_join(carry, total);
    }
}
// tile_v: what k_binidx_run_max_carry left (null: the rows are one tile)
template <class A> __global__ __launch_bounds__(BINIDX_T) void k_binidx_run_max(A a, long long n_rows, long long n_groups, const long long* tile_v, int64_t* rmax, int64_t* gmax) {
    __shared__ long long shv[BINIDX_T / 64]; __shared__ int shf[BINIDX_T / 64];
    BinIdxSeg x[BINIDX_RMAX_ITEMS], total;
    const long long lo = (long long)blockIdx.x * BINIDX_RMAX_TILE;
    const BinIdxSeg mine = binidx_rmax_load(a, lo, n_rows, x);
    BinIdxSeg front = binidx_seg_block_excl(mine, shv, shf, &total);
    if (tile_v) { const BinIdxSeg c{tile_v[blockIdx.x], 0}; front = binidx_seg_join(c, front); }
#pragma unroll
    for (int k = 0; k < BINIDX_RMAX_ITEMS; k++) {
        const long long j = lo + (long long)threadIdx.x * BINIDX_RMAX_ITEMS + k;
        if (j >= n_rows) break;
        const long long v = binidx_seg_join(front, x[k]).v;
        rmax[j] = v;
        const long long g = a.group(j);
        if ((j + 1 == n_rows || a.group(j + 1) != g) && g >= 0 && g < n_groups) gmax[g] = v;
    }
}
// rmax[0 .. n_rows) and gmax[0 .. n_groups) (cleared first: a group without rows keeps 0); tiles: scratch of tiles * 12 bytes (any size when the rows are one tile)
template <class A> int binidx_launch_run_max(hipStream_t st, const A& a, long long n_rows, long long n_groups, int64_t* rmax, int64_t* gmax, long long* tile_v, int* tile_f) {
    const long long tiles = (n_rows + BINIDX_RMAX_TILE - 1) / BINIDX_RMAX_TILE;
    HIPCHK(hipMemsetAsync(gmax, 0, (size_t)n_groups * 8, st));
    if (tiles > 1) {
        k_binidx_run_max_tiles<A><<<(unsigned)tiles, BINIDX_T, 0, st>>>(a, n_rows, tile_v, tile_f);
        k_binidx_run_max_carry<A><<<1, BINIDX_T, 0, st>>>(tiles, tile_v, tile_f);
    }
    k_binidx_run_max<A><<<(unsigned)tiles, BINIDX_T, 0, st>>>(a, n_rows, n_groups, tiles > 1 ? tile_v : nullptr, rmax, gmax);
    HIPCHK(hipGetLastError());
    return SVX_OK;
}
template <class A> __global__ void k_binidx_bin_loff(A a, long long n_chunks, long long n_bins, long long n_rows, int key_shift, const uint64_t* key, const int32_t* bh, const int64_t* binpos,
                                                     const int64_t* rmax, uint64_t* bin_loff, int* err, int err_bit) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_chunks || !bh[p]) return;
    const long long q = binpos[p], t = (long long)(key[p] >> key_shift);
    if (q < 0 || q >= n_bins || !a.group_live(t)) return;
    const int64_t start = binidx_bin_start((uint32_t)(key[p] & ((1ull << key_shift) - 1ull)), a.depth(t));
    long long lo = a.first(t); const long long end = a.last(t);
    if (lo < 0 || end > n_rows || lo >= end) { atomicOr(err, err_bit); return; }
    long long hi = end;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (rmax[mid] > start) hi = mid; else lo = mid + 1; }
    if (lo >= end) { atomicOr(err, err_bit); return; }              // (cannot happen: a row of this bin ends beyond the bin's start)
    bin_loff[q] = a.vbeg(lo);
}
template <class A> __global__ void k_binidx_sizes_csi(A a, long long n_groups, const uint32_t* group_first_bin, const uint32_t* bin_first, int64_t* tsz) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_groups) return;
    long long sz = 0;
    if (t < n_groups) {
        if (a.last(t) <= a.first(t)) sz = BINIDX_CSI_EMPTY_PART_BYTES;
        else if (a.group_live(t)) {
            const uint32_t b0 = group_first_bin[t], b1 = group_first_bin[t + 1];
            sz = binidx_csi_part_bytes((long long)b1 - b0, (long long)bin_first[b1] - bin_first[b0]);
        }
    }
    tsz[t] = sz;
}
template <class A> __global__ void k_binidx_ser_chunks_csi(A a, long long n_chunks, int key_shift, const uint64_t* key, const uint32_t* val, const int32_t* bh, const int64_t* binpos,
                                                           const uint32_t* bin_first, const uint32_t* group_first_bin, const uint32_t* chunk_rec, const uint64_t* bin_loff, BinIdxOut o) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_chunks) return;
    const long long t = (long long)(key[p] >> key_shift);
    if (!a.group_live(t)) return;
    const uint32_t cq = val[p];
    const long long j0 = chunk_rec[cq], j1 = (long long)chunk_rec[cq + 1] - 1;
    const long long q = binpos[p] + bh[p] - 1, fb = group_first_bin[t];
    const long long at = a.part_off(t) + 4 + 16 * (q - fb) + 16 * ((long long)bin_first[q] - bin_first[fb]);
    if (bh[p]) {
        uint8_t* d = binidx_at(o, at, 16);
        if (d) { binidx_put32(d, (uint32_t)(key[p] & ((1ull << key_shift) - 1ull))); binidx_put64(d + 4, bin_loff[q]); binidx_put32(d + 12, bin_first[q + 1] - bin_first[q]); }
    }
    uint8_t* d = binidx_at(o, at + 16 + 16 * (p - (long long)bin_first[q]), 16);
    if (d) { binidx_put64(d, a.vbeg(j0)); binidx_put64(d + 8, a.vend(j1)); }
}
// one lane per group: n_bin and the pseudo-bin (a group without rows keeps the four zero bytes the index was cleared to)
template <class A> __global__ void k_binidx_ser_group_csi(A a, long long n_groups, const uint32_t* group_first_bin, const uint32_t* bin_first, BinIdxOut o) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_groups) return;
    const long long j0 = a.first(t), j1 = a.last(t);
    if (j1 <= j0 || !a.group_live(t)) return;
    const long long base = a.part_off(t);
    const long long nb = (long long)group_first_bin[t + 1] - group_first_bin[t], nc = (long long)bin_first[group_first_bin[t + 1]] - bin_first[group_first_bin[t]];
    uint8_t* d = binidx_at(o, base, 4);
    if (d) binidx_put32(d, (uint32_t)(nb + 1));
    d = binidx_at(o, base + 4 + 16 * nb + 16 * nc, 48);
    if (d) {
        binidx_put32(d, binidx_csi_pseudo_bin(a.depth(t))); binidx_put64(d + 4, 0ull); binidx_put32(d + 12, 2u); binidx_put64(d + 16, a.vbeg(j0)); binidx_put64(d + 24, a.vend(j1 - 1));
        binidx_put64(d + 32, a.n_mapped(t)); binidx_put64(d + 40, a.n_unmapped(t));
    }
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
