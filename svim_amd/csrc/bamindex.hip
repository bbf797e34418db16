// bamindex.hip - the BAM index (.bai) of the file the device reader (bamdev.hip) is reading, built from the reader's own record stream (svx_bam_index*,
// include/svx.h; gfx950).  What an index says: svim_amd/bai.py; the interval and order rules: bamindex_core.hpp, the source svx_bam_index_host is built from
// as well.  This file makes the row table - append, the span kernels, the rows of a sorted file - and, at finish, the check, the first row of every
// reference, the chunk heads, header and trailer; the phases behind them (bins, sizes, the linear index, a reference's part) are those a .tbi has too:
// binidx_kernels.hpp, instantiated with BixRows.
// Replaces: samtools index after the fact (the reference's main() asks for it: "Please generate with 'samtools index'"): one more single-threaded zlib pass
// over a file whose every record this reader has already found.
// While indexing is on, every chunk the reader loads appends one row per record to a table that stays on the device:
//   k_bix_rows       one DPP row (16 lanes) per record: tid, pos, flag copied, the reference span of a placed record of up to BIX_LONG_OPS operations (the
//                    lanes share the CIGAR as k_aln_append's do, cigar_span.hpp), the virtual offset by a bisection of rec_off in the chunk's block table
//   k_bix_span_mid   the longer ones of up to BIX_GIANT_OPS operations (a long read's CIGAR: thousands of them in a chunk), one wave per record
//   k_bix_span_long  the few beyond that (a CG-tag CIGAR has no length limit), one wave per tile of 1024 operations over the whole grid
//   k_bix_end        end = beg + span, or beg + 1 (flag bit 4, no span)
// svx_bam_index_finish, on the loader's stream; counts cross to the host between the phases:
//   check      one lane per neighbour pair: the order; per row: the range, the tid
//   chunks     first row of every reference by bisection; chunk heads where (tid, bin) changes, unmapped marks; both scanned
//   sort       (tid << 16 | bin, chunk) sorted stably (svx_sort_pairs_u64_on); bin heads of the sorted list compacted, first bin of every reference by bisection
//   linear     largest end per reference, sizes, two scans; a record's windows get atomicMin(vbeg): its own lane for one window, the wave for a record of many
//   serialise  one lane per chunk and one wave per reference store every field at its offset; the wave's backward fill of the empty slots is a reverse scan
//              in tiles of 64.  Header and trailer come from the host.
// Every store into the index is checked against the index's size: a layout that disagrees with its sizes is SVX_E_STATE, not a write somewhere else.
// With fmt SVX_INDEX_CSI finish builds the uncompressed .csi of the same rows (svim_amd/csi.py): no range check; behind the references a segmented running
// maximum of the ends (binidx_launch_run_max), whose last entry per reference gives the file's depth; chunk heads, keys and the sort at that depth; in place
// of the linear phase one bisection of the running maximum per bin (k_binidx_bin_loff); the CSI serialisers.
#include "common.hpp"
#include "hostcopy.hpp"
#include "scan.hpp"
#include "cigar_span.hpp"
#include "bamindex_core.hpp"
#include "binidx_kernels.hpp"
#include "bamindex.hpp"
#include <algorithm>

#define BT BINIDX_T
#define BGRID(n) BINIDX_GRID(n)
#define BIX_LONG_OPS 4096
#define BIX_GIANT_OPS 65536
#define BIX_LONG_TILE 1024
#define BIX_LONG_BLOCKS 256
#define BIX_NPOOL 32
enum { BIXF_ORDER = 1, BIXF_RANGE = 2, BIXF_TID = 4, BIXF_LAYOUT = 8 };

struct BixCols { int32_t *tid, *pos; uint16_t* flag; int64_t* end; uint64_t* vbeg; };

// ---- append ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bix_rows(long long n, const int32_t* tid, const int32_t* pos, const uint16_t* flag, const uint64_t* cigar_off, const uint32_t* cigar,
                                                  const uint64_t* rec_off, const uint64_t* blk_start, const uint64_t* blk_vbase, long long n_blk, BixCols out, uint32_t* span,
                                                  uint32_t* long_list, unsigned long long* counters) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = (int)(threadIdx.x & 15);
    const bool in = r < n;
    uint32_t s = 0; bool is_long = false, is_giant = false;
    int t = -1, p = 0; unsigned f = 0;
    if (in) {
        t = tid[r]; p = pos[r]; f = flag[r];
        if (t >= 0) {                                                       // every placed record: an index describes the file, not what COLLECT counts
            const unsigned long long lo = cigar_off[r], hi = cigar_off[r + 1];
            if (hi > lo) { if (hi - lo > BIX_LONG_OPS) { is_long = true; is_giant = hi - lo > BIX_GIANT_OPS; } else s = span_partial(cigar, lo, hi, l, 16); }
        }
    }
    s = (uint32_t)row_sum_i32((int)s);
    if (in && l == 15) {
        out.tid[r] = t; out.pos[r] = p; out.flag[r] = (uint16_t)f; span[r] = s;
        out.vbeg[r] = bix_voff(rec_off[r], blk_start, blk_vbase, n_blk);
        // one list of n entries for both kinds: the long ones from its front, the giant ones from its back (a record is in at most one of them)
        if (is_giant) long_list[n - 1 - (long long)atomicAdd(&counters[1], 1ull)] = (uint32_t)r;
        else if (is_long) long_list[atomicAdd(&counters[0], 1ull)] = (uint32_t)r;
    }
}
__global__ __launch_bounds__(256) void k_bix_span_mid(const unsigned long long* counters, const uint32_t* long_list, const uint64_t* cigar_off, const uint32_t* cigar, uint32_t* span) {
    const unsigned long long n_mid = counters[0];
    const int lane = lane_id();
    const unsigned long long wave = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * 4;
    for (unsigned long long k = wave; k < n_mid; k += n_waves) {
        const uint32_t r = long_list[k];
        const int s = wave_sum_i32((int)span_partial(cigar, cigar_off[r], cigar_off[r + 1], lane, 64));
        if (lane == 0) span[r] = (uint32_t)s;
    }
}
__global__ __launch_bounds__(256) void k_bix_span_long(long long n, const unsigned long long* counters, const uint32_t* long_list, const uint64_t* cigar_off, const uint32_t* cigar, uint32_t* span) {
    const unsigned long long n_long = counters[1];
    const int lane = lane_id();
    const unsigned long long wave = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * 4;
    for (unsigned long long k = 0; k < n_long; k++) {
        const uint32_t r = long_list[n - 1 - (long long)k];
        const unsigned long long lo = cigar_off[r], hi = cigar_off[r + 1];
        const unsigned long long tiles = (hi - lo + BIX_LONG_TILE - 1) / BIX_LONG_TILE;
        for (unsigned long long t = wave; t < tiles; t += n_waves) {
            const unsigned long long a = lo + t * BIX_LONG_TILE, b = a + BIX_LONG_TILE < hi ? a + BIX_LONG_TILE : hi;
            const int s = wave_sum_i32((int)span_partial(cigar, a, b, lane, 64));
            if (lane == 0 && s) atomicAdd(&span[r], (uint32_t)s);
        }
    }
}
__global__ void k_bix_end(long long n, BixCols T, const uint32_t* span) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    T.end[r] = T.tid[r] >= 0 ? bix_end(T.pos[r], span[r], T.flag[r]) : (int64_t)T.pos[r] + 1;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ BinIdxInterval bix_row(const BixCols& T, long long i) { return bix_interval(T.pos[i], T.end[i]); }
__global__ void k_bix_check(long long n, int32_t n_ref, BixCols T, int* err, int check_range) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t t = T.tid[i];
    int e = t >= n_ref ? BIXF_TID : 0;
    if (i > 0 && bix_out_of_order(T.tid[i - 1], T.pos[i - 1], t, T.pos[i])) e |= BIXF_ORDER;
    if (check_range && t >= 0 && bix_row(T, i).end > BINIDX_MAX_END) e |= BIXF_RANGE;
    if (e) atomicOr(err, e);
}
// first row of every reference, and of the unplaced tail (t = n_ref): the table is in order, a negative tid is the largest as an unsigned number
__global__ void k_bix_ref_first(long long n, const int32_t* tid, int32_t n_ref, int64_t* first) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_ref) return;
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((uint32_t)tid[mid] >= (uint32_t)t) hi = mid; else lo = mid + 1; }
    first[t] = lo;
}
// depth: 0 for the five-level bins of a .bai, the depth of the file for a .csi
__device__ __forceinline__ uint32_t bix_bin(const BixCols& T, long long j, int depth) {
    const BinIdxInterval v = bix_row(T, j);
    return depth ? binidx_reg2bin_csi(v.beg, v.end, depth) : binidx_bin(v);
}
__global__ void k_bix_heads(long long n_placed, BixCols T, int32_t* bhead, int32_t* umark, int depth) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_placed) return;
    if (j == n_placed) { bhead[j] = 0; umark[j] = 0; return; }
    bhead[j] = (j == 0 || T.tid[j] != T.tid[j - 1] || bix_bin(T, j, depth) != bix_bin(T, j - 1, depth)) ? 1 : 0;
    umark[j] = (T.flag[j] & 4u) ? 1 : 0;
}
__global__ void k_bix_chunks(long long n_placed, long long n_chunks, BixCols T, const int32_t* bhead, const int64_t* bpos, uint32_t* chunk_rec, uint64_t* key, uint32_t* val, int depth) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_placed) return;
    if (j == n_placed) { chunk_rec[n_chunks] = (uint32_t)n_placed; return; }
    const long long q = bpos[j];
    if (bhead[j] && q < n_chunks) { chunk_rec[q] = (uint32_t)j; key[q] = depth ? binidx_csi_key((uint64_t)(uint32_t)T.tid[j], bix_bin(T, j, depth), depth) : binidx_key((uint64_t)(uint32_t)T.tid[j], bix_bin(T, j, 0)); val[q] = (uint32_t)q; }
}
// the placed rows as binidx_kernels.hpp reads them: a group is a reference, every one of them gets bytes
struct BixRows {
    BixCols T; long long n_rows; uint64_t v_end; const int64_t *first_row, *upos, *toff; int header_bytes, csi_depth;
    __device__ int depth(long long) const { return csi_depth; }
    __device__ long long group(long long j) const { return T.tid[j]; }
    __device__ bool live(long long) const { return true; }
    __device__ BinIdxInterval interval(long long j) const { return bix_row(T, j); }
    __device__ uint64_t vbeg(long long j) const { return T.vbeg[j]; }
    __device__ uint64_t vend(long long j) const { return j + 1 < n_rows ? T.vbeg[j + 1] : v_end; }      // the next row's start (an unplaced one's too), or the end of the data
    __device__ bool group_live(long long) const { return true; }
    __device__ long long first(long long t) const { return first_row[t]; }
    __device__ long long last(long long t) const { return first_row[t + 1]; }
    __device__ long long part_off(long long t) const { return header_bytes + toff[t]; }
    __device__ uint64_t n_unmapped(long long t) const { return (uint64_t)(upos[first_row[t + 1]] - upos[first_row[t]]); }
    __device__ uint64_t n_mapped(long long t) const { return (uint64_t)(first_row[t + 1] - first_row[t]) - n_unmapped(t); }
};

// ---------------------------------------------------------------------------------------------------------------------------------------------------------
struct BamIndex {
    int64_t n = 0, cap = 0;
    DevBuf tid, pos, flag, end, vbeg;                       // the table
    DevBuf span, long_list, counters, blk_start, blk_vbase, scan_tmp, sort_tmp, err;
    ScratchPool<BIX_NPOOL> pool{"BAM index"};
    DevBuf blob; int64_t n_blob = 0; bool have = false;
    double t_mark[6];                                       // host clock at the phase boundaries of finish (the stream is drained at each)
    double t_append = 0; int64_t n_long = 0;
    svx_bam_index_stats stats;
    BixCols cols(int64_t at) const { return BixCols{tid.as<int32_t>() + at, pos.as<int32_t>() + at, flag.as<uint16_t>() + at, end.as<int64_t>() + at, vbeg.as<uint64_t>() + at}; }
};
static inline double bix_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int bamindex_begin(BamIndex** ix) {
    if (!*ix) *ix = new BamIndex();
    BamIndex* S = *ix;
    S->n = 0; S->have = false; S->t_append = 0; S->n_long = 0;
    memset(&S->stats, 0, sizeof S->stats);
    return SVX_OK;
}
void bamindex_drop(BamIndex* S) {
    if (!S) return;
    DevBuf* all[] = {&S->tid, &S->pos, &S->flag, &S->end, &S->vbeg, &S->span, &S->long_list, &S->blk_start, &S->blk_vbase, &S->scan_tmp, &S->sort_tmp};
    for (auto* b : all) b->release();
    S->pool.release();
    S->n = S->cap = 0;
}
void bamindex_destroy(BamIndex* S) {
    if (!S) return;
    bamindex_drop(S);
    S->blob.release(); S->counters.release(); S->err.release();
    delete S;
}

int bamindex_append(BamIndex* S, const BamIndexChunk& c, hipStream_t st) {
    if (!S || c.n < 0 || c.n_blk < 1) return svx_fail(SVX_E_ARG, "BAM index: a chunk without a block table", __FILE__, __LINE__, hipSuccess);
    if (c.n == 0) return SVX_OK;
    const double t0 = bix_now();
    if (S->n + c.n >= (1ll << 31)) return svx_fail(SVX_E_CAPACITY, "BAM index: more than 2^31 records", __FILE__, __LINE__, hipSuccess);
    if (S->n + c.n > S->cap) {                               // the table grows by doubling, its rows kept
        const int64_t ncap = std::max<int64_t>(std::max<int64_t>(S->n + c.n, 2 * S->cap), 1 << 16);
        SVXCHK(S->tid.reserve((size_t)ncap * 4, true, st)); SVXCHK(S->pos.reserve((size_t)ncap * 4, true, st)); SVXCHK(S->flag.reserve((size_t)ncap * 2, true, st));
        SVXCHK(S->end.reserve((size_t)ncap * 8, true, st)); SVXCHK(S->vbeg.reserve((size_t)ncap * 8, true, st));
        S->cap = ncap;
    }
    SVXCHK(S->span.reserve((size_t)c.n * 4)); SVXCHK(S->long_list.reserve((size_t)c.n * 4)); SVXCHK(S->counters.reserve(64));
    SVXCHK(S->blk_start.reserve((size_t)c.n_blk * 8)); SVXCHK(S->blk_vbase.reserve((size_t)c.n_blk * 8));
    {
        HostCopy hc(st);
        SVXCHK(hc.h2d(S->blk_start.p, c.blk_start, (size_t)c.n_blk * 8)); SVXCHK(hc.h2d(S->blk_vbase.p, c.blk_vbase, (size_t)c.n_blk * 8));
        SVXCHK(hc.finish());
    }
    HIPCHK(hipMemsetAsync(S->counters.p, 0, 64, st));
    const BixCols T = S->cols(S->n);
    unsigned long long* cn = S->counters.as<unsigned long long>();
    k_bix_rows<<<(unsigned)((c.n * 16 + 255) / 256), 256, 0, st>>>(c.n, c.tid, c.pos, c.flag, c.cigar_off, c.cigar, c.rec_off, S->blk_start.as<uint64_t>(), S->blk_vbase.as<uint64_t>(), c.n_blk, T,
                                                                 S->span.as<uint32_t>(), S->long_list.as<uint32_t>(), cn);
    k_bix_span_mid<<<BIX_LONG_BLOCKS, 256, 0, st>>>(cn, S->long_list.as<uint32_t>(), c.cigar_off, c.cigar, S->span.as<uint32_t>());
    k_bix_span_long<<<BIX_LONG_BLOCKS, 256, 0, st>>>(c.n, cn, S->long_list.as<uint32_t>(), c.cigar_off, c.cigar, S->span.as<uint32_t>());
    k_bix_end<<<BGRID(c.n), BT, 0, st>>>(c.n, T, S->span.as<uint32_t>());
    HIPCHK(hipGetLastError());
    unsigned long long n_long[2] = {0, 0};
    SVXCHK(svx_d2h(n_long, cn, 16, st));                     // (also the point where the chunk's arrays are no longer read)
    S->n_long += (int64_t)(n_long[0] + n_long[1]);
    S->n += c.n;
    S->t_append += bix_now() - t0;
    return SVX_OK;
}

// row i = row perm[i] of another table, at the virtual offset of its place in a stream cut into blocks of block_bytes (the sorted file of bamsort.hip)
__global__ void k_bix_take(long long n, BixCols src, long long n_src, BixCols dst, const uint32_t* perm, const int64_t* rec_soff, const int64_t* coff, long long n_blk,
                           long long block_bytes, int* err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = perm[i], u = rec_soff[i], b = u / block_bytes;
    if (r >= n_src || u < 0 || b >= n_blk) { atomicOr(err, BIXF_LAYOUT); return; }
    dst.tid[i] = src.tid[r]; dst.pos[i] = src.pos[r]; dst.flag[i] = src.flag[r]; dst.end[i] = src.end[r];
    dst.vbeg[i] = ((uint64_t)coff[b] << 16) | (uint64_t)(u - b * block_bytes);
}
int bamindex_take_rows(BamIndex* S, const BamIndex* src, const uint32_t* perm, const int64_t* rec_soff, const int64_t* coff, int64_t n_blk, int64_t block_bytes, hipStream_t st) {
    if (!S || !src || S == src || n_blk < 1 || block_bytes < 1 || block_bytes > 65536) return svx_fail(SVX_E_ARG, "BAM index: bad rows", __FILE__, __LINE__, hipSuccess);
    const int64_t n = src->n;
    S->n = 0; S->have = false;
    if (n > S->cap) {
        const int64_t ncap = std::max<int64_t>(n, 1 << 16);
        SVXCHK(S->tid.reserve((size_t)ncap * 4)); SVXCHK(S->pos.reserve((size_t)ncap * 4)); SVXCHK(S->flag.reserve((size_t)ncap * 2));
        SVXCHK(S->end.reserve((size_t)ncap * 8)); SVXCHK(S->vbeg.reserve((size_t)ncap * 8));
        S->cap = ncap;
    }
    if (n > 0) {
        SVXCHK(S->err.reserve(64));
        HIPCHK(hipMemsetAsync(S->err.p, 0, 64, st));
        k_bix_take<<<BGRID(n), BT, 0, st>>>(n, src->cols(0), src->n, S->cols(0), perm, rec_soff, coff, n_blk, block_bytes, S->err.as<int>());
        HIPCHK(hipGetLastError());
        int err_h = 0;
        SVXCHK(svx_d2h(&err_h, S->err.p, 4, st));
        if (err_h) return svx_fail(SVX_E_STATE, "BAM index: a row of the sorted file lies outside its tables (internal error)", __FILE__, __LINE__, hipSuccess);
    }
    S->n = n; S->n_long = src->n_long; S->t_append = src->t_append;
    return SVX_OK;
}
int64_t bamindex_rows(const BamIndex* S) { return S ? S->n : 0; }

int bamindex_finish(BamIndex* S, int32_t n_ref, uint64_t v_end, hipStream_t st, int fmt) {
    if (!S || n_ref < 0 || (fmt != SVX_INDEX_CLASSIC && fmt != SVX_INDEX_CSI)) return svx_fail(SVX_E_ARG, "BAM index: bad argument", __FILE__, __LINE__, hipSuccess);
    S->pool.reset(); S->have = false;
    const int64_t n = S->n;
    const BixCols T = S->cols(0);
    const bool csi = fmt == SVX_INDEX_CSI;
    const int header_bytes = csi ? BIX_CSI_HEADER_BYTES : BIX_HEADER_BYTES;
    int depth = 0, key_shift = BINIDX_KEY_SHIFT;                 // (depth 0: the five-level bins)
    SVXCHK(S->err.reserve(64));
    int* err_d = S->err.as<int>();
    HIPCHK(hipMemsetAsync(err_d, 0, 64, st));
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[0] = bix_now();
    // ---- the order, the range ----
    int err_h = 0;
    if (n > 0) {
        k_bix_check<<<BGRID(n), BT, 0, st>>>(n, n_ref, T, err_d, csi ? 0 : 1);
        HIPCHK(hipGetLastError());
        SVXCHK(svx_d2h(&err_h, err_d, 4, st));
    }
    if (err_h & BIXF_TID) return svx_fail(SVX_E_ARG, "BAM index: a record names a reference the header does not have", __FILE__, __LINE__, hipSuccess);   // (first, as in svx_bam_index_host)
    if (err_h & BIXF_ORDER) return svx_fail(SVX_E_ORDER, "BAM index: the file is not in coordinate order", __FILE__, __LINE__, hipSuccess);
    if (err_h & BIXF_RANGE) return svx_fail(SVX_E_RANGE, "BAM index: a record ends beyond 2^29, outside what a .bai can hold", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[1] = bix_now();
    // ---- references, chunk heads ----
    int64_t n_placed = 0, n_chunks = 0, n_bins = 0, n_slots = 0, n_refs_with_rows = 0;
    int64_t *first = nullptr, *bpos = nullptr, *upos = nullptr; int32_t *bhead = nullptr, *umark = nullptr;
    std::vector<int64_t> first_h((size_t)n_ref + 1, 0);
    if (n > 0 && n_ref > 0) {
        SVXCHK(S->pool.get(&first, (size_t)n_ref + 1));
        k_bix_ref_first<<<BGRID(n_ref + 1), BT, 0, st>>>(n, T.tid, n_ref, first);
        HIPCHK(hipGetLastError());
        SVXCHK(svx_d2h(first_h.data(), first, ((size_t)n_ref + 1) * 8, st));
        n_placed = first_h[(size_t)n_ref];
        if (n_placed < 0 || n_placed > n) return svx_fail(SVX_E_STATE, "BAM index: the reference table is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        for (int32_t t = 0; t < n_ref; t++) n_refs_with_rows += first_h[(size_t)t + 1] > first_h[(size_t)t];
    }
    uint32_t* chunk_rec = nullptr; uint64_t *key = nullptr, *key2 = nullptr; uint32_t *val = nullptr, *val2 = nullptr;
    int64_t* rmax = nullptr;
    BixRows rows{T, n, v_end, first, upos, nullptr, header_bytes, 0};
    if (csi) {
        // ---- the running maximum of the ends inside every reference; the file's largest end gives the depth ----
        int64_t max_end = 0;
        if (n_placed > 0) {
            int64_t* gmax; long long* tile_v; int* tile_f;
            const size_t tiles = (size_t)((n_placed + BINIDX_RMAX_TILE - 1) / BINIDX_RMAX_TILE);
            SVXCHK(S->pool.get(&rmax, (size_t)n_placed)); SVXCHK(S->pool.get(&gmax, (size_t)n_ref)); SVXCHK(S->pool.get(&tile_v, tiles)); SVXCHK(S->pool.get(&tile_f, tiles));
            SVXCHK(binidx_launch_run_max(st, rows, n_placed, n_ref, rmax, gmax, tile_v, tile_f));
            HIPCHK(hipGetLastError());
            std::vector<int64_t> gmax_h((size_t)n_ref, 0);
            SVXCHK(svx_d2h(gmax_h.data(), gmax, (size_t)n_ref * 8, st));
            for (int64_t v : gmax_h) max_end = std::max(max_end, v);
        }
        depth = binidx_depth_for(max_end); key_shift = binidx_csi_key_shift(depth);
        if (max_end > (1ll << (BINIDX_CSI_MIN_SHIFT + 3 * depth))) return svx_fail(SVX_E_STATE, "BAM index: an end beyond every depth (internal error)", __FILE__, __LINE__, hipSuccess);
        rows.csi_depth = depth;
    }
    if (n_placed > 0) {
        SVXCHK(S->pool.get(&bhead, (size_t)n_placed + 1)); SVXCHK(S->pool.get(&umark, (size_t)n_placed + 1)); SVXCHK(S->pool.get(&bpos, (size_t)n_placed + 1)); SVXCHK(S->pool.get(&upos, (size_t)n_placed + 1));
        k_bix_heads<<<BGRID(n_placed + 1), BT, 0, st>>>(n_placed, T, bhead, umark, depth);
        SVXCHK((svx_exclusive_scan<int32_t, int64_t>(bhead, bpos, n_placed + 1, st, S->scan_tmp)));
        SVXCHK((svx_exclusive_scan<int32_t, int64_t>(umark, upos, n_placed + 1, st, S->scan_tmp)));
        SVXCHK(svx_d2h(&n_chunks, bpos + n_placed, 8, st));
        if (n_chunks < 1 || n_chunks > n_placed) return svx_fail(SVX_E_STATE, "BAM index: the chunk count is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&chunk_rec, (size_t)n_chunks + 1)); SVXCHK(S->pool.get(&key, (size_t)n_chunks)); SVXCHK(S->pool.get(&val, (size_t)n_chunks));
        SVXCHK(S->pool.get(&key2, (size_t)n_chunks)); SVXCHK(S->pool.get(&val2, (size_t)n_chunks));
        k_bix_chunks<<<BGRID(n_placed + 1), BT, 0, st>>>(n_placed, n_chunks, T, bhead, bpos, chunk_rec, key, val, depth);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[2] = bix_now();
    // ---- chunks sorted by (tid, bin); bins ----
    int32_t *bh = nullptr, *tmax = nullptr; int64_t *binpos = nullptr, *tsz = nullptr, *nintv = nullptr, *toff = nullptr, *loff = nullptr; uint32_t *bin_first = nullptr, *ref_first_bin = nullptr;
    if (n_placed > 0) {
        SVXCHK(S->pool.get(&bh, (size_t)n_chunks + 1)); SVXCHK(S->pool.get(&binpos, (size_t)n_chunks + 1));
        SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, key, key2, val, val2, n_chunks, 0, binidx_sort_end_bit(n_ref, key_shift)));
        k_binidx_bin_heads<BixRows><<<BGRID(n_chunks + 1), BT, 0, st>>>(n_chunks, key2, bh);
        SVXCHK((svx_exclusive_scan<int32_t, int64_t>(bh, binpos, n_chunks + 1, st, S->scan_tmp)));
        SVXCHK(svx_d2h(&n_bins, binpos + n_chunks, 8, st));
        if (n_bins < 1 || n_bins > n_chunks) return svx_fail(SVX_E_STATE, "BAM index: the bin count is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&bin_first, (size_t)n_bins + 1)); SVXCHK(S->pool.get(&ref_first_bin, (size_t)n_ref + 1));
        binidx_launch_bins<BixRows>(st, n_chunks, n_bins, n_ref, key2, bh, binpos, bin_first, ref_first_bin, key_shift);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[3] = bix_now();
    // ---- sizes; the linear index: the smallest vbeg per window ----
    unsigned long long* lin = nullptr;
    uint64_t* bin_loff = nullptr;
    const int64_t empty_part = csi ? BINIDX_CSI_EMPTY_PART_BYTES : BINIDX_EMPTY_PART_BYTES;
    int64_t body = empty_part * n_ref;
    rows.first_row = first; rows.upos = upos;
    if (n_placed > 0 && csi) {
        // (a .csi: the loffset of every bin by bisection of the running maximum; no largest end per reference, no slots)
        SVXCHK(S->pool.get(&tsz, (size_t)n_ref + 1)); SVXCHK(S->pool.get(&toff, (size_t)n_ref + 2)); SVXCHK(S->pool.get(&bin_loff, (size_t)n_bins));
        k_binidx_bin_loff<<<BGRID(n_chunks), BT, 0, st>>>(rows, n_chunks, n_bins, n_placed, key_shift, key2, bh, binpos, rmax, bin_loff, err_d, BIXF_LAYOUT);
        k_binidx_sizes_csi<<<BGRID(n_ref + 1), BT, 0, st>>>(rows, n_ref, ref_first_bin, bin_first, tsz);
        SVXCHK((svx_exclusive_scan<int64_t, int64_t>(tsz, toff, (long long)n_ref + 1, st, S->scan_tmp)));
        HIPCHK(hipGetLastError());
        SVXCHK(svx_d2h(&body, toff + n_ref, 8, st));
        if (body < empty_part * n_ref) return svx_fail(SVX_E_STATE, "BAM index: the sizes are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
    }
    if (n_placed > 0 && !csi) {
        SVXCHK(S->pool.get(&tmax, (size_t)n_ref + 1)); SVXCHK(S->pool.get(&tsz, (size_t)n_ref + 1)); SVXCHK(S->pool.get(&nintv, (size_t)n_ref + 1));
        SVXCHK(S->pool.get(&toff, (size_t)n_ref + 2)); SVXCHK(S->pool.get(&loff, (size_t)n_ref + 2));
        HIPCHK(hipMemsetAsync(tmax, 0, ((size_t)n_ref + 1) * 4, st));
        k_binidx_max_end<<<BGRID(n_placed), BT, 0, st>>>(rows, n_placed, tmax);
        k_binidx_sizes<<<BGRID(n_ref + 1), BT, 0, st>>>(rows, n_ref, tmax, ref_first_bin, bin_first, tsz, nintv);
        SVXCHK((svx_exclusive_scan<int64_t, int64_t>(tsz, toff, (long long)n_ref + 1, st, S->scan_tmp)));
        SVXCHK((svx_exclusive_scan<int64_t, int64_t>(nintv, loff, (long long)n_ref + 1, st, S->scan_tmp)));
        HIPCHK(hipGetLastError());
        {
            HostCopy hc(st);
            SVXCHK(hc.d2h(&body, toff + n_ref, 8)); SVXCHK(hc.d2h(&n_slots, loff + n_ref, 8));
            SVXCHK(hc.finish());
        }
        if (n_slots < 1 || n_slots > (int64_t)n_ref * 32768 || body < (int64_t)BINIDX_EMPTY_PART_BYTES * n_ref)
            return svx_fail(SVX_E_STATE, "BAM index: the sizes are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&lin, (size_t)n_slots));
        HIPCHK(hipMemsetAsync(lin, 0xff, (size_t)n_slots * 8, st));
        k_binidx_linear<<<BGRID(n_placed), BT, 0, st>>>(rows, n_placed, loff, n_slots, lin);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[4] = bix_now();
    // ---- layout: header, the references' parts, trailer; every field at its offset ----
    const int64_t n_blob = header_bytes + body + 8;
    SVXCHK(S->blob.reserve((size_t)n_blob + 64));
    uint8_t* blob = S->blob.as<uint8_t>();
    HIPCHK(hipMemsetAsync(blob, 0, (size_t)n_blob + 64, st));
    {
        uint8_t head[BIX_CSI_HEADER_BYTES], trail[8];
        if (csi) {
            memcpy(head, "CSI\1", 4);
            binidx_put32(head + 4, BINIDX_CSI_MIN_SHIFT); binidx_put32(head + 8, (uint32_t)depth); binidx_put32(head + 12, 0u); binidx_put32(head + 16, (uint32_t)n_ref);
        } else { memcpy(head, "BAI\1", 4); binidx_put32(head + 4, (uint32_t)n_ref); }
        binidx_put64(trail, (uint64_t)(n - n_placed));
        HostCopy hc(st);
        SVXCHK(hc.h2d(blob, head, (size_t)header_bytes)); SVXCHK(hc.h2d(blob + n_blob - 8, trail, sizeof trail));
        SVXCHK(hc.finish());
    }
    if (n_placed > 0) {
        rows.toff = toff;
        const BinIdxOut o{blob, n_blob - 8, err_d, BIXF_LAYOUT};
        if (csi) {
            k_binidx_ser_chunks_csi<<<BGRID(n_chunks), BT, 0, st>>>(rows, n_chunks, key_shift, key2, val2, bh, binpos, bin_first, ref_first_bin, chunk_rec, bin_loff, o);
            k_binidx_ser_group_csi<<<BGRID(n_ref), BT, 0, st>>>(rows, n_ref, ref_first_bin, bin_first, o);
        } else {
            k_binidx_ser_chunks<<<BGRID(n_chunks), BT, 0, st>>>(rows, n_chunks, key2, val2, bh, binpos, bin_first, ref_first_bin, chunk_rec, o);
            k_binidx_ser_group<<<(unsigned)n_ref, 64, 0, st>>>(rows, n_ref, ref_first_bin, bin_first, loff, lin, o);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); S->t_mark[5] = bix_now();
    SVXCHK(svx_d2h(&err_h, err_d, 4, st));
    HIPCHK(hipStreamSynchronize(st));
    if (err_h & BIXF_LAYOUT) return svx_fail(SVX_E_STATE, "BAM index: a field lay outside the index it was sized for (internal error)", __FILE__, __LINE__, hipSuccess);
    double* tp[5] = {&S->stats.t_check_ms, &S->stats.t_chunks_ms, &S->stats.t_sort_ms, &S->stats.t_linear_ms, &S->stats.t_serialise_ms};
    for (int k = 0; k < 5; k++) *tp[k] = (S->t_mark[k + 1] - S->t_mark[k]) * 1e3;
    S->stats.t_total_ms = (S->t_mark[5] - S->t_mark[0]) * 1e3;
    S->stats.t_append_ms = S->t_append * 1e3;
    S->stats.n_rows = n; S->stats.n_placed = n_placed; S->stats.n_refs = n_ref; S->stats.n_refs_with_rows = n_refs_with_rows; S->stats.n_chunks = n_chunks; S->stats.n_bins = n_bins;
    S->stats.n_slots = n_slots; S->stats.n_long_cigars = S->n_long; S->stats.bytes_out = n_blob;
    S->n_blob = n_blob; S->have = true;
    return SVX_OK;
}

bool bamindex_bytes(const BamIndex* S, int64_t* n_bytes) {
    if (!S || !S->have) return false;
    if (n_bytes) *n_bytes = S->n_blob;
    return true;
}
int bamindex_fetch(BamIndex* S, uint8_t* host_dst, hipStream_t st) {
    if (!S || !S->have) return svx_fail(SVX_E_STATE, "no BAM index: svx_bam_index_begin, a pass over the file, svx_bam_index_finish", __FILE__, __LINE__, hipSuccess);
    if (host_dst && S->n_blob > 0) SVXCHK(svx_d2h(host_dst, S->blob.p, (size_t)S->n_blob, st));
    return SVX_OK;
}
void bamindex_stats(const BamIndex* S, svx_bam_index_stats* out) {
    if (S) *out = S->stats; else memset(out, 0, sizeof *out);
}
