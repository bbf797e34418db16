// alnindex.hip - the alignment table of GENOTYPE, resident in HBM and filled while COLLECT runs (gfx950).
//
// genotype() (src/svim/SVIM_genotyping.py:34-93) re-fetches the BAM file around every candidate; svim_amd/SVIM_genotyping.py replaces the fetches by an interval
// join over a structure-of-arrays of every record (AlignmentIndex), which Python builds by a second pass over the file.  svx_collect sees every record of the
// file anyway: while svx_collect_keep_alignments is on, each call appends its batch's records - tid, pos, end, flag, mapq, read_id, file order kept - to a table
// in the context.  EVERY record of the batch is kept (no compaction, and no dependence on the min_mapq of that COLLECT: a later svx_genotype_resident may ask
// for any min_mapq).  What a record that can never count costs is 19 bytes; what it does not cost is its CIGAR: reference_end is computed only for records
// that are placed (tid >= 0), mapped, not secondary and not marked SVX_FLAG_SKIP - the others get end = pos, which no result depends on (genotype() skips
// them before it counts, :64-65; they only bound where a walk starts).  A record marked SVX_FLAG_SKIP is stored with the unmapped bit set so that the walk skips it.
//
//   k_aln_append      one DPP row (16 lanes) per record, four records per wave: the six columns, and reference_end = pos + the lengths of the M D N = X
//                     operations of records of up to ALN_LONG_OPS operations - 16-byte loads of whole aligned chunks, single words at the two edges, the
//                     consumes-reference test as a bit test of a constant mask, the row's sum by DPP.  Longer records go to a list
//   k_aln_span_long   the listed records (a CG-tag CIGAR has no length limit), one wave per tile of 1024 operations over the whole grid, wave sum by DPP, one
//                     atomic add per tile
//   finalisation      once after an append, when the table is first used: order check (tid, pos non-decreasing), contig_first by bisection on tid, and the
//                     running maximum of end inside every contig as ONE max-scan of (tid << 32 | end) - the table is sorted by tid, so the maximum over a
//                     prefix carries the last contig's tid in its high half and that contig's maximum in the low half (three launches, tiles of 2048)
//   any record order  (svx_collect_keep_alignments_mode, SVX_ALN_SORT) a table whose rows are not in coordinate order is brought into it instead of refused:
//                     k_aln_sort_keys (bsort_key of bamsort_core.hpp per row + the row number), ONE stable svx_sort_pairs_u64 over the 33 + tid_bits key bits in
//                     use, k_aln_gather (the six columns and the append positions, every row's source read once).  The gathered columns land in the buffers
//                     the sort has finished with and are copied back, so the gather allocates nothing.  SVX_ALN_FILE_FLAGS: a skip mark is the front end's
//                     (query-name mode), the record keeps flag & 0x0fff and the end its CIGAR gives
#include "common.hpp"
#include "hostcopy.hpp"
#include "cigar_span.hpp"
#include "bamsort_core.hpp"

#define ALN_LONG_OPS 4096
#define ALN_LONG_TILE 1024
#define ALN_LONG_BLOCKS 256
#define PM_T 256
#define PM_ITEMS 8
#define PM_TILE (PM_T * PM_ITEMS)

struct AlnTable {
    int64_t n = 0, cap = 0;
    bool have = false;               // svx_collect has appended to it (an empty file leaves an empty table, not none)
    bool finalised = false; int32_t n_contig = -1;
    DevBuf tid, pos, end, flag, mapq, read_id, prefmax, contig_first, contig_len, long_list, small, tile_max;
    hipEvent_t ev[3]; bool have_ev = false;
    double t_append_ms = 0, t_span_ms = 0, t_finalise_ms = 0;
    int64_t n_ops_read = 0, n_long = 0;
    // any record order: the mode the rows were appended under, the append position of every row (perm_n rows of it are set; identity behind them and when
    // there is none), what the last finalisation did
    uint32_t flags = 0;
    DevBuf perm, key, key2, val, src; int64_t perm_n = 0; bool have_perm = false;
    hipEvent_t sev[4]; bool have_sev = false;
    svx_alignments_sort_stats sort_stats = {};
};

struct AlnCols { int32_t *tid, *pos, *end; uint16_t* flag; uint8_t* mapq; int32_t* read_id; };

__global__ __launch_bounds__(256) void k_aln_append(long long n_rec, const int32_t* tid, const int32_t* pos, const uint16_t* flag, const uint8_t* mapq,
                                                    const int32_t* read_id, const uint64_t* cigar_off, const uint32_t* cigar, AlnCols out, uint32_t* long_list,
                                                    unsigned long long* counters, unsigned drop_mask) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = (int)(threadIdx.x & 15);
    const bool in = r < n_rec;
    uint32_t s = 0; unsigned long long n_ops = 0;
    bool is_long = false;
    int t = -1, p = 0; unsigned f = 0;
    if (in) {
        t = tid[r]; p = pos[r]; f = flag[r] & ~drop_mask;                  // SVX_ALN_FILE_FLAGS drops the front end's skip mark: the record counts as the file has it
        if (t >= 0 && !(f & (4u | 256u | SVX_FLAG_SKIP))) {
            const unsigned long long lo = cigar_off[r], hi = cigar_off[r + 1];
            if (hi > lo) {
                n_ops = hi - lo;
                if (n_ops > ALN_LONG_OPS) is_long = true; else s = span_partial(cigar, lo, hi, l, 16);
            }
        }
    }
    s = (uint32_t)row_sum_i32((int)s);
    if (in && l == 15) {
        out.tid[r] = t; out.pos[r] = p; out.end[r] = p + (int)s;           // a record without reference span: end = pos (what AlignmentIndex stores)
        out.flag[r] = (uint16_t)((f & SVX_FLAG_SKIP) ? (f | 4u) : f); out.mapq[r] = mapq[r]; out.read_id[r] = read_id[r];
        if (is_long) long_list[atomicAdd(&counters[0], 1ull)] = (uint32_t)r;
        if (n_ops) atomicAdd(&counters[1], n_ops);
    }
}

__global__ __launch_bounds__(256) void k_aln_span_long(const unsigned long long* counters, const uint32_t* long_list, const uint64_t* cigar_off, const uint32_t* cigar,
                                                       int32_t* end) {
    const unsigned long long n_long = counters[0];
    const int lane = lane_id();
    const unsigned long long wave = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * 4;
    for (unsigned long long k = 0; k < n_long; k++) {
        const uint32_t r = long_list[k];
        const unsigned long long lo = cigar_off[r], hi = cigar_off[r + 1];
        const unsigned long long tiles = (hi - lo + ALN_LONG_TILE - 1) / ALN_LONG_TILE;
        for (unsigned long long t = wave; t < tiles; t += n_waves) {
            const unsigned long long a = lo + t * ALN_LONG_TILE, b = a + ALN_LONG_TILE < hi ? a + ALN_LONG_TILE : hi;
            const int s = wave_sum_i32((int)span_partial(cigar, a, b, lane, 64));
            if (lane == 0 && s) atomicAdd(&end[r], s);
        }
    }
}

// ---- finalisation ----------------------------------------------------------------------------------------------------------------------------------------
// unplaced records (tid -1) sort behind every contig, as a coordinate-sorted file has them; their positions are not compared
__global__ void k_aln_order(long long n, const int32_t* tid, const int32_t* pos, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (i >= n) return;
    const uint32_t a = (uint32_t)tid[i - 1], b = (uint32_t)tid[i];
    if (a > b || (a == b && (int32_t)b >= 0 && pos[i - 1] > pos[i])) atomicOr(bad, 1ull);
}
__global__ void k_aln_contig_first(long long n, const int32_t* tid, int n_contig, int64_t* contig_first) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c > n_contig) return;
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((uint32_t)tid[mid] >= (uint32_t)c) hi = mid; else lo = mid + 1; }
    contig_first[c] = lo;
}
__device__ __forceinline__ unsigned long long pm_key(const int32_t* tid, const int32_t* pos, const int32_t* end, long long i) {
    const int32_t p = pos[i]; int32_t e = end[i];
    if (e <= p) e = p + 1;                                                    // htslib's overlap rule for a record without reference span
    return ((unsigned long long)(uint32_t)tid[i] << 32) | (uint32_t)e;
}
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long pm_load(const int32_t* tid, const int32_t* pos, const int32_t* end, long long lo, long long n, unsigned long long (&x)[PM_ITEMS]) {
    unsigned long long m = 0;
#pragma unroll
    for (int k = 0; k < PM_ITEMS; k++) {
        const long long i = lo + (long long)threadIdx.x * PM_ITEMS + k;
        x[k] = i < n ? pm_key(tid, pos, end, i) : 0ull;
        m = umax64(m, x[k]);
    }
    return m;
}
// inclusive maximum over the workgroup's threads in thread order, minus the thread's own value: the maximum of the threads in front (0: none); *total: of all
__device__ __forceinline__ unsigned long long pm_block_excl(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
    const int w = (int)(threadIdx.x >> 6), lane = lane_id();
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(incl, o, 64); if (lane >= o) incl = umax64(incl, u); }
    unsigned long long ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = 0;
    __syncthreads();
    if (lane == 63) sh[w] = incl;
    __syncthreads();
    unsigned long long base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < PM_T / 64; k++) { const unsigned long long xk = sh[k]; if (k < w) base = umax64(base, xk); all = umax64(all, xk); }
    *total = all;
    return umax64(base, ex);
}
__global__ __launch_bounds__(PM_T) void k_aln_pm_tile_max(long long n, const int32_t* tid, const int32_t* pos, const int32_t* end, unsigned long long* tile_max) {
    __shared__ unsigned long long sh[PM_T / 64];
    unsigned long long x[PM_ITEMS], total;
    const unsigned long long mine = pm_load(tid, pos, end, (long long)blockIdx.x * PM_TILE, n, x);
    (void)pm_block_excl(mine, sh, &total);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = total;
}
// tile_max[t] <- the maximum of the tiles in front of t (one workgroup walks the tiles)
__global__ __launch_bounds__(PM_T) void k_aln_pm_tile_scan(long long tiles, unsigned long long* tile_max) {
    __shared__ unsigned long long sh[PM_T / 64];
    unsigned long long carry = 0;
    for (long long lo = 0; lo < tiles; lo += PM_T) {
        const long long t = lo + threadIdx.x;
        const unsigned long long v = t < tiles ? tile_max[t] : 0ull;
        unsigned long long total;
        const unsigned long long ex = pm_block_excl(v, sh, &total);
        if (t < tiles) tile_max[t] = umax64(carry, ex);
        carry = umax64(carry, total);
    }
}
__global__ __launch_bounds__(PM_T) void k_aln_pm_tiles(long long n, const int32_t* tid, const int32_t* pos, const int32_t* end, const unsigned long long* tile_start,
                                                       int32_t* prefmax) {
    __shared__ unsigned long long sh[PM_T / 64];
    unsigned long long x[PM_ITEMS], total;
    const long long lo = (long long)blockIdx.x * PM_TILE;
    const unsigned long long mine = pm_load(tid, pos, end, lo, n, x);
    unsigned long long run = umax64(tile_start[blockIdx.x], pm_block_excl(mine, sh, &total));
#pragma unroll
    for (int k = 0; k < PM_ITEMS; k++) {
        const long long i = lo + (long long)threadIdx.x * PM_ITEMS + k;
        run = umax64(run, x[k]);
        if (i < n) prefmax[i] = (int32_t)(uint32_t)run;       // the high half is this record's own tid: the table is sorted
    }
}

// ---- any record order ------------------------------------------------------------------------------------------------------------------------------------
// The order is bamsort.py's coordinate order: bsort_key, stable.  bad |= 1: a row's key is below its predecessor's; |= 2: a row bsort_key cannot take
// (bsort_check: a reference id outside [-1, n_contig), a position below -1)
__global__ void k_aln_order_key(long long n, const int32_t* tid, const int32_t* pos, const uint16_t* flag, int n_contig, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t t = tid[i], p = pos[i];
    if (bsort_check(t, p, BSORT_MIN_BLOCK_SIZE, n_contig)) { atomicOr(bad, 2ull); return; }
    if (i > 0 && bsort_key(tid[i - 1], pos[i - 1], flag[i - 1], n_contig) > bsort_key(t, p, flag[i], n_contig)) atomicOr(bad, 1ull);
}
// rows [from, n) of the append positions: their own numbers
__global__ void k_aln_perm_iota(long long from, long long n, uint32_t* perm) {
    const long long i = from + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}
__global__ void k_aln_sort_keys(long long n, const int32_t* tid, const int32_t* pos, const uint16_t* flag, int n_contig, uint64_t* key, uint32_t* val) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = bsort_key(tid[i], pos[i], flag[i], n_contig);
    val[i] = (uint32_t)i;
}
struct AlnGatherOut { int32_t *tid, *pos, *end, *read_id; uint32_t* perm; uint16_t* flag; uint8_t* mapq; };
// row i of the sorted table = row src[i] of the table as it lies; perm_in / perm_out: the rows' append positions, carried along like a column
__global__ __launch_bounds__(256) void k_aln_gather(long long n, const uint32_t* src, AlnCols in, const uint32_t* perm_in, AlnGatherOut out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = src[i];
    out.tid[i] = in.tid[s]; out.pos[i] = in.pos[s]; out.end[i] = in.end[s]; out.read_id[i] = in.read_id[s];
    out.perm[i] = perm_in[s]; out.flag[i] = in.flag[s]; out.mapq[i] = in.mapq[s];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
void svx_preload_alnindex() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_aln_append)); (void)hipGetLastError(); }

void svx_aln_release(svx_ctx* c) {
    AlnTable* T = c->aln;
    if (!T) return;
    DevBuf* all[] = {&T->tid, &T->pos, &T->end, &T->flag, &T->mapq, &T->read_id, &T->prefmax, &T->contig_first, &T->contig_len, &T->long_list, &T->small, &T->tile_max,
                     &T->perm, &T->key, &T->key2, &T->val, &T->src};
    for (auto* b : all) b->release();
    if (T->have_ev) for (auto& e : T->ev) (void)hipEventDestroy(e);
    if (T->have_sev) for (auto& e : T->sev) (void)hipEventDestroy(e);
    delete T;
    c->aln = nullptr;
}

void svx_aln_clear(svx_ctx* c) {
    AlnTable* T = c->aln;
    if (!T) return;
    T->n = 0; T->have = false; T->finalised = false;
    T->perm_n = 0; T->have_perm = false; T->sort_stats = svx_alignments_sort_stats{};
    T->t_append_ms = T->t_span_ms = T->t_finalise_ms = 0; T->n_ops_read = T->n_long = 0;
}

int svx_aln_append(svx_ctx* c, const svx_batch* b) {
    if (!c->aln) c->aln = new AlnTable();
    AlnTable* T = c->aln;
    hipStream_t st = c->stream;
    if (!T->have_ev) { for (auto& e : T->ev) HIPCHK(hipEventCreate(&e)); T->have_ev = true; }
    T->have = true; T->finalised = false;
    if (T->n == 0) T->flags = c->aln_flags;
    else if (T->flags != c->aln_flags) return svx_fail(SVX_E_STATE, "svx_collect_keep_alignments_mode: the flags changed while the table holds rows", __FILE__, __LINE__, hipSuccess);
    const int64_t n = b->n_rec, at = T->n;
    if (n <= 0) return SVX_OK;
    if (n >= (1ll << 31) - 16) return svx_fail(SVX_E_ARG, "more than 2^31 records in one batch", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipEventRecord(T->ev[0], st));
    if (at + n > T->cap) {
        const int64_t nc = (at + n) + (at + n) / 2 + 1024;
        for (DevBuf* x : {&T->tid, &T->pos, &T->end, &T->read_id}) SVXCHK(x->reserve((size_t)nc * 4, true, st));
        SVXCHK(T->flag.reserve((size_t)nc * 2, true, st)); SVXCHK(T->mapq.reserve((size_t)nc, true, st));
        T->cap = nc;
    }
    SVXCHK(T->long_list.reserve((size_t)n * 4));
    SVXCHK(T->small.reserve(64));
    unsigned long long* counters = T->small.as<unsigned long long>();         // [0] long records, [1] operations read, [2] order flag
    HIPCHK(hipMemsetAsync(counters, 0, 16, st));
    const AlnCols out{T->tid.as<int32_t>() + at, T->pos.as<int32_t>() + at, T->end.as<int32_t>() + at, T->flag.as<uint16_t>() + at, T->mapq.as<uint8_t>() + at,
                      T->read_id.as<int32_t>() + at};
    HIPCHK(hipEventRecord(T->ev[1], st));
    k_aln_append<<<(unsigned)((n * 16 + 255) / 256), 256, 0, st>>>(n, b->tid, b->pos, b->flag, b->mapq, b->read_id, b->cigar_off, b->cigar, out,
                                                                   T->long_list.as<uint32_t>(), counters, (T->flags & SVX_ALN_FILE_FLAGS) ? 0xf000u : 0u);
    k_aln_span_long<<<ALN_LONG_BLOCKS, 256, 0, st>>>(counters, T->long_list.as<uint32_t>(), b->cigar_off, b->cigar, out.end);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(T->ev[2], st));
    unsigned long long h[2] = {0, 0};
    SVXCHK(svx_mail_read(c, st, counters, 2, h));
    HIPCHK(hipEventSynchronize(T->ev[2]));
    float ms = 0;
    if (hipEventElapsedTime(&ms, T->ev[0], T->ev[2]) == hipSuccess) T->t_append_ms += ms;
    if (hipEventElapsedTime(&ms, T->ev[1], T->ev[2]) == hipSuccess) T->t_span_ms += ms;
    T->n_long += (int64_t)h[0]; T->n_ops_read += (int64_t)h[1];
    T->n = at + n;
    return SVX_OK;
}

// SVX_ALN_SORT: the order check on the full key and, when a row is out of order, keys -> one stable sort -> gather.  Afterwards the rows are in coordinate
// order where they lay (same buffers), T->perm holds their append positions, T->sort_stats what ran.  `bad` is zero again on return
static int aln_sort_rows(svx_ctx* c, AlnTable* T, int32_t n_contig, unsigned long long* bad) {
    hipStream_t st = c->stream;
    const long long n = T->n;
    svx_alignments_sort_stats& S = T->sort_stats;
    S = svx_alignments_sort_stats{};
    S.n_rows = n; S.key_bits = bsort_key_bits(n_contig);
    if (n >= (1ll << 32)) return svx_fail(SVX_E_RANGE, "the sorted alignment table holds at most 2^32 - 1 rows (the sort carries 32-bit row numbers)", __FILE__, __LINE__, hipSuccess);
    if (n == 0) return SVX_OK;
    const unsigned grid = (unsigned)((n + 255) / 256);
    const AlnCols in{T->tid.as<int32_t>(), T->pos.as<int32_t>(), T->end.as<int32_t>(), T->flag.as<uint16_t>(), T->mapq.as<uint8_t>(), T->read_id.as<int32_t>()};
    k_aln_order_key<<<grid, 256, 0, st>>>(n, in.tid, in.pos, in.flag, n_contig, bad);
    HIPCHK(hipGetLastError());
    unsigned long long h = 0;
    SVXCHK(svx_mail_read(c, st, bad, 1, &h));
    if (h & 2) return svx_fail(SVX_E_ARG, "an alignment record's reference id or position lies outside the contig table", __FILE__, __LINE__, hipSuccess);
    if (!(h & 1)) return SVX_OK;                                   // in order: nothing moves, the append positions stay what they are
    HIPCHK(hipMemsetAsync(bad, 0, 8, st));
    if (!T->have_sev) { for (auto& e : T->sev) HIPCHK(hipEventCreate(&e)); T->have_sev = true; }
    const size_t N = (size_t)n;
    SVXCHK(T->perm.reserve(N * 4 + 64, T->have_perm, st));
    SVXCHK(T->key.reserve(N * 8 + 64)); SVXCHK(T->key2.reserve(N * 8 + 64)); SVXCHK(T->val.reserve(N * 4 + 64)); SVXCHK(T->src.reserve(N * 4 + 64));
    const long long from = T->have_perm ? T->perm_n : 0;
    if (from < n) k_aln_perm_iota<<<(unsigned)((n - from + 255) / 256), 256, 0, st>>>(from, n, T->perm.as<uint32_t>());
    HIPCHK(hipEventRecord(T->sev[0], st));
    k_aln_sort_keys<<<grid, 256, 0, st>>>(n, in.tid, in.pos, in.flag, n_contig, T->key.as<uint64_t>(), T->val.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(T->sev[1], st));
    SVXCHK(svx_sort_pairs_u64(c, T->key.as<uint64_t>(), T->key2.as<uint64_t>(), T->val.as<uint32_t>(), T->src.as<uint32_t>(), n, 0, S.key_bits));
    HIPCHK(hipEventRecord(T->sev[2], st));
    // the sort has finished with its keys, its row numbers and its scratch: the gathered columns land there (23 bytes per row in 8 + 8 + 4 + 12) and are
    // copied back over the table's own
    uint8_t* tmp = c->sort_tmp.as<uint8_t>();
    const AlnGatherOut out{T->key.as<int32_t>(), T->key.as<int32_t>() + N, T->key2.as<int32_t>(), T->key2.as<int32_t>() + N, T->val.as<uint32_t>(),
                           reinterpret_cast<uint16_t*>(tmp), tmp + 2 * N};
    if (c->sort_tmp.cap < 3 * N) return svx_fail(SVX_E_STATE, "the sort's scratch is smaller than its pairs", __FILE__, __LINE__, hipSuccess);
    k_aln_gather<<<grid, 256, 0, st>>>(n, T->src.as<uint32_t>(), in, T->perm.as<uint32_t>(), out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(T->tid.p, out.tid, N * 4, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(T->pos.p, out.pos, N * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(T->end.p, out.end, N * 4, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(T->read_id.p, out.read_id, N * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(T->perm.p, out.perm, N * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(T->flag.p, out.flag, N * 2, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(T->mapq.p, out.mapq, N, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(T->sev[3], st));
    HIPCHK(hipEventSynchronize(T->sev[3]));
    float ms = 0;
    if (hipEventElapsedTime(&ms, T->sev[0], T->sev[1]) == hipSuccess) S.t_key_ms = ms;
    if (hipEventElapsedTime(&ms, T->sev[1], T->sev[2]) == hipSuccess) S.t_sort_ms = ms;
    if (hipEventElapsedTime(&ms, T->sev[2], T->sev[3]) == hipSuccess) S.t_gather_ms = ms;
    S.sorted = 1;
    T->have_perm = true; T->perm_n = n;
    for (DevBuf* x : {&T->key, &T->key2, &T->val, &T->src}) x->release();      // 28 bytes per row the table does not need until rows arrive out of order again
    return SVX_OK;
}

int svx_aln_table_index(svx_ctx* c, int32_t n_contig, const int64_t* contig_len_host, AlnIndexDev* o) {
    AlnTable* T = c->aln;
    if (!T || !T->have)
        return svx_fail(SVX_E_STATE, "no resident alignment table: svx_collect_keep_alignments and svx_collect_accumulate must be on while the file is collected", __FILE__, __LINE__, hipSuccess);
    hipStream_t st = c->stream;
    const long long n = T->n;
    const int32_t* tid = T->tid.as<int32_t>(); const int32_t* pos = T->pos.as<int32_t>(); const int32_t* end = T->end.as<int32_t>();
    if (!T->finalised) {
        HIPCHK(hipEventRecord(T->ev[0], st));
        SVXCHK(T->small.reserve(64));
        unsigned long long* bad = T->small.as<unsigned long long>() + 2;
        HIPCHK(hipMemsetAsync(bad, 0, 8, st));
        SVXCHK(T->prefmax.reserve((size_t)n * 4 + 64));
        if (T->flags & SVX_ALN_SORT) SVXCHK(aln_sort_rows(c, T, n_contig, bad));
        else if (n > 1) k_aln_order<<<(unsigned)((n - 1 + 255) / 256), 256, 0, st>>>(n, tid, pos, bad);
        if (n > 0) {
            const long long tiles = (n + PM_TILE - 1) / PM_TILE;
            SVXCHK(T->tile_max.reserve((size_t)tiles * 8 + 64));
            unsigned long long* tm = T->tile_max.as<unsigned long long>();
            k_aln_pm_tile_max<<<(unsigned)tiles, PM_T, 0, st>>>(n, tid, pos, end, tm);
            k_aln_pm_tile_scan<<<1, PM_T, 0, st>>>(tiles, tm);
            k_aln_pm_tiles<<<(unsigned)tiles, PM_T, 0, st>>>(n, tid, pos, end, tm, T->prefmax.as<int32_t>());
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(T->ev[1], st));
        unsigned long long h = 0;
        SVXCHK(svx_mail_read(c, st, bad, 1, &h));
        HIPCHK(hipEventSynchronize(T->ev[1]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, T->ev[0], T->ev[1]) == hipSuccess) T->t_finalise_ms = ms;
        if (h) return svx_fail(SVX_E_STATE, "genotyping needs a coordinate-sorted alignment file", __FILE__, __LINE__, hipSuccess);
        T->finalised = true; T->n_contig = -1;
    }
    if (T->n_contig != n_contig) {
        SVXCHK(T->contig_first.reserve(((size_t)n_contig + 1) * 8 + 64));
        k_aln_contig_first<<<(unsigned)(n_contig / 256 + 1), 256, 0, st>>>(n, tid, n_contig, T->contig_first.as<int64_t>());
        HIPCHK(hipGetLastError());
        T->n_contig = n_contig;
    }
    SVXCHK(T->contig_len.reserve((size_t)n_contig * 8 + 64));
    if (n_contig) SVXCHK(svx_h2d(T->contig_len.p, contig_len_host, (size_t)n_contig * 8, st));
    *o = AlnIndexDev{T->n, n_contig, T->contig_first.as<int64_t>(), T->contig_len.as<int64_t>(), pos, end, T->prefmax.as<int32_t>(), T->flag.as<uint16_t>(),
                     T->mapq.as<uint8_t>(), T->read_id.as<int32_t>()};
    return SVX_OK;
}

extern "C" int svx_collect_keep_alignments(svx_ctx* c, int on) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    c->keep_alignments = on != 0; c->aln_flags = 0;
    return SVX_OK;
}

extern "C" int svx_collect_keep_alignments_mode(svx_ctx* c, int on, uint32_t flags) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    if (flags & ~(uint32_t)(SVX_ALN_SORT | SVX_ALN_FILE_FLAGS)) return svx_fail(SVX_E_ARG, "svx_collect_keep_alignments_mode: unknown flag", __FILE__, __LINE__, hipSuccess);
    c->keep_alignments = on != 0; c->aln_flags = flags;
    return SVX_OK;
}

extern "C" int svx_alignments_permutation(svx_ctx* c, uint32_t* src_row) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    const AlnTable* T = c->aln;
    if (!T || !T->have || !T->finalised)
        return svx_fail(SVX_E_STATE, "svx_alignments_permutation: the alignment table has not been finalised since its last append", __FILE__, __LINE__, hipSuccess);
    if (T->n == 0) return SVX_OK;
    if (!src_row) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    const int64_t m = T->have_perm ? T->perm_n : 0;
    if (m) {
        HIPCHK(hipSetDevice(c->device));
        HostCopy hc(c->stream);
        SVXCHK(hc.d2h(src_row, T->perm.p, (size_t)m * 4));
        SVXCHK(hc.finish());
    }
    for (int64_t i = m; i < T->n; i++) src_row[i] = (uint32_t)i;       // rows that never moved
    return SVX_OK;
}

extern "C" int svx_alignments_get_sort_stats(svx_ctx* c, svx_alignments_sort_stats* o) {
    if (!c || !o) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    memset(o, 0, sizeof *o);
    if (const AlnTable* T = c->aln) *o = T->sort_stats;
    return SVX_OK;
}

extern "C" int svx_alignments_count(svx_ctx* c, int64_t* n) {
    if (!c || !n) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    *n = c->aln ? c->aln->n : 0;
    return SVX_OK;
}

extern "C" int svx_alignments_fetch(svx_ctx* c, int32_t* tid, int32_t* pos, int32_t* end, uint16_t* flag, uint8_t* mapq, int32_t* read_id) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    AlnTable* T = c->aln;
    if (!T || T->n == 0) return SVX_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)T->n;
    HostCopy hc(c->stream);
    if (tid) SVXCHK(hc.d2h(tid, T->tid.p, n * 4));
    if (pos) SVXCHK(hc.d2h(pos, T->pos.p, n * 4));
    if (end) SVXCHK(hc.d2h(end, T->end.p, n * 4));
    if (flag) SVXCHK(hc.d2h(flag, T->flag.p, n * 2));
    if (mapq) SVXCHK(hc.d2h(mapq, T->mapq.p, n));
    if (read_id) SVXCHK(hc.d2h(read_id, T->read_id.p, n * 4));
    return hc.finish();
}

extern "C" int svx_alignments_get_stats(svx_ctx* c, svx_alignments_stats* o) {
    if (!c || !o) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    memset(o, 0, sizeof *o);
    if (const AlnTable* T = c->aln) {
        o->t_append_ms = T->t_append_ms; o->t_span_ms = T->t_span_ms; o->t_finalise_ms = T->t_finalise_ms;
        o->n_records = T->n; o->n_ops_read = T->n_ops_read; o->n_long_records = T->n_long;
    }
    return SVX_OK;
}
