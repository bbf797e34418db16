// combine.hip - COMBINE on the device: signature clusters -> SV candidates (gfx950).
//
// Restates combine_clusters (src/svim/SVIM_COMBINE.py:332-478, the --skip_consensus branch), merge_translocations_at_insertions and
// flag_cutpaste_candidates (src/svim/SVIM_merging.py:93-159, :12-29) and partition_and_cluster_candidates (src/svim/SVIM_clustering.py:306-372) on the
// cluster table a svx_cluster call left in the context (or one handed in).  Five stages on the context's stream:
//   1  plain candidates   INV / BND / DUP_TAN column transforms, DEL / INS stream compaction (score > 0, removed insertions)
//   2  breakends at insertions   mirrored BND clusters, fwd/fwd and rev/rev lists per source contig (one stable radix sort), CPython's bisect_left per insertion
//   3  cut&paste flag     min over ALL deletion clusters of the span-position distance per insertion-from cluster (k_cutpaste_min, the hot kernel)
//   4  insertions at duplications   two sorted walks with the reference's forward-only pointer, one wave, windows of 64 entries in registers
//   5  re-clustering      sort, partitions, condensed distances, the LDS linkage of CLUSTER (svx_linkage_batch), consolidation
// What the host does in between: list sizes (mailbox reads), pow() of the few merged scores with libm (bit-equal with CPython's math.pow), and the plan of
// stage 5's partitions - offsets plus random.sample for partitions of more than 100 candidates (a sequential MT19937 walk over a handful of partitions).
// The cluster and signature tables are only read.
#include "common.hpp"
#include "hostcopy.hpp"
#include <algorithm>
#include <cmath>

#define CT 256
#define CGRID(n) (unsigned)(((long long)(n) + CT - 1) / CT)
#define CP_FG 8            /* insertion-from clusters per workgroup of k_cutpaste_min */
#define NPOOL 72

struct CluPtrs {
    const uint8_t* type; const int32_t *contig, *start, *end, *contig2, *start2, *end2; const uint8_t* aux;
    const double *score, *std_span, *std_pos; const int64_t* member_off; const int32_t* members;
};
struct CandPtrs {
    uint8_t* cls; int32_t *contig, *start, *end, *contig2, *start2, *end2; uint8_t* aux; int32_t* copies; double *score, *std_span, *std_pos;
    int64_t* size;          // [n + 1] member counts (last = 0): scanned into member_off
    int64_t* msrc;          // where a row's members come from: offset | (source array << 62)
    int64_t* member_off; int32_t* members;
};
struct CandTab {
    int64_t n = 0, n_members = 0; int64_t class_count[SVX_NCAND] = {0, 0, 0, 0, 0, 0};
    DevBuf cls, contig, start, end, contig2, start2, end2, aux, copies, score, std_span, std_pos, size, msrc, member_off, members;
    int reserve(int64_t c) {
        const size_t m = (size_t)c + 1;
        SVXCHK(cls.reserve(m)); SVXCHK(aux.reserve(m));
        DevBuf* b4[] = {&contig, &start, &end, &contig2, &start2, &end2, &copies};
        for (auto* b : b4) SVXCHK(b->reserve(m * 4));
        DevBuf* b8[] = {&score, &std_span, &std_pos, &size, &msrc, &member_off};
        for (auto* b : b8) SVXCHK(b->reserve(m * 8));
        return SVX_OK;
    }
    CandPtrs ptrs() const {
        CandPtrs p;
        p.cls = cls.as<uint8_t>(); p.aux = aux.as<uint8_t>(); p.contig = contig.as<int32_t>(); p.start = start.as<int32_t>(); p.end = end.as<int32_t>();
        p.contig2 = contig2.as<int32_t>(); p.start2 = start2.as<int32_t>(); p.end2 = end2.as<int32_t>(); p.copies = copies.as<int32_t>();
        p.score = score.as<double>(); p.std_span = std_span.as<double>(); p.std_pos = std_pos.as<double>(); p.size = size.as<int64_t>();
        p.msrc = msrc.as<int64_t>(); p.member_off = member_off.as<int64_t>(); p.members = members.as<int32_t>();
        return p;
    }
    void release() {
        DevBuf* all[] = {&cls, &contig, &start, &end, &contig2, &start2, &end2, &aux, &copies, &score, &std_span, &std_pos, &size, &msrc, &member_off, &members};
        for (auto* b : all) b->release();
        n = n_members = 0;
    }
};

struct CombineState {
    CandTab merged, flagged, fdup, result, tan;      // tan: the tandem candidates stage 4 walks (scratch)
    DevBuf in[14]; DevBuf in_aux; DevBuf rank;
    ScratchPool<NPOOL> pool{"combine", 0};      // no pad: SVX_ALLOC_GUARD=1 faults on the first byte behind what a phase asked for
    DevBuf rm1_list, rm2_list; int64_t n_rm1 = 0, n_rm2 = 0;
    bool have_stage2 = false, have_result = false;
    bool from_resident = false; long long cluster_call = 0;      // the call took the resident clusters (source 0) of svx_cluster call number cluster_call
    svx_combine_stats stats;
};

void svx_combine_release(svx_ctx* c) {
    CombineState* s = c->combine;
    if (!s) return;
    s->merged.release(); s->flagged.release(); s->fdup.release(); s->result.release(); s->tan.release();
    for (auto& b : s->in) b.release();
    s->in_aux.release(); s->rank.release(); s->rm1_list.release(); s->rm2_list.release();
    s->pool.release();
    delete s;
    c->combine = nullptr;
}

// ---------------------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp0(int v) { return v < 0 ? 0 : v; }
__device__ __forceinline__ long long abs64(long long v) { return v < 0 ? -v : v; }
__device__ __forceinline__ uint32_t bias32(int v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int readlane_i32(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ long long readlane_i64(long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), l), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__global__ void k_cmb_compact(long long n, const int64_t* flag, const int64_t* excl, int32_t* list) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) list[excl[i]] = (int32_t)i;
}

// members of every row of a table, one wave per row: from array A (source tag 0) or B (tag 1) at the row's msrc offset
__global__ __launch_bounds__(CT) void k_cmb_gather(long long n, const int64_t* dst_off, const int64_t* msrc, const int32_t* src_a, const int32_t* src_b, int32_t* dst) {
    const long long r = (long long)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t o = dst_off[r], len = dst_off[r + 1] - o, m = msrc[r];
    const int32_t* src = ((m >> 62) & 1) ? src_b : src_a;
    const int64_t s = m & ((1ll << 62) - 1);
    for (int64_t k = lane_id(); k < len; k += 64) dst[o + k] = src[s + k];
}

// ---------------------------------------------------------------------------------------------------------
// stage 1: candidates that are column transforms of one cluster each (SVIM_COMBINE.py:338-385, :459-470).  rows: cluster rows relative to row_base
// (NULL: 0 .. n - 1).  The constructors clamp starts with max(0, start) (src/svim/SVCandidate.py)
// ---------------------------------------------------------------------------------------------------------
__global__ void k_cmb_emit(CluPtrs cl, int cls, long long n, const int32_t* rows, long long row_base, CandPtrs o, long long out_base, const uint8_t* sig_aux,
                           long long n_sig) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = row_base + (rows ? (long long)rows[i] : i), q = out_base + i;
    const int c1 = cl.contig[r], s1 = cl.start[r], e1 = cl.end[r];
    int oc1 = c1, os1 = clamp0(s1), oe1 = e1, oc2 = -1, os2 = 0, oe2 = 0, copies = 0;
    uint8_t aux = 0;
    const int64_t m0 = cl.member_off[r], m1 = cl.member_off[r + 1];
    if (cls == SVX_CAND_INS) { oc2 = c1; os2 = clamp0(s1); oe2 = e1; oc1 = -1; os1 = 0; oe1 = 0; }
    else if (cls == SVX_CAND_BND) { oe1 = os1; oc2 = cl.contig2[r]; os2 = clamp0(cl.start2[r]); oe2 = os2; aux = cl.aux[r] & 3; }
    else if (cls == SVX_CAND_DUP_TAN) {
        // int(round((dest_end - dest_start) / (source_end - source_start))): round() of a float is half-even = rint of the FP64 quotient
        const int ds = cl.start2[r], de = cl.end2[r];
        if (e1 != s1) copies = (int)rint((double)((long long)de - ds) / (double)((long long)e1 - s1));
        bool fc = false;
        for (int64_t m = m0; m < m1; m++) { const int32_t j = cl.members[m]; if (j >= 0 && j < n_sig) fc |= (sig_aux[j] & 1) != 0; }
        aux = fc ? 1 : 0;
    }
    o.cls[q] = (uint8_t)cls; o.contig[q] = oc1; o.start[q] = os1; o.end[q] = oe1; o.contig2[q] = oc2; o.start2[q] = os2; o.end2[q] = oe2;
    o.aux[q] = aux; o.copies[q] = copies; o.score[q] = cl.score[r]; o.std_span[q] = cl.std_span[r]; o.std_pos[q] = cl.std_pos[r];
    o.size[q] = m1 - m0; o.msrc[q] = m0;
}

// rows of one table copied into another (the re-clustered DUP_INT candidates into the result); members come from the source table's member array (tag 1)
__global__ void k_cmb_copy_rows(CandPtrs s, long long n, CandPtrs o, long long out_base) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long q = out_base + i;
    o.cls[q] = s.cls[i]; o.contig[q] = s.contig[i]; o.start[q] = clamp0(s.start[i]); o.end[q] = s.end[i]; o.contig2[q] = s.contig2[i];
    o.start2[q] = clamp0(s.start2[i]); o.end2[q] = s.end2[i]; o.aux[q] = s.aux[i]; o.copies[q] = 0; o.score[q] = s.score[i]; o.std_span[q] = s.std_span[i];
    o.std_pos[q] = s.std_pos[i]; o.size[q] = s.member_off[i + 1] - s.member_off[i]; o.msrc[q] = s.member_off[i] | (1ll << 62);
}

__global__ void k_flag_positive(const double* score, long long base, long long n, int64_t* flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = score[base + i] > 0 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------
// stage 2: breakend clusters at insertions (SVIM_merging.py:93-159).  The extended list holds the nb BND clusters followed by their mirror images
// ---------------------------------------------------------------------------------------------------------
struct BndEnt { int sc, ss, se, dc, ds, de, d1, d2; double sspan, spos; long long row; };
__device__ __forceinline__ BndEnt bnd_ent(const CluPtrs& cl, long long base, long long nb, long long e) {
    BndEnt b;
    const bool mir = e >= nb;
    const long long r = base + (mir ? e - nb : e);
    const int a = cl.aux[r];
    b.row = r;
    if (!mir) {
        b.sc = cl.contig[r]; b.ss = cl.start[r]; b.se = cl.end[r]; b.dc = cl.contig2[r]; b.ds = cl.start2[r]; b.de = cl.end2[r];
        b.d1 = a & 1; b.d2 = (a >> 1) & 1; b.sspan = cl.std_span[r]; b.spos = cl.std_pos[r];
    } else {        // source and destination swapped, directions flipped (:100-104); the constructor call there passes std_pos where std_span goes and vice versa
        b.sc = cl.contig2[r]; b.ss = cl.start2[r]; b.se = cl.end2[r]; b.dc = cl.contig[r]; b.ds = cl.start[r]; b.de = cl.end[r];
        b.d1 = ((a >> 1) & 1) ? 0 : 1; b.d2 = (a & 1) ? 0 : 1; b.sspan = cl.std_pos[r]; b.spos = cl.std_span[r];
    }
    return b;
}
__device__ __forceinline__ int bnd_source_start(const CluPtrs& cl, long long base, long long nb, long long e) {
    return e >= nb ? cl.start2[base + e - nb] : cl.start[base + e];
}
// key of the two kept lists: list (0 fwd/fwd, 1 rev/rev, 2 neither) | source contig | source end; the stable sort keeps list order among equal keys, which is
// what sorted(..., key=get_key) does per contig
__global__ void k_bnd_keys(CluPtrs cl, long long base, long long nb, uint64_t* key, uint32_t* val) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * nb) return;
    const BndEnt b = bnd_ent(cl, base, nb, e);
    const uint64_t lst = (b.d1 == 0 && b.d2 == 0) ? 0 : ((b.d1 == 1 && b.d2 == 1) ? 1 : 2);
    key[e] = (lst << 62) | ((uint64_t)((uint32_t)b.sc & 0x3fffffffu) << 32) | bias32(b.se);
    val[e] = (uint32_t)e;
}
__device__ __forceinline__ long long lower_bound_u64(const uint64_t* a, long long n, uint64_t x) {
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// get_closest_index (SVIM_merging.py:32-50) over the source starts of entries val[lo .. hi): CPython's bisect_left step for step (the list is ordered by
// source END, so the starts need not be sorted and the search must be the same search), the lower index on a tie
__device__ __forceinline__ long long closest_index(const CluPtrs& cl, long long base, long long nb, const uint32_t* val, long long lo0, long long hi0, int x) {
    const long long len = hi0 - lo0;
    long long lo = 0, hi = len;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (bnd_source_start(cl, base, nb, val[lo0 + mid]) < x) lo = mid + 1; else hi = mid; }
    if (lo == 0) return 0;
    if (lo == len) return len - 1;
    const long long before = bnd_source_start(cl, base, nb, val[lo0 + lo - 1]), after = bnd_source_start(cl, base, nb, val[lo0 + lo]);
    return (after - x < x - before) ? lo : lo - 1;
}
__global__ void k_ins_merge(CluPtrs cl, long long base_ins, long long n_ins, long long base_bnd, long long nb, const uint64_t* key, const uint32_t* val,
                            long long trans_max, int64_t* flag, int32_t* kf_out, int32_t* kr_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ins) return;
    const long long r = base_ins + i, n2 = 2 * nb;
    const int contig = cl.contig[r], s = cl.start[r], e = cl.end[r];
    int64_t f = 0; int32_t kf = 0, kr = 0;
    const uint64_t k0 = (uint64_t)((uint32_t)contig & 0x3fffffffu) << 32, k1 = (1ull << 62) | k0;
    const long long lo0 = lower_bound_u64(key, n2, k0), hi0 = lower_bound_u64(key, n2, k0 + (1ull << 32));
    const long long lo1 = lower_bound_u64(key, n2, k1), hi1 = lower_bound_u64(key, n2, k1 + (1ull << 32));
    if (contig >= 0 && lo0 < hi0 && lo1 < hi1) {                   // (a contig one of the two dicts lacks: KeyError -> continue)
        const uint32_t ef = val[lo0 + closest_index(cl, base_bnd, nb, val, lo0, hi0, s)], er = val[lo1 + closest_index(cl, base_bnd, nb, val, lo1, hi1, s)];
        const BndEnt ff = bnd_ent(cl, base_bnd, nb, ef), rr = bnd_ent(cl, base_bnd, nb, er);
        if (abs64((long long)ff.ss - s) <= trans_max && abs64((long long)rr.ss - s) <= trans_max && ff.dc == rr.dc) {
            const long long distance = abs64((long long)rr.ds - ff.ds);
            const double ratio = (double)((long long)e - s + 1) / (double)(distance + 1);
            if (0.95 <= ratio && ratio <= 1.1) { f = 1; kf = (int32_t)ef; kr = (int32_t)er; }
        }
    }
    flag[i] = f; kf_out[i] = kf; kr_out[i] = kr;
}
__device__ __forceinline__ double scale100_int(long long d) { const long long v = 100 - d; return (double)(v > 0 ? v : 0) / 100.0; }
__device__ __forceinline__ double scale100_std(double s) { if (s != s) return 1.0; const double v = 100.0 - s; return (v > 0 ? v : 0.0) / 100.0; }
// the merged DUP_INT clusters as cluster rows (no clamp), the factors of calculate_score_insertion multiplied in its order, the main score
__global__ void k_merge_rows(CluPtrs cl, long long base_ins, long long n_ins, long long base_bnd, long long nb, const int64_t* flag, const int64_t* excl,
                             const int32_t* kf, const int32_t* kr, CandPtrs o, double* prod, double* main_score, int32_t* rm1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ins || !flag[i]) return;
    const long long r = base_ins + i, j = excl[i];
    const int contig = cl.contig[r], s = cl.start[r];
    const BndEnt ff = bnd_ent(cl, base_bnd, nb, kf[i]), rr = bnd_ent(cl, base_bnd, nb, kr[i]);
    const long long distance = abs64((long long)rr.ds - ff.ds);
    o.cls[j] = SVX_CAND_DUP_INT; o.contig[j] = rr.dc; o.start[j] = rr.ds < ff.ds ? rr.ds : ff.ds; o.end[j] = rr.ds > ff.ds ? rr.ds : ff.ds;
    o.contig2[j] = contig; o.start2[j] = s; o.end2[j] = (int32_t)(s + distance); o.aux[j] = 0; o.copies[j] = 0; o.score[j] = 0;
    o.std_span[j] = cl.std_span[r]; o.std_pos[j] = cl.std_pos[r];
    o.size[j] = (cl.member_off[r + 1] - cl.member_off[r]) + (cl.member_off[ff.row + 1] - cl.member_off[ff.row]) + (cl.member_off[rr.row + 1] - cl.member_off[rr.row]);
    o.msrc[j] = 0;
    double p = scale100_int(abs64((long long)ff.ss - s)) * scale100_int(abs64((long long)rr.ss - s));
    p = p * scale100_std(ff.sspan); p = p * scale100_std(rr.sspan); p = p * scale100_std(ff.spos); p = p * scale100_std(rr.spos);
    prod[j] = p; main_score[j] = cl.score[r]; rm1[j] = (int32_t)i;
}
// members = insertion + fwd/fwd + rev/rev members, in that order; one wave per merged row
__global__ __launch_bounds__(CT) void k_merge_members(CluPtrs cl, long long base_ins, long long base_bnd, long long nb, long long n_new, const int32_t* rm1,
                                                      const int32_t* kf, const int32_t* kr, const int64_t* dst_off, int32_t* dst) {
    const long long j = (long long)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (j >= n_new) return;
    const long long i = rm1[j];
    const long long ef = kf[i], er = kr[i];
    const long long rows[3] = {base_ins + i, base_bnd + (ef >= nb ? ef - nb : ef), base_bnd + (er >= nb ? er - nb : er)};
    int64_t o = dst_off[j];
    for (int k = 0; k < 3; k++) {
        const int64_t s = cl.member_off[rows[k]], len = cl.member_off[rows[k] + 1] - s;
        for (int64_t m = lane_id(); m < len; m += 64) dst[o + m] = cl.members[s + m];
        o += len;
    }
}

// ---------------------------------------------------------------------------------------------------------
// stage 3: cut&paste flag (SVIM_merging.py:12-29)
// ---------------------------------------------------------------------------------------------------------
// insertion-from clusters = CLUSTER's DUP_INT clusters followed by stage 2's -> candidate rows (clamped) + their unclamped source start / end
__global__ void k_flag_rows(CluPtrs cl, long long base_di, long long n_di, CandPtrs mg, long long n_new, CandPtrs o, int32_t* from_s, int32_t* from_e) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_di + n_new) return;
    int sc, ss, se, dc, ds, de; double score, sspan, spos; int64_t size, msrc;
    if (j < n_di) {
        const long long r = base_di + j;
        sc = cl.contig[r]; ss = cl.start[r]; se = cl.end[r]; dc = cl.contig2[r]; ds = cl.start2[r]; de = cl.end2[r];
        score = cl.score[r]; sspan = cl.std_span[r]; spos = cl.std_pos[r]; size = cl.member_off[r + 1] - cl.member_off[r]; msrc = cl.member_off[r];
    } else {
        const long long r = j - n_di;
        sc = mg.contig[r]; ss = mg.start[r]; se = mg.end[r]; dc = mg.contig2[r]; ds = mg.start2[r]; de = mg.end2[r];
        score = mg.score[r]; sspan = mg.std_span[r]; spos = mg.std_pos[r]; size = mg.member_off[r + 1] - mg.member_off[r]; msrc = mg.member_off[r] | (1ll << 62);
    }
    from_s[j] = ss; from_e[j] = se;
    o.cls[j] = SVX_CAND_DUP_INT; o.contig[j] = sc; o.start[j] = clamp0(ss); o.end[j] = se; o.contig2[j] = dc; o.start2[j] = clamp0(ds); o.end2[j] = de;
    o.aux[j] = 0; o.copies[j] = 0; o.score[j] = score; o.std_span[j] = sspan; o.std_pos[j] = spos; o.size[j] = size; o.msrc[j] = msrc;
}
__global__ void k_del_prep(const int32_t* start, const int32_t* end, long long base, long long n, int32_t* mid, int32_t* span) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long s = start[base + i], e = end[base + i];
    mid[i] = (int32_t)((s + e) >> 1);           // (s + e) // 2: floor
    span[i] = (int32_t)(e - s);
}
// For each insertion-from cluster the minimum over ALL deletion clusters of
//     abs(center1 - center2) / normalizer + abs(span1 - span2) / max(span1, span2)          (FP64, this operation order)
// One workgroup takes CP_FG insertion-from clusters, whose centre and span are wave-uniform; the lanes walk the deletion clusters (coalesced reads of the two
// precomputed columns, L2-resident: every workgroup reads them once per CP_FG clusters).  A minimum does not depend on the order of evaluation: per lane, then
// across the wave (DPP), then across the four waves through LDS.  Two FP64 divisions per pair: the kernel is bound by the divide sequence, not by memory.
__global__ __launch_bounds__(CT) void k_cutpaste_min(const int32_t* __restrict__ dmid, const int32_t* __restrict__ dspan, long long n_del,
                                                     const int32_t* __restrict__ from_s, const int32_t* __restrict__ from_e, long long n_from, double normalizer,
                                                     double max_distance, uint8_t* aux_out, double* min_out) {
    __shared__ double sh[CT / 64][CP_FG];
    const long long g0 = (long long)blockIdx.x * CP_FG;
    int mid2[CP_FG], span2[CP_FG];
    double best[CP_FG];
#pragma unroll
    for (int f = 0; f < CP_FG; f++) {
        const long long j = g0 + f < n_from ? g0 + f : n_from - 1;
        const long long s = from_s[j], e = from_e[j];
        mid2[f] = (int)((s + e) >> 1); span2[f] = (int)(e - s);
        best[f] = __longlong_as_double(0x7ff0000000000000ll);
    }
    for (long long i = threadIdx.x; i < n_del; i += CT) {
        const int m1 = dmid[i], sp1 = dspan[i];
#pragma unroll
        for (int f = 0; f < CP_FG; f++) {
            const long long dm = abs64((long long)m1 - mid2[f]), dsp = abs64((long long)sp1 - span2[f]);
            const int mx = sp1 > span2[f] ? sp1 : span2[f];
            const double d = (double)dm / normalizer + (double)dsp / (double)mx;
            best[f] = d < best[f] ? d : best[f];
        }
    }
#pragma unroll
    for (int f = 0; f < CP_FG; f++) {
        const double w = wave_min_f64(best[f]);
        if (lane_id() == 0) sh[threadIdx.x >> 6][f] = w;
    }
    __syncthreads();
    if (threadIdx.x < CP_FG && g0 + threadIdx.x < n_from) {
        double m = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CT / 64; w++) { const double t = sh[w][threadIdx.x]; m = t < m ? t : m; }
        min_out[g0 + threadIdx.x] = m;
        aux_out[g0 + threadIdx.x] = m <= max_distance ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------
// stage 4: insertions that coincide with a duplication (SVIM_COMBINE.py:404-452)
// ---------------------------------------------------------------------------------------------------------
// sort keys of sorted(..., key=get_destination()): (contig name, start, end) -> two stable passes, end first, then rank << 32 | start.
// which 0: flagged DUP_INT candidates (destination columns); 1: tandem candidates, destination (contig, source_end, source_end + copies * (source_end - source_start))
__global__ void k_walk_keys(CandPtrs t, long long base, long long n, int which, const int32_t* rank, int32_t n_contig, uint64_t* key_end, uint64_t* key_cs,
                            long long* end_out, uint32_t* val) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long q = base + i;
    int contig, start; long long end;
    if (which == 0) { contig = t.contig2[q]; start = t.start2[q]; end = t.end2[q]; }
    else { contig = t.contig[q]; const long long s = t.start[q], e = t.end[q]; start = (int)e; end = e + (long long)t.copies[q] * (e - s); }
    const uint32_t rk = contig >= 0 && contig < n_contig ? (uint32_t)rank[contig] : 0xffffffffu;
    key_end[i] = (uint64_t)(end + (1ll << 62)); key_cs[i] = ((uint64_t)rk << 32) | bias32(start); end_out[i] = end; val[i] = (uint32_t)i;
}
__global__ void k_gather_u64c(const uint64_t* src, const uint32_t* idx, uint64_t* dst, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
__global__ void k_gather_i64c(const long long* src, const uint32_t* idx, long long* dst, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
// a sorted list the walk moves through: entry p in registers, 64 entries per window (lane l holds entry base + l)
struct Walk { long long n, p, base; long long wk, we; };
__device__ __forceinline__ void walk_cur(Walk& w, const uint64_t* key, const long long* end, int& rank2, int& start2, long long& end2) {
    if (w.p - w.base >= 64 || w.p < w.base) {
        w.base = w.p;
        const long long q = w.base + lane_id();
        w.wk = q < w.n ? (long long)key[q] : 0; w.we = q < w.n ? end[q] : 0;
    }
    const int l = __builtin_amdgcn_readfirstlane((int)(w.p - w.base));
    const unsigned long long k = (unsigned long long)readlane_i64(w.wk, l);
    rank2 = (int)(k >> 32); start2 = (int)((uint32_t)k ^ 0x80000000u); end2 = readlane_i64(w.we, l);
}
__device__ __forceinline__ bool walk_overlap(int c1, int s1, int e1, int c2, int s2, long long e2) {
    const long long len1 = (long long)e1 - s1, len2 = e2 - s2;
    const long long mx = len1 > len2 ? len1 : len2;
    return c2 == c1 && s2 < e1 && (double)(len1 - len2) / (double)mx < 0.2;
}
// ONE wave.  The pointer of each list only moves forward and stops at the first entry that is not "before" the insertion (contig2 < contig1, or the same
// contig and end2 < start1) - `end` is not monotone in the sort order, so this is the reference's walk and not a search; the tandem list is consulted
// once the interspersed list has run out, the insertion at which it ran out included.  Everything is wave-uniform: the insertions are loaded 64 at a time
// and read with v_readlane, as are the list entries.
__global__ __launch_bounds__(64) void k_walk(const int32_t* ins_contig, const int32_t* ins_start, const int32_t* ins_end, long long n_ins, const int32_t* rank,
                                             int32_t n_contig, const uint64_t* int_key, const long long* int_end, long long n_int, const uint64_t* tan_key,
                                             const long long* tan_end, long long n_tan, uint8_t* rm2) {
    Walk I, Tn;
    I.n = n_int; I.p = 0; I.base = -64; I.wk = 0; I.we = 0;
    Tn.n = n_tan; Tn.p = 0; Tn.base = -64; Tn.wk = 0; Tn.we = 0;
    bool i_end = n_int == 0, t_end = n_tan == 0;
    for (long long k0 = 0; k0 < n_ins; k0 += 64) {
        const long long q = k0 + lane_id();
        const bool valid = q < n_ins;
        const int cq = valid ? ins_contig[q] : -1;
        const int ic = cq >= 0 && cq < n_contig ? rank[cq] : -1, is = valid ? ins_start[q] : 0, ie = valid ? ins_end[q] : 0;
        const int cnt = (int)(n_ins - k0 < 64 ? n_ins - k0 : 64);
        uint8_t mine = 0;
        for (int t = 0; t < cnt; t++) {
            const int c1 = readlane_i32(ic, t), s1 = readlane_i32(is, t), e1 = readlane_i32(ie, t);
            int c2 = 0, s2 = 0; long long e2 = 0;
            bool hit = false;
            if (!i_end) {
                walk_cur(I, int_key, int_end, c2, s2, e2);
                while (c2 < c1 || (c2 == c1 && e2 < s1)) {
                    I.p++;
                    if (I.p >= I.n) { i_end = true; break; }
                    walk_cur(I, int_key, int_end, c2, s2, e2);
                }
            }
            if (!i_end) hit = walk_overlap(c1, s1, e1, c2, s2, e2);
            else {
                if (!t_end) {
                    walk_cur(Tn, tan_key, tan_end, c2, s2, e2);
                    while (c2 < c1 || (c2 == c1 && e2 < s1)) {
                        Tn.p++;
                        if (Tn.p >= Tn.n) { t_end = true; break; }
                        walk_cur(Tn, tan_key, tan_end, c2, s2, e2);
                    }
                }
                if (!t_end) hit = walk_overlap(c1, s1, e1, c2, s2, e2);
            }
            if (lane_id() == t) mine = hit ? 1 : 0;
        }
        if (valid) rm2[q] = mine;
    }
}
__global__ void k_ins_keep(const double* score, long long base_ins, long long n_ins, const int64_t* rm1_flag, const uint8_t* rm2, int64_t* keep, int64_t* rm2_flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ins) return;
    const bool gone = (rm1_flag && rm1_flag[i]) || rm2[i];
    keep[i] = (!gone && score[base_ins + i] > 0) ? 1 : 0;
    rm2_flag[i] = rm2[i] ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------
// stage 5: re-clustering of the interspersed-duplication candidates (SVIM_clustering.py:306-372)
// ---------------------------------------------------------------------------------------------------------
__global__ void k_dup_keys(CandPtrs t, long long n, const int32_t* rank, int32_t n_contig, uint64_t* key, uint32_t* val) {       // get_key(): (type, source contig, source end)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int contig = t.contig[i];
    const uint32_t rk = contig >= 0 && contig < n_contig ? (uint32_t)rank[contig] : 0xffffffffu;
    key[i] = ((uint64_t)rk << 32) | bias32(t.end[i]); val[i] = (uint32_t)i;
}
__global__ void k_dup_part_flags(CandPtrs t, long long n, const uint32_t* sidx, long long max_distance, int64_t* flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t f = 1;
    if (i > 0) {
        const uint32_t a = sidx[i - 1], b = sidx[i];
        if (t.contig[a] == t.contig[b]) { long long d = (long long)t.start[b] - t.end[a]; if (d < 0) d = 0; if (d <= max_distance) f = 0; }
    }
    flag[i] = f;
}
__global__ void k_dup_part_starts(const int64_t* flag, const int64_t* excl, long long n, int64_t* part_start, long long n_part) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) part_start[excl[i]] = i;
    if (i == 0) part_start[n_part] = n;
}
// condensed span_position_distance_intdup_candidates of one partition (sampled where the host said so), rows i < j in scipy's order
__global__ __launch_bounds__(CT) void k_dup_dist(CandPtrs t, const uint32_t* sidx, const int32_t* sel, const int64_t* sel_off, const int32_t* prob_part,
                                                 const int32_t* ns, const int64_t* d_off, double normalizer, double* d) {
    const long long q = blockIdx.x;
    const int n = ns[q];
    const int64_t sb = sel_off[prob_part[q]];
    double* out = d + d_off[q];
    for (int i = threadIdx.x; i < n - 1; i += CT) {
        const uint32_t a = sidx[sel[sb + i]];
        const long long s1 = t.start[a], e1 = t.end[a], ds1 = t.start2[a];
        const long long span1 = e1 - s1, c1 = (s1 + e1) >> 1;
        long long at = (long long)i * n - (long long)i * (i + 1) / 2;
        for (int j = i + 1; j < n; j++, at++) {
            const uint32_t b = sidx[sel[sb + j]];
            const long long s2 = t.start[b], e2 = t.end[b], ds2 = t.start2[b];
            const long long span2 = e2 - s2, c2 = (s2 + e2) >> 1;
            const double pd_source = (double)abs64(c1 - c2) / normalizer, pd_dest = (double)abs64(ds1 - ds2) / normalizer;
            const double span_distance = (double)abs64(span1 - span2) / (double)(span1 > span2 ? span1 : span2);
            out[at] = pd_source + pd_dest + span_distance;
        }
    }
}
__global__ void k_dup_ncl(long long n_part, const int64_t* sel_off, const int32_t* labels, int64_t* ncl) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_part) return;
    const int64_t b = sel_off[p], m = sel_off[p + 1] - b;
    int mx = 1;
    if (m > 1) for (int64_t i = 0; i < m; i++) mx = labels[b + i] > mx ? labels[b + i] : mx;
    ncl[p] = mx;
}
// consolidation, one thread per partition, clusters in label order, candidates in (sampled) list order: int(round(mean)) of the four coordinates = rint(sum / n),
// max score, mean of the stds that are not None, any cutpaste; pass 1 writes the rows and their member counts, pass 2 (members != NULL) the members
__global__ void k_dup_consolidate(CandPtrs t, const uint32_t* sidx, const int32_t* sel, const int64_t* sel_off, const int32_t* labels, long long n_part,
                                  const int64_t* clu_off, CandPtrs o, bool members_pass) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_part) return;
    const int64_t b = sel_off[p], m = sel_off[p + 1] - b;
    const int ncl = (int)(clu_off[p + 1] - clu_off[p]);
    for (int l = 1; l <= ncl; l++) {
        const long long row = clu_off[p] + l - 1;
        long long n = 0, sum_s = 0, sum_e = 0, sum_ds = 0, sum_de = 0, size = 0; int n_sp = 0, n_po = 0; double sp = 0, po = 0, score = 0; bool cut = false; int c1 = -1, c2 = -1;
        int64_t mo = members_pass ? o.member_off[row] : 0;
        for (int64_t i = 0; i < m; i++) {
            if (m > 1 && labels[b + i] != l) continue;
            const uint32_t a = sidx[sel[b + i]];
            const int64_t a0 = t.member_off[a], alen = t.member_off[a + 1] - a0;
            if (members_pass) { for (int64_t k = 0; k < alen; k++) o.members[mo + k] = t.members[a0 + k]; mo += alen; continue; }
            if (n == 0) { c1 = t.contig[a]; c2 = t.contig2[a]; score = t.score[a]; } else if (t.score[a] > score) score = t.score[a];
            n++; sum_s += t.start[a]; sum_e += t.end[a]; sum_ds += t.start2[a]; sum_de += t.end2[a]; size += alen;
            const double x = t.std_span[a], y = t.std_pos[a];
            if (x == x) { sp += x; n_sp++; }
            if (y == y) { po += y; n_po++; }
            cut = cut || (t.aux[a] & 1);
        }
        if (members_pass) continue;
        const double nan = __longlong_as_double(0x7ff8000000000000ll), dn = (double)(n > 0 ? n : 1);
        o.cls[row] = SVX_CAND_DUP_INT; o.contig[row] = c1; o.start[row] = (int32_t)rint((double)sum_s / dn); o.end[row] = (int32_t)rint((double)sum_e / dn);
        o.contig2[row] = c2; o.start2[row] = (int32_t)rint((double)sum_ds / dn); o.end2[row] = (int32_t)rint((double)sum_de / dn);
        o.aux[row] = cut ? 1 : 0; o.copies[row] = 0; o.score[row] = score; o.std_span[row] = n_sp ? sp / (double)n_sp : nan; o.std_pos[row] = n_po ? po / (double)n_po : nan;
        o.size[row] = size; o.msrc[row] = 0;
    }
}

void svx_preload_combine() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_cutpaste_min)); (void)hipGetLastError(); }

// ---------------------------------------------------------------------------------------------------------
// host: random.seed(1524) + random.sample(population, 100) (CPython's Lib/random.py: pool method up to 1045 elements, set method beyond)
// ---------------------------------------------------------------------------------------------------------
struct PyRandom {
    uint32_t s[624]; int at = 624;
    explicit PyRandom(uint32_t key0) {
        s[0] = 19650218u;
        for (int i = 1; i < 624; i++) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i;
        int i = 1;
        for (int k = 624; k; k--) { s[i] = (s[i] ^ ((s[i - 1] ^ (s[i - 1] >> 30)) * 1664525u)) + key0; i++; if (i >= 624) { s[0] = s[623]; i = 1; } }
        for (int k = 623; k; k--) { s[i] = (s[i] ^ ((s[i - 1] ^ (s[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i; i++; if (i >= 624) { s[0] = s[623]; i = 1; } }
        s[0] = 0x80000000u;
    }
    uint32_t word() {
        if (at >= 624) {
            for (int k = 0; k < 624; k++) {
                const uint32_t y = (s[k] & 0x80000000u) | (s[(k + 1) % 624] & 0x7fffffffu);
                s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            at = 0;
        }
        uint32_t y = s[at++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
    int64_t below(int64_t n) {              // _randbelow_with_getrandbits; n < 2^32
        int k = 0;
        while ((n >> k) != 0) k++;
        for (;;) { const int64_t r = (int64_t)(word() >> (32 - k)); if (r < n) return r; }
    }
    void sample100(int64_t n, int32_t* out) {
        const int k = 100;
        if (n <= 1045) {
            std::vector<int32_t> pool((size_t)n);
            for (int64_t i = 0; i < n; i++) pool[(size_t)i] = (int32_t)i;
            for (int i = 0; i < k; i++) { const int64_t j = below(n - i); out[i] = pool[(size_t)j]; pool[(size_t)j] = pool[(size_t)(n - i - 1)]; }
        } else {
            for (int i = 0; i < k; i++) {
                int64_t j;
                for (;;) { j = below(n); bool seen = false; for (int q = 0; q < i; q++) if (out[q] == j) { seen = true; break; } if (!seen) break; }
                out[i] = (int32_t)j;
            }
        }
    }
};
extern "C" int svx_py_sample100(int64_t n, const int64_t* sizes, int32_t* out) {
    if (n < 0 || (n && (!sizes || !out))) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    PyRandom rng(1524u);
    for (int64_t k = 0; k < n; k++) {
        if (sizes[k] < 100 || sizes[k] >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_py_sample100: a population needs 100 .. 2^31 - 1 elements", __FILE__, __LINE__, hipSuccess);
        rng.sample100(sizes[k], out + 100 * k);
    }
    return SVX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// host: the call
// ---------------------------------------------------------------------------------------------------------
// exclusive scan of flag[0 .. n) with the total at excl[n] (flag[n] is set to 0 here)
static int scan_with_total(svx_ctx* c, int64_t* flag, int64_t* excl, int64_t n) {
    HIPCHK(hipMemsetAsync(flag + n, 0, 8, c->stream));
    return svx_exclusive_scan_i64(c, flag, excl, n + 1);
}
static int read_word(svx_ctx* c, const int64_t* dev, int64_t* host) { return svx_mail_read(c, c->stream, dev, 1, host); }
// member_off = exclusive scan of size, total read back, member array reserved
static int finish_offsets(svx_ctx* c, CandTab& t, int64_t n) {
    CandPtrs p = t.ptrs();
    SVXCHK(scan_with_total(c, p.size, p.member_off, n));
    int64_t total = 0;
    SVXCHK(read_word(c, p.member_off + n, &total));
    SVXCHK(t.members.reserve((size_t)(total > 0 ? total : 1) * 4));
    t.n = n; t.n_members = total;
    return SVX_OK;
}
// stable sort of n entries by (rank << 32 | start, end) -> key_cs sorted + the ends in that order
static int sort_destinations(svx_ctx* c, CombineState* S, CandPtrs t, int64_t base, int64_t n, int which, const int32_t* rank, int32_t n_contig,
                             uint64_t** key_out, long long** end_out) {
    uint64_t *k_end, *k_end2, *k_cs, *k_cs_g, *k_cs2; long long *ends, *ends2; uint32_t *v0, *v1, *v2;
    SVXCHK(S->pool.get(&k_end, n)); SVXCHK(S->pool.get(&k_end2, n)); SVXCHK(S->pool.get(&k_cs, n)); SVXCHK(S->pool.get(&k_cs_g, n)); SVXCHK(S->pool.get(&k_cs2, n));
    SVXCHK(S->pool.get(&ends, n)); SVXCHK(S->pool.get(&ends2, n)); SVXCHK(S->pool.get(&v0, n)); SVXCHK(S->pool.get(&v1, n)); SVXCHK(S->pool.get(&v2, n));
    *key_out = k_cs2; *end_out = ends2;
    if (n <= 0) return SVX_OK;
    hipStream_t st = c->stream;
    k_walk_keys<<<CGRID(n), CT, 0, st>>>(t, base, n, which, rank, n_contig, k_end, k_cs, ends, v0);
    SVXCHK(svx_sort_pairs_u64(c, k_end, k_end2, v0, v1, n, 0, 64));
    k_gather_u64c<<<CGRID(n), CT, 0, st>>>(k_cs, v1, k_cs_g, n);
    SVXCHK(svx_sort_pairs_u64(c, k_cs_g, k_cs2, v1, v2, n, 0, 64));
    k_gather_i64c<<<CGRID(n), CT, 0, st>>>(ends, v2, ends2, n);
    HIPCHK(hipGetLastError());
    return SVX_OK;
}

static int combine_body(svx_ctx* c, CombineState* S, const CluPtrs& cl, const int64_t* type_count, const uint8_t* sig_aux, int64_t n_sig, int32_t n_contig,
                        const int32_t* rank, const svx_combine_params& P) {
    hipStream_t st = c->stream;
    svx_combine_stats& X = S->stats;
    int64_t base[SVX_NTYPES + 1];
    base[0] = 0;
    for (int t = 0; t < SVX_NTYPES; t++) base[t + 1] = base[t] + type_count[t];
    const int64_t n_del = type_count[SVX_DEL], n_ins = type_count[SVX_INS], n_inv = type_count[SVX_INV], n_tan = type_count[SVX_DUP_TAN],
                  n_bnd = type_count[SVX_BND], n_di = type_count[SVX_DUP_INT];
    X.n_clusters_in = base[SVX_NTYPES]; X.n_deletions = n_del;

    // ---- stage 2 ----------------------------------------------------------------------------------------------------------------
    int64_t n_new = 0;
    int64_t *mflag = nullptr, *mexcl = nullptr; int32_t *kf = nullptr, *kr = nullptr;
    if (n_ins > 0) {
        X.n_bnd_mirrored = n_bnd;
        SVXCHK(S->pool.get(&mflag, n_ins + 1)); SVXCHK(S->pool.get(&mexcl, n_ins + 1)); SVXCHK(S->pool.get(&kf, n_ins)); SVXCHK(S->pool.get(&kr, n_ins));
        if (n_bnd > 0) {
            uint64_t *bk, *bk2; uint32_t *bv, *bv2;
            SVXCHK(S->pool.get(&bk, 2 * n_bnd)); SVXCHK(S->pool.get(&bk2, 2 * n_bnd)); SVXCHK(S->pool.get(&bv, 2 * n_bnd)); SVXCHK(S->pool.get(&bv2, 2 * n_bnd));
            k_bnd_keys<<<CGRID(2 * n_bnd), CT, 0, st>>>(cl, base[SVX_BND], n_bnd, bk, bv);
            SVXCHK(svx_sort_pairs_u64(c, bk, bk2, bv, bv2, 2 * n_bnd, 0, 64));
            k_ins_merge<<<CGRID(n_ins), CT, 0, st>>>(cl, base[SVX_INS], n_ins, base[SVX_BND], n_bnd, bk2, bv2, (long long)P.trans_sv_max_distance, mflag, kf, kr);
            SVXCHK(scan_with_total(c, mflag, mexcl, n_ins));
            SVXCHK(read_word(c, mexcl + n_ins, &n_new));
        } else {
            HIPCHK(hipMemsetAsync(mflag, 0, (size_t)(n_ins + 1) * 8, st));
        }
    }
    SVXCHK(S->merged.reserve(n_new));
    SVXCHK(S->rm1_list.reserve((size_t)(n_new > 0 ? n_new : 1) * 4));
    if (n_new > 0) {
        double *prod, *mainsc;
        SVXCHK(S->pool.get(&prod, n_new)); SVXCHK(S->pool.get(&mainsc, n_new));
        k_merge_rows<<<CGRID(n_ins), CT, 0, st>>>(cl, base[SVX_INS], n_ins, base[SVX_BND], n_bnd, mflag, mexcl, kf, kr, S->merged.ptrs(), prod, mainsc, S->rm1_list.as<int32_t>());
        std::vector<double> hp((size_t)n_new), hm((size_t)n_new);
        SVXCHK(svx_d2h(hp.data(), prod, (size_t)n_new * 8, st));
        SVXCHK(svx_d2h(hm.data(), mainsc, (size_t)n_new * 8, st));
        for (int64_t j = 0; j < n_new; j++) hp[(size_t)j] = pow(hp[(size_t)j], 1.0 / 6) * hm[(size_t)j];       // libm's pow: what math.pow calls
        SVXCHK(svx_h2d(S->merged.score.p, hp.data(), (size_t)n_new * 8, st));
    }
    SVXCHK(finish_offsets(c, S->merged, n_new));
    if (n_new > 0)
        k_merge_members<<<(unsigned)((n_new + 3) / 4), CT, 0, st>>>(cl, base[SVX_INS], base[SVX_BND], n_bnd, n_new, S->rm1_list.as<int32_t>(), kf, kr,
                                                                    S->merged.member_off.as<int64_t>(), S->merged.members.as<int32_t>());
    S->merged.class_count[SVX_CAND_DUP_INT] = n_new;
    S->n_rm1 = n_new; X.n_merged = n_new; X.n_remove_1 = n_new;
    S->have_stage2 = true;

    // ---- stage 3 ----------------------------------------------------------------------------------------------------------------
    const int64_t n_from = n_di + n_new;
    X.n_insertion_from = n_from; X.n_cutpaste_pairs = n_from * n_del;
    if (n_from > 0 && n_del == 0) { HIPCHK(hipStreamSynchronize(st)); return svx_fail(SVX_E_NO_DELETION, "insertion-from clusters but no deletion cluster", __FILE__, __LINE__, hipSuccess); }
    SVXCHK(S->flagged.reserve(n_from));
    if (n_from > 0) {
        int32_t *from_s, *from_e, *dmid, *dspan; double* dmin;
        SVXCHK(S->pool.get(&from_s, n_from)); SVXCHK(S->pool.get(&from_e, n_from)); SVXCHK(S->pool.get(&dmid, n_del)); SVXCHK(S->pool.get(&dspan, n_del)); SVXCHK(S->pool.get(&dmin, n_from));
        k_flag_rows<<<CGRID(n_from), CT, 0, st>>>(cl, base[SVX_DUP_INT], n_di, S->merged.ptrs(), n_new, S->flagged.ptrs(), from_s, from_e);
        k_del_prep<<<CGRID(n_del), CT, 0, st>>>(cl.start, cl.end, base[SVX_DEL], n_del, dmid, dspan);
        HIPCHK(hipEventRecord(c->ev[22], st));
        k_cutpaste_min<<<(unsigned)((n_from + CP_FG - 1) / CP_FG), CT, 0, st>>>(dmid, dspan, n_del, from_s, from_e, n_from, P.position_distance_normalizer,
                                                                                 P.del_ins_dup_max_distance, S->flagged.aux.as<uint8_t>(), dmin);
        HIPCHK(hipEventRecord(c->ev[23], st));
    }
    SVXCHK(finish_offsets(c, S->flagged, n_from));
    if (n_from > 0)
        k_cmb_gather<<<(unsigned)((n_from + 3) / 4), CT, 0, st>>>(n_from, S->flagged.member_off.as<int64_t>(), S->flagged.msrc.as<int64_t>(), cl.members,
                                                                  S->merged.members.as<int32_t>(), S->flagged.members.as<int32_t>());
    S->flagged.class_count[SVX_CAND_DUP_INT] = n_from;

    // ---- deletion clusters with score > 0 (stream compaction, order kept) -------------------------------------------------------------------
    int64_t *dflag, *dexcl; int32_t* del_rows;
    SVXCHK(S->pool.get(&dflag, n_del + 1)); SVXCHK(S->pool.get(&dexcl, n_del + 1)); SVXCHK(S->pool.get(&del_rows, n_del));
    int64_t n_del_keep = 0;
    if (n_del > 0) {
        k_flag_positive<<<CGRID(n_del), CT, 0, st>>>(cl.score, base[SVX_DEL], n_del, dflag);
        SVXCHK(scan_with_total(c, dflag, dexcl, n_del));
        k_cmb_compact<<<CGRID(n_del), CT, 0, st>>>(n_del, dflag, dexcl, del_rows);
        SVXCHK(read_word(c, dexcl + n_del, &n_del_keep));
    }

    // ---- stage 5 (before stage 4's counts are needed: the result's DUP_INT block sits in front of DUP_TAN and INS) -----------------------
    int64_t n_final = 0, n_part = 0, n_large = 0;
    if (n_from > 0) {
        CandPtrs F = S->flagged.ptrs();
        uint64_t *pk, *pk2; uint32_t *pv, *pv2; int64_t *pflag, *pexcl, *pstart;
        SVXCHK(S->pool.get(&pk, n_from)); SVXCHK(S->pool.get(&pk2, n_from)); SVXCHK(S->pool.get(&pv, n_from)); SVXCHK(S->pool.get(&pv2, n_from));
        SVXCHK(S->pool.get(&pflag, n_from + 1)); SVXCHK(S->pool.get(&pexcl, n_from + 1));
        k_dup_keys<<<CGRID(n_from), CT, 0, st>>>(F, n_from, rank, n_contig, pk, pv);
        SVXCHK(svx_sort_pairs_u64(c, pk, pk2, pv, pv2, n_from, 0, 64));
        k_dup_part_flags<<<CGRID(n_from), CT, 0, st>>>(F, n_from, pv2, (long long)P.partition_max_distance, pflag);
        SVXCHK(scan_with_total(c, pflag, pexcl, n_from));
        SVXCHK(read_word(c, pexcl + n_from, &n_part));
        SVXCHK(S->pool.get(&pstart, n_part + 1));
        k_dup_part_starts<<<CGRID(n_from), CT, 0, st>>>(pflag, pexcl, n_from, pstart, n_part);
        std::vector<int64_t> hps((size_t)n_part + 1);
        SVXCHK(svx_d2h(hps.data(), pstart, (size_t)(n_part + 1) * 8, st));
        // the plan: which list positions every partition clusters (all of them, or random.sample's 100), and the linkage problems of the partitions with >= 2
        std::vector<int32_t> sel, prob_part, ns; std::vector<int64_t> sel_off((size_t)n_part + 1), d_off(1, 0), label_off;
        sel.reserve((size_t)n_from);
        PyRandom rng(1524u);
        for (int64_t p = 0; p < n_part; p++) {
            const int64_t lo = hps[(size_t)p], sz = hps[(size_t)p + 1] - lo;
            sel_off[(size_t)p] = (int64_t)sel.size();
            if (sz > 100) {
                int32_t pick[100];
                rng.sample100(sz, pick);
                for (int k = 0; k < 100; k++) sel.push_back((int32_t)(lo + pick[k]));
                n_large++;
            } else for (int64_t k = 0; k < sz; k++) sel.push_back((int32_t)(lo + k));
            const int64_t m = sz > 100 ? 100 : sz;
            if (m >= 2) { prob_part.push_back((int32_t)p); ns.push_back((int32_t)m); label_off.push_back(sel_off[(size_t)p]); d_off.push_back(d_off.back() + m * (m - 1) / 2); }
        }
        sel_off[(size_t)n_part] = (int64_t)sel.size();
        label_off.push_back((int64_t)sel.size());
        const int64_t nq = (int64_t)ns.size(), n_sel = (int64_t)sel.size();
        int32_t *sel_d, *prob_d, *ns_d, *labels; int64_t *sel_off_d, *d_off_d, *label_off_d, *ncl, *clu_off; double* dist;
        SVXCHK(S->pool.get(&sel_d, n_sel)); SVXCHK(S->pool.get(&prob_d, nq)); SVXCHK(S->pool.get(&ns_d, nq)); SVXCHK(S->pool.get(&labels, n_sel));
        SVXCHK(S->pool.get(&sel_off_d, n_part + 1)); SVXCHK(S->pool.get(&d_off_d, nq + 1)); SVXCHK(S->pool.get(&label_off_d, nq + 1));
        SVXCHK(S->pool.get(&ncl, n_part + 1)); SVXCHK(S->pool.get(&clu_off, n_part + 1)); SVXCHK(S->pool.get(&dist, d_off.back()));
        SVXCHK(svx_h2d(sel_d, sel.data(), (size_t)n_sel * 4, st));
        SVXCHK(svx_h2d(sel_off_d, sel_off.data(), (size_t)(n_part + 1) * 8, st));
        if (nq > 0) {
            SVXCHK(svx_h2d(prob_d, prob_part.data(), (size_t)nq * 4, st)); SVXCHK(svx_h2d(ns_d, ns.data(), (size_t)nq * 4, st));
            SVXCHK(svx_h2d(d_off_d, d_off.data(), (size_t)(nq + 1) * 8, st)); SVXCHK(svx_h2d(label_off_d, label_off.data(), (size_t)(nq + 1) * 8, st));
            k_dup_dist<<<(unsigned)nq, CT, 0, st>>>(F, pv2, sel_d, sel_off_d, prob_d, ns_d, d_off_d, P.position_distance_normalizer, dist);
            SVXCHK(svx_linkage_batch(c, nq, ns_d, d_off_d, dist, P.cluster_max_distance, label_off_d, labels));
        }
        k_dup_ncl<<<CGRID(n_part), CT, 0, st>>>(n_part, sel_off_d, labels, ncl);
        SVXCHK(scan_with_total(c, ncl, clu_off, n_part));
        SVXCHK(read_word(c, clu_off + n_part, &n_final));
        SVXCHK(S->fdup.reserve(n_final));
        k_dup_consolidate<<<CGRID(n_part), CT, 0, st>>>(F, pv2, sel_d, sel_off_d, labels, n_part, clu_off, S->fdup.ptrs(), false);
        SVXCHK(finish_offsets(c, S->fdup, n_final));
        k_dup_consolidate<<<CGRID(n_part), CT, 0, st>>>(F, pv2, sel_d, sel_off_d, labels, n_part, clu_off, S->fdup.ptrs(), true);
    } else {
        SVXCHK(S->fdup.reserve(0));
        SVXCHK(finish_offsets(c, S->fdup, 0));
    }
    X.n_dup_partitions = n_part; X.n_dup_large_partitions = n_large;

    // ---- stage 4 ----------------------------------------------------------------------------------------------------------------
    // the tandem candidates are needed as candidates (clamped start, copies): emitted into a scratch table first
    CandTab& R = S->result;
    int64_t n_ins_keep = 0, n_rm2 = 0;
    int64_t *keep = nullptr, *kexcl = nullptr, *r2flag = nullptr, *r2excl = nullptr; int32_t* ins_rows = nullptr; uint8_t* rm2 = nullptr;
    SVXCHK(S->pool.get(&keep, n_ins + 1)); SVXCHK(S->pool.get(&kexcl, n_ins + 1)); SVXCHK(S->pool.get(&r2flag, n_ins + 1)); SVXCHK(S->pool.get(&r2excl, n_ins + 1));
    SVXCHK(S->pool.get(&ins_rows, n_ins)); SVXCHK(S->pool.get(&rm2, n_ins));
    CandTab& tan_tab = S->tan;
    SVXCHK(tan_tab.reserve(n_tan));
    if (n_tan > 0) k_cmb_emit<<<CGRID(n_tan), CT, 0, st>>>(cl, SVX_CAND_DUP_TAN, n_tan, nullptr, base[SVX_DUP_TAN], tan_tab.ptrs(), 0, sig_aux, n_sig);
    if (n_ins > 0) {
        uint64_t *ik, *tk; long long *ie, *te;
        SVXCHK(sort_destinations(c, S, S->flagged.ptrs(), 0, n_from, 0, rank, n_contig, &ik, &ie));
        SVXCHK(sort_destinations(c, S, tan_tab.ptrs(), 0, n_tan, 1, rank, n_contig, &tk, &te));
        k_walk<<<1, 64, 0, st>>>(cl.contig + base[SVX_INS], cl.start + base[SVX_INS], cl.end + base[SVX_INS], n_ins, rank, n_contig, ik, ie, n_from, tk, te, n_tan, rm2);
        k_ins_keep<<<CGRID(n_ins), CT, 0, st>>>(cl.score, base[SVX_INS], n_ins, mflag, rm2, keep, r2flag);
        SVXCHK(scan_with_total(c, keep, kexcl, n_ins));
        SVXCHK(scan_with_total(c, r2flag, r2excl, n_ins));
        k_cmb_compact<<<CGRID(n_ins), CT, 0, st>>>(n_ins, keep, kexcl, ins_rows);
        int64_t w[2] = {0, 0};
        SVXCHK(svx_mail_read2(c, st, kexcl + n_ins, 1, &w[0], r2excl + n_ins, 1, &w[1]));
        n_ins_keep = w[0]; n_rm2 = w[1];
    }
    SVXCHK(S->rm2_list.reserve((size_t)(n_rm2 > 0 ? n_rm2 : 1) * 4));
    if (n_rm2 > 0) k_cmb_compact<<<CGRID(n_ins), CT, 0, st>>>(n_ins, r2flag, r2excl, S->rm2_list.as<int32_t>());
    S->n_rm2 = n_rm2; X.n_remove_2 = n_rm2;

    // ---- the candidate table, in combine_clusters' return order ---------------------------------------------------------------------------
    const int64_t cnt[SVX_NCAND] = {n_del_keep, n_inv, n_final, n_tan, n_ins_keep, n_bnd};
    int64_t ob[SVX_NCAND + 1];
    ob[0] = 0;
    for (int k = 0; k < SVX_NCAND; k++) { ob[k + 1] = ob[k] + cnt[k]; R.class_count[k] = cnt[k]; }
    const int64_t n_out = ob[SVX_NCAND];
    SVXCHK(R.reserve(n_out));
    CandPtrs RP = R.ptrs();
    if (n_del_keep > 0) k_cmb_emit<<<CGRID(n_del_keep), CT, 0, st>>>(cl, SVX_CAND_DEL, n_del_keep, del_rows, base[SVX_DEL], RP, ob[SVX_CAND_DEL], sig_aux, n_sig);
    if (n_inv > 0) k_cmb_emit<<<CGRID(n_inv), CT, 0, st>>>(cl, SVX_CAND_INV, n_inv, nullptr, base[SVX_INV], RP, ob[SVX_CAND_INV], sig_aux, n_sig);
    if (n_final > 0) k_cmb_copy_rows<<<CGRID(n_final), CT, 0, st>>>(S->fdup.ptrs(), n_final, RP, ob[SVX_CAND_DUP_INT]);
    if (n_tan > 0) k_cmb_emit<<<CGRID(n_tan), CT, 0, st>>>(cl, SVX_CAND_DUP_TAN, n_tan, nullptr, base[SVX_DUP_TAN], RP, ob[SVX_CAND_DUP_TAN], sig_aux, n_sig);
    if (n_ins_keep > 0) k_cmb_emit<<<CGRID(n_ins_keep), CT, 0, st>>>(cl, SVX_CAND_INS, n_ins_keep, ins_rows, base[SVX_INS], RP, ob[SVX_CAND_INS], sig_aux, n_sig);
    if (n_bnd > 0) k_cmb_emit<<<CGRID(n_bnd), CT, 0, st>>>(cl, SVX_CAND_BND, n_bnd, nullptr, base[SVX_BND], RP, ob[SVX_CAND_BND], sig_aux, n_sig);
    SVXCHK(finish_offsets(c, R, n_out));
    if (n_out > 0)
        k_cmb_gather<<<(unsigned)((n_out + 3) / 4), CT, 0, st>>>(n_out, R.member_off.as<int64_t>(), R.msrc.as<int64_t>(), cl.members, S->fdup.members.as<int32_t>(),
                                                                R.members.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    X.n_candidates = n_out; X.n_candidate_members = R.n_members;
    S->have_result = true;
    if (n_from > 0) {
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev[22], c->ev[23])); X.t_cutpaste_ms = ms;
        std::vector<uint8_t> a((size_t)n_from);
        SVXCHK(svx_d2h(a.data(), S->flagged.aux.p, (size_t)n_from, st));
        for (uint8_t v : a) X.n_cutpaste += v & 1;
    }
    return SVX_OK;
}

extern "C" int svx_combine(svx_ctx* c, int source, const svx_cluster_view* cv, const uint8_t* sig_aux, int64_t n_sig, int32_t on_device, int32_t n_contig,
                           const int32_t* contig_rank_host, const svx_combine_params* p) {
    if (!c || !p || n_contig < 0 || n_contig >= (1 << 30) || (n_contig && !contig_rank_host)) return svx_fail(SVX_E_ARG, "svx_combine: bad argument", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    if (!c->combine) c->combine = new CombineState();
    CombineState* S = c->combine;
    S->pool.reset(); S->have_stage2 = false; S->have_result = false; S->n_rm1 = S->n_rm2 = 0;
    S->from_resident = source == 0; S->cluster_call = c->cluster_calls;
    c->combine_calls++;                                             // (genotype columns of an earlier candidate table are void from here on: genotype.hip)
    memset(&S->stats, 0, sizeof S->stats);
    for (CandTab* t : {&S->merged, &S->flagged, &S->fdup, &S->result}) { t->n = t->n_members = 0; for (auto& x : t->class_count) x = 0; }
    hipStream_t st = c->stream;
    CluPtrs cl; int64_t type_count[SVX_NTYPES];
    if (source == 0) {
        if (c->cluster_calls <= 0) return svx_fail(SVX_E_STATE, "no resident clusters: run svx_cluster first", __FILE__, __LINE__, hipSuccess);
        const DevClusters& v = c->clu;
        cl.type = v.type.as<uint8_t>(); cl.contig = v.contig.as<int32_t>(); cl.start = v.start.as<int32_t>(); cl.end = v.end.as<int32_t>();
        cl.contig2 = v.contig2.as<int32_t>(); cl.start2 = v.start2.as<int32_t>(); cl.end2 = v.end2.as<int32_t>(); cl.aux = v.aux.as<uint8_t>();
        cl.score = v.score.as<double>(); cl.std_span = v.std_span.as<double>(); cl.std_pos = v.std_pos.as<double>(); cl.member_off = v.member_off.as<int64_t>();
        cl.members = v.members.as<int32_t>();
        for (int t = 0; t < SVX_NTYPES; t++) type_count[t] = v.type_count[t];
        sig_aux = c->last_cluster_aux; n_sig = c->last_cluster_source_n;
        if (v.n > 0 && !cl.member_off) return svx_fail(SVX_E_STATE, "no resident clusters: run svx_cluster first", __FILE__, __LINE__, hipSuccess);
    } else if (source == 2) {
        if (!cv || n_sig < 0 || (n_sig && !sig_aux)) return svx_fail(SVX_E_ARG, "svx_combine: source 2 needs a cluster table and the signatures' aux column", __FILE__, __LINE__, hipSuccess);
        int64_t total = 0;
        for (int t = 0; t < SVX_NTYPES; t++) { type_count[t] = cv->type_count[t]; if (type_count[t] < 0) return svx_fail(SVX_E_ARG, "svx_combine: negative type_count", __FILE__, __LINE__, hipSuccess); total += type_count[t]; }
        if (total != cv->n || cv->n_members < 0) return svx_fail(SVX_E_ARG, "svx_combine: type_count does not add up to n", __FILE__, __LINE__, hipSuccess);
        if (on_device) {
            cl.type = cv->type; cl.contig = cv->contig; cl.start = cv->start; cl.end = cv->end; cl.contig2 = cv->contig2; cl.start2 = cv->start2; cl.end2 = cv->end2;
            cl.aux = cv->aux; cl.score = cv->score; cl.std_span = cv->std_span; cl.std_pos = cv->std_pos; cl.member_off = cv->member_off; cl.members = cv->members;
        } else {
            const size_t n = (size_t)cv->n, nm = (size_t)cv->n_members;
            if (n && cv->member_off[n] != cv->n_members) return svx_fail(SVX_E_ARG, "svx_combine: member_off[n] != n_members", __FILE__, __LINE__, hipSuccess);
            const void* src[13] = {cv->type, cv->contig, cv->start, cv->end, cv->contig2, cv->start2, cv->end2, cv->aux, cv->score, cv->std_span, cv->std_pos, cv->member_off, cv->members};
            const size_t bytes[13] = {n, n * 4, n * 4, n * 4, n * 4, n * 4, n * 4, n, n * 8, n * 8, n * 8, (n + 1) * 8, nm * 4};
            HostCopy hc(st);
            for (int k = 0; k < 13; k++) {
                SVXCHK(S->in[k].reserve(bytes[k] ? bytes[k] : 8));
                if (k == 11 && n == 0) { HIPCHK(hipMemsetAsync(S->in[k].p, 0, 8, st)); continue; }
                if (bytes[k]) { if (!src[k]) return svx_fail(SVX_E_ARG, "svx_combine: a cluster column is missing", __FILE__, __LINE__, hipSuccess); SVXCHK(hc.h2d(S->in[k].p, src[k], bytes[k])); }
            }
            SVXCHK(S->in_aux.reserve(n_sig ? (size_t)n_sig : 8));
            if (n_sig) SVXCHK(hc.h2d(S->in_aux.p, sig_aux, (size_t)n_sig));
            SVXCHK(hc.finish());
            cl.type = S->in[0].as<uint8_t>(); cl.contig = S->in[1].as<int32_t>(); cl.start = S->in[2].as<int32_t>(); cl.end = S->in[3].as<int32_t>();
            cl.contig2 = S->in[4].as<int32_t>(); cl.start2 = S->in[5].as<int32_t>(); cl.end2 = S->in[6].as<int32_t>(); cl.aux = S->in[7].as<uint8_t>();
            cl.score = S->in[8].as<double>(); cl.std_span = S->in[9].as<double>(); cl.std_pos = S->in[10].as<double>(); cl.member_off = S->in[11].as<int64_t>();
            cl.members = S->in[12].as<int32_t>();
            sig_aux = S->in_aux.as<uint8_t>();
        }
    } else return svx_fail(SVX_E_ARG, "svx_combine: source must be 0 or 2", __FILE__, __LINE__, hipSuccess);
    SVXCHK(S->rank.reserve((size_t)(n_contig ? n_contig : 1) * 4));
    if (n_contig) SVXCHK(svx_h2d(S->rank.p, contig_rank_host, (size_t)n_contig * 4, st));
    HIPCHK(hipEventRecord(c->ev[20], st));
    const int rc = combine_body(c, S, cl, type_count, sig_aux, n_sig, n_contig, S->rank.as<int32_t>(), *p);
    if (rc == SVX_OK) {
        HIPCHK(hipEventRecord(c->ev[21], st));
        HIPCHK(hipEventSynchronize(c->ev[21]));
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev[20], c->ev[21])); S->stats.t_combine_ms = ms;
    }
    return rc;
}

bool svx_combine_resident(svx_ctx* c, CandDev* o) {
    if (!c->combine || !c->combine->have_result) return false;
    const CombineState* S = c->combine;
    const CandTab& t = S->result;
    const CandPtrs p = t.ptrs();
    o->n = t.n; o->n_members = t.n_members;
    for (int k = 0; k < SVX_NCAND; k++) o->class_count[k] = t.class_count[k];
    o->cls = p.cls; o->contig = p.contig; o->start = p.start; o->end = p.end; o->contig2 = p.contig2; o->start2 = p.start2; o->end2 = p.end2; o->aux = p.aux;
    o->copies = p.copies; o->score = p.score; o->std_span = p.std_span; o->std_pos = p.std_pos; o->member_off = p.member_off; o->members = p.members;
    o->from_resident = S->from_resident; o->cluster_call = S->cluster_call;
    return true;
}

extern "C" int svx_combine_count(svx_ctx* c, int64_t* n_candidates, int64_t* n_members) {
    if (!c || !c->combine || !c->combine->have_result) return svx_fail(SVX_E_STATE, "no candidates: run svx_combine first", __FILE__, __LINE__, hipSuccess);
    if (n_candidates) *n_candidates = c->combine->result.n;
    if (n_members) *n_members = c->combine->result.n_members;
    return SVX_OK;
}

static int fetch_table(svx_ctx* c, const CandTab& t, svx_candidate_view* o) {
    if (!o) return SVX_OK;
    const size_t n = (size_t)t.n;
    hipStream_t st = c->stream;
    HostCopy hc(st);
#define D2H(dst, buf, bytes) do { if ((bytes) && (dst)) SVXCHK(hc.out((dst), (buf).p, (bytes))); } while (0)
    D2H(o->cls, t.cls, n); D2H(o->aux, t.aux, n); D2H(o->contig, t.contig, n * 4); D2H(o->start, t.start, n * 4); D2H(o->end, t.end, n * 4);
    D2H(o->contig2, t.contig2, n * 4); D2H(o->start2, t.start2, n * 4); D2H(o->end2, t.end2, n * 4); D2H(o->copies, t.copies, n * 4);
    D2H(o->score, t.score, n * 8); D2H(o->std_span, t.std_span, n * 8); D2H(o->std_pos, t.std_pos, n * 8);
    D2H(o->member_off, t.member_off, (n + 1) * 8);
    D2H(o->members, t.members, (size_t)t.n_members * 4);
#undef D2H
    SVXCHK(hc.finish());
    HIPCHK(hipStreamSynchronize(st));
    o->n = t.n; o->n_members = t.n_members;
    for (int k = 0; k < SVX_NCAND; k++) o->class_count[k] = t.class_count[k];
    return SVX_OK;
}

extern "C" int svx_combine_fetch(svx_ctx* c, svx_candidate_view* o) {
    if (!c || !o || !c->combine || !c->combine->have_result) return svx_fail(SVX_E_STATE, "no candidates: run svx_combine first", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    return fetch_table(c, c->combine->result, o);
}

extern "C" int svx_combine_stages_fetch(svx_ctx* c, svx_candidate_view* merged, int64_t* n_remove_1, int32_t* remove_1, int64_t* n_remove_2, int32_t* remove_2,
                                        svx_candidate_view* flagged) {
    if (!c || !c->combine || !c->combine->have_stage2) return svx_fail(SVX_E_STATE, "no stages: run svx_combine first", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    CombineState* S = c->combine;
    SVXCHK(fetch_table(c, S->merged, merged));
    if (n_remove_1) *n_remove_1 = S->n_rm1;
    if (remove_1 && S->n_rm1) SVXCHK(svx_d2h(remove_1, S->rm1_list.p, (size_t)S->n_rm1 * 4, c->stream));
    if (!S->have_result) {                         // SVX_E_NO_DELETION: stage 2 only
        if (n_remove_2) *n_remove_2 = 0;
        if (flagged) { flagged->n = 0; flagged->n_members = 0; for (auto& x : flagged->class_count) x = 0; }
        return SVX_OK;
    }
    if (n_remove_2) *n_remove_2 = S->n_rm2;
    if (remove_2 && S->n_rm2) SVXCHK(svx_d2h(remove_2, S->rm2_list.p, (size_t)S->n_rm2 * 4, c->stream));
    return fetch_table(c, S->flagged, flagged);
}

extern "C" int svx_combine_get_stats(svx_ctx* c, svx_combine_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->combine) *out = c->combine->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
