// genotype.hip - reads supporting the reference allele around every candidate.
//
// Replaces the inner loop of genotype() (src/svim/SVIM_genotyping.py:34-93): for every candidate the reference re-opens the
// BAM index (bam.fetch(contig, start-1000, end+1000), :48), walks at most 500 eligible alignments (:56-68: not a read of the
// variant, mapped, not secondary, mapq >= min_mapq) and collects the names of those that span the locus (:70-77).  Here the
// alignment records are a structure-of-arrays in HBM in file order; one wavefront per candidate binary-searches its window and
// walks it 64 records at a time.  HBM-bound (20 B per record visited), latency-dominated for the short walks of real data.
#include "common.hpp"
#include "hostcopy.hpp"
#include <cmath>

// running maximum of end_or_pos1 inside every contig: the first record that can overlap a window start is found by bisection
__global__ __launch_bounds__(64) void k_end_prefmax(AlnIndexDev ix, int32_t* prefmax) {       // one wave per contig, 64 records per step
    const int c = blockIdx.x;
    if (c >= ix.n_contig) return;
    const int lane = lane_id();
    const long long first = ix.contig_first[c], last = ix.contig_first[c + 1];
    int32_t carry = INT32_MIN;
    for (long long base = first; base < last; base += 64) {
        const long long i = base + lane;
        int32_t v = INT32_MIN;
        if (i < last) { v = ix.end[i]; if (v <= ix.pos[i]) v = ix.pos[i] + 1; }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int32_t u = __shfl_up(v, o, 64); if (lane >= o && u > v) v = u; }
        if (carry > v) v = carry;
        if (i < last) prefmax[i] = v;
        carry = __shfl(v, 63, 64);
    }
}

#define GENO_LIMIT 500

__global__ __launch_bounds__(64) void k_genotype(AlnIndexDev ix, int mode, long long n_cand, const int32_t* cand_tid, const int32_t* cand_start,
                                                 const int32_t* cand_end, const int64_t* member_off, const int32_t* member_names, int min_mapq,
                                                 int32_t* out_ref) {
    __shared__ int32_t names[GENO_LIMIT + 64];
    const long long c = blockIdx.x;
    if (c >= n_cand) return;
    const int lane = lane_id();
    const int tid = cand_tid[c];
    if (tid < 0 || tid >= ix.n_contig) { if (lane == 0) out_ref[c] = 0; return; }
    const long long start = cand_start[c], end = cand_end[c];
    const long long clen = ix.contig_len[tid];
    const long long ws = start - 1000 > 0 ? start - 1000 : 0, we = end + 1000 < clen ? end + 1000 : clen;      // :48
    const long long first = ix.contig_first[tid], last = ix.contig_first[tid + 1];
    // records [i_lo, i_hi): the first whose running end maximum exceeds ws ... the first with pos >= we
    long long lo = first, hi = last;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)ix.end_prefmax[mid] > ws) hi = mid; else lo = mid + 1; }
    const long long i_lo = lo;
    lo = first; hi = last;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)ix.pos[mid] >= we) hi = mid; else lo = mid + 1; }
    const long long i_hi = ws < we ? lo : i_lo;
    const long long m0 = member_off[c], mn = member_off[c + 1] - m0;
    const long long mo2 = end - start < 4000 ? end - start : 4000;         // 2 * min((end - start) / 2, 2000)  (:71)
    int counted = 0, n_names = 0;
    for (long long base = i_lo; base < i_hi && counted < GENO_LIMIT; base += 64) {
        const long long i = base + lane;
        bool pass = false, support = false;
        int32_t name = -1;
        if (i < i_hi) {
            const long long rs = ix.pos[i];
            long long re = ix.end[i];
            const long long endp = re > rs ? re : rs + 1;
            if (endp > ws) {                                               // overlaps the fetched region
                name = ix.name_id[i];
                long long a = 0, b = mn;                                   // current_alignment.query_name in reads_supporting_variant (:63)
                while (a < b) { const long long mid = (a + b) >> 1; if (member_names[m0 + mid] < name) a = mid + 1; else b = mid; }
                const bool in_variant = a < mn && member_names[m0 + a] == name;
                const unsigned flag = ix.flag[i];
                pass = !in_variant && !(flag & 0x4u) && !(flag & 0x100u) && (int)ix.mapq[i] >= min_mapq;      // :65
                if (mode == 0) support = (2 * rs < 2 * end - mo2 && re > end + 100) || (rs < start - 100 && 2 * re > 2 * start + mo2);   // :72-74
                else support = rs < start - 100 && re > end + 100;                                                                      // :76
            }
        }
        const unsigned long long pm = __ballot(pass);
        const int ordinal = counted + (int)__popcll(pm & lanemask_lt()) + 1;          // aln_no after this alignment (:68)
        const bool take = pass && ordinal <= GENO_LIMIT && support;
        const unsigned long long tm = __ballot(take);
        if (take) names[n_names + (int)__popcll(tm & lanemask_lt())] = name;
        n_names += (int)__popcll(tm);
        counted += (int)__popcll(pm);
    }
    __syncthreads();
    // len(set(names))
    int distinct = 0;
    for (int j = lane; j < n_names; j += 64) {
        const int32_t v = names[j];
        bool first_seen = true;
        for (int k = 0; k < j; k++) if (names[k] == v) { first_seen = false; break; }
        distinct += first_seen;
    }
    distinct = wave_sum_i32(distinct);
    if (lane == 0) out_ref[c] = distinct;
}

int svx_set_alignment_index_impl(svx_ctx* c, const svx_aln_index* h) {
    hipStream_t st = c->stream;
    const size_t n = (size_t)h->n, nc = (size_t)h->n_contig;
    DevBuf* b = c->geno;
    struct Up { DevBuf* d; const void* src; size_t bytes; } ups[] = {
        {&b[0], h->contig_first, (nc + 1) * 8}, {&b[1], h->contig_len, nc * 8}, {&b[2], h->pos, n * 4}, {&b[3], h->end, n * 4},
        {&b[4], h->flag, n * 2}, {&b[5], h->mapq, n}, {&b[6], h->name_id, n * 4}};
    for (auto& u : ups) {
        SVXCHK(u.d->reserve(u.bytes + 64));
        SVXCHK(svx_h2d(u.d->p, u.src, u.bytes, st));
    }
    SVXCHK(b[7].reserve(n * 4 + 64));
    c->geno_n = h->n; c->geno_contigs = h->n_contig;
    AlnIndexDev ix{h->n, h->n_contig, b[0].as<int64_t>(), b[1].as<int64_t>(), b[2].as<int32_t>(), b[3].as<int32_t>(), b[7].as<int32_t>(),
                   b[4].as<uint16_t>(), b[5].as<uint8_t>(), b[6].as<int32_t>()};
    if (h->n_contig > 0) k_end_prefmax<<<(unsigned)h->n_contig, 64, 0, st>>>(ix, b[7].as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return SVX_OK;
}

int svx_genotype_impl(svx_ctx* c, int32_t mode, int64_t n_cand, const int32_t* tid, const int32_t* start, const int32_t* end, const int64_t* moff,
                      const int32_t* mnames, int32_t min_mapq, int32_t* out) {
    if (c->geno_contigs < 0) return svx_fail(SVX_E_STATE, "svx_set_alignment_index must precede svx_genotype", __FILE__, __LINE__, hipSuccess);
    if (n_cand <= 0) return SVX_OK;
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_cand, nm = (size_t)moff[n_cand];
    DevBuf* b = c->geno;
    SVXCHK(b[8].reserve(n * 4 * 4 + 64)); SVXCHK(b[9].reserve((n + 1) * 8 + 64)); SVXCHK(b[10].reserve(nm * 4 + 64));
    int32_t* d_tid = b[8].as<int32_t>(); int32_t* d_start = d_tid + n; int32_t* d_end = d_start + n; int32_t* d_out = d_end + n;
    HostCopy hc(st);
    SVXCHK(hc.h2d(d_tid, tid, n * 4)); SVXCHK(hc.h2d(d_start, start, n * 4)); SVXCHK(hc.h2d(d_end, end, n * 4));
    SVXCHK(hc.h2d(b[9].p, moff, (n + 1) * 8)); SVXCHK(hc.h2d(b[10].p, mnames, nm * 4));
    AlnIndexDev ix{c->geno_n, c->geno_contigs, b[0].as<int64_t>(), b[1].as<int64_t>(), b[2].as<int32_t>(), b[3].as<int32_t>(), b[7].as<int32_t>(),
                   b[4].as<uint16_t>(), b[5].as<uint8_t>(), b[6].as<int32_t>()};
    k_genotype<<<(unsigned)n_cand, 64, 0, st>>>(ix, mode, n_cand, d_tid, d_start, d_end, b[9].as<int64_t>(), b[10].as<int32_t>(), min_mapq, d_out);
    HIPCHK(hipGetLastError());
    SVXCHK(hc.d2h(out, d_out, n * 4));
    return hc.finish();
}

// ---------------------------------------------------------------------------------------------------------
// GENOTYPE from resident tables: candidate table x resident alignment table (alnindex.hip) -> the GT:DP:AD columns, nothing between them on the host.
//   k_geno_loci      class and score select (:38-46): DEL / INV take the source start..end, INS / DUP_INT the destination start with end = start; every
//                    other row, and a row with score < minimum_score, gets contig -1 - the walk returns at once for it
//   distinct         reads_supporting_variant (:50): the distinct read ids of the members, by the sort of (candidate << 32 | read id) that the VCF text
//                    uses for SUPPORT (svx_distinct_member_ids); k_geno_compact keeps the first of every run - per candidate a sorted id list
//   k_genotype       the walk, per class range of the table (it is grouped by class)
//   k_geno_call      the call from the two counts (:79-93); support_fraction is ONE FP64 division
// ---------------------------------------------------------------------------------------------------------
struct GenoState {
    ScratchPool<32> pool{"genotype"};
    DevBuf gt, ref_reads, alt_reads, frac;                       // the resident columns
    int64_t n = 0; bool have = false; int source = -1; long long combine_call = 0, cluster_call = 0;
    hipEvent_t ev[6]; bool have_ev = false;
    svx_genotype_stats stats;
};
void svx_genotype_release(svx_ctx* c) {
    GenoState* S = c->genores;
    if (!S) return;
    S->pool.release();
    S->gt.release(); S->ref_reads.release(); S->alt_reads.release(); S->frac.release();
    if (S->have_ev) for (auto& e : S->ev) (void)hipEventDestroy(e);
    delete S;
    c->genores = nullptr;
}
// the columns are those of the candidate table the context holds now: nothing has been combined or clustered since
static bool geno_current(const svx_ctx* c, const GenoState* S) {
    return S && S->have && S->combine_call == c->combine_calls && S->cluster_call == c->cluster_calls;
}
bool svx_genotype_columns(svx_ctx* c, int64_t n_cand, const uint8_t** gt, const int32_t** rr, const int32_t** ar) {
    const GenoState* S = c->genores;
    if (!geno_current(c, S) || S->source != 0 || S->n != n_cand) return false;
    *gt = S->gt.as<uint8_t>(); *rr = S->ref_reads.as<int32_t>(); *ar = S->alt_reads.as<int32_t>();
    return true;
}

struct GenoCand {
    long long n;
    const uint8_t* cls; const int32_t *contig, *start, *end, *contig2, *start2; const double* score;
};
__global__ void k_geno_loci(GenoCand t, double minimum_score, int32_t* tid, int32_t* start, int32_t* end, uint8_t* sel) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n) return;
    const int k = t.cls[i];
    const bool point = k == SVX_CAND_INS || k == SVX_CAND_DUP_INT;
    const bool on = (point || k == SVX_CAND_DEL || k == SVX_CAND_INV) && !(t.score[i] < minimum_score);        // :38-39
    int32_t c = -1, s = 0, e = 0;
    if (on) {
        if (point) { c = t.contig2[i]; s = t.start2[i]; e = s; }                                               // :43-46
        else { c = t.contig[i]; s = t.start[i]; e = t.end[i]; }
    }
    tid[i] = c; start[i] = s; end[i] = e; sel[i] = on ? 1 : 0;
}
// the first pair of every run of the sorted (candidate << 32 | read id) list: ids[ex[j]]; a read id that is no id sets *err
__global__ void k_geno_compact(long long nm, const uint64_t* key, const int32_t* flag, const int64_t* ex, int32_t* ids, int* err) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nm || !flag[j]) return;
    const uint32_t id = (uint32_t)key[j];
    if (id > 0x7fffffffu) atomicOr(err, 2);
    ids[ex[j]] = (int32_t)id;
}
// where every candidate's ids start in the compacted list: the prefix sum at its first member
__global__ void k_geno_offsets(long long n, const int64_t* member_off, const int64_t* ex, int64_t* ids_off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) ids_off[i] = ex[member_off[i]];
}
__global__ void k_geno_call(long long n, const uint8_t* sel, const int64_t* ids_off, const int32_t* ref, svx_genotype_params P, uint8_t* gt, int32_t* ref_reads,
                            int32_t* alt_reads, double* frac) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!sel[i]) { gt[i] = 0; ref_reads[i] = -1; alt_reads[i] = -1; frac[i] = NAN; return; }
    const long long alt = ids_off[i + 1] - ids_off[i], rf = ref[i], total = alt + rf;
    double f = NAN; int g = 0;
    if (total > 0) f = (double)alt / (double)total;                                    // :80, :90
    if (total >= P.minimum_depth && total > 0) {                                       // :79-88
        if (f >= P.homozygous_threshold) g = 3;
        else if (f >= P.heterozygous_threshold) g = 2;
        else if (f < P.heterozygous_threshold) g = 1;
    }
    gt[i] = (uint8_t)g; ref_reads[i] = (int32_t)rf; alt_reads[i] = (int32_t)alt; frac[i] = f;
}

extern "C" int svx_genotype_resident(svx_ctx* c, int source, const svx_candidate_view* cv, const int32_t* sig_read_id, int64_t n_sig, int32_t n_contig,
                                     const int64_t* contig_len, const svx_genotype_params* pp) {
    if (!c || !pp || n_contig < 0 || (n_contig && !contig_len)) return svx_fail(SVX_E_ARG, "svx_genotype_resident: bad argument", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    if (!c->genores) c->genores = new GenoState();
    GenoState* S = c->genores;
    if (!S->have_ev) { for (auto& e : S->ev) HIPCHK(hipEventCreate(&e)); S->have_ev = true; }
    S->pool.reset(); S->have = false; S->n = 0;
    memset(&S->stats, 0, sizeof S->stats);
    const svx_genotype_params P = *pp;
    hipStream_t st = c->stream;
    HIPCHK(hipEventRecord(S->ev[0], st));
    GenoCand t; memset(&t, 0, sizeof t);
    const int64_t* member_off = nullptr; const int32_t* members = nullptr; const int32_t* rid = nullptr;
    long long nm = 0, ns = 0;
    int64_t class_count[SVX_NCAND];
    if (source == 0) {
        CandDev cd;
        if (!svx_combine_resident(c, &cd)) return svx_fail(SVX_E_STATE, "svx_genotype_resident: no resident candidates: run svx_combine first", __FILE__, __LINE__, hipSuccess);
        if (!cd.from_resident || cd.cluster_call != c->cluster_calls || (cd.n_members > 0 && !c->last_cluster_read_id))
            return svx_fail(SVX_E_STATE, "svx_genotype_resident: the signature table the resident candidates' members index is gone (svx_combine source 0 of the last svx_cluster is required)",
                            __FILE__, __LINE__, hipSuccess);
        t.n = cd.n; t.cls = cd.cls; t.contig = cd.contig; t.start = cd.start; t.end = cd.end; t.contig2 = cd.contig2; t.start2 = cd.start2; t.score = cd.score;
        member_off = cd.member_off; members = cd.members; nm = cd.n_members; rid = c->last_cluster_read_id; ns = c->last_cluster_source_n;
        for (int k = 0; k < SVX_NCAND; k++) class_count[k] = cd.class_count[k];
    } else if (source == 2) {
        if (!cv || cv->n < 0 || cv->n_members < 0 || n_sig < 0 || (n_sig && !sig_read_id))
            return svx_fail(SVX_E_ARG, "svx_genotype_resident: source 2 needs a candidate table and the read ids of its signatures in host memory", __FILE__, __LINE__, hipSuccess);
        const size_t n = (size_t)cv->n, m = (size_t)cv->n_members;
        int64_t total = 0;
        for (int k = 0; k < SVX_NCAND; k++) { class_count[k] = cv->class_count[k]; if (class_count[k] < 0) return svx_fail(SVX_E_ARG, "svx_genotype_resident: negative class_count", __FILE__, __LINE__, hipSuccess); total += class_count[k]; }
        if (total != cv->n) return svx_fail(SVX_E_ARG, "svx_genotype_resident: class_count does not add up to n", __FILE__, __LINE__, hipSuccess);
        if (n && (!cv->cls || !cv->contig || !cv->start || !cv->end || !cv->contig2 || !cv->start2 || !cv->score))
            return svx_fail(SVX_E_ARG, "svx_genotype_resident: a candidate column is missing", __FILE__, __LINE__, hipSuccess);
        if (!cv->member_off || (m && !cv->members) || cv->member_off[0] != 0 || cv->member_off[n] != cv->n_members)
            return svx_fail(SVX_E_ARG, "svx_genotype_resident: member_off does not describe n_members members", __FILE__, __LINE__, hipSuccess);
        for (size_t i = 0, k = 0, hi = (size_t)class_count[0]; i < n; i++) {
            while (k < SVX_NCAND && i >= hi) { k++; if (k < SVX_NCAND) hi += (size_t)class_count[k]; }
            if (k >= SVX_NCAND || cv->cls[i] != k) return svx_fail(SVX_E_ARG, "svx_genotype_resident: the candidate table is not grouped by class as class_count says", __FILE__, __LINE__, hipSuccess);
            if (cv->member_off[i + 1] < cv->member_off[i]) return svx_fail(SVX_E_ARG, "svx_genotype_resident: member_off decreases", __FILE__, __LINE__, hipSuccess);
        }
        HostCopy hc(st);
#define UP(dst, type, host, count) do { type* d_; SVXCHK(S->pool.get(&d_, (count))); if ((count)) SVXCHK(hc.h2d(d_, (host), (size_t)(count) * sizeof(type))); dst = d_; } while (0)
        UP(t.cls, uint8_t, cv->cls, n); UP(t.contig, int32_t, cv->contig, n); UP(t.start, int32_t, cv->start, n); UP(t.end, int32_t, cv->end, n);
        UP(t.contig2, int32_t, cv->contig2, n); UP(t.start2, int32_t, cv->start2, n); UP(t.score, double, cv->score, n);
        UP(member_off, int64_t, cv->member_off, n + 1); UP(members, int32_t, cv->members, m); UP(rid, int32_t, sig_read_id, (size_t)n_sig);
#undef UP
        SVXCHK(hc.finish());
        t.n = cv->n; nm = cv->n_members; ns = n_sig;
    } else return svx_fail(SVX_E_ARG, "svx_genotype_resident: source must be 0 or 2", __FILE__, __LINE__, hipSuccess);
    const long long n = t.n;
    if (n >= (1ll << 30) || nm >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_genotype_resident: table too large", __FILE__, __LINE__, hipSuccess);
    AlnIndexDev ix;
    SVXCHK(svx_aln_table_index(c, n_contig, contig_len, &ix));
    HIPCHK(hipEventRecord(S->ev[1], st));
    SVXCHK(S->gt.reserve((size_t)n + 64)); SVXCHK(S->ref_reads.reserve((size_t)n * 4 + 64)); SVXCHK(S->alt_reads.reserve((size_t)n * 4 + 64)); SVXCHK(S->frac.reserve((size_t)n * 8 + 64));
    S->stats.n_candidates = n; S->stats.n_members = nm; S->stats.n_alignments = ix.n;
    if (n > 0) {
        const unsigned grid = (unsigned)((n + 255) / 256);
        int32_t *tid, *start, *end, *ref, *ids; uint8_t *sel, *zbad; int64_t* ids_off; int* err;
        SVXCHK(S->pool.get(&tid, n)); SVXCHK(S->pool.get(&start, n)); SVXCHK(S->pool.get(&end, n)); SVXCHK(S->pool.get(&ref, n)); SVXCHK(S->pool.get(&sel, n)); SVXCHK(S->pool.get(&zbad, n + 1));
        SVXCHK(S->pool.get(&ids, nm)); SVXCHK(S->pool.get(&ids_off, n + 1)); SVXCHK(S->pool.get(&err, 2));
        HIPCHK(hipMemsetAsync(err, 0, 8, st));
        k_geno_loci<<<grid, 256, 0, st>>>(t, P.minimum_score, tid, start, end, sel);
        // ---- reads_supporting_variant ----
        DistinctBufs b;
        SVXCHK(S->pool.get(&b.k0, nm)); SVXCHK(S->pool.get(&b.k1, nm)); SVXCHK(S->pool.get(&b.v0, nm)); SVXCHK(S->pool.get(&b.v1, nm)); SVXCHK(S->pool.get(&b.flag, nm + 1)); SVXCHK(S->pool.get(&b.ex, nm + 1));
        const MemberIds m{n, nm, ns, 0, member_off, members, rid, nullptr, err};
        SVXCHK(svx_distinct_member_ids(c, m, 0, b, zbad));
        if (nm > 0) k_geno_compact<<<(unsigned)((nm + 255) / 256), 256, 0, st>>>(nm, b.k1, b.flag, b.ex, ids, err);
        k_geno_offsets<<<(unsigned)((n + 256) / 256), 256, 0, st>>>(n, member_off, b.ex, ids_off);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S->ev[2], st));
        // ---- the walk: DEL and INV rows are one range of the class-grouped table (mode 0), DUP_INT and INS one each (mode 1) ----
        int64_t lo[SVX_NCAND + 1]; lo[0] = 0;
        for (int k = 0; k < SVX_NCAND; k++) lo[k + 1] = lo[k] + class_count[k];
        HIPCHK(hipMemsetAsync(ref, 0, (size_t)n * 4, st));
        const struct { int64_t a, b; int mode; } ranges[3] = {{lo[SVX_CAND_DEL], lo[SVX_CAND_INV + 1], 0}, {lo[SVX_CAND_DUP_INT], lo[SVX_CAND_DUP_INT + 1], 1},
                                                            {lo[SVX_CAND_INS], lo[SVX_CAND_INS + 1], 1}};
        for (const auto& r : ranges)
            if (r.b > r.a)
                k_genotype<<<(unsigned)(r.b - r.a), 64, 0, st>>>(ix, r.mode, r.b - r.a, tid + r.a, start + r.a, end + r.a, ids_off + r.a, ids, P.min_mapq, ref + r.a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S->ev[3], st));
        // ---- the call ----
        k_geno_call<<<grid, 256, 0, st>>>(n, sel, ids_off, ref, P, S->gt.as<uint8_t>(), S->ref_reads.as<int32_t>(), S->alt_reads.as<int32_t>(), S->frac.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S->ev[4], st));
        unsigned long long h = 0;
        SVXCHK(svx_mail_read(c, st, err, 1, &h));
        if (h) return svx_fail(SVX_E_ARG, "svx_genotype_resident: a member index outside the signature table, or a negative read id", __FILE__, __LINE__, hipSuccess);
    } else {
        for (int k = 2; k <= 4; k++) HIPCHK(hipEventRecord(S->ev[k], st));
    }
    HIPCHK(hipEventRecord(S->ev[5], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[5]); S->stats.t_total_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]); S->stats.t_tables_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[1], S->ev[2]); S->stats.t_distinct_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[2], S->ev[3]); S->stats.t_walk_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[3], S->ev[4]); S->stats.t_call_ms = ms;
    S->n = n; S->have = true; S->source = source; S->combine_call = c->combine_calls; S->cluster_call = c->cluster_calls;
    return SVX_OK;
}

extern "C" int svx_genotype_count(svx_ctx* c, int64_t* n_cand) {
    if (!c || !n_cand) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (!geno_current(c, c->genores)) return svx_fail(SVX_E_STATE, "no resident genotypes: run svx_genotype_resident after the last svx_combine / svx_cluster", __FILE__, __LINE__, hipSuccess);
    *n_cand = c->genores->n;
    return SVX_OK;
}

extern "C" int svx_genotype_fetch(svx_ctx* c, uint8_t* gt, int32_t* ref_reads, int32_t* alt_reads, double* support_fraction) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    const GenoState* S = c->genores;
    if (!geno_current(c, S)) return svx_fail(SVX_E_STATE, "no resident genotypes: run svx_genotype_resident after the last svx_combine / svx_cluster", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)S->n;
    if (!n) return SVX_OK;
    HostCopy hc(c->stream);
    if (gt) SVXCHK(hc.d2h(gt, S->gt.p, n));
    if (ref_reads) SVXCHK(hc.d2h(ref_reads, S->ref_reads.p, n * 4));
    if (alt_reads) SVXCHK(hc.d2h(alt_reads, S->alt_reads.p, n * 4));
    if (support_fraction) SVXCHK(hc.d2h(support_fraction, S->frac.p, n * 8));
    return hc.finish();
}

extern "C" int svx_genotype_get_stats(svx_ctx* c, svx_genotype_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->genores) *out = c->genores->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
