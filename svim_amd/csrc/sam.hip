// sam.hip - SAM text -> the BAM record stream of the device reader, in HBM (what `samtools view -b` does between an aligner and `samtools sort`; the reference
// runs that pipeline in src/svim/SVIM_alignment.py:run_alignment).  The bytes are those of sam_core.hpp / svim_amd/sam.py; sam_host.cpp writes the same on the host.
//   k_sam_marks / scan / k_sam_ends   newline marks through the exclusive scan of scan.hpp: where every line ends
//   k_sam_measure                     one wave per line: the first eleven tabs from ballots over 64-byte steps, the operation count as the popcount of the
//                                     non-digit bytes of field 6, l_seq from the tab positions, the aux size from the lane at the end of each tag -> record
//                                     size, descriptor, error (every CIGAR letter and length is judged here: emit refuses only fixed fields and names)
//   scan                              record sizes -> rec_off: the record starts are known, the stream needs no anchor search, no walk, no inflate, no CRC
//   k_sam_emit                        one wave per line: name, CIGAR (a lane per text byte; the operation index is the prefix popcount of the non-digit mask, the
//                                     lane at a letter reads its digits back), SEQ (two text bytes to a nibble pair), QUAL (minus 33), aux (the lane at the end of
//                                     a tag writes it; Z and H values are copied wave-wide), then one lane writes the fixed fields - `bin` needs the CIGAR's
//                                     reference length.  Beyond 65 535 operations: the placeholder, and the operations into CG:B:I behind the last aux field.
//   floats off the fast path          listed by k_sam_emit (stream offset, text range), resolved by strtod on the host, written back by k_sam_patch
// Every kernel is sized by the slice (lines or bytes).  Everything is written with plain byte stores: a record starts at any byte of the stream.
#include "sam.hpp"
#include "sam_host.hpp"
#include "hostcopy.hpp"
#include "scan.hpp"
#include <chrono>
#include <string>
#include <vector>

#define SAM_NO_ERR (~0ull)
static inline double sam_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__global__ void k_sam_marks(const uint8_t* text, long long n, uint8_t* mark) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mark[i] = text[i] == '\n' ? 1 : 0;
}
__global__ void k_sam_ends(const uint8_t* text, long long n, const uint32_t* idx, uint32_t* line_end) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && text[i] == '\n') line_end[idx[i]] = (uint32_t)i;
}

__device__ __forceinline__ void sam_flag_error(unsigned long long* first_err, long long line, int code) {
    atomicMin(first_err, ((unsigned long long)line << 8) | (unsigned long long)code);
}
// the value of lane `src` of the wave (src wave-uniform)
__device__ __forceinline__ uint32_t sam_bcast(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }

// the aux fields of a line, 64 text bytes a step: the lane at the byte that ends a tag (a tab, or the end of the line) owns it.  F(start, length, lane_is_owner)
// is called once per step by every lane, so that F may use wave operations; prev: where the tag that is open at the start of the step began
template <class F> __device__ __forceinline__ void sam_aux_walk(const uint8_t* s, uint32_t aux0, uint32_t len, F&& f) {
    const int lane = lane_id();
    uint32_t prev = aux0;
    for (uint32_t base = aux0; base <= len; base += 64u) {
        const uint32_t p = base + (uint32_t)lane;
        const bool is_end = p <= len && (p == len || s[p] == '\t');
        const unsigned long long m = __ballot(is_end);
        if (!m) continue;
        const unsigned long long m_lt = m & lanemask_lt();
        const uint32_t start = m_lt ? base + (63u - (uint32_t)__clzll((long long)m_lt)) + 1u : prev;
        f(start, is_end ? p - start : 0u, is_end);
        prev = base + (63u - (uint32_t)__clzll((long long)m)) + 1u;
    }
}

__global__ __launch_bounds__(256) void k_sam_measure(const uint8_t* text, const uint32_t* line_end, long long n_lines, SamDesc* desc, uint64_t* size, uint32_t* n_patch,
                                                     unsigned long long* counters) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    const int lane = lane_id();
    const uint32_t lo = i ? line_end[i - 1] + 1u : 0u, len = line_end[i] - lo;
    const uint8_t* s = text + lo;
    SamDesc d;
    for (int k = 0; k < 12; k++) d.f[k] = 0;
    d.len = len; d.n_ops = 0; d.l_seq = 0; d.aux_bytes = 0; d.n_patch = 0; d.err = SAM_OK;
    int err = SAM_OK;
    if (len && s[0] == '@') err = SAM_E_HEADER;
    uint32_t nf = 1;
    for (uint32_t base = 0; base < len && nf < 12u && !err; base += 64u) {
        const uint32_t p = base + (uint32_t)lane;
        unsigned long long m = __ballot(p < len && s[p] == '\t');
        while (m && nf < 12u) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1ull;
#pragma unroll
            for (int q = 1; q < 12; q++) if ((uint32_t)q == nf) d.f[q] = base + (uint32_t)k + 1u;
            nf++;
        }
    }
    if (!err && nf < 11u) err = SAM_E_FIELDS;
    if (!err) {
        if (nf == 11u) d.f[11] = len + 1u;
        sam_check_fields(s, d);
        err = (int)d.err;
    }
    if (!err) {
        const uint32_t c0 = d.f[5], c1 = d.f[6] - 1u;
        if (c1 == c0) err = SAM_E_CIGAR;
        else if (!(c1 - c0 == 1u && s[c0] == '*')) {
            uint32_t cnt = 0; bool bad = false;
            for (uint32_t base = c0; base < c1; base += 64u) {
                const uint32_t p = base + (uint32_t)lane;
                const bool isop = p < c1 && !sam_digit(s[p]);
                uint32_t word;
                if (isop && !sam_cigar_at(s, c0, p, &word)) bad = true;          // letter and length are judged here, so that a line's first fault is the host build's
                cnt += (uint32_t)__popcll(__ballot(isop));
            }
            d.n_ops = cnt;
            if (__ballot(bad) || sam_digit(s[c1 - 1u])) err = SAM_E_CIGAR;
        }
    }
    if (!err) {
        uint32_t bytes_sum = 0, np_sum = 0; int aux_err = SAM_OK;
        sam_aux_walk(s, d.f[11], len, [&](uint32_t start, uint32_t n, bool mine) {
            uint32_t bytes = 0, np = 0; int e = SAM_OK;
            if (mine) e = sam_aux_size(s + start, n, &bytes, &np);
            const unsigned long long bad = __ballot(e != SAM_OK);
            if (bad && !aux_err) aux_err = (int)sam_bcast((uint32_t)e, __ffsll((long long)bad) - 1);
            bytes_sum += (uint32_t)wave_sum_i32((int)bytes);
            np_sum += (uint32_t)wave_sum_i32((int)np);
        });
        d.aux_bytes = bytes_sum; d.n_patch = np_sum;
        err = aux_err;
    }
    d.err = (uint32_t)err;
    if (lane == 0) {
        desc[i] = d;
        size[i] = err ? 0ull : sam_record_bytes(d);
        n_patch[i] = err ? 0u : d.n_patch;
        if (err) sam_flag_error(counters, i, err);
        else if (d.n_ops > SAM_MAX_BAM_OPS) atomicAdd(counters + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void k_sam_emit(const uint8_t* text, const uint32_t* line_end, long long n_lines, const SamDesc* desc, const uint64_t* rec_off, const uint32_t* patch_off,
                                                  ContigTable ct, uint8_t* stream, SamPatch* patch, unsigned long long* counters) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    const int lane = lane_id();
    const SamDesc d = desc[i];
    if (d.err) return;
    const uint32_t lo = i ? line_end[i - 1] + 1u : 0u, len = d.len;
    const uint8_t* s = text + lo;
    const uint64_t rec_at = rec_off[i], rec_bytes = rec_off[i + 1] - rec_at;
    uint8_t* r = stream + rec_at;
    const uint32_t l_name = d.f[1] - 1u - d.f[0];
    for (uint32_t k = (uint32_t)lane; k <= l_name; k += 64u) r[36u + k] = k < l_name ? s[k] : (uint8_t)0;
    uint64_t w = 36ull + l_name + 1ull;
    // CIGAR
    const bool lng = d.n_ops > SAM_MAX_BAM_OPS;
    const uint64_t placeholder = w, cg = rec_bytes - 4ull * d.n_ops - 8ull;          // (cg: only for a long CIGAR)
    long long reflen = 0;
    {
        const uint64_t dst = lng ? cg + 8ull : w;
        const uint32_t c0 = d.f[5], c1 = d.f[6] - 1u;
        uint32_t cnt = 0; bool bad = false;
        if (d.n_ops) for (uint32_t base = c0; base < c1; base += 64u) {
            const uint32_t p = base + (uint32_t)lane;
            const bool isop = p < c1 && !sam_digit(s[p]);
            const unsigned long long m = __ballot(isop);
            if (isop) {
                uint32_t word = 0;
                if (sam_cigar_at(s, c0, p, &word)) {
                    sam_w32(r + dst + 4ull * (cnt + (uint32_t)__popcll(m & lanemask_lt())), word);
                    if (sam_op_on_ref((int)(word & 15u))) reflen += (long long)(word >> 4);
                } else bad = true;
            }
            cnt += (uint32_t)__popcll(m);
        }
        reflen = wave_sum_i64(reflen);
        if (__ballot(bad)) { if (lane == 0) sam_flag_error(counters, i, SAM_E_CIGAR); return; }
        w += lng ? 8ull : 4ull * d.n_ops;
    }
    // SEQ, QUAL
    {
        const uint8_t* sq = s + d.f[9];
        const uint32_t nb = (d.l_seq + 1u) / 2u;
        for (uint32_t j = (uint32_t)lane; j < nb; j += 64u) r[w + j] = (uint8_t)((sam_nib(sq[2u * j]) << 4) | (2u * j + 1u < d.l_seq ? sam_nib(sq[2u * j + 1u]) : 0));
        w += nb;
        const uint8_t* ql = s + d.f[10];
        const bool no_qual = d.f[11] - 1u - d.f[10] == 1u && ql[0] == '*';
        for (uint32_t j = (uint32_t)lane; j < d.l_seq; j += 64u) r[w + j] = no_qual ? (uint8_t)0xff : (uint8_t)(ql[j] - 33u);
        w += d.l_seq;
    }
    // aux
    {
        uint32_t aw = 0, pk = 0;
        SamPatch* const my_patch = patch + patch_off[i];
        sam_aux_walk(s, d.f[11], len, [&](uint32_t start, uint32_t n, bool mine) {
            uint32_t bytes = 0, np = 0;
            if (mine) (void)sam_aux_size(s + start, n, &bytes, &np);
            const uint32_t at = aw + (uint32_t)wave_incl_scan_i32((int)bytes) - bytes, pat = pk + (uint32_t)wave_incl_scan_i32((int)np) - np;
            bool wide = false;
            if (mine) {
                sam_aux_emit(s + start, n, r + w + at, false, rec_at + w + at, (uint64_t)lo + start, (uint32_t)i, my_patch + pat);
                wide = (s[start + 3u] == 'Z' || s[start + 3u] == 'H') && n > 5u;
            }
            unsigned long long zm = __ballot(wide);
            while (zm) {                                           // the values of Z and H: copied by the whole wave (an SA tag can be kilobytes)
                const int src = __ffsll((long long)zm) - 1;
                zm &= zm - 1ull;
                const uint32_t from = sam_bcast(start, src) + 5u, cnt = sam_bcast(n, src) - 5u, to = sam_bcast(at, src) + 3u;
                for (uint32_t k = (uint32_t)lane; k < cnt; k += 64u) r[w + to + k] = s[from + k];
            }
            aw += (uint32_t)wave_sum_i32((int)bytes);
            pk += (uint32_t)wave_sum_i32((int)np);
        });
    }
    if (lane == 0) {
        const int e = sam_fixed(s, d, ct, reflen, r);
        if (e) sam_flag_error(counters, i, e);
        if (lng) sam_long_cigar_frame(d, reflen, r + placeholder, r + cg);
    }
}

__global__ void k_sam_patch(const SamPatch* patch, const uint32_t* value, long long n, uint8_t* stream) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) sam_w32(stream + patch[k].at, value[k]);
}

struct SamDev {
    DevBuf text, mark, idx, line_end, desc, size, n_patch, patch_off, patch, values, counters, scan_tmp;
    unsigned long long* h_cnt = nullptr;       // pinned read-backs: [0] first error, [1] long CIGARs, [2] lines - 1, [3] stream bytes, [4] patches, [5] a line start
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};          // around k_sam_measure and k_sam_emit: the kernels' own time
    int64_t n_lines = 0; uint64_t n_text = 0;
    svx_sam_stats stats;
};

int samdev_create(SamDev** out) {
    SamDev* s = new SamDev();
    memset(&s->stats, 0, sizeof s->stats);
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocDefault) != hipSuccess) { delete s; return svx_fail(SVX_E_HIP, "hipHostMalloc", __FILE__, __LINE__, hipSuccess); }
    memset(p, 0, 64);
    s->h_cnt = (unsigned long long*)p;
    for (auto& e : s->ev) if (hipEventCreate(&e) != hipSuccess) { samdev_destroy(s); return svx_fail(SVX_E_HIP, "hipEventCreate", __FILE__, __LINE__, hipSuccess); }
    *out = s;
    return SVX_OK;
}
void samdev_destroy(SamDev* s) {
    if (!s) return;
    DevBuf* all[] = {&s->text, &s->mark, &s->idx, &s->line_end, &s->desc, &s->size, &s->n_patch, &s->patch_off, &s->patch, &s->values, &s->counters, &s->scan_tmp};
    for (auto* b : all) b->release();
    if (s->h_cnt) (void)hipHostFree(s->h_cnt);
    for (auto e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
}
void samdev_stats(const SamDev* s, svx_sam_stats* out) { if (s) *out = s->stats; else memset(out, 0, sizeof *out); }

#define SAM_GRID(n, t) (unsigned)(((n) + (t) - 1) / (t))

static int sam_refuse(int64_t line, int code) {
    const std::string msg = "SAM line " + std::to_string(line) + ": " + sam_strerror(code);
    return svx_fail(code == SAM_E_RANGE ? SVX_E_RANGE : SVX_E_ARG, msg.c_str(), __FILE__, __LINE__, hipSuccess);
}

int samdev_convert(SamDev* s, const uint8_t* host_text, size_t n, int64_t line_base, const ContigTable& ct, DevBuf& stream, uint64_t* stream_bytes, DevBuf& rec_off, int64_t* n_rec,
                   hipStream_t st) {
    *stream_bytes = 0; *n_rec = 0; s->n_lines = 0; s->n_text = 0;
    if (n == 0) { SVXCHK(stream.reserve(256)); HIPCHK(hipMemsetAsync(stream.p, 0, 256, st)); SVXCHK(rec_off.reserve(8)); HIPCHK(hipMemsetAsync(rec_off.p, 0, 8, st)); return SVX_OK; }
    if (n >= ((size_t)1 << 31)) return svx_fail(SVX_E_CAPACITY, "a slice of SAM text must stay below 2^31 bytes", __FILE__, __LINE__, hipSuccess);
    double t0 = sam_now();
    // ---- the text: through the bounce buffers of hostcopy, a newline behind a last line that lacks one ---------------------------------------------------
    const long long nt = (long long)n + (host_text[n - 1] == '\n' ? 0 : 1);
    SVXCHK(s->text.reserve((size_t)nt + 64));
    SVXCHK(svx_h2d(s->text.p, host_text, n, st));
    if (nt > (long long)n) HIPCHK(hipMemsetAsync(s->text.as<uint8_t>() + n, '\n', 1, st));
    HIPCHK(hipStreamSynchronize(st));
    s->stats.t_stage_ms += (sam_now() - t0) * 1e3; t0 = sam_now();
    // ---- lines ---------------------------------------------------------------------------------------------------------------------------------------------
    SVXCHK(s->mark.reserve((size_t)nt)); SVXCHK(s->idx.reserve((size_t)nt * 4)); SVXCHK(s->counters.reserve(64));
    const uint8_t* text = s->text.as<uint8_t>();
    k_sam_marks<<<SAM_GRID(nt, 256), 256, 0, st>>>(text, nt, s->mark.as<uint8_t>());
    SVXCHK((svx_exclusive_scan<uint8_t, uint32_t>(s->mark.as<uint8_t>(), s->idx.as<uint32_t>(), nt, st, s->scan_tmp)));
    HIPCHK(hipMemcpyAsync(&s->h_cnt[2], s->idx.as<uint32_t>() + (nt - 1), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const long long nl = (long long)(uint32_t)s->h_cnt[2] + 1;          // (the last byte is a newline)
    s->stats.t_lines_ms += (sam_now() - t0) * 1e3; t0 = sam_now();
    SVXCHK(s->line_end.reserve((size_t)nl * 4));
    k_sam_ends<<<SAM_GRID(nt, 256), 256, 0, st>>>(text, nt, s->idx.as<uint32_t>(), s->line_end.as<uint32_t>());
    HIPCHK(hipGetLastError());
    // ---- measure -------------------------------------------------------------------------------------------------------------------------------------------
    const size_t N1 = (size_t)nl + 1;
    SVXCHK(s->desc.reserve((size_t)nl * sizeof(SamDesc))); SVXCHK(s->size.reserve(N1 * 8)); SVXCHK(s->n_patch.reserve(N1 * 4)); SVXCHK(s->patch_off.reserve(N1 * 4));
    SVXCHK(rec_off.reserve(N1 * 8));
    unsigned long long* cnt = s->counters.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(cnt, 0xff, 8, st)); HIPCHK(hipMemsetAsync(cnt + 1, 0, 56, st));
    HIPCHK(hipMemsetAsync(s->size.as<uint64_t>() + nl, 0, 8, st)); HIPCHK(hipMemsetAsync(s->n_patch.as<uint32_t>() + nl, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[0], st));
    k_sam_measure<<<SAM_GRID(nl, 4), 256, 0, st>>>(text, s->line_end.as<uint32_t>(), nl, s->desc.as<SamDesc>(), s->size.as<uint64_t>(), s->n_patch.as<uint32_t>(), cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[1], st));
    SVXCHK((svx_exclusive_scan<uint64_t, uint64_t>(s->size.as<uint64_t>(), rec_off.as<uint64_t>(), (long long)N1, st, s->scan_tmp)));
    SVXCHK((svx_exclusive_scan<uint32_t, uint32_t>(s->n_patch.as<uint32_t>(), s->patch_off.as<uint32_t>(), (long long)N1, st, s->scan_tmp)));
    HIPCHK(hipMemcpyAsync(&s->h_cnt[0], cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&s->h_cnt[3], rec_off.as<uint64_t>() + nl, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&s->h_cnt[4], s->patch_off.as<uint32_t>() + nl, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->stats.t_measure_ms += (sam_now() - t0) * 1e3; t0 = sam_now();
    // a line refused here has size 0 and is passed over by k_sam_emit, which runs all the same: the line to report is the first one that EITHER kernel refuses
    // (the fixed fields and the reference names are judged there), as the host build, which walks the lines in order, reports it
    const uint64_t total = s->h_cnt[3];
    const long long np = (long long)(uint32_t)s->h_cnt[4];
    const long long n_long = (long long)s->h_cnt[1];
    // ---- emit ----------------------------------------------------------------------------------------------------------------------------------------------
    SVXCHK(stream.reserve((size_t)total + 256));
    HIPCHK(hipMemsetAsync(stream.as<uint8_t>() + total, 0, 256, st));
    SVXCHK(s->patch.reserve((size_t)(np + 1) * sizeof(SamPatch)));
    HIPCHK(hipEventRecord(s->ev[2], st));
    k_sam_emit<<<SAM_GRID(nl, 4), 256, 0, st>>>(text, s->line_end.as<uint32_t>(), nl, s->desc.as<SamDesc>(), rec_off.as<uint64_t>(), s->patch_off.as<uint32_t>(), ct, stream.as<uint8_t>(),
                                               s->patch.as<SamPatch>(), cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[3], st));
    HIPCHK(hipMemcpyAsync(&s->h_cnt[0], cnt, 8, hipMemcpyDeviceToHost, st));
    std::vector<SamPatch> hp((size_t)np);
    if (np) SVXCHK(svx_d2h(hp.data(), s->patch.p, (size_t)np * sizeof(SamPatch), st));
    HIPCHK(hipStreamSynchronize(st));
    s->stats.t_emit_ms += (sam_now() - t0) * 1e3; t0 = sam_now();
    { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1])); s->stats.t_measure_kernel_ms += ms; HIPCHK(hipEventElapsedTime(&ms, s->ev[2], s->ev[3])); s->stats.t_emit_kernel_ms += ms; }
    if (s->h_cnt[0] != SAM_NO_ERR) {
        const int64_t bad = (int64_t)(s->h_cnt[0] >> 8);
        // a float that strtod refuses on an earlier line comes first (the list is in line order)
        for (const SamPatch& p : hp) {
            float f;
            if ((int64_t)p.line >= bad) break;
            if (p.text_at + p.text_len > n || !sam_host_strtod(host_text + p.text_at, p.text_len, &f)) return sam_refuse(line_base + (int64_t)p.line + 1, SAM_E_FLOAT);
        }
        return sam_refuse(line_base + bad + 1, (int)(s->h_cnt[0] & 0xffu));
    }
    // ---- the floats left to strtod ---------------------------------------------------------------------------------------------------------------------------
    if (np) {
        std::vector<uint32_t> val((size_t)np);
        for (long long k = 0; k < np; k++) {
            const SamPatch& p = hp[(size_t)k];
            float f;
            if (p.text_at + p.text_len > n || !sam_host_strtod(host_text + p.text_at, p.text_len, &f)) return sam_refuse(line_base + (int64_t)p.line + 1, SAM_E_FLOAT);
            memcpy(&val[(size_t)k], &f, 4);
        }
        SVXCHK(s->values.reserve((size_t)np * 4));
        SVXCHK(svx_h2d(s->values.p, val.data(), (size_t)np * 4, st));
        k_sam_patch<<<SAM_GRID(np, 256), 256, 0, st>>>(s->patch.as<SamPatch>(), s->values.as<uint32_t>(), np, stream.as<uint8_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        s->stats.t_patch_ms += (sam_now() - t0) * 1e3;
    }
    s->n_lines = nl; s->n_text = n;
    s->stats.n_chunks++; s->stats.n_lines += nl; s->stats.n_records += nl; s->stats.text_bytes += (int64_t)n; s->stats.stream_bytes += (int64_t)total;
    s->stats.n_long_cigars += n_long; s->stats.n_patched_floats += np;
    *stream_bytes = total; *n_rec = nl;
    return SVX_OK;
}

int samdev_line_start(SamDev* s, int64_t k, uint64_t* at, hipStream_t st) {
    if (k < 0 || k > s->n_lines) return svx_fail(SVX_E_ARG, "line outside the slice", __FILE__, __LINE__, hipSuccess);
    if (k == 0) { *at = 0; return SVX_OK; }
    if (k == s->n_lines) { *at = s->n_text; return SVX_OK; }
    HIPCHK(hipMemcpyAsync(&s->h_cnt[5], s->line_end.as<uint32_t>() + (k - 1), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *at = (uint64_t)(uint32_t)s->h_cnt[5] + 1;
    return SVX_OK;
}
