// textindex.hip - the tabix index (.tbi, uncompressed bytes) of every file of the BGZF stream the last svx_text_gz left in the context, built where the text
// and the block table lie (svx_text_index*, include/svx.h; gfx950).  What an index says: svim_amd/tabix.py; the line parser: textindex_core.hpp, the source
// svx_text_index_host is built from as well.  This file makes the row table - lines, records, contig runs, names, the status of every file - and the headers;
// the phases behind it (bins, sizes, the linear index, a contig's part) are those a .bai has too: binidx_kernels.hpp, instantiated with TixRows.
// Replaces: tabix / bcftools index after the fact (the reference writes plain text; its users compress and index it).
// Phases, all on the context's stream; counts cross to the host between them:
//   lines      line starts counted per 64-byte piece of the text, scanned, written (one table for the three sources; the files' first bytes start lines too)
//   records    one lane per line: tabs, integers, END=, the virtual offset by a binary search in block_uoff; only the head of a long line is read.
//              Lines that are skipped ('#', empty) are compacted away by a scan
//   contigs    run heads where column 1 differs from the record before (or the file does); chunk heads where the bin does too; the order and range checks
//              raise per-file flags; the run-head names go to the host, which looks for a name with two runs and settles every file's status
//   chunks     (contig << 16 | bin, chunk) sorted stably (svx_sort_pairs_u64), bin heads of the sorted list compacted, first bin of every contig by bisection
//   linear     a record's windows get atomicMin(vbeg): its own lane for one window, the whole wave for a record of many (an inversion over a contig has 32 768)
//   serialise  sizes per contig, a scan, the headers and names written by the host, then one lane per chunk and one wave per contig store every field at its
//              offset; the wave's backward fill of the empty slots is a reverse scan in tiles of 64.
// A file whose status is not 0 gets no bytes; its records still pass through the kernels (their sizes count as 0).  Every store into the index is checked
// against the index's size: a layout that disagrees with its sizes is SVX_E_STATE, not a write somewhere else.
// svx_text_index_fmt with SVX_INDEX_CSI builds the uncompressed .csi of every file instead (svim_amd/csi.py): a depth per file from the running maximum of the
// ends inside every contig run, chunk heads and keys at those depths, a loffset per bin by bisection in place of the linear phase, no SVX_E_RANGE.
#include "common.hpp"
#include "hostcopy.hpp"
#include "textindex_core.hpp"
#include "binidx_kernels.hpp"
#include <algorithm>
#include <string>
#include <unordered_set>

#define XT BINIDX_T
#define XGRID(n) BINIDX_GRID(n)
#define TIX_PIECE 64
#define TIX_NPOOL 64
enum { TIXF_ORDER = 1, TIXF_RANGE = 2 };

struct TixIn {
    const uint8_t* text; long long n_text; int n_files; long long n_blocks; int preset;
    const int64_t *fo, *ffb, *coff, *uoff, *sbase; const uint64_t* eofv;      // per file: text offsets, first block, stream base, where the last line ends
    int* fflag;
};

// is i the first byte of a line?  kk: a cursor into fo that only moves forward (fo[kk] >= every i asked before)
__device__ __forceinline__ bool tix_line_start(const TixIn& in, long long i, int& kk) {
    if (i == 0 || in.text[i - 1] == '\n') return true;
    while (kk < in.n_files && in.fo[kk] < i) kk++;
    return in.fo[kk] == i;
}
__device__ __forceinline__ int tix_first_file_at(const TixIn& in, long long i) {      // first k with fo[k] >= i
    int lo = 0, hi = in.n_files;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (in.fo[mid] >= i) hi = mid; else lo = mid + 1; }
    return lo;
}
__global__ void k_tix_line_count(TixIn in, long long n_pieces, int32_t* cnt) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_pieces) return;
    if (c == n_pieces) { cnt[c] = 0; return; }
    const long long lo = c * TIX_PIECE, hi = lo + TIX_PIECE < in.n_text ? lo + TIX_PIECE : in.n_text;
    int kk = tix_first_file_at(in, lo), n = 0;
    for (long long i = lo; i < hi; i++) n += tix_line_start(in, i, kk) ? 1 : 0;
    cnt[c] = n;
}
__global__ void k_tix_line_write(TixIn in, long long n_pieces, const int64_t* lpos, long long n_lines, int64_t* line) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_pieces) return;
    const long long lo = c * TIX_PIECE, hi = lo + TIX_PIECE < in.n_text ? lo + TIX_PIECE : in.n_text;
    int kk = tix_first_file_at(in, lo);
    long long at = lpos[c];
    for (long long i = lo; i < hi; i++) if (tix_line_start(in, i, kk)) { if (at < n_lines) line[at] = i; at++; }
}
struct TixLines { int64_t *beg, *end; uint64_t* vbeg; int32_t *name_len, *file, *isrec; };
__global__ void k_tix_parse(TixIn in, long long n_lines, const int64_t* line, TixLines o) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_lines) return;
    if (i == n_lines) { o.isrec[i] = 0; return; }
    const long long s = line[i];
    int lo = 0, hi = in.n_files - 1;                     // the file: first k with fo[k + 1] > s
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (in.fo[mid + 1] > s) hi = mid; else lo = mid + 1; }
    const int k = lo;
    long long e = i + 1 < n_lines ? line[i + 1] : in.n_text;
    if (e > in.fo[k + 1]) e = in.fo[k + 1];
    const TixLine L = tix_parse_line(in.text, s, e, in.preset);
    o.beg[i] = L.beg; o.end[i] = L.end; o.name_len[i] = L.name_len; o.file[i] = k; o.isrec[i] = L.skip ? 0 : 1;
    o.vbeg[i] = tix_voff(s, in.coff, in.uoff, in.ffb[k], in.ffb[k + 1], in.coff[in.ffb[k]], in.sbase[k]);
    if (!L.skip && L.end > BINIDX_MAX_END) atomicOr(in.fflag + k, TIXF_RANGE);
}
__global__ void k_tix_compact_records(long long n_lines, const int32_t* isrec, const int64_t* rpos, long long n_rec, uint32_t* r_line) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_lines && isrec[i] && rpos[i] < n_rec) r_line[rpos[i]] = (uint32_t)i;
}
// fdepth: null for the five-level bins of a .tbi, the depth of every file for a .csi
__device__ __forceinline__ uint32_t tix_bin_of(const TixLines& L, long long i, const int32_t* fdepth) {
    return fdepth ? binidx_reg2bin_csi(L.beg[i], L.end[i], fdepth[L.file[i]]) : binidx_bin(BinIdxInterval{L.beg[i], L.end[i]});
}
// contig run heads, chunk heads, the order check
__global__ void k_tix_heads(TixIn in, long long n_rec, const uint32_t* r_line, const int64_t* line, TixLines L, int32_t* chead, int32_t* bhead, const int32_t* fdepth) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rec) return;
    if (j == n_rec) { chead[j] = 0; bhead[j] = 0; return; }
    const long long i = r_line[j];
    bool ch = j == 0;
    long long ip = 0;
    if (!ch) {
        ip = r_line[j - 1];
        ch = L.file[ip] != L.file[i] || L.name_len[ip] != L.name_len[i];
        if (!ch) {
            const uint8_t *a = in.text + line[i], *b = in.text + line[ip];
            for (int k = 0, n = L.name_len[i]; k < n; k++) if (a[k] != b[k]) { ch = true; break; }
        }
        if (!ch && L.beg[i] < L.beg[ip]) atomicOr(in.fflag + L.file[i], TIXF_ORDER);
    }
    chead[j] = ch ? 1 : 0;
    bhead[j] = (ch || tix_bin_of(L, i, fdepth) != tix_bin_of(L, ip, fdepth)) ? 1 : 0;
}
struct TixRuns { uint32_t* run_rec; int32_t *run_file, *run_nlen; uint32_t* chunk_rec; uint64_t* chunk_key; uint32_t* chunk_val; };
__global__ void k_tix_runs(long long n_rec, long long n_runs, long long n_chunks, const uint32_t* r_line, TixLines L, const int32_t* chead, const int32_t* bhead, const int64_t* cpos,
                           const int64_t* bpos, TixRuns o, const int32_t* fdepth, int key_shift) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rec) return;
    if (j == n_rec) { o.run_rec[n_runs] = (uint32_t)n_rec; o.run_nlen[n_runs] = 0; o.run_file[n_runs] = 0; o.chunk_rec[n_chunks] = (uint32_t)n_rec; return; }
    const long long i = r_line[j];
    const long long t = cpos[j] + chead[j] - 1;                 // the run j lies in
    if (chead[j] && t < n_runs) { o.run_rec[t] = (uint32_t)j; o.run_file[t] = L.file[i]; o.run_nlen[t] = L.name_len[i] + 1; }
    const long long q = bpos[j];
    if (bhead[j] && q < n_chunks) { o.chunk_rec[q] = (uint32_t)j; o.chunk_key[q] = ((uint64_t)t << key_shift) | tix_bin_of(L, i, fdepth); o.chunk_val[q] = (uint32_t)q; }
}
// the file of every contig run, before the run table exists (a .csi needs the files' depths before it can tell the chunks apart)
__global__ void k_tix_run_files(long long n_rec, long long n_runs, const uint32_t* r_line, TixLines L, const int32_t* chead, const int64_t* cpos, int32_t* gfile) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_rec && chead[j] && cpos[j] < n_runs) gfile[cpos[j]] = L.file[r_line[j]];
}
__global__ void k_tix_names(long long n_runs, const uint8_t* text, const int64_t* line, const uint32_t* r_line, const uint32_t* run_rec, const int32_t* run_nlen, const int64_t* nm_off,
                            long long n_names, uint8_t* names) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_runs) return;
    const uint8_t* src = text + line[r_line[run_rec[t]]];
    const long long at = nm_off[t]; const int n = run_nlen[t] - 1;
    if (at < 0 || at + n + 1 > n_names) return;
    for (int k = 0; k < n; k++) names[at + k] = src[k];
    names[at + n] = 0;
}
// the row table as binidx_kernels.hpp reads it: row j is record j of the stream, a group is a contig run
struct TixRows {
    const uint32_t* r_line; TixLines L; long long n_lines; const int32_t* chead; const int64_t* cpos; const int32_t* fstat; const uint64_t* eofv;
    const uint32_t* run_rec; const int32_t* run_file; const int64_t *toff, *shift; const int32_t* fdepth;
    __device__ int depth(long long t) const { return fdepth ? fdepth[run_file[t]] : BINIDX_CSI_MIN_DEPTH; }
    __device__ long long group(long long j) const { return cpos[j] + chead[j] - 1; }
    __device__ bool live(long long j) const { return fstat[L.file[r_line[j]]] == 0; }
    __device__ BinIdxInterval interval(long long j) const { const long long i = r_line[j]; return BinIdxInterval{L.beg[i], L.end[i]}; }
    __device__ uint64_t vbeg(long long j) const { return L.vbeg[r_line[j]]; }
    __device__ uint64_t vend(long long j) const {                 // the next line's start, or where the file's last line ends
        const long long i = r_line[j]; const int f = L.file[i];
        return (i + 1 < n_lines && L.file[i + 1] == f) ? L.vbeg[i + 1] : eofv[f];
    }
    __device__ bool group_live(long long t) const { return fstat[run_file[t]] == 0; }
    __device__ long long first(long long t) const { return run_rec[t]; }
    __device__ long long last(long long t) const { return run_rec[t + 1]; }
    __device__ long long part_off(long long t) const { return toff[t] + shift[run_file[t]]; }
    __device__ uint64_t n_mapped(long long t) const { return (uint64_t)run_rec[t + 1] - run_rec[t]; }
    __device__ uint64_t n_unmapped(long long) const { return 0; }
};

struct TextIndexState {
    ScratchPool<TIX_NPOOL> pool{"text index"};
    DevBuf blob;
    std::vector<int64_t> file_off; std::vector<int32_t> status;
    long long gz_gen = -1; bool have = false;
    hipEvent_t ev[8]; bool have_ev = false;
    svx_text_index_stats stats;
};
void svx_textindex_release(svx_ctx* c) {
    TextIndexState* s = c->textindex;
    if (!s) return;
    s->pool.release();
    s->blob.release();
    if (s->have_ev) for (auto& e : s->ev) (void)hipEventDestroy(e);
    delete s;
    c->textindex = nullptr;
}
static bool tix_valid(svx_ctx* c, TextGzView* v) {
    return c && c->textindex && c->textindex->have && svx_textgz_view(c, v) && v->gen == c->textindex->gz_gen;
}

extern "C" int svx_text_index_fmt(svx_ctx* c, int preset, const int64_t* stream_base, int fmt) {
    if (fmt != SVX_INDEX_CLASSIC && fmt != SVX_INDEX_CSI) return svx_fail(SVX_E_ARG, "svx_text_index_fmt: unknown index format (SVX_INDEX_CLASSIC or SVX_INDEX_CSI)", __FILE__, __LINE__, hipSuccess);
    const bool csi = fmt == SVX_INDEX_CSI;
    if (!c || (preset != SVX_INDEX_VCF && preset != SVX_INDEX_BED)) return svx_fail(SVX_E_ARG, "svx_text_index: bad argument (preset SVX_INDEX_VCF or SVX_INDEX_BED)", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    TextGzView V;
    if (!svx_textgz_view(c, &V)) return svx_fail(SVX_E_STATE, "svx_text_index: no BGZF stream: run svx_text_gz first (a later svx_vcf / svx_bed voids the stream of its text)", __FILE__, __LINE__, hipSuccess);
    if (!c->textindex) { c->textindex = new TextIndexState(); }
    TextIndexState* S = c->textindex;
    if (!S->have_ev) { for (auto& e : S->ev) HIPCHK(hipEventCreate(&e)); S->have_ev = true; }
    S->pool.reset(); S->have = false;
    memset(&S->stats, 0, sizeof S->stats);
    hipStream_t st = c->stream;
    const int nf = V.n_files; const long long nb = V.n_blocks, n_text = V.file_off_text[nf];
    for (int k = 0; k < nf; k++) if (stream_base && stream_base[k] < 0) return svx_fail(SVX_E_ARG, "svx_text_index: negative stream_base", __FILE__, __LINE__, hipSuccess);
    if (n_text >= (1ll << 40)) return svx_fail(SVX_E_CAPACITY, "svx_text_index: text too large", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipEventRecord(S->ev[0], st));
    // ---- what the kernels know about the files ----
    std::vector<int64_t> sbase((size_t)nf, 0); std::vector<uint64_t> eofv((size_t)nf, 0);
    for (int k = 0; k < nf; k++) {
        if (stream_base) sbase[k] = stream_base[k];
        eofv[k] = (uint64_t)(sbase[k] + V.h_coff[V.file_first_block[k + 1] - 1] - V.h_coff[V.file_first_block[k]]) << 16;
    }
    TixIn in; memset(&in, 0, sizeof in);
    in.text = V.text; in.n_text = n_text; in.n_files = nf; in.n_blocks = nb; in.preset = preset; in.coff = V.d_coff;
    int32_t* fstat_d; int* err_d;
    {
        int64_t *fo, *ffb, *uoff, *sb; uint64_t* ev;
        SVXCHK(S->pool.get(&fo, (size_t)nf + 1)); SVXCHK(S->pool.get(&ffb, (size_t)nf + 1)); SVXCHK(S->pool.get(&uoff, (size_t)nb + 1)); SVXCHK(S->pool.get(&sb, (size_t)nf)); SVXCHK(S->pool.get(&ev, (size_t)nf));
        SVXCHK(S->pool.get(&in.fflag, (size_t)nf)); SVXCHK(S->pool.get(&fstat_d, (size_t)nf)); SVXCHK(S->pool.get(&err_d, 2));
        HostCopy hc(st);
        SVXCHK(hc.h2d(fo, V.file_off_text, ((size_t)nf + 1) * 8)); SVXCHK(hc.h2d(ffb, V.file_first_block, ((size_t)nf + 1) * 8)); SVXCHK(hc.h2d(uoff, V.h_uoff, ((size_t)nb + 1) * 8));
        SVXCHK(hc.h2d(sb, sbase.data(), (size_t)nf * 8)); SVXCHK(hc.h2d(ev, eofv.data(), (size_t)nf * 8));
        SVXCHK(hc.finish());
        in.fo = fo; in.ffb = ffb; in.uoff = uoff; in.sbase = sb; in.eofv = ev;
        HIPCHK(hipMemsetAsync(in.fflag, 0, (size_t)nf * 4, st)); HIPCHK(hipMemsetAsync(err_d, 0, 8, st));
    }
    // ---- lines ----
    const long long n_pieces = (n_text + TIX_PIECE - 1) / TIX_PIECE;
    int64_t n_lines = 0;
    int64_t* line = nullptr;
    if (n_pieces > 0) {
        int32_t* cnt; int64_t* lpos;
        SVXCHK(S->pool.get(&cnt, (size_t)n_pieces + 1)); SVXCHK(S->pool.get(&lpos, (size_t)n_pieces + 1));
        k_tix_line_count<<<XGRID(n_pieces + 1), XT, 0, st>>>(in, n_pieces, cnt);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, cnt, lpos, n_pieces + 1));
        SVXCHK(svx_d2h(&n_lines, lpos + n_pieces, 8, st));
        if (n_lines < 0 || n_lines > n_text || n_lines >= (1ll << 31)) return svx_fail(SVX_E_CAPACITY, "svx_text_index: too many lines", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&line, (size_t)n_lines + 1));
        if (n_lines) k_tix_line_write<<<XGRID(n_pieces), XT, 0, st>>>(in, n_pieces, lpos, n_lines, line);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(S->ev[1], st));
    // ---- records ----
    TixLines L; memset(&L, 0, sizeof L);
    int64_t n_rec = 0; uint32_t* r_line = nullptr;
    if (n_lines > 0) {
        int64_t* rpos;
        SVXCHK(S->pool.get(&L.beg, (size_t)n_lines)); SVXCHK(S->pool.get(&L.end, (size_t)n_lines)); SVXCHK(S->pool.get(&L.vbeg, (size_t)n_lines)); SVXCHK(S->pool.get(&L.name_len, (size_t)n_lines));
        SVXCHK(S->pool.get(&L.file, (size_t)n_lines)); SVXCHK(S->pool.get(&L.isrec, (size_t)n_lines + 1)); SVXCHK(S->pool.get(&rpos, (size_t)n_lines + 1));
        k_tix_parse<<<XGRID(n_lines + 1), XT, 0, st>>>(in, n_lines, line, L);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, L.isrec, rpos, n_lines + 1));
        SVXCHK(svx_d2h(&n_rec, rpos + n_lines, 8, st));
        if (n_rec < 0 || n_rec > n_lines) return svx_fail(SVX_E_STATE, "svx_text_index: the record count is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&r_line, (size_t)n_rec + 1));
        if (n_rec) k_tix_compact_records<<<XGRID(n_lines), XT, 0, st>>>(n_lines, L.isrec, rpos, n_rec, r_line);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(S->ev[2], st));
    // ---- contig runs and chunks; the status of every file ----
    int64_t n_runs = 0, n_chunks = 0, n_names = 0;
    std::vector<int32_t> fflag((size_t)nf, 0), run_file_h;
    std::vector<int64_t> nm_off_h; std::vector<uint8_t> names_h;
    int32_t *chead = nullptr, *bhead = nullptr; int64_t *cpos = nullptr, *bpos = nullptr, *nm_off = nullptr; uint8_t* names = nullptr;
    TixRuns R; memset(&R, 0, sizeof R);
    std::vector<int32_t> fdepth_h((size_t)nf, BINIDX_CSI_MIN_DEPTH);
    int32_t* fdepth = nullptr; int64_t* rmax = nullptr; int key_shift = BINIDX_KEY_SHIFT;
    TixRows rows; memset(&rows, 0, sizeof rows);
    if (n_rec > 0) {
        SVXCHK(S->pool.get(&chead, (size_t)n_rec + 1)); SVXCHK(S->pool.get(&bhead, (size_t)n_rec + 1)); SVXCHK(S->pool.get(&cpos, (size_t)n_rec + 1)); SVXCHK(S->pool.get(&bpos, (size_t)n_rec + 1));
        k_tix_heads<<<XGRID(n_rec + 1), XT, 0, st>>>(in, n_rec, r_line, line, L, chead, bhead, nullptr);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, chead, cpos, n_rec + 1));
        if (csi) {
            // a .csi: the running maximum of the ends inside every contig run; the largest end of a file gives its depth, and only then can the chunk heads
            // be told (k_tix_heads once more, now with the depths)
            SVXCHK(svx_d2h(&n_runs, cpos + n_rec, 8, st));
            if (n_runs < 1 || n_runs > n_rec) return svx_fail(SVX_E_STATE, "svx_text_index: the run counts are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
            int64_t* gmax; int32_t* gfile; long long* tile_v; int* tile_f;
            const size_t tiles = (size_t)((n_rec + BINIDX_RMAX_TILE - 1) / BINIDX_RMAX_TILE);
            SVXCHK(S->pool.get(&rmax, (size_t)n_rec)); SVXCHK(S->pool.get(&gmax, (size_t)n_runs)); SVXCHK(S->pool.get(&gfile, (size_t)n_runs)); SVXCHK(S->pool.get(&tile_v, tiles)); SVXCHK(S->pool.get(&tile_f, tiles));
            SVXCHK(S->pool.get(&fdepth, (size_t)nf));
            rows.r_line = r_line; rows.L = L; rows.n_lines = n_lines; rows.chead = chead; rows.cpos = cpos;
            SVXCHK(binidx_launch_run_max(st, rows, n_rec, n_runs, rmax, gmax, tile_v, tile_f));
            k_tix_run_files<<<XGRID(n_rec), XT, 0, st>>>(n_rec, n_runs, r_line, L, chead, cpos, gfile);
            HIPCHK(hipGetLastError());
            std::vector<int64_t> gmax_h((size_t)n_runs, 0); std::vector<int32_t> gfile_h((size_t)n_runs, 0);
            {
                HostCopy hc(st);
                SVXCHK(hc.d2h(gmax_h.data(), gmax, (size_t)n_runs * 8)); SVXCHK(hc.d2h(gfile_h.data(), gfile, (size_t)n_runs * 4));
                SVXCHK(hc.finish());
            }
            std::vector<int64_t> fmax((size_t)nf, 0);
            for (int64_t t = 0; t < n_runs; t++) {
                const int f = gfile_h[(size_t)t];
                if (f < 0 || f >= nf) return svx_fail(SVX_E_STATE, "svx_text_index: a run names no file (internal error)", __FILE__, __LINE__, hipSuccess);
                fmax[(size_t)f] = std::max(fmax[(size_t)f], gmax_h[(size_t)t]);
            }
            int dmax = BINIDX_CSI_MIN_DEPTH;
            for (int k = 0; k < nf; k++) { fdepth_h[(size_t)k] = binidx_depth_for(fmax[(size_t)k]); dmax = std::max(dmax, (int)fdepth_h[(size_t)k]); }
            key_shift = binidx_csi_key_shift(dmax);
            SVXCHK(svx_h2d(fdepth, fdepth_h.data(), (size_t)nf * 4, st));
            k_tix_heads<<<XGRID(n_rec + 1), XT, 0, st>>>(in, n_rec, r_line, line, L, chead, bhead, fdepth);
        }
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, bhead, bpos, n_rec + 1));
        {
            HostCopy hc(st);
            SVXCHK(hc.d2h(&n_runs, cpos + n_rec, 8)); SVXCHK(hc.d2h(&n_chunks, bpos + n_rec, 8)); SVXCHK(hc.d2h(fflag.data(), in.fflag, (size_t)nf * 4));
            SVXCHK(hc.finish());
        }
        if (n_runs < 1 || n_runs > n_rec || n_chunks < n_runs || n_chunks > n_rec) return svx_fail(SVX_E_STATE, "svx_text_index: the run counts are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&R.run_rec, (size_t)n_runs + 1)); SVXCHK(S->pool.get(&R.run_file, (size_t)n_runs + 1)); SVXCHK(S->pool.get(&R.run_nlen, (size_t)n_runs + 1));
        SVXCHK(S->pool.get(&R.chunk_rec, (size_t)n_chunks + 1)); SVXCHK(S->pool.get(&R.chunk_key, (size_t)n_chunks)); SVXCHK(S->pool.get(&R.chunk_val, (size_t)n_chunks));
        SVXCHK(S->pool.get(&nm_off, (size_t)n_runs + 1));
        k_tix_runs<<<XGRID(n_rec + 1), XT, 0, st>>>(n_rec, n_runs, n_chunks, r_line, L, chead, bhead, cpos, bpos, R, fdepth, key_shift);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, R.run_nlen, nm_off, n_runs + 1));
        run_file_h.assign((size_t)n_runs + 1, 0); nm_off_h.assign((size_t)n_runs + 1, 0);
        {
            HostCopy hc(st);
            SVXCHK(hc.d2h(nm_off_h.data(), nm_off, ((size_t)n_runs + 1) * 8)); SVXCHK(hc.d2h(run_file_h.data(), R.run_file, ((size_t)n_runs + 1) * 4));
            SVXCHK(hc.finish());
        }
        n_names = nm_off_h[(size_t)n_runs];
        if (n_names < n_runs || n_names > n_text + n_runs) return svx_fail(SVX_E_STATE, "svx_text_index: the name lengths are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&names, (size_t)n_names));
        k_tix_names<<<XGRID(n_runs), XT, 0, st>>>(n_runs, in.text, line, r_line, R.run_rec, R.run_nlen, nm_off, n_names, names);
        HIPCHK(hipGetLastError());
        names_h.assign((size_t)n_names, 0);
        SVXCHK(svx_d2h(names_h.data(), names, (size_t)n_names, st));
    }
    std::vector<int32_t>& status = S->status;
    status.assign((size_t)nf, 0);
    std::vector<int64_t> first_run((size_t)nf + 1, n_runs);       // the runs of file k: [first_run[k], first_run[k + 1])
    {
        std::unordered_set<std::string> seen; int cur = -1;
        for (int64_t t = 0; t < n_runs; t++) {
            const int f = run_file_h[(size_t)t];
            if (f < cur || f >= nf) return svx_fail(SVX_E_STATE, "svx_text_index: the runs are not in file order (internal error)", __FILE__, __LINE__, hipSuccess);
            if (f != cur) { for (int k = cur + 1; k <= f; k++) first_run[(size_t)k] = t; cur = f; seen.clear(); }
            if (!seen.insert(std::string((const char*)names_h.data() + nm_off_h[(size_t)t], (size_t)(nm_off_h[(size_t)t + 1] - nm_off_h[(size_t)t] - 1))).second) fflag[(size_t)f] |= TIXF_ORDER;
        }
        for (int k = 0; k < nf; k++) status[(size_t)k] = (fflag[(size_t)k] & TIXF_ORDER) ? SVX_E_ORDER : (!csi && (fflag[(size_t)k] & TIXF_RANGE)) ? SVX_E_RANGE : 0;
    }
    SVXCHK(svx_h2d(fstat_d, status.data(), (size_t)nf * 4, st));
    HIPCHK(hipEventRecord(S->ev[3], st));
    // ---- chunks sorted by (contig, bin); bins ----
    int64_t n_bins = 0, n_slots = 0;
    rows.fdepth = fdepth;
    rows.r_line = r_line; rows.L = L; rows.n_lines = n_lines; rows.chead = chead; rows.cpos = cpos; rows.fstat = fstat_d; rows.eofv = in.eofv; rows.run_rec = R.run_rec; rows.run_file = R.run_file;
    uint64_t* key2 = nullptr; uint32_t *val2 = nullptr, *bin_first = nullptr, *tid_first_bin = nullptr; int32_t *bh = nullptr, *tmax = nullptr; int64_t *binpos = nullptr, *tsz = nullptr, *nintv = nullptr,
              *toff = nullptr, *loff = nullptr;
    std::vector<int64_t> toff_h((size_t)n_runs + 1, 0);
    uint64_t* bin_loff = nullptr;
    if (n_rec > 0) {
        SVXCHK(S->pool.get(&key2, (size_t)n_chunks)); SVXCHK(S->pool.get(&val2, (size_t)n_chunks)); SVXCHK(S->pool.get(&bh, (size_t)n_chunks + 1)); SVXCHK(S->pool.get(&binpos, (size_t)n_chunks + 1));
        SVXCHK(svx_sort_pairs_u64(c, R.chunk_key, key2, R.chunk_val, val2, n_chunks, 0, binidx_sort_end_bit(n_runs, key_shift)));
        k_binidx_bin_heads<TixRows><<<XGRID(n_chunks + 1), XT, 0, st>>>(n_chunks, key2, bh);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, bh, binpos, n_chunks + 1));
        SVXCHK(svx_d2h(&n_bins, binpos + n_chunks, 8, st));
        if (n_bins < n_runs || n_bins > n_chunks) return svx_fail(SVX_E_STATE, "svx_text_index: the bin count is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        SVXCHK(S->pool.get(&bin_first, (size_t)n_bins + 1)); SVXCHK(S->pool.get(&tid_first_bin, (size_t)n_runs + 1));
        SVXCHK(S->pool.get(&tsz, (size_t)n_runs + 1)); SVXCHK(S->pool.get(&toff, (size_t)n_runs + 2));
        binidx_launch_bins<TixRows>(st, n_chunks, n_bins, n_runs, key2, bh, binpos, bin_first, tid_first_bin, key_shift);
        if (csi) {
            // (a .csi: the loffset of every bin by bisection of the running maximum; no largest end per contig, no slots)
            SVXCHK(S->pool.get(&bin_loff, (size_t)n_bins));
            k_binidx_bin_loff<<<XGRID(n_chunks), XT, 0, st>>>(rows, n_chunks, n_bins, n_rec, key_shift, key2, bh, binpos, rmax, bin_loff, err_d, 1);
            k_binidx_sizes_csi<<<XGRID(n_runs + 1), XT, 0, st>>>(rows, n_runs, tid_first_bin, bin_first, tsz);
            SVXCHK(svx_exclusive_scan_i64(c, tsz, toff, n_runs + 1));
            HIPCHK(hipGetLastError());
            SVXCHK(svx_d2h(toff_h.data(), toff, ((size_t)n_runs + 1) * 8, st));
        } else {
            SVXCHK(S->pool.get(&tmax, (size_t)n_runs + 1)); SVXCHK(S->pool.get(&nintv, (size_t)n_runs + 1)); SVXCHK(S->pool.get(&loff, (size_t)n_runs + 2));
            HIPCHK(hipMemsetAsync(tmax, 0, ((size_t)n_runs + 1) * 4, st));
            k_binidx_max_end<<<XGRID(n_rec), XT, 0, st>>>(rows, n_rec, tmax);
            k_binidx_sizes<<<XGRID(n_runs + 1), XT, 0, st>>>(rows, n_runs, tmax, tid_first_bin, bin_first, tsz, nintv);
            SVXCHK(svx_exclusive_scan_i64(c, tsz, toff, n_runs + 1));
            SVXCHK(svx_exclusive_scan_i64(c, nintv, loff, n_runs + 1));
            HIPCHK(hipGetLastError());
            HostCopy hc(st);
            SVXCHK(hc.d2h(toff_h.data(), toff, ((size_t)n_runs + 1) * 8)); SVXCHK(hc.d2h(&n_slots, loff + n_runs, 8));
            SVXCHK(hc.finish());
        }
        if (n_slots < 0 || n_slots > (int64_t)n_runs * 32768) return svx_fail(SVX_E_STATE, "svx_text_index: the window count is out of range (internal error)", __FILE__, __LINE__, hipSuccess);
    }
    HIPCHK(hipEventRecord(S->ev[4], st));
    // ---- linear index: the smallest vbeg per window ----
    unsigned long long* lin = nullptr;
    if (n_rec > 0 && !csi) {
        SVXCHK(S->pool.get(&lin, (size_t)n_slots));
        if (n_slots) HIPCHK(hipMemsetAsync(lin, 0xff, (size_t)n_slots * 8, st));
        k_binidx_linear<<<XGRID(n_rec), XT, 0, st>>>(rows, n_rec, loff, n_slots, lin);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(S->ev[5], st));
    // ---- layout: header, names, the contigs' parts, trailer per file; then every field at its offset ----
    std::vector<int64_t>& foff = S->file_off;
    foff.assign((size_t)nf + 1, 0);
    std::vector<int64_t> shift((size_t)nf, 0);
    std::vector<std::vector<uint8_t>> heads((size_t)nf);
    int n_ok = 0;
    for (int k = 0; k < nf; k++) {
        foff[(size_t)k + 1] = foff[(size_t)k];
        if (status[(size_t)k] != 0) continue;
        n_ok++;
        const int64_t t0 = first_run[(size_t)k], t1 = first_run[(size_t)k + 1];
        const int64_t l_nm = n_runs ? nm_off_h[(size_t)t1] - nm_off_h[(size_t)t0] : 0, body = n_runs ? toff_h[(size_t)t1] - toff_h[(size_t)t0] : 0;
        std::vector<uint8_t>& h = heads[(size_t)k];
        const int64_t head_bytes = csi ? TIX_CSI_HEADER_BYTES : TIX_HEADER_BYTES;
        h.assign((size_t)(head_bytes + l_nm), 0);
        const uint32_t w[8] = {(uint32_t)(t1 - t0), preset == SVX_INDEX_BED ? 0x10000u : 2u, 1u, 2u, preset == SVX_INDEX_BED ? 3u : 0u, (uint32_t)'#', 0u, (uint32_t)l_nm};
        if (csi) {                                              // magic, min_shift, depth, l_aux; aux: the seven int32 of a .tbi header and the names; n_ref
            memcpy(h.data(), "CSI\1", 4);
            binidx_put32(h.data() + 4, BINIDX_CSI_MIN_SHIFT); binidx_put32(h.data() + 8, (uint32_t)fdepth_h[(size_t)k]); binidx_put32(h.data() + 12, (uint32_t)(28 + l_nm));
            for (int q = 1; q < 8; q++) binidx_put32(h.data() + 12 + 4 * q, w[q]);
            if (l_nm) memcpy(h.data() + 44, names_h.data() + nm_off_h[(size_t)t0], (size_t)l_nm);
            binidx_put32(h.data() + 44 + l_nm, w[0]);
        } else {
            memcpy(h.data(), "TBI\1", 4);
            for (int q = 0; q < 8; q++) binidx_put32(h.data() + 4 + 4 * q, w[q]);
            if (l_nm) memcpy(h.data() + TIX_HEADER_BYTES, names_h.data() + nm_off_h[(size_t)t0], (size_t)l_nm);
        }
        shift[(size_t)k] = foff[(size_t)k] + head_bytes + l_nm - (n_runs ? toff_h[(size_t)t0] : 0);
        foff[(size_t)k + 1] = foff[(size_t)k] + head_bytes + l_nm + body + 8;
    }
    const int64_t n_blob = foff[(size_t)nf];
    SVXCHK(S->blob.reserve((size_t)n_blob + 64));
    uint8_t* blob = S->blob.as<uint8_t>();
    HIPCHK(hipMemsetAsync(blob, 0, (size_t)n_blob + 64, st));
    {
        int64_t* shift_d; SVXCHK(S->pool.get(&shift_d, (size_t)nf));
        HostCopy hc(st);
        SVXCHK(hc.h2d(shift_d, shift.data(), (size_t)nf * 8));
        for (int k = 0; k < nf; k++) if (!heads[(size_t)k].empty()) SVXCHK(hc.h2d(blob + foff[(size_t)k], heads[(size_t)k].data(), heads[(size_t)k].size()));
        SVXCHK(hc.finish());
        if (n_rec > 0) {
            rows.toff = toff; rows.shift = shift_d;
            const BinIdxOut o{blob, n_blob, err_d, 1};
            if (csi) {
                k_binidx_ser_chunks_csi<<<XGRID(n_chunks), XT, 0, st>>>(rows, n_chunks, key_shift, key2, val2, bh, binpos, bin_first, tid_first_bin, R.chunk_rec, bin_loff, o);
                k_binidx_ser_group_csi<<<XGRID(n_runs), XT, 0, st>>>(rows, n_runs, tid_first_bin, bin_first, o);
            } else {
                k_binidx_ser_chunks<<<XGRID(n_chunks), XT, 0, st>>>(rows, n_chunks, key2, val2, bh, binpos, bin_first, tid_first_bin, R.chunk_rec, o);
                k_binidx_ser_group<<<(unsigned)n_runs, 64, 0, st>>>(rows, n_runs, tid_first_bin, bin_first, loff, lin, o);
            }
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(S->ev[6], st));
    int errw[2] = {0, 0};
    SVXCHK(svx_d2h(errw, err_d, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    if (errw[0]) return svx_fail(SVX_E_STATE, "svx_text_index: a field lay outside the index it was sized for (internal error)", __FILE__, __LINE__, hipSuccess);
    float ms = 0;
    double* tp[6] = {&S->stats.t_lines_ms, &S->stats.t_records_ms, &S->stats.t_contigs_ms, &S->stats.t_chunks_ms, &S->stats.t_linear_ms, &S->stats.t_serialise_ms};
    for (int k = 0; k < 6; k++) { (void)hipEventElapsedTime(&ms, S->ev[k], S->ev[k + 1]); *tp[k] = ms; }
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[6]); S->stats.t_total_ms = ms;
    S->stats.n_files = nf; S->stats.n_files_indexed = n_ok; S->stats.n_lines = n_lines; S->stats.n_records = n_rec; S->stats.n_contigs = n_runs; S->stats.n_chunks = n_chunks;
    S->stats.n_bins = n_bins; S->stats.n_slots = n_slots; S->stats.bytes_text = n_text; S->stats.bytes_out = n_blob;
    S->gz_gen = V.gen; S->have = true;
    return SVX_OK;
}

extern "C" int svx_text_index(svx_ctx* c, int preset, const int64_t* stream_base) { return svx_text_index_fmt(c, preset, stream_base, SVX_INDEX_CLASSIC); }

extern "C" int svx_text_index_count(svx_ctx* c, int32_t* n_files, int64_t* n_bytes) {
    TextGzView V;
    if (!tix_valid(c, &V)) return svx_fail(SVX_E_STATE, "no index: run svx_text_index after svx_text_gz (the index is void whenever its stream is)", __FILE__, __LINE__, hipSuccess);
    if (n_files) *n_files = (int32_t)c->textindex->status.size();
    if (n_bytes) *n_bytes = c->textindex->file_off.back();
    return SVX_OK;
}

extern "C" int svx_text_index_fetch(svx_ctx* c, uint8_t* host_dst, int64_t* file_off, int32_t* file_status) {
    TextGzView V;
    if (!tix_valid(c, &V)) return svx_fail(SVX_E_STATE, "no index: run svx_text_index after svx_text_gz (the index is void whenever its stream is)", __FILE__, __LINE__, hipSuccess);
    TextIndexState* S = c->textindex;
    HIPCHK(hipSetDevice(c->device));
    if (file_off) memcpy(file_off, S->file_off.data(), S->file_off.size() * 8);
    if (file_status) memcpy(file_status, S->status.data(), S->status.size() * 4);
    if (host_dst && S->file_off.back() > 0) {
        SVXCHK(svx_d2h(host_dst, S->blob.p, (size_t)S->file_off.back(), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SVX_OK;
}

extern "C" int svx_text_index_get_stats(svx_ctx* c, svx_text_index_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->textindex) *out = c->textindex->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
