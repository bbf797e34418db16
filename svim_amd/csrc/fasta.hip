// fasta.hip - the reference genome loaded on the device: the bytes of a FASTA file (plain, BGZF or one gzip stream) go into HBM whole and are parsed, compacted and
// encoded there into the layout svx_set_genome takes (off[n + 1], one 4-bit code per byte).  Specification: svim_amd/convert.py:genome_arrays - the result is
// byte-for-byte what that function returns; whatever this file does not restate of it (blanks inside lines, symbols outside the alphabet, odd names, odd
// containers) is answered with a return code of its own and Python takes the genome_arrays route.
//
// Replaces: FastaFile(options.genome) + fetch(...).upper() of the reference (src/svim/SVIM_clustering.py:377, :37-43) as a whole-genome load.
//
// Passes over the raw bytes (tiles of FA_TILE bytes, one workgroup of 256 threads per tile, 16 bytes per lane, grid capped and grid-strided):
//   k_fa_lastnl      per tile: position of its last '\n' (or -1)
//   k_fa_maxscan     exclusive prefix maximum of that array (two levels): every tile learns where the line it starts in began, hence whether it starts inside a header
//   k_fa_tiles<0>    classify + count: per tile kept bytes and header starts; per workgroup one atomic each for blanks and dropped bytes
//   svx_exclusive_scan of both per-tile arrays
//   k_fa_tiles<2>    header table (raw offset of the '>', kept-byte rank there) in file order - only tiles that hold a header start read their bytes again
//   k_fa_names       the first FA_NAME bytes behind every '>' gathered into a blob; the host extracts names, applies last-wins and the order of `references`
//   k_fa_tiles<1>    encode + place: kept bytes through the 256-entry table to dest[record] + rank within the record.  A tile without a header start belongs to one
//                    record: its codes are staged in LDS at the alignment of their destination and leave as 16-byte stores; tiles of dropped records are skipped
//                    before their bytes are read
#include "common.hpp"
#include "hostcopy.hpp"
#include "scan.hpp"
#include <zlib.h>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>
#include <sys/mman.h>
#include <atomic>
#include <string>
#include <thread>
#include <unordered_map>
#include <cstdlib>

#define FA_TILE SVX_FASTA_TILE
#define FA_T 256
#define FA_PIECE ((size_t)SVX_FASTA_PIECE)
#define FA_NAME SVX_FASTA_NAME_BYTES
#define FA_GRID 2048                       /* 256 CUs x 8 workgroups: the rest of the tiles by grid stride */
#define FA_MAX_HDR ((long long)1 << 22)    /* more records than this: the name blob alone would be a gigabyte - host route */
static_assert(FA_TILE == FA_T * 16, "one 16-byte load per lane and tile");

// ---- classification of 16 bytes --------------------------------------------------------------------------------------------------------------------------
// 16-bit masks, bit k = byte pos + k: newline, header start ('>' in the first column), '\r', blank (space, \t, \v, \f), inside the file
struct FaCls { uint32_t nl, hs, cr, bl, valid, prev_cr; };

__device__ __forceinline__ uint32_t fa_byte(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

// pos: multiple of 16.  The buffer is allocated to a multiple of 16 bytes, so the load stays inside it whenever pos < n_raw.
__device__ __forceinline__ void fa_load(const uint8_t* __restrict__ raw, long long n_raw, long long pos, uint32_t (&w)[4], FaCls& c) {
    c.nl = c.hs = c.cr = c.bl = c.valid = c.prev_cr = 0u;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (pos >= n_raw) return;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + pos);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    const long long left = n_raw - pos;
    c.valid = left >= 16 ? 0xffffu : ((1u << (int)left) - 1u);
    uint32_t prev = pos > 0 ? (uint32_t)raw[pos - 1] : (uint32_t)'\n';
    c.prev_cr = prev == '\r' ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t ch = fa_byte(w, k);
        c.nl |= (ch == '\n' ? 1u : 0u) << k;
        c.hs |= ((ch == '>' && prev == '\n') ? 1u : 0u) << k;
        c.cr |= (ch == '\r' ? 1u : 0u) << k;
        c.bl |= ((ch == ' ' || ch == '\t' || ch == 0x0bu || ch == 0x0cu) ? 1u : 0u) << k;
        prev = ch;
    }
    c.nl &= c.valid; c.hs &= c.valid; c.cr &= c.valid; c.bl &= c.valid;
}

// "inside a header line" when this thread's bytes begin: the state the nearest earlier thread with an event (header start -> 1, newline -> 0) leaves, found with
// wave ballots; across the waves of the workgroup through sh[FA_T / 64]; before the tile: tile_init.  Every thread of the workgroup must call.
__device__ __forceinline__ int fa_in_state(const FaCls& c, int tile_init, int* sh) {
    const uint32_t ev = c.nl | c.hs;
    const bool has = ev != 0u;
    const bool out = has && ((c.hs >> (31 - __clz((int)ev))) & 1u);
    const uint64_t hb = __ballot(has), ob = __ballot(out);
    const int w = (int)(threadIdx.x >> 6);
    __syncthreads();                                   // (sh may still be read from the tile before)
    if (lane_id() == 0) sh[w] = hb ? (int)(1u | (uint32_t)(((ob >> (63 - __clzll((long long)hb))) & 1ull) << 1)) : 0;
    __syncthreads();
    int st = tile_init;
    for (int k = 0; k < w; k++) { const int s = sh[k]; if (s & 1) st = s >> 1; }
    const uint64_t m = hb & lanemask_lt();
    if (m) st = (int)((ob >> (63 - __clzll((long long)m))) & 1ull);
    return st;
}

// bytes that belong to sequence lines (a newline belongs to the line it ends) and the ones of them that are kept
__device__ __forceinline__ void fa_masks(const FaCls& c, int st, uint32_t& seq, uint32_t& keep) {
    uint32_t hd = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if ((c.hs >> k) & 1u) st = 1;
        hd |= (uint32_t)st << k;
        if ((c.nl >> k) & 1u) st = 0;
    }
    seq = c.valid & ~hd;
    keep = seq & ~(c.nl | c.cr | c.bl);
}

// ---- pass A: last newline of every tile ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FA_T) void k_fa_lastnl(const uint8_t* __restrict__ raw, long long n_raw, long long n_tiles, long long* __restrict__ nlpos) {
    __shared__ int sh[FA_T / 64];
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long long pos = t * FA_TILE + (long long)threadIdx.x * 16;
        uint32_t nl = 0u;
        if (pos < n_raw) {
            const uint4 v = *reinterpret_cast<const uint4*>(raw + pos);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const long long left = n_raw - pos;
#pragma unroll
            for (int k = 0; k < 16; k++) nl |= (fa_byte(w, k) == '\n' ? 1u : 0u) << k;
            nl &= left >= 16 ? 0xffffu : ((1u << (int)left) - 1u);
        }
        int best = nl ? (int)threadIdx.x * 16 + (31 - __clz((int)nl)) : -1;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(best, o, 64); best = x > best ? x : best; }
        __syncthreads();
        if (lane_id() == 0) sh[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            int b = sh[0];
            for (int k = 1; k < FA_T / 64; k++) b = sh[k] > b ? sh[k] : b;
            nlpos[t] = b >= 0 ? t * FA_TILE + b : -1ll;
        }
    }
}

// exclusive prefix maximum in chunks of 1024 (identity -1).  carry == 0: every chunk on its own, its maximum to chunk_max; carry != 0 (one workgroup): the running
// maximum goes from chunk to chunk.  in == out is allowed.
#define FA_MS_T 1024
__global__ __launch_bounds__(FA_MS_T) void k_fa_maxscan(const long long* in, long long* out, long long n, long long* chunk_max, int carry) {
    __shared__ long long sh[FA_MS_T / 64];
    long long run = -1;
    for (long long lo = (long long)blockIdx.x * FA_MS_T; lo < n; lo += (long long)gridDim.x * FA_MS_T) {
        const long long i = lo + threadIdx.x;
        const long long v = i < n ? in[i] : -1ll;
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const long long x = __shfl_up(inc, o, 64); if (lane_id() >= o && x > inc) inc = x; }
        long long ex = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) ex = -1;
        __syncthreads();
        if (lane_id() == 63) sh[threadIdx.x >> 6] = inc;
        __syncthreads();
        long long base = -1, total = -1;
        const int w = (int)(threadIdx.x >> 6);
        for (int k = 0; k < FA_MS_T / 64; k++) { const long long x = sh[k]; if (k < w && x > base) base = x; if (x > total) total = x; }
        long long r = ex > base ? ex : base;
        if (run > r) r = run;
        if (i < n) out[i] = r;
        if (carry) { if (total > run) run = total; }
        else if (threadIdx.x == 0) chunk_max[lo / FA_MS_T] = total;
    }
}

// ---- the tile pass: MODE 0 count, 1 encode + place, 2 header table -----------------------------------------------------------------------------------------------
struct FaArgs {
    const uint8_t* raw; long long n_raw; long long n_tiles;
    const long long* nl_before; const long long* nl_chunk;         // exclusive prefix maximum of the tiles' last newlines: within chunks of 1024 tiles, of the chunks
    int* kcnt; int* hcnt;                                          // [n_tiles + 1] kept bytes / header starts per tile
    const long long* kscan; const long long* hscan;               // their exclusive scans
    unsigned long long* counters;                                  // [0] blanks on sequence lines (net of "\r\n" pairs), [1] bytes not kept, [2] stores refused by the bounds check
    long long* hpos; long long* hrank;                             // [n_hdr] header table
    const long long* dest;                                         // [n_hdr] offset of the record in codes, -1: dropped
    uint8_t* codes; long long n_codes;
    uint32_t* bad;                                                 // [8] bit per byte value outside the alphabet seen in a placed record
};

template <int MODE> __global__ __launch_bounds__(FA_T) void k_fa_tiles(const FaArgs a) {
    __shared__ int sh_state[FA_T / 64];
    __shared__ int sh_scan[FA_T / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint8_t stage[MODE == 1 ? FA_TILE + 32 : 16];
    __shared__ uint8_t tab[256];
    if (MODE == 1) {
        // ASCII (either case) -> 4-bit code, 255 outside "=ACMGRSVTWYHKDBN"
        const uint32_t ch = threadIdx.x, up = (ch >= 'a' && ch <= 'z') ? ch - 32u : ch;
        const char* alpha = "=ACMGRSVTWYHKDBN";
        uint32_t code = 255u;
#pragma unroll
        for (int k = 0; k < 16; k++) if (up == (uint32_t)alpha[k]) code = (uint32_t)k;
        tab[threadIdx.x] = (uint8_t)code;
    }
    long long my_blank = 0, my_drop = 0, my_refused = 0;
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        int hc = 0, kc = 0;
        long long dst0 = 0;                                        // MODE 1, tile of one record: output index of the tile's first kept byte
        if (MODE != 0) { hc = a.hcnt[t]; kc = a.kcnt[t]; }
        if (MODE == 2 && hc == 0) continue;
        if (MODE == 1) {
            if (kc == 0) continue;
            if (hc == 0) {
                const long long h0 = a.hscan[t] - 1;
                if (h0 < 0) continue;                              // text before the first header
                const long long d = a.dest[h0];
                if (d < 0) continue;                               // a record nobody asked for
                dst0 = d - a.hrank[h0] + a.kscan[t];
                if (dst0 < 0 || dst0 + kc > a.n_codes) { my_refused += threadIdx.x == 0 ? 1 : 0; continue; }
            }
        }
        const long long tile0 = t * FA_TILE;
        // the line this tile starts in: a header line?
        int init = 0;
        {
            const long long b0 = a.nl_before[t], b1 = a.nl_chunk[t / FA_MS_T];
            const long long ls = (b0 > b1 ? b0 : b1) + 1;
            if (ls < tile0) init = a.raw[ls] == '>' ? 1 : 0;
        }
        const long long pos = tile0 + (long long)threadIdx.x * 16;
        uint32_t w[4]; FaCls c;
        fa_load(a.raw, a.n_raw, pos, w, c);
        const int st = fa_in_state(c, init, sh_state);
        uint32_t seq, keep;
        fa_masks(c, st, seq, keep);
        const int nk = __popc(keep), nh = __popc(c.hs);
        if (MODE == 0) {
            int blank = __popc(seq & (c.bl | c.cr)) - __popc(seq & c.nl & ((c.cr << 1) | c.prev_cr));
            const long long last = a.n_raw - 1 - pos;              // a '\r' that ends the file is stripped like one before '\n'
            if (last >= 0 && last < 16 && ((seq & c.cr) >> (int)last) & 1u) blank--;
            my_blank += blank;
            my_drop += __popc(c.valid & ~keep);
            int total;
            (void)scan_block_excl<int, FA_T>(nk | (nh << 16), sh_scan, &total);
            if (threadIdx.x == 0) { a.kcnt[t] = total & 0xffff; a.hcnt[t] = total >> 16; }
            continue;
        }
        int total;
        const int ex = scan_block_excl<int, FA_T>(nk | (nh << 16), sh_scan, &total);
        const int k_ex = ex & 0xffff, h_ex = ex >> 16;
        if (MODE == 2) {
            const long long h_base = a.hscan[t] + h_ex, k_base = a.kscan[t] + k_ex;
            uint32_t m = c.hs;
            while (m) {
                const int k = __ffs((int)m) - 1;
                m &= m - 1u;
                const uint32_t below = (1u << k) - 1u;
                const long long h = h_base + __popc(c.hs & below);
                a.hpos[h] = pos + k;
                a.hrank[h] = k_base + __popc(keep & below);
            }
            continue;
        }
        // MODE 1
        if (hc == 0) {
            const int al = (int)(dst0 & 15);
            int q = al + k_ex;
            uint32_t m = keep;
            while (m) {
                const int k = __ffs((int)m) - 1;
                m &= m - 1u;
                const uint32_t ch = fa_byte(w, k);
                const uint32_t code = tab[ch];
                if (code == 255u) atomicOr(&a.bad[ch >> 5], 1u << (ch & 31u));
                stage[q++] = (uint8_t)code;
            }
            __syncthreads();
            const int end = al + kc;
            uint8_t* out = a.codes + (dst0 - al);                  // 16-byte aligned: the codes buffer is, and so is dst0 - al
            for (int lo = (int)threadIdx.x * 16; lo < end; lo += FA_T * 16) {
                if (lo >= al && lo + 16 <= end) *reinterpret_cast<uint4*>(out + lo) = *reinterpret_cast<const uint4*>(stage + lo);
                else { const int j1 = lo + 16 < end ? lo + 16 : end; for (int j = lo > al ? lo : al; j < j1; j++) out[j] = stage[j]; }
            }
            __syncthreads();
        } else {
            // a tile with record boundaries: every kept byte finds its record
            const long long h_base = a.hscan[t] + h_ex - 1, k_base = a.kscan[t] + k_ex;
            uint32_t m = keep;
            while (m) {
                const int k = __ffs((int)m) - 1;
                m &= m - 1u;
                const long long h = h_base + __popc(c.hs & ((2u << k) - 1u));
                if (h < 0) continue;
                const long long d = a.dest[h];
                if (d < 0) continue;
                const long long o = d + (k_base + __popc(keep & ((1u << k) - 1u)) - a.hrank[h]);
                if (o < 0 || o >= a.n_codes) { my_refused++; continue; }
                const uint32_t ch = fa_byte(w, k);
                const uint32_t code = tab[ch];
                if (code == 255u) atomicOr(&a.bad[ch >> 5], 1u << (ch & 31u));
                a.codes[o] = (uint8_t)code;
            }
        }
    }
    if (MODE == 0) {
        // one atomic per workgroup and counter
        __shared__ long long red[2][FA_T / 64];
        const long long b = wave_sum_i64(my_blank), d = wave_sum_i64(my_drop);
        __syncthreads();
        if (lane_id() == 0) { red[0][threadIdx.x >> 6] = b; red[1][threadIdx.x >> 6] = d; }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long sb = 0, sd = 0;
            for (int k = 0; k < FA_T / 64; k++) { sb += red[0][k]; sd += red[1][k]; }
            if (sb) atomicAdd(&a.counters[0], (unsigned long long)sb);
            if (sd) atomicAdd(&a.counters[1], (unsigned long long)sd);
        }
    }
    if (MODE == 1 && my_refused) atomicAdd(&a.counters[2], (unsigned long long)my_refused);
}

// the first FA_NAME bytes behind every '>' (zero behind the end of the file): one wavefront per header
__global__ __launch_bounds__(64) void k_fa_names(const uint8_t* __restrict__ raw, long long n_raw, const long long* __restrict__ hpos, long long n_hdr, uint8_t* __restrict__ blob) {
    const long long h = blockIdx.x;
    if (h >= n_hdr) return;
    const long long p = hpos[h] + 1;
    for (int j = lane_id(); j < FA_NAME; j += 64) blob[h * FA_NAME + j] = p + j < n_raw ? raw[p + j] : (uint8_t)0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
double fa_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int fa_host(svx_fasta_stats* s, int reason, const char* what) {
    if (s) s->host_reason = reason;
    return svx_fail(SVX_E_FASTA_HOST, what, __FILE__, __LINE__, hipSuccess);
}

struct FaFile {
    int fd = -1; size_t size = 0; const uint8_t* map = nullptr;
    ~FaFile() { if (map) munmap((void*)map, size); if (fd >= 0) close(fd); }
    bool open_(const char* path) {
        fd = open(path, O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
        size = (size_t)sb.st_size;
        return true;
    }
    bool map_() {
        if (map || !size) return true;
        void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) return false;
        map = (const uint8_t*)p;
        return true;
    }
};

struct FaBlock { uint64_t payload; uint32_t clen, isize; };

// a BGZF member at `at`: gzip header with exactly the FEXTRA flag and a 'B' 'C' subfield of two bytes (the block size - 1)
bool fa_bgzf_block(const uint8_t* f, size_t size, size_t at, FaBlock* b, size_t* next) {
    if (at + 18 > size) return false;
    const uint8_t* p = f + at;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return false;
    const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
    if (at + 12 + xlen + 8 > size) return false;
    size_t bsize = 0;
    for (size_t x = 0; x + 4 <= xlen;) {
        const uint8_t* e = p + 12 + x;
        const size_t slen = (size_t)e[2] | ((size_t)e[3] << 8);
        if (e[0] == 'B' && e[1] == 'C' && slen == 2 && x + 6 <= xlen) { bsize = ((size_t)e[4] | ((size_t)e[5] << 8)) + 1; break; }
        x += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || at + bsize > size) return false;
    b->payload = at + 12 + xlen;
    b->clen = (uint32_t)(bsize - 12 - xlen - 8);
    const uint8_t* tr = p + bsize - 4;
    b->isize = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
    if (b->isize > 65536u) return false;
    *next = at + bsize;
    return true;
}

// container of the file: plain text, BGZF (every member a BGZF block: `blocks` filled, *raw = the sum of their sizes) or some other gzip file (*raw unknown: -1)
int fa_probe(FaFile& f, std::vector<FaBlock>* blocks, long long* raw) {
    uint8_t magic[2] = {0, 0};
    if (f.size < 2 || pread(f.fd, magic, 2, 0) != 2 || magic[0] != 0x1f || magic[1] != 0x8b) { *raw = (long long)f.size; return SVX_FASTA_PLAIN; }
    *raw = -1;
    if (!f.map_()) return SVX_FASTA_GZIP;
    std::vector<FaBlock> bl;
    long long total = 0;
    size_t at = 0;
    while (at < f.size) {
        FaBlock b; size_t next = 0;
        if (!fa_bgzf_block(f.map, f.size, at, &b, &next)) return SVX_FASTA_GZIP;
        bl.push_back(b); total += b.isize; at = next;
    }
    *raw = total;
    if (blocks) blocks->swap(bl);
    return SVX_FASTA_BGZF;
}

// page-locked staging of the library (svx_host_alloc: mapped once, reused by later loads), two buffers and an event each per reader
struct FaStage {
    void* p[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false};
    ~FaStage() { for (int k = 0; k < 2; k++) { if (ev[k]) { if (used[k]) (void)hipEventSynchronize(ev[k]); (void)hipEventDestroy(ev[k]); } if (p[k]) svx_host_free(p[k]); } }
    bool init() {
        for (int k = 0; k < 2; k++) {
            p[k] = svx_host_alloc(FA_PIECE);
            if (!p[k] || hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        }
        return true;
    }
    // the buffer is free again when the copy that read it last is over
    bool acquire(int k) { if (used[k] && hipEventSynchronize(ev[k]) != hipSuccess) { (void)hipGetLastError(); return false; } used[k] = false; return true; }
    bool send(int k, void* dev_dst, size_t n, hipStream_t st) {
        if (hipMemcpyAsync(dev_dst, p[k], n, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(ev[k], st) != hipSuccess) { (void)hipGetLastError(); return false; }
        used[k] = true;
        return true;
    }
};

// plain text: pieces of FA_PIECE read straight into page-locked staging (pread) and sent on; a few readers take the pieces in turn
int fa_stage_plain(svx_ctx* c, FaFile& f, uint8_t* raw_dev) {
    const size_t pieces = (f.size + FA_PIECE - 1) / FA_PIECE;
    static const int max_t = []() { const char* e = getenv("SVX_UPLOAD_THREADS"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
    const int T = pieces < (size_t)max_t ? (int)(pieces ? pieces : 1) : max_t;
    std::vector<int> rc((size_t)T, 0);
    std::vector<std::thread> th;
    const int dev = c->device; hipStream_t st = c->stream; const int fd = f.fd; const size_t size = f.size;
    for (int t = 0; t < T; t++) th.emplace_back([=, &rc]() {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); rc[(size_t)t] = 1; return; }
        FaStage sg;
        if (!sg.init()) { rc[(size_t)t] = 1; return; }
        int b = 0;
        for (size_t k = (size_t)t; k < pieces; k += (size_t)T, b ^= 1) {
            const size_t off = k * FA_PIECE, n = size - off < FA_PIECE ? size - off : FA_PIECE;
            if (!sg.acquire(b)) { rc[(size_t)t] = 1; return; }
            size_t got = 0;
            while (got < n) { const ssize_t r = pread(fd, (char*)sg.p[b] + got, n - got, (off_t)(off + got)); if (r <= 0) { rc[(size_t)t] = 2; return; } got += (size_t)r; }
            if (!sg.send(b, raw_dev + off, n, st)) { rc[(size_t)t] = 1; return; }
        }
    });
    for (auto& x : th) x.join();
    for (int t = 0; t < T; t++) {
        if (rc[(size_t)t] == 2) return svx_fail(SVX_E_ARG, "FASTA file could not be read", __FILE__, __LINE__, hipSuccess);
        if (rc[(size_t)t]) return svx_fail(SVX_E_HIP, "staging of the FASTA file failed", __FILE__, __LINE__, hipSuccess);
    }
    HIPCHK(hipStreamSynchronize(st));
    return SVX_OK;
}

// BGZF: the file slices of sub-batches of blocks into the inflater's page-locked staging, inflated by the device (one wavefront per block) straight into the raw buffer
int fa_stage_bgzf(svx_ctx* c, FaFile& f, const std::vector<FaBlock>& blocks, uint8_t* raw_dev, long long n_raw, double* t_inflate) {
    svx_inflater* inf = nullptr;
    SVXCHK(svx_inflater_create(c->device, &inf));
    struct Guard { svx_inflater* f; ~Guard() { svx_inflater_destroy(f); } } guard{inf};
    const int NS = 3;
    bool used[NS] = {false, false, false};
    int rc = SVX_OK, sl = 0;
    std::vector<uint64_t> in_off, o_at; std::vector<uint32_t> clen, isz;
    uint64_t out_at = 0;
    double ms_sum = 0;
    for (size_t a = 0; a < blocks.size() && rc == SVX_OK;) {
        size_t b = a;
        uint64_t out_bytes = 0;
        const uint64_t f0 = blocks[a].payload;
        while (b < blocks.size() && b - a < 8192 && (b == a || blocks[b].payload + blocks[b].clen - f0 <= FA_PIECE)) { out_bytes += blocks[b].isize; b++; }
        const uint64_t staged = blocks[b - 1].payload + blocks[b - 1].clen - f0;
        if (used[sl]) { float ms = 0; rc = svx_inflater_wait(inf, sl, &ms); ms_sum += ms; used[sl] = false; if (rc != SVX_OK) break; }
        in_off.clear(); o_at.clear(); clen.clear(); isz.clear();
        uint64_t o = 0;
        for (size_t k = a; k < b; k++) {
            if (blocks[k].isize) { in_off.push_back(blocks[k].payload - f0); clen.push_back(blocks[k].clen); isz.push_back(blocks[k].isize); o_at.push_back(o); }
            o += blocks[k].isize;
        }
        if (!in_off.empty()) {
            uint8_t* stage = (uint8_t*)svx_inflater_staging(inf, sl, staged + 8);
            if (!stage) { rc = svx_fail(SVX_E_HIP, "no page-locked staging memory", __FILE__, __LINE__, hipSuccess); break; }
            memcpy(stage, f.map + f0, (size_t)staged);
            if (out_at + out_bytes > (uint64_t)n_raw) { rc = svx_fail(SVX_E_CAPACITY, "BGZF blocks beyond the raw buffer", __FILE__, __LINE__, hipSuccess); break; }
            rc = svx_inflater_enqueue(inf, sl, (int64_t)in_off.size(), in_off.data(), clen.data(), isz.data(), o_at.data(), staged, raw_dev + out_at, out_bytes, 1);
            if (rc != SVX_OK) break;
            used[sl] = true;
            sl = (sl + 1) % NS;
        }
        out_at += out_bytes;
        a = b;
    }
    for (int k = 0; k < NS; k++) if (used[k]) { float ms = 0; const int r = svx_inflater_wait(inf, k, &ms); ms_sum += ms; if (rc == SVX_OK) rc = r; }
    *t_inflate = ms_sum * 1e-3;
    return rc;
}

// any other gzip file: zlib on the host, member after member, piece by piece into the staging buffers.  The inflated size is not known in advance: the raw buffer
// grows (contents kept).  *host_route: the stream is not what zlib / Python's gzip take without complaint - Python shall say so.
int fa_stage_gzip(svx_ctx* c, FaFile& f, DevBuf& raw, long long* n_raw, size_t budget, double* t_inflate, int* host_route) {
    FaStage sg;
    if (!sg.init()) return svx_fail(SVX_E_HIP, "no page-locked staging memory", __FILE__, __LINE__, hipSuccess);
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return svx_fail(SVX_E_HIP, "inflateInit2", __FILE__, __LINE__, hipSuccess);
    struct ZGuard { z_stream* z; ~ZGuard() { inflateEnd(z); } } zg{&zs};
    std::vector<uint8_t> in((size_t)1 << 20);
    size_t file_at = 0, done = 0;
    int b = 0;
    bool in_member = true, eof = false;
    *host_route = 0;
    if (!sg.acquire(b)) return svx_fail(SVX_E_HIP, "staging event", __FILE__, __LINE__, hipSuccess);
    zs.next_out = (Bytef*)sg.p[b]; zs.avail_out = (uInt)FA_PIECE;
    auto flush = [&]() -> int {
        const size_t n = FA_PIECE - zs.avail_out;
        if (n) {
            if (done + n > budget) { *host_route = 2; return SVX_OK; }
            if (raw.cap < done + n + 16) {
                HIPCHK(hipStreamSynchronize(c->stream));
                SVXCHK(raw.reserve((done + n) * 3 / 2 + (4u << 20), true, c->stream));
            }
            if (!sg.send(b, raw.as<uint8_t>() + done, n, c->stream)) return svx_fail(SVX_E_HIP, "host -> device copy of inflated FASTA bytes", __FILE__, __LINE__, hipSuccess);
            done += n;
            b ^= 1;
            if (!sg.acquire(b)) return svx_fail(SVX_E_HIP, "staging event", __FILE__, __LINE__, hipSuccess);
        }
        zs.next_out = (Bytef*)sg.p[b]; zs.avail_out = (uInt)FA_PIECE;
        return SVX_OK;
    };
    while (!*host_route) {
        if (zs.avail_in == 0 && !eof) {
            const ssize_t r = pread(f.fd, in.data(), in.size(), (off_t)file_at);
            if (r < 0) return svx_fail(SVX_E_ARG, "FASTA file could not be read", __FILE__, __LINE__, hipSuccess);
            if (r == 0) eof = true;
            file_at += (size_t)r; zs.next_in = in.data(); zs.avail_in = (uInt)r;
        }
        if (!in_member) {
            // between members: zero padding is skipped (as Python's gzip does); anything else must be another member
            while (zs.avail_in && *zs.next_in == 0) { zs.next_in++; zs.avail_in--; }
            if (zs.avail_in == 0) { if (eof) break; continue; }
            if (inflateReset(&zs) != Z_OK) { *host_route = 4; break; }
            in_member = true;
        }
        if (zs.avail_in == 0 && eof) { *host_route = 4; break; }                 // the stream ends inside a member
        const double t0 = fa_now();
        const int r = inflate(&zs, Z_NO_FLUSH);
        *t_inflate += fa_now() - t0;
        if (r != Z_OK && r != Z_STREAM_END && r != Z_BUF_ERROR) { *host_route = 4; break; }
        if (zs.avail_out == 0) SVXCHK(flush());
        if (r == Z_STREAM_END) in_member = false;
    }
    if (!*host_route) SVXCHK(flush());
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_raw = (long long)done;
    return SVX_OK;
}

bool fa_space(uint8_t ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == 0x0b || ch == 0x0c; }
}  // namespace

// ---- pure host helpers, exported for the tests ---------------------------------------------------------------------------------------------------------------------
extern "C" int svx_fasta_probe(const char* path, int32_t* kind, int64_t* raw_bytes, int64_t* n_blocks) {
    if (!path) return svx_fail(SVX_E_ARG, "null path", __FILE__, __LINE__, hipSuccess);
    FaFile f;
    if (!f.open_(path)) return svx_fail(SVX_E_ARG, "FASTA file cannot be opened", __FILE__, __LINE__, hipSuccess);
    std::vector<FaBlock> blocks; long long raw = 0;
    const int k = fa_probe(f, &blocks, &raw);
    if (kind) *kind = k;
    if (raw_bytes) *raw_bytes = raw;
    if (n_blocks) *n_blocks = k == SVX_FASTA_BGZF ? (int64_t)blocks.size() : 0;
    return SVX_OK;
}

// names out of the header blob, last record of a name wins, order of `names`: dest[h] = offset of record h in codes or -1, off_out[n_contig + 1]
extern "C" int svx_fasta_plan(int64_t n_hdr, const uint8_t* name_blob, const int64_t* hdr_pos, const int64_t* hdr_rank, int64_t raw_bytes, int32_t n_contig,
                              const char* names_nul_separated, int64_t* dest, int64_t* off_out, int64_t* records_kept) {
    if (n_hdr < 0 || n_contig < 0 || !off_out || (n_hdr && (!name_blob || !hdr_pos || !hdr_rank || !dest)) || (n_contig && !names_nul_separated))
        return svx_fail(SVX_E_ARG, "bad argument", __FILE__, __LINE__, hipSuccess);
    std::unordered_map<std::string, int64_t> last;
    last.reserve((size_t)n_hdr * 2 + 16);
    for (int64_t h = 0; h < n_hdr; h++) {
        const uint8_t* p = name_blob + h * FA_NAME;
        const int64_t behind = raw_bytes - (hdr_pos[h] + 1);
        const int avail = behind < FA_NAME ? (int)behind : FA_NAME;
        int len = 0;
        while (len < avail && !fa_space(p[len])) { if (p[len] >= 0x80u) return svx_fail(SVX_E_FASTA_HOST, "record name outside ASCII", __FILE__, __LINE__, hipSuccess); len++; }
        if (len == 0) return svx_fail(SVX_E_FASTA_HOST, "record without a name", __FILE__, __LINE__, hipSuccess);
        if (len == avail && avail == FA_NAME) return svx_fail(SVX_E_FASTA_HOST, "record name longer than the header blob holds", __FILE__, __LINE__, hipSuccess);
        last[std::string((const char*)p, (size_t)len)] = h;
        dest[h] = -1;
    }
    const char* nm = names_nul_separated;
    int64_t kept = 0;
    off_out[0] = 0;
    for (int32_t j = 0; j < n_contig; j++) {
        const std::string name(nm);
        nm += name.size() + 1;
        int64_t len = 0;
        auto it = last.find(name);
        if (it != last.end()) {
            const int64_t h = it->second;
            if (dest[h] >= 0) return svx_fail(SVX_E_FASTA_HOST, "one name twice among the requested contigs", __FILE__, __LINE__, hipSuccess);
            dest[h] = off_out[j];
            len = hdr_rank[h + 1] - hdr_rank[h];
            kept++;
        }
        off_out[j + 1] = off_out[j] + len;
    }
    if (records_kept) *records_kept = kept;
    return SVX_OK;
}

// ---- the loader ----------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct FaBufs {
    DevBuf raw, nlpos, nlchunk, kcnt, hcnt, kscan, hscan, counters, hpos, hrank, blob, dest, codes, goff, scan_tmp;
    ~FaBufs() { DevBuf* all[] = {&raw, &nlpos, &nlchunk, &kcnt, &hcnt, &kscan, &hscan, &counters, &hpos, &hrank, &blob, &dest, &codes, &goff, &scan_tmp}; for (auto* b : all) b->release(); }
};
}

extern "C" int svx_genome_load_fasta(svx_ctx* c, const char* path, int32_t n_contig, const char* names_nul_separated, int64_t* off_out, svx_fasta_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c || !path || n_contig < 0 || !off_out || (n_contig && !names_nul_separated)) return svx_fail(SVX_E_ARG, "bad argument", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    const double t_begin = fa_now();
    FaFile f;
    if (!f.open_(path)) return svx_fail(SVX_E_ARG, "FASTA file cannot be opened", __FILE__, __LINE__, hipSuccess);
    std::vector<FaBlock> blocks;
    long long n_raw = 0;
    const int kind = fa_probe(f, &blocks, &n_raw);
    if (stats) { stats->kind = kind; stats->blocks = (int64_t)blocks.size(); }
    // raw bytes + codes must fit a quarter of the free device memory (codes <= raw); beyond that: the host route rather than a chunked variant
    size_t mem_free = 0, mem_total = 0;
    HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
    size_t budget = mem_free / 4;
    { const char* e = getenv("SVX_FASTA_BUDGET_MB"); if (e && atoll(e) > 0) budget = (size_t)atoll(e) << 20; }
    if (n_raw >= 0 && (size_t)n_raw * 2 > budget) return fa_host(stats, 2, "FASTA file beyond the device-memory budget of the loader");
    FaBufs B;
    hipStream_t st = c->stream;
    double t_inflate = 0;
    // ---- the raw bytes into HBM
    if (kind == SVX_FASTA_PLAIN) {
        SVXCHK(B.raw.reserve(((size_t)n_raw + 15) / 16 * 16 + 16));
        SVXCHK(fa_stage_plain(c, f, B.raw.as<uint8_t>()));
    } else if (kind == SVX_FASTA_BGZF) {
        if (!f.map_()) return svx_fail(SVX_E_ARG, "FASTA file cannot be mapped", __FILE__, __LINE__, hipSuccess);
        SVXCHK(B.raw.reserve(((size_t)n_raw + 15) / 16 * 16 + 16));
        SVXCHK(fa_stage_bgzf(c, f, blocks, B.raw.as<uint8_t>(), n_raw, &t_inflate));
    } else {
        int host_route = 0;
        SVXCHK(B.raw.reserve((size_t)f.size * 4 + (4u << 20) < budget / 2 ? (size_t)f.size * 4 + (4u << 20) : budget / 2 + 16));
        SVXCHK(fa_stage_gzip(c, f, B.raw, &n_raw, budget / 2, &t_inflate, &host_route));
        if (host_route) return fa_host(stats, host_route, host_route == 2 ? "FASTA file beyond the device-memory budget of the loader" : "gzip stream zlib does not take as it is");
        SVXCHK(B.raw.reserve(((size_t)n_raw + 15) / 16 * 16 + 16, true, st));
    }
    const double t_staged = fa_now();
    if (stats) { stats->raw_bytes = n_raw; stats->t_inflate_s = t_inflate; stats->t_read_stage_s = t_staged - t_begin - (kind == SVX_FASTA_GZIP ? t_inflate : 0); }
    // ---- classify and count
    const long long n_tiles = (n_raw + FA_TILE - 1) / FA_TILE;
    const long long n_chunks = (n_tiles + FA_MS_T - 1) / FA_MS_T;
    long long n_hdr = 0, n_seq = 0;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    FaArgs a; memset(&a, 0, sizeof a);
    a.raw = B.raw.as<uint8_t>(); a.n_raw = n_raw; a.n_tiles = n_tiles;
    const unsigned grid = (unsigned)(n_tiles < FA_GRID ? n_tiles : FA_GRID);
    SVXCHK(B.counters.reserve(64 + 32));
    HIPCHK(hipMemsetAsync(B.counters.p, 0, 64 + 32, st));
    a.counters = B.counters.as<unsigned long long>(); a.bad = reinterpret_cast<uint32_t*>(B.counters.as<uint8_t>() + 64);
    if (n_tiles > 0) {
        SVXCHK(B.nlpos.reserve((size_t)n_tiles * 8)); SVXCHK(B.nlchunk.reserve((size_t)n_chunks * 8));
        SVXCHK(B.kcnt.reserve((size_t)(n_tiles + 1) * 4)); SVXCHK(B.hcnt.reserve((size_t)(n_tiles + 1) * 4));
        SVXCHK(B.kscan.reserve((size_t)(n_tiles + 1) * 8)); SVXCHK(B.hscan.reserve((size_t)(n_tiles + 1) * 8));
        k_fa_lastnl<<<grid, FA_T, 0, st>>>(a.raw, n_raw, n_tiles, B.nlpos.as<long long>());
        k_fa_maxscan<<<(unsigned)n_chunks, FA_MS_T, 0, st>>>(B.nlpos.as<long long>(), B.nlpos.as<long long>(), n_tiles, B.nlchunk.as<long long>(), 0);
        k_fa_maxscan<<<1, FA_MS_T, 0, st>>>(B.nlchunk.as<long long>(), B.nlchunk.as<long long>(), n_chunks, nullptr, 1);
        HIPCHK(hipGetLastError());
        a.nl_before = B.nlpos.as<long long>(); a.nl_chunk = B.nlchunk.as<long long>();
        a.kcnt = B.kcnt.as<int>(); a.hcnt = B.hcnt.as<int>();
        HIPCHK(hipMemsetAsync(a.kcnt + n_tiles, 0, 4, st)); HIPCHK(hipMemsetAsync(a.hcnt + n_tiles, 0, 4, st));
        k_fa_tiles<0><<<grid, FA_T, 0, st>>>(a);
        HIPCHK(hipGetLastError());
        SVXCHK((svx_exclusive_scan<int, long long>(a.kcnt, B.kscan.as<long long>(), n_tiles + 1, st, B.scan_tmp)));
        SVXCHK((svx_exclusive_scan<int, long long>(a.hcnt, B.hscan.as<long long>(), n_tiles + 1, st, B.scan_tmp)));
        a.kscan = B.kscan.as<long long>(); a.hscan = B.hscan.as<long long>();
        HostCopy hc(st);
        SVXCHK(hc.d2h(&n_seq, B.kscan.as<long long>() + n_tiles, 8));
        SVXCHK(hc.d2h(&n_hdr, B.hscan.as<long long>() + n_tiles, 8));
        SVXCHK(hc.d2h(cnt, B.counters.p, 16));
        SVXCHK(hc.finish());
    }
    if (stats) { stats->seq_bytes = n_seq; stats->dropped_bytes = (int64_t)cnt[1]; stats->records_in_file = n_hdr; stats->blank_bytes = (int64_t)cnt[0]; }
    if (cnt[0] != 0) return fa_host(stats, 1, "blanks on sequence lines");
    if (n_hdr > FA_MAX_HDR) return fa_host(stats, 3, "more records than the loader takes");
    // ---- headers
    std::vector<int64_t> hpos((size_t)n_hdr), hrank((size_t)n_hdr + 1), dest((size_t)n_hdr);
    std::vector<uint8_t> blob((size_t)n_hdr * FA_NAME);
    if (n_hdr > 0) {
        SVXCHK(B.hpos.reserve((size_t)n_hdr * 8)); SVXCHK(B.hrank.reserve((size_t)(n_hdr + 1) * 8)); SVXCHK(B.blob.reserve((size_t)n_hdr * FA_NAME)); SVXCHK(B.dest.reserve((size_t)n_hdr * 8));
        a.hpos = B.hpos.as<long long>(); a.hrank = B.hrank.as<long long>();
        k_fa_tiles<2><<<grid, FA_T, 0, st>>>(a);
        k_fa_names<<<(unsigned)n_hdr, 64, 0, st>>>(a.raw, n_raw, a.hpos, n_hdr, B.blob.as<uint8_t>());
        HIPCHK(hipGetLastError());
        HostCopy hc(st);
        SVXCHK(hc.d2h(hpos.data(), B.hpos.p, (size_t)n_hdr * 8));
        SVXCHK(hc.d2h(hrank.data(), B.hrank.p, (size_t)n_hdr * 8));
        SVXCHK(hc.d2h(blob.data(), B.blob.p, (size_t)n_hdr * FA_NAME));
        SVXCHK(hc.finish());
    }
    hrank[(size_t)n_hdr] = n_seq;
    int64_t kept_rec = 0;
    {
        const int rc = svx_fasta_plan(n_hdr, blob.data(), hpos.data(), hrank.data(), n_raw, n_contig, names_nul_separated, dest.data(), off_out, &kept_rec);
        if (rc == SVX_E_FASTA_HOST) { if (stats) stats->host_reason = 3; return rc; }
        SVXCHK(rc);
    }
    const long long n_codes = off_out[n_contig];
    if (stats) { stats->bases_kept = n_codes; stats->records_kept = kept_rec; }
    // ---- encode and place
    SVXCHK(B.codes.reserve(((size_t)n_codes + 15) / 16 * 16 + 64));
    SVXCHK(B.goff.reserve((size_t)(n_contig + 1) * 8 + 64));
    HIPCHK(hipMemsetAsync(B.codes.p, 0, 16, st));                    // (no bases at all: codes is one zero byte)
    SVXCHK(svx_h2d(B.goff.p, off_out, (size_t)(n_contig + 1) * 8, st));
    if (n_hdr > 0 && n_codes > 0) {
        SVXCHK(svx_h2d(B.dest.p, dest.data(), (size_t)n_hdr * 8, st));
        a.dest = B.dest.as<long long>(); a.codes = B.codes.as<uint8_t>(); a.n_codes = n_codes;
        k_fa_tiles<1><<<grid, FA_T, 0, st>>>(a);
        HIPCHK(hipGetLastError());
    }
    uint32_t bad[8];
    {
        HostCopy hc(st);
        SVXCHK(hc.d2h(cnt, B.counters.p, 24));
        SVXCHK(hc.d2h(bad, B.counters.as<uint8_t>() + 64, 32));
        SVXCHK(hc.finish());
    }
    HIPCHK(hipStreamSynchronize(st));
    if (stats) { stats->t_kernels_s = fa_now() - t_staged; memcpy(stats->bad_mask, bad, 32); }
    if (cnt[2]) return svx_fail(SVX_E_CAPACITY, "FASTA loader: a store outside the codes buffer was refused", __FILE__, __LINE__, hipSuccess);
    for (int k = 0; k < 8; k++) if (bad[k]) return svx_fail(SVX_E_FASTA_SYMBOL, "sequence symbols outside the IUPAC/BAM alphabet in a requested record", __FILE__, __LINE__, hipSuccess);
    // ---- the genome of the context
    c->g_off.release(); c->g_codes.release();
    c->g_off = B.goff; c->g_codes = B.codes;
    B.goff = DevBuf(); B.codes = DevBuf();
    c->g_n = n_contig; c->g_borrowed = false;
    c->g_off_p = c->g_off.as<int64_t>(); c->g_codes_p = c->g_codes.as<uint8_t>();
    if (stats) stats->t_total_s = fa_now() - t_begin;
    return SVX_OK;
}

// the resident genome back on the host (tests); NULL arrays: the counts only.  Works for a borrowed device genome, too.
extern "C" int svx_genome_fetch(svx_ctx* c, int32_t* n_contig, int64_t* n_codes, int64_t* off, uint8_t* codes) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    const int32_t n = c->g_n;
    if (n_contig) *n_contig = n;
    if (!c->g_off_p) { if (n_codes) *n_codes = 0; if (n == 0) return SVX_OK; return svx_fail(SVX_E_STATE, "no genome set", __FILE__, __LINE__, hipSuccess); }
    int64_t total = 0;
    SVXCHK(svx_d2h(&total, c->g_off_p + n, 8, c->stream));
    if (n_codes) *n_codes = total;
    if (off) SVXCHK(svx_d2h(off, c->g_off_p, (size_t)(n + 1) * 8, c->stream));
    if (codes && total) SVXCHK(svx_d2h(codes, c->g_codes_p, (size_t)total, c->stream));
    return SVX_OK;
}
