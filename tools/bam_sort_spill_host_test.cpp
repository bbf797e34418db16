// bam_sort_spill_host_test.cpp - svx_bam_sort_spill_host (svim_amd/csrc/bamsort_host.cpp) under a seeded fuzz: record streams in order, shuffled, with records
// the definition refuses, cut short and plain garbage; run ends anywhere (empty runs, one record per run, one run), pieces of 1 block to more than the file; the
// run file in the call's own memory or behind callbacks, which now and then move fewer bytes than asked.  Every call must give the bytes and the permutation of
// svx_bam_sort_host, the same refusal, or SVX_E_IO exactly when a callback was short.  Built with the sanitizers by tests/test_bam_sort_spill.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I svim_amd/csrc tools/bam_sort_spill_host_test.cpp svim_amd/csrc/bamsort_host.cpp -o bam_sort_spill_host_test
//   ./bam_sort_spill_host_test fuzz <seed> <streams>
#include "../include/svx.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

static void add_record(std::vector<uint8_t>& s, int32_t tid, int32_t pos, uint32_t flag, uint32_t extra, uint32_t serial) {
    put32(s, 32u + extra);
    put32(s, (uint32_t)tid); put32(s, (uint32_t)pos); put32(s, 0x00001401u); put32(s, flag << 16);
    put32(s, serial); put32(s, 0xffffffffu); put32(s, 0xffffffffu); put32(s, 0u);
    for (uint32_t k = 0; k < extra; k++) s.push_back((uint8_t)(serial + k));
}

// the caller's run file: a vector that holds exactly what was written; the call that fails is chosen beforehand
struct File { std::vector<uint8_t> bytes; long calls = 0, fail_at = -1; bool failed = false, out_of_range = false; };
static int64_t file_write(void* user, int64_t offset, const uint8_t* src, int64_t n) {
    File* f = (File*)user;
    if (offset < 0 || n < 0 || offset != (int64_t)f->bytes.size()) { f->out_of_range = true; return -1; }       // (runs are appended back to back)
    if (f->calls++ == f->fail_at) { f->failed = true; n = (int64_t)below((uint32_t)n); }
    f->bytes.insert(f->bytes.end(), src, src + n);
    return n;
}
static int64_t file_read(void* user, int64_t offset, uint8_t* dst, int64_t n) {
    File* f = (File*)user;
    if (offset < 0 || n < 0 || offset + n > (int64_t)f->bytes.size()) { f->out_of_range = true; return -1; }
    if (f->calls++ == f->fail_at) { f->failed = true; n = (int64_t)below((uint32_t)n); }
    memcpy(dst, f->bytes.data() + offset, (size_t)n);
    return n;
}

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz <seed> <streams>\n", argv[0]); return 2; }
    g_x = (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull;
    const long n_streams = atol(argv[3]);
    long n_equal = 0, n_refused = 0, n_io = 0, n_bad_runs = 0, n_malformed = 0;
    for (long it = 0; it < n_streams; it++) {
        const int kind = (int)below(8);                       // 0-1 in order, 2-4 shuffled, 5 a bad record somewhere, 6 cut short, 7 garbage
        const int32_t n_ref = (int32_t)below(2) ? (int32_t)below(6) + 1 : (int32_t)below(70000);
        const uint32_t n = below(5) ? below(400) : 0;
        std::vector<uint8_t> s;
        if (kind == 7) {
            const uint32_t m = below(400);
            for (uint32_t k = 0; k < m; k++) s.push_back((uint8_t)rnd());
        } else {
            int32_t tid = 0, pos = -1;
            for (uint32_t k = 0; k < n; k++) {
                if (kind <= 1) {
                    if (below(10) == 0 && tid + 1 < n_ref) { tid++; pos = -1; }
                    if (below(3)) pos += (int32_t)below(1000);
                } else { tid = n_ref ? (int32_t)below((uint32_t)n_ref + 1) : (int32_t)n_ref; pos = (int32_t)below(50) - 1; }
                const int32_t t = tid >= n_ref ? -1 : tid;
                // now and then a record of several blocks: it straddles pieces and is its run's only contribution to them
                add_record(s, t, t < 0 && below(2) ? -1 : pos, (below(2) ? 16u : 0u) | (below(2) ? 256u : 0u), below(120) ? below(60) : below(200000), k);
            }
            if (kind == 5 && n) {
                size_t at = 0; const uint32_t which = below(n);
                for (uint32_t k = 0; k < which; k++) at += 4 + rd32(s.data() + at);
                uint8_t* r = s.data() + at;
                auto w32 = [](uint8_t* p, uint32_t x) { for (int k = 0; k < 4; k++) p[k] = (uint8_t)(x >> (8 * k)); };
                const int what = (int)below(4);
                if (what == 0) w32(r + 4, (uint32_t)n_ref); else if (what == 1) w32(r + 4, (uint32_t)-2); else if (what == 2) w32(r + 8, (uint32_t)-2 - below(1000)); else w32(r, below(32));
            }
            if (kind == 6 && s.size() > 1) s.resize(s.size() - 1 - below((uint32_t)std::min<size_t>(s.size() - 1, 40)));
        }
        // what the in-memory host build says
        std::vector<uint8_t> want(s.size() ? s.size() : 1), out(s.size() ? s.size() : 1);
        const int64_t cap = (int64_t)s.size() / 36 + 1;
        std::vector<uint32_t> want_perm((size_t)cap), perm((size_t)cap);
        int64_t n_want = -1, n_rec = -1;
        const int rc0 = svx_bam_sort_host(s.data(), (int64_t)s.size(), n_ref, want.data(), want_perm.data(), cap, &n_want);
        // run ends: none but the end, a few, many, one record per run; sometimes an end too many or out of order (refused)
        std::vector<int64_t> ends;
        const int64_t nr = rc0 == SVX_OK ? n_want : (int64_t)below(20);
        const int how = (int)below(5);
        if (how == 0) ends.push_back(nr);
        else if (how == 1) for (int64_t k = 1; k <= nr; k++) ends.push_back(k);
        else {
            const uint32_t cuts = how == 2 ? below(4) : below(300);
            for (uint32_t k = 0; k < cuts; k++) ends.push_back((int64_t)below((uint32_t)nr + 1));
            std::sort(ends.begin(), ends.end());
            ends.push_back(nr);
        }
        if (nr == 0 && below(2)) ends.clear();
        bool runs_bad = false;
        if (rc0 == SVX_OK && below(25) == 0) {
            runs_bad = true;
            if (below(2) || ends.empty()) ends.push_back(nr + 1 + (int64_t)below(3));                         // an end beyond the records
            else if (ends.size() >= 2 && ends[0] != ends.back()) std::swap(ends[0], ends.back());              // out of order
            else ends.back() = nr + 1;
        }
        const int64_t piece_blocks = (int)below(3) == 0 ? 1 : (int)below(2) ? 1 + (int64_t)below(4) : 4096;
        File f;
        const bool callbacks = below(3) != 0;
        if (callbacks && below(4) == 0) f.fail_at = (long)below(2 * (uint32_t)ends.size() + 4);
        const int rc = svx_bam_sort_spill_host(s.data(), (int64_t)s.size(), n_ref, ends.empty() ? nullptr : ends.data(), (int64_t)ends.size(), piece_blocks, out.data(), perm.data(), cap,
                                               &n_rec, callbacks ? file_write : nullptr, callbacks ? file_read : nullptr, &f);
        if (f.out_of_range) { n_malformed++; continue; }
        if (rc0 != SVX_OK) { if (rc == rc0) n_refused++; else n_malformed++; continue; }
        if (runs_bad) { if (rc == SVX_E_ARG) n_bad_runs++; else n_malformed++; continue; }
        if (f.failed) { if (rc == SVX_E_IO) n_io++; else n_malformed++; continue; }
        if (rc != SVX_OK || n_rec != n_want || memcmp(out.data(), want.data(), s.size()) != 0 ||
            (n_want && memcmp(perm.data(), want_perm.data(), (size_t)n_want * 4) != 0)) { n_malformed++; continue; }
        if (callbacks && f.bytes.size() != s.size()) { n_malformed++; continue; }                             // every record was written to the run file once
        n_equal++;
    }
    printf("%ld streams: %ld equal, %ld refused, %ld short io, %ld bad runs, %ld malformed\n", n_streams, n_equal, n_refused, n_io, n_bad_runs, n_malformed);
    return n_malformed ? 1 : 0;
}
