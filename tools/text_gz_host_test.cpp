// text_gz_host_test.cpp - the DEFLATE encoder of svim_amd/csrc/deflate_core.hpp built for the host (-DDEF_HOST: the lane operations emulated), held against
// zlib: every stream must inflate back to its text.  Meant for -fsanitize=address,undefined (tests/test_text_gz.py builds it so).
//   text_gz_host_test fuzz SEED COUNT     COUNT seeded buffers of the kinds the writers meet and the corners of the format -> "COUNT buffers, 0 mismatches"
//   text_gz_host_test file IN OUT         the BGZF stream of file IN written to OUT; prints bytes in / out and blocks by kind
// build: g++ -O1 -g -std=c++17 -DDEF_HOST -fsanitize=address,undefined -I svim_amd/csrc tools/text_gz_host_test.cpp -lz
#include "deflate_core.hpp"
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static uint32_t host_crc(const uint8_t* p, uint32_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, n); }

static uint64_t g_state;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }

// inflate every gzip member of s (zlib, window bits 31) -> false on any error
static bool gunzip_members(const std::vector<uint8_t>& s, std::vector<uint8_t>& out) {
    out.clear();
    size_t at = 0;
    std::vector<uint8_t> buf(1 << 17);
    while (at < s.size()) {
        z_stream z; memset(&z, 0, sizeof z);
        if (inflateInit2(&z, 31) != Z_OK) return false;
        z.next_in = const_cast<uint8_t*>(s.data()) + at; z.avail_in = (uInt)(s.size() - at);
        int rc;
        do {
            z.next_out = buf.data(); z.avail_out = (uInt)buf.size();
            rc = inflate(&z, Z_NO_FLUSH);
            if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&z); return false; }
            out.insert(out.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
        } while (rc != Z_STREAM_END);
        at = s.size() - z.avail_in;
        inflateEnd(&z);
    }
    return true;
}

static void make_buffer(std::vector<uint8_t>& t) {
    static const uint32_t edge[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 4095, 4096, 32767, 32768, 32769, 65279, 65280, 65281, 65284, 130560, 130561};
    const uint32_t kind = rnd() % 8;
    uint32_t n = rnd() % 3 == 0 ? edge[rnd() % (sizeof edge / sizeof edge[0])] : rnd() % (rnd() % 4 == 0 ? 140000u : 3000u);
    t.resize(n);
    if (kind == 0) { for (auto& b : t) b = (uint8_t)rnd(); }                                      // random bytes: stored blocks
    else if (kind == 1) { const uint8_t c = (uint8_t)rnd(); for (auto& b : t) b = c; }                // one repeated byte
    else if (kind == 2) {                                                                           // one repeated line
        const uint32_t l = 1 + rnd() % 400; std::vector<uint8_t> line(l);
        for (auto& b : line) b = (uint8_t)("ACGT\t0123456789chr;=\n"[rnd() % 21]);
        for (uint32_t i = 0; i < n; i++) t[i] = line[i % l];
    } else if (kind == 3) { for (auto& b : t) b = (uint8_t)"ACGT"[rnd() & 3]; }                     // bases: literals only, short codes
    else if (kind == 4) {                                                                           // lines that repeat their neighbours with edits
        std::string line = "chr1\t10000\tsvim.INS.1\tN\t<INS>\t12\tPASS\tSVTYPE=INS;END=10000;SVLEN=300;SUPPORT=12;STD_SPAN=1.2;STD_POS=3.4\tGT:DP:AD\t0/1:20:8,12\n";
        uint32_t i = 0;
        while (i < n) {
            for (int k = 0; k < 3; k++) line[rnd() % (line.size() - 1)] = (char)('0' + rnd() % 10);
            for (size_t k = 0; k < line.size() && i < n; k++) t[i++] = (uint8_t)line[k];
        }
    } else if (kind == 5) {                                                                         // random bytes with one repeat at a chosen distance
        for (auto& b : t) b = (uint8_t)rnd();
        const uint32_t d = (rnd() & 1) ? 32768u + rnd() % 3 - 1 : 1 + rnd() % 40000, l = 4 + rnd() % 300;
        if (n > d + l) { const uint32_t at = d + rnd() % (n - d - l); for (uint32_t k = 0; k < l; k++) t[at + k] = t[at + k - d]; }
    } else if (kind == 6) {                                                                         // runs of chosen lengths between random bytes
        uint32_t i = 0;
        while (i < n) { const uint32_t run = 250 + rnd() % 20; const uint8_t c = (uint8_t)rnd(); for (uint32_t k = 0; k < run && i < n; k++) t[i++] = c; if (i < n) t[i++] = (uint8_t)rnd(); }
    } else { for (uint32_t i = 0; i < n; i++) t[i] = (uint8_t)(rnd() % (1 + i % 7) + 'a'); }           // skewed small alphabet
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "fuzz") {
        g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atoll(argv[2]);
        const long count = atol(argv[3]);
        long bad = 0; int64_t kinds[3] = {0, 0, 0};
        std::vector<uint8_t> t, out, back;
        for (long it = 0; it < count; it++) {
            make_buffer(t);
            out.assign(t.size() + (t.size() / DEF_BLOCK + 2) * 64 + 64, 0);
            const int64_t got = def_file_host(t.data(), (int64_t)t.size(), out.data(), (int64_t)out.size(), host_crc, nullptr, nullptr, kinds);
            if (got < 0) { printf("buffer %ld: no room\n", it); bad++; continue; }
            out.resize((size_t)got);
            if (!gunzip_members(out, back) || back != t) { printf("buffer %ld (%zu bytes): does not inflate back\n", it, t.size()); bad++; }
        }
        printf("%ld buffers, %ld mismatches (blocks: %lld end-of-file, %lld stored, %lld dynamic)\n", count, bad, (long long)kinds[0], (long long)kinds[1], (long long)kinds[2]);
        return bad ? 1 : 0;
    }
    if (argc == 4 && std::string(argv[1]) == "file") {
        FILE* f = fopen(argv[2], "rb");
        if (!f) { perror(argv[2]); return 2; }
        std::vector<uint8_t> t; uint8_t buf[65536]; size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) t.insert(t.end(), buf, buf + k);
        fclose(f);
        std::vector<uint8_t> out(t.size() + (t.size() / DEF_BLOCK + 2) * 64 + 64);
        int64_t kinds[3] = {0, 0, 0};
        const int64_t got = def_file_host(t.data(), (int64_t)t.size(), out.data(), (int64_t)out.size(), host_crc, nullptr, nullptr, kinds);
        if (got < 0) return 1;
        FILE* o = fopen(argv[3], "wb");
        if (!o || fwrite(out.data(), 1, (size_t)got, o) != (size_t)got) { perror(argv[3]); return 2; }
        fclose(o);
        printf("%zu bytes -> %lld bytes (blocks: %lld end-of-file, %lld stored, %lld dynamic)\n", t.size(), (long long)got, (long long)kinds[0], (long long)kinds[1], (long long)kinds[2]);
        return 0;
    }
    fprintf(stderr, "usage: %s fuzz SEED COUNT | file IN OUT\n", argv[0]);
    return 2;
}
