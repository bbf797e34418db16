// text_gz_host_test.cpp - the DEFLATE encoder of svim_amd/csrc/deflate_core.hpp built for the host (-DDEF_HOST: the lane operations emulated), held against
// zlib: every stream must inflate back to its text.  Meant for -fsanitize=address,undefined (tests/test_text_gz.py builds it so).
//   text_gz_host_test fuzz SEED COUNT     COUNT seeded buffers of the kinds the writers meet and the corners of the format -> "COUNT buffers, 0 mismatches"
//   text_gz_host_test file IN OUT         the BGZF stream of file IN written to OUT; prints bytes in / out and blocks by kind
//   text_gz_host_test cases FILE          the phase-level cases of tests/deflate_encode_cases.py (write_case_file: inputs and what tests/deflate_model.py answers)
//                                         through the host phases (textgz_phase.hpp) -> "cases: N blocks, 0 mismatches"; exit status 3 when a block differs
// build: g++ -O1 -g -std=c++17 -DDEF_HOST -fsanitize=address,undefined -I svim_amd/csrc tools/text_gz_host_test.cpp -lz
#include "deflate_core.hpp"
#include "textgz_phase.hpp"
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

// ---- cases FILE: sections of (phase, nb, text, text_off, n, crc, inputs, expected results), little-endian, as write_case_file lays them out ----
template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t count) { v.resize(count); return count == 0 || fread(v.data(), sizeof(T), count, f) == count; }
static int run_cases(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    std::vector<int64_t> head;
    long blocks = 0, bad = 0;
    if (!rd(f, head, 1) || head[0] != 0x3143464544585653ll) { fprintf(stderr, "%s: not a case file\n", path); return 2; }
    while (rd(f, head, 3)) {
        const int phase = (int)head[0]; const int64_t nb = head[1], n_text = head[2];
        if (phase < 0 || phase > 2 || nb < 1 || nb > TGZ_PHASE_MAXBLOCKS || n_text < 0) { fprintf(stderr, "%s: bad section\n", path); return 2; }
        std::vector<uint8_t> text, want_bytes, slots;
        std::vector<int64_t> off;
        std::vector<uint32_t> n, crc, nt, want_nt, hist, want_hist, dense, codes, want_codes, want_size, tok((size_t)(phase == 1 ? 1 : nb * (int64_t)DEF_BLOCK), 0u);
        bool ok = rd(f, text, (size_t)n_text) && rd(f, off, (size_t)nb + 1) && rd(f, n, (size_t)nb) && rd(f, crc, (size_t)nb);
        auto dense_sum = [&](const std::vector<uint32_t>& c) { size_t t = 0; for (uint32_t x : c) t += x; return t; };
        if (ok && phase == TGZ_PHASE_MATCH) ok = rd(f, want_nt, (size_t)nb) && rd(f, want_hist, (size_t)nb * DEF_NHIST) && rd(f, dense, dense_sum(want_nt));
        if (ok && phase == TGZ_PHASE_CODES) ok = rd(f, hist, (size_t)nb * DEF_NHIST) && rd(f, want_codes, (size_t)nb * TGZ_CODES_WORDS);
        if (ok && phase == TGZ_PHASE_BITS) ok = rd(f, nt, (size_t)nb) && rd(f, dense, dense_sum(nt)) && rd(f, codes, (size_t)nb * TGZ_CODES_WORDS) && rd(f, want_size, (size_t)nb) && rd(f, want_bytes, dense_sum(want_size));
        if (!ok) { fprintf(stderr, "%s: truncated\n", path); return 2; }
        text.resize(text.size() + 1);                   // (data() of an empty vector may be null)
        if (phase == TGZ_PHASE_MATCH) { nt.assign((size_t)nb, 0u); hist.assign((size_t)nb * DEF_NHIST, 0u); }
        if (phase == TGZ_PHASE_CODES) codes.assign((size_t)nb * TGZ_CODES_WORDS, 0xffffffffu);
        if (phase == TGZ_PHASE_BITS) {
            slots.assign((size_t)nb * DEF_SLOT, 0);
            size_t at = 0;
            for (int64_t b = 0; b < nb; b++) { if (nt[b] > DEF_BLOCK) return 2; memcpy(tok.data() + b * (int64_t)DEF_BLOCK, dense.data() + at, (size_t)nt[b] * 4); at += nt[b]; }
        }
        if (const char* why = tgz_phase_host(phase, nb, text.data(), off.data(), n.data(), crc.data(), tok.data(), nt.data(), hist.data(), codes.data(), slots.data())) {
            printf("phase %d: refused: %s\n", phase, why);
            return 2;
        }
        size_t at = 0;
        for (int64_t b = 0; b < nb; b++) {
            bool same = true;
            if (phase == TGZ_PHASE_MATCH) {
                same = nt[b] == want_nt[b] && !memcmp(&hist[b * DEF_NHIST], &want_hist[b * DEF_NHIST], DEF_NHIST * 4) && !memcmp(&tok[b * (int64_t)DEF_BLOCK], dense.data() + at, (size_t)want_nt[b] * 4);
                at += want_nt[b];
            } else if (phase == TGZ_PHASE_CODES) same = !memcmp(&codes[b * TGZ_CODES_WORDS], &want_codes[b * TGZ_CODES_WORDS], TGZ_CODES_WORDS * 4);
            else { same = !memcmp(&slots[b * (int64_t)DEF_SLOT], want_bytes.data() + at, want_size[b]); at += want_size[b]; }
            if (!same) { if (bad < 10) printf("phase %d, block %lld differs\n", phase, (long long)b); bad++; }
        }
        blocks += nb;
    }
    fclose(f);
    printf("cases: %ld blocks, %ld mismatches\n", blocks, bad);
    return bad ? 3 : 0;
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
    if (argc == 3 && std::string(argv[1]) == "cases") return run_cases(argv[2]);
    fprintf(stderr, "usage: %s fuzz SEED COUNT | file IN OUT | cases FILE\n", argv[0]);
    return 2;
}
