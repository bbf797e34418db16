// sam_host_test.cpp - svx_sam_convert_host (svim_amd/csrc/sam_host.cpp over sam_core.hpp) under a seeded fuzz: valid alignment lines, the same lines with bytes
// changed, cut short, with overlong numbers put in, and texts of several such lines with and without a last newline.  Every call must end in SVX_OK, SVX_E_ARG or
// SVX_E_RANGE with the number of a line of the text; a size asked for with no room must be the size written into exactly that room, and the records must walk
// back block_size by block_size to exactly that size.  Meant for -fsanitize=address,undefined (tests/test_sam.py builds it so): text and output are exact-size
// heap buffers, so a read or a write one byte outside either is a report.
//   sam_host_test SEED COUNT   -> "sam_host_test ok: COUNT texts, A converted, B refused, 0 malformed"
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I svim_amd/csrc tools/sam_host_test.cpp svim_amd/csrc/sam_host.cpp
#include "sam_core.hpp"
#include "../include/svx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

thread_local std::string g_svx_err;          // (the library keeps its last error here: api.hip)

static uint64_t g_state;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }
static std::string pick(const char* const* v, int n) { return v[rnd() % (uint32_t)n]; }
static std::string digits(int n) { std::string s; for (int k = 0; k < n; k++) s += (char)('0' + rnd() % 10); return s; }

static std::string valid_line() {
    static const char* const refs[] = {"chr1", "chr2", "chrM", "*"};
    static const char* const next[] = {"chr1", "=", "*"};
    static const char* const aux[] = {"NM:i:12", "AS:i:-70000", "XA:A:x", "XZ:Z:", "SA:Z:chr2,100,+,5M5S,60,1;", "XH:H:1AE3", "de:f:0.0123", "XF:f:1e-40", "XF:f:inf", "XB:B:c,1,-2,3",
                                      "XB:B:f,1.5,2e30,nan", "XB:B:S", "XI:i:4294967295", "XJ:i:-2147483648", "XS:B:I,1,2,4294967295"};
    const uint32_t l_seq = rnd() % 5 == 0 ? 0 : rnd() % 70;
    std::string seq, qual, cig;
    for (uint32_t k = 0; k < l_seq; k++) { seq += "ACGTNacgtn=RYK."[rnd() % 15]; qual += (char)(33 + rnd() % 94); }
    const uint32_t n_ops = rnd() % 4 == 0 ? 0 : 1 + rnd() % (rnd() % 20 == 0 ? 200 : 6);
    for (uint32_t k = 0; k < n_ops; k++) { cig += std::to_string(1 + rnd() % (rnd() % 8 == 0 ? 268435455u : 300u)); cig += "MIDNSHP=X"[rnd() % 9]; }
    std::string name;
    for (uint32_t k = 0, n = 1 + rnd() % (rnd() % 10 == 0 ? 254 : 20); k < n; k++) name += (char)('!' + rnd() % 90);
    if (name[0] == '@') name[0] = 'r';
    std::string l = name + "\t" + std::to_string(rnd() % 65536) + "\t" + pick(refs, 4) + "\t" + std::to_string(rnd() % 2 ? rnd() % 100000 : 0) + "\t" + std::to_string(rnd() % 256) + "\t" +
                    (n_ops ? cig : "*") + "\t" + pick(next, 3) + "\t" + std::to_string(rnd() % 5000) + "\t" + std::to_string((int)(rnd() % 2000) - 1000) + "\t" + (l_seq ? seq : "*") + "\t" +
                    ((l_seq && rnd() % 3) ? qual : "*");
    for (uint32_t k = 0, n = rnd() % 6; k < n; k++) l += "\t" + pick(aux, 15);
    return l;
}

static std::string mutate(std::string l) {
    switch (rnd() % 6) {
        case 0: break;                                                                                       // valid
        case 1: for (uint32_t k = 0, n = 1 + rnd() % 3; k < n && !l.empty(); k++) l[rnd() % l.size()] = (char)(rnd() % 256 == '\n' ? 'x' : rnd() % 256); break;
        case 2: l.resize(rnd() % (l.size() + 1)); break;                                                     // cut short
        case 3: { const size_t at = rnd() % (l.size() + 1); l.insert(at, digits(1 + rnd() % 40)); break; }   // an overlong number somewhere
        case 4: { const size_t at = rnd() % (l.size() + 1); l.insert(at, 1, "\t:,*@-+.eB"[rnd() % 10]); break; }
        case 5: { const size_t a = rnd() % (l.size() + 1), b = rnd() % (l.size() + 1); if (a < b) l.erase(a, b - a); break; }
    }
    for (char& c : l) if (c == '\n') c = 'n';
    return l;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sam_host_test SEED COUNT\n"); return 2; }
    g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atoll(argv[1]);
    const long count = atol(argv[2]);
    static const char names[] = "chr1\0chr2\0chrM\0";
    long converted = 0, refused = 0, malformed = 0;
    for (long t = 0; t < count; t++) {
        std::string text;
        const int n_lines = 1 + (int)(rnd() % 4);
        for (int k = 0; k < n_lines; k++) { text += mutate(valid_line()); if (k + 1 < n_lines || rnd() % 2) text += '\n'; }
        uint8_t* in = (uint8_t*)malloc(text.size() ? text.size() : 1);          // exact size: the sanitizer sees a read behind the text
        memcpy(in, text.data(), text.size());
        int64_t need = -1, n_rec = -1, bad = -1;
        const int rc0 = svx_sam_convert_host(in, (int64_t)text.size(), 3, names, nullptr, 0, &need, &n_rec, &bad);
        if (rc0 == SVX_E_ARG || rc0 == SVX_E_RANGE) {
            if (bad < 1 || bad > n_lines + 1) { malformed++; fprintf(stderr, "text %ld: refused at line %lld of %d\n", t, (long long)bad, n_lines); }
            refused++;
        } else if (rc0 == SVX_E_CAPACITY || (rc0 == SVX_OK && need == 0)) {
            uint8_t* out = (uint8_t*)malloc(need ? (size_t)need : 1);
            int64_t got = -1;
            const int rc = svx_sam_convert_host(in, (int64_t)text.size(), 3, names, out, need, &got, &n_rec, &bad);
            int64_t p = 0, walked = 0;
            while (rc == SVX_OK && p + 4 <= got) { uint32_t bs; memcpy(&bs, out + p, 4); if (bs < 32 || p + 4 + (int64_t)bs > got) break; p += 4 + (int64_t)bs; walked++; }
            if (rc != SVX_OK || got != need || p != got || walked != n_rec) { malformed++; fprintf(stderr, "text %ld: rc %d, %lld of %lld bytes, walked %lld of %lld records\n", t, rc, (long long)got, (long long)need, (long long)walked, (long long)n_rec); }
            if (need > 1 && rc == SVX_OK) {                                      // one byte too little room: the size again, nothing written behind the room
                int64_t again = -1;
                uint8_t* tight = (uint8_t*)malloc((size_t)need - 1);
                if (svx_sam_convert_host(in, (int64_t)text.size(), 3, names, tight, need - 1, &again, &n_rec, &bad) != SVX_E_CAPACITY || again != need) malformed++;
                free(tight);
            }
            free(out);
            converted++;
        } else { malformed++; fprintf(stderr, "text %ld: status %d\n", t, rc0); }
        free(in);
    }
    printf("sam_host_test %s: %ld texts, %ld converted, %ld refused, %ld malformed\n", malformed ? "FAILED" : "ok", count, converted, refused, malformed);
    return malformed ? 1 : 0;
}
