// text_index_host_test.cpp - svx_text_index_host (svim_amd/csrc/textindex_host.cpp over textindex_core.hpp) under a seeded fuzz: texts of well-formed, short,
// truncated and garbage lines over block tables of uneven blocks.  Every call must end in SVX_OK, SVX_E_ORDER or SVX_E_RANGE; an index must walk back field
// by field to exactly its size.  Meant for -fsanitize=address,undefined (tests/test_tabix.py builds it so): the text is an exact-size heap buffer, so a
// parser that reads one byte past a line's window or the text's end is reported.
//   text_index_host_test fuzz SEED COUNT   -> "COUNT texts, A indexed, B out of order, C out of range, 0 malformed"
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I svim_amd/csrc tools/text_index_host_test.cpp svim_amd/csrc/textindex_host.cpp
#include "textindex_core.hpp"
#include "../include/svx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_state;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }

static std::string make_text(int preset) {
    std::string t;
    const int n_lines = (int)(rnd() % 60);
    const int mode = (int)(rnd() % 4);                // 0: sorted, 1: sorted with huge coordinates, 2: shuffled contigs, 3: garbage mixed in
    long long pos = 1 + rnd() % 1000; int contig = 0;
    for (int k = 0; k < n_lines; k++) {
        if (rnd() % 12 == 0) contig += mode == 2 ? (int)(rnd() % 3) - 1 : 1, pos = 1 + rnd() % 1000;
        if (contig < 0) contig = 0;
        pos += rnd() % (mode == 1 ? 60000000u : 40000u);
        const long long len = 1 + rnd() % (rnd() % 8 == 0 ? 90000000u : 3000u);
        char buf[256];
        if (mode == 3 && rnd() % 4 == 0) {
            const int g = (int)(rnd() % 5);
            if (g == 0) t += "\n"; else if (g == 1) t += "#comment\tline\n"; else if (g == 2) t += "chrX\n"; else if (g == 3) t += "chr1\t\t\t\t\t\t\tEND=\n";
            else { for (int q = 0, m = (int)(rnd() % 40); q < m; q++) t += (char)(rnd() % 256 == 10 ? 'x' : rnd() % 256); t += "\n"; }
            continue;
        }
        if (preset == SVX_INDEX_BED) snprintf(buf, sizeof buf, "chr%d\t%lld\t%lld\tname;%u\n", contig, pos, pos + len, rnd() % 100);
        else snprintf(buf, sizeof buf, "chr%d\t%lld\tsvim.DEL.%d\tN\t<DEL>\t%u\tPASS\tSVTYPE=DEL;%sEND=%lld;SVLEN=-%lld;READS=", contig, pos, k, rnd() % 60, rnd() % 5 == 0 ? "SEND=7;" : "", pos + len, len);
        t += buf;
        if (preset == SVX_INDEX_VCF) {
            const size_t reads = rnd() % 20 == 0 ? 70000 + rnd() % 140000 : rnd() % 200;
            for (size_t q = 0; q < reads; q++) t += (char)('a' + q % 23);
            t += "\tGT:DP:AD\t./.:.:.,.\n";
        }
    }
    if (!t.empty() && rnd() % 6 == 0) t.resize(t.size() - 1 - rnd() % (t.size() < 30 ? t.size() : 30));      // the last line cut, newline gone
    return t;
}

static bool walk(const std::vector<uint8_t>& b) {
    if (b.size() < 44 || memcmp(b.data(), "TBI\1", 4) != 0) return false;
    auto u32 = [&](size_t at) { uint32_t v; memcpy(&v, b.data() + at, 4); return v; };
    const size_t n_ref = u32(4), l_nm = u32(32);
    size_t at = 36 + l_nm;
    if (at > b.size()) return false;
    for (size_t t = 0; t < n_ref; t++) {
        if (at + 4 > b.size()) return false;
        const size_t n_bin = u32(at); at += 4;
        uint32_t prev = 0;
        for (size_t k = 0; k < n_bin; k++) {
            if (at + 8 > b.size()) return false;
            const uint32_t bin = u32(at), n_chunk = u32(at + 4);
            if ((k && bin <= prev) || n_chunk == 0) return false;
            prev = bin; at += 8 + 16 * (size_t)n_chunk;
        }
        if (prev != BINIDX_PSEUDO_BIN || at + 4 > b.size()) return false;
        at += 4 + 8 * (size_t)u32(at);
    }
    return at + 8 == b.size();
}

int main(int argc, char** argv) {
    if (argc != 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz SEED COUNT\n", argv[0]); return 2; }
    g_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)atoll(argv[2]);
    const long count = atol(argv[3]);
    long ok = 0, order = 0, range = 0, bad = 0;
    for (long it = 0; it < count; it++) {
        const int preset = (int)(rnd() % 2);
        const std::string s = make_text(preset);
        uint8_t* text = (uint8_t*)malloc(s.size() ? s.size() : 1);
        memcpy(text, s.data(), s.size());
        std::vector<int64_t> coff, uoff;
        int64_t u = 0, co = 0;
        while (u < (int64_t)s.size()) { coff.push_back(co); uoff.push_back(u); u += 1 + rnd() % 65280; if (u > (int64_t)s.size()) u = (int64_t)s.size(); co += 30 + rnd() % 40000; }
        coff.push_back(co); uoff.push_back((int64_t)s.size());          // the end-of-file block
        coff.push_back(co + 28); uoff.push_back((int64_t)s.size());
        int64_t n = 0;
        int rc = svx_text_index_host(text, (int64_t)s.size(), coff.data(), uoff.data(), (int64_t)coff.size() - 1, preset, rnd() % 100000, nullptr, 0, &n);
        if (rc == SVX_E_CAPACITY) {
            uint8_t* out = (uint8_t*)malloc((size_t)n);
            int64_t n2 = 0;
            rc = svx_text_index_host(text, (int64_t)s.size(), coff.data(), uoff.data(), (int64_t)coff.size() - 1, preset, 0, out, n, &n2);
            if (rc != SVX_OK || n2 != n || !walk(std::vector<uint8_t>(out, out + n))) bad++; else ok++;
            free(out);
        } else if (rc == SVX_E_ORDER) order++; else if (rc == SVX_E_RANGE) range++; else bad++;
        free(text);
    }
    printf("%ld texts, %ld indexed, %ld out of order, %ld out of range, %ld malformed\n", count, ok, order, range, bad);
    return bad ? 1 : 0;
}
