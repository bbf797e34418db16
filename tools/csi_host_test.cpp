// csi_host_test.cpp - svx_bam_index_csi_host and svx_text_index_csi_host (svim_amd/csrc/bamindex_host.cpp, textindex_host.cpp over binidx_host.hpp) under a
// seeded fuzz: row tables that are sorted, sorted with coordinates up to 2^31 and spans up to 2^32, shuffled, or garbage (negative positions, ends in front of
// their begins or far beyond every depth, tids beyond the header); BED and VCF texts with coordinates up to the parser's cap of 2^40, sorted or not.  Every call
// must end in SVX_OK, SVX_E_ORDER or - for a tid the header does not have - SVX_E_ARG, never in SVX_E_RANGE; an index must walk back field by field to exactly
// its size, with a depth of 5 .. 9, ascending bins below the pseudo-bin and the pseudo-bin last.  Meant for -fsanitize=address,undefined (tests/test_csi.py
// builds it so): the inputs are exact-size heap buffers.
//   csi_host_test fuzz SEED COUNT   -> "COUNT inputs, A indexed, B out of order, C bad tid, D deeper than 5, 0 malformed"
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I svim_amd/csrc tools/csi_host_test.cpp svim_amd/csrc/bamindex_host.cpp svim_amd/csrc/textindex_host.cpp
#include "binidx_core.hpp"
#include "../include/svx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_state;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }

struct Table { int32_t n_ref; std::vector<int32_t> tid, pos; std::vector<int64_t> end; std::vector<uint16_t> flag; std::vector<uint64_t> vbeg; uint64_t v_end; };

static Table make_table() {
    Table t;
    t.n_ref = (int32_t)(rnd() % 9);
    const int n = (int)(rnd() % 80);
    const int mode = (int)(rnd() % 4);                // 0: sorted, 1: sorted with huge coordinates, 2: shuffled, 3: garbage mixed in
    int32_t tid = t.n_ref ? (int32_t)(rnd() % (uint32_t)t.n_ref) : -1;
    int64_t pos = rnd() % 1000;
    uint64_t v = ((uint64_t)(rnd() % 100000) << 16) | (rnd() % 65536);
    for (int k = 0; k < n; k++) {
        if (rnd() % 10 == 0) {
            if (mode == 2) tid += (int32_t)(rnd() % 3) - 1; else tid = tid < 0 ? -1 : tid + 1 + (int32_t)(rnd() % 2);
            pos = rnd() % 1000;
        }
        if (tid >= t.n_ref && !(mode == 3 && rnd() % 8 == 0)) tid = -1;
        if (tid < -1) tid = -1;
        pos += mode == 2 && rnd() % 6 == 0 ? -(int64_t)(rnd() % 5000) : (int64_t)(rnd() % (mode == 1 ? 400000000u : 40000u));
        if (pos > 0x7fffff00ll) pos = 0x7fffff00ll;
        int64_t p = pos, e = pos + 1 + (rnd() % 8 == 0 ? (int64_t)rnd() * (mode == 1 ? 16 : 1) % 4294967295ll : (int64_t)(rnd() % 3000u));
        if (mode == 3) {
            const int g = (int)(rnd() % 6);
            if (g == 0) p = -1 - (int64_t)(rnd() % 100); else if (g == 1) e = p - (int64_t)(rnd() % 100); else if (g == 2) e = (int64_t)(rnd() % 7) << 40;
            else if (g == 3 && tid < 0 && t.n_ref) tid = (int32_t)(rnd() % (uint32_t)t.n_ref);
        }
        if (p < -2147483647ll) p = -2147483647ll;
        t.tid.push_back(tid); t.pos.push_back((int32_t)p); t.end.push_back(e); t.flag.push_back((uint16_t)(rnd() % 4096)); t.vbeg.push_back(v);
        v += rnd() % 4 == 0 ? ((uint64_t)(1 + rnd() % 3000) << 16) : 36 + rnd() % 400;
    }
    t.v_end = ((v >> 16) + 1 + rnd() % 100) << 16;
    return t;
}

// the parts of n_ref groups from `at` to the trailer -> false when a field is out of place
static bool walk_groups(const std::vector<uint8_t>& b, size_t at, uint32_t n_ref, int depth, uint64_t want_no_coor) {
    auto u32 = [&](size_t p) { uint32_t v; memcpy(&v, b.data() + p, 4); return v; };
    const uint32_t pseudo = binidx_csi_pseudo_bin(depth);
    for (uint32_t r = 0; r < n_ref; r++) {
        if (at + 4 > b.size()) return false;
        const size_t n_bin = u32(at); at += 4;
        uint32_t prev = 0;
        for (size_t k = 0; k < n_bin; k++) {
            if (at + 16 > b.size()) return false;
            const uint32_t bin = u32(at), n_chunk = u32(at + 12);
            uint64_t loff; memcpy(&loff, b.data() + at + 4, 8);
            if ((k && bin <= prev) || n_chunk == 0 || bin > pseudo || (bin == pseudo && (loff != 0 || n_chunk != 2))) return false;
            prev = bin; at += 16 + 16 * (size_t)n_chunk;
        }
        if (n_bin && prev != pseudo) return false;
    }
    if (at + 8 != b.size()) return false;
    uint64_t no_coor; memcpy(&no_coor, b.data() + at, 8);
    return no_coor == want_no_coor;
}
static int header_depth(const std::vector<uint8_t>& b) {
    if (b.size() < 20 || memcmp(b.data(), "CSI\1", 4) != 0) return -1;
    int32_t ms, depth; memcpy(&ms, b.data() + 4, 4); memcpy(&depth, b.data() + 8, 4);
    return ms == BINIDX_CSI_MIN_SHIFT && depth >= BINIDX_CSI_MIN_DEPTH && depth <= BINIDX_CSI_MAX_DEPTH ? depth : -1;
}

static std::string make_text(int* preset) {
    *preset = (int)(rnd() % 2);
    const int n = (int)(rnd() % 60), mode = (int)(rnd() % 3);      // 0: sorted, 1: sorted with huge coordinates, 2: shuffled now and then
    std::string s;
    int contig = 0; int64_t pos = rnd() % 1000;
    for (int k = 0; k < n; k++) {
        if (rnd() % 12 == 0) { contig += mode == 2 && rnd() % 3 == 0 ? -1 : 1; pos = rnd() % 1000; }
        if (contig < 0) contig = 0;
        pos += mode == 2 && rnd() % 7 == 0 ? -(int64_t)(rnd() % 3000) : mode == 1 ? ((int64_t)rnd() << (rnd() % 10)) : (int64_t)(rnd() % 50000);
        if (pos < 0) pos = 0;
        const int64_t end = pos + 1 + (rnd() % 6 == 0 ? ((int64_t)rnd() << (rnd() % 12)) : (int64_t)(rnd() % 2000));
        char line[256];
        if (rnd() % 25 == 0) snprintf(line, sizeof line, "#comment %d\n", k);
        else if (*preset == SVX_INDEX_BED) snprintf(line, sizeof line, "c%d\t%lld\t%lld\tx\n", contig, (long long)pos, (long long)end);
        else snprintf(line, sizeof line, "c%d\t%lld\tid\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=%lld\n", contig, (long long)pos + 1, (long long)end);
        s += line;
    }
    if (!s.empty() && rnd() % 5 == 0) s.pop_back();                 // no newline at the end
    return s;
}

int main(int argc, char** argv) {
    if (argc != 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz SEED COUNT\n", argv[0]); return 2; }
    g_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)atoll(argv[2]);
    const long count = atol(argv[3]);
    long ok = 0, order = 0, badtid = 0, deep = 0, bad = 0;
    for (long it = 0; it < count; it++) {
        if (it % 2 == 0) {
            const Table t = make_table();
            const size_t n = t.tid.size();
            int32_t* tid = (int32_t*)malloc(n ? n * 4 : 1); int32_t* pos = (int32_t*)malloc(n ? n * 4 : 1); int64_t* end = (int64_t*)malloc(n ? n * 8 : 1);
            uint16_t* flag = (uint16_t*)malloc(n ? n * 2 : 1); uint64_t* vbeg = (uint64_t*)malloc(n ? n * 8 : 1);
            if (n) { memcpy(tid, t.tid.data(), n * 4); memcpy(pos, t.pos.data(), n * 4); memcpy(end, t.end.data(), n * 8); memcpy(flag, t.flag.data(), n * 2); memcpy(vbeg, t.vbeg.data(), n * 8); }
            bool beyond = false; uint64_t unplaced = 0;
            for (int32_t x : t.tid) { beyond = beyond || x >= t.n_ref; unplaced += x < 0; }
            int64_t nb = 0;
            int rc = svx_bam_index_csi_host(t.n_ref, (int64_t)n, tid, pos, end, flag, vbeg, t.v_end, nullptr, 0, &nb);
            if (rc == SVX_E_CAPACITY) {
                uint8_t* out = (uint8_t*)malloc((size_t)nb);
                int64_t nb2 = 0;
                rc = svx_bam_index_csi_host(t.n_ref, (int64_t)n, tid, pos, end, flag, vbeg, t.v_end, out, nb, &nb2);
                const std::vector<uint8_t> b(out, out + nb);
                const int depth = header_depth(b);
                uint32_t l_aux = 1, n_ref = 0;
                if (depth > 0) { memcpy(&l_aux, b.data() + 12, 4); memcpy(&n_ref, b.data() + 16, 4); }
                if (rc != SVX_OK || nb2 != nb || beyond || depth < 0 || l_aux != 0 || n_ref != (uint32_t)t.n_ref || !walk_groups(b, 20, n_ref, depth, unplaced)) bad++;
                else { ok++; deep += depth > 5; }
                free(out);
            } else if (rc == SVX_E_ORDER && !beyond) order++; else if (rc == SVX_E_ARG && beyond) badtid++; else bad++;
            free(tid); free(pos); free(end); free(flag); free(vbeg);
        } else {
            int preset;
            const std::string s = make_text(&preset);
            uint8_t* text = (uint8_t*)malloc(s.size() ? s.size() : 1);
            memcpy(text, s.data(), s.size());
            std::vector<int64_t> coff, uoff;                         // blocks of 65 280 bytes, 100 compressed bytes each, and the end-of-file block
            for (int64_t u = 0; u < (int64_t)s.size(); u += 65280) { uoff.push_back(u); coff.push_back(100 * (int64_t)coff.size()); }
            uoff.push_back((int64_t)s.size()); coff.push_back(100 * (int64_t)coff.size());
            uoff.push_back((int64_t)s.size()); coff.push_back(coff.back() + 28);
            int64_t nb = 0;
            int rc = svx_text_index_csi_host(text, (int64_t)s.size(), coff.data(), uoff.data(), (int64_t)coff.size() - 1, preset, rnd() % 100000, nullptr, 0, &nb);
            if (rc == SVX_E_CAPACITY) {
                uint8_t* out = (uint8_t*)malloc((size_t)nb);
                int64_t nb2 = 0;
                rc = svx_text_index_csi_host(text, (int64_t)s.size(), coff.data(), uoff.data(), (int64_t)coff.size() - 1, preset, 0, out, nb, &nb2);
                const std::vector<uint8_t> b(out, out + nb);
                const int depth = header_depth(b);
                uint32_t l_aux = 0, n_ref = 0;
                bool fine = rc == SVX_OK && nb2 == nb && depth > 0;
                if (fine) { memcpy(&l_aux, b.data() + 12, 4); fine = l_aux >= 28 && 16 + (size_t)l_aux + 4 <= b.size(); }
                if (fine) { memcpy(&n_ref, b.data() + 16 + l_aux, 4); fine = walk_groups(b, 16 + (size_t)l_aux + 4, n_ref, depth, 0); }
                if (!fine) bad++; else { ok++; deep += depth > 5; }
                free(out);
            } else if (rc == SVX_E_ORDER) order++; else bad++;
            free(text);
        }
    }
    printf("%ld inputs, %ld indexed, %ld out of order, %ld bad tid, %ld deeper than 5, %ld malformed\n", count, ok, order, badtid, deep, bad);
    return bad ? 1 : 0;
}
