// bam_index_host_test.cpp - svx_bam_index_host (svim_amd/csrc/bamindex_host.cpp over bamindex_core.hpp) under a seeded fuzz: row tables that are sorted,
// sorted with huge coordinates, shuffled, or garbage (negative positions, ends in front of their begins, placed rows behind unplaced ones, tids beyond the
// header).  Every call must end in SVX_OK, SVX_E_ORDER, SVX_E_RANGE or - for a tid the header does not have - SVX_E_ARG; an index must walk back field by
// field to exactly its size.  Meant for -fsanitize=address,undefined (tests/test_bai.py builds it so): the columns are exact-size heap buffers.
//   bam_index_host_test fuzz SEED COUNT   -> "COUNT tables, A indexed, B out of order, C out of range, D bad tid, 0 malformed"
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I svim_amd/csrc tools/bam_index_host_test.cpp svim_amd/csrc/bamindex_host.cpp
#include "bamindex_core.hpp"
#include "../include/svx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        if (tid >= t.n_ref && !(mode == 3 && rnd() % 8 == 0)) tid = -1;          // the unplaced tail (a garbage table keeps a tid beyond the header now and then)
        if (tid < -1) tid = -1;
        pos += mode == 2 && rnd() % 6 == 0 ? -(int64_t)(rnd() % 5000) : (int64_t)(rnd() % (mode == 1 ? 40000000u : 40000u));
        if (pos > 0x7fffff00ll) pos = 0x7fffff00ll;
        int64_t p = pos, e = pos + 1 + rnd() % (rnd() % 8 == 0 ? 90000000u : 3000u);
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

static bool walk(const std::vector<uint8_t>& b, const Table& t) {
    if (b.size() < 16 || memcmp(b.data(), "BAI\1", 4) != 0) return false;
    auto u32 = [&](size_t at) { uint32_t v; memcpy(&v, b.data() + at, 4); return v; };
    if (u32(4) != (uint32_t)t.n_ref) return false;
    size_t at = 8;
    for (int32_t r = 0; r < t.n_ref; r++) {
        if (at + 4 > b.size()) return false;
        const size_t n_bin = u32(at); at += 4;
        uint32_t prev = 0;
        for (size_t k = 0; k < n_bin; k++) {
            if (at + 8 > b.size()) return false;
            const uint32_t bin = u32(at), n_chunk = u32(at + 4);
            if ((k && bin <= prev) || n_chunk == 0) return false;
            prev = bin; at += 8 + 16 * (size_t)n_chunk;
        }
        if ((n_bin && prev != BINIDX_PSEUDO_BIN) || at + 4 > b.size()) return false;
        const size_t n_intv = u32(at);
        if ((n_bin == 0) != (n_intv == 0)) return false;
        at += 4 + 8 * n_intv;
    }
    if (at + 8 != b.size()) return false;
    uint64_t no_coor; memcpy(&no_coor, b.data() + at, 8);
    uint64_t unplaced = 0;
    for (int32_t x : t.tid) unplaced += x < 0;
    return no_coor == unplaced;
}

int main(int argc, char** argv) {
    if (argc != 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz SEED COUNT\n", argv[0]); return 2; }
    g_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)atoll(argv[2]);
    const long count = atol(argv[3]);
    long ok = 0, order = 0, range = 0, badtid = 0, bad = 0;
    for (long it = 0; it < count; it++) {
        const Table t = make_table();
        const size_t n = t.tid.size();
        // exact-size heap copies: a read one row past the table is reported
        int32_t* tid = (int32_t*)malloc(n ? n * 4 : 1); int32_t* pos = (int32_t*)malloc(n ? n * 4 : 1); int64_t* end = (int64_t*)malloc(n ? n * 8 : 1);
        uint16_t* flag = (uint16_t*)malloc(n ? n * 2 : 1); uint64_t* vbeg = (uint64_t*)malloc(n ? n * 8 : 1);
        if (n) { memcpy(tid, t.tid.data(), n * 4); memcpy(pos, t.pos.data(), n * 4); memcpy(end, t.end.data(), n * 8); memcpy(flag, t.flag.data(), n * 2); memcpy(vbeg, t.vbeg.data(), n * 8); }
        bool beyond = false;
        for (int32_t x : t.tid) beyond = beyond || x >= t.n_ref;
        int64_t nb = 0;
        int rc = svx_bam_index_host(t.n_ref, (int64_t)n, tid, pos, end, flag, vbeg, t.v_end, nullptr, 0, &nb);
        if (rc == SVX_E_CAPACITY) {
            uint8_t* out = (uint8_t*)malloc((size_t)nb);
            int64_t nb2 = 0;
            rc = svx_bam_index_host(t.n_ref, (int64_t)n, tid, pos, end, flag, vbeg, t.v_end, out, nb, &nb2);
            if (rc != SVX_OK || nb2 != nb || beyond || !walk(std::vector<uint8_t>(out, out + nb), t)) bad++; else ok++;
            free(out);
        } else if (rc == SVX_E_ORDER && !beyond) order++; else if (rc == SVX_E_RANGE && !beyond) range++; else if (rc == SVX_E_ARG && beyond) badtid++; else bad++;
        free(tid); free(pos); free(end); free(flag); free(vbeg);
    }
    printf("%ld tables, %ld indexed, %ld out of order, %ld out of range, %ld bad tid, %ld malformed\n", count, ok, order, range, badtid, bad);
    return bad ? 1 : 0;
}
