// bam_sort_host_test.cpp - svx_bam_sort_host and svx_bam_sort_header_host (svim_amd/csrc/bamsort_host.cpp) under a seeded fuzz of record streams: already in
// order, shuffled, with records the definition refuses, cut short, and plain garbage.  Every call must end in a sorted stream that is checked here record by
// record (same records, keys ascending, equal keys in file order, the permutation names them) or in one of the refusals.  Built with the sanitizers by
// tests/test_bam_sort.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I svim_amd/csrc tools/bam_sort_host_test.cpp svim_amd/csrc/bamsort_host.cpp -o bam_sort_host_test
//   ./bam_sort_host_test fuzz <seed> <streams>
#include "../include/svx.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

struct Rec { int32_t tid, pos; uint32_t flag; size_t at, len; };

static void add_record(std::vector<uint8_t>& s, int32_t tid, int32_t pos, uint32_t flag, uint32_t extra, uint32_t serial) {
    put32(s, 32u + extra);
    put32(s, (uint32_t)tid); put32(s, (uint32_t)pos); put32(s, 0x00001401u); put32(s, flag << 16);
    put32(s, serial); put32(s, 0xffffffffu); put32(s, 0xffffffffu); put32(s, 0u);         // (l_seq holds a serial number: records are told apart by their bytes)
    for (uint32_t k = 0; k < extra; k++) s.push_back((uint8_t)(serial + k));
}

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz <seed> <streams>\n", argv[0]); return 2; }
    g_x = (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull;
    const long n_streams = atol(argv[3]);
    long n_sorted = 0, n_arg = 0, n_range = 0, n_malformed = 0, n_headers = 0;
    for (long it = 0; it < n_streams; it++) {
        const int kind = (int)below(8);                       // 0-1 in order, 2-4 shuffled, 5 a bad record somewhere, 6 cut short, 7 garbage
        const int32_t n_ref = (int32_t)below(2) ? (int32_t)below(6) + 1 : (int32_t)below(70000);
        const uint32_t n = below(4) ? below(300) : 0;
        std::vector<uint8_t> s;
        int expect = SVX_OK;
        if (kind == 7) {
            const uint32_t m = below(400);
            for (uint32_t k = 0; k < m; k++) s.push_back((uint8_t)rnd());
        } else {
            int32_t tid = 0, pos = -1;
            for (uint32_t k = 0; k < n; k++) {
                if (kind <= 1) {                              // ascending: sometimes the same place twice, the unplaced tail at the end
                    if (below(10) == 0 && tid + 1 < n_ref) { tid++; pos = -1; }
                    if (below(3)) pos += (int32_t)below(1000);
                } else { tid = n_ref ? (int32_t)below((uint32_t)n_ref + 1) : (int32_t)n_ref; pos = (int32_t)below(50) - 1; }
                int32_t t = tid >= n_ref ? -1 : tid;
                add_record(s, t, t < 0 && below(2) ? -1 : pos, (below(2) ? 16u : 0u) | (below(2) ? 256u : 0u), below(5) ? below(40) : below(3000), k);
            }
            if (kind == 5 && n) {
                // one record the definition refuses, written over the fields of a record somewhere
                size_t at = 0; uint32_t which = below(n);
                for (uint32_t k = 0; k < which; k++) at += 4 + rd32(s.data() + at);
                const int what = (int)below(4);
                uint8_t* r = s.data() + at;
                auto w32 = [](uint8_t* p, uint32_t x) { for (int k = 0; k < 4; k++) p[k] = (uint8_t)(x >> (8 * k)); };
                if (what == 0) { w32(r + 4, (uint32_t)n_ref); expect = SVX_E_ARG; }
                else if (what == 1) { w32(r + 4, (uint32_t)-2); expect = SVX_E_ARG; }
                else if (what == 2) { w32(r + 8, (uint32_t)-2 - below(1000)); expect = SVX_E_RANGE; }
                else { w32(r, below(32)); expect = SVX_E_ARG; }
            }
            if (kind == 6 && s.size() > 1) { s.resize(s.size() - 1 - below((uint32_t)std::min<size_t>(s.size() - 1, 40))); expect = -100; }      // (cut inside the last record, or exactly at a record's end)
        }
        // the call writes into buffers of exactly the sizes it is told
        std::vector<uint8_t> out(s.size() ? s.size() : 1);
        const int64_t cap = (int64_t)s.size() / 36 + 1;
        std::vector<uint32_t> perm((size_t)cap);
        int64_t n_rec = -1;
        const int rc = svx_bam_sort_host(s.data(), (int64_t)s.size(), n_ref, out.data(), perm.data(), cap, &n_rec);
        if (rc == SVX_E_ARG) { n_arg++; if ((expect == SVX_OK && kind < 5) || expect == SVX_E_RANGE) n_malformed++; continue; }
        if (rc == SVX_E_RANGE) { n_range++; if (expect != SVX_E_RANGE) n_malformed++; continue; }
        if (rc != SVX_OK || (expect != SVX_OK && expect != -100 && kind != 7)) { n_malformed++; continue; }
        // walk the input and the output, compare through the permutation
        std::vector<Rec> in;
        bool ok = true;
        for (size_t p = 0; p < s.size();) {
            const uint32_t bs = rd32(s.data() + p);
            in.push_back(Rec{(int32_t)rd32(s.data() + p + 4), (int32_t)rd32(s.data() + p + 8), rd32(s.data() + p + 16) >> 16, p, 4 + (size_t)bs});
            p += 4 + bs;
        }
        if ((int64_t)in.size() != n_rec) ok = false;
        size_t at = 0;
        std::vector<bool> used(in.size(), false);
        for (size_t k = 0; ok && k < in.size(); k++) {
            const uint32_t r = perm[k];
            if (r >= in.size() || used[r]) { ok = false; break; }
            used[r] = true;
            if (memcmp(out.data() + at, s.data() + in[r].at, in[r].len) != 0) { ok = false; break; }
            at += in[r].len;
            if (k) {
                const Rec &a = in[perm[k - 1]], &b = in[r];
                const uint64_t ka[3] = {(uint32_t)a.tid, (uint32_t)(a.pos + 1), a.flag & 16u}, kb[3] = {(uint32_t)b.tid, (uint32_t)(b.pos + 1), b.flag & 16u};
                int cmp = 0;
                for (int j = 0; j < 3 && !cmp; j++) cmp = ka[j] < kb[j] ? -1 : ka[j] > kb[j] ? 1 : 0;
                if (cmp > 0 || (cmp == 0 && perm[k - 1] > r)) ok = false;
            }
        }
        if (ok && at != s.size()) ok = false;
        if (!ok) { n_malformed++; continue; }
        n_sorted++;
        // a permutation buffer that is too small is refused with the count, nothing written beyond it
        if (in.size() > 1) {
            std::vector<uint32_t> small(in.size() - 1);
            int64_t n2 = -1;
            if (svx_bam_sort_host(s.data(), (int64_t)s.size(), n_ref, nullptr, small.data(), (int64_t)small.size(), &n2) != SVX_E_CAPACITY || n2 != (int64_t)in.size()) n_malformed++;
        }
    }
    // headers: texts with and without @HD, fields in any order, NUL padding, garbage
    for (long it = 0; it < n_streams; it++) {
        std::string text;
        const int kind = (int)below(6);
        if (kind <= 3) {
            text = kind == 0 ? "@HD" : "@HD\t";
            const char* fields[] = {"VN:1.6", "SO:queryname", "SO:unsorted", "GO:query", "SS:coordinate:queryname", "XY:z", "", "SO:"};
            const uint32_t nf = below(5);
            for (uint32_t k = 0; k < nf; k++) { if (k || kind == 0) text += '\t'; text += fields[below(8)]; }
            if (below(4)) text += '\n';
            if (below(2)) text += "@SQ\tSN:c\tLN:5\n";
        } else if (kind == 4) text = "@SQ\tSN:c\tLN:5\n@HD\tVN:1.0\n";
        else { const uint32_t m = below(60); for (uint32_t k = 0; k < m; k++) text += (char)rnd(); }
        if (below(3) == 0) text.append(below(9), '\0');
        std::vector<uint8_t> h = {'B', 'A', 'M', 1};
        put32(h, (uint32_t)text.size());
        h.insert(h.end(), text.begin(), text.end());
        const uint32_t tail = below(30);
        put32(h, below(3));
        for (uint32_t k = 0; k < tail; k++) h.push_back((uint8_t)rnd());
        int64_t need = -1;
        int rc = svx_bam_sort_header_host(h.data(), (int64_t)h.size(), nullptr, 0, &need);
        if (rc != SVX_E_CAPACITY || need < 12) { n_malformed++; continue; }
        std::vector<uint8_t> out((size_t)need);
        int64_t got = -1;
        rc = svx_bam_sort_header_host(h.data(), (int64_t)h.size(), out.data(), need, &got);
        if (rc != SVX_OK || got != need || memcmp(out.data(), "BAM\1", 4) != 0) { n_malformed++; continue; }
        const uint32_t lt = rd32(out.data() + 4);
        const std::string made((const char*)out.data() + 8, lt);
        const size_t eol = made.find('\n');
        const std::string line = made.substr(0, eol);
        // the new text starts with an @HD line that says coordinate and no longer groups; what followed the old text still follows the new one
        if (line.compare(0, 4, "@HD\t") != 0 || line.find("\tSO:coordinate") == std::string::npos || line.find("\tGO:") != std::string::npos || line.find("\tSS:") != std::string::npos ||
            made.find('\0') != std::string::npos || (size_t)need != 8 + (size_t)lt + 4 + tail || memcmp(out.data() + 8 + lt, h.data() + 8 + text.size(), 4 + tail) != 0) { n_malformed++; continue; }
        n_headers++;
    }
    printf("%ld streams: %ld sorted, %ld bad argument, %ld bad range, %ld headers, %ld malformed\n", n_streams, n_sorted, n_arg, n_range, n_headers, n_malformed);
    return n_malformed ? 1 : 0;
}
