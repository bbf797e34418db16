// bam_name_sort_host_test.cpp - svx_bam_sort_host_order and svx_bam_sort_header_host_order in query-name order (svim_amd/csrc/bamsort_host.cpp) under a seeded
// fuzz of record streams: names of 1 to 254 bytes from a small alphabet (many equal names, many shared prefixes), high bytes, name fields padded behind their
// NUL or without one, every flag bit of the rank, records the definition refuses (no name field, a name field past the record, a reference the header does not
// have, pos < -1), streams cut short.  Every call is held to a plain reimplementation that shares no code with the host build: its own walk of the stream
// decides the status, its own comparison of (name as a string of unsigned bytes, rank from a table of the four flag bits, file index) the permutation, and
// the output must be the records in that order.  Built with the sanitizers by tests/test_bam_name_sort.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I svim_amd/csrc tools/bam_name_sort_host_test.cpp svim_amd/csrc/bamsort_host.cpp -o bam_name_sort_host_test
//   ./bam_name_sort_host_test fuzz <seed> <streams>
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
static uint32_t get32(const std::vector<uint8_t>& v, size_t p) { return (uint32_t)v[p] | ((uint32_t)v[p + 1] << 8) | ((uint32_t)v[p + 2] << 16) | ((uint32_t)v[p + 3] << 24); }

static void add_record(std::vector<uint8_t>& s, int32_t tid, int32_t pos, uint32_t flag, const std::vector<uint8_t>& field, uint32_t l_name, uint32_t extra, uint32_t serial) {
    put32(s, 32u + (uint32_t)field.size() + extra);
    put32(s, (uint32_t)tid); put32(s, (uint32_t)pos); put32(s, 0x12480000u | l_name); put32(s, flag << 16);
    put32(s, serial); put32(s, 0xffffffffu); put32(s, 0xffffffffu); put32(s, 0u);         // (l_seq holds a serial number: records are told apart by their bytes)
    s.insert(s.end(), field.begin(), field.end());
    for (uint32_t k = 0; k < extra; k++) s.push_back((uint8_t)(serial * 7u + k));
}

struct Rec { std::vector<uint8_t> name; int rank; size_t at, len; };      // (vectors of unsigned bytes compare lexicographically, a proper prefix first)

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz <seed> <streams>\n", argv[0]); return 2; }
    g_x = (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull;
    const long n_streams = atol(argv[3]);
    long n_sorted = 0, n_arg = 0, n_range = 0, n_malformed = 0, n_headers = 0, n_bad_names = 0, n_cut = 0;
    // rank by the four bits, written as a table: READ2 READ1 supplementary secondary
    int rank_of[2][2][2][2];
    { int r = 0; for (int r2 = 0; r2 < 2; r2++) for (int r1 = 0; r1 < 2; r1++) for (int sup = 0; sup < 2; sup++) for (int sec = 0; sec < 2; sec++) rank_of[r2][r1][sup][sec] = r++; }
    const uint8_t high[3] = {0x7f, 0x80, 0xff};                // a signed compare puts the last two in front of every letter
    for (long it = 0; it < n_streams; it++) {
        const int kind = (int)below(8);                       // 0-4 sound streams of several name shapes, 5 a record the definition refuses, 6 cut short, 7 both refusals
        const int32_t n_ref = (int32_t)below(6) + 1;
        const uint32_t n = below(5) ? below(250) : 0;
        const uint32_t alphabet = 1 + below(3), max_len = below(3) == 0 ? 254u : 1u + below(12);
        std::vector<uint8_t> s;
        for (uint32_t k = 0; k < n; k++) {
            std::vector<uint8_t> field;
            const uint32_t len = 1 + below(max_len);
            for (uint32_t j = 0; j < len; j++) field.push_back(below(40) == 0 ? high[below(3)] : (uint8_t)('a' + below(alphabet)));
            const int pad = (int)below(6);                    // 0-2 a NUL, 3 a NUL and junk behind it, 4 no NUL at all, 5 a NUL, junk, a NUL
            if (pad != 4) field.push_back(0);
            if (pad == 3 || pad == 5) { const uint32_t j = below((uint32_t)(255 - field.size()) + 1); for (uint32_t q = 0; q < j && field.size() < 255; q++) field.push_back((uint8_t)rnd()); }
            if (pad == 5 && field.size() < 255) field.push_back(0);
            const uint32_t flag = (below(2) ? 64u : 0u) | (below(3) == 0 ? 128u : 0u) | (below(3) == 0 ? 2048u : 0u) | (below(4) == 0 ? 256u : 0u) | (below(2) ? 16u : 0u) | (below(5) == 0 ? 4u : 0u);
            add_record(s, (int32_t)below((uint32_t)n_ref + 1) - 1, (int32_t)below(60) - 1, flag, field, (uint32_t)field.size(), below(4) ? 0u : below(70), k);
        }
        if ((kind == 5 || kind == 7) && n) {
            // a record the definition refuses, written over the fields of a record somewhere
            size_t at = 0; const uint32_t which = below(n);
            for (uint32_t k = 0; k < which; k++) at += 4 + get32(s, at);
            const int what = kind == 7 ? 4 + (int)below(2) : (int)below(5);
            auto w32 = [&](size_t p, uint32_t x) { for (int k = 0; k < 4; k++) s[p + k] = (uint8_t)(x >> (8 * k)); };
            const uint32_t bs = get32(s, at);
            if (what == 0) w32(at + 4, (uint32_t)n_ref);
            else if (what == 1) w32(at + 8, (uint32_t)-2 - below(1000));
            else if (what == 2) s[at + 12] = 0;                                                   // no name field
            else if (what == 3) s[at + 12] = (uint8_t)std::min<uint32_t>(255u, bs - 32u + 1u + below(20));      // a name field past the record (when 255 does not fit either: left as it is)
            else { s[at + 12] = what == 4 ? 0 : (uint8_t)std::min<uint32_t>(255u, bs - 31u); w32(at + 8, (uint32_t)-5); }      // a bad name and pos < -1 in one record
            if (n > 1) { size_t other = 0; const uint32_t w2 = below(n); for (uint32_t k = 0; k < w2; k++) other += 4 + get32(s, other); if (kind == 7 && other != at) w32(other + 8, (uint32_t)-3); }
        }
        if (kind == 6 && s.size() > 1) s.resize(s.size() - 1 - below((uint32_t)std::min<size_t>(s.size() - 1, 300)));
        // ---- the plain reimplementation: walk, status, order ----
        std::vector<Rec> in;
        bool cut = false, bad_arg = false, bad_range = false, bad_name = false;
        for (size_t p = 0; p < s.size();) {
            if (s.size() - p < 4) { cut = true; break; }
            const uint32_t bs = get32(s, p);
            if (bs < 32 || (size_t)bs > s.size() - p - 4) { cut = true; break; }
            const int32_t tid = (int32_t)get32(s, p + 4), pos = (int32_t)get32(s, p + 8);
            const uint32_t l_name = s[p + 12], flag = get32(s, p + 16) >> 16;
            if (tid < -1 || tid >= n_ref) bad_arg = true;
            if (pos < -1) bad_range = true;
            Rec r; r.at = p; r.len = 4 + (size_t)bs; r.rank = rank_of[(flag >> 7) & 1][(flag >> 6) & 1][(flag >> 11) & 1][(flag >> 8) & 1];
            if (l_name == 0 || 32 + l_name > bs) bad_name = true;
            else for (uint32_t j = 0; j < l_name && s[p + 36 + j] != 0; j++) r.name.push_back(s[p + 36 + j]);
            in.push_back(r);
            p += 4 + (size_t)bs;
        }
        const int expect = cut || bad_arg || bad_name ? SVX_E_ARG : bad_range ? SVX_E_RANGE : SVX_OK;
        if (bad_name) n_bad_names++;
        if (cut) n_cut++;
        // the call writes into buffers of exactly the sizes it is told
        std::vector<uint8_t> out(s.size() ? s.size() : 1);
        const int64_t cap = (int64_t)s.size() / 36 + 1;
        std::vector<uint32_t> perm((size_t)cap);
        int64_t n_rec = -1;
        const int rc = svx_bam_sort_host_order(s.data(), (int64_t)s.size(), n_ref, SVX_SORT_QUERYNAME, out.data(), perm.data(), cap, &n_rec);
        if (rc != expect) { n_malformed++; continue; }
        if (rc == SVX_E_ARG) { n_arg++; continue; }
        if (rc == SVX_E_RANGE) { n_range++; continue; }
        std::vector<uint32_t> want(in.size());
        for (size_t k = 0; k < want.size(); k++) want[k] = (uint32_t)k;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return in[a].name != in[b].name ? in[a].name < in[b].name : in[a].rank < in[b].rank; });
        bool ok = (int64_t)in.size() == n_rec;
        size_t at = 0;
        for (size_t k = 0; ok && k < in.size(); k++) {
            const Rec& r = in[want[k]];
            if (perm[k] != want[k] || memcmp(out.data() + at, s.data() + r.at, r.len) != 0) ok = false;
            at += r.len;
        }
        if (ok && at != s.size()) ok = false;
        if (!ok) { n_malformed++; continue; }
        n_sorted++;
        // the coordinate case of the same entry point is the old entry point
        std::vector<uint8_t> o1(out.size()), o2(out.size());
        std::vector<uint32_t> p1((size_t)cap, 0u), p2((size_t)cap, 0u);
        int64_t n1 = -1, n2 = -1;
        const int rc1 = svx_bam_sort_host_order(s.data(), (int64_t)s.size(), n_ref, SVX_SORT_COORDINATE, o1.data(), p1.data(), cap, &n1);
        const int rc2 = svx_bam_sort_host(s.data(), (int64_t)s.size(), n_ref, o2.data(), p2.data(), cap, &n2);
        if (rc1 != rc2 || n1 != n2 || (rc1 == SVX_OK && (memcmp(o1.data(), o2.data(), s.size()) != 0 || p1 != p2))) n_malformed++;
        if (svx_bam_sort_host_order(s.data(), (int64_t)s.size(), n_ref, 2, nullptr, nullptr, 0, &n1) != SVX_E_ARG) n_malformed++;
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
        int rc = svx_bam_sort_header_host_order(h.data(), (int64_t)h.size(), SVX_SORT_QUERYNAME, nullptr, 0, &need);
        if (rc != SVX_E_CAPACITY || need < 12) { n_malformed++; continue; }
        std::vector<uint8_t> out((size_t)need);
        int64_t got = -1;
        rc = svx_bam_sort_header_host_order(h.data(), (int64_t)h.size(), SVX_SORT_QUERYNAME, out.data(), need, &got);
        if (rc != SVX_OK || got != need || memcmp(out.data(), "BAM\1", 4) != 0) { n_malformed++; continue; }
        const uint32_t lt = get32(out, 4);
        const std::string made((const char*)out.data() + 8, lt);
        const std::string line = made.substr(0, made.find('\n'));
        // the new text starts with an @HD line that says queryname, carries the one sub-sort field behind the first SO: and no longer groups
        const std::string ss = "\tSS:queryname:lexicographical";
        const size_t so_at = line.find("\tSO:queryname"), ss_at = line.find("\tSS:");
        if (line.compare(0, 4, "@HD\t") != 0 || so_at == std::string::npos || ss_at != so_at + 13 || line.compare(ss_at, ss.size(), ss) != 0 || line.find("\tSS:", ss_at + 1) != std::string::npos ||
            line.find("\tGO:") != std::string::npos || line.find("SO:coordinate") != std::string::npos || line.find("SO:unsorted") != std::string::npos ||
            made.find('\0') != std::string::npos || (size_t)need != 8 + (size_t)lt + 4 + tail || memcmp(out.data() + 8 + lt, h.data() + 8 + text.size(), 4 + tail) != 0) { n_malformed++; continue; }
        if (svx_bam_sort_header_host_order(h.data(), (int64_t)h.size(), 7, out.data(), need, &got) != SVX_E_ARG) { n_malformed++; continue; }
        n_headers++;
    }
    printf("%ld streams: %ld sorted, %ld bad argument, %ld bad range, %ld headers, %ld malformed; %ld with a bad name, %ld cut short\n", n_streams, n_sorted, n_arg, n_range, n_headers,
           n_malformed, n_bad_names, n_cut);
    return n_malformed ? 1 : 0;
}
