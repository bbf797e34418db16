// bam_name_merge_host_test.cpp - svx_bam_merge_host_order in query-name order (svim_amd/csrc/bamsort_host.cpp) under a seeded fuzz of multi-file record
// streams, and the name table of bamsort_core.hpp (bsort_name_tab_words / _pack / _word) against the name's own bytes.
// Streams: 1 to 4 files, each with a dictionary size and an id map of its own (the identity, or any map into the merged dictionary), names of 1 to 254 bytes
// from a small alphabet (equal names and shared prefixes within and ACROSS files), high bytes, name fields padded behind their NUL or without one, every flag
// bit of the rank, mate ids of every kind, records the definition refuses (a reference or - in a translated file - a mate reference the file's header does not
// have, no name field, a name field past the record, pos < -1), files cut short.  Every call is held to a plain reimplementation that shares no code with the
// host build: its own walk decides the status (SVX_E_ARG in any file before SVX_E_RANGE in any file), its own translation makes the expected bytes, and its
// own comparison of (name as a string of unsigned bytes, rank from a table of the four flag bits, global record number) the permutation.
// The table: every length 1..255 at every word offset of a small table, first and last word included - the words written are exactly the name's, every round
// 0..63 reads the big-endian word of the name's bytes, and the source is an allocation of exactly the name's length (a read behind it is a sanitizer report).
// Built with the sanitizers by tests/test_bam_name_merge.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I svim_amd/csrc tools/bam_name_merge_host_test.cpp svim_amd/csrc/bamsort_host.cpp -o bam_name_merge_host_test
//   ./bam_name_merge_host_test fuzz <seed> <streams>
#include "../include/svx.h"
#include "bamsort_core.hpp"
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
static void set32(std::vector<uint8_t>& v, size_t p, uint32_t x) { for (int k = 0; k < 4; k++) v[p + k] = (uint8_t)(x >> (8 * k)); }

static void add_record(std::vector<uint8_t>& s, int32_t tid, int32_t pos, uint32_t flag, int32_t mate, const std::vector<uint8_t>& field, uint32_t extra, uint32_t serial) {
    put32(s, 32u + (uint32_t)field.size() + extra);
    put32(s, (uint32_t)tid); put32(s, (uint32_t)pos); put32(s, 0x12480000u | (uint32_t)field.size()); put32(s, flag << 16);
    put32(s, serial); put32(s, (uint32_t)mate); put32(s, 0xffffffffu); put32(s, 0u);        // (l_seq holds a serial number: records are told apart by their bytes)
    s.insert(s.end(), field.begin(), field.end());
    for (uint32_t k = 0; k < extra; k++) s.push_back((uint8_t)(serial * 7u + k));
}

struct Rec { std::vector<uint8_t> name, bytes; int rank; };

static long table_checks(long* n_wrong) {
    long n = 0;
    for (uint32_t len = 1; len <= 255; len++) {
        std::vector<uint8_t> name(len);                                  // exactly the name: nothing behind it may be read
        for (uint32_t k = 0; k < len; k++) name[k] = (uint8_t)(1 + (rnd() % 255));
        const uint32_t words = (len + 3) / 4;
        if (bsort_name_tab_words(len) != words) (*n_wrong)++;
        const uint32_t tab_words = 64 + 3;
        const uint32_t offs[4] = {0u, tab_words - words, 1u + below(tab_words - words), below(tab_words - words + 1)};      // the table's first word, its last word, two in between
        for (uint32_t off : offs) {
            std::vector<uint32_t> tab(tab_words, 0xdeadbeefu);           // (a heap block of exactly the table: a word behind it is a report)
            bsort_name_tab_pack(name.data(), len, tab.data() + off);
            for (uint32_t w = 0; w < tab_words; w++) if ((w < off || w >= off + words) && tab[w] != 0xdeadbeefu) (*n_wrong)++;
            for (uint32_t r = 0; r < 64; r++) {
                uint32_t want = 0;
                for (uint32_t k = 0; k < 4; k++) want = (want << 8) | (4 * r + k < len ? name[4 * r + k] : 0u);
                if (bsort_name_tab_word(tab.data(), off, len, r) != want || bsort_name_word(name.data(), len, r) != want) (*n_wrong)++;
                n++;
            }
        }
    }
    if (bsort_name_tab_words(0) != 1) (*n_wrong)++;
    return n;
}

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz <seed> <streams>\n", argv[0]); return 2; }
    g_x = (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull;
    const long n_streams = atol(argv[3]);
    long n_merged = 0, n_arg = 0, n_range = 0, n_malformed = 0, n_bad_names = 0, n_cut = 0, n_both = 0, n_translated = 0, n_table_wrong = 0;
    int rank_of[2][2][2][2];
    { int r = 0; for (int r2 = 0; r2 < 2; r2++) for (int r1 = 0; r1 < 2; r1++) for (int sup = 0; sup < 2; sup++) for (int sec = 0; sec < 2; sec++) rank_of[r2][r1][sup][sec] = r++; }
    const uint8_t high[3] = {0x7f, 0x80, 0xff};
    for (long it = 0; it < n_streams; it++) {
        const uint32_t k = 1 + below(4);
        const int32_t n_ref_merged = (int32_t)below(7) + 1;
        const uint32_t alphabet = 1 + below(3), max_len = below(3) == 0 ? 254u : 1u + below(10);
        const int kind = (int)below(8);                       // 0-4 sound, 5 one refused record, 6 a file cut short, 7 an E_ARG and an E_RANGE refusal in different files
        std::vector<std::vector<uint8_t>> files(k);
        std::vector<int32_t> n_ref(k), flat;
        std::vector<std::vector<int32_t>> maps(k);
        std::vector<uint32_t> n_of(k);
        uint32_t serial = 0;
        for (uint32_t f = 0; f < k; f++) {
            n_ref[f] = (int32_t)below((uint32_t)n_ref_merged + 1);
            const bool ident = below(3) == 0;
            for (int32_t i = 0; i < n_ref[f]; i++) maps[f].push_back(ident ? i : (int32_t)below((uint32_t)n_ref_merged));
            n_of[f] = below(5) ? below(120) : 0;
            for (uint32_t j = 0; j < n_of[f]; j++) {
                std::vector<uint8_t> field;
                const uint32_t len = 1 + below(max_len);
                for (uint32_t q = 0; q < len; q++) field.push_back(below(40) == 0 ? high[below(3)] : (uint8_t)('a' + below(alphabet)));
                const int pad = (int)below(6);
                if (pad != 4) field.push_back(0);
                if (pad == 3 || pad == 5) { const uint32_t q = below((uint32_t)(255 - field.size()) + 1); for (uint32_t u = 0; u < q && field.size() < 255; u++) field.push_back((uint8_t)rnd()); }
                if (pad == 5 && field.size() < 255) field.push_back(0);
                const uint32_t flag = (below(2) ? 64u : 0u) | (below(3) == 0 ? 128u : 0u) | (below(3) == 0 ? 2048u : 0u) | (below(4) == 0 ? 256u : 0u) | (below(2) ? 16u : 0u);
                add_record(files[f], (int32_t)below((uint32_t)n_ref[f] + 1) - 1, (int32_t)below(60) - 1, flag, (int32_t)below((uint32_t)n_ref[f] + 1) - 1, field, below(4) ? 0u : below(70), serial++);
            }
        }
        auto spoil = [&](uint32_t f, int what) {              // one record of file f gets a fault: 0 refID, 1 mate id, 2 no name field, 3 a name field past the record, 4 pos < -1
            if (!n_of[f]) return;
            std::vector<uint8_t>& s = files[f];
            size_t at = 0; const uint32_t which = below(n_of[f]);
            for (uint32_t j = 0; j < which; j++) at += 4 + get32(s, at);
            const uint32_t bs = get32(s, at);
            if (what == 0) set32(s, at + 4, below(2) ? (uint32_t)n_ref[f] : (uint32_t)-2);
            else if (what == 1) set32(s, at + 24, below(2) ? (uint32_t)n_ref[f] + below(3) : (uint32_t)-2 - below(9));
            else if (what == 2) s[at + 12] = 0;
            else if (what == 3) s[at + 12] = (uint8_t)std::min<uint32_t>(255u, bs - 32u + 1u + below(20));
            else set32(s, at + 8, (uint32_t)-2 - below(1000));
        };
        if (kind == 5) spoil(below(k), (int)below(5));
        if (kind == 7) { const uint32_t f = below(k); spoil(f, (int)below(4)); spoil(k > 1 ? (f + 1 + below(k - 1)) % k : f, 4); }
        if (kind == 6) { const uint32_t f = below(k); if (files[f].size() > 1) files[f].resize(files[f].size() - 1 - below((uint32_t)std::min<size_t>(files[f].size() - 1, 300))); }
        // ---- the plain reimplementation: walk every file, translate, status, order ----
        std::vector<Rec> in;
        bool cut = false, bad_arg = false, bad_range = false, bad_name = false;
        for (uint32_t f = 0; f < k; f++) {
            const std::vector<uint8_t>& s = files[f];
            bool ident = true;
            for (int32_t i = 0; i < n_ref[f]; i++) if (maps[f][(size_t)i] != i) ident = false;
            if (!ident) n_translated++;
            for (size_t p = 0; p < s.size();) {
                if (s.size() - p < 4) { cut = true; break; }
                const uint32_t bs = get32(s, p);
                if (bs < 32 || (size_t)bs > s.size() - p - 4) { cut = true; break; }
                const int32_t tid = (int32_t)get32(s, p + 4), pos = (int32_t)get32(s, p + 8), mate = (int32_t)get32(s, p + 24);
                const uint32_t l_name = s[p + 12], flag = get32(s, p + 16) >> 16;
                Rec r; r.bytes.assign(s.begin() + (long)p, s.begin() + (long)(p + 4 + bs));
                r.rank = rank_of[(flag >> 7) & 1][(flag >> 6) & 1][(flag >> 11) & 1][(flag >> 8) & 1];
                if (tid < -1 || tid >= n_ref[f]) bad_arg = true;
                else if (!ident) set32(r.bytes, 4, tid < 0 ? 0xffffffffu : (uint32_t)maps[f][(size_t)tid]);
                if (!ident) { if (mate < -1 || mate >= n_ref[f]) bad_arg = true; else set32(r.bytes, 24, mate < 0 ? 0xffffffffu : (uint32_t)maps[f][(size_t)mate]); }
                if (pos < -1) bad_range = true;
                if (l_name == 0 || 32 + l_name > bs) bad_name = true;
                else for (uint32_t j = 0; j < l_name && s[p + 36 + j] != 0; j++) r.name.push_back(s[p + 36 + j]);
                in.push_back(r);
                p += 4 + (size_t)bs;
            }
            if (cut) break;
        }
        const int expect = cut || bad_arg || bad_name ? SVX_E_ARG : bad_range ? SVX_E_RANGE : SVX_OK;
        if (bad_name) n_bad_names++;
        if (cut) n_cut++;
        if ((bad_arg || bad_name) && bad_range) n_both++;
        std::vector<const uint8_t*> sp(k); std::vector<int64_t> ss(k);
        size_t total = 0;
        static const uint8_t nothing[1] = {0};
        for (uint32_t f = 0; f < k; f++) { sp[f] = files[f].empty() ? nothing : files[f].data(); ss[f] = (int64_t)files[f].size(); total += files[f].size(); for (int32_t t : maps[f]) flat.push_back(t); }
        std::vector<uint8_t> out(total ? total : 1);
        const int64_t cap = (int64_t)total / 36 + 1;
        std::vector<uint32_t> perm((size_t)cap);
        int64_t n_rec = -1;
        const int rc = svx_bam_merge_host_order(sp.data(), ss.data(), n_ref.data(), (int64_t)k, n_ref_merged, flat.empty() ? nullptr : flat.data(), SVX_SORT_QUERYNAME, out.data(), perm.data(), cap, &n_rec);
        if (rc != expect) { n_malformed++; continue; }
        if (rc == SVX_E_ARG) { n_arg++; continue; }
        if (rc == SVX_E_RANGE) { n_range++; continue; }
        std::vector<uint32_t> want(in.size());
        for (size_t j = 0; j < want.size(); j++) want[j] = (uint32_t)j;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return in[a].name != in[b].name ? in[a].name < in[b].name : in[a].rank < in[b].rank; });
        bool ok = (int64_t)in.size() == n_rec;
        size_t at = 0;
        for (size_t j = 0; ok && j < in.size(); j++) {
            const Rec& r = in[want[j]];
            if (perm[j] != want[j] || memcmp(out.data() + at, r.bytes.data(), r.bytes.size()) != 0) ok = false;
            at += r.bytes.size();
        }
        if (ok && at != total) ok = false;
        if (!ok) { n_malformed++; continue; }
        n_merged++;
        // the coordinate case of the same entry point is the old entry point; any other order is refused
        std::vector<uint8_t> o1(out.size()), o2(out.size());
        std::vector<uint32_t> p1((size_t)cap, 0u), p2((size_t)cap, 0u);
        int64_t n1 = -1, n2 = -1;
        const int rc1 = svx_bam_merge_host_order(sp.data(), ss.data(), n_ref.data(), (int64_t)k, n_ref_merged, flat.empty() ? nullptr : flat.data(), SVX_SORT_COORDINATE, o1.data(), p1.data(), cap, &n1);
        const int rc2 = svx_bam_merge_host(sp.data(), ss.data(), n_ref.data(), (int64_t)k, n_ref_merged, flat.empty() ? nullptr : flat.data(), o2.data(), p2.data(), cap, &n2);
        if (rc1 != rc2 || n1 != n2 || (rc1 == SVX_OK && (memcmp(o1.data(), o2.data(), total) != 0 || p1 != p2))) n_malformed++;
        if (svx_bam_merge_host_order(sp.data(), ss.data(), n_ref.data(), (int64_t)k, n_ref_merged, flat.empty() ? nullptr : flat.data(), 2, nullptr, nullptr, 0, &n1) != SVX_E_ARG) n_malformed++;
    }
    const long n_words = table_checks(&n_table_wrong);
    printf("%ld streams: %ld merged, %ld bad argument, %ld bad range, %ld malformed; %ld with a bad name, %ld cut short, %ld with both kinds of refusal, %ld translated files; "
           "%ld table words, %ld wrong\n", n_streams, n_merged, n_arg, n_range, n_malformed, n_bad_names, n_cut, n_both, n_translated, n_words, n_table_wrong);
    return n_malformed || n_table_wrong ? 1 : 0;
}
