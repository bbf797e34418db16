// bam_merge_host_test.cpp - svx_bam_merge_header_host and svx_bam_merge_host (svim_amd/csrc/bamsort_host.cpp) under a seeded fuzz, against a plain
// reimplementation of the rule of svim_amd/bammerge.py that shares no code with them (tuples and std::map here, the packed key and bsort_translate there):
// dictionaries drawn from a small pool of names (now and then a name twice, or with another length), header texts put together from @HD, @SQ, @RG, @PG and @CO
// lines that collide on purpose (with empty lines, NUL tails and last lines without a newline), record streams with ids all over each file's dictionary, mate
// ids in and out of range, positions below -1, records cut short.  Every call must give the plain build's bytes, maps and permutation, or its refusal.
// Built with the sanitizers by tests/test_bam_merge.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I svim_amd/csrc tools/bam_merge_host_test.cpp svim_amd/csrc/bamsort_host.cpp -o bam_merge_host_test
//   ./bam_merge_host_test fuzz <seed> <merges>
#include "../include/svx.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

static uint64_t g_x = 1;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void w32(uint8_t* p, uint32_t x) { for (int k = 0; k < 4; k++) p[k] = (uint8_t)(x >> (8 * k)); }

typedef std::vector<std::pair<std::string, int32_t>> Dict;
struct Input { std::string text; uint32_t pad = 0; Dict dict; std::vector<uint8_t> stream; };

static std::vector<uint8_t> header_bytes(const std::string& text, uint32_t pad, const Dict& d) {
    std::vector<uint8_t> h = {'B', 'A', 'M', 1};
    put32(h, (uint32_t)text.size() + pad);
    h.insert(h.end(), text.begin(), text.end());
    for (uint32_t k = 0; k < pad; k++) h.push_back(k ? (uint8_t)('a' + k % 7) : 0);            // (what lies behind the first NUL is not text)
    put32(h, (uint32_t)d.size());
    for (const auto& r : d) { put32(h, (uint32_t)r.first.size() + 1); h.insert(h.end(), r.first.begin(), r.first.end()); h.push_back(0); put32(h, (uint32_t)r.second); }
    return h;
}
static std::vector<std::string> cut(const std::string& s, char sep, bool keep_empty) {
    std::vector<std::string> out; std::string cur;
    for (char c : s) { if (c == sep) { if (keep_empty || !cur.empty()) out.push_back(cur); cur.clear(); } else cur += c; }
    if (keep_empty || !cur.empty()) out.push_back(cur);
    return out;
}
static bool begins(const std::string& s, const std::string& t) { return s.size() >= t.size() && std::equal(t.begin(), t.end(), s.begin()); }
static std::string glue(const std::vector<std::string>& f) { std::string s; for (size_t i = 0; i < f.size(); i++) s += (i ? "\t" : "") + f[i]; return s; }

// the rule, plainly: -3 for what it refuses
static int plain_header(const std::vector<Input>& in, std::string* text, Dict* merged, std::vector<std::vector<int32_t>>* maps) {
    std::map<std::string, int32_t> place;
    for (const Input& x : in) {
        std::set<std::string> own; std::vector<int32_t> m;
        for (const auto& r : x.dict) {
            if (!own.insert(r.first).second) return -3;
            auto it = place.find(r.first);
            if (it == place.end()) { it = place.insert({r.first, (int32_t)merged->size()}).first; merged->push_back(r); }
            else if ((*merged)[(size_t)it->second].second != r.second) return -3;
            m.push_back(it->second);
        }
        maps->push_back(m);
    }
    std::vector<std::vector<std::string>> lines;
    for (const Input& x : in) lines.push_back(cut(x.text, '\n', false));
    std::vector<std::string> out; std::set<std::string> seen;
    std::string hd = "@HD\tVN:1.6\tSO:coordinate";
    if (begins(in[0].text, "@HD\t")) {
        std::vector<std::string> f = cut(cut(in[0].text, '\n', true)[0], '\t', true), g;
        bool so = false;
        for (size_t i = 0; i < f.size(); i++) {
            if (i && (begins(f[i], "GO:") || begins(f[i], "SS:"))) continue;
            if (i && begins(f[i], "SO:")) { g.push_back("SO:coordinate"); so = true; } else g.push_back(f[i]);
        }
        if (!so) g.push_back("SO:coordinate");
        hd = glue(g);
    }
    out.push_back(hd); seen.insert(hd);
    bool any_sq = false;
    for (const auto& ls : lines) for (const auto& l : ls) if (begins(l, "@SQ\t")) any_sq = true;
    if (any_sq)
        for (const auto& r : *merged) {
            std::string line = "@SQ\tSN:" + r.first + "\tLN:" + std::to_string(r.second);
            bool found = false;
            for (const auto& ls : lines) { for (const auto& l : ls) { if (found || !begins(l, "@SQ\t")) continue; const auto f = cut(l, '\t', true); for (size_t i = 1; i < f.size(); i++) if (f[i] == "SN:" + r.first) { line = l; found = true; break; } } }
            out.push_back(line); seen.insert(line);
        }
    std::set<std::string> rg, pg;
    for (size_t k = 0; k < in.size(); k++) {
        std::map<std::string, std::string> renamed;
        for (size_t j = 0; j < lines[k].size(); j++) {
            std::string l = lines[k][j];
            if (begins(l, "@SQ\t") || (j == 0 && begins(in[k].text, "@HD\t"))) continue;
            std::vector<std::string> f = cut(l, '\t', true);
            if (f[0] == "@PG") { for (size_t i = 1; i < f.size(); i++) if (begins(f[i], "PP:") && renamed.count(f[i].substr(3))) f[i] = "PP:" + renamed[f[i].substr(3)]; l = glue(f); }
            if (seen.count(l)) continue;
            size_t id_at = 0;
            for (size_t i = 1; i < f.size() && !id_at; i++) if (begins(f[i], "ID:")) id_at = i;
            if (f[0] == "@RG" && id_at) { if (!rg.insert(f[id_at].substr(3)).second) return -3; }
            if (f[0] == "@PG" && id_at) {
                std::string id = f[id_at].substr(3);
                if (k >= 1 && pg.count(id)) {
                    std::string nid = id;
                    do nid += "-" + std::to_string(k); while (pg.count(nid));
                    renamed[id] = nid; f[id_at] = "ID:" + nid; l = glue(f); id = nid;
                }
                pg.insert(id);
            }
            out.push_back(l); seen.insert(l);
        }
    }
    for (const auto& l : out) *text += l + "\n";
    return 0;
}

// the records, plainly: ordering tuples, stable
static int plain_merge(const std::vector<Input>& in, const std::vector<std::vector<int32_t>>& maps, std::vector<uint8_t>* out, std::vector<uint32_t>* perm) {
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> keys;      // (uint32(refID), uint32(pos + 1), flag & 16, global number)
    std::vector<std::vector<uint8_t>> recs;
    bool bad_arg = false, bad_range = false;
    for (size_t f = 0; f < in.size(); f++) {
        const std::vector<uint8_t>& s = in[f].stream;
        const int32_t n_ref = (int32_t)in[f].dict.size();
        bool identity = true;
        for (int32_t i = 0; i < n_ref; i++) identity = identity && maps[f][(size_t)i] == i;
        for (size_t p = 0; p < s.size();) {
            if (s.size() - p < 4) return -3;
            const uint32_t bs = rd32(s.data() + p);
            if (bs < 32 || bs > s.size() - p - 4) return -3;
            std::vector<uint8_t> r(s.begin() + (long)p, s.begin() + (long)(p + 4 + bs));
            int32_t tid = (int32_t)rd32(r.data() + 4), mate = (int32_t)rd32(r.data() + 24);
            const int32_t pos = (int32_t)rd32(r.data() + 8);
            if (tid < -1 || tid >= n_ref) { bad_arg = true; tid = -1; }
            if (pos < -1) bad_range = true;
            if (!identity) {
                if (mate < -1 || mate >= n_ref) { bad_arg = true; mate = -1; }
                if (tid >= 0) tid = maps[f][(size_t)tid];
                if (mate >= 0) mate = maps[f][(size_t)mate];
                w32(r.data() + 4, (uint32_t)tid); w32(r.data() + 24, (uint32_t)mate);
            }
            keys.push_back(std::make_tuple((uint32_t)tid, (uint32_t)(pos + 1), (rd32(r.data() + 16) >> 16) & 16u, (uint32_t)recs.size()));
            recs.push_back(r);
            p += 4 + bs;
        }
    }
    if (bad_arg) return -3;
    if (bad_range) return -10;
    std::sort(keys.begin(), keys.end());                                       // (the global number is the last component: stable by construction)
    for (const auto& k : keys) { const auto& r = recs[std::get<3>(k)]; out->insert(out->end(), r.begin(), r.end()); perm->push_back(std::get<3>(k)); }
    return 0;
}

static const char* NAMES[] = {"c0", "c1", "chrX", "c", "c10", "scaffold_7", "M", "c1_alt"};
static const char* PG_IDS[] = {"x", "y", "x-1", "bwa", "x-1-1", "x-2"};

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz <seed> <merges>\n", argv[0]); return 2; }
    g_x = (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull;
    const long n_merges = atol(argv[3]);
    long n_equal = 0, n_refused = 0, n_headers = 0, n_header_refused = 0, n_different = 0;
    for (long it = 0; it < n_merges; it++) {
        const uint32_t k = 1 + below(below(3) ? 3 : 6);
        std::vector<Input> in(k);
        for (uint32_t f = 0; f < k; f++) {
            Input& x = in[f];
            const uint32_t n_ref = below(7);
            std::vector<int> pool = {0, 1, 2, 3, 4, 5, 6, 7};
            for (uint32_t i = 0; i < n_ref; i++) {
                const uint32_t j = i + below(8 - i);
                std::swap(pool[i], pool[j]);
                const int name = below(60) == 0 && i ? pool[0] : pool[i];                           // now and then a name twice
                x.dict.push_back({NAMES[name], (int32_t)(1000 * (name + 1) + (below(80) == 0 ? 1 : 0))});      // now and then another length
            }
            if (below(6)) {
                const uint32_t hd = below(5);
                if (hd == 1) x.text += "@HD\tVN:1.6\tSO:unsorted\tGO:query\n"; else if (hd == 2) x.text += "@HD\tVN:1.5\n"; else if (hd == 3) x.text += "@HD\tVN:1.6\tSS:x\tSO:queryname\tXX:1\n";
                const bool sq_first = below(3) != 0, sq = below(4) != 0;
                std::string sqs, rest;
                if (sq) for (const auto& r : x.dict) if (below(8)) sqs += "@SQ\tSN:" + r.first + "\tLN:" + std::to_string(r.second) + (below(3) ? "" : "\tM5:" + std::to_string(f)) + "\n";
                const uint32_t n_lines = below(7);
                for (uint32_t l = 0; l < n_lines; l++) {
                    const uint32_t what = below(6);
                    if (what == 0) rest += "@RG\tID:rg" + std::to_string(below(3)) + "\tSM:s" + std::to_string(below(12) ? 0 : f) + "\n";
                    else if (what <= 3) {
                        rest += std::string("@PG\tID:") + PG_IDS[below(6)] + (below(2) ? std::string("\tPP:") + PG_IDS[below(6)] : std::string()) + "\tCL:run " + std::to_string(below(3) ? f : 0) + "\n";
                    } else if (what == 4) rest += "@CO\tcomment " + std::to_string(below(4)) + "\n";
                    else rest += "\n";
                }
                x.text += sq_first ? sqs + rest : rest + sqs;
                if (below(5) == 0 && !x.text.empty()) x.text.pop_back();                             // a last line without its newline
                if (below(4) == 0) x.pad = 1 + below(9);
            }
            // the records: ids over the file's own dictionary
            const uint32_t n = below(4) ? below(120) : 0;
            const int bad = below(5) == 0 ? (int)below(5) : -1;                                      // what is wrong with one record of this file, if anything
            const uint32_t bad_at = below(n);
            for (uint32_t r = 0; r < n; r++) {
                int32_t tid = n_ref && below(8) ? (int32_t)below(n_ref) : -1, mate = n_ref && below(2) ? (int32_t)below(n_ref) : -1, pos = (int32_t)below(40) - 1;
                if (r == bad_at) { if (bad == 0) tid = (int32_t)n_ref; else if (bad == 1) mate = (int32_t)n_ref + (int32_t)below(3); else if (bad == 2) mate = -2 - (int32_t)below(5); else if (bad == 3) pos = -2; }
                const uint32_t extra = below(40);
                put32(x.stream, 32u + extra);
                put32(x.stream, (uint32_t)tid); put32(x.stream, (uint32_t)pos); put32(x.stream, 0x00001401u); put32(x.stream, (below(2) ? 16u : 0u) << 16);
                put32(x.stream, r); put32(x.stream, (uint32_t)mate); put32(x.stream, 0xffffffffu); put32(x.stream, 0u);
                for (uint32_t b = 0; b < extra; b++) x.stream.push_back((uint8_t)(r + b + f));
            }
            if (bad == 4 && x.stream.size() > 1) x.stream.resize(x.stream.size() - 1 - below((uint32_t)std::min<size_t>(x.stream.size() - 1, 30)));
        }
        // ---- the header ----
        std::vector<std::vector<uint8_t>> hb;
        for (const Input& x : in) hb.push_back(header_bytes(x.text, x.pad, x.dict));
        std::vector<const uint8_t*> hp; std::vector<int64_t> hs; size_t n_map = 0;
        for (size_t f = 0; f < hb.size(); f++) { hp.push_back(hb[f].data()); hs.push_back((int64_t)hb[f].size()); n_map += in[f].dict.size(); }
        std::vector<int32_t> got_maps(n_map + 1, -7);
        int64_t n_out = -1;
        int rc = svx_bam_merge_header_host(hp.data(), hs.data(), (int64_t)k, nullptr, 0, &n_out, nullptr);
        std::vector<uint8_t> got_header((size_t)(n_out > 0 ? n_out : 1));
        if (rc == SVX_E_CAPACITY) rc = svx_bam_merge_header_host(hp.data(), hs.data(), (int64_t)k, got_header.data(), n_out, &n_out, got_maps.data());
        std::string text; Dict merged; std::vector<std::vector<int32_t>> maps;
        int want_rc;
        std::vector<uint8_t> want_header;
        if (k == 1) {                                                                                // one file: the sort's own header
            want_header.resize(hb[0].size() + 64);
            int64_t n1 = 0;
            want_rc = svx_bam_sort_header_host(hb[0].data(), (int64_t)hb[0].size(), want_header.data(), (int64_t)want_header.size(), &n1);
            want_header.resize((size_t)n1);
            merged = in[0].dict; maps.push_back({});
            for (size_t i = 0; i < merged.size(); i++) maps[0].push_back((int32_t)i);
        } else {
            want_rc = plain_header(in, &text, &merged, &maps);
            if (want_rc == 0) want_header = header_bytes(text, 0, merged);
        }
        if (want_rc != 0) { if (rc == want_rc) n_header_refused++; else { n_different++; fprintf(stderr, "merge %ld: header status %d, expected %d\n", it, rc, want_rc); } continue; }
        std::vector<int32_t> flat;
        for (const auto& m : maps) flat.insert(flat.end(), m.begin(), m.end());
        if (rc != SVX_OK || (size_t)n_out != want_header.size() || memcmp(got_header.data(), want_header.data(), want_header.size()) != 0 ||
            !std::equal(flat.begin(), flat.end(), got_maps.begin()) || got_maps[n_map] != -7) {
            n_different++; fprintf(stderr, "merge %ld: the header or the maps differ (status %d)\n", it, rc);
            continue;
        }
        n_headers++;
        // ---- the records ----
        std::vector<const uint8_t*> sp; std::vector<int64_t> ss; std::vector<int32_t> nr; size_t total = 0;
        for (const Input& x : in) { sp.push_back(x.stream.data()); ss.push_back((int64_t)x.stream.size()); nr.push_back((int32_t)x.dict.size()); total += x.stream.size(); }
        std::vector<uint8_t> want, got(total + 1, 0xAB);
        std::vector<uint32_t> want_perm, got_perm(total / 36 + 2, 0xABABABABu);
        const int want_m = plain_merge(in, maps, &want, &want_perm);
        int64_t n_rec = -1;
        const int rc_m = svx_bam_merge_host(sp.data(), ss.data(), nr.data(), (int64_t)k, (int32_t)merged.size(), flat.empty() ? nullptr : flat.data(), got.data(), got_perm.data(),
                                            (int64_t)(total / 36 + 1), &n_rec);
        if (want_m != 0) { if (rc_m == want_m) n_refused++; else { n_different++; fprintf(stderr, "merge %ld: status %d, expected %d\n", it, rc_m, want_m); } continue; }
        if (rc_m != SVX_OK || n_rec != (int64_t)want_perm.size() || want.size() != total || (total && memcmp(got.data(), want.data(), total) != 0) || got[total] != 0xAB ||
            !std::equal(want_perm.begin(), want_perm.end(), got_perm.begin()) || got_perm[want_perm.size()] != 0xABABABABu) {
            n_different++; fprintf(stderr, "merge %ld: the stream or the permutation differ (status %d)\n", it, rc_m);
            continue;
        }
        n_equal++;
    }
    printf("%ld merges: %ld equal, %ld refused, %ld headers, %ld headers refused, %ld different\n", n_merges, n_equal, n_refused, n_headers, n_header_refused, n_different);
    return n_different ? 1 : 0;
}
