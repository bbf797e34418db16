// bamsort_host.cpp - svx_bam_sort_host_order and svx_bam_sort_header_host_order (svx_bam_sort_host and svx_bam_sort_header_host are their coordinate case): the
// sort of a record stream in coordinate or query-name order and the header of the sorted file by the rule of bamsort_core.hpp and svim_amd/bamsort.py, built
// for the host; no GPU involved.  The kernels of bamsort.hip write the same bytes and the same permutation:
// there the keys go through the radix sort and the records through a gather, here through std::stable_sort and memcpy.
// svx_bam_merge_header_host_order and svx_bam_merge_host_order (svx_bam_merge_header_host and svx_bam_merge_host are their coordinate case): the same for
// several files merged into one (svim_amd/bammerge.py; bsort_translate).
#include "bamsort_core.hpp"
#include "../../include/svx.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

static inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// order SVX_SORT_QUERYNAME: a row's key is the name's rank, and the name lies at records + at + BSORT_NAME_AT, name_len bytes long (bamsort_core.hpp); names
// compare as unsigned bytes (memcmp), a proper prefix first, then the rank; equal keys keep file order (the sort is stable)
extern "C" int svx_bam_sort_host_order(const uint8_t* records, int64_t n_bytes, int32_t n_ref, int which, uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records) {
    if (n_bytes < 0 || n_ref < 0 || perm_cap < 0 || (n_bytes && !records) || !n_records || (which != SVX_SORT_COORDINATE && which != SVX_SORT_QUERYNAME)) return SVX_E_ARG;
    *n_records = 0;
    const bool by_name = which == SVX_SORT_QUERYNAME;
    struct Row { uint64_t key; int64_t at; uint32_t len, name_len; };
    std::vector<Row> rows;
    int bad = 0;
    for (int64_t p = 0; p < n_bytes;) {
        if (n_bytes - p < 4) return SVX_E_ARG;
        const uint32_t bs = rd32(records + p);
        if (bs < BSORT_MIN_BLOCK_SIZE || (int64_t)bs > n_bytes - p - 4) return SVX_E_ARG;          // (nothing behind a record that cannot be walked is a record)
        const int32_t tid = (int32_t)rd32(records + p + 4), pos = (int32_t)rd32(records + p + 8);
        const uint32_t flag = rd32(records + p + 16) >> 16;
        bad |= bsort_check(tid, pos, bs, n_ref);
        if (by_name) {
            const uint32_t l_name = records[p + BSORT_LNAME_AT];
            const int b = bsort_name_check(l_name, bs);
            bad |= b;
            rows.push_back(Row{bsort_name_rank(flag), p, 4u + bs, b ? 0u : bsort_name_len(records + p + BSORT_NAME_AT, l_name)});
        } else rows.push_back(Row{bsort_key(tid, pos, flag, n_ref), p, 4u + bs, 0u});
        p += 4 + (int64_t)bs;
    }
    if (bad) return bsort_status(bad);
    if (rows.size() > 0xffffffffull) return SVX_E_CAPACITY;
    *n_records = (int64_t)rows.size();
    if (perm && (int64_t)rows.size() > perm_cap) return SVX_E_CAPACITY;
    std::vector<uint32_t> order(rows.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = (uint32_t)k;
    if (by_name)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const Row &x = rows[a], &y = rows[b];
            const int c = memcmp(records + x.at + BSORT_NAME_AT, records + y.at + BSORT_NAME_AT, std::min(x.name_len, y.name_len));
            if (c != 0) return c < 0;
            if (x.name_len != y.name_len) return x.name_len < y.name_len;
            return x.key < y.key;
        });
    else std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[a].key < rows[b].key; });
    int64_t at = 0;
    for (size_t k = 0; k < order.size(); k++) {
        const Row& r = rows[order[k]];
        if (out) memcpy(out + at, records + r.at, r.len);
        if (perm) perm[k] = order[k];
        at += r.len;
    }
    return SVX_OK;
}
extern "C" int svx_bam_sort_host(const uint8_t* records, int64_t n_bytes, int32_t n_ref, uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records) {
    return svx_bam_sort_host_order(records, n_bytes, n_ref, SVX_SORT_COORDINATE, out, perm, perm_cap, n_records);
}

// The spilled sort as bamsort.hip does it, on the host: every run sorted stably and written to a run file, one stable sort over the run-sorted keys (ties: run,
// then place in the run), and the stream written piece by piece, every piece from one contiguous byte range per run (bamsort_core.hpp: bsort_piece_cut) read
// back into a staging buffer.  The stream has no header here: segment j is the record at global position j.
extern "C" int svx_bam_sort_spill_host(const uint8_t* records, int64_t n_bytes, int32_t n_ref, const int64_t* run_ends, int64_t n_runs, int64_t piece_blocks, uint8_t* out,
                                       uint32_t* perm, int64_t perm_cap, int64_t* n_records, svx_spill_write_fn write_fn, svx_spill_read_fn read_fn, void* user) {
    if (n_bytes < 0 || n_ref < 0 || perm_cap < 0 || (n_bytes && !records) || !n_records || n_runs < 0 || (n_runs && !run_ends) || piece_blocks < 1 || (!write_fn) != (!read_fn)) return SVX_E_ARG;
    *n_records = 0;
    struct Row { uint64_t key; int64_t at; uint32_t len; };
    std::vector<Row> rows;
    int bad = 0;
    for (int64_t p = 0; p < n_bytes;) {
        if (n_bytes - p < 4) return SVX_E_ARG;
        const uint32_t bs = rd32(records + p);
        if (bs < BSORT_MIN_BLOCK_SIZE || (int64_t)bs > n_bytes - p - 4) return SVX_E_ARG;
        const int32_t tid = (int32_t)rd32(records + p + 4), pos = (int32_t)rd32(records + p + 8);
        const uint32_t flag = rd32(records + p + 16) >> 16;
        bad |= bsort_check(tid, pos, bs, n_ref);
        rows.push_back(Row{bsort_key(tid, pos, flag, n_ref), p, 4u + bs});
        p += 4 + (int64_t)bs;
    }
    if (bad) return bsort_status(bad);
    if (rows.size() > 0xffffffffull) return SVX_E_CAPACITY;
    const int64_t n = (int64_t)rows.size();
    *n_records = n;
    if (perm && n > perm_cap) return SVX_E_CAPACITY;
    for (int64_t r = 0; r < n_runs; r++)
        if (run_ends[r] < (r ? run_ends[r - 1] : 0) || run_ends[r] > n) return SVX_E_ARG;
    if ((n_runs ? run_ends[n_runs - 1] : 0) != n) return SVX_E_ARG;
    // run formation: per place q of the concatenation of the runs its key, length, file index and offset in its run's stream; the streams go to the run file
    std::vector<uint8_t> memory_file;
    std::vector<int64_t> run_base((size_t)n_runs + 1, n), run_bytes((size_t)n_runs, 0), run_at((size_t)n_runs, 0), roff((size_t)n + 1, 0);
    std::vector<uint64_t> rkey((size_t)n);
    std::vector<uint32_t> rlen((size_t)n), rfile((size_t)n), order;
    std::vector<uint8_t> buf;
    int64_t file_bytes = 0;
    for (int64_t r = 0; r < n_runs; r++) {
        const int64_t first = r ? run_ends[r - 1] : 0, m = run_ends[r] - first;
        run_base[(size_t)r] = first; run_at[(size_t)r] = file_bytes;
        order.resize((size_t)m);
        for (int64_t k = 0; k < m; k++) order[(size_t)k] = (uint32_t)k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[(size_t)(first + a)].key < rows[(size_t)(first + b)].key; });
        int64_t total = 0;
        for (int64_t k = 0; k < m; k++) total += rows[(size_t)(first + order[(size_t)k])].len;
        buf.resize((size_t)total);
        int64_t at = 0;
        for (int64_t k = 0; k < m; k++) {
            const Row& w = rows[(size_t)(first + order[(size_t)k])];
            rkey[(size_t)(first + k)] = w.key; rlen[(size_t)(first + k)] = w.len; rfile[(size_t)(first + k)] = (uint32_t)(first + order[(size_t)k]); roff[(size_t)(first + k)] = at;
            memcpy(buf.data() + at, records + w.at, w.len);
            at += w.len;
        }
        run_bytes[(size_t)r] = total;
        if (write_fn) { if (total && write_fn(user, file_bytes, buf.data(), total) != total) return SVX_E_IO; }
        else memory_file.insert(memory_file.end(), buf.begin(), buf.end());
        file_bytes += total;
    }
    // the merge: places sorted stably by key; gpos the inverse
    std::vector<uint32_t> gp((size_t)n), gpos((size_t)n), srun((size_t)n);
    for (int64_t q = 0; q < n; q++) gp[(size_t)q] = (uint32_t)q;
    std::stable_sort(gp.begin(), gp.end(), [&](uint32_t a, uint32_t b) { return rkey[a] < rkey[b]; });
    std::vector<int64_t> soff((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; j++) {
        const uint32_t q = gp[(size_t)j];
        gpos[q] = (uint32_t)j; srun[(size_t)j] = (uint32_t)bsort_run_of(run_base.data(), n_runs, (int64_t)q);
        soff[(size_t)j + 1] = soff[(size_t)j] + rlen[q];
        if (perm) perm[j] = rfile[q];
    }
    if (!out) return SVX_OK;
    // the pieces
    const int64_t total = soff[(size_t)n], step = std::min<int64_t>(piece_blocks, total / BSORT_BLOCK + 1) * BSORT_BLOCK;
    std::vector<uint8_t> stage;
    std::vector<int64_t> stage_at((size_t)n_runs), cut0((size_t)n_runs);
    for (int64_t lo = 0; lo < total; lo += step) {
        const int64_t hi = lo + step < total ? lo + step : total;
        // the segments that hold bytes lo and hi - 1: the largest j with soff[j] <= x
        const int64_t j0 = (std::upper_bound(soff.begin(), soff.begin() + n, lo) - soff.begin()) - 1, j1 = (std::upper_bound(soff.begin(), soff.begin() + n, hi - 1) - soff.begin()) - 1;
        int64_t at = 0;
        for (int64_t r = 0; r < n_runs; r++) {
            const int64_t base = run_base[(size_t)r], cnt = run_base[(size_t)r + 1] - base;
            int64_t a, b;
            bsort_piece_cut(gpos.data() + base, cnt, j0, j1 + 1, &a, &b);
            const int64_t c0 = a < cnt ? roff[(size_t)(base + a)] : run_bytes[(size_t)r], c1 = b < cnt ? roff[(size_t)(base + b)] : run_bytes[(size_t)r];
            stage_at[(size_t)r] = at; cut0[(size_t)r] = c0;
            if (c1 <= c0) continue;
            stage.resize((size_t)(at + c1 - c0));
            if (read_fn) { if (read_fn(user, run_at[(size_t)r] + c0, stage.data() + at, c1 - c0) != c1 - c0) return SVX_E_IO; }
            else memcpy(stage.data() + at, memory_file.data() + run_at[(size_t)r] + c0, (size_t)(c1 - c0));
            at += c1 - c0;
        }
        for (int64_t j = j0; j <= j1; j++) {                                  // the bytes of segment j inside [lo, hi)
            const uint32_t q = gp[(size_t)j], r = srun[(size_t)j];
            const int64_t s0 = std::max<int64_t>(soff[(size_t)j], lo), s1 = std::min<int64_t>(soff[(size_t)j + 1], hi);
            const int64_t src = stage_at[r] + (roff[q] - cut0[r]) + (s0 - soff[(size_t)j]);
            if (src < 0 || src + (s1 - s0) > at) return SVX_E_STATE;           // (a cut that does not cover its records: internal error)
            memcpy(out + s0, stage.data() + src, (size_t)(s1 - s0));
        }
    }
    return SVX_OK;
}

// header: magic, l_text, text, n_ref, the reference dictionary (the inflated file up to its first record)
// order SVX_SORT_QUERYNAME: SO:queryname, and SS:queryname:lexicographical behind the first SO: field (every other SS: field goes, as in coordinate order)
extern "C" int svx_bam_sort_header_host_order(const uint8_t* header, int64_t n_bytes, int order, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (!header || n_bytes < 12 || cap < 0 || (cap && !out) || !n_out || memcmp(header, "BAM\1", 4) != 0 || (order != SVX_SORT_COORDINATE && order != SVX_SORT_QUERYNAME)) return SVX_E_ARG;
    const bool by_name = order == SVX_SORT_QUERYNAME;
    const std::string so = by_name ? "SO:queryname" : "SO:coordinate", ss = by_name ? "\tSS:queryname:lexicographical" : "";
    *n_out = 0;
    const uint32_t l_text = rd32(header + 4);
    if ((int64_t)l_text > n_bytes - 12) return SVX_E_ARG;
    std::string text((const char*)header + 8, l_text);
    const size_t nul = text.find('\0');
    if (nul != std::string::npos) text.resize(nul);
    if (text.compare(0, 4, "@HD\t") == 0) {
        const size_t eol = text.find('\n');
        const std::string line = text.substr(0, eol), tail = eol == std::string::npos ? std::string() : text.substr(eol);
        std::string made = "@HD";
        bool seen = false;
        for (size_t a = 4; a <= line.size();) {                                  // the fields behind "@HD\t" (an empty one between two tabs is a field)
            size_t b = line.find('\t', a);
            if (b == std::string::npos) b = line.size();
            const std::string f = line.substr(a, b - a);
            if (f.compare(0, 3, "GO:") != 0 && f.compare(0, 3, "SS:") != 0) {
                made += '\t';
                if (f.compare(0, 3, "SO:") == 0) { made += so; if (!seen) made += ss; seen = true; } else made += f;
            }
            a = b + 1;
        }
        if (!seen) made += "\t" + so + ss;
        text = made + tail;
    } else text = "@HD\tVN:1.6\t" + so + ss + "\n" + text;
    const int64_t rest = n_bytes - 8 - (int64_t)l_text, total = 8 + (int64_t)text.size() + rest;
    *n_out = total;
    if (total > cap) return SVX_E_CAPACITY;
    memcpy(out, "BAM\1", 4);
    wr32(out + 4, (uint32_t)text.size());
    memcpy(out + 8, text.data(), text.size());
    memcpy(out + 8 + text.size(), header + 8 + l_text, (size_t)rest);
    return SVX_OK;
}
extern "C" int svx_bam_sort_header_host(const uint8_t* header, int64_t n_bytes, uint8_t* out, int64_t cap, int64_t* n_out) {
    return svx_bam_sort_header_host_order(header, n_bytes, SVX_SORT_COORDINATE, out, cap, n_out);
}

// ---- the merge of several files (svim_amd/bammerge.py) ------------------------------------------------------------------------------------------------------
namespace {
struct MergeHeader { std::string text; std::vector<std::string> names; std::vector<int32_t> lens; };
// header bytes (magic .. dictionary) -> the text up to its first NUL and the dictionary; false: it cannot be walked
bool merge_parse(const uint8_t* h, int64_t n, MergeHeader* o) {
    if (!h || n < 12 || memcmp(h, "BAM\1", 4) != 0) return false;
    const int64_t l_text = (int32_t)rd32(h + 4);
    if (l_text < 0 || l_text > n - 12) return false;
    o->text.assign((const char*)h + 8, (size_t)l_text);
    const size_t nul = o->text.find('\0');
    if (nul != std::string::npos) o->text.resize(nul);
    int64_t p = 8 + l_text;
    const int64_t n_ref = (int32_t)rd32(h + p);
    p += 4;
    if (n_ref < 0) return false;
    for (int64_t i = 0; i < n_ref; i++) {
        if (n - p < 8) return false;
        const int64_t l_name = (int32_t)rd32(h + p);
        if (l_name < 0 || l_name > n - p - 8) return false;
        std::string name((const char*)h + p + 4, (size_t)l_name);
        const size_t z = name.find('\0');
        if (z != std::string::npos) name.resize(z);
        o->names.push_back(name); o->lens.push_back((int32_t)rd32(h + p + 4 + l_name));
        p += 8 + l_name;
    }
    return true;
}
std::vector<std::string> merge_split(const std::string& s, char sep, bool keep_empty) {
    std::vector<std::string> out;
    for (size_t a = 0; a <= s.size();) {
        size_t b = s.find(sep, a);
        if (b == std::string::npos) b = s.size();
        if (keep_empty || b > a) out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}
bool merge_starts(const std::string& s, const char* t) { return s.compare(0, strlen(t), t) == 0; }
// the value of the first field behind the record type that starts with tag; false: none
bool merge_field(const std::string& line, const char* tag, std::string* v) {
    const std::vector<std::string> f = merge_split(line, '\t', true);
    for (size_t i = 1; i < f.size(); i++) if (merge_starts(f[i], tag)) { *v = f[i].substr(strlen(tag)); return true; }
    return false;
}
std::string merge_join(const std::vector<std::string>& f) {
    std::string s;
    for (size_t i = 0; i < f.size(); i++) { if (i) s += '\t'; s += f[i]; }
    return s;
}
bool merge_has(const std::vector<std::string>& v, const std::string& s) { return std::find(v.begin(), v.end(), s) != v.end(); }
}  // namespace

// order SVX_SORT_QUERYNAME: rule 1 takes the first line of the first file's header as query-name order rewrites it; every other rule is the same
extern "C" int svx_bam_merge_header_host_order(const uint8_t* const* headers, const int64_t* sizes, int64_t k, int order, uint8_t* out, int64_t cap, int64_t* n_out, int32_t* tid_maps_out) {
    if (!headers || !sizes || k < 1 || cap < 0 || (cap && !out) || !n_out || (order != SVX_SORT_COORDINATE && order != SVX_SORT_QUERYNAME)) return SVX_E_ARG;
    *n_out = 0;
    std::vector<MergeHeader> H((size_t)k);
    for (int64_t f = 0; f < k; f++) if (!merge_parse(headers[f], sizes[f], &H[(size_t)f])) return SVX_E_ARG;
    if (k == 1) {                                                                // the merge of one file is the sort of that file
        if (tid_maps_out) for (size_t i = 0; i < H[0].names.size(); i++) tid_maps_out[i] = (int32_t)i;
        return svx_bam_sort_header_host_order(headers[0], sizes[0], order, out, cap, n_out);
    }
    // the dictionary: the first file's, then the names not yet present; the maps
    std::vector<std::string> names; std::vector<int32_t> lens;
    size_t at = 0;
    for (int64_t f = 0; f < k; f++) {
        const MergeHeader& h = H[(size_t)f];
        for (size_t i = 0; i < h.names.size(); i++) {
            for (size_t j = 0; j < i; j++) if (h.names[j] == h.names[i]) return SVX_E_ARG;              // a name twice in one dictionary
            const size_t m = (size_t)(std::find(names.begin(), names.end(), h.names[i]) - names.begin());
            if (m == names.size()) { names.push_back(h.names[i]); lens.push_back(h.lens[i]); }
            else if (lens[m] != h.lens[i]) return SVX_E_ARG;                                            // one name, two lengths
            if (tid_maps_out) tid_maps_out[at] = (int32_t)m;
            at++;
        }
    }
    // the text: rule 1 to 5 of svim_amd/bammerge.py
    std::vector<std::vector<std::string>> lines((size_t)k);
    for (int64_t f = 0; f < k; f++) lines[(size_t)f] = merge_split(H[(size_t)f].text, '\n', false);
    std::vector<std::string> made;
    {
        std::vector<uint8_t> fake(12 + H[0].text.size(), 0), sorted(12 + H[0].text.size() + 64, 0);
        memcpy(fake.data(), "BAM\1", 4); wr32(fake.data() + 4, (uint32_t)H[0].text.size());
        if (!H[0].text.empty()) memcpy(fake.data() + 8, H[0].text.data(), H[0].text.size());
        int64_t n = 0;
        if (svx_bam_sort_header_host_order(fake.data(), (int64_t)fake.size(), order, sorted.data(), (int64_t)sorted.size(), &n) != SVX_OK) return SVX_E_ARG;
        const std::string text((const char*)sorted.data() + 8, (size_t)rd32(sorted.data() + 4));
        made.push_back(text.substr(0, text.find('\n')));
    }
    bool any_sq = false;
    for (const auto& ls : lines) for (const auto& ln : ls) any_sq = any_sq || merge_starts(ln, "@SQ\t");
    if (any_sq)
        for (size_t r = 0; r < names.size(); r++) {
            const std::string want = "SN:" + names[r];
            const std::string* hit = nullptr;
            for (size_t f = 0; f < lines.size() && !hit; f++)
                for (const auto& ln : lines[f]) {
                    if (!merge_starts(ln, "@SQ\t")) continue;
                    const std::vector<std::string> fl = merge_split(ln, '\t', true);
                    if (std::find(fl.begin() + 1, fl.end(), want) != fl.end()) { hit = &ln; break; }
                }
            made.push_back(hit ? *hit : "@SQ\tSN:" + names[r] + "\tLN:" + std::to_string(lens[r]));
        }
    std::vector<std::string> rg_ids, pg_ids;
    for (int64_t f = 0; f < k; f++) {
        std::vector<std::pair<std::string, std::string>> renamed;
        const std::string suffix = "-" + std::to_string(f);
        for (size_t j = 0; j < lines[(size_t)f].size(); j++) {
            std::string ln = lines[(size_t)f][j];
            if ((j == 0 && merge_starts(H[(size_t)f].text, "@HD\t")) || merge_starts(ln, "@SQ\t")) continue;
            const bool pg = merge_starts(ln, "@PG\t");
            if (pg && !renamed.empty()) {                                        // PP: follows the renames of this file so far
                std::vector<std::string> fl = merge_split(ln, '\t', true);
                for (auto& x : fl)
                    if (merge_starts(x, "PP:")) for (const auto& rn : renamed) if (x.compare(3, std::string::npos, rn.first) == 0) { x = "PP:" + rn.second; break; }
                ln = merge_join(fl);
            }
            if (merge_has(made, ln)) continue;
            std::string id;
            if (merge_starts(ln, "@RG\t")) {
                if (merge_field(ln, "ID:", &id)) { if (merge_has(rg_ids, id)) return SVX_E_ARG; rg_ids.push_back(id); }      // read groups are not renamed (RG:Z tags: out of scope)
            } else if (pg && merge_field(ln, "ID:", &id)) {
                if (f >= 1 && merge_has(pg_ids, id)) {
                    std::string nid = id + suffix;
                    while (merge_has(pg_ids, nid)) nid += suffix;
                    bool found = false;
                    for (auto& rn : renamed) if (rn.first == id) { rn.second = nid; found = true; }
                    if (!found) renamed.push_back({id, nid});
                    std::vector<std::string> fl = merge_split(ln, '\t', true);
                    for (size_t i = 1; i < fl.size(); i++) if (merge_starts(fl[i], "ID:")) { fl[i] = "ID:" + nid; break; }
                    ln = merge_join(fl); id = nid;
                }
                pg_ids.push_back(id);
            }
            made.push_back(ln);
        }
    }
    std::string text;
    for (const auto& ln : made) { text += ln; text += '\n'; }
    int64_t total = 12 + (int64_t)text.size();
    for (const auto& nm : names) total += 9 + (int64_t)nm.size();
    *n_out = total;
    if (total > cap) return SVX_E_CAPACITY;
    uint8_t* p = out;
    memcpy(p, "BAM\1", 4); wr32(p + 4, (uint32_t)text.size()); memcpy(p + 8, text.data(), text.size());
    p += 8 + text.size();
    wr32(p, (uint32_t)names.size()); p += 4;
    for (size_t r = 0; r < names.size(); r++) {
        wr32(p, (uint32_t)names[r].size() + 1); memcpy(p + 4, names[r].c_str(), names[r].size() + 1);
        wr32(p + 5 + names[r].size(), (uint32_t)lens[r]);
        p += 9 + names[r].size();
    }
    return SVX_OK;
}

extern "C" int svx_bam_merge_header_host(const uint8_t* const* headers, const int64_t* sizes, int64_t k, uint8_t* out, int64_t cap, int64_t* n_out, int32_t* tid_maps_out) {
    return svx_bam_merge_header_host_order(headers, sizes, k, SVX_SORT_COORDINATE, out, cap, n_out, tid_maps_out);
}

// order SVX_SORT_QUERYNAME: a row's key is the rank and the name lies in the translated copy (svx_bam_sort_host_order's comparison); the names' refusals are per file
extern "C" int svx_bam_merge_host_order(const uint8_t* const* streams, const int64_t* sizes, const int32_t* n_ref, int64_t k, int32_t n_ref_merged, const int32_t* tid_maps, int order,
                                        uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records) {
    if (!streams || !sizes || !n_ref || k < 1 || n_ref_merged < 0 || perm_cap < 0 || !n_records || (order != SVX_SORT_COORDINATE && order != SVX_SORT_QUERYNAME)) return SVX_E_ARG;
    *n_records = 0;
    const bool by_name = order == SVX_SORT_QUERYNAME;
    struct Row { uint64_t key; int64_t at; uint32_t len, name_len; };
    std::vector<Row> rows;
    std::vector<uint8_t> all;                                                    // the concatenation of the inputs, translated
    int bad = 0;
    const int32_t* map = tid_maps;
    for (int64_t f = 0; f < k; f++) {
        const int64_t n_bytes = sizes[f];
        const uint8_t* records = streams[f];
        if (n_bytes < 0 || n_ref[f] < 0 || (n_bytes && !records) || (n_ref[f] && !map)) return SVX_E_ARG;
        bool identity = true;
        for (int32_t i = 0; i < n_ref[f]; i++) {
            if (map[i] < 0 || map[i] >= n_ref_merged) return SVX_E_ARG;
            identity = identity && map[i] == i;
        }
        const int64_t base = (int64_t)all.size();
        if (n_bytes) all.insert(all.end(), records, records + n_bytes);
        for (int64_t p = 0; p < n_bytes;) {
            if (n_bytes - p < 4) return SVX_E_ARG;
            const uint32_t bs = rd32(records + p);
            if (bs < BSORT_MIN_BLOCK_SIZE || (int64_t)bs > n_bytes - p - 4) return SVX_E_ARG;
            int32_t tid = (int32_t)rd32(records + p + BSORT_REFID_AT);
            const int32_t pos = (int32_t)rd32(records + p + 8);
            const uint32_t flag = rd32(records + p + 16) >> 16;
            if (!identity) {                                                     // the ids of this file's records go through its map, in the copy
                int32_t t, m;
                bad |= bsort_translate(tid, (int32_t)rd32(records + p + BSORT_MATE_AT), map, n_ref[f], &t, &m);
                wr32(all.data() + base + p + BSORT_REFID_AT, (uint32_t)t); wr32(all.data() + base + p + BSORT_MATE_AT, (uint32_t)m);
                tid = t;
            }
            bad |= bsort_check(tid, pos, bs, identity ? n_ref[f] : n_ref_merged);
            if (by_name) {
                const uint32_t l_name = records[p + BSORT_LNAME_AT];
                const int b = bsort_name_check(l_name, bs);
                bad |= b;
                rows.push_back(Row{bsort_name_rank(flag), base + p, 4u + bs, b ? 0u : bsort_name_len(records + p + BSORT_NAME_AT, l_name)});
            } else rows.push_back(Row{bsort_key(tid, pos, flag, n_ref_merged), base + p, 4u + bs, 0u});
            p += 4 + (int64_t)bs;
        }
        map += n_ref[f];
    }
    if (bad) return bsort_status(bad);
    if (rows.size() > 0xffffffffull) return SVX_E_CAPACITY;
    *n_records = (int64_t)rows.size();
    if (perm && (int64_t)rows.size() > perm_cap) return SVX_E_CAPACITY;
    std::vector<uint32_t> idx(rows.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)i;
    if (by_name)
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
            const Row &x = rows[a], &y = rows[b];
            const int c = memcmp(all.data() + x.at + BSORT_NAME_AT, all.data() + y.at + BSORT_NAME_AT, std::min(x.name_len, y.name_len));
            if (c != 0) return c < 0;
            if (x.name_len != y.name_len) return x.name_len < y.name_len;
            return x.key < y.key;
        });
    else std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return rows[a].key < rows[b].key; });
    int64_t at = 0;
    for (size_t i = 0; i < idx.size(); i++) {
        const Row& r = rows[idx[i]];
        if (out) memcpy(out + at, all.data() + r.at, r.len);
        if (perm) perm[i] = idx[i];
        at += r.len;
    }
    return SVX_OK;
}
extern "C" int svx_bam_merge_host(const uint8_t* const* streams, const int64_t* sizes, const int32_t* n_ref, int64_t k, int32_t n_ref_merged, const int32_t* tid_maps, uint8_t* out,
                                  uint32_t* perm, int64_t perm_cap, int64_t* n_records) {
    return svx_bam_merge_host_order(streams, sizes, n_ref, k, n_ref_merged, tid_maps, SVX_SORT_COORDINATE, out, perm, perm_cap, n_records);
}
// the name table's word against the name's own (bamsort_core.hpp), for one name packed at word_off of a table of tab_words words: what the tests hold
// bsort_name_tab_word to.  -> the number of rounds r in [0, 64) at which the two differ (0: none), or SVX_E_ARG
extern "C" int svx_bam_name_tab_check_host(const uint8_t* name, int32_t name_len, int64_t word_off, int64_t tab_words) {
    if (!name || name_len < 1 || name_len > 255 || word_off < 0 || word_off + (int64_t)bsort_name_tab_words((uint32_t)name_len) > tab_words) return SVX_E_ARG;
    std::vector<uint32_t> tab((size_t)tab_words, 0xa5a5a5a5u);
    std::vector<uint8_t> field(name, name + name_len);                          // (exactly the name: a read behind its end is a read behind the allocation)
    bsort_name_tab_pack(field.data(), (uint32_t)name_len, tab.data() + word_off);
    int wrong = 0;
    for (uint32_t r = 0; r < 64u; r++) wrong += bsort_name_tab_word(tab.data(), (uint64_t)word_off, (uint32_t)name_len, r) != bsort_name_word(field.data(), (uint32_t)name_len, r);
    for (int64_t w = 0; w < tab_words; w++)                                      // nothing outside the name's words is written
        if ((w < word_off || w >= word_off + (int64_t)bsort_name_tab_words((uint32_t)name_len)) && tab[(size_t)w] != 0xa5a5a5a5u) wrong++;
    return wrong;
}
