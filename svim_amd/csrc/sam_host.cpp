// sam_host.cpp - svx_sam_convert_host and svx_sam_header_host: SAM text -> BAM records and BAM header by the rule of sam_core.hpp and svim_amd/sam.py, built for
// the host; no GPU involved.  The kernels of sam.hip write the same bytes: there a wave walks a line, here one loop does.
#include "sam_core.hpp"
#include "sam_host.hpp"
#include "../../include/svx.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern thread_local std::string g_svx_err;

// strtod on the text of a float the fast path left alone; false: strtod does not take the whole text
bool sam_host_strtod(const uint8_t* s, uint32_t n, float* out) {
    // the grammar of svim_amd/sam.py, narrower than strtod's (which also takes leading blanks, hexadecimal floats and "nan(...)"):
    //   [+-] ( digits [ . [digits] ] | . digits ) [ (e|E) [+-] digits ]   |   [+-] ( inf | infinity | nan ), the words in either case
    uint32_t i = 0;
    if (i < n && (s[i] == '+' || s[i] == '-')) i++;
    auto word = [&](const char* w) { const uint32_t l = (uint32_t)strlen(w); if (n - i != l) return false; for (uint32_t k = 0; k < l; k++) if ((s[i + k] | 0x20) != (uint8_t)w[k]) return false; return true; };
    if (!(word("inf") || word("infinity") || word("nan"))) {
        uint32_t nd = 0;
        for (; i < n && sam_digit(s[i]); i++) nd++;
        if (i < n && s[i] == '.') for (i++; i < n && sam_digit(s[i]); i++) nd++;
        if (!nd) return false;
        if (i < n && (s[i] == 'e' || s[i] == 'E')) {
            i++;
            if (i < n && (s[i] == '+' || s[i] == '-')) i++;
            uint32_t ed = 0;
            for (; i < n && sam_digit(s[i]); i++) ed++;
            if (!ed) return false;
        }
        if (i != n) return false;
    }
    const std::string z((const char*)s, n);
    char* end = nullptr;
    const double v = strtod(z.c_str(), &end);
    if (end != z.c_str() + n) return false;
    *out = (float)v;
    return true;
}

// one line (no newline) -> the size of its record, and the record at dst when cap_left holds it (*fits).  != 0: the SAM_E_* that refuses the line
static int convert_line(const uint8_t* s, uint32_t len, const ContigTable& ct, uint64_t* n_out, uint64_t cap_left, uint8_t* dst, bool* fits) {
    if (len && s[0] == '@') return SAM_E_HEADER;
    SamDesc d;
    memset(&d, 0, sizeof d);
    d.len = len;
    uint32_t nf = 1;
    d.f[0] = 0;
    for (uint32_t i = 0; i < len && nf < 12; i++) if (s[i] == '\t') d.f[nf++] = i + 1;
    if (nf < 11) return SAM_E_FIELDS;
    if (nf == 11) d.f[11] = len + 1;
    sam_check_fields(s, d);
    if (d.err) return (int)d.err;
    // CIGAR: operations and reference length
    const uint32_t c0 = d.f[5], c1 = d.f[6] - 1;
    std::vector<uint32_t> ops;
    int64_t reflen = 0;
    if (c1 == c0) return SAM_E_CIGAR;
    if (!(c1 - c0 == 1 && s[c0] == '*')) {
        uint32_t lo = c0;
        for (uint32_t p = c0; p < c1; p++) {
            if (sam_digit(s[p])) continue;
            uint32_t w;
            if (!sam_cigar_at(s, lo, p, &w)) return SAM_E_CIGAR;
            lo = p + 1;
            ops.push_back(w);
            if (sam_op_on_ref((int)(w & 15u))) reflen += w >> 4;
        }
        if (sam_digit(s[c1 - 1])) return SAM_E_CIGAR;
    }
    d.n_ops = (uint32_t)ops.size();
    // aux: sizes
    uint32_t n_patch = 0;
    for (uint32_t a = d.f[11]; a <= len;) {
        uint32_t b = a;
        while (b < len && s[b] != '\t') b++;
        uint32_t bytes, np;
        const int e = sam_aux_size(s + a, b - a, &bytes, &np);
        if (e) return e;
        d.aux_bytes += bytes; n_patch += np;
        a = b + 1;
    }
    d.n_patch = n_patch;
    const uint64_t size = sam_record_bytes(d);
    *n_out = size;
    *fits = size <= cap_left;
    std::vector<uint8_t> scratch;
    if (!*fits) { scratch.resize((size_t)size); dst = scratch.data(); }          // a line is refused whether or not its record fits: written all the same, beside the room
    uint8_t* r = dst;
    const int e = sam_fixed(s, d, ct, reflen, r);
    if (e) return e;
    uint8_t* w = r + 36;
    const uint32_t l_name = d.f[1] - 1 - d.f[0];
    memcpy(w, s, l_name); w[l_name] = 0; w += l_name + 1;
    const bool lng = d.n_ops > SAM_MAX_BAM_OPS;
    uint8_t* placeholder = w;
    if (lng) w += 8; else { for (uint32_t k = 0; k < d.n_ops; k++) sam_w32(w + 4 * k, ops[k]); w += 4 * (size_t)d.n_ops; }
    const uint8_t* sq = s + d.f[9];
    for (uint32_t j = 0; j < (d.l_seq + 1) / 2; j++) w[j] = (uint8_t)((sam_nib(sq[2 * j]) << 4) | (2 * j + 1 < d.l_seq ? sam_nib(sq[2 * j + 1]) : 0));
    w += (d.l_seq + 1) / 2;
    const uint8_t* ql = s + d.f[10];
    const bool no_qual = d.f[11] - 1 - d.f[10] == 1 && ql[0] == '*';
    for (uint32_t j = 0; j < d.l_seq; j++) w[j] = no_qual ? 0xff : (uint8_t)(ql[j] - 33);
    w += d.l_seq;
    std::vector<SamPatch> patch(n_patch ? n_patch : 1);
    uint32_t pk = 0;
    for (uint32_t a = d.f[11]; a <= len;) {
        uint32_t b = a;
        while (b < len && s[b] != '\t') b++;
        uint32_t bytes, np;
        (void)sam_aux_size(s + a, b - a, &bytes, &np);
        sam_aux_emit(s + a, b - a, w, true, (uint64_t)(w - r), a, 0, patch.data() + pk);
        pk += np;
        w += bytes;
        a = b + 1;
    }
    for (uint32_t k = 0; k < pk; k++) {
        float f;
        if (!sam_host_strtod(s + patch[k].text_at, patch[k].text_len, &f)) return SAM_E_FLOAT;
        uint32_t u; memcpy(&u, &f, 4);
        sam_w32(r + patch[k].at, u);
    }
    if (lng) {
        sam_long_cigar_frame(d, reflen, placeholder, w);
        for (uint32_t k = 0; k < d.n_ops; k++) sam_w32(w + 8 + 4 * (size_t)k, ops[k]);
    }
    return SAM_OK;
}

extern "C" int svx_sam_convert_host(const uint8_t* text, int64_t n, int32_t n_ref, const char* names_blob, uint8_t* out, int64_t cap, int64_t* n_out, int64_t* n_records,
                                    int64_t* bad_line) {
    if (n < 0 || n_ref < 0 || cap < 0 || (n && !text) || (cap && !out) || !n_out || !n_records || !bad_line || (n_ref && !names_blob)) return SVX_E_ARG;
    *n_out = 0; *n_records = 0; *bad_line = 0;
    ContigTableHost hc;
    hc.build(n_ref, names_blob);
    const ContigTable ct = hc.view();
    int64_t at = 0, line = 0, recs = 0;
    bool all_fit = true;
    for (int64_t p = 0; p < n;) {
        const uint8_t* nl = (const uint8_t*)memchr(text + p, '\n', (size_t)(n - p));
        const int64_t e = nl ? nl - text : n;
        line++;
        if (recs == 0 && e > p && text[p] == '@') { p = e + 1; continue; }          // the header in front of the first alignment
        if (e - p > 0x7fffffff) { *bad_line = line; g_svx_err = "SAM line " + std::to_string(line) + ": longer than 2^31 bytes"; return SVX_E_ARG; }
        uint64_t size = 0; bool fits = false;
        const int err = convert_line(text + p, (uint32_t)(e - p), ct, &size, all_fit && cap > at ? (uint64_t)(cap - at) : 0, (all_fit && out) ? out + at : nullptr, &fits);
        if (err) { *bad_line = line; g_svx_err = "SAM line " + std::to_string(line) + ": " + sam_strerror(err); return err == SAM_E_RANGE ? SVX_E_RANGE : SVX_E_ARG; }
        if (!fits) all_fit = false;
        at += (int64_t)size; recs++;
        p = e + 1;
    }
    *n_out = at; *n_records = recs;
    return all_fit ? SVX_OK : SVX_E_CAPACITY;
}

// header text -> magic, l_text, the text verbatim, n_ref and the dictionary of its @SQ lines in order.  names / lengths (optional): the dictionary
int sam_header_parse(const char* text, size_t n, std::vector<std::string>* names, std::vector<int32_t>* lengths, std::string* sort_order) {
    for (size_t p = 0; p < n;) {
        const char* nl = (const char*)memchr(text + p, '\n', n - p);
        const size_t e = nl ? (size_t)(nl - text) : n;
        const std::string line(text + p, e - p);
        if (line.compare(0, 4, "@SQ\t") == 0) {
            std::string nm; long long ln = -1;
            for (size_t a = 4; a <= line.size();) {
                size_t b = line.find('\t', a);
                if (b == std::string::npos) b = line.size();
                if (line.compare(a, 3, "SN:") == 0) nm = line.substr(a + 3, b - a - 3);
                else if (line.compare(a, 3, "LN:") == 0) { int64_t v; if (sam_parse_int((const uint8_t*)line.data() + a + 3, (uint32_t)(b - a - 3), 0, 2147483647ll, &v)) ln = v; }
                a = b + 1;
            }
            if (nm.empty() || ln < 0) return SVX_E_ARG;
            if (names) names->push_back(nm);
            if (lengths) lengths->push_back((int32_t)ln);
        } else if (line.compare(0, 4, "@HD\t") == 0 && sort_order) {
            const size_t so = line.find("\tSO:");
            if (so != std::string::npos) { const size_t t = line.find('\t', so + 4); *sort_order = line.substr(so + 4, t == std::string::npos ? std::string::npos : t - so - 4); }
        }
        p = e + 1;
    }
    return SVX_OK;
}

extern "C" int svx_sam_header_host(const char* header_text, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (n < 0 || cap < 0 || (n && !header_text) || (cap && !out) || !n_out) return SVX_E_ARG;
    std::vector<std::string> names; std::vector<int32_t> lengths;
    if (sam_header_parse(header_text, (size_t)n, &names, &lengths, nullptr) != SVX_OK) { g_svx_err = "svx_sam_header_host: an @SQ line without SN or LN"; return SVX_E_ARG; }
    int64_t total = 12 + n;
    for (auto& s : names) total += 8 + (int64_t)s.size() + 1;
    *n_out = total;
    if (total > cap) return SVX_E_CAPACITY;
    uint8_t* w = out;
    memcpy(w, "BAM\1", 4); sam_w32(w + 4, (uint32_t)n); memcpy(w + 8, header_text, (size_t)n); w += 8 + n;
    sam_w32(w, (uint32_t)names.size()); w += 4;
    for (size_t k = 0; k < names.size(); k++) {
        sam_w32(w, (uint32_t)names[k].size() + 1); memcpy(w + 4, names[k].c_str(), names[k].size() + 1); w += 4 + names[k].size() + 1;
        sam_w32(w, (uint32_t)lengths[k]); w += 4;
    }
    return SVX_OK;
}
