// bed.hip - the BED files of the signature clusters and of the candidates, and the body of signatures/all.vcf, on the device (gfx950).
//
// Restates write_signature_clusters_bed / write_signature_clusters_vcf (src/svim/SVIM_CLUSTER.py:29-106), write_candidates (src/svim/SVIM_COMBINE.py:18-58), the
// get_bed_entry / get_bed_entries / get_vcf_entry methods of the two cluster classes (src/svim/SVSignature.py:252-260, :293-303) and of the six candidate classes
// (src/svim/SVCandidate.py:52, :219, :302, :455, :618), and the five as_string forms of a member signature (SVSignature.py:36, :99, :150, :183, :224) on the
// cluster table of the last svx_cluster, the candidate table of the last svx_combine (or tables handed in) and the signature table their members index.
// Phases, all on the context's stream, in the shape of vcf.hip:
//   1  entries     products 0 and 2: the tables are grouped by type / class and every file takes the rows of one group (one line each, or the source and the
//                  destination line interleaved), so a line's row and form are a closed form of the group counts.  Product 1: the DEL, INS, INV and DUP_TAN rows in
//                  table order ARE the reference's append order; two stable radix passes (end; contig rank in Python str order << 32 | start) give the order
//   2  lengths     the text of one member - '[' as_string('|') ']' - depends on the member signature alone: its length per entry of the member list, one
//                  prefix sum; a line's member payload is then a difference of that prefix.  The line emitter with a counting sink gives the line lengths;
//                  int64 scans -> line offsets, payload tile offsets; one mailbox read brings the file offsets and the totals; the host allocates the text
//   3  skeleton    the same emitter with a writing sink: one lane per line stores everything but the member list (the repr of the score and the deviations
//                  included) and leaves a descriptor of the member payload
//      payload     one wave per tile of 1 KiB of ONE line's member list.  A lane owns one 16-byte chunk at a 16-byte aligned destination, finds the member its
//                  first byte falls into by bisection in the piece prefix and runs the piece emitter with a sink that keeps only the bytes of its window (a
//                  piece is longer than 16 bytes, so a chunk touches at most two).  No lane walks a member list.
// The counting, the writing and the window pass are ONE function template each (emit_line, emit_piece) over different sinks, so lengths and bytes cannot
// disagree; the writing sink additionally refuses to leave its line.
#include "common.hpp"
#include "hostcopy.hpp"
#include "text_put.hpp"
#include "fmt_repr.hpp"
#include <algorithm>

#define BT 256
#define BGRID(n) (unsigned)(((long long)(n) + BT - 1) / BT)
#define BED_TILE 1024          /* payload bytes per wave: 64 lanes x one 16-byte chunk */
#define BED_NPOOL 64

enum { L_CL_UNI = 0, L_CL_SRC, L_CL_DST, L_CL_VCF, L_CA_PLAIN, L_CA_INS, L_CA_TAN_SRC, L_CA_TAN_DST, L_CA_INT_SRC, L_CA_INT_DST, L_CA_BND_SRC, L_CA_BND_DST };
enum { BERR_STD = 1, BERR_INDEX = 2, BERR_OVERRUN = 4, BERR_HUGE = 8 };

struct BedSeg { long long dst, len, a, b; };
struct BedSlots { long long base[SVX_BED_MAX_FILES + 1]; long long lo[SVX_BED_MAX_FILES]; int form[SVX_BED_MAX_FILES]; int two[SVX_BED_MAX_FILES]; int n_files; };
struct BedIn {
    long long n_rows, n_members, n_sig, n_reads;
    // rows: a cluster table (kind = type, extra = size) or a candidate table (kind = cls, extra = copies)
    const uint8_t* kind; const int32_t *contig, *start, *end, *contig2, *start2, *end2; const uint8_t* aux; const int32_t* extra;
    const double *score, *std_span, *std_pos; const int64_t* member_off; const int32_t* members;
    // the signature table the members index
    const uint8_t *s_type, *s_src, *s_aux; const int32_t *s_contig, *s_start, *s_end, *s_contig2, *s_pos2, *s_read_id;
    const char* cname; const int32_t* cname_off; const int32_t* cname_len; const int32_t* crank; int n_contig;
    const char* rname; const int64_t* rname_off;
    const int64_t* P;                      // prefix sums of the member piece lengths over the member list
    const uint64_t* rtab;                  // multiplier tables of repr(float)
    long long short_line;                  // tests: this line + 1 is counted one byte short (0: none)
    int* err; unsigned long long* counters;
};

// ---------------------------------------------------------------------------------------------------------
// sinks
// ---------------------------------------------------------------------------------------------------------
struct BedCount {
    long long n = 0, seg = 0;
    __device__ __forceinline__ void ch(char) { n++; }
    __device__ __forceinline__ void bytes(const char*, int len) { n += len; }
    __device__ __forceinline__ void payload(long long, long long, long long len) { seg = len; n += len; }
};
// Bytes gather in a 64-bit word that leaves as ONE store when it fills an aligned 8 bytes of the output, byte by byte otherwise.  Nothing is stored outside
// [pos0, end): a disagreement with the counted length sets BERR_OVERRUN instead
struct BedWrite {
    uint8_t* base; long long pos, end; unsigned long long acc; int nacc; BedSeg* seg; int* err;
    __device__ __forceinline__ void flush() {
        if (nacc == 0) return;
        if (pos + nacc > end) { atomicOr(err, BERR_OVERRUN); acc = 0; nacc = 0; return; }
        if (nacc == 8) *reinterpret_cast<unsigned long long*>(base + pos) = acc;
        else for (int k = 0; k < nacc; k++) base[pos + k] = (uint8_t)(acc >> (8 * k));
        pos += nacc; acc = 0; nacc = 0;
    }
    __device__ __forceinline__ void ch(char c) {
        acc |= (unsigned long long)(uint8_t)c << (8 * nacc);
        nacc++;
        if (((pos + nacc) & 7) == 0) flush();
    }
    __device__ __forceinline__ void bytes(const char* p, int len) { for (int k = 0; k < len; k++) ch(p[k]); }
    __device__ __forceinline__ void payload(long long a, long long b, long long len) {
        flush();
        BedSeg d; d.dst = pos; d.len = pos + len <= end ? len : 0; d.a = a; d.b = b;
        if (pos + len > end) atomicOr(err, BERR_OVERRUN);
        *seg = d;
        pos += d.len;
    }
};
// keeps the bytes [lo, hi) of what is emitted, at byte qb + (position - lo) of a 16-byte register pair
struct BedWindow {
    int pos, lo, hi, qb; unsigned long long r0, r1;
    __device__ __forceinline__ void put(int q, unsigned v) { if (q < 8) r0 |= (unsigned long long)v << (8 * q); else r1 |= (unsigned long long)v << (8 * (q - 8)); }
    __device__ __forceinline__ void ch(char c) { if (pos >= lo && pos < hi) put(qb + pos - lo, (uint8_t)c); pos++; }
    __device__ __forceinline__ void bytes(const char* p, int len) {
        const int a = lo > pos ? lo - pos : 0, b = hi - pos < len ? hi - pos : len;
        for (int k = a; k < b; k++) put(qb + pos + k - lo, (uint8_t)p[k]);
        pos += len;
    }
};

// ---------------------------------------------------------------------------------------------------------
// emitters
// ---------------------------------------------------------------------------------------------------------
template <class S> __device__ __forceinline__ void bed_contig(S& s, const BedIn& in, int c) {
    if (c < 0 || c >= in.n_contig) { atomicOr(in.err, BERR_INDEX); return; }
    s.bytes(in.cname + in.cname_off[c], in.cname_len[c]);
}
template <class S> __device__ __forceinline__ void bed_type_name(S& s, unsigned t) {
    put_str(s, t == SVX_DEL ? "DEL" : t == SVX_INS ? "INS" : t == SVX_INV ? "INV" : t == SVX_DUP_TAN ? "DUP_TAN" : t == SVX_BND ? "BND" : "DUP_INT");
}
template <class S> __device__ __forceinline__ void bed_locus(S& s, const BedIn& in, int c, long long a, long long b) {      // contig:a-b
    bed_contig(s, in, c); s.ch(':'); put_i64(s, a); s.ch('-'); put_i64(s, b);
}
// '[' + as_string('|') + ']' of signature m (a valid row of the signature table: k_bed_member_len has checked it)
template <class S> __device__ __forceinline__ void emit_piece(S& s, const BedIn& in, long long m) {
    const unsigned t = in.s_type[m], aux = in.s_aux[m];
    const int c1 = in.s_contig[m], c2 = in.s_contig2[m];
    const long long st = in.s_start[m], en = in.s_end[m], p2 = in.s_pos2[m];
    s.ch('[');
    if (t <= SVX_INV) {
        bed_contig(s, in, c1); s.ch('|'); put_i64(s, st); s.ch('|'); put_i64(s, en); s.ch('|');
    } else if (t == SVX_DUP_INT) {
        bed_locus(s, in, c1, st, en); s.ch('|'); bed_locus(s, in, c2, p2, p2 + (en - st)); s.ch('|');
    } else if (t == SVX_DUP_TAN) {
        bed_locus(s, in, c1, st, en); s.ch('|'); bed_locus(s, in, c1, en, en + p2 * (en - st)); s.ch('|');
    } else {
        bed_locus(s, in, c1, st, st + 1); s.ch('|'); bed_locus(s, in, c2, p2, p2 + 1); s.ch('|');
    }
    bed_type_name(s, t); s.ch(';');
    if (t == SVX_INV) { put_str(s, aux == 0 ? "left_fwd" : aux == 1 ? "left_rev" : aux == 2 ? "right_fwd" : aux == 3 ? "right_rev" : "all"); s.ch(';'); }
    put_str(s, in.s_src[m] == SVX_SRC_CIGAR ? "cigar" : "suppl");
    if (t == SVX_DUP_TAN) { s.ch(';'); put_i64(s, p2); }
    s.ch('|');
    const int r = in.s_read_id[m];
    if (r >= 0 && r < in.n_reads) { const long long o = in.rname_off[r]; s.bytes(in.rname + o, (int)(in.rname_off[r + 1] - o)); }
    s.ch(']');
}
// "{}".format(x) of a cluster's deviation: None for NaN, repr otherwise
template <class S> __device__ __forceinline__ void put_repr_or_none(S& s, const BedIn& in, double x) {
    if (x != x) put_str(s, "None"); else put_repr(s, x, in.rtab);
}
template <class S> __device__ __forceinline__ bool put_std_pair(S& s, const BedIn& in, long long i) {
    bool ok = put_std(s, in.std_span[i]); s.ch(';'); ok &= put_std(s, in.std_pos[i]);
    return ok;
}

// one line.  form: L_*, i: row of the table
template <class S> __device__ __forceinline__ void emit_line(S& s, const BedIn& in, int form, long long i) {
    const int c1 = in.contig[i], c2 = in.contig2[i];
    const long long s1 = in.start[i], e1 = in.end[i], s2 = in.start2[i], e2 = in.end2[i], extra = in.extra[i];
    const unsigned kind = in.kind[i], aux = in.aux[i];
    bool ok = true;
    if (form == L_CL_VCF) {
        bed_contig(s, in, c1); s.ch('\t'); put_i64(s, s1 + 1); put_str(s, "\t.\tN\t<");
        if (kind == SVX_DUP_TAN) put_str(s, "DUP:TANDEM"); else bed_type_name(s, kind);
        put_str(s, ">\t.\tPASS\tSVTYPE=");
        if (kind == SVX_DUP_TAN) put_str(s, "DUP:TANDEM"); else bed_type_name(s, kind);
        put_str(s, ";END="); put_i64(s, e1); put_str(s, ";SVLEN="); put_i64(s, e1 - s1);
        put_str(s, ";STD_SPAN="); put_repr_or_none(s, in, in.std_span[i]); put_str(s, ";STD_POS="); put_repr_or_none(s, in, in.std_pos[i]);
        s.ch('\n');
        return;
    }
    const long long dend = e1 + extra * (e1 - s1);            // the tandem duplication's destination end: leaves int32
    // the three locus columns
    const bool at_dest = form == L_CL_DST || form == L_CA_INS || form == L_CA_INT_DST || form == L_CA_BND_DST;
    bed_contig(s, in, at_dest ? c2 : c1); s.ch('\t');
    long long a, b;
    if (form == L_CA_TAN_DST) { a = e1; b = dend; }
    else if (form == L_CA_BND_SRC) { a = s1; b = s1 + 1; }
    else if (form == L_CA_BND_DST) { a = s2; b = s2 + 1; }
    else if (at_dest) { a = s2; b = e2; }
    else { a = s1; b = e1; }
    put_i64(s, a); s.ch('\t'); put_i64(s, b); s.ch('\t');
    // the name column
    if (form == L_CL_UNI || form == L_CL_SRC) {
        bed_type_name(s, kind);
        if (form == L_CL_SRC) { put_str(s, "_source;"); bed_locus(s, in, c2, s2, e2); }
        s.ch(';'); put_i64(s, extra); s.ch(';'); put_repr_or_none(s, in, in.std_span[i]); s.ch(';'); put_repr_or_none(s, in, in.std_pos[i]);
    } else if (form == L_CL_DST) {
        bed_type_name(s, kind); put_str(s, "_dest;"); bed_locus(s, in, c1, s1, e1); s.ch(';'); put_i64(s, extra);
    } else {
        if (form == L_CA_PLAIN) put_str(s, kind == SVX_CAND_DEL ? "DEL" : "INV");
        else if (form == L_CA_INS) put_str(s, "INS");
        else if (form == L_CA_TAN_SRC) { put_str(s, "tan_dup_source;>"); bed_locus(s, in, c1, e1, dend); }
        else if (form == L_CA_TAN_DST) { put_str(s, "tan_dup_dest;<"); bed_locus(s, in, c1, s1, e1); }
        else if (form == L_CA_INT_SRC) { put_str(s, "int_dup_source;>"); bed_locus(s, in, c2, s2, e2); }
        else if (form == L_CA_INT_DST) { put_str(s, "int_dup_dest;<"); bed_locus(s, in, c1, s1, e1); }
        else if (form == L_CA_BND_SRC) { put_str(s, "bnd;>"); bed_contig(s, in, c2); s.ch(':'); put_i64(s, s2); }
        else { put_str(s, "bnd;<"); bed_contig(s, in, c1); s.ch(':'); put_i64(s, s1); }
        s.ch(';'); ok &= put_std_pair(s, in, i);
    }
    if (!ok) atomicOr(in.err, BERR_STD);
    s.ch('\t'); put_repr(s, in.score[i], in.rtab); s.ch('\t');
    if (form >= L_CA_PLAIN && form <= L_CA_INT_DST) {
        if ((form == L_CA_INT_SRC || form == L_CA_INT_DST) && (aux & 1u)) put_str(s, "origin potentially deleted"); else s.ch('.');
        s.ch('\t');
    }
    const long long m_lo = in.member_off[i], m_hi = in.member_off[i + 1];
    if (m_hi > m_lo) s.payload(m_lo, m_hi, in.P[m_hi] - in.P[m_lo]); else { s.ch('['); s.ch(']'); }
    s.ch('\n');
}

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------
__global__ void k_bed_entries(long long n, BedSlots sl, uint32_t* line_row, uint8_t* line_form) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int k = 0;
#pragma unroll
    for (int j = 1; j < SVX_BED_MAX_FILES; j++) k += (j < sl.n_files && e >= sl.base[j]) ? 1 : 0;
    const long long r = e - sl.base[k];
    line_row[e] = (uint32_t)(sl.lo[k] + (sl.two[k] ? r >> 1 : r));
    line_form[e] = (uint8_t)(sl.form[k] + ((sl.two[k] && (r & 1)) ? 1 : 0));
}
// product 1: sort keys of the first n rows (source tuple: contig name as a string, start, end)
__global__ void k_bed_vcf_keys(long long n, BedIn in, uint64_t* key_end, uint64_t* key_cs, uint32_t* idx, uint8_t* line_form) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int c = in.contig[e];
    unsigned rank = 0;
    if (c < 0 || c >= in.n_contig) atomicOr(in.err, BERR_INDEX); else rank = (unsigned)in.crank[c];
    key_end[e] = (uint64_t)((uint32_t)in.end[e] ^ 0x80000000u);
    key_cs[e] = ((uint64_t)rank << 32) | (uint64_t)((uint32_t)in.start[e] ^ 0x80000000u);
    idx[e] = (uint32_t)e; line_form[e] = (uint8_t)L_CL_VCF;
}
__global__ void k_bed_gather_u64(const uint64_t* src, const uint32_t* perm, uint64_t* dst, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}
// length of the piece of member-list entry j (0 behind the list), after checking every id the piece emitter will read
__global__ void k_bed_member_len(BedIn in, int32_t* len) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > in.n_members) return;
    if (j == in.n_members) { len[j] = 0; return; }
    const long long m = in.members[j];
    long long l = 0;
    bool ok = m >= 0 && m < in.n_sig;
    if (ok) {
        const unsigned t = in.s_type[m];
        const int c1 = in.s_contig[m], c2 = in.s_contig2[m], r = in.s_read_id[m];
        ok = t < SVX_NTYPES && c1 >= 0 && c1 < in.n_contig && r >= 0 && r < in.n_reads && in.s_src[m] <= SVX_SRC_SUPPL;
        if (ok && (t == SVX_BND || t == SVX_DUP_INT)) ok = c2 >= 0 && c2 < in.n_contig;
        if (ok && t == SVX_INV) ok = in.s_aux[m] <= 4;
        if (ok) { const long long nl = in.rname_off[r + 1] - in.rname_off[r]; ok = nl >= 0 && nl < (1ll << 24); }
    }
    if (ok) { BedCount cs; emit_piece(cs, in, m); l = cs.n; } else atomicOr(in.err, BERR_INDEX);
    len[j] = (int32_t)l;
}
__device__ __forceinline__ long long bed_seg_tiles(long long len) { return len > 0 ? (len + 15 + BED_TILE - 1) / BED_TILE : 0; }      // whatever the destination's alignment turns out to be

__global__ __launch_bounds__(BT) void k_bed_lengths(long long n, const uint32_t* line_row, const uint8_t* line_form, BedIn in, int64_t* line_len, int64_t* tiles) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    BedCount cs;
    if (s < n) {
        emit_line(cs, in, line_form[s], line_row[s]);
        line_len[s] = cs.n - (in.short_line == s + 1 ? 1 : 0);
        tiles[s] = bed_seg_tiles(cs.seg);
        if (cs.seg >> 40) atomicOr(in.err, BERR_HUGE);
    } else if (s == n) {
        line_len[s] = 0; tiles[s] = 0;
    }
    const long long t = wave_sum_i64(cs.seg);
    if (lane_id() == 0 && t) atomicAdd(in.counters, (unsigned long long)t);
}
struct BedFileLines { long long first[SVX_BED_MAX_FILES + 1]; int n_files; };
// the few words the host waits for, gathered into one array: file offsets, tiles, error word, payload bytes
__global__ void k_bed_totals(BedFileLines fl, const int64_t* line_off, const int64_t* tile_total, const int* err, const unsigned long long* counters, unsigned long long* tot) {
    const int k = (int)threadIdx.x;
    if (k <= fl.n_files) tot[k] = (unsigned long long)line_off[fl.first[k]];
    if (k == 0) { tot[SVX_BED_MAX_FILES + 1] = (unsigned long long)*tile_total; tot[SVX_BED_MAX_FILES + 2] = (unsigned)*err; tot[SVX_BED_MAX_FILES + 3] = counters[0]; }
}

__global__ __launch_bounds__(BT) void k_bed_skeleton(long long n, const uint32_t* line_row, const uint8_t* line_form, BedIn in, const int64_t* line_off, uint8_t* out, BedSeg* segs) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    BedSeg none; none.dst = 0; none.len = 0; none.a = 0; none.b = 0;
    segs[s] = none;
    BedWrite ws; ws.base = out; ws.pos = line_off[s]; ws.end = line_off[s + 1]; ws.acc = 0; ws.nacc = 0; ws.seg = segs + s; ws.err = in.err;
    emit_line(ws, in, line_form[s], line_row[s]);
    ws.flush();
    if (ws.pos != ws.end) atomicOr(in.err, BERR_OVERRUN);
}

// One wave per tile.  Lane l of tile t of a payload owns the 16 bytes at the aligned address (dst & ~15) + 16 * (64 * t + l), cut to the payload.
__global__ __launch_bounds__(BT) void k_bed_payload(int n_tiles, const int64_t* tile_start, long long n_seg, const BedSeg* segs, BedIn in, uint8_t* out) {
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BT / 64) + (threadIdx.x >> 6)));
    if (t >= n_tiles) return;
    long long lo = 0, hi = n_seg;                         // first payload with tile_start[g + 1] > t (wave-uniform: scalar loads)
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (tile_start[mid + 1] > t) hi = mid; else lo = mid + 1; }
    if (lo >= n_seg) return;
    const BedSeg d = segs[lo];
    if (d.len <= 0) return;
    const long long chunk = ((long long)t - tile_start[lo]) * 64 + lane_id();
    const long long a0 = (d.dst & ~15ll) + 16 * chunk;    // aligned address of this lane's chunk
    const long long w0 = a0 > d.dst ? a0 : d.dst, w1 = a0 + 16 < d.dst + d.len ? a0 + 16 : d.dst + d.len;
    if (w0 >= w1) return;
    const int nb = (int)(w1 - w0), q0 = (int)(w0 - a0);
    const int64_t* P = in.P;
    const long long v = P[d.a] + (w0 - d.dst);
    long long jl = d.a, jh = d.b;                         // the member whose piece holds virtual position v: first j with P[j + 1] > v
    while (jl < jh) { const long long mid = (jl + jh) >> 1; if (P[mid + 1] > v) jh = mid; else jl = mid + 1; }
    long long j = jl;
    BedWindow ws; ws.r0 = 0; ws.r1 = 0;
    int k = 0;
    long long tpos = j < d.b ? v - P[j] : 0;
    while (k < nb && j < d.b) {
        const long long left = P[j + 1] - P[j] - tpos;
        const int take = (int)(left < (long long)(nb - k) ? left : (long long)(nb - k));
        const long long m = in.members[j];
        if (m < 0 || m >= in.n_sig || take <= 0) break;
        ws.pos = 0; ws.lo = (int)tpos; ws.hi = (int)tpos + take; ws.qb = q0 + k;
        emit_piece(ws, in, m);
        k += take; j++; tpos = 0;
    }
    if (nb == 16) {
        ulonglong2 w; w.x = ws.r0; w.y = ws.r1;
        *reinterpret_cast<ulonglong2*>(out + a0) = w;
    } else {
        for (int b = 0; b < nb; b++) { const int q = q0 + b; out[a0 + q] = (uint8_t)((q < 8 ? ws.r0 >> (8 * q) : ws.r1 >> (8 * (q - 8))) & 0xffull); }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host: state and the call
// ---------------------------------------------------------------------------------------------------------
struct BedState {
    ScratchPool<BED_NPOOL> pool{"bed"};
    DevBuf out, line_off, rname, rname_off;
    int64_t n_reads = 0; bool have_names = false;
    int64_t n_lines = 0, n_bytes = 0; int n_files = 0;
    int64_t file_off[SVX_BED_MAX_FILES + 1], file_line[SVX_BED_MAX_FILES + 1];
    bool have = false;
    hipEvent_t ev[7]; bool have_ev = false;
    svx_bed_stats stats;
};
static int bed_state(svx_ctx* c, BedState** out) {
    if (!c->bed) { c->bed = new BedState(); memset(&c->bed->stats, 0, sizeof c->bed->stats); }
    BedState* S = c->bed;
    if (!S->have_ev) { for (auto& e : S->ev) HIPCHK(hipEventCreate(&e)); S->have_ev = true; }
    *out = S;
    return SVX_OK;
}
void svx_bed_release(svx_ctx* c) {
    BedState* s = c->bed;
    if (!s) return;
    s->pool.release();
    s->out.release(); s->line_off.release(); s->rname.release(); s->rname_off.release();
    if (s->have_ev) for (auto& e : s->ev) (void)hipEventDestroy(e);
    delete s;
    c->bed = nullptr;
}
void svx_preload_bed() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_bed_payload)); (void)hipGetLastError(); }

extern "C" int svx_bed_set_read_names(svx_ctx* c, const char* blob, const int64_t* off, int64_t n_reads) {
    if (!c || !off || n_reads < 0 || off[0] != 0) return svx_fail(SVX_E_ARG, "svx_bed_set_read_names: bad argument (offsets are required and start at 0)", __FILE__, __LINE__, hipSuccess);
    for (int64_t r = 0; r < n_reads; r++) if (off[r + 1] < off[r]) return svx_fail(SVX_E_ARG, "svx_bed_set_read_names: read_name_off decreases", __FILE__, __LINE__, hipSuccess);
    if (off[n_reads] > 0 && !blob) return svx_fail(SVX_E_ARG, "svx_bed_set_read_names: the names are missing", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    BedState* S; SVXCHK(bed_state(c, &S));
    S->have_names = false;
    SVXCHK(S->rname_off.reserve((size_t)(n_reads + 1) * 8 + 64)); SVXCHK(S->rname.reserve((size_t)off[n_reads] + 64));
    HostCopy hc(c->stream);
    SVXCHK(hc.h2d(S->rname_off.p, off, (size_t)(n_reads + 1) * 8));
    if (off[n_reads] > 0) SVXCHK(hc.h2d(S->rname.p, blob, (size_t)off[n_reads]));
    SVXCHK(hc.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    S->n_reads = n_reads; S->have_names = true;
    return SVX_OK;
}

extern "C" int svx_bed(svx_ctx* c, int product, int source, const svx_cluster_view* cl, const svx_candidate_view* cv, const svx_sig_view* sv, const svx_bed_inputs* ip) {
    if (!c || !ip || ip->n_contig < 0 || (ip->n_contig && !ip->contig_names_nul_separated) || product < SVX_BED_SIGNATURE_BEDS || product > SVX_BED_CANDIDATE_BEDS ||
        (product == SVX_BED_SIGNATURE_VCF && ip->n_contig && !ip->contig_str_rank))
        return svx_fail(SVX_E_ARG, "svx_bed: bad argument (product 0..2; the inputs and the contig names are required, product 1 needs the contig ranks)", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    BedState* S; SVXCHK(bed_state(c, &S));
    S->pool.reset(); S->have = false; S->n_lines = S->n_bytes = 0; S->n_files = 0;
    c->bed_calls++;                    // (a BGZF stream made of the text before is void from here on)
    memset(&S->stats, 0, sizeof S->stats);
    const bool cand = product == SVX_BED_CANDIDATE_BEDS, with_members = product != SVX_BED_SIGNATURE_VCF;
    hipStream_t st = c->stream;
    HIPCHK(hipEventRecord(S->ev[0], st));
    BedIn in; memset(&in, 0, sizeof in);
    int64_t group_count[6];
    HostCopy hc(st);
#define UP(field, type, host, count) do { type* d_; SVXCHK(S->pool.get(&d_, (count))); if ((count)) SVXCHK(hc.h2d(d_, (host), (size_t)(count) * sizeof(type))); in.field = d_; } while (0)
    if (source == 0) {
        if (cand) {
            CandDev cd;
            if (!svx_combine_resident(c, &cd)) return svx_fail(SVX_E_STATE, "svx_bed: no resident candidates: run svx_combine first", __FILE__, __LINE__, hipSuccess);
            if (!cd.from_resident || cd.cluster_call != c->cluster_calls)
                return svx_fail(SVX_E_STATE, "svx_bed: the signature table the resident candidates' members index is gone (svx_combine source 0 of the last svx_cluster is required)",
                                __FILE__, __LINE__, hipSuccess);
            in.n_rows = cd.n; in.n_members = cd.n_members;
            in.kind = cd.cls; in.contig = cd.contig; in.start = cd.start; in.end = cd.end; in.contig2 = cd.contig2; in.start2 = cd.start2; in.end2 = cd.end2; in.aux = cd.aux;
            in.extra = cd.copies; in.score = cd.score; in.std_span = cd.std_span; in.std_pos = cd.std_pos; in.member_off = cd.member_off; in.members = cd.members;
            for (int k = 0; k < 6; k++) group_count[k] = cd.class_count[k];
        } else {
            if (c->cluster_calls <= 0) return svx_fail(SVX_E_STATE, "svx_bed: no resident clusters: run svx_cluster first", __FILE__, __LINE__, hipSuccess);
            const DevClusters& d = c->clu;
            in.n_rows = d.n; in.n_members = d.n_members;
            in.kind = d.type.as<uint8_t>(); in.contig = d.contig.as<int32_t>(); in.start = d.start.as<int32_t>(); in.end = d.end.as<int32_t>();
            in.contig2 = d.contig2.as<int32_t>(); in.start2 = d.start2.as<int32_t>(); in.end2 = d.end2.as<int32_t>(); in.aux = d.aux.as<uint8_t>();
            in.extra = d.size.as<int32_t>(); in.score = d.score.as<double>(); in.std_span = d.std_span.as<double>(); in.std_pos = d.std_pos.as<double>();
            in.member_off = d.member_off.as<int64_t>(); in.members = d.members.as<int32_t>();
            for (int k = 0; k < 6; k++) group_count[k] = d.type_count[k];
        }
        const ClusterIn& ci = c->last_cluster_in;
        if (with_members && in.n_members > 0 && (c->cluster_calls <= 0 || !ci.src || !ci.type || !ci.read_id))
            return svx_fail(SVX_E_STATE, "svx_bed: the signature table the members index is not resident with all its columns (svx_cluster of resident or device signatures is required)",
                            __FILE__, __LINE__, hipSuccess);
        in.n_sig = c->last_cluster_source_n;
        in.s_type = ci.type; in.s_src = ci.src; in.s_aux = ci.aux; in.s_contig = ci.contig; in.s_start = ci.start; in.s_end = ci.end; in.s_contig2 = ci.contig2;
        in.s_pos2 = ci.pos2; in.s_read_id = ci.read_id;
    } else if (source == 2) {
        if ((cand ? !cv : !cl) || (with_members && (!sv || sv->on_device || sv->n < 0)))
            return svx_fail(SVX_E_ARG, "svx_bed: source 2 needs a cluster table (products 0, 1) or a candidate table (product 2) and the signature columns in host memory", __FILE__, __LINE__, hipSuccess);
        const int64_t n64 = cand ? cv->n : cl->n, nm64 = cand ? cv->n_members : cl->n_members;
        if (n64 < 0 || nm64 < 0) return svx_fail(SVX_E_ARG, "svx_bed: negative table size", __FILE__, __LINE__, hipSuccess);
        const size_t n = (size_t)n64, nm = (size_t)nm64;
        int64_t total = 0;
        for (int k = 0; k < 6; k++) { group_count[k] = cand ? cv->class_count[k] : cl->type_count[k]; if (group_count[k] < 0) return svx_fail(SVX_E_ARG, "svx_bed: negative group count", __FILE__, __LINE__, hipSuccess); total += group_count[k]; }
        if (total != n64) return svx_fail(SVX_E_ARG, "svx_bed: the group counts do not add up to n", __FILE__, __LINE__, hipSuccess);
        const uint8_t* kind = cand ? cv->cls : cl->type; const int32_t* extra = cand ? cv->copies : cl->size;
        const int32_t *h_c = cand ? cv->contig : cl->contig, *h_s = cand ? cv->start : cl->start, *h_e = cand ? cv->end : cl->end, *h_c2 = cand ? cv->contig2 : cl->contig2,
                      *h_s2 = cand ? cv->start2 : cl->start2, *h_e2 = cand ? cv->end2 : cl->end2;
        const uint8_t* h_aux = cand ? cv->aux : cl->aux;
        const double *h_sc = cand ? cv->score : cl->score, *h_sp = cand ? cv->std_span : cl->std_span, *h_po = cand ? cv->std_pos : cl->std_pos;
        const int64_t* h_mo = cand ? cv->member_off : cl->member_off; const int32_t* h_m = cand ? cv->members : cl->members;
        if (n && (!kind || !extra || !h_c || !h_s || !h_e || !h_c2 || !h_s2 || !h_e2 || !h_aux || !h_sc || !h_sp || !h_po)) return svx_fail(SVX_E_ARG, "svx_bed: a table column is missing", __FILE__, __LINE__, hipSuccess);
        if (!h_mo || (nm && !h_m) || h_mo[0] != 0 || h_mo[n] != nm64) return svx_fail(SVX_E_ARG, "svx_bed: member_off does not describe n_members members", __FILE__, __LINE__, hipSuccess);
        for (size_t i = 0, k = 0, hi = (size_t)group_count[0]; i < n; i++) {
            while (k < 6 && i >= hi) { k++; if (k < 6) hi += (size_t)group_count[k]; }
            if (k >= 6 || kind[i] != k) return svx_fail(SVX_E_ARG, "svx_bed: the table is not grouped by type / class as its counts say", __FILE__, __LINE__, hipSuccess);
            if (h_mo[i + 1] < h_mo[i]) return svx_fail(SVX_E_ARG, "svx_bed: member_off decreases", __FILE__, __LINE__, hipSuccess);
        }
        in.n_rows = n64; in.n_members = nm64;
        UP(kind, uint8_t, kind, n); UP(aux, uint8_t, h_aux, n);
        UP(contig, int32_t, h_c, n); UP(start, int32_t, h_s, n); UP(end, int32_t, h_e, n); UP(contig2, int32_t, h_c2, n); UP(start2, int32_t, h_s2, n); UP(end2, int32_t, h_e2, n);
        UP(extra, int32_t, extra, n); UP(score, double, h_sc, n); UP(std_span, double, h_sp, n); UP(std_pos, double, h_po, n);
        UP(member_off, int64_t, h_mo, n + 1); UP(members, int32_t, h_m, nm);
        if (with_members) {
            const size_t ns = (size_t)sv->n;
            if (ns && (!sv->type || !sv->src || !sv->aux || !sv->contig || !sv->start || !sv->end || !sv->contig2 || !sv->pos2 || !sv->read_id))
                return svx_fail(SVX_E_ARG, "svx_bed: a signature column is missing (type, src, aux, contig, start, end, contig2, pos2, read_id)", __FILE__, __LINE__, hipSuccess);
            in.n_sig = sv->n;
            UP(s_type, uint8_t, sv->type, ns); UP(s_src, uint8_t, sv->src, ns); UP(s_aux, uint8_t, sv->aux, ns);
            UP(s_contig, int32_t, sv->contig, ns); UP(s_start, int32_t, sv->start, ns); UP(s_end, int32_t, sv->end, ns); UP(s_contig2, int32_t, sv->contig2, ns);
            UP(s_pos2, int32_t, sv->pos2, ns); UP(s_read_id, int32_t, sv->read_id, ns);
        }
    } else return svx_fail(SVX_E_ARG, "svx_bed: source must be 0 or 2", __FILE__, __LINE__, hipSuccess);
    const long long n = in.n_rows, nm = with_members ? in.n_members : 0;
    if (n >= (1ll << 30) || nm >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_bed: table too large", __FILE__, __LINE__, hipSuccess);
    if (with_members && nm > 0 && !S->have_names) return svx_fail(SVX_E_STATE, "svx_bed: the lines end with read names: svx_bed_set_read_names first", __FILE__, __LINE__, hipSuccess);
    in.n_reads = S->have_names ? S->n_reads : 0; in.rname = S->rname.as<char>(); in.rname_off = S->rname_off.as<int64_t>();
    // contig names: offsets and lengths of the NUL-separated names
    {
        const int nc = ip->n_contig;
        std::vector<int32_t> off((size_t)nc + 1, 0), len((size_t)nc + 1, 0);
        size_t at = 0;
        for (int k = 0; k < nc; k++) {
            const size_t l = strlen(ip->contig_names_nul_separated + at);
            if (at + l + 1 >= (1ull << 31)) return svx_fail(SVX_E_ARG, "svx_bed: contig names too long", __FILE__, __LINE__, hipSuccess);
            off[k] = (int32_t)at; len[k] = (int32_t)l; at += l + 1;
        }
        UP(cname, char, ip->contig_names_nul_separated, at); UP(cname_off, int32_t, off.data(), (size_t)nc + 1); UP(cname_len, int32_t, len.data(), (size_t)nc + 1);
        if (product == SVX_BED_SIGNATURE_VCF) UP(crank, int32_t, ip->contig_str_rank, (size_t)nc);
        in.n_contig = nc;
        SVXCHK(hc.finish());               // (the vectors leave scope)
    }
#undef UP
    SVXCHK(svx_repr_device_tables(c, &in.rtab));
    in.short_line = ip->debug_short_line;
    unsigned long long* tot;
    { int* err; unsigned long long* cnt; SVXCHK(S->pool.get(&err, 2)); SVXCHK(S->pool.get(&cnt, 8)); SVXCHK(S->pool.get(&tot, 16)); HIPCHK(hipMemsetAsync(err, 0, 8, st)); HIPCHK(hipMemsetAsync(cnt, 0, 64, st)); in.err = err; in.counters = cnt; }
    HIPCHK(hipEventRecord(S->ev[1], st));

    // ---- 1: files and lines over the grouped table ----
    int64_t lo[7]; lo[0] = 0;
    for (int k = 0; k < 6; k++) lo[k + 1] = lo[k] + group_count[k];
    BedSlots sl; memset(&sl, 0, sizeof sl);
    BedFileLines fl; memset(&fl, 0, sizeof fl);
    long long n_lines = 0;
    if (product == SVX_BED_SIGNATURE_VCF) {
        sl.n_files = 1; sl.base[0] = 0; n_lines = lo[SVX_DUP_TAN + 1];      // DEL, INS, INV, DUP_TAN: the first four groups
        sl.base[1] = n_lines;
    } else {
        // (group, form, both lines interleaved) per file, in the reference's order of opening
        static const int sig_files[7][3] = {{SVX_DEL, L_CL_UNI, 0}, {SVX_INS, L_CL_UNI, 0}, {SVX_INV, L_CL_UNI, 0}, {SVX_DUP_TAN, L_CL_SRC, 0}, {SVX_DUP_TAN, L_CL_DST, 0},
                                            {SVX_BND, L_CL_SRC, 1}, {SVX_DUP_INT, L_CL_SRC, 1}};
        static const int cand_files[8][3] = {{SVX_CAND_DEL, L_CA_PLAIN, 0}, {SVX_CAND_INV, L_CA_PLAIN, 0}, {SVX_CAND_DUP_TAN, L_CA_TAN_SRC, 0}, {SVX_CAND_DUP_TAN, L_CA_TAN_DST, 0},
                                             {SVX_CAND_DUP_INT, L_CA_INT_SRC, 0}, {SVX_CAND_DUP_INT, L_CA_INT_DST, 0}, {SVX_CAND_INS, L_CA_INS, 0}, {SVX_CAND_BND, L_CA_BND_SRC, 1}};
        sl.n_files = cand ? 8 : 7;
        for (int k = 0; k < sl.n_files; k++) {
            const int* f = cand ? cand_files[k] : sig_files[k];
            sl.base[k] = n_lines; sl.lo[k] = lo[f[0]]; sl.form[k] = f[1]; sl.two[k] = f[2];
            n_lines += group_count[f[0]] * (f[2] ? 2 : 1);
        }
        sl.base[sl.n_files] = n_lines;
    }
    if (n_lines >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_bed: too many lines", __FILE__, __LINE__, hipSuccess);
    fl.n_files = sl.n_files;
    for (int k = 0; k <= sl.n_files; k++) { fl.first[k] = sl.base[k]; S->file_line[k] = sl.base[k]; S->file_off[k] = 0; }
    S->n_files = sl.n_files;
    S->stats.n_rows = n; S->stats.n_members = nm; S->stats.n_lines = n_lines; S->stats.n_files = sl.n_files;
    for (int k = 0; k < sl.n_files; k++) S->stats.lines_per_file[k] = sl.base[k + 1] - sl.base[k];
    SVXCHK(S->line_off.reserve((size_t)(n_lines + 2) * 8));
    int64_t* line_off = S->line_off.as<int64_t>();
    if (n_lines == 0) {
        HIPCHK(hipMemsetAsync(line_off, 0, 8, st));
        HIPCHK(hipEventRecord(S->ev[6], st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0; (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[6]); S->stats.t_total_ms = ms;
        (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]); S->stats.t_upload_ms = ms;
        S->have = true;
        return SVX_OK;
    }
    const long long ne = n_lines;
    uint32_t* line_row; uint8_t* line_form;
    SVXCHK(S->pool.get(&line_row, ne)); SVXCHK(S->pool.get(&line_form, ne));
    if (product == SVX_BED_SIGNATURE_VCF) {
        uint32_t *idx, *v1; uint64_t *key_end, *key_end2, *key_cs, *key_cs_g, *key_cs2;
        SVXCHK(S->pool.get(&idx, ne)); SVXCHK(S->pool.get(&v1, ne));
        SVXCHK(S->pool.get(&key_end, ne)); SVXCHK(S->pool.get(&key_end2, ne)); SVXCHK(S->pool.get(&key_cs, ne)); SVXCHK(S->pool.get(&key_cs_g, ne)); SVXCHK(S->pool.get(&key_cs2, ne));
        k_bed_vcf_keys<<<BGRID(ne), BT, 0, st>>>(ne, in, key_end, key_cs, idx, line_form);
        SVXCHK(svx_sort_pairs_u64(c, key_end, key_end2, idx, v1, ne, 0, 32));
        k_bed_gather_u64<<<BGRID(ne), BT, 0, st>>>(key_cs, v1, key_cs_g, ne);
        SVXCHK(svx_sort_pairs_u64(c, key_cs_g, key_cs2, v1, line_row, ne, 0, std::min(64, 32 + std::max(1, svx_ceil_log2((long long)ip->n_contig + 1)))));
    } else {
        k_bed_entries<<<BGRID(ne), BT, 0, st>>>(ne, sl, line_row, line_form);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[2], st));
    // ---- 2: member piece lengths and their prefix, line lengths, offsets ----
    if (with_members) {
        int32_t* len; int64_t* pre;
        SVXCHK(S->pool.get(&len, nm + 1)); SVXCHK(S->pool.get(&pre, nm + 1));
        BedIn mi = in; mi.n_members = nm;
        k_bed_member_len<<<BGRID(nm + 1), BT, 0, st>>>(mi, len);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, len, pre, nm + 1));
        in.P = pre;
    }
    int64_t *line_len, *tiles, *tile_start;
    SVXCHK(S->pool.get(&line_len, ne + 1)); SVXCHK(S->pool.get(&tiles, ne + 1)); SVXCHK(S->pool.get(&tile_start, ne + 1));
    k_bed_lengths<<<BGRID(ne + 1), BT, 0, st>>>(ne, line_row, line_form, in, line_len, tiles);
    SVXCHK(svx_exclusive_scan_i64(c, line_len, line_off, ne + 1));
    SVXCHK(svx_exclusive_scan_i64(c, tiles, tile_start, ne + 1));
    k_bed_totals<<<1, 64, 0, st>>>(fl, line_off, tile_start + ne, in.err, in.counters, tot);
    HIPCHK(hipGetLastError());
    unsigned long long words[SVX_BED_MAX_FILES + 4];
    SVXCHK(svx_mail_read(c, st, tot, SVX_BED_MAX_FILES + 4, words));
    HIPCHK(hipEventRecord(S->ev[3], st));
    const auto check_err = [&](unsigned long long e) -> int {
        if (e & BERR_STD) return svx_fail(SVX_E_ARG, "svx_bed: a candidate's standard deviation is infinite or >= 1e10 (only values below are printed as Python prints them)", __FILE__, __LINE__, hipSuccess);
        if (e & BERR_INDEX) return svx_fail(SVX_E_ARG, "svx_bed: a contig, member, read id or type code lies outside its table", __FILE__, __LINE__, hipSuccess);
        if (e & BERR_HUGE) return svx_fail(SVX_E_CAPACITY, "svx_bed: a member list of more than 2^40 bytes", __FILE__, __LINE__, hipSuccess);
        if (e & BERR_OVERRUN) return svx_fail(SVX_E_STATE, "svx_bed: a line did not match its counted length (internal error)", __FILE__, __LINE__, hipSuccess);
        return SVX_OK;
    };
    SVXCHK(check_err(words[SVX_BED_MAX_FILES + 2]));
    const int64_t total_bytes = (int64_t)words[sl.n_files], total_tiles = (int64_t)words[SVX_BED_MAX_FILES + 1];
    if (total_tiles >= (1ll << 31)) return svx_fail(SVX_E_CAPACITY, "svx_bed: too many payload tiles", __FILE__, __LINE__, hipSuccess);
    {
        size_t free_b = 0, total_b = 0;
        const bool fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || (size_t)total_bytes + 64 <= S->out.cap || (size_t)total_bytes + (size_t)total_bytes / 8 + 512 + (size_t)ne * sizeof(BedSeg) < free_b + S->out.cap;
        if (!fits || S->out.reserve((size_t)total_bytes + 64) != SVX_OK) {
            (void)hipGetLastError();
            char msg[160]; snprintf(msg, sizeof msg, "svx_bed: the text of %lld bytes does not fit into device memory", (long long)total_bytes);
            return svx_fail(SVX_E_CAPACITY, msg, __FILE__, __LINE__, hipSuccess);
        }
    }
    uint8_t* out = S->out.as<uint8_t>();
    BedSeg* segs; SVXCHK(S->pool.get(&segs, (size_t)ne));
    // ---- 3: skeleton, payload ----
    k_bed_skeleton<<<BGRID(ne), BT, 0, st>>>(ne, line_row, line_form, in, line_off, out, segs);
    HIPCHK(hipEventRecord(S->ev[4], st));
    if (total_tiles > 0) k_bed_payload<<<(unsigned)((total_tiles + BT / 64 - 1) / (BT / 64)), BT, 0, st>>>((int)total_tiles, tile_start, ne, segs, in, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[5], st));
    { unsigned long long errw = 0; SVXCHK(svx_mail_read(c, st, in.err, 1, &errw)); SVXCHK(check_err(errw & 0xffffffffull)); }
    HIPCHK(hipEventRecord(S->ev[6], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    double* tp[5] = {&S->stats.t_upload_ms, &S->stats.t_entries_ms, &S->stats.t_lengths_ms, &S->stats.t_skeleton_ms, &S->stats.t_payload_ms};
    for (int k = 0; k < 5; k++) { (void)hipEventElapsedTime(&ms, S->ev[k], S->ev[k + 1]); *tp[k] = ms; }
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[6]); S->stats.t_total_ms = ms;
    S->stats.n_bytes = total_bytes; S->stats.n_tiles = total_tiles; S->stats.bytes_members = (int64_t)words[SVX_BED_MAX_FILES + 3];
    for (int k = 0; k <= sl.n_files; k++) S->file_off[k] = (int64_t)words[k];
    S->n_lines = n_lines; S->n_bytes = total_bytes; S->have = true;
    return SVX_OK;
}

extern "C" int svx_bed_count(svx_ctx* c, int32_t* n_files, int64_t* n_lines, int64_t* n_bytes) {
    if (!c || !c->bed || !c->bed->have) return svx_fail(SVX_E_STATE, "no BED text: run svx_bed first", __FILE__, __LINE__, hipSuccess);
    if (n_files) *n_files = c->bed->n_files;
    if (n_lines) *n_lines = c->bed->n_lines;
    if (n_bytes) *n_bytes = c->bed->n_bytes;
    return SVX_OK;
}

extern "C" int svx_bed_fetch(svx_ctx* c, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* file_off, int64_t* file_line_off, int64_t* line_off) {
    if (!c || !c->bed || !c->bed->have) return svx_fail(SVX_E_STATE, "no BED text: run svx_bed first", __FILE__, __LINE__, hipSuccess);
    BedState* S = c->bed;
    if (byte_offset < 0 || bytes < 0 || byte_offset + bytes > S->n_bytes || (bytes && !host_dst)) return svx_fail(SVX_E_ARG, "svx_bed_fetch: range outside the text", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    for (int k = 0; k <= S->n_files; k++) { if (file_off) file_off[k] = S->file_off[k]; if (file_line_off) file_line_off[k] = S->file_line[k]; }
    HostCopy hc(c->stream);
    if (bytes) SVXCHK(hc.d2h(host_dst, S->out.as<uint8_t>() + byte_offset, (size_t)bytes));
    if (line_off) SVXCHK(hc.d2h(line_off, S->line_off.p, (size_t)(S->n_lines + 1) * 8));
    SVXCHK(hc.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return SVX_OK;
}

bool svx_bed_text(svx_ctx* c, const uint8_t** text, int32_t* n_files, const int64_t** file_off_host) {
    if (!c->bed || !c->bed->have) return false;
    *text = c->bed->out.as<uint8_t>(); *n_files = c->bed->n_files; *file_off_host = c->bed->file_off;
    return true;
}

extern "C" int svx_bed_get_stats(svx_ctx* c, svx_bed_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->bed) *out = c->bed->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
