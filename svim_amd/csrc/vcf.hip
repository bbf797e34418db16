// vcf.hip - the body of variants.vcf on the device: candidate table -> VCF lines (gfx950).
//
// Restates the entry loop, sorted_nicely and the id numbering of write_final_vcf (src/svim/SVIM_COMBINE.py:61-68, :139-184) and the nine get_vcf_entry*
// methods of src/svim/SVCandidate.py on the candidate table a svx_combine call left in the context (or one handed in).  Phases, all on the context's stream:
//   1  entries     one per candidate of an enabled class, two per breakend (forward, reverse), in the reference's append order DEL, INV, INS, DUP_TAN,
//                  DUP_INT, BND - the table is grouped by class, so an entry's index is a closed form of the class counts (no compaction needed);
//                  sort keys (natural contig rank, start, end) with start / end as the method's get_source() / get_destination() in 64 bits
//   2  order       two stable radix passes (end, then rank << 32 | start: svx_sort_pairs_u64), then the running index of every line among the lines of
//                  its ID label in sorted order: one more stable pass by label, the index is the position inside the label's run
//   3  distinct    SUPPORT = distinct reads among the members (and ZMWS = distinct zmw ids): (candidate << 32 | id) of the member list sorted once,
//                  adjacent difference, prefix sum read at the member offsets - no lane walks a member list
//   4  lengths     the line emitter run with a counting sink: line lengths and payload lengths -> int64 scans -> line offsets, payload tile offsets;
//                  the host reads the totals (mailbox) and allocates the text
//   5  skeleton    the same emitter with a writing sink: one lane per line stores the short fields (aligned 8-byte words where the line allows, single
//                  bytes at its edges) and leaves a descriptor (destination, length, kind, source) for each of the line's payloads
//      payload     one wave per tile of 1 KiB of ONE payload: reference range forward / reverse-complemented / repeated, member sequences, member names.
//                  A lane owns one 16-byte chunk at a 16-byte aligned destination: whole chunks leave as one dwordx4 store, the partial chunks at a payload's
//                  head and tail byte by byte.  A 100 kb allele spreads over 98 waves; a 40-base one costs one wave.
// What the host does in between: sizes between the phases (one mailbox read), the uploads of a handed-in table, of the genotype columns and of contig / read
// names and zmw ids when a switch asks for them.  The counting and the writing pass are ONE function template (emit_line) over two sinks, so a line's
// length and its bytes cannot disagree; the writing sink additionally refuses to leave its line.
#include "common.hpp"
#include "hostcopy.hpp"
#include "text_put.hpp"
#include <algorithm>
#include <cmath>

#define VT 256
#define VGRID(n) (unsigned)(((long long)(n) + VT - 1) / VT)
#define VCF_TILE 1024          /* payload bytes per wave: 64 lanes x one 16-byte chunk */
#define VCF_NSEG 4             /* payloads a line can have: REF, ALT, SEQS, READS */
#define VCF_NPOOL 96
#define VCF_STD_LIMIT 1e10

enum { F_DEL = 0, F_INV, F_INS, F_TAN_INS, F_TAN_DUP, F_INT_INS, F_INT_DUP, F_BND, F_BND_REV, F_NFORM };
enum { K_NONE = 0, K_FWD, K_REV, K_REP, K_SEQS, K_READS, K_NKIND };
enum { VERR_STD = 1, VERR_INDEX = 2, VERR_OVERRUN = 4, VERR_HUGE = 8 };

struct SegDesc { long long dst, len, a, b; int kind, pad; };
struct VcfSlots { long long base[7]; long long lo[6]; int form[6]; int two[6]; };      // the six append slots: first entry, first candidate row, method, entries per candidate - 1
struct VcfIn {
    long long n_cand, n_members, n_sig, n_reads;
    const uint8_t* cls; const int32_t *contig, *start, *end, *contig2, *start2, *end2; const uint8_t* aux; const int32_t* copies;
    const double *score, *std_span, *std_pos; const int64_t* member_off; const int32_t* members;
    const int32_t* sig_read_id; const int64_t* seq_off; const uint8_t* seq;
    const uint8_t* gt; const int32_t *ref_reads, *alt_reads;
    const char* cname; const int32_t* cname_off; const int32_t* cname_len; const int32_t* crank; int n_contig;
    const int32_t* cporder;                                   // position order only: a contig's place among the contigs sorted by (natural rank, index)
    const char* rname; const int64_t* rname_off; const int32_t* zmw;
    const int64_t* g_off; const uint8_t* g_codes; int g_n;
    const int64_t *sup_ex, *zmw_ex; const uint8_t* zbad;      // prefix sums of the 'new id' flags over the sorted member list; candidates with an invalid name
    const int64_t *pseq, *pread;                              // prefix sums of the member piece lengths (sequence + ',' / name + ',')
    svx_vcf_params P;
    int* err; unsigned long long* counters;
};

// ---------------------------------------------------------------------------------------------------------
// text helpers (host and device: svx_vcf_format_std runs the same code on the host)
// ---------------------------------------------------------------------------------------------------------
struct HostSink { char* out; int n; void ch(char c) { if (n < 31) out[n++] = c; } };

extern "C" int svx_vcf_format_std(double x, char out[32]) {
    if (!out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    HostSink s{out, 0};
    const bool ok = put_std(s, x);
    out[s.n] = 0;
    if (!ok) return svx_fail(SVX_E_ARG, "svx_vcf_format_std: |x| must be below 1e10", __FILE__, __LINE__, hipSuccess);
    return SVX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// device: sinks and the line emitter
// ---------------------------------------------------------------------------------------------------------
// 4-bit code -> letter of "=ACMGRSVTWYHKDBN" (two 8-byte tables in registers); comp: A<->T and C<->G swapped, every other letter unchanged (the inversion's
// complement dictionary, src/svim/SVCandidate.py:140)
__device__ __forceinline__ unsigned code_letter(unsigned code, bool comp) {
    const unsigned long long lo = comp ? 0x565352434d47543dull : 0x565352474d43413dull, hi = comp ? 0x4e42444b48595741ull : 0x4e42444b48595754ull;
    code &= 15u;
    return (unsigned)(((code < 8u ? lo : hi) >> (8u * (code & 7u))) & 0xffull);
}

struct CountSink {
    long long n = 0, seg0 = 0, seg1 = 0, seg2 = 0, seg3 = 0;
    int k0 = 0, k1 = 0;
    __device__ __forceinline__ void ch(char) { n++; }
    template <int SLOT> __device__ __forceinline__ void payload(int kind, long long, long long, long long len) {
        if (SLOT == 0) { seg0 = len; k0 = kind; } else if (SLOT == 1) { seg1 = len; k1 = kind; } else if (SLOT == 2) seg2 = len; else seg3 = len;
        n += len;
    }
};
// Bytes are gathered into a 64-bit word that leaves as ONE store when it fills an aligned 8 bytes of the output, byte by byte otherwise (a line's first and
// last bytes, the bytes next to a payload).  Nothing is stored outside [pos0, end): a disagreement with the counted length sets VERR_OVERRUN instead
struct WriteSink {
    uint8_t* base; long long pos, end; unsigned long long acc; int nacc; SegDesc* segs; int* err;
    __device__ __forceinline__ void flush() {
        if (nacc == 0) return;
        if (pos + nacc > end) { atomicOr(err, VERR_OVERRUN); acc = 0; nacc = 0; return; }
        if (nacc == 8) *reinterpret_cast<unsigned long long*>(base + pos) = acc;
        else for (int k = 0; k < nacc; k++) base[pos + k] = (uint8_t)(acc >> (8 * k));
        pos += nacc; acc = 0; nacc = 0;
    }
    __device__ __forceinline__ void ch(char c) {
        acc |= (unsigned long long)(uint8_t)c << (8 * nacc);
        nacc++;
        if (((pos + nacc) & 7) == 0) flush();
    }
    template <int SLOT> __device__ __forceinline__ void payload(int kind, long long a, long long b, long long len) {
        flush();
        SegDesc d; d.dst = pos; d.len = pos + len <= end ? len : 0; d.a = a; d.b = b; d.kind = kind; d.pad = 0;
        if (pos + len > end) atomicOr(err, VERR_OVERRUN);
        segs[SLOT] = d;
        pos += d.len;
    }
};

struct Range { long long a, len; };
// reference.fetch(contig, s, e) as the repo reads it: clipped to the contig, a contig the genome lacks has length 0
__device__ __forceinline__ Range ref_range(const VcfIn& in, int contig, long long s, long long e) {
    Range r; r.a = 0; r.len = 0;
    if (contig < 0 || contig >= in.g_n) return r;
    const long long o = in.g_off[contig], L = in.g_off[contig + 1] - o;
    if (s < 0) s = 0;
    if (s > L) s = L;
    if (e > L) e = L;
    if (e < s) e = s;
    r.a = o + s; r.len = e - s;
    return r;
}
template <class S> __device__ __forceinline__ void put_contig(S& s, const VcfIn& in, int c) {
    if (c < 0 || c >= in.n_contig) { atomicOr(in.err, VERR_INDEX); return; }
    const char* t = in.cname + in.cname_off[c];
    const int n = in.cname_len[c];
    for (int k = 0; k < n; k++) s.ch(t[k]);
}

// CHROM and POS as the line of method `form` for candidate row i prints them
__device__ __forceinline__ int line_contig(const VcfIn& in, int form, long long i) {
    return (form == F_INS || form == F_INT_INS || form == F_BND_REV) ? in.contig2[i] : in.contig[i];
}
__device__ __forceinline__ long long line_pos(const VcfIn& in, int form, long long i) {
    const long long s1 = in.start[i], s2 = in.start2[i];
    if (form == F_DEL) return s1 > 1 ? s1 : 1;
    if (form == F_INS || form == F_INT_INS) return s2 > 1 ? s2 : 1;
    if (form == F_BND_REV) return s2 + 1;
    return s1 + 1;
}
// one line.  form: the method (F_*), i: candidate row, k: the line's number among the lines of its label
template <class S> __device__ __forceinline__ void emit_line(S& s, const VcfIn& in, int form, long long i, long long k) {
    const int c1 = in.contig[i], c2 = in.contig2[i];
    const long long s1 = in.start[i], e1 = in.end[i], s2 = in.start2[i], e2 = in.end2[i], copies = in.copies[i];
    const unsigned aux = in.aux[i];
    const bool seq = in.P.sequence_alleles != 0;
    const long long m_lo = in.member_off[i], m_hi = in.member_off[i + 1];
    // CHROM, POS
    put_contig(s, in, line_contig(in, form, i)); s.ch('\t');
    put_i64(s, line_pos(in, form, i)); s.ch('\t');
    // ID
    put_str(s, "svim.");
    put_str(s, form == F_DEL ? "DEL" : form == F_INV ? "INV" : (form == F_INS || form == F_TAN_INS || form == F_INT_INS) ? "INS" : form == F_TAN_DUP ? "DUP_TANDEM"
               : form == F_INT_DUP ? "DUP_INT" : "BND");
    s.ch('.'); put_i64(s, k); s.ch('\t');
    // REF, ALT
    if (form == F_DEL && seq) {
        const long long p = s1 - 1 > 0 ? s1 - 1 : 0;
        const Range r = ref_range(in, c1, p, e1), a = ref_range(in, c1, p, s1);
        s.template payload<0>(K_FWD, r.a, 0, r.len); s.ch('\t');
        if (a.len > 0) s.ch((char)code_letter(in.g_codes[a.a], false));
    } else if (form == F_INV && seq) {
        const Range r = ref_range(in, c1, s1, e1);
        s.template payload<0>(K_FWD, r.a, 0, r.len); s.ch('\t');
        s.template payload<1>(K_REV, r.a, 0, r.len);
    } else if (form == F_TAN_INS && seq) {
        const Range r = ref_range(in, c1, s1, e1);
        s.template payload<0>(K_FWD, r.a, 0, r.len); s.ch('\t');
        const long long reps = copies + 1 > 0 ? copies + 1 : 0;
        s.template payload<1>(K_REP, r.a, r.len, r.len * reps);
    } else if (form == F_INT_INS && seq) {
        const long long p = s2 - 1 > 0 ? s2 - 1 : 0;
        const Range b = ref_range(in, c2, p, p + 1), r = ref_range(in, c1, s1, e1);
        const char base = b.len > 0 ? (char)code_letter(in.g_codes[b.a], false) : 0;
        if (base) s.ch(base);
        s.ch('\t');
        if (base) s.ch(base);
        s.template payload<1>(K_FWD, r.a, 0, r.len);
    } else {
        s.ch('N'); s.ch('\t');
        if (form == F_BND || form == F_BND_REV) {
            const bool src_rev = (aux & 1u) != 0, dst_rev = (aux & 2u) != 0;
            const bool n_first = form == F_BND ? !src_rev : dst_rev;
            const char br = (form == F_BND ? !dst_rev : src_rev) ? '[' : ']';
            if (n_first) s.ch('N');
            s.ch(br); put_contig(s, in, form == F_BND ? c2 : c1); s.ch(':'); put_i64(s, (form == F_BND ? s2 : s1) + 1); s.ch(br);
            if (!n_first) s.ch('N');
        } else {
            put_str(s, form == F_DEL ? "<DEL>" : form == F_INV ? "<INV>" : form == F_INS ? "<INS>" : form == F_TAN_INS ? "<DUP_TAN>" : form == F_TAN_DUP ? "<DUP:TANDEM>"
                       : form == F_INT_INS ? "<DUP_INT>" : "<DUP:INT>");
        }
    }
    s.ch('\t');
    // QUAL, FILTER
    put_i64(s, (long long)in.score[i]); s.ch('\t');
    const unsigned gt = in.gt[i];
    const bool hom_ref = gt == 1u, nfc = (form == F_TAN_INS || form == F_TAN_DUP) && !(aux & 1u);
    if (hom_ref) put_str(s, "hom_ref");
    if (hom_ref && nfc) s.ch(';');
    if (nfc) put_str(s, "not_fully_covered");
    if (!hom_ref && !nfc) put_str(s, "PASS");
    s.ch('\t');
    // INFO
    put_str(s, "SVTYPE=");
    put_str(s, form == F_DEL ? "DEL" : form == F_INV ? "INV" : (form == F_INS || form == F_TAN_INS || form == F_INT_INS) ? "INS" : form == F_TAN_DUP ? "DUP:TANDEM"
               : form == F_INT_DUP ? "DUP:INT" : "BND");
    if ((form == F_INT_INS || form == F_INT_DUP) && (aux & 1u)) put_str(s, ";CUTPASTE");
    if (form != F_BND && form != F_BND_REV) {
        put_str(s, ";END="); put_i64(s, (form == F_INS || form == F_INT_INS) ? s2 : e1);
        if (form != F_INV) {
            put_str(s, ";SVLEN=");
            put_i64(s, form == F_DEL ? s1 - e1 : (form == F_INS || form == F_INT_INS) ? e2 - s2 : form == F_TAN_INS ? copies * (e1 - s1) : e1 - s1);
        }
    }
    put_str(s, ";SUPPORT="); put_i64(s, in.sup_ex[m_hi] - in.sup_ex[m_lo]);
    bool ok = true;
    if (form == F_BND || form == F_BND_REV) {
        put_str(s, ";STD_POS1="); ok &= put_std(s, form == F_BND ? in.std_span[i] : in.std_pos[i]);
        put_str(s, ";STD_POS2="); ok &= put_std(s, form == F_BND ? in.std_pos[i] : in.std_span[i]);
    } else {
        put_str(s, ";STD_SPAN="); ok &= put_std(s, in.std_span[i]);
        put_str(s, ";STD_POS="); ok &= put_std(s, in.std_pos[i]);
    }
    if (!ok) atomicOr(in.err, VERR_STD);
    if (form == F_INS && in.P.insertion_sequences) {
        put_str(s, ";SEQS=");
        s.template payload<2>(K_SEQS, m_lo, m_hi, m_hi > m_lo ? in.pseq[m_hi] - in.pseq[m_lo] - 1 : 0);
    }
    if (in.P.read_names) {
        put_str(s, ";READS=");
        s.template payload<3>(K_READS, m_lo, m_hi, m_hi > m_lo ? in.pread[m_hi] - in.pread[m_lo] - 1 : 0);
    }
    if (in.P.zmws && !in.zbad[i]) { put_str(s, ";ZMWS="); put_i64(s, in.zmw_ex[m_hi] - in.zmw_ex[m_lo]); }
    s.ch('\t');
    // FORMAT, sample
    put_str(s, form == F_TAN_DUP ? "GT:CN:DP:AD" : "GT:DP:AD"); s.ch('\t');
    put_str(s, gt == 1u ? "0/0" : gt == 2u ? "0/1" : gt == 3u ? "1/1" : "./."); s.ch(':');
    if (form == F_TAN_DUP) { put_i64(s, copies + 1); s.ch(':'); }
    const long long rr = in.ref_reads[i], ar = in.alt_reads[i];
    if (rr >= 0 && ar >= 0) put_i64(s, rr + ar); else s.ch('.');
    s.ch(':');
    if (rr >= 0) put_i64(s, rr); else s.ch('.');
    s.ch(',');
    if (ar >= 0) put_i64(s, ar); else s.ch('.');
    s.ch('\n');
}

// ---------------------------------------------------------------------------------------------------------
// phase 1 / 2: entries, keys, label index
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int form_label(int form) {
    return form == F_DEL ? SVX_VCF_DEL : form == F_INV ? SVX_VCF_INV : (form == F_INS || form == F_TAN_INS || form == F_INT_INS) ? SVX_VCF_INS
           : form == F_TAN_DUP ? SVX_VCF_DUP_TANDEM : form == F_INT_DUP ? SVX_VCF_DUP_INT : SVX_VCF_BND;
}
__global__ void k_vcf_entries(long long n, VcfSlots sl, VcfIn in, uint32_t* ent_cand, uint8_t* ent_form, uint64_t* key_end, uint64_t* key_cs, uint32_t* idx) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int k = 0;
#pragma unroll
    for (int j = 1; j < 6; j++) k += e >= sl.base[j] ? 1 : 0;
    const long long r = e - sl.base[k];
    const long long i = sl.lo[k] + (sl.two[k] ? r >> 1 : r);
    const int form = sl.form[k] + ((sl.two[k] && (r & 1)) ? 1 : 0);
    int c; long long st, en;
    const long long s1 = in.start[i], e1 = in.end[i], s2 = in.start2[i], e2 = in.end2[i];
    if (form == F_INS || form == F_INT_INS) { c = in.contig2[i]; st = s2; en = e2; }
    else if (form == F_TAN_INS) { c = in.contig[i]; st = e1; en = e1 + (long long)in.copies[i] * (e1 - s1); }
    else if (form == F_BND) { c = in.contig[i]; st = s1; en = s1 + 1; }
    else if (form == F_BND_REV) { c = in.contig2[i]; st = s2; en = s2 + 1; }
    else { c = in.contig[i]; st = s1; en = e1; }
    unsigned rank = 0;
    if (c < 0 || c >= in.n_contig) atomicOr(in.err, VERR_INDEX); else rank = (unsigned)in.crank[c];
    ent_cand[e] = (uint32_t)i; ent_form[e] = (uint8_t)form; idx[e] = (uint32_t)e;
    key_end[e] = (uint64_t)en ^ (1ull << 63);
    key_cs[e] = ((uint64_t)rank << 32) | (uint64_t)((uint32_t)(int32_t)st ^ 0x80000000u);
}
__global__ void k_vcf_gather_u64(const uint64_t* src, const uint32_t* perm, uint64_t* dst, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}
__global__ void k_vcf_label_keys(long long n, const uint32_t* order, const uint8_t* ent_form, uint64_t* key, uint32_t* idx) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) { key[s] = (uint64_t)form_label(ent_form[order[s]]); idx[s] = (uint32_t)s; }
}
// position order (svx_vcf_position_order): (contig's place << 32 | POS) of the line at sorted position s, and the permutation applied to order and kidx
__global__ void k_vcf_pos_keys(long long n, const uint32_t* order, const uint32_t* ent_cand, const uint8_t* ent_form, VcfIn in, uint64_t* key, uint32_t* idx) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t e = order[s];
    const int form = ent_form[e]; const long long i = ent_cand[e];
    const int c = line_contig(in, form, i);
    const unsigned place = (c < 0 || c >= in.n_contig) ? 0u : (unsigned)in.cporder[c];       // (k_vcf_entries has raised VERR_INDEX for such a contig)
    key[s] = ((uint64_t)place << 32) | (uint64_t)((uint32_t)(int32_t)line_pos(in, form, i) ^ 0x80000000u);
    idx[s] = (uint32_t)s;
}
__global__ void k_vcf_permute_lines(long long n, const uint32_t* perm, const uint32_t* order, const int64_t* kidx, uint32_t* order2, int64_t* kidx2) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) { order2[p] = order[perm[p]]; kidx2[p] = kidx[perm[p]]; }
}
struct LabelBase { long long b[SVX_VCF_NLABEL]; };
__global__ void k_vcf_label_index(long long n, const uint64_t* key_sorted, const uint32_t* line_of, LabelBase lb, int64_t* kidx) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned lab = (unsigned)key_sorted[j];
    kidx[line_of[j]] = j - lb.b[lab < SVX_VCF_NLABEL ? lab : 0] + 1;
}

// ---------------------------------------------------------------------------------------------------------
// phase 3: distinct ids per candidate
// ---------------------------------------------------------------------------------------------------------
// candidate of member j: the last row whose member_off is <= j (rows without members are skipped by the upper bound)
__device__ __forceinline__ long long member_row(const int64_t* moff, long long n_cand, long long j) {
    long long lo = 0, hi = n_cand;                        // first row with moff[row + 1] > j
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (moff[mid + 1] > j) hi = mid; else lo = mid + 1; }
    return lo;
}
// mode 0: id = read id of the member; mode 1: id = zmw id of that read (-1 = 0xffffffff sorts last)
__global__ void k_vcf_member_keys(MemberIds in, int mode, uint64_t* key, uint32_t* idx) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= in.n_members) return;
    const long long row = member_row(in.member_off, in.n_cand, j);
    const long long m = in.members[j];
    uint32_t id = 0xfffffffeu;
    if (m < 0 || m >= in.n_sig) atomicOr(in.err, VERR_INDEX);
    else {
        const int r = in.sig_read_id[m];
        if (mode == 0) id = (uint32_t)r;
        else if (r < 0 || r >= in.n_reads) atomicOr(in.err, VERR_INDEX);
        else id = (uint32_t)in.zmw[r];
    }
    key[j] = ((uint64_t)row << 32) | id;
    idx[j] = (uint32_t)j;
}
__global__ void k_vcf_distinct_flags(long long n, const uint64_t* key, int mode, int32_t* flag, uint8_t* zbad) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { flag[j] = 0; return; }
    const uint64_t k = key[j];
    flag[j] = (j == 0 || key[j - 1] != k) ? 1 : 0;
    if (mode == 1 && (uint32_t)k == 0xffffffffu) zbad[k >> 32] = 1;
}

// ---------------------------------------------------------------------------------------------------------
// phase 4: member piece lengths, line lengths
// ---------------------------------------------------------------------------------------------------------
// mode 0: inserted sequence of the member + ','; mode 1: read name of the member + ','   (the last ',' of a candidate is never written)
__global__ void k_vcf_member_len(VcfIn in, int mode, int32_t* len) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > in.n_members) return;
    if (j == in.n_members) { len[j] = 0; return; }
    const long long m = in.members[j];
    long long l = 0;
    if (m < 0 || m >= in.n_sig) atomicOr(in.err, VERR_INDEX);
    else if (mode == 0) l = in.seq_off[m + 1] - in.seq_off[m];
    else {
        const int r = in.sig_read_id[m];
        if (r < 0 || r >= in.n_reads) atomicOr(in.err, VERR_INDEX); else l = in.rname_off[r + 1] - in.rname_off[r];
    }
    if (l < 0 || l >= (1ll << 30)) { atomicOr(in.err, VERR_INDEX); l = 0; }
    len[j] = (int32_t)l + 1;
}
__device__ __forceinline__ long long seg_tiles(long long len) { return len > 0 ? (len + 15 + VCF_TILE - 1) / VCF_TILE : 0; }      // whatever the destination's alignment turns out to be

__global__ __launch_bounds__(VT) void k_vcf_lengths(long long n, const uint32_t* order, const uint32_t* ent_cand, const uint8_t* ent_form, const int64_t* kidx, VcfIn in,
                                                    int64_t* line_len, int64_t* tiles) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    CountSink cs;
    if (s < n) {
        const uint32_t e = order[s];
        emit_line(cs, in, ent_form[e], ent_cand[e], kidx[s]);
        line_len[s] = cs.n;
        tiles[VCF_NSEG * s + 0] = seg_tiles(cs.seg0); tiles[VCF_NSEG * s + 1] = seg_tiles(cs.seg1);
        tiles[VCF_NSEG * s + 2] = seg_tiles(cs.seg2); tiles[VCF_NSEG * s + 3] = seg_tiles(cs.seg3);
        if ((cs.seg0 | cs.seg1 | cs.seg2 | cs.seg3) >> 40) atomicOr(in.err, VERR_HUGE);
    } else if (s == n) {
        line_len[s] = 0; tiles[VCF_NSEG * s] = 0;
    }
    // payload bytes by kind (statistics): one atomic per wave and kind
    const long long fwd = (cs.k0 == K_FWD ? cs.seg0 : 0) + (cs.k1 == K_FWD ? cs.seg1 : 0), rev = cs.k1 == K_REV ? cs.seg1 : 0, rep = cs.k1 == K_REP ? cs.seg1 : 0;
    const long long v[5] = {fwd, rev, rep, cs.seg2, cs.seg3};
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const long long t = wave_sum_i64(v[k]);
        if (lane_id() == 0 && t) atomicAdd(in.counters + k, (unsigned long long)t);
    }
}

// ---------------------------------------------------------------------------------------------------------
// phase 5: skeleton and payload
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT) void k_vcf_skeleton(long long n, const uint32_t* order, const uint32_t* ent_cand, const uint8_t* ent_form, const int64_t* kidx, VcfIn in,
                                                     const int64_t* line_off, uint8_t* out, SegDesc* segs) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    SegDesc none; none.dst = 0; none.len = 0; none.a = 0; none.b = 0; none.kind = K_NONE; none.pad = 0;
#pragma unroll
    for (int k = 0; k < VCF_NSEG; k++) segs[VCF_NSEG * s + k] = none;
    WriteSink ws; ws.base = out; ws.pos = line_off[s]; ws.end = line_off[s + 1]; ws.acc = 0; ws.nacc = 0; ws.segs = segs + VCF_NSEG * s; ws.err = in.err;
    const uint32_t e = order[s];
    emit_line(ws, in, ent_form[e], ent_cand[e], kidx[s]);
    ws.flush();
    if (ws.pos != ws.end) atomicOr(in.err, VERR_OVERRUN);
}

// One wave per tile.  Lane l of tile t of a payload owns the 16 bytes at the aligned address (dst & ~15) + 16 * (64 * t + l), cut to the payload.
__global__ __launch_bounds__(VT) void k_vcf_payload(int n_tiles, const int64_t* tile_start, long long n_seg, const SegDesc* segs, VcfIn in, uint8_t* out) {
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (VT / 64) + (threadIdx.x >> 6)));
    if (t >= n_tiles) return;
    long long lo = 0, hi = n_seg;                         // first payload with tile_start[g + 1] > t (wave-uniform: scalar loads)
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (tile_start[mid + 1] > t) hi = mid; else lo = mid + 1; }
    if (lo >= n_seg) return;
    const SegDesc d = segs[lo];
    if (d.len <= 0) return;
    const long long chunk = ((long long)t - tile_start[lo]) * 64 + lane_id();
    const long long a0 = (d.dst & ~15ll) + 16 * chunk;    // aligned address of this lane's chunk
    const long long w0 = a0 > d.dst ? a0 : d.dst, w1 = a0 + 16 < d.dst + d.len ? a0 + 16 : d.dst + d.len;
    if (w0 >= w1) return;
    const long long x0 = w0 - d.dst;
    const int nb = (int)(w1 - w0), q0 = (int)(w0 - a0);
    unsigned long long r0 = 0, r1 = 0;
#define PUT_BYTE(k_, b_) { const int q_ = q0 + (k_); const unsigned long long v_ = (unsigned long long)(b_); if (q_ < 8) r0 |= v_ << (8 * q_); else r1 |= v_ << (8 * (q_ - 8)); }
    if (d.kind == K_FWD) {
        const uint8_t* src = in.g_codes + d.a + x0;
        for (int k = 0; k < nb; k++) PUT_BYTE(k, code_letter(src[k], false));
    } else if (d.kind == K_REV) {
        const uint8_t* src = in.g_codes + d.a + (d.len - 1 - x0);
        for (int k = 0; k < nb; k++) PUT_BYTE(k, code_letter(src[-k], true));
    } else if (d.kind == K_REP) {
        long long r = d.b > 0 ? x0 % d.b : 0;
        for (int k = 0; k < nb; k++) { PUT_BYTE(k, code_letter(in.g_codes[d.a + r], false)); if (++r >= d.b) r = 0; }
    } else if (d.kind == K_SEQS || d.kind == K_READS) {
        const int64_t* P = d.kind == K_SEQS ? in.pseq : in.pread;
        const long long v = P[d.a] + x0;
        long long jl = d.a, jh = d.b;                     // the member whose piece holds virtual position v: first j with P[j + 1] > v
        while (jl < jh) { const long long mid = (jl + jh) >> 1; if (P[mid + 1] > v) jh = mid; else jl = mid + 1; }
        long long j = jl, tpos = v - P[j < d.b ? j : d.a];
        long long so = 0, sl = 0;
        const uint8_t* src = nullptr;
        bool load = true;
        for (int k = 0; k < nb; k++) {
            if (load) {
                so = 0; sl = 0; src = nullptr;
                if (j < d.b) {
                    const long long m = in.members[j];
                    if (m >= 0 && m < in.n_sig) {
                        if (d.kind == K_SEQS) { so = in.seq_off[m]; sl = in.seq_off[m + 1] - so; src = in.seq; }
                        else { const int r = in.sig_read_id[m]; if (r >= 0 && r < in.n_reads) { so = in.rname_off[r]; sl = in.rname_off[r + 1] - so; src = reinterpret_cast<const uint8_t*>(in.rname); } }
                    }
                    if (sl < 0 || sl >= (1ll << 30)) sl = 0;
                }
                load = false;
            }
            unsigned b = ',';
            if (tpos < sl && src) b = d.kind == K_SEQS ? code_letter(src[so + tpos], false) : src[so + tpos];
            PUT_BYTE(k, b);
            if (++tpos > sl) { j++; tpos = 0; load = true; }
        }
    }
#undef PUT_BYTE
    if (nb == 16) {
        ulonglong2 w; w.x = r0; w.y = r1;
        *reinterpret_cast<ulonglong2*>(out + a0) = w;
    } else {
        for (int k = 0; k < nb; k++) { const int q = q0 + k; out[a0 + q] = (uint8_t)((q < 8 ? r0 >> (8 * q) : r1 >> (8 * (q - 8))) & 0xffull); }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host: state and the call
// ---------------------------------------------------------------------------------------------------------
struct VcfState {
    ScratchPool<VCF_NPOOL> pool{"vcf"};
    DevBuf out, line_off;
    int64_t n_lines = 0, n_bytes = 0;
    bool have = false;
    hipEvent_t ev[8]; bool have_ev = false;
    svx_vcf_stats stats;
};
void svx_vcf_release(svx_ctx* c) {
    VcfState* s = c->vcf;
    if (!s) return;
    s->pool.release();
    s->out.release(); s->line_off.release();
    if (s->have_ev) for (auto& e : s->ev) (void)hipEventDestroy(e);
    delete s;
    c->vcf = nullptr;
}
void svx_preload_vcf() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_vcf_payload)); (void)hipGetLastError(); }

int svx_distinct_member_ids(svx_ctx* c, const MemberIds& m, int mode, const DistinctBufs& b, uint8_t* zbad) {
    const long long nm = m.n_members;
    hipStream_t st = c->stream;
    if (nm > 0) {
        k_vcf_member_keys<<<VGRID(nm), VT, 0, st>>>(m, mode, b.k0, b.v0);
        SVXCHK(svx_sort_pairs_u64(c, b.k0, b.k1, b.v0, b.v1, nm, 0, std::min(64, 32 + std::max(1, svx_ceil_log2(m.n_cand + 1)))));
    }
    k_vcf_distinct_flags<<<VGRID(nm + 1), VT, 0, st>>>(nm, b.k1, mode, b.flag, zbad);
    SVXCHK(svx_exclusive_scan_i32_to_i64(c, b.flag, b.ex, nm + 1));
    HIPCHK(hipGetLastError());
    return SVX_OK;
}
// prefix sums of the 'first occurrence' flags of (candidate, id) over the member list sorted by that pair -> ex[n_members + 1]
static int distinct_ids(svx_ctx* c, VcfState* S, const VcfIn& in, int mode, int64_t** ex_out, uint8_t* zbad) {
    const long long nm = in.n_members;
    DistinctBufs b;
    SVXCHK(S->pool.get(&b.k0, nm)); SVXCHK(S->pool.get(&b.k1, nm)); SVXCHK(S->pool.get(&b.v0, nm)); SVXCHK(S->pool.get(&b.v1, nm)); SVXCHK(S->pool.get(&b.flag, nm + 1)); SVXCHK(S->pool.get(&b.ex, nm + 1));
    *ex_out = b.ex;
    const MemberIds m{in.n_cand, nm, in.n_sig, in.n_reads, in.member_off, in.members, in.sig_read_id, in.zmw, in.err};
    return svx_distinct_member_ids(c, m, mode, b, zbad);
}

extern "C" int svx_vcf(svx_ctx* c, int source, const svx_candidate_view* cv, const svx_sig_view* sv, const svx_vcf_params* pp, const svx_vcf_inputs* ip) {
    if (!c || !pp || !ip || ip->n_contig < 0 || (ip->n_contig && (!ip->contig_names_nul_separated || !ip->contig_natural_rank)))
        return svx_fail(SVX_E_ARG, "svx_vcf: bad argument (parameters, inputs and the contig names are required)", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    if (!c->vcf) c->vcf = new VcfState();
    VcfState* S = c->vcf;
    if (!S->have_ev) { for (auto& e : S->ev) HIPCHK(hipEventCreate(&e)); S->have_ev = true; }
    S->pool.reset(); S->have = false; S->n_lines = S->n_bytes = 0;
    c->vcf_calls++;                    // (a BGZF stream made of the text before is void from here on)
    memset(&S->stats, 0, sizeof S->stats);
    const svx_vcf_params P = *pp;
    if (P.sequence_alleles && !c->g_off_p) return svx_fail(SVX_E_STATE, "svx_vcf: sequence alleles need a genome in the context (svx_set_genome / svx_genome_load_fasta)", __FILE__, __LINE__, hipSuccess);
    if ((P.read_names && (!ip->read_name_off || ip->n_reads < 0 || (ip->n_reads && !ip->read_names_blob))) || (P.zmws && (ip->n_reads < 0 || (ip->n_reads && !ip->zmw_id))))
        return svx_fail(SVX_E_ARG, "svx_vcf: read_names / zmws need the read names / zmw ids", __FILE__, __LINE__, hipSuccess);
    hipStream_t st = c->stream;
    HIPCHK(hipEventRecord(S->ev[0], st));
    VcfIn in; memset(&in, 0, sizeof in);
    in.P = P;
    int64_t class_count[SVX_NCAND];
    HostCopy hc(st);
#define UP(field, type, host, count) do { type* d_; SVXCHK(S->pool.get(&d_, (count))); if ((count)) SVXCHK(hc.h2d(d_, (host), (size_t)(count) * sizeof(type))); in.field = d_; } while (0)
    if (source == 0) {
        CandDev cd;
        if (!svx_combine_resident(c, &cd)) return svx_fail(SVX_E_STATE, "svx_vcf: no resident candidates: run svx_combine first", __FILE__, __LINE__, hipSuccess);
        if (!cd.from_resident || cd.cluster_call != c->cluster_calls || (cd.n_members > 0 && !c->last_cluster_read_id))
            return svx_fail(SVX_E_STATE, "svx_vcf: the signature table the resident candidates' members index is gone (svx_combine source 0 of the last svx_cluster is required)",
                            __FILE__, __LINE__, hipSuccess);
        in.n_cand = cd.n; in.n_members = cd.n_members; in.n_sig = c->last_cluster_source_n;
        in.cls = cd.cls; in.contig = cd.contig; in.start = cd.start; in.end = cd.end; in.contig2 = cd.contig2; in.start2 = cd.start2; in.end2 = cd.end2; in.aux = cd.aux;
        in.copies = cd.copies; in.score = cd.score; in.std_span = cd.std_span; in.std_pos = cd.std_pos; in.member_off = cd.member_off; in.members = cd.members;
        in.sig_read_id = c->last_cluster_read_id; in.seq_off = c->last_cluster_seq_off; in.seq = c->last_cluster_seq;
        for (int k = 0; k < SVX_NCAND; k++) class_count[k] = cd.class_count[k];
    } else if (source == 2) {
        if (!cv || !sv || sv->on_device || cv->n < 0 || cv->n_members < 0 || sv->n < 0) return svx_fail(SVX_E_ARG, "svx_vcf: source 2 needs a candidate table and signature columns in host memory", __FILE__, __LINE__, hipSuccess);
        const size_t n = (size_t)cv->n, nm = (size_t)cv->n_members, ns = (size_t)sv->n;
        int64_t total = 0;
        for (int k = 0; k < SVX_NCAND; k++) { class_count[k] = cv->class_count[k]; if (class_count[k] < 0) return svx_fail(SVX_E_ARG, "svx_vcf: negative class_count", __FILE__, __LINE__, hipSuccess); total += class_count[k]; }
        if (total != cv->n) return svx_fail(SVX_E_ARG, "svx_vcf: class_count does not add up to n", __FILE__, __LINE__, hipSuccess);
        if (n && (!cv->cls || !cv->contig || !cv->start || !cv->end || !cv->contig2 || !cv->start2 || !cv->end2 || !cv->aux || !cv->copies || !cv->score || !cv->std_span || !cv->std_pos))
            return svx_fail(SVX_E_ARG, "svx_vcf: a candidate column is missing", __FILE__, __LINE__, hipSuccess);
        if (!cv->member_off || (nm && !cv->members) || cv->member_off[0] != 0 || cv->member_off[n] != cv->n_members) return svx_fail(SVX_E_ARG, "svx_vcf: member_off does not describe n_members members", __FILE__, __LINE__, hipSuccess);
        for (size_t i = 0, k = 0, hi = (size_t)class_count[0]; i < n; i++) {
            while (k < SVX_NCAND && i >= hi) { k++; if (k < SVX_NCAND) hi += (size_t)class_count[k]; }
            if (k >= SVX_NCAND || cv->cls[i] != k) return svx_fail(SVX_E_ARG, "svx_vcf: the candidate table is not grouped by class as class_count says", __FILE__, __LINE__, hipSuccess);
            if (cv->member_off[i + 1] < cv->member_off[i]) return svx_fail(SVX_E_ARG, "svx_vcf: member_off decreases", __FILE__, __LINE__, hipSuccess);
        }
        if (ns && !sv->read_id) return svx_fail(SVX_E_ARG, "svx_vcf: the signatures' read_id column is missing", __FILE__, __LINE__, hipSuccess);
        if (P.insertion_sequences && (!sv->seq_off || (ns && sv->seq_off[ns] > 0 && !sv->seq))) return svx_fail(SVX_E_ARG, "svx_vcf: insertion_sequences needs seq_off and seq", __FILE__, __LINE__, hipSuccess);
        in.n_cand = cv->n; in.n_members = cv->n_members; in.n_sig = sv->n;
        UP(cls, uint8_t, cv->cls, n); UP(aux, uint8_t, cv->aux, n);
        UP(contig, int32_t, cv->contig, n); UP(start, int32_t, cv->start, n); UP(end, int32_t, cv->end, n);
        UP(contig2, int32_t, cv->contig2, n); UP(start2, int32_t, cv->start2, n); UP(end2, int32_t, cv->end2, n); UP(copies, int32_t, cv->copies, n);
        UP(score, double, cv->score, n); UP(std_span, double, cv->std_span, n); UP(std_pos, double, cv->std_pos, n);
        UP(member_off, int64_t, cv->member_off, n + 1); UP(members, int32_t, cv->members, nm);
        UP(sig_read_id, int32_t, sv->read_id, ns);
        if (P.insertion_sequences) { UP(seq_off, int64_t, sv->seq_off, ns + 1); UP(seq, uint8_t, sv->seq, (size_t)sv->seq_off[ns]); }
    } else return svx_fail(SVX_E_ARG, "svx_vcf: source must be 0 or 2", __FILE__, __LINE__, hipSuccess);
    const long long n = in.n_cand, nm = in.n_members;
    if (n >= (1ll << 30) || nm >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_vcf: table too large", __FILE__, __LINE__, hipSuccess);
    if (P.insertion_sequences && nm > 0 && !in.seq_off) return svx_fail(SVX_E_STATE, "svx_vcf: the resident signature table has no inserted sequences", __FILE__, __LINE__, hipSuccess);
    // genotype columns: the caller's, or - source 0, no column handed in, svx_vcf_use_resident_genotypes on - the ones svx_genotype_resident left for this table
    if (source == 0 && c->vcf_resident_gt && !ip->gt && !ip->ref_reads && !ip->alt_reads) {
        if (!svx_genotype_columns(c, n, &in.gt, &in.ref_reads, &in.alt_reads))
            return svx_fail(SVX_E_STATE, "svx_vcf: no resident genotypes for the resident candidates (svx_genotype_resident source 0 after the last svx_combine is required)",
                            __FILE__, __LINE__, hipSuccess);
    } else {
        uint8_t* gt; int32_t *rr, *ar;
        SVXCHK(S->pool.get(&gt, (size_t)n)); SVXCHK(S->pool.get(&rr, (size_t)n)); SVXCHK(S->pool.get(&ar, (size_t)n));
        if (n) {
            if (ip->gt) SVXCHK(hc.h2d(gt, ip->gt, (size_t)n)); else HIPCHK(hipMemsetAsync(gt, 0, (size_t)n, st));
            if (ip->ref_reads) SVXCHK(hc.h2d(rr, ip->ref_reads, (size_t)n * 4)); else HIPCHK(hipMemsetAsync(rr, 0xff, (size_t)n * 4, st));
            if (ip->alt_reads) SVXCHK(hc.h2d(ar, ip->alt_reads, (size_t)n * 4)); else HIPCHK(hipMemsetAsync(ar, 0xff, (size_t)n * 4, st));
        }
        in.gt = gt; in.ref_reads = rr; in.alt_reads = ar;
    }
    // contig names: offsets and lengths of the NUL-separated names
    {
        const int nc = ip->n_contig;
        std::vector<int32_t> off((size_t)nc + 1, 0), len((size_t)nc + 1, 0);
        size_t at = 0;
        for (int k = 0; k < nc; k++) {
            const size_t l = strlen(ip->contig_names_nul_separated + at);
            if (at + l + 1 >= (1ull << 31)) return svx_fail(SVX_E_ARG, "svx_vcf: contig names too long", __FILE__, __LINE__, hipSuccess);
            off[k] = (int32_t)at; len[k] = (int32_t)l; at += l + 1;
        }
        UP(cname, char, ip->contig_names_nul_separated, at); UP(cname_off, int32_t, off.data(), (size_t)nc + 1); UP(cname_len, int32_t, len.data(), (size_t)nc + 1);
        UP(crank, int32_t, ip->contig_natural_rank, (size_t)nc);
        std::vector<int32_t> by_rank((size_t)nc), place((size_t)nc + 1, 0);
        for (int k = 0; k < nc; k++) by_rank[k] = k;
        std::stable_sort(by_rank.begin(), by_rank.end(), [&](int32_t a, int32_t b) { return ip->contig_natural_rank[a] < ip->contig_natural_rank[b]; });
        for (int k = 0; k < nc; k++) place[by_rank[k]] = k;
        UP(cporder, int32_t, place.data(), (size_t)nc);
        in.n_contig = nc;
        SVXCHK(hc.finish());               // (the vectors leave scope)
    }
    in.n_reads = (P.read_names || P.zmws) ? ip->n_reads : 0;
    if (P.read_names) {
        const size_t nr = (size_t)ip->n_reads;
        if (ip->read_name_off[0] != 0) return svx_fail(SVX_E_ARG, "svx_vcf: read_name_off[0] must be 0", __FILE__, __LINE__, hipSuccess);
        for (size_t r = 0; r < nr; r++) if (ip->read_name_off[r + 1] < ip->read_name_off[r]) return svx_fail(SVX_E_ARG, "svx_vcf: read_name_off decreases", __FILE__, __LINE__, hipSuccess);
        UP(rname_off, int64_t, ip->read_name_off, nr + 1); UP(rname, char, ip->read_names_blob, (size_t)ip->read_name_off[nr]);
    }
    if (P.zmws) UP(zmw, int32_t, ip->zmw_id, (size_t)ip->n_reads);
    SVXCHK(hc.finish());
#undef UP
    in.g_off = c->g_off_p; in.g_codes = c->g_codes_p; in.g_n = P.sequence_alleles ? c->g_n : 0;
    { int* err; unsigned long long* cnt; SVXCHK(S->pool.get(&err, 2)); SVXCHK(S->pool.get(&cnt, 8)); HIPCHK(hipMemsetAsync(err, 0, 8, st)); HIPCHK(hipMemsetAsync(cnt, 0, 64, st)); in.err = err; in.counters = cnt; }
    HIPCHK(hipEventRecord(S->ev[1], st));

    // ---- 1: the six append slots (SVIM_COMBINE.py:145-173) over the class-grouped table ----
    int64_t cls_lo[SVX_NCAND + 1]; cls_lo[0] = 0;
    for (int k = 0; k < SVX_NCAND; k++) cls_lo[k + 1] = cls_lo[k] + class_count[k];
    const bool tan_ins = P.tandem_duplications_as_insertions != 0, int_ins = P.interspersed_duplications_as_insertions != 0;
    const int slot_cls[6] = {SVX_CAND_DEL, SVX_CAND_INV, SVX_CAND_INS, SVX_CAND_DUP_TAN, SVX_CAND_DUP_INT, SVX_CAND_BND};
    const int slot_form[6] = {F_DEL, F_INV, F_INS, tan_ins ? F_TAN_INS : F_TAN_DUP, int_ins ? F_INT_INS : F_INT_DUP, F_BND};
    const int slot_label[6] = {SVX_VCF_DEL, SVX_VCF_INV, SVX_VCF_INS, tan_ins ? SVX_VCF_INS : SVX_VCF_DUP_TANDEM, int_ins ? SVX_VCF_INS : SVX_VCF_DUP_INT, SVX_VCF_BND};
    VcfSlots sl; memset(&sl, 0, sizeof sl);
    long long n_lines = 0; int64_t per_label[SVX_VCF_NLABEL] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 6; k++) {
        const bool on = ((P.types_mask >> slot_label[k]) & 1u) != 0;
        const long long cnt = on ? class_count[slot_cls[k]] * (k == 5 ? 2 : 1) : 0;
        sl.base[k] = n_lines; sl.lo[k] = cls_lo[slot_cls[k]]; sl.form[k] = slot_form[k]; sl.two[k] = k == 5 ? 1 : 0;
        n_lines += cnt; per_label[slot_label[k]] += cnt;
    }
    sl.base[6] = n_lines;
    // base[j] of an empty slot equals the next one's: the kernel's count of 'e >= base[j]' then skips it, as it must
    if (n_lines >= (1ll << 31)) return svx_fail(SVX_E_ARG, "svx_vcf: too many lines", __FILE__, __LINE__, hipSuccess);
    S->stats.n_candidates = n; S->stats.n_lines = n_lines;
    for (int k = 0; k < SVX_VCF_NLABEL; k++) S->stats.lines_per_label[k] = per_label[k];
    SVXCHK(S->line_off.reserve((size_t)(n_lines + 2) * 8));
    int64_t* line_off = S->line_off.as<int64_t>();
    if (n_lines == 0) {
        HIPCHK(hipMemsetAsync(line_off, 0, 8, st));
        HIPCHK(hipEventRecord(S->ev[7], st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0; (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[7]); S->stats.t_total_ms = ms;
        (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]); S->stats.t_upload_ms = ms;
        S->have = true;
        return SVX_OK;
    }
    const long long ne = n_lines;
    uint32_t *ent_cand, *idx, *v1, *order, *v3; uint8_t* ent_form; uint64_t *key_end, *key_end2, *key_cs, *key_cs_g, *key_cs2, *lab, *lab2; int64_t* kidx;
    SVXCHK(S->pool.get(&ent_cand, ne)); SVXCHK(S->pool.get(&idx, ne)); SVXCHK(S->pool.get(&v1, ne)); SVXCHK(S->pool.get(&order, ne)); SVXCHK(S->pool.get(&v3, ne)); SVXCHK(S->pool.get(&ent_form, ne));
    SVXCHK(S->pool.get(&key_end, ne)); SVXCHK(S->pool.get(&key_end2, ne)); SVXCHK(S->pool.get(&key_cs, ne)); SVXCHK(S->pool.get(&key_cs_g, ne)); SVXCHK(S->pool.get(&key_cs2, ne));
    SVXCHK(S->pool.get(&lab, ne)); SVXCHK(S->pool.get(&lab2, ne)); SVXCHK(S->pool.get(&kidx, ne));
    k_vcf_entries<<<VGRID(ne), VT, 0, st>>>(ne, sl, in, ent_cand, ent_form, key_end, key_cs, idx);
    // ---- 2: stable sort by (rank, start, end); running index per label ----
    SVXCHK(svx_sort_pairs_u64(c, key_end, key_end2, idx, v1, ne, 0, 64));
    k_vcf_gather_u64<<<VGRID(ne), VT, 0, st>>>(key_cs, v1, key_cs_g, ne);
    SVXCHK(svx_sort_pairs_u64(c, key_cs_g, key_cs2, v1, order, ne, 0, std::min(64, 32 + std::max(1, svx_ceil_log2((long long)ip->n_contig + 1)))));
    k_vcf_label_keys<<<VGRID(ne), VT, 0, st>>>(ne, order, ent_form, lab, idx);
    SVXCHK(svx_sort_pairs_u64(c, lab, lab2, idx, v3, ne, 0, 3));
    LabelBase lb; { long long b = 0; for (int k = 0; k < SVX_VCF_NLABEL; k++) { lb.b[k] = b; b += per_label[k]; } }
    k_vcf_label_index<<<VGRID(ne), VT, 0, st>>>(ne, lab2, v3, lb, kidx);
    if (c->vcf_position_order) {
        // the ids are given; one more stable pass by (contig, POS) - lines that tie keep the reference's order
        uint64_t *pk, *pk2; uint32_t *pv, *perm, *order2; int64_t* kidx2;
        SVXCHK(S->pool.get(&pk, ne)); SVXCHK(S->pool.get(&pk2, ne)); SVXCHK(S->pool.get(&pv, ne)); SVXCHK(S->pool.get(&perm, ne)); SVXCHK(S->pool.get(&order2, ne)); SVXCHK(S->pool.get(&kidx2, ne));
        k_vcf_pos_keys<<<VGRID(ne), VT, 0, st>>>(ne, order, ent_cand, ent_form, in, pk, pv);
        SVXCHK(svx_sort_pairs_u64(c, pk, pk2, pv, perm, ne, 0, std::min(64, 32 + std::max(1, svx_ceil_log2((long long)ip->n_contig + 1)))));
        k_vcf_permute_lines<<<VGRID(ne), VT, 0, st>>>(ne, perm, order, kidx, order2, kidx2);
        order = order2; kidx = kidx2;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[2], st));
    // ---- 3: distinct reads / zmws per candidate ----
    {
        int64_t* ex; uint8_t* zbad;
        SVXCHK(S->pool.get(&zbad, (size_t)n + 1));
        HIPCHK(hipMemsetAsync(zbad, 0, (size_t)n + 1, st));
        SVXCHK(distinct_ids(c, S, in, 0, &ex, zbad)); in.sup_ex = ex;
        if (P.zmws) { SVXCHK(distinct_ids(c, S, in, 1, &ex, zbad)); in.zmw_ex = ex; }
        in.zbad = zbad;
    }
    HIPCHK(hipEventRecord(S->ev[3], st));
    // ---- 4: member piece offsets, line lengths, offsets ----
    for (int mode = 0; mode < 2; mode++) {
        if (!(mode == 0 ? P.insertion_sequences : P.read_names)) continue;
        int32_t* len; int64_t* pre;
        SVXCHK(S->pool.get(&len, nm + 1)); SVXCHK(S->pool.get(&pre, nm + 1));
        k_vcf_member_len<<<VGRID(nm + 1), VT, 0, st>>>(in, mode, len);
        SVXCHK(svx_exclusive_scan_i32_to_i64(c, len, pre, nm + 1));
        if (mode == 0) in.pseq = pre; else in.pread = pre;
    }
    const long long n_seg = ne * VCF_NSEG;
    int64_t *line_len, *tiles, *tile_start;
    SVXCHK(S->pool.get(&line_len, ne + 1)); SVXCHK(S->pool.get(&tiles, n_seg + 1)); SVXCHK(S->pool.get(&tile_start, n_seg + 1));
    k_vcf_lengths<<<VGRID(ne + 1), VT, 0, st>>>(ne, order, ent_cand, ent_form, kidx, in, line_len, tiles);
    SVXCHK(svx_exclusive_scan_i64(c, line_len, line_off, ne + 1));
    SVXCHK(svx_exclusive_scan_i64(c, tiles, tile_start, n_seg + 1));
    HIPCHK(hipGetLastError());
    int64_t total_bytes = 0, total_tiles = 0; unsigned long long words[6] = {0, 0, 0, 0, 0, 0};      // 5 counters + the error word
    static_assert(sizeof(unsigned long long) == 8, "");
    {
        // the error word sits behind the counters in memory of its own: gather the three pieces in one mailbox read
        unsigned long long cnt5[5]; unsigned long long errw = 0;
        SVXCHK(svx_mail_read3(c, st, line_off + ne, 1, &total_bytes, tile_start + n_seg, 1, &total_tiles, in.counters, 5, cnt5));
        SVXCHK(svx_mail_read(c, st, in.err, 1, &errw));
        for (int k = 0; k < 5; k++) words[k] = cnt5[k];
        words[5] = errw & 0xffffffffull;
    }
    HIPCHK(hipEventRecord(S->ev[4], st));
    const auto check_err = [&](unsigned long long e) -> int {
        if (e & VERR_STD) return svx_fail(SVX_E_ARG, "svx_vcf: a standard deviation is infinite or >= 1e10 (only values below are printed as Python prints them)", __FILE__, __LINE__, hipSuccess);
        if (e & VERR_INDEX) return svx_fail(SVX_E_ARG, "svx_vcf: a contig, member or read id lies outside its table", __FILE__, __LINE__, hipSuccess);
        if (e & VERR_HUGE) return svx_fail(SVX_E_CAPACITY, "svx_vcf: an allele of more than 2^40 bytes", __FILE__, __LINE__, hipSuccess);
        if (e & VERR_OVERRUN) return svx_fail(SVX_E_STATE, "svx_vcf: a line did not match its counted length (internal error)", __FILE__, __LINE__, hipSuccess);
        return SVX_OK;
    };
    SVXCHK(check_err(words[5]));
    if (total_tiles >= (1ll << 31)) return svx_fail(SVX_E_CAPACITY, "svx_vcf: too many payload tiles", __FILE__, __LINE__, hipSuccess);
    {
        size_t free_b = 0, total_b = 0;
        const bool fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || (size_t)total_bytes + 64 <= S->out.cap || (size_t)total_bytes + (size_t)total_bytes / 8 + 512 + (size_t)n_seg * sizeof(SegDesc) < free_b + S->out.cap;
        if (!fits || S->out.reserve((size_t)total_bytes + 64) != SVX_OK) {
            (void)hipGetLastError();
            char msg[160]; snprintf(msg, sizeof msg, "svx_vcf: the text of %lld bytes does not fit into device memory", (long long)total_bytes);
            return svx_fail(SVX_E_CAPACITY, msg, __FILE__, __LINE__, hipSuccess);
        }
    }
    uint8_t* out = S->out.as<uint8_t>();
    SegDesc* segs; SVXCHK(S->pool.get(&segs, (size_t)n_seg));
    // ---- 5: skeleton, payload ----
    k_vcf_skeleton<<<VGRID(ne), VT, 0, st>>>(ne, order, ent_cand, ent_form, kidx, in, line_off, out, segs);
    HIPCHK(hipEventRecord(S->ev[5], st));
    if (total_tiles > 0) k_vcf_payload<<<(unsigned)((total_tiles + VT / 64 - 1) / (VT / 64)), VT, 0, st>>>((int)total_tiles, tile_start, n_seg, segs, in, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[6], st));
    { unsigned long long errw = 0; SVXCHK(svx_mail_read(c, st, in.err, 1, &errw)); SVXCHK(check_err(errw & 0xffffffffull)); }
    HIPCHK(hipEventRecord(S->ev[7], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    double* tp[7] = {&S->stats.t_upload_ms, &S->stats.t_entries_ms, &S->stats.t_distinct_ms, &S->stats.t_lengths_ms, &S->stats.t_skeleton_ms, &S->stats.t_payload_ms, nullptr};
    for (int k = 0; k < 6; k++) { (void)hipEventElapsedTime(&ms, S->ev[k], S->ev[k + 1]); *tp[k] = ms; }
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[7]); S->stats.t_total_ms = ms;
    S->stats.n_bytes = total_bytes; S->stats.n_tiles = total_tiles;
    S->stats.bytes_ref_forward = (int64_t)words[0]; S->stats.bytes_ref_revcomp = (int64_t)words[1]; S->stats.bytes_ref_repeat = (int64_t)words[2];
    S->stats.bytes_seqs = (int64_t)words[3]; S->stats.bytes_reads = (int64_t)words[4];
    S->n_lines = n_lines; S->n_bytes = total_bytes; S->have = true;
    return SVX_OK;
}

extern "C" int svx_vcf_use_resident_genotypes(svx_ctx* c, int on) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    c->vcf_resident_gt = on != 0;
    return SVX_OK;
}

extern "C" int svx_vcf_position_order(svx_ctx* c, int on) {
    if (!c) return svx_fail(SVX_E_ARG, "null context", __FILE__, __LINE__, hipSuccess);
    c->vcf_position_order = on != 0;
    return SVX_OK;
}

extern "C" int svx_vcf_count(svx_ctx* c, int64_t* n_lines, int64_t* n_bytes) {
    if (!c || !c->vcf || !c->vcf->have) return svx_fail(SVX_E_STATE, "no VCF text: run svx_vcf first", __FILE__, __LINE__, hipSuccess);
    if (n_lines) *n_lines = c->vcf->n_lines;
    if (n_bytes) *n_bytes = c->vcf->n_bytes;
    return SVX_OK;
}

extern "C" int svx_vcf_fetch(svx_ctx* c, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* line_off) {
    if (!c || !c->vcf || !c->vcf->have) return svx_fail(SVX_E_STATE, "no VCF text: run svx_vcf first", __FILE__, __LINE__, hipSuccess);
    VcfState* S = c->vcf;
    if (byte_offset < 0 || bytes < 0 || byte_offset + bytes > S->n_bytes || (bytes && !host_dst)) return svx_fail(SVX_E_ARG, "svx_vcf_fetch: range outside the text", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    HostCopy hc(c->stream);
    if (bytes) SVXCHK(hc.d2h(host_dst, S->out.as<uint8_t>() + byte_offset, (size_t)bytes));
    if (line_off) SVXCHK(hc.d2h(line_off, S->line_off.p, (size_t)(S->n_lines + 1) * 8));
    SVXCHK(hc.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return SVX_OK;
}

bool svx_vcf_text(svx_ctx* c, const uint8_t** text, int64_t* n_bytes) {
    if (!c->vcf || !c->vcf->have) return false;
    *text = c->vcf->out.as<uint8_t>(); *n_bytes = c->vcf->n_bytes;
    return true;
}

extern "C" int svx_vcf_get_stats(svx_ctx* c, svx_vcf_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->vcf) *out = c->vcf->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
