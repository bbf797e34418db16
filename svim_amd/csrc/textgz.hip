// textgz.hip - BGZF output on the device: a text resident in the context (the lines of svx_vcf or svx_bed, or uploaded bytes) -> a BGZF stream resident in the
// context (svx_text_gz*, include/svx.h).  The encoder is deflate_core.hpp (one source for these kernels and for svx_text_gz_host); this file is its launch:
//   k_tgz_crc      CRC32 of every block's text (crc32_wave.hpp: the arithmetic of the reader's k_crc32), stored
//   k_tgz_match    one wave per block: LZ77 tokens and histograms            \
//   k_tgz_codes    one wave per block: Huffman codes, headers, the size       >  in chunks of TGZ_CHUNK blocks (the tokens of a chunk live in one scratch buffer)
//   k_tgz_bits     one wave per block: the block written into its slot       /
//   scan of the sizes, k_tgz_compact: the slots copied into one dense stream (aligned words, the edges by bytes).
// Replaces: bgzip after the fact (the reference writes plain text, src/svim/SVIM_COMBINE.py:71-186, SVIM_CLUSTER.py:29-106; its users compress and index it).
// One workgroup = one wave: a block's table, histograms and staging window are private to it, so nothing is shared across waves and the order of lanes is the
// only order there is.  LDS: 17.3 KiB (match), 7 KiB (codes), 1.7 KiB (bits) per wave.
#include "common.hpp"
#include "hostcopy.hpp"
#include "textgz_kernels.hpp"
#include "textgz_phase.hpp"
#include <algorithm>

struct TextGzState {
    DevBuf text, blocks, crc, crc_shift, tok, hist, nt, codes, bsize, coff, kinds, slots, out;
    std::vector<int64_t> file_off_text, file_first_block, h_coff, h_uoff;
    int32_t n_files = 0; int64_t n_blocks = 0, n_bytes = 0;
    int source = -1; long long of_call = 0, gen = 0;
    bool have = false;
    hipEvent_t ev[10]; bool have_ev = false;
    svx_text_gz_stats stats;
};
void svx_textgz_release(svx_ctx* c) {
    TextGzState* s = c->textgz;
    if (!s) return;
    DevBuf* all[] = {&s->text, &s->blocks, &s->crc, &s->crc_shift, &s->tok, &s->hist, &s->nt, &s->codes, &s->bsize, &s->coff, &s->kinds, &s->slots, &s->out};
    for (auto* b : all) b->release();
    if (s->have_ev) for (auto& e : s->ev) (void)hipEventDestroy(e);
    delete s;
    c->textgz = nullptr;
}
static bool tgz_valid(svx_ctx* c) {
    const TextGzState* S = c ? c->textgz : nullptr;
    if (!S || !S->have) return false;
    return S->source == 2 || (S->source == 0 && S->of_call == c->vcf_calls) || (S->source == 1 && S->of_call == c->bed_calls);
}

extern "C" int svx_text_gz(svx_ctx* c, int source, const uint8_t* host_text, const int64_t* host_file_off, int32_t n_files) {
    if (!c || source < 0 || source > 2) return svx_fail(SVX_E_ARG, "svx_text_gz: bad argument (source 0, 1 or 2)", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    if (!c->textgz) { c->textgz = new TextGzState(); memset(&c->textgz->stats, 0, sizeof c->textgz->stats); }
    TextGzState* S = c->textgz;
    if (!S->have_ev) { for (auto& e : S->ev) HIPCHK(hipEventCreate(&e)); S->have_ev = true; }
    S->have = false; S->n_bytes = 0; S->n_blocks = 0; S->gen++;
    memset(&S->stats, 0, sizeof S->stats);
    hipStream_t st = c->stream;
    const uint8_t* text = nullptr;
    std::vector<int64_t>& fo = S->file_off_text;
    if (source == 0) {
        int64_t n = 0;
        if (!svx_vcf_text(c, &text, &n)) return svx_fail(SVX_E_STATE, "svx_text_gz: no VCF text: run svx_vcf first", __FILE__, __LINE__, hipSuccess);
        fo.assign({0, n}); S->of_call = c->vcf_calls;
    } else if (source == 1) {
        int32_t nf = 0; const int64_t* off = nullptr;
        if (!svx_bed_text(c, &text, &nf, &off)) return svx_fail(SVX_E_STATE, "svx_text_gz: no BED text: run svx_bed first", __FILE__, __LINE__, hipSuccess);
        fo.assign(off, off + nf + 1); S->of_call = c->bed_calls;
    } else {
        if (n_files < 1 || !host_file_off || host_file_off[0] != 0) return svx_fail(SVX_E_ARG, "svx_text_gz: source 2 needs at least one file and offsets that start at 0", __FILE__, __LINE__, hipSuccess);
        for (int32_t k = 0; k < n_files; k++) if (host_file_off[k + 1] < host_file_off[k]) return svx_fail(SVX_E_ARG, "svx_text_gz: host_file_off decreases", __FILE__, __LINE__, hipSuccess);
        if (host_file_off[n_files] > 0 && !host_text) return svx_fail(SVX_E_ARG, "svx_text_gz: the text is missing", __FILE__, __LINE__, hipSuccess);
        fo.assign(host_file_off, host_file_off + n_files + 1);
    }
    const int32_t nf = (int32_t)fo.size() - 1;
    const int64_t n_text = fo[nf];
    // the block table: every file's text in pieces of DEF_BLOCK bytes, then its end-of-file block (len 0)
    std::vector<TgzBlock> hb;
    S->h_uoff.clear(); S->file_first_block.assign((size_t)nf + 1, 0);
    for (int32_t k = 0; k < nf; k++) {
        S->file_first_block[k] = (int64_t)hb.size();
        for (int64_t at = fo[k]; at < fo[k + 1]; at += DEF_BLOCK) { hb.push_back(TgzBlock{(unsigned long long)at, (uint32_t)std::min<int64_t>(DEF_BLOCK, fo[k + 1] - at), 0u}); S->h_uoff.push_back(at); }
        hb.push_back(TgzBlock{(unsigned long long)fo[k + 1], 0u, 0u}); S->h_uoff.push_back(fo[k + 1]);
    }
    const long long nb = (long long)hb.size();
    S->file_first_block[nf] = nb; S->h_uoff.push_back(n_text);
    const long long chunk = std::min<long long>(nb, TGZ_CHUNK);
    {
        // what this call allocates at most, against what is free (buffers of an earlier call are reused)
        const size_t need = (source == 2 ? (size_t)n_text : 0) + (size_t)nb * DEF_SLOT + (size_t)n_text + (size_t)nb * 64 + (size_t)chunk * (DEF_BLOCK * 4 + sizeof(DefBlockCodes) + DEF_NHIST * 4);
        const size_t have = S->text.cap + S->slots.cap + S->out.cap + S->tok.cap;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + need / 8 + (1u << 20) > free_b + have) {
            char msg[160]; snprintf(msg, sizeof msg, "svx_text_gz: the working buffers of %lld blocks (%zu bytes) do not fit into device memory", nb, need);
            return svx_fail(SVX_E_CAPACITY, msg, __FILE__, __LINE__, hipSuccess);
        }
    }
    HIPCHK(hipEventRecord(S->ev[0], st));
    {
        HostCopy hc(st);
        if (source == 2) {
            SVXCHK(S->text.reserve((size_t)n_text + 64));
            if (n_text) SVXCHK(hc.h2d(S->text.p, host_text, (size_t)n_text));
            text = S->text.as<uint8_t>();
        }
        SVXCHK(S->blocks.reserve((size_t)nb * sizeof(TgzBlock)));
        SVXCHK(hc.h2d(S->blocks.p, hb.data(), (size_t)nb * sizeof(TgzBlock)));
        if (!S->crc_shift.p) {
            uint32_t m[CRC_POW][32];
            crc_shift_matrices(m);
            SVXCHK(S->crc_shift.reserve(sizeof m));
            SVXCHK(hc.h2d(S->crc_shift.p, m, sizeof m));
        }
        SVXCHK(hc.finish());
    }
    SVXCHK(S->crc.reserve((size_t)nb * 4)); SVXCHK(S->bsize.reserve((size_t)(nb + 1) * 8)); SVXCHK(S->coff.reserve((size_t)(nb + 1) * 8)); SVXCHK(S->kinds.reserve(64));
    SVXCHK(S->tok.reserve((size_t)chunk * DEF_BLOCK * 4)); SVXCHK(S->hist.reserve((size_t)chunk * DEF_NHIST * 4)); SVXCHK(S->nt.reserve((size_t)chunk * 4));
    SVXCHK(S->codes.reserve((size_t)chunk * sizeof(DefBlockCodes))); SVXCHK(S->slots.reserve((size_t)nb * DEF_SLOT));
    const TgzBlock* blocks = S->blocks.as<TgzBlock>();
    uint32_t *tok = S->tok.as<uint32_t>(), *hist = S->hist.as<uint32_t>(), *nt = S->nt.as<uint32_t>(), *crc = S->crc.as<uint32_t>();
    int64_t *bsize = S->bsize.as<int64_t>(), *coff = S->coff.as<int64_t>();
    unsigned long long* kinds = S->kinds.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(kinds, 0, 64, st));
    HIPCHK(hipMemsetAsync(bsize + nb, 0, 8, st));
    HIPCHK(hipEventRecord(S->ev[1], st));
    k_tgz_crc<<<(unsigned)nb, 64, 0, st>>>(text, blocks, nb, S->crc_shift.as<uint32_t>(), crc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[2], st));
    double t_phase[3] = {0, 0, 0};
    for (long long b0 = 0; b0 < nb; b0 += chunk) {
        const unsigned g = (unsigned)std::min<long long>(chunk, nb - b0);
        HIPCHK(hipEventRecord(S->ev[3], st));
        k_tgz_match<<<g, 64, 0, st>>>(text, blocks, b0, tok, hist, nt);
        HIPCHK(hipEventRecord(S->ev[4], st));
        k_tgz_codes<<<g, 64, 0, st>>>(blocks, b0, hist, crc, S->codes.as<DefBlockCodes>(), bsize, kinds);
        HIPCHK(hipEventRecord(S->ev[5], st));
        k_tgz_bits<<<g, 64, 0, st>>>(text, blocks, b0, tok, nt, S->codes.as<DefBlockCodes>(), S->slots.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S->ev[6], st));
        HIPCHK(hipEventSynchronize(S->ev[6]));          // (the next chunk reuses the token buffer and the events)
        for (int k = 0; k < 3; k++) { float ms = 0; (void)hipEventElapsedTime(&ms, S->ev[3 + k], S->ev[4 + k]); t_phase[k] += ms; }
    }
    HIPCHK(hipEventRecord(S->ev[7], st));
    SVXCHK(svx_exclusive_scan_i64(c, bsize, coff, nb + 1));
    S->h_coff.assign((size_t)nb + 1, 0);
    unsigned long long hk[3] = {0, 0, 0};
    {
        HostCopy hc(st);
        SVXCHK(hc.d2h(S->h_coff.data(), coff, (size_t)(nb + 1) * 8));
        SVXCHK(hc.d2h(hk, kinds, sizeof hk));
        SVXCHK(hc.finish());
    }
    const int64_t n_out = S->h_coff[nb];
    if (n_out < 28 * (int64_t)nf || n_out > (int64_t)nb * DEF_SLOT) return svx_fail(SVX_E_STATE, "svx_text_gz: the block sizes are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
    SVXCHK(S->out.reserve((size_t)n_out + 64));
    k_tgz_compact<<<(unsigned)nb, TGZ_CT, 0, st>>>(S->slots.as<uint8_t>(), coff, nb, S->out.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S->ev[8], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[1]); S->stats.t_upload_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[1], S->ev[2]); S->stats.t_crc_ms = ms;
    S->stats.t_matches_ms = t_phase[0]; S->stats.t_codes_ms = t_phase[1]; S->stats.t_bits_ms = t_phase[2];
    (void)hipEventElapsedTime(&ms, S->ev[7], S->ev[8]); S->stats.t_compaction_ms = ms;
    (void)hipEventElapsedTime(&ms, S->ev[0], S->ev[8]); S->stats.t_total_ms = ms;
    S->stats.n_files = nf; S->stats.n_blocks = nb; S->stats.blocks_eof = (int64_t)hk[DEF_KIND_EOF]; S->stats.blocks_stored = (int64_t)hk[DEF_KIND_STORED];
    S->stats.blocks_dynamic = (int64_t)hk[DEF_KIND_DYNAMIC]; S->stats.bytes_in = n_text; S->stats.bytes_out = n_out;
    S->n_files = nf; S->n_blocks = nb; S->n_bytes = n_out; S->source = source; S->have = true;
    return SVX_OK;
}

extern "C" int svx_text_gz_count(svx_ctx* c, int32_t* n_files, int64_t* n_blocks, int64_t* n_bytes) {
    if (!tgz_valid(c)) return svx_fail(SVX_E_STATE, "no BGZF stream: run svx_text_gz first (a later svx_vcf / svx_bed voids the stream of its text)", __FILE__, __LINE__, hipSuccess);
    if (n_files) *n_files = c->textgz->n_files;
    if (n_blocks) *n_blocks = c->textgz->n_blocks;
    if (n_bytes) *n_bytes = c->textgz->n_bytes;
    return SVX_OK;
}

extern "C" int svx_text_gz_fetch(svx_ctx* c, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* file_off, int64_t* block_coff, int64_t* block_uoff) {
    if (!tgz_valid(c)) return svx_fail(SVX_E_STATE, "no BGZF stream: run svx_text_gz first (a later svx_vcf / svx_bed voids the stream of its text)", __FILE__, __LINE__, hipSuccess);
    TextGzState* S = c->textgz;
    if (byte_offset < 0 || bytes < 0 || byte_offset + bytes > S->n_bytes || (bytes && !host_dst)) return svx_fail(SVX_E_ARG, "svx_text_gz_fetch: range outside the stream", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    if (file_off) for (int32_t k = 0; k <= S->n_files; k++) file_off[k] = S->h_coff[(size_t)S->file_first_block[k]];
    if (block_coff) memcpy(block_coff, S->h_coff.data(), (size_t)(S->n_blocks + 1) * 8);
    if (block_uoff) memcpy(block_uoff, S->h_uoff.data(), (size_t)(S->n_blocks + 1) * 8);
    if (bytes) {
        HostCopy hc(c->stream);
        SVXCHK(hc.d2h(host_dst, S->out.as<uint8_t>() + byte_offset, (size_t)bytes));
        SVXCHK(hc.finish());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SVX_OK;
}

// Test infrastructure (include/svx.h): one phase of the encoder over a batch of blocks, its inputs and results in host memory.  The kernels are the ones
// svx_text_gz launches, one wave per block, one launch; the buffers live for the call only and the context's stream of the last svx_text_gz is left alone.
extern "C" int svx_text_gz_phase(svx_ctx* c, int phase, int64_t nb, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, uint32_t* tok,
                                 uint32_t* nt, uint32_t* hist, uint32_t* codes, uint8_t* slots) {
    if (!c) return svx_fail(SVX_E_ARG, "svx_text_gz_phase: no context", __FILE__, __LINE__, hipSuccess);
    if (const char* bad = tgz_phase_check(phase, nb, text, text_off, n, crc, tok, nt, hist, codes, slots)) {
        char msg[200]; snprintf(msg, sizeof msg, "svx_text_gz_phase: %s", bad);
        return svx_fail(SVX_E_ARG, msg, __FILE__, __LINE__, hipSuccess);
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    struct Bufs { DevBuf text, blocks, crc, tok, hist, nt, codes, bsize, kinds, slots; ~Bufs() { for (DevBuf* b : {&text, &blocks, &crc, &tok, &hist, &nt, &codes, &bsize, &kinds, &slots}) b->release(); } } B;
    std::vector<TgzBlock> hb((size_t)nb);
    for (int64_t b = 0; b < nb; b++) hb[(size_t)b] = TgzBlock{(unsigned long long)(phase == TGZ_PHASE_CODES ? 0 : text_off[b]), n[b], 0u};
    const int64_t n_text = phase == TGZ_PHASE_CODES ? 0 : text_off[nb];
    const size_t tok_b = (size_t)nb * DEF_BLOCK * 4, hist_b = (size_t)nb * DEF_NHIST * 4, codes_b = (size_t)nb * sizeof(DefBlockCodes), slots_b = (size_t)nb * DEF_SLOT;
    SVXCHK(B.blocks.reserve((size_t)nb * sizeof(TgzBlock))); SVXCHK(B.text.reserve((size_t)n_text + 64)); SVXCHK(B.nt.reserve((size_t)nb * 4));
    {
        HostCopy hc(st);
        SVXCHK(hc.h2d(B.blocks.p, hb.data(), (size_t)nb * sizeof(TgzBlock)));
        if (n_text) SVXCHK(hc.h2d(B.text.p, text, (size_t)n_text));
        if (phase == TGZ_PHASE_CODES) {
            SVXCHK(B.hist.reserve(hist_b)); SVXCHK(B.crc.reserve((size_t)nb * 4));
            SVXCHK(hc.h2d(B.hist.p, hist, hist_b)); SVXCHK(hc.h2d(B.crc.p, crc, (size_t)nb * 4));
        }
        if (phase == TGZ_PHASE_BITS) {
            SVXCHK(B.tok.reserve(tok_b)); SVXCHK(B.codes.reserve(codes_b));
            SVXCHK(hc.h2d(B.tok.p, tok, tok_b)); SVXCHK(hc.h2d(B.nt.p, nt, (size_t)nb * 4)); SVXCHK(hc.h2d(B.codes.p, codes, codes_b));
        }
        SVXCHK(hc.finish());
    }
    if (phase == TGZ_PHASE_MATCH) {
        SVXCHK(B.tok.reserve(tok_b)); SVXCHK(B.hist.reserve(hist_b));
        HIPCHK(hipMemsetAsync(B.tok.p, 0, tok_b, st));
        k_tgz_match<<<(unsigned)nb, 64, 0, st>>>(B.text.as<uint8_t>(), B.blocks.as<TgzBlock>(), 0, B.tok.as<uint32_t>(), B.hist.as<uint32_t>(), B.nt.as<uint32_t>());
    } else if (phase == TGZ_PHASE_CODES) {
        SVXCHK(B.codes.reserve(codes_b)); SVXCHK(B.bsize.reserve((size_t)nb * 8)); SVXCHK(B.kinds.reserve(64));
        HIPCHK(hipMemsetAsync(B.codes.p, 0, codes_b, st));
        HIPCHK(hipMemsetAsync(B.kinds.p, 0, 64, st));
        k_tgz_codes<<<(unsigned)nb, 64, 0, st>>>(B.blocks.as<TgzBlock>(), 0, B.hist.as<uint32_t>(), B.crc.as<uint32_t>(), B.codes.as<DefBlockCodes>(), B.bsize.as<int64_t>(),
                                                 B.kinds.as<unsigned long long>());
    } else {
        SVXCHK(B.slots.reserve(slots_b));
        HIPCHK(hipMemsetAsync(B.slots.p, 0, slots_b, st));
        k_tgz_bits<<<(unsigned)nb, 64, 0, st>>>(B.text.as<uint8_t>(), B.blocks.as<TgzBlock>(), 0, B.tok.as<uint32_t>(), B.nt.as<uint32_t>(), B.codes.as<DefBlockCodes>(), B.slots.as<uint32_t>());
    }
    HIPCHK(hipGetLastError());
    {
        HostCopy hc(st);
        if (phase == TGZ_PHASE_MATCH) { SVXCHK(hc.d2h(tok, B.tok.p, tok_b)); SVXCHK(hc.d2h(nt, B.nt.p, (size_t)nb * 4)); SVXCHK(hc.d2h(hist, B.hist.p, hist_b)); }
        else if (phase == TGZ_PHASE_CODES) SVXCHK(hc.d2h(codes, B.codes.p, codes_b));
        else SVXCHK(hc.d2h(slots, B.slots.p, slots_b));
        SVXCHK(hc.finish());
    }
    HIPCHK(hipStreamSynchronize(st));
    return SVX_OK;
}

bool svx_textgz_view(svx_ctx* c, TextGzView* v) {
    if (!tgz_valid(c)) return false;
    TextGzState* S = c->textgz;
    int64_t n = 0; int32_t nf = 0; const int64_t* off = nullptr;
    if (S->source == 0) { if (!svx_vcf_text(c, &v->text, &n)) return false; }
    else if (S->source == 1) { if (!svx_bed_text(c, &v->text, &nf, &off)) return false; }
    else v->text = S->text.as<uint8_t>();
    v->n_files = S->n_files; v->n_blocks = S->n_blocks; v->gen = S->gen;
    v->file_off_text = S->file_off_text.data(); v->file_first_block = S->file_first_block.data();
    v->h_coff = S->h_coff.data(); v->h_uoff = S->h_uoff.data(); v->d_coff = S->coff.as<int64_t>();
    return true;
}

extern "C" int svx_text_gz_get_stats(svx_ctx* c, svx_text_gz_stats* out) {
    if (!c || !out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    if (c->textgz) *out = c->textgz->stats; else memset(out, 0, sizeof *out);
    return SVX_OK;
}
