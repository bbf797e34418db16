// textgz_kernels.hpp - the launchable phases of the BGZF encoder (deflate_core.hpp, crc32_wave.hpp), shared by the two streams that are encoded on the device:
// the text of svx_text_gz (textgz.hip) and the sorted BAM stream of svx_bam_sort_encode (bamsort.hip).  One workgroup = one wave = one block.  Every
// translation unit that includes this header gets kernels of its own (static): the launch code stays with its stream.
#pragma once
#include "common.hpp"
#include "crc32_wave.hpp"
#include "deflate_core.hpp"

#define TGZ_CHUNK 2048                      /* blocks per round of the three phases: 2048 x 255 KiB of tokens */
struct TgzBlock { unsigned long long at; uint32_t len, pad; };

static __global__ __launch_bounds__(64) void k_tgz_crc(const uint8_t* text, const TgzBlock* blocks, long long nb, const uint32_t* __restrict__ shift, uint32_t* crc) {
    __shared__ CrcTables S;
    crc32_wave_tables(S);
    const long long b = blockIdx.x;
    if (b >= nb) return;
    const TgzBlock j = blocks[b];
    const uint32_t v = j.len ? crc32_wave(text + j.at, (long long)j.len, shift, S) : 0u;
    if (lane_id() == 0) crc[b] = v;
}
// (b0: first block of the chunk; tokens, histograms and token counts are indexed by the block's place in the chunk)
static __global__ __launch_bounds__(64) void k_tgz_match(const uint8_t* text, const TgzBlock* blocks, long long b0, uint32_t* tok, uint32_t* hist, uint32_t* nt) {
    __shared__ DefMatchLds L;
    const TgzBlock j = blocks[b0 + blockIdx.x];
    if (j.len == 0u) { if (lane_id() == 0) nt[blockIdx.x] = 0u; return; }
    def_match(text + j.at, j.len, tok + (size_t)blockIdx.x * DEF_BLOCK, hist + (size_t)blockIdx.x * DEF_NHIST, nt + blockIdx.x, L);
}
static __global__ __launch_bounds__(64) void k_tgz_codes(const TgzBlock* blocks, long long b0, const uint32_t* hist, const uint32_t* crc, DefBlockCodes* codes, int64_t* bsize,
                                                   unsigned long long* kinds) {
    __shared__ DefCodesLds S;
    const long long b = b0 + blockIdx.x;
    DefBlockCodes* bc = codes + blockIdx.x;
    def_codes(hist + (size_t)blockIdx.x * DEF_NHIST, blocks[b].len, crc[b], bc, S);
    if (lane_id() == 0) { bsize[b] = (int64_t)bc->size; atomicAdd(kinds + bc->kind, 1ull); }
}
static __global__ __launch_bounds__(64) void k_tgz_bits(const uint8_t* text, const TgzBlock* blocks, long long b0, const uint32_t* tok, const uint32_t* nt, const DefBlockCodes* codes,
                                                  uint32_t* slots) {
    __shared__ DefBitsLds L;
    const long long b = b0 + blockIdx.x;
    const TgzBlock j = blocks[b];
    def_bits(text + j.at, j.len, tok + (size_t)blockIdx.x * DEF_BLOCK, nt[blockIdx.x], codes + blockIdx.x, slots + (size_t)b * (DEF_SLOT / 4), L);
}
// slot b, bsize bytes -> out[coff[b] ..): aligned words of the destination from unaligned reads of the slot, the bytes in front of and behind them one by one
#define TGZ_CT 256
static __global__ __launch_bounds__(TGZ_CT) void k_tgz_compact(const uint8_t* slots, const int64_t* coff, long long nb, uint8_t* out) {
    const long long b = blockIdx.x;
    if (b >= nb) return;
    const int64_t lo = coff[b], hi = coff[b + 1];
    const uint8_t* src = slots + (size_t)b * DEF_SLOT;
    const int64_t up = (lo + 3) & ~(int64_t)3, down = hi & ~(int64_t)3;
    const int64_t wlo = up < hi ? up : hi, whi = down > wlo ? down : wlo;
    for (int64_t p = lo + threadIdx.x; p < wlo; p += TGZ_CT) out[p] = src[p - lo];
    for (int64_t p = wlo + 4 * (int64_t)threadIdx.x; p < whi; p += 4 * TGZ_CT) *reinterpret_cast<uint32_t*>(out + p) = def_ld32(src + (p - lo));
    for (int64_t p = whi + threadIdx.x; p < hi; p += TGZ_CT) out[p] = src[p - lo];
}
