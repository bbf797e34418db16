// textgz_host.cpp - svx_text_gz_host: the encoder of deflate_core.hpp built for the host (the lane operations emulated), no GPU involved.  The bytes are those
// the kernels of textgz.hip write for the same text: sizes are measured, and zlib and the host builds of both decoders judge the stream, on a CPU.
#define DEF_HOST 1
#include "deflate_core.hpp"
#include "textgz_phase.hpp"
#include "../../include/svx.h"
#include <zlib.h>

static uint32_t host_crc(const uint8_t* p, uint32_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, n); }

extern "C" int svx_text_gz_host(const uint8_t* text, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (n < 0 || cap < 0 || (n && !text) || (cap && !out) || !n_out) return SVX_E_ARG;
    const int64_t got = def_file_host(text, n, out, cap, host_crc);
    if (got < 0) return SVX_E_CAPACITY;
    *n_out = got;
    return SVX_OK;
}

extern "C" int svx_text_gz_phase_host(int phase, int64_t n_blocks, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, uint32_t* tok, uint32_t* nt,
                                      uint32_t* hist, uint32_t* codes, uint8_t* slots) {
    return tgz_phase_host(phase, n_blocks, text, text_off, n, crc, tok, nt, hist, codes, slots) ? SVX_E_ARG : SVX_OK;
}
