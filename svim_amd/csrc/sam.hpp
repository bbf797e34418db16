// sam.hpp - internal interface between the device reader (bamdev.hip) and the SAM text front end (sam.hip): a slice of SAM text made of whole lines goes in,
// the BAM record stream the reader's decode kernels consume and the offsets of its records come out, both in HBM.  The bytes: sam_core.hpp, svim_amd/sam.py.
#pragma once
#include "common.hpp"
#include "sam_core.hpp"
#include "../../include/svx.h"

struct SamDev;
int  samdev_create(SamDev** out);
void samdev_destroy(SamDev* s);
// host_text[0, n): whole alignment lines (the last one may lack its newline), n < 2^31.  line_base: lines of the file in front of the slice (for messages).
// ct: the reference-name table in device memory.  stream is (re)allocated to hold the records from byte 0 on, *stream_bytes of them, 256 zero bytes behind;
// rec_off gets n_rec + 1 offsets (uint64).  SVX_E_ARG / SVX_E_RANGE: a line is refused - svx_last_error names it by its number in the file.
int  samdev_convert(SamDev* s, const uint8_t* host_text, size_t n, int64_t line_base, const ContigTable& ct, DevBuf& stream, uint64_t* stream_bytes, DevBuf& rec_off, int64_t* n_rec,
                    hipStream_t st);
// where line `k` of the last slice starts in it (k <= its line count)
int  samdev_line_start(SamDev* s, int64_t k, uint64_t* at, hipStream_t st);
void samdev_stats(const SamDev* s, svx_sam_stats* out);
