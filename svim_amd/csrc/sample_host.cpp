// sample_host.cpp - svx_sample_used_host: one window of the consumption table of cluster.hip by sample_core.hpp built for the host; no GPU involved.
// method 0 is the per-start walk (k_sample_tables), method 1 the backward sweep (k_sample_sweep): the same table.
#include "sample_core.hpp"
#include "../../include/svx.h"

extern "C" int svx_sample_used_host(const uint32_t* stream, int64_t cap, int32_t n, int64_t lo, int32_t width, int32_t method, int32_t chunk, int32_t margin,
                                    uint16_t* out) {
    if (!stream || !out || cap < 0 || n <= SAMPLE_DRAWS || n > 1045 || lo < 0 || width < 1 || (method != 0 && method != 1)) return SVX_E_ARG;
    if (method == 0) {
        for (int32_t s = 0; s < width; s++) out[s] = sample_walk(n, lo + s, cap, [&](long long p) { return stream[p]; });
        return SVX_OK;
    }
    if (chunk == 0 && margin == 0) { chunk = SAMPLE_SWEEP_C; margin = SAMPLE_SWEEP_M; }
    if (chunk < 1 || chunk > 16384 || margin < 0 || margin > 16384) return SVX_E_ARG;
    sample_sweep_host(stream, cap, n, lo, width, chunk, margin, out);
    return SVX_OK;
}
