// fmtrepr.hip - repr(float) entry points: the host forms (no GPU needed) and the device form, all over fmt_repr.hpp.
//
// The multiplier tables are generated once per process on the host (repr_build_tables) and uploaded once per context for the kernels (svx_repr_device_tables:
// 10.7 KB in global memory, read through the scalar / vector caches; bed.hip formats the score and deviation columns with the same copy).
#include "common.hpp"
#include "hostcopy.hpp"
#include "fmt_repr.hpp"
#include <mutex>

static uint64_t g_repr_tab[REPR_TABLE_WORDS];
static std::once_flag g_repr_once;
const uint64_t* svx_repr_host_tables() {
    std::call_once(g_repr_once, [] { repr_build_tables(g_repr_tab); });
    return g_repr_tab;
}
int svx_repr_device_tables(svx_ctx* c, const uint64_t** out) {
    if (!c->repr_tab_ready) {
        SVXCHK(c->repr_tab.reserve(sizeof g_repr_tab));
        SVXCHK(svx_h2d(c->repr_tab.p, svx_repr_host_tables(), sizeof g_repr_tab, c->stream));
        c->repr_tab_ready = true;
    }
    *out = c->repr_tab.as<uint64_t>();
    return SVX_OK;
}

struct ReprHostSink { char* out; int n; void ch(char c) { if (n < 31) out[n++] = c; } };

extern "C" int svx_format_repr(double x, char out[32]) {
    if (!out) return svx_fail(SVX_E_ARG, "null argument", __FILE__, __LINE__, hipSuccess);
    ReprHostSink s{out, 0};
    put_repr(s, x, svx_repr_host_tables());
    memset(out + s.n, 0, (size_t)(32 - s.n));
    return SVX_OK;
}

extern "C" int svx_format_repr_many(int64_t n, const double* x, char* out) {
    if (n < 0 || (n && (!x || !out))) return svx_fail(SVX_E_ARG, "svx_format_repr_many: bad argument", __FILE__, __LINE__, hipSuccess);
    const uint64_t* tab = svx_repr_host_tables();
    for (int64_t i = 0; i < n; i++) {
        ReprHostSink s{out + 32 * i, 0};
        put_repr(s, x[i], tab);
        memset(out + 32 * i + s.n, 0, (size_t)(32 - s.n));
    }
    return SVX_OK;
}

// one lane per value: the text gathers in a 64-bit word that leaves as one store when full; every lane writes the four words of its 32-byte slot
struct ReprSlotSink {
    unsigned long long* dst; unsigned long long acc; int nacc, w;
    __device__ __forceinline__ void ch(char c) {
        acc |= (unsigned long long)(uint8_t)c << (8 * nacc);
        if (++nacc == 8) { if (w < 4) dst[w] = acc; w++; acc = 0; nacc = 0; }
    }
    __device__ __forceinline__ void finish() { for (; w < 4; w++) { dst[w] = acc; acc = 0; } }
};
__global__ __launch_bounds__(256) void k_format_repr(long long n, const double* x, const uint64_t* tab, unsigned long long* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ReprSlotSink s; s.dst = out + 4 * i; s.acc = 0; s.nacc = 0; s.w = 0;
    put_repr(s, x[i], tab);
    s.finish();
}

extern "C" int svx_format_repr_device(svx_ctx* c, int64_t n, const double* host_x, char* host_out) {
    if (!c || n < 0 || n >= (1ll << 31) || (n && (!host_x || !host_out))) return svx_fail(SVX_E_ARG, "svx_format_repr_device: bad argument", __FILE__, __LINE__, hipSuccess);
    if (n == 0) return SVX_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t* tab;
    SVXCHK(svx_repr_device_tables(c, &tab));
    DevBuf xin, text;
    int rc = xin.reserve((size_t)n * 8);
    if (rc == SVX_OK) rc = text.reserve((size_t)n * 32);
    if (rc == SVX_OK) rc = svx_h2d(xin.p, host_x, (size_t)n * 8, c->stream);
    if (rc == SVX_OK) {
        k_format_repr<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(n, xin.as<double>(), tab, text.as<unsigned long long>());
        if (hipGetLastError() != hipSuccess) rc = svx_fail(SVX_E_HIP, "k_format_repr launch", __FILE__, __LINE__, hipSuccess);
    }
    if (rc == SVX_OK) rc = svx_d2h(host_out, text.p, (size_t)n * 32, c->stream);
    (void)hipStreamSynchronize(c->stream);
    xin.release(); text.release();
    return rc;
}
