// contig_core.hpp - reference name -> id: the open-addressing table the device reader builds from the header's dictionary, one source for whoever builds it
// (bamdev.hip: devdec_create; sam_host.cpp) and whoever reads it (bamdev.hip: the SA tags; sam_core.hpp: RNAME and RNEXT), on the host and on the device.
// key = FNV-1a of the name, mixed, | 1 (0 marks an empty slot); the table has at least four slots per name, so a probe always ends.
#pragma once
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CTG_FN __host__ __device__ inline
#else
#define CTG_FN static inline
#endif

CTG_FN uint64_t ctg_fnv(const uint8_t* p, uint32_t n, uint64_t seed) {
    uint64_t h = 0xcbf29ce484222325ull ^ seed;
    for (uint32_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return h;
}

struct ContigTable { const uint64_t* key; const int32_t* tid; uint32_t mask; const char* names; const uint32_t* name_off; };

// the id of a name, -1 when the dictionary does not hold it
CTG_FN int32_t ctg_lookup(const ContigTable& ct, const uint8_t* s, uint32_t n) {
    const uint64_t hk = ctg_fnv(s, n, 0) | 1ull;
    for (uint32_t q = (uint32_t)hk & ct.mask;; q = (q + 1u) & ct.mask) {
        const uint64_t k = ct.key[q];
        if (!k) return -1;
        if (k == hk) {
            const int32_t cand = ct.tid[q];
            const uint32_t o0 = ct.name_off[cand], o1 = ct.name_off[cand + 1];
            bool same = o1 - o0 == n;
            for (uint32_t c = 0; same && c < n; c++) same = (uint8_t)ct.names[o0 + c] == s[c];
            if (same) return cand;
        }
    }
}

// the table on the host, in the layout ContigTable reads; names_blob: n_ref names, NUL-separated, header order
struct ContigTableHost {
    std::vector<uint64_t> key; std::vector<int32_t> tid; std::vector<uint32_t> off; std::string blob; uint32_t mask = 0;
    void build(int32_t n_ref, const char* names_blob) {
        const size_t nr = (size_t)(n_ref > 0 ? n_ref : 1);
        uint32_t cap = 16; while (cap < 4u * (uint32_t)nr) cap <<= 1;
        key.assign(cap, 0); tid.assign(cap, -1); off.assign(nr + 1, 0); blob.clear();
        const char* p = names_blob;
        for (int32_t t = 0; t < n_ref; t++) {
            const size_t ln = strlen(p);
            off[(size_t)t] = (uint32_t)blob.size(); blob.append(p, ln);
            const uint64_t h = ctg_fnv(reinterpret_cast<const uint8_t*>(p), (uint32_t)ln, 0) | 1ull;
            uint32_t s = (uint32_t)h & (cap - 1);
            while (key[s]) s = (s + 1) & (cap - 1);
            key[s] = h; tid[s] = t;
            p += ln + 1;
        }
        off[(size_t)(n_ref > 0 ? n_ref : 0)] = (uint32_t)blob.size();
        mask = cap - 1;
    }
    ContigTable view() const { return ContigTable{key.data(), tid.data(), mask, blob.data(), off.data()}; }
};
