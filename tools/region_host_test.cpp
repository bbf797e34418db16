// region_host_test.cpp - region reads (svx_bam_seek_region: svim_amd/csrc/bamio.cpp over region_core.hpp) under a seeded fuzz: seeded coordinate-sorted record
// streams cut into small BGZF blocks, seeded regions under both rules, read from a record start at or in front of the region's first kept record - through the
// host reader, and through the host side of the device reader (the chunk loader of bamio.cpp: dropped chunks, trimmed fronts, the stop) over the CPU stand-in of
// tools/bamio_fuzz.cpp - with chunks of 1, 2, 5 blocks and the default.  What comes back must be the run a plain scan gives: the records from the first kept one to
// the stop, the others of it marked SVX_FLAG_SKIP, and the counts of svx_bam_region_stats.  Meant for -fsanitize=address,undefined (tests/test_regions.py builds it
// so and runs it as a stand-alone child program).
//   region_host_test fuzz SEED FILES DIR   -> "FILES files, R region reads, K kept records, M marked records, 0 wrong"
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined svim_amd/csrc/bamio.cpp tools/region_host_test.cpp -lz -lpthread
#define BAMIO_FUZZ_NO_MAIN
#include "bamio_fuzz.cpp"

static uint64_t g_state;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }

struct Rec { int32_t tid, pos; uint16_t flag; uint32_t span; uint64_t at; };      // at: offset of the record in the stream
static const int N_REF = 4;

// a header of N_REF references and n records in coordinate order (now and then: no CIGAR, flag bit 4, clips and insertions only, an unplaced tail)
static std::vector<uint8_t> make_stream(int n, std::vector<Rec>& recs) {
    std::vector<uint8_t> raw = {'B', 'A', 'M', 1};
    put32(raw, 0); put32(raw, N_REF);
    for (int r = 0; r < N_REF; r++) { put32(raw, 3); raw.push_back('c'); raw.push_back((uint8_t)('0' + r)); raw.push_back(0); put32(raw, 1 << 20); }
    int32_t tid = (int32_t)(rnd() % 2), pos = (int32_t)(rnd() % 300);
    const int n_unplaced = (int)(rnd() % 4);
    for (int k = 0; k < n + n_unplaced; k++) {
        if (k >= n) { tid = -1; pos = -1; }
        else if (rnd() % 12 == 0 && tid < N_REF - 1) { tid += 1 + (int32_t)(rnd() % 2 && tid < N_REF - 2); pos = (int32_t)(rnd() % 300); }
        else pos += (int32_t)(rnd() % (rnd() % 5 == 0 ? 3000u : 60u));
        std::vector<uint32_t> cig;
        uint16_t flag = (uint16_t)((rnd() % 2 ? 16 : 0) | (rnd() % 9 == 0 ? 256 : 0));
        if (tid >= 0 && rnd() % 10) {
            const int ops = 1 + (int)(rnd() % 6);
            for (int c = 0; c < ops; c++) cig.push_back(((1 + rnd() % (rnd() % 6 == 0 ? 2000u : 90u)) << 4) | (uint32_t)("\0\1\2\3\4\7\10\0\2"[rnd() % 9]));
            if (rnd() % 8 == 0) for (auto& w : cig) w = (w & ~15u) | (rnd() % 2 ? 1u : 4u);      // no reference span at all
        }
        if (tid < 0 || rnd() % 15 == 0) flag |= 4;
        uint32_t span = 0, l_seq = 0;
        for (uint32_t w : cig) { if ((0x18Du >> (w & 15u)) & 1u) span += w >> 4; if ((0x193u >> (w & 15u)) & 1u) l_seq += w >> 4; }
        l_seq %= 50;                                                                 // (SEQ need not match the CIGAR for a reader)
        char name[16]; const int l_name = snprintf(name, sizeof name, "q%d", k / 2) + 1;
        recs.push_back(Rec{tid, pos, flag, span, (uint64_t)raw.size()});
        put32(raw, (uint32_t)(32 + l_name + 4 * cig.size() + (l_seq + 1) / 2 + l_seq));
        put32(raw, (uint32_t)tid); put32(raw, (uint32_t)pos);
        raw.push_back((uint8_t)l_name); raw.push_back((uint8_t)(rnd() % 61)); raw.push_back(0); raw.push_back(0);
        raw.push_back((uint8_t)cig.size()); raw.push_back(0); raw.push_back((uint8_t)flag); raw.push_back((uint8_t)(flag >> 8));
        put32(raw, l_seq); put32(raw, 0xffffffffu); put32(raw, 0xffffffffu); put32(raw, 0);
        raw.insert(raw.end(), name, name + l_name);
        for (uint32_t w : cig) put32(raw, w);
        for (uint32_t b = 0; b < (l_seq + 1) / 2 + l_seq; b++) raw.push_back((uint8_t)(0x11 * (1 + b % 8)));
    }
    return raw;
}

// the scan: stop, keep (the definition in words: svim_amd/regions.py), written out here and not taken from region_core.hpp
static bool scan_stops(const Rec& r, int32_t tid, int32_t end) { return r.tid < 0 || r.tid > tid || (r.tid == tid && r.pos >= end); }
static bool scan_keeps(const Rec& r, int32_t tid, int32_t beg, int32_t end, int rule) {
    if (r.tid != tid) return false;
    if (rule == SVX_REGION_START) return r.pos >= beg && r.pos < end;
    const int64_t lo = r.pos > 0 ? r.pos : 0, hi = (r.flag & 4) || r.span == 0 ? lo + 1 : lo + r.span;
    return lo < end && hi > beg;
}

int main(int argc, char** argv) {
    if (argc != 5 || strcmp(argv[1], "fuzz") != 0) { fprintf(stderr, "usage: %s fuzz SEED FILES DIR\n", argv[0]); return 2; }
    g_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)atoll(argv[2]);
    const long files = atol(argv[3]);
    const std::string path = std::string(argv[4]) + "/region_host_test.bam";
    long reads = 0, kept_total = 0, marked_total = 0, wrong = 0;
    for (long it = 0; it < files; it++) {
        std::vector<Rec> recs;
        const std::vector<uint8_t> raw = make_stream(20 + (int)(rnd() % 150), recs);
        const size_t block = 90 + rnd() % 700;
        const std::vector<uint8_t> file = bgzf_all(raw, block);
        FILE* f = fopen(path.c_str(), "wb");
        if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) { perror(path.c_str()); return 2; }
        fclose(f);
        std::vector<uint64_t> coff;                                                  // file offset of every block
        for (size_t at = 0; at + 18 <= file.size(); at += (size_t)(file[at + 16] | (file[at + 17] << 8)) + 1) coff.push_back(at);
        static const char* chunkings[] = {"1", "2", "5", nullptr};
        const char* cb = chunkings[it % 4];
        for (const char* var : {"SVX_BAM_CHUNK_BLOCKS", "SVX_BAM_DEV_CHUNK_BLOCKS"}) { if (cb) setenv(var, cb, 1); else unsetenv(var); }
        for (int device = 0; device < 2; device++) {
            svx_bam* h = nullptr;
            if (svx_bam_open(path.c_str(), 2, &h) != SVX_OK) { fprintf(stderr, "open: %s\n", svx_last_error()); return 2; }
            if (device && svx_bam_set_device_decode(h, 0) != SVX_OK) { fprintf(stderr, "device decode: %s\n", svx_last_error()); return 2; }
            for (int q = 0; q < 12; q++) {
                const int rule = (int)(rnd() % 2);
                const Rec& a = recs[rnd() % recs.size()];
                const int32_t tid = a.tid >= 0 ? a.tid : (int32_t)(rnd() % N_REF);
                const int32_t beg = (int32_t)std::max<int64_t>(0, (int64_t)a.pos + (int64_t)(rnd() % 400) - 200), end = beg + 1 + (int32_t)(rnd() % (rnd() % 3 ? 300u : 5000u));
                // expected: from a start at or in front of the first kept record (as an index gives it) the run [first kept, stop)
                size_t first = recs.size();
                for (size_t k = 0; k < recs.size() && first == recs.size(); k++) if (scan_keeps(recs[k], tid, beg, end, rule)) first = k;
                const size_t start = first == recs.size() ? rnd() % recs.size() : first - std::min<size_t>(first, rnd() % 9);
                size_t stop = start;
                while (stop < recs.size() && !scan_stops(recs[stop], tid, end)) stop++;
                size_t lo = start;
                while (lo < stop && !scan_keeps(recs[lo], tid, beg, end, rule)) lo++;
                const uint64_t voff = (coff[recs[start].at / block] << 16) | (recs[start].at % block);
                if (svx_bam_seek_region(h, voff, tid, beg, end, rule) != SVX_OK) { fprintf(stderr, "seek_region: %s\n", svx_last_error()); return 2; }
                size_t at = lo; long kept = 0, marked = 0; bool bad = false;
                for (;;) {
                    svx_batch b; int64_t n = 0;
                    if (svx_bam_read_batch(h, 1 + (int64_t)(rnd() % 40), 0, 20, &b, &n) != SVX_OK) { fprintf(stderr, "read: %s\n", svx_last_error()); return 2; }
                    if (n == 0) break;
                    for (int64_t i = 0; i < n; i++, at++) {
                        if (at >= stop) { bad = true; break; }
                        const bool keep = scan_keeps(recs[at], tid, beg, end, rule);
                        const uint16_t want = (uint16_t)((recs[at].flag & 0x0fff) | (keep ? 0 : SVX_FLAG_SKIP));
                        if (b.tid[i] != recs[at].tid || b.pos[i] != recs[at].pos || (uint16_t)(b.flag[i] & ~SVX_FLAG_SA) != want) bad = true;
                        kept += keep; marked += !keep;
                    }
                    if (bad) break;
                }
                struct svx_bam_region_stats st;
                svx_bam_region_stats(h, &st);
                if (bad || at != stop || st.n_kept != kept || st.n_marked != marked || st.n_seen != (int64_t)(stop - start)) {
                    wrong++;
                    fprintf(stderr, "file %ld %s chunk %s region (%d, %d, %d) rule %d from record %zu: run [%zu, %zu), got to %zu; stats seen %lld kept %lld marked %lld, scan %zu %ld %ld\n", it,
                            device ? "device loader" : "host reader", cb ? cb : "default", tid, beg, end, rule, start, lo, stop, at, (long long)st.n_seen, (long long)st.n_kept,
                            (long long)st.n_marked, stop - start, kept, marked);
                }
                reads++; kept_total += kept; marked_total += marked;
            }
            svx_bam_close(h);
        }
    }
    remove(path.c_str());
    printf("%ld files, %ld region reads, %ld kept records, %ld marked records, %ld wrong\n", files, reads, kept_total, marked_total, wrong);
    return wrong ? 1 : 0;
}
