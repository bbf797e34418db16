// bam_merge_session_test.cpp - the life cycle of a merge session (svx_bam_merge_*: the host logic in svim_amd/csrc/bamio.cpp) and of the readers that feed it,
// walked in every order on the CPU.  bamio.cpp and bamsort_host.cpp are the library's; the device side is a stand-in: the decoder of tools/bamio_fuzz.cpp (chunk
// slots, a loader thread per chunk) and, below, a model of the sort (BamSort), of what it ends as for either owner (SortOut) and of the session's device side
// (MergeDev) that keeps appended records in host memory and sorts with std::stable_sort.  The model POISONS what it frees and COUNTS owners and borrowers: a sort destroyed twice, used after its destruction,
// dropped or destroyed while a decoder still borrows it, or appended to by a decoder that does not hold it, ends the program with a message even where the
// allocator would forgive it.  Meant for -fsanitize=address,undefined (with LeakSanitizer) and, in a second build, -fsanitize=thread: appends run on the loader
// threads bamio.cpp starts, the feed is set and cleared on the caller's.  tests/test_bam_merge_session.py builds both and runs them as stand-alone programs.
//   bam_merge_session_test DIR [light]   -> "S scenarios, A adds, F injected failures, R reader sorts, 0 wrong"      (light: a sample of the orders)
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. svim_amd/csrc/bamio.cpp svim_amd/csrc/bamsort_host.cpp
//        tools/bam_merge_session_test.cpp -lz -lpthread
#define BAMIO_FUZZ_NO_MAIN
#define BAMIO_FUZZ_SORT_MODEL
#include "bamio_fuzz.cpp"
#include "../svim_amd/csrc/bamsort_core.hpp"
#include <algorithm>
#include <atomic>
#include <mutex>

[[noreturn]] static void model_die(const char* what) { fprintf(stderr, "OWNERSHIP: %s\n", what); fflush(stderr); abort(); }

// ---- the model of the sort -------------------------------------------------------------------------------------------------------------------------------
enum : uint32_t { MODEL_ALIVE = 0x534f5254u, MODEL_DEAD = 0xdeadbeefu };
struct ModelRow { uint64_t key; size_t slab, off, len; };
struct BamSort {
    uint32_t magic = MODEL_ALIVE;
    std::atomic<int> borrowers{0};                           // decoders whose feed points here
    int32_t n_ref = 0; int64_t max_bytes = 0, arena = 0;
    std::vector<std::vector<uint8_t>*> slabs; std::vector<ModelRow> rows; int bad = 0;
    bool begun = false, finished = false, have_piece = false;
    std::vector<uint8_t> stream, piece; std::vector<uint32_t> perm;
};
static std::mutex g_grave_m;
static std::vector<BamSort*> g_grave;                        // destroyed models stay allocated (and poisoned) to the end: a later touch finds MODEL_DEAD
static std::atomic<long long> g_appends{0};                  // appends to SESSION sorts since the counter was reset
static std::atomic<long long> g_fail_at{-1}; static int g_fail_code = SVX_E_CAPACITY;      // failure injection: the append with this number fails
static std::atomic<long long> g_own_appends{0}, g_own_fail_at{-1};                         // the same for a reader's own sort

static BamSort* model_alive(BamSort* S, const char* where) {
    if (!S) model_die(where);
    if (S->magic != MODEL_ALIVE) { fprintf(stderr, "in %s: ", where); model_die(S->magic == MODEL_DEAD ? "a sort was used after its destruction" : "not a sort"); }
    return S;
}
static void model_drop(BamSort* S) {
    if (!S) return;
    model_alive(S, "drop");
    if (S->borrowers.load() != 0) model_die("a sort was dropped while a reader still feeds it");
    for (auto* v : S->slabs) { memset(v->data(), 0xDD, v->size()); delete v; }
    S->slabs.clear(); S->rows.clear(); S->bad = 0; S->arena = 0; S->begun = S->finished = S->have_piece = false;
    std::vector<uint8_t>().swap(S->stream); std::vector<uint8_t>().swap(S->piece); std::vector<uint32_t>().swap(S->perm);
}
static void model_begin(BamSort** s, int64_t max_bytes, int32_t n_ref) {
    if (!*s) *s = new BamSort();
    model_drop(*s);
    (*s)->n_ref = n_ref; (*s)->max_bytes = max_bytes; (*s)->begun = true;
}
static void model_destroy(BamSort* S) {
    if (!S) return;
    if (S->magic == MODEL_DEAD) model_die("a sort was destroyed twice");
    model_alive(S, "destroy");
    if (S->borrowers.load() != 0) model_die("a sort was destroyed while a reader still feeds it");
    model_drop(S);
    S->magic = MODEL_DEAD; S->n_ref = -0x22222222; S->max_bytes = -1;
    std::lock_guard<std::mutex> g(g_grave_m);
    g_grave.push_back(S);
}
// the records of a loaded slot: what bamsort_append does with a BamSortChunk (bamsort.hip), record by record
static int model_append(BamSort* S, const MockSlot& slot, const uint64_t* rec, size_t n_rec, const int32_t* map, int32_t n_ref_file, bool identity, bool session) {
    model_alive(S, "append");
    if (!S->begun || S->finished) { g_svx_err = "model: append to a sort that is not open"; return SVX_E_ARG; }
    if (n_rec == 0) return SVX_OK;
    if (session ? g_fail_at.load() == g_appends++ : g_own_fail_at.load() == g_own_appends++) { g_svx_err = "model: injected failure"; return session ? g_fail_code : SVX_E_CAPACITY; }
    const uint64_t first = rec[0], end = slot.tail_start;
    if (S->max_bytes > 0 && S->arena + (int64_t)(end - first) > S->max_bytes) { g_svx_err = "model: the arena is full"; return SVX_E_CAPACITY; }
    auto* slab = new std::vector<uint8_t>(slot.stream->begin() + (long)first, slot.stream->begin() + (long)end);
    S->slabs.push_back(slab); S->arena += (int64_t)slab->size();
    const bool translated = n_ref_file >= 0 && !identity;
    for (size_t i = 0; i < n_rec; i++) {
        uint8_t* r = slab->data() + (rec[i] - first);
        const uint32_t bs = m32(r);
        int32_t tid = slot.tid[i]; const int32_t pos = slot.pos[i];
        int32_t n_check = n_ref_file >= 0 ? n_ref_file : S->n_ref;
        if (translated && bs >= BSORT_MIN_BLOCK_SIZE) {
            int32_t t, mt;
            S->bad |= bsort_translate(tid, (int32_t)m32(r + BSORT_MATE_AT), map, n_ref_file, &t, &mt);
            for (int k = 0; k < 4; k++) { r[BSORT_REFID_AT + k] = (uint8_t)((uint32_t)t >> (8 * k)); r[BSORT_MATE_AT + k] = (uint8_t)((uint32_t)mt >> (8 * k)); }
            tid = t; n_check = S->n_ref;
        }
        S->bad |= bsort_check(tid, pos, bs, n_check);
        S->rows.push_back(ModelRow{bsort_key(tid, pos, slot.flag[i], S->n_ref), S->slabs.size() - 1, (size_t)(rec[i] - first), 4 + (size_t)bs});
    }
    return SVX_OK;
}
static int model_finish(BamSort* S, const uint8_t* header, int64_t n) {
    model_alive(S, "finish");
    if (!S->begun || S->finished) { g_svx_err = "model: finish of a sort that is not open"; return SVX_E_ARG; }
    if (S->borrowers.load() != 0) model_die("a sort was finished while a reader still feeds it");
    if (bsort_status(S->bad)) { g_svx_err = "model: a record the definition refuses"; return bsort_status(S->bad); }
    std::vector<uint32_t> order(S->rows.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return S->rows[a].key < S->rows[b].key; });
    S->stream.assign(header, header + n);
    for (uint32_t i : order) { const ModelRow& R = S->rows[i]; const uint8_t* p = S->slabs[R.slab]->data() + R.off; S->stream.insert(S->stream.end(), p, p + R.len); }
    S->perm = order; S->finished = true;
    return SVX_OK;
}
static int64_t model_blocks(const BamSort* S) { return ((int64_t)S->stream.size() + BSORT_BLOCK - 1) / BSORT_BLOCK + 1; }
static void model_count(BamSort* S, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks) {
    model_alive(S, "count");
    if (n_records) *n_records = (int64_t)S->rows.size();
    if (stream_bytes) *stream_bytes = (int64_t)S->stream.size();
    if (n_blocks) *n_blocks = model_blocks(S);
}
// (no compression here: a piece's "compressed" bytes are its stream bytes)
static int model_encode(BamSort* S, int64_t first, int64_t nb, int64_t* n_bytes) {
    model_alive(S, "encode");
    if (!S->finished) return SVX_E_STATE;
    if (first < 0 || nb < 1 || first > model_blocks(S) - nb) return SVX_E_ARG;
    const int64_t total = (int64_t)S->stream.size(), lo = std::min(first * BSORT_BLOCK, total), hi = std::min((first + nb) * BSORT_BLOCK, total);
    S->piece.assign(S->stream.begin() + lo, S->stream.begin() + hi); S->have_piece = true;
    if (n_bytes) *n_bytes = hi - lo;
    return SVX_OK;
}
static int model_fetch(BamSort* S, uint8_t* a, uint8_t* b) {
    model_alive(S, "fetch");
    if (!S->finished || !S->have_piece) return SVX_E_STATE;
    if (a && !S->piece.empty()) memcpy(a, S->piece.data(), S->piece.size());
    if (b && !S->piece.empty()) memcpy(b, S->piece.data(), S->piece.size());
    return SVX_OK;
}
static int model_permutation(BamSort* S, uint32_t* perm) {
    model_alive(S, "permutation");
    if (!S->finished) return SVX_E_STATE;
    if (perm && !S->perm.empty()) memcpy(perm, S->perm.data(), S->perm.size() * 4);
    return SVX_OK;
}

// ---- what a sort ends as, whoever owns it (devdec.hpp: sortout_*): the model, directly ------------------------------------------------------------------------
struct SortOut { BamSort* sort = nullptr; bool on = false; std::vector<uint8_t> index; bool have_index = false; };
void sortout_drop(SortOut* o) { o->on = false; model_drop(o->sort); }
int sortout_finish(SortOut* o, const uint8_t* header, int64_t n) { o->on = false; const int rc = model_finish(o->sort, header, n); if (rc != SVX_OK) model_drop(o->sort); return rc; }
bool sortout_finished(const SortOut* o) { return o->sort && model_alive(o->sort, "finished")->finished; }
void sortout_count(const SortOut* o, int64_t* a, int64_t* b, int64_t* c) { model_count(o->sort, a, b, c); }
int sortout_encode(SortOut* o, int64_t first, int64_t nb, int64_t* n_bytes) { return model_encode(o->sort, first, nb, n_bytes); }
int sortout_fetch(SortOut* o, uint8_t* a, uint8_t* b) { return model_fetch(o->sort, a, b); }
int sortout_index(SortOut* o, int fmt) {                    // (the index is the kernels' work: the model's holds the record count and the format)
    if (!model_alive(o->sort, "index")->finished) return SVX_E_STATE;
    const uint64_t n = o->sort->rows.size();
    o->index.assign(12, 0); memcpy(o->index.data(), &n, 8); memcpy(o->index.data() + 8, &fmt, 4); o->have_index = true;
    return SVX_OK;
}
bool sortout_index_bytes(const SortOut* o, int64_t* n) { if (o->have_index && n) *n = (int64_t)o->index.size(); return o->have_index; }
int sortout_index_fetch(SortOut* o, uint8_t* dst) { memcpy(dst, o->index.data(), o->index.size()); return SVX_OK; }
int sortout_permutation(SortOut* o, uint32_t* perm) { return model_permutation(o->sort, perm); }
void sortout_stats(const SortOut*, svx_bam_sort_stats* out) { memset(out, 0, sizeof *out); }
void sortout_spill_stats(const SortOut*, svx_bam_sort_spill_stats* out) { memset(out, 0, sizeof *out); }
void sortout_name_stats(const SortOut*, svx_bam_name_sort_stats* out) { memset(out, 0, sizeof *out); }
void sortout_name_spill_stats(const SortOut*, svx_bam_name_spill_stats* out) { memset(out, 0, sizeof *out); }
void sortout_translate_stats(const SortOut*, int64_t* c, int64_t* r, int64_t* by, double* t) { *c = *r = *by = 0; *t = 0; }

// ---- the decoder's side (devdec.hpp): its own sort, and the feed it borrows --------------------------------------------------------------------------------
static int model_after_load(svx_devdec* d, const MockSlot& S, const uint64_t* rec, size_t n_rec) {
    if (d->out->on && n_rec > 0) {
        const int rc = model_append(d->out->sort, S, rec, n_rec, nullptr, -1, true, false);
        if (rc != SVX_OK) { sortout_drop(d->out); return rc; }
    }
    if (d->feed && n_rec > 0) {
        BamSort* const fed = d->feed->sort;
        if (fed->borrowers.load() < 1) model_die("a decoder appends to a sort it has not borrowed");
        const int rc = model_append(fed, S, rec, n_rec, d->feed_map, d->feed_n_ref, d->feed_identity, true);
        if (rc != SVX_OK) { fed->borrowers--; d->feed = nullptr; return rc; }
    }
    return SVX_OK;
}
static void model_create_decoder(svx_devdec* d) { d->out = new SortOut(); }
static void model_destroy_decoder(svx_devdec* d) {
    if (d->feed) model_die("a decoder was destroyed while it feeds a session");
    model_destroy(d->out->sort);
    delete d->out; d->out = nullptr;
}
void devdec_feed_set(svx_devdec* d, SortOut* session, const int32_t* map, int32_t n_ref_file, bool identity) {
    model_alive(session->sort, "feed_set");
    if (d->feed) model_die("a decoder that feeds a session was given a second feed");
    session->sort->borrowers++;
    d->feed_map = map; d->feed_n_ref = n_ref_file; d->feed_identity = identity; d->feed = session;
}
void devdec_feed_clear(svx_devdec* d) { if (d->feed) { model_alive(d->feed->sort, "feed_clear"); d->feed->sort->borrowers--; } d->feed = nullptr; d->feed_map = nullptr; }
bool devdec_feed_on(const svx_devdec* d) { return d->feed != nullptr; }
int devdec_device(const svx_devdec*) { return 0; }
int devdec_sort_begin(svx_devdec* d, int64_t max_bytes, const char*, int) { model_begin(&d->out->sort, max_bytes, (int32_t)d->rank.size()); d->out->on = true; return SVX_OK; }
bool devdec_sort_on(const svx_devdec* d) { return d->out->on; }
SortOut* devdec_sort_out(svx_devdec* d) { return d->out; }

// ---- the session's device side (devdec.hpp: mergedev_*) ------------------------------------------------------------------------------------------------------
struct MergeDev { uint32_t magic = MODEL_ALIVE; SortOut out; std::vector<int32_t>* maps = nullptr; };
static std::atomic<int> g_sessions_alive{0};
static MergeDev* md_alive(const MergeDev* m, const char* where) { if (!m || m->magic != MODEL_ALIVE) { fprintf(stderr, "in %s: ", where); model_die("a session's device side was used after its destruction"); } return const_cast<MergeDev*>(m); }
int mergedev_create(int, int64_t max_bytes, int32_t n_ref_merged, const char*, int /* the model sorts in coordinate order */, const int32_t* maps, int64_t n_maps, MergeDev** out) {
    MergeDev* m = new MergeDev();
    model_begin(&m->out.sort, max_bytes, n_ref_merged); m->out.on = true;
    m->maps = new std::vector<int32_t>(maps, maps + n_maps);
    g_sessions_alive++;
    *out = m;
    return SVX_OK;
}
void mergedev_destroy(MergeDev* m) {
    if (!m) return;
    md_alive(m, "destroy");
    model_destroy(m->out.sort); m->out.sort = nullptr;
    if (m->maps) { std::fill(m->maps->begin(), m->maps->end(), 0x55555555); delete m->maps; m->maps = nullptr; }
    m->magic = MODEL_DEAD;
    g_sessions_alive--;
    delete m;
}
int mergedev_device(const MergeDev* m) { md_alive(m, "device"); return 0; }
void mergedev_feed(MergeDev* m, svx_devdec* d, int64_t map_at, int32_t n_ref_file, bool identity) { md_alive(m, "feed"); devdec_feed_set(d, &m->out, m->maps->data() + map_at, n_ref_file, identity); }
SortOut* mergedev_sort_out(MergeDev* m) { return &md_alive(m, "sort_out")->out; }

// ---- inputs and a plain reimplementation of the merge ---------------------------------------------------------------------------------------------------------
static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
struct Input { std::string path; std::vector<std::string> names; std::vector<int32_t> lens; std::vector<uint8_t> header; std::vector<std::vector<uint8_t>> recs; };
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 20); }
static std::vector<uint8_t> make_record(int32_t tid, int32_t pos, uint16_t flag, int32_t mate, const std::string& name) {
    std::vector<uint8_t> b;
    put32(b, tid); put32(b, (uint32_t)pos);
    b.push_back((uint8_t)(name.size() + 1)); b.push_back(30); b.push_back(0x48); b.push_back(0x12);      // l_read_name, mapq, bin
    b.push_back(1); b.push_back(0); b.push_back((uint8_t)flag); b.push_back((uint8_t)(flag >> 8));       // n_cigar_op, flag
    put32(b, 0); put32(b, (uint32_t)mate); put32(b, (uint32_t)(pos + 7)); put32(b, 0);                   // l_seq, next_refID, next_pos, tlen
    b.insert(b.end(), name.begin(), name.end()); b.push_back(0);
    put32(b, (10u << 4) | 0u);
    std::vector<uint8_t> r; put32(r, (uint32_t)b.size()); r.insert(r.end(), b.begin(), b.end());
    return r;
}
static Input make_input(const std::string& dir, int f, const std::vector<std::string>& names, int n, size_t block, int32_t bad_mate = -99) {
    Input x; x.path = dir + "/merge_in_" + std::to_string(f) + (bad_mate != -99 ? "_bad" : "") + ".bam"; x.names = names;
    std::string text = "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t i = 0; i < names.size(); i++) { x.lens.push_back(100000 + 1000 * (int32_t)(names[i][1] - '0')); text += "@SQ\tSN:" + names[i] + "\tLN:" + std::to_string(x.lens.back()) + "\n"; }
    text += "@PG\tID:aln\tCL:file " + std::to_string(f) + "\n";
    x.header = {'B', 'A', 'M', 1};
    put32(x.header, (uint32_t)text.size()); x.header.insert(x.header.end(), text.begin(), text.end());
    put32(x.header, (uint32_t)names.size());
    for (size_t i = 0; i < names.size(); i++) { put32(x.header, (uint32_t)names[i].size() + 1); x.header.insert(x.header.end(), names[i].begin(), names[i].end()); x.header.push_back(0); put32(x.header, (uint32_t)x.lens[i]); }
    const int32_t nr = (int32_t)names.size();
    for (int k = 0; k < n; k++) {
        const int32_t tid = nr ? (int32_t)(rnd() % (uint32_t)(nr + 1)) - 1 : -1;
        const int32_t mate = nr ? (int32_t)(rnd() % (uint32_t)(nr + 1)) - 1 : -1;
        x.recs.push_back(make_record(tid, tid < 0 ? -1 : (int32_t)(rnd() % 40), (uint16_t)((rnd() & 1 ? 16 : 0) | (tid < 0 ? 4 : 0)), k == n / 2 && bad_mate != -99 ? bad_mate : mate,
                                     std::string(1 + rnd() % 5, (char)('a' + f)) + std::to_string(k)));
    }
    std::vector<uint8_t> raw = x.header;
    for (auto& r : x.recs) raw.insert(raw.end(), r.begin(), r.end());
    const std::vector<uint8_t> img = bgzf_all(raw, block);
    FILE* fh = fopen(x.path.c_str(), "wb"); if (!fh) { perror(x.path.c_str()); exit(2); }
    fwrite(img.data(), 1, img.size(), fh); fclose(fh);
    return x;
}
// order of the definition, written out on its own: (refID with -1 last, pos + 1, reverse strand), ties by place in the concatenation
struct PlainRec { int64_t t; int64_t p; int s; std::vector<uint8_t> bytes; };
static bool plain_less(const PlainRec& a, const PlainRec& b) { if (a.t != b.t) return a.t < b.t; if (a.p != b.p) return a.p < b.p; return a.s < b.s; }
// -> the records of the merged stream (no header) and the permutation; false: the definition refuses (a mate id outside a translated file's dictionary)
static bool plain_merge(const std::vector<const Input*>& in, std::vector<uint8_t>& out, std::vector<uint32_t>& perm) {
    std::vector<std::string> dict;
    std::vector<PlainRec> all;
    bool ok = true;
    for (const Input* x : in) {
        std::vector<int32_t> map; bool ident = true;
        for (size_t i = 0; i < x->names.size(); i++) {
            size_t at = std::find(dict.begin(), dict.end(), x->names[i]) - dict.begin();
            if (at == dict.size()) dict.push_back(x->names[i]);
            map.push_back((int32_t)at); if (at != i) ident = false;
        }
        for (const auto& r : x->recs) {
            PlainRec q; q.bytes = r;
            int32_t tid, mate; memcpy(&tid, r.data() + 4, 4); memcpy(&mate, r.data() + 24, 4);
            if (!ident) {
                if (mate < -1 || mate >= (int32_t)map.size()) ok = false;
                else { const int32_t t2 = tid < 0 ? -1 : map[(size_t)tid], m2 = mate < 0 ? -1 : map[(size_t)mate]; memcpy(q.bytes.data() + 4, &t2, 4); memcpy(q.bytes.data() + 24, &m2, 4); tid = t2; }
            }
            int32_t pos; memcpy(&pos, r.data() + 8, 4);
            q.t = tid < 0 ? (1ll << 40) : tid; q.p = (int64_t)pos + 1; q.s = (r[4 + 14] >> 4) & 1;
            all.push_back(std::move(q));
        }
    }
    std::vector<uint32_t> order(all.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return plain_less(all[a], all[b]); });
    out.clear(); perm = order;
    for (uint32_t i : order) out.insert(out.end(), all[i].bytes.begin(), all[i].bytes.end());
    return ok;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------------------------------
static long long g_wrong = 0, g_scenarios = 0, g_adds = 0, g_failures = 0, g_reader_sorts = 0;
#define WRONG(...) do { g_wrong++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", svx_last_error()); } while (0)

static svx_bam* open_reader(const Input& x) {
    svx_bam* h = nullptr;
    if (svx_bam_open(x.path.c_str(), 1, &h) != SVX_OK || svx_bam_set_device_decode(h, 0) != SVX_OK) { WRONG("cannot open %s", x.path.c_str()); exit(1); }
    return h;
}
static long long read_all(svx_bam* h) {
    long long total = 0;
    for (;;) { svx_batch b; int64_t n = 0; if (svx_bam_read_batch(h, 17, 0, 0, &b, &n) != SVX_OK) return -1; if (n == 0) return total; total += n; }
}
// a reader's own sort pass.  kind 1: to the end, finish, the bytes compared, the finished sort left in the handle; 2: the same, then abort; 3: abort in the middle of the pass
static void own_sort(svx_bam* h, const Input& x, int kind) {
    g_reader_sorts++;
    if (svx_bam_rewind(h) != SVX_OK) { WRONG("rewind in front of a reader's own sort"); return; }
    if (svx_bam_sort_begin(h, 0) != SVX_OK) { WRONG("sort_begin of a reader that has fed a session"); return; }
    if (kind == 3) {
        svx_batch b; int64_t n = 0;
        if (svx_bam_read_batch(h, 5, 0, 0, &b, &n) != SVX_OK) WRONG("read in a reader's own sort pass");
        if (svx_bam_sort_abort(h) != SVX_OK) WRONG("sort_abort in the middle of a pass");
        return;
    }
    if (read_all(h) != (long long)x.recs.size()) { WRONG("a reader's own sort pass did not see every record"); return; }
    if (svx_bam_sort_finish(h) != SVX_OK) { WRONG("sort_finish of a reader that has fed a session"); return; }
    int64_t n = 0, bytes = 0, blocks = 0;
    if (svx_bam_sort_count(h, &n, &bytes, &blocks) != SVX_OK) { WRONG("sort_count"); return; }
    std::vector<uint8_t> got;
    for (int64_t b0 = 0; b0 < blocks; b0++) {
        int64_t nb = 0;
        if (svx_bam_sort_encode(h, b0, 1, &nb) != SVX_OK) { WRONG("sort_encode"); return; }
        const size_t at = got.size(); got.resize(at + (size_t)nb);
        if (svx_bam_sort_fetch(h, got.data() + at, nullptr) != SVX_OK) { WRONG("sort_fetch"); return; }
    }
    std::vector<uint8_t> want, body; std::vector<uint32_t> perm;
    (void)plain_merge({&x}, body, perm);
    int64_t hn = 0;
    std::vector<uint8_t> hdr(x.header.size() + 64);
    if (svx_bam_sort_header_host(x.header.data(), (int64_t)x.header.size(), hdr.data(), (int64_t)hdr.size(), &hn) != SVX_OK) { WRONG("sort_header_host"); return; }
    want.assign(hdr.begin(), hdr.begin() + hn); want.insert(want.end(), body.begin(), body.end());
    if (n != (int64_t)x.recs.size() || got != want) WRONG("a reader's own sort after feeding a session gives other bytes (%zu, %zu expected)", got.size(), want.size());
    if (kind == 2 && svx_bam_sort_abort(h) != SVX_OK) WRONG("sort_abort after finish");
}
// the session's output against the plain merge
static void check_output(svx_bam_merge* m, const std::vector<const Input*>& in) {
    int64_t n = 0, bytes = 0, blocks = 0;
    if (svx_bam_merge_count(m, &n, &bytes, &blocks) != SVX_OK) { WRONG("merge_count"); return; }
    std::vector<uint8_t> got;
    const int64_t step = 1 + (int64_t)(rnd() % 3);
    for (int64_t b0 = 0; b0 < blocks; b0 += step) {
        int64_t nb = 0; const int64_t cnt = std::min(step, blocks - b0);
        if (svx_bam_merge_encode(m, b0, cnt, &nb) != SVX_OK) { WRONG("merge_encode"); return; }
        const size_t at = got.size(); got.resize(at + (size_t)nb);
        if (nb && svx_bam_merge_fetch(m, got.data() + at, nullptr) != SVX_OK) { WRONG("merge_fetch"); return; }
    }
    std::vector<const uint8_t*> hp; std::vector<int64_t> hs; size_t n_maps = 0;
    for (const Input* x : in) { hp.push_back(x->header.data()); hs.push_back((int64_t)x->header.size()); n_maps += x->names.size(); }
    std::vector<int32_t> maps(n_maps + 1);
    int64_t hn = 0;
    (void)svx_bam_merge_header_host(hp.data(), hs.data(), (int64_t)in.size(), nullptr, 0, &hn, maps.data());
    std::vector<uint8_t> want((size_t)hn);
    if (svx_bam_merge_header_host(hp.data(), hs.data(), (int64_t)in.size(), want.data(), hn, &hn, maps.data()) != SVX_OK) { WRONG("merge_header_host"); return; }
    std::vector<uint8_t> body; std::vector<uint32_t> perm;
    (void)plain_merge(in, body, perm);
    want.insert(want.end(), body.begin(), body.end());
    if (n != (int64_t)perm.size() || got != want) { WRONG("the merged bytes differ from the plain merge (%zu bytes, %zu expected)", got.size(), want.size()); return; }
    std::vector<uint32_t> gp(perm.size() + 1);
    if (svx_bam_merge_permutation(m, gp.data()) != SVX_OK || !std::equal(perm.begin(), perm.end(), gp.begin())) WRONG("the permutation differs from the plain merge");
    int64_t ib = 0;
    if (svx_bam_merge_index_count(m, &ib) != SVX_E_STATE) WRONG("an index before it was built");
    if (svx_bam_merge_index_fmt(m, SVX_INDEX_CLASSIC) != SVX_OK || svx_bam_merge_index_count(m, &ib) != SVX_OK || ib != 12) { WRONG("merge_index"); return; }
    std::vector<uint8_t> ix((size_t)ib);
    uint64_t cnt = 0;
    if (svx_bam_merge_index_fetch(m, ix.data()) != SVX_OK || (memcpy(&cnt, ix.data(), 8), cnt != (uint64_t)n)) WRONG("merge_index_fetch");
}

// when reader r is closed: 0 right after open (a fresh handle is opened for its add), 1 right after its add, 2 after the last add, 3 after the session's output was
// fetched, 4 after the session is closed.  sorter: the reader that sorts on its own after it has fed (-1: none), sort_kind as own_sort, sort_late: not right behind
// its add but as late as its closing time allows.  session_end: 0 finish .. close, 1 closed after the adds without a finish, 2 closed after the first add
struct Plan { int k; int close_when[3]; int sorter, sort_kind, sort_late, session_end; };
static void run_plan(const std::vector<Input>& files, const Plan& P) {
    g_scenarios++;
    std::vector<const Input*> in; for (int r = 0; r < P.k; r++) in.push_back(&files[(size_t)r]);
    svx_bam* H[3] = {nullptr, nullptr, nullptr};
    for (int r = 0; r < P.k; r++) H[r] = open_reader(files[(size_t)r]);
    svx_bam_merge* m = nullptr;
    if (svx_bam_merge_open(H, P.k, 0, 0, nullptr, &m) != SVX_OK) { WRONG("merge_open"); for (int r = 0; r < P.k; r++) svx_bam_close(H[r]); return; }
    for (int r = 0; r < P.k; r++) if (P.close_when[r] == 0) { svx_bam_close(H[r]); H[r] = open_reader(files[(size_t)r]); }
    bool sorted = P.sorter < 0;
    auto maybe_sort = [&](int stage) {     // stage: the closing time that is about to be served
        if (sorted || !H[P.sorter]) return;
        const int limit = P.close_when[P.sorter] == 0 ? 4 : P.close_when[P.sorter];
        if (!P.sort_late || stage >= limit) { own_sort(H[P.sorter], files[(size_t)P.sorter], P.sort_kind); sorted = true; }
    };
    int64_t dummy = 0;
    if (svx_bam_merge_finish(m) != SVX_E_STATE || svx_bam_merge_count(m, &dummy, nullptr, nullptr) != SVX_E_STATE) WRONG("finish / count before the adds are not SVX_E_STATE");
    bool closed_session = false;
    for (int r = 0; r < P.k && !closed_session; r++) {
        if (r + 1 < P.k && svx_bam_merge_add(m, H[r + 1]) != SVX_E_ARG && files[(size_t)r + 1].names != files[(size_t)r].names) WRONG("an add out of order is not SVX_E_ARG");
        if (svx_bam_merge_add(m, H[r]) != SVX_OK) { WRONG("merge_add of file %d", r); break; }
        g_adds++;
        if (svx_bam_merge_encode(m, 0, 1, &dummy) != SVX_E_STATE) WRONG("encode before finish is not SVX_E_STATE");
        if (r == 0 && P.session_end == 2) { svx_bam_merge_close(m); m = nullptr; closed_session = true; }
        if (P.sorter == r) maybe_sort(1);
        if (P.close_when[r] == 1) { svx_bam_close(H[r]); H[r] = nullptr; }
    }
    if (P.sorter >= 0) maybe_sort(2);
    for (int r = 0; r < P.k; r++) if (P.close_when[r] == 2 && H[r]) { svx_bam_close(H[r]); H[r] = nullptr; }
    if (m && P.session_end == 1) { svx_bam_merge_close(m); m = nullptr; }
    if (m) {
        if (svx_bam_merge_finish(m) != SVX_OK) WRONG("merge_finish");
        else check_output(m, in);
    }
    if (P.sorter >= 0) maybe_sort(3);
    for (int r = 0; r < P.k; r++) if (P.close_when[r] == 3 && H[r]) { svx_bam_close(H[r]); H[r] = nullptr; }
    if (m) { svx_bam_merge_close(m); m = nullptr; }
    if (P.sorter >= 0) maybe_sort(4);
    for (int r = 0; r < P.k; r++) if (H[r]) { svx_bam_close(H[r]); H[r] = nullptr; }
    if (g_sessions_alive.load() != 0) WRONG("a session's device side outlived svx_bam_merge_close");
}
// an append fails at chunk `at` of the session: the add carries the code, the session is broken, the reader rewinds clean, sorts on its own and closes in either order
static void run_injected(const std::vector<Input>& files, int k, long long at, int code, bool session_first) {
    g_scenarios++;
    svx_bam* H[3] = {nullptr, nullptr, nullptr};
    for (int r = 0; r < k; r++) H[r] = open_reader(files[(size_t)r]);
    svx_bam_merge* m = nullptr;
    if (svx_bam_merge_open(H, k, 0, 0, nullptr, &m) != SVX_OK) { WRONG("merge_open"); exit(1); }
    g_appends = 0; g_fail_code = code; g_fail_at = at;
    int failed = -1;
    for (int r = 0; r < k; r++) {
        const int rc = svx_bam_merge_add(m, H[r]);
        if (rc == SVX_OK) { g_adds++; continue; }
        if (rc != code) WRONG("an injected failure left the add as %d, not %d", rc, code);
        failed = r; g_failures++;
        break;
    }
    g_fail_at = -1;
    if (failed < 0) { WRONG("no append number %lld", at); }
    else {
        int64_t d = 0;
        if (svx_bam_merge_add(m, H[failed]) != SVX_E_STATE || svx_bam_merge_finish(m) != SVX_E_STATE || svx_bam_merge_count(m, &d, &d, &d) != SVX_E_STATE ||
            svx_bam_merge_encode(m, 0, 1, &d) != SVX_E_STATE || svx_bam_merge_index_fmt(m, SVX_INDEX_CLASSIC) != SVX_E_STATE || svx_bam_merge_permutation(m, nullptr) != SVX_E_STATE)
            WRONG("a broken session answers something else than SVX_E_STATE");
        if (session_first) { svx_bam_merge_close(m); m = nullptr; }
        if (svx_bam_rewind(H[failed]) != SVX_OK || read_all(H[failed]) != (long long)files[(size_t)failed].recs.size()) WRONG("the reader of a failed add does not rewind clean");
        own_sort(H[failed], files[(size_t)failed], 1 + (int)(at % 3));
    }
    if (m && (at & 1)) { svx_bam_merge_close(m); m = nullptr; }
    for (int r = 0; r < k; r++) svx_bam_close(H[r]);
    if (m) svx_bam_merge_close(m);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: bam_merge_session_test DIR [light]\n"); return 2; }
    const std::string dir = argv[1];
    const bool light = argc > 2 && std::string(argv[2]) == "light";
    // three files: a dictionary, its reverse with one name more (translated), a prefix of the first (identity, fewer references than the merged dictionary)
    std::vector<Input> files;
    files.push_back(make_input(dir, 0, {"c0", "c1", "c2"}, 70, 700));
    files.push_back(make_input(dir, 1, {"c2", "c1", "c0", "c7"}, 90, 600));
    files.push_back(make_input(dir, 2, {"c0", "c1"}, 50, 500));
    const Input bad_translated = make_input(dir, 1, {"c2", "c1", "c0", "c7"}, 40, 600, 4);
    const Input bad_identity = make_input(dir, 2, {"c0", "c1"}, 40, 600, 3);
    // both prefetch settings: chunks of one BGZF block (the loader decodes the next chunk while the batches of this one are handed out) and whole files
    const char* chunk_blocks[2] = {"1", "1000000"};
    for (int cb = 0; cb < 2; cb++) {
        setenv("SVX_BAM_DEV_CHUNK_BLOCKS", chunk_blocks[cb], 1);
        long long n_plans = 0;
        for (int k = 1; k <= 3; k++) {
            int n_close = 1; for (int r = 0; r < k; r++) n_close *= 5;
            for (int c = 0; c < n_close; c++)
                for (int sorter = -1; sorter < k; sorter++)
                    for (int kind = 1; kind <= (sorter < 0 ? 1 : 3); kind++)
                        for (int late = 0; late <= (sorter < 0 ? 0 : 1); late++) {
                            Plan P; P.k = k; int cc = c; for (int r = 0; r < 3; r++) { P.close_when[r] = cc % 5; cc /= 5; }
                            P.sorter = sorter; P.sort_kind = kind; P.sort_late = late;
                            P.session_end = (int)(n_plans % 7 == 3 ? 1 : n_plans % 7 == 5 ? 2 : 0);
                            if (light && k == 3 && n_plans % 9 != 0) { n_plans++; continue; }
                            n_plans++;
                            run_plan(files, P);
                        }
        }
        // an append that fails, at every chunk of every file, with both codes and both closing orders
        for (int k = 1; k <= 3; k++) {
            svx_bam* H[3]; for (int r = 0; r < k; r++) H[r] = open_reader(files[(size_t)r]);
            svx_bam_merge* m = nullptr;
            g_appends = 0;
            if (svx_bam_merge_open(H, k, 0, 0, nullptr, &m) != SVX_OK) { WRONG("merge_open"); return 1; }
            for (int r = 0; r < k; r++) { if (svx_bam_merge_add(m, H[r]) != SVX_OK) WRONG("merge_add"); svx_bam_close(H[r]); }
            const long long total = g_appends.load();
            svx_bam_merge_close(m);
            if (cb == 0 && total < 3 * k) WRONG("chunks of one block gave only %lld appends for %d files", total, k);
            for (long long at = 0; at < total; at++) run_injected(files, k, at, (at & 2) ? SVX_E_IO : SVX_E_CAPACITY, (at & 4) != 0);
        }
        // a reader's OWN sort fails (its arena is full) after it has fed a session: the session is untouched
        {
            g_scenarios++;
            svx_bam* H[1] = {open_reader(files[1])};
            svx_bam_merge* m = nullptr;
            if (svx_bam_merge_open(H, 1, 0, 0, nullptr, &m) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_OK) WRONG("open / add");
            g_own_appends = 0; g_own_fail_at = 0;
            if (svx_bam_rewind(H[0]) != SVX_OK || svx_bam_sort_begin(H[0], 0) != SVX_OK || read_all(H[0]) != -1) WRONG("an injected failure of a reader's own sort was not seen");
            g_own_fail_at = -1;
            if (svx_bam_merge_finish(m) != SVX_OK) WRONG("merge_finish beside a reader whose own sort failed"); else check_output(m, {&files[1]});
            svx_bam_close(H[0]); svx_bam_merge_close(m);
        }
        // the definition's refusals through the session: a mate id outside a translated file's dictionary is SVX_E_ARG at finish, verbatim in an identity file
        for (int which = 0; which < 2; which++) {
            g_scenarios++;
            const Input& second = which ? bad_identity : bad_translated;
            svx_bam* H[2] = {open_reader(files[0]), open_reader(second)};
            svx_bam_merge* m = nullptr;
            if (svx_bam_merge_open(H, 2, 0, 0, nullptr, &m) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_OK || svx_bam_merge_add(m, H[1]) != SVX_OK) WRONG("open / add");
            const int rc = svx_bam_merge_finish(m);
            if (which == 0 && (rc != SVX_E_ARG || svx_bam_merge_finish(m) != SVX_E_STATE)) WRONG("a bad mate id in a translated file: %d", rc);
            if (which == 1) { if (rc != SVX_OK) WRONG("a bad mate id in an identity file: %d", rc); else check_output(m, {&files[0], &second}); }
            svx_bam_merge_close(m); svx_bam_close(H[0]); svx_bam_close(H[1]);
        }
        // states an add refuses: a reader in a sort pass, not at its first record, on a region read, on a contig range, with another dictionary, without device decode
        {
            g_scenarios++;
            svx_bam* H[2] = {open_reader(files[0]), open_reader(files[1])};
            svx_bam_merge* m = nullptr;
            if (svx_bam_merge_open(H, 2, 0, 0, nullptr, &m) != SVX_OK) WRONG("merge_open");
            if (svx_bam_merge_add(m, H[1]) != SVX_E_ARG) WRONG("a foreign dictionary is not SVX_E_ARG");
            if (svx_bam_sort_begin(H[0], 0) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_E_STATE || svx_bam_sort_abort(H[0]) != SVX_OK) WRONG("an add during a sort pass is not SVX_E_STATE");
            svx_batch b; int64_t n = 0;
            if (svx_bam_read_batch(H[0], 3, 0, 0, &b, &n) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_E_STATE || svx_bam_rewind(H[0]) != SVX_OK) WRONG("an add behind the first record is not SVX_E_STATE");
            if (svx_bam_seek_region(H[0], 0, 0, 0, 100, SVX_REGION_OVERLAP) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_E_STATE || std::string(svx_last_error()).find("region read") == std::string::npos ||
                svx_bam_rewind(H[0]) != SVX_OK) WRONG("an add on a region read is not SVX_E_STATE");
            if (svx_bam_seek(H[0], 0, 1) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_E_STATE || std::string(svx_last_error()).find("contig range") == std::string::npos ||
                svx_bam_rewind(H[0]) != SVX_OK) WRONG("an add on a contig range is not SVX_E_STATE");
            if (svx_bam_set_device_decode(H[0], -1) != SVX_OK || svx_bam_merge_add(m, H[0]) != SVX_E_STATE || svx_bam_set_device_decode(H[0], 0) != SVX_OK) WRONG("an add without device decode is not SVX_E_STATE");
            if (svx_bam_merge_add(m, H[0]) != SVX_OK || svx_bam_merge_add(m, H[1]) != SVX_OK || svx_bam_merge_add(m, H[1]) != SVX_E_STATE) WRONG("the adds after the refused ones");
            g_adds += 2;
            if (svx_bam_merge_finish(m) != SVX_OK) WRONG("merge_finish"); else check_output(m, {&files[0], &files[1]});
            svx_bam_close(H[0]); svx_bam_close(H[1]); svx_bam_merge_close(m);
        }
    }
    unsetenv("SVX_BAM_DEV_CHUNK_BLOCKS");
    {   // header refusals leave at open, with nothing made on the device side
        g_scenarios++;
        std::vector<Input> clash; clash.push_back(make_input(dir, 0, {"c0", "c1"}, 5, 600));
        Input other = make_input(dir, 3, {"c1"}, 5, 600);
        // the same name with another length: the dictionary entry and the @SQ line
        const size_t at = other.header.size() - 4; other.header[at] ^= 1;
        std::vector<uint8_t> raw = other.header; for (auto& r : other.recs) raw.insert(raw.end(), r.begin(), r.end());
        const std::vector<uint8_t> img = bgzf_all(raw, 600);
        FILE* fh = fopen(other.path.c_str(), "wb"); fwrite(img.data(), 1, img.size(), fh); fclose(fh);
        svx_bam* H[2] = {open_reader(clash[0]), open_reader(other)};
        svx_bam_merge* m = nullptr;
        if (svx_bam_merge_open(H, 2, 0, 0, nullptr, &m) != SVX_E_ARG || m != nullptr || g_sessions_alive.load() != 0) WRONG("one name with two lengths is not SVX_E_ARG at open");
        svx_bam_close(H[0]); svx_bam_close(H[1]);
        remove(other.path.c_str()); remove(clash[0].path.c_str());
    }
    for (auto& x : files) remove(x.path.c_str());
    remove(bad_translated.path.c_str()); remove(bad_identity.path.c_str());
    {   // every model that was destroyed is still poisoned, and nothing else is left
        std::lock_guard<std::mutex> g(g_grave_m);
        for (BamSort* S : g_grave) { if (S->magic != MODEL_DEAD || !S->slabs.empty()) WRONG("a destroyed sort was written to"); delete S; }
        g_grave.clear();
    }
    printf("%lld scenarios, %lld adds, %lld injected failures, %lld reader sorts, %lld wrong\n", g_scenarios, g_adds, g_failures, g_reader_sorts, g_wrong);
    return g_wrong ? 1 : 0;
}
