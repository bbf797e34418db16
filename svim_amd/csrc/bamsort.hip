// bamsort.hip - the file the device reader (bamdev.hip) is reading, put into coordinate order on the device: the sorted BGZF file piece by piece and its .bai
// (svx_bam_sort*, include/svx.h; gfx950).  What the sorted file is: svim_amd/bamsort.py; the key and the checks: bamsort_core.hpp, the source
// svx_bam_sort_host is built from as well.
// Replaces: samtools view | samtools sort and samtools index in front of the pipeline (the reference's run_alignment hands the aligner's output to them,
// src/svim/SVIM_alignment.py:48-50): single-threaded zlib both ways and a merge on the host, for records this reader has already found.
//   append   while sorting is on, every chunk the reader loads leaves its records' bytes - they lie back to back in the inflated stream - in a slab of their own
//            (one device-to-device copy; slabs are never moved or regrown) and one row per record: k_bs_rows the key, the length, the address in the slab, the
//            checks; the index rows (tid, pos, end, flag) by bamindex.hip's own append.  A chunk of a file of a merge session (bammerge.hip) whose dictionary is
//            not the merged one passes k_bs_translate first: refID and next_refID mapped, patched in the slab by byte stores, the merged id in a column of its own
//   finish   the keys sorted stably (svx_sort_pairs_u64_on over the key's used bits) with the record number as payload = the permutation; k_bs_layout the
//            segments of the output stream (the header, then the records in order) with their lengths and addresses; a scan gives every segment's offset
//            In query-name order (svx_bam_sort_begin_order; a merge session: svx_bam_merge_open_order) the permutation comes from the names instead: the
//            k_ns_* kernels below.  Runs in that order (a session with a spill directory): "query-name order beyond device memory" below
//   encode   a range of 65 280-byte blocks: k_bs_gather lays the stream bytes of the range out in the piece buffer, then the encoder's phases over the piece
//            (textgz_kernels.hpp: CRC, matches, codes, bits, compaction), every block's compressed size kept on the host
//   index    the sorted rows with the virtual offsets the block sizes give, through bamindex.hip's phases (bamindex_take_rows, bamindex_finish)
// Files whose records do not fit (svx_bam_sort_begin_spill): only the record BYTES are spilled, the rows stay.
//   run      the chunk that would take the arena past the limit closes a run: its (key, record number) pairs sorted stably, k_bs_run_layout the segments of the
//            run's stream (no header) and the run-order rows that stay resident (key, length, file index, offset in the run's stream), the stream gathered
//            piece by piece by k_bs_gather and appended to ONE spill file (created in the caller's directory, unlinked at once), the slabs freed
//   merge    finish: one stable radix sort over the concatenation of the run-sorted keys, payload the place in the concatenation.  Equal keys tie by run, then
//            by place in the run; runs are consecutive file ranges and each run's sort is stable: the permutation of the in-memory sort.  k_bs_spill_layout
//            the segment table (run, offset in the run's stream, length) and gpos, the global positions of each run's records, increasing within a run
//   encode   k_bs_piece_cuts: for every run the in-run range of the piece's records, by two bisections in the run's gpos (bamsort_core.hpp: bsort_piece_cut -
//            a run contributes a CONTIGUOUS range to any contiguous range of the global order); the byte ranges are read back from the file into a staging
//            buffer, back to back, k_bs_piece_addr gives the piece's segments their addresses there, and the gather and the encoder run unchanged
// k_bs_gather: a workgroup owns tiles of BS_TILE bytes of the piece; work follows the bytes of the destination, not the records (a record is between 36 bytes and
// hundreds of kilobytes long).  Wave 0 finds the tile's first and last segment in the stream offsets by a 64-ary search (one probe per lane and step), the
// tile's segment table goes to LDS, and every lane takes aligned 16-byte words of the destination: the segment of a word's first byte by bisection in LDS, the
// word from two aligned 16-byte loads of the source merged by a byte funnel shift (v_alignbyte_b32), one 16-byte store.  A word that holds a segment edge (at
// most one in 36 bytes) is put together byte by byte and still stored whole; only the last, partial word of a piece is written in bytes.  No atomics, no LDS
// traffic per byte: the kernel moves every byte once in and once out.
#include "common.hpp"
#include "hostcopy.hpp"
#include "scan.hpp"
#include "bamsort_core.hpp"
#include "bamsort.hpp"
#include "textgz_kernels.hpp"
#include <algorithm>
#include <string>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#define BS_T 256
#define BS_GRID(n) (unsigned)(((long long)(n) + BS_T - 1) / BS_T)
#define BS_TILE 16384                 /* bytes of the piece per workgroup and step: 4 words of 16 bytes per lane */
#define BS_SEGS 512                   /* segments of a tile kept in LDS: a record is at least 36 bytes, so a tile touches at most 16384 / 36 + 2 = 457 */
#define BS_MAX_GRID 2048
#define BS_SPILL_PIECE (32ll << 20)   /* bytes of a run's stream gathered and written at a time (a multiple of 16) */
#define BSORT_NAME_ROW_BYTES (26 + 37)  /* per record of a spilling query-name sort, in the free-memory rule of bamsort_append */
#define BS_PAD 64                     /* bytes behind a slab, the header and the piece: the aligned loads around a record's last bytes stay inside the allocation */
static_assert(BSORT_BLOCK == DEF_BLOCK, "the output's blocks are the encoder's");
static_assert(BSORT_NAME_MAX_ROUNDS <= 64, "svx_bam_name_sort_stats.active_rows holds every round");
static_assert(BSORT_BLOCK % 16 == 0 && BS_TILE % 16 == 0, "a piece and its tiles start at aligned words of the destination");

typedef unsigned int bs_u32x4 __attribute__((ext_vector_type(4)));

// ---- append ---------------------------------------------------------------------------------------------------------------------------------------------
// n_ref_check: the dictionary the record's id must lie in (of a file of a merge: that file's own); n_ref: the dictionary the key is built over
__global__ void k_bs_rows(long long n, const uint8_t* st, const uint64_t* rec_off, uint64_t first_byte, uint64_t end_byte, uint64_t slab, const int32_t* tid, const int32_t* pos,
                          const uint16_t* flag, int32_t n_ref_check, int32_t n_ref, uint64_t* key, uint32_t* len, uint64_t* addr, int* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = rec_off[i];
    const uint32_t bs = (uint32_t)st[p] | ((uint32_t)st[p + 1] << 8) | ((uint32_t)st[p + 2] << 16) | ((uint32_t)st[p + 3] << 24);
    int b = bsort_check(tid[i], pos[i], bs, n_ref_check);
    if (p < first_byte || p + 4ull + bs > end_byte) b |= BSORT_BAD_SIZE;            // (cannot happen: the reader walked these records)
    if (b) atomicOr(bad, b);
    key[i] = bsort_key(tid[i], pos[i], flag[i], n_ref);
    len[i] = 4u + bs;
    addr[i] = slab + (p - first_byte);
}
// a chunk of a file of a merge whose dictionary is not the merged one (svim_amd/bammerge.py), in front of k_bs_rows: a thread per record.  refID is the decoded
// column, next_refID the record's bytes - records are 4-byte aligned only by accident, so bytes are loaded - and bsort_translate maps both.  The merged refID goes
// to tid_out (the key's and the index row's column), and the two fields are patched in the SLAB's copy by byte stores: two 36-byte neighbours may share an
// aligned word, which a read-modify-write of it by both their threads would tear.  A record shorter than its fixed fields is left alone (k_bs_rows refuses it)
__global__ void k_bs_translate(long long n, const uint64_t* rec_off, uint64_t first_byte, uint64_t end_byte, uint8_t* slab, const int32_t* tid, const int32_t* map, int32_t n_ref_file,
                               int32_t* tid_out, int* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = rec_off[i];
    if (p < first_byte || p + 4ull + BSORT_MIN_BLOCK_SIZE > end_byte) { tid_out[i] = -1; return; }
    uint8_t* r = slab + (p - first_byte);
    const uint32_t bs = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
    if (bs < BSORT_MIN_BLOCK_SIZE) { tid_out[i] = -1; return; }
    const uint8_t* m = r + BSORT_MATE_AT;
    const int32_t mate = (int32_t)((uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24));
    int32_t t, mt;
    const int b = bsort_translate(tid[i], mate, map, n_ref_file, &t, &mt);
    tid_out[i] = t;
    for (int k = 0; k < 4; k++) { r[BSORT_REFID_AT + k] = (uint8_t)((uint32_t)t >> (8 * k)); r[BSORT_MATE_AT + k] = (uint8_t)((uint32_t)mt >> (8 * k)); }
    if (b) atomicOr(bad, b);
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ void k_bs_iota(long long n, uint32_t* v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}
// segment 0 is the header, segment i + 1 the record perm[i]; slen has one entry more (0) so that its scan ends with the stream's size
__global__ void k_bs_layout(long long n, const uint32_t* perm, const uint32_t* len, const uint64_t* addr, uint64_t hdr, long long hdr_bytes, int64_t* slen, uint64_t* saddr) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n + 1) return;
    if (j == n + 1) { slen[j] = 0; return; }
    if (j == 0) { slen[0] = hdr_bytes; saddr[0] = hdr; return; }
    const uint32_t r = perm[j - 1];
    slen[j] = (int64_t)len[r]; saddr[j] = addr[r];
}

// a run is closed: segment j of its stream is the record first + order[j] (order: the run's stable sort, indices inside the run; len / addr: the run's rows in
// file order); slen has one entry more (0).  What stays resident of the run, in run order: length and file index (the key comes from the sort itself)
__global__ void k_bs_run_layout(long long m, const uint32_t* order, const uint32_t* len, const uint64_t* addr, uint32_t first, int64_t* slen, uint64_t* saddr, uint32_t* rlen,
                                uint32_t* rfile) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    if (j == m) { slen[j] = 0; return; }
    const uint32_t r = order[j];
    slen[j] = (int64_t)len[r]; saddr[j] = addr[r];
    rlen[j] = len[r]; rfile[j] = first + r;
}
// the merge: gp[j - 1] = the place in the concatenation of the runs of the record at global position j - 1 (segment j; segment 0 is the header).  Per segment
// its run, its offset in the run's stream and its length; per place its global position (gpos: increasing within a run); the permutation
__global__ void k_bs_spill_layout(long long n, const uint32_t* gp, const uint32_t* rlen, const uint32_t* rfile, const int64_t* roff, const int64_t* run_base, long long n_runs,
                                  uint64_t hdr, long long hdr_bytes, uint32_t* perm, int64_t* slen, uint32_t* srun, int64_t* sroff, uint32_t* gpos, uint64_t* saddr) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n + 1) return;
    if (j == n + 1) { slen[j] = 0; return; }
    if (j == 0) { slen[0] = hdr_bytes; saddr[0] = hdr; srun[0] = 0u; sroff[0] = 0; return; }
    const uint32_t q = gp[j - 1];
    perm[j - 1] = rfile[q];
    slen[j] = (int64_t)rlen[q]; srun[j] = (uint32_t)bsort_run_of(run_base, n_runs, (int64_t)q); sroff[j] = roff[q];
    gpos[q] = (uint32_t)(j - 1);
}

// ---- query-name order: the permutation ------------------------------------------------------------------------------------------------------------------
// The key is (name, name_rank) (bamsort_core.hpp): a string of up to 255 bytes at any byte alignment in a slab, which no 64-bit radix key holds.  The order is
// made least significant part first, then most significant word first:
//   k_ns_names   a thread per record: l_read_name and the name's extent through addr[i] by byte loads (records are 4-byte aligned only by accident), the checks
//                (BSORT_BAD_NAME), the name's length and name_rank as the key of the rank pass
//   rank pass    one stable radix pass over the 4 bits of name_rank, payload the record number: perm = the records in (rank, file) order.  Every later sort is
//                stable, so records whose names are equal stay in that order
//   round r      over the ACTIVE rows only - the places of perm whose order is still open, in ascending place, each with the label of its segment (a maximal run
//                of places whose names agree in every byte in front of 4 r; labels ascend with the place).  k_ns_keys: (label << 32) | the big-endian word of
//                name bytes [4 r, 4 r + 4), zero-filled behind the name's end; one stable radix sort over 32 + ceil(log2(labels)) bits; the k-th sorted row
//                goes to the k-th active place (a segment's rows are a contiguous range of the active list before and after the sort).  k_ns_heads: a row
//                starts a new segment where its key differs from its neighbour's, and it stays active unless its segment has one member or its word's last
//                byte is 0 - a name holds no NUL, so that name ended inside the word and every name of the segment is the same name; both flags go through ONE
//                scan as the two halves of a 64-bit word.  k_ns_apply: perm written, the rows that stay compacted with their new labels
//   end          the host reads the scan's last entry (8 bytes: rows that stay, segments) once per round; no rows left ends the rounds - after at most
//                BSORT_NAME_MAX_ROUNDS = 64, the round in which a name of 255 bytes ends inside its word
// A name that ends exactly at a word's edge stays active for one more round, where its word is 0 and sorts in front of every longer name: a proper prefix first.
__global__ void k_ns_names(long long n, const uint64_t* addr, const uint32_t* len, uint8_t* name_len, uint64_t* rank, int* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = reinterpret_cast<const uint8_t*>(addr[i]);                 // (the whole record lies in its slab and holds its fixed fields: k_bs_rows saw to it)
    const uint32_t l_name = r[BSORT_LNAME_AT];
    const int b = bsort_name_check(l_name, len[i] - 4u);
    if (b) atomicOr(bad, b);
    name_len[i] = b ? (uint8_t)0 : (uint8_t)bsort_name_len(r + BSORT_NAME_AT, l_name);
    rank[i] = bsort_name_rank((uint32_t)r[BSORT_FLAG_AT] | ((uint32_t)r[BSORT_FLAG_AT + 1] << 8));
}
// the m active rows of round r; place and seg null: round 0, every place active in one segment
__global__ void k_ns_keys(long long m, uint32_t r, const uint32_t* perm, const uint32_t* place, const uint32_t* seg, const uint64_t* addr, const uint8_t* name_len, uint64_t* key,
                          uint32_t* val) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t rec = perm[place ? place[k] : (uint32_t)k];
    const uint32_t w = bsort_name_word(reinterpret_cast<const uint8_t*>(addr[rec]) + BSORT_NAME_AT, name_len[rec], r);      // (reads nothing behind the name's end)
    key[k] = ((uint64_t)(seg ? seg[k] : 0u) << 32) | w;
    val[k] = rec;
}
// flags has m + 1 entries (the last one 0, so that the scan ends with the totals): bit 32 a segment starts here, bit 0 the row stays active
__global__ void k_ns_heads(long long m, const uint64_t* key, int64_t* flags) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > m) return;
    if (k == m) { flags[k] = 0; return; }
    const uint64_t x = key[k];
    const bool head = k == 0 || key[k - 1] != x, last = k == m - 1 || key[k + 1] != x;
    const bool stays = !(head && last) && (x & 0xffull) != 0;
    flags[k] = ((int64_t)head << 32) | (int64_t)stays;
}
// ex: the exclusive scan of flags.  The k-th sorted row goes to the k-th active place; the rows that stay are compacted, with the number of their segment
__global__ void k_ns_apply(long long m, const uint32_t* val, const int64_t* flags, const int64_t* ex, const uint32_t* place, uint32_t* perm, uint32_t* place_out, uint32_t* seg_out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t at = place ? place[k] : (uint32_t)k;
    perm[at] = val[k];
    const uint64_t f = (uint64_t)flags[k], e = (uint64_t)ex[k];
    if (f & 1ull) {
        const uint32_t j = (uint32_t)e;                                           // (j <= k: rows that stay in front of this one)
        place_out[j] = at;
        seg_out[j] = (uint32_t)((e >> 32) + (f >> 32) - 1ull);                    // (segments started up to and including this row, less one)
    }
}

// ---- query-name order beyond device memory: runs and their merge ----------------------------------------------------------------------------------------
// A run that closes in query-name order (bs_close_run) gets its permutation from the rank pass and the rounds above, over the open run's rows.  Its records
// leave the device, so the NAMES stay: one table of 32-bit words (bamsort_core.hpp: bsort_name_tab_*), every name at a word's edge, zero-filled to the next.
//   k_ns_tab_words  a thread per place of the run's order: the words its name takes (one entry more, 0, so that the scan ends with the run's total)
//   k_ns_pack       a thread per place j of the run's order: the name of record order[j] copied byte by byte from its slab to tab[base + woff[j] ..] (a name is
//                   4-byte aligned in its slab only by accident; the stores are whole words), and what stays per record beside rlen / rfile / roff: the word
//                   offset (64 bits, in rkey's place: this order has no radix key), the name's length and the rank (a byte each)
// The merge at finish (bs_finish_spilled) is the same rank pass and the same rounds over all n places of the concatenation of the runs, with
//   k_ns_rank_keys  the ranks widened to the rank pass's keys
//   k_ns_keys_tab   k_ns_keys with the word read from the table: one aligned 32-bit load per row and round instead of four byte loads through addr
// Every sort is stable, the initial order is (run, place in the run), a run's own order is stable over file order and runs are consecutive ranges of the
// global numbering: equal (name, rank) leave in global record order, which is the definition's rule for ties (svim_amd/bammerge.py).
__global__ void k_ns_tab_words(long long m, const uint32_t* order, const uint8_t* name_len, int64_t* words) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    words[j] = j == m ? 0 : (int64_t)bsort_name_tab_words(name_len[order[j]]);
}
__global__ void k_ns_pack(long long m, const uint32_t* order, const uint64_t* addr, const uint8_t* name_len, const int64_t* woff, uint64_t base, uint32_t* tab, uint64_t* rwoff,
                          uint8_t* rnlen, uint8_t* rrank) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = order[j];
    const uint8_t* r = reinterpret_cast<const uint8_t*>(addr[i]);                 // (the record lies in its slab with its fixed fields and its name field: k_bs_rows, k_ns_names)
    const uint32_t nl = name_len[i];
    const uint64_t at = base + (uint64_t)woff[j];
    bsort_name_tab_pack(r + BSORT_NAME_AT, nl, tab + at);                         // (reads nl bytes, writes bsort_name_tab_words(nl) words: the range the scan gave this name)
    rwoff[j] = at; rnlen[j] = (uint8_t)nl;
    rrank[j] = (uint8_t)bsort_name_rank((uint32_t)r[BSORT_FLAG_AT] | ((uint32_t)r[BSORT_FLAG_AT + 1] << 8));
}
__global__ void k_ns_rank_keys(long long n, const uint8_t* rrank, uint64_t* key) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) key[q] = (uint64_t)rrank[q];
}
// the m active rows of round r over the places of the concatenation of the runs (perm holds places q; rwoff, rnlen: per place)
__global__ void k_ns_keys_tab(long long m, uint32_t r, const uint32_t* perm, const uint32_t* place, const uint32_t* seg, const uint32_t* tab, const uint64_t* rwoff, const uint8_t* rnlen,
                              uint64_t* key, uint32_t* val) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t q = perm[place ? place[k] : (uint32_t)k];
    key[k] = ((uint64_t)(seg ? seg[k] : 0u) << 32) | bsort_name_tab_word(tab, rwoff[q], rnlen[q], r);      // (reads no word behind the name's own)
    val[k] = q;
}

// ---- the gather -----------------------------------------------------------------------------------------------------------------------------------------
struct BsSegs { const int64_t* soff; const uint64_t* saddr; long long n_seg; };      // soff: n_seg + 1 entries, soff[0] = 0, soff[n_seg] = the stream's size

// largest j in [0, n) with soff[j] <= x (soff[0] <= x), by the 64 lanes of one wave: a probe per lane and step
__device__ __forceinline__ long long bs_find(const int64_t* soff, long long n, long long x) {
    long long a = 0, b = n;
    const int lane = lane_id();
    while (b - a > 1) {
        const long long step = (b - a + 63) >> 6, p = a + (long long)lane * step;
        const unsigned long long ok = __ballot(p < b && soff[p] <= x);          // (lane 0 probes a: always set; the set lanes are a prefix)
        const long long c = (long long)__popcll(ok) - 1;
        a += c * step;
        b = a + step < b ? a + step : b;
    }
    return a;
}
// 16 bytes from any address: the two aligned 16-byte words around them, shifted into place.  Reads at most 15 bytes in front of src and 15 behind src + 16
__device__ __forceinline__ bs_u32x4 bs_load16(uint64_t src) {
    const unsigned sh = (unsigned)(src & 15ull);
    const bs_u32x4* q = reinterpret_cast<const bs_u32x4*>(src - sh);
    const bs_u32x4 lo = q[0];
    if (sh == 0u) return lo;
    const bs_u32x4 hi = q[1];
    const unsigned ws = sh >> 2, bsh = sh & 3u;
    const uint32_t s0 = ws == 0u ? lo.x : ws == 1u ? lo.y : ws == 2u ? lo.z : lo.w;
    const uint32_t s1 = ws == 0u ? lo.y : ws == 1u ? lo.z : ws == 2u ? lo.w : hi.x;
    const uint32_t s2 = ws == 0u ? lo.z : ws == 1u ? lo.w : ws == 2u ? hi.x : hi.y;
    const uint32_t s3 = ws == 0u ? lo.w : ws == 1u ? hi.x : ws == 2u ? hi.y : hi.z;
    const uint32_t s4 = ws == 0u ? hi.x : ws == 1u ? hi.y : ws == 2u ? hi.z : hi.w;
    bs_u32x4 r;
    r.x = __builtin_amdgcn_alignbyte(s1, s0, bsh); r.y = __builtin_amdgcn_alignbyte(s2, s1, bsh);
    r.z = __builtin_amdgcn_alignbyte(s3, s2, bsh); r.w = __builtin_amdgcn_alignbyte(s4, s3, bsh);
    return r;
}
// stream bytes [lo, lo + n_bytes) -> dst[0, n_bytes); lo is a multiple of 16 and dst 16-byte aligned
__global__ __launch_bounds__(BS_T) void k_bs_gather(BsSegs G, long long lo, long long n_bytes, uint8_t* dst) {
    __shared__ long long s_off[BS_SEGS + 1];
    __shared__ unsigned long long s_addr[BS_SEGS];
    __shared__ long long s_j[2];
    const long long tiles = (n_bytes + BS_TILE - 1) / BS_TILE, end = lo + n_bytes;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long t_lo = lo + t * BS_TILE, t_hi = t_lo + BS_TILE < end ? t_lo + BS_TILE : end;
        __syncthreads();                                                       // (the tile before is done with the table)
        if (threadIdx.x < 64) {
            const long long j0 = bs_find(G.soff, G.n_seg, t_lo), j1 = bs_find(G.soff, G.n_seg, t_hi - 1);
            if (threadIdx.x == 0) { s_j[0] = j0; s_j[1] = j1; }
        }
        __syncthreads();
        const long long j0 = s_j[0], m = s_j[1] - j0 + 1;                      // the m segments that hold bytes of the tile
        const bool staged = m <= BS_SEGS;                                      // (always, for records of at least 36 bytes; the table is read in place otherwise)
        if (staged) for (long long k = threadIdx.x; k <= m; k += BS_T) { s_off[k] = G.soff[j0 + k]; if (k < m) s_addr[k] = G.saddr[j0 + k]; }
        __syncthreads();
        const int64_t* goff = G.soff + j0; const uint64_t* gaddr = G.saddr + j0;
#define BS_OFF(k) (staged ? s_off[(k)] : (long long)goff[(k)])
#define BS_ADDR(k) (staged ? (uint64_t)s_addr[(k)] : gaddr[(k)])
        for (long long w = t_lo + 16ll * threadIdx.x; w < t_hi; w += 16ll * BS_T) {
            long long a = 0, b = m;                                            // the segment of byte w: the largest k with off[k] <= w
            while (b - a > 1) { const long long mid = (a + b) >> 1; if (BS_OFF(mid) <= w) a = mid; else b = mid; }
            long long k = a;
            uint8_t* d = dst + (w - lo);
            if (w + 16 <= t_hi && w + 16 <= BS_OFF(k + 1)) {
                *reinterpret_cast<bs_u32x4*>(d) = bs_load16(BS_ADDR(k) + (uint64_t)(w - BS_OFF(k)));
                continue;
            }
            // a word with a segment edge inside, or the piece's last, partial word: byte by byte
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            const int nb = (int)(t_hi - w < 16 ? t_hi - w : 16);
            for (int i = 0; i < nb; i++) {
                const long long p = w + i;
                while (p >= BS_OFF(k + 1)) k++;                                // (p < t_hi <= off[m]: k stays below m)
                const uint32_t byte = *reinterpret_cast<const uint8_t*>(BS_ADDR(k) + (uint64_t)(p - BS_OFF(k)));
                v[i >> 2] |= byte << (8 * (i & 3));
            }
            if (nb == 16) { bs_u32x4 r; r.x = v[0]; r.y = v[1]; r.z = v[2]; r.w = v[3]; *reinterpret_cast<bs_u32x4*>(d) = r; }
            else for (int i = 0; i < nb; i++) d[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
        }
#undef BS_OFF
#undef BS_ADDR
    }
}

// ---- a piece of a spilled sort ----------------------------------------------------------------------------------------------------------------------------
// stream bytes [lo, hi) lie in segments j0 .. j1 (found as the gather finds them, by wave 0 of every workgroup); a thread per run: the in-run range [a, b) of
// the records at global positions [max(j0, 1) - 1, j1) and its byte range in the run's stream -> cuts[2 r], cuts[2 r + 1]; j0, j1 -> cuts[2 n_runs ..]
__global__ __launch_bounds__(BS_T) void k_bs_piece_cuts(const int64_t* soff, long long n_seg, long long lo, long long hi, const uint32_t* gpos, const int64_t* roff, const int64_t* run_base,
                                                        const int64_t* run_bytes, long long n_runs, int64_t* cuts) {
    __shared__ long long s_j[2];
    if (threadIdx.x < 64) {
        const long long j0 = bs_find(soff, n_seg, lo), j1 = bs_find(soff, n_seg, hi - 1);
        if (threadIdx.x == 0) { s_j[0] = j0; s_j[1] = j1; }
    }
    __syncthreads();
    const long long j0 = s_j[0], j1 = s_j[1];
    const long long r = (long long)blockIdx.x * BS_T + threadIdx.x;
    if (r == 0) { cuts[2 * n_runs] = j0; cuts[2 * n_runs + 1] = j1; }
    if (r >= n_runs) return;
    const int64_t base = run_base[r], cnt = run_base[r + 1] - base;
    int64_t a, b;
    bsort_piece_cut(gpos + base, cnt, (j0 > 0 ? j0 : 1) - 1, j1, &a, &b);
    cuts[2 * r] = a < cnt ? roff[base + a] : run_bytes[r];
    cuts[2 * r + 1] = b < cnt ? roff[base + b] : run_bytes[r];
}
// the records of the piece, segments max(j0, 1) .. j1: where they lie in the staging buffer (stage[r]: where the run's byte range starts there)
__global__ void k_bs_piece_addr(long long j_first, long long j_last, const uint32_t* srun, const int64_t* sroff, const uint64_t* stage, const int64_t* cuts, uint64_t* saddr) {
    const long long j = j_first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > j_last) return;
    const uint32_t r = srun[j];
    saddr[j] = stage[r] + (uint64_t)(sroff[j] - cuts[2 * r]);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------
struct BsRun { int64_t base, count, file_off, bytes; };     // records [base, base + count) of the file; the run's stream at file_off of the spill file
struct BamSort {
    int32_t n_ref = 0; int64_t max_bytes = 0;
    int64_t n = 0, cap = 0;
    std::vector<void*> slabs; int64_t arena_bytes = 0;
    DevBuf key, len, addr, bad;                              // rows, in file order
    BamIndex* rows = nullptr;                                // tid, pos, end, flag of every record, in file order (bamindex.hip's table)
    DevBuf key2, val, perm, sort_tmp, scan_tmp, slen, soff, saddr, hdr;
    bool finished = false;
    int64_t stream_bytes = 0, n_blocks = 0, next_block = 0; bool broken = false;
    std::vector<int64_t> h_csize;                            // compressed size of every block encoded so far
    // the encoder's buffers, one piece
    DevBuf piece, blocks, crc, crc_shift, tok, hist, nt, codes, bsize, coff, kinds, slots, out, coff_all;
    int64_t piece_bytes = 0, out_bytes = 0; bool have_piece = false;
    double t_append = 0;
    svx_bam_sort_stats stats;
    // spilling (bamsort_begin with a directory): the runs closed so far lie in one unlinked file; key / len / addr hold the rows of the open run only
    bool spill = false; std::string spill_dir; int fd = -1; int64_t spill_piece = BS_SPILL_PIECE;
    int64_t file_bytes = 0, total_bytes = 0 /* record bytes of all runs and the arena */, run_first = 0 /* the open run's first record */, n_slabs_all = 0;
    std::vector<BsRun> runs;
    DevBuf rkey, rlen, rfile, roff; int64_t rcap = 0;        // every record of a closed run, in run order: key, length, file index, offset in the run's stream
    DevBuf gp, srun, sroff, gpos, run_base, run_bytes, cuts, stage_at, stage;
    std::vector<uint8_t> h_io;                               // the host's side of the file's traffic
    std::vector<int64_t> h_cuts;                             // of the piece being encoded: 2 n_runs byte offsets, j0, j1
    svx_bam_sort_spill_stats sp;
    // chunks of a merge (BamSortChunk::tid_map): the merged refID column of the chunk being appended, and what k_bs_translate has done since begin
    DevBuf xtid; hipEvent_t tr_ev[2] = {nullptr, nullptr}; int64_t tr_chunks = 0, tr_records = 0, tr_bytes = 0; double tr_ms = 0;
    // query-name order (bamsort_begin with BSORT_QUERYNAME): the name lengths, the sorted payload, the active places and their segments (two of each: a round
    // reads one and writes the other), the flags of a round and their scan; all of it goes back at the end of finish
    int order = BSORT_COORDINATE;
    DevBuf ns_len, ns_val, ns_place[2], ns_seg[2], ns_flags, ns_ex;
    svx_bam_name_sort_stats ns;
    // runs in query-name order: the name table (32-bit words, grows by doubling, kept), per record of a closed run its name length and rank (rkey holds the
    // word offset of its name), the words per place of the run being closed and their scan; all of it goes back at the end of finish
    DevBuf ntab, rnlen, rrank, ns_words, ns_woff; int64_t ntab_words = 0;
    svx_bam_name_spill_stats nsp;
};
static inline double bs_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int bamsort_begin(BamSort** s, int64_t max_bytes, int32_t n_ref, const char* spill_dir, int order) {
    if (max_bytes < 0 || n_ref < 0 || (order != BSORT_COORDINATE && order != BSORT_QUERYNAME)) return svx_fail(SVX_E_ARG, "BAM sort: bad argument", __FILE__, __LINE__, hipSuccess);
    if (spill_dir) {
        struct stat sb;
        if (!*spill_dir || stat(spill_dir, &sb) != 0 || !S_ISDIR(sb.st_mode) || access(spill_dir, W_OK | X_OK) != 0)
            return svx_fail(SVX_E_ARG, "BAM sort: the spill directory does not exist or cannot be written to", __FILE__, __LINE__, hipSuccess);
    }
    if (!*s) *s = new BamSort();
    BamSort* S = *s;
    bamsort_drop(S);
    S->n_ref = n_ref; S->max_bytes = max_bytes; S->order = order;
    S->spill = spill_dir != nullptr; S->spill_dir = spill_dir ? spill_dir : "";
    S->spill_piece = BS_SPILL_PIECE;                         // test hook: SVX_BAM_SORT_SPILL_PIECE_KB, so that small runs leave in several pieces
    { const char* e = getenv("SVX_BAM_SORT_SPILL_PIECE_KB"); if (e && atoll(e) > 0 && atoll(e) <= (BS_SPILL_PIECE >> 10)) S->spill_piece = atoll(e) << 10; }
    memset(&S->stats, 0, sizeof S->stats); memset(&S->sp, 0, sizeof S->sp); memset(&S->ns, 0, sizeof S->ns); memset(&S->nsp, 0, sizeof S->nsp);
    SVXCHK(bamindex_begin(&S->rows));
    SVXCHK(S->bad.reserve(64));
    HIPCHK(hipMemset(S->bad.p, 0, 64));
    return SVX_OK;
}
void bamsort_drop(BamSort* S) {
    if (!S) return;
    for (void* p : S->slabs) (void)hipFree(p);
    S->slabs.clear(); S->arena_bytes = 0;
    DevBuf* all[] = {&S->key, &S->len, &S->addr, &S->key2, &S->val, &S->perm, &S->sort_tmp, &S->scan_tmp, &S->slen, &S->soff, &S->saddr, &S->hdr, &S->piece, &S->blocks, &S->crc, &S->tok,
                     &S->hist, &S->nt, &S->codes, &S->bsize, &S->coff, &S->kinds, &S->slots, &S->out, &S->coff_all,
                     &S->rkey, &S->rlen, &S->rfile, &S->roff, &S->gp, &S->srun, &S->sroff, &S->gpos, &S->run_base, &S->run_bytes, &S->cuts, &S->stage_at, &S->stage,
                     &S->ns_len, &S->ns_val, &S->ns_place[0], &S->ns_place[1], &S->ns_seg[0], &S->ns_seg[1], &S->ns_flags, &S->ns_ex,
                     &S->ntab, &S->rnlen, &S->rrank, &S->ns_words, &S->ns_woff};
    for (auto* b : all) b->release();
    S->ntab_words = 0;
    if (S->fd >= 0) { (void)close(S->fd); S->fd = -1; }      // (unlinked when it was opened: its blocks go back now)
    S->runs.clear(); S->file_bytes = S->total_bytes = S->run_first = S->n_slabs_all = 0; S->rcap = 0;
    S->h_io.clear(); S->h_io.shrink_to_fit(); S->h_cuts.clear();
    bamindex_drop(S->rows);
    S->n = S->cap = 0; S->finished = false; S->have_piece = false; S->stream_bytes = S->n_blocks = S->next_block = 0; S->broken = false; S->t_append = 0;
    S->piece_bytes = S->out_bytes = 0;
    S->h_csize.clear(); S->h_csize.shrink_to_fit();
    S->xtid.release(); S->tr_chunks = S->tr_records = S->tr_bytes = 0; S->tr_ms = 0;
}
void bamsort_destroy(BamSort* S) {
    if (!S) return;
    bamsort_drop(S);
    bamindex_destroy(S->rows);
    S->bad.release(); S->crc_shift.release();
    for (auto& e : S->tr_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    delete S;
}

// ---- spilling: a run is closed ----------------------------------------------------------------------------------------------------------------------------
static int bs_io_fail(const char* what, long long at, long long n_bytes) {
    char msg[200]; snprintf(msg, sizeof msg, "BAM sort: %s of %lld bytes at offset %lld of the spill file failed or was short (%s)", what, n_bytes, at, errno ? strerror(errno) : "no error code");
    return svx_fail(SVX_E_IO, msg, __FILE__, __LINE__, hipSuccess);
}
static int bs_spill_open(BamSort* S) {
    std::string path = S->spill_dir + "/svx_sort_spill_XXXXXX";
    S->fd = mkostemp(&path[0], O_CLOEXEC);
    if (S->fd < 0) return svx_fail(SVX_E_IO, "BAM sort: the spill file cannot be created", __FILE__, __LINE__, hipSuccess);
    (void)unlink(path.c_str());                              // nothing is left behind, whatever ends the process
    S->file_bytes = 0;
    return SVX_OK;
}
static int bs_name_extents(BamSort* S, int64_t n, int* bad, hipStream_t st);
static int bs_name_order(BamSort* S, int64_t n, uint32_t* perm, const uint32_t* tab, const uint64_t* rwoff, const uint8_t* rnlen, svx_bam_name_sort_stats& X, double t0, hipStream_t st);
static void bs_name_release(BamSort* S);
// a run closes in query-name order: the checks whose records are about to leave the device, the run's permutation into S->perm by the rank pass and the rounds
// over the open run's m rows, and the run's names into the table, in the run's order, BEFORE the slabs go back.  rkey / rnlen / rrank hold first + m entries
static int bs_close_run_names(BamSort* S, int64_t first, int64_t m, hipStream_t st) {
    int bad = 0;
    SVXCHK(svx_d2h(&bad, S->bad.p, 4, st));                  // (k_ns_names relies on every record holding its fixed fields)
    if (bad & BSORT_BAD_MATE) return svx_fail(SVX_E_ARG, "BAM merge: a record of a file whose ids are translated names a mate reference its header does not have", __FILE__, __LINE__, hipSuccess);
    if (bad & (BSORT_BAD_SIZE | BSORT_BAD_TID)) return svx_fail(SVX_E_ARG, "BAM sort: a record names a reference the header does not have, or is shorter than its fixed fields", __FILE__, __LINE__, hipSuccess);
    const double t0 = bs_now();
    SVXCHK(bs_name_extents(S, m, &bad, st));
    if (bad & BSORT_BAD_NAME) return svx_fail(SVX_E_ARG, "BAM sort: a record has no name field, or one that runs past the record's end (query-name order)", __FILE__, __LINE__, hipSuccess);
    // (BSORT_BAD_POS waits for finish, behind every SVX_E_ARG of every run, as the definition orders them)
    svx_bam_name_sort_stats X;
    memset(&X, 0, sizeof X);
    SVXCHK(bs_name_order(S, m, S->perm.as<uint32_t>(), nullptr, nullptr, nullptr, X, bs_now(), st));
    const double t1 = bs_now();
    SVXCHK(S->ns_words.reserve((size_t)(m + 1) * 8)); SVXCHK(S->ns_woff.reserve((size_t)(m + 1) * 8));
    k_ns_tab_words<<<BS_GRID(m + 1), BS_T, 0, st>>>(m, S->perm.as<uint32_t>(), S->ns_len.as<uint8_t>(), S->ns_words.as<int64_t>());
    HIPCHK(hipGetLastError());
    SVXCHK((svx_exclusive_scan<int64_t, int64_t>(S->ns_words.as<int64_t>(), S->ns_woff.as<int64_t>(), m + 1, st, S->scan_tmp)));
    int64_t words = 0;
    SVXCHK(svx_d2h(&words, S->ns_woff.as<int64_t>() + m, 8, st));
    if (words < m || words > m * 64) return svx_fail(SVX_E_STATE, "BAM sort: a run's names take less than a word or more than 64 words each (internal error)", __FILE__, __LINE__, hipSuccess);
    const int64_t need = S->ntab_words + words;
    if ((size_t)need * 4 > S->ntab.cap) SVXCHK(S->ntab.reserve((size_t)std::max<int64_t>(std::max<int64_t>(need, 2 * (int64_t)(S->ntab.cap / 4)), 1 << 16) * 4, true, st));
    k_ns_pack<<<BS_GRID(m), BS_T, 0, st>>>(m, S->perm.as<uint32_t>(), S->addr.as<uint64_t>(), S->ns_len.as<uint8_t>(), S->ns_woff.as<int64_t>(), (uint64_t)S->ntab_words, S->ntab.as<uint32_t>(),
                                           S->rkey.as<uint64_t>() + first, S->rnlen.as<uint8_t>() + first, S->rrank.as<uint8_t>() + first);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    S->ntab_words = need;
    bs_name_release(S);
    svx_bam_name_spill_stats& P = S->nsp;
    P.n_runs++; P.run_rounds += X.rounds; P.run_active_rows += X.active_total; P.table_bytes = S->ntab_words * 4;
    P.t_run_sort_ms += (t1 - t0) * 1e3; P.t_pack_ms += (bs_now() - t1) * 1e3;
    return SVX_OK;
}
// the open run - records [run_first, n), their bytes in the slabs - sorted, laid out, written behind the runs before it; the slabs go back
static int bs_close_run(BamSort* S, hipStream_t st) {
    const int64_t first = S->run_first, m = S->n - first;
    if (m <= 0) return SVX_OK;
    const double t0 = bs_now();
    const bool by_name = S->order == BSORT_QUERYNAME;
    if (S->fd < 0) SVXCHK(bs_spill_open(S));
    if (S->n + 1 > S->rcap) {                                // (roff takes one entry more: the scan ends with the run's size)
        const int64_t ncap = std::max<int64_t>(std::max<int64_t>(S->n + 1, 2 * S->rcap), 1 << 16);
        SVXCHK(S->rkey.reserve((size_t)ncap * 8, true, st)); SVXCHK(S->rlen.reserve((size_t)ncap * 4, true, st)); SVXCHK(S->rfile.reserve((size_t)ncap * 4, true, st));
        SVXCHK(S->roff.reserve((size_t)ncap * 8, true, st));
        if (by_name) { SVXCHK(S->rnlen.reserve((size_t)ncap, true, st)); SVXCHK(S->rrank.reserve((size_t)ncap, true, st)); }
        S->rcap = ncap;
    }
    SVXCHK(S->val.reserve((size_t)m * 4)); SVXCHK(S->perm.reserve((size_t)(m + 1) * 4)); SVXCHK(S->slen.reserve((size_t)(m + 1) * 8)); SVXCHK(S->saddr.reserve((size_t)(m + 1) * 8));
    if (by_name) SVXCHK(bs_close_run_names(S, first, m, st));
    else {
        k_bs_iota<<<BS_GRID(m), BS_T, 0, st>>>(m, S->val.as<uint32_t>());
        SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, S->key.as<uint64_t>(), S->rkey.as<uint64_t>() + first, S->val.as<uint32_t>(), S->perm.as<uint32_t>(), m, 0, bsort_key_bits(S->n_ref)));
    }
    k_bs_run_layout<<<BS_GRID(m + 1), BS_T, 0, st>>>(m, S->perm.as<uint32_t>(), S->len.as<uint32_t>(), S->addr.as<uint64_t>(), (uint32_t)first, S->slen.as<int64_t>(), S->saddr.as<uint64_t>(),
                                                     S->rlen.as<uint32_t>() + first, S->rfile.as<uint32_t>() + first);
    HIPCHK(hipGetLastError());
    int64_t* roff = S->roff.as<int64_t>() + first;
    SVXCHK((svx_exclusive_scan<int64_t, int64_t>(S->slen.as<int64_t>(), roff, m + 1, st, S->scan_tmp)));
    int64_t total = 0;
    SVXCHK(svx_d2h(&total, roff + m, 8, st));
    if (total != S->arena_bytes) return svx_fail(SVX_E_STATE, "BAM sort: a run's stream is not the size of its slabs (internal error)", __FILE__, __LINE__, hipSuccess);
    const int64_t step = std::min<int64_t>(S->spill_piece, total);
    SVXCHK(S->piece.reserve((size_t)step + 256));
    if ((int64_t)S->h_io.size() < step) S->h_io.resize((size_t)step);
    const BsSegs G{roff, S->saddr.as<uint64_t>(), m};
    for (int64_t lo = 0; lo < total; lo += step) {
        const int64_t pb = std::min<int64_t>(step, total - lo);
        const long long tiles = (pb + BS_TILE - 1) / BS_TILE;
        k_bs_gather<<<(unsigned)std::min<long long>(tiles, BS_MAX_GRID), BS_T, 0, st>>>(G, lo, pb, S->piece.as<uint8_t>());
        HIPCHK(hipGetLastError());
        SVXCHK(svx_d2h(S->h_io.data(), S->piece.p, (size_t)pb, st));
        for (int64_t done = 0; done < pb;) {
            errno = 0;
            const ssize_t w = pwrite(S->fd, S->h_io.data() + done, (size_t)(pb - done), (off_t)(S->file_bytes + lo + done));
            if (w <= 0) { if (w < 0 && errno == EINTR) continue; return bs_io_fail("a write", S->file_bytes + lo + done, pb - done); }
            done += w;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    S->runs.push_back(BsRun{first, m, S->file_bytes, total});
    S->file_bytes += total;
    for (void* p : S->slabs) (void)hipFree(p);
    S->slabs.clear(); S->arena_bytes = 0; S->run_first = S->n;
    S->sp.n_runs = (int64_t)S->runs.size(); S->sp.spilled_bytes = S->file_bytes; S->sp.max_run_bytes = std::max<int64_t>(S->sp.max_run_bytes, total);
    S->sp.t_spill_ms += (bs_now() - t0) * 1e3;
    return SVX_OK;
}

int bamsort_append(BamSort* S, const BamSortChunk& c, hipStream_t st) {
    if (!S || S->finished || c.n < 0 || c.end_byte < c.first_byte) return svx_fail(SVX_E_ARG, "BAM sort: bad chunk", __FILE__, __LINE__, hipSuccess);
    const bool translated = c.n_ref_file >= 0 && !c.identity;
    if (c.n_ref_file > S->n_ref || (translated && c.n_ref_file > 0 && !c.tid_map)) return svx_fail(SVX_E_ARG, "BAM sort: a chunk of a file whose dictionary is not part of the sort's", __FILE__, __LINE__, hipSuccess);
    if (c.n == 0) return SVX_OK;
    const double t0 = bs_now();
    if (S->n + c.n > 0xffffffffll) return svx_fail(SVX_E_CAPACITY, "BAM sort: more than 2^32 - 1 records", __FILE__, __LINE__, hipSuccess);
    const size_t need = (size_t)(c.end_byte - c.first_byte);
    double t_closing = 0;
    // runs in query-name order take more than the chunk and its rows when they close: the table (it doubles: as much again as it holds), per record so far
    // and coming the rows that stay of this order (26 bytes: word offset, length, file index, offset in the run, name length, rank) and the 37 bytes the rounds take
    const size_t name_extra = S->spill && S->order == BSORT_QUERYNAME ? S->ntab.cap + (size_t)(S->n + c.n) * BSORT_NAME_ROW_BYTES : 0;
    for (int attempt = 0;; attempt++) {
        char msg[200]; msg[0] = 0;
        size_t free_b = 0, total_b = 0;
        if (S->max_bytes > 0 && S->arena_bytes + (int64_t)need > S->max_bytes)
            snprintf(msg, sizeof msg, "BAM sort: the records do not fit into the arena (%lld bytes held, %zu more, limit %lld)", (long long)S->arena_bytes, need, (long long)S->max_bytes);
        else if (S->max_bytes == 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + name_extra + (size_t)c.n * 64 + ((size_t)64 << 20) > free_b)
            snprintf(msg, sizeof msg, "BAM sort: the records do not fit into device memory (%lld bytes held, %zu more, %zu free)", (long long)S->arena_bytes, need, free_b);
        if (!msg[0]) break;
        // with a spill directory the open run is closed and the chunk starts the next one; a chunk that alone passes the limit has nowhere to go
        if (!S->spill || attempt > 0 || S->arena_bytes == 0) return svx_fail(SVX_E_CAPACITY, msg, __FILE__, __LINE__, hipSuccess);
        const double tc = bs_now();
        SVXCHK(bs_close_run(S, st));
        t_closing = bs_now() - tc;
    }
    const int64_t n_run = S->n - S->run_first;               // rows of the open run (all rows, when nothing spills)
    if (n_run + c.n > S->cap) {                              // the rows grow by doubling, kept; the slabs never move
        const int64_t ncap = std::max<int64_t>(std::max<int64_t>(n_run + c.n, 2 * S->cap), 1 << 16);
        SVXCHK(S->key.reserve((size_t)ncap * 8, true, st)); SVXCHK(S->len.reserve((size_t)ncap * 4, true, st)); SVXCHK(S->addr.reserve((size_t)ncap * 8, true, st));
        S->cap = ncap;
    }
    void* slab = nullptr;
    HIPCHK(hipMalloc(&slab, need + BS_PAD));
    S->slabs.push_back(slab); S->arena_bytes += (int64_t)need; S->total_bytes += (int64_t)need; S->n_slabs_all++;
    S->sp.max_chunk_bytes = std::max<int64_t>(S->sp.max_chunk_bytes, (int64_t)need);
    HIPCHK(hipMemcpyAsync(slab, c.stream + c.first_byte, need, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync((uint8_t*)slab + need, 0, BS_PAD, st));
    const int32_t* tid = c.tid;                              // the column the key and the index row are made of
    int32_t n_ref_check = c.n_ref_file >= 0 ? c.n_ref_file : S->n_ref;
    if (translated) {
        // the ids of this file are not the merged ones: mapped for the rows, patched in the slab (an identity file takes no launch and keeps its bytes)
        SVXCHK(S->xtid.reserve((size_t)c.n * 4));
        for (auto& e : S->tr_ev) if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(S->tr_ev[0], st));
        k_bs_translate<<<BS_GRID(c.n), BS_T, 0, st>>>(c.n, c.rec_off, c.first_byte, c.end_byte, (uint8_t*)slab, c.tid, c.tid_map, c.n_ref_file, S->xtid.as<int32_t>(), S->bad.as<int>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S->tr_ev[1], st));
        tid = S->xtid.as<int32_t>(); n_ref_check = S->n_ref;  // (the mapped ids lie in the merged dictionary; what the file's own did not hold is flagged)
    }
    k_bs_rows<<<BS_GRID(c.n), BS_T, 0, st>>>(c.n, c.stream, c.rec_off, c.first_byte, c.end_byte, (uint64_t)(uintptr_t)slab, tid, c.pos, c.flag, n_ref_check, S->n_ref,
                                             S->key.as<uint64_t>() + n_run, S->len.as<uint32_t>() + n_run, S->addr.as<uint64_t>() + n_run, S->bad.as<int>());
    HIPCHK(hipGetLastError());
    // the index rows: end from the CIGAR (CG included) by bamindex.hip's append; its virtual offsets are replaced when the sorted file's are known
    const uint64_t blk_start = 0, blk_vbase = 0;
    const BamIndexChunk ic{c.n, tid, c.pos, c.flag, c.cigar_off, c.cigar, c.rec_off, &blk_start, &blk_vbase, 1};
    SVXCHK(bamindex_append(S->rows, ic, st));               // (drains the stream: the chunk's arrays, its stream and xtid are no longer read)
    if (translated) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, S->tr_ev[0], S->tr_ev[1]) == hipSuccess) S->tr_ms += ms;
        S->tr_chunks++; S->tr_records += c.n; S->tr_bytes += c.n * 32;      // per record: 8 of rec_off, 4 + 4 + 4 read (size, refID column, mate), 4 written, 8 patched
    }
    S->n += c.n;
    S->t_append += bs_now() - t0 - t_closing;
    return SVX_OK;
}

// finish with runs in the file: the open run joins them, then the merge.  The header lies in S->hdr.
static int bs_finish_spilled(BamSort* S, int64_t header_bytes, double t0, hipStream_t st) {
    const int64_t n = S->n;
    SVXCHK(bs_close_run(S, st));
    const double t1 = bs_now();
    const int64_t n_runs = (int64_t)S->runs.size();
    std::vector<int64_t> h_base((size_t)n_runs + 1, n), h_bytes((size_t)n_runs, 0);
    for (int64_t r = 0; r < n_runs; r++) { h_base[(size_t)r] = S->runs[(size_t)r].base; h_bytes[(size_t)r] = S->runs[(size_t)r].bytes; }
    SVXCHK(S->run_base.reserve((size_t)(n_runs + 1) * 8)); SVXCHK(S->run_bytes.reserve((size_t)n_runs * 8));
    SVXCHK(svx_h2d(S->run_base.p, h_base.data(), (size_t)(n_runs + 1) * 8, st)); SVXCHK(svx_h2d(S->run_bytes.p, h_bytes.data(), (size_t)n_runs * 8, st));
    // the run-sorted keys lie back to back in rkey: one stable sort, the place in the concatenation as payload.  Equal keys keep the order run, place in the run
    const bool by_name = S->order == BSORT_QUERYNAME;
    SVXCHK(S->key2.reserve((size_t)n * 8)); SVXCHK(S->val.reserve((size_t)n * 4)); SVXCHK(S->gp.reserve((size_t)n * 4));
    if (by_name) {
        // query-name order: the rank pass and the rounds over all n places, the words from the name table; gp = the places in (name, rank, run, place in the run) order
        SVXCHK(S->key.reserve((size_t)n * 8));
        k_ns_rank_keys<<<BS_GRID(n), BS_T, 0, st>>>(n, S->rrank.as<uint8_t>(), S->key.as<uint64_t>());
        HIPCHK(hipGetLastError());
        SVXCHK(bs_name_order(S, n, S->gp.as<uint32_t>(), S->ntab.as<uint32_t>(), S->rkey.as<uint64_t>(), S->rnlen.as<uint8_t>(), S->ns, t1, st));
        bs_name_release(S);
    } else {
        k_bs_iota<<<BS_GRID(n), BS_T, 0, st>>>(n, S->val.as<uint32_t>());
        SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, S->rkey.as<uint64_t>(), S->key2.as<uint64_t>(), S->val.as<uint32_t>(), S->gp.as<uint32_t>(), n, 0, bsort_key_bits(S->n_ref)));
    }
    HIPCHK(hipStreamSynchronize(st));
    const double t2 = bs_now();
    SVXCHK(S->slen.reserve((size_t)(n + 2) * 8)); SVXCHK(S->soff.reserve((size_t)(n + 2) * 8)); SVXCHK(S->saddr.reserve((size_t)(n + 2) * 8));
    SVXCHK(S->srun.reserve((size_t)(n + 2) * 4)); SVXCHK(S->sroff.reserve((size_t)(n + 2) * 8)); SVXCHK(S->gpos.reserve((size_t)n * 4));
    k_bs_spill_layout<<<BS_GRID(n + 2), BS_T, 0, st>>>(n, S->gp.as<uint32_t>(), S->rlen.as<uint32_t>(), S->rfile.as<uint32_t>(), S->roff.as<int64_t>(), S->run_base.as<int64_t>(), n_runs,
                                                       (uint64_t)(uintptr_t)S->hdr.p, header_bytes, S->perm.as<uint32_t>(), S->slen.as<int64_t>(), S->srun.as<uint32_t>(),
                                                       S->sroff.as<int64_t>(), S->gpos.as<uint32_t>(), S->saddr.as<uint64_t>());
    HIPCHK(hipGetLastError());
    SVXCHK((svx_exclusive_scan<int64_t, int64_t>(S->slen.as<int64_t>(), S->soff.as<int64_t>(), n + 2, st, S->scan_tmp)));
    int64_t total = 0;
    SVXCHK(svx_d2h(&total, S->soff.as<int64_t>() + n + 1, 8, st));
    if (total != header_bytes + S->total_bytes || S->file_bytes != S->total_bytes)
        return svx_fail(SVX_E_STATE, "BAM sort: the stream's size is not the header's plus the runs' (internal error)", __FILE__, __LINE__, hipSuccess);
    // resident from here on: the permutation, the segment table (offset, run, offset in the run), gpos, the runs' record offsets and the index rows
    S->key.release(); S->key2.release(); S->val.release(); S->len.release(); S->addr.release(); S->slen.release(); S->sort_tmp.release();
    S->rkey.release(); S->rlen.release(); S->rfile.release(); S->gp.release();
    S->ntab.release(); S->rnlen.release(); S->rrank.release();             // (the table's size stays in the stats)
    S->cap = 0;
    const double t3 = bs_now();
    if (by_name) { S->ns.t_layout_ms = (t3 - t2) * 1e3; S->ns.n_records = n; S->ns.word_bytes = BSORT_NAME_WORD; }
    S->stream_bytes = total; S->n_blocks = (total + BSORT_BLOCK - 1) / BSORT_BLOCK + 1; S->next_block = 0; S->broken = false;
    S->h_csize.assign((size_t)S->n_blocks, 0);
    S->finished = true;
    S->stats.t_append_ms = S->t_append * 1e3; S->stats.t_sort_ms = (t2 - t1) * 1e3; S->stats.t_layout_ms = (t3 - t2) * 1e3; S->stats.t_finish_ms = (t3 - t0) * 1e3;
    S->stats.n_records = n; S->stats.n_slabs = S->n_slabs_all; S->stats.arena_bytes = S->total_bytes; S->stats.stream_bytes = total; S->stats.n_blocks = S->n_blocks;
    S->stats.key_bits = by_name ? 0 : bsort_key_bits(S->n_ref);
    S->sp.t_merge_ms += (t3 - t1) * 1e3;
    return SVX_OK;
}

// query-name order, in front of the sort: the names' extents, ranks and checks (k_ns_names); *bad gets BSORT_BAD_NAME.  The caller has refused BSORT_BAD_SIZE:
// every record lies inside its slab and holds its fixed fields
static int bs_name_extents(BamSort* S, int64_t n, int* bad, hipStream_t st) {
    if (n == 0) return SVX_OK;
    SVXCHK(S->ns_len.reserve((size_t)n));
    k_ns_names<<<BS_GRID(n), BS_T, 0, st>>>(n, S->addr.as<uint64_t>(), S->len.as<uint32_t>(), S->ns_len.as<uint8_t>(), S->key.as<uint64_t>(), S->bad.as<int>());
    HIPCHK(hipGetLastError());
    SVXCHK(svx_d2h(bad, S->bad.p, 4, st));
    return SVX_OK;
}
// the permutation of query-name order of n rows into perm (the kernels and the rounds: above); S->key holds their ranks.  The rows are records in their slabs
// (S->addr, S->ns_len: the in-memory sort and a run being closed; tab null) or places of the concatenation of the closed runs, their names in the table
// (rwoff, rnlen: the merge at finish).  X: what the rounds were.  The caller gives the round buffers back (bs_name_release)
static int bs_name_order(BamSort* S, int64_t n, uint32_t* perm, const uint32_t* tab, const uint64_t* rwoff, const uint8_t* rnlen, svx_bam_name_sort_stats& X, double t0, hipStream_t st) {
    if (n == 0) return SVX_OK;
    SVXCHK(S->key2.reserve((size_t)n * 8)); SVXCHK(S->val.reserve((size_t)n * 4)); SVXCHK(S->ns_val.reserve((size_t)n * 4));
    for (int k = 0; k < 2; k++) { SVXCHK(S->ns_place[k].reserve((size_t)n * 4)); SVXCHK(S->ns_seg[k].reserve((size_t)n * 4)); }
    SVXCHK(S->ns_flags.reserve((size_t)(n + 1) * 8)); SVXCHK(S->ns_ex.reserve((size_t)(n + 1) * 8));
    uint64_t *key = S->key.as<uint64_t>(), *key2 = S->key2.as<uint64_t>();
    uint32_t *val = S->val.as<uint32_t>(), *val2 = S->ns_val.as<uint32_t>();
    k_bs_iota<<<BS_GRID(n), BS_T, 0, st>>>(n, val);
    SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, key, key2, val, perm, n, 0, 4));
    HIPCHK(hipStreamSynchronize(st));
    const double t1 = bs_now();
    X.t_rank_ms = (t1 - t0) * 1e3;
    int64_t m = n > 1 ? n : 0, n_seg = 1;                    // the active rows and their segments; one record is in order
    int cur = 0;
    for (uint32_t r = 0; m > 0; r++, cur ^= 1) {
        if (r >= BSORT_NAME_MAX_ROUNDS) return svx_fail(SVX_E_STATE, "BAM sort: names still open behind their last possible byte (internal error)", __FILE__, __LINE__, hipSuccess);
        const uint32_t *place = r ? S->ns_place[cur].as<uint32_t>() : nullptr, *seg = r ? S->ns_seg[cur].as<uint32_t>() : nullptr;
        if (tab) k_ns_keys_tab<<<BS_GRID(m), BS_T, 0, st>>>(m, r, perm, place, seg, tab, rwoff, rnlen, key, val);
        else k_ns_keys<<<BS_GRID(m), BS_T, 0, st>>>(m, r, perm, place, seg, S->addr.as<uint64_t>(), S->ns_len.as<uint8_t>(), key, val);
        SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, key, key2, val, val2, m, 0, 32 + (n_seg > 1 ? svx_ceil_log2(n_seg) : 0)));
        k_ns_heads<<<BS_GRID(m + 1), BS_T, 0, st>>>(m, key2, S->ns_flags.as<int64_t>());
        SVXCHK((svx_exclusive_scan<int64_t, int64_t>(S->ns_flags.as<int64_t>(), S->ns_ex.as<int64_t>(), m + 1, st, S->scan_tmp)));
        k_ns_apply<<<BS_GRID(m), BS_T, 0, st>>>(m, val2, S->ns_flags.as<int64_t>(), S->ns_ex.as<int64_t>(), place, perm, S->ns_place[cur ^ 1].as<uint32_t>(), S->ns_seg[cur ^ 1].as<uint32_t>());
        HIPCHK(hipGetLastError());
        uint64_t totals = 0;                                 // the round's one read-back: rows that stay (low half), segments of this round (high half)
        SVXCHK(svx_d2h(&totals, S->ns_ex.as<int64_t>() + m, 8, st));
        X.active_rows[r] = m; X.active_total += m; X.active_max = std::max<int64_t>(X.active_max, m); X.rounds = (int64_t)r + 1;
        const int64_t stay = (int64_t)(totals & 0xffffffffull);
        n_seg = (int64_t)(totals >> 32);
        if (stay > m || n_seg < 1 || n_seg > m) return svx_fail(SVX_E_STATE, "BAM sort: a round's totals are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
        m = stay;
    }
    HIPCHK(hipStreamSynchronize(st));
    X.t_rounds_ms = (bs_now() - t1) * 1e3;
    return SVX_OK;
}
static void bs_name_release(BamSort* S) {
    DevBuf* done[] = {&S->ns_len, &S->ns_val, &S->ns_place[0], &S->ns_place[1], &S->ns_seg[0], &S->ns_seg[1], &S->ns_flags, &S->ns_ex, &S->ns_words, &S->ns_woff};
    for (auto* b : done) b->release();
}

int bamsort_finish(BamSort* S, const uint8_t* header, int64_t header_bytes, hipStream_t st) {
    if (!S || S->finished || !header || header_bytes < 12) return svx_fail(SVX_E_ARG, "BAM sort: bad argument", __FILE__, __LINE__, hipSuccess);
    const int64_t n = S->n;
    if (bamindex_rows(S->rows) != n) return svx_fail(SVX_E_STATE, "BAM sort: the row tables disagree (internal error)", __FILE__, __LINE__, hipSuccess);
    HIPCHK(hipStreamSynchronize(st));
    const double t0 = bs_now();
    int bad = 0;
    SVXCHK(svx_d2h(&bad, S->bad.p, 4, st));
    if (bad & BSORT_BAD_MATE) return svx_fail(SVX_E_ARG, "BAM merge: a record of a file whose ids are translated names a mate reference its header does not have", __FILE__, __LINE__, hipSuccess);
    if (bad & (BSORT_BAD_SIZE | BSORT_BAD_TID)) return svx_fail(SVX_E_ARG, "BAM sort: a record names a reference the header does not have, or is shorter than its fixed fields", __FILE__, __LINE__, hipSuccess);
    const bool by_name = S->order == BSORT_QUERYNAME;
    double t_names = t0;
    if (by_name && !S->runs.empty()) SVXCHK(bs_close_run(S, st));      // (runs in query-name order: the open run's names are checked where every run's were, SVX_E_ARG in front of SVX_E_RANGE)
    else if (by_name) {                                      // (the names' checks are SVX_E_ARG, which goes before SVX_E_RANGE)
        SVXCHK(bs_name_extents(S, n, &bad, st));
        t_names = bs_now();
        if (bad & BSORT_BAD_NAME) return svx_fail(SVX_E_ARG, "BAM sort: a record has no name field, or one that runs past the record's end (query-name order)", __FILE__, __LINE__, hipSuccess);
    }
    if (bad & BSORT_BAD_POS) return svx_fail(SVX_E_RANGE, "BAM sort: a record has a position below -1", __FILE__, __LINE__, hipSuccess);
    SVXCHK(S->hdr.reserve((size_t)header_bytes + BS_PAD));
    HIPCHK(hipMemsetAsync((uint8_t*)S->hdr.p + header_bytes, 0, BS_PAD, st));
    SVXCHK(svx_h2d(S->hdr.p, header, (size_t)header_bytes, st));
    SVXCHK(S->perm.reserve((size_t)(n + 1) * 4));
    if (!S->runs.empty()) return bs_finish_spilled(S, header_bytes, t0, st);      // (no run was closed: exactly the in-memory path, no file)
    if (by_name) { SVXCHK(bs_name_order(S, n, S->perm.as<uint32_t>(), nullptr, nullptr, nullptr, S->ns, t_names, st)); bs_name_release(S); }
    else if (n > 0) {
        SVXCHK(S->key2.reserve((size_t)n * 8)); SVXCHK(S->val.reserve((size_t)n * 4));
        k_bs_iota<<<BS_GRID(n), BS_T, 0, st>>>(n, S->val.as<uint32_t>());
        SVXCHK(svx_sort_pairs_u64_on(st, S->sort_tmp, S->key.as<uint64_t>(), S->key2.as<uint64_t>(), S->val.as<uint32_t>(), S->perm.as<uint32_t>(), n, 0, bsort_key_bits(S->n_ref)));
    }
    HIPCHK(hipStreamSynchronize(st));
    const double t1 = bs_now();
    SVXCHK(S->slen.reserve((size_t)(n + 2) * 8)); SVXCHK(S->soff.reserve((size_t)(n + 2) * 8)); SVXCHK(S->saddr.reserve((size_t)(n + 2) * 8));
    k_bs_layout<<<BS_GRID(n + 2), BS_T, 0, st>>>(n, S->perm.as<uint32_t>(), S->len.as<uint32_t>(), S->addr.as<uint64_t>(), (uint64_t)(uintptr_t)S->hdr.p, header_bytes, S->slen.as<int64_t>(),
                                                 S->saddr.as<uint64_t>());
    HIPCHK(hipGetLastError());
    SVXCHK((svx_exclusive_scan<int64_t, int64_t>(S->slen.as<int64_t>(), S->soff.as<int64_t>(), n + 2, st, S->scan_tmp)));
    int64_t total = 0;
    SVXCHK(svx_d2h(&total, S->soff.as<int64_t>() + n + 1, 8, st));
    if (total != header_bytes + S->arena_bytes) return svx_fail(SVX_E_STATE, "BAM sort: the stream's size is not the header's plus the arena's (internal error)", __FILE__, __LINE__, hipSuccess);
    // what only the sort needed goes back: resident from here on are the arena, the permutation, the segment table and the index rows
    S->key.release(); S->key2.release(); S->val.release(); S->len.release(); S->addr.release(); S->slen.release(); S->sort_tmp.release();
    S->cap = 0;
    const double t2 = bs_now();
    if (by_name) { S->ns.t_names_ms = (t_names - t0) * 1e3; S->ns.t_layout_ms = (t2 - t1) * 1e3; S->ns.n_records = n; S->ns.word_bytes = BSORT_NAME_WORD; }
    S->stream_bytes = total; S->n_blocks = (total + BSORT_BLOCK - 1) / BSORT_BLOCK + 1; S->next_block = 0; S->broken = false;
    S->h_csize.assign((size_t)S->n_blocks, 0);
    S->finished = true;
    S->stats.t_append_ms = S->t_append * 1e3; S->stats.t_sort_ms = (t1 - t0) * 1e3; S->stats.t_layout_ms = (t2 - t1) * 1e3; S->stats.t_finish_ms = (t2 - t0) * 1e3;
    S->stats.n_records = n; S->stats.n_slabs = (int64_t)S->slabs.size(); S->stats.arena_bytes = S->arena_bytes; S->stats.stream_bytes = total; S->stats.n_blocks = S->n_blocks;
    S->stats.key_bits = by_name ? 0 : bsort_key_bits(S->n_ref);
    S->sp.n_runs = n > 0 ? 1 : 0; S->sp.max_run_bytes = S->arena_bytes;      // one run, resident
    return SVX_OK;
}
bool bamsort_finished(const BamSort* S) { return S && S->finished; }
void bamsort_count(const BamSort* S, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks) {
    if (n_records) *n_records = S->n;
    if (stream_bytes) *stream_bytes = S->stream_bytes;
    if (n_blocks) *n_blocks = S->n_blocks;
}

// ---- a piece of a spilled sort: cuts, read-back, addresses ---------------------------------------------------------------------------------------------------
// stream bytes [lo, hi) -> h_cuts (per run the byte range of its stream the piece needs, then j0 and j1); *stage_bytes: the ranges back to back, each padded
static int bs_piece_cuts(BamSort* S, int64_t lo, int64_t hi, int64_t* stage_bytes, hipStream_t st) {
    const double t0 = bs_now();
    const int64_t n_runs = (int64_t)S->runs.size();
    SVXCHK(S->cuts.reserve((size_t)(2 * n_runs + 2) * 8));
    k_bs_piece_cuts<<<BS_GRID(n_runs), BS_T, 0, st>>>(S->soff.as<int64_t>(), S->n + 1, lo, hi, S->gpos.as<uint32_t>(), S->roff.as<int64_t>(), S->run_base.as<int64_t>(), S->run_bytes.as<int64_t>(),
                                                      n_runs, S->cuts.as<int64_t>());
    HIPCHK(hipGetLastError());
    S->h_cuts.assign((size_t)(2 * n_runs + 2), 0);
    SVXCHK(svx_d2h(S->h_cuts.data(), S->cuts.p, (size_t)(2 * n_runs + 2) * 8, st));
    int64_t total = 0;
    for (int64_t r = 0; r < n_runs; r++) {
        const int64_t a = S->h_cuts[(size_t)(2 * r)], b = S->h_cuts[(size_t)(2 * r + 1)];
        if (a < 0 || b < a || b > S->runs[(size_t)r].bytes) return svx_fail(SVX_E_STATE, "svx_bam_sort_encode: a run's byte range lies outside the run (internal error)", __FILE__, __LINE__, hipSuccess);
        if (b > a) total += b - a + BS_PAD;
    }
    const int64_t j0 = S->h_cuts[(size_t)(2 * n_runs)], j1 = S->h_cuts[(size_t)(2 * n_runs + 1)];
    if (j0 < 0 || j1 < j0 || j1 > S->n) return svx_fail(SVX_E_STATE, "svx_bam_sort_encode: the piece's segments lie outside the table (internal error)", __FILE__, __LINE__, hipSuccess);
    *stage_bytes = total;
    S->sp.t_merge_ms += (bs_now() - t0) * 1e3;
    return SVX_OK;
}
static int bs_piece_stage(BamSort* S, int64_t stage_bytes, hipStream_t st) {
    const double t0 = bs_now();
    const int64_t n_runs = (int64_t)S->runs.size();
    const int64_t j0 = S->h_cuts[(size_t)(2 * n_runs)], j1 = S->h_cuts[(size_t)(2 * n_runs + 1)];
    if (j1 < 1) return SVX_OK;                               // (the piece lies inside the header)
    SVXCHK(S->stage.reserve((size_t)stage_bytes + BS_PAD)); SVXCHK(S->stage_at.reserve((size_t)n_runs * 8));
    if ((int64_t)S->h_io.size() < stage_bytes) S->h_io.resize((size_t)stage_bytes);
    std::vector<uint64_t> h_at((size_t)n_runs, 0);
    int64_t at = 0, n_read = 0;
    for (int64_t r = 0; r < n_runs; r++) {
        const int64_t a = S->h_cuts[(size_t)(2 * r)], len = S->h_cuts[(size_t)(2 * r + 1)] - a;
        h_at[(size_t)r] = (uint64_t)(uintptr_t)S->stage.p + (uint64_t)at;
        if (len <= 0) continue;
        for (int64_t done = 0; done < len;) {
            errno = 0;
            const ssize_t g = pread(S->fd, S->h_io.data() + at + done, (size_t)(len - done), (off_t)(S->runs[(size_t)r].file_off + a + done));
            if (g <= 0) { if (g < 0 && errno == EINTR) continue; return bs_io_fail("a read", S->runs[(size_t)r].file_off + a + done, len - done); }
            done += g;
        }
        memset(S->h_io.data() + at + len, 0, BS_PAD);
        at += len + BS_PAD; n_read += len;
    }
    {
        HostCopy hc(st);
        if (at > 0) SVXCHK(hc.h2d(S->stage.p, S->h_io.data(), (size_t)at));
        SVXCHK(hc.h2d(S->stage_at.p, h_at.data(), (size_t)n_runs * 8));
        SVXCHK(hc.finish());
    }
    HIPCHK(hipStreamSynchronize(st));
    const double t1 = bs_now();
    const int64_t j_first = std::max<int64_t>(j0, 1);
    k_bs_piece_addr<<<BS_GRID(j1 - j_first + 1), BS_T, 0, st>>>(j_first, j1, S->srun.as<uint32_t>(), S->sroff.as<int64_t>(), S->stage_at.as<uint64_t>(), S->cuts.as<int64_t>(), S->saddr.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    S->sp.max_stage_bytes = std::max<int64_t>(S->sp.max_stage_bytes, at); S->sp.readback_bytes += n_read;
    S->sp.t_readback_ms += (t1 - t0) * 1e3; S->sp.t_merge_ms += (bs_now() - t1) * 1e3;
    return SVX_OK;
}

int bamsort_encode(BamSort* S, int64_t first, int64_t nb, int64_t* n_bytes, hipStream_t st) {
    if (!S || !S->finished) return svx_fail(SVX_E_STATE, "svx_bam_sort_encode before svx_bam_sort_finish", __FILE__, __LINE__, hipSuccess);
    if (first < 0 || nb < 1 || first > S->n_blocks - nb) return svx_fail(SVX_E_ARG, "svx_bam_sort_encode: block range outside the file", __FILE__, __LINE__, hipSuccess);
    S->have_piece = false;
    const int64_t total = S->stream_bytes;
    const int64_t lo = std::min<int64_t>(first * BSORT_BLOCK, total), hi = std::min<int64_t>((first + nb) * BSORT_BLOCK, total), pb = hi - lo;
    const long long chunk = std::min<long long>(nb, TGZ_CHUNK);
    const bool spilled = !S->runs.empty();
    int64_t stage_bytes = 0;
    if (spilled && pb > 0) SVXCHK(bs_piece_cuts(S, lo, hi, &stage_bytes, st));          // what the piece needs of every run: known before anything is allocated
    {
        const size_t need = (size_t)pb + (size_t)nb * DEF_SLOT + (size_t)pb + (size_t)nb * 64 + (size_t)chunk * (DEF_BLOCK * 4 + sizeof(DefBlockCodes) + DEF_NHIST * 4) + (size_t)stage_bytes;
        const size_t have = S->piece.cap + S->slots.cap + S->out.cap + S->tok.cap + S->stage.cap;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + need / 8 + (1u << 20) > free_b + have) {
            char msg[240]; snprintf(msg, sizeof msg, "svx_bam_sort_encode: the working buffers of %lld blocks (%zu bytes, %lld of them the staging buffer of the runs' records) do not fit into device memory",
                                    (long long)nb, need, (long long)stage_bytes);
            return svx_fail(SVX_E_CAPACITY, msg, __FILE__, __LINE__, hipSuccess);
        }
    }
    std::vector<TgzBlock> hb((size_t)nb);
    for (int64_t k = 0; k < nb; k++) {
        const int64_t at = std::min<int64_t>((first + k) * BSORT_BLOCK, total);
        hb[(size_t)k] = TgzBlock{(unsigned long long)(at - lo), (uint32_t)std::min<int64_t>(BSORT_BLOCK, total - at), 0u};
    }
    SVXCHK(S->piece.reserve((size_t)pb + 256)); SVXCHK(S->blocks.reserve((size_t)nb * sizeof(TgzBlock)));
    SVXCHK(S->crc.reserve((size_t)nb * 4)); SVXCHK(S->bsize.reserve((size_t)(nb + 1) * 8)); SVXCHK(S->coff.reserve((size_t)(nb + 1) * 8)); SVXCHK(S->kinds.reserve(64));
    SVXCHK(S->tok.reserve((size_t)chunk * DEF_BLOCK * 4)); SVXCHK(S->hist.reserve((size_t)chunk * DEF_NHIST * 4)); SVXCHK(S->nt.reserve((size_t)chunk * 4));
    SVXCHK(S->codes.reserve((size_t)chunk * sizeof(DefBlockCodes))); SVXCHK(S->slots.reserve((size_t)nb * DEF_SLOT));
    {
        HostCopy hc(st);
        SVXCHK(hc.h2d(S->blocks.p, hb.data(), (size_t)nb * sizeof(TgzBlock)));
        if (!S->crc_shift.p) {
            uint32_t m[CRC_POW][32];
            crc_shift_matrices(m);
            SVXCHK(S->crc_shift.reserve(sizeof m));
            SVXCHK(hc.h2d(S->crc_shift.p, m, sizeof m));
        }
        SVXCHK(hc.finish());
    }
    uint8_t* piece = S->piece.as<uint8_t>();
    const TgzBlock* blocks = S->blocks.as<TgzBlock>();
    uint32_t *tok = S->tok.as<uint32_t>(), *hist = S->hist.as<uint32_t>(), *nt = S->nt.as<uint32_t>(), *crc = S->crc.as<uint32_t>();
    int64_t *bsize = S->bsize.as<int64_t>(), *coff = S->coff.as<int64_t>();
    unsigned long long* kinds = S->kinds.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(kinds, 0, 64, st));
    HIPCHK(hipMemsetAsync(bsize + nb, 0, 8, st));
    HIPCHK(hipMemsetAsync(piece + pb, 0, 192, st));
    HIPCHK(hipStreamSynchronize(st));
    if (spilled && pb > 0) SVXCHK(bs_piece_stage(S, stage_bytes, st));                  // the runs' byte ranges read back; the piece's segments point into the staging buffer
    double t[7]; t[0] = bs_now();
    if (pb > 0) {
        const BsSegs G{S->soff.as<int64_t>(), S->saddr.as<uint64_t>(), S->n + 1};
        const long long tiles = (pb + BS_TILE - 1) / BS_TILE;
        k_bs_gather<<<(unsigned)std::min<long long>(tiles, BS_MAX_GRID), BS_T, 0, st>>>(G, lo, pb, piece);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); t[1] = bs_now();
    k_tgz_crc<<<(unsigned)nb, 64, 0, st>>>(piece, blocks, nb, S->crc_shift.as<uint32_t>(), crc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st)); t[2] = bs_now();
    double t_phase[3] = {0, 0, 0};
    for (long long b0 = 0; b0 < nb; b0 += chunk) {
        const unsigned g = (unsigned)std::min<long long>(chunk, nb - b0);
        double u[4]; u[0] = bs_now();
        k_tgz_match<<<g, 64, 0, st>>>(piece, blocks, b0, tok, hist, nt);
        HIPCHK(hipStreamSynchronize(st)); u[1] = bs_now();
        k_tgz_codes<<<g, 64, 0, st>>>(blocks, b0, hist, crc, S->codes.as<DefBlockCodes>(), bsize, kinds);
        HIPCHK(hipStreamSynchronize(st)); u[2] = bs_now();
        k_tgz_bits<<<g, 64, 0, st>>>(piece, blocks, b0, tok, nt, S->codes.as<DefBlockCodes>(), S->slots.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st)); u[3] = bs_now();
        for (int k = 0; k < 3; k++) t_phase[k] += u[k + 1] - u[k];
    }
    t[3] = bs_now();
    SVXCHK((svx_exclusive_scan<int64_t, int64_t>(bsize, coff, nb + 1, st, S->scan_tmp)));
    std::vector<int64_t> h_coff((size_t)nb + 1, 0);
    unsigned long long hk[3] = {0, 0, 0};
    {
        HostCopy hc(st);
        SVXCHK(hc.d2h(h_coff.data(), coff, (size_t)(nb + 1) * 8));
        SVXCHK(hc.d2h(hk, kinds, sizeof hk));
        SVXCHK(hc.finish());
    }
    const int64_t n_out = h_coff[(size_t)nb];
    if (n_out < 28 || n_out > nb * (int64_t)DEF_SLOT) return svx_fail(SVX_E_STATE, "svx_bam_sort_encode: the block sizes are out of range (internal error)", __FILE__, __LINE__, hipSuccess);
    SVXCHK(S->out.reserve((size_t)n_out + 64));
    k_tgz_compact<<<(unsigned)nb, TGZ_CT, 0, st>>>(S->slots.as<uint8_t>(), coff, nb, S->out.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st)); t[4] = bs_now();
    if (first == S->next_block) {
        for (int64_t k = 0; k < nb; k++) S->h_csize[(size_t)(first + k)] = h_coff[(size_t)k + 1] - h_coff[(size_t)k];
        S->next_block = first + nb;
    } else S->broken = true;
    S->piece_bytes = pb; S->out_bytes = n_out; S->have_piece = true;
    if (n_bytes) *n_bytes = n_out;
    svx_bam_sort_stats& X = S->stats;
    X.t_gather_ms += (t[1] - t[0]) * 1e3; X.t_crc_ms += (t[2] - t[1]) * 1e3; X.t_matches_ms += t_phase[0] * 1e3; X.t_codes_ms += t_phase[1] * 1e3; X.t_bits_ms += t_phase[2] * 1e3;
    X.t_compaction_ms += (t[4] - t[3]) * 1e3; X.t_encode_ms += (t[4] - t[0]) * 1e3;
    X.n_pieces++; X.gather_bytes += pb; X.piece_bytes_max = std::max<int64_t>(X.piece_bytes_max, pb);
    X.blocks_stored += (int64_t)hk[DEF_KIND_STORED]; X.blocks_dynamic += (int64_t)hk[DEF_KIND_DYNAMIC]; X.blocks_eof += (int64_t)hk[DEF_KIND_EOF]; X.bytes_out += n_out;
    return SVX_OK;
}

int bamsort_fetch(BamSort* S, uint8_t* compressed_dst, uint8_t* stream_dst, hipStream_t st) {
    if (!S || !S->finished || !S->have_piece) return svx_fail(SVX_E_STATE, "svx_bam_sort_fetch without an encoded piece (svx_bam_sort_encode first)", __FILE__, __LINE__, hipSuccess);
    HostCopy hc(st);
    if (compressed_dst && S->out_bytes) SVXCHK(hc.d2h(compressed_dst, S->out.p, (size_t)S->out_bytes));
    if (stream_dst && S->piece_bytes) SVXCHK(hc.d2h(stream_dst, S->piece.p, (size_t)S->piece_bytes));
    SVXCHK(hc.finish());
    HIPCHK(hipStreamSynchronize(st));
    return SVX_OK;
}

int bamsort_index(BamSort* S, BamIndex* ix, hipStream_t st, int fmt) {
    if (!S || !S->finished || !ix) return svx_fail(SVX_E_STATE, "svx_bam_sort_index before svx_bam_sort_finish", __FILE__, __LINE__, hipSuccess);
    if (S->order == BSORT_QUERYNAME) return svx_fail(SVX_E_STATE, "svx_bam_sort_index: a query-name-sorted file has no index", __FILE__, __LINE__, hipSuccess);
    if (S->broken || S->next_block != S->n_blocks)
        return svx_fail(SVX_E_STATE, "svx_bam_sort_index: the file's blocks have not all been encoded in ascending, gap-free ranges", __FILE__, __LINE__, hipSuccess);
    const double t0 = bs_now();
    const int64_t nb = S->n_blocks;
    std::vector<int64_t> h_coff((size_t)nb + 1, 0);
    for (int64_t b = 0; b < nb; b++) h_coff[(size_t)b + 1] = h_coff[(size_t)b] + S->h_csize[(size_t)b];
    SVXCHK(S->coff_all.reserve((size_t)(nb + 1) * 8));
    SVXCHK(svx_h2d(S->coff_all.p, h_coff.data(), (size_t)(nb + 1) * 8, st));
    SVXCHK(bamindex_take_rows(ix, S->rows, S->perm.as<uint32_t>(), S->soff.as<int64_t>() + 1, S->coff_all.as<int64_t>(), nb, BSORT_BLOCK, st));
    // the data ends where the end-of-file block starts
    SVXCHK(bamindex_finish(ix, S->n_ref, (uint64_t)h_coff[(size_t)nb - 1] << 16, st, fmt));
    S->stats.t_index_ms = (bs_now() - t0) * 1e3;
    return SVX_OK;
}

int bamsort_permutation(BamSort* S, uint32_t* host_perm, hipStream_t st) {
    if (!S || !S->finished) return svx_fail(SVX_E_STATE, "svx_bam_sort_permutation before svx_bam_sort_finish", __FILE__, __LINE__, hipSuccess);
    if (host_perm && S->n > 0) SVXCHK(svx_d2h(host_perm, S->perm.p, (size_t)S->n * 4, st));
    return SVX_OK;
}
void bamsort_spill_stats(const BamSort* S, svx_bam_sort_spill_stats* out) {
    if (S) *out = S->sp; else memset(out, 0, sizeof *out);
}
void bamsort_stats(const BamSort* S, svx_bam_sort_stats* out) {
    if (S) *out = S->stats; else memset(out, 0, sizeof *out);
}
void bamsort_name_stats(const BamSort* S, svx_bam_name_sort_stats* out) {
    if (S) *out = S->ns; else memset(out, 0, sizeof *out);
}
void bamsort_name_spill_stats(const BamSort* S, svx_bam_name_spill_stats* out) {
    if (S) *out = S->nsp; else memset(out, 0, sizeof *out);
}
void bamsort_translate_stats(const BamSort* S, int64_t* n_chunks, int64_t* n_records, int64_t* n_bytes, double* ms) {
    *n_chunks = S ? S->tr_chunks : 0; *n_records = S ? S->tr_records : 0; *n_bytes = S ? S->tr_bytes : 0; *ms = S ? S->tr_ms : 0;
}
