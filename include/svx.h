/*
 * svx.h - C ABI of the MI355X-native COLLECT+CLUSTER path (libsvx.so).
 *
 * The reference (eldariont/svim v2.0.0) has no FFI seam: its hot path is the Python call boundary
 *   analyze_alignment_file_coordsorted / _querysorted   src/svim/SVIM_COLLECT.py:132 / :96
 *   analyze_alignment_indel / analyze_cigar_indel        src/svim/SVIM_intra.py:33 / :8
 *   analyze_read_segments                                src/svim/SVIM_inter.py:24
 *   cluster_sv_signatures -> partition_and_cluster       src/svim/SVIM_CLUSTER.py:7, SVIM_clustering.py:375
 * The entry points below are what a ctypes binding behind those Python functions binds
 * (INTEGRATION.md shows the stub).  Plain pointers and sizes only; every array is Structure-of-Arrays.
 *
 * Conventions
 *   - return value: 0 = ok, negative = SVX_E_* (no exceptions cross the boundary)
 *   - pointers in svx_batch / svx_sig_view / svx_genome may be HOST or DEVICE memory; the `on_device`
 *     member says which (device pointers let a caller keep everything resident in HBM)
 *   - results stay resident in the context (HBM) until fetched with svx_*_fetch into caller-allocated
 *     host arrays sized from svx_*_count
 *   - HOST arrays handed to the library are pageable memory as far as it is concerned: it never registers them with the GPU (no
 *     hipHostRegister, no copy call of the runtime ever sees their address) - every host <-> device copy goes through page-locked
 *     buffers the library owns (csrc/hostcopy.hip).  An input array may be changed or freed as soon as the call returns; an output
 *     array holds its data when the call returns
 *   - the exception a caller can ask for: an input array that lies in memory from svx_host_alloc (page-locked, owned by the library, mapped
 *     until the process ends) is read by the copy engine in place - no bounce pass (what a numpy array costs: one memcpy of its bytes)
 *   - one context per GPU / per process; a context is not re-entrant
 */
#ifndef SVX_H
#define SVX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SVX_OK               0
#define SVX_E_NODEVICE     (-1)   /* no HIP device / extension cannot run: the product path never falls back to CPU */
#define SVX_E_HIP          (-2)   /* a HIP runtime call failed (svx_last_error() has the text) */
#define SVX_E_ARG          (-3)
#define SVX_E_CAPACITY     (-4)   /* an internal fixed-capacity buffer overflowed */
#define SVX_E_STATE        (-5)   /* call order violated (e.g. cluster before collect/set_signatures) */
#define SVX_E_FASTA_SYMBOL (-6)   /* svx_genome_load_fasta: a requested record holds symbols outside "=ACMGRSVTWYHKDBN" (svx_fasta_stats.bad_mask says which) */
#define SVX_E_FASTA_HOST   (-7)   /* svx_genome_load_fasta: a file the device loader leaves to the caller's host parser (svx_fasta_stats.host_reason says why) */
#define SVX_E_ORDER        (-9)   /* svx_text_index: records of a contig not contiguous, or positions decreasing inside one */
#define SVX_E_RANGE        (-10)  /* svx_text_index: a record ends beyond 2^29: outside what a .tbi can hold */
#define SVX_E_IO           (-11)  /* svx_bam_sort_*: a write to or a read from the spill file failed or came back short */
#define SVX_E_NO_DELETION  (-8)   /* svx_combine: insertion-from clusters but no deletion cluster (the reference raises IndexError at src/svim/SVIM_merging.py:20) */

/* signature types, in the order CLUSTER processes them (src/svim/SVIM_CLUSTER.py:19-24) */
enum { SVX_DEL = 0, SVX_INS = 1, SVX_INV = 2, SVX_DUP_TAN = 3, SVX_BND = 4, SVX_DUP_INT = 5, SVX_NTYPES = 6 };
/* sig.src */
enum { SVX_SRC_CIGAR = 0, SVX_SRC_SUPPL = 1 };
/* sig.aux for INV (src/svim/SVIM_inter.py:159-198) */
enum { SVX_LEFT_FWD = 0, SVX_LEFT_REV = 1, SVX_RIGHT_FWD = 2, SVX_RIGHT_REV = 3, SVX_DIR_ALL = 4 };
/* sig.aux for BND: bit0 = direction1 is 'rev', bit1 = direction2 is 'rev'; for DUP_TAN: bit0 = fully_covered */

/* host-set marker in svx_batch.flag: record is to be ignored (query-sorted mode: read without exactly one
 * good primary, src/svim/SVIM_COLLECT.py:108) */
#define SVX_FLAG_SKIP 0x8000u
/* host-set marker: this record's segment rows were rebuilt from its SA tag, so they are void when the
 * record has hard-clipped bases (get_cigar_stats()[0][5] > 0, src/svim/SVIM_COLLECT.py:47) */
#define SVX_FLAG_SA   0x4000u

/* options read on the path (src/svim/SVIM_input_parsing.py:279-371) */
typedef struct svx_params {
    int32_t min_mapq;                      /* 20     */
    int32_t min_sv_size;                   /* 40     */
    int32_t max_sv_size;                   /* 100000 */
    int32_t segment_gap_tolerance;         /* 10     */
    int32_t segment_overlap_tolerance;     /* 5      */
    int32_t all_bnds;                      /* 0      */
    int64_t partition_max_distance;        /* 1000   */
    double  position_distance_normalizer;  /* 900    */
    double  edit_distance_normalizer;      /* 1.0    */
    double  cluster_max_distance;          /* 0.5    */
} svx_params;

/* One batch of BAM records in file order (SoA).  Replaces the per-record pysam accessors used at
 * src/svim/SVIM_COLLECT.py:143-161 and the SA-tag re-materialisation at :44-93 (the host parses the SA
 * string into the segment table; the device derives every coordinate from the packed CIGARs). */
typedef struct svx_batch {
    int32_t on_device;
    int64_t n_rec;
    const uint16_t* flag;        /* [n_rec] SAM FLAG (+ SVX_FLAG_SKIP) */
    const int32_t*  tid;         /* [n_rec] reference_id */
    const int32_t*  pos;         /* [n_rec] 0-based reference_start */
    const uint8_t*  mapq;        /* [n_rec] */
    const int32_t*  lseq;        /* [n_rec] l_qseq of the stored SEQ (0 = none) */
    const int32_t*  read_id;     /* [n_rec] interned query_name */
    const uint32_t* order;       /* [n_rec] emission slot of this record's CIGAR indels */
    const uint32_t* seg_order;   /* [n_rec] emission slot of this read's split-alignment signatures */
    const uint64_t* cigar_off;   /* [n_rec+1] */
    const uint32_t* cigar;       /* BAM packed: len<<4 | op */
    const uint64_t* seq_off;     /* [n_rec+1] byte offsets into seq */
    const uint8_t*  seq;         /* 4-bit packed bases, BAM layout (high nibble first) */
    const uint32_t* seg_off;     /* [n_rec+1] rows of the segment table per record (other alignments of the read) */
    int64_t n_seg;
    const int32_t*  seg_tid;     /* [n_seg] */
    const int32_t*  seg_pos;     /* [n_seg] 0-based */
    const uint8_t*  seg_rev;     /* [n_seg] 1 = reverse strand */
    const uint8_t*  seg_mapq;    /* [n_seg] (SA mapq > 255 already mapped to 0, src/svim/SVIM_COLLECT.py:81-84) */
    const int32_t*  seg_lseq;    /* [n_seg] l_qseq of the segment record (SA rebuild: the primary's) */
    const uint64_t* seg_cigar_off; /* [n_seg+1] */
    const uint32_t* seg_cigar;
    int32_t n_contig;
    const int32_t*  contig_rank; /* [n_contig] rank of each contig NAME in Python str order */
    /* optional sparse SEQ (NULL: every record's whole SEQ sits at seq_off): COLLECT reads a record's bases only for reported insertions,
     * so a reader may keep just those ranges (svx_bam_set_seq_filter).  Record i then owns ranges seq_rng_off[i] .. seq_rng_off[i+1]-1,
     * range r holds bases seq_rng_q0[r] (even) .. +seq_rng_len[r]-1 of the read, packed from byte seq_rng_byte[r] of seq on. */
    const uint32_t* seq_rng_off; /* [n_rec+1] */
    const int32_t*  seq_rng_q0;
    const int32_t*  seq_rng_len;
    const uint64_t* seq_rng_byte;
    int64_t n_seq_rng;
} svx_batch;

/* Signature table (SoA).  Mirrors the fields of the six Signature classes (src/svim/SVSignature.py:3-233). */
typedef struct svx_sig_view {
    int32_t on_device;
    int64_t n;
    uint64_t* key;       /* emission order key: slot<<32 | phase<<30 | ordinal (ascending = reference list order) */
    uint8_t*  type;      /* SVX_DEL .. SVX_DUP_INT */
    uint8_t*  src;       /* SVX_SRC_* */
    uint8_t*  aux;
    int32_t*  contig;    /* contig / contig1 / source contig (tid) */
    int32_t*  start;     /* start / pos1 */
    int32_t*  end;       /* end   / pos1+1 for BND */
    int32_t*  contig2;   /* BND contig2, DUP_INT destination contig, else -1 */
    int32_t*  pos2;      /* BND pos2, DUP_INT pos, DUP_TAN copies, else 0 */
    int32_t*  read_id;
    int64_t*  seq_off;   /* [n+1] INS: offsets into seq; other types have empty ranges */
    uint8_t*  seq;       /* inserted bases, one 4-bit code ("=ACMGRSVTWYHKDBN") per byte */
} svx_sig_view;

/* Reference genome, one 4-bit code per byte, upper-cased (pysam.FastaFile.fetch(...).upper() at
 * src/svim/SVIM_clustering.py:37-43). */
typedef struct svx_genome {
    int32_t on_device;
    int32_t n_contig;
    const int64_t* off;      /* [n_contig+1] */
    const uint8_t* codes;
} svx_genome;

/* Consolidated clusters (src/svim/SVSignature.py:236-311, SVIM_clustering.py:214-303), grouped by type
 * in SVX_* order; unilocal types already sorted by (contig name, (start+end)/2) as at :381. */
typedef struct svx_cluster_view {
    int64_t n;                 /* capacity on input to fetch, count on output */
    int64_t type_count[SVX_NTYPES];
    uint8_t* type;
    int32_t* contig;  int32_t* start;  int32_t* end;      /* unilocal / source */
    int32_t* contig2; int32_t* start2; int32_t* end2;     /* destination (bilocal types) */
    uint8_t* aux;              /* BND: direction bits */
    double*  score;
    double*  std_span;         /* NaN = None */
    double*  std_pos;
    int32_t* size;
    int64_t* member_off;       /* [n+1] */
    int32_t* members;          /* [n_members] indices into the clustered signature table, cluster-major */
    int64_t  n_members;
} svx_cluster_view;

typedef struct svx_ctx svx_ctx;

/* timing / traffic counters of the last collect / cluster call (seconds measured with HIP events on the
 * context's stream) */
typedef struct svx_stats {
    double  t_collect_ms, t_cluster_ms;
    double  t_cigar_scan_ms, t_segments_ms, t_sort_ms, t_partition_ms, t_edit_ms, t_linkage_ms, t_gather_ms;
    int64_t n_rec_used, n_ops, n_seg, n_seg_ops, n_sig, n_bnd_side, n_ins_bases;
    int64_t n_partitions, n_large_partitions, n_pairs, n_edit_pairs, n_edit_cells, n_clusters, n_hap_bytes;
    /* edit-distance work actually executed by the last svx_cluster: 32-bit word-columns (32 DP cells each) the waves issued (lock-step
     * and padding included), the ones the pairs needed, the issued ones of retry rounds (>= 1) and of the band kernels; the band
     * speculation fraction the call's pilot chose */
    int64_t n_edit_wordcols_issued, n_edit_wordcols_useful, n_edit_wordcols_retry, n_edit_wordcols_band;
    double  edit_guess;
} svx_stats;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int  svx_ctx_create(int device_ordinal, svx_ctx** out);     /* SVX_E_NODEVICE when no GPU is present */
void svx_ctx_destroy(svx_ctx* ctx);
const char* svx_last_error(void);
int  svx_version(void);
int  svx_get_stats(svx_ctx* ctx, svx_stats* out);
void* svx_stream(svx_ctx* ctx);                              /* hipStream_t the kernels run on */
int  svx_memcpy_d2h(void* host_dst, const void* device_src, uint64_t bytes);   /* inspection of device-resident results (tests) */
int  svx_memcpy_h2d(void* device_dst, const void* host_src, uint64_t bytes);
void* svx_dev_alloc(uint64_t bytes);                                              /* library-owned device memory (tests, stress tools); NULL on failure */
void svx_dev_free(void* p);
/* page-locked host memory for the caller's batch arrays (svx_batch with on_device = 0): arrays built here are uploaded without the bounce pass.  The reference
   builds its per-read Python objects from pysam (src/svim/SVIM_COLLECT.py:133-167); the batcher that replaces that loop (svim_amd/batch.py) fills these arrays.
   svx_host_free hands the block back to the library (it is reused by a later svx_host_alloc, never unmapped); NULL on failure */
void* svx_host_alloc(uint64_t bytes);
void svx_host_free(void* p);
int  svx_device_synchronize(void);                                               /* SVX_OK iff no kernel / copy of the process has faulted */
/* self-test of the library's own radix sort (64-bit keys + 32-bit values, key bits [begin_bit, end_bit), stable) and exclusive scan on n pseudo-random
   elements, checked on the host against std::stable_sort / a serial sum: 0 = identical (tests) */
int  svx_selftest_prims(svx_ctx* ctx, int64_t n, int32_t begin_bit, int32_t end_bit, uint64_t seed);

/* ---- COLLECT: replaces analyze_alignment_file_* (src/svim/SVIM_COLLECT.py:96-167) -------------- */
int  svx_collect(svx_ctx* ctx, const svx_batch* batch, const svx_params* p);
/* One input file usually arrives as several record batches (svx_bam_read_batch).  With accumulation on (mode 1; it also clears what was
 * accumulated before) every svx_collect APPENDS its two lists to the lists resident in the context, so that svx_collect_count / _fetch and
 * svx_cluster(source 0 / 1) see the whole file - the loop of src/svim/SVIM_COLLECT.py:132-167 over all records - without a table ever
 * leaving HBM.  The emission keys of a batch are shifted by slot_base << 32: pass the number of emission slots of all earlier batches
 * (2 per record is always enough).  mode 0: back to one batch per call; what was accumulated stays resident as "the result of the last
 * COLLECT" (count / fetch / svx_cluster source 0 and 1 keep seeing the whole file). */
int  svx_collect_accumulate(svx_ctx* ctx, int mode);
int  svx_collect_set_slot_base(svx_ctx* ctx, uint64_t slot_base);
int  svx_collect_count(svx_ctx* ctx, int64_t* n_sig, int64_t* n_seq_bytes, int64_t* n_bnd_side);
/* which: 0 = sv_signatures, 1 = translocation_signatures_all_bnds (second list of the reference's tuple) */
int  svx_collect_fetch(svx_ctx* ctx, int which, svx_sig_view* host_out);
/* geometry table of the last svx_collect: five int32 per item {reference length, query_alignment_start, query_alignment_end, infer_read_length (0: None),
 * hard-clipped bases}, the n_rec records first, then the n_seg segment rows.  Filled in for every segment row and for the records whose split-read analysis
 * runs (pass the filters, not supplementary, own segment rows); other entries are undefined.  Inspection hook (tests compare it with the oracle's);
 * NULL array: counts only */
int  svx_collect_geom_fetch(svx_ctx* ctx, int64_t* n_rec, int64_t* n_seg, int32_t* geom /* [5 * (n_rec + n_seg)], host */);

/* ---- the reference genome from a FASTA file, parsed on the device: replaces FastaFile(options.genome) (src/svim/SVIM_clustering.py:377) ----------
 * The bytes of the file (plain text; BGZF, inflated by the device; any other gzip file, inflated by zlib on the host) go into HBM whole, through page-locked
 * staging pieces of SVX_FASTA_PIECE bytes, and kernels working on tiles of SVX_FASTA_TILE bytes find the records, drop headers and line ends, encode the bases
 * and place the requested records in the order of the caller's contig list (csrc/fasta.hip).  A record starts at a '>' in the first column, its name is the
 * first whitespace-separated token behind it (looked for in the SVX_FASTA_NAME_BYTES bytes behind the '>'), the later of two records of one name wins, a contig
 * the file lacks gets length 0.  On SVX_OK the genome is set in the context as after svx_set_genome with host arrays, and off_out holds its offsets.
 * SVX_E_FASTA_SYMBOL: a REQUESTED record holds a byte outside the alphabet.  SVX_E_FASTA_HOST: the loader does not restate what a host parser does with this
 * file - the caller parses it there and calls svx_set_genome.  Either way the genome of the context is what it was before the call.  SVX_E_ARG: no such file. */
#define SVX_FASTA_TILE        4096
#define SVX_FASTA_PIECE       (8 << 20)
#define SVX_FASTA_NAME_BYTES  256
enum { SVX_FASTA_PLAIN = 0, SVX_FASTA_BGZF = 1, SVX_FASTA_GZIP = 2 };
/* svx_fasta_stats.host_reason */
enum { SVX_FASTA_HOST_NONE = 0, SVX_FASTA_HOST_BLANKS = 1 /* space, tab, \v, \f or a '\r' not in front of '\n' on a sequence line */,
       SVX_FASTA_HOST_BUDGET = 2 /* raw bytes + codes beyond a quarter of the free device memory (environment SVX_FASTA_BUDGET_MB: another limit) */,
       SVX_FASTA_HOST_NAMES = 3 /* empty, non-ASCII or over-long record name; one name twice in the contig list; millions of records */,
       SVX_FASTA_HOST_CONTAINER = 4 /* a gzip stream zlib does not take as it is */ };
typedef struct svx_fasta_stats {
    int32_t kind;                /* SVX_FASTA_PLAIN / _BGZF / _GZIP */
    int32_t host_reason;
    int64_t raw_bytes;           /* bytes of text */
    int64_t seq_bytes;           /* bytes of sequence lines that are bases, of every record of the file */
    int64_t dropped_bytes;       /* every other byte: seq_bytes + dropped_bytes == raw_bytes */
    int64_t blank_bytes;
    int64_t bases_kept;          /* == off_out[n_contig] */
    int64_t records_in_file, records_kept;
    int64_t blocks;              /* BGZF blocks */
    double  t_read_stage_s;      /* file -> page-locked staging -> HBM (BGZF: with the device inflate it overlaps; gzip: without the time inside zlib) */
    double  t_inflate_s;         /* BGZF: sum of the inflate kernels' times; gzip: time inside zlib */
    double  t_kernels_s;         /* the passes over the raw bytes, with the header table's trip to the host */
    double  t_total_s;
    uint32_t bad_mask[8];        /* bit b of word b / 32: byte value b, outside the alphabet, seen in a requested record */
} svx_fasta_stats;
int  svx_genome_load_fasta(svx_ctx* ctx, const char* path, int32_t n_contig, const char* names_nul_separated,
                           int64_t* off_out /* [n_contig+1], host */, svx_fasta_stats* stats /* may be NULL */);
/* the genome resident in the context, however it was set (a borrowed device genome included), back on the host; NULL arrays: the counts only */
int  svx_genome_fetch(svx_ctx* ctx, int32_t* n_contig, int64_t* n_codes, int64_t* off /* [n_contig+1] */, uint8_t* codes /* [n_codes] */);
/* host-only pieces of the loader (no GPU needed; tests): the container of a file (raw_bytes: -1 when only inflating tells; n_blocks: BGZF blocks), and the step
 * from the header table to the placement: name_blob holds SVX_FASTA_NAME_BYTES bytes behind each of the n_hdr '>' (at hdr_pos), hdr_rank[n_hdr + 1] the number of
 * bases in front of each header (last entry: all of them); dest[h] = where record h starts in codes, or -1 */
int  svx_fasta_probe(const char* path, int32_t* kind, int64_t* raw_bytes, int64_t* n_blocks);
int  svx_fasta_plan(int64_t n_hdr, const uint8_t* name_blob, const int64_t* hdr_pos, const int64_t* hdr_rank, int64_t raw_bytes, int32_t n_contig,
                    const char* names_nul_separated, int64_t* dest, int64_t* off_out, int64_t* records_kept /* may be NULL */);

/* ---- CLUSTER: replaces cluster_sv_signatures (src/svim/SVIM_CLUSTER.py:7-26) -------------------- */
int  svx_set_genome(svx_ctx* ctx, const svx_genome* g);      /* FastaFile(options.genome), SVIM_clustering.py:377 */
/* source: 0 = signatures resident from the last svx_collect, 1 = its all_bnds side list,
 *         2 = the table passed in `sigs` (host or device memory) */
int  svx_cluster(svx_ctx* ctx, int source, const svx_sig_view* sigs, int32_t n_contig,
                 const int32_t* contig_rank_host, const svx_params* p);
int  svx_cluster_count(svx_ctx* ctx, int64_t* n_clusters, int64_t* n_members);
int  svx_cluster_fetch(svx_ctx* ctx, svx_cluster_view* out);  /* destination arrays: host or device memory */
/* partitions of the last svx_cluster as form_partitions (src/svim/SVIM_clustering.py:17-29) makes them: sorted_index[n_sig] = signature indices in partition
 * order, part_start[n_part + 1] = where each partition begins in it.  Inspection hook (tests compare it with the reference's partitions); NULL arrays: counts only */
int  svx_cluster_partitions_fetch(svx_ctx* c, int64_t* n_sig, int64_t* n_part, uint32_t* sorted_index, int64_t* part_start);

/* multi-GPU, sharded ranks: each rank clusters ONLY the signatures it owns, and the caller deals them out so that every partition of
 * src/svim/SVIM_clustering.py:17-29 is local to one rank.  What still couples the ranks is the random.sample word stream, which a signature type's
 * > 100-member partitions consume in global sorted order without re-seeding (src/svim/SVIM_clustering.py:129-134).  Ranks own consecutive ranges of the
 * partition keys in (contig name, key coordinate) order - coordinate windows whose cuts may lie INSIDE a contig, in a stretch wider than
 * partition_max_distance that no signature touches (svim_amd/multigpu.py: Windows; whole contigs are the special case of cuts at contig starts) - so that
 * order is rank-major: rank r continues each type's stream where the partitions of ranks 0..r-1 stop, those of its own first contig included.
 * svx_cluster finds those positions itself, with ALL-GATHERS ONLY (no rank waits for another rank's sampling): (1) the sizes of everybody's large
 * partitions (4 B each); (2) every rank builds, concurrently, its transfer table "stream position before my partitions -> position after them" for a
 * 6-sigma window around the start it expects from (1) (a few thousand 8 B entries per type), the tables are all-gathered and composed.  Only when a
 * partition beyond 1045 members exists somewhere (random.sample's set method: its consumption depends on the values drawn) or a start leaves its
 * window do the ranks fall back to publishing exact end positions rank after rank (world all-gathers of 128 B).
 * The transport is injected: `fn` must all-gather `bytes` bytes of host memory per rank into `recv` (rank-major, world * bytes) and return 0 - e.g. one
 * torch.distributed.all_gather_into_tensor over RCCL.  Every rank must call svx_cluster once per step (a rank without signatures takes part with an
 * empty table); a rank that fails sends a poison header so that the others fail instead of hanging (svx_cluster_abort_ranks: the same for a failure
 * before the call).  fn == NULL or world <= 1: single rank, every stream starts at 0. */
typedef int (*svx_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes);
int  svx_cluster_set_ranks(svx_ctx* ctx, int rank, int world, svx_allgather_fn fn, void* user);
int  svx_cluster_abort_ranks(svx_ctx* ctx);
/* where each type's stream started / stopped on this rank in the last svx_cluster (32-bit words after seed(1524), SVX_* type order) */
int  svx_cluster_stream_positions(svx_ctx* ctx, int64_t* start /* [SVX_NTYPES] */, int64_t* end /* [SVX_NTYPES] */);

/* ---- COMBINE: replaces combine_clusters (src/svim/SVIM_COMBINE.py:332-478, the --skip_consensus branch) with merge_translocations_at_insertions and
 * flag_cutpaste_candidates (src/svim/SVIM_merging.py:93-159, :12-29) and partition_and_cluster_candidates (src/svim/SVIM_clustering.py:306-372) -----
 * Signature clusters -> SV candidates on the device (csrc/combine.hip).  The cluster and signature tables are only read. */
typedef struct svx_combine_params {
    int64_t trans_sv_max_distance;         /* 500  */
    double  del_ins_dup_max_distance;      /* 1.0  */
    double  position_distance_normalizer;  /* 900  */
    int64_t partition_max_distance;        /* 1000 */
    double  cluster_max_distance;          /* 0.5  */
} svx_combine_params;
/* candidate classes in the order of combine_clusters' return tuple */
enum { SVX_CAND_DEL = 0, SVX_CAND_INV = 1, SVX_CAND_DUP_INT = 2, SVX_CAND_DUP_TAN = 3, SVX_CAND_INS = 4, SVX_CAND_BND = 5, SVX_NCAND = 6 };
/* Candidate table (SoA), grouped by class in SVX_CAND_* order.  DEL / INV / DUP_TAN use the source columns, INS the destination columns (its source contig
 * is -1), DUP_INT and BND both (BND: end = start, end2 = start2).  The constructors' max(0, start) is applied.  aux: BND direction bits as in the cluster
 * table, DUP_INT bit 0 = cutpaste, DUP_TAN bit 0 = fully_covered.  BND: std_span = std_pos1, std_pos = std_pos2.  NaN = None. */
typedef struct svx_candidate_view {
    int64_t n;                 /* count on output */
    int64_t n_members;
    int64_t class_count[SVX_NCAND];
    uint8_t* cls;
    int32_t* contig;  int32_t* start;  int32_t* end;
    int32_t* contig2; int32_t* start2; int32_t* end2;
    uint8_t* aux;
    int32_t* copies;           /* DUP_TAN, else 0 */
    double*  score;
    double*  std_span;
    double*  std_pos;
    int64_t* member_off;       /* [n+1] */
    int32_t* members;          /* [n_members] indices into the clustered signature table */
} svx_candidate_view;
typedef struct svx_combine_stats {
    double  t_combine_ms;      /* HIP events around the whole call on the context's stream (host steps in between included) */
    double  t_cutpaste_ms;     /* the cut&paste kernel alone */
    int64_t n_clusters_in, n_bnd_mirrored, n_merged, n_insertion_from, n_deletions, n_cutpaste_pairs, n_cutpaste;
    int64_t n_remove_1, n_remove_2, n_dup_partitions, n_dup_large_partitions, n_candidates, n_candidate_members;
} svx_combine_stats;
/* source: 0 = the clusters resident from the last svx_cluster (SVX_E_STATE if there are none; the signature table that call clustered must still exist),
 *         2 = the cluster table in `clusters` (grouped by type in SVX_* order, type_count set) plus `sig_aux`, the aux column of the n_sig signatures its
 *             members index - both host or both device memory (on_device).
 * contig_rank_host[n_contig]: rank of each contig NAME in Python str order.  SVX_E_NO_DELETION: see above; stage 2's results stay fetchable. */
int  svx_combine(svx_ctx* ctx, int source, const svx_cluster_view* clusters, const uint8_t* sig_aux, int64_t n_sig, int32_t on_device, int32_t n_contig,
                 const int32_t* contig_rank_host, const svx_combine_params* p);
int  svx_combine_count(svx_ctx* ctx, int64_t* n_candidates, int64_t* n_members);
int  svx_combine_fetch(svx_ctx* ctx, svx_candidate_view* out);   /* destination arrays: host or device memory; NULL arrays are skipped */
/* inspection hook (tests compare with the reference's intermediates): the DUP_INT clusters stage 2 merged from an insertion and two breakend clusters (as
 * cluster rows: cls = SVX_CAND_DUP_INT, source / destination as the cluster has them, no clamp), inserted_regions_to_remove_1 and _2 (indices into the
 * insertion cluster list, ascending) and the flagged interspersed-duplication candidates before the re-clustering.  NULL arrays: counts only. */
int  svx_combine_stages_fetch(svx_ctx* ctx, svx_candidate_view* merged, int64_t* n_remove_1, int32_t* remove_1, int64_t* n_remove_2, int32_t* remove_2,
                              svx_candidate_view* flagged);
int  svx_combine_get_stats(svx_ctx* ctx, svx_combine_stats* out);
/* host-only (no GPU needed; tests): random.seed(1524) followed by random.sample(range(sizes[k]), 100) for k = 0 .. n - 1, as partition_and_cluster_candidates
 * consumes the stream; out[100 * n] */
int  svx_py_sample100(int64_t n, const int64_t* sizes, int32_t* out);
/* host-only (no GPU needed; tests): one window of CLUSTER's consumption table by the host build of csrc/sample_core.hpp.  out[s], s = 0 .. width - 1: the words
 * of stream[0 .. cap) a pool-method random.sample(range(n), 100), 101 <= n <= 1045, consumes from position lo + s; 0xffff for a walk that leaves the stream.
 * method 0: the walk from every start; method 1: the backward sweep in chunks of `chunk` starts, begun `margin` words behind each chunk (0, 0: the kernel's
 * constants), what it leaves open walked - the same table. */
int  svx_sample_used_host(const uint32_t* stream, int64_t cap, int32_t n, int64_t lo, int32_t width, int32_t method, int32_t chunk, int32_t margin,
                          uint16_t* out);

/* ---- VCF text: replaces the body of write_final_vcf (src/svim/SVIM_COMBINE.py:139-184: entries, sorted_nicely :61-68, the svim.<label>.<k> ids) and the nine
 * get_vcf_entry* methods of src/svim/SVCandidate.py (:79, :149, :222, :323, :376, :476, :528, :640, :690) ---------------------------------------------------
 * Candidate table -> the lines of variants.vcf behind the header, byte for byte, in device memory (csrc/vcf.hip).  The header block (SVIM_COMBINE.py:86-137)
 * carries a time stamp and stays with the caller.  The candidate and signature tables are only read. */
enum { SVX_VCF_DEL = 0, SVX_VCF_INV = 1, SVX_VCF_INS = 2, SVX_VCF_DUP_TANDEM = 3, SVX_VCF_DUP_INT = 4, SVX_VCF_BND = 5, SVX_VCF_NLABEL = 6 };   /* ID labels, bits of types_mask */
typedef struct svx_vcf_params {
    uint32_t types_mask;          /* bit per label (options.types, SVIM_COMBINE.py:145-173); a duplication written as an insertion is governed by the INS bit */
    int32_t  sequence_alleles;    /* not options.symbolic_alleles: needs a genome in the context, else SVX_E_STATE */
    int32_t  insertion_sequences; /* ;SEQS=  (novel insertions only) */
    int32_t  read_names;          /* ;READS= */
    int32_t  zmws;                /* ;ZMWS=  */
    int32_t  tandem_duplications_as_insertions;
    int32_t  interspersed_duplications_as_insertions;
} svx_vcf_params;
typedef struct svx_vcf_inputs {   /* everything optional unless a switch needs it; all HOST memory */
    const uint8_t* gt;            /* [n_cand] 0 "./." 1 "0/0" 2 "0/1" 3 "1/1"; NULL: all "./." */
    const int32_t* ref_reads;     /* [n_cand] -1 = None; NULL: all None */
    const int32_t* alt_reads;
    const char*    contig_names_nul_separated;      /* names of the contig ids of the candidate table, each followed by a NUL */
    int32_t        n_contig;
    const int32_t* contig_natural_rank;             /* [n_contig] rank under sorted_nicely's key; EQUAL for names with equal keys ("chr1" / "chr01") */
    const char*    read_names_blob;                 /* read_names: name of read_id r = bytes read_name_off[r] .. read_name_off[r + 1] */
    const int64_t* read_name_off;                   /* [n_reads + 1] */
    int64_t        n_reads;
    const int32_t* zmw_id;        /* [n_reads] zmws: id of "/".join(fields[0:2]) when the name has exactly three '/'-fields, else -1 */
} svx_vcf_inputs;
typedef struct svx_vcf_stats {
    double  t_total_ms;           /* HIP events on the context's stream around the whole call (host steps in between included) */
    double  t_upload_ms;          /* source 2 tables, genotype columns, names */
    double  t_entries_ms;         /* entries, keys, the stable sorts, ids */
    double  t_distinct_ms;        /* distinct reads / ZMWs per candidate */
    double  t_lengths_ms;         /* member piece offsets, line lengths, the two scans and the mailbox read */
    double  t_skeleton_ms;        /* the skeleton kernel alone */
    double  t_payload_ms;         /* the payload kernel alone */
    int64_t n_candidates, n_lines, n_bytes, n_tiles;
    int64_t lines_per_label[SVX_VCF_NLABEL];
    int64_t bytes_ref_forward, bytes_ref_revcomp, bytes_ref_repeat, bytes_seqs, bytes_reads;     /* payload bytes by kind */
} svx_vcf_stats;
/* source: 0 = the candidate table resident from the last svx_combine, which must have taken the resident clusters (its source 0), and the signature table
 *             its members index - SVX_E_STATE if either is gone (no svx_combine yet, a svx_cluster call since);
 *         2 = `cand` (grouped by class in SVX_CAND_* order, class_count set) plus, in `sigs`, the columns of the signatures its members index that the text
 *             needs: n, read_id, and - with insertion_sequences - seq_off and seq.  Host memory.
 * STD_* values must be NaN or below 1e10 in magnitude (they are standard deviations of int32 coordinates): SVX_E_ARG otherwise.  SVX_E_CAPACITY: the text does
 * not fit into device memory (svx_last_error names the byte count).  SVX_E_ARG also for a contig, member or read id outside its table. */
int  svx_vcf(svx_ctx* ctx, int source, const svx_candidate_view* cand, const svx_sig_view* sigs, const svx_vcf_params* p, const svx_vcf_inputs* in);
int  svx_vcf_count(svx_ctx* ctx, int64_t* n_lines, int64_t* n_bytes);
/* bytes [byte_offset, byte_offset + bytes) of the text into host_dst (NULL or bytes 0: none); line_off: [n_lines + 1] offsets of the lines (NULL: not fetched) */
int  svx_vcf_fetch(svx_ctx* ctx, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* line_off);
int  svx_vcf_get_stats(svx_ctx* ctx, svx_vcf_stats* out);
/* host-only (no GPU needed; tests): the text get_std_span() / get_std_pos() put into a line (SVCandidate.py:39-50: "." for None - NaN here - and for 0.0,
 * else str(round(x, 2))), by the integer arithmetic the kernels use.  SVX_E_ARG: |x| >= 1e10 or infinite. */
int  svx_vcf_format_std(double x, char out[32]);

/* ---- repr(float): the bare "{}" the BED and signature-VCF lines print score, std_span and std_pos with --------------------------------------------------------
 * FP64 -> the bytes of CPython's repr(x): the shortest digit string that parses back to x (among the shortest the one closest to x), fixed notation with at
 * least one digit behind the point while the decimal exponent is in [-4, 16), d[.ddd]e+XX / e-XX otherwise; -0.0, inf, -inf, nan.  Integer arithmetic only
 * (csrc/fmt_repr.hpp, one source for host and device); right for every double.  out: NUL-padded to 32 bytes (the longest text has 24).
 * svx_format_repr / _many: host-only (no GPU needed).  _device: the same header compiled for the GPU, one lane per value; host arrays in, host text out. */
int  svx_format_repr(double x, char out[32]);
int  svx_format_repr_many(int64_t n, const double* x, char* out /* [32 * n] */);
int  svx_format_repr_device(svx_ctx* ctx, int64_t n, const double* host_x, char* host_out /* [32 * n] */);

/* ---- BED / signature-VCF text: replaces write_signature_clusters_bed, the body of write_signature_clusters_vcf (src/svim/SVIM_CLUSTER.py:29-106) and
 * write_candidates (src/svim/SVIM_COMBINE.py:18-58) with the get_bed_entry / get_bed_entries / get_vcf_entry methods of the cluster and candidate classes and
 * the five as_string forms of their member signatures (csrc/bed.hip) -------------------------------------------------------------------------------------------
 * One call makes the text of all files of one product in one device buffer, file after file; a file without lines is an empty range. */
enum { SVX_BED_SIGNATURE_BEDS = 0,   /* 7 files: del, ins, inv, dup_tan_source, dup_tan_dest, trans, dup_int (.bed), the reference's order of opening */
       SVX_BED_SIGNATURE_VCF  = 1,   /* 1 file: the lines of signatures/all.vcf behind its header */
       SVX_BED_CANDIDATE_BEDS = 2 }; /* 8 files: candidates_{deletions, inversions, tan_duplications_source, tan_duplications_dest, int_duplications_source,
                                        int_duplications_dest, novel_insertions, breakends}.bed */
#define SVX_BED_MAX_FILES 8
typedef struct svx_bed_inputs {      /* all HOST memory */
    const char*    contig_names_nul_separated;      /* names of the contig ids of the tables, each followed by a NUL */
    int32_t        n_contig;
    const int32_t* contig_str_rank;                 /* [n_contig] rank of each NAME in Python str order: the sort of all.vcf (product 1 only; NULL otherwise) */
    int64_t        debug_short_line;                /* tests: k > 0 counts line k - 1 one byte short, which the skeleton must refuse (SVX_E_STATE); 0 in use */
} svx_bed_inputs;
typedef struct svx_bed_stats {
    double  t_total_ms;           /* HIP events on the context's stream around the whole call (host steps in between included) */
    double  t_upload_ms;          /* source 2 tables, contig names */
    double  t_entries_ms;         /* lines, and for product 1 the keys and the two stable sorts */
    double  t_lengths_ms;         /* member piece lengths and their prefix, line lengths, the two scans and the mailbox read */
    double  t_skeleton_ms;        /* the skeleton kernel alone */
    double  t_payload_ms;         /* the payload kernel alone */
    int64_t n_rows, n_members, n_lines, n_bytes, n_tiles, n_files;
    int64_t bytes_members;        /* payload bytes: the member lists */
    int64_t lines_per_file[SVX_BED_MAX_FILES];
} svx_bed_stats;
/* The read names every member piece ends with: uploaded once per context and kept until replaced or the context dies (name of read_id r = bytes
 * read_name_off[r] .. read_name_off[r + 1] of the blob).  Products 0 and 2 need them (SVX_E_STATE without). */
int  svx_bed_set_read_names(svx_ctx* ctx, const char* read_names_blob, const int64_t* read_name_off /* [n_reads + 1] */, int64_t n_reads);
/* source: 0 = the tables resident in the context: products 0 / 1 the clusters of the last svx_cluster, product 2 the candidates of the last svx_combine (which
 *             must have taken the resident clusters), and the signature table their members index, src column included - SVX_E_STATE if one of them is gone
 *             (no such call yet, a svx_cluster since the svx_combine, a svx_cluster of a host table without src);
 *         2 = `clusters` (products 0 / 1; grouped by type, type_count set) or `cand` (product 2; grouped by class, class_count set) plus, in `sigs`, the columns
 *             of the signatures their members index: n, type, src, aux, contig, start, end, contig2, pos2, read_id.  Host memory.
 * Candidate deviations are printed as svx_vcf prints them (NaN or below 1e10, else SVX_E_ARG), cluster deviations as repr (NaN = None).  SVX_E_ARG also for
 * a contig, member or read id outside its table; SVX_E_CAPACITY: the text does not fit into device memory. */
int  svx_bed(svx_ctx* ctx, int product, int source, const svx_cluster_view* clusters, const svx_candidate_view* cand, const svx_sig_view* sigs,
             const svx_bed_inputs* in);
int  svx_bed_count(svx_ctx* ctx, int32_t* n_files, int64_t* n_lines, int64_t* n_bytes);
/* bytes [byte_offset, byte_offset + bytes) of the text into host_dst (NULL or bytes 0: none); file_off [n_files + 1]: byte offsets of the files; file_line_off
 * [n_files + 1]: first line of every file; line_off [n_lines + 1]: byte offsets of the lines (each NULL: not fetched) */
int  svx_bed_fetch(svx_ctx* ctx, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* file_off, int64_t* file_line_off, int64_t* line_off);
int  svx_bed_get_stats(svx_ctx* ctx, svx_bed_stats* out);

/* ---- BGZF output: a text resident in the context -> a BGZF stream resident in the context (csrc/deflate_core.hpp, csrc/textgz.hip) ---------------------------
 * The reference writes plain text and leaves compression to bgzip; here the text is compressed where it lies and only the stream crosses to the host.
 * Every file of the text becomes BGZF blocks of 65 280 text bytes (the last one shorter) followed by the 28-byte end-of-file block; a file without bytes is that
 * block alone.  Block kinds: dynamic Huffman, or stored where coding would not make the block smaller.  The bytes are a pure function of the text: the host
 * build of the same header (svx_text_gz_host) writes the same stream.
 * source: 0 = the text of the last svx_vcf (one file); 1 = the text of the last svx_bed (its n_files files);
 *         2 = host bytes, uploaded: n_files files, file k = host_text[host_file_off[k] .. host_file_off[k + 1]) (host_file_off[0] = 0).
 * SVX_E_STATE: no such text.  SVX_E_CAPACITY: the working buffers do not fit into device memory.
 * The stream is void after a later svx_vcf (source 0) / svx_bed (source 1): SVX_E_STATE from count and fetch. */
typedef struct svx_text_gz_stats {
    double  t_total_ms;           /* HIP events on the context's stream around the whole call */
    double  t_upload_ms;          /* source 2 text, the block table */
    double  t_crc_ms;             /* CRC32 of every block's text */
    double  t_matches_ms;         /* LZ77 matches and the parse: tokens and histograms */
    double  t_codes_ms;           /* Huffman codes, block headers, sizes */
    double  t_bits_ms;            /* the blocks written into their slots */
    double  t_compaction_ms;      /* scan of the sizes, the dense stream, the block table's way to the host */
    int64_t n_files, n_blocks, blocks_eof, blocks_stored, blocks_dynamic, bytes_in, bytes_out;
} svx_text_gz_stats;
int  svx_text_gz(svx_ctx* ctx, int source, const uint8_t* host_text, const int64_t* host_file_off, int32_t n_files);
int  svx_text_gz_count(svx_ctx* ctx, int32_t* n_files, int64_t* n_blocks /* end-of-file blocks included */, int64_t* n_bytes);
/* bytes [byte_offset, byte_offset + bytes) of the stream into host_dst (NULL or bytes 0: none); file_off [n_files + 1]: offsets of the files in the stream;
 * block_coff [n_blocks + 1]: offsets of the blocks in the stream; block_uoff [n_blocks + 1]: offsets of their text in the text (an end-of-file block holds
 * none) - what a .gzi or tabix index would be built from (each NULL: not fetched) */
int  svx_text_gz_fetch(svx_ctx* ctx, int64_t byte_offset, int64_t bytes, uint8_t* host_dst, int64_t* file_off, int64_t* block_coff, int64_t* block_uoff);
int  svx_text_gz_get_stats(svx_ctx* ctx, svx_text_gz_stats* out);
/* host-only, no GPU: the same encoder built for the host, one file.  SVX_E_CAPACITY: cap is too small (n + 64 * (n / 65280 + 2) always suffices). */
int  svx_text_gz_host(const uint8_t* text, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out);
/* Test infrastructure (as svx_selftest_prims): ONE phase of the encoder over a batch of 1 .. 2048 blocks, one wave per block, by the kernels svx_text_gz launches;
 * the context's stream of the last svx_text_gz is left alone.  All arrays are host memory with one fixed stride per block b:
 *   text[text_off[b] .. + n[b])  the block's text (text_off: n_blocks + 1 entries from 0, the last one the size of `text`; its alignment is that of text_off[b])
 *   tok[b * 65280 ..), nt[b]     the token list (literal byte, or 0x80000000 | (distance - 1) << 9 | (length - 3)) and its length
 *   hist[b * 320 ..)             counts of the 288 literal/length and 32 distance symbols, the end-of-block symbol counted once
 *   codes[b * 692 ..)            the words of DefBlockCodes (csrc/deflate_core.hpp): codes, header items, trailer items, n_pre, n_suf, size, kind; unused words 0
 *   slots[b * 65536 ..)          the block as it is written; the first `size` bytes count
 * phase 0 (match): text, n -> tok, nt, hist.  phase 1 (codes): hist, n, crc -> codes (n 0: the end-of-file block).  phase 2 (bits): text, n, tok, nt, codes -> slots;
 * the codes may be synthetic (any lengths up to 15, any items up to 48 bits) as long as the block fits its slot.  SVX_E_ARG for anything a phase would index
 * out of range with.  svx_text_gz_phase_host: the host build of the same header, no GPU. */
int  svx_text_gz_phase(svx_ctx* ctx, int phase, int64_t n_blocks, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, uint32_t* tok,
                       uint32_t* nt, uint32_t* hist, uint32_t* codes, uint8_t* slots);
int  svx_text_gz_phase_host(int phase, int64_t n_blocks, const uint8_t* text, const int64_t* text_off, const uint32_t* n, const uint32_t* crc, uint32_t* tok, uint32_t* nt,
                            uint32_t* hist, uint32_t* codes, uint8_t* slots);

/* ---- tabix index of the BGZF stream (textindex.hip, textindex_core.hpp; bins and layout: binidx_core.hpp; the definition in words: svim_amd/tabix.py) ----
 * svx_text_index builds, for every file of the last svx_text_gz, the uncompressed bytes of its .tbi from the text AND the block table of that call, both where
 * they lie on the device (SVX_E_STATE without a valid stream; the index is void whenever its stream is).  preset: how a line gives its interval
 * (SVX_INDEX_VCF: POS, len(REF), END=; SVX_INDEX_BED: columns 2 and 3).  stream_base[k]: bytes written in front of file k's stream in its file (a header
 * compressed on the host), NULL = 0.  The call returns SVX_OK even when single files cannot be indexed: file_status says so (SVX_E_ORDER, SVX_E_RANGE) and
 * their bytes are empty.  Chunks are the maximal runs of records of one (contig, bin) in file order; htslib's merging of bins and chunks is not reproduced. */
enum { SVX_INDEX_VCF = 0, SVX_INDEX_BED = 1 };
typedef struct svx_text_index_stats {
    double  t_total_ms, t_lines_ms, t_records_ms, t_contigs_ms, t_chunks_ms, t_linear_ms, t_serialise_ms;
    int64_t n_files, n_files_indexed, n_lines, n_records, n_contigs, n_chunks, n_bins, n_slots, bytes_text, bytes_out;
} svx_text_index_stats;
int  svx_text_index(svx_ctx* ctx, int preset, const int64_t* stream_base);
int  svx_text_index_count(svx_ctx* ctx, int32_t* n_files, int64_t* n_bytes);
int  svx_text_index_fetch(svx_ctx* ctx, uint8_t* host_dst, int64_t* file_off /* [n_files + 1] */, int32_t* file_status /* [n_files] */);
int  svx_text_index_get_stats(svx_ctx* ctx, svx_text_index_stats* out);
/* host-only, no GPU: one file.  block_coff / block_uoff: n_blocks + 1 entries as svx_text_gz_fetch returns them, the last block the end-of-file block.
 * *n_out is the size also when cap is too small (SVX_E_CAPACITY).  SVX_E_ORDER / SVX_E_RANGE: the file has no index. */
int  svx_text_index_host(const uint8_t* text, int64_t n, const int64_t* block_coff, const int64_t* block_uoff, int64_t n_blocks, int preset, int64_t stream_base,
                         uint8_t* out, int64_t cap, int64_t* n_out);
/* The format of an index is an argument: SVX_INDEX_CLASSIC is the five-level .tbi / .bai, which ends at 2^29; SVX_INDEX_CSI is the .csi of the same rows (the
 * definition in words: svim_amd/csi.py): min_shift 14, a depth chosen per file from its largest end (5 .. 9), a loffset per bin in place of the linear index.
 * svx_text_index_fmt(.., SVX_INDEX_CLASSIC) is svx_text_index; with SVX_INDEX_CSI a file's status is 0 or SVX_E_ORDER, never SVX_E_RANGE.  count / fetch /
 * get_stats serve whichever was built last; the fetched bytes are uncompressed (a .csi on disk is BGZF-framed, as a .tbi is).  Any other fmt: SVX_E_ARG. */
enum { SVX_INDEX_CLASSIC = 0, SVX_INDEX_CSI = 1 };
int  svx_text_index_fmt(svx_ctx* ctx, int preset, const int64_t* stream_base, int fmt);
/* host-only: the uncompressed .csi of one file; arguments and results of svx_text_index_host, without SVX_E_RANGE */
int  svx_text_index_csi_host(const uint8_t* text, int64_t n, const int64_t* block_coff, const int64_t* block_uoff, int64_t n_blocks, int preset, int64_t stream_base,
                             uint8_t* out, int64_t cap, int64_t* n_out);

/* ---- GENOTYPE: replaces the per-candidate BAM re-fetch of genotype() (src/svim/SVIM_genotyping.py:34-93) --------
 * by an interval join over the alignment records, resident in HBM.  Records are in file order of a coordinate-sorted BAM
 * (tid, pos non-decreasing); AlignmentFile.fetch(contig, start, stop) of the reference (:48) becomes "records of that contig with
 * pos < stop and end_or_pos1 > start, in order" (htslib's overlap rule; end_or_pos1 = reference_end, or pos + 1 for a record
 * without reference span). */
typedef struct svx_aln_index {
    int64_t n;                      /* records */
    int32_t n_contig;
    int32_t reserved;
    const int64_t* contig_first;    /* [n_contig+1] first record of every contig */
    const int64_t* contig_len;      /* [n_contig]   bam.get_reference_length */
    const int32_t* pos;             /* reference_start */
    const int32_t* end;             /* reference_end (pos when the record has no reference span) */
    const uint16_t* flag;
    const uint8_t*  mapq;
    const int32_t* name_id;         /* query_name interned: records of one read share the id */
} svx_aln_index;
int  svx_set_alignment_index(svx_ctx* ctx, const svx_aln_index* host_index);
/* mode 0 = DEL / INV candidates (locus = source start..end), 1 = INS / DUP_INT (locus = destination start, end == start).
 * member_names: interned read names of the candidate's members, SORTED within every candidate; out_ref_reads[i] =
 * len(reads_supporting_reference) of candidate i (:52-77: first 500 eligible alignments around the locus, distinct names). */
int  svx_genotype(svx_ctx* ctx, int32_t mode, int64_t n_cand, const int32_t* cand_tid, const int32_t* cand_start, const int32_t* cand_end,
                  const int64_t* member_off /* [n_cand+1] */, const int32_t* member_names, int32_t min_mapq, int32_t* out_ref_reads);

/* ---- GENOTYPE from resident tables: the candidate table against an alignment table filled while COLLECT runs ----------------------------------------------
 * svx_collect_keep_alignments(ctx, 1): while it and svx_collect_accumulate are on, every svx_collect appends ALL records of its batch, in file order, to a table
 * resident in the context: tid, pos, end, flag, mapq, read_id.  end = reference_end (pos + the lengths of the M D N = X operations, by a kernel of its own:
 * csrc/alnindex.hip) for records that are placed (tid >= 0), mapped, not secondary and not marked SVX_FLAG_SKIP; every other record is kept with end = pos and
 * its CIGAR is not read (genotype() skips such a record before it counts, src/svim/SVIM_genotyping.py:64-65).  A record marked SVX_FLAG_SKIP is stored with the
 * unmapped bit (4) set.  Nothing is filtered by mapping quality, so a later svx_genotype_resident may ask for any min_mapq.  svx_collect_accumulate(ctx, 1)
 * empties the table as it empties the lists.  Off (the default): svx_collect does what it did, no kernel, no allocation.
 * Records of one read must share their read_id across the batches of the file (the readers of svx_bam_* intern names per handle). */
int  svx_collect_keep_alignments(svx_ctx* ctx, int on);
int  svx_alignments_count(svx_ctx* ctx, int64_t* n);
int  svx_alignments_fetch(svx_ctx* ctx, int32_t* tid, int32_t* pos, int32_t* end, uint16_t* flag, uint8_t* mapq, int32_t* read_id);   /* host, [n]; NULL skipped */
typedef struct svx_alignments_stats {
    double  t_append_ms;       /* HIP events around the appends since the table was emptied (growth copies included), summed */
    double  t_span_ms;         /* the append and long-record kernels alone, summed */
    double  t_finalise_ms;     /* order check + running end maximum of the last finalisation */
    int64_t n_records, n_ops_read, n_long_records;
} svx_alignments_stats;
int  svx_alignments_get_stats(svx_ctx* ctx, svx_alignments_stats* out);
/* Any record order.  svx_collect_keep_alignments_mode(ctx, on, flags) is svx_collect_keep_alignments with a mode for the rows appended from now on
 * (svx_collect_keep_alignments(ctx, on) means flags 0: everything above, every error text and byte as it was).  The flags hold for a whole table: changing
 * them while it holds rows is SVX_E_STATE at the next append.
 *   SVX_ALN_SORT        the rows may arrive in any order.  The finalisation (at the first svx_genotype_resident after an append) checks the order on the
 *                       full key of the coordinate sort (svim_amd/bamsort.py: (uint32(refID), uint32(pos + 1), flag & 16), refID -1 last) and, where a row
 *                       is out of order, sorts the table stably by that key instead of refusing it: ties keep append order, so the table is that of the
 *                       file svx_bam_sort would write.  Rows in order: nothing runs but the check.  Appending after a finalisation and finalising again
 *                       sorts sorted old rows + new rows, which is the stable sort of the whole append order.  At most 2^32 - 1 rows (SVX_E_RANGE); a
 *                       reference id outside [-1, n_contig) or a position below -1 is SVX_E_ARG.
 *   SVX_ALN_FILE_FLAGS  SVX_FLAG_SKIP is the front end's mark, not the record's (query-name mode marks what COLLECT does not analyse, yet genotype() counts
 *                       such records): the row keeps flag & 0x0fff and its end is computed from its CIGAR under the usual rule.  Not for region reads,
 *                       where the mark means "outside the region".
 * svx_alignments_fetch returns the table in its CURRENT order: append order until a finalisation has sorted it, coordinate order afterwards.
 * svx_alignments_permutation: src_row[i] = the append position (0-based, over all appends since the table was emptied) of row i; SVX_E_STATE while the
 * table has not been finalised since its last append.  Without a sort it is the identity. */
enum { SVX_ALN_SORT = 1, SVX_ALN_FILE_FLAGS = 2 };
typedef struct svx_alignments_sort_stats {
    double  t_key_ms, t_sort_ms, t_gather_ms;   /* HIP events of the last finalisation: keys + row numbers, the radix sort, gather + copy back (0 when it did not sort) */
    int64_t n_rows;
    int32_t sorted;                             /* 1: the last finalisation sorted; 0: the rows were in order (or SVX_ALN_SORT was off) */
    int32_t key_bits;                           /* 33 + tid bits: the key bits the sort ran over */
} svx_alignments_sort_stats;
int  svx_collect_keep_alignments_mode(svx_ctx* ctx, int on, uint32_t flags);
int  svx_alignments_permutation(svx_ctx* ctx, uint32_t* src_row /* host, [n] */);
int  svx_alignments_get_sort_stats(svx_ctx* ctx, svx_alignments_sort_stats* out);
typedef struct svx_genotype_params {
    double  minimum_score;          /* 3   : candidates with score < minimum_score are not genotyped (:38-39) */
    int32_t min_mapq;               /* 20  */
    int32_t minimum_depth;          /* 4   */
    double  homozygous_threshold;   /* 0.8 */
    double  heterozygous_threshold; /* 0.2 */
} svx_genotype_params;
typedef struct svx_genotype_stats {
    double  t_total_ms;        /* HIP events on the context's stream around the whole call */
    double  t_tables_ms;       /* source 2 upload + finalisation of the alignment table (order check, contig_first, running end maximum: once per append) */
    double  t_distinct_ms;     /* loci, distinct member reads, compaction */
    double  t_walk_ms;         /* k_genotype */
    double  t_call_ms;
    int64_t n_candidates, n_members, n_alignments;
} svx_genotype_stats;
/* genotype() (src/svim/SVIM_genotyping.py:34-93) for the DEL, INV, INS and DUP_INT rows of a candidate table in one call, against the resident alignment table
 * (SVX_E_STATE when there is none, or when its records are not in coordinate order: "genotyping needs a coordinate-sorted alignment file").
 * source: 0 = the candidate table resident from the last svx_combine, which must have taken the resident clusters, and the signature table its members index;
 *         2 = `cand` (host memory, grouped by class in SVX_CAND_* order, class_count set; the columns cls, contig, start, end, contig2, start2, score,
 *             member_off and members are read) plus sig_read_id[n_sig], the read_id of the signatures its members index.
 * Read identity is the read_id: the ids of the signatures and of the alignment table must come from one interning.  contig_len[n_contig]: reference lengths.
 * Rows of other classes and rows with score < minimum_score get gt 0 ("./."), reads -1 (None) and support fraction NaN (".").  The columns stay resident
 * until the next svx_genotype_resident; a later svx_combine or svx_cluster voids them (SVX_E_STATE from svx_genotype_fetch and from a svx_vcf that asks
 * for them). */
int  svx_genotype_resident(svx_ctx* ctx, int source, const svx_candidate_view* cand, const int32_t* sig_read_id, int64_t n_sig, int32_t n_contig,
                           const int64_t* contig_len, const svx_genotype_params* p);
int  svx_genotype_count(svx_ctx* ctx, int64_t* n_cand);
/* gt: codes of svx_vcf_inputs.gt; ref_reads / alt_reads: -1 = None; support_fraction: NaN = ".".  Host arrays [n_cand]; NULL skipped */
int  svx_genotype_fetch(svx_ctx* ctx, uint8_t* gt, int32_t* ref_reads, int32_t* alt_reads, double* support_fraction);
int  svx_genotype_get_stats(svx_ctx* ctx, svx_genotype_stats* out);
/* on: a svx_vcf with source 0 and no genotype column handed in (gt, ref_reads and alt_reads all NULL) prints the columns svx_genotype_resident (source 0) left
 * for that table, read in place; SVX_E_STATE if there are none for it.  Off (the default): such a call prints "./." as before. */
int  svx_vcf_use_resident_genotypes(svx_ctx* ctx, int on);
/* On: the lines of later svx_vcf calls leave in position order - after the ids are given in the reference's order, one more stable pass sorts the lines by
 * (contig, POS as printed); contigs in natural order, those that share a natural rank by their index.  The same lines with the same ids, every contig
 * contiguous and POS non-decreasing inside it: what tabix asks for.  Off (the default): the reference's order, byte for byte. */
int  svx_vcf_position_order(svx_ctx* ctx, int on);

/* ---- single-function entry points kept importable by the reference's API ------------------------ */
/* analyze_cigar_indel (src/svim/SVIM_intra.py:8-30) on one packed CIGAR; out arrays sized n_ops */
int  svx_cigar_indel(svx_ctx* ctx, const uint32_t* cigar_host, int64_t n_ops, int32_t min_length,
                     int64_t* out_pos_ref, int64_t* out_pos_read, int32_t* out_len, uint8_t* out_is_del,
                     int64_t* out_n);
/* edlib.align(a,b)["editDistance"] (src/svim/SVIM_clustering.py:45) for n pairs of code strings */
int  svx_edit_distance(svx_ctx* ctx, int64_t n_pairs, const uint8_t* codes_host, const int64_t* a_off,
                       const int64_t* b_off /* [n_pairs+1] each, a and b ranges in codes */, int32_t* out_dist);
/* scipy linkage(method='average') + fcluster(criterion='distance') (SVIM_clustering.py:170-171) for a
 * batch of condensed matrices; labels out (1-based) */
int  svx_linkage_fcluster(svx_ctx* ctx, int64_t n_problems, const int32_t* n_host, const int64_t* d_off,
                          const double* d_host, double cutoff, const int64_t* label_off, int32_t* labels_out);

/* test / debug hook: span_position_distance (src/svim/SVIM_clustering.py:47-96) of n_pairs pairs (a[k], b[k]) of a HOST signature table
 * through the device code the clustering itself runs - FP64 operation order and haplotype edit distances included (svx_set_genome
 * first when insertions are among them) */
int  svx_pair_distances(svx_ctx* ctx, const svx_sig_view* host_sigs, int64_t n_pairs, const int64_t* a, const int64_t* b, const svx_params* p,
                        double* out);

/* ---- BGZF inflate on the GPU (first piece of a device-resident BAM front-end) ----------------------
 * Replaces zlib's inflate() as htslib runs it under pysam.AlignmentFile (src/svim/SVIM_COLLECT.py:132-137): every BGZF block is an independent
 * raw DEFLATE stream; one wavefront inflates one block (svim_amd/csrc/inflate_core.hpp, bit-identical to zlib).  The caller packs the payloads
 * (the bytes between the block header and the CRC32/ISIZE trailer) into the pinned staging buffer at 8-byte aligned offsets. */
typedef struct svx_inflater svx_inflater;
int   svx_inflater_create(int device, svx_inflater** out);
void  svx_inflater_destroy(svx_inflater* f);
/* eight slots (0..7; the readers use three with the wave-per-block decoder), each with its own stream, device buffers and pinned staging buffer: while one sub-batch is inflated and copied back, the
 * caller packs the next.  enqueue = H2D + inflate + copy of the inflated range to `out` (host, or device when out_on_device), asynchronous;
 * wait = its completion (error if a block was not a sound DEFLATE stream of ISIZE bytes).  run = enqueue + wait on slot 0. */
void* svx_inflater_staging(svx_inflater* f, int slot, uint64_t bytes);   /* NULL (SVX_E_STATE) while the slot is busy and the buffer would have to grow: wait first */
int   svx_inflater_enqueue(svx_inflater* f, int slot, int64_t n, const uint64_t* in_off, const uint32_t* clen, const uint32_t* isize,
                           const uint64_t* out_at, uint64_t staged_bytes, uint8_t* out, uint64_t out_bytes, int out_on_device);
int   svx_inflater_wait(svx_inflater* f, int slot, float* kernel_ms /* may be NULL */);
int   svx_inflater_run(svx_inflater* f, int64_t n, const uint64_t* in_off, const uint32_t* clen, const uint32_t* isize, const uint64_t* out_at,
                       uint64_t staged_bytes, uint8_t* out, uint64_t out_bytes, int out_on_device, float* kernel_ms /* may be NULL */);

/* ---- native BAM front-end (host side) --------------------------------------------------
 * Replaces pysam.AlignmentFile(bam).fetch(until_eof=True) + the per-record accessors + the SA-tag string handling of
 * src/svim/SVIM_COLLECT.py:8-41,44-85,133 for BAM inputs: multi-threaded BGZF inflate, records decoded straight into
 * a record batch whose host arrays are owned by the handle and stay valid until the next read or close.  mode 0 = coordinate-sorted rules
 * (:132-167), 1 = query-name-sorted rules (:96-129; a read's group is never split across batches). */
typedef struct svx_bam svx_bam;
int  svx_bam_open(const char* path, int n_threads /* 0 = auto */, svx_bam** out);
void svx_bam_close(svx_bam* h);
int  svx_bam_header(svx_bam* h, int32_t* n_ref, const char** names_nul_separated, const int32_t** lengths, const char** sort_order);
int  svx_bam_read_batch(svx_bam* h, int64_t max_records, int mode, int min_mapq, svx_batch* out, int64_t* n_out);
/* The arrays of a batch stay valid until the SECOND next svx_bam_read_batch (two sets alternate): the caller can upload / collect batch i
 * while another thread already reads batch i+1.
 * svx_bam_set_seq_filter(h, min_ins_len > 0): coordinate mode keeps only the SEQ ranges COLLECT can read - insertions of at least
 * min_ins_len bases (pass params.min_sv_size) and the whole SEQ of records with an SA tag - and describes them in svx_batch.seq_rng_*. */
int  svx_bam_set_seq_filter(svx_bam* h, int min_ins_len);
/* back to the first record, keeping buffers, worker threads and the interned read names (a second pass = the steady state of a long file) */
int  svx_bam_rewind(svx_bam* h);
/* contig-sharded ranks: continue at BGZF virtual offset `voff` (the .bai gives the first record of every contig) and report end-of-file at
 * the first record whose reference id exceeds last_tid or that is unplaced (-2: no limit) */
int  svx_bam_seek(svx_bam* h, uint64_t voff, int32_t last_tid);
/* Region reads (coordinate mode only; the definition in words: svim_amd/regions.py, the tests in one place: csrc/region_core.hpp).  Reading continues at
 * virtual offset `voff` (from the .bai / .csi: regions.plan) and reports end-of-file at the first record that is unplaced, lies on a reference behind `tid`,
 * or lies on `tid` with pos >= end.  Records of an earlier reference are not kept and do not stop the read.  What is handed out is ONE contiguous run of the
 * file: from the first kept record to the last record in front of the stop; inside it a record the rule does not keep carries SVX_FLAG_SKIP (COLLECT, the
 * alignment table and the oracle pass over it), and n_out of svx_bam_read_batch counts the run, marked records included.  A region without a kept record
 * hands out nothing.  SVX_REGION_OVERLAP keeps a record whose interval - the index's own: pos .. pos + reference span of the effective CIGAR (CG rule), a
 * record without a span occupies [pos, pos + 1) - overlaps [beg, end): what `samtools view file region` prints.  SVX_REGION_START keeps beg <= pos < end:
 * a record belongs to exactly one of a set of abutting regions.
 * SVX_E_STATE: SAM text, an index build or a sort pass in progress; a svx_bam_read_batch in query-name mode while a region is set.  SVX_E_ARG: end <= beg,
 * beg < 0, a tid outside the header, an unknown rule, an offset beyond the file.  svx_bam_rewind and svx_bam_seek lift the bound; while it is set
 * svx_bam_index_begin and svx_bam_sort_begin answer SVX_E_STATE (their pass runs over the whole file).
 * Device decode: chunks in front of the first kept record are decoded and dropped without being handed out; they are loaded into the slot that was loaded
 * last, so the lifetime of earlier batches is what it is without regions. */
#define SVX_REGION_OVERLAP 0
#define SVX_REGION_START   1
int  svx_bam_seek_region(svx_bam* h, uint64_t voff, int32_t tid, int32_t beg, int32_t end, int rule);
/* since the last svx_bam_seek_region: records examined in front of the stop, records kept, records handed out with SVX_FLAG_SKIP by the rule, bytes of the
 * BGZF blocks loaded (in the file / inflated; a reader that loads ahead counts what it has loaded).  Kept and marked records are those of the run: in a
 * file that is not sorted a record behind the first stop is neither, whatever the rule says of it */
struct svx_bam_region_stats { int64_t n_seen, n_kept, n_marked, bytes_compressed, bytes_inflated; };      /* (a tag, no typedef: the function has the name) */
int  svx_bam_region_stats(svx_bam* h, struct svx_bam_region_stats* out);
/* BGZF inflate shared between the GPU (svx_inflater on `device`; < 0: off) and the host's cores: of every chunk of blocks the GPU takes sub-batches
 * from the front while the worker threads take blocks from the back - whoever is faster inflates more.  stats: blocks inflated by either so far. */
int  svx_bam_set_gpu_inflate(svx_bam* h, int device);
int  svx_bam_gpu_inflate_stats(svx_bam* h, int64_t* gpu_blocks, int64_t* cpu_blocks, double* gpu_kernel_ms);
int  svx_bam_read_names(svx_bam* h, int64_t* n_names, const char** nul_separated, int64_t* blob_len);
/* Device-resident front-end (either sort order): the compressed file slice is the only thing that crosses PCIe.  Every chunk of BGZF blocks (8 GB of inflated
 * data) is inflated by the GPU into HBM (one wavefront per block), the record boundaries are found there (BGZF blocks are the restart points of the
 * block_size chain: a speculative record start per block, verified by linking the chains), and fixed fields, CIGAR (CG tag included), the SA tag -> segment
 * table and the read names (interned by 2 x 64-bit hashes) are decoded by kernels.  svx_bam_read_batch then returns an svx_batch whose pointers are DEVICE
 * memory (on_device = 1; seq points into the inflated stream - no bases are copied).  Lifetime: the arrays that are views of the chunk (tid, pos, mapq, lseq,
 * read_id, cigar_off, cigar, seq_off, seq and - mode 0 - flag and the seg_* table) stay valid until the THIRD next chunk is loaded; the arrays made per batch
 * (order, seg_order and - mode 1, query-name order - flag and the seg_* table built from the read's supplementary records) alternate between two sets per chunk
 * and stay valid until the SECOND next svx_bam_read_batch, like the batches of the host reader.  Every
 * inflated block is checked against the CRC32 of its BGZF trailer on the device (as htslib's bgzf_read_block does; environment SVX_BAM_VERIFY_CRC=0: off);
 * a damaged block fails the svx_bam_read_batch that would have handed out its records.  device < 0: back to the host reader. */
int  svx_bam_set_device_decode(svx_bam* h, int device);

/* ---- BAM index from the device reader's record stream (bamindex.hip, bamindex_core.hpp; bins and layout: binidx_core.hpp; the definition in words: svim_amd/bai.py) ----
 * svx_bam_index_begin switches indexing on for the pass that follows: device decode must be on and the handle at its first record (after open,
 * svx_bam_set_device_decode or svx_bam_rewind, before any read), else SVX_E_STATE.  While it is on, every chunk the reader loads appends one row
 * (tid, pos, end, flag, vbeg) per record it discovers to a table resident on the device - before any filter, whatever max_records, min_mapq and mode the
 * reads use - and svx_bam_seek / svx_bam_rewind return SVX_E_STATE.  svx_bam_index_finish, once svx_bam_read_batch has returned 0 records at the end of the
 * file (SVX_E_STATE before), builds the bytes of the .bai from the table: order and range checks, references by bisection, bins, chunk heads, a stable sort by
 * (tid, bin), the linear index, serialisation.  SVX_E_ORDER: the file is not in coordinate order; SVX_E_RANGE: a record ends beyond 2^29 (what a .bai can
 * hold).  Either way, and after success, indexing is off again, the table is dropped and the handle reads on as before (rewind for another pass).
 * svx_bam_index_abort gives a pass up at any point (an interrupted run, a read that failed): indexing off, the table dropped, the handle where it was, so
 * that svx_bam_rewind and svx_bam_seek work again; SVX_E_STATE when no index is being built.  count and
 * fetch give the bytes of the last successful finish (SVX_E_STATE when there are none).  Chunks are the maximal runs of records of one (tid, bin) in file
 * order; htslib's merging of bins and chunks is not reproduced.  With indexing never begun the reader does what it did before these functions existed. */
typedef struct svx_bam_index_stats {
    double  t_total_ms, t_append_ms /* the span and virtual-offset kernels, over all chunks */, t_check_ms /* the phases of finish: host clock, the stream drained at each boundary */, t_chunks_ms, t_sort_ms, t_linear_ms, t_serialise_ms;
    int64_t n_rows, n_placed, n_refs, n_refs_with_rows, n_chunks, n_bins, n_slots, n_long_cigars, bytes_out;
} svx_bam_index_stats;
int  svx_bam_index_begin(svx_bam* h);
int  svx_bam_index_finish(svx_bam* h);
int  svx_bam_index_abort(svx_bam* h);
int  svx_bam_index_count(svx_bam* h, int64_t* n_bytes);
int  svx_bam_index_fetch(svx_bam* h, uint8_t* host_dst);
int  svx_bam_index_get_stats(svx_bam* h, svx_bam_index_stats* out);
/* host-only, no GPU: the .bai of a row table (n_rows rows in file order; v_end: the virtual offset where the file's data ends).  *n_out is the size also when
 * cap is too small (SVX_E_CAPACITY).  SVX_E_ORDER / SVX_E_RANGE: the file has no index; SVX_E_ARG: a tid beyond n_ref. */
int  svx_bam_index_host(int32_t n_ref, int64_t n_rows, const int32_t* tid, const int32_t* pos, const int64_t* end, const uint16_t* flag, const uint64_t* vbeg,
                        uint64_t v_end, uint8_t* out, int64_t cap, int64_t* n_out);
/* The same index in the format asked for (SVX_INDEX_CLASSIC / SVX_INDEX_CSI, above; any other: SVX_E_ARG, the pass stays on): svx_bam_index_finish(h) is
 * svx_bam_index_finish_fmt(h, SVX_INDEX_CLASSIC) and svx_bam_sort_index(h) is svx_bam_sort_index_fmt(h, SVX_INDEX_CLASSIC).  A .csi has no SVX_E_RANGE: a BAM
 * coordinate never needs more than depth 7.  count / fetch serve whichever was built last; the bytes of a .csi are uncompressed (the file on disk is these
 * bytes BGZF-framed). */
int  svx_bam_index_finish_fmt(svx_bam* h, int fmt);
int  svx_bam_sort_index_fmt(svx_bam* h, int fmt);
/* host-only: the uncompressed .csi of a row table; arguments and results of svx_bam_index_host, without SVX_E_RANGE */
int  svx_bam_index_csi_host(int32_t n_ref, int64_t n_rows, const int32_t* tid, const int32_t* pos, const int64_t* end, const uint16_t* flag, const uint64_t* vbeg,
                            uint64_t v_end, uint8_t* out, int64_t cap, int64_t* n_out);

/* ---- coordinate sort of the file the device reader is reading (bamsort.hip, bamsort_core.hpp; the definition in words: svim_amd/bamsort.py) ----
 * The sorted file: the header with SO:coordinate, every record verbatim in the order of (uint32(refID), uint32(pos + 1), flag & 16), equal keys in file order,
 * cut into BGZF blocks of exactly 65 280 stream bytes plus the end-of-file block, compressed by the encoder of svx_text_gz.
 * svx_bam_sort_begin switches sorting on for the pass that follows: device decode must be on, the handle at its first record and no index pass on, else
 * SVX_E_STATE (svx_bam_index_begin during a sort pass is SVX_E_STATE as well).  While it is on, every chunk the reader loads leaves its records' bytes in an
 * arena on the device (a slab per chunk, never moved) and one row per record - before any filter, whatever max_records, min_mapq and mode the reads use - and
 * svx_bam_seek / svx_bam_rewind return SVX_E_STATE.  max_bytes: the most the arena may hold (0: whatever the device has free); the svx_bam_read_batch whose
 * chunk would pass it returns SVX_E_CAPACITY, the sort is dropped and the handle is usable again after svx_bam_rewind.
 * svx_bam_sort_finish, once svx_bam_read_batch has returned 0 records at the end of the file (SVX_E_STATE before): a stable radix sort of the keys, the offsets
 * of the records in the output stream.  SVX_E_ARG: a record with refID < -1 or >= n_ref or block_size < 32; SVX_E_RANGE: pos < -1; SVX_E_CAPACITY: more than
 * 2^32 - 1 records; the sort is dropped then.  The reading pass is over after finish: svx_bam_rewind and svx_bam_seek work again, the sorted records stay.
 * svx_bam_sort_count: records, bytes of the output stream, BGZF blocks (the end-of-file block included).
 * svx_bam_sort_encode(first_block, n_blocks): stream bytes [first_block * 65280, ..) gathered into a piece buffer and encoded; *n_bytes = the compressed size.
 * svx_bam_sort_fetch: the compressed bytes of the last encode, and its uncompressed bytes when stream_dst is not NULL.  Resident are the arena, about 46
 * bytes per record and one piece; the file is never held twice.
 * svx_bam_sort_index: the .bai of the sorted file from the sorted rows and the block sizes, read through svx_bam_index_count / svx_bam_index_fetch.
 * SVX_E_STATE unless every block has been encoded in ascending, gap-free ranges since finish; SVX_E_RANGE: a record ends beyond 2^29.
 * svx_bam_sort_permutation: perm[i] = the file index of the i-th record of the sorted order (n_records entries).
 * svx_bam_sort_abort at any point: sorting off, everything dropped; SVX_E_STATE when no sort is on or finished.
 * With sorting never begun the reader does what it did before these functions existed.
 * Files whose records do not fit into device memory: svx_bam_sort_begin_spill(max_bytes, spill_dir) has the preconditions of svx_bam_sort_begin; spill_dir
 * must be a directory the process can write to (SVX_E_ARG otherwise).  The chunk that would take the arena past the limit (max_bytes, or with 0 what the device
 * has free) no longer fails the read: it CLOSES A RUN - the run's records are sorted, laid out in that order and appended to one spill file in spill_dir, the
 * slabs are freed - and starts the next run.  Only a chunk whose own bytes pass max_bytes is SVX_E_CAPACITY.  The spill file is unlinked as soon as it is
 * open (a killed process leaves nothing behind), holds raw stream bytes, and is closed by abort, by closing the handle and by every failure.  Resident for the
 * whole file stay about 60 bytes per record: key, length, file index and offset of every record in run order, the index rows, and after finish the
 * permutation and the segment table.  If no run was closed when the file ends, finish is the in-memory finish: no file is made.  Otherwise the last run is
 * spilled too, one stable radix sort over the run-sorted keys (payload: the place in the concatenation of the runs) gives the order - equal keys tie by run,
 * then by place in the run, which is file order: the permutation of the in-memory sort - and svx_bam_sort_encode reads, for every piece, one contiguous byte
 * range per run back from the file into a staging buffer (SVX_E_CAPACITY with the size in svx_last_error if it does not fit) before the same gather and
 * encoder.  count, fetch, index and permutation mean what they mean above; the bytes are the same.  SVX_E_IO: a write or read of the spill file failed or was
 * short; the sort is dropped and the handle is usable after svx_bam_rewind.  svx_bam_sort_stats.arena_bytes counts the records' bytes wherever they lie.
 * svx_bam_sort_get_spill_stats: valid after any finish, spilled or not (n_runs 0 without records, 1 when nothing was spilled); n_runs, spilled_bytes,
 * max_chunk_bytes and max_run_bytes are kept up to date during the pass. */
typedef struct svx_bam_sort_spill_stats {
    int64_t n_runs, spilled_bytes /* written to the spill file */, max_chunk_bytes /* the largest slab */, max_run_bytes, max_stage_bytes /* the largest staging buffer of an encode, pads included */,
            readback_bytes /* read from the spill file, over all pieces */;
    double  t_spill_ms /* closing runs: sort, layout, gather, copy out, pwrite */, t_readback_ms /* pread and copy in, over all pieces */,
            t_merge_ms /* the sort over the runs, its layout, and the cuts and addresses of every piece */;
} svx_bam_sort_spill_stats;
typedef struct svx_bam_sort_stats {
    double  t_append_ms /* slab copies and row kernels, over all chunks */, t_finish_ms, t_sort_ms, t_layout_ms,
            t_encode_ms /* over all pieces: host clock, the stream drained at each phase */, t_gather_ms, t_crc_ms, t_matches_ms, t_codes_ms, t_bits_ms, t_compaction_ms, t_index_ms;
    int64_t n_records, n_slabs, arena_bytes, stream_bytes, n_blocks, key_bits, n_pieces, gather_bytes, piece_bytes_max, blocks_stored, blocks_dynamic, blocks_eof, bytes_out;
} svx_bam_sort_stats;
int  svx_bam_sort_begin(svx_bam* h, int64_t max_bytes);
int  svx_bam_sort_begin_spill(svx_bam* h, int64_t max_bytes, const char* spill_dir);
int  svx_bam_sort_finish(svx_bam* h);
int  svx_bam_sort_abort(svx_bam* h);
int  svx_bam_sort_count(svx_bam* h, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks);
int  svx_bam_sort_encode(svx_bam* h, int64_t first_block, int64_t n_blocks, int64_t* n_bytes);
int  svx_bam_sort_fetch(svx_bam* h, uint8_t* compressed_dst, uint8_t* stream_dst_or_null);
int  svx_bam_sort_index(svx_bam* h);
int  svx_bam_sort_permutation(svx_bam* h, uint32_t* perm);
int  svx_bam_sort_get_stats(svx_bam* h, svx_bam_sort_stats* out);
int  svx_bam_sort_get_spill_stats(svx_bam* h, svx_bam_sort_spill_stats* out);
/* host-only, no GPU: records in file order (n_bytes of block_size + body each) -> the sorted record stream (out: n_bytes, may be NULL) and the permutation
 * (perm: perm_cap entries, may be NULL; n_bytes / 36 + 1 always suffice).  *n_records is set also when perm_cap is too small (SVX_E_CAPACITY).
 * SVX_E_ARG / SVX_E_RANGE: what the definition refuses (a stream that ends inside a record is SVX_E_ARG). */
int  svx_bam_sort_host(const uint8_t* records, int64_t n_bytes, int32_t n_ref, uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records);
/* host-only, no GPU: the spilled sort by the rules the kernels use (bamsort_core.hpp: bsort_piece_cut).  run_ends[n_runs]: the number of records in front of
 * the end of every run, in file order, non-decreasing (an empty run is allowed), the last one the number of records (SVX_E_ARG otherwise; n_runs 0 only for a
 * stream without records).  Every run is sorted stably and written in that order to a "run file"; one stable sort over the run-sorted keys gives the order;
 * the sorted record stream is then written in pieces of piece_blocks * 65280 bytes, every piece from one contiguous byte range per run read back from the run
 * file.  out, perm, perm_cap, *n_records and the refusals: as svx_bam_sort_host, and the same bytes and permutation.  The run file is memory of the call unless
 * write_fn / read_fn are given (both or neither): they move n_bytes at `offset` of the caller's file and return the bytes moved; fewer than asked is SVX_E_IO. */
typedef int64_t (*svx_spill_write_fn)(void* user, int64_t offset, const uint8_t* src, int64_t n_bytes);
typedef int64_t (*svx_spill_read_fn)(void* user, int64_t offset, uint8_t* dst, int64_t n_bytes);
int  svx_bam_sort_spill_host(const uint8_t* records, int64_t n_bytes, int32_t n_ref, const int64_t* run_ends, int64_t n_runs, int64_t piece_blocks, uint8_t* out,
                             uint32_t* perm, int64_t perm_cap, int64_t* n_records, svx_spill_write_fn write_fn, svx_spill_read_fn read_fn, void* user);
/* host-only: the header of the sorted file from a file's header (magic .. reference dictionary).  *n_out is the size also when cap is too small (SVX_E_CAPACITY) */
int  svx_bam_sort_header_host(const uint8_t* header, int64_t n_bytes, uint8_t* out, int64_t cap, int64_t* n_out);

/* ---- query-name order for the sort above: `samtools sort -N` (bamsort.hip: the k_ns_* kernels; the definition in words: svim_amd/bamsort.py) ----
 * The order: records compare by (name, name_rank).  The name is the l_read_name bytes at body offset 32 cut at their first NUL (the whole field when it holds
 * none); names compare as unsigned bytes, a proper prefix first.  name_rank = ((flag >> 6) & 3) << 2 | ((flag >> 11) & 1) << 1 | ((flag >> 8) & 1): READ1 /
 * READ2 first, then primary < secondary < supplementary.  Equal keys keep file order.  The header gets SO:queryname and SS:queryname:lexicographical behind it
 * (GO: and every other SS: field go).  This is the input of the query-name front end (svx_bam_read_batch mode 1): the records of a read lie next to each other.
 * svx_bam_sort_begin_order(h, max_bytes, order): svx_bam_sort_begin is this call with SVX_SORT_COORDINATE; any other order than the two: SVX_E_ARG.  The pass,
 * finish, count, encode, fetch, permutation, get_stats and abort are those above.  svx_bam_sort_finish refuses, besides what it refuses above, a record with
 * l_read_name = 0 or 32 + l_read_name > block_size (SVX_E_ARG, which goes before SVX_E_RANGE).  The permutation comes from one stable 4-bit radix pass by
 * name_rank and then most-significant-first rounds of 4 name bytes over the rows whose order is still open, at most 64 of them; a round costs the host one
 * 8-byte read-back.  A query-name-sorted file has no index: svx_bam_sort_index and svx_bam_sort_index_fmt answer SVX_E_STATE after such a sort.
 * Not built, and refused: a spilled query-name sort of the READER (svx_bam_sort_begin_spill is coordinate order; a query-name sort that passes max_bytes ends
 * with SVX_E_CAPACITY as an in-memory coordinate sort does; a merge session over the one file with a spill directory, svx_bam_merge_open_order below, is that
 * sort), samtools' natural order (-n).
 * svx_bam_sort_get_name_stats: valid after the finish of a query-name sort (zeros otherwise): rounds run, rows that took part in round r (active_rows[r],
 * r < 64), their sum and maximum, and the host-clock times of the phases of finish with the stream drained at each edge. */
#define SVX_SORT_COORDINATE 0
#define SVX_SORT_QUERYNAME  1
typedef struct svx_bam_name_sort_stats {
    double  t_names_ms /* name extents, ranks and checks */, t_rank_ms /* the radix pass by name_rank */, t_rounds_ms, t_layout_ms;
    int64_t n_records, word_bytes /* 4 */, rounds, active_total, active_max, active_rows[64];
} svx_bam_name_sort_stats;
int  svx_bam_sort_begin_order(svx_bam* h, int64_t max_bytes, int order);
int  svx_bam_sort_get_name_stats(svx_bam* h, svx_bam_name_sort_stats* out);
/* host-only, no GPU: svx_bam_sort_host and svx_bam_sort_header_host in the order asked for (they are these calls with SVX_SORT_COORDINATE); any other order
 * than the two: SVX_E_ARG.  Query-name order adds the two refusals above to those of svx_bam_sort_host. */
int  svx_bam_sort_host_order(const uint8_t* records, int64_t n_bytes, int32_t n_ref, int order, uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records);
int  svx_bam_sort_header_host_order(const uint8_t* header, int64_t n_bytes, int order, uint8_t* out, int64_t cap, int64_t* n_out);

/* ---- several files merged into one sorted file: the definition's host build (the definition in words: svim_amd/bammerge.py) ----
 * The merged dictionary is the first file's references, then file by file the names not yet present; tid_map[f][i] is the merged id of file f's reference i.
 * A record of a file whose map is the identity is copied verbatim; any other record gets refID and next_refID replaced by their mapped values (-1 stays -1),
 * and there a next_refID outside [-1, n_ref of that file) is SVX_E_ARG, as a refID outside it always is.  The order is that of svx_bam_sort_host over the
 * translated records, stable over the record numbers of the concatenation of the files.  The device build is the session below. */
/* host-only: the merged header (magic .. merged reference dictionary) of k headers, in the order given, by the rule of svim_amd/bammerge.py.  tid_maps_out (may
 * be NULL): the maps back to back, the sum of the files' n_ref entries.  *n_out is the size also when cap is too small (SVX_E_CAPACITY).  SVX_E_ARG: a header
 * that cannot be walked, a name twice in one dictionary, one name with two lengths, two @RG lines with one ID and different bytes. */
int  svx_bam_merge_header_host(const uint8_t* const* headers, const int64_t* sizes, int64_t k, uint8_t* out, int64_t cap, int64_t* n_out, int32_t* tid_maps_out);
/* host-only: the merged record stream of k record streams (file order; n_ref[f] references each, tid_maps: the maps back to back) and the permutation over the
 * record numbers of their concatenation.  out (may be NULL) takes the sum of the sizes; perm, perm_cap, *n_records and the refusals as svx_bam_sort_host, and
 * SVX_E_ARG for a mate id outside a translated file's dictionary or a map entry outside [0, n_ref_merged). */
int  svx_bam_merge_host(const uint8_t* const* streams, const int64_t* sizes, const int32_t* n_ref, int64_t k, int32_t n_ref_merged, const int32_t* tid_maps, uint8_t* out,
                        uint32_t* perm, int64_t perm_cap, int64_t* n_records);
/* host-only: the two calls above in the order asked for (they are these with SVX_SORT_COORDINATE; any other order than the two: SVX_E_ARG).  In
 * SVX_SORT_QUERYNAME rule 1 of the header takes the first line of the first file's header as svx_bam_sort_header_host_order rewrites it (one file: that whole
 * header), the records are translated exactly as above and compare by (name, name_rank), stable over the record numbers of the concatenation, and the two name
 * refusals of svx_bam_sort_host_order hold per file (SVX_E_ARG in any file before SVX_E_RANGE in any file). */
int  svx_bam_merge_header_host_order(const uint8_t* const* headers, const int64_t* sizes, int64_t k, int order, uint8_t* out, int64_t cap, int64_t* n_out, int32_t* tid_maps_out);
int  svx_bam_merge_host_order(const uint8_t* const* streams, const int64_t* sizes, const int32_t* n_ref, int64_t k, int32_t n_ref_merged, const int32_t* tid_maps, int order,
                              uint8_t* out, uint32_t* perm, int64_t perm_cap, int64_t* n_records);
/* host-only, for tests: one name (1..255 bytes, no NUL) packed at word word_off of a name table of tab_words 32-bit words (bamsort_core.hpp: bsort_name_tab_*)
 * -> how many of the rounds 0..63 read another word from the table than from the name itself, plus the words written outside the name's own (0: none);
 * SVX_E_ARG for a name that does not fit. */
int  svx_bam_name_tab_check_host(const uint8_t* name, int32_t name_len, int64_t word_off, int64_t tab_words);
/* ---- the merge on the device: a session that readers only feed (bammerge.hip, bamsort.hip: k_bs_translate) ----
 * A session is an object of its own.  It owns its sort, its HIP stream and its output index; a reader never owns any of it, and a reader's own sort
 * (svx_bam_sort_*) and index are not touched by a merge.
 * svx_bam_merge_open: readers are k >= 1 open handles (BAM, or SAM text) in file order.  They are used ONLY inside this call, to read their headers and
 * dictionaries: the session keeps no pointer to any of them, and they may be closed as soon as it returns.  The merged header and the id maps are those of
 * svx_bam_merge_header_host, and its refusals (one name with two lengths, a name twice in one file, @RG lines that clash) leave here with SVX_E_ARG before
 * any device work.  max_bytes and spill_dir (may be NULL) mean what they mean to svx_bam_sort_begin and svx_bam_sort_begin_spill, over all files together.
 * svx_bam_merge_add, k times, file i as the i-th call: h must satisfy the preconditions of svx_bam_sort_begin (device decode on, at its first record, no
 * index pass, no sort pass, no region read and no contig limit of svx_bam_seek: SVX_E_STATE), decode on the session's device, and have the dictionary file i had at open (SVX_E_ARG).  The call
 * drives the whole pass itself: it reads the file to its end, discards the batches, waits until the reader's loader is idle and only then returns; the appends
 * run in the reader's loader thread but on the session's stream, so that no command on a reader's stream ever touches the session's memory.  A reader
 * is attached for the length of this one call; afterwards it stands at the end of its file, rewinds, sorts on its own or is closed exactly as before.
 * A file whose map is the identity is copied verbatim (a refID beyond its OWN dictionary is still refused); any other file's records get refID and
 * next_refID translated in the session's copy.  SVX_E_CAPACITY / SVX_E_IO from the arena or the spill file, and any failed read: the session's sort is
 * dropped and the session is broken - every later call but close is SVX_E_STATE - while the reader is usable after svx_bam_rewind.
 * svx_bam_merge_finish after k adds (SVX_E_STATE before): the sort and the layout under the merged header; SVX_E_ARG / SVX_E_RANGE as svx_bam_sort_finish,
 * and SVX_E_ARG for a next_refID outside the dictionary of a translated file.  count, encode, fetch, permutation, get_stats and get_spill_stats mean what
 * they mean for svx_bam_sort_*; record numbers are places in the concatenation of the files.  svx_bam_merge_index_fmt builds the merged file's .bai or .csi
 * into the session's own index, read by svx_bam_merge_index_count / svx_bam_merge_index_fetch.  svx_bam_merge_close at any point frees what the session
 * owns and nothing else. */
typedef struct svx_bam_merge svx_bam_merge;
typedef struct svx_bam_merge_stats {
    int64_t n_files, n_added, n_ref_merged, header_bytes, n_translated_files /* of those added */, n_translated_chunks, n_translated_records,
            translate_bytes /* read and written by k_bs_translate */;
    double  t_open_ms, t_add_ms /* the reading passes, over all files */, t_translate_ms /* k_bs_translate between events on the session's stream */;
} svx_bam_merge_stats;
int  svx_bam_merge_open(svx_bam* const* readers, int64_t k, int device, int64_t max_bytes, const char* spill_dir_or_null, svx_bam_merge** out);
int  svx_bam_merge_add(svx_bam_merge* m, svx_bam* h);
int  svx_bam_merge_finish(svx_bam_merge* m);
int  svx_bam_merge_count(svx_bam_merge* m, int64_t* n_records, int64_t* stream_bytes, int64_t* n_blocks);
int  svx_bam_merge_encode(svx_bam_merge* m, int64_t first_block, int64_t n_blocks, int64_t* n_bytes);
int  svx_bam_merge_fetch(svx_bam_merge* m, uint8_t* compressed_dst, uint8_t* stream_dst_or_null);
int  svx_bam_merge_index_fmt(svx_bam_merge* m, int fmt);
int  svx_bam_merge_index_count(svx_bam_merge* m, int64_t* n_bytes);
int  svx_bam_merge_index_fetch(svx_bam_merge* m, uint8_t* host_dst);
int  svx_bam_merge_permutation(svx_bam_merge* m, uint32_t* perm);
int  svx_bam_merge_get_stats(svx_bam_merge* m, svx_bam_sort_stats* out);
int  svx_bam_merge_get_spill_stats(svx_bam_merge* m, svx_bam_sort_spill_stats* out);
int  svx_bam_merge_get_merge_stats(svx_bam_merge* m, svx_bam_merge_stats* out);
void svx_bam_merge_close(svx_bam_merge* m);
/* ---- a merge session in query-name order, spilled runs too (bamsort.hip: k_ns_pack, k_ns_keys_tab) ----
 * svx_bam_merge_open_order: svx_bam_merge_open is this call with SVX_SORT_COORDINATE; any other order than the two: SVX_E_ARG.  With SVX_SORT_QUERYNAME the
 * merged header is svx_bam_merge_header_host_order's and the merged file svx_bam_merge_host_order's.  Without a spill directory, or when no run is closed,
 * finish is the in-memory query-name sort over all files.  With one, a run that closes is sorted by name on the device and its names stay there in a table
 * of aligned words while its records go to the spill file; a record finish would refuse with SVX_E_ARG (refID, mate id, record size, name field) fails the
 * svx_bam_merge_add that closes its run, a position below -1 waits for finish (SVX_E_RANGE, behind every SVX_E_ARG).  Finish merges the runs by the same rank
 * pass and rounds over the table.  A session over ONE file with a spill directory is the spilled query-name sort of that file.  No index:
 * svx_bam_merge_index_fmt answers SVX_E_STATE after a query-name finish.
 * svx_bam_merge_get_name_stats: svx_bam_sort_get_name_stats for the session; after a finish over closed runs it describes the merge's rounds.
 * svx_bam_merge_get_name_spill_stats: the runs closed in query-name order - their number, the rounds and active rows summed over the runs' own sorts, the
 * bytes of the name table at finish, the host-clock times of the runs' name sorts and of the table's packing (zeros when no run was closed). */
typedef struct svx_bam_name_spill_stats {
    int64_t n_runs, run_rounds, run_active_rows, table_bytes;
    double  t_run_sort_ms, t_pack_ms;
} svx_bam_name_spill_stats;
int  svx_bam_merge_open_order(svx_bam* const* readers, int64_t k, int device, int64_t max_bytes, const char* spill_dir_or_null, int order, svx_bam_merge** out);
int  svx_bam_merge_get_name_stats(svx_bam_merge* m, svx_bam_name_sort_stats* out);
int  svx_bam_merge_get_name_spill_stats(svx_bam_merge* m, svx_bam_name_spill_stats* out);

/* ---- SAM text through the device reader (sam.hip, sam_core.hpp; the definition in words: svim_amd/sam.py) ----
 * svx_sam_open gives the handle type of svx_bam_open for a file of uncompressed SAM text (what an aligner writes): the header is parsed on the host
 * (svx_bam_header answers as for a BAM, sort_order from @HD), the alignment lines are turned into the BAM record stream on the device, slice by slice, and
 * everything behind that - field, CIGAR, SA and name decode, query-name grouping, svx_bam_sort_*, svx_bam_rewind, the contig limit - is the BAM path.
 * Device decode is the only reading route: svx_bam_read_batch before svx_bam_set_device_decode is SVX_E_STATE, and so are svx_bam_seek, svx_bam_index_begin
 * and svx_bam_set_gpu_inflate on such a handle (text has no virtual offsets).  After a sort pass svx_bam_sort_index gives the .bai of the sorted file.
 * A line the definition refuses fails the svx_bam_read_batch that would hand out the records of its slice: SVX_E_RANGE for a number that is missing, malformed
 * or out of its field's range, SVX_E_ARG otherwise; svx_last_error names the line by its number in the file: the first bad line, and of several faults in it
 * the first in the order svim_amd/sam.py states, as svx_sam_convert_host reports it.  The handle is usable again after svx_bam_rewind.
 * An RNAME or RNEXT the @SQ lines do not hold is refused (htslib warns and writes -1): deliberate.  A file with alignment lines and no @SQ line does not open.
 * Floats: at most 15 significant digits and a decimal exponent of at most 22 in magnitude are converted on the device (one correctly rounded operation on
 * exact operands, then the cast to float); every other value is resolved by strtod on the host before the slice is handed out (n_patched_floats).
 * SVX_SAM_DEV_CHUNK_BYTES (tests): the text bytes of a slice; a line longer than the slice makes it grow, and the grown slice ends behind that line. */
typedef struct svx_sam_stats {
    /* host clock, the stream drained at each boundary.  lines: newline marks and their scan; measure: the line ends, k_sam_measure, the scans of sizes and patch
     * counts and their read-back; emit: k_sam_emit and the read-back of the patch list; patch: strtod, the values to the device, k_sam_patch */
    double  t_stage_ms /* text to the device */, t_lines_ms, t_measure_ms, t_emit_ms, t_patch_ms;
    double  t_measure_kernel_ms, t_emit_kernel_ms;      /* k_sam_measure and k_sam_emit alone, between events on the stream */
    int64_t n_chunks, n_lines, n_records /* a read group re-read with the next slice (query-name mode) counts again */, text_bytes, stream_bytes, n_long_cigars, n_patched_floats;
} svx_sam_stats;
int  svx_sam_open(const char* path, int n_threads, svx_bam** out);
int  svx_sam_get_stats(svx_bam* h, svx_sam_stats* out);          /* zeros for a BAM handle, and before device decode is on */
/* host-only, no GPU: SAM text (header lines in front are skipped) -> the BAM records of its alignment lines.  names_blob: n_ref reference names, NUL-separated.
 * *n_out is the size also when cap is too small (SVX_E_CAPACITY).  SVX_E_ARG / SVX_E_RANGE: *bad_line is the 1-based number of the first line refused. */
int  svx_sam_convert_host(const uint8_t* text, int64_t n, int32_t n_ref, const char* names_blob, uint8_t* out, int64_t cap, int64_t* n_out, int64_t* n_records,
                          int64_t* bad_line);
/* host-only: the BAM header (magic, l_text, the text verbatim, the dictionary of its @SQ lines in order) of a SAM header text */
int  svx_sam_header_host(const char* header_text, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif
