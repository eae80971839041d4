/*
 * rappas_place.h -- C ABI of the MI355X-native phylo-kmer placement engine.
 *
 * Drop-in boundary for RAPPAS's query-placement hot path (`-p p`).  The reference (Java) has no
 * FFI seam; the boundary is cut where SURVEY.md section 8(b) puts it.  Paths below are relative to
 * the reference root.  Each entry point names the reference code it replaces; INTEGRATION.md shows
 * the JNI stub a RAPPAS maintainer would add on the Java side.
 *
 *   rk_db_create          <- the lookup structure behind session.hash:
 *                            src/core/hash/CustomHash_v4_FastUtil81.java:36,146-153 (+ HashStrategy.java:22-29)
 *                            fed from the walk SessionNext_v2.saveToJSON does (src/main_v2/SessionNext_v2.java:250-261)
 *                            and the scalars of src/main_v2/SessionNext_v2.java:43-66 (k, states, PPStarThreshold*).
 *   rk_place_batch        <- the per-read body of PlacementProcess.processQueries,
 *                            src/core/algos/PlacementProcess.java:645-1025 (knife init, k-mer loop, accumulate,
 *                            ambiguity mean/max :1129-1236, fillBestScoreList :396-451, LWR + keep-factor :974-1025),
 *                            with src/core/algos/AmbigSequenceKnife.java:98-272 and
 *                            src/core/DNAStatesShifted.java:115-143,182-243 / src/core/AAStates.java:48-197 underneath.
 *   rk_pack_reads_device  <- AmbigSequenceKnife.initTables char->state part (AmbigSequenceKnife.java:103-130) as a
 *                            device kernel: ASCII -> 2-bit / 5-bit packed records + per-read flags.
 *   rk_place_packed_device<- same body as rk_place_batch for reads already packed and resident in HBM.
 *
 * Conventions: plain C types only; inputs are borrowed for the duration of a call, outputs are
 * caller-owned; return 0 on success, <0 on error with a message in rk_last_error() (thread-local);
 * the library never calls exit().  The product path has no CPU fallback: every entry point that
 * computes placements requires a HIP device and fails with RK_ERR_NO_DEVICE otherwise.
 */
#ifndef RAPPAS_PLACE_H
#define RAPPAS_PLACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RK_VERSION 101 /* 0.1.1: rk_db_save / rk_db_save_desc / rk_db_load / rk_db_image_info / rk_db_image_user, rk_reserve_host_path, rk_count_work_device, RK_ERR_IO */

/* alphabets = number of unambiguous states (States.getNonAmbiguousStatesCount()) */
#define RK_ALPHABET_DNA 4  /* src/core/DNAStatesShifted.java : A=0 T/U=1 C=2 G=3, 2 bits/base   */
#define RK_ALPHABET_AA 20  /* src/core/AAStates.java : R H K D E S T N Q C G P A I L M F W Y V, 5 bits/residue */

/* ambiguity handling (src/main_v2/ArgumentsParser_v2.java:90-91; PlacementProcess.java:738-749) */
#define RK_AMB_SKIP 0 /* --noamb      */
#define RK_AMB_MEAN 1 /* default      */
#define RK_AMB_MAX 2  /* --ambwithmax */

/* k-mer -> row lookup structure */
#define RK_TABLE_AUTO 0   /* direct when sigma^k slots fit the budget, else hash */
#define RK_TABLE_HASH 1   /* open-addressed (linear probing), 16-byte slots {key, row descriptor} */
#define RK_TABLE_DIRECT 2 /* identity-hashed, collision-free special case over all sigma^k codes: compact 16-byte blocks of
                             12 k-mers (1.33 bytes per k-mer, L2-resident); falls back to DIRECT8 if a row exceeds 2040 entries */
#define RK_TABLE_DIRECT8 4 /* identity-hashed, one 8-byte row descriptor per code */

/* per-read result flags */
#define RK_FLAG_PLACED 1u         /* >=1 k-mer matched (L non-empty, PlacementProcess.java:797) */
#define RK_FLAG_BAD_CHAR 2u       /* unsupported character; the reference would System.exit(1) (AmbigSequenceKnife.java:124-128) */
#define RK_FLAG_TOO_SHORT 4u      /* R < k : no k-mer (the reference crashes for R < k-1) */
#define RK_FLAG_AMBIGUOUS 8u      /* read contains an ambiguity character */
#define RK_FLAG_BELOW_NSBOUND 16u /* best score < ns_bound: no jplace record (PlacementProcess.java:974) */
#define RK_FLAG_REVERSE 32u       /* the reported result of this read comes from its reverse complement (rk_place_*_strands; *_translated: frames 3..5) */
#define RK_FLAG_TOO_LONG 64u      /* device pack only: read longer than the packed record; not placed */

/* strand(s) a DNA read is placed on (rk_place_packed_device_strands / rk_place_batch_strands; the reference knows forward only) */
#define RK_STRAND_FORWARD 0 /* as given: the orientation of the reference alignment */
#define RK_STRAND_REVERSE 1 /* the reverse complement of every read */
#define RK_STRAND_BOTH 2    /* both, and per read the result with the better best score */

/* error codes */
#define RK_OK 0
#define RK_ERR_INVALID -1
#define RK_ERR_NO_DEVICE -2
#define RK_ERR_HIP -3
#define RK_ERR_NOMEM -4
#define RK_ERR_UNSUPPORTED -5
#define RK_ERR_IO -6 /* a database image file could not be read / written, or failed its size / checksum tests */

typedef struct rk_db rk_db;

typedef struct rk_db_desc {
    uint32_t alphabet;    /* RK_ALPHABET_DNA | RK_ALPHABET_AA */
    uint32_t convert_uo;  /* AA only: U->C, O->L (src/core/AAStates.java:118-123) */
    uint32_t k;           /* DNA: 2..31 (hashed table from k = 16: 4^k codes), AA: 2..12 */
    uint32_t n_branches;  /* originalTree.getNodeCount() (PlacementProcess.java:495-496); branch ids < n_branches <= 65535 */
    float thr_log10;      /* session.PPStarThresholdAsLog10 (T) */
    float thr;            /* session.PPStarThreshold (P), used by the ambiguity-mean path */
    uint64_t n_keys;
    const uint64_t *key_codes;   /* [n_keys] DNA: sum state_i<<(2i) (== little-endian compressMer bytes); AA: sum state_i<<(5i) */
    const uint64_t *row_offsets; /* [n_keys+1] CSR offsets into branch_ids/scores */
    const uint16_t *branch_ids;  /* [n_entries] (char)nodeId of CustomHash_v4_FastUtil81.java:79,87; unique within a row */
    const float *scores;         /* [n_entries] log10 PP*, finite */
    int32_t device;              /* HIP device ordinal */
    uint32_t table_mode;         /* RK_TABLE_* */
} rk_db_desc;

typedef struct rk_db_info {
    uint32_t alphabet, k, n_branches, table_mode;
    float thr_log10, thr;
    uint64_t n_keys, n_entries;
    uint64_t table_slots, table_bytes, rows_bytes; /* HBM footprint */
    uint32_t bits_per_symbol, max_row_len;
    int32_t device;
} rk_db_info;

typedef struct rk_params {
    uint32_t keep_at_most; /* --keep-at-most, default 7 (ArgumentsParser_v2.java:87); 1..16 */
    float keep_factor;     /* --keep-factor, default 0.01f (ArgumentsParser_v2.java:88) */
    uint32_t amb_mode;     /* RK_AMB_* */
    float ns_bound;        /* --nsbound / calibrationNormScore, default -INFINITY */
} rk_params;

typedef struct rk_counters {
    uint64_t reads, placed, unplaced, bad_char, too_short, ambiguous;
} rk_counters;

/* Result arrays, n_reads x keep_at_most, rows ordered best -> worse and already cut by keep_factor.
 * Unused rows: branch 0xFFFF, score -inf, lwr 0.  Host pointers for rk_place_batch, device pointers
 * for rk_place_packed_device.  Tie rule (the reference's is map-layout dependent): score desc, branch id asc. */
typedef struct rk_result {
    uint8_t *n_rows;   /* [n_reads]   rows emitted (0 => unplaced or gated) */
    uint16_t *branch;  /* [n_reads*K] original-tree node id of the edge's child */
    float *score;      /* [n_reads*K] S[x], bit-exact float32 */
    double *lwr;       /* [n_reads*K] likelihood weight ratio */
    uint32_t *flags;   /* [n_reads]   RK_FLAG_* */
} rk_result;

int rk_version(void);
const char *rk_last_error(void);

/* Main_DBBUILD_3.java:165-166 (float32 threshold pair from omega, #states, k) */
void rk_thresholds(float omega, uint32_t n_states, uint32_t k, float *thr, float *thr_log10);

int rk_db_create(const rk_db_desc *desc, rk_db **out);
/* Same argument checks and host-side image construction as rk_db_create, but no device is touched: lets the caller
 * (or a CPU-only test) validate a DB and learn its HBM footprint / table flavour.  info may be NULL. */
int rk_db_validate(const rk_db_desc *desc, rk_db_info *info);
void rk_db_destroy(rk_db *db);
/* Another handle of the same database on `device` (it may be the source's own device), copied device to device -- over xGMI
 * between GPUs -- instead of being rebuilt and uploaded once per GPU: what a single-process caller (one JVM, rk_place_batch_multi)
 * does after the first rk_db_create, and the only way to replicate an image that exists in HBM only (rk_db_create_synth). */
int rk_db_clone(const rk_db *src, int32_t device, rk_db **out);
int rk_db_get_info(const rk_db *db, rk_db_info *info);

/* The database as a file: the HBM image exactly as the kernels read it (k-mer table, row blob, window spans) behind a fixed header,
 * so that loading is mmap + one host-to-device copy per section -- no parse, no rebuild.  Stands where the reference stores and
 * reloads its Java-serialised session (src/main_v2/SessionNext_v2.java:110-154 storeHash, :158-207 load); only the lookup structure
 * and the scalars of rk_db_desc are kept -- whatever else the caller needs next to it (rk_place: the reference tree) travels as an
 * opaque `user` blob the engine never looks inside.
 *   rk_db_save        a handle's image, read back from the device.
 *   rk_db_save_desc   the same file from the caller's CSR arrays, built on the host: no device is touched (desc->device is ignored).
 *   rk_db_load        a new handle on `device`; size, header and payload checksums are verified before the device is looked at, a
 *                     truncated / overwritten / bit-flipped file is refused with RK_ERR_IO.  (Integrity, not authenticity: an image
 *                     is trusted input, like the library itself.)
 *   rk_db_image_info  the same checks without a device; info (device = -1) and the user blob's length, either may be NULL.
 *   rk_db_image_user  the user blob: at most `cap` bytes into buf, *len = its full length.
 * Files are little-endian and specific to the image version this library writes (a newer / older file is refused, not guessed at). */
int rk_db_save(const rk_db *db, const char *path, const void *user, uint64_t user_bytes);
int rk_db_save_desc(const rk_db_desc *desc, const char *path, const void *user, uint64_t user_bytes);
int rk_db_load(const char *path, int32_t device, rk_db **out);
int rk_db_image_info(const char *path, rk_db_info *info, uint64_t *user_bytes);
int rk_db_image_user(const char *path, void *buf, uint64_t cap, uint64_t *len);

/* One row read back out of the HBM image through the same table lookup and entry decode the placement kernels use:
 * the engine's counterpart of CustomHash_v4_FastUtil81.getPairsOfTopPosition2 (src/core/hash/CustomHash_v4_FastUtil81.java:146-153;
 * null there <=> *len == 0 here).  Entries come back in the image's order (large-tree images: ascending branch id).  At most
 * `cap` entries are written; *len is the row's full length.  For checkers and tools, not for the hot path (one launch per call). */
int rk_db_fetch_row(rk_db *db, uint64_t code, uint32_t cap, uint32_t *len, uint16_t *branch_ids, float *scores);

/* The seeded synthetic database of the measurement plan (keys = a random subset of the code space,
 * row length 1 + geometric, branch ids a contiguous window, scores v = T*u), generated ON THE DEVICE straight into the HBM
 * image -- the only way a C5-class (~200 GB) database can exist, since no host holds its CSR form.  Every value is a pure
 * function of (seed, dense k-mer index, entry index) in integer arithmetic plus one float32 multiply (definition at the top of
 * rappas_amd/csrc/rk_synth_impl.h), so a checker regenerates any row on the host (rappas_amd/synth.py: synth_rows) and
 * rk_db_fetch_row reads it back.  The reference has no counterpart (its databases come out of `-p b`); this is bench / test
 * input, built by the same library because only the library knows the image format. */
typedef struct rk_synth_desc {
    uint32_t alphabet, convert_uo, k, n_branches;
    float thr_log10, thr;
    uint64_t seed;
    double key_fraction;  /* probability that a code of the k-mer space carries a row, in (0, 1] */
    double mean_row_len;  /* rows are 1 + geometric with this mean, capped at n_branches - 1 */
    int32_t device;
    uint32_t table_mode;  /* RK_TABLE_* */
} rk_synth_desc;
int rk_db_create_synth(const rk_synth_desc *desc, rk_db **out);

/* Host-buffer entry point: ASCII reads (concatenated, seq_off[n_reads+1]) -> results in host memory.
 * Internally: H2D, device-side pack, placement kernel(s), D2H; chunked to bound device memory. */
int rk_place_batch(rk_db *db, const rk_params *p, uint64_t n_reads, const uint8_t *seq_ascii,
                   const uint64_t *seq_off, rk_result *out, rk_counters *counters);

/* Optional: sets up ahead of time what the first rk_place_batch / rk_place_batch_packed of a handle otherwise sets up on its way
 * (streams, device buffers and page-locked staging for full chunks of reads of up to max_read_len symbols: ~80 ms), e.g. while the
 * caller is still reading its input.  Nothing is placed. */
int rk_reserve_host_path(rk_db *db, uint32_t keep_at_most, uint32_t max_read_len);

/* The same for reads the host has already packed (2 bits per base / 5 per residue, symbol i at bits [i*b, (i+1)*b) of the
 * record's little-endian bit string -- the layout rk_pack_reads_device produces): 38 instead of 150 bytes per 150-bp read cross
 * PCIe.  lens NULL => every read has fixed_len symbols; flags NULL => no read carries BAD_CHAR / AMBIGUOUS.  seq_ascii / seq_off
 * (both or neither) are consulted only for chunks that hold a read flagged AMBIGUOUS (the ambiguity path of
 * PlacementProcess.java:1129-1236 works on characters); without them such reads come back unplaced with the flag set.
 * rk_pack_reads_host is the matching host-side packer (AmbigSequenceKnife.java:103-130 char -> state, threaded; n_threads 0 =
 * auto): it writes the records, lengths and flags exactly as the device packer does. */
int rk_place_batch_packed(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                          const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                          const uint64_t *seq_off, rk_result *out, rk_counters *counters);
int rk_pack_reads_host(const rk_db *db, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off, uint32_t words_per_read,
                       uint32_t *packed, uint32_t *lens, uint32_t *flags, uint32_t n_threads);
/* The same packer without a database handle (no GPU involved): `alphabet` RK_ALPHABET_DNA / RK_ALPHABET_AA, `convert_uo` the
 * database's --convertUO switch (AAStates.java:118-123), `k` for RK_FLAG_TOO_SHORT.  words_per_read >= ceil(longest read * b / 32),
 * b = 2 (DNA) / 5 (amino acids); longer reads are cut and flagged RK_FLAG_TOO_LONG. */
int rk_pack_reads(uint32_t alphabet, int convert_uo, uint32_t k, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off,
                  uint32_t words_per_read, uint32_t *packed, uint32_t *lens, uint32_t *flags, uint32_t n_threads);

/* The same over several GPUs from ONE host process (RAPPAS is a single JVM): dbs[g] are handles of the same database created
 * on different devices (rk_db_create with desc.device = g); the batch is cut into n_dbs contiguous shards, shard g goes to
 * dbs[g] on its own host thread, and every shard writes its slice of the caller's result arrays -- reads are independent
 * (PlacementProcess.java:1067-1075 resets all per-read state), so there is no exchange step and no collective.  Results are
 * identical to one rk_place_batch call over the whole batch.  If a shard's device fails (a HIP error, out of memory) the shard is
 * placed again on the handles that finished, in a fresh host thread; the call then still returns RK_OK and rk_last_error()
 * names the device that dropped out ("" when nothing failed).  The call fails only when no healthy device is left for a shard. */
int rk_place_batch_multi(rk_db *const *dbs, uint32_t n_dbs, const rk_params *p, uint64_t n_reads, const uint8_t *seq_ascii,
                         const uint64_t *seq_off, rk_result *out, rk_counters *counters);

/* Page-locked host memory for the buffers handed to rk_place_batch: the DMA then reads / writes them directly.  Pageable
 * buffers work too (they are staged through page-locked memory inside the library, ~1.2e8 reads/s either way on C2); pinned
 * ones save the host threads that staging keeps busy.  A JVM can wrap the allocation with NewDirectByteBuffer. */
void *rk_host_alloc(uint64_t bytes);
void rk_host_free(void *p);

/* Packed-record geometry for a given maximum read length: 32-bit words per record. */
uint32_t rk_packed_words(const rk_db *db, uint32_t max_len);

/* Device entry points (all pointers are device pointers on db's device; stream = hipStream_t or NULL).
 * rk_pack_reads_device: ASCII -> packed records [n_reads][words_per_read] + lens[n_reads] + flags[n_reads]. */
int rk_pack_reads_device(rk_db *db, uint64_t n_reads, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off,
                         uint32_t words_per_read, uint32_t *d_packed, uint32_t *d_lens, uint32_t *d_flags,
                         void *stream);
/* rk_place_packed_device: d_lens may be NULL (every read has fixed_len symbols); d_flags_in may be NULL
 * (no read carries BAD_CHAR/AMBIGUOUS).  Reads flagged AMBIGUOUS need d_seq_ascii/d_seq_off (else they are
 * reported unplaced with the flag set).  Asynchronous on `stream`.  d_flags_in may be the output flag array itself (in place).
 * What the call allocates: nothing from the device's memory pools; the handle keeps one grow-only scratch block per stream it has
 * been launched on (the order the kernels take a large batch's reads in, the marks of tiles one kernel hands to the next: ~5 bytes a
 * read, plain hipMalloc, freed by rk_db_destroy) -- so calls on ONE stream must not overlap in time from different threads, and a
 * call made while the stream is being captured into a graph does without the block if it would have to grow. */
int rk_place_packed_device(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *d_packed,
                           uint32_t words_per_read, const uint32_t *d_lens, uint32_t fixed_len,
                           const uint32_t *d_flags_in, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off,
                           const rk_result *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DNA reads on either strand.  The reference places a read in the orientation it arrives in only
 * (src/core/algos/PlacementProcess.java:645-1025 walks the query as given); shotgun and amplicon reads arrive in either.  With
 * A=0 T=1 C=2 G=3 (src/core/DNAStatesShifted.java:182-209) the complement of a state is state ^ 1, so the other strand of a packed
 * record is made on the device, and reads being independent (PlacementProcess.java:1067-1075) the better strand is a per-read
 * choice.  DNA only: on an amino-acid handle every entry point below fails with RK_ERR_UNSUPPORTED.  Device pointers and `stream`
 * as for rk_place_packed_device.
 *   rk_revcomp_packed_device  records [n_reads][words_per_read] -> d_packed_out (same geometry; must not alias d_packed): for a read
 *                             of R symbols (d_lens[r], or fixed_len when d_lens is NULL) output symbol j = input symbol R-1-j xor 1,
 *                             every bit from 2R on is zero (the packer's padding).  Lengths and flags do not depend on the strand
 *                             and are not rewritten.
 *   rk_revcomp_ascii_device   the same for characters, offsets unchanged: read r's bytes reversed and complemented -- A<->T, U->A,
 *                             C<->G, R<->Y, K<->M, B<->V, D<->H; S W N . - stay; case is kept; any other byte is copied (an
 *                             unsupported character stays one).  d_out_ascii must not alias d_seq_ascii.
 *   rk_merge_strands_device   d_fwd (in/out) and d_rev: two result sets of the same reads and keep_at_most.  Per read the reverse
 *                             result is taken if and only if n_rows_rev > 0 and (n_rows_fwd == 0 or score_rev[0] > score_fwd[0] as
 *                             float32); a tie keeps forward.  Taking it copies n_rows, all keep_at_most rows of branch / score / lwr
 *                             and the flags, and sets RK_FLAG_REVERSE.
 *   rk_strands_work_bytes     bytes of caller-owned device workspace rk_place_packed_device_strands needs for such a batch: the
 *                             reverse records, a second result set and -- ascii_bytes > 0: the total length of the reads' characters,
 *                             d_seq_off[n_reads] -- the reversed characters.  0 (and a message) on a bad argument.
 *   rk_place_packed_device_strands
 *                             rk_place_packed_device on the strand(s) asked for.  RK_STRAND_FORWARD is exactly that call (d_work may
 *                             be NULL).  RK_STRAND_REVERSE makes the reverse records in the workspace, places them into d_out and sets
 *                             RK_FLAG_REVERSE on every read.  RK_STRAND_BOTH places the reverse records into the workspace's result
 *                             set and the reads as given into d_out, then merges into d_out.  Two placement passes: a fused kernel is
 *                             not part of this version.  Allocates nothing; a workspace smaller than rk_strands_work_bytes(...,
 *                             ascii_bytes = 0) or an unknown strand is RK_ERR_INVALID, and nothing is launched.  The reversed
 *                             characters (made only for the reads the ambiguity kernel takes, and only when d_flags_in, d_seq_ascii
 *                             and d_seq_off are all given) go behind that part: the call cannot see d_seq_off[n_reads] without
 *                             waiting for the stream, so what the workspace holds beyond it is their room -- none at all is
 *                             RK_ERR_INVALID, no byte is written past it.  Asynchronous on `stream`; the one-stream rule of
 *                             rk_place_packed_device holds (the handle's launch scratch is used through that call).
 *   rk_place_batch_strands    rk_place_batch on the strand(s) asked for: the same chunked host path, the workspace part of the
 *                             handle's host-path buffers (grow-only, freed by rk_db_destroy); a chunk's characters are reversed only
 *                             if it holds a read flagged AMBIGUOUS.  counters are taken from the final flags.  Results equal
 *                             rk_place_packed_device_strands over the whole batch, whatever the chunking.
 * ------------------------------------------------------------------------------------------------------------------ */
int rk_revcomp_packed_device(rk_db *db, uint64_t n_reads, const uint32_t *d_packed, uint32_t words_per_read, const uint32_t *d_lens,
                             uint32_t fixed_len, uint32_t *d_packed_out, void *stream);
int rk_revcomp_ascii_device(rk_db *db, uint64_t n_reads, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off, uint8_t *d_out_ascii,
                            void *stream);
int rk_merge_strands_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_fwd, const rk_result *d_rev,
                            void *stream);
uint64_t rk_strands_work_bytes(const rk_db *db, uint64_t n_reads, uint32_t words_per_read, uint32_t keep_at_most, uint64_t ascii_bytes);
int rk_place_packed_device_strands(rk_db *db, const rk_params *p, uint32_t strand, uint64_t n_reads, const uint32_t *d_packed,
                                   uint32_t words_per_read, const uint32_t *d_lens, uint32_t fixed_len, const uint32_t *d_flags_in,
                                   const uint8_t *d_seq_ascii, const uint64_t *d_seq_off, const rk_result *d_out, void *d_work,
                                   uint64_t work_bytes, void *stream);
int rk_place_batch_strands(rk_db *db, const rk_params *p, uint32_t strand, uint64_t n_reads, const uint8_t *seq_ascii,
                           const uint64_t *seq_off, rk_result *out, rk_counters *counters);

/* ------------------------------------------------------------------------------------------------------------------
 * DNA reads on amino-acid databases: six-frame translation on the device.  The reference places a read as given
 * (src/core/algos/PlacementProcess.java:645-1025), so a DNA read meets a protein database only after the caller has translated it;
 * here the 2-bit record is translated on the device, each frame is placed, and the best frame is a per-read merge, as for strands.
 * Amino-acid databases only: on a DNA handle every entry point below that takes one fails with RK_ERR_UNSUPPORTED and launches
 * nothing.  These entry points were added without a bump of RK_VERSION (no struct changed).
 *   Input      2-bit DNA records as rk_pack_reads(RK_ALPHABET_DNA, ...) writes them (A=0 T=1 C=2 G=3, symbol i at bits [2i, 2i+2)),
 *              their lengths (or fixed_len) and, optionally, the packer's flags.
 *   Frames     0, 1, 2: the record as given from base offset 0, 1, 2; 3, 4, 5: its reverse complement (state ^ 1,
 *              src/core/DNAStatesShifted.java:182-209) from offset 0, 1, 2, read straight from the forward record: codon j of frame
 *              3+o is bases R-1-o-3j, R-2-o-3j, R-3-o-3j, each xor 1.  A frame has floor((R - o) / 3) codons, none when R < o + 3.
 *   Code       the standard genetic code (NCBI table 1) only; residue states in the order of src/core/AAStates.java:48-197 (R=0 H=1
 *              K=2 D=3 E=4 S=5 T=6 N=7 Q=8 C=9 G=10 P=11 A=12 I=13 L=14 M=15 F=16 W=17 Y=18 V=19); convert_uo plays no part.
 *   Stops      the reference reads '*' as a fully ambiguous residue (AAStates.java:103) and a packed record cannot carry ambiguity,
 *              so a frame's record is its LONGEST STOP-FREE RUN of residues (TAA, TAG, TGA end a run; of runs of equal length the
 *              first): 5 bits a residue from bit 0, every bit from 5 * len on zero (the packer's padding), len 0 for a frame without
 *              residues.  A frame shorter than k comes back RK_FLAG_TOO_SHORT from the placement itself.
 *   Flags      RK_FLAG_BAD_CHAR / RK_FLAG_AMBIGUOUS / RK_FLAG_TOO_LONG of the DNA read are handed to every frame's placement as
 *              d_flags_in: such reads come back unplaced with the flag set (rk_place_packed_device without characters).  Translating
 *              ambiguous bases into ambiguous residues is NOT part of this version.  The packer's RK_FLAG_TOO_SHORT speaks of bases,
 *              not residues, and is dropped.
 *   rk_translate_packed_device   one frame of every read: records -> d_aa_out [n_reads][aa_words] and d_aa_lens_out [n_reads].
 *                                aa_words >= rk_packed_words(db, L / 3), L = fixed_len when d_dna_lens is NULL, else the 16 * dna_words
 *                                bases a record holds (lengths beyond it are cut to it); anything smaller, or frame > 5, is
 *                                RK_ERR_INVALID.  Words beyond the run are written as zero.
 *   rk_translate_packed_host     the same words and lengths in plain C++ on the host: no handle, no GPU (the alphabet is implied).
 *   rk_merge_frames_device       d_best (in/out, with its frame bytes d_best_frame) and d_cand, the result set of frame cand_frame
 *                                (0..5): per read the candidate is taken if and only if n_rows_c > 0 and (n_rows_best == 0 or
 *                                score_c[0] > score_best[0] as float32); a tie keeps the earlier frame.  Taking it copies n_rows, all
 *                                keep_at_most rows of branch / score / lwr and the flags, writes cand_frame into d_best_frame[r] and,
 *                                for cand_frame >= 3, sets RK_FLAG_REVERSE.
 *   rk_translated_work_bytes     bytes of caller-owned device workspace rk_place_packed_device_translated needs: one amino-acid
 *                                record set, one array of lengths, one result set -- frames are processed one after the other, so it
 *                                does not grow with their number.  0 (and a message) on a bad argument.
 *   rk_place_packed_device_translated
 *                                frame 0 is placed straight into d_out, frames 1..5 one at a time into the workspace's result set and
 *                                merged into d_out; d_frame[r] is the frame the reported result comes from, 0xFF for a read with
 *                                n_rows == 0.  ns_bound gates each frame on its own.  Six placement passes: a fused kernel is not part
 *                                of this version.  d_dna_flags may be NULL but must not be d_out->flags.  Allocates nothing; a
 *                                workspace smaller than rk_translated_work_bytes is RK_ERR_INVALID and nothing is launched.
 *                                Asynchronous on `stream`; the one-stream rule of rk_place_packed_device holds.
 *   rk_place_batch_translated    DNA characters from the host: packed there (rk_pack_reads), then the device call, chunk by chunk, in
 *                                buffers that are part of the handle's host-path block (grow-only, freed by rk_db_destroy); counters
 *                                are taken from the final flags (too_short: the reported frame has fewer than k residues).  Results
 *                                equal one rk_place_packed_device_translated call over the whole batch, whatever the chunking.
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_FRAME_NONE 0xFFu /* d_frame of a read without a result */
int rk_translate_packed_device(rk_db *db, uint32_t frame, uint64_t n_reads, const uint32_t *d_dna, uint32_t dna_words,
                               const uint32_t *d_dna_lens, uint32_t fixed_len, uint32_t *d_aa_out, uint32_t aa_words, uint32_t *d_aa_lens_out,
                               void *stream);
int rk_translate_packed_host(uint32_t frame, uint64_t n_reads, const uint32_t *dna, uint32_t dna_words, const uint32_t *dna_lens,
                             uint32_t fixed_len, uint32_t *aa_out, uint32_t aa_words, uint32_t *aa_lens_out);
int rk_merge_frames_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_best, uint8_t *d_best_frame,
                           const rk_result *d_cand, uint32_t cand_frame, void *stream);
uint64_t rk_translated_work_bytes(const rk_db *db, uint64_t n_reads, uint32_t dna_words, uint32_t keep_at_most);
int rk_place_packed_device_translated(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *d_dna, uint32_t dna_words,
                                      const uint32_t *d_dna_lens, uint32_t fixed_len, const uint32_t *d_dna_flags, const rk_result *d_out,
                                      uint8_t *d_frame, void *d_work, uint64_t work_bytes, void *stream);
int rk_place_batch_translated(rk_db *db, const rk_params *p, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off,
                              rk_result *out, uint8_t *frame_out, rk_counters *counters);

/* ------------------------------------------------------------------------------------------------------------------
 * Edge masses: the per-branch LWR sums of a result set.  The reference writes one jplace record per read
 * (src/main_v2/Main_PLACEMENT_v07.java:150-320) and leaves the table most users are after -- how much likelihood weight landed on each
 * branch -- to the tools behind it; here it is summed where the results are, so a device caller copies 2 * B + 4 words instead of
 * ~100 bytes a read.  Works on the result set of any placement entry point (plain, strands, translated), either alphabet.
 *   Mass buffer  2 * B + 4 little-endian 64-bit words for a tree of B = n_branches:
 *                  [0, B)    mass_q30[x]  sum over the counted rows on branch x of w_r * q(lwr)
 *                  [B, 2B)   best[x]      sum of w_r over the reads whose row 0 is branch x
 *                  2B + 0    sum of w_r over all reads of the calls
 *                  2B + 1    sum of w_r over the reads with at least one counted row
 *                  2B + 2    sum of w_r * (counted rows of r)
 *                  2B + 3    rows skipped because their branch id was >= B (not weighted)
 *   Terms        w_r = weights[r], or 1 when weights is NULL (0 is legal: such a read adds 0 everywhere).  The rows of read r are
 *                e < min(n_rows[r], keep_at_most); what lies behind them is never looked at.  q(l) = llrint(min(l, 1.0) * 2^30) for
 *                l >= 0 (ties to even; the product is exact in binary64), 0 for a negative or NaN.  A row with branch >= B is never
 *                used as an index: it is skipped, counted in word 2B + 3 and adds to no other word (as row 0: nothing to best either)
 *                -- a bounds check, the engine's own results never meet it.  score and flags of the result are not read and may be
 *                NULL; n_rows == 0 already says unplaced or gated.
 *   Exactness    all sums are integers, so they do not depend on the order of the adds: device, host and any split into calls give
 *                the same words.  One add is below 2^62, so a buffer is exact while the sum of w_r stays below 2^33 (not checked).
 *   Adding       calls ADD into the buffer; zeroing it is the caller's hipMemsetAsync / memset.  Buffers of chunks, batches, streams
 *                and GPUs combine by element-wise integer addition.  The result set is read, never written.
 *   rk_masses_words              words of a mass buffer: 2 * n_branches + 4; 0 for n_branches == 0 or > 65535.
 *   rk_masses_accumulate_device  device pointers on db's device, B from the handle.  Asynchronous on `stream`, allocates nothing and
 *                                does not use the handle's per-stream launch scratch: the one-stream rule of rk_place_packed_device
 *                                does not apply to it.
 *   rk_masses_accumulate_host    the same words in plain C++: no handle, no GPU.  Every thread sums privately, the partial sums are
 *                                added at the end; n_threads 0 = automatic, at most 16.
 * RK_ERR_INVALID (and a message) for a NULL n_rows / branch / lwr / mass buffer, keep_at_most outside 1..16 and n_reads >= 2^32: then
 * nothing is launched and no byte is written.  n_reads == 0 is RK_OK and touches nothing.  Added without a bump of RK_VERSION (no
 * struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
uint64_t rk_masses_words(uint32_t n_branches);
int rk_masses_accumulate_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, const uint32_t *d_weights,
                                uint64_t *d_masses, void *stream);
int rk_masses_accumulate_host(uint32_t n_branches, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, const uint32_t *weights,
                              uint64_t *masses, uint32_t n_threads);

/* ------------------------------------------------------------------------------------------------------------------
 * Profile-only placement: reads from the host in, a mass buffer out, no result set on the host.  Each chunk of the host path is
 * placed as by the corresponding entry point and summed where its results lie (rk_masses_accumulate_device on the chunk's stream,
 * into a buffer of the handle's); of a chunk's results only the flags (4 bytes a read) come back.
 *   rk_place_batch_masses         characters; `step` is RK_STRAND_FORWARD / _REVERSE / _BOTH or RK_STEP_TRANSLATED (six reading frames of
 *                                 DNA characters on an amino-acid handle).
 *   rk_place_batch_packed_masses  the arguments of rk_place_batch_packed (forward).
 * Contract.  Let R be the result set that the corresponding existing entry point -- rk_place_batch, rk_place_batch_strands,
 * rk_place_batch_translated or rk_place_batch_packed -- returns for the same arguments.  After the call `masses` (host memory,
 * rk_masses_words(B) words) holds its previous content plus exactly what rk_masses_accumulate_host(B, p->keep_at_most, n_reads, R,
 * weights, masses, ...) would add; flags_out (optional, [n_reads]) equals R.flags; counters (optional) equal that call's counters.
 * weights is NULL or [n_reads].  The frame bytes of the translated step do not come back.  The result does not depend on how the
 * batch is cut into chunks.  Exactness as for the other masses calls: while the sum of the weights stays below 2^33.
 * The handle keeps one device mass buffer of rk_masses_words(B) * 8 bytes (at most 1 MB), allocated at the first such call (or by
 * rk_reserve_host_path) and freed by rk_db_destroy; it is zeroed at the start of a call, the chunks' streams add into it side by side
 * and one copy brings it to the host at the end.  Calls on one handle are serialised, as all host calls are.
 * Errors.  RK_ERR_INVALID (and a message) for a NULL handle or masses, NULL reads with n_reads > 0, keep_at_most outside 1..16 and
 * step > 3; RK_ERR_UNSUPPORTED for a strand step other than forward on an amino-acid handle and for the translated step on a DNA
 * handle: then nothing is launched and no byte of masses or flags_out is written.  An error later in the call leaves masses as it
 * was.  n_reads == 0 is RK_OK and touches neither.  Added without a bump of RK_VERSION (no struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_STEP_TRANSLATED 3u /* `step` beside RK_STRAND_FORWARD/REVERSE/BOTH: six reading frames, amino-acid handles only */
int rk_place_batch_masses(rk_db *db, const rk_params *p, uint32_t step, uint64_t n_reads, const uint8_t *seq_ascii,
                          const uint64_t *seq_off, const uint32_t *weights, uint64_t *masses, uint32_t *flags_out, rk_counters *counters);
int rk_place_batch_packed_masses(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                                 const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                                 const uint64_t *seq_off, const uint32_t *weights, uint64_t *masses, uint32_t *flags_out,
                                 rk_counters *counters);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-sample edge masses from one batch: a membership list per read.  A study pools and deduplicates the reads of many samples,
 * places each distinct sequence once and hands its abundance back to every sample it occurs in.  A unique read belongs to several
 * samples with a multiplicity of its own in each, so the input is a sparse list of entries, not one sample per read.
 *   Membership entry    (read index, sample index, weight), all uint32.  A read may have zero, one or many entries; the same (read,
 *                       sample) pair may repeat.
 *   Sample mass buffer  for S samples on a tree of B branches: S * W + 1 little-endian 64-bit words, W = rk_masses_words(B) = 2B + 4.
 *                         [s * W, (s + 1) * W)  an ordinary mass buffer for sample s: exactly what rk_masses_accumulate_host adds for
 *                                               the result set gathered by the entries of sample s -- row i of the gathered set is the
 *                                               result of read member_read[i], its weight member_weight[i].  A read with two entries
 *                                               in one sample counts twice there, the skipped-row word included.
 *                         S * W                 entries skipped because sample >= S or read >= n_reads.  Such an entry is never used
 *                                               as an index and adds to no other word -- a bounds check, as the branch >= B rule is.
 *   Exactness           every term is an integer: device, host twin and any split into calls, chunks, streams or GPUs give the same
 *                       words.  Per sample: exact while the sum of its weights stays below 2^33 (not checked).
 *   Limits              1 <= S <= 65535 and S * W + 1 <= 2^29 words (4 GiB).
 *   Adding              calls ADD into the buffer; zeroing it is the caller's job.
 *   rk_masses_samples_words              S * W + 1; 0 on a bad argument or beyond the limit.
 *   rk_masses_accumulate_samples_device  device pointers on db's device, B from the handle.  d_member_read NULL: entry i is read i
 *                                        (n_members == n_reads); d_member_weight NULL: 1.  Asynchronous on `stream`, allocates nothing
 *                                        and does not use the handle's launch scratch.
 *   rk_masses_accumulate_samples_host    the same words in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16: threads
 *                                        share the entries and sum privately while the partial buffers stay small, else they share the
 *                                        samples and need none.
 *   rk_place_batch_masses_samples        rk_place_batch_masses with the membership in place of `weights`: member_off [n_reads + 1] is
 *   rk_place_batch_packed_masses_samples a CSR over the reads (read r owns entries member_off[r] .. member_off[r + 1] of member_sample
 *                                        and member_weight); member_off NULL: one entry per read, entry r is read r.  member_weight
 *                                        NULL: 1.  `step` and its RK_ERR_UNSUPPORTED cases as in rk_place_batch_masses.  Let R be the
 *                                        result set of the corresponding existing entry point for the same reads: `masses` (host
 *                                        memory, rk_masses_samples_words(B, S) words) ends as its previous content plus what
 *                                        rk_masses_accumulate_samples_host adds over R with the CSR expanded; flags_out and counters
 *                                        equal that call's.  The result does not depend on the chunking.  The handle's device mass
 *                                        buffer grows to S * W + 1 words at the first such call; an error later in the call leaves
 *                                        `masses` as it was.
 * RK_ERR_INVALID (and a message), before anything is launched or written, for a NULL required pointer, keep_at_most outside 1..16,
 * n_reads or n_members >= 2^32 (the accumulate calls), S outside its limits, d_member_read == NULL with n_members != n_reads, member_off[0] != 0 or a
 * decreasing member_off.  n_members == 0 is RK_OK and touches nothing.  Added without a bump of RK_VERSION (no struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
uint64_t rk_masses_samples_words(uint32_t n_branches, uint32_t n_samples);
int rk_masses_accumulate_samples_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, uint32_t n_samples,
                                        uint64_t n_members, const uint32_t *d_member_read, const uint32_t *d_member_sample,
                                        const uint32_t *d_member_weight, uint64_t *d_masses, void *stream);
int rk_masses_accumulate_samples_host(uint32_t n_branches, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, uint32_t n_samples,
                                      uint64_t n_members, const uint32_t *member_read, const uint32_t *member_sample,
                                      const uint32_t *member_weight, uint64_t *masses, uint32_t n_threads);
int rk_place_batch_masses_samples(rk_db *db, const rk_params *p, uint32_t step, uint64_t n_reads, const uint8_t *seq_ascii,
                                  const uint64_t *seq_off, uint32_t n_samples, const uint64_t *member_off, const uint32_t *member_sample,
                                  const uint32_t *member_weight, uint64_t *masses, uint32_t *flags_out, rk_counters *counters);
int rk_place_batch_packed_masses_samples(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                                         const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                                         const uint64_t *seq_off, uint32_t n_samples, const uint64_t *member_off,
                                         const uint32_t *member_sample, const uint32_t *member_weight, uint64_t *masses,
                                         uint32_t *flags_out, rk_counters *counters);

/* ------------------------------------------------------------------------------------------------------------------
 * Sample-level output: clade masses and the pairwise Kantorovich-Rubinstein (earth mover's, "phylogenetic KR") distances between
 * the samples of a sample mass buffer (what `guppy kr` / `gappa krd` compute from jplace files).  The reference has no counterpart.
 *   Tree handle         rk_tree_create uploads the shape of a tree of B = n_branches nodes (1..65535, the B of the mass buffers):
 *                       parent[x] = node id of x's parent, -1 for the one root (branch id = node id, as everywhere here; the ids need
 *                       not be in pre-order); branch_len[x] = length of the edge above x, the root's entry ignored and taken as 0.
 *                       The host walks the tree once, iteratively, children in ascending id.  rk_tree_validate: the same checks
 *                       without a device.  RK_ERR_INVALID and a message, before any device is touched, for a NULL pointer, B out of
 *                       range, no root or more than one, a parent >= B or equal to x, a node that does not reach the root (a cycle),
 *                       a length that is negative, NaN or infinite.  rk_tree_destroy(NULL) is a no-op; it is the only thing that
 *                       frees.  A handle is read-only after creation: any number of calls on any streams may share it.
 *   Clade masses        `masses` is a sample mass buffer as rk_masses_samples_words(B, S) lays it out (S blocks of W = 2B + 4 words and
 *                       the skipped-entries word, which is never read: with S = 1 an ordinary mass buffer of W words is accepted as it
 *                       is).  clade[s * B + x] = the sum of mass_q30 of sample s over x's subtree, x included: the clade_mass_q30
 *                       column of the per-edge table.  Integers: device, host twin and the table agree word for word (exact while a
 *                       sample's total stays below 2^63, which sum of weights < 2^33 gives).  The output is WRITTEN, not added into.
 *                       rk_clade_masses_device is asynchronous on `stream`, allocates nothing and uses no scratch of any handle.
 *   KR distance         RAPPAS gives no position along an edge: a branch's mass sits at the midpoint of its edge, mass on the root at
 *                       the root node.  For sample s: m_s(x) = mass_q30[x], c_s(x) its clade sum, T_s = c_s(root), h[x] =
 *                       (double)branch_len[x] * 0.5 (h[root] = 0).  The KR integral of |P_s(y) - P_t(y)| over the tree, P(y) the share
 *                       of the mass on the distal side of y, splits every edge into a proximal half (distal mass c) and a distal half
 *                       (distal mass c - m):
 *                           u_s(x) = (double)c_s(x) / (double)T_s        v_s(x) = (double)(c_s(x) - m_s(x)) / (double)T_s
 *                           term1  = h[x] * fabs(u_s(x) - u_t(x))        term2  = h[x] * fabs(v_s(x) - v_t(x))
 *                       all in binary64 with IEEE conversions and division, no contraction.
 *   Order of the sum    fixed, so that every implementation gives the same bits: nodes in ascending id, in chunks of RK_KR_CHUNK ids;
 *                       a chunk's partial p_c starts at +0.0 and takes acc = (acc + term1) + term2 node after node; D[s][t] = p_0,
 *                       then + p_1, + p_2, ... in chunk order (B <= RK_KR_CHUNK: one sequential sum).
 *   Consequences        D is bitwise symmetric.  D[s][s] is +0.0 for a non-empty sample.  A sample with T_s = 0 has u = v = 0 / 0 =
 *                       NaN: its whole row and column, the diagonal included, are NaN (no special case).  The result does not depend
 *                       on grid, tile shape or stream.
 *   rk_kr_work_bytes        bytes of the caller-owned device workspace for S samples (the clade sums, the profiles, per-chunk partials
 *                           when the matrix is small); 0 and a message on a bad argument or when it would pass 2^40 bytes.
 *   rk_kr_distances_device  d_out [S * S] doubles, row-major, written.  d_work 16-byte aligned, work_bytes >= rk_kr_work_bytes: too
 *                           small (or a NULL pointer) is RK_ERR_INVALID and nothing is launched.  1 <= S <= 65535.  Asynchronous on
 *                           `stream`; calls that share a workspace must be ordered by the caller.
 *   rk_kr_distances_host    the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_kr_distances_batch   the drivers' call: host buffer in, host matrix out, through rk_kr_distances_device on db's device (the tree
 *                           must be on it and have the database's B).  masses NULL: the buffer the last per-sample profile-only call
 *                           (rk_place_batch_masses_samples / _packed_masses_samples, the same S) left on the device in the handle.
 *                           Allocates and frees its workspace; returns when `out` is filled.
 * Added without a bump of RK_VERSION (no struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_KR_CHUNK 2048u
typedef struct rk_tree rk_tree;
int rk_tree_create(int32_t device, uint32_t n_branches, const int32_t *parent, const float *branch_len, rk_tree **out);
int rk_tree_validate(uint32_t n_branches, const int32_t *parent, const float *branch_len);
void rk_tree_destroy(rk_tree *t);
int rk_clade_masses_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint64_t *d_clade, void *stream);
int rk_clade_masses_host(uint32_t n_branches, const int32_t *parent, uint32_t n_samples, const uint64_t *masses, uint64_t *clade);
uint64_t rk_kr_work_bytes(const rk_tree *t, uint32_t n_samples);
int rk_kr_distances_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, double *d_out, void *d_work, uint64_t work_bytes,
                           void *stream);
int rk_kr_distances_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses,
                         double *out, uint32_t n_threads);
int rk_kr_distances_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, double *out);

/* ------------------------------------------------------------------------------------------------------------------
 * Squash clustering of the samples of a sample mass buffer (what `guppy squash` / `gappa` squash compute from jplace files): a
 * hierarchical clustering in which a merged cluster is a new mass distribution, the average of its members, whose KR distances to
 * every other cluster are computed afresh.  The clade profile is linear in the masses, so the profile of an averaged cluster is
 * the average of the profiles.  The reference has no counterpart.  Fixed so that every implementation gives the same bits:
 *   Start               u_s, v_s, h and D exactly as the KR block above defines them.  Sample s is a cluster of size n_s = 1; it is
 *                       active iff T_s != 0.  A sample without mass never takes part: it is only counted.
 *   Step                while two or more clusters are active: take the active pair a < b with the smallest D[a][b]; on equal
 *                       distances the smaller a, then the smaller b.  The comparison is plain < on doubles (no NaN and no -0.0
 *                       occurs among active pairs).
 *   Merge               the cluster keeps slot a, b becomes inactive.  For every node x, in binary64 without contraction:
 *                           u_a(x) = ((double)n_a * u_a(x) + (double)n_b * u_b(x)) / (double)(n_a + n_b)
 *                       and v_a(x) likewise; then n_a += n_b.
 *   New distances       for every other active t, D[a][t] = D[t][a] = the KR pair sum over the new u_a, v_a and u_t, v_t: the same
 *                       terms, the same RK_KR_CHUNK rule and the same order as the KR block.
 *   Output row k        rk_squash_merge {a, b, size, reserved = 0, distance}, 24 bytes: a and b are the smallest sample indices of
 *                       the two clusters (by induction from a < b), size is n_a after the merge, distance is D[a][b] as picked.
 *   Row count           n_merges = max(active - 1, 0).  Rows n_merges .. S - 2 are written as {0xFFFFFFFF, 0xFFFFFFFF, 0, 0, +0.0}.
 *   Monotonicity        the distances need not increase from row to row (an averaged cluster may lie nearer to a third one than
 *                       either member did).  Nothing is clamped.
 *   rk_squash_work_bytes  bytes of the caller-owned device workspace: the KR workspace, D, the merged profile, the row partials, the
 *                         pick scratch, the active flags and the sizes; 0 and a message on a bad argument.
 *   rk_squash_device      d_merges [S - 1] rows and d_n_merges (one uint32_t), written.  Runs the KR matrix, then S - 1 steps of
 *                         plain launches in stream order: no host synchronisation, which pair was picked stays on the device.
 *                         2 <= S <= RK_SQUASH_MAX_SAMPLES (the pick rescans the matrix every step: S^3 beside the S^2 * B of the
 *                         sums).  Otherwise the argument rules of rk_kr_distances_device: RK_ERR_INVALID and a message, nothing
 *                         launched.  Asynchronous on `stream`.
 *   rk_squash_host        the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_squash_batch       the drivers' call, with the contract of rk_kr_distances_batch: masses NULL = the buffer the last per-sample
 *                         profile-only call left in the handle.  merges [S - 1] rows and n_merges on the host; returns when they
 *                         are filled.
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_SQUASH_MAX_SAMPLES 4096u
#define RK_SQUASH_NONE 0xFFFFFFFFu
typedef struct rk_squash_merge {
    uint32_t a, b, size, reserved;
    double distance;
} rk_squash_merge;
uint64_t rk_squash_work_bytes(const rk_tree *t, uint32_t n_samples);
int rk_squash_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, rk_squash_merge *d_merges, uint32_t *d_n_merges, void *d_work,
                     uint64_t work_bytes, void *stream);
int rk_squash_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses,
                   rk_squash_merge *merges, uint32_t *n_merges, uint32_t n_threads);
int rk_squash_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, rk_squash_merge *merges, uint32_t *n_merges);

/* ------------------------------------------------------------------------------------------------------------------
 * Phylogenetic k-means of the samples of a sample mass buffer (what `gappa analyze phylogenetic-kmeans` computes from jplace
 * files): k clusters whose centroids are mass distributions, the averages of their members, with the KR distance between a sample
 * and a centroid.  The method for many samples and a handful of clusters: S * k * B terms a round and no S x S object.  The
 * reference has no counterpart.  Fixed so that every implementation gives the same bits; u_s, v_s, h, T_s, the KR pair sum,
 * RK_KR_CHUNK and the order of the sum are exactly those of the KR block, all binary64 without contraction.
 *   Limits              1 <= S <= 65535, 1 <= k <= RK_KMEANS_MAX_K, 1 <= max_rounds <= RK_KMEANS_MAX_ROUNDS.
 *   Active samples      sample s is active iff T_s != 0; an inactive sample never takes part.  n_active = their number.  Without
 *                       caller seeds k_eff = min(k, n_active); with them k_eff = k.
 *   Seeds               farthest-first when the caller gives none: seed_0 = the smallest active s; for j = 1 .. k_eff - 1, mind[s] =
 *                       the minimum over i < j of the KR pair sum between seed_i's profile and sample s, and seed_j = the active s
 *                       that is not yet a seed with the largest mind[s] under plain >, ties to the smaller s.
 *   Caller's seeds      `seeds`: a host array of k sample indices, read during the call.  An index >= S or a repeated index is
 *                       RK_ERR_INVALID on the host and nothing is launched.  Whether a seed has mass is known on the device only:
 *                       an inactive seed gives status = 1 and every output is written as its filler.
 *   Start               cluster j's centroid profile cu_j = u_{seed_j}, cv_j = v_{seed_j}; the previous assignment of every sample is
 *                       RK_KMEANS_NONE.
 *   Round               1 Distances: for every j < k_eff and active s, Dc[j][s] = the KR pair sum with cu_j, cv_j in the place of the
 *                       first operand's u, v: the same terms, chunk rule and order.  2 Assignment: assign[s] = the j with the
 *                       smallest Dc[j][s] under plain <, ties to the smaller j; changed = the number of active s whose assignment
 *                       differs from the previous one.  3 changed == 0: the run has converged and ends.  Otherwise every cluster
 *                       gets a new centroid and the next round starts.
 *   Update              a cluster with n_j >= 1 members: cu_j(x) = sum / (double)n_j, cv_j(x) likewise from v.  sum adds u_s(x) over
 *                       the members in ascending s with one partial per RK_KMEANS_GROUP sample indices (group = s / 256): a partial
 *                       starts at +0.0 and adds member after member; the partials of the groups that hold a member are added in
 *                       group order, the first one as it is.  A cluster that lost every member keeps its profile.
 *   End                 after the round that found no change, or after max_rounds rounds (the last of those still updates).
 *                       info = {k_eff, n_active, rounds run (the one that found no change included), converged | status << 1}.
 *   Outputs             all written, none added into.  assign [S] uint32_t: RK_KMEANS_NONE for an inactive sample.  dist [S]:
 *                       Dc[assign[s]][s] of the last distance step, +0.0 for an inactive sample.  sizes [k]: the member counts.
 *                       within [k]: the dist of the members added in ascending s from +0.0.  centroids [k][2][B], optional: cu_j then
 *                       cv_j as they stand at the end.  Rows j >= k_eff of sizes, within and centroids are 0 / +0.0.
 *   Fillers             n_active == 0 or status != 0: every assign is RK_KMEANS_NONE, every other output 0 / +0.0, info reports 0
 *                       rounds and converged = 1.
 *   rk_kmeans_work_bytes  bytes of the caller-owned device workspace: the clade sums, the profiles, the centroid profiles, the
 *                         chunk partials [chunks][k][S], the nearest centroid of every sample, the seeding's minima, the active
 *                         flags and the control words; 0 and a message on a bad argument.
 *   rk_kmeans_device      plain launches in stream order: no host synchronisation, no grid-wide wait, no cross-block atomics.
 *                         Whether the run has converged is a word of the workspace: the kernels of the rounds behind it return at
 *                         once.  Every workspace word is written before it is read.  d_centroids may be NULL.  Otherwise the
 *                         argument rules of rk_squash_device: RK_ERR_INVALID and a message, nothing launched, nothing written.
 *                         Asynchronous on `stream`.
 *   rk_kmeans_host        the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_kmeans_batch       the drivers' call, with the contract of rk_squash_batch: masses NULL = the buffer the last per-sample
 *                         profile-only call left in the handle.  The outputs on the host; returns when they are filled.
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_KMEANS_MAX_K 64u
#define RK_KMEANS_MAX_ROUNDS 1024u
#define RK_KMEANS_GROUP 256u
#define RK_KMEANS_NONE 0xFFFFFFFFu
uint64_t rk_kmeans_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t k);
int rk_kmeans_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t k, uint32_t max_rounds, const uint32_t *seeds /* host, may be NULL */,
                     uint32_t *d_assign, double *d_dist, uint32_t *d_sizes, double *d_within, uint32_t *d_info /*[4]*/, double *d_centroids /* may be NULL */,
                     void *d_work, uint64_t work_bytes, void *stream);
int rk_kmeans_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t k,
                   uint32_t max_rounds, const uint32_t *seeds, uint32_t *assign, double *dist, uint32_t *sizes, double *within, uint32_t *info,
                   double *centroids, uint32_t n_threads);
int rk_kmeans_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t k, uint32_t max_rounds, const uint32_t *seeds,
                    uint32_t *assign, double *dist, uint32_t *sizes, double *within, uint32_t *info, double *centroids);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-sample phylogenetic diversity of the samples of a sample mass buffer (what `guppy fpd` computes from jplace files): phylogenetic
 * diversity (PD), balance-weighted PD, quadratic entropy and phylogenetic entropy of every sample, and the one-parameter families
 * of McCoy & Matsen.  The reference has no counterpart.  Fixed so that every implementation gives the same bits; c = c_s(x), m =
 * m_s(x), T = T_s and h[x] are those of the KR block, all binary64 with IEEE conversion, *, +, -, /, no contraction.
 *   Limits              1 <= S <= 65535, 0 <= n_theta <= RK_DIVERSITY_MAX_THETA, every theta finite and in [0, 8].
 *   Half-edges          every node x other than the root gives two half-edges of length h[x]: the proximal half with distal mass
 *                       a = c, the distal half with a = c - m (integers until the one division).  The root contributes nothing
 *                       (h[root] = 0: its terms are zeros).  For a half-edge:
 *                           D = (double)a / (double)T        E = 1.0 - D        M = 2.0 * (E < D ? E : D)
 *   Indicators          tested on the integers ((T - 1) / T rounds to 1.0 once T >= 2^54): rooted = a > 0; split = a > 0 && a < T.
 *                       A term whose indicator is false is +0.0; it is still added, so no control flow changes the order of the sum.
 *   Functions           lg(x) = rk_log2(x), pw(x, theta) = rk_exp2(theta * rk_log2(x)) for x > 0: the project's own binary logarithm
 *                       and exponential (rappas_amd/csrc/rk_divmath.h), written with + - * /, comparisons and integer operations
 *                       on the bits alone -- the platforms' log and pow round differently.  rk_log2 is exact on powers of two
 *                       (rk_log2(1.0) = +0.0, rk_log2(0.5) = -1.0); rk_exp2(+-0.0) = 1.0 exactly, so theta = 0 reproduces the plain
 *                       column.  For x <= 0 -- reachable only for M, where E rounds to 0 -- pw(x, theta) is 1.0 for theta == 0 and
 *                       +0.0 otherwise (the limit).  Accuracy against exact values: profiles/diversity_math_accuracy.txt.
 *   Fixed columns       each the sum of its term over both half-edges of every node:
 *                           0 rooted_pd      rooted ? h : 0
 *                           1 pd             split ? h : 0                       (unrooted PD)
 *                           2 bwpd           split ? h * M : 0                   (guppy's awpd; theta = 1 without a transcendental)
 *                           3 quadratic      split ? h * (D * E) : 0
 *                           4 phylo_entropy  rooted ? h * (-(D * lg(D)) * RK_LN2) : 0,  RK_LN2 = 0x1.62e42fefa39efp-1
 *   Columns per theta   for i < n_theta:  5 + 2i rooted_pd_theta = rooted ? h * pw(D, theta_i) : 0;  6 + 2i bwpd_theta = split ? h *
 *                       pw(M, theta_i) : 0.
 *   Output              [S][RK_DIVERSITY_FIXED + 2 * n_theta] doubles, WRITTEN, not added into.
 *   Order of the sum    a per-sample reduction has no pairs to spread over a device, so the definition carries the parallelism:
 *                       nodes in chunks of RK_KR_CHUNK ids; within a chunk RK_DIVERSITY_LANES = 256 lane partials, lane j starts
 *                       at +0.0 and takes the nodes base + j, base + j + 256, ... in ascending order with acc = (acc +
 *                       term_proximal) + term_distal; the partials are folded by halving, stride 128, 64, ..., 1: p[j] = p[j] +
 *                       p[j + stride]; a column is chunk_0, then + chunk_1, ... in chunk order.
 *   Sample without mass T = 0: its whole row is the quiet NaN 0x7FF8000000000000.
 *   rk_diversity_work_bytes  bytes of the caller-owned device workspace: the clade sums and the chunk partials; 0 and a message on a
 *                            bad argument.
 *   rk_diversity_device      the clade sums, the measure kernel, an in-order reduce over the chunks: plain launches in stream order,
 *                            no atomics, no host synchronisation, no grid-wide wait.  `theta` is a host array, read during the
 *                            call.  A bad theta (NaN, negative, above 8), n_theta above 8 or a NULL theta with n_theta > 0 is
 *                            RK_ERR_INVALID on the host.  Otherwise the argument rules of rk_kmeans_device: RK_ERR_INVALID and a
 *                            message, nothing launched, nothing written.  Asynchronous on `stream`.
 *   rk_diversity_host        the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_diversity_batch       the drivers' call, with the contract of rk_kmeans_batch: masses NULL = the buffer the last per-sample
 *                            profile-only call left in the handle.  The table on the host; returns when it is filled.
 *   rk_diversity_math_host   for tests: out[i] = rk_log2(x[i]) (op 0), rk_exp2(x[i]) (op 1) or pw(x[i], y[i]) (op 2; y is read by
 *                            op 2 only).
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_DIVERSITY_FIXED 5u
#define RK_DIVERSITY_MAX_THETA 8u
#define RK_DIVERSITY_LANES 256u
uint64_t rk_diversity_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t n_theta);
int rk_diversity_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t n_theta, const double *theta /* host */, double *d_out,
                        void *d_work, uint64_t work_bytes, void *stream);
int rk_diversity_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t n_theta,
                      const double *theta, double *out, uint32_t n_threads);
int rk_diversity_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t n_theta, const double *theta, double *out);
int rk_diversity_math_host(uint32_t op /* 0 log2, 1 exp2, 2 pw */, uint64_t n, const double *x, const double *y, double *out);

/* ------------------------------------------------------------------------------------------------------------------
 * Edge principal components of the samples of a sample mass buffer (Matsen & Evans; what `guppy epca` / `gappa edgepca` compute
 * from jplace files): for every edge the difference between the mass on its two sides, per sample, and the principal components of
 * that S x B matrix -- the projections of the samples and the loadings of the edges.  The reference has no counterpart.  Fixed so
 * that every implementation gives the same bits.  All arithmetic is binary64 with IEEE conversion, *, +, -, /, no contraction and
 * no square root on the device: the two roots a caller needs are taken on the host (Finish).
 *   Sums over nodes     the RK_KR_CHUNK rule of the KR block: ascending id, a partial per RK_KR_CHUNK ids that starts at +0.0, the
 *                       partials added in chunk order, the first one as it is.
 *   Sums over samples   the lane rule LS(f): for l = 0..63, p_l = the sequential sum from +0.0 of f(s) over s = l, l + 64, l + 128,
 *                       ... < S; LS = (((+0.0 + p_0) + p_1) + ...) + p_63.  dot(a, b) = LS(s -> a[s] * b[s]): the product is
 *                       rounded, then added.
 *   1 Active samples    u_s(x), v_s(x), T_s as the KR block defines them.  Sample s is active iff T_s != 0; n = the number of active
 *                       samples; k_eff = min(k, n - 1), 0 when n < 2.  k_eff == 0: every output double is +0.0 and nothing below
 *                       applies.
 *   2 Imbalance         for an active s and x != root: X[x][s] = (u_s(x) + v_s(x)) - 1.0 -- the share of the mass strictly below
 *                       the edge minus the share strictly above it; the edge's own mass is left out.  The root, or an inactive s:
 *                       X[x][s] = +0.0.
 *   3 Centring          mean[x] = LS(s -> X[x][s]) / (double)n.  Xc[x][s] = X[x][s] - mean[x] for an active s and x != root,
 *                       otherwise +0.0.
 *   4 Gram matrix       G[s][t] = the chunk-rule sum over x of Xc[x][s] * Xc[x][t], as acc = acc + (a * b).  G is bitwise
 *                       symmetric; rows and columns of inactive samples are +0.0.  trace = LS(s -> G[s][s]).
 *   5 Start vectors     for j < k_eff: Q[j][s] = (double)(((s * 8 + j + 1) * 2654435761) mod 2^32) / 4294967296.0 - 0.5.
 *   6 Iteration         `iters` times: Y[j][s] = LS(t -> G[s][t] * Q[j][t]) for every j < k_eff, and top0_j = the largest
 *                       fabs(Y[j][s]) of the column as this product delivered it.  Then for j = 0 .. k_eff - 1 in order, with
 *                       p = the number of columns before j that were not zero columns (the projections column j has been through),
 *                       but p = 0 throughout the first of the iterations, and scale_j = the largest of top0_j and the top0 of
 *                       those columns before j that were not zero columns:
 *                       let i be the smallest s with the largest fabs(Y[j][s]) (plain >), top that value.  If
 *                       top <= (((double)S * 2^-40) * (double)p) * scale_j -- two exact products, then one rounding; +0.0 for
 *                       p == 0, where it is the test top == 0 --, column j is a zero column: it becomes all +0.0 and is skipped by
 *                       the projections below.  Otherwise Y[j][s] = Y[j][s] / Y[j][i] for every s (the divisor is the value before
 *                       the division: the largest element becomes exactly +1.0, which is also the sign convention); then
 *                       nn = dot(Y[j], Y[j]) and for every l > j: d = dot(Y[j], Y[l]) / nn, Y[l][s] = Y[l][s] - d * Y[j][s].
 *                       Then Q = Y.
 *     The zero rule     A column beyond the rank of G lies, as the product delivers it, in the span of the columns before it, and
 *                       what its projections leave is their rounding.  Dividing that by its largest element would blow it up to
 *                       O(1), still with an O(1) share of the leading vector in it, which the projections on it would put back
 *                       into the later columns: a leading eigenvalue reported twice.  So such a column must be recognised.  Not
 *                       in the first iteration: its columns are G times the start vectors, and two start vectors can differ by a
 *                       constant vector, which G of a centred matrix takes to zero (S = 3, all samples active: columns 0 and 1
 *                       of the first product are the same bits).  A column lost that way must come back, and what the division
 *                       makes of its rounding is a start vector as good as another; the first product of a rank-deficient G
 *                       gets the same treatment and is caught one iteration later (with iters == 1 not at all).  From the second
 *                       iteration on every live column lies in the range of G, orthogonal to the live ones before it, and G is
 *                       one-to-one there: a column that its projections then reduce to rounding is beyond the rank for good, and
 *                       a zero column stays one (G times it is zero).  That also holds for a column whose first product is
 *                       exactly zero although G is not: the start vectors are affine in s between the wraps of the hash, and
 *                       the G of a few interleaved profiles can take such a vector to +0.0 in every entry.  That column is a
 *                       zero column for good and the components sit in the columns that are left, in order.
 *                       The scale: what the division of iteration one makes of a column's rounding lies almost in the null
 *                       space of G, so every later product delivers it tiny -- top0_j about 2^-53 of the leading column's --
 *                       with an O(1) share of the range of G in that little.  Measured against its own top0_j alone it would
 *                       pass for a live column for ever and be reported as a component of about 2^-53 of the leading
 *                       eigenvalue.  Every live column enters the product with its largest entry 1, so top0 of a live column
 *                       is |G q|_max for a q of that size: against the largest of them, a delivered column that small is the
 *                       rounding of the product itself (at most S u sum_t |G[s][t]| an entry), and the same factor covers it.
 *                       The factor, with u = 2^-53, to first order in u: a = Y[j] after its division (|a[s]| <= 1, one entry 1, so
 *                       |a|_2 >= 1 and nn >= 1), b = Y[l] before this projection.  A term of a dot goes through one product and at
 *                       most S - 1 inexact additions of the lane rule (an addition onto +0.0 is exact), so the computed dot(a, b)
 *                       is off by at most S u |a|_2 |b|_2 and nn by S u |a|_2^2; with the division d is off by at most
 *                       (2 S + 1) u |b|_2 / |a|_2, and |d| <= |b|_2 / |a|_2 <= |b|_2.  The two roundings of b[s] - d * a[s] add
 *                       u |d a[s]| + u |b'[s]| <= 2 u |b|_2.  So one projection moves no entry further than (2 S + 3) u |b|_2 from
 *                       the exact projection, and the whole column no further than sqrt(S) times that in length.  An exact
 *                       projection lengthens neither the column nor an error it carries, and |b|_2 <= sqrt(S) top0 at the start.
 *                       After p projections a column whose exact remainder is zero therefore has no entry beyond
 *                       p sqrt(S) (2 S + 3) u sqrt(S) top0 = p S (2 S + 3) u top0 <= p * S * 2^13 u * top0 for every
 *                       S <= RK_EPCA_MAX_SAMPLES (2 * 4096 + 3 rounded to the power of two, so that the factor is exact), and
 *                       top0 <= scale: S * 2^13 * 2^-53 = S * 2^-40 per projection.  A worst case: what was seen on replicate
 *                       samples is a few times S * 2^-53 per projection (tests/test_replicates_host.py prints it), which
 *                       includes what the rounding of G itself adds to such a column.  What the rule costs: a component whose
 *                       eigenvalue is below about p S 2^-40 of the leading one (at most 7 * 4096 * 2^-40 = 2.6e-8, 1e-11 at
 *                       S = 10) is taken for such a column -- in the early iterations, where what the projections leave of
 *                       column j is about eigenvalue_j / eigenvalue_0 of it, or later by its top0 against the scale -- and
 *                       stays zero.  The call claims components down to an eigenvalue ratio of 2^-20 (a share of one in a
 *                       million) and none below.
 *   7 Results           Z[j][s] = LS(t -> G[s][t] * Q[j][t]); nn_j = dot(Q[j], Q[j]); lambda_j = dot(Q[j], Z[j]) / nn_j;
 *                       rr_j = dot(r, r) with r[s] = Z[j][s] - lambda_j * Q[j][s].  A zero column (nn_j == 0) gives nn_j =
 *                       lambda_j = rr_j = +0.0.  w[j][x] = LS(s -> Xc[x][s] * Q[j][s]).
 *   8 Raw output        rk_epca_out_doubles(B, S, k) = 1 + k * (3 + S + B) doubles: trace | lambda[k] | nn[k] | rr[k] | q[k][S] |
 *                       w[k][B]; components j >= k_eff are +0.0.  Two uint32_t: {n_active, k_eff}.
 *   Finish              rk_epca_finish_host, host only, the one place with a square root: eigenvalue_j = lambda_j (the eigenvalue
 *                       of G; divide by n - 1 for the covariance's), share_j = lambda_j / trace, residual_j = sqrt(rr_j / nn_j),
 *                       projection[s][j] = q[j][s] * sqrt(lambda_j / nn_j), loading[x][j] = w[j][x] / sqrt(lambda_j * nn_j) (the
 *                       unit-norm edge eigenvector).  A component with lambda_j <= 0 or nn_j == 0 is all +0.0.
 *   Consequences        The result does not depend on grid, tile or stream.  residual_j is |G q - lambda q| for the unit vector q:
 *                       it tells how far the fixed number of iterations got -- some eigenvalue of G lies within residual_j of
 *                       eigenvalue_j; nothing is iterated "until converged".  Components come out in descending eigenvalue once
 *                       converged; they are not sorted.  They exist only up to the rank of G: hence k_eff, and where the samples
 *                       hold fewer distinct profiles than that (replicates), the zero rule of step 6 -- a component beyond the
 *                       rank is all +0.0, eigenvalue, share and residual included, not a second copy of a leading one.  The q
 *                       entry of an inactive sample is a zero whose sign is that of the divisor of step 6.
 *   rk_epca_out_doubles   the length of the raw output; 0 for arguments out of range.
 *   rk_epca_work_bytes    bytes of the caller-owned device workspace: the clade sums, the profiles (the centred matrix takes the
 *                         place of u), G, its per-chunk partials when the matrix is small, two [k][S] column blocks and the
 *                         active flags; 0 and a message on a bad argument.
 *   rk_epca_device        d_raw [rk_epca_out_doubles] and d_info [2], written.  Clade sums and profiles, then plain launches in
 *                         stream order (two an iteration): no host synchronisation, n_active and k_eff stay on the device.
 *                         2 <= S <= RK_EPCA_MAX_SAMPLES, 1 <= k <= RK_EPCA_MAX_COMPONENTS, 1 <= iters <= 10000.  Otherwise the
 *                         argument rules of rk_kr_distances_device: RK_ERR_INVALID and a message, nothing launched.  Asynchronous
 *                         on `stream`.
 *   rk_epca_host          the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_epca_batch         the drivers' call, with the contract of rk_kr_distances_batch: masses NULL = the buffer the last
 *                         per-sample profile-only call left in the handle.  raw and info on the host; returns when they are filled.
 *   rk_epca_finish_host   eigenvalue[k], share[k], residual[k], projection[S][k], loading[B][k] from a raw output, all written.
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_EPCA_MAX_SAMPLES 4096u
#define RK_EPCA_MAX_COMPONENTS 8u
uint64_t rk_epca_out_doubles(uint32_t n_branches, uint32_t n_samples, uint32_t k);
uint64_t rk_epca_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t k);
int rk_epca_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t k, uint32_t iters, double *d_raw, uint32_t *d_info,
                   void *d_work, uint64_t work_bytes, void *stream);
int rk_epca_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t k,
                 uint32_t iters, double *raw, uint32_t *info, uint32_t n_threads);
int rk_epca_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t k, uint32_t iters, double *raw, uint32_t *info);
int rk_epca_finish_host(uint32_t n_branches, uint32_t n_samples, uint32_t k, const double *raw, double *eigenvalue, double *share,
                        double *residual, double *projection /*[S][k]*/, double *loading /*[B][k]*/);

/* ------------------------------------------------------------------------------------------------------------------
 * Edge dispersion and edge correlation of the samples of a sample mass buffer (what `gappa analyze dispersion` / `gappa analyze
 * correlation` compute from jplace files): for every edge how much its share of the mass and its imbalance vary across the samples,
 * and the Pearson and Spearman correlation of both with every column of sample metadata.  The reference has no counterpart.  Fixed
 * so that every implementation gives the same bits; the tree handle, the sample mass buffer, c_s(x), m_s(x), T_s, u_s(x), v_s(x)
 * are those of the KR block; binary64 with IEEE conversion, /, +, -, *, no contraction; no square root outside the Finish.
 *   Limits              1 <= S <= RK_EDGESTAT_MAX_SAMPLES (an edge's row is ranked inside the LDS of one block; squash and edge PCA
 *                       have the same limit), 0 <= F <= RK_EDGESTAT_MAX_FEATURES metadata columns.
 *   Active samples      sample s is active iff T_s != 0; n = the number of active samples.
 *   Profiles            two quantities per edge x and active sample s:
 *                           q = 0, mass share    P0[x][s] = (double)m_s(x) / (double)T_s
 *                           q = 1, imbalance     P1[x][s] = (u_s(x) + v_s(x)) - 1.0        (step 2 of the edge PCA block)
 *                       P0 is taken from the integers, not from u - v: the difference cancels under a heavy clade, and the ranks
 *                       must not see ties that are not there.  For the root, or an inactive s, both are +0.0; the root's row is
 *                       otherwise computed like any other.  Neither formula gives -0.0.
 *   Metadata            d_meta [F][S] doubles, g_f[s].  Column f is usable iff g_f[s] is finite for every active s -- decided on
 *                       the device, where alone the activity is known.  An unusable column: every raw word of the column is
 *                       written as its filler, the quiet NaN 0x7FF8000000000000 for a double and 0 for an integer, and bit f of
 *                       info[1] is set.  The value of an inactive sample is never used.
 *   Sums over samples   the lane rule LS of the edge PCA block (64 lane partials, each sequential over s = l, l + 64, ..., folded
 *                       in lane order from +0.0); a product is rounded, then added (gram_term).
 *   Moments             per edge x and quantity q, a[s] = Pq[x][s]: mean = LS(s -> a[s]) / (double)n (inactive entries are +0.0);
 *                       c[s] = a[s] - mean for an active s, +0.0 otherwise; ss = LS(s -> c[s] * c[s]).  Per usable column f,
 *                       once: gmean_f, gc_f[s], gss_f likewise from g_f (an inactive entry counts as +0.0).  Per edge:
 *                       cross_{q,f} = LS(s -> c[s] * gc_f[s]).
 *   Ranks, in integers  for an active s: rank2(a)[s] = 2 * #{active t : a[t] < a[s]} + #{active t : a[t] == a[s]} + 1 -- twice the
 *                       1-based mid-rank; t = s counts in the second term.  Plain < and == on the doubles (no NaN occurs among
 *                       active samples; an implementation that sorts bit keys must still treat the values as numbers).
 *                       d[s] = rank2 - (n + 1) for an active s, 0 otherwise: sum d = 0 and |d| <= n - 1.  rss = sum d[s]^2.
 *                       Per usable column gd_f, grss_f likewise from g_f; per edge rcross_{q,f} = sum d[s] * gd_f[s].  All int64,
 *                       exact below 4096^3: no order in it.
 *   Raw output          rk_edgestat_out_words(B, F) = B * (6 + 4F) + 3F eight-byte words, WRITTEN, not added into.  Row x:
 *                           mean0 | ss0 | rss0 | mean1 | ss1 | rss1 | then per f: cross_{0,f} | rcross_{0,f} | cross_{1,f} | rcross_{1,f}
 *                       doubles and int64 as named.  Behind the B rows a row per column f: gmean_f | gss_f | grss_f.
 *                       info [2] uint32_t = {n, the mask of the unusable columns}.  n == 0: every raw word is 0 / +0.0.
 *   Finish              rk_edgestat_finish_host, host only, the one place with a square root.  table [B][8 + 4F] doubles:
 *                           0 mass_mean = mean0   1 mass_var = ss0 / (double)n   2 mass_sd = sqrt(var)   3 mass_cv = sd / mean
 *                           4 mass_vmr = var / mean   5 imb_mean = mean1   6 imb_var = ss1 / (double)n   7 imb_sd = sqrt(var)
 *                       then per f: mass_pearson = cross_{0,f} / sqrt(ss0 * gss_f), mass_spearman = (double)rcross_{0,f} /
 *                       sqrt((double)rss0 * (double)grss_f), imb_pearson, imb_spearman likewise.  feature_table [F][2]: gmean_f,
 *                       gss_f / (double)n.  The variance is the population form (a caller who wants n - 1 rescales).  Nothing is
 *                       clamped and the formulas have no special case: a constant row gives 0 / 0 = NaN, an unusable column is
 *                       NaN.  With n == 0 the raw words are fillers, not sums: both tables are the quiet NaN throughout.  Each
 *                       stated operation is one rounding.
 *   Consequences        The result does not depend on grid, block shape or stream.  Spearman's integer words do not change under a
 *                       strictly increasing transform of a metadata column, nor under one permutation applied to the samples of
 *                       buffer and metadata.  A row strictly increasing with a column has rcross == rss == grss: Spearman is
 *                       exactly 1.0 (strictly decreasing: -1.0).
 *   rk_edgestat_out_words   the length of the raw output; 0 for arguments out of range.
 *   rk_edgestat_work_bytes  bytes of the caller-owned device workspace: the clade sums, P0 and P1 node-major, gc and gd of every
 *                           column and the active flags; 0 and a message on a bad argument.
 *   rk_edgestat_device      d_raw [rk_edgestat_out_words] and d_info [2], written.  Clade sums, profiles, the column prelude and
 *                           the edge kernel: plain launches in stream order, no host synchronisation, no grid-wide wait, no
 *                           cross-block atomics; every workspace word is written before it is read.  A row of at most
 *                           RK_EDGESTAT_COUNT_MAX_SAMPLES samples is ranked by counting, a longer one by a sort in the LDS (the
 *                           same integers).  RK_ERR_INVALID and a message -- nothing launched, nothing written -- for a NULL
 *                           pointer, d_meta == NULL with F > 0, S outside 1..4096, F > 8, a short or misaligned workspace.
 *                           Asynchronous on `stream`; calls on two streams may share a tree handle, each with its own workspace.
 *   rk_edgestat_host        the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_edgestat_batch       the drivers' call, with the contract of rk_epca_batch: masses NULL = the buffer the last per-sample
 *                           profile-only call left in the handle.  `meta` is a host array [F][S]; a value that is not finite is
 *                           RK_ERR_INVALID on the host.  raw and info on the host; returns when they are filled.
 *   rk_edgestat_finish_host table and feature_table (may be NULL when F == 0) from a raw output and its info words, all written.
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_EDGESTAT_MAX_SAMPLES 4096u
#define RK_EDGESTAT_MAX_FEATURES 8u
#define RK_EDGESTAT_COUNT_MAX_SAMPLES 128u
uint64_t rk_edgestat_out_words(uint32_t n_branches, uint32_t n_features);
uint64_t rk_edgestat_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t n_features);
int rk_edgestat_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t n_features, const double *d_meta, uint64_t *d_raw,
                       uint32_t *d_info, void *d_work, uint64_t work_bytes, void *stream);
int rk_edgestat_host(uint32_t n_branches, const int32_t *parent, uint32_t n_samples, const uint64_t *masses, uint32_t n_features, const double *meta,
                     uint64_t *raw, uint32_t *info, uint32_t n_threads);
int rk_edgestat_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t n_features, const double *meta /* host */,
                      uint64_t *raw, uint32_t *info);
int rk_edgestat_finish_host(uint32_t n_branches, uint32_t n_samples, uint32_t n_features, const uint64_t *raw, const uint32_t *info, double *table,
                            double *feature_table);

/* ------------------------------------------------------------------------------------------------------------------
 * EDPL, the expected distance between placement locations of a read (Matsen et al. 2010; what `guppy edpl` / `gappa examine edpl`
 * compute from jplace files): the sum over the pairs of a read's placements of LWR x LWR x the tree path between them -- small for
 * a read whose rows sit on neighbouring edges, large for one whose weight is split between distant clades.  The reference has no
 * counterpart.  A placement sits at the midpoint of its edge, as in the KR block and as the jplace writers put it (distal_length =
 * branch_len / 2, pendant_length = 0).  Fixed so that every implementation gives the same bits: all arithmetic is binary64 with
 * IEEE conversion, *, + and -, no contraction.
 *   Tree quantities     on the tree of rk_tree_create (parent, branch_len, B nodes): D[root] = +0.0; D[x] = D[parent[x]] +
 *                       (double)branch_len[x], one add per node from its parent's value; h[x] as in the KR block; pos[x] = D[x] -
 *                       h[x], the root distance of the midpoint of the edge above x (pos[root] = +0.0).
 *   Distance            between branches a != b, l their lowest common ancestor (which may be a or b):
 *                           l == a (a is an ancestor of b)      d(a, b) = pos[b] - pos[a]
 *                           l == b                              d(a, b) = pos[a] - pos[b]
 *                           otherwise                           d(a, b) = (pos[a] - D[l]) + (pos[b] - D[l])
 *                       d(a, a) = +0.0.  Nothing is clamped.  The ancestor cases are not a special form of the third line: the midpoint
 *                       of a's edge lies above node a, so that line with l = a would be wrong by 2 h[a].  l is unique, so the bits do
 *                       not depend on how it is found.
 *   Read r              K = keep_at_most.  The usable rows are e < min(n_rows[r], K) with branch < B and lwr > 0, in row order (a NaN
 *                       or a weight that is not positive fails the comparison: the row is skipped).  Weights are taken as given, not
 *                       renormalised.  acc starts at +0.0; for i ascending and, inside it, j > i ascending over the usable rows:
 *                       acc = acc + ((w_i * w_j) * d(b_i, b_j)).  edpl[r] = 2.0 * acc: the sum over ordered pairs, as the paper has
 *                       it.  Fewer than two usable rows, an unplaced read included, give +0.0.  score and flags are not read and may
 *                       be NULL.
 *   rk_edpl_device        d_res and d_edpl [n_reads] are device pointers on the tree's device; d_edpl is WRITTEN, not added into.
 *                         Asynchronous on `stream`, allocates nothing and uses no scratch of any handle; the result does not depend on
 *                         grid, stream or how a batch is split into calls.  The query cost does not grow with the depth of the tree.
 *   rk_edpl_host          the same bits in plain C++: no handle, no GPU.  n_threads 0 = automatic, at most 16.
 *   rk_edpl_batch         the drivers' call: a host result set in, host doubles out, in chunks through rk_edpl_device on db's device
 *                         (the tree must be on it and have the database's B).  Uploads only n_rows, branch and lwr; allocates and
 *                         frees its buffers; returns when `edpl` is filled.
 *   rk_tree_distance_host d[i] = d(a[i], b[i]) for n_pairs pairs, for tests and callers; a branch >= B is RK_ERR_INVALID.
 *   rk_edpl_lds_bytes     which form of the kernel a tree gets: the bytes of its distance tables when they are copied into the LDS of
 *                         every block, 0 when they are read from global memory (DESIGN.md 4.12 has the rule).
 *   Errors                with the rules of rk_masses_accumulate_device: RK_ERR_INVALID and a message for a NULL tree, n_rows, branch,
 *                         lwr or output, keep_at_most outside 1..RK_EDPL_MAX_KEEP, n_reads >= 2^32; nothing is launched and no byte
 *                         written.  n_reads == 0 is RK_OK and touches nothing.
 * Added without a bump of RK_VERSION (no existing struct changed).
 * ------------------------------------------------------------------------------------------------------------------ */
#define RK_EDPL_MAX_KEEP 16u
int rk_edpl_device(const rk_tree *t, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, double *d_edpl, void *stream);
int rk_edpl_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t keep_at_most, uint64_t n_reads,
                 const rk_result *res, double *edpl, uint32_t n_threads);
int rk_edpl_batch(rk_db *db, const rk_tree *t, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, double *edpl);
int rk_tree_distance_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_pairs, const uint16_t *a,
                          const uint16_t *b, double *d);
uint64_t rk_edpl_lds_bytes(const rk_tree *t);

/* Optional diagnostics (round 4): the work a batch of packed reads asks of the database, counted by a kernel of its own -- the
 * placement kernels carry no counters.  kmers_probed = sum of sk.getMerCount() (AmbigSequenceKnife.java:191) over the reads the
 * packed kernels place (not BAD_CHAR / TOO_LONG / AMBIGUOUS, at least k symbols); kmers_hit = those with a row in the database
 * (hash.getPairsOfTopPosition2(word) != null, PlacementProcess.java:705-707); entries = (branch, score) pairs of those rows, i.e.
 * iterations of the loop at PlacementProcess.java:719-735.  d_out is device memory (zeroed by the call on `stream`, then filled). */
typedef struct rk_work {
    uint64_t kmers_probed, kmers_hit, entries;
} rk_work;
int rk_count_work_device(rk_db *db, uint64_t n_reads, const uint32_t *d_packed, uint32_t words_per_read, const uint32_t *d_lens,
                         uint32_t fixed_len, const uint32_t *d_flags_in, rk_work *d_out, void *stream);

/* Launch geometry knob (0 = auto): lanes cooperating on one read (8,16,32,64). For tuning/benchmarks. */
int rk_set_lanes_per_read(rk_db *db, uint32_t lanes);
/* Name of the placement kernel variant the next launch will use (for profiles). */
const char *rk_kernel_name(const rk_db *db);

/* ------------------------------------------------------------------------------------------------------------------
 * Phylo-kmer database construction (`-p b` hot loop).
 * Replaces, for one reference tree, the triple loop of src/main_v2/Main_DBBUILD_3.java:648-750 -- for every tested node,
 * for every alignment position pos in [0, L-k+2), a fresh src/core/algos/WordExplorer_v3.java explorer (:98-199: the
 * branch-and-bound recursion with its running float32 sum) started from every state rank -- together with the insertions
 * of src/core/hash/CustomHash_v4_FastUtil81.java:73-89 (addTuple: per (k-mer, original branch) keep the largest PP*).
 * Input is what src/core/PProbasSorted.java:19-25 holds after the ancestral reconstruction has been parsed: per node and
 * site the states ranked by descending posterior, with log10 posteriors.  Output is the CSR form rk_db_create takes
 * (keys ascending, branches ascending inside a row), in host memory owned by the library.  The reference's
 * registered scores depend on the order of exploration (a running float is incremented and decremented); the kernel
 * replays each explorer's statements in order, one lane per (node, pos), so the scores are bit-identical.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct rk_build_desc {
    uint32_t alphabet;            /* RK_ALPHABET_DNA | RK_ALPHABET_AA (word -> key code as for rk_db_desc.key_codes) */
    uint32_t k;                   /* DNA: 2..15, AA: 2..9 (code << 16 | branch must fit 64 bits) */
    uint32_t n_nodes;             /* tested nodes = rows of the posterior table (Main_DBBUILD_3.java:648 nodesTested) */
    uint32_t n_sites;             /* alignment length == PProbasSorted.getSiteCount() */
    uint32_t n_states;            /* PProbasSorted.getStateCount() */
    uint32_t do_gap_jumps;        /* gapJumpsActivated (Main_DBBUILD_3.java:239-258) */
    uint32_t limit_to_1_jump;     /* ArgumentsParser_v2.java:76 (default true) */
    float thr_log10;              /* session.PPStarThresholdAsLog10 */
    const uint8_t *states;        /* [n_nodes][n_sites][n_states] PProbasSorted.states */
    const float *pp_log10;        /* [n_nodes][n_sites][n_states] PProbasSorted.pp, descending along the last axis */
    const uint16_t *node_branch;  /* [n_nodes] original branch id of each tested node (WordExplorer_v3.java:93-94) */
    const uint32_t *gap_off;      /* [n_sites+1] CSR over sites of Alignment.getGapIntervals(); NULL unless do_gap_jumps */
    const int32_t *gap_len;       /* interval lengths */
    int32_t device;               /* HIP device ordinal */
    uint32_t reserved;
} rk_build_desc;

typedef struct rk_built_db {
    uint64_t n_keys, n_entries;
    uint64_t *key_codes;          /* [n_keys] ascending */
    uint64_t *row_offsets;        /* [n_keys+1] */
    uint16_t *branch_ids;         /* [n_entries] ascending inside a row */
    float *scores;                /* [n_entries] */
    uint64_t tuples;              /* addTuple calls ("Tuples explored", Main_DBBUILD_3.java:760) */
    uint64_t visits;              /* exploreWords calls that passed the alignment-limit test */
    double explore_ms, reduce_ms; /* device time of the two stages (HIP events) */
} rk_built_db;

int rk_build_db(const rk_build_desc *desc, rk_built_db *out);
void rk_built_free(rk_built_db *b);

#ifdef __cplusplus
}
#endif
#endif
