/* rufus_hip.h -- C-ABI of librufus_hip.so, the MI355X (gfx950) implementation of the RUFUS
 * k-mer count -> unique-k-mer set difference -> read filter hot path.
 *
 * The reference (jandrewrfarrell/RUFUS) has no FFI: its boundary is a set of executables glued by
 * bash (runRufus.sh:748-759).  The drop-in executables under rufus_amd/csrc/host/ keep that argv /
 * file contract and call the entry points below; each entry point names the reference code whose
 * arithmetic it replaces (paths relative to the reference root, "jf/" = src/modifiedJellyfish/).
 *
 * Conventions: plain C, opaque handles, return 0 on success or a negative RFX_E_* code; the
 * caller owns every host buffer, the library owns device memory unless a function name ends in
 * _dev (caller-provided device pointers).  One rfx_ctx per (process, device); a ctx and the
 * objects made from it must be used from one thread at a time.  There is NO CPU fallback: every
 * device entry point fails with RFX_E_NODEVICE when no gfx950 GPU is visible.
 */
#ifndef RUFUS_HIP_H
#define RUFUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFX_OK 0
#define RFX_E_NODEVICE (-1) /* no usable gfx950 device / HIP runtime error at open */
#define RFX_E_INVAL (-2)    /* bad argument */
#define RFX_E_NOMEM (-3)    /* device or host allocation failed / hbm budget exceeded */
#define RFX_E_FULL (-4)     /* count table cannot grow inside the budget (use a key range pass) */
#define RFX_E_HIP (-5)      /* a HIP call failed; see rfx_last_error() */
#define RFX_E_MIXEDCASE (-6) /* lower-case acgt present: count and filter encodings differ, pack separately */
#define RFX_E_RANGE (-7)    /* output buffer too small */
#define RFX_E_FORMAT (-8)   /* malformed input text / file */

#define RFX_HISTO_BINS 10002 /* jf/sub_commands/histo_main.cc:33-89 with the default low=1 high=10000 inc=1 */

typedef struct rfx_ctx rfx_ctx;
typedef struct rfx_reads rfx_reads;     /* a block of 2-bit packed reads resident in HBM */
typedef struct rfx_table rfx_table;     /* exact k-mer count table in HBM */
typedef struct rfx_records rfx_records; /* (pos,key)-sorted records in HBM == payload of a .Jhash file */
typedef struct rfx_set rfx_set;         /* mutant k-mer set (filter / annotate) */

const char* rfx_version(void);
const char* rfx_strerror(int code);
const char* rfx_last_error(void); /* text of the last HIP failure on this thread */

/* ---------------------------------------------------------------------------------------------
 * Host-only helpers (no device needed)
 * ------------------------------------------------------------------------------------------- */

/* Hash matrix of a 2^lsize-slot jellyfish table for k-mers: 2k columns of lsize bits.
 * Replaces jf/include/jellyfish/large_hash_array.hpp:942-950 (RectangularBinaryMatrix(ceilLog2(size),
 * 2k).randomize_pseudo_inverse()), jf/lib/misc.cc:74-80 (random_bits over the unseeded glibc
 * random()) and jf/lib/rectangular_binary_matrix.cc:138-186,:209-216. */
int rfx_jf_matrix(int lsize, int k, uint64_t* cols);
/* pos = (M * key) & (2^lsize - 1); jf/include/jellyfish/rectangular_binary_matrix.hpp:206-243. */
uint64_t rfx_jf_pos(const uint64_t* cols, int k, int lsize, uint64_t key);

/* Packing.  A read of L bases occupies ceil(L/32) 64-bit code words (base i of the read at bits
 * 2*(i%32) of word i/32, jellyfish codes A0 C1 G2 T3) and as many 32-bit mask words.
 *   RFX_PACK_COUNT : acgt mask bit = base is one of ACGTacgt (jf/include/jellyfish/mer_dna.hpp:46-63);
 *                    codes follow that table (lower case accepted).
 *   RFX_PACK_FILTER: good mask bit = (qual-33 >= min_q as signed char) && base != 'N'
 *                    (src/RUFUS.Filter.cpp:205); codes follow Util::HashToLong (src/Util.cpp:51-84):
 *                    upper-case ACGT only, anything else encodes as A.
 * Both flags together return RFX_E_MIXEDCASE if a lower-case c/g/t is present (the encodings differ).
 * seq/qual are concatenated bytes, off[n_reads+1] their byte offsets (qual shares off; a missing
 * quality byte -- qual == NULL -- reads as '\0', i.e. bad).  Outputs sized by rfx_pack_words();
 * a block holds fewer than 2^32 words. */
#define RFX_PACK_COUNT 1
#define RFX_PACK_FILTER 2
uint64_t rfx_pack_words(const uint64_t* off, uint32_t n_reads);
int rfx_pack_reads(const char* seq, const char* qual, const uint64_t* off, uint32_t n_reads, int min_q, int flags,
                   uint64_t* codes, uint32_t* acgt, uint32_t* good, uint32_t* word_off /* n_reads+1 */,
                   uint32_t* len /* n_reads */);

/* The same packing for reads that lie scattered in a text buffer (FASTQ parsed in place): read i = seq_len[i]
 * bytes at base + seq_start[i], qualities (RFX_PACK_FILTER only) as many bytes at base + qual_start[i] (byte
 * distances modulo 2^64: a span may lie in another allocation than `base`, e.g. a rewritten copy of the read).
 * Single-threaded, so that a caller can pack disjoint ranges of one block from several threads: word_off[0] is
 * an INPUT (first word of this range in the block); word_off[1..n] and len[0..n) are written, codes / acgt / good
 * are indexed by those offsets. */
int rfx_pack_spans(const char* base, const uint64_t* seq_start, const uint32_t* seq_len, const uint64_t* qual_start,
                   uint32_t n_reads, int min_q, int flags, uint64_t* codes, uint32_t* acgt, uint32_t* good,
                   uint32_t* word_off /* n_reads+1 */, uint32_t* len /* n_reads */);

/* RUFUS.Filter hash-list loader (src/RUFUS.Filter.cpp:121-143; single_end: src/RUFUS.Filter.ss.cpp:
 * 100-118): every line contributes HashToLong(kmer) and HashToLong(RevComp(kmer)) (src/Util.cpp:51-84,
 * :187-210), returned here as forward keys in jellyfish encoding (first base most significant).
 * keys_out may be NULL to query the count.  Returns the number of keys (2 per accepted line, not
 * de-duplicated) or a negative code. */
long rfx_hashlist_keys(const char* text, size_t n, int k, int single_end, uint64_t* keys_out, size_t cap);

/* .Jhash header (jf/include/jellyfish/generic_file_header.hpp:96-121, file_header.hpp:33-110):
 * 9-digit length + terse JSON + NUL pad to 8 bytes.  Writes into buf (cap bytes), returns its
 * length or a negative code.  cmdline may be NULL. */
long rfx_jhash_header(int k, int lsize, const uint64_t* cols, int canonical, int counter_len, int argc,
                      const char* const* argv, char* buf, size_t cap);

/* ---------------------------------------------------------------------------------------------
 * Device context
 * ------------------------------------------------------------------------------------------- */
rfx_ctx* rfx_open(int device, size_t hbm_budget_bytes); /* NULL on failure (no CPU fallback) */
void rfx_close(rfx_ctx*);
int rfx_sync(rfx_ctx*);
/* Page-locked host memory for staging buffers of the ingest pipelines (uploads from it run at PCIe speed). */
void* rfx_host_alloc(size_t bytes);
/* The same memory without a call into the HIP runtime: usable as host memory at once -- a tool fills its staging
 * buffers while the device is still being opened on another thread -- and page-locked later, by rfx_host_pin (idempotent;
 * ~1 ms per 320 MB of huge pages), before the first upload from it.  Freed by rfx_host_free. */
void* rfx_host_alloc_lazy(size_t bytes);
int rfx_host_pin(void* p);
void rfx_host_free(void*);
/* Host threads this process can keep busy: hardware threads, cut to its CPU affinity and to the CPU-bandwidth quota
 * of its cgroup (a container given 16 CPUs' worth of time on a 256-thread host runs 64 parser threads three times
 * SLOWER than 16: measured).  The -t / Threads arguments of the drop-in tools are capped by this. */
unsigned rfx_host_cpus(void);
void* rfx_stream(rfx_ctx*); /* the hipStream_t every kernel of this ctx is launched on */
/* Device memory of the ctx: bytes in use now, the high-water mark of that, and bytes of HBM mapped into the ctx's
 * arena (the library sub-allocates one growable virtual range; mapped memory is kept until rfx_close). */
/* The device memory a ctx hands out is mapped into its address range as it is first needed (and kept); mapping costs
 * ~4 ms per GiB.  A caller that knows it will need `bytes` in total -- `jellyfish count` while it still parses its
 * input: the shard passes at finish take ~130 GB for a 30x sample -- has them mapped ahead, off its critical path.
 * Never more than the device can give: a request beyond 90 % of the device's free memory is refused with RFX_E_NOMEM
 * before anything is mapped (nothing is lost and nothing is taken from other users of the device; the memory is mapped
 * when it is needed). */
int rfx_mem_reserve(rfx_ctx*, uint64_t bytes);
int rfx_mem_stats(rfx_ctx*, uint64_t* used, uint64_t* peak, uint64_t* mapped);
/* Device-to-device copy on the ctx stream, then stream sync (hand-off to / from buffers another
 * runtime owns, e.g. the RCCL exchange buffers of the multi-GPU path). */
int rfx_memcpy_dev(rfx_ctx*, void* d_dst, const void* d_src, size_t bytes);

/* Per-kernel HIP-event timing on the ctx stream (used by bench.py for roofline.achieved). */
int rfx_prof_enable(rfx_ctx*, int on);
/* Restrict the brackets to a comma-separated list of kernel names (NULL or "" = every launch): an
 * event pair per launch costs ~10 us of host time, which matters when a step is ~100 launches. */
int rfx_prof_filter(rfx_ctx*, const char* kernel_names);
int rfx_prof_reset(rfx_ctx*);
int rfx_prof_query(rfx_ctx*, const char* kernel, double* total_ms, uint64_t* launches);
int rfx_prof_names(rfx_ctx*, char* buf, size_t cap); /* '\n'-separated kernel names seen so far */

/* ---------------------------------------------------------------------------------------------
 * Read blocks
 * ------------------------------------------------------------------------------------------- */
/* H2D copy of a packed block (arrays as produced by rfx_pack_reads; good/acgt may be NULL when
 * the block will only be counted / only be filtered). */
rfx_reads* rfx_reads_upload(rfx_ctx*, const uint64_t* codes, const uint32_t* acgt, const uint32_t* good,
                            const uint32_t* word_off, const uint32_t* len, uint32_t n_reads);
void rfx_reads_free(rfx_reads*);
uint32_t rfx_reads_count(const rfx_reads*);
uint64_t rfx_reads_bases(const rfx_reads*);
uint64_t rfx_reads_words(const rfx_reads*);
/* Reads of the block that are exactly `len` bases long, for len < 32 (kept with the block since it was made; 0 for len
 * >= 32).  len = 0: the empty sequence lines the paired filter rejects (src/RUFUS.Filter.cpp:203 reads length() - 1). */
uint64_t rfx_reads_of_length(const rfx_reads*, uint32_t len);
/* The block's longest read, in bases (kept with the block since it was made): what rfx_count_add compares with the
 * tiler's switch length (the buffers of jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-178, see below). */
uint32_t rfx_reads_max_len(const rfx_reads*);
/* D2H copy of a block's arrays (sized by rfx_reads_words / rfx_reads_count; any pointer may be NULL). */
int rfx_reads_get(const rfx_reads*, uint64_t* codes, uint32_t* acgt, uint32_t* good, uint32_t* word_off, uint32_t* len);

/* Long sequences as reads.  The reference counts a FASTA of chromosomes or contigs with the loop it counts reads with:
 * the parser hands every sequence out in buffers that overlap by k - 1 bases
 * (jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-251) and the k-mer iterator slides over each
 * (jf/include/jellyfish/mer_iterator.hpp:59-88).  Here every count kernel gives one lane to one read, so a block of long
 * sequences is cut -- on the device -- into TILES of at most tile_len bases that start every step = tile_len - k + 1
 * bases: the k-mer window that starts at base p of a sequence lies in tile p / step and in no other, so the tiled block
 * has exactly the source's windows, invalid bases included (the ACGT mask is carried along).
 *
 * rfx_tile_plan: the plan for one sequence (pure host code).  A sequence of len <= tile_len bases is one tile, unchanged
 * (len < k and len == 0 included); otherwise *n_tiles = ceil((len - k + 1) / step), tile t starts at base t * step and is
 * min(tile_len, len - t * step) bases long (at least k).  RFX_E_INVAL for tile_len < k, k < 1 or k > 32.
 *
 * rfx_reads_tile: a new block (owned by the caller, rfx_reads_free) that holds the tiles of every read of `src`, a dense
 * or a compact count block, in read order: codes, ACGT mask, offsets and lengths as rfx_pack_reads would make them of the
 * tile substrings.  The `good` mask is not carried: a tiled block is for counting.  NULL on failure (rfx_last_error); a
 * source whose tiled form would reach 2^32 tiles or words is refused, the text then starts with "rfx_reads_tile:
 * RFX_E_RANGE".
 *
 * rfx_count_add does this by itself: a block whose longest read exceeds 1024 bases is counted through its tiled twin
 * (tile_len 150), which belongs to the source block -- made at the first add for a given k, kept for the later shard
 * passes and their run maps, replaced by another k's, freed (pending adds settled first) by rfx_reads_free of the source.
 * The run-map calls that name the source (rfx_count_prepare_maps, rfx_count_prefetch_maps, rfx_runmaps_drop) act on the
 * twin.  A twin that cannot be made (no memory, 2^32 tiles) leaves the untiled add: the same counts, slowly.
 * RFX_NO_TILE=1 keeps the untiled route; RFX_TILE_LEN (<= 160) and RFX_TILE_SWITCH move the two lengths.  No knob changes
 * a result. */
int rfx_tile_plan(uint64_t len, int k, uint32_t tile_len, uint64_t* n_tiles, uint32_t* step);
rfx_reads* rfx_reads_tile(rfx_ctx*, const rfx_reads* src, int k, uint32_t tile_len);

/* -------------------------------------------------------------------------------------------
 * Text in, packed reads out -- on the device (kernel K1)
 * Replaces, for strict 4-line FASTQ, the reference's text parser and base packer
 * (jf/include/jellyfish/mer_overlap_sequence_parser.hpp:179-206 -- header, sequence, '+', quality line --;
 * jf/include/jellyfish/mer_dna.hpp:46-63; for the filter's blocks src/Util.cpp:51-84 and the quality test of
 * src/RUFUS.Filter.cpp:205), which the drop-in executables ran on the host until round 6.  The host only moves
 * bytes: it appends RECORD-ALIGNED pieces of the text (every piece begins at a record's '@' line and ends with the
 * newline of a quality line) to a device arena, each piece one host-to-device copy queued on the ctx stream -- from
 * page-locked memory (rfx_host_alloc) it runs at PCIe speed and the call returns at once -- and rfx_text_parse
 * turns what was appended into a read block exactly as rfx_pack_reads(flags, min_q) would have packed the same
 * records (flags = RFX_PACK_COUNT or RFX_PACK_FILTER, one of them).
 *   rfx_text_open    an arena for up to cap_bytes (< 4 GiB) of text; NULL on failure
 *   rfx_text_append  >= 0: a ticket for this piece; < 0: an RFX_E_* code (RFX_E_RANGE: no room).  The host buffer must
 *                    stay as it is until rfx_text_copied(ticket) returns 1 (0: the copy has not run yet; < 0: error),
 *                    rfx_text_wait(ticket) or rfx_text_parse has returned.  The copies run on a stream of the arena's
 *                    own: with two arenas the next block's text crosses PCIe while this block is parsed and counted.
 *                    append / copied / wait may be called from several host threads; parse, fetch, reset and close
 *                    from one, while nobody appends
 *   rfx_text_parse   the block, or NULL: *strict == 0 then says the text is NOT strict 4-line FASTQ (a blank line
 *                    between records, a multi-line record, a quality line of another length, a missing final
 *                    newline ...) -- no error: the caller parses that text on the host (rfx_text_fetch copies it
 *                    back); *strict == 1 with NULL is a failure (rfx_last_error).  Waits for its kernels: when it
 *                    returns the arena is free for the next block's text (rfx_text_reset).
 *   rfx_text_fetch   the appended bytes, copied to `host` (rfx_text_bytes of them)
 * ------------------------------------------------------------------------------------------- */
typedef struct rfx_text rfx_text;
rfx_text* rfx_text_open(rfx_ctx*, uint64_t cap_bytes);
void rfx_text_close(rfx_text*);
uint64_t rfx_text_room(const rfx_text*);
uint64_t rfx_text_bytes(const rfx_text*);
long rfx_text_append(rfx_text*, const void* host, uint64_t n);
int rfx_text_copied(rfx_text*, long ticket);
int rfx_text_wait(rfx_text*, long ticket); /* blocks until that append's bytes have left the host buffer */
rfx_reads* rfx_text_parse(rfx_text*, int flags, int min_q, int* strict);
int rfx_text_fetch(rfx_text*, void* host);
void rfx_text_reset(rfx_text*);

/* -------------------------------------------------------------------------------------------
 * bgzip'd text in: BGZF inflated on the device, straight into the text arena
 * Replaces the host inflater in front of the counter, `zcat F.fastq.gz | ...` (runRufus.sh:157-160, :229-232, :974-977):
 * one host thread there, one wavefront per BGZF block here (k_bgzf_inflate, rufus_amd/csrc/rfx_bgzf.hip; the decoder
 * itself, RFC 1951 / RFC 1952 / the BGZF section of the SAM specification: rufus_amd/csrc/rfx_bgzf_core.h).
 *
 * rfx_bgzf_scan (replaces runRufus.sh:157-160's zcat as the reader of the container; pure host code): walks whole BGZF
 * blocks from buf[0] -- magic 1f 8b 08, FLG = FEXTRA, the `BC` subfield of length 2 wherever it lies among the extra
 * subfields, BSIZE, ISIZE <= 65536 from the footer -- and stops at the first block that is not complete in buf (no
 * error: *consumed says where) or after max_blocks.  *n_blocks, *consumed (bytes), *inflated (sum of ISIZE); any may be
 * NULL.  RFX_E_FORMAT for a header that is not BGZF (plain gzip without `BC` included).  This is the one function that
 * cuts a file into appends.
 *
 * rfx_text_append_bgzf (replaces runRufus.sh:157-160): host[0, n) must be whole BGZF blocks (rfx_bgzf_scan consumes
 * exactly n; else RFX_E_FORMAT) whose inflated total fits rfx_text_room (else RFX_E_RANGE, nothing queued).  The
 * compressed bytes and one descriptor per block go to a staging area the arena owns, on the arena's copy stream; the
 * kernel runs behind them on a second stream of the arena's, so the inflate of one append overlaps the copy of the next.
 * The ticket means what rfx_text_append's means (the host buffer is free when rfx_text_copied / rfx_text_wait say so);
 * rfx_text_bytes counts INFLATED bytes.  Empty blocks (the 28-byte EOF marker) are legal anywhere and add nothing; plain
 * and BGZF appends may be mixed in one arena.  A block that does not inflate (a refusal of rfx_bgzf_core.h, a CRC
 * mismatch) writes nothing outside its own ISIZE bytes and makes rfx_text_settle, rfx_text_parse (NULL, *strict == 1)
 * and rfx_text_fetch fail with RFX_E_FORMAT until the next rfx_text_reset; rfx_last_error() then reads
 * "rfx_bgzf: block <index in this arena>: <reason>".
 *
 * rfx_text_settle (replaces runRufus.sh:157-160: a pipe hands the parser whole lines, BGZF blocks end anywhere): waits
 * for t's appends, finds the end of the last whole group of four lines, shortens t to it and copies the tail, device to
 * device, to the front of `next` (which must be empty: RFX_E_INVAL; too small: RFX_E_RANGE); *carried = the tail's bytes.
 * next == NULL with a tail is RFX_E_FORMAT (a file that ends inside a record).  An arena with fewer than four newlines
 * carries everything.  Called like parse: from one thread, while nobody appends to t or next.
 * ------------------------------------------------------------------------------------------- */
int rfx_bgzf_scan(const void* buf, uint64_t n, uint32_t max_blocks, uint32_t* n_blocks, uint64_t* consumed, uint64_t* inflated);
long rfx_text_append_bgzf(rfx_text*, const void* host, uint64_t n);
int rfx_text_settle(rfx_text* t, rfx_text* next, uint64_t* carried);

/* -------------------------------------------------------------------------------------------
 * Plain-gzip text in: a deflate stream without BGZF's framing, inflated on the device
 * Replaces the host inflater in front of the counter, `zcat F.fastq.gz | ...` (runRufus.sh:157-160, :229-232, :974-977),
 * for the .fastq.gz a sequencer or an archive hands out: gzip members (RFC 1952) of any size with no block index.  The
 * stream is cut speculatively (rufus_amd/csrc/rfx_gzip_core.h, rfx_gzip.hip): k_gz_find looks behind every nominal
 * boundary (RFX_GZIP_CHUNK compressed bytes, a power of two >= 1024) for the first bit offset at which a non-final
 * dynamic block's header checks out; k_gz_walk decodes every chunk from its start to the next chunk's, storing nothing,
 * for its end bit and size; the host confirms the chain (a chunk that ends where the next starts confirms it; a candidate
 * the chunk before runs past is dropped; a gap gets a chunk of its own and a second walk); k_gz_inflate decodes the
 * confirmed chunks into 16-bit values -- a byte, or a reference into the 32 KiB in front of the chunk -- and
 * k_gz_windows / k_gz_resolve turn those into the arena's bytes; k_gz_crc gives each chunk's CRC, combined on the host
 * against the member's trailer.
 *
 * rfx_gzip_open / rfx_gzip_close: the state of ONE compressed stream -- bit offset, member state, running CRC and ISIZE,
 * the stream's last 32 KiB (on the device) -- and the device buffers of the kernels.
 *
 * rfx_text_append_gzip: host[0, n) are the stream's next bytes (eof != 0: its last).  Returns the inflated bytes
 * appended to the arena, or a negative error; *consumed = the whole bytes of host that are done with: the caller presents
 * the rest again, from there, with more behind it.  Only whole confirmed chunks are appended, the longest prefix whose
 * bytes fit rfx_text_room.  A return of 0 with nothing consumed means the arena is full (rfx_gzip_need() != 0: the room
 * the next chunk wants; settle and switch) or that no chunk lies whole in host yet (rfx_gzip_need() == 0: present more).
 * A chunk larger than an empty arena is refused.  A malformed file -- a walk status other than "ok" on a confirmed
 * chunk, a CRC or ISIZE that does not match, a bad or truncated member header or trailer -- is RFX_E_FORMAT, and
 * rfx_last_error() reads "rfx_gzip: member M, chunk C: <reason>" (or "rfx_gzip: member M: <reason>").  Waits for the
 * device: the host needs the walk table.  Called like parse: from one thread, while nobody else appends to the arena.
 *
 * rfx_gzip_stats: out[0 .. 8) = candidates found, chunks confirmed, candidates dropped, chunks inserted, walk rounds,
 * members, batches, bytes out.  rfx_gzip_starts: the confirmed chunks' starts as bit offsets in the whole compressed
 * stream, the first `cap` of them in out (may be NULL); returns how many there are.
 * ------------------------------------------------------------------------------------------- */
typedef struct rfx_gzip rfx_gzip;
rfx_gzip* rfx_gzip_open(rfx_ctx*);
void rfx_gzip_close(rfx_gzip*);
long rfx_text_append_gzip(rfx_text*, rfx_gzip*, const void* host, uint64_t n, int eof, uint64_t* consumed);
int rfx_gzip_stats(const rfx_gzip*, uint64_t out[8]);
uint64_t rfx_gzip_need(const rfx_gzip*);
long rfx_gzip_starts(const rfx_gzip*, uint64_t* out, uint64_t cap);

/* -------------------------------------------------------------------------------------------
 * Two bgzip'd mate files in lock step, and the text of the hit records gathered on the device
 * Replaces the two host inflaters in front of the filter, `RUFUS.Filter HashList <(zcat A) <(zcat B) ...`
 * (runRufus.sh:974-977), and, for text that exists only in HBM, the write loop of src/RUFUS.Filter.cpp after :196-277.
 *
 * rfx_text_records (replaces the `getline` x 4 count of src/RUFUS.Filter.cpp:165-173 as the measure of what an arena
 * holds): waits for t's appends as rfx_text_settle does and reports floor(N / 4) for the arena's N newlines.  Changes
 * nothing.  RFX_E_FORMAT for a BGZF block that did not inflate.
 *
 * rfx_text_settle_records (replaces the lock step of src/RUFUS.Filter.cpp:165-173: record i of file 1 with record i of
 * file 2): rfx_text_settle with the cut behind newline number 4 * min(floor(N / 4), max_records); *records = that
 * minimum.  Two arenas filled from two files hold different numbers of whole records: both are cut at the smaller
 * number.  max_records == 0 carries everything.  Preconditions and error codes are rfx_text_settle's.
 *
 * rfx_text_gather (replaces the output loop of src/RUFUS.Filter.cpp:237-277 on lines the host no longer has): for every
 * set bit r < n_records of hitmask (host memory, ceil(n_records / 64) words; bits at and above n_records are ignored),
 * ascending, the arena's bytes from the beginning of line 4r to the beginning of line 4r + 4, as they are ('\r'
 * included), concatenated, to host_out.  "Four lines per record" is all it asks of the text.  The arena must hold exactly
 * n_records whole records -- 4 * n_records newlines, the last byte a newline -- else RFX_E_INVAL.  *bytes = the bytes the
 * selection has, *n_selected (may be NULL) its records; cap too small: RFX_E_RANGE with *bytes set and nothing written.
 * Works before or after rfx_text_parse on the same arena (it finds the lines itself), until rfx_text_reset.  One wait
 * for the device between the mask upload and the copy of the result.  Called like parse: from one thread, while nobody
 * appends.
 * ------------------------------------------------------------------------------------------- */
int rfx_text_records(rfx_text* t, uint64_t* records);
int rfx_text_settle_records(rfx_text* t, rfx_text* next, uint64_t max_records, uint64_t* records, uint64_t* carried);
int rfx_text_gather(rfx_text* t, const uint64_t* hitmask, uint64_t n_records, void* host_out, uint64_t cap, uint64_t* bytes,
                    uint64_t* n_selected);

/* -------------------------------------------------------------------------------------------
 * bgzip'd FASTA in: the arena cut at a FASTA record, a record's lines joined into one read on the device
 * Replaces `zcat ref.fa.gz | jellyfish count ... /dev/stdin` in front of the -e / -f databases (runRufus.sh:77, :115)
 * and the contig and window counts of scripts/Overlap.shorter.sh:245, :255: the FASTA grammar of
 * jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-251 on text that exists only in HBM.  The rule is
 * rufus_amd/csrc/rfx_fasta_core.h, one source for host and device; the kernels are rufus_amd/csrc/rfx_fasta.hip.  A line
 * ends at '\n' ('\r' stays a base); a line is a header when it is non-empty and begins with '>'; a record is a header and
 * every line up to the next header or the end of the text, its sequence the bytes of those lines without their '\n'.
 *
 * rfx_text_settle_fasta (replaces the pipe of runRufus.sh:77 as what hands the parser whole records; the FASTA twin of
 * rfx_text_settle, with its waits and preconditions): the cut lies at the last line start p > 0 whose byte is '>';
 * t keeps [0, p) and [p, bytes) moves, device to device, to the front of `next` -- the arena's last record is always
 * carried, because nothing says it is whole before the next header or the end of the file.  *carried = the tail's bytes.
 * next == NULL: the file ends here, nothing is carried and a last line without '\n' is a line.  No such p (one record
 * fills the arena): RFX_E_RANGE, rfx_last_error() = "rfx_fasta: one sequence fills the text arena of <bytes> bytes".  A
 * first byte that is not '>': RFX_E_FORMAT.  A block that did not inflate: RFX_E_FORMAT with the "rfx_bgzf:" text.
 *
 * rfx_text_parse_fasta (replaces mer_overlap_sequence_parser.hpp:124-178 and mer_dna.hpp:46-63): the block of the
 * arena's records, in order: codes, ACGT mask, offsets, lengths, read / word / base counts and the longest read are what
 * rfx_pack_reads(RFX_PACK_COUNT) makes of the joined sequences, reads of length 0 (a header directly followed by a
 * header) included, so rfx_count_add tiles a block of chromosomes as it tiles the host route's.  Works the same on text
 * appended without BGZF.  NULL with *fasta == 0: the arena is empty or does not begin with '>' (no error).  NULL with
 * *fasta == 1 is a failure, rfx_last_error() = "rfx_text_parse_fasta: RFX_E_INVAL ..." for flags other than
 * RFX_PACK_COUNT (FASTA has no qualities), "... RFX_E_RANGE ..." for 2^32 reads or words, or the "rfx_bgzf:" text of a
 * block that did not inflate, as rfx_text_parse.  Waits for its kernels, like rfx_text_parse.
 * ------------------------------------------------------------------------------------------- */
int rfx_text_settle_fasta(rfx_text* t, rfx_text* next, uint64_t* carried);
rfx_reads* rfx_text_parse_fasta(rfx_text* t, int flags, int* fasta);

/* -------------------------------------------------------------------------------------------
 * BAM in: the records of a BAM found and their 4-bit sequences packed on the device
 * Replaces the generator of every sample, `samtools view -F 3328 X.bam | PassThroughSamCheck CHR | jellyfish count`
 * (runRufus.sh:599, :639; scripts/RunJellyForRUFUS.sh:28-29).  The container is BGZF: the arena is filled with the
 * unchanged rfx_text_append_bgzf.  The record layout (section 4.2 of the SAM specification) is
 * rufus_amd/csrc/rfx_bam_core.h, one source for host and device; the kernels are rufus_amd/csrc/rfx_bam.hip.
 *
 * rfx_bam_header (replaces samtools view's header read in front of runRufus.sh:599; pure host code, needs no device):
 * buf[0, n) = the first bytes of the compressed file.  Inflates BGZF blocks until the BAM header is whole -- magic
 * BAM\1, l_text, the text, n_ref, and for every reference l_name, name, l_ref -- and reports *n_ref, the references'
 * names (each with its NUL, one behind the other, in names[0, *names_bytes); names may be NULL; names_cap too small:
 * RFX_E_RANGE with *names_bytes set), *first_block = the compressed byte offset of the block that holds the first
 * record's first byte and *skip = that byte's offset inside the block's inflated data (a header that ends with its block:
 * the block behind it, skip 0).  *complete = 0 and RFX_OK when the header is not whole in these bytes -- no error, as
 * rfx_bgzf_scan's incomplete tail: the caller maps more.  RFX_E_FORMAT for bytes that are not BGZF, for BGZF that is
 * not BAM (a bgzip'd FASTQ) and for a block that does not inflate.
 *
 * rfx_bam_settle (replaces the line framing `samtools view | PassThroughSamCheck` gives the reference,
 * scripts/RunJellyForRUFUS.sh:28): the BAM twin of rfx_text_settle, with its preconditions.  Waits for t's appends,
 * finds the chain of records from byte `skip` (rfx_bam_header's for the arena that holds the first record, 0 behind it)
 * -- in parallel and exactly: a guess per tile of 16 KiB, a walk per tile, repair rounds until every tile starts where
 * its predecessor ends -- shortens t to the end of its last whole record and copies the tail, device to device, to the
 * front of `next`.  *n_records = the whole records, *carried = the tail's bytes.  The record starts are kept with the
 * arena until rfx_text_reset.  n_ref = the header's.  next == NULL with a tail: RFX_E_FORMAT (the file ends inside a
 * record); no whole record in an arena no further BGZF block fits into (room < 64 KiB): RFX_E_RANGE; a record on the
 * chain that rfx_bam_core.h's bam_valid refuses: RFX_E_FORMAT, rfx_last_error() = "rfx_bam: record at byte <offset in
 * this arena>: <reason>" for the lowest such record, and nothing is changed; a block that did not inflate: RFX_E_FORMAT
 * with the "rfx_bgzf:" text.  RFX_BAM_TILE (a power of two >= 256) and RFX_BAM_NO_GUESS=1 (no guesses: the whole chain
 * comes from repair) are test knobs that change no result.
 *
 * rfx_bam_parse (replaces src/PassThroughSamCheck.cpp:51-155 and the `-F 3328` of runRufus.sh:599): the records of an
 * arena settled by rfx_bam_settle with (flag & exclude_flags) == 0, in file order, as a dense count block -- exactly what
 * rfx_pack_reads(RFX_PACK_COUNT) makes of the SEQ strings samtools view prints for them ("=ACMGRSVTWYHKDBN"[nibble], high
 * nibble first, `*` for l_seq == 0).  ref_runs[2 i], [2 i + 1] = (first kept index, refID as uint32) wherever a kept
 * record's refID differs from the kept record before it; *n_runs = their number (more than cap: NULL, "RFX_E_RANGE" in the
 * error text, *n_runs set; cap = the arena's records always suffices).  NULL on failure, rfx_last_error() says why.
 *
 * rfx_bam_set_region (replaces the REGION argument of `samtools view -F 3328 X.bam REGION`, what runRufus.sh -R puts into
 * the generators of :599, :639 and :964-967): on an arena settled by rfx_bam_settle (else RFX_E_INVAL), one keep byte per
 * record -- refID == tid, pos < end and pos + rlen > beg (0-based, half open; rlen = the reference bases the CIGAR consumes,
 * 1 for flag 4, no CIGAR or none consumed: rfx_bam_core.h bam_in_region, 64-bit) -- that lives with the arena until
 * rfx_text_reset or the next rfx_bam_settle.  While it is set, "kept" means the flag test AND that byte in rfx_bam_parse
 * and in the five functions of the next section and rfx_bam_locate; without it they are what they were.  *n_in = the
 * records inside the region, before any flag filter.  A second call replaces the first.
 *
 * rfx_bam_region_parse, rfx_bai_query (pure host code, need no device; rufus_amd/csrc/host/rfx_bai.hpp): the region's text
 * -- a reference's name as a whole, else NAME:BEG[-END] cut at the LAST colon, 1-based inclusive, commas dropped -- to
 * (tid, [beg, end)), names as rfx_bam_header gives them; and the ONE range of virtual offsets [start, stop) of a .bai
 * (section 5.2 of the SAM specification) in which every record of the region starts, or *empty.  A superset is exact,
 * because rfx_bam_set_region decides every record.  RFX_E_FORMAT with the reason in why[0, why_cap) for a text or an index
 * that is refused (unknown name, BEG < 1, END < BEG, trailing characters; wrong magic, n_ref that is not the BAM's, counts
 * or offsets beyond the file's bytes, a chunk with beg >= end or beyond bam_size).
 *
 * rfx_bam_stats: of the last rfx_bam_settle on this ctx -- out[0] tiles, out[1] guesses that repair had to change, out[2]
 * repair rounds, out[3] records.  For tests and measurements, like rfx_binned_strike_stats.
 * ------------------------------------------------------------------------------------------- */
int rfx_bam_header(const void* buf, uint64_t n, int* complete, int32_t* n_ref, char* names, uint64_t names_cap,
                   uint64_t* names_bytes, uint64_t* first_block, uint32_t* skip);
int rfx_bam_settle(rfx_text* t, rfx_text* next, uint64_t skip, int32_t n_ref, uint64_t* n_records, uint64_t* carried);
rfx_reads* rfx_bam_parse(rfx_text* t, uint32_t exclude_flags, uint32_t* ref_runs, uint64_t cap, uint64_t* n_runs);
int rfx_bam_set_region(rfx_text* t, int32_t tid, int64_t beg, int64_t end, uint64_t* n_in);
int rfx_bam_region_parse(const char* text, const char* names, uint64_t names_bytes, int32_t* tid, int64_t* beg, int64_t* end,
                         char* why, uint64_t why_cap);
int rfx_bai_query(const void* bai, uint64_t n, int32_t n_ref, uint64_t bam_size, int32_t tid, int64_t beg, int64_t end, int* empty,
                  uint64_t* start, uint64_t* stop, char* why, uint64_t why_cap);
int rfx_bam_stats(const rfx_ctx*, uint64_t out[4]);

/* -------------------------------------------------------------------------------------------
 * BAM in, for the filter: the subject's records scanned as the stranded feeder prints them, and the records of the hit
 * names pulled out of the arena -- on the device
 * Replaces the read pull's generator, `samtools view -F 3328 X.bam | PassThroughSamCheck.stranded CHR STUB.temp |
 * RUFUS.Filter` (runRufus.sh:964-967).  All five work on an arena settled by rfx_bam_settle (else RFX_E_INVAL; the
 * error texts begin with the function's name) and look at the records with (flag & exclude_flags) == 0, the KEPT
 * records, numbered in file order.  Masks are host memory, ceil(n_kept / 64) words, bit i % 64 of word i / 64 = kept
 * record i; input bits at and above n_kept are ignored.  An arena with no kept record and an empty selection are valid.
 * The per-base and per-name rules are rufus_amd/csrc/rfx_bam_core.h's, one source for host and device.
 *
 * rfx_bam_parse_filter (replaces src/PassThroughSamCheck.stranded.cpp:184-281 and the packing in front of
 * src/RUFUS.Filter.cpp:196-277): the kept records as a filter block -- codes, `good`, offsets and lengths byte for byte
 * what the host packer makes, with RFX_PACK_FILTER and min_q, of the SEQ / QUAL strings the stranded feeder prints:
 * SEQ = "=ACMGRSVTWYHKDBN"[nibble], `*` for l_seq == 0; QUAL = 33 + min(q, 93), `*` for l_seq == 0 or qual[0] == 0xFF;
 * a record with flag & 16 reversed and complemented, every base other than A C G T N dropped (the read gets shorter,
 * down to 0 bases), its whole quality string reversed, so that position j of the read meets reversed quality j; a
 * position without a quality character is bad.  No ACGT mask: the block is for the scan.  ref_runs / cap / n_runs and
 * the failures are rfx_bam_parse's, under this function's name.
 *
 * rfx_bam_name_hashes (replaces the QNAME column of runRufus.sh:964's stream as the key the mates are found by): out[j]
 * = the hash of the QNAME -- the name field's bytes up to its first NUL; FNV-1a, then the splitmix64 finaliser -- of
 * the j-th kept record whose mask bit is set (mask == NULL: of every kept record).  n_kept must be the arena's number
 * of kept records (RFX_E_INVAL).  *n = the selected records; more than cap: RFX_E_RANGE with *n set, nothing written.
 *
 * rfx_nameset_build / rfx_nameset_size / rfx_nameset_free (replace the name -> waiting-mate map of
 * src/PassThroughSamCheck.stranded.cpp:225-281 as the thing that finds a hit record's mate): a set of 64-bit hashes in
 * device memory; any values, duplicates count once.  NULL on failure.
 *
 * rfx_bam_mark_names: mask_out bit i = the name hash of kept record i is in the set; *n_kept = the arena's kept records
 * (mask_out must hold ceil(*n_kept / 64) words: the arena's record count always suffices), *n_marked (may be NULL) = the
 * set bits.  A hash collision marks a record too many, never one too few.
 *
 * rfx_bam_gather (replaces the output loop of src/RUFUS.Filter.cpp:237-277 on records the host never saw): for every
 * set bit of mask, ascending, the record's bytes from its block_size field to its end, as they lie, concatenated, to
 * host_out.  *bytes = the bytes of the selection, *n_selected (may be NULL) its records; cap too small: RFX_E_RANGE
 * with *bytes set and nothing written.  One wait for the device between the mask upload and the copy of the result.
 * ------------------------------------------------------------------------------------------- */
typedef struct rfx_nameset rfx_nameset;
rfx_reads* rfx_bam_parse_filter(rfx_text* t, uint32_t exclude_flags, int min_q, uint32_t* ref_runs, uint64_t cap,
                                uint64_t* n_runs);
int rfx_bam_name_hashes(rfx_text* t, uint32_t exclude_flags, const uint64_t* mask, uint64_t n_kept, uint64_t* out, uint64_t cap,
                        uint64_t* n);
rfx_nameset* rfx_nameset_build(rfx_ctx*, const uint64_t* hashes, uint64_t n);
uint64_t rfx_nameset_size(const rfx_nameset*);
void rfx_nameset_free(rfx_nameset*);
int rfx_bam_mark_names(rfx_text* t, uint32_t exclude_flags, const rfx_nameset*, uint64_t* mask_out, uint64_t* n_kept,
                       uint64_t* n_marked);
int rfx_bam_gather(rfx_text* t, uint32_t exclude_flags, const uint64_t* mask, uint64_t n_kept, void* host_out, uint64_t cap,
                   uint64_t* bytes, uint64_t* n_selected);

/* -------------------------------------------------------------------------------------------
 * BAM in, by address: where the kept records lie, and records fetched out of blocks inflated on their own
 * Replaces the repeated inflate of the subject's file: `samtools view` runs over all of X.bam once for the count
 * (scripts/RunJellyForRUFUS.sh:28-29) and again for the read pull (runRufus.sh:964-967).  The count notes every kept
 * record's address; the pull inflates only the blocks that hold the records it wants.
 *
 * rfx_bam_locate: for the kept records of an arena settled by rfx_bam_settle, in file order, start_out[i] = the arena
 * offset of record i's block_size field and bytes_out[i] = 4 + block_size (host memory, n_kept entries each).  n_kept
 * must be the arena's number of kept records (RFX_E_INVAL).
 *
 * rfx_bam_fetch: the arena need NOT be settled: it holds whatever BGZF blocks were appended, in any context, and the call
 * waits for their inflate (a block that did not inflate: RFX_E_FORMAT with the "rfx_bgzf:" text).  start / bytes are host
 * memory, n entries, in any order, duplicates allowed; the bytes [start[i], start[i] + bytes[i]) of the arena go to
 * host_out one behind the other, in list order.  Before anything is copied every entry is checked on the device:
 * bytes[i] >= 36, start[i] + bytes[i] <= rfx_text_bytes(t), and the little-endian word at start[i] (any residue) equals
 * bytes[i] - 4.  One failure: RFX_E_FORMAT, rfx_last_error() = "rfx_bam_fetch: entry <the lowest failing index> ...",
 * nothing written.  *out_bytes = the sum of bytes[]; cap too small: RFX_E_RANGE with *out_bytes set, nothing written.
 * n == 0 is valid.  One wait for the device between the upload of the lists and the copy of the result.
 *
 * rfx_nameset_mark: rfx_bam_mark_names with the hashes from host memory instead of from records: bit i % 64 of
 * mask_out[i / 64] = hashes[i] is in the set (ceil(n / 64) words, the bits at and above n clear), *n_marked (may be
 * NULL) = the set bits.  The hashes cross in pieces of 2^22 (RFX_NAMESET_PIECE, a multiple of 64: a test knob that
 * changes no result), so device memory does not grow with n.
 * ------------------------------------------------------------------------------------------- */
int rfx_bam_locate(rfx_text* t, uint32_t exclude_flags, uint64_t n_kept, uint32_t* start_out, uint32_t* bytes_out);
int rfx_bam_fetch(rfx_text* t, const uint32_t* start, const uint32_t* bytes, uint64_t n, void* host_out, uint64_t cap,
                  uint64_t* out_bytes);
int rfx_nameset_mark(const rfx_nameset*, const uint64_t* hashes, uint64_t n, uint64_t* mask_out, uint64_t* n_marked);

/* -------------------------------------------------------------------------------------------
 * BAM in, for the single-end filter: the hit records of an arena, with their hit counts, in one call
 * Replaces the single-end read pull, `samtools view -F 3328 X.bam | PassThroughSamCheck.stranded.se CHR |
 * RUFUS.Filter.single HashList stdin ...` (runRufus.sh:1031-1032).  Nothing is paired by name there: the feeder prints
 * a record (src/PassThroughSamCheck.stranded.se.cpp:155-203, the same switch as the paired stranded feeder's), the filter
 * counts its windows in the set (src/RUFUS.Filter.ss.cpp:164-193; `i < length()`: the last base IS examined, which is
 * last_base_skipped = 0) and writes the record with ":MH<count>" when the count reaches the threshold (:194-203).  What
 * becomes of a record depends on that record alone, so one pass over the file is exact.
 *
 * rfx_bam_gather_hits: t is an arena settled by rfx_bam_settle, with or without rfx_bam_set_region; block is the filter
 * block rfx_bam_parse_filter made of that arena in that state with the same exclude_flags -- block->n must be the
 * arena's number of kept records (RFX_E_INVAL); the arena, the set and the block must belong to one context
 * (RFX_E_INVAL).  The block is scanned by the filter in its counting mode (every read by itself), and kept record i is
 * SELECTED when (int)count[i] >= thresh; thresh <= 0 selects every kept record, as the reference's `>=` does.  For the
 * selected records, ascending: host_out = their bytes from the block_size field to the record's end, concatenated
 * (rfx_bam_gather's form); hits_out[j] = the count of the j-th selected record; index_out[j] (may be NULL) = its kept
 * index in this arena.  *bytes and *n_selected are set once the sizes are known; *bytes > cap or *n_selected > sel_cap:
 * RFX_E_RANGE with both set and nothing written -- the caller grows its buffers and calls again.  An arena without a kept
 * record and an empty selection are valid.  The error texts begin with the function's name.  Behind the wait that finds
 * the kept records (as in rfx_bam_gather) there are two waits for the device: for the sizes, and for the copies of the
 * result.  Neither the per-read counts nor a mask cross to the host.
 * ------------------------------------------------------------------------------------------- */
int rfx_bam_gather_hits(rfx_text* t, uint32_t exclude_flags, rfx_set* set, const rfx_reads* block, int thresh, int last_base_skipped,
                        void* host_out, uint64_t cap, uint64_t* bytes, uint32_t* hits_out, uint32_t* index_out, uint64_t sel_cap,
                        uint64_t* n_selected);

/* Synthetic trio workload (BASELINE.json configs[1]-[4]) -- benchmark and scale-test input,
 * not a replacement of any reference code.  Every base is a pure function of (parameters, pair, mate, base
 * index) -- see rufus_amd/csrc/rfx_synth.h -- so a 30x WGS sample (6.2e8 reads) is generated straight into
 * packed read blocks in HBM, and any slice of it can be regenerated as text on the host for the oracle. */
typedef struct rfx_synth {
  uint64_t genome_len;  /* bases, 4000 <= genome_len < 2^32 */
  uint64_t genome_seed; /* uniform random genome */
  uint64_t snv_seed;    /* planted SNVs: one per stratum of (genome_len - 2000) / n_snv bases */
  uint64_t read_seed;   /* one per sample */
  uint32_t n_snv;       /* (genome_len - 2000) / n_snv must be >= 2 * read_len + 64 */
  uint32_t read_len;    /* <= 256 */
  uint32_t insert_lo, insert_span; /* insert = insert_lo + U[0, insert_span), insert_lo >= read_len */
  uint32_t err_1024;    /* substitution errors per 1024 bases */
  uint32_t lowq_256;    /* bases with quality '#' (else 'J') per 256 */
  uint32_t n_1024;      /* 'N' per 1024 bases */
  uint32_t carrier;     /* 1: pairs of haplotype 1 carry the SNVs (the child); 0: reference only (a parent) */
} rfx_synth;
/* Reads 2*first_pair .. 2*(first_pair+n_pairs)-1 of the sample (read 2p = mate 1 of pair p, 2p+1 = mate 2),
 * packed as rfx_pack_reads(RFX_PACK_COUNT [| RFX_PACK_FILTER with min_q]) would pack their text. */
/* want_good: bit 0 = also the filter's `good` mask; bit 1 (RFX_SYNTH_COMPACT) = the compact block form -- reads of
 * one length need no offset / length arrays, and the ACGT mask is kept only for the reads that hold an N (a bit per
 * read says which): 43 instead of 68 bytes per 150 bp read resident in HBM.  The kernels read both forms; the
 * global-table count path (k = 32) takes only the dense one.  rfx_reads_get hands out the dense arrays either way. */
#define RFX_SYNTH_GOOD 1
#define RFX_SYNTH_COMPACT 2
rfx_reads* rfx_synth_reads(rfx_ctx*, const rfx_synth*, uint64_t first_pair, uint32_t n_pairs, int min_q,
                           int want_good);
/* Bytes of device memory a read block holds. */
uint64_t rfx_reads_device_bytes(const rfx_reads*);
/* Host twin: the same reads as text, read after read: seq and qual hold 2*n_pairs*read_len bytes each. */
int rfx_synth_text(const rfx_synth*, uint64_t first_pair, uint32_t n_pairs, char* seq, char* qual);
/* SNV i: 0-based genome position, reference and alternative base ('A','C','G','T'). */
int rfx_synth_snv(const rfx_synth*, uint32_t i, uint64_t* pos, char* ref, char* alt);
/* Genome bases [first, first+n) as text (host). */
int rfx_synth_genome(const rfx_synth*, uint64_t first, uint64_t n, char* out);

/* ---------------------------------------------------------------------------------------------
 * K2: canonical k-mer count  (jellyfish count: jf/sub_commands/count_main.cc:148-180;
 * jf/include/jellyfish/mer_iterator.hpp:59-88; hash_counter.hpp:98-119; large_hash_array.hpp:298-302)
 * ------------------------------------------------------------------------------------------- */
/* k <= 31 (32 when canonical).  lsize = ceilLog2 of jellyfish's -s.  Only k-mers whose pos lies in
 * [pos_lo, pos_hi) are counted (pos_hi == 0 means 2^lsize): key-range passes / multi-GPU ownership.
 * capacity_slots == 0 picks an initial size; the table grows by rehash inside the ctx budget. */
rfx_table* rfx_count_begin(rfx_ctx*, int k, int canonical, int lsize, uint64_t capacity_slots, uint64_t pos_lo,
                           uint64_t pos_hi);
/* Three exact implementations sit behind rfx_count_add(); results are identical.
 *  RFX_COUNT_MSP   (23 <= k <= 31) cuts reads into super-k-mers (ALL consecutive k-mers of a read that share their
 *                  minimizer: one record of 12 bytes -- a 64-bit word + a 32-bit plane -- per ~5.7 k-mers at k = 25),
 *                  partitions those, counts every bin in LDS and sorts only the surviving (key,count) pairs into
 *                  (pos,key) order.  Fastest, least HBM.
 *  RFX_COUNT_P2L   (2k <= 62) partitions one 8-byte sortable word per k-mer instance by (pos,key) prefix
 *                  and counts + sorts every bin in LDS.
 *  RFX_COUNT_TABLE inserts into an open-addressed table in HBM (any k, grows by rehash; also what
 *                  rfx_count_add_pairs_dev uses).
 * RFX_COUNT_AUTO (default) takes MSP where it applies, else P2L, and falls back to the table when the
 * transient buffers do not fit the budget.  MSP sizes its buffers optimistically; if the device reports
 * that one did not hold, the affected read block is partitioned again with exact sizes -- at
 * rfx_count_finish, or inside rfx_reads_free if the block is freed first (the redo needs the reads). */
#define RFX_COUNT_AUTO 0
#define RFX_COUNT_TABLE 1
#define RFX_COUNT_P2L 2
#define RFX_COUNT_MSP 3
int rfx_count_set_mode(rfx_table*, int mode);
/* Shard passes (MSP path only, call before the first add): count only the k-mers whose minimizer bin belongs
 * to shard `shard` of `n_shards` (<= 256) -- the same cut as the multi-GPU owner ranges.  The shards of a
 * sample are disjoint and cover it (their records interleave to the full result in (pos,key) order), and
 * the shard of a k-mer is the same for every sample, so count -> set difference can run shard by shard
 * when a sample's records do not fit the HBM at once, or on every GPU over all reads without any exchange. */
int rfx_count_set_shard(rfx_table*, int shard, int n_shards);
/* Shard passes hash every read once per pass: what cuts a read into super-k-mers is the same work whichever shard's
 * runs are kept.  rfx_count_set_early(t, 1) on a table of shard s < S - 1: while a BIG block (>= 2^29 windows) is
 * added, the runs of shard s + 1 are kept too -- the one k_msp_part1 launch covers both shards' bins (and, when those
 * are all the bins, no longer asks whose a run is) -- and partitioned into segments of their own, held aside (at the
 * cost of their memory: 12 bytes per record of shard s + 1) until rfx_count_adopt_early(t_next, t) hands them to the
 * table of shard s + 1 of the same sample; that table is then NOT given those blocks.  Applies only where the boundary
 * between the two shards is a boundary of coarse bins (S = 2, 4, ...; otherwise the add is an ordinary one:
 * rfx_count_early_segments() says how many blocks went early, in the order they were added).  The WGS driver uses it
 * for as many blocks of the subject as the headroom of the device allows (rufus_amd/wgs.py). */
int rfx_count_set_early(rfx_table*, int on);
int rfx_count_early_segments(const rfx_table*);
int rfx_count_adopt_early(rfx_table* next_shard, rfx_table* from);
/* Hash every base ONCE over all shard passes (the reference hashes a k-mer once: jf/sub_commands/count_main.cc:148-180;
 * its spill-and-merge analogue, jf/include/jellyfish/hash_counter.hpp:182-202, does not re-read the input either).  A
 * store of RUN MAPS is shared by the tables of one sample's shard passes (rfx_count_set_runmaps on each, before its
 * adds): the first table that adds a big block (>= 2^29 windows, reads of <= 160 bases, its shard at most half of the
 * bins) also writes the block's map -- 32 bytes per read that say how the read falls into super-k-mers and where
 * their minimizers sit -- and every later table of another shard rebuilds ITS records from reads + map (k_msp_replay)
 * instead of hashing the block again: the same records, bit for bit.  budget_bytes bounds the maps held (0: no bound);
 * a block beyond it is hashed by every pass as before.  rfx_runmaps_drop frees one block's map (after the last
 * pass has added it); the store must be freed before the read blocks it was made from.  rfx_count_set_passes tables
 * make and use a store of their own when the device has room.  rfx_count_replayed: blocks a table added by replay. */
typedef struct rfx_runmaps rfx_runmaps;
rfx_runmaps* rfx_runmaps_create(rfx_ctx*, uint64_t budget_bytes);
/* the same with ONE device allocation of pool_bytes made now, out of which the maps are cut: a store that serves many
 * samples one after the other (the WGS driver) does not leave the device memory in pieces; NULL when it does not fit */
rfx_runmaps* rfx_runmaps_create_pooled(rfx_ctx*, uint64_t pool_bytes);
void rfx_runmaps_free(rfx_runmaps*);
uint64_t rfx_runmaps_bytes(const rfx_runmaps*);
int rfx_runmaps_blocks(const rfx_runmaps*);
int rfx_runmaps_drop(rfx_runmaps*, const rfx_reads*);
int rfx_runmaps_clear(rfx_runmaps*); /* every map of the store */
/* A block's map as it lies in the store, for tests and tools: 32 bytes per read of `reads` to out_bytes (host memory,
 * 32 * the block's reads) and the indices of the reads that went without a map (count 31: more than 27 entries), in no
 * particular order, to out_ovf[0, cap).  Returns their number (>= 0); RFX_E_INVAL when the store holds no map of the
 * block, RFX_E_RANGE (the 32-byte rows are written) when there are more of them than cap.  Waits for the device. */
int rfx_runmaps_read(rfx_runmaps*, const rfx_reads* reads, void* out_bytes, uint32_t* out_ovf, uint32_t cap);
int rfx_count_set_runmaps(rfx_table*, rfx_runmaps*);
/* the maps of several blocks the table is about to add, made with ONE wait for the device (a map made by rfx_count_add
 * waits for its own launch); blocks that have a map, or are no blocks for one, are skipped; no store: nothing happens */
int rfx_count_prepare_maps(rfx_table*, rfx_reads* const* blocks, int n);
/* The same launches queued on the ctx's SECOND stream, no wait: the maps of the sample that is counted next are made
 * beside this sample's partition, refinement and sort (the hashing launch is bound by the instructions it issues, those
 * by the memory; they share a CU).  Pooled store only, as far as it has room; whoever next asks the store about one of
 * these blocks (rfx_count_prepare_maps, rfx_count_add, rfx_runmaps_drop / _clear / _free) waits for the launches first.
 * The blocks must stay alive until then.  Returns the number of launches queued (0: nothing to do or no room), < 0: error. */
int rfx_count_prefetch_maps(rfx_table*, rfx_reads* const* blocks, int n);
uint64_t rfx_count_replayed(const rfx_table*);
/* Bounded-HBM counting of a whole sample (MSP path, call before the first add): rfx_count_add() only
 * REMEMBERS the read blocks -- they must stay alive until finish -- and rfx_count_finish() runs `passes`
 * minimizer-shard passes over them (0: planned from the free HBM, 1 if everything fits): per pass the shard's
 * super-k-mer records of every block are built, counted and freed again, the survivors of all passes are sorted
 * once.  A 30x human sample is 187 GB of records but 42 GB of packed reads: this is how one GPU counts it, the
 * analogue of jellyfish's --disk spill-and-merge (jf/include/jellyfish/hash_counter.hpp:182-202,
 * jf/sub_commands/count_main.cc:326-339).  The table is consumed by its finish. */
int rfx_count_set_passes(rfx_table*, int passes);
int rfx_count_add(rfx_table*, const rfx_reads*);
/* Several devices behind ONE executable (runRufus.sh:776-797 calls binaries, so the N GPUs of a node have
 * to be reachable from `jellyfish count` itself, RUFUS_GPUS=0-7).  N tables, one per device.  Each is given ITS read
 * blocks only -- block b goes to table b mod N: the sample is sharded by read block, a device uploads and hashes 1/N of
 * it.  At finish, pass by pass, every table partitions its blocks; the minimizer bins of a pass are cut into N owner
 * ranges (the cut of rfx_count_set_shard, the same on every device) and table g PULLS the record runs of its range
 * from every table (device-to-device, xGMI) before it counts them: every instance of a canonical k-mer has the same
 * minimizer, so an owner sees complete bins -- exact counts, no partial sums, no reduce (runRufus.sh shards by
 * chromosome on the CPU; here by read block and minimizer owner).  Before the survivors are sorted they change hands
 * once more so that table i ends up with slice i of the OUTPUT POSITIONS: rfx_count_finish of table i returns slice i
 * of the (pos,key)-ordered payload, and the .Jhash is the slices one after the other -- the owner partition of jf's
 * sorted dumper (jf/include/jellyfish/sorted_dumper.hpp:80-112) without a merge.  A table that was given no block
 * still takes part.  (RFX_PEERS_REPLICATE=1 in the environment when the group is created: round 3's fallback -- every
 * table is given EVERY block and keeps minimizer shard i of N; only survivors change hands.)
 *   rfx_ctx_allow_peers   before the first allocation of a ctx: the devices that may read its memory directly
 *   rfx_peers_create(n)   the meeting point of n tables
 *   rfx_count_set_peers   after rfx_count_set_passes, before the first add: this table is number `index` of the group
 * The n rfx_count_finish calls must run concurrently (one host thread each): they meet at barriers (two to agree on the
 * number of passes, two per pass, two for the survivors); if one fails they all fail. */
typedef struct rfx_peers rfx_peers;
int rfx_ctx_allow_peers(rfx_ctx*, const int* devices, int n);
rfx_peers* rfx_peers_create(int n);
void rfx_peers_free(rfx_peers*);
int rfx_count_set_peers(rfx_table*, rfx_peers*, int index);
/* Merge pre-aggregated (key,count) pairs (device pointers): owner-side reduce of the multi-GPU
 * exchange, and the rehash path. */
int rfx_count_add_pairs_dev(rfx_table*, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n);
int rfx_count_stats(rfx_table*, uint64_t* distinct, uint64_t* capacity, uint64_t* max_displacement);

/* Multi-GPU sharding of the MSP path (rufus_amd/dist.py): the super-k-mer records of a read block are
 * grouped by minimizer bin, and every instance of a canonical k-mer lives in the same bin on every
 * rank.  So ranks exchange RECORDS by bin owner (contiguous runs of the record array) and each owner
 * counts complete bins: no partial counts, no reduce.
 *   rfx_count_segments       number of record segments held (one per rfx_count_add), after settling
 *                            any pending capacity check; < 0 on error, 0 if the table is not on the MSP path.
 *   rfx_count_segment_get    device pointers of segment i: records grouped by bin, bin_start[bins+1].
 *                            Valid until the next add/finish/free on the table.
 *   rfx_count_add_records_ext_dev  append a copy of records grouped the same way (bin b = bin_start[b]..
 *                            bin_start[b+1]); `bins` is a power of two >= 256 and the table must be MSP
 *                            capable (23 <= k <= 31).  A record is a 64-bit word AND a 32-bit plane entry
 *                            (rfx_count_segment_ext): both arrays travel.  All segments of a table must come from
 *                            the same k / canonical setting; bins may differ (finish refines to a common count). */
int rfx_count_segments(rfx_table*);
int rfx_count_segment_get(rfx_table*, int i, const uint64_t** d_records, const uint64_t** d_bin_start, uint32_t* bins,
                          uint64_t* n_records);
int rfx_count_add_records_dev(rfx_table*, const uint64_t* d_records, uint64_t n_records, const uint64_t* d_bin_start,
                              uint32_t bins);
/* The same import without the copy: the table reads d_records (and d_ext) where they are until rfx_count_finish /
 * rfx_count_free -- the caller keeps them alive that long; only the bin offsets are copied. */
int rfx_count_adopt_records_dev(rfx_table*, const uint64_t* d_records, const uint32_t* d_ext, uint64_t n_records,
                                const uint64_t* d_bin_start, uint32_t bins);
/* A record is a 64-bit word plus a 32-bit plane entry (the bases of a super-k-mer beyond the 28 the word holds: up to
 * 35 bases at k = 25, 43 at k = 31); the plane is grouped like the words and travels with them.  (Until round 3 only
 * k = 26 .. 31 had a plane; rfx_count_add_records_dev -- words alone -- now always fails.) */
int rfx_count_segment_ext(rfx_table*, int i, const uint32_t** d_ext);
int rfx_count_add_records_ext_dev(rfx_table*, const uint64_t* d_records, const uint32_t* d_ext, uint64_t n_records,
                                  const uint64_t* d_bin_start, uint32_t bins);
void rfx_count_free(rfx_table*);

/* K3: table -> records with lower <= count <= upper in (pos,key) order (jf/include/jellyfish/
 * sorted_dumper.hpp:80-112, mer_heap.hpp:34-38; -L/-U at output count_main.cc:318-324) plus the
 * count-of-counts histogram of exactly those records (histo_main.cc:33-89), histo may be NULL.
 * A table may be finished more than once (different bounds, more reads in between) -- except an MSP table
 * holding more than 4 GB of super-k-mer records: its finish frees them before the survivors are sorted
 * (at WGS scale both do not fit side by side), so it can only be freed afterwards. */
rfx_records* rfx_count_finish(rfx_table*, uint64_t lower, uint64_t upper, uint64_t* histo /* RFX_HISTO_BINS */);
/* The same in two steps, so that several tables can be queued on the device before the host waits for
 * the first: _begin launches the work (nothing is waited for on the MSP path; other paths finish inside
 * _begin), _end waits, returns the records (NULL on error) and frees the handle.  `histo` must stay
 * valid until _end; the table must not be touched in between. */
typedef struct rfx_finish rfx_finish;
rfx_finish* rfx_count_finish_begin(rfx_table*, uint64_t lower, uint64_t upper, uint64_t* histo /* RFX_HISTO_BINS */);
rfx_records* rfx_count_finish_end(rfx_finish*);

/* ---------------------------------------------------------------------------------------------
 * Records (the .Jhash payload; jf/include/jellyfish/binary_dumper.hpp:44-48)
 * ------------------------------------------------------------------------------------------- */
uint64_t rfx_records_size(const rfx_records*);
int rfx_records_k(const rfx_records*);
int rfx_records_lsize(const rfx_records*);
/* Formatted file records (ceil(2k/8) key bytes + counter_len count bytes, saturating) -> host. */
int rfx_records_payload(const rfx_records*, void* out, size_t cap_bytes, int counter_len);
/* The same for records [first, first + n): lets a writer stream a 30 GB payload through a small buffer. */
int rfx_records_payload_range(const rfx_records*, uint64_t first, uint64_t n, void* out, size_t cap_bytes,
                              int counter_len);
int rfx_records_get(const rfx_records*, uint64_t* keys, uint32_t* counts, uint64_t* pos); /* any may be NULL */
/* Load a payload read from a .Jhash file back into HBM (verifies (pos,key) order). */
rfx_records* rfx_records_load(rfx_ctx*, int k, int lsize, const uint64_t* cols, const void* payload, uint64_t n,
                              int counter_len);
/* The same straight from an open .Jhash file: n records at byte `offset` of fd, streamed through a ring of
 * page-locked buffers (several threads pread, the copies and the parsing overlap) -- neither a host copy of the
 * payload nor a device copy of it is ever whole (a 30x sample's file is 35 GB).  The file is only read. */
rfx_records* rfx_records_load_fd(rfx_ctx*, int k, int lsize, const uint64_t* cols, int fd, uint64_t offset, uint64_t n,
                                 int counter_len);
rfx_records* rfx_records_from_dev(rfx_ctx*, int k, int lsize, const uint64_t* cols, const uint64_t* d_keys,
                                  const uint32_t* d_counts, uint64_t n); /* copies; computes pos */
const uint64_t* rfx_records_dev_keys(const rfx_records*);
const uint32_t* rfx_records_dev_counts(const rfx_records*);
const uint64_t* rfx_records_dev_pos(const rfx_records*);
int rfx_records_histo(const rfx_records*, uint64_t* histo /* RFX_HISTO_BINS */);
/* Self-check of a record set where it lies (full-size runs are beyond any CPU oracle): out[0] = records out of the
 * strict (pos,key) order of jf/include/jellyfish/sorted_dumper.hpp:80-112, out[1] = records whose pos is not M * key
 * (jf/include/jellyfish/rectangular_binary_matrix.hpp:206-243), out[2] = counts outside [min_count, max_count],
 * out[3] = sum of the counts.  A correct set gives 0, 0, 0. */
int rfx_records_verify(const rfx_records*, uint32_t min_count, uint32_t max_count, uint64_t out[4]);
/* A checksum of the record MULTISET that does not depend on how the count was cut into shard passes, devices or slices
 * (sums over the slices add up, mod 2^64): out[0] = sum of mix(key) * count, out[1] = sum of mix(key), mix = the
 * splitmix64 finaliser (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) *
 * 0x94D049BB133111EB; x ^ x >> 31).  The full-size runs compare it between S and S + 1 passes (there is no .Jhash of a
 * real jellyfish to hold a 3e9-record table against: same (key, count) pairs from two different cuts of the work is the
 * strongest statement available); the parity tests hold it against the oracle's records. */
int rfx_records_checksum(const rfx_records*, uint64_t out[2]);
void rfx_records_free(rfx_records*);

/* ---------------------------------------------------------------------------------------------
 * K4: set difference
 * ------------------------------------------------------------------------------------------- */
/* RUFUS's modified `jellyfish merge` (jf/jellyfish/merge_files.cc:69-155): keys present in exactly
 * one of the inputs with count >= min_count (5 in the reference), in global (pos,key) order. */
int rfx_merge_unique(rfx_ctx*, const rfx_records* const* files, int n_files, uint32_t min_count, uint64_t* keys_out,
                     uint32_t* counts_out, uint64_t cap, uint64_t* n_out);
/* `jellyfish query` lookups (jf/include/jellyfish/binary_dumper.hpp:156-203): count of each key, 0 if
 * absent.  Keys must already be canonical when the database is. */
int rfx_query(const rfx_records* db, const uint64_t* keys, uint64_t n, uint32_t* counts_out);
/* Fused net semantics of runRufus.sh:925-926 + scripts/CheckJellyHashList.sh:12: subject keys with
 * max(min_count,min_cov) <= count <= max_cov that occur in no other input, in (pos,key) order. */
int rfx_unique_to_subject(rfx_ctx*, const rfx_records* subject, const rfx_records* const* others, int n_others,
                          uint32_t min_count, uint32_t min_cov, uint32_t max_cov, uint64_t* keys_out,
                          uint32_t* counts_out, uint64_t cap, uint64_t* n_out);
/* The same difference one input at a time, device to device: the records of `a` with min_count <= count <=
 * max_count that occur in none of `others`, as a new (pos,key)-ordered record set (NULL on error).  A caller that
 * counts the controls one after the other keeps only the shrinking candidate set of the subject instead of every
 * sample's records: subtract(subject, {}, MinCov, MaxDepth), then subtract(candidates, {control_i}, 0, ~0) per control
 * gives the keys of rfx_unique_to_subject (jf/jellyfish/merge_files.cc:69-155 + scripts/CheckJellyHashList.sh:12). */
rfx_records* rfx_records_subtract(rfx_ctx*, const rfx_records* a, const rfx_records* const* others, int n_others,
                                  uint32_t min_count, uint32_t max_count);

/* The same net semantics (jf/jellyfish/merge_files.cc:69-155 + scripts/CheckJellyHashList.sh:12) WITHOUT the (pos,key)
 * order, for a driver that needs of a sample's count only the histogram, the number of records and the set
 * difference (a trio on one device).  (pos,key) is the order of jellyfish's FILE (sorted_dumper.hpp:80-112); a set
 * difference needs only that both sides are grouped alike, and they are before any sort: every instance of a k-mer has
 * the same minimizer, hence the same fine minimizer bin in every sample, and the leaf leaves its survivors bin after bin.
 *
 * rfx_count_finish_binned stands in for rfx_count_finish (count_main.cc:318-324 -L/-U, histo_main.cc:33-89): the
 * survivors with lower <= count <= upper stay where the leaf staged them, grouped by fine minimizer bin (2^bits bins,
 * rfx_binned_bits: chosen by the table, samples of different depth may differ -- bins are prefixes of one hash, so
 * the coarser side's bin is 2^d whole bins of the other); histo as for rfx_count_finish.  MSP tables that were given
 * their read blocks directly, over all positions, one device; shard passes (rfx_count_set_shard) and run maps as ever.
 * A table of more than 4 GB of records is consumed.  NULL on error. */
typedef struct rfx_binned rfx_binned;
typedef struct rfx_candidates rfx_candidates;
rfx_binned* rfx_count_finish_binned(rfx_table*, uint64_t lower, uint64_t upper, uint64_t* histo /* RFX_HISTO_BINS */);
uint64_t rfx_binned_size(const rfx_binned*); /* number of records */
int rfx_binned_bits(const rfx_binned*);
void rfx_binned_free(rfx_binned*);
/* rfx_records_subtract(subject, {control}, min_count, max_count), bin against bin: the survivors of `subject` with
 * min_count <= count <= max_count that `control` (NULL: nobody) does not hold, as a candidate list.  Both of the same
 * shard and k.  The subject's store is used up (counts of fallen candidates may be overwritten): strike once. */
rfx_candidates* rfx_binned_strike(rfx_ctx*, rfx_binned* subject, const rfx_binned* control, uint32_t min_count,
                                  uint32_t max_count);
/* The route the context's last rfx_binned_strike took: out[0] = its units of work (a unit: a bin of the coarser of the two
 * sides), out[1] = how many of them went through the workgroup-per-unit kernel -- the units beyond the capacities of the
 * wave-per-unit kernel that takes the plain ones, or all of them under RFX_STRIKE_WG=1.  For tests and measurements. */
int rfx_binned_strike_stats(const rfx_ctx*, uint64_t out[2]);
/* The kernel the context's last minimizer-bin count launch (k_msp_leaf) took: out[0] = the k it was compiled for, 0 for
 * the kernel that takes k as an argument, -1 when the context has launched none; out[1] = 1 when it was the single-segment
 * form.  k = 25 and 31 with one segment take the compiled ones unless RFX_LEAF_GENERIC or RFX_LEAF_FORCE_MIXED is set.
 * Host-side bookkeeping, for tests and measurements. */
int rfx_leaf_variant(const rfx_ctx*, int out[2]);
/* The form the context's last k_msp_replay launch (a shard pass's records from reads + run map) took: 0 a lane cuts the
 * runs of its own read (RFX_REPLAY_OLD=1), 1 the per-wave queue with one scattered store per record (RFX_REPLAY_SCATTER=1,
 * or a pass whose bins span more than 64 coarse bins), 2 the per-wave queue with a wave's records sorted by coarse bin in
 * LDS and written in bin order (the default), -1 when the context has launched none.  Both knobs are read at every launch.
 * Host-side bookkeeping, for tests and measurements. */
int rfx_replay_variant(const rfx_ctx*, int* out);
/* rfx_records_subtract(candidates, {control}, 0, ~0) for every further control: its keys are struck off the list */
int rfx_candidates_strike(rfx_candidates*, const rfx_binned* control);
/* entries of the list (struck ones included); _get: all of them, a struck one as ~0 -- canonical keys, no order */
uint64_t rfx_candidates_size(const rfx_candidates*);
int rfx_candidates_get(const rfx_candidates*, uint64_t* keys_out);
/* The subject's count of every entry, in the order of rfx_candidates_get (a struck entry's count is unspecified): the
 * second column of the hash list, `kmer count` (runRufus.sh:925-926, scripts/CheckJellyHashList.sh:12).  The strike
 * notes it when it lists the candidate, so the subject's store may be freed before this is asked. */
int rfx_candidates_get_counts(const rfx_candidates*, uint32_t* counts_out);
/* The exclude databases of runRufus.sh -e (:738-740; merged into the set difference at :925 by jf/jellyfish/
 * merge_files.cc:69-155): every live candidate that the (pos,key)-ordered record set holds is struck off, on the device
 * (pos from the records' own matrix, then rfx_query's search).  The records may come from a count or from a .Jhash
 * (rfx_records_load / _load_fd).  RFX_E_FORMAT when k differs, RFX_E_INVAL for records of another context. */
int rfx_candidates_strike_records(rfx_candidates*, const rfx_records* exclude);
void rfx_candidates_free(rfx_candidates*);
/* A binned store read where it lies; none of these changes it.
 * _get: every survivor in bin order (within a bin: the order the leaf left) -- key, count (count_main.cc:318-324 -L/-U),
 * fine minimizer bin and flat index in the store, chunk * chunk size + offset (entry i of rfx_binned_dev_keys /
 * _dev_counts); any output may be NULL.  *n_out is the number of survivors; RFX_E_RANGE (with *n_out set) when cap is
 * short.  What `jellyfish dump` (jf/include/jellyfish/binary_dumper.hpp:156-203) is to a .Jhash, in no file's order.
 * _checksum: the two sums of rfx_records_checksum over the store -- the shards of a count add up to the sorted route's.
 * _verify: what the strike relies on, a workgroup per bin: out[0] = survivors that do not lie in the bin their own
 * minimizer names, out[1] = counts outside [lower, upper] (count_main.cc:318-324), out[2] = keys that are not
 * canonical (jf/include/jellyfish/mer_dna.hpp canonical(): the smaller of a k-mer and its reverse complement),
 * out[3] = keys a bin holds more than once (each occurrence after the first, per tile of the bin),
 * out[4] = sum of the counts (histo_main.cc:33-89: sum of i * histo[i]).  A correct store gives 0, 0, 0, 0.
 * _query: `jellyfish query` (binary_dumper.hpp:156-203) on the store: the count of each canonical key, 0 if absent. */
int rfx_binned_get(const rfx_binned*, uint64_t* keys_out, uint32_t* counts_out, uint32_t* bins_out, uint64_t* at_out,
                   uint64_t cap, uint64_t* n_out);
int rfx_binned_checksum(const rfx_binned*, uint64_t out[2]);
int rfx_binned_verify(const rfx_binned*, uint64_t lower, uint64_t upper, uint64_t out[5]);
int rfx_binned_query(const rfx_binned*, const uint64_t* canonical_keys, uint64_t n, uint32_t* counts_out);
const uint64_t* rfx_binned_dev_keys(const rfx_binned*);   /* device addresses of the store's keys / counts */
const uint32_t* rfx_binned_dev_counts(const rfx_binned*);

/* ---------------------------------------------------------------------------------------------
 * K5: read filter (src/RUFUS.Filter.cpp:196-277, src/RUFUS.Filter.ss.cpp:164-203)
 * ------------------------------------------------------------------------------------------- */
rfx_set* rfx_set_build(rfx_ctx*, const uint64_t* fwd_keys, uint64_t n, int k); /* keys from rfx_hashlist_keys */
uint64_t rfx_set_size(const rfx_set*);
void rfx_set_free(rfx_set*);
/* Per read: number of good-streak windows found in the set.  last_base_skipped = 1 reproduces the
 * paired tool's `i < length-1` loop bound (src/RUFUS.Filter.cpp:203), 0 the single-end tool.
 * hits_out[n_reads] and hitmask_out[ceil(n_reads/64)] (bit r%64 of word r/64 set when
 * hits >= thresh) are host buffers, either may be NULL; *n_hit_reads counts reads over threshold. */
int rfx_filter(rfx_set*, const rfx_reads*, int thresh, int last_base_skipped, uint32_t* hits_out,
               uint64_t* hitmask_out, uint64_t* n_hit_reads);
/* The blocks of a sample behind ONE wait for the device: hitmask_out[i] (may be NULL, as may the array) and n_hit_reads[i]
 * per block as rfx_filter gives them; no per-read counts. */
int rfx_filter_many(rfx_set*, const rfx_reads* const* blocks, int n, int thresh, int last_base_skipped,
                    uint64_t* const* hitmask_out, uint64_t* n_hit_reads);

/* The pull of the hit reads (the write loop of src/RUFUS.Filter.cpp after :196-277: "a pair is written when either mate
 * reached the threshold"), for reads that live in device blocks: the selected reads become a block of their own.
 *
 * rfx_reads_select: a new block (owned by the caller, rfx_reads_free) with the selected reads of `src` in source order.  It
 * is a DENSE block whether `src` is dense or compact: codes, word_off and len always, `good` if the source has it, the ACGT
 * mask if the source has one (a compact read without a mask entry gets all ones up to its length) -- every array
 * byte-identical to what rfx_pack_reads makes of the selected reads' text, read / word / base counts exact, so the block
 * counts and filters like any other.  Mask bits at or above the read count are ignored.  No read selected or an empty
 * source: a valid block of 0 reads.  The result owns nothing of the source and outlives it.  NULL on refusal, the error text
 * then starts with the function's name and the code: "rfx_reads_select: RFX_E_RANGE" for a selection of 2^32 reads or words
 * or more, RFX_E_INVAL for a bad mode, a NULL mask or a block of another context.
 *
 * rfx_reads_origin: where the reads of a block made by rfx_reads_select / rfx_filter_pull came from: block_out[i] = index
 * of the source block in the call's array (0 for rfx_reads_select), read_out[i] = read index in that block; either may be
 * NULL.  RFX_E_INVAL for a block that was not made by these two.
 *
 * rfx_filter_pull: rfx_filter_many, plus the pulled reads of all n blocks as ONE block (block 0's first); the masks never
 * leave the device unless hitmask_out asks for them.  hitmask_out / n_hit_reads exactly as rfx_filter_many gives them (the
 * per-read bits BEFORE the pair rule).  The ACGT mask is present only if every block has one.  n = 0: a valid empty block.
 * NULL on refusal as above under its own name; a block without `good` is RFX_E_INVAL.  Two waits for the device per call,
 * however many blocks. */
#define RFX_SELECT_READS 0   /* read r is selected when bit r of the mask is set */
#define RFX_SELECT_PAIRS 1   /* reads 2p and 2p+1 are mates (the driver's and rfx_synth_reads' layout): read r is selected
                                when bit r or bit r^1 is set; the last read of a block with an odd read count has no
                                mate and goes by its own bit */
rfx_reads* rfx_reads_select(rfx_ctx*, const rfx_reads* src, const uint64_t* hitmask /* host, ceil(n/64) words */, int mode);
int rfx_reads_origin(const rfx_reads*, uint32_t* block_out, uint32_t* read_out);
rfx_reads* rfx_filter_pull(rfx_set*, const rfx_reads* const* blocks, int n, int thresh, int last_base_skipped, int mode,
                           uint64_t* const* hitmask_out, uint64_t* n_hit_reads);

/* ---------------------------------------------------------------------------------------------
 * N4: coverage model fit (src/ModelDist.cpp; runRufus.sh:849 runs it on every sample's histogram,
 * :862-868 read MutantMinCov and MutantSC from lines 2 and 4 of HISTO.7.7.model)
 * ------------------------------------------------------------------------------------------- */
/* One candidate model: the arguments of testModel / testModelLog (src/ModelDist.cpp:72-74, :200-202). */
typedef struct rfx_model_params {
  double sc, stdev, factor, skew, power;
} rfx_model_params;
/* Residuals of n_cand (<= 64) candidates against one histogram in one pass: what the reference computes by
 * n_cand calls of testModelLog (log_resid = 1: sum of (ln histo[i] - ln model[i])^2, src/ModelDist.cpp:72-198) or
 * testModel (0: sum of (histo[i] - model[i])^2, :200-318) inside its `omp parallel for` (:548-553 and the four
 * loops after it), i running over [inflection, sc * max_copy).  histo[0..n) as the reference indexes it (entry 0
 * unused, entry 1 = the first non-empty row of the file).  RFX_E_INVAL / RFX_E_RANGE where the reference would
 * index outside its tables (sc/2 < 1, fewer than 2 copies, sc * max_copy > n). */
int rfx_model_residuals(rfx_ctx*, const int64_t* histo, uint32_t n, const rfx_model_params* cand, int n_cand,
                        int log_resid, int inflection, int max_copy, double* resid_out);
/* Tables of one model as main() builds them for the output files (src/ModelDist.cpp:716-772; columns are summed
 * from row 0 there): dist[n][*n_cols + 1] row-major (column 0 is zero, column 1 the half-copy curve, column 1 + j
 * the j-copy curve; the last column is not normalised, as in the reference) and rowtot[n] = sum of columns
 * 1..*n_cols - 1 of each row.  *n_cols is set even when dist_cap (in doubles) is too small (RFX_E_RANGE). */
int rfx_model_tables(rfx_ctx*, uint32_t n, const rfx_model_params* model, uint32_t* n_cols, double* dist,
                     size_t dist_cap, double* rowtot);

/* ---------------------------------------------------------------------------------------------
 * K6: overlap scoring of the greedy assemblers; K7: per-base mutant k-mer coverage of contigs
 * ------------------------------------------------------------------------------------------- */
/* Align3 of OverlapSam / Overlap / OverlapRegion (src/OverlapSam.cpp:33-241, src/Overlap.cpp:169-360,
 * src/OverlapRegion.cpp:31-231) for ONE query `a` against `nb` candidates: every offset of the three
 * alignment phases is scored on the device and reduced in the reference's loop order (first offset
 * with the strictly greatest accepted score).  Per candidate j, out[5j..5j+4] =
 *   { phase-1 best score, its overlap, perfect flag (score == window),
 *     best score over all three phases (== phase 1 when perfect), its overlap };
 * a score equal to RFX_OVL_NONE_* (the variant's initial LocalBestScore) means "nothing accepted".
 * The caller applies the reference's cross-candidate rules (shared PerfectMatch, first-best wins).
 * variant: RFX_OVL_SAM / RFX_OVL_REGION (LocalBestScore starts at 0, '>=' in every phase) or
 * RFX_OVL_CONTIG (Overlap.cpp: starts at -1, phase 3 accepts with a strict '>'). */
#define RFX_OVL_SAM 0
#define RFX_OVL_CONTIG 1
#define RFX_OVL_REGION 2
int rfx_overlap_score(rfx_ctx*, const char* a, int alen, const char* const* b, const int* blen, int nb, float min_pct,
                      int min_ovl, int variant, int* out /* nb x 5 */);
/* The same scoring against a DEVICE-RESIDENT pool of sequences: the assemblers' outer loops are sequential (read i
 * merges into its best partner, which is seen later: src/OverlapSam.cpp:866-1024, src/Overlap.cpp:935-1126,
 * src/OverlapRegion.cpp:702-841), so one scoring call per read is unavoidable -- but not uploading the candidates
 * again for every call (OverlapRegion scores read i against ALL later reads).  The pool is uploaded once,
 * rfx_ovl_pool_set() patches the one entry a merge changes, a score call moves only the candidate indices and the
 * results, with no allocation.  query: a pool entry, or an explicit string (a_explicit != NULL).  strands: 0 = the
 * query as it is, 1 = its reverse complement (built on the device: the query must consist of ACGTN only, as
 * Util::RevComp drops other characters), 2 = both in one launch: out holds nb x 5 for the forward strand, then
 * nb x 5 for the reverse complement. */
typedef struct rfx_ovl_pool rfx_ovl_pool;
rfx_ovl_pool* rfx_ovl_pool_create(rfx_ctx*, const char* const* seqs, const int* lens, int n);
int rfx_ovl_pool_set(rfx_ovl_pool*, int idx, const char* seq, int len);
int rfx_ovl_pool_score(rfx_ovl_pool*, int query, const char* a_explicit, int a_len, const int* cand, int nb,
                       float min_pct, int min_ovl, int variant, int strands, int* out);
void rfx_ovl_pool_free(rfx_ovl_pool*);
/* AnnotateOverlap (src/AnnotateOverlap.cpp:88-134): for each packed contig of the block (good mask =
 * base != 'N' && qual-33 >= 3, i.e. RFX_PACK_FILTER with min_q 3) the number of mutant windows that
 * cover every base; cov_out holds rfx_reads_bases() counters, contig after contig. */
int rfx_annotate(rfx_set*, const rfx_reads*, uint32_t* cov_out);

#ifdef __cplusplus
}
#endif
#endif /* RUFUS_HIP_H */
