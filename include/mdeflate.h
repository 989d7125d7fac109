/* mdeflate.h — C ABI of the MI355X-native many-stream DEFLATE engine.
 *
 * This is the drop-in boundary for the hot path of mirage/decompress
 * (lib/de.ml, lib/zl.ml).  The reference has no FFI for this path (its old
 * ctypes reverse binding was removed in v1.5.3, CHANGES.md:21-26), so the
 * boundary is the OCaml module signature; each entry point below names the
 * signature it stands behind.  An OCaml stub layer keeps
 * `De.Inf.Ns.inflate`, `Zl.Inf.Ns.inflate`, `De.Higher.*`, `Zl.Higher.*`
 * unchanged on top of these calls.
 *
 * Conventions:
 *  - caller owns every buffer; the engine never allocates caller-visible memory;
 *  - errors are integer status codes, 1:1 with the reference's variants,
 *    never exceptions / aborts;
 *  - a context (md_ctx) is single-owner, distinct contexts are independent
 *    and thread-safe with respect to each other (one context per GPU);
 *  - all sizes/offsets are bytes; descriptor arrays are structure-of-arrays.
 *  - there is NO CPU fallback: every compute entry point runs HIP kernels and
 *    returns MD_E_NO_DEVICE when no gfx950 device is usable.
 *  - limits per stream (the kernels keep 32-bit cursors): inflate reads at most
 *    MD_MAX_INFLATE_IN (512 MiB - 16: bit positions are 32-bit) of compressed input and writes at most
 *    MD_MAX_STREAM (4 GiB - 16); deflate / LZO read and write at most MD_MAX_STREAM.  The host-pointer
 *    entry points reject larger descriptors with MD_E_INVALID_ARGUMENT; with device descriptors the
 *    stream's status[i] is MD_E_INVALID_ARGUMENT and nothing is read or written for it.
 *    A batch holds at most 2^31 - 1 streams.
 */
#ifndef MDEFLATE_H
#define MDEFLATE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MD_VERSION 0x000300 /* 0.3.0 */
#define MD_MAX_INFLATE_IN 0x1ffffff0ull
#define MD_MAX_STREAM 0xfffffff0ull

/* Per-stream status: De.Inf.Ns.error (lib/de.ml:1548-1566, lib/de.mli:150-157)
 * + Zl.Inf.Ns.error (lib/zl.ml:383).  Strings: md_status_string(). */
enum {
  MD_OK = 0,
  MD_UNEXPECTED_END_OF_INPUT = 1,
  MD_UNEXPECTED_END_OF_OUTPUT = 2,
  MD_INVALID_KIND_OF_BLOCK = 3,
  MD_INVALID_DICTIONARY = 4,
  MD_INVALID_COMPLEMENT_OF_LENGTH = 5,
  MD_INVALID_DISTANCE = 6,
  MD_INVALID_DISTANCE_CODE = 7,
  MD_INVALID_HEADER = 8,   /* Zl: "Invalid Zlib header", lib/zl.ml:183 */
  MD_INVALID_CHECKSUM = 9, /* Zl: "Invalid checksum", lib/zl.ml:179-181; Gz: lib/gz.ml:287-289 */
  /* Gz.Inf's `Malformed strings, lib/gz.ml:284-296 */
  MD_INVALID_GZIP_HEADER = 10,          /* "Invalid GZip header" */
  MD_INVALID_GZIP_HEADER_CHECKSUM = 11, /* "Invalid GZip header checksum" */
  MD_INVALID_SIZE = 12,                 /* "Invalid input size (expect:.., inflated:..)" */
  /* deflate: the reference raises exception De.Queue.Full (lib/de.ml:2211-2217) — only the CLI
   * driver can, when its unconditional end-of-block push (bin/decompress.ml:67) meets a full queue */
  MD_QUEUE_FULL = 13,
  /* Lzo.error, lib/lzo.ml:4-12 (LZO entry points below) */
  MD_LZO_INVALID_INPUT = 14, /* `Malformed "Invalid input" (count, lib/lzo.ml:236) */
  MD_LZO_NO_DICTIONARY = 15, /* `Malformed "No dictionary at offset 0 available" (lib/lzo.ml:376) */
  MD_LZO_OUT_OF_BOUND = 16,  /* `Invalid_argument "Input is malformed or output is not large enough"
                              * (lib/lzo.ml:401-402); compress: "lzo: output is not large enough" (:655) */
  MD_LZO_MALFORMED_INPUT = 17, /* `Malformed "Malformed input" (Lzo.uncompress_with_buffer, lib/lzo.ml:414) */
  /* ZIP archives (md_zip_* below; PKWARE APPNOTE) */
  MD_INVALID_ZIP_DIRECTORY = 18, /* "Invalid ZIP directory": end record(s) or central directory */
  MD_INVALID_ZIP_HEADER = 19,    /* "Invalid ZIP local header": an entry's local header or where its body lies */
  MD_ZIP_UNSUPPORTED = 20,       /* "Unsupported ZIP entry": encrypted, or a method other than 0 and 8 */
  /* the index of a long stream (md_inflate_index_* below) and of a blocked GZip file (md_bgzf_index_*) */
  MD_INVALID_INDEX = 21,         /* "Invalid index": a serialised index that breaks a rule of its layout, an index used with
                                  * another src than it was built from, a piece that does not end on the next point; a file
                                  * without BC size fields, a virtual offset or a member that is not as the index says;
                                  * a pack .idx that breaks a rule of its layout or belongs to another pack */
  /* git packfiles (md_pack_* below) */
  MD_INVALID_PACK = 22,      /* "Invalid pack": the pack's magic, an object's header, an OFS_DELTA offset, a REF_DELTA cycle */
  MD_INVALID_DELTA = 23,     /* "Invalid delta": a delta's instructions or sizes */
  MD_INVALID_PACK_BASE = 24, /* "Invalid delta base": the object is a delta and an object of its chain of bases failed */
  MD_PACK_MISSING_BASE = 25, /* "Missing delta base": a REF_DELTA names an object the pack does not hold (a thin pack) */
  MD_PACK_UNSUPPORTED = 26,  /* "Unsupported pack": a pack version other than 2 and 3, an idx version other than 2 */
  /* the object graph of a pack (md_pack_graph_* below): a status of md_pack_graph_status alone - no call returns it and
   * md_status_string does not name it */
  MD_INVALID_OBJECT = 27     /* "Invalid object": a commit, tree or tag whose links cannot be read */
};

/* Call-level errors (negative): misuse raises Invalid_argument in the
 * reference (lib/de.ml:146-147); here the call returns one of these. */
enum {
  MD_E_INVALID_ARGUMENT = -1,
  MD_E_NO_DEVICE = -2,
  MD_E_HIP = -3,
  MD_E_OUT_OF_MEMORY = -4
};

/* Container formats */
enum {
  MD_FORMAT_DEFLATE = 0, /* raw RFC1951: De.Inf.Ns.inflate, lib/de.ml:1807-1822 */
  MD_FORMAT_ZLIB = 1,    /* RFC1950: Zl.Inf.Ns.inflate, lib/zl.ml:400-417 */
  MD_FORMAT_GZIP = 2     /* RFC1952 as lib/gz.ml reads and writes it: Gz.Inf (lib/gz.ml:248-633),
                          * Gz.Def (lib/gz.ml:636-918).  Inflate: checksum[i] = CRC-32 of the output;
                          * the body follows De.Inf.Ns status semantics.  Deflate: header from
                          * md_deflate_params.gz_header, body = the Zl driver's with dynamic blocks (Gz.Def's
                          * make_block, lib/gz.ml:724-729), CRC-32 + ISIZE trailer; `driver` and
                          * `dynamic` are ignored, checksum[i] = CRC-32 of the input. */
};

/* The reference's three encoder drivers: they decide WHEN a new block is sent, hence the
 * block structure of the stream. */
enum {
  MD_DRIVER_ZL = 0,     /* Zl.Def.encode / Zl.Higher.compress, lib/zl.ml:509-555 */
  MD_DRIVER_HIGHER = 1, /* De.Higher.compress / to_string, lib/de.ml:4518-4553 (always level 4) */
  MD_DRIVER_CLI = 2     /* bin/decompress.ml:47-75 (Dynamic per fill, Fixed last block) */
};

/* The reference's two match finders (same queue / histograms / drivers around them). */
enum {
  MD_MATCHER_DE = 0, /* De.Lz77, lib/de.ml:4013-4515: 4-byte multiplicative hash (default) */
  MD_MATCHER_LZ = 1  /* Lz (decompress.lz), lib/lz.ml:136-573: zlib's 3-byte rolling hash, levels 0..4 = 4,
                      * no copy mode, `End without an end-of-block command (the driver pushes it) */
};

typedef struct md_ctx md_ctx;

int md_version(void);
/* human strings of lib/de.ml:1557-1567 ("Unexpected end of input", ...) */
const char *md_status_string(int status);
/* last call-level error text of this context (HIP error string etc.) */
const char *md_last_error_string(const md_ctx *ctx);

/* Number of usable gfx950 devices (0 when none / no driver). */
int md_device_count(void);

/* Multi-GPU: streams are independent, so a batch shards with no data-path exchange - one context
 * (md_create(device)), one host thread and one HIP stream per device, every device given a contiguous range of the
 * stream index.  md_shard_plan cuts a batch of n streams into `world` such ranges balanced by the sum of `lengths`
 * (normally the uncompressed sizes): rank r owns streams [lo[r], hi[r]); the ranges are contiguous, cover 0..n and may
 * be empty.  Pure host arithmetic (no device is touched), the same cut as decompress_amd.shard.shard_by_bytes.
 * Returns MD_OK, or MD_E_INVALID_ARGUMENT (world < 1, a null pointer with n or world != 0). */
int md_shard_plan(uint64_t n, const uint64_t *lengths, int world, uint64_t *lo, uint64_t *hi);

/* One context per GPU.  `hip_stream`:
 *   NULL            the context creates its own non-blocking stream (not ordered with any other stream:
 *                   the caller synchronises, e.g. md_synchronize, before touching the buffers elsewhere);
 *   MD_STREAM_NULL  the device's legacy default stream (hipStream_t 0): ordered with everything the caller
 *                   enqueues there;
 *   otherwise       an existing hipStream_t to enqueue on (e.g. the caller's current stream).
 * Every entry point sets the context's device for the call and restores the caller's current device.
 * Replaces nothing in the reference: state objects there are the window/queue bigarrays the caller
 * allocates (lib/de.mli:93-106); here they are LDS buffers owned by the kernels. */
#define MD_STREAM_NULL ((void *)(intptr_t)-1)
md_ctx *md_create(int device, void *hip_stream);
void md_destroy(md_ctx *ctx);
int md_synchronize(md_ctx *ctx);

/* Timing of the dominant kernel with HIP events recorded on the context's
 * stream: begin/end bracket any number of batch calls; end returns elapsed
 * milliseconds (synchronises). */
/* Options of a context.  Keys:
 *   "deflate_workspace_cap_mib"  value >= 0 (default: a sixth of the device's memory, 48 GiB on MI355X; 0 = none).  The
 *                                deflate kernels keep a per-position workspace of 13 bytes per input byte of what one
 *                                launch covers; a md_deflate_batch_device call whose workspace would be larger than the
 *                                cap goes through the kernels in slices of positions - a multiple of 32 KiB of every
 *                                stream per launch, going on from the state the launch before left - and in groups of
 *                                streams if 64 KiB of every stream at once would still be too much.  Same bytes out
 *                                (every fill of the reference's window ends on a 32 KiB boundary).  Batches of
 *                                more than four times 4 096 streams go in groups of streams first (no extra work).
 *                                4 096 x 1 MiB: 52 GiB and 114.7 ms whole; 27.8 GiB (2 slices) 116.3 ms at the default;
 *                                14.8 GiB (4 slices) 119.1 ms at 16 GiB; 6.7 GiB 127 ms at 8 GiB.  32 768 corpus files
 *                                (7.1 GB, 93 GB whole): 573 ms whole, 576 ms at the default (two groups), 656 ms at
 *                                29 GiB (two groups, each in slices: a slice lasts as long as its slowest stream).
 *                                A capped call reads lengths and results back between the launches, i.e. it
 *                                synchronises with the context's stream instead of only enqueueing.
 *   "encoder_piece_bytes"        value >= 1 (default 1 MiB): how much input a md_def_* encoder gathers before it launches
 *                                the kernels on it.  The bytes out are those of the reference handed the input in the
 *                                same pieces (which are, but for corner cases at the very end of a stream, the same for
 *                                any pieces).
 *   "release_workspace"          (value ignored) waits for the context's stream and frees its grow-only device scratch
 *                                (deflate workspaces, launch orders, decoder-piece buffers, the host entry points' device copies); it grows again on demand.
 *   "host_pipeline_slices"       1 .. 64 (default 16): most slices of streams a md_*_batch_host call cuts a batch into so that
 *                                its copies overlap with its kernels (1: copy-in, kernels, copy-out one after the other).
 *   "inflate_waves"              1 or 2 (default): wavefronts per stream of the inflate kernel (2 = decoder + copier).
 *   "inflate_parallel_min"       KiB (default 96; 0 = never): a SINGLE stream handed to md_*_inf_ns_inflate /
 *                                md_*_higher_uncompress with at least this much compressed input is decoded in pieces by the
 *                                whole device (csrc/inflate_chunked.hip: candidate block starts, every piece decoded twice
 *                                with placeholder windows by the batch kernel, windows resolved afterwards, checksum verified)
 *                                instead of by one pair of wavefronts.  Results are the same by construction: whatever is not
 *                                a well-formed stream that fits its buffer falls back to the serial path and gets its status.
 *   "inflate_parallel_chunk"     KiB of compressed input per piece (default 64, 4 .. 2^20).
 *   "inflate_parallel_last"      a QUERY (value ignored; the return value is the answer, not a status): pieces of the last
 *                                single stream that went that way | decode rounds << 24; 0 = it took the serial path.
 *   "deflate_link_segment_min"   KiB (default 128; 0 = never): a SINGLE stream handed to md_deflate_batch_host (and so to
 *                                md_de/zl/gz_higher_compress) with at least this much input, format DEFLATE / ZLIB / GZIP,
 *                                driver ZL / HIGHER / CLI, level 1..9 and De's matcher gets its hash chains from the whole
 *                                device, in segments (csrc/deflate_chunked.hip), instead of from one workgroup.  The chains
 *                                are the same, so every status, byte and checksum is the same.
 *   "deflate_link_segment"       KiB of input per segment (0 = default: the stream spread over the CUs, at least 64 KiB).
 *   "gz_members_speculate"       0 or 1 (default): md_gz_members_uncompress of a file whose members do not all state their
 *                                lengths.  1: the device finds the members by speculation and decodes them as one batch;
 *                                0: the host loop, member by member.  Status, info and bytes are the same either way.
 *   "zip_crc_segment"            KiB (4 .. 2^20; 0 = the default, 256): bytes of an entry's output that one wavefront of
 *                                md_zip_uncompress / md_zip_compress copies and checksums.  Results do not depend on it.
 *   "index_read_workspace"       MiB (0 .. 2^20; default 256): device memory for the pieces that ONE round of
 *                                md_inflate_index_read decodes - every piece's window and output, laid end to end.  A read
 *                                whose pieces need more goes in several rounds, one inflate launch each; a piece larger
 *                                than the value gets a round to itself.  0 is the minimum: one piece a round.
 *   "bgzf_read_workspace"        MiB (0 .. 2^20; default 256): device memory for the members that ONE round of md_bgzf_read
 *                                decodes - their bytes packed back to back plus their output slots.  A read whose members
 *                                need more goes in several rounds, one inflate launch each.  0: one member a round.
 *   "pack_workspace"             MiB (0 .. 2^20; default 256): device memory for what ONE round of md_pack_open / md_pack_read
 *                                keeps beside the caller's output - delta payloads, and the bases and intermediate results
 *                                that were not asked for.  A call that needs more goes in several rounds, one inflate launch
 *                                each.  0: one selected object (and its chain of bases) a round.
 *   "sha1_launch_blocks"         1 .. 2^24 (default 4096): blocks of 64 bytes by which ONE launch of the SHA-1 kernel advances
 *                                a message (md_sha1_batch_*, MD_PACK_VERIFY_NAME).  Longer messages take further launches, the
 *                                state kept on the device.  Digests do not depend on it.
 *   "deflate_span_kib"           KiB (0 .. MD_MAX_STREAM / 1024; 0 = the default, 64): the text per span of md_deflate_spans_*
 *                                called with span = 0.  Smaller spans are more parallel, larger ones keep more of the ratio.
 *   "deflate_span_prime"         0 or 1 (default 0; anything else is MD_E_INVALID_ARGUMENT): 1 = md_deflate_spans_* primes
 *                                every span's matcher with the 32 KiB of text in front of it ("Primed spans" below).  Only
 *                                md_deflate_spans_* read it.
 *   "debug_inflate_lds_pad", "debug_known_bounds"  measurement aids of tools/dbg (occupancy curve, known-boundaries floor).
 *   "profile"                    0 / 1: in-kernel phase profile of stream 0 (md_get_profile, a debugging aid).
 * Unknown keys and values out of range: MD_E_INVALID_ARGUMENT. */
int md_set_option(md_ctx *ctx, const char *key, int value);
/* Pinned (page-locked) host memory for the buffers handed to the md_*_host entry points: copies from and to it are DMA
 * transfers that overlap with the kernels.  NULL when the allocation fails.  (An OCaml caller wraps it in a Bigarray with
 * caml_ba_alloc and frees it from the custom block's finaliser: INTEGRATION.md.) */
void *md_host_alloc(md_ctx *ctx, size_t bytes);
void md_host_free(md_ctx *ctx, void *p); /* (ctx may be NULL, or already destroyed: it is not used) */
int md_timing_begin(md_ctx *ctx);
int md_timing_end(md_ctx *ctx, float *ms);

/* Batched inflate of n independent streams, everything resident in HBM.
 *   stream i reads  d_in [in_off[i],  in_off[i]  + in_len[i])
 *            writes d_out[out_off[i], out_off[i] + out_cap[i])
 * Results per stream (device arrays, may not be NULL unless noted):
 *   out_len[i]   bytes written          (the `o` of Ok (i, o))
 *   consumed[i]  input bytes consumed   (the `i` of Ok (i, o); 0 on error)
 *   status[i]    MD_OK or the error variant
 *   checksum[i]  Adler-32 of the output (may be NULL)
 * Semantics per stream = De.Inf.Ns.inflate (lib/de.ml:1807-1822) for
 * MD_FORMAT_DEFLATE, Zl.Inf.Ns.inflate (lib/zl.ml:400-417) for MD_FORMAT_ZLIB.
 * Asynchronous on the context's stream.  Returns MD_OK or a call-level error. */
int md_inflate_batch_device(md_ctx *ctx, int format, size_t n,
                            const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint64_t *d_in_len, uint8_t *d_out,
                            const uint64_t *d_out_off, const uint64_t *d_out_cap,
                            uint64_t *d_out_len, uint64_t *d_consumed,
                            int32_t *d_status, uint32_t *d_checksum);

/* Same with HOST pointers (the reference's callers own host bigarrays, lib/de.mli:93-106): copies inputs H2D, runs the
 * kernels, copies results D2H and synchronises.  h_in/h_out are the packed buffers the offsets index.  A batch of many
 * streams goes through in slices of consecutive streams (md_set_option "host_pipeline_slices", default up to 16; a slice
 * keeps enough streams to fill the device), the copy-in of the next slice and the copy-out of the one before running
 * under the kernels of the current one - which they only do when h_in / h_out are PINNED host memory (md_host_alloc
 * below, or the caller's own hipHostMalloc / hipHostRegister); pageable buffers give the same results, copied one
 * after the other.  The device copies of the blobs belong to the context and are kept between calls
 * (md_set_option "release_workspace" frees them). */
int md_inflate_batch_host(md_ctx *ctx, int format, size_t n, const uint8_t *h_in,
                          size_t in_bytes, const uint64_t *in_off,
                          const uint64_t *in_len, uint8_t *h_out, size_t out_bytes,
                          const uint64_t *out_off, const uint64_t *out_cap,
                          uint64_t *out_len, uint64_t *consumed, int32_t *status,
                          uint32_t *checksum);

/* Every stream's inflated size WITHOUT decoding it: what a caller of md_inflate_batch_* needs to make room for raw
 * DEFLATE and ZLIB streams, which do not say how large they are.  Streams as md_inflate_batch_device; results per
 * stream (device arrays, none may be NULL).  Let R be what md_inflate_batch_device reports for the stream with room
 * that never runs out:
 *   R is MD_OK                 the same status, out_len and consumed.
 *   R is MD_INVALID_CHECKSUM   the size call cannot see this: no byte is produced, so no checksum is compared.  It
 *                              reports MD_OK (MD_INVALID_SIZE for MD_FORMAT_GZIP when ISIZE is wrong too), R's out_len
 *                              and the consumed a correct checksum would have given.
 *   R is any other status      the same status, consumed = 0, and R's out_len: the bytes in front of the failing token.
 * out_len is 64-bit and exact: a stream whose output exceeds MD_MAX_STREAM reports its true size with MD_OK, although
 * md_inflate_batch_device would refuse such a stream with MD_E_INVALID_ARGUMENT.  in_len > MD_MAX_INFLATE_IN is
 * refused per stream, as the decoder refuses it.  MD_UNEXPECTED_END_OF_OUTPUT is not reported for any stream that has a
 * size; the one stream that has none - an incomplete one-code block read at its unused code, which the reference
 * decodes as literals that consume no input, without end - gets that status (what every finite room gives it) and
 * the bytes in front of that point.
 * Asynchronous on the context's stream.  Returns MD_OK or a call-level error (MD_E_INVALID_ARGUMENT: NULL context, a
 * NULL array with n != 0, unknown format). */
int md_inflate_sizes_batch_device(md_ctx *ctx, int format, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                  const uint64_t *d_in_len, uint64_t *d_out_len, uint64_t *d_consumed, int32_t *d_status);
/* The same with HOST pointers: copies the span of h_in the streams lie in, runs the device form, copies the 20 bytes
 * per stream back and synchronises. */
int md_inflate_sizes_batch_host(md_ctx *ctx, int format, size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                                const uint64_t *in_len, uint64_t *out_len, uint64_t *consumed, int32_t *status);
/* The output plan for md_inflate_batch_device from the sizes, on the device: d_out_cap[i] = d_out_len[i], d_out_off =
 * the exclusive sum of the capacities rounded up to `align` (a power of two >= 1), d_total[0] = the bytes to allocate.
 * So sizes -> plan -> 8 bytes read back -> allocate -> decode needs no other round trip.  The plan takes no status: a
 * stream that fails gets the bytes in front of its failure as room, and decoding with that room reports what unlimited
 * room would (every other check of a token precedes the output check).  n is not limited.  Asynchronous on the
 * context's stream.  MD_E_INVALID_ARGUMENT: NULL context, a NULL array with n != 0 (d_total never NULL), an align that
 * is not a power of two.
 * The plan is format-blind: it is also the plan step behind md_lzo_sizes_batch_device (a failing LZO stream has size 0,
 * so its room is 0). */
int md_inflate_plan_device(md_ctx *ctx, size_t n, const uint64_t *d_out_len, size_t align, uint64_t *d_out_off,
                           uint64_t *d_out_cap, uint64_t *d_total);

/* Single-stream mirrors of the reference's whole-buffer entry points (host
 * pointers, batch of one):
 *   De.Inf.Ns.inflate : bigstring -> bigstring -> (int * int, error) result
 *   (lib/de.mli:146-173)  and  Zl.Inf.Ns.inflate (lib/zl.mli, lib/zl.ml:400). */
int md_de_inf_ns_inflate(md_ctx *ctx, const uint8_t *src, size_t src_len,
                         uint8_t *dst, size_t dst_cap, size_t *consumed,
                         size_t *written);
int md_zl_inf_ns_inflate(md_ctx *ctx, const uint8_t *src, size_t src_len,
                         uint8_t *dst, size_t dst_cap, size_t *consumed,
                         size_t *written);

/* The header fields Gz.Def.encoder takes (lib/gz.ml:859-918): ?ascii ?hcrc ?filename ?comment ~mtime os.
 * filename / comment may be NULL (absent; both must be NUL-free and < 256 bytes).  XFL follows the level
 * (2 for level 9, else 0, lib/gz.ml:888-890).  A NULL md_gz_header* means mtime 0, os 3 (Unix), nothing else. */
typedef struct md_gz_header {
  uint32_t mtime;
  int os, hcrc, ascii;
  const char *filename, *comment;
} md_gz_header;

/* What `Zl.Def.encoder ?dynamic ~q ~w ~level` / `De.Lz77.state ?level ~q ~w` / `Lz.state` / `Gz.Def.encoder` take
 * as arguments (lib/zl.mli, lib/de.mli:453-524, lib/lz.mli:1-19, lib/gz.ml:859): per call, nothing is kept in the
 * context. */
typedef struct md_deflate_params {
  int level;     /* 0..9 (lib/de.ml:4030-4049; De.Higher ignores it: always 4, H6) */
  int queue_len; /* De.Queue capacity, a power of two (4096 in the reference's bench / CLI) */
  int driver;    /* MD_DRIVER_* */
  int dynamic;   /* Zl.Def's ?dynamic: 0 -> Fixed blocks */
  int matcher;   /* MD_MATCHER_* */
  const md_gz_header *gz_header; /* MD_FORMAT_GZIP only; NULL = default header */
  int wbits;     /* log2 of the sliding window `De.Lz77.state ~w` derives from its window buffer (lib/de.ml:4462-4464):
                  * 0 or 15 = De.make_window ~bits:15, the only size the reference's callers use and the only one
                  * the kernels implement; anything else is MD_E_INVALID_ARGUMENT */
  size_t total_in_bytes; /* batch calls with device descriptors: an upper bound of the sum of in_len[i], or 0 when the
                  * caller does not know it.  The engine sizes a per-position workspace (13 bytes per input byte
                  * plus 319 positions of padding per stream: hash-chain links, flags and two look-ahead verdicts;
                  * grow-only for the life of the context, and never above md_set_option "deflate_workspace_cap_mib": a batch
                  * that would need more goes in slices of positions) from it; with 0 it reads the sum back from the device first,
                  * i.e. the call waits for the work already enqueued on the context's stream.  A batch whose descriptors
                  * add up to more than the hint gets status[i] = MD_E_INVALID_ARGUMENT for every stream. */
} md_deflate_params;

/* Batched deflate of n independent buffers, everything resident in HBM.
 *   stream i reads d_in[in_off[i], +in_len[i]), writes d_out[out_off[i], +out_cap[i]).
 * Per stream the output is byte-identical to the reference's De.Lz77 (lib/de.ml:4013-4515; or Lz, lib/lz.ml)
 * + De.Def (lib/de.ml:2354-3038) run by params->driver with a command queue of params->queue_len entries:
 *   MD_FORMAT_DEFLATE  the raw body,
 *   MD_FORMAT_ZLIB     Zl.Def framing: 0x78xx header + body + Adler-32 (lib/zl.ml:511-522, 494-499),
 *   MD_FORMAT_GZIP     Gz.Def framing (see MD_FORMAT_GZIP).
 * Results: out_len[i], status[i] (MD_OK, MD_UNEXPECTED_END_OF_OUTPUT when out_cap[i] is too small,
 * MD_QUEUE_FULL), checksum[i] = Adler-32 (CRC-32 for GZip) of the input (may be NULL).  Asynchronous on the
 * context's stream. */
int md_deflate_batch_device(md_ctx *ctx, int format, const md_deflate_params *params, size_t n,
                            const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                            uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                            uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum);

/* Same with HOST pointers (H2D, kernels, D2H, synchronise). */
int md_deflate_batch_host(md_ctx *ctx, int format, const md_deflate_params *params, size_t n,
                          const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                          const uint64_t *in_len, uint8_t *h_out, size_t out_bytes,
                          const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                          int32_t *status, uint32_t *checksum);

/* Single-buffer mirrors of the reference's drivers (host pointers, batch of one):
 *   De.Higher.compress ~w ~q ~refill ~flush i o   (lib/de.mli:533-600): raw DEFLATE, level 4
 *   Zl.Higher.compress ?level ?dynamic ~w ~q ...  (lib/zl.mli, lib/zl.ml:634-648): zlib stream
 *   De.Higher.uncompress / Zl.Higher.uncompress   (lib/de.ml:4555-4571, lib/zl.ml:650-666)
 * The reference's refill/flush callbacks become one source and one destination buffer;
 * *written is the output size.  Returns MD_OK / a status (its md_status_string is the reference's
 * `Msg) / a call error. */
int md_de_higher_compress(md_ctx *ctx, int queue_len, const uint8_t *src, size_t src_len,
                          uint8_t *dst, size_t dst_cap, size_t *written);
int md_zl_higher_compress(md_ctx *ctx, int level, int dynamic, int queue_len, const uint8_t *src,
                          size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written);
int md_de_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                            size_t *written);
int md_zl_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                            size_t *written);

/* The two halves of the encoder on their own (host pointers, batch of one), on the same HIP kernel:
 *
 * De.Lz77.compress (lib/de.mli:453-524; `Lz.compress` with MD_MATCHER_LZ): the match finder alone.  cmds
 * receives the commands of every queue fill in order, in De.Queue's encoding (lib/de.ml:2245-2266: a literal is
 * its byte, end-of-block is 256, a copy is 0x2000000 | (length - 3) << 16 | (offset - 1)); a fill ends with the
 * end-of-block command the reference pushes when one cell is left (H1).  literals[286] / distances[30] receive
 * De.Lz77.literals / distances, cumulative over the input (may be NULL).  MD_UNEXPECTED_END_OF_OUTPUT when
 * cmds_cap is too small (*ncmds is then the number needed).
 *
 * De.Def.encode (lib/de.mli:300-412): the bit encoder alone, the way test/test.ml's `encode` uses it — the
 * commands are ONE last block of `kind`; a Dynamic block gets its trees from the commands' own frequencies
 * (dynamic_of_frequencies, lib/de.ml:2367-2403). */
enum { MD_BLOCK_FLAT = 0, MD_BLOCK_FIXED = 1, MD_BLOCK_DYNAMIC = 2 };
int md_de_lz77_compress(md_ctx *ctx, int level, int queue_len, int matcher, const uint8_t *src, size_t src_len,
                        uint32_t *cmds, size_t cmds_cap, size_t *ncmds, uint32_t *literals, uint32_t *distances);
int md_de_def_encode(md_ctx *ctx, int kind, const uint32_t *cmds, size_t ncmds, uint8_t *dst, size_t dst_cap,
                     size_t *written);

/* De.Def.encode (lib/de.ml:2965-3038) driven step by step, the way the reference's own tests drive it
 * (test/test_ns.ml:388-615, test/test.ml:533-767): one encoder over a queue of queue_len cells and an unbounded
 * `Buffer destination, fed a list of operations (32-bit words):
 *   MD_OP_FILL n c1..cn        Queue.push_exn of n commands (De.Queue's encoding, see md_de_lz77_compress);
 *                              MD_QUEUE_FULL when the queue has no room (exception Queue.Full)
 *   MD_OP_BLOCK kind last      Def.encode e (`Block {kind; last}); kind MD_BLOCK_*; a Dynamic block is
 *                              Def.dynamic_of_frequencies ~literals ~distances of the frequencies counted so far
 *                              (and mutates them the way T.make does)
 *   MD_OP_FLUSH                Def.encode e `Flush
 *   MD_OP_SUCC_LITERAL chr / MD_OP_SUCC_LENGTH len / MD_OP_SUCC_DISTANCE dist   De.succ_* (lib/de.ml:2339-2351)
 *   MD_OP_NEW_FREQS            make_literals () / make_distances ()
 *   MD_OP_QUEUE_RESET          Queue.reset
 * results[k] = what the k-th encode answered: 0 `Ok, 1 `Block (`Partial cannot happen with a `Buffer); *nresults =
 * how many answers results[] received.  At most 315 encodes per call (and results_cap): a list with more is
 * MD_E_INVALID_ARGUMENT after its bytes have been written.  dst receives the bytes written.  A malformed list is
 * MD_E_INVALID_ARGUMENT. */
enum { MD_OP_FILL = 1, MD_OP_BLOCK = 2, MD_OP_FLUSH = 3, MD_OP_SUCC_LITERAL = 4, MD_OP_SUCC_LENGTH = 5,
       MD_OP_SUCC_DISTANCE = 6, MD_OP_NEW_FREQS = 7, MD_OP_QUEUE_RESET = 8 };
int md_de_def_run(md_ctx *ctx, int queue_len, const uint32_t *ops, size_t nops, uint8_t *dst, size_t dst_cap,
                  size_t *written, uint8_t *results, size_t results_cap, size_t *nresults);

/* ---- De.Def.Ns / Zl.Def.Ns (lib/de.ml:3040-4010, lib/zl.ml:596-629): the reference's whole-buffer compressor ----
 * `De.Def.Ns.deflate ?level src dst : (int, [> error ]) result`, an OCaml port of libdeflate's greedy path with its own
 * block splitting and Huffman construction; output byte-identical to it:
 *   level 1..4        compress_greedy (search depth 2 / 6 / 12 / 24, nice length 8 / 10 / 14 / 24);
 *   level 5..12       upstream's compress_lazy is a stub: MD_OK with *written = 0 (lib/de.ml:3927);
 *   level 0           MD_UNEXPECTED_END_OF_OUTPUT for inputs of 56 bytes or more — upstream's write_uncompressed_blocks
 *                     never advances its input and can only leave through that error (lib/de.ml:3411-3420); the same
 *                     when a block of levels 1..4 would be cheapest uncompressed;
 *   inputs shorter than 56 - 4 * level bytes are one stored block; dst needs 8 bytes of slack (compress_bound has them);
 *   other levels      MD_E_INVALID_ARGUMENT (`Invalid_compression_level).
 * md_zl_def_ns_deflate adds Zl.Def.Ns's header (FLEVEL from its own level map, H9) and the Adler-32.
 * Batch form: as md_deflate_batch_device, format MD_FORMAT_DEFLATE or MD_FORMAT_ZLIB, total_in_bytes as in
 * md_deflate_params; checksum[i] = Adler-32 of the input (may be NULL). */
int md_de_def_ns_deflate(md_ctx *ctx, int level, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                         size_t *written);
int md_zl_def_ns_deflate(md_ctx *ctx, int level, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                         size_t *written);
size_t md_de_def_ns_compress_bound(size_t len); /* De.Def.Ns.compress_bound, lib/de.ml:3994-3997 */
size_t md_zl_def_ns_compress_bound(size_t len); /* lib/zl.ml:600 */
int md_def_ns_batch_device(md_ctx *ctx, int format, int level, size_t total_in_bytes, size_t n, const uint8_t *d_in,
                           const uint64_t *d_in_off, const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                           const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum);

/* ---- a DEFLATE stream decoded in pieces (De.Inf.decode's `Flush while input is still arriving, lib/de.ml:1427-1474) ----
 * md_de_inf_continue_host decodes as much of a raw DEFLATE stream as the piece src[0, src_len) holds.  The piece
 * starts start_bit (0..7) bits into src[0]; dst begins with hist_len (<= 32768) bytes of what was decoded before
 * it — the window: matches may reach into them —, decoding writes from dst[hist_len] on, and adler_in is the Adler-32
 * state to go on from (1 for a new stream).  On return *dst_len is the output position reached (history included),
 * *status the stream status for this piece (MD_OK: the final block ended inside it; MD_UNEXPECTED_END_OF_INPUT: the
 * piece ended inside a block — decode the next piece from `resume`; anything else as md_inflate_batch_host), and
 * resume describes the end of the last block that was complete in the piece: bits from src[0] (start_bit included),
 * output position and checksum state there, whether it was the final block.  What lies between resume->out and
 * *dst_len belongs to the incomplete block: it is valid output, but the next piece starts at the block boundary and
 * produces it again.  (md_inf_decode does this by itself once a stream is longer than md_inf_chunk_bytes.) */
typedef struct md_inf_resume {
  uint64_t bits, out;       /* end of the last complete block: input bits from src[0], output position (history included) */
  uint32_t adler, last;     /* Adler-32 state there; 1 when that block was the final one */
  uint64_t consumed;        /* status MD_OK: input bytes of the piece the stream used (as md_inflate_batch_host) */
  uint32_t checksum;        /* Adler-32 state at *dst_len */
  uint32_t crc_out, crc_end; /* flags & MD_CONT_CRC32: CRC-32 of dst[hist_len, out) and of dst[hist_len, *dst_len) */
} md_inf_resume;
enum { MD_CONT_CRC32 = 1 }; /* also compute the CRC-32 of the piece's new output (Gz.Inf's checksum, lib/gz.ml:503) */
/* The same for n streams at once, everything resident in HBM (raw DEFLATE; descriptors as md_inflate_batch_device):
 * piece i starts d_start_bit[i] bits into its first byte, its output buffer begins with d_hist_len[i] bytes of window,
 * its checksum goes on from d_adler_in[i]; results as md_inflate_batch_device (d_out_len includes the window) plus the
 * last block boundary inside each piece: d_resume_bits / d_resume_out (u64), d_resume_adler, d_resume_last (u32). */
int md_inflate_continue_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                     const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                     const uint64_t *d_out_cap, const uint32_t *d_start_bit, const uint32_t *d_hist_len,
                                     const uint32_t *d_adler_in, uint64_t *d_out_len, uint64_t *d_consumed,
                                     int32_t *d_status, uint32_t *d_checksum, uint64_t *d_resume_bits,
                                     uint64_t *d_resume_out, uint32_t *d_resume_adler, uint32_t *d_resume_last);
int md_de_inf_continue_host(md_ctx *ctx, const uint8_t *src, size_t src_len, unsigned start_bit, uint8_t *dst, size_t hist_len,
                            size_t dst_cap, uint32_t adler_in, unsigned flags, size_t *dst_len, int *status,
                            md_inf_resume *resume);

/* ---- the resumable state machines (host side; one launch at the end of input) ----
 * De.Inf.decoder / decode / src / flush / dst_rem / src_rem / checksum (lib/de.mli:82-144) and the encoder loop of
 * Zl.Def / Gz.Def / De.Higher with `Manual source and destination (lib/zl.ml:509-555): the caller supplies input
 * with src (length 0 = end of input, as in the reference), calls decode / encode, and consumes its output buffer
 * whenever it gets MD_FLUSH (then md_inf_flush / md_def_dst), until MD_END or MD_MALFORMED (md_*_status gives
 * the MD_* status whose string is the reference's `Malformed message).  See csrc/stream_shim.cpp. */
/* Memory: the encoder works in pieces, like the reference's (whose state is its window, its queue and one output
 * buffer).  md_def_src appends to a host buffer; once md_set_option "encoder_piece_bytes" (default 1 MiB) have gathered -
 * or the end of the input is signalled - md_def_encode launches the kernels on them: they go on from the state the
 * launch before left in device memory (12 KiB and the command queue), answer `Await inside the kernel exactly where
 * De.Lz77 would (lookahead under 262 and nothing left of the piece), and the piece's output is handed out through
 * `Flush steps while more input arrives.  Host and device each hold the last 64 KiB of the stream and the piece in
 * flight; a stream may be of any length (positions are rebased inside, gzip's ISIZE wraps at 2^32 as lib/gz.ml's);
 * one md_def_src call takes at most 1 GiB, and so does what md_def_src calls have handed over since the last md_def_encode
 * (MD_E_INVALID_ARGUMENT beyond that: call md_def_encode between sources - it launches what has arrived).  The bytes are those of the reference handed the input in the same pieces
 * (fill_window's slide depends on how much each fill finds; for whole streams and for pieces the oracle agrees).  The decoder
 * (DEFLATE, ZLIB, GZip) works in pieces: once md_inf_chunk_bytes (default 8 MiB; a piece of at least "inflate_parallel_min" is decoded by the whole device) of input are buffered
 * it decodes up to the last block boundary inside them (md_de_inf_continue_host), hands that output out through
 * `Flush steps while input is still arriving, and keeps only the undecoded tail and the 32 KiB window; a stream that
 * ends before a piece is full is decoded in one launch as before.
 * md_inf_message: the reference's `Malformed string with its numbers, e.g. "Invalid checksum (expect:%04lx,
 * has:%04lx)" (lib/zl.ml:179-181, lib/gz.ml:287-289), "Invalid input size (expect:%ld, inflated:%ld)"
 * (lib/gz.ml:291-293); md_status_string(md_inf_status) is its fixed part.  md_inf_reset = De.Inf.reset
 * (lib/de.ml:1512-1532): the same decoder for another stream. */
enum { MD_AWAIT = 0, MD_FLUSH = 1, MD_END = 2, MD_MALFORMED = 3 };
typedef struct md_inf_stream md_inf_stream;
md_inf_stream *md_inf_decoder(md_ctx *ctx, int format, uint8_t *o, size_t o_len);
void md_inf_reset(md_inf_stream *s);
void md_inf_chunk_bytes(md_inf_stream *s, size_t bytes); /* input buffered before a piece is decoded (>= 1) */
const char *md_inf_message(const md_inf_stream *s);
int md_inf_src(md_inf_stream *s, const uint8_t *buf, size_t off, size_t len);
int md_inf_decode(md_inf_stream *s);
void md_inf_flush(md_inf_stream *s);
size_t md_inf_dst_rem(const md_inf_stream *s);
size_t md_inf_src_rem(const md_inf_stream *s);
int md_inf_status(const md_inf_stream *s);
uint32_t md_inf_checksum(const md_inf_stream *s);
void md_inf_free(md_inf_stream *s);
typedef struct md_def_stream md_def_stream;
md_def_stream *md_def_encoder(md_ctx *ctx, int format, const md_deflate_params *params, uint8_t *o, size_t o_len);
int md_def_src(md_def_stream *s, const uint8_t *buf, size_t off, size_t len);
int md_def_encode(md_def_stream *s);
void md_def_dst(md_def_stream *s, uint8_t *o, size_t o_len);
size_t md_def_dst_rem(const md_def_stream *s);
int md_def_status(const md_def_stream *s);
uint32_t md_def_checksum(const md_def_stream *s);
void md_def_free(md_def_stream *s);

/* ---- many streaming encoders at once ----
 * n independent Zl.Def / Gz.Def / De.Def encoders (lib/zl.ml:509-555: every `Zl.Def.encoder` is its own state machine) with
 * the same parameters, advanced TOGETHER: md_def_batch_src hands input to encoder i (host memory, copied; length 0 = the
 * end of its input, as in the reference), md_def_batch_encode is ONE launch of the kernels over what has arrived for all
 * of them since the last one - whatever n is - and leaves every encoder's output of that launch in device memory, from
 * where md_def_batch_out copies it out (md_def_batch_pending says how much waits; what is not fetched before the next
 * encode is kept on the host side).  md_def_batch_status: MD_AWAIT (more input wanted), MD_END (the trailer is written:
 * the stream is complete once its pending output is fetched) or MD_MALFORMED (md_def_batch_error: that stream's MD_* status).  An encoder's window
 * (the last 64 KiB of its text), its state and its queue stay in device memory between launches: only new bytes cross the
 * link, in one copy per launch.  The bytes of every encoder are those of md_def_* - and of the reference - handed the same
 * pieces (a piece = what arrived between two md_def_batch_encode calls).  One md_def_batch_src hands over 1 GiB at most. */
typedef struct md_def_batch md_def_batch;
md_def_batch *md_def_batch_open(md_ctx *ctx, int format, const md_deflate_params *params, size_t n);
int md_def_batch_src(md_def_batch *b, size_t i, const uint8_t *buf, size_t len);
int md_def_batch_encode(md_def_batch *b);
size_t md_def_batch_pending(const md_def_batch *b, size_t i);
size_t md_def_batch_out(md_def_batch *b, size_t i, uint8_t *dst, size_t cap);
int md_def_batch_status(const md_def_batch *b, size_t i);
int md_def_batch_error(const md_def_batch *b, size_t i);
uint32_t md_def_batch_checksum(const md_def_batch *b, size_t i);
void md_def_batch_close(md_def_batch *b);

/* ---- many streaming decoders at once ----
 * n independent De.Inf / Zl.Inf / Gz.Inf decoders (format MD_FORMAT_DEFLATE, _ZLIB or _GZIP; NULL on misuse), advanced
 * TOGETHER: md_inf_batch_src hands input to decoder i (host memory, copied; length 0 = the end of its input, as in the
 * reference), md_inf_batch_decode is ONE launch of the inflate kernel over every decoder that received input or its end
 * since the last round - whatever n is; decoders with nothing new sit the round out, and a round without work launches
 * nothing.  (A decoder whose output room ran out gets 4x the room and one more launch in the same call.)  Each round
 * decodes a decoder's undecoded input up to the last complete block boundary and hands that output out; the round that
 * ends a stream - or fails it - hands out everything decoded.  md_inf_batch_pending / md_inf_batch_out: output waits on
 * the host side until fetched, across rounds.  md_inf_batch_status: MD_AWAIT (more input wanted), MD_END or MD_MALFORMED
 * (md_inf_batch_error: the MD_* status; md_inf_batch_message: the reference's `Malformed string, as md_inf_message).
 * md_inf_batch_checksum: Adler-32 (DEFLATE, ZLIB) or CRC-32 (GZIP) once the stream ended; md_inf_batch_src_rem: input
 * after the stream's end; md_inf_batch_reset: De.Inf.reset for slot i.  Every decoder's results - bytes, status, message,
 * checksum, src_rem - are those of md_inf_* with md_inf_chunk_bytes(1) handed the same pieces.  A decoder that found no
 * block end takes part again only once its buffered input has doubled (or at its end of input), as md_inf_* does.  The
 * undecoded tail and the window (the last <= 32 KiB of output) stay in device memory between rounds; a round costs one
 * copy of the fresh bytes in, and two copies back.  md_inf_batch_src refuses (MD_E_INVALID_ARGUMENT) input after the end of
 * input, on a finished slot, and more than 1 GiB per decoder and round. */
typedef struct md_inf_batch md_inf_batch;
md_inf_batch *md_inf_batch_open(md_ctx *ctx, int format, size_t n);
int md_inf_batch_src(md_inf_batch *b, size_t i, const uint8_t *buf, size_t len);
int md_inf_batch_decode(md_inf_batch *b);
size_t md_inf_batch_pending(const md_inf_batch *b, size_t i);
size_t md_inf_batch_out(md_inf_batch *b, size_t i, uint8_t *dst, size_t cap);
int md_inf_batch_status(const md_inf_batch *b, size_t i);
int md_inf_batch_error(const md_inf_batch *b, size_t i);
const char *md_inf_batch_message(const md_inf_batch *b, size_t i);
uint32_t md_inf_batch_checksum(const md_inf_batch *b, size_t i);
size_t md_inf_batch_src_rem(const md_inf_batch *b, size_t i);
void md_inf_batch_reset(md_inf_batch *b, size_t i);
void md_inf_batch_close(md_inf_batch *b);

/* ---- GZip (lib/gz.ml) ---- */

/* What Gz.Inf.filename / comment / os / extra report (lib/gz.ml:612-633): offsets into src. */
typedef struct md_gz_meta {
  uint32_t flg, mtime, xfl, os;
  int has_extra, has_name, has_comment;
  size_t extra_off, extra_len, name_off, name_len, comment_off, comment_len;
} md_gz_meta;

/* Single-buffer mirrors (host pointers, batch of one):
 *   Gz.Higher.compress ?level ?filename ?comment ~w ~q ... (lib/gz.ml:927-950; NB its ?level
 *   defaults to 0 there — pass the level you mean)
 *   Gz.Higher.uncompress ~refill ~flush i o            (lib/gz.ml:959-982); meta may be NULL. */
int md_gz_higher_compress(md_ctx *ctx, int level, int queue_len, const md_gz_header *header, const uint8_t *src,
                          size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written);
int md_gz_higher_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                            size_t *consumed, size_t *written, md_gz_meta *meta);

/* Checkseum.Crc32 of n buffers resident in HBM (call sites lib/gz.ml:503, :682): crc[i] =
 * CRC-32 of d_data[off[i], off[i] + len[i]).  Asynchronous on the context's stream. */
int md_crc32_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *d_off,
                          const uint64_t *d_len, uint32_t *d_crc);

/* ---- LZO1X (lib/lzo.ml; SURVEY 8(f) row 3, BASELINE config 5) ---- */

/* Lzo.uncompress input output (lib/lzo.ml:395-403) over n independent streams resident in HBM:
 * status[i] = MD_OK, MD_UNEXPECTED_END_OF_INPUT or one of MD_LZO_*; out_len[i] = bytes written
 * (0 on error).  Asynchronous on the context's stream. */
int md_lzo_uncompress_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                   const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status);
/* Lzo.compress in_data out_data wrkmem (lib/lzo.ml:642-660; the 16 K-entry wrkmem is a per-stream
 * workspace owned by the context)
 * over n independent buffers: status[i] = MD_OK or MD_LZO_OUT_OF_BOUND when out_cap[i] is too
 * small (n + n/16 + 64 + 3 always suffices). */
int md_lzo_compress_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                                 const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                 const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status);
/* Every LZO stream's uncompressed size WITHOUT decoding it: an LZO1X stream does not say how large its output is.
 * Streams as md_lzo_uncompress_batch_device; results per stream (device arrays, none may be NULL).  The statuses are
 * those of Lzo.uncompress_with_buffer (lib/lzo.ml:199-216, :405-414), whose buffer grows.  Let U be what
 * md_lzo_uncompress_batch_device reports for the stream with room that never runs out:
 *   U is MD_OK                      MD_OK and U's out_len.  It is 64-bit and exact, also beyond MD_MAX_STREAM (every zero
 *                                   byte of a length adds 255 bytes: 17 MB of input can describe more than 4 GiB), although
 *                                   the decoder writes at most MD_MAX_STREAM.
 *   U is MD_UNEXPECTED_END_OF_INPUT, MD_LZO_INVALID_INPUT or MD_LZO_NO_DICTIONARY
 *                                   the same status, out_len 0.
 *   U is MD_LZO_OUT_OF_BOUND        because a match's offset reaches back beyond the output so far: MD_INVALID_DICTIONARY
 *                                   (`Invalid_dictionary, lib/lzo.ml:216); because literals or a two-byte operand run over
 *                                   the input's end: MD_LZO_MALFORMED_INPUT (lib/lzo.ml:414).  out_len 0.
 * "Output not large enough" does not exist here, and the size call never reports MD_LZO_OUT_OF_BOUND.  Inside one
 * instruction the checks come in the reference's order: operand bytes, the dictionary check of the copy, the literals
 * behind it.  An empty input is MD_UNEXPECTED_END_OF_INPUT; in_len > MD_MAX_STREAM gets MD_E_INVALID_ARGUMENT for that
 * stream with nothing read, as the decoder does.
 * sizes -> md_inflate_plan_device -> 8 bytes read back -> allocate -> md_lzo_uncompress_batch_device needs no other round
 * trip.  On that path a stream's status is the size call's; of a stream it called valid the decode reports MD_OK and the
 * same out_len.
 * Asynchronous on the context's stream.  Returns MD_OK or a call-level error (MD_E_INVALID_ARGUMENT: NULL context, a NULL
 * array with n != 0, more than 2^31 - 1 streams). */
int md_lzo_sizes_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                              uint64_t *d_out_len, int32_t *d_status);
/* The same with HOST pointers: checks the ranges against in_bytes (and MD_MAX_STREAM), copies the span of h_in the streams
 * lie in, runs the device form, copies the 12 bytes per stream back and synchronises. */
int md_lzo_sizes_batch_host(md_ctx *ctx, size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                            const uint64_t *in_len, uint64_t *out_len, int32_t *status);
/* Single-buffer mirrors (host pointers, batch of one): Lzo.uncompress / Lzo.compress. */
int md_lzo_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                      size_t *written);
int md_lzo_compress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                    size_t *written);
/* Lzo.uncompress_with_buffer ?chunk input (lib/lzo.ml:405-414): the library makes the room.  One upload, the size call,
 * 12 bytes back, *dst = md_host_alloc(size), a decode into exactly that room from the input already on the device, one
 * copy back.  Returns the stream's status as md_lzo_sizes_batch_device states it, or a negative call error; a size beyond
 * MD_MAX_STREAM is MD_E_INVALID_ARGUMENT.  On MD_OK the caller frees *dst with md_host_free (an empty result is a valid
 * block too); on anything else *dst = NULL and *dst_len = 0.  (?chunk is only the initial size of the reference's
 * buffer: there is nothing to pass.) */
int md_lzo_uncompress_with_buffer(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t **dst, size_t *dst_len);

/* ---- A GZip FILE of many members (RFC 1952 2.2): `cat a.gz b.gz`, bgzip / BGZF (.bam, .vcf.gz), pigz -i -----------------
 * These entry points read and write RFC 1952 as libz does - NOT Gz.Inf's reading, which MD_FORMAT_GZIP keeps (FEXTRA's
 * length big-endian, its own header CRC, one member and stop): XLEN is little-endian, CM must be 8, the reserved flag
 * bits must be clear, FHCRC is the low half of the CRC-32 of the whole header, members follow each other until the
 * input ends, and NUL bytes behind a member are padding.  Host pointers: copy in, kernels, copy out, synchronise.
 *
 * A file is INDEXED when every member carries its own length - the extra subfield 'B' 'C' (SLEN 2, BSIZE = length - 1)
 * that bgzip writes - and the chain of those lengths leads from offset 0 to the end of the file (or to NUL padding that
 * reaches it).  The device finds the members of such a file without decoding (a scan of every byte position, pointer
 * jumping over the candidates), parses their headers and decodes ALL of them in one inflate launch, each into a window of
 * its own ISIZE bytes.  Workspace: 1 bit per input byte, 4 bytes per 16 KiB and O(members), grow-only.
 * Any other file (cat *.gz, WARC / ARC, rotated logs, mgzip, a BGZF file with one damaged BSIZE) is read by SPECULATION:
 * every position that looks like a member's start (1f 8b 08, no reserved flag bit) is a candidate, the bytes between two
 * candidates are a span, and every plausible span is decoded as if it were a member, all of them in ONE inflate launch,
 * each into the size the four bytes at its end promise.  A span is VERIFIED when that decode ends exactly where the next
 * candidate begins and the CRC-32 and ISIZE found there match.  The host then walks the file as libz does: where it stands
 * on a verified span it takes the member from the batch (consecutive ones leave by one copy); anywhere else - a candidate
 * that was none (magic bytes inside a body or a header field), NUL padding behind a member, a member long enough to set
 * the batch's time (it goes to the whole chip), a member without room, a damaged member - it takes ONE step of the
 * GENERAL path: header on the host, the body through the raw-DEFLATE path of md_de_inf_ns_inflate, CRC-32 and ISIZE
 * checked on the host.  The walk only ever stands where libz's reading stands, a verified span is the same header, body
 * and trailer check that step would make there, and everything else IS that step: status, members, consumed, written and
 * the bytes are those of the general path for valid and damaged files alike.  A file with fewer than two candidates, or
 * md_set_option "gz_members_speculate" = 0, takes the general path member by member - one round of launches per member.
 * md_gz_members_last says which way the last call went.  A member is bound by MD_MAX_INFLATE_IN / MD_MAX_STREAM; the file
 * may be longer. */
typedef struct md_gz_members_info {
  size_t members;  /* members decoded (or found, for _scan) */
  size_t consumed; /* bytes of src taken: src_len on success; on failure the offset of the failing member */
  size_t written;  /* bytes in dst from the members before that; with MD_UNEXPECTED_END_OF_OUTPUT on an indexed file:
                    * the room needed (the sum of the members' ISIZE fields; such a call goes member by member) */
  int indexed;     /* 1: every member carried a BC size field - found on the device, decoded by one inflate launch */
} md_gz_members_info;
/* The .gzi index of an indexed file without decoding it: info->members, info->written = the uncompressed size (the sum of
 * the members' ISIZE fields), and the first `cap` pairs (offset of member i in src, offset of its output).  c_off / u_off
 * may be NULL when cap is 0.  A file that is not indexed: MD_OK, indexed = 0, nothing else filled. */
int md_gz_members_scan(md_ctx *ctx, const uint8_t *src, size_t src_len, md_gz_members_info *info, uint64_t *c_off,
                       uint64_t *u_off, size_t cap);
/* Every member of src, in order, into dst.  Returns MD_OK or the status of the first member that failed (info says where):
 * MD_INVALID_GZIP_HEADER (magic, CM, reserved flag bits, bytes other than NUL behind a member),
 * MD_INVALID_GZIP_HEADER_CHECKSUM, MD_INVALID_CHECKSUM, MD_INVALID_SIZE, MD_UNEXPECTED_END_OF_INPUT (truncated),
 * MD_UNEXPECTED_END_OF_OUTPUT (dst_cap), or what the inflate kernel says about the body.  Empty input: MD_OK, 0 members. */
int md_gz_members_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                             md_gz_members_info *info);
/* Which way the last md_gz_members_uncompress of this context went, and what the speculative path made of the file. */
typedef struct md_gz_members_stats {
  int path;              /* 0 general (the host loop alone), 1 indexed, 2 speculative */
  size_t candidates;     /* path 2: positions that look like a member's start */
  size_t spans_decoded;  /* path 2: spans the batch launch decoded */
  size_t members_device; /* members accepted from a batch launch */
  size_t members_host;   /* members the host step decoded */
  size_t spans_long, spans_no_room, spans_implausible; /* path 2: spans the batch left out - a body of a 1 024th of all
                          * bodies or more (and "inflate_parallel_min"); a promised size that ends behind dst_cap; no
                          * member's header, or a promised size above 1 032 x body + 8, which DEFLATE cannot reach */
} md_gz_members_stats;
/* MD_OK, or MD_E_INVALID_ARGUMENT for a NULL pointer.  All zero before the first md_gz_members_uncompress. */
int md_gz_members_last(const md_ctx *ctx, md_gz_members_stats *out);
/* Blocked gzip, as bgzip writes it: src cut into blocks of `block` bytes (1..0xff00; 0 = 0xff00), each a member
 * 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' 02 00 BSIZE | body | CRC-32 | ISIZE, then the 28-byte empty
 * member that marks the end.  All blocks are compressed by ONE deflate launch; a member's body is byte for byte what
 * MD_FORMAT_GZIP writes for that block at `level` (Gz.Def: Zl driver, dynamic blocks, queue 4096) - unless one stored block
 * (01 LEN NLEN + the bytes) is shorter (input that does not compress: the reference's body for 0xff00 random bytes would make
 * a member of 65 898 bytes, and none may pass 65 536), then it is that stored block.  The output depends on (src, level,
 * block) alone and is an indexed file for md_gz_members_*.  md_bgzf_compress_bound: room that always suffices (host
 * arithmetic: 31 bytes per block, the stored form, + 28); 0 for a block size out of range. */
size_t md_bgzf_compress_bound(size_t src_len, size_t block);
int md_bgzf_compress(md_ctx *ctx, int level, size_t block, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                     size_t *written);

/* ---- One long stream written as joined spans ---------------------------------------------------------------------------
 * md_zl_higher_compress and its kin write ONE stream byte for byte as the reference does, which is sequential work for one
 * wavefront.  This writer is the whole chip's, the way pigz does it: the text is cut into n = max(1, ceil(src_len / span))
 * spans, the spans are compressed independently by ONE deflate launch, and the bodies are joined into one standard stream
 * that Zl.Inf / Gz.Inf / De.Inf and libz read to its end.  Exactly:
 *   B_i   the raw body md_deflate_batch_device writes for span i under `params` (MD_FORMAT_GZIP: the Zl driver with dynamic
 *         blocks, as for MD_FORMAT_GZIP everywhere); h_i the bit offset of its closing block's header, e_i the bit offset
 *         behind that block's last bit (its end-of-block code; a stored block: its byte-aligned end)
 *   J_i   the last span: B_i.  Any other: the first e_i bits of B_i with bit h_i (BFINAL) cleared, the three bits 0 00, zero
 *         bits up to the byte, then 00 00 FF FF - an empty stored block, so the span ends on a byte
 *   S_i   the span's bytes as stored blocks of at most 65 535 bytes, all but the last full (the empty text: one empty
 *         block), BFINAL only on the last block of the last span
 * Span i goes out as S_i exactly when J_i is strictly longer than S_i, else as J_i.  The body is the chosen forms end to
 * end; MD_FORMAT_ZLIB puts Zl.Def's two header bytes in front and the big-endian Adler-32 of the text behind,
 * MD_FORMAT_GZIP the header of params->gz_header in front and CRC-32 and length mod 2^32 behind.  With one span the bytes
 * are md_deflate_batch_host's for that text (unless the stored form wins).  A span cannot refer back across a joint, so
 * the stream is somewhat longer than the single stream (README); it depends on (text, params, span) alone.
 * Primed spans (md_set_option "deflate_span_prime" = 1): span i is text [s_i, e_i) and has a prefix of
 * w_i = min(s_i, 32768) bytes.  Its body B_i is defined over the stream X_i = text[s_i - w_i, e_i), whose position 0 is the
 * prefix's first byte: B_i is what the reference's matcher (De.Lz77 or Lz) and De.Def write under `params` for X_i when the
 * matcher has first walked positions [0, w_i) in this way - at each position it inserts the position if lookahead >=
 * MIN_MATCH, then does strstart += 1, lookahead -= 1; it never calls longest_match and emits nothing; it then stands at
 * strstart = w_i with match_available = false and match_length at its initial value (so De's first longest_match, entered
 * with prev_length 0, also compares the byte in front of the span).  Everything else follows the reference in the positions
 * of X_i: fill_window, the slide at strstart - base >= WSIZE + MAX_DIST, NIL at position 0, positions inserted ahead below
 * the stream's end, the tail heads of its last string, the automatic end-of-block commands.  Histograms, queue and encoder
 * start fresh; the input checksum covers [w_i, |X_i|) only; at level 0, or where the matcher only copies, the copy starts
 * at w_i.  With w_i = 0 this is the unprimed B_i: span 0 and one-span calls keep their bytes.  h_i, e_i, J_i, S_i (chosen
 * against the span's own bytes), marker, headers, trailers and checksums are as above.  The stream is nearly as short as the
 * single stream; the per-position workspace covers src_len + 32768 (n - 1) positions at the most.
 *   span    bytes of text per span, 1 .. MD_MAX_STREAM; 0 = md_set_option "deflate_span_kib" (KiB; default 64)
 *   params  as md_deflate_batch_device takes them (levels 0-9, the three drivers, both matchers, dynamic 0 / 1, wbits 0 / 15);
 *           anything else is MD_E_INVALID_ARGUMENT.  total_in_bytes is ignored.  At most 0x7ffffff0 spans.
 * md_deflate_spans_bound: room that always suffices (host arithmetic: every span stored, header, trailer; span 0: the bound
 *   of the smallest span the option selects); 0 for bad arguments and for a sum that size_t does not hold.
 * md_deflate_spans_host: host buffers; MD_UNEXPECTED_END_OF_OUTPUT when dst_cap is short (nothing is written then), a span's
 *   MD_QUEUE_FULL is the call's status; *checksum (may be NULL): Adler-32 of the text, CRC-32 for MD_FORMAT_GZIP.
 * md_deflate_spans_device: everything in device memory, asynchronous on the context's stream, nothing read back (unless the
 *   spans' workspace is above md_set_option "deflate_workspace_cap_mib": the deflate launch then goes in slices of positions,
 *   which waits for the stream and reads the slices' results back, as md_deflate_batch_device does): *d_written
 *   = the stream's length (what it needs when *d_status is MD_UNEXPECTED_END_OF_OUTPUT: no byte of d_dst is written then),
 *   *d_status and *d_checksum as above.  The per-position workspace and its cap are md_deflate_batch_device's.
 * md_deflate_spans_last: spans, stored spans and span bytes of the context's last call (after the device form it waits for
 *   the context's stream). */
typedef struct md_deflate_spans_info {
  size_t spans;        /* n */
  size_t stored_spans; /* spans that went out in the stored form */
  size_t span_bytes;   /* the span in bytes, the option resolved */
} md_deflate_spans_info;
size_t md_deflate_spans_bound(int format, size_t src_len, size_t span, const md_gz_header *hdr);
int md_deflate_spans_host(md_ctx *ctx, int format, const md_deflate_params *params, size_t span, const uint8_t *src, size_t src_len,
                          uint8_t *dst, size_t dst_cap, size_t *written, uint32_t *checksum);
int md_deflate_spans_device(md_ctx *ctx, int format, const md_deflate_params *params, size_t span, const uint8_t *d_src,
                            size_t src_len, uint8_t *d_dst, size_t dst_cap, uint64_t *d_written, int32_t *d_status,
                            uint32_t *d_checksum);
int md_deflate_spans_last(md_ctx *ctx, md_deflate_spans_info *info);

/* ---- ZIP archives (PKWARE APPNOTE; .zip .jar .whl .npz .docx .apk .epub): every entry in one batch ----------------------
 * An entry is a raw RFC 1951 stream (method 8) or plain bytes (method 0), and the central directory states every entry's
 * offset, sizes and CRC-32: nothing is scanned for, guessed or sized by a pass of its own.
 *
 * md_zip_directory reads the directory of the archive src[0, src_len) on the HOST: it takes no context and touches no
 * device (like md_bgzf_compress_bound and md_shard_plan).  It fills the first `cap` entries; info->entries says how many
 * there are, so a caller calls it twice (entries may be NULL when cap is 0).  Returns MD_OK, MD_E_INVALID_ARGUMENT (a NULL
 * src or info, NULL entries with cap != 0) or MD_INVALID_ZIP_DIRECTORY.  Every read is checked against src_len.  Rules:
 *  - the end record is the LAST position p within the final 65 557 bytes that holds 50 4b 05 06 and whose comment ends
 *    exactly at the end (p + 22 + comment length == src_len): a comment that contains a record's signature is not taken
 *    for one, and an archive with bytes behind its comment is refused;
 *  - a ZIP64 locator (50 4b 06 07) at p - 20 demands the 56-byte ZIP64 end record (50 4b 06 06, no extensible data) at
 *    p - 76; its counts, directory size and offset are then the archive's.  A locator without that record is refused;
 *  - prefix = (start of the ZIP64 end record if present, else p) - directory size - directory offset must be >= 0: the
 *    directory ends where the end record begins, and bytes in front of the archive (a self-extracting stub) move every
 *    offset by `prefix`;
 *  - disk numbers are 0 (or all-ones where ZIP64 replaces them), the entry counts of "this disk" and "all disks" agree;
 *  - every central header has its signature and lies, with name, extra field and comment, inside the directory; the ZIP64
 *    extra field 0x0001 gives usize, csize, offset and disk - in that order, only for those fixed fields that are
 *    all-ones - and a missing or short one is refused; the headers are as many as the end record says and fill the
 *    directory exactly; the sum of usize fits 64 bits.
 * Local headers and bodies are NOT looked at here. */
typedef struct md_zip_entry { /* fixed-width fields only */
  uint64_t header_off;        /* the local header in src (prefix added) */
  uint64_t csize, usize;      /* as the directory states them */
  uint64_t name_off;          /* the directory's copy of the name, in src */
  uint32_t crc32, external_attr;
  uint16_t name_len, method, flags, dos_time, dos_date;
  uint16_t reserved[3];
} md_zip_entry;
typedef struct md_zip_info {
  size_t entries;
  uint64_t total_usize;       /* the sum of usize */
  uint64_t dir_off, dir_size; /* as the end record states them: the directory begins at prefix + dir_off in src */
  uint64_t prefix, comment_off;
  uint32_t comment_len;
  int zip64;                  /* 1: a ZIP64 end record was read */
} md_zip_info;
int md_zip_directory(const uint8_t *src, size_t src_len, md_zip_info *info, md_zip_entry *entries, size_t cap);

/* Entries of the archive, decoded, checked and packed back to back into dst: host pointers (copy in, kernels, copy out,
 * synchronise).  select == NULL: every entry in directory order (k = entries); otherwise the nselect directory indices in
 * select, repeats allowed (an index out of range: MD_E_INVALID_ARGUMENT).  out_off (k + 1 words) and status (k words) are
 * the caller's; out_off[j + 1] - out_off[j] is the directory's usize of selected entry j whatever its status, out_off[k] =
 * res->written.  If that sum exceeds dst_cap the call returns MD_UNEXPECTED_END_OF_OUTPUT with res->written = the room
 * needed; nothing is launched and dst is untouched (so dst_cap also bounds what a lying directory can make the call
 * allocate).  Entries are independent files: the call returns MD_OK once the directory was read and every selected entry
 * has a status, and res->failed counts those that are not MD_OK; a damaged entry touches neither the bytes nor the status
 * of another.  A directory failure returns MD_INVALID_ZIP_DIRECTORY; an empty archive is MD_OK with 0 entries.
 * Only the span of src from the first selected local header to where the last selected body can end goes to the device.
 * On the device: one thread per entry checks the local header (it lies in front of the directory, signature 50 4b 03 04,
 * the name has the directory's length and bytes - the one comparison Python's zipfile makes; the local sizes, CRC and
 * extra field are not trusted or compared, a data descriptor makes them zero anyway - and the body ends in front of the
 * directory); ONE inflate launch over the method-8 entries, each into exactly its usize bytes; then the outputs are cut
 * into segments of md_set_option "zip_crc_segment" bytes (the table segment -> entry is built on the host, from the
 * directory) and one wavefront per segment copies a stored entry's bytes and computes the segment's CRC-32, so one entry
 * of 1 GiB is copied and checked by the whole chip; a last kernel joins each entry's segment CRCs.  status[j], the first
 * that applies:
 *   MD_INVALID_ZIP_HEADER        a check of the local header above failed
 *   MD_ZIP_UNSUPPORTED           flag bit 0 (encrypted), 6 or 13, or a method other than 0 and 8
 *   MD_INVALID_SIZE              a stored entry with csize != usize
 *   the decoder's status         if not MD_OK.  A directory whose usize is too SMALL shows here, as the decoder's
 *                                MD_UNEXPECTED_END_OF_OUTPUT; csize > MD_MAX_INFLATE_IN or usize > MD_MAX_STREAM of a
 *                                method-8 entry is MD_E_INVALID_ARGUMENT, as with device descriptors (stored entries
 *                                have no such limit)
 *   MD_INVALID_SIZE              the stream ended before csize bytes were consumed or usize bytes written
 *   MD_INVALID_CHECKSUM          the CRC-32 is not the directory's
 * Out of scope: an entry long enough to set the batch's time is not taken out of the batch to the whole-chip decoder;
 * encrypted entries and methods 9 / 12 / 14 / 93 (MD_ZIP_UNSUPPORTED); archives of several disks (refused by the
 * directory); entries that share or overlap bodies are decoded independently (dst_cap bounds the total). */
typedef struct md_zip_result {
  size_t entries, failed; /* selected entries; those whose status is not MD_OK */
  uint64_t written;       /* bytes of dst the entries take (or, with MD_UNEXPECTED_END_OF_OUTPUT, would take) */
} md_zip_result;
int md_zip_uncompress(md_ctx *ctx, const uint8_t *src, size_t src_len, const uint64_t *select, size_t nselect, uint8_t *dst,
                      size_t dst_cap, uint64_t *out_off, int32_t *status, md_zip_result *res);

/* The writer.  File i is src[off, off + len) under `name` (name_len bytes, not NUL-terminated).  ONE deflate launch over
 * all files - raw DEFLATE with the parameters of MD_FORMAT_GZIP's body (Zl driver, dynamic blocks, queue 4096, De's
 * matcher) at `level` - each into a slot of len bytes; a file whose body does not come out shorter than the file is
 * written stored (method 0), as is every file at level 0 and every empty file.  The CRC-32 of the inputs comes from the
 * segmented kernel of the reader, one launch packs local headers and bodies into the file image, and the host writes the
 * central directory and the end record(s).  Local headers carry no extra field and no data descriptor, version needed is
 * 20 (deflated) or 10 (stored), flag 0x0800 (UTF-8) is set exactly when the name has a byte >= 0x80; the ZIP64 end record
 * and locator appear exactly when n > 0xfffe.  The bytes depend on (files, src, level) alone.
 * md_zip_compress_bound: room that always suffices, the sum of (76 + 2 name_len + len) + 98 (host arithmetic); 0 when the
 * arguments are refused (NULL files with n != 0, a name_len of 0 or above 0xffff, a sum that does not fit).
 * MD_E_INVALID_ARGUMENT: a file beyond src_len, len > MD_MAX_STREAM, a NULL name, name_len 0 or > 0xffff, level outside
 * 0..9, or an archive whose bound reaches 4 GiB: the writer has no 64-bit offset fields (the reader has no such limit).
 * MD_UNEXPECTED_END_OF_OUTPUT: dst_cap is less than the archive takes. */
typedef struct md_zip_source {
  const char *name;
  size_t name_len;
  uint64_t off, len;
  uint32_t external_attr;
  uint16_t dos_time, dos_date;
} md_zip_source;
size_t md_zip_compress_bound(size_t n, const md_zip_source *files);
int md_zip_compress(md_ctx *ctx, int level, size_t n, const md_zip_source *files, const uint8_t *src, size_t src_len,
                    uint8_t *dst, size_t dst_cap, size_t *written);

/* ---- The index of ONE long stream: read any byte range without decoding what lies in front of it ------------------------
 * An index in the zran / gztool / indexed_gzip sense over a raw DEFLATE, ZLIB or GZip stream (the first member, as
 * md_gz_higher_uncompress reads it): P >= 1 access points.  Point k is the START OF A DEFLATE BLOCK: `bit` counts from
 * src[0] (the frame's header included), `out` is the offset of the block's first byte in the inflated output, and the
 * point carries the min(32768, out) bytes of output in front of it - the window a decoder needs to start there.  Point 0
 * is the first block (out 0, no window); bits and outs increase strictly; no two points are closer than `span` bytes of
 * output.  Piece k is what lies between point k and point k + 1 (the last piece runs to the end of the stream).
 *
 * md_inflate_index_build decodes the stream ONCE (pieces that go to one pair of wavefronts may be decoded again: one that
 * held no complete block with half as much input again, the one that holds the stream's end cut by bisection), in pieces of bounded size (as md_inf_decode does: a long piece by the
 * whole device, "inflate_parallel_min", any other by one pair of wavefronts), so a stream of any length needs a piece's
 * worth of device memory; MD_MAX_INFLATE_IN does not bound src_len here.  The return value is the stream's status as
 * md_de_higher_uncompress / md_zl_higher_uncompress / md_gz_higher_uncompress report it (header, body, trailer); any
 * status but MD_OK leaves *idx = NULL.  dst == NULL: the output is not wanted and is not copied to the host (only the
 * windows are); otherwise dst receives it and MD_UNEXPECTED_END_OF_OUTPUT applies when dst_cap is short.  span = 0 means
 * 1 MiB; span < 4096 is MD_E_INVALID_ARGUMENT.  Every block start the decode learns is considered in order and kept when
 * it lies at least `span` bytes of output behind the last one kept.  info may be NULL.  The index is the caller's
 * (md_inflate_index_free) and does not refer to the context or to src.
 *
 * The serialised form (md_inflate_index_save / _load; _load takes no context and touches no device), little-endian:
 *   offset  0  8 bytes  "MDZINDEX"
 *           8  u32      version, 1
 *          12  u32      format (MD_FORMAT_*)
 *          16  u64      src_len      bytes of the src the index was built from
 *          24  u64      header_len   bytes in front of the DEFLATE body (0 raw, 2 ZLIB, >= 10 GZip)
 *          32  u64      consumed     bytes of src the stream used, trailer included
 *          40  u64      size         inflated bytes
 *          48  u64      span
 *          56  u64      points       P
 *          64  u32      checksum     Adler-32 of the output (raw, ZLIB) or its CRC-32 (GZip)
 *          68  u32      0
 *          72  P records of 24 bytes: u64 bit, u64 out, u32 win_len, u32 0
 *   72 + 24 P  the windows back to back, win_len bytes each; the blob ends with the last one.
 * md_inflate_index_load returns MD_INVALID_INDEX unless: magic, version and both zero words are as above; format is one of
 * the three; consumed <= src_len < 2^60, header_len + trailer (0 / 4 / 8) <= consumed, header_len fits the format;
 * span >= 4096; P >= 1; point 0 is (8 header_len, 0); bits and outs increase strictly; win_len == min(32768, out);
 * 8 header_len <= bit < 8 (consumed - trailer): inside the body; out < size, or out == size for the last point (an empty block at the very end);
 * and the blob is exactly 72 + 24 P + the sum of win_len bytes long.
 *
 * md_inflate_index_read: n ranges [off[i], off[i] + len[i]) of the inflated output into dst + dst_off[i] (host pointers;
 * copy in, kernels, copy out, synchronise).  src_len other than the index's: MD_INVALID_INDEX as the call's return value;
 * a range with off + len > size: MD_E_INVALID_ARGUMENT; len 0 is fine.  Otherwise MD_OK and status[i] per range.  The call
 * works in rounds bounded by md_set_option "index_read_workspace", each round ONE inflate launch
 * (md_inflate_continue_batch_device): the device marks the pieces any range touches - every piece is decoded once, however
 * many ranges touch it - and writes the launch's descriptors; only the compressed bytes of those pieces and their windows
 * are copied to the device; a piece is GOOD only if its last complete block ends exactly on the next point (bit and output
 * offset), or, for the last piece, the final block ended and the output is exactly size - out; the good pieces' bytes are
 * gathered into the ranges.  status[i] is MD_OK when every piece of range i is good, otherwise the first failing piece's
 * inflate status, or MD_INVALID_INDEX where the decode itself found nothing wrong.  A failing range leaves its dst bytes
 * unspecified (as it stands nothing is written to them); other ranges are not affected.  The bytes are not checked against a checksum: a src that differs from the
 * indexed one in a way that moves no block boundary is not noticed.
 * md_inflate_index_last: the counts of the context's last md_inflate_index_read - pieces decoded, inflate launches, bytes
 * of src and of windows copied to the device, bytes of piece scratch (summed over the rounds). */
typedef struct md_inflate_index md_inflate_index;
typedef struct md_inflate_index_info {
  int32_t format;
  uint32_t checksum;
  uint64_t src_len, header_len, consumed, size, span, points;
} md_inflate_index_info;
typedef struct md_inflate_index_stats {
  uint64_t pieces, launches, bytes_in, bytes_windows, bytes_scratch;
} md_inflate_index_stats;
int md_inflate_index_build(md_ctx *ctx, int format, const uint8_t *src, size_t src_len, uint64_t span, uint8_t *dst,
                           size_t dst_cap, md_inflate_index **idx, md_inflate_index_info *info);
int md_inflate_index_get(const md_inflate_index *idx, md_inflate_index_info *info);
/* the first `cap` points; bit / out may be NULL when cap is 0 */
int md_inflate_index_points(const md_inflate_index *idx, uint64_t *bit, uint64_t *out, size_t cap);
size_t md_inflate_index_save_size(const md_inflate_index *idx); /* 0 for NULL */
/* MD_UNEXPECTED_END_OF_OUTPUT when cap is short; *len = the bytes written (or needed) */
int md_inflate_index_save(const md_inflate_index *idx, uint8_t *buf, size_t cap, size_t *len);
int md_inflate_index_load(const uint8_t *buf, size_t len, md_inflate_index **idx);
void md_inflate_index_free(md_inflate_index *idx);
int md_inflate_index_read(md_ctx *ctx, const md_inflate_index *idx, const uint8_t *src, size_t src_len, size_t n,
                          const uint64_t *off, const uint64_t *len, uint8_t *dst, const uint64_t *dst_off, int32_t *status);
int md_inflate_index_last(const md_ctx *ctx, md_inflate_index_stats *stats);

/* ---- Random access to a blocked GZip file (BGZF: bgzip, htslib, .bam, .vcf.gz, tabix) ------------------------------------
 * Such a file exists so that a reader fetches a few kilobytes out of gigabytes: every member is a complete stream of at
 * most 64 KiB with its own CRC-32 and says how long it is, so a read needs no windows and can check every byte it returns.
 *
 * md_bgzf_index: src_len and, for the file's M members, M + 1 pairs (c_off[k], u_off[k]), all on the host.  c_off[0] =
 * u_off[0] = 0; member k is src[c_off[k], c_off[k + 1]) and its output is bytes [u_off[k], u_off[k + 1]) of the file's;
 * c_off[M] is the byte behind the last member (<= src_len: NUL padding may follow) and u_off[M] = size.  Empty members -
 * the 28-byte EOF marker, or one in the middle - are ordinary entries with u_off[k + 1] == u_off[k].
 *
 * md_bgzf_index_build runs the member scan of md_gz_members_scan (nothing is decoded) and keeps its table.  A file that is
 * not indexed in that call's sense: MD_INVALID_INDEX and *idx = NULL.  An empty src gives an index of 0 members.
 *
 * md_bgzf_index_from_gzi takes no context and touches no device.  The .gzi layout is htslib's, written here from its
 * description (nobody could run htslib against it): a little-endian u64 count N, then N pairs of u64 (compressed offset,
 * uncompressed offset); the first block (0, 0) is not stored.  MD_INVALID_INDEX unless the blob is exactly 8 + 16 N bytes,
 * the compressed offsets increase strictly (from the implied 0) and are < src_len, the uncompressed offsets do not decrease,
 * and no member's output is more than 1 032 times its length (DEFLATE's limit: it bounds what a read allocates).  .gzi
 * says neither where the file ends nor how large its output is, so the host completes the table from src: from the last
 * entry on (offset 0 when N is 0) it follows the BSIZE fields member by member - the member scan's rule for a member: 1f 8b
 * 08, FEXTRA, a BC subfield of length 2 whose BSIZE + 1 fits the header and src - to the end of src or to NUL padding that
 * reaches it, and takes each ISIZE from its trailer; whether the writer of the .gzi listed the EOF marker does not matter.
 * Anything that does not chain to the end: MD_INVALID_INDEX.  The entries in front of the last are not compared with src
 * here: a read checks every member it decodes against them.
 * md_bgzf_index_to_gzi writes members 1 .. M - 1 in that layout (count 0 for an index of <= 1 member);
 * MD_UNEXPECTED_END_OF_OUTPUT when cap is short, *len = the bytes written (or needed) = md_bgzf_index_gzi_size.
 * from_gzi(to_gzi(x), src) reproduces x entry for entry.  md_bgzf_index_entries: the first `cap` of the M + 1 pairs.
 *
 * md_bgzf_read: n ranges [off[i], off[i] + len[i]) of the file's output into dst + dst_off[i] (host pointers; copy in,
 * kernels, copy out, synchronise).  src_len other than the index's: MD_INVALID_INDEX as the call's return value; a range
 * with off + len > size: MD_E_INVALID_ARGUMENT; len 0 is fine and touches nothing.  Otherwise MD_OK and status[i] per range.
 * md_bgzf_read_virtual: the same with BGZF virtual offsets, voff = c_off << 16 | offset in that member's output.  voff >> 16
 * must be some c_off[k] with k < M (binary search on the host) and voff & 0xffff at most that member's output length;
 * otherwise that range alone gets MD_INVALID_INDEX and the call is still MD_OK.  A valid one is the byte range that starts
 * at u_off[k] + (voff & 0xffff); it runs on into the following members.
 * The HOST plans, from the index alone: a binary search over u_off gives each range its first and last member with output,
 * the touched members are marked once however many ranges touch them (empty ones never), and they go in member order, in
 * rounds of as many as fit md_set_option "bgzf_read_workspace" (MiB of packed input plus output slots per round, 0 .. 2^20,
 * default 256; a member that alone needs more gets a round to itself; 0 = one member a round).  Per round only the touched
 * members' bytes are copied to the device, packed back to back (a run of consecutive members by one copy); nothing comes
 * back between the rounds.  On the device, per round: the header walk (RFC 1952, as md_gz_members_uncompress), ONE inflate
 * launch over the bodies, each into a slot of exactly the output length the index gives, CRC-32 and ISIZE per member, and
 * the member's verdict - the first of:
 *   the header's status
 *   the decoder's status         except MD_UNEXPECTED_END_OF_OUTPUT: the slot's size is the index's word, so running out of
 *                                it is MD_INVALID_INDEX unless the member's own ISIZE is that size (then MD_INVALID_SIZE)
 *   MD_INVALID_SIZE              the body did not end exactly at the trailer
 *   MD_INVALID_CHECKSUM, MD_INVALID_SIZE   the trailer's CRC-32, then its ISIZE, against the decoded bytes
 *   MD_INVALID_INDEX             the member is sound but not the one the index describes: the BSIZE + 1 of its BC subfield
 *                                is not the length the index gives, or its ISIZE is not the output length the index gives
 * and a gather of the good members' bytes into the ranges (one wavefront per range and 16 KiB).  status[i] is MD_OK when
 * every member of range i is good, otherwise the first failing member's verdict.  A failing range leaves its dst bytes
 * unspecified (as it stands nothing is written to them); other ranges are not affected: a damaged member never fails the
 * call.  The ranges' bytes are staged on the device as they lie in dst, max(dst_off + len) bytes.
 * md_bgzf_read_last: the counts of the context's last read - distinct members decoded, inflate launches, bytes of src
 * copied to the device, bytes of output slots (summed over the rounds). */
typedef struct md_bgzf_index md_bgzf_index;
typedef struct md_bgzf_index_info {
  uint64_t src_len, members, size;
} md_bgzf_index_info;
typedef struct md_bgzf_read_stats {
  uint64_t members, launches, bytes_in, bytes_scratch;
} md_bgzf_read_stats;
int md_bgzf_index_build(md_ctx *ctx, const uint8_t *src, size_t src_len, md_bgzf_index **idx);
int md_bgzf_index_from_gzi(const uint8_t *gzi, size_t gzi_len, const uint8_t *src, size_t src_len, md_bgzf_index **idx);
size_t md_bgzf_index_gzi_size(const md_bgzf_index *idx); /* 0 for NULL */
int md_bgzf_index_to_gzi(const md_bgzf_index *idx, uint8_t *buf, size_t cap, size_t *len);
int md_bgzf_index_get(const md_bgzf_index *idx, md_bgzf_index_info *info);
/* c_off / u_off may be NULL when cap is 0 */
int md_bgzf_index_entries(const md_bgzf_index *idx, uint64_t *c_off, uint64_t *u_off, size_t cap);
void md_bgzf_index_free(md_bgzf_index *idx);
int md_bgzf_read(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t src_len, size_t n, const uint64_t *off,
                 const uint64_t *len, uint8_t *dst, const uint64_t *dst_off, int32_t *status);
int md_bgzf_read_virtual(md_ctx *ctx, const md_bgzf_index *idx, const uint8_t *src, size_t src_len, size_t n, const uint64_t *voff,
                         const uint64_t *len, uint8_t *dst, const uint64_t *dst_off, int32_t *status);
int md_bgzf_read_last(const md_ctx *ctx, md_bgzf_read_stats *stats);

/* ---- git packfiles (pack v2 / v3 with an idx v2 beside it): every object in one batch, deltas applied -------------------------
 * A pack holds n objects, each a header and one zlib stream; most are deltas (copy / insert instructions against a base
 * object that may itself be a delta).  The .idx beside the pack says where each object begins.
 *
 * md_pack_index reads an idx version 2 on the HOST: it takes no context and touches no device.  It is called twice, like
 * md_zip_directory: first with cap = 0 for info->n, then with room for n entries (at most cap are written), in the idx's
 * order - ascending by name.  Every read is checked against idx_len.  Layout: ff 74 4f 63, u32 version (big-endian, as all
 * of it), 256 fan-out counts, n 20-byte names, n CRC-32s of the packed objects, n 31-bit offsets whose most significant
 * bit marks an index into the table of m 64-bit offsets that follows, the pack's 20-byte checksum, the idx's own.
 *   MD_PACK_UNSUPPORTED   no magic (idx version 1), or a version other than 2
 *   MD_INVALID_INDEX      a file too short for its magic, its fan-out or what n implies; a fan-out that decreases; names
 *                         that do not ascend strictly or do not lie where the fan-out says; an escape that points outside
 *                         the 64-bit table; a length other than 8 + 1024 + 28 n + 8 m + 40, m = the number of escapes
 * A SHA-256 repository's idx has 32-byte names and cannot be told apart from the idx alone: it ends as MD_INVALID_INDEX by
 * the length rule.  MD_E_INVALID_ARGUMENT: NULL idx or info, NULL entries with cap != 0.
 *
 * md_pack_open builds the table of all n objects (host pointers; copy in, kernels, copy out, synchronise) and keeps it in
 * the handle.  Call-level checks first: the pack begins with "PACK" (else MD_INVALID_PACK) and version 2 or 3 (else
 * MD_PACK_UNSUPPORTED); its object count is the idx's n and its last 20 bytes are the idx's pack checksum (else
 * MD_INVALID_INDEX: a 20-byte compare, nothing is hashed); every offset of the idx lies behind the pack's header and in
 * front of its trailer, and no two are equal (else MD_INVALID_INDEX).  Then, with the idx's offsets sorted on the host - object i is
 * pack[off_i, the next offset), the last one ends at pack_len - 20 -, per object:
 *  - the header (one thread each): type and size varint.  Types 1-4, 6, 7; type 0 or 5, a size beyond 64 bits or a header
 *    that passes the object's end: MD_INVALID_PACK.  OFS_DELTA: the offset varint v (+1 per continuation byte); the base is
 *    the object at off_i - v; v = 0, v > off_i or no object there: MD_INVALID_PACK.  REF_DELTA: the base's name, looked up
 *    in the idx; absent: MD_PACK_MISSING_BASE;
 *  - depth and the chain's root by pointer jumping over the base links, ceil(log2 n) + 1 launches, no lane waits for
 *    another: what has not reached a root by then is on a REF_DELTA cycle or hangs off one: MD_INVALID_PACK;
 *  - a delta's final size: the delta payloads are inflated (rounds of "pack_workspace"; the status rules of md_pack_read's
 *    inflate step apply) and the two varints in front of the instructions are read: base size and result size.  One that
 *    does not fit 64 bits or passes the payload's end: MD_INVALID_DELTA; a base size that is not the base's final size:
 *    MD_INVALID_DELTA.  The payloads are not kept;
 *  - a delta with an object that failed above somewhere on its chain of bases: MD_INVALID_PACK_BASE (this last step walks
 *    the table on the host, in order of depth).
 * The type of a delta is its root's.  md_pack_get / md_pack_objects (idx order; objs may be NULL when cap is 0) / md_pack_find
 * (host, by the fan-out; the index or -1) report the table; md_pack_free frees it.
 *
 * md_pack_read decodes the objects select[0 .. nselect) - indices in idx order, repeats allowed; select == NULL: all n -
 * into dst, object j at out_off[j] (k + 1 words; sizes are the table's whatever the status).  If they need more than
 * dst_cap the call returns MD_UNEXPECTED_END_OF_OUTPUT with res->written = the room needed and launches nothing.  Every
 * object has its own status; a damaged object touches neither the bytes nor the status of another, except that a delta
 * whose chain of bases holds a failed object gets MD_INVALID_PACK_BASE.  An object that failed in md_pack_open keeps that
 * status and is not decoded.  pack must be the pack the table was built from: another length or trailer is MD_INVALID_INDEX
 * as the call's return value; a selected index >= n or an unknown bit in flags (one that is neither MD_PACK_VERIFY_CRC
 * nor MD_PACK_VERIFY_NAME) is MD_E_INVALID_ARGUMENT.  Steps:
 *  - plan (host, the table alone): the selected objects and the closure of their bases, each once a round;
 *  - memory: a selected object that is no delta decodes straight into its place; a selected delta's result is applied
 *    straight into its place; payloads, bases and intermediate results go to scratch.  Selected objects are taken into a
 *    round while its scratch fits "pack_workspace"; an object whose own chain needs more gets MD_E_OUT_OF_MEMORY as its
 *    status (with "pack_workspace" = 0 nothing is refused: one selected object a round);
 *  - inflate: ONE launch per round over every needed zlib stream, each into exactly its header size.  MD_INVALID_SIZE: the
 *    stream did not consume its whole packed length (git leaves no byte between objects), did not fill its size or holds
 *    more; MD_INVALID_CHECKSUM: the zlib trailer; any other status is the decoder's;
 *  - verify, with MD_PACK_VERIFY_CRC in flags: the idx's CRC-32 over each needed object's packed bytes, header included;
 *    a mismatch is MD_INVALID_CHECKSUM;
 *  - apply: one launch per depth 1, 2, .. of the round, ordered by the stream alone; one wavefront per delta.  An opcode
 *    with bit 7 set copies from the base: its low 7 bits say which of 4 offset and 3 size bytes follow, size 0 means
 *    0x10000; an opcode 1 .. 127 inserts that many bytes that follow it.  MD_INVALID_DELTA: opcode 0, a copy that leaves
 *    the base, output beyond the result size, a payload that ends inside an instruction or with the result size not
 *    reached, a base-size or result-size varint other than the table's.  A failing object leaves its bytes unspecified.
 * md_pack_last: rounds, inflate launches, apply launches, objects decoded (a base decoded in two rounds counts twice) and
 * bytes of the pack copied in, of the context's last md_pack_read, and the device time its apply launches took (two events
 * a round around them, read when the call has synchronised).
 * Limits per object: a packed length above MD_MAX_INFLATE_IN or a size above MD_MAX_STREAM is MD_E_INVALID_ARGUMENT as
 * that object's status.
 *
 * Names.  An object's name is SHA-1("<type> <size>\0" + content), type being "commit", "tree", "blob" or "tag" - a delta's is
 * its root's - and size the content's length in decimal.  With MD_PACK_VERIFY_NAME in flags a hash pass (md_sha1_batch_*'s
 * kernel) runs in every round behind the round's last apply launch, over every object of the round - the selected ones and
 * the bases alike - where its bytes stand, and the 20 bytes are compared with the idx's name on the device.  The rules, per
 * object and in this order: a status of its own from the steps above stays (with both flags a CRC failure comes first, as
 * without names); else a failed object anywhere on its chain of bases - failed by name included - is MD_INVALID_PACK_BASE;
 * else a name other than the idx's is MD_INVALID_CHECKSUM (the CRC rule's status for "the idx says otherwise": there is no
 * status of its own).  A failing object's bytes are unspecified; every other object's bytes are what they are without the
 * flag.  md_sha1_last has the hash passes' counts and device time, summed over the rounds of the call.
 *
 * md_pack_verify is md_pack_read without output: the same plan, rounds and statuses for the same flags, but the selected
 * objects stand in the round's scratch, so "pack_workspace" cuts the rounds with a selected object's own size counted (and
 * an object may get MD_E_OUT_OF_MEMORY here that a read has room for), a repeated selection costs no copy, and nothing
 * comes back but the statuses: res->written is 0.  With flags = 0 it still says which objects decode.
 *
 * md_pack_check_trailers runs on the HOST, without a context: *pack_ok = the pack's last 20 bytes are the SHA-1 of all that
 * is in front of them, *idx_ok the same for the idx (one serial message each: not a shape for the device).  An idx shorter
 * than an empty idx (8 + 1024 + 40 bytes) is MD_INVALID_INDEX, a pack shorter than an empty pack (32) MD_INVALID_PACK, and
 * neither flag is written; NULL pointers are MD_E_INVALID_ARGUMENT.
 * Out of scope (writing packs: md_pack_write below): idx v1, .rev, multi-pack-index, bitmaps, the SHA-256 object
 * format, SHA-1 collision detection, hashing the trailers on the device, completing a thin pack from another, objects above
 * MD_MAX_STREAM, handing one very long object to the whole-chip decoder. */
#define MD_PACK_VERIFY_CRC 1u
#define MD_PACK_VERIFY_NAME 2u
#define MD_PACK_NO_BASE 0xffffffffffffffffull
typedef struct md_pack_index_entry {
  uint64_t offset;
  uint32_t crc32;
  uint8_t name[20];
} md_pack_index_entry;
typedef struct md_pack_index_info {
  uint64_t n;
  int has_64bit_table;
  uint8_t pack_checksum[20];
} md_pack_index_info;
int md_pack_index(const uint8_t *idx, size_t idx_len, md_pack_index_info *info, md_pack_index_entry *entries, size_t cap);
typedef struct md_pack md_pack;
typedef struct md_pack_info {
  uint64_t n, deltas, max_depth, total_size, failed;
} md_pack_info;
typedef struct md_pack_object {
  uint64_t size, offset, packed_len, base; /* base: the index of the delta's base, MD_PACK_NO_BASE if none (or not found) */
  uint32_t depth, type;                    /* type: 1 commit, 2 tree, 3 blob, 4 tag - the chain's root's; 0 if unknown */
  int32_t status;
  uint8_t name[20];
} md_pack_object;
typedef struct md_pack_result {
  size_t entries, failed;
  uint64_t written;
} md_pack_result;
typedef struct md_pack_stats {
  uint64_t rounds, inflate_launches, apply_launches, objects, bytes_in;
  uint64_t apply_ns; /* device time from the first apply launch of a round to the end of its last, summed over the rounds */
} md_pack_stats;
int md_pack_open(md_ctx *ctx, const uint8_t *pack, size_t pack_len, const uint8_t *idx, size_t idx_len, md_pack **p);
int md_pack_get(const md_pack *p, md_pack_info *info);
int md_pack_objects(const md_pack *p, md_pack_object *objs, size_t cap);
int64_t md_pack_find(const md_pack *p, const uint8_t *name20);
void md_pack_free(md_pack *p);
int md_pack_read(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, const uint64_t *select, size_t nselect,
                 unsigned flags, uint8_t *dst, size_t dst_cap, uint64_t *out_off, int32_t *status, md_pack_result *res);
int md_pack_last(const md_ctx *ctx, md_pack_stats *stats);
int md_pack_verify(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, const uint64_t *select, size_t nselect,
                   unsigned flags, int32_t *status, md_pack_result *res);
int md_pack_check_trailers(const uint8_t *pack, size_t pack_len, const uint8_t *idx, size_t idx_len, int *pack_ok, int *idx_ok);

/* ---- git packs: the idx from the pack alone (index-pack; csrc/pack_build_kernels.hip, csrc/pack_build.hpp) ------------------
 * A pack that came over the wire (git fetch, a bundle, git pack-objects --stdout) has no idx.  md_pack_index_build writes
 * the idx version 2 that git index-pack writes for it, byte for byte, so that md_pack_open can follow with no git in between.
 *
 * Call-level checks, as md_pack_open's: "PACK" and at least 32 bytes, else MD_INVALID_PACK; version 2 or 3, else
 * MD_PACK_UNSUPPORTED; a flag other than MD_PACK_BUILD_CHECK_TRAILER is MD_E_INVALID_ARGUMENT.  With that flag the HOST hashes
 * pack[0, pack_len - 20) (one serial message, under the device's count pass) and compares it with the trailer: a mismatch
 * is MD_INVALID_CHECKSUM as the call's return value, res->bad_offset = pack_len - 20.  Without it the trailer is copied into
 * the idx as it is.
 *
 * Where the objects begin.  Object k + 1 begins where the zlib stream of object k ends, which only a decoder knows.  So
 * every position z of [12, pack_len - 20 - 6] whose two bytes pass the decoder's own test of a zlib header
 * (((cmf << 8) + flg) % 31 == 0 and (cmf & 15) == 8) is a CANDIDATE; they are marked and compacted on the device and ONE
 * md_inflate_sizes_batch_device launch (MD_FORMAT_ZLIB, in_len = min(pack_len - 20 - z, MD_MAX_INFLATE_IN)) says of every one
 * what a stream that began there would consume and inflate to.  Candidates are stream starts, not header starts: a size
 * varint of two or more bytes almost always has a second start one byte in that parses and leads to the same stream.
 * In compressed bytes about one position in 496 is a candidate (132 of the 65 536 pairs of bytes pass).  The host then walks from byte 12: it parses the header it
 * stands on (type, size varint, an OFS_DELTA's distance or a REF_DELTA's 20 bytes; the bound is pack_len - 20), finds the
 * stream's z among the candidates and steps to z + consumed.  A false candidate is never on this chain - the chain is a
 * function of the pack's bytes - it only costs time.  The walk stops, and the call returns MD_INVALID_PACK with
 * res->bad_offset = where it stood, when no z can be told (type 0 or 5, a size varint beyond 64 bits, an OFS_DELTA distance
 * beyond 2^63, a header that passes the end), z is no candidate, z's count did not end MD_OK (res->bad_status has its
 * status), the chain ends anywhere but on pack_len - 20 (bad_offset = the first byte that is no object's), or it finds
 * fewer objects than the pack's header states (bad_offset = pack_len - 20).  It goes on past an object whose stream
 * inflates to another size than its header states and past an OFS_DELTA whose distance is 0, beyond its own offset or to
 * no object's start: those get statuses of their own below.
 * After the walk res->n and res->idx_len are known and offsets[0 .. min(cap, n)) are written, in pack order.  An idx_cap
 * below res->idx_len returns MD_UNEXPECTED_END_OF_OUTPUT before anything further is launched.
 *
 * Names, CRCs and bases.  The CRC-32 of every object's packed bytes is one md_crc32 launch.  The names come in GENERATIONS,
 * as in git index-pack, because a REF_DELTA names its base by the SHA-1 nobody knows yet.  A generation builds md_pack_open's
 * table from the offsets and the names known so far - a REF_DELTA whose base is not among them is MD_PACK_MISSING_BASE for
 * now and what hangs off it MD_INVALID_PACK_BASE - and then runs md_pack_verify's rounds ("pack_workspace") over every object
 * that table calls sound and that has no verdict yet, with the hash pass behind each round's last apply launch.  The pass
 * writes the name of an object that has none and compares the name of one that has (a base decoded again).  The next
 * generation looks the pending REF_DELTAs up among the new names.  The loop ends when a generation names nothing or
 * nothing is pending.  A pack as git writes it to disk has no REF_DELTA and takes ONE generation; every REF link along a
 * chain costs one more (a fan of REF_DELTAs on one base: 2; a chain of 64 alternating OFS and REF: 33).  That is accepted.
 * Per object, in this order: MD_INVALID_SIZE (the stream does not inflate to the header's size), MD_INVALID_CHECKSUM (the
 * Adler-32) and the decoder's own statuses by md_pack_read's rules; MD_INVALID_PACK for the OFS_DELTA faults above;
 * MD_INVALID_DELTA by the apply kernel's rules; MD_PACK_MISSING_BASE for a REF_DELTA whose base never got a name - a thin
 * pack, and also a REF_DELTA cycle, which cannot be told from one here - and MD_INVALID_PACK_BASE for what hangs off a failed
 * object; MD_E_INVALID_ARGUMENT for the size limits (MD_MAX_INFLATE_IN / MD_MAX_STREAM); MD_INVALID_PACK for the later, by
 * offset, of two objects with one name (git index-pack --strict refuses those, and md_pack_index an idx whose names do not
 * ascend strictly: no idx is written here that is not read here).
 * status[0 .. min(cap, n)) is written in pack order (offsets and status may be NULL with cap 0).  If any object failed the
 * call returns the status of the first failing one in pack order, res->failed counts them, res->bad_offset is that object's
 * offset and no byte of idx is written.  Otherwise MD_OK and idx[0, res->idx_len).  An empty pack gives the idx of 1 072 bytes.
 *
 * md_pack_index_write (HOST, no context) is the inverse of md_pack_index: entries in any order are sorted by name (two equal
 * names: MD_INVALID_INDEX; more than 2^32 - 1 entries: MD_E_INVALID_ARGUMENT), then magic, version 2, fan-out, names, CRCs,
 * 31-bit offsets - one above 0x7fffffff escapes into the 64-bit table, in idx order, as git does -, the pack's checksum
 * and the idx's own SHA-1.  *idx_len = 8 + 1024 + 28 n + 8 m + 40; an idx_cap below it returns MD_UNEXPECTED_END_OF_OUTPUT
 * with *idx_len set and nothing written.  For any valid idx, writing what md_pack_index read gives the same bytes.
 *
 * md_pack_build_last: of the context's last md_pack_index_build the candidates, the generations, and summed over their
 * reads the rounds, inflate launches, apply launches and objects decoded; bytes of the pack copied in.
 * Known limit: a crafted pack can make the count pass slow - a stored blob full of nested zlib streams makes every one of
 * them a candidate that is walked to its end - never wrong.  There is no defence.
 * Out of scope: completing a thin pack (--fix-thin), .rev, idx v1, SHA-256, objects beyond MD_MAX_INFLATE_IN /
 * MD_MAX_STREAM, the slow crafted pack. */
#define MD_PACK_BUILD_CHECK_TRAILER 1u
typedef struct md_pack_build_result {
  uint64_t n, failed, idx_len, bad_offset; /* bad_offset: MD_PACK_NO_BASE if none */
  int32_t bad_status;
} md_pack_build_result;
typedef struct md_pack_build_stats {
  uint64_t candidates, generations, rounds, inflate_launches, apply_launches, objects, bytes_in;
} md_pack_build_stats;
int md_pack_index_write(const md_pack_index_entry *entries, size_t n, const uint8_t pack_checksum[20], uint8_t *idx, size_t idx_cap,
                        size_t *idx_len);
int md_pack_index_build(md_ctx *ctx, const uint8_t *pack, size_t pack_len, unsigned flags, uint8_t *idx, size_t idx_cap,
                        uint64_t *offsets, int32_t *status, size_t cap, md_pack_build_result *res);
int md_pack_build_last(const md_ctx *ctx, md_pack_build_stats *stats);

/* ---- SHA-1 of many buffers: one message a lane, 64 a wavefront (csrc/sha1_kernels.hip) ---------------------------------------
 * SHA-1 is serial inside a message, so one long message is hashed by one lane, at tens of MB/s; the batch is what is fast.
 * Message i is data[off[i], off[i] + len[i]), at any byte address; the kernel reads no dword that holds no byte of a
 * message, so the buffer may end with the last one.  type == NULL or type[i] == 0: the SHA-1 of the bytes as they are;
 * type[i] = 1 .. 4: the git object name of a commit / tree / blob / tag with that content (the header "<type> <size>\0" is
 * the kernel's own).  digest receives 20 bytes a message.  n == 0 is MD_OK and launches nothing.
 *
 * One launch advances every message by at most "sha1_launch_blocks" blocks of 64 bytes (md_set_option; 1 .. 2^24), the
 * state waits in device memory between launches: no launch runs longer than that many blocks take, whatever the lengths.
 *
 * md_sha1_batch_host (host pointers; copy in, kernels, copy out, synchronise): every range is checked against data_len and
 * every length against MD_MAX_STREAM, a type above 4 is refused: MD_E_INVALID_ARGUMENT, as are NULL data (with data_len
 * != 0), off, len or digest.  The host knows the lengths: it orders the messages longest first, so that the lanes of a
 * wavefront are of similar length, and launches ceil(blocks of the longest / "sha1_launch_blocks") times over a shrinking
 * prefix of that order, nothing read back in between.
 *
 * md_sha1_batch_device (device pointers, asynchronous on the context's stream like md_crc32_batch_device): the lengths
 * live on the device, so the launch count comes from an extra argument, max_len: the caller's bound on the longest
 * len[i], at most MD_MAX_STREAM.  Every launch covers all n messages, in index order; a message that is through drops out
 * at once.  The caller's duties, which the host cannot check: len[i] <= max_len (a longer message is not finished and its
 * digest is not written; no byte outside its range is read whatever it says) and type[i] <= 4 (a larger one is hashed as 0).
 *
 * md_sha1_last: messages, blocks of 64 bytes (header and padding included), launches and the device time between two
 * events around them, of the context's last batch - that of md_sha1_batch_*, or the hash passes of the last md_pack_read /
 * md_pack_verify with MD_PACK_VERIFY_NAME, summed over its rounds.  After the device form it waits for the second event. */
typedef struct md_sha1_stats {
  uint64_t messages, blocks, launches, device_ns;
} md_sha1_stats;
int md_sha1_batch_device(md_ctx *ctx, size_t n, const uint8_t *d_data, const uint64_t *d_off, const uint64_t *d_len,
                         const uint8_t *d_type, uint64_t max_len, uint8_t *d_digest);
int md_sha1_batch_host(md_ctx *ctx, size_t n, const uint8_t *data, size_t data_len, const uint64_t *off, const uint64_t *len,
                       const uint8_t *type, uint8_t *digest);
int md_sha1_last(const md_ctx *ctx, md_sha1_stats *stats);

/* ---- git packs: writing one, the deltas made by a batched kernel (csrc/pack_write_kernels.hip, csrc/pack_write.hpp) ----------
 * THE DELTA of a target T (nt bytes) against a base B (nb bytes) is defined here byte for byte.  The bytes are this
 * library's own, not git diff-delta's; every reader of git's delta format applies them (md_pack_read's apply step among them).
 * They are a pure function of B and T.
 *  Index of the base.  Block j is B[16 j, 16 j + 16) for j < nb / 16 (integer division).  Its hash: the four little-endian
 *   32-bit words w0 .. w3 of the block, x = 0, then x = (x + w) * 0x9E3779B1 mod 2^32 for each word in turn.  k is the smallest
 *   integer >= 10 with 2^k >= 2 * (nb / 16); slot = x >> (32 - k).  A slot holds the LOWEST block index that maps to it; a
 *   block that loses its slot is never found: that costs size, never correctness.
 *  Parse, greedy.  lit is the end of the previous copy, 0 at the start.  (1) Find the smallest p >= lit with p + 16 <= nt
 *   whose slot holds a block j with B[16 j, 16 j + 16) == T[p, p + 16).  (2) Forward: L = 16 + the common prefix of
 *   B[16 j + 16 ..) and T[p + 16 ..).  (3) Backward: e = the largest value with e <= p - lit, e <= 16 j and the e bytes in
 *   front of both places equal.  (4) T[lit, p - e) goes out as inserts, then a copy of (16 j - e, L + e); lit = p + L.
 *   (5) Behind the last match T[lit, nt) goes out as inserts.
 *  Encoding.  varint(nb) varint(nt) (7 bits a byte, least significant first), then the ops.  An insert has 1 .. 127 bytes: a
 *   run is cut into 127s with the rest last.  A copy longer than 0x10000 is cut into 0x10000s with the rest last.  A copy op
 *   is 0x80 | mask and only the NON-ZERO bytes of its 32-bit offset (mask bits 0 - 3) and 16-bit size (bits 4, 5); a size
 *   of exactly 0x10000 has no size byte (pack version 2 has no third size byte, bit 6 is never set).
 *
 * md_pack_delta_batch_device makes n deltas in one launch (two with the index), asynchronously on the context's stream.
 * `pairs` is a HOST array - the host sizes the bases' tables from the lengths and finds the DISTINCT bases: a base that
 * several targets share (same base_off and base_len) is indexed once -; d_src, d_out, d_out_len and d_status are device
 * pointers.  Pair i: base = d_src[base_off, base_off + base_len), target = d_src[tgt_off, tgt_off + tgt_len), at any byte
 * address, overlapping or not; the delta goes to d_out[out_off, out_off + out_cap).  status[i] = MD_OK and out_len[i] = its
 * length, or, as soon as an op would pass out_cap, MD_UNEXPECTED_END_OF_OUTPUT and out_len[i] = 0 (the bytes of the room
 * are then unspecified; nothing outside it is written).  Pairs are independent.  The caller's duties, which the host cannot
 * check: the ranges lie in d_src and d_out, the rooms do not overlap.  md_pack_delta_batch_host (host pointers; copy in,
 * kernels, copy out, synchronise) checks every range against src_len and out_bytes; it writes out[0, max(out_off + out_cap))
 * as a whole, so what lies between the rooms is unspecified too.
 * MD_E_INVALID_ARGUMENT: a NULL pointer, n above 2^31 - 16, base_len or tgt_len above MD_MAX_STREAM, a range that overflows
 * (host form: that leaves its buffer).  n == 0 is MD_OK and launches nothing.  The tables take 4 * 2^k bytes a distinct base
 * - between half the base's size and its size, 4 KiB at the least - in one workspace; one that cannot be allocated is
 * MD_E_OUT_OF_MEMORY: this first version has no rounds.
 * Known limit: one wavefront makes one delta, so one very large target is slow (it scans 64 positions a step); many pairs
 * are what is fast.
 *
 * md_pack_write writes the pack (version 2, OFS_DELTA only) of n objects in INPUT order.  Object i is src[off, off + len)
 * of type 1 .. 4; base is an EARLIER index whose content its delta may be made against, or MD_PACK_NO_BASE.  The caller
 * chooses the bases, or has md_pack_choose_bases (below) choose them.  MD_E_INVALID_ARGUMENT as the call's return value:
 * NULL pointers, base >= i, a base of another type, a type outside 1 .. 4, len > MD_MAX_STREAM, an object beyond src_len, an
 * unknown flag, a level outside 0 .. 9, n above 2^31 - 16.  Steps: copy in; the names of all objects by one
 * md_sha1_batch_device; the deltas - tried iff a base is given, len >= 64 and the base's len >= 16, with out_cap = len / 2 - 20 -
 * always against the base's CONTENT, so all pairs are independent and go in one launch; the delta lengths are read back and
 * the host decides in index order: a delta is KEPT iff it fitted and its chain of kept deltas stays within max_depth (0: no
 * limit); an object whose delta is dropped is written whole and counts as depth 0 for what hangs off it.  Then ONE
 * md_deflate_batch_device (MD_FORMAT_ZLIB, the parameters md_zip_compress derives from `level`) over all payloads - a kept
 * delta's payload is the delta, otherwise the content -, the lengths are read back, the host walks offsets and headers
 * (an OFS_DELTA's distance varint depends on the offsets in front of it), a kernel places every header and stream, one
 * CRC-32 launch runs over the packed objects, the pack is copied out and the HOST hashes the trailer (one serial message, as
 * in md_pack_check_trailers).  MD_PACK_WRITE_NO_DELTA in flags ignores the bases.
 * entries[i] = {offset, crc32, name} in input order, ready for md_pack_index_write - which is the call that reports two
 * objects with one name (MD_INVALID_INDEX); md_pack_write writes both.  res: objects, deltas kept, the pack's deepest chain.
 * n == 0 gives the empty pack of 32 bytes.  A pack_cap below the pack's length returns MD_UNEXPECTED_END_OF_OUTPUT with
 * *pack_len = the need; nothing valid is promised in pack or entries.  md_pack_write_bound: room that always suffices (host
 * arithmetic: 32 + the sum of 16 + len + len / 8 + 256; 0 for NULL objs with n != 0 or a len above MD_MAX_STREAM; len + len / 8
 * + 256 is also the room every payload's stream gets on the device, and one that passed it would fail the call).  Workspace
 * that cannot be allocated is MD_E_OUT_OF_MEMORY: no rounds in this first version, everything of the call is resident at once.
 * md_pack_write_last: of the context's last md_pack_write or md_pack_delta_batch_* the pairs tried, the deltas kept, dropped by
 * size and dropped by depth, the bytes of payload before the deltas (the contents) and after (what went to the encoder), the
 * kernel launches of the call's own steps (index, delta, assembly, CRC; not those inside the SHA-1 and deflate batches) and
 * the device time of the index and delta launches (two events around them).  After the delta batch alone only pairs,
 * launches and delta_ns are set; after its device form the call waits for the second event.
 * Out of scope: REF_DELTA and thin packs, .rev and bitmaps, SHA-256, reusing an existing pack's deltas. */
#define MD_PACK_WRITE_NO_DELTA 1u
typedef struct md_pack_delta_pair {
  uint64_t base_off, base_len, tgt_off, tgt_len, out_off, out_cap;
} md_pack_delta_pair;
typedef struct md_pack_source {
  uint64_t off, len, base; /* base: an earlier index, or MD_PACK_NO_BASE */
  uint32_t type;           /* 1 commit, 2 tree, 3 blob, 4 tag */
} md_pack_source;
typedef struct md_pack_write_result {
  uint64_t n, deltas, max_depth;
} md_pack_write_result;
typedef struct md_pack_write_stats {
  uint64_t pairs, kept, dropped_size, dropped_depth, payload_before, payload_after, launches, delta_ns;
} md_pack_write_stats;
int md_pack_delta_batch_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint8_t *d_out,
                               uint64_t *d_out_len, int32_t *d_status);
int md_pack_delta_batch_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len, uint8_t *out,
                             size_t out_bytes, uint64_t *out_len, int32_t *status);
size_t md_pack_write_bound(size_t n, const md_pack_source *objs);
int md_pack_write(md_ctx *ctx, int level, unsigned flags, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src,
                  size_t src_len, uint8_t *pack, size_t pack_cap, size_t *pack_len, md_pack_index_entry *entries,
                  md_pack_write_result *res);
int md_pack_write_last(const md_ctx *ctx, md_pack_write_stats *stats);

/* ---- git packs: choosing the bases by content sketches (csrc/pack_search_kernels.hip, csrc/pack_search.hpp) -----------------
 * THE SKETCH of an object T of n bytes is defined here byte for byte.  For n >= 16 and every position p with p + 16 <= n,
 * h(p) is the delta index's block hash over T[p, p + 16): the four little-endian 32-bit words w0 .. w3, x = 0, then
 * x = (x + w) * 0x9E3779B1 mod 2^32 for each word in turn.  Feature i (i < 4) is
 *   F_i = min over p of ((h(p) XOR S_i) * 0x9E3779B1 mod 2^32),   S = {0, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F}.
 * An object shorter than 16 bytes has NO features: its four words are written as all ones, and it is never a candidate and
 * never a target - by its length, not by the stored value (an object of 16 bytes or more may have a feature of all ones).
 * The features are a pure function of the bytes.  Two objects that share most of their 16-byte windows share a feature with
 * a probability near the share, and each of the four independently.
 *
 * md_pack_sketch_device writes features[4 i .. 4 i + 3] of object i = d_src[off[i], off[i] + len[i]), at any byte address;
 * off and len are HOST arrays (the host cuts every object into segments of 4 096 positions, one wavefront each, so that
 * one very large object is not the call's length), d_src and d_features device pointers; one launch, asynchronous on the
 * context's stream.  Nothing outside an object's range is read.  md_pack_sketch_host: host pointers, ranges checked against
 * src_len, synchronous.  MD_E_INVALID_ARGUMENT: a NULL pointer, n above 2^31 - 16, len above MD_MAX_STREAM, a range that
 * overflows (host form: that leaves src), more than 2^31 - 16 segments.  n == 0 is MD_OK.
 *
 * md_pack_delta_sizes_device / _host take md_pack_delta_batch_*'s pairs and return exactly the out_len and status that call
 * returns for them - out_cap is the bound, the first op that would pass it ends the pair with MD_UNEXPECTED_END_OF_OUTPUT and
 * out_len 0 - and write no delta byte: out_off is ignored and there is no output buffer.  One launch (two with the index).
 * Arguments, errors and workspace as md_pack_delta_batch_*'s; md_pack_write_last counts the call as a delta batch.
 *
 * md_pack_choose_bases picks for every object of a batch the base that gives the smallest delta and returns the objects in
 * an order md_pack_write accepts as they stand.  objs[i] = {off, len, type} in src (host), base is ignored.
 *  1. Pack order: by (type, len descending, input index).  order[r] = the input index at rank r.
 *  2. Candidates of a target t: for each feature i the at most `window` objects nearest in front of t in pack order that
 *     have t's type and t's F_i; the union over the four features counts each object once (at most 4 * window).  A pair is
 *     scored iff md_pack_write would try it: the target's len >= 64, the base's len >= 16; its bound is len / 2 - 20.  A base
 *     always stands in front of its target, so no cycle can arise.
 *  3. Scores: one index launch over all distinct candidates, one md_pack_delta_sizes launch over all pairs.
 *  4. Choice, on the host in pack order: among the candidates whose delta fitted and whose depth is < max_depth (0: no
 *     limit) the smallest delta, on a tie the candidate earlier in pack order; depth[t] = depth[base] + 1.  No such
 *     candidate: the object is written whole, depth 0.
 *  5. sorted[r] = {off, len, type} of objs[order[r]] with base = the RANK of the chosen base or MD_PACK_NO_BASE.
 *     md_pack_write(.., max_depth, n, sorted, ..) with the same max_depth keeps every chosen delta: its deltas equal the
 *     bases chosen and it drops none.
 * MD_E_INVALID_ARGUMENT: NULL pointers, window outside 1 .. 64, n * 4 * window above 2^31 - 16, a type outside 1 .. 4, len >
 * MD_MAX_STREAM, an object beyond src_len.  n == 0 is MD_OK.  Everything of the call is resident at once (the objects,
 * then the candidates' tables): workspace that cannot be had is MD_E_OUT_OF_MEMORY, there are no rounds.
 * md_pack_search_last: of the context's last md_pack_choose_bases the objects with features, the pairs scored, the pairs that
 * fitted, the bases chosen, the kernel launches (sketch, index, size), the device time of the sketch launch and that of the
 * index and size launches (two events around each) and the host time of order, grouping and choice.
 * Out of scope: path-name heuristics, a device sort (the grouping is host sorts), rounds, other feature counts or seeds. */
typedef struct md_pack_search_stats {
  uint64_t featured, pairs, fitted, chosen, launches, sketch_ns, score_ns, host_ns;
} md_pack_search_stats;
int md_pack_sketch_device(md_ctx *ctx, size_t n, const uint64_t *off, const uint64_t *len, const uint8_t *d_src, uint32_t *d_features);
int md_pack_sketch_host(md_ctx *ctx, size_t n, const uint64_t *off, const uint64_t *len, const uint8_t *src, size_t src_len,
                        uint32_t *features);
int md_pack_delta_sizes_device(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *d_src, uint64_t *d_out_len,
                               int32_t *d_status);
int md_pack_delta_sizes_host(md_ctx *ctx, size_t n, const md_pack_delta_pair *pairs, const uint8_t *src, size_t src_len,
                             uint64_t *out_len, int32_t *status);
int md_pack_choose_bases(md_ctx *ctx, uint32_t window, uint32_t max_depth, size_t n, const md_pack_source *objs, const uint8_t *src,
                         size_t src_len, md_pack_source *sorted, uint64_t *order);
int md_pack_search_last(const md_ctx *ctx, md_pack_search_stats *stats);

/* ---- git packs: the object graph and what is reachable from roots (csrc/pack_graph_kernels.hip, csrc/pack_graph.hpp) ---------
 * A commit names a tree and parents, a tree names blobs and trees, a tag names a target.  md_pack_graph_build reads those
 * links on the device for every object of a table (md_pack_open) and keeps them as a graph; md_pack_reachable walks it.
 * Objects are indexed in idx order, as in md_pack_objects; an object's type is its root's.  Only commits (1), trees (2) and
 * tags (4) whose status in the table is MD_OK are decoded - by md_pack_verify's plan and rounds ("pack_workspace"), with
 * the bases they hang off - and parsed behind each round's last apply launch.  BLOBS ARE NEVER INFLATED: a blob's damage is
 * md_pack_verify's to find.  flags: 0 or MD_PACK_VERIFY_CRC (the read's meaning, for what is decoded); anything else is
 * MD_E_INVALID_ARGUMENT.  A pack other than the table's is MD_INVALID_INDEX, as in md_pack_read.  Limit: n < 2^31.
 *
 * An edge is (from, to, kind).  to: a uint32_t index, or MD_PACK_NO_LINK.  kind: one byte, its low bits one of
 *   1 COMMIT_TREE  2 COMMIT_PARENT  3 TAG_TARGET  4 TREE_BLOB  5 TREE_TREE  6 TREE_GITLINK
 * with two flags that may be or-ed in:
 *   0x40 MD_PACK_EDGE_ABSENT     the name is not among the pack's names; to is MD_PACK_NO_LINK
 *   0x80 MD_PACK_EDGE_MISTYPED   the name is found, the target's type is known (1 .. 4) and is not the type the edge calls
 *                                for: a tree for COMMIT_TREE and TREE_TREE, a commit for COMMIT_PARENT, a blob for TREE_BLOB,
 *                                the type its `type` line states for TAG_TARGET
 * A TREE_GITLINK is never looked up: to = MD_PACK_NO_LINK and neither flag.  A target whose own status is not MD_OK is still
 * linked to.  Edges stand in the object's own order - tree entries as they lie; a commit's tree, then its parents; a tag's
 * one target -, so the edge list is a function of the pack's bytes.
 *
 * The parse rules are those of git's readers (decode_tree_entry, parse_commit_buffer, parse_tag_buffer).
 * Tree of `size` bytes, at entry start s with rem = size - s: rem == 0 ends the tree (an empty tree is well formed, 0 edges);
 * otherwise rem >= 23 and byte[size - 21] == 0 are required; the mode is one or more bytes '0' .. '7' up to a space (an empty
 * mode or any other byte in front of the space is malformed), its value mode = (mode << 3) + digit in 32 bits, wrapping; the
 * name runs from behind the space to the first NUL and must not be empty; 20 name bytes follow and must fit in size; the next
 * entry starts behind them.  Kind by mode & 0170000 (git's canon_mode): 0100000 or 0120000 TREE_BLOB, 0040000 TREE_TREE
 * ("040000" with the leading zero is accepted), anything else - mode 0 and wrapped modes included - TREE_GITLINK.
 * Commit: size > 46, "tree ", 40 hex digits of either case, '\n' at byte 45.  At p = 46: while p + 47 < size and the bytes at
 * p are "parent ": size > p + 48, 40 hex digits and '\n' at p + 47 are required, else the commit is malformed; p += 48.
 * Nothing behind that is read: a parent line in the message is no parent; a commit that ends in "parent " + 40 hex without a
 * newline has no parent from that line, and with the newline and nothing behind it is malformed.
 * Tag: size >= 64; "object " + 40 hex + '\n'; "type " + one of blob, tree, commit, tag + '\n'; then, at p, p + 4 < size and
 * the bytes "tag ".
 * A malformed object gets MD_INVALID_OBJECT and has NO EDGES AT ALL, not the ones in front of the fault.  An object that did
 * not decode keeps md_pack_read's status for it (MD_INVALID_PACK_BASE for what hangs off it) and has no edges.  A failed
 * object never fails the call or its neighbours.  md_pack_graph_status: every object's status - the table's for what is not
 * decoded (blobs, objects that failed in md_pack_open), else the above.
 *
 * md_pack_graph_edges: first (n + 1 entries) is a CSR over all n objects - blobs and failed objects have empty ranges -, to and
 * kind the edges, cap of them at least info.edges (else MD_UNEXPECTED_END_OF_OUTPUT); cap == 0 with NULL arrays only asks:
 * md_pack_graph_get's info.edges says how many.  info: n; edges, and how many of them are absent and mistyped; malformed
 * objects; failed = objects whose status is neither MD_OK nor MD_INVALID_OBJECT; parsed = objects decoded and parsed (a base
 * decoded in two rounds counts twice, as md_pack_stats::objects does); rounds as md_pack_last's; parse_launches = launches of
 * the two link kernels; device_ns = their device time (two events around them, per round).
 * The graph keeps first, to and kind resident on the context's device, and its COMMIT_PARENT and TAG_TARGET edges on the host.
 *
 * md_pack_reachable: mark[i] = 1 iff i is a root or is reached from a root over edges with to != MD_PACK_NO_LINK.  An object
 * is walked through by the edges it has, whatever type the edge expected.  With an exclude list the result is
 * R(roots) \ R(exclude), the exact set difference.  This is this library's definition, not git rev-list's boundary
 * heuristics; on graphs with no MISTYPED edges and no exclusions it is the object set of
 * `git rev-list --objects --missing=print <roots>`.  *count = the marks set.  A root or exclude index >= n, a NULL array with
 * a non-zero count: MD_E_INVALID_ARGUMENT.  How it walks: a history is a long thin chain, so the HOST first closes the roots
 * over COMMIT_PARENT and TAG_TARGET edges; what that reached seeds the device's first frontier, and one launch per
 * non-empty frontier follows all edges, one wavefront per frontier object, with the next frontier's length (4 bytes) read
 * back between launches.  Without MISTYPED edges that is at most d + 2 launches, d = the deepest nesting of trees below a root
 * tree.  With exclusions the exclude walk runs first into a second mark.
 * md_pack_reach_last, summed over both walks of the context's last md_pack_reachable: host_closed = objects the host's closure
 * held (the roots included), seeds = objects of the first frontiers (the closed ones that have an edge), rounds = launches of
 * the step kernel, expanded = objects that stood on a frontier (each exactly once a walk), marked = *count, device_ns. */
#define MD_PACK_NO_LINK 0xffffffffu
#define MD_PACK_EDGE_COMMIT_TREE 1
#define MD_PACK_EDGE_COMMIT_PARENT 2
#define MD_PACK_EDGE_TAG_TARGET 3
#define MD_PACK_EDGE_TREE_BLOB 4
#define MD_PACK_EDGE_TREE_TREE 5
#define MD_PACK_EDGE_TREE_GITLINK 6
#define MD_PACK_EDGE_ABSENT 0x40
#define MD_PACK_EDGE_MISTYPED 0x80
typedef struct md_pack_graph md_pack_graph;
typedef struct md_pack_graph_info {
  uint64_t n, edges, absent, mistyped, malformed, failed, parsed, rounds, parse_launches, device_ns;
} md_pack_graph_info;
typedef struct md_pack_reach_stats {
  uint64_t host_closed, seeds, rounds, expanded, marked, device_ns;
} md_pack_reach_stats;
int md_pack_graph_build(md_ctx *ctx, const md_pack *p, const uint8_t *pack, size_t pack_len, unsigned flags, md_pack_graph **g);
int md_pack_graph_get(const md_pack_graph *g, md_pack_graph_info *info);
int md_pack_graph_edges(const md_pack_graph *g, uint64_t *first, uint32_t *to, uint8_t *kind, size_t cap);
int md_pack_graph_status(const md_pack_graph *g, int32_t *status);
int md_pack_reachable(md_ctx *ctx, const md_pack_graph *g, const uint64_t *roots, size_t nroots, const uint64_t *exclude, size_t nexclude,
                      uint8_t *mark, uint64_t *count);
int md_pack_reach_last(const md_ctx *ctx, md_pack_reach_stats *stats);
void md_pack_graph_free(md_pack_graph *g);

/* ---- git packs: trees diffed, what every commit changed (csrc/pack_diff_kernels.hip, csrc/pack_diff.hpp) ----------------------
 * md_pack_diff diffs npairs pairs of trees (a[q], b[q]) - indices of the table's objects, or MD_TREE_NONE for the empty tree -
 * on the device: `git diff-tree` (flags 0) or `git diff-tree -r -t` (MD_PACK_DIFF_RECURSIVE) for every pair at once, without
 * rename detection.  The graph g (md_pack_graph_build of the same table) gives the objects that entries name.
 *
 * Canonical mode: git's canon_mode of the entry's octal mode, parsed as above (32 bits, wrapping): (m & 0170000) == 0100000
 * gives 0100755 if m & 0100, else 0100644; 0120000 gives 0120000; 0040000 gives 0040000; anything else 0160000.  An entry is a
 * directory iff its canonical mode is 040000.
 * Key and order: an entry's key is its name bytes, with '/' appended iff it is a directory; keys compare bytewise, a proper
 * prefix first (git's base_name_compare).  A tree is sorted iff its keys ascend strictly.
 * A tree is unreadable for the diff when the tree rules above refuse it, when it is not sorted, when its status in the graph is
 * not MD_OK, when its type is not tree, and when the read refused it.
 *
 * A pair (A, B): entries match iff their keys are equal and both or neither is a directory (a file and a directory of one name
 * never match).  Matched non-directories: equal canonical modes and equal 20 bytes give nothing, otherwise 'T' if the canonical
 * modes differ in & 0170000, else 'M'.  Matched directories: equal 20 bytes give nothing, otherwise one 'M' record with
 * MD_TREE_CHANGE_TREE and, when recursive, the sub-pair (A's subtree, B's subtree).  An entry only in A gives 'D', with
 * MD_TREE_CHANGE_TREE and the sub-pair (subtree, MD_TREE_NONE) if it is a directory; one only in B gives 'A', with the sub-pair
 * (MD_TREE_NONE, subtree).  Gitlinks are leaves: their 20 bytes are compared and never looked up.  A sub-pair with an unreadable
 * side (or whose subtree the pack does not hold) is not descended: its directory record gets MD_TREE_CHANGE_OPAQUE.  A pair of
 * the call with an unreadable side has no records and the status MD_INVALID_OBJECT, or the graph's or the read's own status
 * where there is one (A's in front of B's); it never fails the call or its neighbours.  A == B gives MD_OK and no records, and
 * neither tree is read.
 *
 * Records stand breadth first: level 0 holds every pair's records in pair order, level k + 1 the sub-pairs' records in the order
 * of their directory records; within one pair first the records of A's entries in A's order ('D', 'M', 'T'), then those of the
 * entries only B has in B's order ('A').  So the records are a function of pack, graph and pairs; it is not the order git
 * prints in.  A record's path is the chain of names through `parent`.  name_off counts in the names blob, where the records'
 * names stand in record order; a_obj / b_obj are the graph's `to` of the entry.
 *
 * How: per level, the host lists the level's distinct trees, the read decodes them and KEEPS THEM ON THE DEVICE, one launch
 * writes every tree's table of entries (once a tree however many pairs share it), the diff kernel counts, two scans place the
 * records, the diff kernel writes them, and the host derives the next level's sub-pairs.  A level's trees must fit the device
 * beside the read's rounds ("pack_workspace"): a tree the read refuses (MD_E_OUT_OF_MEMORY) is unreadable.
 * info: pairs; changes = records; name_bytes; levels = levels that had a pair to diff; opaque = records with
 * MD_TREE_CHANGE_OPAQUE; failed = pairs whose status is not MD_OK; trees_read = trees decoded, summed over the levels; launches
 * of the table and diff kernels and the scans (at most 5 a level, whatever the number of pairs); device_ns of the two kernels.
 * md_pack_diff_changes: cap records and names_cap bytes at least info's (else MD_UNEXPECTED_END_OF_OUTPUT); cap == 0 with NULL
 * arrays only asks.  An index >= n that is not MD_TREE_NONE, a flag other than MD_PACK_DIFF_RECURSIVE: MD_E_INVALID_ARGUMENT; a
 * graph of another table or a pack other than the table's: MD_INVALID_INDEX.
 * Not built: renames and copies, combined diffs of merges, pathspecs, blob contents. */
#define MD_TREE_NONE 0xffffffffu
#define MD_PACK_DIFF_RECURSIVE 1u
#define MD_TREE_CHANGE_TREE 1
#define MD_TREE_CHANGE_OPAQUE 2
typedef struct md_tree_change {
  uint32_t pair, parent;        /* the caller's pair; the directory record this one lies in, or MD_TREE_NONE at level 0 (parent < own index) */
  uint8_t  kind, flags;         /* 'A' 'D' 'M' 'T'; MD_TREE_CHANGE_TREE, MD_TREE_CHANGE_OPAQUE */
  uint32_t a_mode, b_mode;      /* canonical; 0 on the side that has no entry */
  uint32_t a_obj, b_obj;        /* the graph's `to` for the entry, MD_PACK_NO_LINK where absent / gitlink / no entry */
  uint32_t name_len; uint64_t name_off;   /* the entry's own name (not the path) in the names blob */
  uint8_t  a_name[20], b_name[20];        /* zeros on the side that has no entry */
} md_tree_change;
typedef struct md_pack_diff_result md_pack_diff_result;
typedef struct md_pack_diff_info {
  uint64_t pairs, changes, name_bytes, levels, opaque, failed, trees_read, launches, device_ns;
} md_pack_diff_info;
int md_pack_diff(md_ctx *ctx, const md_pack *p, const md_pack_graph *g, const uint8_t *pack, size_t pack_len, size_t npairs, const uint32_t *a,
                 const uint32_t *b, unsigned flags, md_pack_diff_result **r);
int md_pack_diff_get(const md_pack_diff_result *r, md_pack_diff_info *info);
int md_pack_diff_changes(const md_pack_diff_result *r, md_tree_change *changes, size_t cap, uint8_t *names, size_t names_cap);
int md_pack_diff_status(const md_pack_diff_result *r, int32_t *status);
void md_pack_diff_free(md_pack_diff_result *r);

#ifdef __cplusplus
}
#endif
#endif
