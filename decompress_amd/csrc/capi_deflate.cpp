// capi_deflate.cpp — the encoder's entry points: the launch of the deflate kernels over a batch, Def.Ns, batches in
// slices of positions, the stream in pieces of stream_def.cpp, host buffers, and the partial drivers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <vector>

#include "ctx.hpp"
#include "host_pipeline.hpp"

// a stream's slot in the per-position workspace: its length + 64, rounded up to the match kernel's chunk
constexpr uint64_t kSlotPad = 64 + md::defl::kChunk - 1;
constexpr size_t kOrderFromDeflate = 257;  // the link kernel holds one stream per CU

// The bytes Gz.Def writes in front of the body (lib/gz.ml:796-812) for the header fields of Gz.Def.encoder
// (lib/gz.ml:859-918); returns the length, 0 when a field is out of range.
uint32_t gz_header_bytes(const md_gz_header *g, int level, uint8_t h[544]) {
  static const md_gz_header dflt = {0, 3, 0, 0, nullptr, nullptr};
  if (!g) g = &dflt;
  const size_t nl = g->filename ? strlen(g->filename) : 0, cl = g->comment ? strlen(g->comment) : 0;
  if (nl > 255 || cl > 255 || g->os < 0 || g->os > 255) return 0;
  memset(h, 0, 544);
  // flg, lib/gz.ml:851-857; mtime big-endian, lib/gz.ml:801
  h[0] = 0x1f;
  h[1] = 0x8b;
  h[2] = 8;
  h[3] = (uint8_t)((g->ascii ? 1 : 0) | (g->hcrc ? 2 : 0) | (g->filename ? 8 : 0) | (g->comment ? 16 : 0));
  h[4] = (uint8_t)(g->mtime >> 24);
  h[5] = (uint8_t)(g->mtime >> 16);
  h[6] = (uint8_t)(g->mtime >> 8);
  h[7] = (uint8_t)g->mtime;
  h[8] = level == 9 ? 2 : 0;  // xfl, lib/gz.ml:888-890
  h[9] = (uint8_t)g->os;
  uint32_t p = 10;
  if (g->filename) {
    memcpy(h + p, g->filename, nl + 1);
    p += (uint32_t)nl + 1;
  }
  if (g->comment) {
    memcpy(h + p, g->comment, cl + 1);
    p += (uint32_t)cl + 1;
  }
  if (g->hcrc) {  // the upper half of the CRC-32 of what precedes, big-endian (H10, lib/gz.ml:771-789)
    const uint32_t c16 = (md::crc32_update(0, h, p) & 0xffff0000u) >> 16;
    h[p] = (uint8_t)(c16 >> 8);
    h[p + 1] = (uint8_t)c16;
    p += 2;
  }
  return p;
}

// One piece of one stream (md_i_piece_run below): device pointers of what differs from a batch of whole streams.
struct PieceArgs {
  const uint64_t *d_front_len;  // length of the text the launch holds, n - w0 (d_in_len is the absolute length n)
  void *queue;                  // the stream's own command queue: it lives across launches
  md::defl::Piece piece;        // flags, state, pos, sum
  uint32_t match_skip;          // leading positions of the text no stream of the launch will take (the window brought along)
};

// ONE long stream whose hash chains are built in segments (deflate_chunked.hip): seg positions per segment, p_end the
// stream's first position not inserted ahead (len - 3)
struct LinkSegs {
  uint32_t seg, p_end;
};

// The front workspace of a launch over n streams, sized and carved, with the plan kernel run over d_len: *fr, and in
// *chunks the match kernel's grid.  total_in: an upper bound of the sum of the lengths when the caller knows one
// (md_deflate_params.total_in_bytes), else 0: the per-position part is then sized from the totals the plan kernel
// computes, which costs one 16-byte read-back (a synchronisation with the context's stream).
static int front_workspace(md_ctx *ctx, size_t n, const uint64_t *d_len, int driver, int matcher, int level, bool matcher_runs,
                           size_t total_in, md::defl::Front *fr, uint32_t *chunks) {
  md::DevBuf &fsmall = ctx->scratch[kFsmall], &fbig = ctx->scratch[kFbig];
  int rc = fsmall.reserve(ctx, md_front_small_bytes((uint32_t)n), "hipMalloc(deflate plan)");
  if (rc != MD_OK) return rc;
  uint64_t positions = 0;
  *chunks = 0;
  if (matcher_runs && total_in != 0) {
    // slot <= len + 64 + (chunk - 1) positions and <= len / chunk + 2 chunks per stream
    positions = (uint64_t)total_in + kSlotPad * n;
    const uint64_t c64 = (uint64_t)total_in / md::defl::kChunk + 2ull * n;
    if (c64 > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "batch too large for one launch");
    *chunks = (uint32_t)c64;
    rc = fbig.reserve(ctx, md_front_big_bytes(positions), "hipMalloc(deflate front workspace)");
    if (rc != MD_OK) return rc;
  }
  md_front_carve(fsmall.p, fbig.p, (uint32_t)n, positions, fr);
  MD_LAUNCH_TRY(ctx, md_launch_deflate_plan((uint32_t)n, d_len, driver, matcher, level, positions, *chunks, fr, ctx->stream));
  if (matcher_runs && total_in == 0) {
    uint64_t tot_pos = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&tot_pos, fr->slot + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(chunks, fr->chunk0 + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = fbig.reserve(ctx, md_front_big_bytes(tot_pos), "hipMalloc(deflate front workspace)");
    if (rc != MD_OK) return rc;
    md_front_carve(fsmall.p, fbig.p, (uint32_t)n, tot_pos, fr);
  }
  return MD_OK;
}

// total_in as in front_workspace.  d_tail: SeqArgs::tail (two words per stream), or null.  d_first: SeqArgs::first (where
// each stream begins to emit), or null; the match kernel then leaves out the chunks below it (deflate_test_flags bit 5:
// it does not - a measurement, the bytes are the same).
static int deflate_launch(md_ctx *ctx, int format, int level, int queue_len, int driver, int dynamic, int matcher,
                          const md_gz_header *gz, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                          const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                          uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum, uint32_t *d_hist, size_t total_in,
                          const PieceArgs *pa = nullptr, const LinkSegs *ls = nullptr, uint64_t *d_tail = nullptr,
                          const uint32_t *d_first = nullptr) {
  int grc_ = MD_OK;
  // (the Lz77-alone / encode-alone / scripted drivers leave the kernel before it saves a piece's state)
  if (pa && driver >= md::defl::DRV_LZ77) return fail(ctx, MD_E_INVALID_ARGUMENT, "a stream in pieces needs one of the three public drivers");
  if (!pa) grc_ = ctx->scratch[kWs].reserve(ctx, md_deflate_queue_bytes((uint32_t)n, queue_len), "hipMalloc(deflate command queues)");
  if (grc_ != MD_OK) return grc_;
  const uint64_t *d_front_len = pa ? pa->d_front_len : d_in_len;  // (a piece: the front kernels see [w0, n) as a stream)
  uint32_t max_chain = 0, nice = 0;
  md_deflate_level_params(driver, matcher, level, &max_chain, &nice);
  const bool matcher_runs = max_chain != 0 && driver < md::defl::DRV_ENCODE;  // level 0 copies; De.Def.encode has no text
  md::defl::Front fr;
  uint32_t chunks = 0;
  grc_ = front_workspace(ctx, n, d_front_len, driver, matcher, level, matcher_runs, total_in, &fr, &chunks);
  if (grc_ != MD_OK) return grc_;
  const uint8_t *gz_hdr = nullptr;
  uint32_t *gz_crc = nullptr;
  uint32_t gz_hdr_len = 0;
  if (format == MD_FORMAT_GZIP) {
    uint8_t h[544];
    gz_hdr_len = gz_header_bytes(gz, level, h);
    if (!gz_hdr_len) return fail(ctx, MD_E_INVALID_ARGUMENT, "gzip header field out of range");
    int grc = ctx->gz_tmp.reserve(ctx, n * 24, "hipMalloc(gzip scratch)");
    if (grc != MD_OK) return grc;
    gz_crc = (uint32_t *)((uint8_t *)ctx->gz_tmp.p + n * 20);
    grc = ctx->gz_hdr_dev.reserve(ctx, sizeof h, "hipMalloc(gzip header)");
    if (grc != MD_OK) return grc;
    if (!ctx->gz_hdr_valid || memcmp(ctx->gz_hdr_sent, h, sizeof h) != 0) {
      // pageable source: the runtime stages the bytes before the call returns, the copy itself is stream-ordered
      HIP_TRY(ctx, hipMemcpyAsync(ctx->gz_hdr_dev.p, h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
      memcpy(ctx->gz_hdr_sent, h, sizeof h);
      ctx->gz_hdr_valid = true;
    }
    gz_hdr = ctx->gz_hdr_dev.as<const uint8_t>();
    // (in pieces the CRC-32 is the caller's running one)
    if (!pa) MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_in, d_in_off, d_in_len, gz_crc, ctx->stream));
  }
  // more streams than the link kernel (one per CU) or the sequential kernel (16 per CU) hold at once: longest first
  uint32_t *order = nullptr;
  const int orc = launch_order(ctx, n, kOrderFromDeflate, &order);
  if (orc != MD_OK) return orc;
  // (a slice of a batch: by what the slice brings, not by the absolute length so far - idle streams bring nothing)
  if (order) MD_LAUNCH_TRY(ctx, md_launch_stream_order((uint32_t)n, d_front_len, order, ctx->stream));
  if (matcher_runs && chunks != 0) {
    bool linked = false;
    if (ls && n == 1 && !pa && matcher == MD_MATCHER_DE) {
      // ONE long stream (link_segments): its hash chains by segments on the whole chip, the same link[] and tails
      if (md_launch_link_chunked(d_in, d_in_off, d_front_len, ls->p_end, ls->seg, (uint32_t)ctx->cus, &fr, ctx->stream) == 0) {
        linked = true;
        ctx->link_last_segments = (ls->p_end + ls->seg - 1) / ls->seg;
      } else {
        (void)hipGetLastError();  // a launch that failed: the one-workgroup link kernel instead
      }
    }
    if (d_first && !pa && !(ctx->test_flags & 32))
      MD_LAUNCH_TRY(ctx, md_launch_deflate_front_first((uint32_t)n, chunks, d_in, d_in_off, d_front_len, matcher, max_chain, nice, &fr, order, d_first,
                                                       ctx->stream));
    else
    MD_LAUNCH_TRY(ctx, linked ? md_launch_deflate_match((uint32_t)n, chunks, d_in, d_in_off, d_front_len, max_chain, nice, &fr, 0u, ctx->stream)
                              : md_launch_deflate_front((uint32_t)n, chunks, d_in, d_in_off, d_front_len, matcher, max_chain, nice, &fr, order,
                                                        pa ? pa->match_skip : 0u, ctx->stream));
  }
  md::defl::SeqArgs args = {};
  args.format = format, args.level = level, args.qcap = queue_len, args.driver = driver, args.dynamic = dynamic, args.matcher = matcher;
  args.n = (uint32_t)n;
  args.in = d_in, args.in_off = d_in_off, args.in_len = d_in_len;
  args.out = d_out, args.out_off = d_out_off, args.out_cap = d_out_cap;
  args.out_len = d_out_len, args.status = d_status, args.checksum = d_checksum;
  args.fr = fr;
  args.queue_ws = (int *)(pa ? pa->queue : ctx->scratch[kWs].p);
  args.dbg = ctx->dbg.as<uint64_t>();
  args.gz_hdr = gz_hdr, args.gz_hdr_len = gz_hdr_len, args.gz_crc = gz_crc;
  args.hist = d_hist;
  args.order = order;
  if (pa) args.pcs = pa->piece;
  args.tail = d_tail;
  args.first = d_first;
  MD_LAUNCH_TRY(ctx, md_launch_deflate(&args, ctx->stream));
  return MD_OK;
}

// De.Def.Ns / Zl.Def.Ns: the front workspace as for deflate_launch (no command queues), then the three kernels of
// deflate_ns.hip.  total_in as in front_workspace.
static int def_ns_launch(md_ctx *ctx, int format, int level, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                         uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum, size_t total_in) {
  md::defl::Front fr;
  uint32_t chunks = 0;
  int grc_ = front_workspace(ctx, n, d_in_len, md::defl::DRV_NS, MD_MATCHER_DE, level, level >= 1 && level <= 4, total_in, &fr, &chunks);
  if (grc_ != MD_OK) return grc_;
  MD_LAUNCH_TRY(ctx, md_launch_def_ns(format, level, (uint32_t)n, chunks, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                                      d_checksum, &fr, ctx->stream));
  return MD_OK;
}

int md_def_ns_batch_device(md_ctx *ctx, int format, int level, size_t total_in_bytes, size_t n, const uint8_t *d_in,
                           const uint64_t *d_in_off, const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                           const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (level < 0 || level > 12) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid compression level");  // lib/de.ml:3930
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in_off || !d_in_len || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  MD_ON_DEVICE(ctx);
  return def_ns_launch(ctx, format, level, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                       d_checksum, total_in_bytes);
}

static int def_ns_one(md_ctx *ctx, int format, int level, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                      size_t *written) {
  if (!ctx || !written || (!src && src_len) || (!dst && dst_cap)) return MD_E_INVALID_ARGUMENT;
  if (level < 0 || level > 12) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid compression level");
  if (src_len > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_STREAM");
  MD_ON_DEVICE(ctx);
  return one_through_batch(ctx, src, src_len, dst, dst_cap, written,
                           [&](const uint8_t *d_in, uint64_t *d64, uint8_t *d_out, int32_t *d_status, uint32_t *) {
                             return def_ns_launch(ctx, format, level, 1, d_in, d64, d64 + 1, d_out, d64 + 2, d64 + 3, d64 + 4, d_status,
                                                  nullptr, src_len ? src_len : 1);
                           });
}
int md_de_def_ns_deflate(md_ctx *ctx, int level, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  return def_ns_one(ctx, MD_FORMAT_DEFLATE, level, src, src_len, dst, dst_cap, written);
}
int md_zl_def_ns_deflate(md_ctx *ctx, int level, const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  return def_ns_one(ctx, MD_FORMAT_ZLIB, level, src, src_len, dst, dst_cap, written);
}
size_t md_de_def_ns_compress_bound(size_t len) {  // lib/de.ml:3994-3997
  size_t max_blocks = (len + 10000 - 1) / 10000;
  if (max_blocks < 1) max_blocks = 1;
  return 5 * max_blocks + len + 1 + 8;
}
size_t md_zl_def_ns_compress_bound(size_t len) { return md_de_def_ns_compress_bound(len) + 6; }  // lib/zl.ml:600

static int check_params(md_ctx *ctx, int format, const md_deflate_params *p, md_deflate_params *q) {
  if (!p) return fail(ctx, MD_E_INVALID_ARGUMENT, "null md_deflate_params");
  *q = *p;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown format");
  if (format == MD_FORMAT_GZIP) {  // Gz.Def's driver is Zl's with block_of_frequencies (lib/gz.ml:724-729)
    q->driver = MD_DRIVER_ZL;
    q->dynamic = 1;
  }
  if (q->level < 0 || q->level > 9)  // Lz77.state: "Invalid level of compression", lib/de.ml:4477
    return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid level of compression");
  if (q->queue_len < 4 || q->queue_len > (1 << 20) || (q->queue_len & (q->queue_len - 1)))  // lib/de.ml:2286-2288
    return fail(ctx, MD_E_INVALID_ARGUMENT, "Length of queue MUST be a power of two");
  if (q->driver < MD_DRIVER_ZL || q->driver > MD_DRIVER_CLI) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown driver");
  if (q->matcher != MD_MATCHER_DE && q->matcher != MD_MATCHER_LZ) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown matcher");
  q->dynamic = q->dynamic ? 1 : 0;
  if (q->wbits != 0 && q->wbits != 15)  // De.Lz77.state ~w: only make_window ~bits:15 (lib/de.ml:4462-4464, :4513)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "only 32 KiB windows (wbits 15) are implemented");
  return MD_OK;
}

// what md_def_encoder checks before it keeps the parameters (stream_def.cpp); not part of the public header
int md_validate_deflate_params(md_ctx *ctx, int format, const md_deflate_params *params) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  md_deflate_params q;
  return check_params(ctx, format, params, &q);
}

// ---- a batch in slices of positions ----------------------------------------------------------------------------------
// The per-position workspace is 13 bytes per input byte of what ONE launch covers.  With a cap set (md_set_option
// "deflate_workspace_cap_mib") a batch that would need more goes through the kernels S positions of every stream at a
// time: a launch covers [k*S - kSliceKeep, (k+1)*S) of each stream that reaches that far and goes on from the state
// the launch before left (the machinery of the encoder in pieces, md_i_piece_run below).  S is a multiple of 32 KiB:
// every fill of De.Lz77's window ends on such a boundary (lib/de.ml:4294-4342: more = 2 * wsize - lookahead - strstart
// after a slide tops the window up, and the window's base moves 32 KiB at a time), so no fill ever finds less than it
// would with the whole stream at hand and the bytes out are the same.  kSliceKeep: what a launch sees again of the
// slice before - the matcher stopped less than 262 short of its end and reaches back 32 KiB - 262 from there.
static const uint64_t kSliceKeep = 33792;
static const uint64_t kSliceMin = 65536;

static uint64_t slice_positions(const uint64_t *len, size_t n, uint64_t S) {  // most text one launch covers
  uint64_t first = 0, second = 0;
  for (size_t i = 0; i < n; i++) {
    if (len[i] > MD_MAX_STREAM) continue;
    first += len[i] < S ? len[i] : S;
    if (len[i] > S) second += (len[i] - S < S ? len[i] - S : S) + kSliceKeep;
  }
  return (first > second ? first : second) + kSlotPad * n;
}

// md_deflate_batch_host feeds the slices from host memory and takes finished output away under them: before_slice(k) is
// called in front of the launches of slice k (it makes the context's stream wait for that slice's input and starts the
// copy of the next one), after_slice(k, fin) behind them, once the stream has been waited for, with fin[i] = the output
// bytes of stream i that are final
struct SliceHooks {
  std::function<int(uint64_t)> before_slice;  // in front of the launches of slice k
  std::function<int(uint64_t)> launched;      // right behind them: the place to enqueue copies that should run under them
  std::function<int(uint64_t, const std::vector<uint64_t> &)> after_slice;
};
static int deflate_in_slices(md_ctx *ctx, int format, const md_deflate_params &q, size_t n, uint64_t S, const uint8_t *d_in,
                             const uint64_t *h_in_off, const uint64_t *h_in_len, uint8_t *d_out, const uint64_t *h_out_off,
                             const uint64_t *h_out_cap, uint64_t *h_out_len, int32_t *h_status, uint32_t *h_checksum,
                             const uint32_t *h_crc, const SliceHooks *hooks = nullptr, uint64_t *d_tail = nullptr,
                             uint64_t *h_tail = nullptr, const uint32_t *d_first = nullptr) {
  // (d_tail / h_tail: SeqArgs::tail of the n streams.  The launch that ends a stream leaves its two words in d_tail, counted
  // from that piece's output; h_tail gets them counted from the stream's first byte.  d_first: SeqArgs::first of the n
  // streams; the first piece of a stream reads it, and S >= kSliceMin, so that piece holds all of [0, first))
  std::vector<uint64_t> tl(d_tail ? 2 * n : 0);
  // state slots for the streams that do not end in the first slice
  std::vector<uint64_t> slot(n, 0), used(n, 0);
  std::vector<uint8_t> done(n, 0);
  size_t n_long = 0;
  uint64_t longest = 0;
  for (size_t i = 0; i < n; i++) {
    if (h_in_len[i] > MD_MAX_STREAM) {  // 32-bit cursors (mdeflate.h): refused as the kernel refuses it in a whole batch
      done[i] = 1;
      h_status[i] = MD_E_INVALID_ARGUMENT;
      h_out_len[i] = 0;
      h_checksum[i] = 0;
      continue;
    }
    if (h_in_len[i] > S) slot[i] = n_long++;
    if (h_in_len[i] > longest) longest = h_in_len[i];
  }
  int rc = ctx->scratch[kSliceState].reserve(ctx, (n_long ? n_long : 1) * md::defl::kPieceState, "hipMalloc(deflate slice states)");
  if (rc != MD_OK) return rc;
  rc = ctx->scratch[kWs].reserve(ctx, md_deflate_queue_bytes((uint32_t)n, q.queue_len), "hipMalloc(deflate command queues)");
  if (rc != MD_OK) return rc;
  // descriptors of a slice: ten 64-bit and six 32-bit words per stream
  const size_t desc_bytes = n * (10 * 8 + 6 * 4);
  rc = ctx->scratch[kSliceDesc].reserve(ctx, desc_bytes, "hipMalloc(deflate slice descriptors)");
  if (rc != MD_OK) return rc;
  std::vector<uint64_t> hbuf((desc_bytes + 7) / 8);
  uint64_t *h64 = hbuf.data();
  uint64_t *in_off = h64, *front_len = h64 + n, *abs_len = h64 + 2 * n, *out_off = h64 + 3 * n, *out_cap = h64 + 4 * n,
           *out_len = h64 + 5 * n, *pos = h64 + 6 * n;
  uint32_t *h32 = (uint32_t *)(h64 + 10 * n);
  uint32_t *st = h32, *sum_out = h32 + n, *flags = h32 + 2 * n, *sums = h32 + 3 * n;  // (sums: 2 per stream)
  uint64_t *d64 = (uint64_t *)ctx->scratch[kSliceDesc].p;
  uint32_t *d32 = (uint32_t *)(d64 + 10 * n);
  const uint64_t nslices = longest ? (longest + S - 1) / S : 1;
  for (uint64_t k = 0; k < nslices; k++) {
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
      const uint64_t len = h_in_len[i];
      const uint64_t end = len < (k + 1) * S ? len : (k + 1) * S;
      const uint64_t w0 = k == 0 ? 0 : k * S - kSliceKeep;
      const bool idle = done[i] || (k > 0 && len <= k * S);
      in_off[i] = h_in_off[i] + (idle ? 0 : w0);
      front_len[i] = idle ? 0 : end - w0;
      abs_len[i] = idle ? 0 : end;
      out_off[i] = h_out_off[i] + used[i];
      out_cap[i] = h_out_cap[i] - used[i];
      out_len[i] = 0;
      pos[4 * i] = idle ? 0 : w0;
      pos[4 * i + 1] = 0;
      pos[4 * i + 2] = slot[i];
      pos[4 * i + 3] = i;
      st[i] = 0;
      sum_out[i] = 0;
      flags[i] = idle ? 8u : (k == 0 ? 1u : 0u) | (end == len ? 2u : 0u) | 4u;
      sums[2 * i] = h_crc ? h_crc[i] : 1u;
      sums[2 * i + 1] = (uint32_t)len;
      total += front_len[i];
    }
    if (hooks) {
      rc = hooks->before_slice(k);
      if (rc != MD_OK) return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(d64, h64, desc_bytes, hipMemcpyHostToDevice, ctx->stream));
    // (every stream of a later slice stopped less than 262 + 64 short of the slice before's end)
    PieceArgs pa{d64 + n, ctx->scratch[kWs].p, {d32 + 2 * n, (uint8_t *)ctx->scratch[kSliceState].p, d64 + 6 * n, d32 + 3 * n}, k == 0 ? 0u : (uint32_t)kSliceKeep - 512u};
    rc = deflate_launch(ctx, format, q.level, q.queue_len, q.driver, q.dynamic, q.matcher, q.gz_header, n, d_in, d64, d64 + 2 * n,
                        d_out, d64 + 3 * n, d64 + 4 * n, d64 + 5 * n, (int32_t *)d32, d32 + n, nullptr, total ? total : 1, &pa, nullptr, d_tail,
                        d_first);
    if (rc != MD_OK) return rc;
    if (hooks) {  // (in front of the read-backs: a copy to pageable memory keeps the calling thread until the kernels are done)
      rc = hooks->launched(k);
      if (rc != MD_OK) return rc;
    }
    HIP_TRY(ctx, md::to_host(out_len, d64 + 5 * n, n, ctx->stream));
    HIP_TRY(ctx, md::to_host(st, d32, 2 * n, ctx->stream));
    if (d_tail) HIP_TRY(ctx, md::to_host(tl.data(), d_tail, 2 * n, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) {
      if (flags[i] & 8) continue;
      if ((int32_t)st[i] == MD_PIECE_AWAIT) {  // more of the stream to come
        used[i] += out_len[i];
        continue;
      }
      done[i] = 1;
      if (h_tail) h_tail[2 * i] = 8 * used[i] + tl[2 * i], h_tail[2 * i + 1] = 8 * used[i] + tl[2 * i + 1];
      h_status[i] = (int32_t)st[i];
      h_checksum[i] = sum_out[i];
      h_out_len[i] = (int32_t)st[i] == MD_OK ? used[i] + out_len[i] : 0;
    }
    if (hooks) {
      std::vector<uint64_t> fin(n);
      for (size_t i = 0; i < n; i++) fin[i] = done[i] ? h_out_len[i] : used[i];
      rc = hooks->after_slice(k, fin);
      if (rc != MD_OK) return rc;
    }
  }
  for (size_t i = 0; i < n; i++)
    if (!done[i]) return fail(ctx, MD_E_HIP, "deflate in slices: a stream did not end");
  return MD_OK;
}

// the batch whose workspace is above the cap: lengths to the host, slices sized to the cap (in groups of streams if a
// slice of every stream at once would still be too much), results back to the caller's device arrays
static int deflate_capped(md_ctx *ctx, int format, const md_deflate_params &q, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                          const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                          uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum, uint64_t *d_tail, const uint32_t *d_first,
                          bool *whole, uint64_t *total_out) {
  std::vector<uint64_t> h(4 * n);
  uint64_t *in_off = h.data(), *in_len = in_off + n, *out_off = in_len + n, *out_cap = out_off + n;
  HIP_TRY(ctx, md::to_host(in_off, d_in_off, n, ctx->stream));
  HIP_TRY(ctx, md::to_host(in_len, d_in_len, n, ctx->stream));
  HIP_TRY(ctx, md::to_host(out_off, d_out_off, n, ctx->stream));
  HIP_TRY(ctx, md::to_host(out_cap, d_out_cap, n, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t total = 0, longest = 0;
  for (size_t i = 0; i < n; i++) {
    if (in_len[i] > MD_MAX_STREAM) in_len[i] = MD_MAX_STREAM + 1;  // (the kernel refuses it)
    else total += in_len[i];
    if (in_len[i] > longest) longest = in_len[i];
  }
  (void)longest;
  *total_out = total ? total : 1;  // what the lengths add up to: the one launch sizes its workspace from this, not from the hint
  *whole = md_front_big_bytes(total + kSlotPad * n) <= ctx->front_cap_bytes;
  if (*whole) return MD_OK;  // (fits after all: the caller's one launch)
  std::vector<uint64_t> r_len(n);
  std::vector<int32_t> r_st(n);
  std::vector<uint32_t> r_sum(n), crc;
  std::vector<uint64_t> r_tail(d_tail ? 2 * n : 0);
  if (format == MD_FORMAT_GZIP) {  // the CRC-32 of every stream, once
    int grc = ctx->gz_tmp.reserve(ctx, n * 24, "hipMalloc(gzip scratch)");
    if (grc != MD_OK) return grc;
    uint32_t *d_crc = (uint32_t *)((uint8_t *)ctx->gz_tmp.p + n * 20);
    MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_in, d_in_off, d_in_len, d_crc, ctx->stream));
    crc.resize(n);
    HIP_TRY(ctx, md::to_host(crc.data(), d_crc, n, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  // First in groups of consecutive streams, as long as a group still fills the device several times over (16 streams
  // per CU: 4 096 at a time - more streams than that take turns anyway; but a group lasts as long as its longest stream at
  // least, so it has to bring enough work to cover that: four turns); then, within a group, in slices of positions, each
  // group with the largest slice that fits (at least kSliceMin, else fewer streams)
  const size_t kGeneration = 4 * 4096;
  size_t groups = (size_t)((md_front_big_bytes(total + kSlotPad * n) + ctx->front_cap_bytes - 1) / ctx->front_cap_bytes);
  if (groups > n / kGeneration) groups = n / kGeneration;
  if (groups < 1) groups = 1;
  const size_t per_group = (n + groups - 1) / groups;
  for (size_t i0 = 0; i0 < n;) {
    size_t k = n - i0 < per_group ? n - i0 : per_group;
    uint64_t S = 0;
    for (;;) {
      uint64_t lo = kSliceMin / 32768, hi = 0;
      uint64_t gl = 0;
      for (size_t i = i0; i < i0 + k; i++) gl = in_len[i] <= MD_MAX_STREAM && in_len[i] > gl ? in_len[i] : gl;
      hi = (gl + 32767) / 32768;
      if (hi < lo) hi = lo;
      if (md_front_big_bytes(slice_positions(in_len + i0, k, lo * 32768)) > ctx->front_cap_bytes && k > 1) {
        k = (k + 1) / 2;  // too many streams for the smallest slice: fewer of them
        continue;
      }
      while (lo < hi) {  // the largest S (in 32 KiB units) whose launches fit
        const uint64_t mid = (lo + hi + 1) / 2;
        if (md_front_big_bytes(slice_positions(in_len + i0, k, mid * 32768)) <= ctx->front_cap_bytes) lo = mid;
        else hi = mid - 1;
      }
      S = lo * 32768;
      if (gl > S) {  // as many slices as that takes, of even size
        const uint64_t ns = (gl + S - 1) / S;
        S = ((gl + ns - 1) / ns + 32767) / 32768 * 32768;
      }
      break;
    }
    int rc = deflate_in_slices(ctx, format, q, k, S, d_in, in_off + i0, in_len + i0, d_out, out_off + i0, out_cap + i0, r_len.data() + i0,
                               r_st.data() + i0, r_sum.data() + i0, crc.empty() ? nullptr : crc.data() + i0, nullptr,
                               d_tail ? d_tail + 2 * i0 : nullptr, d_tail ? r_tail.data() + 2 * i0 : nullptr, d_first ? d_first + i0 : nullptr);
    if (rc != MD_OK) return rc;
    i0 += k;
  }
  HIP_TRY(ctx, md::to_device(d_out_len, r_len.data(), n, ctx->stream));
  HIP_TRY(ctx, md::to_device(d_status, r_st.data(), n, ctx->stream));
  if (d_checksum) HIP_TRY(ctx, md::to_device(d_checksum, r_sum.data(), n, ctx->stream));
  if (d_tail) HIP_TRY(ctx, md::to_device(d_tail, r_tail.data(), 2 * n, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors go out of scope)
  *whole = false;
  return MD_OK;
}

// ls: ONE stream whose hash chains go in segments (md_deflate_batch_host), else null; d_tail: SeqArgs::tail, or null;
// d_first: SeqArgs::first, or null
static int deflate_batch_device(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_in,
                                const uint64_t *d_in_off, const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                                const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum,
                                const LinkSegs *ls, uint64_t *d_tail = nullptr, const uint32_t *d_first = nullptr) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  ctx->link_last_segments = 0;
  md_deflate_params q;
  int rc = check_params(ctx, format, params, &q);
  if (rc != MD_OK) return rc;
  if (n == 0) return MD_OK;
  if (n > 0x7fffffffull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many streams in one batch");
  if (!d_in_off || !d_in_len || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  MD_ON_DEVICE(ctx);
  // The per-position workspace is 13 bytes per input byte of what one launch covers (md_front_big_bytes): with a cap set
  // (md_set_option "deflate_workspace_cap_mib") a batch that would need more is taken in slices of positions - same bytes
  // out (deflate_in_slices above).  Without params->total_in_bytes the lengths have to be read back to know.
  {
    uint32_t max_chain = 0, nice = 0;
    md_deflate_level_params(q.driver, q.matcher, q.level, &max_chain, &nice);
    if (ctx->front_cap_bytes && max_chain != 0 &&
        (!q.total_in_bytes || md_front_big_bytes((uint64_t)q.total_in_bytes + kSlotPad * n) > ctx->front_cap_bytes)) {
      bool whole = true;
      uint64_t total = 0;
      rc = deflate_capped(ctx, format, q, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_checksum, d_tail, d_first,
                          &whole, &total);
      if (rc != MD_OK || !whole) return rc;
      // the batch fits the cap after all: one launch, sized from the sum just read back (no second read-back in
      // deflate_launch, and a loose hint cannot make the workspace grow above the cap)
      q.total_in_bytes = (size_t)total;
    }
  }
  return deflate_launch(ctx, format, q.level, q.queue_len, q.driver, q.dynamic, q.matcher, q.gz_header, n, d_in, d_in_off,
                        d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_checksum, nullptr, q.total_in_bytes,
                        nullptr, ls, d_tail, d_first);
}

int deflate_batch_tails(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_in, const uint64_t *d_in_off,
                        const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap, uint64_t *d_out_len,
                        int32_t *d_status, uint32_t *d_checksum, uint64_t *d_tail, const uint32_t *d_first) {
  return deflate_batch_device(ctx, format, params, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                              d_checksum, nullptr, d_tail, d_first);
}

int md_deflate_batch_device(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_in,
                            const uint64_t *d_in_off, const uint64_t *d_in_len, uint8_t *d_out, const uint64_t *d_out_off,
                            const uint64_t *d_out_cap, uint64_t *d_out_len, int32_t *d_status, uint32_t *d_checksum) {
  return deflate_batch_device(ctx, format, params, n, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                              d_checksum, nullptr);
}

// ---- the encoder shim's stream in pieces (stream_def.cpp): not part of the public ABI ------------------------------
// A launch takes the text [w0, n) of ONE stream - the last 64 KiB the launch before already saw plus what arrived since -
// and goes on from the state that launch left in device memory (the two structs of the sequential kernel, 12 KiB, and
// the stream's command queue): the matcher answers `Await at the end of the piece exactly where the reference's would
// (deflate_kernel.hip, LZ_AWAIT), so the bytes are those of the reference fed the same pieces.  Neither side keeps
// more of the stream than the window and the piece.
struct md_piece {
  md::DevBuf d_text, d_out, d_state, d_queue, d_desc;
};
md_piece *md_i_piece_open(md_ctx *ctx, int queue_len) {
  if (!ctx || queue_len < 4) return nullptr;
  md::DeviceGuard guard(ctx->device);
  md_piece *p = new md_piece();
  const char *what = "hipMalloc(encoder state)";
  if (p->d_state.reserve(ctx, md::defl::kPieceState, what) != MD_OK || p->d_queue.reserve(ctx, (size_t)queue_len * 4, what) != MD_OK ||
      p->d_desc.reserve(ctx, 128, what) != MD_OK) {
    delete p;
    return nullptr;
  }
  return p;
}
void md_i_piece_close(md_ctx *ctx, md_piece *p) {
  if (!ctx || !p) return;
  md::DeviceGuard guard(ctx->device);
  hipStreamSynchronize(ctx->stream);
  delete p;
}
// text: the bytes at positions [w0, w0 + text_len) (w0 a multiple of 64, at most 65536 - 64 behind the end of the piece
// before), of which the first `seen` went through the piece before already.  Positions count from an origin the caller moves up now and then so that they stay below MD_MAX_STREAM:
// rebase is how far it moved since the piece before (a multiple of 65536, at least 65536 below w0 as that piece counted
// it).  sum / isize: Adler-32 (CRC-32 for gzip) and length mod 2^32 of the whole input so far.  The piece's output
// stays in device memory (md_i_piece_out reads it); *status is MD_PIECE_AWAIT when the encoder waits for more.
int md_i_piece_run(md_ctx *ctx, md_piece *p, int format, const md_deflate_params *params, const uint8_t *text, size_t text_len,
                   size_t seen, uint64_t w0, uint64_t rebase, int first, int last, uint32_t sum, uint32_t isize, size_t out_cap,
                   size_t *out_len, int *status) {
  if (!ctx || !p || !params || !out_len || !status || (!text && text_len)) return MD_E_INVALID_ARGUMENT;
  md_deflate_params q;
  int rc = check_params(ctx, format, params, &q);
  if (rc != MD_OK) return rc;
  if (w0 + text_len > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "piece beyond MD_MAX_STREAM");
  MD_ON_DEVICE(ctx);
  rc = p->d_text.reserve(ctx, text_len + 320, "hipMalloc(encoder text)");
  if (rc == MD_OK) rc = p->d_out.reserve(ctx, out_cap ? out_cap : 16, "hipMalloc(encoder output)");
  if (rc != MD_OK) return rc;
  uint64_t h[13] = {0, (uint64_t)text_len, w0 + text_len, 0, (uint64_t)out_cap, 0, w0, rebase, 0, 0, 0, 0, 0};  // ([8], [9]: state and queue slot)
  uint32_t *h32 = (uint32_t *)(h + 10);  // status, checksum, flags, -, sum, isize
  h32[2] = (first ? 1u : 0u) | (last ? 2u : 0u);
  h32[4] = sum;
  h32[5] = isize;
  uint64_t *d64 = p->d_desc.as<uint64_t>();
  uint32_t *d32 = (uint32_t *)(d64 + 10);
  HIP_TRY(ctx, hipMemcpyAsync(d64, h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
  if (text_len) HIP_TRY(ctx, hipMemcpyAsync(p->d_text.p, text, text_len, hipMemcpyHostToDevice, ctx->stream));
  PieceArgs pa{d64 + 1, p->d_queue.p, {d32 + 2, p->d_state.as<uint8_t>(), d64 + 6, d32 + 4}, seen > 512 ? (uint32_t)(seen - 512) : 0u};
  rc = deflate_launch(ctx, format, q.level, q.queue_len, q.driver, q.dynamic, q.matcher, q.gz_header, 1, p->d_text.as<const uint8_t>(),
                      d64 + 0, d64 + 2, p->d_out.as<uint8_t>(), d64 + 3, d64 + 4, d64 + 5, (int32_t *)d32, d32 + 1, nullptr,
                      text_len ? text_len : 1, &pa);
  if (rc != MD_OK) return rc;
  uint64_t olen = 0;
  int32_t st = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&olen, d64 + 5, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&st, d32, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (and the caller's text is his again)
  *out_len = (size_t)olen;
  *status = st;
  return MD_OK;
}
// One piece of each of n streams in ONE launch of the kernels (md_def_batch, stream_def.cpp): texts, outputs, states
// and queues are the caller's device buffers, the descriptors host arrays of n entries.  flags as struct Piece's (bit 3:
// the stream takes no part in this launch).  Synchronous: the results are read back.
int md_i_pieces_run(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *d_text, uint8_t *d_out,
                    void *d_state, void *d_queue, md::DevBuf &d_desc, const md_pieces_io *io, uint32_t match_skip) {
  if (!ctx || !params || !io || n == 0) return MD_E_INVALID_ARGUMENT;
  md_deflate_params q;
  int rc = check_params(ctx, format, params, &q);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  const size_t desc_bytes = n * (10 * 8 + 6 * 4);
  rc = d_desc.reserve(ctx, desc_bytes, "hipMalloc(encoder batch descriptors)");
  if (rc != MD_OK) return rc;
  std::vector<uint64_t> hbuf((desc_bytes + 7) / 8);
  uint64_t *h64 = hbuf.data();
  uint64_t *in_off = h64, *front_len = h64 + n, *abs_len = h64 + 2 * n, *out_off = h64 + 3 * n, *out_cap = h64 + 4 * n,
           *out_len = h64 + 5 * n, *pos = h64 + 6 * n;
  uint32_t *h32 = (uint32_t *)(h64 + 10 * n);
  uint32_t *st = h32, *flags = h32 + 2 * n, *sums = h32 + 3 * n;
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    const bool idle = (io->flags[i] & 8u) != 0;
    if (!idle && io->abs_len[i] > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "piece beyond MD_MAX_STREAM");
    in_off[i] = io->text_off[i];
    front_len[i] = idle ? 0 : io->text_len[i];
    abs_len[i] = idle ? 0 : io->abs_len[i];
    out_off[i] = io->out_off[i];
    out_cap[i] = io->out_cap[i];
    out_len[i] = 0;
    pos[4 * i] = idle ? 0 : io->w0[i];
    pos[4 * i + 1] = idle ? 0 : io->rebase[i];
    pos[4 * i + 2] = i;
    pos[4 * i + 3] = i;
    st[i] = 0;
    h32[n + i] = 0;
    flags[i] = io->flags[i];
    sums[2 * i] = io->sum[i];
    sums[2 * i + 1] = io->isize[i];
    total += front_len[i];
  }
  uint64_t *d64 = d_desc.as<uint64_t>();
  uint32_t *d32 = (uint32_t *)(d64 + 10 * n);
  HIP_TRY(ctx, hipMemcpyAsync(d64, h64, desc_bytes, hipMemcpyHostToDevice, ctx->stream));
  PieceArgs pa{d64 + n, d_queue, {d32 + 2 * n, (uint8_t *)d_state, d64 + 6 * n, d32 + 3 * n}, match_skip};
  rc = deflate_launch(ctx, format, q.level, q.queue_len, q.driver, q.dynamic, q.matcher, q.gz_header, n, d_text, d64, d64 + 2 * n,
                      d_out, d64 + 3 * n, d64 + 4 * n, d64 + 5 * n, (int32_t *)d32, d32 + n, nullptr, total ? total : 1, &pa);
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(io->out_len, d64 + 5 * n, n, ctx->stream));
  HIP_TRY(ctx, md::to_host(io->status, (const int32_t *)d32, n, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MD_OK;
}
int md_i_piece_out(md_ctx *ctx, const md_piece *p, size_t off, uint8_t *host, size_t len) {
  if (!ctx || !p || (!host && len)) return MD_E_INVALID_ARGUMENT;
  MD_ON_DEVICE(ctx);
  if (len) HIP_TRY(ctx, hipMemcpy(host, p->d_out.as<const uint8_t>() + off, len, hipMemcpyDeviceToHost));
  return MD_OK;
}

// md_deflate_batch_host for a batch of LONG streams laid out at equal distances (what a caller with n equal buffers has; C3):
// cutting it into slices of streams would leave the sequential kernel short of streams (it wants 4 096), so it is cut into
// slices of positions (deflate_in_slices: the kernels go on from the state the slice before left, same bytes out) and the
// copies ride along - the columns [k S, (k + 1) S) of every stream's input as ONE strided copy under the kernels of slice
// k - 1, and every output column that is final for all streams as one strided copy under the kernels of the next slice.
// Returns MD_NOT_HANDLED when the batch is not of that kind (GZip: the CRC-32 of a whole stream comes first; level 0; short or
// irregular streams): the caller then pipelines slices of streams as before.
static int deflate_host_positions(md_ctx *ctx, int format, const md_deflate_params *params, size_t n, const uint8_t *h_in, size_t in_bytes,
                                  const uint64_t *in_off, const uint64_t *in_len, uint8_t *h_out, size_t out_bytes, const uint64_t *out_off,
                                  const uint64_t *out_cap, uint64_t *out_len, int32_t *status, uint32_t *checksum, uint8_t *din, uint8_t *dout) {
  if (format == MD_FORMAT_GZIP || n < 2 || ctx->host_slices_max < 2) return MD_NOT_HANDLED;
  md_deflate_params q;
  if (check_params(ctx, format, params, &q) != MD_OK) return MD_NOT_HANDLED;  // (the usual path reports it)
  uint32_t max_chain = 0, nice = 0;
  md_deflate_level_params(q.driver, q.matcher, q.level, &max_chain, &nice);
  if (max_chain == 0) return MD_NOT_HANDLED;
  const uint64_t ip = in_off[1] - in_off[0], op = out_off[1] - out_off[0];
  uint64_t longest = 0, cap_max = 0;
  for (size_t i = 0; i < n; i++) {
    if (in_off[i] != in_off[0] + i * ip || out_off[i] != out_off[0] + i * op || in_len[i] > ip || out_cap[i] > op) return MD_NOT_HANDLED;
    longest = in_len[i] > longest ? in_len[i] : longest;
    cap_max = out_cap[i] > cap_max ? out_cap[i] : cap_max;
  }
  if (in_off[1] <= in_off[0] || out_off[1] <= out_off[0] || longest < 4 * kSliceMin || longest > MD_MAX_STREAM) return MD_NOT_HANDLED;
  // four slices (more if the workspace cap asks for smaller ones), S a multiple of 32 KiB
  uint64_t S = ((longest + 3) / 4 + 32767) / 32768 * 32768;
  while (S > kSliceMin && ctx->front_cap_bytes && md_front_big_bytes(slice_positions(in_len, n, S)) > ctx->front_cap_bytes) S -= 32768;
  if (ctx->front_cap_bytes && md_front_big_bytes(slice_positions(in_len, n, S)) > ctx->front_cap_bytes) return MD_NOT_HANDLED;
  const uint64_t nslices = (longest + S - 1) / S;
  if (!ctx->s_in && hipStreamCreateWithFlags(&ctx->s_in, hipStreamNonBlocking) != hipSuccess) return fail(ctx, MD_E_HIP, "hipStreamCreate");
  if (!ctx->s_out && hipStreamCreateWithFlags(&ctx->s_out, hipStreamNonBlocking) != hipSuccess) return fail(ctx, MD_E_HIP, "hipStreamCreate");
  EventList evs;
  std::vector<hipEvent_t> e_in(nslices + 1, nullptr);
  for (auto &e : e_in)
    if (!(e = evs.make())) return fail(ctx, MD_E_HIP, "hipEventCreate");
  hipError_t herr = hipSuccess;
  // columns [c0, c1) of every row of a blob laid out at `pitch`: rows 0 .. n - 2 as one strided copy, the last row by itself
  // (it may end where the blob ends)
  auto band = [&](bool to_device, uint64_t c0, uint64_t c1, hipStream_t cs) {
    if (c1 <= c0 || herr != hipSuccess) return;
    const uint64_t pitch = to_device ? ip : op, off0 = to_device ? in_off[0] : out_off[0], bytes = to_device ? in_bytes : out_bytes;
    uint8_t *d = (to_device ? din : dout) + off0 + c0;
    const uint8_t *hs = h_in + off0 + c0;
    uint8_t *hd = h_out + off0 + c0;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const uint64_t w = c1 - c0;
    if (n > 1) herr = to_device ? hipMemcpy2DAsync(d, pitch, hs, pitch, w, n - 1, kind, cs) : hipMemcpy2DAsync(hd, pitch, d, pitch, w, n - 1, kind, cs);
    const uint64_t last = off0 + (n - 1) * pitch + c0;
    uint64_t wl = w;
    if (last >= bytes) wl = 0;
    else if (last + wl > bytes) wl = bytes - last;
    if (wl && herr == hipSuccess)
      herr = to_device ? hipMemcpyAsync(d + (n - 1) * pitch, hs + (n - 1) * pitch, wl, kind, cs) : hipMemcpyAsync(hd + (n - 1) * pitch, d + (n - 1) * pitch, wl, kind, cs);
  };
  auto columns = [&](uint64_t k) { return std::make_pair(k * S < longest ? k * S : longest, (k + 1) * S < longest ? (k + 1) * S : longest); };
  // (the strided copies are enqueued right BEHIND a slice's kernel launches: should the runtime keep the calling thread
  // until such a copy is done, the kernels it is meant to run under are on the device already)
  uint64_t c_done = 0, c_ready = 0;  // output columns [0, c_done) are on their way to the host, [c_done, c_ready) are final
  const bool dbg_t = getenv("MD_DEBUG_HOSTPATH") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto stamp = [&](const char *what, uint64_t k) {
    if (dbg_t) fprintf(stderr, "[hostpath] %-14s slice %llu at %.2f ms\n", what, (unsigned long long)k,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  };
  SliceHooks hooks;
  hooks.before_slice = [&](uint64_t k) -> int {
    if (k == 0) {
      hipEvent_t e0 = evs.make();  // (what the caller queued on the context's stream comes first)
      if (!e0) return fail(ctx, MD_E_HIP, "hipEventCreate");
      if (hipEventRecord(e0, ctx->stream) != hipSuccess || hipStreamWaitEvent(ctx->s_in, e0, 0) != hipSuccess) return fail(ctx, MD_E_HIP, "hipEventRecord");
      const auto c = columns(0);
      band(true, c.first, c.second, ctx->s_in);
      if (herr == hipSuccess) herr = hipEventRecord(e_in[0], ctx->s_in);
    }
    if (herr == hipSuccess) herr = hipStreamWaitEvent(ctx->stream, e_in[k], 0);
    stamp("before", k);
    return herr == hipSuccess ? MD_OK : fail(ctx, MD_E_HIP, "deflate host path: copy-in", herr);
  };
  hooks.launched = [&](uint64_t k) -> int {
    stamp("launched", k);
    if (k + 1 < nslices) {  // the next slice's input under this slice's kernels
      const auto c = columns(k + 1);
      band(true, c.first, c.second, ctx->s_in);
      if (herr == hipSuccess) herr = hipEventRecord(e_in[k + 1], ctx->s_in);
    }
    stamp("h2d queued", k);
    if (c_ready > c_done) {  // what the slices before made final leaves under them too
      if (dbg_t) fprintf(stderr, "[hostpath] d2h columns [%llu, %llu)\n", (unsigned long long)c_done, (unsigned long long)c_ready);
      band(false, c_done, c_ready, ctx->s_out);
      c_done = c_ready;
    }
    stamp("copies queued", k);
    return herr == hipSuccess ? MD_OK : fail(ctx, MD_E_HIP, "deflate host path: copies", herr);
  };
  hooks.after_slice = [&](uint64_t k, const std::vector<uint64_t> &fin) -> int {
    // (the context's stream has been waited for: what the slice wrote is there)
    stamp("kernels done", k);
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t f : fin) {
      lo = f < lo ? f : lo;
      hi = f > hi ? f : hi;
    }
    // (bands begin and end on 4 KiB columns: a strided copy of odd offsets and widths ran at a quarter of the link's rate;
    // behind the longest output the rows hold nothing anybody reads, up to the distance between two of them)
    c_ready = k + 1 == nslices ? ((hi + 4095) & ~(uint64_t)4095) : (lo & ~(uint64_t)4095);  // at the end: everything, ragged rows included
    if (c_ready > op) c_ready = op;
    if (c_ready < c_done) c_ready = c_done;
    if (k + 1 == nslices && c_ready > c_done) {
      band(false, c_done, c_ready, ctx->s_out);
      c_done = c_ready;
    }
    return herr == hipSuccess ? MD_OK : fail(ctx, MD_E_HIP, "deflate host path: copy-out", herr);
  };
  std::vector<int32_t> r_st(n);
  std::vector<uint32_t> r_sum(n);
  int rc = deflate_in_slices(ctx, format, q, n, S, din, in_off, in_len, dout, out_off, out_cap, out_len, r_st.data(), r_sum.data(), nullptr, &hooks);
  // everything in flight ends before the call returns, whatever happened (the buffers are the caller's)
  const hipError_t a = hipStreamSynchronize(ctx->s_in), b2 = hipStreamSynchronize(ctx->stream), c = hipStreamSynchronize(ctx->s_out);
  stamp("all done", nslices);
  if (rc != MD_OK) return rc;
  if (a != hipSuccess || b2 != hipSuccess || c != hipSuccess) return fail(ctx, MD_E_HIP, "deflate host path", a != hipSuccess ? a : b2 != hipSuccess ? b2 : c);
  for (size_t i = 0; i < n; i++) {
    status[i] = r_st[i];
    if (checksum) checksum[i] = r_sum[i];
  }
  (void)cap_max;
  return MD_OK;
}

static int deflate_batch_host(md_ctx *ctx, int format, const md_deflate_params *params,
                              size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                              const uint64_t *in_len, uint8_t *h_out, size_t out_bytes,
                              const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                              int32_t *status, uint32_t *checksum, const LinkSegs *ls) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (n == 0) return MD_OK;
  if (!params || !in_off || !in_len || !out_off || !out_cap || !out_len || !status)
    return fail(ctx, MD_E_INVALID_ARGUMENT, "null descriptor array");
  for (size_t i = 0; i < n; i++) {
    if (in_off[i] > in_bytes || in_len[i] > in_bytes - in_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "input range out of bounds");
    if (in_len[i] > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "stream longer than MD_MAX_STREAM");
    if (out_off[i] > out_bytes || out_cap[i] > out_bytes - out_off[i])
      return fail(ctx, MD_E_INVALID_ARGUMENT, "output range out of bounds");
  }
  MD_ON_DEVICE(ctx);
  int rc = ctx->scratch[kHostIn].reserve(ctx, in_bytes + 64, "hipMalloc(host path input)");
  if (rc == MD_OK) rc = ctx->scratch[kHostOut].reserve(ctx, out_bytes + 64, "hipMalloc(host path output)");
  if (rc != MD_OK) return rc;
  uint8_t *din = (uint8_t *)ctx->scratch[kHostIn].p, *dout = (uint8_t *)ctx->scratch[kHostOut].p;
  uint64_t *d_in_off = nullptr, *d_in_len = nullptr, *d_out_off = nullptr, *d_out_cap = nullptr, *d_out_len = nullptr;
  int32_t *dstatus = nullptr;
  uint32_t *dsum = nullptr;
  rc = carve(ctx, ctx->scratch[kHostDesc], "hipMalloc(host path descriptors)", [&](md::Carver &c) {
    d_in_off = c.take<uint64_t>(n), d_in_len = c.take<uint64_t>(n), d_out_off = c.take<uint64_t>(n), d_out_cap = c.take<uint64_t>(n);
    d_out_len = c.take<uint64_t>(n);
    dstatus = c.take<int32_t>(n);
    dsum = c.take<uint32_t>(n);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, md::to_device(d_in_off, in_off, n, st));
  HIP_TRY(ctx, md::to_device(d_in_len, in_len, n, st));
  HIP_TRY(ctx, md::to_device(d_out_off, out_off, n, st));
  HIP_TRY(ctx, md::to_device(d_out_cap, out_cap, n, st));
  {  // long streams in a regular layout: slices of POSITIONS, input arriving and output leaving under the kernels
    const int prc = deflate_host_positions(ctx, format, params, n, h_in, in_bytes, in_off, in_len, h_out, out_bytes, out_off, out_cap,
                                           out_len, status, checksum, din, dout);
    if (prc != MD_NOT_HANDLED) return prc;  // (not this kind of batch: slices of streams below)
  }
  // the sequential kernel holds 16 streams per CU: a slice of fewer than 4 096 streams leaves the chip part empty for as
  // long as a stream takes, so a batch is only cut where every slice still has that many
  const std::vector<HostSlice> sl = host_slices(n, in_off, in_len, out_off, out_cap, 4096, (size_t)ctx->host_slices_max, in_bytes, out_bytes);
  rc = host_pipeline(ctx, sl, h_in, din, h_out, dout, [&](size_t i0, size_t cnt) {
    md_deflate_params hp = *params;
    hp.total_in_bytes = 0;
    for (size_t i = i0; i < i0 + cnt; i++) hp.total_in_bytes += (size_t)in_len[i];
    if (hp.total_in_bytes == 0) hp.total_in_bytes = 1;  // all empty: still no read-back
    return deflate_batch_device(ctx, format, &hp, cnt, din, d_in_off + i0, d_in_len + i0, dout, d_out_off + i0, d_out_cap + i0, d_out_len + i0,
                                dstatus + i0, dsum + i0, cnt == 1 ? ls : nullptr);
  });
  if (rc != MD_OK) return rc;
  HIP_TRY(ctx, md::to_host(out_len, d_out_len, n, st));
  HIP_TRY(ctx, md::to_host(status, dstatus, n, st));
  if (checksum) HIP_TRY(ctx, md::to_host(checksum, dsum, n, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return MD_OK;
}

// ONE long stream: whether its hash chains are built in segments by the whole chip (deflate_chunked.hip)
// instead of by one workgroup, and in which.  This changes only who computes link[] and the tails, not their values, so
// every status, byte and checksum is the one-workgroup path's whatever happens afterwards (a dst_cap too small included).
// Taken: DEFLATE / ZLIB / GZIP, drivers ZL / HIGHER / CLI, levels 1..9 (HIGHER: 4), De's matcher, at least
// "deflate_link_segment_min" of input and at least two segments of positions [0, len - 3).  Segments:
// "deflate_link_segment", or by default the stream spread over the CUs - a multiple of 32 KiB and at least 64 KiB (a
// segment inserts 32 KiB in front of its own positions without writing).  The segmented kernel needs no workspace of its
// own; a launch that fails leaves the one-workgroup kernel to do it (deflate_launch).
static bool link_segments(const md_ctx *ctx, int format, const md_deflate_params *params, uint64_t len, LinkSegs *ls) {
  if (ctx->link_seg_min == 0 || len < ctx->link_seg_min || len > MD_MAX_STREAM || len < 4) return false;
  if (format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) return false;
  const int d = params->driver, lv = d == MD_DRIVER_HIGHER ? 4 : params->level;
  if (d != MD_DRIVER_ZL && d != MD_DRIVER_HIGHER && d != MD_DRIVER_CLI) return false;
  if (lv < 1 || lv > 9 || params->matcher != MD_MATCHER_DE) return false;
  const uint64_t p_end = len - 3;  // (deflate_common.hpp stream_p_end: De's matcher, a level above 0)
  uint64_t seg = ctx->link_seg;
  if (seg == 0) {
    const uint64_t cus = ctx->cus > 0 ? (uint64_t)ctx->cus : 256;
    seg = ((p_end + cus - 1) / cus + 32767) / 32768 * 32768;
    if (seg < 65536) seg = 65536;
  }
  if (p_end <= seg) return false;  // (one segment: nothing to spread)
  ls->seg = (uint32_t)seg;
  ls->p_end = (uint32_t)p_end;
  return true;
}

int md_deflate_batch_host(md_ctx *ctx, int format, const md_deflate_params *params,
                          size_t n, const uint8_t *h_in, size_t in_bytes, const uint64_t *in_off,
                          const uint64_t *in_len, uint8_t *h_out, size_t out_bytes,
                          const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                          int32_t *status, uint32_t *checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  ctx->link_last_segments = 0;
  LinkSegs ls;
  const bool seg = n == 1 && params && in_len && link_segments(ctx, format, params, in_len[0], &ls);
  return deflate_batch_host(ctx, format, params, n, h_in, in_bytes, in_off, in_len, h_out, out_bytes, out_off, out_cap, out_len,
                            status, checksum, seg ? &ls : nullptr);
}

// (tests) segments the last deflate batch call of ctx built its hash chains in; 0 = one workgroup per stream
int md_i_link_segments(const md_ctx *ctx) { return ctx ? (int)ctx->link_last_segments : -1; }

static int deflate_one(md_ctx *ctx, int format, int level, int queue_len, int driver, int dynamic, const md_gz_header *gz,
                       const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  if (!ctx || !written || (!src && src_len) || (!dst && dst_cap)) return MD_E_INVALID_ARGUMENT;
  uint64_t in_off = 0, in_len = src_len, out_off = 0, out_cap = dst_cap, out_len = 0;
  int32_t status = 0;
  const md_deflate_params p = {level, queue_len, driver, dynamic, MD_MATCHER_DE, gz, 0, 0};
  int rc = md_deflate_batch_host(ctx, format, &p, 1, src, src_len, &in_off, &in_len, dst, dst_cap, &out_off, &out_cap,
                                 &out_len, &status, nullptr);
  if (rc != MD_OK) return rc;
  *written = (size_t)out_len;
  return status;
}

int md_de_higher_compress(md_ctx *ctx, int queue_len, const uint8_t *src, size_t src_len,
                          uint8_t *dst, size_t dst_cap, size_t *written) {
  return deflate_one(ctx, MD_FORMAT_DEFLATE, 4, queue_len, MD_DRIVER_HIGHER, 1, nullptr, src, src_len, dst, dst_cap, written);
}

int md_zl_higher_compress(md_ctx *ctx, int level, int dynamic, int queue_len, const uint8_t *src,
                          size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  return deflate_one(ctx, MD_FORMAT_ZLIB, level, queue_len, MD_DRIVER_ZL, dynamic, nullptr, src, src_len, dst, dst_cap, written);
}

int md_gz_higher_compress(md_ctx *ctx, int level, int queue_len, const md_gz_header *header, const uint8_t *src,
                          size_t src_len, uint8_t *dst, size_t dst_cap, size_t *written) {
  return deflate_one(ctx, MD_FORMAT_GZIP, level, queue_len, MD_DRIVER_ZL, 1, header, src, src_len, dst, dst_cap, written);
}

// One batch-of-one launch of the deflate kernel in one of its two partial modes (drivers 3 and 4 of
// deflate_kernel.hip): host buffers in, host buffers out.
static int deflate_partial(md_ctx *ctx, int level, int queue_len, int driver, int dynamic, int matcher, const void *src,
                           size_t src_len, void *dst, size_t dst_cap, size_t *out_bytes, uint32_t *hist316) {
  MD_ON_DEVICE(ctx);
  return one_through_batch(
      ctx, src, src_len, dst, dst_cap, out_bytes,
      [&](const uint8_t *d_in, uint64_t *d64, uint8_t *d_out, int32_t *d_status, uint32_t *d_hist) {
        return deflate_launch(ctx, MD_FORMAT_DEFLATE, level, queue_len, driver, dynamic, matcher, nullptr, 1, d_in, d64, d64 + 1, d_out,
                              d64 + 2, d64 + 3, d64 + 4, d_status, nullptr, d_hist, src_len ? src_len : 1);
      },
      316 * 4, hist316);
}

int md_de_lz77_compress(md_ctx *ctx, int level, int queue_len, int matcher, const uint8_t *src, size_t src_len,
                        uint32_t *cmds, size_t cmds_cap, size_t *ncmds, uint32_t *literals, uint32_t *distances) {
  if (!ctx || !ncmds || (!src && src_len) || (!cmds && cmds_cap)) return MD_E_INVALID_ARGUMENT;
  if (level < 0 || level > 9) return fail(ctx, MD_E_INVALID_ARGUMENT, "Invalid level of compression");
  if (queue_len < 4 || queue_len > (1 << 20) || (queue_len & (queue_len - 1)))
    return fail(ctx, MD_E_INVALID_ARGUMENT, "Length of queue MUST be a power of two");
  if (matcher != MD_MATCHER_DE && matcher != MD_MATCHER_LZ) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown matcher");
  if (src_len > MD_MAX_STREAM || cmds_cap > MD_MAX_STREAM / 4) return fail(ctx, MD_E_INVALID_ARGUMENT, "buffer too long");
  uint32_t hist[316];
  size_t bytes = 0;
  int st = deflate_partial(ctx, level, queue_len, 3, 1, matcher, src, src_len, cmds, cmds_cap * 4, &bytes, hist);
  *ncmds = bytes / 4;
  if (st == MD_OK) {
    if (literals) memcpy(literals, hist, 286 * 4);
    if (distances) memcpy(distances, hist + 286, 30 * 4);
  }
  return st;
}

int md_de_def_encode(md_ctx *ctx, int kind, const uint32_t *cmds, size_t ncmds, uint8_t *dst, size_t dst_cap,
                     size_t *written) {
  if (!ctx || !written || (!cmds && ncmds) || (!dst && dst_cap)) return MD_E_INVALID_ARGUMENT;
  if (kind < MD_BLOCK_FLAT || kind > MD_BLOCK_DYNAMIC) return fail(ctx, MD_E_INVALID_ARGUMENT, "unknown block kind");
  if (ncmds >= (1u << 20)) return fail(ctx, MD_E_INVALID_ARGUMENT, "more commands than the largest queue holds");
  for (size_t i = 0; i < ncmds; i++) {  // De.Queue's encodings only (lib/de.ml:2245-2266): the kernel indexes tables with the fields
    const uint32_t c = cmds[i];
    const bool ok = (c & 0x2000000u) ? ((c & ~0x2ffffffu) == 0 && ((c >> 16) & 0x1ff) <= 255 && (c & 0xffff) <= 32767) : c <= 256;
    if (!ok) return fail(ctx, MD_E_INVALID_ARGUMENT, "not a De.Queue command");
  }
  int queue_len = 4;
  while ((size_t)queue_len < ncmds + 1) queue_len <<= 1;  // Queue.create: a power of two that holds them all
  return deflate_partial(ctx, 4, queue_len, 4, kind, MD_MATCHER_DE, cmds, ncmds * 4, dst, dst_cap, written, nullptr);
}

int md_de_def_run(md_ctx *ctx, int queue_len, const uint32_t *ops, size_t nops, uint8_t *dst, size_t dst_cap, size_t *written,
                  uint8_t *results, size_t results_cap, size_t *nresults) {
  if (!ctx || !written || (!ops && nops) || (!dst && dst_cap) || (!results && results_cap)) return MD_E_INVALID_ARGUMENT;
  if (queue_len < 4 || queue_len > (1 << 20) || (queue_len & (queue_len - 1)))
    return fail(ctx, MD_E_INVALID_ARGUMENT, "Length of queue MUST be a power of two");
  if (nops > MD_MAX_STREAM / 4) return fail(ctx, MD_E_INVALID_ARGUMENT, "operation list too long");
  uint32_t res[316];
  memset(res, 0, sizeof res);
  int st = deflate_partial(ctx, 4, queue_len, 5, 0, MD_MATCHER_DE, ops, nops * 4, dst, dst_cap, written, res);
  if (st < 0 && st != MD_E_INVALID_ARGUMENT) return st;
  // the kernel reports the first 315 answers; *nresults = how many of them results[] received
  size_t n = res[0] < 315 ? res[0] : 315;
  if (n > results_cap) n = results_cap;
  for (size_t i = 0; i < n; i++) results[i] = (uint8_t)res[1 + i];
  if (nresults) *nresults = n;
  if (st == MD_E_INVALID_ARGUMENT) return fail(ctx, st, "not a De.Def operation list");
  if (st >= 0 && res[0] > n) return fail(ctx, MD_E_INVALID_ARGUMENT, "more encode answers than results[] (or the kernel's 315) can hold");
  return st;
}
