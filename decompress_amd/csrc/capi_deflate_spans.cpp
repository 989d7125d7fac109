// capi_deflate_spans.cpp — one stream written as joined spans (mdeflate.h: md_deflate_spans_*).
#include <string.h>

#include "ctx.hpp"

using md::spn::stored_size;

// the header's bytes for the format; false when a gzip header field is out of range
static bool spans_frame(int format, int level, const md_gz_header *gz, md::spn::Frame *f) {
  memset(f, 0, sizeof *f);
  f->format = format;
  if (format == MD_FORMAT_ZLIB) {  // Zl.Def's header (frame_header of deflate_kernel.hip: lib/zl.ml:511-517, :580-581)
    const unsigned flevel = level == 0 ? 0 : level <= 5 ? 1 : level == 6 ? 2 : 3;
    unsigned h = ((8 + ((15 - 8) << 4)) << 8) | (flevel << 6);
    h += 31 - (h % 31);
    f->hdr[0] = (uint8_t)(h >> 8), f->hdr[1] = (uint8_t)h;
    f->hdr_len = 2;
  } else if (format == MD_FORMAT_GZIP) {
    f->hdr_len = gz_header_bytes(gz, level, f->hdr);
    if (!f->hdr_len) return false;
  }
  return true;
}

static size_t span_count(size_t len, size_t span) { return len ? len / span + (len % span ? 1 : 0) : 1; }

// every span in its stored form: no span goes out longer
static unsigned __int128 spans_body_bound(size_t len, size_t span) {
  const size_t full = len / span, rest = len % span;
  return (unsigned __int128)full * stored_size(span) + (rest || !len ? stored_size(rest) : 0);
}

size_t md_deflate_spans_bound(int format, size_t src_len, size_t span, const md_gz_header *hdr) {
  md::spn::Frame f;
  if ((format != MD_FORMAT_DEFLATE && format != MD_FORMAT_ZLIB && format != MD_FORMAT_GZIP) || span > MD_MAX_STREAM) return 0;
  if (!spans_frame(format, 0, hdr, &f)) return 0;
  if (span == 0) span = 1024;  // (the smallest span "deflate_span_kib" selects: smaller spans, more stored blocks)
  const unsigned __int128 need = spans_body_bound(src_len, span) + f.hdr_len + md::spn::trailer_len(format);
  return need > (unsigned __int128)SIZE_MAX ? 0 : (size_t)need;  // (a text that long in spans that short: no room holds it)
}

// Plan, ONE deflate launch over the spans, the stored spans' Adler-32, sizes, scan, join: the stream goes to d_dst if it fits
// dst_cap.  Everything is enqueued on the context's stream and nothing is read back - but by the deflate launch itself where
// the workspace cap sends it through slices of positions.
// Primed (md_set_option "deflate_span_prime"): the deflate launch alone takes a second set of descriptors - span i with the
// w_i = min(i * span, 32 768) bytes in front of it as one stream that begins to emit at w_i.  The streams overlap in the
// text, which is only read; the front workspace is 13 bytes per position of len + 32 768 (n - 1) positions at the most.
static int spans_run(md_ctx *ctx, int format, const md_deflate_params *params, size_t span, const uint8_t *d_src, size_t len, uint8_t *d_dst,
                     size_t dst_cap, uint64_t *d_written, int32_t *d_status, uint32_t *d_checksum) {
  md_deflate_params q = *params;
  if (format == MD_FORMAT_GZIP) q.driver = MD_DRIVER_ZL, q.dynamic = 1;  // Gz.Def's body (MD_FORMAT_GZIP)
  if (span == 0) span = ctx->span_bytes;
  if (span > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "span longer than MD_MAX_STREAM");
  const size_t n = span_count(len, span);
  if (n > 0x7ffffff0ull) return fail(ctx, MD_E_INVALID_ARGUMENT, "too many spans in one call");
  md::spn::Frame f;
  if (!spans_frame(format, q.level, q.gz_header, &f)) return fail(ctx, MD_E_INVALID_ARGUMENT, "gzip header field out of range");
  ctx->spans_last = md_deflate_spans_info{n, 0, span};
  // a slot holds the span's stored form and no more: a body that does not fit has lost against that form (the encoder then
  // says MD_UNEXPECTED_END_OF_OUTPUT for the slot, and the join kernel writes the span stored)
  const size_t stride = ((size_t)stored_size(span < len ? span : len) + 15) & ~(size_t)15;
  int rc = ctx->scratch[kHostOut].reserve(ctx, n * stride + 64, "hipMalloc(span slots)");
  if (rc == MD_OK) rc = ctx->spans_count.reserve(ctx, sizeof(uint64_t), "hipMalloc(span count)");
  if (rc != MD_OK) return rc;
  uint8_t *slots = (uint8_t *)ctx->scratch[kHostOut].p;
  uint64_t *in_off = nullptr, *in_len = nullptr, *out_off = nullptr, *out_cap = nullptr, *out_len = nullptr, *size = nullptr, *off = nullptr,
           *tail = nullptr, *x_off = nullptr, *x_len = nullptr;
  uint32_t *first = nullptr;
  const bool prime = ctx->span_prime && n > 1;  // (one span has nothing in front of it)
  int32_t *status = nullptr, *err = nullptr;
  uint32_t *adler = nullptr, *crc = nullptr;
  rc = carve(ctx, ctx->scratch[kGzmDesc], "hipMalloc(span descriptors)", [&](md::Carver &desc) {
    in_off = desc.take<uint64_t>(n), in_len = desc.take<uint64_t>(n), out_off = desc.take<uint64_t>(n), out_cap = desc.take<uint64_t>(n);
    out_len = desc.take<uint64_t>(n), size = desc.take<uint64_t>(n), off = desc.take<uint64_t>(n + 1), tail = desc.take<uint64_t>(2 * n);
    status = desc.take<int32_t>(n), err = desc.take<int32_t>(2);
    adler = desc.take<uint32_t>(n), crc = desc.take<uint32_t>(n);
    if (prime) x_off = desc.take<uint64_t>(n), x_len = desc.take<uint64_t>(n), first = desc.take<uint32_t>(n);
  });
  if (rc != MD_OK) return rc;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, md::zero(err, 2, st));
  HIP_TRY(ctx, md::zero(ctx->spans_count.as<uint64_t>(), 1, st));
  MD_LAUNCH_TRY(ctx, md_launch_spans_plan(n, len, span, stride, in_off, in_len, out_off, out_cap, x_off, x_len, first, st));
  // (primed: span i brings min(i * span, kPrime) bytes along - summed exactly, the prefixes below kPrime first)
  size_t primed = 0;
  if (prime) {
    const size_t growing = (size_t)(md::spn::kPrime / span) < n - 1 ? (size_t)(md::spn::kPrime / span) : n - 1;  // spans 1 .. growing: i * span
    primed = span * (growing * (growing + 1) / 2) + (n - 1 - growing) * (size_t)md::spn::kPrime;
  }
  q.total_in_bytes = len ? len + primed : 1;
  q.gz_header = nullptr;
  rc = deflate_batch_tails(ctx, MD_FORMAT_DEFLATE, &q, n, d_src, prime ? x_off : in_off, prime ? x_len : in_len, slots, out_off, out_cap, out_len,
                           status, adler, tail, first);
  if (rc != MD_OK) return rc;
  if (format == MD_FORMAT_GZIP) MD_LAUNCH_TRY(ctx, md_launch_crc32((uint32_t)n, d_src, in_off, in_len, crc, st));
  md::spn::Spans s = {};
  s.n = n, s.len = len;
  s.in_off = in_off, s.in_len = in_len, s.slot_off = out_off, s.out_len = out_len, s.tail = tail;
  s.status = status, s.adler = adler, s.crc = format == MD_FORMAT_GZIP ? crc : nullptr;
  s.size = size, s.off = off, s.err = err, s.stored = ctx->spans_count.as<uint64_t>();
  // a span that goes out stored for want of room: its Adler-32 from the text (in a batch in slices of positions the encoder's
  // word for a stream that ran out of room early stops where that piece ended)
  if (format != MD_FORMAT_GZIP) MD_LAUNCH_TRY(ctx, md_launch_spans_adler(&s, d_src, adler, st));
  MD_LAUNCH_TRY(ctx, md_launch_spans_sizes(&s, st));
  MD_LAUNCH_TRY(ctx, md_launch_gzm_scan64(size, n, off, st));
  MD_LAUNCH_TRY(ctx, md_launch_spans_join(&f, &s, d_src, slots, d_dst, dst_cap, d_written, d_status, d_checksum, st));
  ctx->spans_pending = true;
  return MD_OK;
}

static int spans_args(md_ctx *ctx, int format, const md_deflate_params *params, size_t span) {
  const int rc = md_validate_deflate_params(ctx, format, params);
  if (rc != MD_OK) return rc;
  if (span > MD_MAX_STREAM) return fail(ctx, MD_E_INVALID_ARGUMENT, "span longer than MD_MAX_STREAM");
  return MD_OK;
}

int md_deflate_spans_device(md_ctx *ctx, int format, const md_deflate_params *params, size_t span, const uint8_t *d_src, size_t src_len,
                            uint8_t *d_dst, size_t dst_cap, uint64_t *d_written, int32_t *d_status, uint32_t *d_checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if ((!d_src && src_len) || (!d_dst && dst_cap) || !d_written || !d_status || !d_checksum) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  int rc = spans_args(ctx, format, params, span);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  return spans_run(ctx, format, params, span, d_src, src_len, d_dst, dst_cap, d_written, d_status, d_checksum);
}

int md_deflate_spans_host(md_ctx *ctx, int format, const md_deflate_params *params, size_t span, const uint8_t *src, size_t src_len, uint8_t *dst,
                          size_t dst_cap, size_t *written, uint32_t *checksum) {
  if (!ctx) return MD_E_INVALID_ARGUMENT;
  if (!written || (!src && src_len) || (!dst && dst_cap)) return fail(ctx, MD_E_INVALID_ARGUMENT, "null pointer");
  *written = 0;
  int rc = spans_args(ctx, format, params, span);
  if (rc != MD_OK) return rc;
  MD_ON_DEVICE(ctx);
  if (span == 0) span = ctx->span_bytes;
  const size_t bound = md_deflate_spans_bound(format, src_len, span, format == MD_FORMAT_GZIP ? params->gz_header : nullptr);
  if (!bound) return fail(ctx, MD_E_INVALID_ARGUMENT, "gzip header field out of range");
  rc = upload_host_in(ctx, src, src_len);
  if (rc == MD_OK) rc = ctx->scratch[kGzmOut].reserve(ctx, bound + 64 + 16, "hipMalloc(joined stream)");
  if (rc != MD_OK) return rc;
  uint8_t *d_file = (uint8_t *)ctx->scratch[kGzmOut].p;
  // (the three result words live behind the stream's bound, on an 8-byte boundary)
  uint64_t *d_res = (uint64_t *)(d_file + ((bound + 7) & ~(size_t)7));
  rc = spans_run(ctx, format, params, span, (const uint8_t *)ctx->scratch[kHostIn].p, src_len, d_file, bound, d_res, (int32_t *)(d_res + 1),
                 (uint32_t *)(d_res + 1) + 1);
  if (rc != MD_OK) return rc;
  uint64_t res[2] = {0, 0}, stored = 0;
  HIP_TRY(ctx, md::to_host(res, d_res, 2, ctx->stream));
  HIP_TRY(ctx, md::to_host(&stored, ctx->spans_count.as<uint64_t>(), 1, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->spans_last.stored_spans = (size_t)stored;
  ctx->spans_pending = false;
  int32_t status;
  uint32_t sum;
  memcpy(&status, &res[1], 4);
  memcpy(&sum, (const uint8_t *)&res[1] + 4, 4);
  if (checksum) *checksum = sum;
  if (status == MD_E_HIP) return fail(ctx, MD_E_HIP, "joined spans: a span's tail does not fit its body");
  if (status < 0) return fail(ctx, status, "joined spans: the deflate launch refused a span");
  if (status == MD_UNEXPECTED_END_OF_OUTPUT) return fail(ctx, MD_E_HIP, "joined spans: sizes above the bound");
  if (status != MD_OK) return status;  // (MD_QUEUE_FULL: a span's, and so the call's)
  if (res[0] > dst_cap) return MD_UNEXPECTED_END_OF_OUTPUT;
  if (res[0]) HIP_TRY(ctx, hipMemcpy(dst, d_file, (size_t)res[0], hipMemcpyDeviceToHost));
  *written = (size_t)res[0];
  return MD_OK;
}

int md_deflate_spans_last(md_ctx *ctx, md_deflate_spans_info *info) {
  if (!ctx || !info) return MD_E_INVALID_ARGUMENT;
  if (ctx->spans_pending) {  // the device form reads nothing back: the count of stored spans is fetched when it is asked for
    MD_ON_DEVICE(ctx);
    uint64_t stored = 0;
    HIP_TRY(ctx, md::to_host(&stored, ctx->spans_count.as<uint64_t>(), 1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->spans_last.stored_spans = (size_t)stored;
    ctx->spans_pending = false;
  }
  *info = ctx->spans_last;
  return MD_OK;
}
